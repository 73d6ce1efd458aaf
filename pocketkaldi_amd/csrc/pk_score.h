// pk_score.h -- what crosses between the online scorer's kernels (stream.hip) and its host object (capi_stream.hip),
// and what the scorers share: the scorer core and the one copy of the operand layout, the span expansion, the chunk
// walk, the calibration loop and the way rows become a host decodable (internal).
#ifndef PK_SCORE_H_
#define PK_SCORE_H_

#include <functional>

#include "pk_create.h"
#include "pk_frontend.h"
#include "pk_host.h"

namespace pkmi {

struct TransformStage;                      // pk_transform_kernel.h
constexpr int kTailCap = kFrameLength;     // a carried tail holds at most 399 samples (fewer than one frame's 400)

// One slot's share of a step (device array, one entry per slot taking part).
struct StreamRec {
  int32_t slot;
  int32_t tail_len;    // samples carried from earlier steps (global samples 160 n_old ...)
  int32_t new_len;     // samples pushed since the last step
  int32_t tail_par;    // the slot's tail buffer that holds the carried samples (the step writes the other one)
  int32_t n_old;       // CMVN frames computed before this step
  int32_t m;           // frames this step computes: n_old .. n_old + m - 1
  int32_t a, b;        // rows scored: frames [a, b)
  int32_t closed;      // 1: the right edge is the last frame (am.cc:73-75)
  int32_t cols;        // columns of the slot's region of Yt: RoundUp(b - a, 4) + L + R (0: no rows)
  int32_t kind;        // -1: audio; PK_MI355_FEATS_RAW / _NORMALIZED: a feature slot (tail_len = new_len = 0, an empty
                       // segment; m = frames pushed since the last step, [m][D] floats at new_off of the upload staging)
  int32_t hist_par;    // NORMALIZED: the slot's history buffer that holds the frames below n_old (the step writes the other one)
  int32_t ring_par;    // a deltas object: the slot's delta ring buffer that holds the base frames below n_old
  int32_t xf_bits;     // a transform object.  Bit 0: the slot's transform ring buffer that holds the input
                       // frames below the step's first fresh one; bits 1-2: the slot's own matrix (kSlotMat*: none, linear,
                       // affine).  (It lies where the struct had padding: a record is the 96 bytes it was.)
  int64_t woff;        // first sample of the segment in the wave staging
  int64_t new_off;     // first pushed sample in the upload staging
  int64_t raw_base;    // first row of the slot's new frames in the step's raw rows
  int64_t col_base;    // first column of the slot's region of Yt
  int64_t row_off;     // StreamCmvnChainKernel, StreamFeatureLayoutKernel: the first float of the slot's fresh rows [m][D] in the
                       // upload staging -- new_off for a feature slot; for an audio slot of a front-end spec at D != 40
                       //  the rows FbankAnyKernel wrote into the staging's row area, behind the samples
};
static_assert(sizeof(StreamRec) == 96, "StreamRec: xf_bits fills the padding behind ring_par");
enum { kSlotMatNone = 0, kSlotMatLinear = 1, kSlotMatAffine = 2 };      // StreamRec::xf_bits >> 1

// launchers (stream.hip): one workgroup (StreamAssembleKernel) / one wavefront (StreamCmvnKernel) for each of n records
void LaunchStreamAssemble(const StreamRec *recs, int n, const float *upload, float *tails, float *wave, hipStream_t stream);
void LaunchStreamCmvn(const StreamRec *recs, int n, float *rows, const float *g, const CmvnTables *tab, float *sums,
                      float *raw_hist, float *hist, int hist_len, int left, int right, float *yt, int64_t ldy, hipStream_t stream);

// launchers (stream.hip), feature slots.  LaunchStreamRawRows: one workgroup for each of n records; those of kind
// PK_MI355_FEATS_RAW have their m pushed rows copied from the upload staging to rows + 40 raw_base, where FbankKernel
// would have written them.  LaunchStreamFeatureLayout: (tiles of 64 columns) x (n records, all NORMALIZED): the slot's
// region of Yt[dim][ldy] as StreamCmvnKernel defines it, frame f from the new frames (f >= n_old, at row_off) or from the slot's
// history hist[slot][hist_par][f % hist_len][dim]; the other history buffer receives frames [max(n - hist_len, 0), n).
// max_cols: the widest region.  The caller has checked every base and count against the buffers.
void LaunchStreamRawRows(const StreamRec *recs, int n, const float *upload, float *rows, hipStream_t stream);
void LaunchStreamFeatureLayout(const StreamRec *recs, int n, int max_cols, const float *upload, float *hist, int hist_len, int dim,
                               int left, int right, float *yt, int64_t ldy, hipStream_t stream);

// launcher (features.hip): features frame-major [sum T][dim], utterance u's rows from raw_base[u] on -> the padded
// feature-major Yt[dim][ldy], frame t at column pad_base[u] + left + t, the first / last frame replicated into the
// pads (what LaunchCmvn writes, without the arithmetic: a copy, bit for bit).  One launch for all utterances;
// max_frames: the longest utterance.  The caller has checked every base and count against the buffers.
void LaunchFeatureLayout(const float *feats, const UttLayout &utts, int num_utts, int max_frames, int dim, int left, int right,
                         float *yt, int64_t ldy, hipStream_t stream);

// launchers, CMVN at any feature dimension: the chain of cmvn.cc:44-101 with lane = feature, one
// wavefront per (utterance or record, block of 64 features); g: dim sums (the count lives in tab).
// LaunchCmvnChain (features.hip): raw rows [sum T][dim] -> normalised rows `out` of the same shape (never in place:
// frame t - 600 is read raw), utterance u's rows from raw_base[u] on; LaunchFeatureLayout then lays `out` out.
// LaunchStreamCmvnChain (stream.hip): the RAW and the audio records among the n given have their m fresh rows, [m][dim] at
// row_off of the upload staging, normalised in place; sums[slot][dim] and raw_hist[slot][600][dim] carry the slot from step to step.
// The caller has checked every base and count against the buffers.
void LaunchCmvnChain(const float *raw, const UttLayout &utts, int num_utts, int dim, const float *d_global, const CmvnTables *d_cmvn_tab,
                     float *out, hipStream_t stream);
void LaunchStreamCmvnChain(const StreamRec *recs, int n, int dim, float *upload, const float *g, const CmvnTables *tab, float *sums,
                           float *raw_hist, hipStream_t stream);

}  // namespace pkmi

namespace pkhost {

// ------------------------------------------------------------------ scorer core (capi_batch.hip)
// What the batch and the online scorer both are: the front-end tables on the device, the first layer's feature-major
// operand Yt with its zero span, the log-likelihood rows and one set of layer buffers, on one stream.  A row of Yt is
// RoundUp(max_cols, chunk) columns (whole passes), 256 of slack behind them, then zero_span columns nobody writes: the
// padding rows of the spliced operand read zeros there, at their column shift (at most `pad` columns per unit).
struct ScorerCore {
  pk_mi355_am *am = nullptr; int device = 0; hipStream_t stream = nullptr;
  FrontendTables *d_tables = nullptr; float *d_global = nullptr; CmvnTables *d_cmvn_tab = nullptr;   // front-end tables
  int64_t max_frames = 0, max_cols = 0, chunk = 0, zero_span = 0, ldy = 0;
  float *d_yt = nullptr, *d_ll = nullptr;   // [feat_dim][ldy], [max_cols][num_pdfs]
  ExecBufs exec;
};

inline int64_t ZeroSpan(int64_t units, int pad) { return RoundUp(units * pad + 2 * kTile, 256); }
inline const float *ZeroSource(const float *yt, int64_t ld, int64_t zero_span) { return yt + (ld - zero_span); }
inline const float *ZeroSource(const ScorerCore &c) { return ZeroSource(c.d_yt, c.ldy, c.zero_span); }

// The first HIP failure of a create entry becomes its fail text; the entry goes on and destroys the object at its end.
struct CreateCheck {
  const char *name; bool ok = true;
  void operator()(hipError_t e) { if (e != hipSuccess && ok) { ok = false; Fail(PK_MI355_E_DEVICE, "%s: %s", name, hipGetErrorString(e)); } }
};
// On the selected device (am's): `units` utterances or slots of at most max_frames frames and max_rows rows of the
// layer stack together, passes of at most chunk_cap rows.  Yt has am->feat_dim rows.  global_stats (stats_dim sums,
// then the count) may be null (a scorer that is only ever fed normalised features): no table is then made.  The fbank
// tables are made for stats_dim == 40 only; at any other dimension there is no front-end, only the CMVN tables.
// On failure (chk.ok false) the caller still calls FreeScorerCore.
void CreateScorerCore(ScorerCore *c, pk_mi355_am *am, const float *global_stats, int stats_dim, int units, int64_t max_frames,
                      int64_t max_rows, int64_t chunk_cap, CreateCheck &chk);
void FreeScorerCore(ScorerCore *c);             // (the owner has waited for the stream)

// What the create entries of both scorers share.  UploadSpecTables: a front-end spec's tables to *d_any (the owner frees
// it), and FbankKernel's own tables, which FbankAnyKernel reads too, where the core made none.  FrontendFits: false and
// the fail text when a front-end of `dim` features (spec: one made from a front-end spec) does not feed base_dim -- the
// model's own dimension, or with deltas of `order` in between the one in front of them.  StatsLenFits: the same for
// statistics of stats_len entries at `dim` (base: a dimension in front of deltas).
inline void UploadSpecTables(ScorerCore *c, const pkmi::FrontendAnyTables *any, pkmi::FrontendAnyTables **d_any, CreateCheck &chk) {
  if (!c->d_tables && chk.ok) {                      // (the scorer core makes FbankKernel's tables for 40-dim statistics only)
    pkmi::FrontendTables host;
    if (BuildFrontendTables(&host)) { chk.ok = false; Fail(PK_MI355_E_INVALID, "front-end table construction failed"); }
    chk(hipMalloc(&c->d_tables, sizeof(pkmi::FrontendTables)));
    if (chk.ok) chk(hipMemcpy(c->d_tables, &host, sizeof(pkmi::FrontendTables), hipMemcpyHostToDevice));
  }
  chk(hipMalloc(d_any, sizeof(pkmi::FrontendAnyTables)));
  if (chk.ok) chk(hipMemcpy(*d_any, any, sizeof(pkmi::FrontendAnyTables), hipMemcpyHostToDevice));
}

inline bool FrontendFits(int dim, bool spec, const pk_mi355_am *am, int base_dim, int order) {
  if (dim == base_dim) return true;
  if (order > 0)
    Fail(PK_MI355_E_INVALID, "the front-end spec produces %d-dim features, the model's %d with deltas of order %d need %d", dim, am->feat_dim, order, base_dim);
  else if (spec)
    Fail(PK_MI355_E_INVALID, "the front-end spec produces %d-dim features, the model expects %d", dim, am->feat_dim);
  else
    Fail(PK_MI355_E_INVALID, "the front-end produces %d-dim features, the model expects %d", dim, am->feat_dim);
  return false;
}

inline bool StatsLenFits(int stats_len, int dim, bool base) {
  if (stats_len == dim + 1) return true;
  if (base)
    Fail(PK_MI355_E_INVALID, "the CMVN statistics have %d entries, %d-dim base features need %d (the sums, then the count)", stats_len, dim, dim + 1);
  else
    Fail(PK_MI355_E_INVALID, "the CMVN statistics have %d entries, a %d-dim model needs %d (the sums, then the count)", stats_len, dim, dim + 1);
  return false;
}

// The request (pk_create.h) through its checks, in the one order of DESIGN.md section 28 (capi_batch.hip); an entry
// runs those its request gives rise to.  False: refused, the text is pk_mi355_last_error's.  True: *dims is filled.
bool CheckCreate(const pk_mi355_am *am, const CreateRequest &r, CreateDims *dims);
// Every way to a scorer behind the public entries' one-line request fillers: CheckCreate, then the object (capi_batch.hip,
// capi_stream.hip).  Null: refused or failed, the text is pk_mi355_last_error's.
pk_mi355_batch *CheckedBatch(pk_mi355_am *am, const CreateRequest &r);
pk_mi355_stream *CheckedStream(pk_mi355_am *am, const CreateRequest &r);

// What both recognizers load behind their files (capi_recognizer.hip): the model at `precision` and its statistics into
// stats[kMaxCmvnStats] -- the reference's 41 without a front-end spec, else at the base dimension of (frontend, deltas,
// xform) -- and in *r the audio request that hands them to a scorer of `units` and `capacity` samples (the caller says live).
int LoadModelAndStats(const char *config_path, int precision, const pk_mi355_frontend_spec_t *frontend, const pk_mi355_deltas_spec_t *deltas,
                      const pk_mi355_transform_spec_t *xform, int units, int64_t capacity, pk_mi355_am_t **am, float *stats, CreateRequest *r);

// What both creates upload for the stages of a checked request (capi_batch.hip).  UploadDeltaScales: the spec's scale
// table (pkdelta::BuildScales); the owner frees it.  UploadTransform: the spec's stage record (pk_transform_kernel.h), its
// matrix (if it has one) transposed and padded (pkxf::PackTransposed) on the device; the owner frees mt.
float *UploadDeltaScales(const pk_mi355_deltas_spec_t &deltas, CreateCheck &chk);
pkmi::TransformStage UploadTransform(const pk_mi355_transform_spec_t &x, CreateCheck &chk);

// ------------------------------------------------------------------ column shifts (capi_batch.hip)
// Spans of rows (a multiple of four each) with one column shift -> one entry per group of four rows, for every row a
// tile of the layer stack can touch (the last tile's padding rows and the rows past a span's last frame read real
// memory and are ignored); the groups past the last span keep the last shift.  False, *bad (if given) = the shift, when one lies
// outside [0, zero_span - kTile]: a negative one would wrap in the kernels' unsigned lane offsets.
struct ShiftSpan { int64_t end_row; int32_t shift; };
inline int64_t Shift4Groups(int64_t total_rows) { return RoundUp(total_rows, kTileF16) / 4 + kTileF16 / 4; }
// entries of a scorer's host and device arrays: total_rows <= max_cols, a multiple of kTileF16, so Shift4Groups <=
// max_cols / 4 + kTileF16 / 4 (the rest is slack)
inline int64_t Shift4Cap(int64_t max_cols) { return max_cols / 4 + kTileF16; }
bool ExpandShift4(const std::vector<ShiftSpan> &spans, int64_t total_rows, int64_t zero_span, int32_t *shift4, int32_t *bad);

// ------------------------------------------------------------------ chunk walk (capi_exec.hip)
// The spliced first-layer operand: Yt [feat_dim][ld] or (f16 modes) its split copy [ld][2 feat_dim].  zero: zero floats
// in the same allocation as yt (128 + the largest column shift of them) -- the tail of feature row 0 of every Yt this
// library allocates is never written.  shift4: GemmArgs::splice_shift, or null.
struct Operand { const float *yt; const _Float16 *y2; int64_t ld; const float *zero; const int32_t *shift4; };
struct Lane { hipStream_t stream; const ExecBufs *exec; };
// RunLayers / RunLayersF16 over rows [0, total_rows), `chunk` at a time, chunk k on lane k % nlanes; row r at out + r * num_pdfs
int WalkChunks(const pk_mi355_am *am, const Operand &op, int64_t total_rows, int64_t chunk, const Lane *lanes, int nlanes,
               bool want_tail, float scale, float *out, Timer *timer);

// ------------------------------------------------------------------ calibration (capi_exec.hip), rows to the host
// pass(): queue one scoring pass and synchronise, so that e's range words are the pass's.
int CalibrateLoop(pk_mi355_am *am, const ExecBufs &e, const std::function<int()> &pass);

// ------------------------------------------------------------------ the single-utterance entries' scorer (capi_batch.hip)
constexpr int64_t kSingleChunk = 4096;   // frames per pass of pk_decodable_init, pk_mi355_am_calibrate and nnet_propagate
// am->mu held: the model's one-utterance features batch (a features request without statistics, passes of kSingleChunk
// rows, through no check), remade when `frames` do not fit.  Null: the create failed (its text is in pk_mi355_last_error).
pk_mi355_batch *SingleBatch(pk_mi355_am *am, int64_t frames);
// pk_mi355_batch_calibrate behind its argument checks, for a caller that holds am->mu
int BatchCalibrateLocked(pk_mi355_batch *b);

inline void ClearDecodable(pk_decodable_t *out, pk_mi355_am_t *am) { out->am = am; out->log_prob = pk_matrix_t{0, 0, nullptr}; }
// rows x N floats at src -> a malloc'd matrix in *out (pk_decodable_destroy frees it); verdict() may still withhold
// them once the stream has been synchronised.  `what` names the entry in the fail text.
template <class Verdict>
int FetchRows(const float *src, int rows, int N, hipStream_t stream, const char *what, pk_decodable_t *out, Verdict verdict) {
  const size_t bytes = sizeof(float) * (size_t)rows * N;
  float *host = static_cast<float *>(malloc(bytes));
  if (!host) return Fail(PK_MI355_E_INVALID, "out of host memory");
  hipError_t e = hipMemcpyAsync(host, src, bytes, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) { free(host); return Fail(PK_MI355_E_DEVICE, "%s: %s", what, hipGetErrorString(e)); }
  if (int rc = verdict()) { free(host); return rc; }
  out->log_prob = pk_matrix_t{rows, N, host};
  return 0;
}

}  // namespace pkhost

#endif  // PK_SCORE_H_
