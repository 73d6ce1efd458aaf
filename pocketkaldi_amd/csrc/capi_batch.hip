// capi_batch.hip -- the scorer core (pk_score.h) and the batched, device-resident scorer over it (PCM in HBM ->
// fbank -> CMVN -> layer stack -> log-likelihoods in HBM; or features in at the CMVN or at the layer stack, DESIGN.md
// section 12), the page-locked result arenas and the decodable views handed
// out over them, and the acoustic half of pk_process (pocketkaldi.cc:186-218).  Host C++ over the HIP runtime.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <unordered_set>
#include <vector>

#include "pk_delta_kernel.h"
#include "pk_frontend.h"
#include "pk_norm_kernel.h"
#include "pk_plan.h"
#include "pk_resample.h"
#include "pk_score.h"
#include "pk_transform_kernel.h"

using namespace pkmi;
using namespace pkhost;

// Page-locked host arenas of pk_mi355_batch_fetch_all.  A decodable handed out by fetch_all is a
// VIEW into its batch's arena; pk_decodable_destroy must not free() such a pointer, and the
// reference's caller destroys its decodable unconditionally, whenever it likes
// (pocketkaldi.cc:247) -- also after the batch is gone.  So the arena is shared property: the
// page-locked memory is released when the batch has been destroyed AND the views of its LAST
// fetch_all have been destroyed, whichever comes last.  (A caller that never destroys its views
// keeps the arena until the process ends.)
//
// Every fetch_all makes one ViewGen -- the generation its views belong to -- and a view's `am` field
// points at it (tagged, bit 0; opaque to every caller; pk_decodable_destroy and pk_decodable_loglikelihood resolve it).
// ViewGen records are 64-byte aligned and RECYCLED, never returned to the heap: bits 1-5 of a handle carry the
// record's serial, which moves on every time the record is retired, and retired records are reused oldest first --
// a bitwise copy of a view that has already been destroyed therefore names a (record, serial) pair that is not
// alive and is ignored, also after the record has been given to a later fetch_all (the guard used
// to key on the record's address alone).
// A view therefore always decrements the count of ITS OWN generation: a stale view of an earlier
// fetch_all, or of another batch whose arena once occupied the same addresses, can never drive the
// current generation's count to zero under views that are still outstanding (the
// counts used to be found by address range).  Whether a decodable is a view is not guessed from its
// address either, so pk_decodable_destroy free()s exactly the matrices malloc() made.
namespace pkhost {
struct ArenaRec {
  void *mem;
  bool batch_alive;
  ViewGen *cur;
};
}  // namespace pkhost

namespace {
std::mutex g_arena_mu;
// live generations: a handle that is not in here (a view destroyed twice through a bitwise copy)
// is ignored instead of dereferenced
std::unordered_set<const ViewGen *> g_gens;
std::vector<ViewGen *> g_retired;     // FIFO of records waiting for reuse (head index below)
size_t g_retired_head = 0;

inline unsigned SerialOf(const pk_mi355_am_t *am) { return (unsigned)((reinterpret_cast<uintptr_t>(am) >> 1) & 31u); }
inline pk_mi355_am_t *TagView(ViewGen *g) { return reinterpret_cast<pk_mi355_am_t *>(reinterpret_cast<uintptr_t>(g) | (uintptr_t(g->serial) << 1) | 1u); }
// under g_arena_mu
ViewGen *NewGenRecord(pk_mi355_am_t *am, ArenaRec *a, int views) {
  ViewGen *v;
  if (g_retired.size() - g_retired_head >= 64) {       // reuse only once 64 later records have been retired after it
    v = g_retired[g_retired_head++];
    if (g_retired_head > 4096) { g_retired.erase(g_retired.begin(), g_retired.begin() + g_retired_head); g_retired_head = 0; }
  } else {
    v = new ViewGen();
    v->serial = 0;
  }
  v->am = am; v->arena = a; v->live = views; v->current = true; v->withheld = false;
  g_gens.insert(v);
  return v;
}
void RetireGenRecord(ViewGen *v) {
  g_gens.erase(v);
  v->serial = (v->serial + 1) & 31u;
  g_retired.push_back(v);
}
ArenaRec *RegisterArena(void *p) { return new ArenaRec{p, true, nullptr}; }
// a new fetch_all: its generation replaces the previous one, whose outstanding views are void by
// contract (they still own their generation record, nothing else)
pk_mi355_am_t *NewViewGen(ArenaRec *a, pk_mi355_am_t *am, int views) {
  std::lock_guard<std::mutex> g(g_arena_mu);
  if (a->cur) {
    a->cur->current = false;
    if (a->cur->live <= 0) RetireGenRecord(a->cur);
  }
  a->cur = NewGenRecord(am, a, views);
  return TagView(a->cur);
}
// The batch is going away: release the arena now, or leave that to the last view of its last fetch_all.
void RetireArena(ArenaRec *a) {
  void *release = nullptr;
  {
    std::lock_guard<std::mutex> g(g_arena_mu);
    a->batch_alive = false;
    if (!a->cur || a->cur->live <= 0) {
      if (a->cur) RetireGenRecord(a->cur);
      release = a->mem;
      delete a;
    }
  }
  if (release) hipHostFree(release);
}
// pk_decodable_destroy on a view: one view fewer in ITS generation; the last view of the current
// generation of a batch that is gone releases the arena.
}  // namespace

namespace pkhost {
void ReleaseArenaView(pk_mi355_am_t *handle) {
  void *release = nullptr;
  {
    std::lock_guard<std::mutex> g(g_arena_mu);
    ViewGen *v = GenOf(handle);
    if (!g_gens.count(v) || v->serial != SerialOf(handle)) return;   // generation already gone: a copy destroyed twice
    if (--v->live > 0) return;
    if (v->current) {
      ArenaRec *a = v->arena;
      if (a->batch_alive) return;                 // the batch releases it (RetireArena) or re-uses it
      release = a->mem;
      delete a;
    }
    RetireGenRecord(v);
  }
  if (release) hipHostFree(release);
}
}  // namespace pkhost

namespace {
// One device-to-host result stream per device (pk_mi355_batch_fetch_all); lives for the process.
hipStream_t ResultStream(int device) {
  static hipStream_t streams[64] = {};
  if (device < 0 || device >= 64) { Fail(PK_MI355_E_INVALID, "device index %d", device); return nullptr; }
  std::lock_guard<std::mutex> g(g_arena_mu);
  if (!streams[device]) {
    hipError_t e = hipStreamCreateWithFlags(&streams[device], hipStreamNonBlocking);
    if (e != hipSuccess) { Fail(PK_MI355_E_DEVICE, "result stream: %s", hipGetErrorString(e)); return nullptr; }
  }
  return streams[device];
}
}  // namespace

// ================================================================== front-end + batch

struct pk_mi355_batch {
  ScorerCore core;         // model, stream, front-end tables, Yt, log-likelihood rows, the first lane's layer buffers
  Timer timer;
  int max_utts = 0;
  int64_t max_samples = 0;
  // PCM
  float *d_wave = nullptr;          // owned float buffer
  int16_t *d_wave_i16 = nullptr;    // owned int16 buffer
  const float *wave_f32 = nullptr;  // what the kernels read (owned or external)
  const int16_t *wave_i16 = nullptr;
  // What the last set_* call handed over, and so what score's plan (pk_plan.h) starts from: audio, raw features in
  // d_raw or normalised features at `feats`.
  pkplan::Source source = pkplan::kNoSource;
  bool features_only = false;       // made by pk_mi355_features_batch_create: no PCM capacity, the wave entries are refused
  bool have_stats = false;          // the CMVN tables and d_raw exist (always, for a wave batch)
  // made by pk_mi355_frontend_batch_create: the spec's tables; score then runs FbankAnyKernel instead of FbankKernel
  FrontendAnyTables *d_any = nullptr;
  // owned [max_frames][feat_dim], made by EnsureBuffers: what every normalising kernel writes, and the staging of host
  // features handed over as NORMALIZED
  float *d_feats = nullptr;
  const float *feats = nullptr;     // normalised features, frame-major (d_feats or the caller's device pointer)
  // pk_mi355_resample_set_waves: the utterances that are not at 16 kHz wait here at their own rate, page-locked and
  // on the device (both made and grown on demand), and are converted straight into d_wave
  Resampler resampler;
  float *h_native = nullptr, *d_native = nullptr;
  int64_t native_cap = 0;
  // per-utterance placement
  int num_utts = 0;
  int max_T = 0;
  int64_t total_frames = 0, total_cols = 0;
  int64_t dirty_cols = 0;           // columns of d_yt that may hold an earlier layout's features (SetLayout zeroes what a smaller one leaves behind)
  // What a set call uploads -- wave_off, raw_base, pad_base, T (num_utts entries each) and, when a shift is not zero,
  // shift4 -- lies in ONE page-locked block, packed, and goes to a device block of the same shape in one copy with
  // ev_layout recorded behind it; the next set call waits for that event before it rewrites the host block.
  char *h_lay = nullptr, *d_lay = nullptr;
  hipEvent_t ev_layout = nullptr;
  int64_t *h_wave_off = nullptr, *h_raw_base = nullptr, *h_pad_base = nullptr;   // into h_lay
  int32_t *h_T = nullptr;
  UttLayout lay{};                  // the same arrays in d_lay
  // Rows of the layer stack and of d_ll: COMPACT -- utterance after utterance, each padded to a multiple of four rows, no
  // rows for the L + R context pads that separate two utterances in Yt (1 % of the matrix work at 10 s); the first
  // layer finds row j's features at column (f16 modes: row of the split copy) j + shift4[j / 4].
  // The rows end at the last frame of the last utterance that has frames: the padding behind it belongs to nobody.
  std::vector<int64_t> h_out_base;  // first row of utterance u
  int64_t total_rows = 0;
  bool compact = false;
  const int32_t *d_shift4 = nullptr;   // in d_lay; null when every shift of the layout is zero (one utterance at column 0) or rows = columns
  // stages
  float *d_raw_alloc = nullptr;
  float *d_raw = nullptr;   // [max_frames][base_dim]; kCmvnRawLead floats into d_raw_alloc where CmvnKernel runs (EnsureBuffers)
  // The normalisation spec (pk_mi355_norm_set).  Anything but SLIDING: NormKernel (or, for NONE,
  // nothing) stands in front of FeatureLayoutKernel, from d_raw into d_feats; the buffers below are made by norm_set.
  pk_mi355_norm_spec_t norm{PK_MI355_NORM_SLIDING, 1, 0};
  double *d_norm_stats = nullptr;   // [max_utts][2][feat_dim + 1]: the records an UTTERANCE-mode score writes
  float *d_spk_table = nullptr;     // [max_utts][2][feat_dim]: offsets and scales of the speaker records handed over
  int spk_utts = -1;                // the utterances the pending speaker records are for (-1: none pending)
  bool norm_stats_valid = false;    // the last score call was one in UTTERANCE mode on raw rows or audio
  // Online CMVN (pk_mi355_norm_set_online_cmvn): norm.mode is pknorm::kNormOnlineCmvn and
  // OnlineCmvnKernel stands where NormKernel would; the buffers are made by the first such call.
  pk_mi355_online_cmvn_spec_t online_cmvn{600, 600, 200, 0};
  double *d_online_glob = nullptr;  // [2][feat_dim + 1]: the global record
  double *d_online_spk = nullptr;   // [max_utts][2][feat_dim + 1]: the speaker records handed over for the next score
  // Deltas (pk_mi355_deltas_batch_create): everything in front of DeltaKernel -- the front-end,
  // the raw rows, the normalisation, its records -- works at base_dim = feat_dim / (order + 1); on every other batch
  // base_dim is feat_dim and nothing below is made.
  int base_dim = 0;
  bool has_deltas = false;
  pk_mi355_deltas_spec_t deltas{0, 0};
  float *d_delta_scales = nullptr;  // the spec's scale table (pkdelta::BuildScales)
  float *d_delta = nullptr;         // [max_frames][in_dim]: DeltaKernel's result, which the next stage reads
  // The transform (pk_mi355_transform_batch_create): the last stages in front of the layout.
  // in_dim is the width of the rows the global matrix reads (feat_dim on every other batch, and without a global matrix).
  int in_dim = 0;
  bool is_xform = false;            // made by pk_mi355_transform_batch_create
  pkmi::TransformStage xform{};     // the global stage (mt null: none); mt is owned
  float *d_xform = nullptr;         // [max_frames][feat_dim]: the global stage's result
  float *d_umats = nullptr;         // [max_utts][feat_dim + 1][Ldo(feat_dim)]: the matrices handed over for the next score
  float *d_uxform = nullptr;        // [max_frames][feat_dim]: the per-utterance stage's result
  int umat_utts = -1;               // the utterances the pending matrices are for (-1: none pending)
  bool umat_affine = false;
  _Float16 *d_y2 = nullptr;   // f16x3: interleaved (hi, lo) rows [ldy][2 feat_dim]
  float *h_ll = nullptr;    // page-locked mirror of d_ll (pk_mi355_batch_fetch_all), made on first use
  ArenaRec *arena = nullptr;  // its shared-ownership record
  hipEvent_t ev_scored = nullptr, ev_fetched = nullptr;
  // Optional second lane for the layer stack (PK_MI355_LANES=2): odd chunks run on their own
  // stream and buffers, so the HBM-bound tail of one chunk overlaps the MFMA-bound GEMMs of the
  // next (+1.7 % f32, +2.8 % f16x3 on 256 x 10 s).  Off by default: two GEMMs then share the
  // chip, every launch takes twice as long, and per-launch durations stop being a roofline
  // measurement.
  int lanes = 1;
  hipStream_t stream2 = nullptr;
  ExecBufs exec2;
  hipEvent_t ev_front = nullptr, ev_lane2 = nullptr;
  bool scored = false;
  // f16 modes: the range words of the last score call wait in the page-locked mirrors until the stream has
  // been synchronised; the verdict is then sticky until the next score (every delivering call repeats it)
  bool range_pending = false;
  int range_status = 0;
  char range_msg[512] = "";
};

namespace {

constexpr size_t kLayoutEntry = 3 * sizeof(int64_t) + sizeof(int32_t);   // bytes of one utterance in the layout block (h_lay, d_lay)

// Frames and columns (every utterance with its context pads) against the batch's capacity.
int FramesFit(const pk_mi355_batch *b, const int *frames, int num_utts) {
  const int pad = ContextPad(b->core.am);
  int64_t raw = 0, col = 0;
  for (int u = 0; u < num_utts; ++u) {
    raw += frames[u];
    col += frames[u] > 0 ? frames[u] + pad : 0;
  }
  if (raw > b->core.max_frames || RoundUp(col, kTile) > b->core.max_cols)
    return Fail(PK_MI355_E_INVALID, "frame capacity exceeded (%lld frames, %lld columns; the batch holds %lld and %lld)", (long long)raw,
                (long long)RoundUp(col, kTile), (long long)b->core.max_frames, (long long)b->core.max_cols);
  return 0;
}

// The layout of a call, from the utterances' frame counts: placement in the raw rows and in Yt, compact rows, shift4,
// the capacity checks and the dirty_cols rule.  num_samples: the PCM behind the frames (null for features).  The
// counts have been checked (utterances, no negative one, PCM capacity); nothing changes when the frames do not fit.
// Queues one upload and waits for nothing but the upload before it: the callers' own copies out of pageable memory
// (waves, features) have read their source when hipMemcpyAsync returns, as for every pageable source.
int SetLayoutFrames(pk_mi355_batch *b, const int *frames, const int *num_samples, int num_utts) {
  if (int rc = FramesFit(b, frames, num_utts)) return rc;
  ScorerCore &c = b->core;
  const int pad = ContextPad(c.am);
  HIP_TRY(hipEventSynchronize(b->ev_layout));      // the last layout's upload has left the page-locked block
  const size_t n = (size_t)num_utts;
  size_t bytes = kLayoutEntry * n;                 // wave_off | raw_base | pad_base | T, then shift4 at the next multiple of 256
  b->h_wave_off = reinterpret_cast<int64_t *>(b->h_lay); b->h_raw_base = b->h_wave_off + n; b->h_pad_base = b->h_raw_base + n;
  b->h_T = reinterpret_cast<int32_t *>(b->h_pad_base + n);
  const int64_t *d64 = reinterpret_cast<const int64_t *>(b->d_lay);
  b->lay = UttLayout{d64, reinterpret_cast<const int32_t *>(d64 + 3 * n), d64 + n, d64 + 2 * n};
  int64_t woff = 0, raw = 0, col = 0;
  b->max_T = 0;
  for (int u = 0; u < num_utts; ++u) {
    const int T = frames[u];
    b->h_wave_off[u] = woff; b->h_raw_base[u] = raw; b->h_pad_base[u] = col; b->h_T[u] = T;
    woff += num_samples ? num_samples[u] : 0;
    raw += T;
    col += T > 0 ? T + pad : 0;
    b->max_T = std::max(b->max_T, T);
  }
  // Columns behind this layout's last one that an earlier, larger layout filled: the padded rows of the last tile
  // are computed from them, and in the f16 modes whatever they produce counts towards the range verdict (a loud
  // batch followed by a smaller healthy one must not fail on the loud one's leftovers).  Zero again.
  if (col < b->dirty_cols)
    HIP_TRY(hipMemset2DAsync(c.d_yt + col, sizeof(float) * c.ldy, 0, sizeof(float) * (size_t)(b->dirty_cols - col), c.am->feat_dim, c.stream));
  b->dirty_cols = col;
  b->num_utts = num_utts;
  b->total_frames = raw;
  b->total_cols = col;
  b->scored = false;
  b->h_out_base.resize(num_utts);
  b->total_rows = 0;
  int64_t row = 0;
  std::vector<ShiftSpan> spans;
  bool shifted = false;
  for (int u = 0; u < num_utts; ++u) {
    const int T = b->h_T[u];
    b->h_out_base[u] = b->compact ? row : b->h_pad_base[u] + c.am->time_left;      // (row pad_base + i is virtual frame i - Lh)
    if (T == 0) continue;
    b->total_rows = b->h_out_base[u] + T;
    row += RoundUp(T, 4);
    spans.push_back({row, b->compact ? (int32_t)(b->h_pad_base[u] - b->h_out_base[u]) : 0});
    shifted = shifted || spans.back().shift != 0;
  }
  b->d_shift4 = nullptr;
  if (num_utts == 0) return 0;
  if (shifted) {                                 // (compact rows only; batch_create keeps L + R < 3, whose shifts go negative, out of them)
    bytes = RoundUp(bytes, 256);
    if (!ExpandShift4(spans, b->total_rows, c.zero_span, reinterpret_cast<int32_t *>(b->h_lay + bytes), nullptr))
      return Fail(PK_MI355_E_INVALID, "internal: column shift outside [0, %lld]", (long long)(c.zero_span - kTile));
    b->d_shift4 = reinterpret_cast<const int32_t *>(b->d_lay + bytes);
    bytes += sizeof(int32_t) * Shift4Groups(b->total_rows);
  }
  HIP_TRY(hipMemcpyAsync(b->d_lay, b->h_lay, bytes, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipEventRecord(b->ev_layout, c.stream));
  return 0;
}

// The wave form: fbank's frame count for every utterance's samples (fbank.cc:35-42), then the layout of those frames.
int SetLayout(pk_mi355_batch *b, const int *num_samples, int num_utts) {
  if (num_utts < 0 || num_utts > b->max_utts) return Fail(PK_MI355_E_INVALID, "too many utterances (%d > %d)", num_utts, b->max_utts);
  std::vector<int> frames(num_utts);
  int64_t total = 0;
  for (int u = 0; u < num_utts; ++u) {
    if (num_samples[u] < 0) return Fail(PK_MI355_E_INVALID, "negative sample count");
    frames[u] = pk_mi355_num_frames(num_samples[u]);
    total += num_samples[u];
  }
  if (total > b->max_samples) return Fail(PK_MI355_E_INVALID, "too many samples (%lld > %lld)", (long long)total, (long long)b->max_samples);
  if (int rc = SetLayoutFrames(b, frames.data(), num_samples, num_utts)) return rc;
  b->source = pkplan::kWaves;
  return 0;
}

// What both feature entries check before the device is touched (kind, and RAW's needs).
int CheckFeatureKind(const pk_mi355_batch *b, int kind) {
  if (kind != PK_MI355_FEATS_NORMALIZED && kind != PK_MI355_FEATS_RAW) return Fail(PK_MI355_E_INVALID, "unknown feature kind %d", kind);
  // (statistics are only ever held at the model's own dimension: 41 floats through the 40-dim entries, feat_dim + 1
  // through pk_mi355_features_batch_create_stats)
  if (kind == PK_MI355_FEATS_RAW && !b->have_stats && b->norm.mode == PK_MI355_NORM_SLIDING) {
    if (b->is_xform)
      return Fail(PK_MI355_E_INVALID, "raw features need the CMVN statistics: this batch of %d-dim base features was made without them "
                  "(pk_mi355_transform_batch_create takes %d)", b->base_dim, b->base_dim + 1);
    if (b->has_deltas)
      return Fail(PK_MI355_E_INVALID, "raw features need the CMVN statistics: this batch of %d-dim base features was made without them "
                  "(pk_mi355_deltas_batch_create takes %d)", b->base_dim, b->base_dim + 1);
    if (b->core.am->feat_dim == kNumBins)
      return Fail(PK_MI355_E_INVALID, "raw features need the CMVN statistics and a %d-dim model (this batch: no statistics, %d-dim)", kNumBins,
                  kNumBins);
    return Fail(PK_MI355_E_INVALID, "raw features need the CMVN statistics: this %d-dim batch was made without them "
                "(pk_mi355_features_batch_create_stats takes the %d of a %d-dim model)", b->core.am->feat_dim, b->core.am->feat_dim + 1,
                b->core.am->feat_dim);
  }
  return 0;
}
int CheckFeatureCounts(const pk_mi355_batch *b, const int *frames, int num_utts) {
  if (num_utts < 0 || num_utts > b->max_utts) return Fail(PK_MI355_E_INVALID, "too many utterances (%d > %d)", num_utts, b->max_utts);
  for (int u = 0; u < num_utts; ++u)
    if (frames[u] < 0) return Fail(PK_MI355_E_INVALID, "utterance %d has a negative frame count (%d)", u, frames[u]);
  return FramesFit(b, frames, num_utts);
}
pkplan::BatchShape ShapeOf(const pk_mi355_batch *b) {
  return pkplan::BatchShape{b->base_dim, b->core.am->feat_dim, b->d_any != nullptr, b->has_deltas, b->have_stats, b->is_xform,
                            b->xform.mt ? b->in_dim : 0};
}
// The own rows a plan reads or writes (pkplan::BatchPlan::buffers), made by the first call that needs them: create, for
// what a set call could not make in time, then features_set* and norm_set*.  d_raw [max_frames][base_dim] has its lead
// and its zeroed slack exactly where CmvnKernel runs, which reads around every utterance; every other kernel stays
// within an utterance's own rows.  b->feats is not touched: a caller's NORMALIZED device pointer stays.
hipError_t EnsureBuffers(pk_mi355_batch *b, unsigned need) {
  const size_t frames = (size_t)b->core.max_frames, D = (size_t)b->core.am->feat_dim;
  hipError_t e = hipSuccess;
  if ((need & pkplan::kRawRows) && !b->d_raw) {
    const size_t lead = pkplan::FusedCmvn(ShapeOf(b)) ? kCmvnRawLead : 0, floats = frames * b->base_dim + (lead ? lead + kCmvnRawSlack : 0);
    e = hipMalloc(&b->d_raw_alloc, sizeof(float) * floats);
    if (e == hipSuccess && lead) e = hipMemset(b->d_raw_alloc, 0, sizeof(float) * floats);
    if (e == hipSuccess) b->d_raw = b->d_raw_alloc + lead;
  }
  // (d_feats holds the normalisation's rows at base_dim or the NORMALIZED staging at D; a transform object's base_dim
  // may be the larger.  in_dim is D on every batch without a global matrix.)
  if (e == hipSuccess && (need & pkplan::kFeatRows) && !b->d_feats)
    e = hipMalloc(&b->d_feats, sizeof(float) * frames * std::max(D, (size_t)b->base_dim));
  if (e == hipSuccess && (need & pkplan::kDeltaRows) && !b->d_delta) e = hipMalloc(&b->d_delta, sizeof(float) * frames * (size_t)b->in_dim);
  if (e == hipSuccess && (need & pkplan::kXformRows) && !b->d_xform) e = hipMalloc(&b->d_xform, sizeof(float) * frames * D);
  if (e == hipSuccess && (need & pkplan::kUttXformRows) && !b->d_uxform) e = hipMalloc(&b->d_uxform, sizeof(float) * frames * D);
  return e;
}
// what scoring `source` under `mode` needs of them
unsigned BuffersFor(const pk_mi355_batch *b, pkplan::Source source, int mode) { return pkplan::PlanBatch(ShapeOf(b), source, mode, false).buffers; }
int WaveEntryAllowed(const pk_mi355_batch *b) {
  if (b->features_only) return Fail(PK_MI355_E_STATE, "this batch was made by pk_mi355_features_batch_create: it takes features, not audio");
  return 0;
}

// After the batch's stream has been synchronised: evaluate (once) the range words of the last score call.
int BatchRangeStatus(pk_mi355_batch *b) {
  if (b->range_pending) {
    const ExecBufs *eb[2] = {&b->core.exec, &b->exec2};
    b->range_status = EvalRange(b->core.am, eb, b->lanes == 2 ? 2 : 1);
    if (b->range_status) {
      snprintf(b->range_msg, sizeof(b->range_msg), "%s", LastError());
      // views handed out by fetch_all(sync = 0) before this verdict hold withheld results: make them say so
      std::lock_guard<std::mutex> g(g_arena_mu);
      if (b->arena && b->arena->cur) b->arena->cur->withheld = true;
    }
    b->range_pending = false;
  }
  if (b->range_status) return Fail(b->range_status, "%s", b->range_msg);
  return 0;
}

int64_t TotalSamples(const int *num_samples, int n) {
  int64_t s = 0;
  for (int i = 0; i < n; ++i) s += num_samples[i];
  return s;
}

}  // namespace

namespace pkhost {
bool BatchScored(const pk_mi355_batch *b) { return b->scored; }
const pk_mi355_am *BatchModel(const pk_mi355_batch *b) { return b->core.am; }

void CreateScorerCore(ScorerCore *c, pk_mi355_am *am, const float *global_stats, int stats_dim, int units, int64_t max_frames,
                      int64_t max_rows, int64_t chunk_cap, CreateCheck &chk) {
  const int pad = ContextPad(am);
  c->am = am; c->device = am->device; c->max_frames = max_frames;
  c->max_cols = RoundUp(max_rows + (int64_t)units * pad, kTileF16);
  c->chunk = std::min<int64_t>(chunk_cap, c->max_cols);
  c->zero_span = ZeroSpan(units, pad);
  c->ldy = RoundUp(c->max_cols, c->chunk) + 256 + c->zero_span;
  // a time-splice model's last pass starts up to HaloLeft rows off a tile boundary and runs the virtual frames behind the
  // last utterance: its last tile's padding rows read that much further
  if (HasTimeSplice(am)) c->ldy += RoundUp(HaloLeft(am) + HaloRight(am) + kTile, 256);
  auto table = [&](auto **d, const void *h, size_t bytes) {
    chk(hipMalloc(d, bytes));
    if (chk.ok) chk(hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice));
  };
  chk(hipStreamCreate(&c->stream));
  if (global_stats) {
    if (stats_dim == kNumBins) {
      FrontendTables host;
      if (BuildFrontendTables(&host)) { chk.ok = false; Fail(PK_MI355_E_INVALID, "front-end table construction failed"); }
      table(&c->d_tables, &host, sizeof(FrontendTables));
    }
    CmvnTables ctab;
    BuildCmvnTables(global_stats[stats_dim], &ctab);
    table(&c->d_global, global_stats, sizeof(float) * (stats_dim + 1));
    table(&c->d_cmvn_tab, &ctab, sizeof(CmvnTables));
  }
  chk(hipMalloc(&c->d_yt, sizeof(float) * c->ldy * am->feat_dim));
  if (chk.ok) chk(hipMemset(c->d_yt, 0, sizeof(float) * c->ldy * am->feat_dim));   // the zero span at the end of feature row 0
  chk(hipMalloc(&c->d_ll, sizeof(float) * c->max_cols * am->num_pdfs));
  if (chk.ok && AllocExec(am, ExecRows(am, c->chunk), &c->exec)) chk.ok = false;
}

void FreeScorerCore(ScorerCore *c) {
  FreeExec(&c->exec);
  hipFree(c->d_tables); hipFree(c->d_global); hipFree(c->d_cmvn_tab); hipFree(c->d_yt); hipFree(c->d_ll);
  if (c->stream) hipStreamDestroy(c->stream);
}

bool ExpandShift4(const std::vector<ShiftSpan> &spans, int64_t total_rows, int64_t zero_span, int32_t *shift4, int32_t *bad) {
  int32_t shift = 0;
  int64_t g = 0;                                   // the next group to fill
  for (const ShiftSpan &sp : spans) {
    shift = sp.shift;
    if (shift < 0 || shift + kTile > zero_span) { if (bad) *bad = shift; return false; }
    for (; g < sp.end_row / 4; ++g) shift4[g] = shift;
  }
  for (const int64_t groups = Shift4Groups(total_rows); g < groups; ++g) shift4[g] = shift;
  return true;
}
}  // namespace pkhost

extern "C" {

int pk_mi355_num_frames(int num_samples) {      // fbank.cc:35-42
  if (num_samples < kFrameLength) return 0;
  return 1 + (num_samples - kFrameLength) / kFrameShift;
}

}  // extern "C"

namespace {
// Frames per pass through the layer stack at most, for a batch made through the ABI (PK_MI355_CHUNK overrides).  Without
// the fused tail the size hardly matters (256 x 10 s: 65536 -> 25.92, 131072 -> 25.79, 262144 -> 25.78 ms per step); with
// it every last-layer launch ends in ~0.25 ms of tail phases on an emptying chip, so fewer, larger passes win:
// 65536 -> 25.45, 131072 -> 25.0, 262144 -> 24.75 (profiles/r04_fused_tail32.txt)
int64_t PublicChunkCap() {
  const char *e = getenv("PK_MI355_CHUNK");
  return e && atol(e) >= kTile ? RoundUp(atol(e), kTileF16) : 262144;
}

// Every way to a batch: the request and what its checks worked out (SingleBatch: through no check).  max_samples PCM
// samples (0: features only), max_frames frames, passes of at most chunk_cap frames.
pk_mi355_batch *CreateBatch(pk_mi355_am_t *am, const CreateRequest &r, const CreateDims &dims) {
  if (UseDevice(am->device)) return nullptr;
  const pk_mi355_deltas_spec_t *deltas = r.deltas;
  const int64_t max_frames = r.audio ? r.capacity / kFrameShift + r.units : r.capacity;
  pk_mi355_batch *b = new pk_mi355_batch();
  ScorerCore &c = b->core;
  b->max_utts = r.units; b->max_samples = r.audio ? r.capacity : 0;
  b->features_only = !r.audio;
  b->have_stats = r.stats != nullptr;
  b->has_deltas = deltas != nullptr;
  if (deltas) b->deltas = *deltas;
  b->is_xform = r.xform != nullptr;
  b->in_dim = dims.in_dim; b->base_dim = dims.base_dim;
  const int pad = ContextPad(am);
  CreateCheck chk{b->features_only ? "batch_create_features" : "batch_create"};
  CreateScorerCore(&c, am, r.stats, b->base_dim, r.units, max_frames, max_frames, r.chunk_cap ? r.chunk_cap : PublicChunkCap(), chk);
  // Compact rows pad every utterance's rows to four but not its columns: the column shift of utterance u is the sum over
  // the utterances before it of T + pad - RoundUp(T, 4), which goes negative once pad < 3 (pad = 0: after any length that
  // is not a multiple of four), and the rows can then outnumber the columns every buffer is sized for.  The kernels add
  // the shift to UNSIGNED 32-bit lane offsets of scalar-base LDS-DMA (gemm.hip issue_splice, gemm_f16.hip xoff), where a
  // negative value addresses 4 GiB further on.  With fewer than three context frames there are next to no pad rows to
  // save anyway: such models keep row = column of Yt.
  // A time-splice model's rows include the virtual frames in front of and behind every utterance: row = column of Yt too.
  b->compact = pad >= 3 && !HasTimeSplice(am);
  if (const char *e = getenv("PK_MI355_COMPACT_ROWS")) b->compact = b->compact && atoi(e) != 0;    // (A/B switch: 0 = row = column of Yt)
  const size_t lay_bytes = RoundUp(kLayoutEntry * r.units, 256) + (b->compact ? sizeof(int32_t) * Shift4Cap(c.max_cols) : 0);
  chk(hipHostMalloc(reinterpret_cast<void **>(&b->h_lay), lay_bytes, hipHostMallocDefault));
  chk(hipMalloc(&b->d_lay, lay_bytes));
  chk(hipEventCreateWithFlags(&b->ev_layout, hipEventDisableTiming));
  if (dims.any()) UploadSpecTables(&c, dims.any(), &b->d_any, chk);
  // TransformKernel's global matrix (before the plan below is asked for its rows)
  if (r.xform && pkxf::HasMatrix(*r.xform)) b->xform = UploadTransform(*r.xform, chk);
  // The rows of the SLIDING plan of an object with statistics; every other plan's are made by the set call that brings it
  // about.  A wave batch has no such call for its audio (everything now); a features-only one gets its raw rows.
  if (b->have_stats) chk(EnsureBuffers(b, b->features_only ? pkplan::kRawRows : BuffersFor(b, pkplan::kWaves, PK_MI355_NORM_SLIDING)));
  if (deltas) b->d_delta_scales = UploadDeltaScales(*deltas, chk);     // DeltaKernel's table
  if (IsF16(am->precision)) chk(hipMalloc(&b->d_y2, sizeof(_Float16) * 2 * c.ldy * am->feat_dim));
  if (const char *e = getenv("PK_MI355_LANES")) b->lanes = atoi(e) >= 2 ? 2 : 1;
  if (c.max_cols <= c.chunk) b->lanes = 1;           // a single chunk has nothing to overlap with
  if (b->lanes == 2) {
    chk(hipStreamCreate(&b->stream2));
    chk(hipEventCreateWithFlags(&b->ev_front, hipEventDisableTiming));
    chk(hipEventCreateWithFlags(&b->ev_lane2, hipEventDisableTiming));
    if (chk.ok && AllocExec(am, ExecRows(am, c.chunk), &b->exec2)) chk.ok = false;
  }
  if (!chk.ok) { pk_mi355_batch_destroy(b); return nullptr; }
  return b;
}

// am->mu held.  One of the model's own one-utterance scorers for a call of `need` samples or frames: kept while the call
// fits and `keep` holds, otherwise destroyed and made again by make(capacity), the capacity at least doubled.
template <class Make>
pk_mi355_batch *EnsureOwned(OwnedBatch *o, int64_t need, bool keep, Make make) {
  if (o->b && need <= o->cap && keep) return o->b;
  if (o->b) pk_mi355_batch_destroy(o->b);
  o->cap = std::max<int64_t>(need, 2 * o->cap);
  o->b = make(o->cap);
  if (!o->b) o->cap = 0;
  return o->b;
}
}  // namespace

namespace pkhost {
// The argument checks of every public create entry of both scorers (pk_score.h), in the one order of DESIGN.md section
// 28, also when several arguments are bad at once; an entry runs those its request gives rise to.
bool CheckCreate(const pk_mi355_am *am, const CreateRequest &r, CreateDims *dims) {
  if (!CheckRequestArgs(am && (r.live || am->finalized), r, dims)) return false;      // the model, null arguments, the specs
  if (r.live) {                      // an online scorer: the model is looked at from here on, so the above is said without a device
    if (am->precision != PK_MI355_PRECISION_F32) {
      Fail(PK_MI355_E_INVALID, "the online scorer runs f32 models only (the f16 modes' calibration and range verdict are per batch)");
      return false;
    }
    if (!am->finalized) { Fail(PK_MI355_E_STATE, "model not finalized"); return false; }
    if (HasTimeSplice(am)) { Fail(PK_MI355_E_INVALID, "time-splice layers are not supported by the online scorers yet"); return false; }
  }
  const int D = am->feat_dim, order = r.deltas ? r.deltas->order : 0;
  // what the stages in front of the first layer start from: the model's features, or the rows a transform reads
  const int Din = r.xform ? r.xform->in_dim : D;
  if (r.xform && Din % (order + 1) != 0) {
    Fail(PK_MI355_E_INVALID, "deltas of order %d make %d blocks, which does not divide the transform's in_dim %d", order, order + 1, Din);
    return false;
  }
  if (Din % (order + 1) != 0) {
    Fail(PK_MI355_E_INVALID, "deltas of order %d make %d blocks, which does not divide the model's %d-dim features", order, order + 1, D);
    return false;
  }
  const int Db = Din / (order + 1);
  if (!r.live && !BuildRequestTables(r, dims)) return false;      // (a batch entry names a bad front-end spec here)
  const int front_dim = r.frontend ? dims->any()->dim : kNumBins;
  if (r.xform && r.audio && front_dim != Db) {
    Fail(PK_MI355_E_INVALID, "the front-end spec produces %d-dim features, the transform's in_dim %d with %d delta blocks needs %d", front_dim, Din,
         order + 1, Db);
    return false;
  }
  if (!r.xform && r.audio && !FrontendFits(front_dim, r.frontend != nullptr, am, Db, order)) return false;
  if (r.stats && !r.stats41 && !StatsLenFits(r.stats_len, Db, r.deltas != nullptr || r.xform != nullptr)) return false;
  if (r.xform && pkxf::OutDim(*r.xform) != D) {
    Fail(PK_MI355_E_INVALID, "the transform produces %d-dim features, the model expects %d", pkxf::OutDim(*r.xform), D);
    return false;
  }
  // The one place where capacity is refused.  An audio object without statistics has always been named so (only
  // pk_mi355_batch_create and pk_mi355_stream_create can ask for one); a live step's staging is indexed in 32 bits.
  const bool no_stats = r.audio && !r.stats && (r.live || !r.frontend);
  if (r.units <= 0 || r.capacity <= 0 || no_stats || (r.live && r.capacity > ((int64_t)1 << 30) / (r.audio ? 1 : std::max(D, Db)))) {
    Fail(PK_MI355_E_INVALID, r.live ? "bad stream capacity" : "bad batch capacity");
    return false;
  }
  if (r.stats && r.stats41 && D != kNumBins) {
    Fail(PK_MI355_E_INVALID, "the CMVN statistics are for %d-dim features, the model expects %d", kNumBins, D);
    return false;
  }
  if (IsF16(am->precision) && D % 8 != 0) {      // as pk_decodable_init: the spliced view of the split copy needs whole 8-k chunks
    Fail(PK_MI355_E_INVALID, "f16x3 / f16 precision needs a feature dimension that is a multiple of 8 (got %d)", D);
    return false;
  }
  dims->in_dim = Din; dims->base_dim = Db;
  return true;
}

pk_mi355_batch *CheckedBatch(pk_mi355_am *am, const CreateRequest &r) {
  CreateDims dims;
  return CheckCreate(am, r, &dims) ? CreateBatch(am, r, dims) : nullptr;
}

float *UploadDeltaScales(const pk_mi355_deltas_spec_t &deltas, CreateCheck &chk) {
  float table[pkdelta::kMaxTable], *d_scales = nullptr;
  pkdelta::BuildScales(deltas, table);
  const size_t bytes = sizeof(float) * (size_t)(deltas.order + 1) * pkdelta::RowLen(deltas);
  chk(hipMalloc(&d_scales, bytes));
  if (chk.ok) chk(hipMemcpy(d_scales, table, bytes, hipMemcpyHostToDevice));
  return d_scales;
}

pkmi::TransformStage UploadTransform(const pk_mi355_transform_spec_t &x, CreateCheck &chk) {
  pkmi::TransformStage stage{x.in_dim, x.left_context, x.right_context, pkxf::OutDim(x), false, nullptr, 0};
  if (!pkxf::HasMatrix(x)) return stage;
  std::vector<float> packed((size_t)x.cols * pkxf::Ldo(x.rows));
  pkxf::PackTransposed(x.matrix, x.rows, x.cols, packed.data());
  float *d_mt = nullptr;
  chk(hipMalloc(&d_mt, sizeof(float) * packed.size()));
  if (chk.ok) chk(hipMemcpy(d_mt, packed.data(), sizeof(float) * packed.size(), hipMemcpyHostToDevice));
  stage.affine = pkxf::Affine(x); stage.mt = d_mt;
  return stage;
}

pk_mi355_batch *SingleBatch(pk_mi355_am *am, int64_t frames) {      // (at least one whole pass: every pass is kSingleChunk rows)
  return EnsureOwned(&am->single, std::max(frames, kSingleChunk), true, [&](int64_t cap) {
    CreateRequest r{nullptr, 0, false, 1, cap, false, false, nullptr, nullptr};
    r.chunk_cap = kSingleChunk;
    CreateDims dims;
    dims.in_dim = dims.base_dim = am->feat_dim;
    return CreateBatch(am, r, dims);
  });
}
}  // namespace pkhost

extern "C" {

pk_mi355_batch_t *pk_mi355_batch_create(pk_mi355_am_t *am, const float *global_stats41, int max_utts, int64_t max_total_samples) {
  return CheckedBatch(am, CreateRequest{global_stats41, 0, true, max_utts, max_total_samples, true, false, nullptr, nullptr});
}

pk_mi355_batch_t *pk_mi355_features_batch_create(pk_mi355_am_t *am, const float *global_stats41, int max_utts, int64_t max_total_frames) {
  return CheckedBatch(am, CreateRequest{global_stats41, 0, true, max_utts, max_total_frames, false, false, nullptr, nullptr});
}

pk_mi355_batch_t *pk_mi355_features_batch_create_stats(pk_mi355_am_t *am, const float *global_stats, int stats_len, int max_utts,
                                                       int64_t max_total_frames) {
  return CheckedBatch(am, CreateRequest{global_stats, stats_len, false, max_utts, max_total_frames, false, !global_stats, nullptr, nullptr});
}

pk_mi355_batch_t *pk_mi355_frontend_batch_create(pk_mi355_am_t *am, const pk_mi355_frontend_spec_t *spec, const float *global_stats,
                                                 int stats_len, int max_utts, int64_t max_total_samples) {
  return CheckedBatch(am, CreateRequest{global_stats, stats_len, false, max_utts, max_total_samples, true, !spec || !global_stats, spec, nullptr});
}

pk_mi355_batch_t *pk_mi355_deltas_batch_create(pk_mi355_am_t *am, const pk_mi355_deltas_spec_t *deltas, const pk_mi355_frontend_spec_t *frontend,
                                               const float *global_stats, int stats_len, int max_utts, int64_t capacity) {
  return CheckedBatch(am, CreateRequest{global_stats, stats_len, false, max_utts, capacity, frontend != nullptr, !deltas || (frontend && !global_stats),
                                       frontend, deltas});
}

int pk_mi355_deltas_base_dim(const pk_mi355_batch_t *b) { return b ? b->base_dim : 0; }

pk_mi355_batch_t *pk_mi355_transform_batch_create(pk_mi355_am_t *am, const pk_mi355_transform_spec_t *transform, const pk_mi355_deltas_spec_t *deltas,
                                                  const pk_mi355_frontend_spec_t *frontend, const float *global_stats, int stats_len, int max_utts,
                                                  int64_t capacity) {
  return CheckedBatch(am, CreateRequest{global_stats, stats_len, false, max_utts, capacity, frontend != nullptr, !transform || (frontend && !global_stats),
                                       frontend, deltas, transform});
}

int pk_mi355_transform_in_dim(const pk_mi355_batch_t *b) { return b ? b->in_dim : 0; }

int pk_mi355_transform_set_utt(pk_mi355_batch_t *b, const float *mats, int rows, int cols, int num_utts) {
  if (!b || (num_utts > 0 && !mats)) return Fail(PK_MI355_E_INVALID, "null argument");
  if (!b->is_xform) return Fail(PK_MI355_E_STATE, "per-utterance transforms need a batch made by pk_mi355_transform_batch_create");
  if (num_utts < 0 || num_utts > b->max_utts) return Fail(PK_MI355_E_INVALID, "too many utterances (%d > %d)", num_utts, b->max_utts);
  const int D = b->core.am->feat_dim;
  if (rows != D) return Fail(PK_MI355_E_INVALID, "per-utterance transforms have %d rows, the model's features need %d", rows, D);
  if (cols != D && cols != D + 1)
    return Fail(PK_MI355_E_INVALID, "per-utterance transforms have %d columns, the model's %d-dim features need %d (linear) or %d (affine)", cols, D, D,
                D + 1);
  const size_t each = (size_t)rows * cols, packed_each = (size_t)cols * pkxf::Ldo(rows);
  const int64_t bad = pkxf::FirstNonFinite(mats, (int64_t)(each * (size_t)num_utts));
  if (bad >= 0)
    return Fail(PK_MI355_E_INVALID, "the transform of utterance %d has an entry that is not finite (row %d, column %d)", (int)(bad / (int64_t)each),
                (int)(bad % (int64_t)each / cols), (int)(bad % cols));
  if (int rc = UseDevice(b->core.device)) return rc;
  HIP_TRY(EnsureBuffers(b, pkplan::kUttXformRows));
  if (!b->d_umats) HIP_TRY(hipMalloc(&b->d_umats, sizeof(float) * (size_t)(D + 1) * pkxf::Ldo(D) * (size_t)b->max_utts));
  if (num_utts > 0) {                                   // (pageable memory: the copy has read the matrices when the call returns)
    std::vector<float> packed(packed_each * (size_t)num_utts);
    for (int u = 0; u < num_utts; ++u) pkxf::PackTransposed(mats + each * u, rows, cols, packed.data() + packed_each * u);
    HIP_TRY(hipMemcpyAsync(b->d_umats, packed.data(), sizeof(float) * packed.size(), hipMemcpyHostToDevice, b->core.stream));
    HIP_TRY(hipStreamSynchronize(b->core.stream));
  }
  b->umat_utts = num_utts;
  b->umat_affine = cols == D + 1;
  return 0;
}

int pk_mi355_features_dim(const pk_mi355_batch_t *b) { return b ? b->core.am->feat_dim : 0; }

void pk_mi355_batch_destroy(pk_mi355_batch_t *b) {
  if (!b) return;
  hipSetDevice(b->core.device);
  if (b->core.stream) hipStreamSynchronize(b->core.stream);
  if (b->stream2) hipStreamSynchronize(b->stream2);
  FreeExec(&b->exec2);
  for (hipEvent_t e : {b->ev_front, b->ev_lane2, b->ev_scored, b->ev_fetched, b->ev_layout}) if (e) hipEventDestroy(e);
  if (b->stream2) hipStreamDestroy(b->stream2);
  hipFree(b->d_wave); hipFree(b->d_wave_i16); hipFree(b->d_raw_alloc); hipFree(b->d_y2); hipFree(b->d_feats); hipFree(b->d_any);
  hipFree(b->d_delta); hipFree(b->d_delta_scales);
  hipFree(const_cast<float *>(b->xform.mt)); hipFree(b->d_xform); hipFree(b->d_umats); hipFree(b->d_uxform);
  hipFree(b->d_norm_stats); hipFree(b->d_spk_table); hipFree(b->d_online_glob); hipFree(b->d_online_spk);
  b->resampler.Free();
  if (b->h_native) hipHostFree(b->h_native);
  hipFree(b->d_native);
  if (b->h_lay) hipHostFree(b->h_lay);
  hipFree(b->d_lay);
  if (b->arena) RetireArena(b->arena);   // released now, or by the last outstanding view of the last fetch_all
  FreeScorerCore(&b->core);
  delete b;
}

int pk_mi355_batch_set_waves(pk_mi355_batch_t *b, const pk_vector_t *waves, int num_utts) {
  if (!b || !waves) return Fail(PK_MI355_E_INVALID, "null argument");
  if (int rc = WaveEntryAllowed(b)) return rc;
  if (int rc = UseDevice(b->core.device)) return rc;
  std::vector<int> ns(num_utts);
  for (int u = 0; u < num_utts; ++u) ns[u] = waves[u].dim;
  if (TotalSamples(ns.data(), num_utts) > b->max_samples) return Fail(PK_MI355_E_INVALID, "too many samples");
  if (!b->d_wave) HIP_TRY(hipMalloc(&b->d_wave, sizeof(float) * b->max_samples));
  int64_t off = 0;
  for (int u = 0; u < num_utts; ++u) {
    if (ns[u] > 0)
      HIP_TRY(hipMemcpyAsync(b->d_wave + off, waves[u].data, sizeof(float) * ns[u], hipMemcpyHostToDevice, b->core.stream));
    off += ns[u];
  }
  b->wave_f32 = b->d_wave;
  b->wave_i16 = nullptr;
  return SetLayout(b, ns.data(), num_utts);
}

int pk_mi355_resample_set_waves(pk_mi355_batch_t *b, const pk_vector_t *waves, const int *rates, int num_utts) {
  if (!b || !waves) return Fail(PK_MI355_E_INVALID, "null argument");
  if (int rc = WaveEntryAllowed(b)) return rc;
  bool native = false;
  for (int u = 0; rates && u < num_utts; ++u) native = native || rates[u] != kSampleRate;
  if (!native) return pk_mi355_batch_set_waves(b, waves, num_utts);      // 16 kHz throughout: today's call, launch for launch
  if (num_utts > b->max_utts) return Fail(PK_MI355_E_INVALID, "too many utterances (%d > %d)", num_utts, b->max_utts);
  if (int rc = UseDevice(b->core.device)) return rc;
  // every utterance's length at 16 kHz and the native samples to stage, checked before anything is copied
  std::vector<int> ns(num_utts);
  std::vector<const DeviceResampleTable *> tab(num_utts, nullptr);
  int64_t total_native = 0;
  for (int u = 0; u < num_utts; ++u) {
    if (waves[u].dim < 0) return Fail(PK_MI355_E_INVALID, "negative sample count");
    if (rates[u] == kSampleRate) { ns[u] = waves[u].dim; continue; }
    if (int rc = b->resampler.Table(rates[u], &tab[u])) return rc;
    const int64_t n_out = ResampleNumOutput(tab[u]->host, waves[u].dim);
    if (n_out > b->max_samples) return Fail(PK_MI355_E_INVALID, "too many samples");
    ns[u] = (int)n_out;
    total_native += waves[u].dim;
  }
  if (TotalSamples(ns.data(), num_utts) > b->max_samples) return Fail(PK_MI355_E_INVALID, "too many samples");
  if (!b->d_wave) HIP_TRY(hipMalloc(&b->d_wave, sizeof(float) * b->max_samples));
  HIP_TRY(hipStreamSynchronize(b->core.stream));       // the previous call has left the staging buffers
  if (total_native > b->native_cap) {
    const int64_t cap = std::max<int64_t>(total_native, 2 * b->native_cap);
    if (b->h_native) hipHostFree(b->h_native);
    hipFree(b->d_native);
    b->h_native = nullptr; b->d_native = nullptr; b->native_cap = 0;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&b->h_native), sizeof(float) * cap, hipHostMallocDefault));
    HIP_TRY(hipMalloc(&b->d_native, sizeof(float) * cap));
    b->native_cap = cap;
  }
  std::vector<ResampleItem> items;
  int64_t off = 0, noff = 0;
  for (int u = 0; u < num_utts; ++u) {
    const int n = waves[u].dim;
    if (!tab[u]) {
      if (n > 0) HIP_TRY(hipMemcpyAsync(b->d_wave + off, waves[u].data, sizeof(float) * n, hipMemcpyHostToDevice, b->core.stream));
    } else {
      if (n > 0) memcpy(b->h_native + noff, waves[u].data, sizeof(float) * n);
      if (ns[u] > 0) items.push_back(Resampler::Item(*tab[u], b->d_native + noff, 0, n, 0, ns[u], b->d_wave + off));
      noff += n;
    }
    off += ns[u];
  }
  if (total_native > 0)
    HIP_TRY(hipMemcpyAsync(b->d_native, b->h_native, sizeof(float) * total_native, hipMemcpyHostToDevice, b->core.stream));
  if (int rc = b->resampler.Run(items, b->core.stream)) return rc;
  b->wave_f32 = b->d_wave;
  b->wave_i16 = nullptr;
  return SetLayout(b, ns.data(), num_utts);
}

int pk_mi355_batch_set_waves_i16(pk_mi355_batch_t *b, const int16_t *samples, const int *num_samples,
                                 int num_utts) {
  if (!b || !samples || !num_samples) return Fail(PK_MI355_E_INVALID, "null argument");
  if (int rc = WaveEntryAllowed(b)) return rc;
  if (int rc = UseDevice(b->core.device)) return rc;
  const int64_t total = TotalSamples(num_samples, num_utts);
  if (total > b->max_samples) return Fail(PK_MI355_E_INVALID, "too many samples");
  if (!b->d_wave_i16) HIP_TRY(hipMalloc(&b->d_wave_i16, sizeof(int16_t) * b->max_samples));
  if (total > 0)
    HIP_TRY(hipMemcpyAsync(b->d_wave_i16, samples, sizeof(int16_t) * total, hipMemcpyHostToDevice, b->core.stream));
  b->wave_i16 = b->d_wave_i16;
  b->wave_f32 = nullptr;
  return SetLayout(b, num_samples, num_utts);
}

int pk_mi355_batch_set_waves_device(pk_mi355_batch_t *b, const float *d_samples, const int *num_samples,
                                    int num_utts) {
  if (!b || !d_samples || !num_samples) return Fail(PK_MI355_E_INVALID, "null argument");
  if (int rc = WaveEntryAllowed(b)) return rc;
  if (int rc = UseDevice(b->core.device)) return rc;
  b->wave_f32 = d_samples;
  b->wave_i16 = nullptr;
  return SetLayout(b, num_samples, num_utts);
}

int pk_mi355_features_set(pk_mi355_batch_t *b, const pk_matrix_t *feats, int num_utts, int kind) {
  if (!b || (num_utts > 0 && !feats)) return Fail(PK_MI355_E_INVALID, "null argument");
  if (int rc = CheckFeatureKind(b, kind)) return rc;
  const int D = kind == PK_MI355_FEATS_RAW ? b->base_dim : b->core.am->feat_dim;      // (a deltas batch: RAW rows are in front of the deltas)
  std::vector<int> frames(std::max(num_utts, 0));
  for (int u = 0; u < num_utts; ++u) {
    if (feats[u].nrow != D && b->is_xform)
      return Fail(PK_MI355_E_INVALID, "features of utterance %d have %d rows, this batch expects %d (%s)", u, feats[u].nrow, D,
                  kind == PK_MI355_FEATS_RAW ? "raw rows in front of the transform" : "normalised rows at the model's dimension");
    if (feats[u].nrow != D && b->has_deltas)
      return Fail(PK_MI355_E_INVALID, "features of utterance %d have %d rows, this batch expects %d (%s)", u, feats[u].nrow, D,
                  kind == PK_MI355_FEATS_RAW ? "raw rows in front of the deltas" : "normalised rows at the model's dimension");
    if (feats[u].nrow != D) return Fail(PK_MI355_E_INVALID, "features of utterance %d have %d rows, the model expects %d", u, feats[u].nrow, D);
    if (feats[u].ncol > 0 && !feats[u].data) return Fail(PK_MI355_E_INVALID, "features of utterance %d: null data", u);
    frames[u] = feats[u].ncol;                          // (a negative one is named by CheckFeatureCounts)
  }
  if (int rc = CheckFeatureCounts(b, frames.data(), num_utts)) return rc;
  if (int rc = UseDevice(b->core.device)) return rc;
  // RAW: where FbankKernel would have written them; NORMALIZED: the staging FeatureLayoutKernel reads
  HIP_TRY(EnsureBuffers(b, kind == PK_MI355_FEATS_RAW ? BuffersFor(b, pkplan::kRaw, b->norm.mode) : pkplan::kFeatRows));
  float *dst = b->d_raw;
  if (kind == PK_MI355_FEATS_NORMALIZED) dst = b->d_feats;
  // The layout first: its upload travels while the host stages the features below (a copy out of pageable memory
  // holds the host until it is done), and the first kernel of the score call is then queued straight behind them.
  if (int rc = SetLayoutFrames(b, frames.data(), nullptr, num_utts)) return rc;
  b->source = pkplan::kNoSource;             // (until the features are there too)
  int64_t row = 0;
  for (int u = 0; u < num_utts; ++u) {
    if (frames[u] > 0)
      HIP_TRY(hipMemcpyAsync(dst + row * D, feats[u].data, sizeof(float) * (size_t)frames[u] * D, hipMemcpyHostToDevice, b->core.stream));
    row += frames[u];
  }
  if (kind == PK_MI355_FEATS_NORMALIZED) b->feats = b->d_feats;
  b->source = kind == PK_MI355_FEATS_RAW ? pkplan::kRaw : pkplan::kNormalized;
  return 0;
}

int pk_mi355_features_set_device(pk_mi355_batch_t *b, const float *d_feats, const int *num_frames, int num_utts, int kind) {
  if (!b || (num_utts > 0 && (!d_feats || !num_frames))) return Fail(PK_MI355_E_INVALID, "null argument");
  if (int rc = CheckFeatureKind(b, kind)) return rc;
  if (int rc = CheckFeatureCounts(b, num_frames, num_utts)) return rc;
  if (int rc = UseDevice(b->core.device)) return rc;
  if (kind == PK_MI355_FEATS_RAW) {                     // CMVN reads around every utterance: into d_raw with its lead and slack
    const int D = b->base_dim;                          // (any other dimension than 40: as a host call's rows, fetch_fbank's source)
    HIP_TRY(EnsureBuffers(b, BuffersFor(b, pkplan::kRaw, b->norm.mode)));
    int64_t total = 0;
    for (int u = 0; u < num_utts; ++u) total += num_frames[u];
    if (total > 0)
      HIP_TRY(hipMemcpyAsync(b->d_raw, d_feats, sizeof(float) * (size_t)total * D, hipMemcpyDeviceToDevice, b->core.stream));
  }
  if (int rc = SetLayoutFrames(b, num_frames, nullptr, num_utts)) return rc;
  if (kind == PK_MI355_FEATS_NORMALIZED) b->feats = d_feats;   // read where they lie
  b->source = kind == PK_MI355_FEATS_RAW ? pkplan::kRaw : pkplan::kNormalized;
  return 0;
}

int pk_mi355_norm_set(pk_mi355_batch_t *b, const pk_mi355_norm_spec_t *spec) {
  if (!b || !spec) return Fail(PK_MI355_E_INVALID, "null argument");
  if (int rc = pknorm::CheckSpec(spec)) return rc;      // (names the field)
  if (int rc = UseDevice(b->core.device)) return rc;
  HIP_TRY(EnsureBuffers(b, BuffersFor(b, pkplan::kRaw, spec->mode)));      // (audio needs the same rows)
  if (spec->mode != PK_MI355_NORM_SLIDING) {            // what NormKernel writes and reads, made at the first spec that needs it
    const size_t D = (size_t)b->base_dim;
    if (!b->d_norm_stats) HIP_TRY(hipMalloc(&b->d_norm_stats, sizeof(double) * 2 * (D + 1) * (size_t)b->max_utts));
    if (!b->d_spk_table) HIP_TRY(hipMalloc(&b->d_spk_table, sizeof(float) * 2 * D * (size_t)b->max_utts));
  }
  b->norm = *spec;
  b->spk_utts = -1;                                     // records finalised under another spec are not this spec's
  return 0;
}

int pk_mi355_norm_set_online_cmvn(pk_mi355_batch_t *b, const pk_mi355_online_cmvn_spec_t *spec, const double *global_stats) {
  if (!b || !spec) return Fail(PK_MI355_E_INVALID, "null argument");
  const size_t D = (size_t)b->base_dim;
  if (int rc = pknorm::CheckOnlineSpec(spec, global_stats, (int)D)) return rc;      // (names the field)
  if (int rc = UseDevice(b->core.device)) return rc;
  HIP_TRY(EnsureBuffers(b, BuffersFor(b, pkplan::kRaw, pknorm::kNormOnlineCmvn)));
  const size_t rec = 2 * (D + 1);
  if (!b->d_online_glob) HIP_TRY(hipMalloc(&b->d_online_glob, sizeof(double) * rec));
  if (!b->d_online_spk) HIP_TRY(hipMalloc(&b->d_online_spk, sizeof(double) * rec * (size_t)b->max_utts));
  if (spec->global_frames > 0) {                        // (pageable memory: the copy has read the record when the call returns)
    HIP_TRY(hipMemcpyAsync(b->d_online_glob, global_stats, sizeof(double) * rec, hipMemcpyHostToDevice, b->core.stream));
    HIP_TRY(hipStreamSynchronize(b->core.stream));
  }
  b->online_cmvn = *spec;
  b->norm = pk_mi355_norm_spec_t{pknorm::kNormOnlineCmvn, 1, spec->norm_vars};
  b->spk_utts = -1;                                     // records handed over under another spec are not this spec's
  return 0;
}

int pk_mi355_norm_set_speaker_stats(pk_mi355_batch_t *b, const double *stats, int num_utts) {
  if (!b || (num_utts > 0 && !stats)) return Fail(PK_MI355_E_INVALID, "null argument");
  if (b->norm.mode != PK_MI355_NORM_SPEAKER && b->norm.mode != pknorm::kNormOnlineCmvn)
    return Fail(PK_MI355_E_STATE, "speaker statistics need mode speaker (pk_mi355_norm_set) or online CMVN (pk_mi355_norm_set_online_cmvn)");
  if (num_utts < 0 || num_utts > b->max_utts) return Fail(PK_MI355_E_INVALID, "too many utterances (%d > %d)", num_utts, b->max_utts);
  const int D = b->base_dim;
  if (b->norm.mode == pknorm::kNormOnlineCmvn) {        // the records as they are: the kernel smooths with them
    if (int rc = pknorm::CheckOnlineSpeakerCounts(stats, num_utts, D)) return rc;
    if (int rc = UseDevice(b->core.device)) return rc;
    if (num_utts > 0) {
      HIP_TRY(hipMemcpyAsync(b->d_online_spk, stats, sizeof(double) * 2 * ((size_t)D + 1) * (size_t)num_utts, hipMemcpyHostToDevice, b->core.stream));
      HIP_TRY(hipStreamSynchronize(b->core.stream));
    }
    b->spk_utts = num_utts;
    return 0;
  }
  std::vector<float> table((size_t)std::max(num_utts, 1) * 2 * D);
  if (int rc = pknorm::FinalizeSpeakerStats(stats, num_utts, D, b->norm.norm_means != 0, b->norm.norm_vars != 0, table.data())) return rc;
  if (int rc = UseDevice(b->core.device)) return rc;
  if (num_utts > 0) {                                   // (pageable memory: the copy has read the table when the call returns)
    HIP_TRY(hipMemcpyAsync(b->d_spk_table, table.data(), sizeof(float) * 2 * D * (size_t)num_utts, hipMemcpyHostToDevice, b->core.stream));
    HIP_TRY(hipStreamSynchronize(b->core.stream));
  }
  b->spk_utts = num_utts;
  return 0;
}

int pk_mi355_norm_fetch_stats(pk_mi355_batch_t *b, int utt, double *out) {
  if (!b || !out || utt < 0 || utt >= b->num_utts) return Fail(PK_MI355_E_INVALID, "bad utterance index");
  if (!b->scored || !b->norm_stats_valid) return Fail(PK_MI355_E_STATE, "the last score call computed no statistics (mode utterance on raw rows or audio does)");
  const size_t rec = 2 * ((size_t)b->base_dim + 1);
  HIP_TRY(hipMemcpyAsync(out, b->d_norm_stats + utt * rec, sizeof(double) * rec, hipMemcpyDeviceToHost, b->core.stream));
  HIP_TRY(hipStreamSynchronize(b->core.stream));
  return 0;
}

int pk_mi355_batch_score(pk_mi355_batch_t *b, float prob_scale, int sync) {
  if (!b) return Fail(PK_MI355_E_INVALID, "null batch");
  if (b->source == pkplan::kNoSource) return Fail(PK_MI355_E_STATE, "no waves or features set");
  ScorerCore &c = b->core;
  int rc = UseDevice(c.device);
  if (rc) return rc;
  pk_mi355_am *am = c.am;
  Timer *tm = b->timer.enabled ? &b->timer : nullptr;
  if (tm) tm->Reset();
  // the range verdict belongs to ONE score call: an empty batch, or a call that fails half-way, must not report
  // (or deliver under) the verdict of the call before it
  b->range_pending = false;
  b->range_status = 0;
  b->range_msg[0] = 0;
  b->scored = false;
  // The normalisation of this call (raw rows or audio; normalised features pass it by).  Speaker records belong to one
  // score call: this one consumes them, whatever becomes of it.
  const int spk_utts = b->spk_utts;
  b->spk_utts = -1;
  b->norm_stats_valid = false;
  const int umat_utts = b->umat_utts;            // (the per-utterance transforms likewise)
  b->umat_utts = -1;
  const int D = am->feat_dim;
  const int Db = b->base_dim;                    // the dimension in front of the deltas (D without them)
  const int mode = b->source == pkplan::kNormalized ? PK_MI355_NORM_NONE : b->norm.mode;
  if (b->source != pkplan::kNormalized) {
    if (mode == PK_MI355_NORM_SLIDING && !b->have_stats)
      return Fail(PK_MI355_E_STATE, "raw features in mode sliding need the CMVN statistics: this batch was made without them");
    if (mode == PK_MI355_NORM_SPEAKER && spk_utts < 0)
      return Fail(PK_MI355_E_STATE, "mode speaker: no speaker statistics set for this score call (pk_mi355_norm_set_speaker_stats)");
    if (mode == PK_MI355_NORM_SPEAKER && spk_utts != b->num_utts)
      return Fail(PK_MI355_E_STATE, "mode speaker: statistics for %d utterances, the call has %d", spk_utts, b->num_utts);
    if (mode == pknorm::kNormOnlineCmvn && spk_utts >= 0 && spk_utts != b->num_utts)
      return Fail(PK_MI355_E_STATE, "online CMVN: speaker statistics for %d utterances, the call has %d", spk_utts, b->num_utts);
    if (umat_utts >= 0 && umat_utts != b->num_utts)
      return Fail(PK_MI355_E_STATE, "per-utterance transforms for %d utterances, the call has %d", umat_utts, b->num_utts);
  }
  if (b->num_utts == 0 || b->total_frames == 0) {
    if (mode == PK_MI355_NORM_UTTERANCE && b->num_utts > 0) {      // records of no frames: zeros
      HIP_TRY(hipMemsetAsync(b->d_norm_stats, 0, sizeof(double) * 2 * (Db + 1) * (size_t)b->num_utts, c.stream));
      b->norm_stats_valid = true;
    }
    b->scored = true;
    return 0;
  }
  const UttLayout &lay = b->lay;
  // The plan (pk_plan.h; DESIGN.md, "The two plans"): the front-end, then raw rows (fbank's, or the caller's) or
  // normalised features -> Yt.  What it reads and writes was made by create and the set calls (EnsureBuffers).
  const pkplan::BatchPlan plan = pkplan::PlanBatch(ShapeOf(b), b->source, b->norm.mode, spk_utts >= 0, umat_utts >= 0);
  HIP_TRY(EnsureBuffers(b, plan.buffers));        // (made by create and the set calls already: nothing happens here)
  auto own = [b](pkplan::Rows r) {
    return r == pkplan::kRawRows ? b->d_raw : r == pkplan::kFeatRows ? b->d_feats : r == pkplan::kDeltaRows ? b->d_delta
         : r == pkplan::kXformRows ? b->d_xform : b->d_uxform;
  };
  // what the writers of Yt replicate in front of and behind an utterance: the first layer's context and the virtual
  // frames of the time-splice layers
  const int yl = am->left + am->time_left, yr = am->right + am->time_right;
  auto run = [&](int first, int last) {
    for (int k = first; k < last; ++k) {
      const pkplan::Step &st = plan.step[k];
      const float *in = st.in == pkplan::kCallerRows ? b->feats : own(st.in);
      float *out = own(st.out);                  // (the stages that write Yt do not look at it)
      switch (st.stage) {
        case pkplan::kFbank: LaunchFbank(b->wave_f32, b->wave_i16, lay, b->num_utts, b->max_T, c.d_tables, out, c.stream); break;
        case pkplan::kFbankAny: LaunchFbankAny(b->wave_f32, b->wave_i16, lay, b->num_utts, b->max_T, c.d_tables, b->d_any, st.dim, out, c.stream); break;
        case pkplan::kCmvn: LaunchCmvn(in, lay, b->num_utts, c.d_global, c.d_cmvn_tab, yl, yr, c.d_yt, c.ldy, c.stream); break;
        case pkplan::kCmvnChain: LaunchCmvnChain(in, lay, b->num_utts, st.dim, c.d_global, c.d_cmvn_tab, out, c.stream); break;
        case pkplan::kNorm:
          LaunchNorm(in, lay, b->num_utts, st.dim, mode, b->norm.norm_means != 0, b->norm.norm_vars != 0, b->d_spk_table, b->d_norm_stats, out, c.stream);
          break;
        case pkplan::kOnlineCmvn:
          LaunchOnlineCmvn(in, lay, b->num_utts, st.dim, b->online_cmvn, b->d_online_glob, plan.speaker ? b->d_online_spk : nullptr, out, c.stream);
          break;
        case pkplan::kDelta: LaunchDelta(in, lay, b->num_utts, b->max_T, st.dim, b->deltas, b->d_delta_scales, out, c.stream); break;
        case pkplan::kTransform: LaunchTransform(in, lay, b->num_utts, b->max_T, b->xform, out, c.stream); break;
        case pkplan::kUttTransform:
          LaunchTransform(in, lay, b->num_utts, b->max_T,
                          TransformStage{D, 0, 0, D, b->umat_affine, b->d_umats, (int64_t)(D + (b->umat_affine ? 1 : 0)) * pkxf::Ldo(D)}, out, c.stream);
          break;
        case pkplan::kFeatureLayout: LaunchFeatureLayout(in, lay, b->num_utts, b->max_T, st.dim, yl, yr, c.d_yt, c.ldy, c.stream); break;
      }
    }
  };
  if (plan.front) {
    Scoped t(tm, PK_MI355_K_FBANK, c.stream);
    run(0, plan.front);
  }
  {
    Scoped t(tm, PK_MI355_K_CMVN, c.stream);
    run(plan.front, plan.n);
  }
  b->norm_stats_valid = plan.writes_stats;
  // Rows of the layer stack: compact (row out_base[u] + t is frame t of utterance u; the first layer finds its
  // features shift4[row / 4] columns -- f16 modes: rows of the split copy -- further on; no shift4 when all are zero).
  const bool f16 = IsF16(am->precision);
  if (f16) {
    if ((rc = BeginRange(c.exec, c.stream))) return rc;
    Scoped t(tm, PK_MI355_K_OTHER, c.stream);
    // only the rows the layer stack reads (the last chunk's padded rows and their right context): columns further
    // out hold zeros or an earlier call's split, and their maxima are not this call's
    // (compact rows: the last tile's padding rows sit at most one tile + the context behind the last column)
    const int split_rows = (int)std::min<int64_t>(c.ldy, RoundUp(b->total_cols, kTileF16) + 2 * kTileF16);
    LaunchSplitF16(c.d_yt, 1, c.ldy, split_rows, D, D, b->d_y2, 2 * D, ExpX(am, 0), RangeOf(c.exec, 0), c.stream);
  }
  const bool two = b->lanes == 2 && b->total_rows > c.chunk;
  if (f16 && b->lanes == 2 && !two) ClearHostRange(b->exec2);     // lane 2 takes no part in this call: no stale maxima
  if (two) {                                   // lane 2 starts when the features are ready
    HIP_TRY(hipEventRecord(b->ev_front, c.stream));
    HIP_TRY(hipStreamWaitEvent(b->stream2, b->ev_front, 0));
    if (f16 && (rc = BeginRange(b->exec2, b->stream2))) return rc;
  }
  const Operand op{c.d_yt, b->d_y2, c.ldy, ZeroSource(c), b->d_shift4};
  const Lane lanes[2] = {{c.stream, &c.exec}, {b->stream2, &b->exec2}};
  if ((rc = WalkChunks(am, op, b->total_rows, c.chunk, lanes, two ? 2 : 1, true, prob_scale, c.d_ll, tm))) return rc;
  if (two) {                                   // everything is ordered on the batch's stream again
    if (f16 && (rc = CollectRange(b->exec2, b->stream2))) return rc;
    HIP_TRY(hipEventRecord(b->ev_lane2, b->stream2));
    HIP_TRY(hipStreamWaitEvent(c.stream, b->ev_lane2, 0));
  }
  if (f16) {
    if ((rc = CollectRange(c.exec, c.stream))) return rc;
    b->range_pending = true;
    b->range_status = 0;
  }
  b->scored = true;
  if (sync) return pk_mi355_batch_synchronize(b);
  return 0;
}

int pk_mi355_batch_synchronize(pk_mi355_batch_t *b) {
  if (!b) return Fail(PK_MI355_E_INVALID, "null batch");
  HIP_TRY(hipStreamSynchronize(b->core.stream));
  return BatchRangeStatus(b);
}

int pk_mi355_batch_calibrate(pk_mi355_batch_t *b) {
  if (!b) return Fail(PK_MI355_E_INVALID, "null batch");
  pk_mi355_am *am = b->core.am;
  if (!IsF16(am->precision)) return 0;
  if (b->source == pkplan::kNoSource) return Fail(PK_MI355_E_STATE, "no waves or features set");
  if (b->total_frames == 0) return Fail(PK_MI355_E_INVALID, "calibration needs at least one frame");
  if (int rc = UseDevice(b->core.device)) return rc;
  std::lock_guard<std::mutex> lock(am->mu);
  return BatchCalibrateLocked(b);
}

}  // extern "C"

int pkhost::BatchCalibrateLocked(pk_mi355_batch *b) {
  pk_mi355_am *am = b->core.am;
  if (am->exps_stale) if (int rc = RefreshExps(am)) return rc;
  const ExecBufs &e = b->core.exec;
  const int spk_utts = b->spk_utts;              // calibration passes do not consume the speaker records: the score behind them does
  const int umat_utts = b->umat_utts;            // (nor the per-utterance transforms)
  return CalibrateLoop(am, e, [&]() -> int {
    b->spk_utts = spk_utts;
    b->umat_utts = umat_utts;
    const int rc = pk_mi355_batch_score(b, 1.0f, 0);
    b->spk_utts = spk_utts;
    b->umat_utts = umat_utts;
    b->scored = false;                           // calibration passes are not results
    b->range_pending = false;
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(b->core.stream));
    if (b->lanes == 2)
      for (int i = 0; i < e.range_words; ++i) e.h_range[i] = std::max(e.h_range[i], b->exec2.h_range[i]);
    return 0;
  });
}

extern "C" {

int pk_mi355_batch_num_utts(const pk_mi355_batch_t *b) { return b ? b->num_utts : 0; }
int pk_mi355_batch_num_frames(const pk_mi355_batch_t *b, int utt) {
  return (b && utt >= 0 && utt < b->num_utts) ? b->h_T[utt] : 0;
}
int64_t pk_mi355_batch_total_frames(const pk_mi355_batch_t *b) { return b ? b->total_frames : 0; }

const float *pk_mi355_batch_loglik_device(const pk_mi355_batch_t *b, int utt) {
  if (!b || utt < 0 || utt >= b->num_utts) return nullptr;
  return b->core.d_ll + b->h_out_base[utt] * b->core.am->num_pdfs;
}

int pk_mi355_batch_fetch(pk_mi355_batch_t *b, int utt, pk_decodable_t *out) {
  if (!b || !out || utt < 0 || utt >= b->num_utts) return Fail(PK_MI355_E_INVALID, "bad utterance index");
  if (!b->scored) return Fail(PK_MI355_E_STATE, "batch not scored");
  if (int rc = UseDevice(b->core.device)) return rc;
  ClearDecodable(out, b->core.am);
  if (b->h_T[utt] == 0) return 0;
  return FetchRows(pk_mi355_batch_loglik_device(b, utt), b->h_T[utt], b->core.am->num_pdfs, b->core.stream, "fetch", out,
                   [&] { return BatchRangeStatus(b); });      // f16 modes: out-of-range results are withheld
}

int pk_mi355_batch_fetch_all(pk_mi355_batch_t *b, pk_decodable_t *out, int num_out, int sync) {
  if (!b || !out || num_out != b->num_utts) return Fail(PK_MI355_E_INVALID, "fetch_all: expected %d decodables", b ? b->num_utts : 0);
  if (!b->scored) return Fail(PK_MI355_E_STATE, "batch not scored");
  int rc = UseDevice(b->core.device);
  if (rc) return rc;
  const int N = b->core.am->num_pdfs;
  if (!b->h_ll) {
    const size_t bytes = sizeof(float) * (size_t)b->core.max_cols * N;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&b->h_ll), bytes, hipHostMallocDefault));
    b->arena = RegisterArena(b->h_ll);
  }
  // One transfer of the used part of d_ll (the 10 rows between two utterances travel too:
  // 1 % at T = 998, and one large copy runs at the link rate).
  // The transfer is queued on ONE result stream per device, ordered after this batch's scoring
  // and before anything later on the batch's stream.  Results of several batches in flight
  // then leave the device first come, first served at the full link rate -- on their own
  // streams the copies would share the link, finish together, and the batches would fall into
  // step (all scoring, then all copying) instead of overlapping.
  if (b->total_rows > 0) {
    hipStream_t rs = ResultStream(b->core.device);
    if (!rs) return PK_MI355_E_DEVICE;
    if (!b->ev_scored) {
      HIP_TRY(hipEventCreateWithFlags(&b->ev_scored, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&b->ev_fetched, hipEventDisableTiming));
    }
    HIP_TRY(hipEventRecord(b->ev_scored, b->core.stream));
    HIP_TRY(hipStreamWaitEvent(rs, b->ev_scored, 0));
    HIP_TRY(hipMemcpyAsync(b->h_ll, b->core.d_ll, sizeof(float) * (size_t)b->total_rows * N, hipMemcpyDeviceToHost, rs));
    HIP_TRY(hipEventRecord(b->ev_fetched, rs));
    HIP_TRY(hipStreamWaitEvent(b->core.stream, b->ev_fetched, 0));
  }
  pk_mi355_am_t *gen = NewViewGen(b->arena, b->core.am, num_out);   // the views of an earlier fetch_all are void by contract
  for (int u = 0; u < num_out; ++u) {
    const int T = b->h_T[u];
    out[u].am = gen;
    out[u].log_prob.ncol = T;
    out[u].log_prob.nrow = T > 0 ? N : 0;
    out[u].log_prob.data = T > 0 ? b->h_ll + (size_t)b->h_out_base[u] * N : nullptr;
  }
  if (sync && (rc = pk_mi355_batch_synchronize(b))) {   // f16 modes: the range verdict of the score call comes with it
    for (int u = 0; u < num_out; ++u) {                 // nothing is delivered: hand back empty decodables, drop the views
      ReleaseArenaView(gen);
      ClearDecodable(&out[u], b->core.am);
    }
    return rc;
  }
  return 0;
}

int pk_mi355_batch_fetch_fbank(pk_mi355_batch_t *b, int utt, float *out) {
  if (!b || !out || utt < 0 || utt >= b->num_utts) return Fail(PK_MI355_E_INVALID, "bad utterance index");
  if (!b->scored) return Fail(PK_MI355_E_STATE, "batch not scored");
  if (b->source == pkplan::kNormalized) return Fail(PK_MI355_E_STATE, "the batch was fed normalised features: there is no fbank");
  const int T = b->h_T[utt];
  if (T == 0) return 0;
  const int D = b->base_dim;                   // (the front-end's dimension)
  HIP_TRY(hipMemcpyAsync(out, b->d_raw + b->h_raw_base[utt] * D, sizeof(float) * (size_t)T * D, hipMemcpyDeviceToHost, b->core.stream));
  HIP_TRY(hipStreamSynchronize(b->core.stream));
  return 0;
}

int pk_mi355_batch_fetch_cmvn(pk_mi355_batch_t *b, int utt, float *out) {
  if (!b || !out || utt < 0 || utt >= b->num_utts) return Fail(PK_MI355_E_INVALID, "bad utterance index");
  if (!b->scored) return Fail(PK_MI355_E_STATE, "batch not scored");
  const int T = b->h_T[utt];
  if (T == 0) return 0;
  const int D = b->core.am->feat_dim;
  std::vector<float> tmp((size_t)D * T);
  HIP_TRY(hipMemcpy2DAsync(tmp.data(), sizeof(float) * T, b->core.d_yt + b->h_pad_base[utt] + b->core.am->left + b->core.am->time_left,
                           sizeof(float) * b->core.ldy, sizeof(float) * T, D, hipMemcpyDeviceToHost, b->core.stream));
  HIP_TRY(hipStreamSynchronize(b->core.stream));
  for (int t = 0; t < T; ++t)
    for (int d = 0; d < D; ++d) out[(size_t)t * D + d] = tmp[(size_t)d * T + t];
  return 0;
}

int pk_mi355_batch_gather_loglik(pk_mi355_batch_t *b, int utt, const int32_t *d_frames,
                                 const int32_t *d_trans_ids, int n, float *d_out) {
  if (!b || utt < 0 || utt >= b->num_utts || !d_frames || !d_trans_ids || !d_out)
    return Fail(PK_MI355_E_INVALID, "bad gather arguments");
  if (!b->scored) return Fail(PK_MI355_E_STATE, "batch not scored");
  if (int rc = UseDevice(b->core.device)) return rc;
  LaunchGather(pk_mi355_batch_loglik_device(b, utt), b->core.am->num_pdfs, b->core.am->d_tid2pdf,
               (int)b->core.am->tid2pdf.size(), d_frames, d_trans_ids, n, d_out, b->core.stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return Fail(PK_MI355_E_DEVICE, "gather: %s", hipGetErrorString(e));
  return 0;
}

void *pk_mi355_batch_stream(pk_mi355_batch_t *b) { return b ? (void *)b->core.stream : nullptr; }

int pk_mi355_batch_enable_timing(pk_mi355_batch_t *b, int enable) {
  if (!b) return Fail(PK_MI355_E_INVALID, "null batch");
  b->timer.enabled = enable != 0;
  if (!enable) b->timer.Reset();
  return 0;
}

int pk_mi355_batch_get_timing(pk_mi355_batch_t *b, float ms[PK_MI355_K_COUNT], int launches[PK_MI355_K_COUNT]) {
  if (!b) return Fail(PK_MI355_E_INVALID, "null batch");
  for (int k = 0; k < PK_MI355_K_COUNT; ++k) { ms[k] = 0; launches[k] = 0; }
  HIP_TRY(hipStreamSynchronize(b->core.stream));
  for (auto &r : b->timer.recs) {
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, r.a, r.b));
    ms[r.kind] += t;
    launches[r.kind] += 1;
  }
  return 0;
}

// The three acoustic stages of pk_process (pocketkaldi.cc:186-218) fused on the device:
// wave -> fbank -> CMVN -> nnet -> decodable.  With verbose != 0 the reference's stage
// lines go to stderr ("Fbank: ..ms", "CMVN: ..ms", "NNET: ..ms"), timed with HIP events.
int pk_mi355_process_acoustic(pk_mi355_am_t *am, const pk_vector_t *cmvn_global_stats,
                              const pk_vector_t *raw_wave, float prob_scale, pk_decodable_t *out,
                              int verbose) {
  if (!am || !cmvn_global_stats || !raw_wave || !out) return Fail(PK_MI355_E_INVALID, "null argument");
  if (cmvn_global_stats->dim != kNumBins + 1) return Fail(PK_MI355_E_INVALID, "cmvn_global_stats must have 41 entries");
  ClearDecodable(out, am);
  if (raw_wave->dim == 0) return 0;                           // pocketkaldi.cc:180-184
  std::lock_guard<std::mutex> lock(am->mu);
  const float *stats = cmvn_global_stats->data;
  pk_mi355_batch *b = EnsureOwned(&am->proc, std::max<int64_t>(raw_wave->dim, 16000), memcmp(am->proc_stats, stats, sizeof(am->proc_stats)) == 0,
                                  [&](int64_t cap) { return CheckedBatch(am, CreateRequest{stats, 0, true, 1, cap, true, false, nullptr, nullptr}); });
  if (!b) return PK_MI355_E_DEVICE;
  memcpy(am->proc_stats, stats, sizeof(am->proc_stats));
  int rc = pk_mi355_batch_set_waves(b, raw_wave, 1);
  if (rc) return rc;
  pk_mi355_batch_enable_timing(b, verbose);
  if ((rc = pk_mi355_batch_score(b, prob_scale, 1))) return rc;
  if (verbose) {
    float ms[PK_MI355_K_COUNT];
    int launches[PK_MI355_K_COUNT];
    if ((rc = pk_mi355_batch_get_timing(b, ms, launches))) return rc;
    fprintf(stderr, "Fbank: %lfms\n", (double)ms[PK_MI355_K_FBANK]);
    fprintf(stderr, "CMVN: %lfms\n", (double)ms[PK_MI355_K_CMVN]);
    fprintf(stderr, "NNET: %lfms\n", (double)(ms[PK_MI355_K_GEMM] + ms[PK_MI355_K_TAIL] + ms[PK_MI355_K_OTHER]));
  }
  return pk_mi355_batch_fetch(b, 0, out);
}

}  // extern "C"
