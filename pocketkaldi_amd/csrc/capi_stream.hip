// capi_stream.hip -- the online scorer (pk_mi355_stream_*): live PCM, or live features, pushed in
// chunks per slot, and every step scores, for every slot, the frames that became final since the last step.  Host C++
// over the HIP runtime; the kernels that carry a slot's state from one step to the next are in stream.hip, and why the
// result is exact is told there (DESIGN.md section 10 walks through one step).
#include <hip/hip_runtime.h>

#include <algorithm>
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

namespace {
enum SlotState { kFree = 0, kOpen = 1, kClosed = 2 };

struct Slot {
  int state = kFree;
  int n = 0;               // CMVN frames computed
  int nd = 0;              // a deltas object: delta frames final, n - M at most while open
  int ring_par = 0;        //   the delta ring buffer that holds the base frames below n
  int nx = 0;              // a transform object: transform frames final, nin - Rt at most while open
  int xf_par = 0;          //   the transform ring buffer that holds the input frames below nin (= nd with deltas, else n)
  int mat = kSlotMatNone;  //   this opening's own matrix (pk_mi355_stream_transform_set_slot): none, linear or affine
  int a = 0;               // frames scored (the next row to score)
  int tail_len = 0;
  int tail_par = 0;
  std::vector<float> pending;   // pushed since the last step
  // the last step's rows of this slot
  int last_first = 0, last_count = 0;
  int64_t last_out = 0;
  bool last_flushed = false;     // the last step was the slot's final one
  // A slot opened at another rate than 16 kHz (tab != null): its pushes are samples at that rate and `pending` stays
  // empty.  `native` holds the input samples from index nat_x0 on -- the carry (what the next output's window still
  // reads, at most Q + max_taps samples) and what was pushed since the last step.  n_in inputs received, n_prod
  // outputs handed to the front-end; `reserve` = floor(n_in P / Q) - n_prod is what the slot counts against the step
  // capacity: the outputs a close would make final.
  int rate = kSampleRate;
  const DeviceResampleTable *tab = nullptr;
  std::vector<float> native;
  int64_t nat_x0 = 0, n_in = 0, n_prod = 0, reserve = 0;
  // A feature slot (kind PK_MI355_FEATS_*; -1: audio): its pushes are frames, `pending` holds them frame-major, n counts
  // the frames handed to a step.  hist_par: the NORMALIZED history buffer that holds the frames below n.
  int kind = -1;
  int hist_par = 0;
  bool spk_set = false;    // pk_mi355_stream_norm_set_speaker_stats has handed over this opening's record
};

// the most input samples a native-rate slot carries from one step to the next (Q + max_taps <= 8190 + 74)
constexpr int64_t kNativeCarryCap = 8448;

}  // namespace

struct pk_mi355_stream {
  ScorerCore core;                    // model, stream, front-end tables, Yt, log-likelihood rows, layer buffers
  int max_streams = 0;
  int64_t max_step_samples = 0, pending_total = 0;   // (a features-only object: frames, not samples)
  bool features_only = false;         // pk_mi355_features_stream_create: no front-end, no PCM buffers
  bool have_stats = false;            // RAW feature slots are possible
  int frame_cost = kFrameShift;       // what a pushed frame counts against max_step_samples (features-only: 1)
  int64_t upload_cap = 0;             // floats of h_upload / d_upload
  std::vector<Slot> slots;
  int hist_len = 1;                   // max(L + R, 1)
  int64_t wave_cap = 0;
  // per-slot state in HBM
  float *d_tails = nullptr;           // [slots][2][kTailCap]
  float *d_sums = nullptr;            // [slots][feat_dim] (40 wherever there is a front-end)
  float *d_raw_hist = nullptr;        // [slots][600][feat_dim]
  float *d_hist = nullptr;            // [slots][hist_len][40] (StreamCmvnKernel's; not made at another dimension)
  float *d_feat_hist = nullptr;       // [slots][2][hist_len][feat_dim]: slots laid out by StreamFeatureLayoutKernel (made at the first such open)
  // per-step staging
  float *h_upload = nullptr, *d_upload = nullptr;    // pushed samples, page-locked -> HBM
  float *d_wave = nullptr;            // segments
  float *d_rows = nullptr;            // raw -> CMVN'd rows of the step's new frames
  char *h_meta = nullptr, *d_meta = nullptr;          // records, UttLayout arrays, column shifts
  size_t meta_bytes = 0;
  hipEvent_t ev_staged = nullptr;     // the last step's uploads have left the page-locked buffers
  // native-rate slots (made at the first pk_mi355_stream_open_rate other than 16000): the tables of the rates met, and
  // the step's native samples, page-locked -> HBM, which ResampleKernel converts into d_upload
  Resampler resampler;
  float *h_native = nullptr, *d_native = nullptr;
  int64_t native_cap = 0;
  bool staged = false;
  // made by pk_mi355_frontend_stream_create: the spec's tables; a step then runs FbankAnyKernel
  // instead of FbankKernel.  At a dimension other than 40 the audio slots' fresh rows lie in the upload staging from
  // float rows_area on (behind the max_step_samples samples), where the chain and the layout kernel find them.
  FrontendAnyTables *d_any = nullptr;
  int64_t rows_area = 0;
  // The normalisation spec (pk_mi355_stream_norm_set*).  Anything but SLIDING: the audio and RAW
  // slots' fresh rows go through StreamNormKernel (NONE: through nothing) and StreamFeatureLayoutKernel at every
  // dimension; norm.mode is pknorm::kNormOnlineCmvn under online CMVN.  The state below is made by the set calls.
  pk_mi355_norm_spec_t norm{PK_MI355_NORM_SLIDING, 1, 0};
  pk_mi355_online_cmvn_spec_t online_cmvn{600, 600, 200, 0};
  double *d_norm_glob = nullptr, *d_norm_spk = nullptr;      // [2][feat_dim + 1], [slots][2][feat_dim + 1]
  double *d_norm_win = nullptr, *d_norm_total = nullptr;     // [slots][2][feat_dim] each
  float *d_norm_table = nullptr, *d_norm_ring = nullptr;     // [slots][2][feat_dim], [slots][ring_window][feat_dim]
  int ring_window = 0;
  // Made by pk_mi355_deltas_stream_create: StreamDeltaKernel between the normaliser and the layout.
  // Everything in front of it -- the front-end, the statistics, every normaliser's state above, RAW slots -- is at base_dim
  // = feat_dim / (order + 1); on every other object base_dim = feat_dim.  An audio object has a row area at every
  // dimension.  The delta staging, (max_frames + max_streams M) rows of feat_dim floats, lies in d_upload from float
  // delta_area on, where the layout launch finds it through the step's second record array.
  int base_dim = 0;
  bool has_deltas = false;
  pk_mi355_deltas_spec_t deltas{0, 0};
  int reach = 0;                      // M = order * window
  float *d_delta_scales = nullptr;    // the spec's scale table (pkdelta::BuildScales)
  float *d_delta_ring = nullptr;      // [slots][2][2 M][base_dim]
  int64_t delta_area = 0, delta_rows = 0;
  // Made by pk_mi355_transform_stream_create: StreamTransformKernel behind the normaliser or the
  // deltas, with the spec's matrix (xf.mt, owned; null: the spec has none) and then with the slots' own (d_slot_mats,
  // [slots][feat_dim + 1][Ldo(feat_dim)], made at the first pk_mi355_stream_transform_set_slot).  in_dim: the width of
  // the rows the transform reads, (order + 1) base_dim; feat_dim on every other object.  Its staging, xf_rows =
  // max_frames + max_streams (M + Rt) rows of feat_dim floats, lies in d_upload from float xf_area on, behind the delta
  // staging; the per-slot stage's, as large, from uxf_area on (0: not made yet), behind that.  upload_floats: d_upload's size.
  bool has_xform = false;
  int in_dim = 0;
  TransformStage xf{};
  float *d_xf_ring = nullptr;         // [slots][2][max(Lt + Rt, 1)][in_dim]
  float *d_slot_mats = nullptr;
  int64_t xf_area = 0, xf_rows = 0, uxf_area = 0, upload_floats = 0;
  int extra_recs = 0;                 // StreamRec arrays behind the UttLayout arrays: deltas 1, a transform 2 more
};

namespace {
StreamNormState NormState(const pk_mi355_stream *s) {
  const pk_mi355_online_cmvn_spec_t &o = s->online_cmvn;
  return StreamNormState{s->norm.mode, s->norm.norm_vars, o.cmn_window, o.speaker_frames, o.global_frames, s->d_norm_glob, s->d_norm_spk,
                         s->d_norm_table, s->d_norm_win, s->d_norm_total, s->d_norm_ring};
}

int SlotIndex(const pk_mi355_stream *s, int slot) {
  if (!s) return Fail(PK_MI355_E_INVALID, "null stream");
  if (slot < 0 || slot >= s->max_streams) return Fail(PK_MI355_E_INVALID, "slot %d out of range [0, %d)", slot, s->max_streams);
  return 0;
}

// The per-slot CMVN state and the step's raw rows (audio and RAW slots), the upload staging and the step's plan.
void CreateStepBuffers(pk_mi355_stream *s, CreateCheck &chk) {
  const ScorerCore &c = s->core;
  const int max_streams = s->max_streams;
  // (a deltas or transform object: the later stages' records lie behind the UttLayout arrays, a StreamRec array each)
  s->meta_bytes = RoundUp(sizeof(StreamRec) * max_streams, 256) + RoundUp((sizeof(int64_t) * 2 + sizeof(int32_t)) * max_streams, 256) +
                  s->extra_recs * RoundUp(sizeof(StreamRec) * max_streams, 256) + sizeof(int32_t) * Shift4Cap(c.max_cols);
  chk(hipEventCreateWithFlags(&s->ev_staged, hipEventDisableTiming));
  const int Db = s->base_dim;
  if (s->has_deltas || s->has_xform)   // every slot is laid out by StreamFeatureLayoutKernel: the history, at create
    chk(hipMalloc(&s->d_feat_hist, sizeof(float) * max_streams * 2 * s->hist_len * c.am->feat_dim));
  if (s->have_stats && (Db != kNumBins || s->has_deltas || s->has_xform)) {   // StreamCmvnChainKernel's state; its rows stay in the upload staging
    chk(hipMalloc(&s->d_sums, sizeof(float) * max_streams * Db));
    chk(hipMalloc(&s->d_raw_hist, sizeof(float) * max_streams * kCmvnWindow * Db));
    if (s->rows_area && !s->d_feat_hist)   // audio slots are laid out by StreamFeatureLayoutKernel: their history, at create
      chk(hipMalloc(&s->d_feat_hist, sizeof(float) * max_streams * 2 * s->hist_len * c.am->feat_dim));
  } else if (s->have_stats) {
    chk(hipMalloc(&s->d_sums, sizeof(float) * max_streams * kNumBins));
    chk(hipMalloc(&s->d_raw_hist, sizeof(float) * max_streams * kCmvnWindow * kNumBins));
    chk(hipMalloc(&s->d_hist, sizeof(float) * max_streams * s->hist_len * kNumBins));
    chk(hipMalloc(&s->d_rows, sizeof(float) * c.max_frames * kNumBins));
  }
  chk(hipHostMalloc(reinterpret_cast<void **>(&s->h_upload), sizeof(float) * (s->rows_area ? s->rows_area : s->upload_cap), hipHostMallocDefault));
  s->upload_floats = s->has_xform ? s->xf_area + s->xf_rows * c.am->feat_dim : s->has_deltas ? s->delta_area + s->delta_rows * c.am->feat_dim : s->upload_cap;
  chk(hipMalloc(&s->d_upload, sizeof(float) * s->upload_floats));
  chk(hipHostMalloc(reinterpret_cast<void **>(&s->h_meta), s->meta_bytes, hipHostMallocDefault));
  chk(hipMalloc(&s->d_meta, s->meta_bytes));
}

int EnsureFeatureHistory(pk_mi355_stream *s) {
  if (s->d_feat_hist) return 0;
  if (int rc = UseDevice(s->core.device)) return rc;
  HIP_TRY(hipMalloc(&s->d_feat_hist, sizeof(float) * s->max_streams * 2 * s->hist_len * s->core.am->feat_dim));
  return 0;
}

// A slot that is being opened starts without a speaker record; under online CMVN its record on the device says "count 0".
int ResetSlotNorm(pk_mi355_stream *s, int slot) {
  s->slots[slot].spk_set = false;
  if (s->norm.mode != pknorm::kNormOnlineCmvn) return 0;
  if (int rc = UseDevice(s->core.device)) return rc;
  const size_t rec = 2 * ((size_t)s->base_dim + 1);
  HIP_TRY(hipMemsetAsync(s->d_norm_spk + slot * rec, 0, sizeof(double) * rec, s->core.stream));
  return 0;
}

// The norm entries change what a slot's life looks like: only while every slot is free.
int NoSlotInUse(const pk_mi355_stream *s) {
  for (size_t k = 0; k < s->slots.size(); ++k)
    if (s->slots[k].state != kFree)
      return Fail(PK_MI355_E_STATE, "slot %d is %s: the normalisation spec is set while no slot is open", (int)k,
                  s->slots[k].state == kOpen ? "open" : "closed and not yet flushed by a step");
  return 0;
}
}  // namespace

namespace pkhost {
const pk_mi355_am *StreamModel(const pk_mi355_stream *s) { return s->core.am; }
int StreamSlots(const pk_mi355_stream *s) { return s->max_streams; }
hipStream_t StreamHipStream(const pk_mi355_stream *s) { return s->core.stream; }
const float *StreamLoglikBase(const pk_mi355_stream *s) { return s->core.d_ll; }
bool StreamSlotFlushed(const pk_mi355_stream *s, int slot) { return slot >= 0 && slot < s->max_streams && s->slots[slot].last_flushed; }
}  // namespace pkhost

namespace {
// Every way to a stream object: the request and what its checks worked out.  Audio: live PCM through a front-end (the
// spec's tables, or without one the reference's 40 bins), the step capacity in samples; else features only, in frames.
// The statistics, like a front-end, are at the base dimension.
pk_mi355_stream *CreateStream(pk_mi355_am_t *am, const CreateRequest &sh, const CreateDims &dims) {
  const int D = am->feat_dim, max_streams = sh.units, Din = dims.in_dim, Db = dims.base_dim;
  const int Dw = std::max(D, Db);                       // the widest pushed frame: NORMALIZED at D, RAW at Db
  const int64_t step_cap = sh.capacity;
  if (UseDevice(am->device)) return nullptr;
  pk_mi355_stream *s = new pk_mi355_stream();
  s->max_streams = max_streams; s->max_step_samples = step_cap;
  s->features_only = !sh.audio; s->have_stats = sh.stats != nullptr;
  s->has_deltas = sh.deltas != nullptr;
  if (sh.deltas) { s->deltas = *sh.deltas; s->reach = pkdelta::Reach(*sh.deltas); }
  s->has_xform = sh.xform != nullptr;
  s->in_dim = Din; s->base_dim = Db;
  s->extra_recs = (sh.deltas ? 1 : 0) + (sh.xform ? 2 : 0);
  const int M = s->reach, Rt = sh.xform ? sh.xform->right_context : 0, Ct = sh.xform ? sh.xform->left_context + Rt : 0;
  // (a NORMALIZED frame of a deltas object can be wider than 160 floats: it counts as what it takes in the staging)
  s->frame_cost = sh.audio ? std::max(kFrameShift, Dw) : 1;
  s->slots.resize(max_streams);
  s->hist_len = std::max(am->left + am->right, 1);
  // Audio: a slot's segment holds at most 399 carried samples and its pushes.  A slot's rows are its new frames and the
  // (at most R) frames held back for look-ahead, padded to four.
  s->wave_cap = sh.audio ? step_cap + (int64_t)max_streams * kTailCap : 0;
  const int64_t max_frames = sh.audio ? s->wave_cap / kFrameShift + max_streams : step_cap;
  // Audio at D == 40: the fbank writes d_rows, where StreamCmvnKernel reads.  At another dimension the staging holds the
  // step's samples (a pushed frame is D <= 128 < 160 floats and counts as 160 samples), then max_frames rows of D floats.
  // With deltas the row area is there at every base dimension, its rows Db floats wide; a closing
  // slot emits up to M + R rows more than it was pushed, and the delta staging lies behind everything else.
  // A transform object likewise has a row area wherever it has a front-end; a closing slot emits up
  // to M + Rt + R rows more than it was pushed, and the transform's staging lies behind the delta staging.
  s->rows_area = sh.audio && (D != kNumBins || sh.deltas || sh.xform) ? RoundUp(step_cap, 64) : 0;
  s->upload_cap = !sh.audio ? step_cap * Dw : s->rows_area ? s->rows_area + max_frames * Db : step_cap;
  if (sh.deltas) { s->delta_area = RoundUp(s->upload_cap, 64); s->delta_rows = max_frames + (int64_t)max_streams * M; }
  if (sh.xform) {
    s->xf_area = sh.deltas ? RoundUp(s->delta_area + s->delta_rows * Din, 64) : RoundUp(s->upload_cap, 64);
    s->xf_rows = max_frames + (int64_t)max_streams * (M + Rt);
  }
  // the name a device failure is told under: the public entry such a request comes from
  CreateCheck chk{sh.xform ? "transform_stream_create" : sh.deltas ? "deltas_stream_create" : sh.frontend ? "frontend_stream_create"
                  : sh.audio ? "stream_create" : "features_stream_create"};
  CreateScorerCore(&s->core, am, sh.stats, Db, max_streams, max_frames, max_frames + (int64_t)max_streams * (am->right + M + Rt + 3), 262144, chk);
  if (dims.any()) UploadSpecTables(&s->core, dims.any(), &s->d_any, chk);
  CreateStepBuffers(s, chk);
  if (sh.deltas) {     // StreamDeltaKernel's table and the slots' rings
    s->d_delta_scales = UploadDeltaScales(*sh.deltas, chk);
    chk(hipMalloc(&s->d_delta_ring, sizeof(float) * max_streams * 2 * 2 * M * Db));      // (delta rows are Din = (order + 1) Db floats wide)
  }
  if (sh.xform) {      // StreamTransformKernel's global matrix and the slots' rings
    s->xf = UploadTransform(*sh.xform, chk);
    chk(hipMalloc(&s->d_xf_ring, sizeof(float) * max_streams * 2 * std::max(Ct, 1) * Din));
  }
  if (sh.audio) {
    chk(hipMalloc(&s->d_tails, sizeof(float) * max_streams * 2 * kTailCap));
    chk(hipMalloc(&s->d_wave, sizeof(float) * s->wave_cap));
  }
  if (!chk.ok) { pk_mi355_stream_destroy(s); return nullptr; }
  return s;
}
}  // namespace

pk_mi355_stream *pkhost::CheckedStream(pk_mi355_am *am, const CreateRequest &r) {
  CreateDims dims;
  return CheckCreate(am, r, &dims) ? CreateStream(am, r, dims) : nullptr;
}

// The entries fill a CreateRequest (pk_create.h) in its fields' order; the last two say `live`, and whether a null model
// is "null model" (the four entries older than the deltas) or "model not finalized".
extern "C" {

pk_mi355_stream_t *pk_mi355_stream_create(pk_mi355_am_t *am, const float *global_stats41, int max_streams, int64_t max_step_samples) {
  return CheckedStream(am, CreateRequest{global_stats41, 0, true, max_streams, max_step_samples, true, false, nullptr, nullptr, nullptr, true, true});
}

pk_mi355_stream_t *pk_mi355_frontend_stream_create(pk_mi355_am_t *am, const pk_mi355_frontend_spec_t *spec, const float *global_stats,
                                                   int stats_len, int max_streams, int64_t max_step_samples) {
  return CheckedStream(am, CreateRequest{global_stats, stats_len, false, max_streams, max_step_samples, true, !spec || !global_stats, spec, nullptr, nullptr, true, true});
}

pk_mi355_stream_t *pk_mi355_features_stream_create(pk_mi355_am_t *am, const float *global_stats41, int max_streams, int64_t max_step_frames) {
  return CheckedStream(am, CreateRequest{global_stats41, 0, true, max_streams, max_step_frames, false, false, nullptr, nullptr, nullptr, true, true});
}

pk_mi355_stream_t *pk_mi355_features_stream_create_stats(pk_mi355_am_t *am, const float *global_stats, int stats_len, int max_streams,
                                                         int64_t max_step_frames) {
  return CheckedStream(am, CreateRequest{global_stats, stats_len, false, max_streams, max_step_frames, false, !global_stats, nullptr, nullptr, nullptr, true, true});
}

pk_mi355_stream_t *pk_mi355_deltas_stream_create(pk_mi355_am_t *am, const pk_mi355_deltas_spec_t *deltas, const pk_mi355_frontend_spec_t *frontend,
                                                 const float *global_stats, int stats_len, int max_streams, int64_t capacity) {
  return CheckedStream(am, CreateRequest{global_stats, stats_len, false, max_streams, capacity, frontend != nullptr, !deltas || (frontend && !global_stats),
                                frontend, deltas, nullptr, true, false});
}

pk_mi355_stream_t *pk_mi355_transform_stream_create(pk_mi355_am_t *am, const pk_mi355_transform_spec_t *transform,
                                                    const pk_mi355_deltas_spec_t *deltas, const pk_mi355_frontend_spec_t *frontend,
                                                    const float *global_stats, int stats_len, int max_streams, int64_t capacity) {
  return CheckedStream(am, CreateRequest{global_stats, stats_len, false, max_streams, capacity, frontend != nullptr, !transform || (frontend && !global_stats),
                                frontend, deltas, transform, true, false});
}

int pk_mi355_stream_in_dim(const pk_mi355_stream_t *s) {
  if (!s) return Fail(PK_MI355_E_INVALID, "null stream");
  return s->in_dim;
}

int pk_mi355_stream_transform_set_slot(pk_mi355_stream_t *s, int slot, const float *matrix, int rows, int cols) {
  if (int rc = SlotIndex(s, slot)) return rc;
  if (!matrix) return Fail(PK_MI355_E_INVALID, "null argument");
  if (!s->has_xform) return Fail(PK_MI355_E_STATE, "a slot's own transform needs a stream made by pk_mi355_transform_stream_create");
  const int D = s->core.am->feat_dim;
  if (rows != D) return Fail(PK_MI355_E_INVALID, "the slot's transform has %d rows, the model's features need %d", rows, D);
  if (cols != D && cols != D + 1)
    return Fail(PK_MI355_E_INVALID, "the slot's transform has %d columns, the model's %d-dim features need %d (linear) or %d (affine)", cols, D, D, D + 1);
  if (D > kMaxSlotTransformDim)         // (the stage keeps kTransformFrames rows of D floats in LDS)
    return Fail(PK_MI355_E_INVALID, "a slot's own transform needs a feature dimension of at most %d (got %d)", kMaxSlotTransformDim, D);
  const int64_t bad = pkxf::FirstNonFinite(matrix, (int64_t)rows * cols);
  if (bad >= 0)
    return Fail(PK_MI355_E_INVALID, "the slot's transform has an entry that is not finite (row %d, column %d)", (int)(bad / cols), (int)(bad % cols));
  Slot &z = s->slots[slot];
  if (z.state == kOpen && z.kind == PK_MI355_FEATS_NORMALIZED)
    return Fail(PK_MI355_E_STATE, "slot %d takes normalised features: no transform applies", slot);
  if (z.state != kOpen || z.nx != 0)
    return Fail(PK_MI355_E_STATE, "slot %d: a transform belongs to an open slot before its first transform frame is computed", slot);
  if (int rc = UseDevice(s->core.device)) return rc;
  const size_t each = (size_t)(D + 1) * pkxf::Ldo(D);
  if (!s->d_slot_mats) HIP_TRY(hipMalloc(&s->d_slot_mats, sizeof(float) * each * (size_t)s->max_streams));
  if (!s->uxf_area) {
    // The per-slot stage's staging, behind the global stage's in the allocation of the upload staging.  Nothing in that
    // allocation outlives a step: once the stream is idle it is made anew, larger.
    const int64_t at = RoundUp(s->upload_floats, 64), floats = at + s->xf_rows * D;
    float *grown = nullptr;
    HIP_TRY(hipStreamSynchronize(s->core.stream));
    HIP_TRY(hipMalloc(&grown, sizeof(float) * floats));
    hipFree(s->d_upload);
    s->d_upload = grown; s->upload_floats = floats; s->uxf_area = at;
  }
  std::vector<float> packed((size_t)cols * pkxf::Ldo(D));
  pkxf::PackTransposed(matrix, rows, cols, packed.data());
  HIP_TRY(hipMemcpyAsync(s->d_slot_mats + each * (size_t)slot, packed.data(), sizeof(float) * packed.size(), hipMemcpyHostToDevice, s->core.stream));
  HIP_TRY(hipStreamSynchronize(s->core.stream));        // (pageable memory: the copy has read its source)
  z.mat = cols == D + 1 ? kSlotMatAffine : kSlotMatLinear;
  return 0;
}

int pk_mi355_stream_feat_dim(const pk_mi355_stream_t *s) {
  if (!s) return Fail(PK_MI355_E_INVALID, "null stream");
  return s->core.am->feat_dim;
}

int pk_mi355_stream_base_dim(const pk_mi355_stream_t *s) {
  if (!s) return Fail(PK_MI355_E_INVALID, "null stream");
  return s->base_dim;
}

void pk_mi355_stream_destroy(pk_mi355_stream_t *s) {
  if (!s) return;
  hipSetDevice(s->core.device);
  if (s->core.stream) hipStreamSynchronize(s->core.stream);
  hipFree(s->d_delta_scales); hipFree(s->d_delta_ring);
  hipFree(const_cast<float *>(s->xf.mt)); hipFree(s->d_xf_ring); hipFree(s->d_slot_mats);
  hipFree(s->d_tails); hipFree(s->d_sums); hipFree(s->d_raw_hist); hipFree(s->d_hist); hipFree(s->d_feat_hist);
  hipFree(s->d_upload); hipFree(s->d_wave); hipFree(s->d_rows); hipFree(s->d_meta); hipFree(s->d_any);
  hipFree(s->d_norm_glob); hipFree(s->d_norm_spk); hipFree(s->d_norm_win); hipFree(s->d_norm_total); hipFree(s->d_norm_table); hipFree(s->d_norm_ring);
  s->resampler.Free();
  if (s->h_native) hipHostFree(s->h_native);
  hipFree(s->d_native);
  if (s->h_upload) hipHostFree(s->h_upload);
  if (s->h_meta) hipHostFree(s->h_meta);
  if (s->ev_staged) hipEventDestroy(s->ev_staged);
  FreeScorerCore(&s->core);
  delete s;
}

int pk_mi355_stream_open(pk_mi355_stream_t *s, int slot) { return pk_mi355_stream_open_rate(s, slot, kSampleRate); }

int pk_mi355_stream_open_rate(pk_mi355_stream_t *s, int slot, int rate) {
  if (int rc = SlotIndex(s, slot)) return rc;
  if (s->features_only) return Fail(PK_MI355_E_STATE, "a features-only stream object takes no audio (pk_mi355_stream_open_features)");
  Slot &z = s->slots[slot];
  if (z.state != kFree) return Fail(PK_MI355_E_STATE, "slot %d is %s", slot, z.state == kOpen ? "open" : "closed and not yet flushed by a step");
  const DeviceResampleTable *tab = nullptr;
  if (rate != kSampleRate) {
    if (int rc = UseDevice(s->core.device)) return rc;
    if (int rc = s->resampler.Table(rate, &tab)) return rc;
    if (!s->h_native) {
      const int64_t cap = 6 * s->max_step_samples + (int64_t)s->max_streams * kNativeCarryCap;
      HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&s->h_native), sizeof(float) * cap, hipHostMallocDefault));
      HIP_TRY(hipMalloc(&s->d_native, sizeof(float) * cap));
      s->native_cap = cap;
    }
  }
  if (int rc = ResetSlotNorm(s, slot)) return rc;
  z.state = kOpen;
  z.n = z.a = z.nd = z.nx = z.tail_len = 0;
  z.mat = kSlotMatNone;
  z.pending.clear();
  z.rate = rate; z.tab = tab;
  z.kind = -1;
  z.native.clear();
  z.nat_x0 = z.n_in = z.n_prod = 0;
  s->pending_total -= z.reserve;      // (zero unless the slot's last opening ended without its flush)
  z.reserve = 0;
  return 0;
}

int pk_mi355_stream_open_features(pk_mi355_stream_t *s, int slot, int kind) {
  if (int rc = SlotIndex(s, slot)) return rc;
  if (kind != PK_MI355_FEATS_NORMALIZED && kind != PK_MI355_FEATS_RAW) return Fail(PK_MI355_E_INVALID, "unknown feature kind %d", kind);
  if (kind == PK_MI355_FEATS_RAW && !s->have_stats && s->norm.mode == PK_MI355_NORM_SLIDING)
    return Fail(PK_MI355_E_INVALID, "raw features need the CMVN statistics the stream object was made without");
  Slot &z = s->slots[slot];
  if (z.state != kFree) return Fail(PK_MI355_E_STATE, "slot %d is %s", slot, z.state == kOpen ? "open" : "closed and not yet flushed by a step");
  // (RAW at another dimension than 40, or under another normalisation spec than SLIDING, is laid out as NORMALIZED is)
  if (kind == PK_MI355_FEATS_NORMALIZED || s->base_dim != kNumBins || s->norm.mode != PK_MI355_NORM_SLIDING)
    if (int rc = EnsureFeatureHistory(s)) return rc;
  if (int rc = ResetSlotNorm(s, slot)) return rc;
  z.state = kOpen;
  z.n = z.a = z.nd = z.nx = z.tail_len = 0;
  z.mat = kSlotMatNone;
  z.pending.clear();
  z.rate = kSampleRate; z.tab = nullptr;
  z.kind = kind;
  z.native.clear();
  z.nat_x0 = z.n_in = z.n_prod = 0;
  s->pending_total -= z.reserve;      // (as pk_mi355_stream_open_rate)
  z.reserve = 0;
  return 0;
}

int pk_mi355_stream_slot_kind(const pk_mi355_stream_t *s, int slot) {
  if (int rc = SlotIndex(s, slot)) return rc;
  return s->slots[slot].kind;
}

int pk_mi355_stream_push_features(pk_mi355_stream_t *s, int slot, const float *frames, int num_frames) {
  if (int rc = SlotIndex(s, slot)) return rc;
  Slot &z = s->slots[slot];
  if (z.state != kOpen) return Fail(PK_MI355_E_STATE, "slot %d is not open", slot);
  if (z.kind < 0) return Fail(PK_MI355_E_STATE, "slot %d is open for audio (pk_mi355_stream_push)", slot);
  if (num_frames < 0 || (num_frames > 0 && !frames)) return Fail(PK_MI355_E_INVALID, "bad frames");
  if (s->pending_total + (int64_t)num_frames * s->frame_cost > s->max_step_samples)
    return Fail(PK_MI355_E_INVALID, "push of %d frames exceeds the step capacity (%lld pending of %lld, a frame counts %d)", num_frames,
                (long long)s->pending_total, (long long)s->max_step_samples, s->frame_cost);
  // (a deltas object: RAW frames are in front of the deltas, base_dim wide; NORMALIZED ones are past them)
  z.pending.insert(z.pending.end(), frames, frames + (size_t)num_frames * (z.kind == PK_MI355_FEATS_RAW ? s->base_dim : s->core.am->feat_dim));
  s->pending_total += (int64_t)num_frames * s->frame_cost;
  return 0;
}

int pk_mi355_stream_rate(const pk_mi355_stream_t *s, int slot) {
  if (int rc = SlotIndex(s, slot)) return rc;
  return s->slots[slot].rate;
}

int pk_mi355_stream_push(pk_mi355_stream_t *s, int slot, const float *samples, int num_samples) {
  if (int rc = SlotIndex(s, slot)) return rc;
  if (s->features_only) return Fail(PK_MI355_E_STATE, "a features-only stream object takes no audio (pk_mi355_stream_push_features)");
  Slot &z = s->slots[slot];
  if (z.state != kOpen) return Fail(PK_MI355_E_STATE, "slot %d is not open", slot);
  if (z.kind >= 0) return Fail(PK_MI355_E_STATE, "slot %d is open for features (pk_mi355_stream_push_features)", slot);
  if (num_samples < 0 || (num_samples > 0 && !samples)) return Fail(PK_MI355_E_INVALID, "bad samples");
  if (z.tab) {                         // samples at the slot's rate: what counts is the 16 kHz samples they become
    const int64_t reserve = ResampleNumOutput(z.tab->host, z.n_in + num_samples) - z.n_prod;
    if (s->pending_total + reserve - z.reserve > s->max_step_samples)
      return Fail(PK_MI355_E_INVALID, "push of %d samples at %d Hz exceeds the step capacity (%lld pending of %lld at 16 kHz)", num_samples,
                  z.rate, (long long)s->pending_total, (long long)s->max_step_samples);
    z.native.insert(z.native.end(), samples, samples + num_samples);
    z.n_in += num_samples;
    s->pending_total += reserve - z.reserve;
    z.reserve = reserve;
    return 0;
  }
  if (s->pending_total + num_samples > s->max_step_samples)
    return Fail(PK_MI355_E_INVALID, "push of %d samples exceeds the step capacity (%lld pending of %lld)", num_samples,
                (long long)s->pending_total, (long long)s->max_step_samples);
  z.pending.insert(z.pending.end(), samples, samples + num_samples);
  s->pending_total += num_samples;
  return 0;
}

int pk_mi355_stream_push_i16(pk_mi355_stream_t *s, int slot, const int16_t *samples, int num_samples) {
  if (int rc = SlotIndex(s, slot)) return rc;
  if (num_samples < 0 || (num_samples > 0 && !samples)) return Fail(PK_MI355_E_INVALID, "bad samples");
  std::vector<float> f(samples, samples + num_samples);    // exact: 16-bit integers
  return pk_mi355_stream_push(s, slot, f.data(), num_samples);
}

int pk_mi355_stream_close(pk_mi355_stream_t *s, int slot) {
  if (int rc = SlotIndex(s, slot)) return rc;
  Slot &z = s->slots[slot];
  if (z.state != kOpen) return Fail(PK_MI355_E_STATE, "slot %d is not open", slot);
  z.state = kClosed;
  return 0;
}

int pk_mi355_stream_norm_set(pk_mi355_stream_t *s, const pk_mi355_norm_spec_t *spec) {
  if (!s || !spec) return Fail(PK_MI355_E_INVALID, "null argument");
  if (int rc = pknorm::CheckSpec(spec)) return rc;      // (names the field)
  if (spec->mode == PK_MI355_NORM_UTTERANCE)
    return Fail(PK_MI355_E_INVALID, "norm spec: mode utterance cannot run on a live stream: an utterance's statistics do not exist while it is "
                "live (mode speaker, or online CMVN, pk_mi355_stream_norm_set_online_cmvn)");
  if (int rc = NoSlotInUse(s)) return rc;
  if (spec->mode != PK_MI355_NORM_SLIDING) {
    if (int rc = EnsureFeatureHistory(s)) return rc;
    if (int rc = UseDevice(s->core.device)) return rc;
    const size_t D = (size_t)s->base_dim, n = (size_t)s->max_streams;
    if (!s->d_norm_total) HIP_TRY(hipMalloc(&s->d_norm_total, sizeof(double) * 2 * D * n));
    if (!s->d_norm_table) HIP_TRY(hipMalloc(&s->d_norm_table, sizeof(float) * 2 * D * n));
  }
  s->norm = *spec;
  return 0;
}

int pk_mi355_stream_norm_set_online_cmvn(pk_mi355_stream_t *s, const pk_mi355_online_cmvn_spec_t *spec, const double *global_stats) {
  if (!s || !spec) return Fail(PK_MI355_E_INVALID, "null argument");
  const size_t D = (size_t)s->base_dim, n = (size_t)s->max_streams, rec = 2 * (D + 1);
  if (int rc = pknorm::CheckOnlineSpec(spec, global_stats, (int)D)) return rc;      // (names the field)
  if (int rc = NoSlotInUse(s)) return rc;
  if (int rc = EnsureFeatureHistory(s)) return rc;
  if (int rc = UseDevice(s->core.device)) return rc;
  if (!s->d_norm_total) HIP_TRY(hipMalloc(&s->d_norm_total, sizeof(double) * 2 * D * n));
  if (!s->d_norm_win) HIP_TRY(hipMalloc(&s->d_norm_win, sizeof(double) * 2 * D * n));
  if (!s->d_norm_glob) HIP_TRY(hipMalloc(&s->d_norm_glob, sizeof(double) * rec));
  if (!s->d_norm_spk) HIP_TRY(hipMalloc(&s->d_norm_spk, sizeof(double) * rec * n));
  if (s->ring_window < spec->cmn_window) {              // (no slot is in use: nothing is carried in the ring)
    HIP_TRY(hipStreamSynchronize(s->core.stream));
    hipFree(s->d_norm_ring);
    s->d_norm_ring = nullptr; s->ring_window = 0;
    HIP_TRY(hipMalloc(&s->d_norm_ring, sizeof(float) * n * (size_t)spec->cmn_window * D));
    s->ring_window = spec->cmn_window;
  }
  if (spec->global_frames > 0) {                        // (pageable memory: the copy has read the record when the call returns)
    HIP_TRY(hipMemcpyAsync(s->d_norm_glob, global_stats, sizeof(double) * rec, hipMemcpyHostToDevice, s->core.stream));
    HIP_TRY(hipStreamSynchronize(s->core.stream));
  }
  s->online_cmvn = *spec;
  s->norm = pk_mi355_norm_spec_t{pknorm::kNormOnlineCmvn, 1, spec->norm_vars};
  return 0;
}

int pk_mi355_stream_norm_set_speaker_stats(pk_mi355_stream_t *s, int slot, const double *stats) {
  if (int rc = SlotIndex(s, slot)) return rc;
  if (!stats) return Fail(PK_MI355_E_INVALID, "null argument");
  const int mode = s->norm.mode;
  if (mode != PK_MI355_NORM_SPEAKER && mode != pknorm::kNormOnlineCmvn)
    return Fail(PK_MI355_E_STATE, "speaker statistics need mode speaker (pk_mi355_stream_norm_set) or online CMVN (pk_mi355_stream_norm_set_online_cmvn)");
  Slot &z = s->slots[slot];
  if (z.state != kOpen || z.n != 0)
    return Fail(PK_MI355_E_STATE, "slot %d: speaker statistics belong to an open slot before its first frame is computed", slot);
  if (z.kind == PK_MI355_FEATS_NORMALIZED) return Fail(PK_MI355_E_STATE, "slot %d takes normalised features: no normalisation applies", slot);
  const int D = s->base_dim;
  if (mode == PK_MI355_NORM_SPEAKER) {
    std::vector<float> table((size_t)2 * D);
    if (int rc = pknorm::FinalizeSpeakerStats(stats, 1, D, s->norm.norm_means != 0, s->norm.norm_vars != 0, table.data())) return rc;
    if (int rc = UseDevice(s->core.device)) return rc;
    HIP_TRY(hipMemcpyAsync(s->d_norm_table + (size_t)slot * 2 * D, table.data(), sizeof(float) * 2 * D, hipMemcpyHostToDevice, s->core.stream));
  } else {
    if (int rc = pknorm::CheckOnlineSpeakerCounts(stats, 1, D)) return rc;
    if (int rc = UseDevice(s->core.device)) return rc;
    const size_t rec = 2 * ((size_t)D + 1);
    HIP_TRY(hipMemcpyAsync(s->d_norm_spk + slot * rec, stats, sizeof(double) * rec, hipMemcpyHostToDevice, s->core.stream));
  }
  HIP_TRY(hipStreamSynchronize(s->core.stream));        // (pageable memory: the copy has read its source)
  z.spk_set = true;
  return 0;
}

int pk_mi355_stream_norm_fetch_stats(pk_mi355_stream_t *s, int slot, double *out) {
  if (int rc = SlotIndex(s, slot)) return rc;
  if (!out) return Fail(PK_MI355_E_INVALID, "null argument");
  if (s->norm.mode != PK_MI355_NORM_SPEAKER && s->norm.mode != pknorm::kNormOnlineCmvn)
    return Fail(PK_MI355_E_STATE, "statistics are accumulated in mode speaker and under online CMVN only");
  const Slot &z = s->slots[slot];
  if (z.kind == PK_MI355_FEATS_NORMALIZED) return Fail(PK_MI355_E_STATE, "slot %d takes normalised features: no statistics", slot);
  const size_t D = (size_t)s->base_dim;
  for (size_t i = 0; i < 2 * (D + 1); ++i) out[i] = 0.0;
  if (z.n == 0) return 0;                               // (no frame computed since the slot was opened: the record of no frames)
  if (int rc = UseDevice(s->core.device)) return rc;
  std::vector<double> sums(2 * D);
  HIP_TRY(hipMemcpyAsync(sums.data(), s->d_norm_total + (size_t)slot * 2 * D, sizeof(double) * 2 * D, hipMemcpyDeviceToHost, s->core.stream));
  HIP_TRY(hipStreamSynchronize(s->core.stream));
  for (size_t d = 0; d < D; ++d) { out[d] = sums[d]; out[D + 1 + d] = sums[D + d]; }
  out[D] = (double)z.n;
  return 0;
}

int pk_mi355_stream_step(pk_mi355_stream_t *s, float prob_scale, int sync) {
  if (!s) return Fail(PK_MI355_E_INVALID, "null stream");
  ScorerCore &c = s->core;
  int rc = UseDevice(c.device);
  if (rc) return rc;
  pk_mi355_am *am = c.am;
  const int L = am->left, R = am->right, pad = L + R;
  bool any = false;
  for (const Slot &z : s->slots) any = any || z.state != kFree;
  if (!any) return Fail(PK_MI355_E_STATE, "step with no open slot");
  if (s->staged) HIP_TRY(hipEventSynchronize(s->ev_staged));   // the page-locked staging is free again
  s->staged = false;
  for (Slot &z : s->slots) { z.last_count = 0; z.last_flushed = false; }   // a step's rows are readable until the next step
  // ---- the step's plan, on the host
  StreamRec *recs = reinterpret_cast<StreamRec *>(s->h_meta);
  char *lay_base = s->h_meta + RoundUp(sizeof(StreamRec) * s->max_streams, 256);
  const size_t shift4_at = s->meta_bytes - sizeof(int32_t) * Shift4Cap(c.max_cols);
  // A deltas object: lrecs[k] is what the layout launch sees for the slot of recs[k] -- for an audio
  // or RAW slot the delta frames [nd, nd1) that StreamDeltaKernel makes final, as rows of the delta staging; for a
  // NORMALIZED slot recs[k] itself.  On every other object the layout reads recs.
  // A transform object has two arrays more, behind the deltas' where there is one: xrecs[k], the
  // transform frames [nx, nx1) that become final -- rows of the transform's staging when the spec has a matrix, else the
  // rows the stage in front left -- and urecs[k], the same frames as rows of the per-slot stage's staging.  The layout reads
  // the last stage that runs in this step (lrecs, chosen once the records are made).
  const bool dl = s->has_deltas, xf = s->has_xform, chained = dl || xf;
  auto extra = [&](int i) {
    return reinterpret_cast<StreamRec *>(lay_base + RoundUp((sizeof(int64_t) * 2 + sizeof(int32_t)) * s->max_streams, 256) +
                                         i * RoundUp(sizeof(StreamRec) * s->max_streams, 256));
  };
  StreamRec *drecs = dl ? extra(0) : recs, *xrecs = xf ? extra(dl ? 1 : 0) : drecs, *urecs = xf ? extra(dl ? 2 : 1) : xrecs;
  const bool xf_global = xf && s->xf.mt != nullptr;
  const int Din = s->in_dim, Rt = s->xf.right;          // (Rt: 0 on every other object)
  int64_t xout = 0;                                   // rows of the transform stagings taken
  int max_xnew = 0, n_xf = 0;                         // the most transform frames a record makes final; records StreamTransformKernel serves
  bool slot_mats = false;                             // a record's slot holds a matrix of its own: the per-slot stage runs
  // Records.  A 40-dim object: audio and RAW slots (StreamAssembleKernel, FbankKernel or FbankAnyKernel,
  // StreamCmvnKernel) from the front of the array, NORMALIZED slots (StreamFeatureLayoutKernel) from its back.  Another
  // dimension: audio slots from the front, feature slots of both kinds from the back; on an object with a front-end spec
  // (rows_area != 0) the back block is then moved up behind the front one, in slot order (below, once the plan is known
  // to fit), so that records [0, n_front) are exactly the audio slots -- what the assembly and the fbank see -- and records
  // [0, n_front + n_back) exactly the slots taking part -- what StreamCmvnChainKernel and StreamFeatureLayoutKernel see.
  // Rows and columns are in slot order whichever the type and wherever the record lies.
  std::vector<int> who, at, flushed;                  // slots taking part, their records; closed slots with nothing left
  int64_t woff = 0, upl = 0, raw = 0, out = 0, col = 0, native_total = 0;
  int max_m = 0, n_front = 0, n_back = 0, n_audio = 0, raw_pushed = 0, chain_pushed = 0, max_feat_cols = 0;
  int64_t dout = 0;                                   // rows of the delta staging taken
  int max_new = 0, n_delta = 0;                       // the most delta frames a record makes final; records StreamDeltaKernel serves
  const int D = am->feat_dim, Db = s->base_dim, M = s->reach;
  // Another normalisation spec than SLIDING: nothing goes through StreamCmvnKernel's fused path.  RAW
  // slots at 40 become back records as at every other dimension (normalised where they lie in the upload staging); audio
  // slots at 40 stay in front, their rows in d_rows (row_off counts from there), and are laid out from there.
  const int nmode = s->norm.mode;
  const bool sliding = nmode == PK_MI355_NORM_SLIDING;
  if (nmode == PK_MI355_NORM_SPEAKER)
    for (int slot = 0; slot < s->max_streams; ++slot) {
      const Slot &z = s->slots[slot];
      if (z.state != kFree && z.kind != PK_MI355_FEATS_NORMALIZED && !z.spk_set)
        return Fail(PK_MI355_E_STATE, "mode speaker: slot %d has no speaker statistics (pk_mi355_stream_norm_set_speaker_stats)", slot);
    }
  std::vector<ShiftSpan> spans;                       // (end row, column shift) per slot with rows
  for (int slot = 0; slot < s->max_streams; ++slot) {
    const Slot &z = s->slots[slot];
    if (z.state == kFree) continue;
    const bool closed = z.state == kClosed;
    // a native-rate slot's new samples are the outputs that became final (all of them once it is closed)
    // (a feature slot: no samples, an empty segment; its frames are what was pushed)
    // (RAW at a dimension other than 40: StreamCmvnChainKernel normalises the pushed rows where they lie, and the
    // record then goes with the NORMALIZED ones)
    // (a front-end spec at a dimension other than 40, DESIGN.md section 18: audio records go the same way, their rows
    // written into the staging's row area by FbankAnyKernel; they stay in front, where the assembly and the fbank look)
    const bool feats = z.kind >= 0, spec_rows = !feats && s->rows_area > 0;
    const bool layout = z.kind == PK_MI355_FEATS_NORMALIZED || (feats && (Db != kNumBins || !sliding || chained));
    const bool delta_rec = dl && z.kind != PK_MI355_FEATS_NORMALIZED, xf_rec = xf && z.kind != PK_MI355_FEATS_NORMALIZED;
    const int width = z.kind == PK_MI355_FEATS_NORMALIZED ? D : Db;       // floats of a pushed frame
    const bool front_rows = !feats && !sliding && !spec_rows;       // an audio slot at 40 under a norm spec: laid out from d_rows
    const int new_len = feats    ? 0
                        : !z.tab ? (int)z.pending.size()
                                 : (int)((closed ? ResampleNumOutput(z.tab->host, z.n_in) : ResampleNumFinal(z.tab->host, z.n_in)) - z.n_prod);
    const int seg = z.tail_len + new_len;
    const int m = feats ? (int)(z.pending.size() / width) : pk_mi355_num_frames(seg);
    const int n = z.n + m;
    // open: R frames of look-ahead held back -- and in front of deltas M base frames more (pkdelta::StreamDeltaAdvance)
    const pkdelta::StreamDeltaCounts dc = delta_rec ? pkdelta::StreamDeltaAdvance(n, z.nd, z.a, M, R, closed) : pkdelta::StreamDeltaCounts{n, 0};
    // (behind a transform Rt input frames more: pkxf::StreamTransformAdvance, over the delta frames where there are deltas)
    const pkxf::StreamTransformCounts tc = xf_rec ? pkxf::StreamTransformAdvance(dc.nd1, z.nx, z.a, Rt, R, closed) : pkxf::StreamTransformCounts{0, 0};
    const int b = xf_rec ? tc.b : delta_rec ? dc.b : closed ? n : std::max(z.a, n - R);
    if (new_len == 0 && m == 0 && b == z.a) {
      if (closed) flushed.push_back(slot);
      continue;
    }
    const int rec_at = layout ? s->max_streams - 1 - n_back++ : n_front++;
    StreamRec &r = recs[rec_at];
    r.kind = z.kind; r.hist_par = z.hist_par; r.ring_par = z.ring_par; r.xf_bits = z.xf_par | (z.mat << 1);
    r.slot = slot; r.tail_len = z.tail_len; r.new_len = new_len; r.tail_par = z.tail_par;
    r.n_old = z.n; r.m = m; r.a = z.a; r.b = b; r.closed = closed ? 1 : 0;
    r.woff = woff; r.new_off = upl; r.raw_base = layout ? 0 : raw;
    r.row_off = spec_rows ? s->rows_area + raw * Db : front_rows ? raw * Db : upl;
    r.col_base = 0; r.cols = 0;
    if (b > z.a) {
      // Rows slot after slot, each padded to four; the slot's columns a - L .. b + R - 1 in a region of RoundUp(b - a, 4)
      // + L + R columns.  The column of row j is j + (the number of earlier slots with rows) x (L + R): never negative.
      // (The batch scorer's compact rows pad the rows but not the columns: their shift goes negative when L + R < 3.)
      const int32_t shift = (int32_t)(col - out);
      r.col_base = col;
      r.cols = (int)RoundUp(b - z.a, 4) + pad;
      out += RoundUp(b - z.a, 4);
      col += r.cols;
      spans.push_back({out, shift});
      if (layout || spec_rows || front_rows) max_feat_cols = std::max(max_feat_cols, r.cols);
    }
    if (dl) {
      StreamRec &lr = drecs[rec_at];
      lr = r;
      if (delta_rec) {
        lr.n_old = z.nd; lr.m = dc.nd1 - z.nd;
        lr.row_off = s->delta_area + dout * Din;
        dout += lr.m;
        max_new = std::max(max_new, lr.m);
        ++n_delta;
      }
    }
    if (xf) {
      StreamRec &xr = xrecs[rec_at], &ur = urecs[rec_at];
      xr = drecs[rec_at];                // (without a matrix in the spec nx = nin: the rows the stage in front left, as they lie)
      if (xf_rec) {
        xr.n_old = z.nx; xr.m = tc.nx1 - z.nx;
        if (xf_global) xr.row_off = s->xf_area + xout * D;
      }
      ur = xr;
      if (xf_rec) {
        ur.row_off = s->uxf_area + xout * D;
        xout += xr.m;
        max_xnew = std::max(max_xnew, xr.m);
        ++n_xf;
        slot_mats = slot_mats || z.mat != kSlotMatNone;
      }
    }
    woff += seg; upl += feats ? (int64_t)m * width : new_len;
    if (!layout) raw += m;
    if (z.tab && new_len) native_total += (int64_t)z.native.size();
    if (!feats) { max_m = std::max(max_m, m); ++n_audio; }
    if (z.kind == PK_MI355_FEATS_RAW) (layout ? chain_pushed : raw_pushed) += m;
    who.push_back(slot);
    at.push_back(rec_at);
  }
  const int64_t upl_cap = s->rows_area ? s->rows_area : s->upload_cap;      // (a row area: the pushes end where it begins)
  const bool staging_fits = woff <= s->wave_cap && upl <= upl_cap && native_total <= s->native_cap &&
                            (!s->rows_area || s->rows_area + raw * Db <= s->upload_cap) && dout <= s->delta_rows && xout <= s->xf_rows &&
                            (!slot_mats || s->uxf_area > 0);
  const bool rows_fit = raw <= c.max_frames && RoundUp(out, kTileF16) <= c.max_cols && col <= c.max_cols;
  if (chained && n_front > 0 && !s->rows_area)        // (pk_plan.cc: no plan serves front records of a deltas or transform object without a row area)
    return Fail(PK_MI355_E_INVALID, "internal: a deltas stream with audio records and no row area");
  if (!staging_fits || !rows_fit || ((n_back > 0 || (!sliding && n_front > 0)) && !s->d_feat_hist))
    return Fail(PK_MI355_E_INVALID, "internal: step exceeds the stream's capacity");
  // A front-end spec at D != 40: the back block (taken last first) moves up behind the front one, as told above.
  if (s->rows_area) {
    const std::vector<StreamRec> back(recs + (s->max_streams - n_back), recs + s->max_streams);
    for (int j = 0; j < n_back; ++j) recs[n_front + j] = back[n_back - 1 - j];
    for (int i = 0; i < s->extra_recs; ++i) {
      StreamRec *e = extra(i);
      const std::vector<StreamRec> eback(e + (s->max_streams - n_back), e + s->max_streams);
      for (int j = 0; j < n_back; ++j) e[n_front + j] = eback[n_back - 1 - j];
    }
    for (int &k : at)
      if (k >= n_front) k = n_front + (s->max_streams - 1 - k);
  }
  // the column shift of every group of four rows (the groups past the last row keep the last shift)
  const int64_t total_rows = out;
  int32_t bad = 0;
  if (total_rows > 0 && !ExpandShift4(spans, total_rows, c.zero_span, reinterpret_cast<int32_t *>(s->h_meta + shift4_at), &bad))
    return Fail(PK_MI355_E_INVALID, "internal: column shift %d outside [0, %lld]", bad, (long long)(c.zero_span - kTile));
  StreamRec *lrecs = slot_mats ? urecs : xrecs;       // (xrecs is drecs without a transform, drecs is recs without deltas)
  // the plan holds: consume every pushed sample, advance the slots
  std::vector<ResampleItem> items;
  int64_t native_at = 0;
  for (size_t k = 0; k < who.size(); ++k) {
    const StreamRec &r = recs[at[k]];
    Slot &z = s->slots[r.slot];
    const bool delta_rec = dl && z.kind != PK_MI355_FEATS_NORMALIZED;
    const bool xf_rec = xf && z.kind != PK_MI355_FEATS_NORMALIZED;
    const int lay_m = lrecs[at[k]].m;    // the fresh rows the layout sees (behind deltas or a transform: the frames that became final)
    if (z.kind >= 0) {                   // pushed frames, frame-major
      if (r.m) memcpy(s->h_upload + r.new_off, z.pending.data(), sizeof(float) * (size_t)r.m * (z.kind == PK_MI355_FEATS_NORMALIZED ? D : Db));
      if (lay_m && (z.kind == PK_MI355_FEATS_NORMALIZED || Db != kNumBins || !sliding || chained)) z.hist_par ^= 1;    // the step writes the other history buffer
    } else if (z.tab && r.new_len) {
      // outputs [n_prod, n_prod + new_len) from the samples held, straight to where pushed 16 kHz samples would lie
      const ResampleTable &t = z.tab->host;
      memcpy(s->h_native + native_at, z.native.data(), sizeof(float) * z.native.size());
      items.push_back(Resampler::Item(*z.tab, s->d_native + native_at, z.nat_x0, (int64_t)z.native.size(), z.n_prod, z.n_prod + r.new_len,
                                      s->d_upload + r.new_off));
      native_at += (int64_t)z.native.size();
      z.n_prod += r.new_len;
      // the carry: nothing before the first sample the next output's window can read is read again
      const int64_t keep = std::min(z.n_in, std::max(z.nat_x0, z.n_prod / t.P * t.Q + t.min_first));
      z.native.erase(z.native.begin(), z.native.begin() + (keep - z.nat_x0));
      z.nat_x0 = keep;
      z.reserve = ResampleNumOutput(t, z.n_in) - z.n_prod;
    } else if (r.new_len) {
      memcpy(s->h_upload + r.new_off, z.pending.data(), sizeof(float) * r.new_len);
    }
    z.pending.clear();
    if (z.kind < 0) {
      z.tail_len = r.tail_len + r.new_len - kFrameShift * r.m;
      z.tail_par ^= 1;
      if ((s->rows_area || !sliding) && lay_m) z.hist_par ^= 1;     // laid out by StreamFeatureLayoutKernel: the step writes the other history buffer
    }
    if (delta_rec) {
      if (r.m) z.ring_par ^= 1;          // StreamDeltaKernel writes the other ring buffer
      z.nd = drecs[at[k]].n_old + drecs[at[k]].m;
    }
    if (xf_rec) {
      if (drecs[at[k]].m && s->xf.left + s->xf.right > 0) z.xf_par ^= 1;    // StreamTransformKernel writes the other ring buffer
      z.nx = xrecs[at[k]].n_old + xrecs[at[k]].m;
    }
    z.n = r.n_old + r.m;
    z.a = r.b;
    z.last_first = r.a; z.last_count = r.b - r.a;
    if (z.state == kClosed) { z.state = kFree; z.last_flushed = true; }   // flushed: the slot may be opened again
  }
  for (int slot : flushed) { s->slots[slot].state = kFree; s->slots[slot].last_flushed = true; }
  s->pending_total = 0;
  for (Slot &z : s->slots) {
    if (z.state == kFree) z.reserve = 0;
    s->pending_total += z.reserve;     // native-rate slots: the outputs that are not final yet stay counted
  }
  {
    int64_t o = 0;
    for (size_t k = 0; k < who.size(); ++k) {
      Slot &z = s->slots[who[k]];
      z.last_out = o;
      o += RoundUp(z.last_count, 4);
    }
  }
  const int K = (int)who.size();
  if (K == 0) return sync ? pk_mi355_stream_synchronize(s) : 0;
  // UttLayout arrays
  int64_t *h_woff = reinterpret_cast<int64_t *>(lay_base);
  int64_t *h_rawb = h_woff + s->max_streams;
  int32_t *h_T = reinterpret_cast<int32_t *>(h_rawb + s->max_streams);
  for (int k = 0; k < n_front; ++k) { h_woff[k] = recs[k].woff; h_rawb[k] = recs[k].raw_base; h_T[k] = recs[k].kind < 0 ? recs[k].m : 0; }
  // ---- uploads (one for the samples, one for the plan) and the launches, all on the stream
  if (upl) HIP_TRY(hipMemcpyAsync(s->d_upload, s->h_upload, sizeof(float) * upl, hipMemcpyHostToDevice, c.stream));
  if (native_at) {                     // the native-rate slots' new 16 kHz samples, written over their part of d_upload
    HIP_TRY(hipMemcpyAsync(s->d_native, s->h_native, sizeof(float) * native_at, hipMemcpyHostToDevice, c.stream));
    if ((rc = s->resampler.Run(items, c.stream))) return rc;
  }
  HIP_TRY(hipMemcpyAsync(s->d_meta, s->h_meta, s->meta_bytes, hipMemcpyHostToDevice, c.stream));
  HIP_TRY(hipEventRecord(s->ev_staged, c.stream));
  s->staged = true;
  const StreamRec *d_recs = reinterpret_cast<const StreamRec *>(s->d_meta);
  auto on_device = [&](const StreamRec *h) { return reinterpret_cast<const StreamRec *>(s->d_meta + (reinterpret_cast<const char *>(h) - s->h_meta)); };
  const StreamRec *d_lrecs = on_device(lrecs), *d_drecs = on_device(drecs), *d_xrecs = on_device(xrecs), *d_urecs = on_device(urecs);
  const char *d_lay = s->d_meta + (lay_base - s->h_meta);
  const int64_t *d_woff = reinterpret_cast<const int64_t *>(d_lay);
  const int64_t *d_rawb = d_woff + s->max_streams;
  const int32_t *d_T = reinterpret_cast<const int32_t *>(d_rawb + s->max_streams);
  UttLayout lay{d_woff, d_T, d_rawb, d_rawb};
  // The plan (pk_plan.h; DESIGN.md, "The two plans").  The front stage: assembly and fbank over the n_front front records,
  // the rows [raw_base][D] going to d_rows, or on an object with a row area to the staging behind the samples.
  const pkplan::StreamPlan plan = pkplan::PlanStream(s->rows_area != 0, nmode, pkplan::StepCounts{n_front, n_back, n_audio, max_m, raw_pushed, chain_pushed}, dl,
                                                     xf, xf_global, slot_mats);
  if (plan.front) {
    float *dst = s->rows_area ? s->d_upload + s->rows_area : s->d_rows;
    LaunchStreamAssemble(d_recs, n_front, s->d_upload, s->d_tails, s->d_wave, c.stream);
    if (s->d_any) LaunchFbankAny(s->d_wave, nullptr, lay, n_front, max_m, c.d_tables, s->d_any, Db, dst, c.stream);
    else LaunchFbank(s->d_wave, nullptr, lay, n_front, max_m, c.d_tables, dst, c.stream);
  }
  // Then every block of records through its normaliser (the back block's before its layout, which reads the rows the
  // normaliser leaves behind) and its layout.
  for (int k = 0; k < plan.n; ++k) {
    const pkplan::Block &bl = plan.block[k];
    const StreamRec *r = d_recs + (bl.back ? s->max_streams - n_back : 0);
    const int first = bl.back ? s->max_streams - n_back : 0;
    const StreamRec *lr = d_lrecs + first;     // (r itself without deltas and transform)
    const StreamRec *dr = d_drecs + first, *xr = d_xrecs + first, *ur = d_urecs + first;
    float *rows = bl.step_rows ? s->d_rows : s->d_upload;
    if (bl.raw_rows) LaunchStreamRawRows(r, bl.count, s->d_upload, s->d_rows, c.stream);
    if (bl.norm == pkplan::kStreamNorm) LaunchStreamNorm(r, bl.count, Db, rows, NormState(s), c.stream);
    else if (bl.norm == pkplan::kStreamCmvnChain) LaunchStreamCmvnChain(r, bl.count, Db, rows, c.d_global, c.d_cmvn_tab, s->d_sums, s->d_raw_hist, c.stream);
    if (bl.delta && n_delta > 0) LaunchStreamDelta(r, dr, bl.count, max_new, Db, s->deltas, s->d_delta_scales, rows, s->d_delta_ring, c.stream);
    if (bl.transform && n_xf > 0) LaunchStreamTransform(dr, xr, bl.count, max_xnew, s->xf, false, rows, s->d_xf_ring, c.stream);
    if (bl.slot_transform && n_xf > 0)
      LaunchStreamTransform(xr, ur, bl.count, max_xnew, TransformStage{D, 0, 0, D, false, s->d_slot_mats, (int64_t)(D + 1) * pkxf::Ldo(D)}, true, rows,
                            s->d_xf_ring, c.stream);
    if (bl.fused) LaunchStreamCmvn(r, bl.count, rows, c.d_global, c.d_cmvn_tab, s->d_sums, s->d_raw_hist, s->d_hist, s->hist_len, L, R, c.d_yt, c.ldy, c.stream);
    else LaunchStreamFeatureLayout(lr, bl.count, max_feat_cols, rows, s->d_feat_hist, s->hist_len, D, L, R, c.d_yt, c.ldy, c.stream);
  }
  const Operand op{c.d_yt, nullptr, c.ldy, ZeroSource(c), reinterpret_cast<const int32_t *>(s->d_meta + shift4_at)};
  const Lane lane{c.stream, &c.exec};
  if ((rc = WalkChunks(am, op, total_rows, c.chunk, &lane, 1, true, prob_scale, c.d_ll, nullptr))) return rc;
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) return Fail(PK_MI355_E_DEVICE, "stream step launch failed: %s", hipGetErrorString(le));
  if (sync) return pk_mi355_stream_synchronize(s);
  return 0;
}

int pk_mi355_stream_synchronize(pk_mi355_stream_t *s) {
  if (!s) return Fail(PK_MI355_E_INVALID, "null stream");
  HIP_TRY(hipStreamSynchronize(s->core.stream));
  return 0;
}

const float *pk_mi355_stream_loglik_device(const pk_mi355_stream_t *s, int slot, int *first_frame, int *count) {
  if (first_frame) *first_frame = 0;
  if (count) *count = 0;
  if (SlotIndex(s, slot)) return nullptr;
  const Slot &z = s->slots[slot];
  if (first_frame) *first_frame = z.last_first;
  if (count) *count = z.last_count;
  return z.last_count > 0 ? s->core.d_ll + z.last_out * s->core.am->num_pdfs : nullptr;
}

int pk_mi355_stream_fetch(pk_mi355_stream_t *s, int slot, pk_decodable_t *out, int *first_frame) {
  int rc = SlotIndex(s, slot);
  if (rc) return rc;
  if (!out) return Fail(PK_MI355_E_INVALID, "null decodable");
  if ((rc = UseDevice(s->core.device))) return rc;
  int count = 0, first = 0;
  const float *src = pk_mi355_stream_loglik_device(s, slot, &first, &count);
  if (first_frame) *first_frame = first;
  ClearDecodable(out, s->core.am);
  if (count == 0) return 0;
  return FetchRows(src, count, s->core.am->num_pdfs, s->core.stream, "stream fetch", out, [] { return 0; });
}

}  // extern "C"
