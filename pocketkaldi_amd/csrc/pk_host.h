// pk_host.h -- what the host-side translation units of libpk_mi355.so share (internal):
//   pk_files.cc          (plain C++, pk_files.h) the error state and every file reader: model / config / WAV / graph,
//                        the graph's split into the decoder's arc lists
//   capi_model.hip       device selection, model construction, operand exponents
//   capi_exec.hip        the layer executor and (pk_score.h) the chunk walk over it, pk_mi355_nnet_propagate, pk_decodable_*
//   capi_batch.hip       (pk_score.h) the scorer core, the batched device-resident scorer over it (also the model's own
//                        one-utterance scorers), result arenas and views
//   capi_stream.hip      (pk_score.h) the online scorer over the same core
//   capi_io.hip          model files -> device model, the single-utterance front-end entries, test hooks
//   capi_resample.hip    (pk_resample.h) a rate's polyphase table on the device, the checked plan upload and launch of
//                        ResampleKernel (resample.hip) that the batch and the online scorer convert through, pk_mi355_resample
//   capi_collective.hip  the one collective: weight-blob broadcast over the caller's RCCL communicator
//   capi_recognizer.hip  pk_load + pk_process as one object over the entries of the others
//   capi_online_recognizer.hip  pk_load + a live pk_process: the online scorer and the online decoder as one object
//   capi_decoder.hip     (pk_decode.h) the decoder core -- graph, work areas, arenas -- and the batch decoder over it
//   capi_online_decoder.hip  (pk_decode.h) the online decoder over the same core
// (decode.hip and stream.hip hold the decoder's and the online scorer's kernels and their launchers, declared in
// pk_decode.h and pk_score.h; features.hip the batch scorer's layout kernel for features, declared in pk_score.h.)
// Nothing here is part of the ABI (include/pk_mi355.h is); the library exports the C entries only
// (libpk_mi355.map).
#ifndef PK_HOST_H_
#define PK_HOST_H_

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "pk_files.h"
#include "pk_kernels.h"
#include "pk_tables.h"

namespace pkhost {

using namespace pkmi;

// ------------------------------------------------------------------ device selection (capi_model.hip; errors: pk_files.h)

// Like hipSetDevice, the selected device is a per-thread setting (a worker thread that never
// called pk_mi355_set_device creates its objects on device 0).
int CurrentDevice();
int UseDevice(int device);

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return ::pkhost::Fail(PK_MI355_E_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                            __FILE__, __LINE__);                                       \
  } while (0)

inline int64_t RoundUp(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
// the two precisions that run on the fp16 matrix cores share layouts and code paths
inline bool IsF16(int precision) { return precision == PK_MI355_PRECISION_F16X3 || precision == PK_MI355_PRECISION_F16; }

// ------------------------------------------------------------------ environment switches
// Every PK_MI355_* switch is an A/B or test switch, never needed in production.  They are read when an
// OBJECT is made (a model, a batch scorer) and kept in it: no launch path calls getenv.
struct ModelKnobs {
  bool wave_tail32 = true;       // PK_MI355_FUSED_TAIL32 (0: the workgroup-per-row TailKernel instead of the wave tail)
  int fused_tail_min_tiles = 384;  // PK_MI355_FUSED_TAIL_MIN_TILES (tests raise it to force the stand-alone wave tail)
  int tail_walk = 0;             // PK_MI355_TAIL_WALK: super-tile columns of the fused-tail launch's walk (0: the whole row of tiles)
  int l1_ring = 2;               // PK_MI355_L1_RING: LDS slabs of the spliced first layer's big-tile launch (2: four workgroups per CU; 3: three)
  bool tail_strip = true;        // PK_MI355_TAIL_STRIP (0: the last column tile of the fused-tail launch stays a full 128-wide tile)
};
ModelKnobs ReadModelKnobs();

// ------------------------------------------------------------------ timing

struct Timer {
  bool enabled = false;
  struct Rec { int kind; hipEvent_t a, b; };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
  hipEvent_t Get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
  }
  void Reset() {
    for (auto &r : recs) { pool.push_back(r.a); pool.push_back(r.b); }
    recs.clear();
  }
  int Begin(int kind, hipStream_t s) {
    if (!enabled) return -1;
    Rec r{kind, Get(), Get()};
    hipEventRecord(r.a, s);
    recs.push_back(r);
    return (int)recs.size() - 1;
  }
  void End(int id, hipStream_t s) {
    if (id >= 0) hipEventRecord(recs[id].b, s);
  }
  ~Timer() {
    Reset();
    for (auto e : pool) hipEventDestroy(e);
  }
};

struct Scoped {
  Timer *t; int id; hipStream_t s;
  Scoped(Timer *t_, int kind, hipStream_t s_) : t(t_), id(t_ ? t_->Begin(kind, s_) : -1), s(s_) {}
  ~Scoped() { if (t) t->End(id, s); }
};

// ------------------------------------------------------------------ model

struct DevLinear {
  int K = 0, N = 0, Kpad = 0, Npad = 0;
  size_t wt_off = 0, b_off = 0;    // float offsets into the blob (f16x3: wt_off = interleaved
                                   // (hi, lo) rows [Npad][2 Kpad] halves)
};

struct Workspace;   // the buffers of pk_mi355_nnet_propagate (capi_exec.hip)

// A one-utterance scorer the model owns and remakes, at least doubled, when a call does not fit (capi_batch.hip: EnsureOwned)
struct OwnedBatch { pk_mi355_batch *b = nullptr; int64_t cap = 0; };

}  // namespace pkhost

struct pk_mi355_am {
  int device = 0;
  std::vector<pkhost::HostLayer> layers;
  bool finalized = false;
  int precision = PK_MI355_PRECISION_F32;
  bool softmax_reference = false;  // PK_MI355_SOFTMAX_REFERENCE: the reference's softmax operations one by one
  int left = 0, right = 0, num_pdfs = 0;
  int input_dim = 0, output_dim = 0, feat_dim = 0;
  int max_dim_pad = 0;             // widest activation, rounded to the tile
  int time_left = 0, time_right = 0;   // Lh, Rh: what the time-splice layers (kind 9) consume together (0, 0: none)
  std::vector<int32_t> tid2pdf;
  int32_t *d_tid2pdf = nullptr;    // device copy for the on-GPU gather
  std::vector<pkhost::DevLinear> lin;      // one per linear layer, in order
  float *d_blob = nullptr;
  size_t blob_floats = 0;
  size_t logprior_off = 0;
  std::vector<size_t> vec_off;     // by layer index: where an add / mul layer's vector lies in the blob (float offset; others 0);
                                   // a time-splice layer's offsets lie there likewise, as int32 words
  // f16x3 / f16: the operand exponents, int32 words INSIDE the blob (so the one broadcast carries them):
  // [w_exp of linear layer 0 .. n-1 | x_exp of the operand of linear layer 0 .. n-1 | 0].  The kernels read the
  // device words; h_exps mirrors them on the host (refreshed from the device after a broadcast).
  size_t exp_off = 0;
  std::vector<int32_t> h_exps;
  bool exps_stale = false;
  double flops_per_frame = 0;
  pkhost::ModelKnobs knobs;        // the environment switches as they stood when the model was created
  // The reference's pk_decodable_init / AcousticModel::Compute allocate per call and are re-entrant
  // for a shared model (nnet.cc:149-163 is const); here the single-utterance entry points share
  // device buffers the model owns, so they serialise on this mutex instead.  Under mu:
  std::mutex mu;
  pkhost::Workspace *ws = nullptr; // pk_mi355_nnet_propagate's buffers (plain, unspliced input)
  pkhost::OwnedBatch proc;         // pk_mi355_process_acoustic's scorer: audio, cap in samples, made for proc_stats
  pkhost::OwnedBatch single;       // pk_decodable_init's and pk_mi355_am_calibrate's: features only, cap in frames
  float proc_stats[41] = {0};
};

namespace pkhost {

// Time-splice models.  ContextPad: the columns of Yt an utterance takes beyond its frames (the
// first layer's context and the virtual frames the time-splice layers consume).  HaloLeft / HaloRight: the rows a pass of
// the layer stack runs in front of and behind the rows it owns, Lh and Rh rounded up to the four rows the first layer's
// operand and its column shifts are grouped by.  ExecRows: the rows one pass's layer buffers hold for passes of `chunk`.
inline bool HasTimeSplice(const pk_mi355_am *am) { return am->time_left + am->time_right > 0; }
inline int ContextPad(const pk_mi355_am *am) { return am->left + am->right + am->time_left + am->time_right; }
inline int HaloLeft(const pk_mi355_am *am) { return (int)RoundUp(am->time_left, 4); }
inline int HaloRight(const pk_mi355_am *am) { return (int)RoundUp(am->time_right, 4); }
inline int64_t ExecRows(const pk_mi355_am *am, int64_t chunk) {
  return HasTimeSplice(am) ? RoundUp(chunk + HaloLeft(am) + HaloRight(am), kTile) : chunk;
}

// host mirror of the exponent words <- device (after a broadcast, or a write through the blob's device pointer); and back
int RefreshExps(pk_mi355_am *am);
int UploadExps(pk_mi355_am *am);

// ------------------------------------------------------------------ layer executor (capi_exec.hip)

// Activation buffers for one chunk of at most `rows_cap` frames.
struct ExecBufs {
  float *in = nullptr;    // plain (non-spliced) feature-major input, [Kpad0][rows_cap]
  float *a = nullptr;     // ping
  float *b = nullptr;     // pong
  int64_t rows_cap = 0;
  int64_t in_floats = 0, act_floats = 0;
  // f16x3 mode: interleaved (hi, lo) activation rows [rows_cap][2 max Npad], ping/pong; the
  // plain input rows [rows_cap][2 Kpad0]; `a` holds the fp32 logits, `b` softmax probabilities
  _Float16 *h[2] = {nullptr, nullptr};
  _Float16 *xin = nullptr;
  // f16x3 / f16: range words of the operand of every linear layer ([num linear][kRangeSlots], gemm_f16.hip:
  // PublishRange) and their page-locked host mirror, read after the call (EvalRange)
  uint32_t *range = nullptr, *h_range = nullptr;
  int range_words = 0;
  unsigned *row_done = nullptr;   // fused tail (gemm.hip, TAIL variant): one arrival counter per 128-row tile,
  size_t row_done_bytes = 0;      // zeroed in front of every fused-tail launch
};

int AllocExec(const pk_mi355_am *am, int64_t rows_cap, ExecBufs *e);
void FreeExec(ExecBufs *e);

// ---- f16x3 / f16 operand exponents and range words
inline const int32_t *ExpBase(const pk_mi355_am *am) { return reinterpret_cast<const int32_t *>(am->d_blob + am->exp_off); }
inline const int32_t *ExpW(const pk_mi355_am *am, int l) { return ExpBase(am) + l; }
inline const int32_t *ExpX(const pk_mi355_am *am, int l) { return ExpBase(am) + am->lin.size() + l; }
inline const int32_t *ExpZero(const pk_mi355_am *am) { return ExpBase(am) + 2 * am->lin.size(); }
inline uint32_t *RangeOf(const ExecBufs &e, int l) { return e.range ? e.range + (size_t)l * kRangeSlots : nullptr; }

constexpr int kMaxXExp = 30;                     // |operand exponent| (|w_exp| <= 60: 2^(e_out - e_in - e_w) stays a normal float)
constexpr float kRangeSaturated = 65504.0f;      // the split clamps here (pk_f16_layout.h: Split)
constexpr float kRangeTooSmall = 0.03125f;       // 2^-5: below this every lo half of the operand is an fp16 subnormal
                                                 // (|lo| <= 2^-12 |x|), and the mode degrades towards plain fp16

int BeginRange(const ExecBufs &e, hipStream_t s);
int CollectRange(const ExecBufs &e, hipStream_t s);
void ClearHostRange(const ExecBufs &e);          // a lane that took no part in a call must not contribute stale maxima
int EvalRange(const pk_mi355_am *am, const ExecBufs *const *bufs, int nbufs);
void FreeWorkspace(Workspace *w);
int ResizeHostMatrix(pk_matrix_t *m, int nrow, int ncol);

// ------------------------------------------------------------------ result arenas and views (capi_batch.hip)

struct ArenaRec;
struct alignas(64) ViewGen {
  pk_mi355_am_t *am;     // what Untag() resolves a view's handle to
  ArenaRec *arena;       // valid while `current`
  int live;              // views of this generation not yet destroyed
  bool current;          // the batch's latest fetch_all
  bool withheld;         // f16 modes: the views were handed out (sync == 0) before the score call's range verdict, and the
                         // verdict was PK_MI355_E_RANGE: pk_decodable_loglikelihood on them returns NaN
  unsigned serial;       // 0..31, part of the handle
};
inline bool IsView(const pk_mi355_am_t *am) { return (reinterpret_cast<uintptr_t>(am) & 1u) != 0; }
inline ViewGen *GenOf(const pk_mi355_am_t *am) { return reinterpret_cast<ViewGen *>(reinterpret_cast<uintptr_t>(am) & ~uintptr_t(63)); }
// the model behind a decodable's handle (lock-free: a live view keeps its generation alive)
inline pk_mi355_am_t *Untag(pk_mi355_am_t *am) { return IsView(am) ? GenOf(am)->am : am; }
void ReleaseArenaView(pk_mi355_am_t *handle);

// what the batch decoder (capi_decoder.hip) needs to know of a batch beyond the ABI
bool BatchScored(const pk_mi355_batch *b);
const pk_mi355_am *BatchModel(const pk_mi355_batch *b);

// what the online decoder (capi_online_decoder.hip) needs to know of an online scorer (capi_stream.hip) beyond the ABI
const pk_mi355_am *StreamModel(const pk_mi355_stream *s);
int StreamSlots(const pk_mi355_stream *s);
hipStream_t StreamHipStream(const pk_mi355_stream *s);
const float *StreamLoglikBase(const pk_mi355_stream *s);
bool StreamSlotFlushed(const pk_mi355_stream *s, int slot);   // the last step flushed the slot (it was closed)

// what the online recognizer (capi_online_recognizer.hip) needs to know of an online decoder beyond the ABI
bool OnlineDecoderSlotOpen(const pk_mi355_online_decoder *o, int slot);
// the words of the slot's committed prefix as the decoder keeps them (they only grow until the slot ends or is opened
// again; null for a slot out of range), and the words of the tail that follows them
const std::vector<int> *OnlineDecoderCommittedWords(const pk_mi355_online_decoder *o, int slot);
void OnlineDecoderTailWords(const pk_mi355_online_decoder *o, int slot, std::vector<int> *words);

// ------------------------------------------------------------------ pk_load's host half (capi_recognizer.hip)
// What both recognizers read before the device is touched, in pk_load's order (pocketkaldi.cc:81-131): the graph, the
// AcousticModel keys (checked, read again by pk_mi355_load), the symbol table, and every olabel against its size.
struct RecognizerFiles {
  pk_mi355_fst_t *fst = nullptr;
  pk_mi355_symtab_t *symtab = nullptr;
};
// on failure the caller still frees *out.  any_stats: a cmvn_stats vector of any length up to kMaxCmvnStats (the spec'd loads)
int LoadRecognizerFiles(const char *config_path, RecognizerFiles *out, bool any_stats = false);
constexpr int kMaxCmvnStats = 129;   // the widest front-end spec (128 features) and the count
// pk_mi355_load_stats with the statistics at feat_dim / blocks (capi_io.hip; blocks = 1: that entry; blocks = 0: at any
// length -- a transform stands in front of the model and pk_mi355_transform_batch_create holds them to its base dimension)
int LoadStatsBlocks(const char *config_path, int precision, int blocks, pk_mi355_am_t **am_out, float *stats, int stats_cap, int *stats_len);
void FreeRecognizerFiles(RecognizerFiles *f);
// The words' strings joined by one space (pocketkaldi.cc:232-238); PK_MI355_E_INVALID for a word without a name.
int JoinWords(const pk_mi355_symtab_t *symtab, const int *words, int count, std::string *text);

}  // namespace pkhost

#endif  // PK_HOST_H_
