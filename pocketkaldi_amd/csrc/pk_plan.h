// pk_plan.h -- which launches a scorer makes between the audio (or the features handed over) and the splice, as pure
// functions of what the object is and what the call brings ("The two plans").  pk_mi355_batch_score and
// pk_mi355_stream_step execute what these return and decide nothing themselves.  Plain C++: no HIP header; pk_plan.cc is
// compiled by g++ like pk_norm.cc and builds into a stand-alone program (tests/cpp/plan_test.cc).  Internal.
#ifndef PK_PLAN_H_
#define PK_PLAN_H_

#include "pk_norm.h"

namespace pkplan {

// ------------------------------------------------------------------ the batch scorer
enum Source { kNoSource, kWaves, kRaw, kNormalized };      // what the last set call handed over
// (kTransform, kUttTransform: the two stages of a transform object)
enum Stage { kFbank, kFbankAny, kCmvn, kCmvnChain, kNorm, kOnlineCmvn, kDelta, kFeatureLayout, kTransform, kUttTransform };
// Where a stage reads and writes.  kRawRows, kFeatRows, kDeltaRows, kXformRows and kUttXformRows are the batch's own
// buffers (d_raw, d_feats, d_delta, d_xform, d_uxform) and double as the bits of BatchPlan::buffers; kCallerRows: the
// normalised features handed over, where they lie.
enum Rows { kNoRows = 0, kRawRows = 1, kFeatRows = 2, kDeltaRows = 4, kCallerRows = 8, kYt = 16, kXformRows = 32, kUttXformRows = 64 };
constexpr unsigned kOwnRows = kRawRows | kFeatRows | kDeltaRows | kXformRows | kUttXformRows;

// base and model dimension; front-end spec, deltas, CMVN statistics.  transform: an object made by
// pk_mi355_transform_batch_create; Dp: the width of the rows its global matrix reads, 0 when it has none.
struct BatchShape { int Db, D; bool spec, deltas, stats; bool transform = false; int Dp = 0; };
struct Step { Stage stage; Rows in, out; int dim; };
struct BatchPlan {
  int n = 0, front = 0;          // steps, and how many of them (0 or 1, the first) are the front-end
  Step step[6];
  bool speaker = false;          // kOnlineCmvn smooths with the speaker records handed over for this call
  bool writes_stats = false;     // kNorm in mode UTTERANCE leaves every utterance's record behind
  unsigned buffers = 0;          // the own rows the steps read or write
};
// SLIDING at 40 dimensions without deltas: CmvnKernel normalises and writes Yt itself, and reads around every utterance --
// the one plan whose d_raw needs the lead and the slack.
inline bool FusedCmvn(const BatchShape &o) { return o.stats && !o.deltas && !o.transform && o.Db == 40; }
// mode: PK_MI355_NORM_* or pknorm::kNormOnlineCmvn.  Empty for what score refuses in front of the plan (nothing set;
// SLIDING on raw rows or audio without statistics).  utt_transforms: per-utterance matrices were handed over for this
// call (a transform object only).
BatchPlan PlanBatch(const BatchShape &o, Source source, int mode, bool speaker_given, bool utt_transforms = false);

// ------------------------------------------------------------------ the online scorer
enum StreamNormaliser { kNoNormaliser, kStreamNorm, kStreamCmvnChain };
// A run of records that goes through one normaliser and one layout.  back: the records at the array's end (the last
// n_back), else those from record 0.  step_rows: the rows lie in d_rows (the fbank's), else in the upload staging.
// raw_rows: StreamRawRowsKernel first copies the RAW records' pushed rows to d_rows.  fused: StreamCmvnKernel normalises
// and lays out in one launch; else the normaliser (if any), then StreamFeatureLayoutKernel.  delta (a deltas object,
// DESIGN.md section 24): StreamDeltaKernel between the two, and the layout reads the step's second record array.
// transform, slot_transform (a transform object): StreamTransformKernel with the global matrix,
// and once more with the slots' own matrices, behind the deltas; the layout reads the last stage's record array.
struct Block {
  bool back; int count; bool step_rows, raw_rows; StreamNormaliser norm; bool fused; bool delta = false;
  bool transform = false, slot_transform = false;
};
struct StepCounts { int n_front, n_back, n_audio, max_m, raw_pushed, chain_pushed; };
struct StreamPlan {
  bool front = false;            // StreamAssembleKernel and the fbank run over the n_front front records
  int n = 0;
  Block block[2];
};
// row_area: an object with a front-end spec at another dimension than 40, or a deltas object with a front-end, whose
// fresh rows all lie in the upload staging.  deltas: an object made by pk_mi355_deltas_stream_create -- nothing takes the
// fused path (StreamCmvnKernel writes the layout itself, as FusedCmvn on the batch side), SLIDING runs the chain at the
// base dimension, at 40 too, and every block goes normaliser, StreamDeltaKernel, layout.
// transform: an object made by pk_mi355_transform_stream_create -- as deltas: nothing fused, the chain at the base
// dimension, and every block goes normaliser, [StreamDeltaKernel], StreamTransformKernel (global_matrix: the spec has a
// matrix), the per-slot stage (slot_matrices: in this step a record's slot holds a matrix of its own), layout.
StreamPlan PlanStream(bool row_area, int mode, const StepCounts &k, bool deltas = false, bool transform = false, bool global_matrix = false,
                      bool slot_matrices = false);

}  // namespace pkplan

#endif  // PK_PLAN_H_
