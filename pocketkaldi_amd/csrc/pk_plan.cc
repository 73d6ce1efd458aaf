// pk_plan.cc -- the stage plans of the batch and the online scorer (pk_plan.h; DESIGN.md, "The two plans").
#include "pk_plan.h"

namespace pkplan {

BatchPlan PlanBatch(const BatchShape &o, Source source, int mode, bool speaker_given, bool utt_transforms) {
  BatchPlan p;
  auto add = [&p](Stage stage, Rows in, Rows out, int dim) {
    p.step[p.n++] = Step{stage, in, out, dim};
    p.buffers |= (in | out) & kOwnRows;
  };
  if (source == kNormalized) {                        // the mode is ignored
    add(kFeatureLayout, kCallerRows, kYt, o.D);
    return p;
  }
  if (source == kNoSource || (mode == PK_MI355_NORM_SLIDING && !o.stats)) return p;
  if (source == kWaves) {
    add(o.spec ? kFbankAny : kFbank, kNoRows, kRawRows, o.Db);
    p.front = 1;
  }
  Rows rows = kFeatRows;                              // the normalisation at Db, from d_raw
  switch (mode) {
    case PK_MI355_NORM_NONE: rows = kRawRows; break;
    case pknorm::kNormOnlineCmvn:
      add(kOnlineCmvn, kRawRows, kFeatRows, o.Db);
      p.speaker = speaker_given;
      break;
    case PK_MI355_NORM_UTTERANCE:
    case PK_MI355_NORM_SPEAKER:
      add(kNorm, kRawRows, kFeatRows, o.Db);
      p.writes_stats = mode == PK_MI355_NORM_UTTERANCE;
      break;
    default:                                          // SLIDING
      if (FusedCmvn(o)) {
        add(kCmvn, kRawRows, kYt, o.Db);
        return p;
      }
      add(kCmvnChain, kRawRows, kFeatRows, o.Db);
  }
  if (o.deltas) {
    add(kDelta, rows, kDeltaRows, o.Db);
    rows = kDeltaRows;
  }
  if (o.transform && o.Dp > 0) {                      // the global matrix: rows of Dp features -> rows of D
    add(kTransform, rows, kXformRows, o.Dp);
    rows = kXformRows;
  }
  if (o.transform && utt_transforms) {                // this call's own matrices, D -> D
    add(kUttTransform, rows, kUttXformRows, o.D);
    rows = kUttXformRows;
  }
  add(kFeatureLayout, rows, kYt, o.D);
  return p;
}

StreamPlan PlanStream(bool row_area, int mode, const StepCounts &k, bool deltas, bool transform, bool global_matrix, bool slot_matrices) {
  StreamPlan p;
  const bool staged = deltas || transform;            // the layout reads a staging of the object's own: nothing is fused
  auto stages = [&](Block b) {                        // what stands between a block's normaliser and its layout
    b.delta = deltas;
    b.transform = transform && global_matrix;
    b.slot_transform = transform && slot_matrices;
    return b;
  };
  p.front = k.n_audio > 0;
  const bool sliding = mode == PK_MI355_NORM_SLIDING;
  // what normalises fresh rows outside StreamCmvnKernel's fused path (mode none: nothing)
  const StreamNormaliser norm = sliding ? kStreamCmvnChain : mode == PK_MI355_NORM_NONE ? kNoNormaliser : kStreamNorm;
  if (row_area) {       // audio, RAW and NORMALIZED records in one block, all rows in the staging (NORMALIZED ones return from the normaliser)
    p.block[p.n++] = stages(Block{false, k.n_front + k.n_back, false, false, k.max_m > 0 || k.chain_pushed > 0 ? norm : kNoNormaliser, false});
    return p;
  }
  // (A deltas or transform object has front records only with a row area, above: one with a front-end has a row area at every base
  // dimension, a features-only one has no front records.  pk_mi355_stream_step refuses the cell below with either set --
  // its delta staging lies in the upload staging, which a block of d_rows could not address.)
  if (k.n_front > 0 && sliding && !staged)            // audio and RAW records at 40 dimensions
    p.block[p.n++] = Block{false, k.n_front, true, k.raw_pushed > 0, kNoNormaliser, true};
  else if (k.n_front > 0)                             // a norm spec: audio records alone, laid out from d_rows
    p.block[p.n++] = stages(Block{false, k.n_front, true, false, k.max_m > 0 ? norm : kNoNormaliser, false});
  if (k.n_back > 0)                                   // NORMALIZED records, and the RAW ones normalised where they were pushed
    p.block[p.n++] = stages(Block{true, k.n_back, false, false, k.chain_pushed > 0 ? norm : kNoNormaliser, false});
  return p;
}

}  // namespace pkplan
