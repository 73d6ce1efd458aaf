// transform_plan_test.cc -- the batch plan of a transform object (csrc/pk_plan.cc) in a process of
// its own: no HIP, no library, no Python.  Built plain and with -fsanitize=address,undefined by
// tests/test_cpp_transforms.py, which holds the expected lines, written out from the table and not by calling this code.
//
//   transform_plan_test
//
// Prints one line per cell of source x deltas x global matrix or not x matrices handed over or not x mode, for an object
// with statistics whose base dimension is 13 (with deltas of order 2 the transform reads 39; a global matrix makes 40).
#include <stdio.h>

#include "../../pocketkaldi_amd/csrc/pk_plan.h"

using namespace pkplan;

static const char *kModeNames[] = {"sliding", "none", "utterance", "speaker", "online"};     // PK_MI355_NORM_*, kNormOnlineCmvn
static const char *kSourceNames[] = {"nothing", "waves", "raw", "normalized"};
static const char *kStageNames[] = {"Fbank", "FbankAny", "Cmvn", "CmvnChain", "Norm", "OnlineCmvn", "Delta", "FeatureLayout", "Transform", "UttTransform"};

static const char *RowsName(Rows r) {
  switch (r) {
    case kRawRows: return "d_raw";
    case kFeatRows: return "d_feats";
    case kDeltaRows: return "d_delta";
    case kXformRows: return "d_xform";
    case kUttXformRows: return "d_uxform";
    case kCallerRows: return "feats";
    case kYt: return "Yt";
    default: return "-";
  }
}

int main() {
  static_assert(kTransform == kFeatureLayout + 1 && kUttTransform == kFeatureLayout + 2 && kXformRows == 32 && kUttXformRows == 64, "appended at the end");
  const Source sources[] = {kWaves, kRaw, kNormalized};
  for (Source source : sources)
    for (int deltas = 0; deltas < 2; ++deltas)
      for (int global = 0; global < 2; ++global)
        for (int utt = 0; utt < 2; ++utt)
          for (int mode = 0; mode < 5; ++mode) {
            const int Db = 13, in = deltas ? 39 : 13, D = global ? 40 : in;
            const BatchShape o{Db, D, true, deltas != 0, true, true, global ? in : 0};
            const BatchPlan p = PlanBatch(o, source, mode, false, utt != 0);
            printf("batch %s deltas=%d global=%d utt=%d %s:", kSourceNames[source], deltas, global, utt, kModeNames[mode]);
            for (int k = 0; k < p.n; ++k) {
              const Step &st = p.step[k];
              printf(" %s%s(%s->%s@%d)", k < p.front ? "front:" : "", kStageNames[st.stage], RowsName(st.in), RowsName(st.out), st.dim);
            }
            printf(" | buffers=%u\n", p.buffers);
          }
  // SLIDING at 40 on a transform object is the chain kernel, not the fused one; the same shape without the flag is fused
  printf("fused transform=%d plain=%d\n", FusedCmvn(BatchShape{40, 40, false, false, true, true, 0}), FusedCmvn(BatchShape{40, 40, false, false, true}));
  // an object from any existing entry ignores utt_transforms
  const BatchPlan a = PlanBatch(BatchShape{40, 40, false, false, true}, kRaw, PK_MI355_NORM_UTTERANCE, false, true);
  printf("plain utt=1: %d steps, buffers=%u\n", a.n, a.buffers);
  printf("transform_plan_test ok\n");
  return 0;
}
