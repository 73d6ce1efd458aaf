// stream_transform_plan_test.cc -- the transform rows of the online scorer's stage plan (csrc/pk_plan.cc; DESIGN.md, "The
// two plans" and section 26) in a process of its own: no HIP, no library, no Python.  Built plain and with
// -fsanitize=address,undefined by tests/test_cpp_stream_transforms.py, which holds the expected lines, written out from
// the table and not by calling this code.
//
//   stream_transform_plan_test
//
// Prints one line per cell: deltas x global matrix x slot matrices, each over a features-only transform object (no row
// area, no audio: n_front = 0) over mode x n_back in {0, 2} x chain_pushed in {0, 3}, then one with a front-end (a row
// area at every base dimension) over mode x n_front, n_back in {0, 2} x max_m x chain_pushed in {0, 3}.
#include <stdio.h>

#include <initializer_list>

#include "../../pocketkaldi_amd/csrc/pk_plan.h"

using namespace pkplan;

static const char *kModeNames[] = {"sliding", "none", "utterance", "speaker", "online"};     // PK_MI355_NORM_*, kNormOnlineCmvn

static void Print(bool deltas, bool global, bool slots, bool row_area, int mode, int n_front, int n_back, int max_m, int chain_pushed) {
  const StreamPlan p = PlanStream(row_area, mode, StepCounts{n_front, n_back, n_front, max_m, 0, chain_pushed}, deltas, true, global, slots);
  printf("stream transform deltas=%d global=%d slots=%d area=%d %s front=%d back=%d m=%d chain=%d: front=%d", deltas, global, slots, row_area,
         kModeNames[mode], n_front, n_back, max_m, chain_pushed, p.front);
  for (int k = 0; k < p.n; ++k) {
    const Block &b = p.block[k];
    printf(" [%s x%d %s%s %s%s%s%s %s]", b.back ? "back" : "first", b.count, b.step_rows ? "d_rows" : "d_upload", b.raw_rows ? " RawRows" : "",
           b.norm == kStreamNorm ? "StreamNorm" : b.norm == kStreamCmvnChain ? "StreamCmvnChain" : "-", b.delta ? " StreamDelta" : "",
           b.transform ? " StreamTransform" : "", b.slot_transform ? " SlotTransform" : "", b.fused ? "StreamCmvn" : "StreamFeatureLayout");
  }
  printf("\n");
}

int main() {
  static_assert(PK_MI355_NORM_SLIDING == 0 && PK_MI355_NORM_NONE == 1 && PK_MI355_NORM_UTTERANCE == 2 && PK_MI355_NORM_SPEAKER == 3 &&
                pknorm::kNormOnlineCmvn == 4, "kModeNames");
  for (int deltas = 0; deltas < 2; ++deltas)
    for (int global = 0; global < 2; ++global)
      for (int slots = 0; slots < 2; ++slots) {
        for (int mode = 0; mode < 5; ++mode)
          for (int n_back : {0, 2})
            for (int chain_pushed : {0, 3}) Print(deltas, global, slots, false, mode, 0, n_back, 0, chain_pushed);
        for (int mode = 0; mode < 5; ++mode)
          for (int n_front : {0, 2})
            for (int n_back : {0, 2})
              for (int max_m : {0, 3}) {
                if (n_front == 0 && max_m != 0) continue;      // (max_m counts audio frames)
                for (int chain_pushed : {0, 3}) Print(deltas, global, slots, true, mode, n_front, n_back, max_m, chain_pushed);
              }
      }
  // an object made by any other entry: the defaulted parameters change nothing
  const StepCounts k{2, 2, 1, 3, 1, 3};
  for (int mode = 0; mode < 5; ++mode)
    for (int area = 0; area < 2; ++area)
      for (int deltas = 0; deltas < 2; ++deltas) {
        const StreamPlan a = PlanStream(area != 0, mode, k, deltas != 0), b = PlanStream(area != 0, mode, k, deltas != 0, false, true, true);
        bool same = a.front == b.front && a.n == b.n;
        for (int i = 0; same && i < a.n; ++i) {
          const Block &x = a.block[i], &y = b.block[i];
          same = x.back == y.back && x.count == y.count && x.step_rows == y.step_rows && x.raw_rows == y.raw_rows && x.norm == y.norm &&
                 x.fused == y.fused && x.delta == y.delta && !x.transform && !y.transform && !x.slot_transform && !y.slot_transform;
        }
        if (!same) { printf("stream_transform_plan_test FAILED: mode %d area %d deltas %d\n", mode, area, deltas); return 1; }
      }
  printf("stream_transform_plan_test ok\n");
  return 0;
}
