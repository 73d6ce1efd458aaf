// plan_test.cc -- the stage plans of the batch and the online scorer (csrc/pk_plan.cc; DESIGN.md, "The two plans") in a
// process of its own: no HIP, no library, no Python.  Built plain and with -fsanitize=address,undefined by
// tests/test_cpp_plan.py, which holds the expected lines, written out from the table and not by calling this code.
//
//   plan_test
//
// Prints one line per cell of the cross products: the batch plan over source x front-end spec x deltas x Db in {40, 13}
// x mode x speaker records handed over (an object with statistics; then SLIDING without them: no plan), and the stream
// plan over row area x mode x n_front, n_back in {0, 2} x max_m, raw_pushed, chain_pushed in {0, 3}.
#include <stdio.h>

#include <initializer_list>

#include "../../pocketkaldi_amd/csrc/pk_plan.h"

using namespace pkplan;

static const char *kModeNames[] = {"sliding", "none", "utterance", "speaker", "online"};     // PK_MI355_NORM_*, kNormOnlineCmvn
static const char *kSourceNames[] = {"nothing", "waves", "raw", "normalized"};
static const char *kStageNames[] = {"Fbank", "FbankAny", "Cmvn", "CmvnChain", "Norm", "OnlineCmvn", "Delta", "FeatureLayout"};

static const char *RowsName(Rows r) {
  switch (r) {
    case kRawRows: return "d_raw";
    case kFeatRows: return "d_feats";
    case kDeltaRows: return "d_delta";
    case kCallerRows: return "feats";
    case kYt: return "Yt";
    default: return "-";
  }
}

static void PrintBatch(const BatchShape &o, Source source, int mode, bool spk) {
  const BatchPlan p = PlanBatch(o, source, mode, spk);
  printf("batch %s spec=%d deltas=%d Db=%d D=%d stats=%d %s spk=%d:", kSourceNames[source], o.spec, o.deltas, o.Db, o.D, o.stats, kModeNames[mode], spk);
  for (int k = 0; k < p.n; ++k) {
    const Step &st = p.step[k];
    printf(" %s%s(%s->%s@%d)", k < p.front ? "front:" : "", kStageNames[st.stage], RowsName(st.in), RowsName(st.out), st.dim);
  }
  printf(" | speaker=%d stats=%d buffers=%u\n", p.speaker, p.writes_stats, p.buffers);
}

int main() {
  static_assert(PK_MI355_NORM_SLIDING == 0 && PK_MI355_NORM_NONE == 1 && PK_MI355_NORM_UTTERANCE == 2 && PK_MI355_NORM_SPEAKER == 3 &&
                pknorm::kNormOnlineCmvn == 4, "kModeNames");
  const Source sources[] = {kWaves, kRaw, kNormalized};
  for (Source source : sources)
    for (int spec = 1; spec >= 0; --spec)
      for (int deltas = 1; deltas >= 0; --deltas)
        for (int Db : {40, 13})
          for (int mode = 0; mode < 5; ++mode)
            for (int spk = 1; spk >= 0; --spk)
              PrintBatch(BatchShape{Db, deltas ? 3 * Db : Db, spec != 0, deltas != 0, true}, source, mode, spk != 0);
  for (Source source : sources)
    for (int Db : {40, 13}) PrintBatch(BatchShape{Db, Db, false, false, false}, source, PK_MI355_NORM_SLIDING, false);
  PrintBatch(BatchShape{40, 40, false, false, true}, kNoSource, PK_MI355_NORM_NONE, false);
  for (int row_area = 0; row_area < 2; ++row_area)
    for (int mode = 0; mode < 5; ++mode)
      for (int n_front : {0, 2})
        for (int n_back : {0, 2})
          for (int max_m : {0, 3})
            for (int raw_pushed : {0, 3})
              for (int chain_pushed : {0, 3}) {
                const StreamPlan p = PlanStream(row_area != 0, mode, StepCounts{n_front, n_back, n_front, max_m, raw_pushed, chain_pushed});
                printf("stream area=%d %s front=%d back=%d m=%d raw=%d chain=%d: front=%d", row_area, kModeNames[mode], n_front, n_back, max_m,
                       raw_pushed, chain_pushed, p.front);
                for (int k = 0; k < p.n; ++k) {
                  const Block &b = p.block[k];
                  printf(" [%s x%d %s%s %s %s]", b.back ? "back" : "first", b.count, b.step_rows ? "d_rows" : "d_upload", b.raw_rows ? " RawRows" : "",
                         b.norm == kStreamNorm ? "StreamNorm" : b.norm == kStreamCmvnChain ? "StreamCmvnChain" : "-", b.fused ? "StreamCmvn" : "StreamFeatureLayout");
                }
                printf("\n");
              }
  printf("plan_test ok\n");
  return 0;
}
