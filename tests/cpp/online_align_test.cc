// online_align_test.cc -- the path-to-frames rule of the online alignment (PathFrames, csrc/pk_files.cc) in a process
// of its own: no HIP, no library, no Python, so that it builds and runs under the host sanitizers
// (tests/test_online_align_host.py builds it plain and with -fsanitize=address,undefined).
//
//   online_align_test
//
// Every case prints what the function wrote, costs as bit patterns; the Python driver holds the hand-worked
// expectations.  "frames <case> <return> <entries written> | arc tid costbits | ..." and, for the cases whose frames
// feed WordSegments, "segments <case> <n> | word start frames graphbits acousticbits | ...".
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../pocketkaldi_amd/csrc/pk_files.h"

using namespace pkhost;

static int failures = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      printf("FAIL %s:%d: ", __FILE__, __LINE__);          \
      printf(__VA_ARGS__);                                 \
      printf("\n");                                        \
      ++failures;                                          \
    }                                                      \
  } while (0)

static unsigned Bits(float x) {
  unsigned u;
  memcpy(&u, &x, 4);
  return u;
}

// One case: the path's arcs and a cost per ARC (an epsilon arc's must be ignored: they carry a poison value).
static void Frames(const char *name, const ArcLabels &g, const std::vector<int32_t> &path, const std::vector<float> &arc_ac,
                   int expect, int max_frames, bool segments) {
  const int guard = 3;                                      // entries past max_frames must stay untouched
  const int room = (max_frames > 0 ? max_frames : 0) + guard;
  std::vector<int32_t> ids(room, -7), tids(room, -7);
  std::vector<float> ac(room, -7.0f);
  const int n = PathFrames(g, path.data(), arc_ac.data(), (int)path.size(), expect, ids.data(), tids.data(), ac.data(), max_frames);
  const int written = n < 0 ? 0 : (n < max_frames ? n : max_frames);
  printf("frames %s %d %d", name, n, written);
  for (int i = 0; i < written; ++i) printf(" | %d %d %08x", ids[i], tids[i], Bits(ac[i]));
  printf("\n");
  if (n >= 0)
    for (int i = written; i < room; ++i)
      CHECK(ids[i] == -7 && tids[i] == -7 && ac[i] == -7.0f, "%s: entry %d past the %d frames was written", name, i, written);
  if (n < 0) CHECK(strstr(LastError(), "emitting arcs") != nullptr, "%s: message '%s'", name, LastError());
  // null outputs: the count alone
  CHECK(PathFrames(g, path.data(), arc_ac.data(), (int)path.size(), expect, nullptr, nullptr, nullptr, 0) == n, "%s: null outputs", name);
  if (segments && n >= 0 && n <= max_frames) {
    const int count = WordSegments(g, path.data(), (int)path.size(), ac.data(), n, nullptr, 0);
    std::vector<pk_mi355_word_t> seg(count + 1);
    CHECK(WordSegments(g, path.data(), (int)path.size(), ac.data(), n, seg.data(), count) == count, "%s: segments twice", name);
    printf("segments %s %d", name, count);
    for (int i = 0; i < count; ++i)
      printf(" | %d %d %d %08x %08x", seg[i].word, seg[i].start_frame, seg[i].num_frames, Bits(seg[i].graph_cost), Bits(seg[i].acoustic_cost));
    printf("\n");
  }
}

int main() {
  // arcs 0..6 as (ilabel, olabel, weight): the graph of symtab_test.cc
  ArcLabels g;
  g.ilabel = {0, 3, 0, 4, 2, 1, 0};
  g.olabel = {0, 0, 5, 6, 7, 0, 8};
  g.weight = {0.25f, 0.5f, 0.125f, 1.5f, 0.1f, 0.2f, 0.3f};
  const float P = -99.0f;                                   // what an epsilon arc's slot holds: never read
  // epsilon arcs before, between and after the frames
  Frames("eps_between", g, {0, 1, 2, 0, 3, 6, 5, 0}, {P, 1.0f, P, P, 2.5f, P, 0.3f, P}, 3, 8, true);
  // an emitting arc first and last, words on epsilon arcs
  Frames("emitting_ends", g, {3, 2, 6, 5, 4}, {1.0f, P, P, 2.5f, 0.3f}, 3, 3, true);
  // no emitting arc at all; no arc at all
  Frames("no_emitting", g, {0, 2, 6}, {P, P, P}, 0, 4, true);
  Frames("empty", g, {}, {}, 0, 4, true);
  // the count of emitting arcs is not the frames decoded: one too few, one too many
  Frames("mismatch_few", g, {1, 2, 3}, {1.0f, P, 2.5f}, 3, 8, false);
  Frames("mismatch_many", g, {1, 2, 3}, {1.0f, P, 2.5f}, 1, 8, false);
  // max_frames smaller than the path: the count is the path's, the first max_frames are written
  Frames("max_smaller", g, {1, 0, 3, 4, 5}, {1.0f, P, 2.5f, 0.3f, 0.7f}, 4, 2, false);
  Frames("max_zero", g, {1, 3}, {1.0f, 2.5f}, 2, 0, false);
  // an arc id outside the graph counts as an epsilon arc, as WordSegments takes it; +inf and NaN costs pass through
  Frames("outside_and_nonfinite", g, {-1, 1, 7, 3, 5}, {P, __builtin_inff(), P, __builtin_nanf(""), 0.5f}, 3, 8, true);
  if (failures) {
    printf("online_align_test: %d failures\n", failures);
    return 1;
  }
  printf("online_align_test ok\n");
  return 0;
}
