// stream_delta_test.cc -- delta features on a live slot, host side (csrc/pk_delta.h / pk_delta.cc)
// in a process of its own: no HIP, no library, no Python.  Built plain and with -fsanitize=address,undefined by
// tests/test_cpp_stream_deltas.py.
//
//   stream_delta_test
//
//   * pkdelta::StreamDeltaAdvance over n in [0, 3 M + R + 2], open and closed, against the rule written out here: an
//     open slot holds M base frames and R delta frames back, a closed one nothing; counts never go backwards.
//   * pkdelta::StreamDeltaPick: fresh rows from n_old on, ring entries f mod 2 M below, inside [0, 2 M).
//   * pkdelta::StreamDeltaHost (what StreamDeltaKernel does for one slot, with a ring of exactly 2 M frames) against
//     pk_mi355_deltas_apply on the whole matrix, bit for bit: Db = 5, specs (1,1), (2,2), (3,8), T in {0, 1, 2, M, M + 1,
//     2M, 2M + 1, 130}, pushed whole, 1 and 7 frames a push and in seeded random pushes with empty ones, closed with the
//     last push and afterwards.  Every buffer is allocated at exactly its size.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../pocketkaldi_amd/csrc/pk_delta.h"

static int g_failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      ++g_failures;                                                     \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
    }                                                                   \
  } while (0)

static uint32_t g_seed = 12345;
static uint32_t Next() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static void TestAdvance(int M, int R) {
  for (int closed = 0; closed < 2; ++closed)
    for (int n = 0; n <= 3 * M + R + 2; ++n)
      for (int nd = 0; nd <= (n - M > 0 ? n - M : 0); ++nd)
        for (int a = 0; a <= (nd - R > 0 ? nd - R : 0); ++a) {
          const pkdelta::StreamDeltaCounts c = pkdelta::StreamDeltaAdvance(n, nd, a, M, R, closed != 0);
          if (closed) {
            CHECK(c.nd1 == n && c.b == n);
          } else {
            CHECK(c.nd1 == (n - M > nd ? n - M : nd));
            CHECK(c.b == (c.nd1 - R > a ? c.nd1 - R : a));
            CHECK(c.nd1 >= nd && c.nd1 + M <= (n > nd + M ? n : nd + M));      // t + M <= n - 1 for every new frame t < nd1
            CHECK(n - c.b <= M + R || c.b == a);                                // the look-ahead is M + R frames
          }
          CHECK(c.nd1 >= nd && c.b >= a && c.b <= c.nd1 && c.nd1 <= n);
        }
  // a slot's life, one frame a step: rows appear M + R frames late and all of them by the flush
  int n = 0, nd = 0, a = 0;
  for (; n < 3 * M + R + 2;) {
    ++n;
    const pkdelta::StreamDeltaCounts c = pkdelta::StreamDeltaAdvance(n, nd, a, M, R, false);
    CHECK(c.b == (n - M - R > 0 ? n - M - R : 0));
    nd = c.nd1; a = c.b;
  }
  const pkdelta::StreamDeltaCounts c = pkdelta::StreamDeltaAdvance(n, nd, a, M, R, true);
  CHECK(c.b - a == M + R && c.nd1 == n);
}

static void TestPick(int M) {
  for (int n_old = 0; n_old <= 5 * M; ++n_old)
    for (int f = (n_old - 2 * M > 0 ? n_old - 2 * M : 0); f < n_old + 3; ++f) {
      const pkdelta::StreamDeltaSource s = pkdelta::StreamDeltaPick(f, n_old, M);
      CHECK(s.fresh == (f >= n_old));
      CHECK(s.fresh ? s.row == f - n_old : (s.row == f % (2 * M) && s.row >= 0 && s.row < 2 * M));
    }
  // the 2 M frames below n_old take 2 M different entries
  for (int n_old = 2 * M; n_old <= 4 * M; ++n_old) {
    std::vector<int> seen(2 * M, 0);
    for (int f = n_old - 2 * M; f < n_old; ++f) ++seen[pkdelta::StreamDeltaPick(f, n_old, M).row];
    for (int e = 0; e < 2 * M; ++e) CHECK(seen[e] == 1);
  }
}

// chunking: 0 whole, 1 one frame a push, 2 seven, 3 random 1..40 with empty pushes
static std::vector<int> Chunks(int T, int chunking) {
  std::vector<int> out;
  int left = T;
  while (left > 0) {
    int c = chunking == 0 ? left : chunking == 1 ? 1 : chunking == 2 ? 7 : 1 + (int)(Next() % 40);
    if (chunking == 3 && Next() % 10 < 3) out.push_back(0);
    if (c > left) c = left;
    out.push_back(c);
    left -= c;
  }
  return out;
}

static void TestStream(int order, int window, int T, int chunking, int close_delay) {
  const int Db = 5, M = order * window, F = (order + 1) * Db;
  const pk_mi355_deltas_spec_t spec{order, window};
  std::vector<float> x((size_t)T * Db), want((size_t)T * F), got;
  for (size_t i = 0; i < x.size(); ++i) x[i] = ((float)(Next() % 200001) - 100000.0f) / 64.0f;
  if (T > 0) x[(size_t)(T / 2) * Db + 1] = -0.0f;
  CHECK(pk_mi355_deltas_apply(&spec, x.data(), T, Db, want.data()) == 0);
  std::vector<int> chunks = Chunks(T, chunking);
  if (chunks.empty()) chunks.push_back(0);
  for (int k = 0; k < close_delay; ++k) chunks.push_back(0);
  pkdelta::StreamDeltaHost live(spec, Db);
  int pos = 0, rows = 0;
  for (size_t k = 0; k < chunks.size(); ++k) {
    const int m = chunks[k];
    const bool closed = k + 1 == chunks.size();
    std::vector<float> fresh(x.begin() + (size_t)pos * Db, x.begin() + (size_t)(pos + m) * Db);      // exactly the push
    std::vector<float> out((size_t)(m + M) * F);
    const int made = live.Push(fresh.data(), m, closed, out.data());
    CHECK(made >= 0 && made <= m + M);
    if (!closed) CHECK(live.final_frames() == (live.frames() - M > 0 ? live.frames() - M : 0));
    got.insert(got.end(), out.begin(), out.begin() + (size_t)made * F);
    pos += m; rows += made;
  }
  CHECK(pos == T && rows == T && live.frames() == T && live.final_frames() == T);
  CHECK(got.size() == want.size() && (got.empty() || memcmp(got.data(), want.data(), sizeof(float) * got.size()) == 0));
}

int main() {
  const int specs[3][2] = {{1, 1}, {2, 2}, {3, 8}};
  for (const auto &s : specs) {
    const int M = s[0] * s[1];
    for (int R : {0, 1, 5}) TestAdvance(M, R);
    TestPick(M);
    const int lengths[] = {0, 1, 2, M, M + 1, 2 * M, 2 * M + 1, 130};
    int cases = 0;
    for (int T : lengths)
      for (int chunking = 0; chunking < 4; ++chunking)
        for (int close_delay = 0; close_delay < 3; ++close_delay) {
          TestStream(s[0], s[1], T, chunking, close_delay);
          ++cases;
        }
    printf("stream deltas %d %d: %d cases\n", s[0], s[1], cases);
  }
  if (g_failures) { printf("stream_delta_test FAILED (%d)\n", g_failures); return 1; }
  printf("stream_delta_test ok\n");
  return 0;
}
