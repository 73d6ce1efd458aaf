// stream_transform_test.cc -- feature transforms on a live slot, host side (csrc/pk_transform.h / pk_transform.cc,
// DESIGN.md section 26) in a process of its own: no HIP, no library, no Python.  Built plain and with
// -fsanitize=address,undefined by tests/test_cpp_stream_transforms.py.
//
//   stream_transform_test
//
//   * pkxf::StreamTransformAdvance over nin in [0, 3 C + R + 2], open and closed, against the rule written out here: an
//     open slot holds Rt input frames and R transform frames back, a closed one nothing; counts never go backwards.
//   * pkxf::StreamTransformPick: fresh rows from nin_old on, ring entries f mod C below, inside [0, C); the C frames below
//     nin_old take C different entries.
//   * pkxf::StreamTransformHost (what StreamTransformKernel does for one slot, with a ring of exactly C frames) against
//     pk_mi355_transform_apply on the whole matrix, bit for bit: specs (in_dim, Lt, Rt, rows) (1,0,0,1), (13,3,3,40),
//     (40,0,4,40), (5,5,0,7), (3,8,8,65), affine and linear in turn, and one without a matrix; T in {0, 1, 2, Rt, Rt + 1, C,
//     C + 1, 2C, 2C + 1, 70}, pushed whole, 1 and 7 frames a push and in seeded random pushes with empty ones, closed with
//     the last push and afterwards.  Every buffer is allocated at exactly its size.
#include <stdio.h>
#include <string.h>

#include <set>
#include <vector>

#include "../../pocketkaldi_amd/csrc/pk_transform.h"

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

static void TestAdvance(int Rt, int R) {
  const int top = 3 * (Rt + 4) + R + 2;
  for (int closed = 0; closed < 2; ++closed)
    for (int nin = 0; nin <= top; ++nin)
      for (int nx = 0; nx <= (nin - Rt > 0 ? nin - Rt : 0); ++nx)
        for (int a = 0; a <= (nx - R > 0 ? nx - R : 0); ++a) {
          const pkxf::StreamTransformCounts c = pkxf::StreamTransformAdvance(nin, nx, a, Rt, R, closed != 0);
          if (closed) {
            CHECK(c.nx1 == nin && c.b == nin);
          } else {
            CHECK(c.nx1 == (nin - Rt > nx ? nin - Rt : nx));
            CHECK(c.b == (c.nx1 - R > a ? c.nx1 - R : a));
            CHECK(c.nx1 + Rt <= (nin > nx + Rt ? nin : nx + Rt));              // t + Rt <= nin - 1 for every new frame t < nx1
            CHECK(nin - c.b <= Rt + R || c.b == a);                             // the look-ahead is Rt + R frames
          }
          CHECK(c.nx1 >= nx && c.b >= a && c.b <= c.nx1 && c.nx1 <= nin);
        }
  // a slot's life, one frame a step: rows appear Rt + R frames late and all of them by the flush
  int nin = 0, nx = 0, a = 0;
  for (; nin < top;) {
    ++nin;
    const pkxf::StreamTransformCounts c = pkxf::StreamTransformAdvance(nin, nx, a, Rt, R, false);
    CHECK(c.b == (nin - Rt - R > 0 ? nin - Rt - R : 0));
    nx = c.nx1; a = c.b;
  }
  const pkxf::StreamTransformCounts c = pkxf::StreamTransformAdvance(nin, nx, a, Rt, R, true);
  CHECK(c.b - a == Rt + R && c.nx1 == nin);
  const pkxf::StreamTransformCounts none = pkxf::StreamTransformAdvance(0, 0, 0, Rt, R, true);
  CHECK(none.nx1 == 0 && none.b == 0);
}

static void TestPick(int C) {
  for (int nin_old = 0; nin_old <= 5 * C + 3; ++nin_old)
    for (int f = (nin_old - C > 0 ? nin_old - C : 0); f < nin_old + 3; ++f) {
      if (C == 0 && f < nin_old) continue;             // (never asked: there is no ring)
      const pkxf::StreamTransformSource s = pkxf::StreamTransformPick(f, nin_old, C);
      CHECK(s.fresh == (f >= nin_old));
      CHECK(s.fresh ? s.row == f - nin_old : (s.row == f % C && s.row >= 0 && s.row < C));
    }
  for (int nin_old = C; C > 0 && nin_old <= 3 * C; ++nin_old) {
    std::set<int> seen;
    for (int f = nin_old - C; f < nin_old; ++f) seen.insert(pkxf::StreamTransformPick(f, nin_old, C).row);
    CHECK((int)seen.size() == C);
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

// rows == 0: a spec without a matrix (Lt = Rt = 0)
static void TestStream(int Dp, int Lt, int Rt, int rows, bool affine, int T, int chunking, int close_delay) {
  const int K = (Lt + Rt + 1) * Dp, cols = rows ? K + (affine ? 1 : 0) : 0, out_dim = rows ? rows : Dp;
  std::vector<float> m((size_t)rows * cols);
  for (size_t i = 0; i < m.size(); ++i) m[i] = ((float)(Next() % 20001) - 10000.0f) / 65536.0f;
  const pk_mi355_transform_spec_t spec{Lt, Rt, Dp, rows, cols, rows ? m.data() : nullptr};
  CHECK(pk_mi355_transform_check(&spec) == 0);
  std::vector<float> x((size_t)T * Dp), want((size_t)T * out_dim), got;
  for (size_t i = 0; i < x.size(); ++i) x[i] = ((float)(Next() % 200001) - 100000.0f) / 64.0f;
  if (T > 0) x[(size_t)(T / 2) * Dp] = -0.0f;
  CHECK(pk_mi355_transform_apply(&spec, x.data(), T, want.data()) == 0);
  std::vector<int> chunks = Chunks(T, chunking);
  if (chunks.empty()) chunks.push_back(0);
  for (int k = 0; k < close_delay; ++k) chunks.push_back(0);
  pkxf::StreamTransformHost live(spec);
  int pos = 0, made_total = 0;
  for (size_t k = 0; k < chunks.size(); ++k) {
    const int c = chunks[k];
    const bool closed = k + 1 == chunks.size();
    std::vector<float> fresh(x.begin() + (size_t)pos * Dp, x.begin() + (size_t)(pos + c) * Dp);      // exactly the push
    std::vector<float> out((size_t)(c + Rt) * out_dim);
    const int made = live.Push(fresh.data(), c, closed, out.data());
    CHECK(made >= 0 && made <= c + Rt);
    if (!closed) CHECK(live.final_frames() == (live.frames() - Rt > 0 ? live.frames() - Rt : 0));
    got.insert(got.end(), out.begin(), out.begin() + (size_t)made * out_dim);
    pos += c; made_total += made;
  }
  CHECK(pos == T && made_total == T && live.frames() == T && live.final_frames() == T);
  CHECK(got.size() == want.size() && (got.empty() || memcmp(got.data(), want.data(), sizeof(float) * got.size()) == 0));
}

int main() {
  const int specs[6][4] = {{1, 0, 0, 1}, {13, 3, 3, 40}, {40, 0, 4, 40}, {5, 5, 0, 7}, {3, 8, 8, 65}, {6, 0, 0, 0}};
  int index = 0;
  for (const auto &s : specs) {
    const int Lt = s[1], Rt = s[2], C = Lt + Rt;
    for (int R : {0, 1, 5}) TestAdvance(Rt, R);
    TestPick(C);
    const std::set<int> lengths = {0, 1, 2, Rt, Rt + 1, C, C + 1, 2 * C, 2 * C + 1, 70};
    int cases = 0;
    for (int T : lengths)
      for (int chunking = 0; chunking < 4; ++chunking)
        for (int close_delay = 0; close_delay < 3; ++close_delay) {
          TestStream(s[0], Lt, Rt, s[3], index % 2 == 0, T, chunking, close_delay);
          ++cases;
        }
    printf("stream transform %d (%d,%d) -> %d: %d cases\n", s[0], Lt, Rt, s[3], cases);
    ++index;
  }
  if (g_failures) { printf("stream_transform_test FAILED (%d)\n", g_failures); return 1; }
  printf("stream_transform_test ok\n");
  return 0;
}
