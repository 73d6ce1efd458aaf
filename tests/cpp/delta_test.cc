// delta_test.cc -- the host side of delta features (csrc/pk_delta.cc) in a process of its own: no
// HIP, no library, no Python.  Built plain and with -fsanitize=address,undefined by tests/test_cpp_deltas.py, which
// restates the matrix below in numpy and compares the hashes this program prints.
//
//   delta_test
//
// Cases: every refusal of the spec and of the entries' arguments; the edges of the spec's ranges (order 1 and 3, window 1
// and 8: the largest table fills its buffer exactly); T = 0 and T = 1; the scale tables and the rule on a [T][97] matrix
// for every spec of the tests and T in {0, 1, 2, 37, 130}, hashed.
// Matrix entry i: ((h(i + 99) >> 12) / 1024 - 300) as float, with h(k) = k * 2654435761 mod 2^32.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../pocketkaldi_amd/csrc/pk_delta.h"
#include "../../pocketkaldi_amd/csrc/pk_files.h"

using pkhost::LastError;

static int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failures; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static bool Has(const char *text, const std::string &what) { return std::string(text).find(what) != std::string::npos; }
static uint32_t H(uint32_t k) { return k * 2654435761u; }

static unsigned long long Fnv(const void *data, size_t bytes) {
  unsigned long long h = 14695981039346656037ull;
  const unsigned char *p = static_cast<const unsigned char *>(data);
  for (size_t i = 0; i < bytes; ++i) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

int main() {
  // ---- the spec
  struct { pk_mi355_deltas_spec_t s; const char *word; } bad[] = {{{0, 2}, "order"}, {{4, 2}, "order"}, {{-1, 2}, "order"},
                                                                  {{2, 0}, "window"}, {{2, 9}, "window"}, {{2, -2}, "window"}};
  float scratch[pkdelta::kMaxTable];
  for (auto &b : bad) {
    const int rc = pk_mi355_deltas_check(&b.s);
    CHECK(rc == PK_MI355_E_INVALID && Has(LastError(), "deltas spec:") && Has(LastError(), b.word), "spec {%d, %d}: %d (%s)", b.s.order, b.s.window, rc, LastError());
    CHECK(pk_mi355_deltas_dim(&b.s, 13) == PK_MI355_E_INVALID, "dim of a bad spec");
    CHECK(pk_mi355_deltas_scales(&b.s, scratch) == PK_MI355_E_INVALID, "scales of a bad spec");
    CHECK(pk_mi355_deltas_apply(&b.s, scratch, 1, 1, scratch) == PK_MI355_E_INVALID, "apply of a bad spec");
  }
  CHECK(pk_mi355_deltas_check(nullptr) == PK_MI355_E_INVALID, "null spec");
  for (int order = 1; order <= 3; ++order)
    for (int window : {1, 8}) {
      pk_mi355_deltas_spec_t g = {order, window};
      CHECK(pk_mi355_deltas_check(&g) == 0 && pk_mi355_deltas_dim(&g, 13) == 13 * (order + 1), "spec {%d, %d}: %s", order, window, LastError());
    }
  pk_mi355_deltas_spec_t usual = {2, 2}, widest = {3, 8};
  CHECK(pk_mi355_deltas_dim(&usual, 0) == PK_MI355_E_INVALID && pk_mi355_deltas_dim(&usual, -3) == PK_MI355_E_INVALID, "base dimension 0");
  CHECK(pk_mi355_deltas_dim(&usual, 0x7fffffff / 2) == PK_MI355_E_INVALID, "a dimension that overflows");
  CHECK(pk_mi355_deltas_scales(&usual, nullptr) == PK_MI355_E_INVALID, "null table");
  {   // the widest table fills a buffer of exactly its size
    std::vector<float> exact((size_t)(widest.order + 1) * pkdelta::RowLen(widest), -7.0f);
    CHECK(exact.size() == (size_t)pkdelta::kMaxTable && pk_mi355_deltas_scales(&widest, exact.data()) == 0, "widest table");
    CHECK(exact[pkdelta::Reach(widest)] == 1.0f && exact[0] == 0.0f && exact.back() != 0.0f, "widest table: centre %g, last %g", exact[24], exact.back());
  }

  // ---- no frames, one frame
  {
    const int dim = 5;
    float x[dim] = {1.5f, -0.0f, 3.0f, -2.25f, 1e30f}, y[3 * dim];
    for (float &v : y) v = -7.0f;
    CHECK(pk_mi355_deltas_apply(&usual, nullptr, 0, dim, nullptr) == 0, "no frames: %s", LastError());
    CHECK(pk_mi355_deltas_apply(&usual, x, 0, dim, y) == 0 && y[0] == -7.0f, "no frames writes nothing");
    CHECK(pk_mi355_deltas_apply(&usual, x, 1, dim, y) == 0, "one frame: %s", LastError());
    for (int d = 0; d < dim; ++d) CHECK(y[d] == x[d], "one frame, block 0, column %d: %g", d, y[d]);
    CHECK(signbit(x[1]) && !signbit(y[1]), "-0.0 leaves block 0 as +0.0");
    // every tap reads the one frame, and a block's scales sum to zero: the differences cancel within rounding
    for (int d = 0; d < dim; ++d)
      CHECK(fabsf(y[dim + d]) <= 1e-6f * fabsf(x[d]) && fabsf(y[2 * dim + d]) <= 1e-6f * fabsf(x[d]), "one frame, column %d: %g %g", d, y[dim + d], y[2 * dim + d]);
    CHECK(pk_mi355_deltas_apply(&usual, nullptr, 1, dim, y) == PK_MI355_E_INVALID && pk_mi355_deltas_apply(&usual, x, 1, dim, nullptr) == PK_MI355_E_INVALID, "null rows");
    CHECK(pk_mi355_deltas_apply(&usual, x, -1, dim, y) == PK_MI355_E_INVALID && pk_mi355_deltas_apply(&usual, x, 1, 0, y) == PK_MI355_E_INVALID, "bad shape");
  }

  // ---- the tables and the rule, hashed
  const int D = 97;
  const int specs[5][2] = {{1, 1}, {2, 2}, {3, 1}, {2, 5}, {3, 8}};
  for (auto &s : specs) {
    pk_mi355_deltas_spec_t spec = {s[0], s[1]};
    std::vector<float> table((size_t)(spec.order + 1) * pkdelta::RowLen(spec));
    CHECK(pk_mi355_deltas_scales(&spec, table.data()) == 0, "%s", LastError());
    printf("scales %d %d %016llx\n", spec.order, spec.window, Fnv(table.data(), sizeof(float) * table.size()));
    for (int T : {0, 1, 2, 37, 130}) {
      // exactly sized buffers: a read or a write past either end is the sanitizer's to report
      std::vector<float> x((size_t)T * D), y((size_t)T * D * (spec.order + 1));
      for (size_t i = 0; i < x.size(); ++i) x[i] = (float)((double)(H((uint32_t)i + 99u) >> 12) / 1024.0 - 300.0);
      CHECK(pk_mi355_deltas_apply(&spec, x.data(), T, D, y.data()) == 0, "%s", LastError());
      printf("deltas %d %d %d %016llx\n", spec.order, spec.window, T, Fnv(y.data(), sizeof(float) * y.size()));
    }
  }

  if (g_failures) { printf("delta_test FAILED (%d)\n", g_failures); return 1; }
  printf("delta_test ok\n");
  return 0;
}
