// transform_test.cc -- the host side of the feature transforms (csrc/pk_transform.cc) in a process
// of its own: no HIP, no library, no Python.  Built plain and with -fsanitize=address,undefined by
// tests/test_cpp_transforms.py, which restates the matrices below in numpy and compares the hashes this program prints.
//
//   transform_test
//
// Cases: every refusal of the spec and of the entries' arguments; the edges of the spec's ranges; the widest matrix
// (in_dim 512, left + right 16, one row) in a buffer of exactly its size; T = 0 and T = 1; the kernel's matrix layout;
// the rule for every spec of the tests and T in {0, 1, 2, 9, 33}, in exactly sized buffers, hashed.
// Input entry i: ((h(i + 99) >> 12) / 1024 - 300) as float; matrix entry i: ((h(i + 7) >> 12) / 1048576 - 0.5) as float,
// with h(k) = k * 2654435761 mod 2^32.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../pocketkaldi_amd/csrc/pk_files.h"
#include "../../pocketkaldi_amd/csrc/pk_transform.h"

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

static std::vector<float> Matrix(size_t n) {
  std::vector<float> m(n);
  for (size_t i = 0; i < n; ++i) m[i] = (float)((double)(H((uint32_t)i + 7u) >> 12) / 1048576.0 - 0.5);
  return m;
}

int main() {
  // ---- the spec
  const std::vector<float> ones(2049 * 5, 1.0f);
  struct { pk_mi355_transform_spec_t s; const char *word; } bad[] = {
      {{-1, 0, 4, 2, 4, ones.data()}, "left_context"},  {{17, 0, 4, 2, 72, ones.data()}, "left_context"},
      {{0, -1, 4, 2, 4, ones.data()}, "right_context"}, {{0, 17, 4, 2, 72, ones.data()}, "right_context"},
      {{9, 8, 4, 2, 72, ones.data()}, "is above 16"},   {{0, 0, 0, 2, 0, ones.data()}, "in_dim"},
      {{0, 0, 513, 2, 513, ones.data()}, "in_dim"},     {{0, 0, 4, 0, 4, ones.data()}, "rows"},
      {{0, 0, 4, 2049, 4, ones.data()}, "rows"},        {{0, 0, 4, 2, 6, ones.data()}, "cols 6 is neither 4"},
      {{1, 1, 4, 2, 14, ones.data()}, "nor 13"},        {{0, 0, 4, 2, 4, nullptr}, "null matrix"},
      {{1, 0, 4, 0, 0, nullptr}, "null matrix"}};
  float scratch[8] = {0};
  for (auto &b : bad) {
    const int rc = pk_mi355_transform_check(&b.s);
    CHECK(rc == PK_MI355_E_INVALID && Has(LastError(), "transform spec:") && Has(LastError(), b.word), "%s: %d (%s)", b.word, rc, LastError());
    CHECK(pk_mi355_transform_out_dim(&b.s) == PK_MI355_E_INVALID, "out_dim of a bad spec");
    CHECK(pk_mi355_transform_apply(&b.s, scratch, 1, scratch + 4) == PK_MI355_E_INVALID, "apply of a bad spec");
  }
  CHECK(pk_mi355_transform_check(nullptr) == PK_MI355_E_INVALID && Has(LastError(), "null argument"), "null spec");
  {   // the edges of the ranges
    pk_mi355_transform_spec_t edges[] = {{16, 0, 1, 1, 17, ones.data()}, {0, 16, 2, 1, 35, ones.data()}, {0, 0, 512, 1, 512, ones.data()},
                                         {0, 0, 4, 2048, 5, ones.data()}, {0, 0, 1, 1, 1, ones.data()}, {0, 0, 9, 0, 0, nullptr}};
    for (auto &e : edges) CHECK(pk_mi355_transform_check(&e) == 0, "an edge of the ranges: %s", LastError());
    CHECK(pk_mi355_transform_out_dim(&edges[3]) == 2048 && pk_mi355_transform_out_dim(&edges[5]) == 9, "out_dim");
  }
  {   // an entry that is not finite: the first one is named
    std::vector<float> m(3 * 5, 1.0f);
    m[1 * 5 + 4] = NAN; m[2 * 5] = INFINITY;
    pk_mi355_transform_spec_t s = {0, 0, 4, 3, 5, m.data()};
    CHECK(pk_mi355_transform_check(&s) == PK_MI355_E_INVALID && Has(LastError(), "row 1, column 4"), "%s", LastError());
    m[1 * 5 + 4] = 1.0f;
    CHECK(pk_mi355_transform_check(&s) == PK_MI355_E_INVALID && Has(LastError(), "row 2, column 0"), "%s", LastError());
  }
  {   // the widest matrix in a buffer of exactly its size, over inputs and outputs of exactly theirs
    const int Dp = 512, L = 7, R = 9, K = (L + R + 1) * Dp, T = 3;
    std::vector<float> m = Matrix((size_t)K + 1), x((size_t)T * Dp), y(T);
    for (size_t i = 0; i < x.size(); ++i) x[i] = (float)((double)(H((uint32_t)i + 99u) >> 12) / 1024.0 - 300.0);
    pk_mi355_transform_spec_t s = {L, R, Dp, 1, K + 1, m.data()};
    CHECK(pk_mi355_transform_apply(&s, x.data(), T, y.data()) == 0, "widest: %s", LastError());
    printf("widest %016llx\n", Fnv(y.data(), sizeof(float) * y.size()));
    std::vector<float> packed((size_t)(K + 1) * pkxf::Ldo(1));
    pkxf::PackTransposed(m.data(), 1, K + 1, packed.data());
    CHECK(pkxf::Ldo(1) == 64 && packed[0] == m[0] && packed[1] == 0.0f && packed[(size_t)K * 64] == m[K] && packed.back() == 0.0f, "packed layout");
  }
  {   // the kernel's layout: transposed, padded to 64 outputs with zeros
    const int rows = 65, cols = 3;
    std::vector<float> m = Matrix((size_t)rows * cols), packed((size_t)cols * pkxf::Ldo(rows), -7.0f);
    CHECK(pkxf::Ldo(rows) == 128 && pkxf::Ldo(64) == 64 && pkxf::Ldo(63) == 64, "Ldo");
    pkxf::PackTransposed(m.data(), rows, cols, packed.data());
    for (int k = 0; k < cols; ++k)
      for (int o = 0; o < 128; ++o) CHECK(packed[(size_t)k * 128 + o] == (o < rows ? m[(size_t)o * cols + k] : 0.0f), "packed[%d][%d]", k, o);
  }

  // ---- no frames, one frame
  {
    const int Dp = 3;
    const float m[2 * 10] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5f, /* row 1 */ 0, 0, 0, 0, 0, 2, 0, 0, 0, -1};
    pk_mi355_transform_spec_t s = {1, 1, Dp, 2, 10, m};
    float x[Dp] = {1.5f, -0.0f, 3.0f}, y[2] = {-7.0f, -7.0f};
    CHECK(pk_mi355_transform_apply(&s, nullptr, 0, nullptr) == 0, "no frames: %s", LastError());
    CHECK(pk_mi355_transform_apply(&s, x, 0, y) == 0 && y[0] == -7.0f, "no frames writes nothing");
    CHECK(pk_mi355_transform_apply(&s, x, 1, y) == 0, "one frame: %s", LastError());
    CHECK(y[0] == 1.5f + -0.0f + 3.0f + 0.5f && y[1] == 2 * 3.0f - 1, "one frame reads itself in every window slot: %g %g", y[0], y[1]);
    CHECK(pk_mi355_transform_apply(&s, nullptr, 1, y) == PK_MI355_E_INVALID && pk_mi355_transform_apply(&s, x, 1, nullptr) == PK_MI355_E_INVALID, "null rows");
    CHECK(pk_mi355_transform_apply(&s, x, -1, y) == PK_MI355_E_INVALID, "bad shape");
    CHECK(pk_mi355_transform_apply(&s, x, 1, x) == PK_MI355_E_INVALID, "in place");
    const float z[1] = {0.0f};
    pk_mi355_transform_spec_t zero = {0, 0, 1, 1, 1, z};
    float nz = -0.0f, inf = INFINITY, out = -7.0f;
    CHECK(pk_mi355_transform_apply(&zero, &nz, 1, &out) == 0 && out == 0.0f && !signbit(out), "-0.0 does not survive the +0.0f start");
    CHECK(pk_mi355_transform_apply(&zero, &inf, 1, &out) == 0 && isnan(out), "a zero entry times an inf is NaN");
    pk_mi355_transform_spec_t none = {0, 0, Dp, 0, 0, nullptr};
    float c[Dp] = {0};
    CHECK(pk_mi355_transform_apply(&none, x, 1, c) == 0 && memcmp(c, x, sizeof(c)) == 0, "no matrix: a copy");
  }

  // ---- the rule, hashed
  const int specs[6][5] = {{1, 0, 0, 1, 1}, {13, 3, 3, 40, 1}, {40, 4, 4, 40, 0}, {65, 1, 2, 63, 1}, {39, 0, 0, 39, 1}, {512, 8, 8, 3, 0}};
  for (auto &p : specs) {
    const int Dp = p[0], L = p[1], R = p[2], rows = p[3], cols = (L + R + 1) * Dp + p[4];
    const std::vector<float> m = Matrix((size_t)rows * cols);         // exactly sized
    pk_mi355_transform_spec_t spec = {L, R, Dp, rows, cols, m.data()};
    for (int T : {0, 1, 2, 9, 33}) {
      // exactly sized buffers: a read or a write past either end is the sanitizer's to report
      std::vector<float> x((size_t)T * Dp), y((size_t)T * rows);
      for (size_t i = 0; i < x.size(); ++i) x[i] = (float)((double)(H((uint32_t)i + 99u) >> 12) / 1024.0 - 300.0);
      CHECK(pk_mi355_transform_apply(&spec, x.data(), T, y.data()) == 0, "%s", LastError());
      printf("transform %d %d %d %d %d %d %016llx\n", Dp, L, R, rows, p[4], T, Fnv(y.data(), sizeof(float) * y.size()));
    }
  }

  if (g_failures) { printf("transform_test FAILED (%d)\n", g_failures); return 1; }
  printf("transform_test ok\n");
  return 0;
}
