// norm_test.cc -- the normalisation spec's host side (csrc/pk_norm.cc) in a process of its own: no
// HIP, no library, no Python.  Built plain and with -fsanitize=address,undefined by tests/test_cpp_norm.py, which
// restates the records below in numpy and compares the hashes this program prints.
//
//   norm_test
//
// Cases: every refusal of the spec; speaker records with counts of 0, -1, NaN and inf (refused, the utterance named,
// nothing written); the variance floor; records for 1 and 200 utterances at D = 97 in the three switch pairs; and
// pk_mi355_norm_apply on a small matrix in every mode, no frames included; and the sliding rule's two steps
// (pknorm::SlidingSum, SlidingApply over BuildCmvnTables' scalars), walked frame by frame as the chain kernels walk them,
// on 700 frames at D = 40 and 41, whose hash the driver holds to the oracle.
// Sliding input: x[t][d] = float((h(t D + d + 31337) >> 8) / 2^24 * 30 - 12 (+ 1e4 in column D / 2)), the statistics
// float(2500 (3 (+ 1e4))) per column and the count 2500.
// Record (u, d): k = 1000 u + d, N = 50 + 100 (u % 7), m = (h(k) >> 8) / 65536 - 128, v = 0.01 + (h(k + 7777) >> 16) / 4096,
// S0 = m N, S1 = (m m + v) N, with h(k) = k * 2654435761 mod 2^32.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <string>
#include <vector>

#include "../../pocketkaldi_amd/csrc/pk_files.h"
#include "../../pocketkaldi_amd/csrc/pk_norm.h"
#include "../../pocketkaldi_amd/csrc/pk_tables.h"

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

static std::vector<double> Records(int U, int D) {
  std::vector<double> s((size_t)U * 2 * (D + 1), 0.0);
  for (int u = 0; u < U; ++u) {
    double *s0 = &s[(size_t)u * 2 * (D + 1)], *s1 = s0 + D + 1;
    const double n = 50.0 + 100.0 * (u % 7);
    for (int d = 0; d < D; ++d) {
      const uint32_t k = 1000u * u + d;
      const double m = (double)(H(k) >> 8) / 65536.0 - 128.0, v = 0.01 + (double)(H(k + 7777u) >> 16) / 4096.0;
      s0[d] = m * n;
      s1[d] = (m * m + v) * n;
    }
    s0[D] = n;
  }
  return s;
}

int main() {
  // ---- the spec
  struct { pk_mi355_norm_spec_t s; const char *word; } bad[] = {
      {{4, 1, 0}, "mode"}, {{-1, 1, 0}, "mode"}, {{0, 0, 0}, "norm_means"}, {{0, 1, 1}, "norm_vars"}, {{2, 2, 0}, "norm_means"},
      {{3, 1, -1}, "norm_vars"}, {{2, 0, 0}, "use mode none"}, {{3, 0, 0}, "use mode none"}};
  for (auto &b : bad) {
    const int rc = pk_mi355_norm_check(&b.s);
    CHECK(rc == PK_MI355_E_INVALID && Has(LastError(), b.word), "spec {%d, %d, %d}: %d (%s)", b.s.mode, b.s.norm_means, b.s.norm_vars, rc, LastError());
  }
  CHECK(pk_mi355_norm_check(nullptr) == PK_MI355_E_INVALID, "null spec");
  pk_mi355_norm_spec_t good[] = {{0, 1, 0}, {1, 9, -9}, {2, 1, 0}, {2, 1, 1}, {2, 0, 1}, {3, 1, 0}, {3, 1, 1}, {3, 0, 1}};
  for (auto &g : good) CHECK(pk_mi355_norm_check(&g) == 0, "spec {%d, %d, %d}: %s", g.mode, g.norm_means, g.norm_vars, LastError());

  // ---- counts that are no counts: refused by the utterance's number, nothing written
  const int D = 97;
  const double counts[] = {0.0, -1.0, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(),
                           -std::numeric_limits<double>::infinity()};
  for (double c : counts) {
    std::vector<double> s = Records(5, D);
    s[(size_t)3 * 2 * (D + 1) + D] = c;
    std::vector<float> table((size_t)5 * 2 * D, -7.0f);
    const int rc = pknorm::FinalizeSpeakerStats(s.data(), 5, D, true, true, table.data());
    CHECK(rc == PK_MI355_E_INVALID && Has(LastError(), "utterance 3") && Has(LastError(), "count"), "count %g: %d (%s)", c, rc, LastError());
    bool untouched = true;
    for (float t : table) untouched = untouched && t == -7.0f;
    CHECK(untouched, "count %g: the table was written", c);
  }
  CHECK(pknorm::FinalizeSpeakerStats(nullptr, 1, D, true, true, nullptr) == PK_MI355_E_INVALID, "null records");
  CHECK(pknorm::FinalizeSpeakerStats(nullptr, 0, D, true, true, nullptr) == 0, "no utterances");

  // ---- the variance floor: one frame's record, and a variance that rounds below zero
  {
    double s[2][3] = {{3.5, -1e4, 1.0}, {3.5 * 3.5, 1e8, 0.0}};
    float table[2][2];
    CHECK(pknorm::FinalizeSpeakerStats(&s[0][0], 1, 2, true, true, &table[0][0]) == 0, "%s", LastError());
    CHECK(table[1][0] == 1e10f && table[1][1] == 1e10f, "scales %g %g", table[1][0], table[1][1]);
    CHECK(table[0][0] == (float)-(3.5 * 1e10) && table[0][1] == (float)(1e4 * 1e10), "offsets %g %g", table[0][0], table[0][1]);
    s[1][0] = std::numeric_limits<double>::quiet_NaN();                       // a NaN stays a NaN
    CHECK(pknorm::FinalizeSpeakerStats(&s[0][0], 1, 2, true, true, &table[0][0]) == 0, "%s", LastError());
    CHECK(std::isnan(table[1][0]) && std::isnan(table[0][0]) && table[1][1] == 1e10f, "NaN: %g %g", table[1][0], table[1][1]);
    CHECK(pknorm::FinalizeSpeakerStats(&s[0][0], 1, 2, true, false, &table[0][0]) == 0, "%s", LastError());
    CHECK(table[0][0] == -3.5f && table[1][0] == 1.0f, "means only: %g %g", table[0][0], table[1][0]);
    CHECK(pknorm::FinalizeSpeakerStats(&s[0][0], 1, 2, false, true, &table[0][0]) == 0, "%s", LastError());
    CHECK(table[0][1] == -0.0f && table[1][1] == 1e-4f, "variance only: %g %g", table[0][1], table[1][1]);      // var = 1e8
  }

  // ---- records for 1 and 200 utterances
  for (int U : {1, 200}) {
    const std::vector<double> s = Records(U, D);
    printf("records %d %016llx\n", U, Fnv(s.data(), sizeof(double) * s.size()));
    const bool pairs[3][2] = {{true, false}, {true, true}, {false, true}};
    for (auto &p : pairs) {
      std::vector<float> table((size_t)U * 2 * D);
      CHECK(pknorm::FinalizeSpeakerStats(s.data(), U, D, p[0], p[1], table.data()) == 0, "%d utterances: %s", U, LastError());
      printf("table %d %d %d %016llx\n", U, (int)p[0], (int)p[1], Fnv(table.data(), sizeof(float) * table.size()));
    }
  }

  // ---- the rule on a matrix
  {
    const int T = 37, dim = 5;
    std::vector<float> x((size_t)T * dim), y(x.size());
    for (size_t i = 0; i < x.size(); ++i) x[i] = (float)((double)(H((uint32_t)i + 99u) >> 12) / 1024.0 - 300.0);
    printf("matrix %016llx\n", Fnv(x.data(), sizeof(float) * x.size()));
    std::vector<double> rec(2 * (dim + 1)), unused(rec.size(), -1.0);
    pk_mi355_norm_spec_t utt = {PK_MI355_NORM_UTTERANCE, 1, 1}, spk = {PK_MI355_NORM_SPEAKER, 1, 1}, none = {PK_MI355_NORM_NONE, 0, 0},
                         sliding = {PK_MI355_NORM_SLIDING, 1, 0};
    CHECK(pk_mi355_norm_apply(&utt, x.data(), T, dim, nullptr, y.data(), rec.data()) == 0, "%s", LastError());
    printf("utterance %016llx %016llx\n", Fnv(y.data(), sizeof(float) * y.size()), Fnv(rec.data(), sizeof(double) * rec.size()));
    std::vector<float> y2(x.size());
    CHECK(pk_mi355_norm_apply(&spk, x.data(), T, dim, rec.data(), y2.data(), unused.data()) == 0, "%s", LastError());
    CHECK(memcmp(y.data(), y2.data(), sizeof(float) * y.size()) == 0 && unused[0] == -1.0, "speaker on the utterance's own record differs");
    CHECK(pk_mi355_norm_apply(&none, x.data(), T, dim, nullptr, y2.data(), nullptr) == 0 && memcmp(x.data(), y2.data(), sizeof(float) * x.size()) == 0, "none");
    CHECK(pk_mi355_norm_apply(&sliding, x.data(), T, dim, nullptr, y2.data(), nullptr) == PK_MI355_E_INVALID && Has(LastError(), "sliding"), "sliding");
    CHECK(pk_mi355_norm_apply(&spk, x.data(), T, dim, nullptr, y2.data(), nullptr) == PK_MI355_E_INVALID, "speaker without a record");
    CHECK(pk_mi355_norm_apply(&utt, nullptr, 0, dim, nullptr, nullptr, rec.data()) == 0 && rec[dim] == 0.0 && rec[0] == 0.0, "no frames");
    CHECK(pk_mi355_norm_apply(&utt, x.data(), 1, dim, nullptr, y2.data(), rec.data()) == 0 && rec[dim] == 1.0, "one frame");
    for (int d = 0; d < dim; ++d) CHECK(y2[d] == x[d] * 1e10f + (float)-((double)x[d] * 1e10), "one frame, column %d: %g", d, y2[d]);
  }

  // ---- the sliding rule, frame by frame
  for (int dim : {40, 41}) {
    const int T = 700, W = pkmi::kCmvnWindow;
    pkmi::CmvnTables tab;
    pkmi::BuildCmvnTables(2500.0f, &tab);
    std::vector<float> x((size_t)T * dim), y(x.size()), g(dim);
    for (int d = 0; d < dim; ++d) {
      const double big = d == dim / 2 ? 1e4 : 0.0;
      g[d] = (float)(2500.0 * (3.0 + big));
      for (int t = 0; t < T; ++t) x[(size_t)t * dim + d] = (float)((double)(H((uint32_t)(t * dim + d) + 31337u) >> 8) / 16777216.0 * 30.0 - 12.0 + big);
    }
    for (int d = 0; d < dim; ++d) {
      float s = 0.0f;
      for (int t = 0; t < T; ++t) {
        const int tt = t < W ? t : W - 1;
        const float xt = x[(size_t)t * dim + d];
        s = pknorm::SlidingSum(s, xt, t >= W ? x[(size_t)(t - W) * dim + d] : 0.0f, t >= W);
        y[(size_t)t * dim + d] = pknorm::SlidingApply(xt, s, tab.alpha[tt], tab.neg_scale[tt], g[d], t + 1 < W);
      }
    }
    printf("sliding %d %016llx %016llx\n", dim, Fnv(x.data(), sizeof(float) * x.size()), Fnv(y.data(), sizeof(float) * y.size()));
  }

  if (g_failures) { printf("norm_test FAILED (%d)\n", g_failures); return 1; }
  printf("norm_test ok\n");
  return 0;
}
