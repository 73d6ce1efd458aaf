// online_cmvn_test.cc -- online CMVN's host side (csrc/pk_norm.cc) in a process of its own: no HIP,
// no library, no Python.  Built plain and with -fsanitize=address,undefined by tests/test_cpp_online_cmvn.py, which
// restates the inputs below in numpy and compares the hashes this program prints.
//
//   online_cmvn_test
//
// Cases: every refusal of the spec; global counts of 0, -1, NaN and inf (refused); speaker counts of -1, NaN and inf
// (refused, the utterance named) and of 0 (no speaker prior: the bits of a call without a record); W = 1; windows that
// wrap many times (T = 37 at W = 1, 2, 8), one that never fills (W = 50) and T = W; no frames.  Every buffer has exactly
// the size the entry may touch, so the sanitizers see a read of frame t - W before the matrix or a write past it.
// x[i] = (h(i + 99) >> 12) / 1024 - 300; record entry i: S0 = n ((h(i + s) >> 8) / 65536 - 128), S1 = n (m m + 0.01 +
// (h(i + s + 7777) >> 16) / 4096) with h(k) = k * 2654435761 mod 2^32, s = 5000 (global, n = 300) or 9000 (speaker, n = 37).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <string>
#include <vector>

#include "../../pocketkaldi_amd/csrc/pk_files.h"
#include "../../pocketkaldi_amd/csrc/pk_norm.h"

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

static std::vector<double> Record(int D, uint32_t seed, double n) {
  std::vector<double> s(2 * ((size_t)D + 1), 0.0);
  for (int d = 0; d < D; ++d) {
    const double m = (double)(H(d + seed) >> 8) / 65536.0 - 128.0, v = 0.01 + (double)(H(d + seed + 7777u) >> 16) / 4096.0;
    s[d] = m * n;
    s[D + 1 + d] = (m * m + v) * n;
  }
  s[D] = n;
  return s;
}

int main() {
  const int D = 5, T = 37;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const std::vector<double> glob = Record(D, 5000u, 300.0), spk = Record(D, 9000u, 37.0);

  // ---- the spec
  struct { pk_mi355_online_cmvn_spec_t s; const char *word; } bad[] = {
      {{0, 3, 2, 0}, "cmn_window"}, {{-1, 3, 2, 0}, "cmn_window"}, {{6001, 3, 2, 0}, "cmn_window"}, {{8, -1, 2, 0}, "speaker_frames"},
      {{8, 3, -1, 0}, "global_frames"}, {{8, 3, 2, 2}, "norm_vars"}, {{8, 3, 2, -1}, "norm_vars"}};
  for (auto &b : bad) {
    const int rc = pk_mi355_online_cmvn_check(&b.s, glob.data(), D);
    CHECK(rc == PK_MI355_E_INVALID && Has(LastError(), b.word), "spec {%d, %d, %d, %d}: %d (%s)", b.s.cmn_window, b.s.speaker_frames,
          b.s.global_frames, b.s.norm_vars, rc, LastError());
  }
  CHECK(pk_mi355_online_cmvn_check(nullptr, glob.data(), D) == PK_MI355_E_INVALID, "null spec");
  pk_mi355_online_cmvn_spec_t good[] = {{1, 0, 0, 0}, {6000, 0, 1, 1}, {600, 600, 200, 0}, {8, 3, 2, 1}};
  for (auto &g : good) CHECK(pk_mi355_online_cmvn_check(&g, glob.data(), D) == 0, "spec {%d, ...}: %s", g.cmn_window, LastError());
  pk_mi355_online_cmvn_spec_t with_glob = {8, 3, 2, 1}, without_glob = {8, 3, 0, 1};
  CHECK(pk_mi355_online_cmvn_check(&with_glob, nullptr, D) == PK_MI355_E_INVALID && Has(LastError(), "global_frames"), "no global record: %s", LastError());
  CHECK(pk_mi355_online_cmvn_check(&without_glob, nullptr, D) == 0, "global_frames 0 needs no record: %s", LastError());

  std::vector<float> x((size_t)T * D), y(x.size());
  for (size_t i = 0; i < x.size(); ++i) x[i] = (float)((double)(H((uint32_t)i + 99u) >> 12) / 1024.0 - 300.0);
  printf("matrix %016llx\n", Fnv(x.data(), sizeof(float) * x.size()));
  printf("records %016llx %016llx\n", Fnv(glob.data(), sizeof(double) * glob.size()), Fnv(spk.data(), sizeof(double) * spk.size()));

  // ---- counts that are no counts
  for (double c : {0.0, -1.0, nan, inf, -inf}) {
    std::vector<double> g = glob;
    g[D] = c;
    int rc = pk_mi355_online_cmvn_check(&with_glob, g.data(), D);
    CHECK(rc == PK_MI355_E_INVALID && Has(LastError(), "count") && Has(LastError(), "global_frames"), "global count %g: %d (%s)", c, rc, LastError());
    CHECK(pk_mi355_online_cmvn_check(&without_glob, g.data(), D) == 0, "global count %g is not read with global_frames 0", c);
    std::fill(y.begin(), y.end(), -7.0f);
    rc = pk_mi355_online_cmvn_apply(&with_glob, x.data(), T, D, g.data(), nullptr, y.data(), nullptr);
    CHECK(rc == PK_MI355_E_INVALID && y[0] == -7.0f && y.back() == -7.0f, "global count %g: apply %d", c, rc);
  }
  for (double c : {-1.0, nan, inf, -inf}) {
    std::vector<double> s = spk;
    s[D] = c;
    std::fill(y.begin(), y.end(), -7.0f);
    const int rc = pk_mi355_online_cmvn_apply(&with_glob, x.data(), T, D, glob.data(), s.data(), y.data(), nullptr);
    CHECK(rc == PK_MI355_E_INVALID && Has(LastError(), "utterance 0") && Has(LastError(), "count") && y[0] == -7.0f, "speaker count %g: %d (%s)", c, rc, LastError());
    CHECK(pknorm::CheckOnlineSpeakerCounts(s.data(), 1, D) == PK_MI355_E_INVALID, "speaker count %g", c);
  }
  {
    std::vector<double> s = spk;
    s[D] = 0.0;                                                                     // no speaker prior
    std::vector<float> y2(x.size());
    CHECK(pknorm::CheckOnlineSpeakerCounts(s.data(), 1, D) == 0, "speaker count 0: %s", LastError());
    CHECK(pk_mi355_online_cmvn_apply(&with_glob, x.data(), T, D, glob.data(), s.data(), y.data(), nullptr) == 0, "%s", LastError());
    CHECK(pk_mi355_online_cmvn_apply(&with_glob, x.data(), T, D, glob.data(), nullptr, y2.data(), nullptr) == 0, "%s", LastError());
    CHECK(memcmp(y.data(), y2.data(), sizeof(float) * y.size()) == 0, "a speaker count of 0 is not `no record`");
  }
  CHECK(pknorm::CheckOnlineSpeakerCounts(nullptr, 1, D) == PK_MI355_E_INVALID, "null records");
  CHECK(pknorm::CheckOnlineSpeakerCounts(nullptr, 0, D) == 0, "no utterances");

  // ---- the rule: windows that wrap, one that never fills, T = W, with and without variance, with and without the speaker
  for (int W : {1, 2, 8, 37, 50})
    for (int vars : {0, 1})
      for (int speaker : {0, 1}) {
        pk_mi355_online_cmvn_spec_t s = {W, 3, 2, vars};
        std::vector<double> state(2 * (D + 1), -1.0);
        CHECK(pk_mi355_online_cmvn_apply(&s, x.data(), T, D, glob.data(), speaker ? spk.data() : nullptr, y.data(), state.data()) == 0, "%s", LastError());
        CHECK(state[D] == (double)T && state[2 * D + 1] == 0.0, "W = %d: the state's count %g", W, state[D]);
        printf("rule %d %d %d %016llx %016llx\n", W, vars, speaker, Fnv(y.data(), sizeof(float) * y.size()), Fnv(state.data(), sizeof(double) * state.size()));
      }
  {                                                                                   // W = 1 without priors: every frame is its own mean
    pk_mi355_online_cmvn_spec_t s = {1, 0, 0, 0};
    std::vector<double> state(2 * (D + 1), -1.0);
    CHECK(pk_mi355_online_cmvn_apply(&s, x.data(), T, D, nullptr, nullptr, y.data(), state.data()) == 0, "%s", LastError());
    bool zeros = true;
    for (float v : y) zeros = zeros && v == 0.0f;
    CHECK(zeros, "W = 1: a frame minus itself is not 0");
    for (int d = 0; d < D; ++d) CHECK(state[d] == (double)x[(size_t)(T - 1) * D + d], "W = 1: the window holds the last frame (column %d)", d);
    // no frames: nothing is read or written, the state is zero
    CHECK(pk_mi355_online_cmvn_apply(&s, nullptr, 0, D, nullptr, nullptr, nullptr, state.data()) == 0 && state[0] == 0.0 && state[D] == 0.0, "no frames");
    CHECK(pk_mi355_online_cmvn_apply(&s, nullptr, 0, D, nullptr, nullptr, nullptr, nullptr) == 0, "no frames, no state");
    CHECK(pk_mi355_online_cmvn_apply(&s, nullptr, 1, D, nullptr, nullptr, y.data(), nullptr) == PK_MI355_E_INVALID, "null x");
    CHECK(pk_mi355_online_cmvn_apply(&s, x.data(), 1, 0, nullptr, nullptr, y.data(), nullptr) == PK_MI355_E_INVALID, "dim 0");
  }

  if (g_failures) { printf("online_cmvn_test FAILED (%d)\n", g_failures); return 1; }
  printf("online_cmvn_test ok\n");
  return 0;
}
