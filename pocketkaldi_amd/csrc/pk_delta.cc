// pk_delta.cc -- delta features on the host (pk_delta.h): the check, the scale table and the whole
// rule for one matrix; the streaming apply of a live slot (section 24).  No HIP: g++ builds it, into the library and into
// tests/cpp/delta_test.cc and tests/cpp/stream_delta_test.cc.
#include "pk_delta.h"

#include <vector>

#include "pk_files.h"

namespace pkdelta {

using pkhost::Fail;

int CheckSpec(const pk_mi355_deltas_spec_t *spec) {
  if (!spec) return Fail(PK_MI355_E_INVALID, "null argument");
  if (spec->order < 1 || spec->order > kMaxOrder)
    return Fail(PK_MI355_E_INVALID, "deltas spec: order %d is outside [1, %d]", spec->order, kMaxOrder);
  if (spec->window < 1 || spec->window > kMaxWindow)
    return Fail(PK_MI355_E_INVALID, "deltas spec: window %d is outside [1, %d]", spec->window, kMaxWindow);
  return 0;
}

void BuildScales(const pk_mi355_deltas_spec_t &spec, float *table) {
  const int L = RowLen(spec), C = Reach(spec), W = spec.window;
  for (int i = 0; i < (spec.order + 1) * L; ++i) table[i] = 0.0f;
  table[C] = 1.0f;
  for (int i = 1; i <= spec.order; ++i) {
    const float *prev = table + (i - 1) * L + C;      // both centred: entry k of a row at [k]
    float *cur = table + i * L + C;
    const int po = (i - 1) * W;                       // (len(s[i-1]) - 1) / 2
    float normalizer = 0.0f;
    for (int j = -W; j <= W; ++j) {
      normalizer = normalizer + (float)(j * j);
      for (int k = -po; k <= po; ++k) {
        const float p = (float)j * prev[k];
        cur[j + k] = cur[j + k] + p;
      }
    }
    const float inv = (float)(1.0 / (double)normalizer);
    for (int j = -(po + W); j <= po + W; ++j) cur[j] = cur[j] * inv;
  }
}

StreamDeltaHost::StreamDeltaHost(const pk_mi355_deltas_spec_t &spec, int base_dim) : spec_(spec), Db_(base_dim), M_(Reach(spec)) {
  BuildScales(spec_, table_);
  for (int p = 0; p < 2; ++p) ring_[p] = new float[(size_t)2 * M_ * Db_];
}

StreamDeltaHost::~StreamDeltaHost() {
  for (int p = 0; p < 2; ++p) delete[] ring_[p];
}

int StreamDeltaHost::Push(const float *x, int m, bool closed, float *out) {
  const int n_old = n_, n = n_ + m, L = RowLen(spec_), Db = Db_, M = M_;
  const StreamDeltaCounts c = StreamDeltaAdvance(n, nd_, 0, M, 0, closed);
  const float *old = ring_[par_];
  auto frame = [&](int f) {               // f in [max(n_old - 2 M, 0), n)
    const StreamDeltaSource s = StreamDeltaPick(f, n_old, M);
    return s.fresh ? x + (size_t)s.row * Db : old + (size_t)s.row * Db;
  };
  const size_t F = (size_t)(spec_.order + 1) * Db;
  for (int t = nd_; t < c.nd1; ++t)
    for (int i = 0; i <= spec_.order; ++i)
      for (int d = 0; d < Db; ++d)
        out[(size_t)(t - nd_) * F + (size_t)i * Db + d] = DeltaApply<float>(table_ + i * L + M, i * spec_.window, [&](int j) {
          const int tt = t + j;
          return frame(tt < 0 ? 0 : tt > n - 1 ? n - 1 : tt)[d];
        });
  if (m > 0) {                            // frames [max(n - 2 M, 0), n) to the other buffer, which nothing above reads
    float *next = ring_[par_ ^ 1];
    for (int f = n - 2 * M > 0 ? n - 2 * M : 0; f < n; ++f) {
      const float *src = frame(f);
      for (int d = 0; d < Db; ++d) next[(size_t)(f % (2 * M)) * Db + d] = src[d];
    }
    par_ ^= 1;
  }
  const int made = c.nd1 - nd_;
  n_ = n; nd_ = c.nd1;
  return made;
}

}  // namespace pkdelta

extern "C" {

int pk_mi355_deltas_check(const pk_mi355_deltas_spec_t *spec) { return pkdelta::CheckSpec(spec); }

int pk_mi355_deltas_dim(const pk_mi355_deltas_spec_t *spec, int base_dim) {
  if (int rc = pkdelta::CheckSpec(spec)) return rc;
  if (base_dim <= 0 || base_dim > INT32_MAX / (spec->order + 1))
    return pkhost::Fail(PK_MI355_E_INVALID, "deltas: base dimension %d", base_dim);
  return (spec->order + 1) * base_dim;
}

int pk_mi355_deltas_scales(const pk_mi355_deltas_spec_t *spec, float *table) {
  if (int rc = pkdelta::CheckSpec(spec)) return rc;
  if (!table) return pkhost::Fail(PK_MI355_E_INVALID, "null argument");
  pkdelta::BuildScales(*spec, table);
  return 0;
}

int pk_mi355_deltas_apply(const pk_mi355_deltas_spec_t *spec, const float *x, int num_frames, int base_dim, float *y) {
  using namespace pkdelta;
  if (int rc = CheckSpec(spec)) return rc;
  if (num_frames < 0 || base_dim <= 0) return pkhost::Fail(PK_MI355_E_INVALID, "bad shape (%d frames of %d features)", num_frames, base_dim);
  if (num_frames > 0 && (!x || !y)) return pkhost::Fail(PK_MI355_E_INVALID, "null argument");
  float table[kMaxTable];
  BuildScales(*spec, table);
  const int L = RowLen(*spec), C = Reach(*spec);
  const size_t T = (size_t)num_frames, Db = (size_t)base_dim, F = Db * (size_t)(spec->order + 1);
  for (size_t t = 0; t < T; ++t)
    for (int i = 0; i <= spec->order; ++i)
      for (size_t d = 0; d < Db; ++d)
        y[t * F + (size_t)i * Db + d] = DeltaApply<float>(table + i * L + C, i * spec->window, [&](int j) {
          const int64_t tt = (int64_t)t + j;
          return x[(size_t)(tt < 0 ? 0 : tt >= (int64_t)T ? (int64_t)T - 1 : tt) * Db + d];
        });
  return 0;
}

}  // extern "C"
