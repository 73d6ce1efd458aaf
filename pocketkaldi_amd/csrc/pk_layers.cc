// pk_layers.cc -- the layer kinds 4 to 8 on the host (pk_layers.h): the checks of the two entries
// that take a parameter, and the whole rule for a matrix of rows.  No HIP: g++ builds it, into the library and into
// tests/cpp/layers_test.cc.
// Also the time-splice layer's checks and host rule (kind 9; tests/cpp/time_splice_test.cc).
#include "pk_layers.h"

#include <string.h>

#include <cmath>

#include "pk_expf.h"
#include "pk_files.h"

namespace pklayers {

using pkhost::Fail;

namespace {
const uint64_t kExpfTab[pkmi::kExpfTableWords] = PK_EXPF_TABLE_INIT;
}  // namespace

int CheckVectorLayer(int kind, int dim, const float *v) {
  if (!IsVectorKind(kind)) return Fail(PK_MI355_E_INVALID, "unexpected layer type: %d (a vector layer is kind %d or %d)", kind, PK_NNET_ADD_LAYER, PK_NNET_MUL_LAYER);
  if (dim <= 0 || !v) return Fail(PK_MI355_E_INVALID, "bad vector layer (dim %d)", dim);
  for (int i = 0; i < dim; ++i)
    if (!std::isfinite(v[i])) return Fail(PK_MI355_E_INVALID, "vector layer: entry %d is not finite", i);
  return 0;
}

int CheckPnorm(int in_dim, int out_dim) {
  if (out_dim <= 0 || in_dim <= 0) return Fail(PK_MI355_E_INVALID, "bad p-norm layer (%d -> %d)", in_dim, out_dim);
  if (in_dim % out_dim != 0)
    return Fail(PK_MI355_E_INVALID, "p-norm layer: input width %d is not a multiple of the output width %d", in_dim, out_dim);
  return 0;
}

void ApplyHost(int kind, const float *x, int rows, int in_dim, const float *param, int out_dim, float *out) {
  const size_t R = (size_t)rows, D = (size_t)in_dim, O = (size_t)out_dim;
  if (kind == PK_MI355_NNET_PNORM_LAYER) {
    const size_t G = D / O;
    for (size_t r = 0; r < R; ++r)
      for (size_t o = 0; o < O; ++o) {
        float s = 0.0f;
        for (size_t g = 0; g < G; ++g) s = PnormAdd(s, x[r * D + o * G + g]);
        out[r * O + o] = PnormRoot(s);
      }
    return;
  }
  for (size_t r = 0; r < R; ++r)
    for (size_t d = 0; d < D; ++d) {
      const float v = x[r * D + d];
      float y;
      switch (kind) {
        case PK_NNET_ADD_LAYER: y = AddOf(v, param[d]); break;
        case PK_NNET_MUL_LAYER: y = MulOf(v, param[d]); break;
        case PK_MI355_NNET_SIGMOID_LAYER: y = SigmoidOf(v, pkmi::ExpfRestated(ExpArgument(v), kExpfTab)); break;
        default: y = TanhOf(v, pkmi::ExpfRestated(ExpArgument(v), kExpfTab)); break;
      }
      out[r * D + d] = y;
    }
}

int CheckTimeSplice(int in_dim, const int32_t *offsets, int n) {
  if (in_dim <= 0) return Fail(PK_MI355_E_INVALID, "bad time-splice layer (in_dim %d)", in_dim);
  if (n < 1 || n > kMaxTimeOffsets || !offsets)
    return Fail(PK_MI355_E_INVALID, "time-splice layer: %d offsets, between 1 and %d are allowed", n, kMaxTimeOffsets);
  for (int c = 0; c < n; ++c) {
    if (offsets[c] < -kMaxTimeOffset || offsets[c] > kMaxTimeOffset)
      return Fail(PK_MI355_E_INVALID, "time-splice layer: offset %d (index %d) is outside [-%d, %d]", offsets[c], c, kMaxTimeOffset, kMaxTimeOffset);
    if (c > 0 && offsets[c] <= offsets[c - 1])
      return Fail(PK_MI355_E_INVALID, "time-splice layer: the offsets must ascend strictly, offset %d (index %d) follows %d", offsets[c], c,
                  offsets[c - 1]);
  }
  return 0;
}

void TimeSpliceHost(const float *x, int rows, int in_dim, const int32_t *offsets, int n, float *out) {
  const size_t D = (size_t)in_dim;
  const int lo = TimeLo(offsets, n), hi = TimeHi(offsets, n);
  for (int r = 0; r < rows - lo - hi; ++r)
    for (int c = 0; c < n; ++c)
      memcpy(out + ((size_t)r * n + c) * D, x + (size_t)(r + lo + offsets[c]) * D, sizeof(float) * D);   // (bits, not values)
}

}  // namespace pklayers

extern "C" {

int pk_mi355_time_splice_host(const float *x, int rows, int in_dim, const int32_t *offsets, int n, float *out) {
  using namespace pklayers;
  if (int rc = CheckTimeSplice(in_dim, offsets, n)) return rc;
  const int lo = TimeLo(offsets, n), hi = TimeHi(offsets, n);
  if (rows <= lo + hi)
    return pkhost::Fail(PK_MI355_E_INVALID, "time splice: %d rows, the offsets consume %d on the left and %d on the right", rows, lo, hi);
  if (!x || !out) return pkhost::Fail(PK_MI355_E_INVALID, "null argument");
  TimeSpliceHost(x, rows, in_dim, offsets, n, out);
  return 0;
}

int pk_mi355_layer_apply_host(int kind, const float *x, int rows, int in_dim, const float *param, int out_dim, float *out) {
  using namespace pklayers;
  if (kind < PK_NNET_ADD_LAYER || kind > PK_MI355_NNET_PNORM_LAYER) return pkhost::Fail(PK_MI355_E_INVALID, "unexpected layer type: %d", kind);
  if (rows < 0 || in_dim <= 0) return pkhost::Fail(PK_MI355_E_INVALID, "bad shape (%d rows of %d features)", rows, in_dim);
  if (kind == PK_MI355_NNET_PNORM_LAYER) {
    if (int rc = CheckPnorm(in_dim, out_dim)) return rc;
  } else if (out_dim != in_dim) {
    return pkhost::Fail(PK_MI355_E_INVALID, "layer kind %d keeps the width: %d in, %d out", kind, in_dim, out_dim);
  }
  if (IsVectorKind(kind))
    if (int rc = CheckVectorLayer(kind, in_dim, param)) return rc;
  if (rows > 0 && (!x || !out)) return pkhost::Fail(PK_MI355_E_INVALID, "null argument");
  ApplyHost(kind, x, rows, in_dim, param, out_dim, out);
  return 0;
}

}  // extern "C"
