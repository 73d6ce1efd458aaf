// pk_layers.h -- the layer kinds beyond the reference's four: add, mul, sigmoid, tanh and the
// 2-norm of groups (p-norm, p = 2).  Each rule is stated here once and compiled by pk_layers.cc (g++: the host rule,
// pk_mi355_layer_apply_host, and tests/cpp/layers_test.cc) and by layers.hip (the kernels).  Plain C++ unless hipcc
// compiles it; the launchers at the end exist for hipcc only.  Kept out of pk_kernels.h: that header is part of the hash
// that ties the GEMM profiles to the GEMM's sources.  Internal, like pk_host.h.
// Below them the time-splice layer, kind 9: its limits, its host rule and its launcher (time_splice.hip).
//
// The definitions are the project's.  They follow Kaldi's CPU code as recalled (MatrixBase::Sigmoid, MatrixBase::Tanh,
// VectorBase::Norm(2.0)), whose double literals promote the arithmetic; they have not been compared with a Kaldi binary.
// Every operation is IEEE, none is fused (-ffp-contract=off on both compilers), E is float expf.
#ifndef PK_LAYERS_H_
#define PK_LAYERS_H_

#include <stdint.h>

#include "../../include/pk_mi355.h"

#if defined(__HIPCC__)
#define PK_LAYERS_HD __host__ __device__
#else
#define PK_LAYERS_HD
#endif

namespace pklayers {

inline bool IsVectorKind(int kind) { return kind == PK_NNET_ADD_LAYER || kind == PK_NNET_MUL_LAYER; }
inline bool IsPlainKind(int kind) { return kind == PK_MI355_NNET_SIGMOID_LAYER || kind == PK_MI355_NNET_TANH_LAYER; }

// Both branches of sigmoid and tanh exponentiate -|x| (x itself when x > 0 is false: a NaN stays a NaN), so E is
// called once, in front of the branch.
PK_LAYERS_HD inline float ExpArgument(float x) { return x > 0.0f ? -x : x; }

// sigmoid, e = E(ExpArgument(x)):   x > 0: 1.0 / (1.0 + e)      otherwise: e / (e + 1.0)
// in double, rounded to float once.  The two denominators are one value (IEEE addition commutes), so one division
// serves both branches.
PK_LAYERS_HD inline float SigmoidOf(float x, float e) {
  const double ed = (double)e;
  const double num = x > 0.0f ? 1.0 : ed;
  const double y = num / (1.0 + ed);
  return (float)y;
}

// tanh, t = E(ExpArgument(x)), q = t * t in float:   x > 0: -1.0 + 2.0 / (1.0 + q)      otherwise: 1.0 - 2.0 / (1.0 + q)
// in double, rounded to float once.  (NaN: x > 0 is false, the second branch keeps it NaN.)
PK_LAYERS_HD inline float TanhOf(float x, float t) {
  const float q = t * t;
  const double r = 2.0 / (1.0 + (double)q);
  const double y = x > 0.0f ? -1.0 + r : 1.0 - r;
  return (float)y;
}

// p-norm: s = 0, s = s + x * x over the group in ascending order (float), then the correctly rounded float square
// root.  It is taken in double and rounded once more: for a float argument that is the correctly rounded float root
// (53 >= 2 * 24 + 2 bits), on any compiler setting of the float one.  An overflowed sum gives inf (Kaldi's rescaling
// fallback for an overflowed or zero sum is not restated).
PK_LAYERS_HD inline float PnormAdd(float s, float x) {
  const float p = x * x;
  return s + p;
}
PK_LAYERS_HD inline float PnormRoot(float s) { return (float)__builtin_sqrt((double)s); }

PK_LAYERS_HD inline float AddOf(float x, float v) { return x + v; }
PK_LAYERS_HD inline float MulOf(float x, float v) { return x * v; }

// ------------------------------------------------------------------ host (pk_layers.cc)

// what pk_mi355_am_add_vector_layer and pk_mi355_am_add_pnorm refuse, in their words
int CheckVectorLayer(int kind, int dim, const float *v);
int CheckPnorm(int in_dim, int out_dim);
// the rule for rows [rows][in_dim] -> [rows][out_dim] (arguments checked by the caller)
void ApplyHost(int kind, const float *x, int rows, int in_dim, const float *param, int out_dim, float *out);

// ------------------------------------------------------------------ the time-splice layer, kind 9
// y[t][c in_dim + d] = x[t + o_c][d] for strictly ascending offsets o_0 < ... < o_{n-1}: a copy, every bit kept.
constexpr int kMaxTimeOffsets = 16;      // n
constexpr int kMaxTimeOffset = 32;       // |o_c|
constexpr int kMaxTimeContext = 128;     // Lh + Rh of a network
// what one layer consumes on the left and on the right
inline int TimeLo(const int32_t *offsets, int n) { return n > 0 && offsets[0] < 0 ? -offsets[0] : 0; }
inline int TimeHi(const int32_t *offsets, int n) { return n > 0 && offsets[n - 1] > 0 ? offsets[n - 1] : 0; }
// what pk_mi355_am_add_time_splice refuses, in its words
int CheckTimeSplice(int in_dim, const int32_t *offsets, int n);
// the shrinking rule for rows [rows][in_dim] -> [rows - lo - hi][n in_dim] (arguments checked by the caller)
void TimeSpliceHost(const float *x, int rows, int in_dim, const int32_t *offsets, int n, float *out);

}  // namespace pklayers

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace pkmi {

// `frames` vectors of `dim` features, element (f, d) at x[f * stride_f + d * stride_d], exactly one stride being 1:
// feature-major panels (stride_f == 1, stride_d = ld) or frame-major rows (stride_d == 1, stride_f = ld).

// add / mul (v: dim floats on the device), sigmoid / tanh (v ignored), in place.  Only the dim real features are
// touched: a panel's padding rows behind them stay what the layer in front left there.
void LaunchLayerElementwise(int kind, float *x, int frames, int dim, int64_t stride_f, int64_t stride_d, const float *v,
                            hipStream_t stream);

// p-norm of groups of in_dim / out_dim consecutive features, never in place; `out` in the layout of `x` with its own
// ld.  Panels: rows [out_dim, out_pad) of `out` are written as zeros (the next GEMM reads its K rounded up to kBK panel
// rows against zero weights, and 0 * NaN is NaN: what an earlier call left there must not survive).
void LaunchPnorm(const float *x, int frames, int in_dim, int out_dim, int64_t stride_f, int64_t stride_d, float *out,
                 int64_t out_ld, int out_pad, hipStream_t stream);

// The time-splice layer on feature-major panels (time_splice.hip), never in place: panel row c in_dim + d, column j of
// `out` is x[d][clamp(j + o_c, 0, rows - 1)] for j < rows (the clamp only keeps the read inside the pass's buffer: no
// clamped column reaches a valid output row).  offsets_dev: the n offsets on the device.  Rows [n in_dim, out_pad) of
// `out` are written as zeros, for PnormPanelKernel's reason.
void LaunchTimeSplice(const float *x, int64_t ld, int rows, int in_dim, const int32_t *offsets_dev, int n, float *out,
                      int64_t out_ld, int out_pad, hipStream_t stream);

}  // namespace pkmi
#endif

#endif  // PK_LAYERS_H_
