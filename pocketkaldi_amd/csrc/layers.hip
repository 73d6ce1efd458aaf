// layers.hip -- the layer kinds 4 to 8 for gfx950 (pk_layers.h): add, mul, sigmoid and tanh in
// place, p-norm into the other work buffer, each in both activation layouts of the fp32 executor (feature-major panels
// between affine layers, frame-major rows behind the last one).  Separate HBM-bound passes: 8 dim bytes per frame for an
// elementwise kind, 4 (G + 1) out_dim for p-norm.  No LDS; the 32-word expf table is read from global memory (256 bytes,
// resident in the scalar / vector caches).
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#include "pk_expf.h"
#include "pk_layers.h"

namespace pkmi {

namespace {

using namespace pklayers;

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ const uint64_t kLayerExpfTab[kExpfTableWords] = PK_EXPF_TABLE_INIT;

constexpr int kLayerThreads = 256;
constexpr int kLayerWaves = kLayerThreads / 64;      // a workgroup: 4 lines (one per wave) x 64 lanes x VEC inner elements
constexpr int kMaxGridY = 32768;

template <int KIND>
__device__ __forceinline__ float ElementRule(float x, float v) {
  if (KIND == PK_NNET_ADD_LAYER) return AddOf(x, v);
  if (KIND == PK_NNET_MUL_LAYER) return MulOf(x, v);
  const float e = ExpfRestatedWave(ExpArgument(x), kLayerExpfTab);
  return KIND == PK_MI355_NNET_SIGMOID_LAYER ? SigmoidOf(x, e) : TanhOf(x, e);
}

// x as [outer][ld] with `inner` real elements per line, the inner axis contiguous.  Panels: outer = feature, inner =
// frame; rows: outer = frame, inner = feature (PARAM_INNER: that is where v is indexed).  A thread owns VEC consecutive
// inner elements -- VEC = 4: one 16-byte load and store, which the launcher picks when x and ld allow it --, a wave 64 of
// those runs of one line, and walks the lines at stride 4 gridDim.y.  A ragged end of a line (rows layout, dim % 4 != 0) is done element by element.
template <int KIND, int VEC, bool PARAM_INNER>
__global__ __launch_bounds__(kLayerThreads) void LayerElementwiseKernel(float *__restrict__ x, int outer, int inner, int64_t ld,
                                                                        const float *__restrict__ v) {
  const int i0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * VEC;
  if (i0 >= inner) return;
  constexpr bool kHasParam = KIND == PK_NNET_ADD_LAYER || KIND == PK_NNET_MUL_LAYER;
  const bool whole = i0 + VEC <= inner;
  float vi[VEC];
#pragma unroll
  for (int c = 0; c < VEC; ++c) vi[c] = (kHasParam && PARAM_INNER && i0 + c < inner) ? v[i0 + c] : 0.0f;
  for (int o = blockIdx.y * kLayerWaves + (threadIdx.x >> 6); o < outer; o += gridDim.y * kLayerWaves) {
    float *p = x + (int64_t)o * ld + i0;
    const float vo = (kHasParam && !PARAM_INNER) ? v[o] : 0.0f;
    if (VEC == 4 && whole) {
      f32x4 t = *reinterpret_cast<const f32x4 *>(p);
#pragma unroll
      for (int c = 0; c < 4; ++c) t[c] = ElementRule<KIND>(t[c], PARAM_INNER ? vi[c] : vo);
      *reinterpret_cast<f32x4 *>(p) = t;
    } else {
      for (int c = 0; c < VEC && i0 + c < inner; ++c) p[c] = ElementRule<KIND>(p[c], PARAM_INNER ? vi[c] : vo);
    }
  }
}

// Panels: x [in_dim][ld_in] -> out [out_pad][ld_out], a thread owns VEC consecutive frames of one output row and walks the
// G rows of its group at stride ld_in, in ascending order; rows [out_dim, out_pad) receive zeros.
template <int VEC>
__global__ __launch_bounds__(kLayerThreads) void PnormPanelKernel(const float *__restrict__ x, int frames, int G, int out_dim, int out_pad,
                                                                  int64_t ld_in, float *__restrict__ out, int64_t ld_out) {
  const int f0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * VEC;
  if (f0 >= frames) return;
  for (int o = blockIdx.y * kLayerWaves + (threadIdx.x >> 6); o < out_pad; o += gridDim.y * kLayerWaves) {
    float s[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) s[c] = 0.0f;
    if (o < out_dim) {
      const float *p = x + (int64_t)o * G * ld_in + f0;
      for (int g = 0; g < G; ++g, p += ld_in) {
        if (VEC == 4) {
          const f32x4 t = *reinterpret_cast<const f32x4 *>(p);
#pragma unroll
          for (int c = 0; c < 4; ++c) s[c] = PnormAdd(s[c], t[c]);
        } else {
          for (int c = 0; c < VEC; ++c)
            if (f0 + c < frames) s[c] = PnormAdd(s[c], p[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < VEC; ++c) s[c] = PnormRoot(s[c]);        // (a zero sum has the root zero)
    }
    float *q = out + (int64_t)o * ld_out + f0;
    if (VEC == 4) {
      f32x4 t;
#pragma unroll
      for (int c = 0; c < 4; ++c) t[c] = s[c];
      *reinterpret_cast<f32x4 *>(q) = t;
    } else {
      for (int c = 0; c < VEC; ++c)
        if (f0 + c < frames) q[c] = s[c];
    }
  }
}

// Rows: x [frames][ld_in] -> out [frames][ld_out], a group is G contiguous floats; one thread per (frame, output).
__global__ __launch_bounds__(kLayerThreads) void PnormRowsKernel(const float *__restrict__ x, int frames, int G, int out_dim, int64_t ld_in,
                                                                 float *__restrict__ out, int64_t ld_out) {
  const int64_t idx = (int64_t)blockIdx.x * kLayerThreads + threadIdx.x;
  if (idx >= (int64_t)frames * out_dim) return;
  const int o = (int)(idx % out_dim);
  const int64_t f = idx / out_dim;
  const float *p = x + f * ld_in + (int64_t)o * G;
  float s = 0.0f;
  for (int g = 0; g < G; ++g) s = PnormAdd(s, p[g]);
  out[f * ld_out + o] = PnormRoot(s);
}

bool Aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <int KIND, bool PARAM_INNER>
void LaunchElementwiseKind(float *x, int outer, int inner, int64_t ld, const float *v, hipStream_t stream) {
  const bool vec = ld % 4 == 0 && Aligned16(x);
  const int per = vec ? 4 : 1;
  const int lines = (outer + kLayerWaves - 1) / kLayerWaves;
  dim3 grid((inner + 64 * per - 1) / (64 * per), lines < kMaxGridY ? lines : kMaxGridY);
  if (vec)
    hipLaunchKernelGGL((LayerElementwiseKernel<KIND, 4, PARAM_INNER>), grid, dim3(kLayerThreads), 0, stream, x, outer, inner, ld, v);
  else
    hipLaunchKernelGGL((LayerElementwiseKernel<KIND, 1, PARAM_INNER>), grid, dim3(kLayerThreads), 0, stream, x, outer, inner, ld, v);
}

template <int KIND>
void LaunchElementwiseLayout(float *x, int frames, int dim, int64_t stride_f, int64_t stride_d, const float *v, hipStream_t stream) {
  if (stride_f == 1) LaunchElementwiseKind<KIND, false>(x, dim, frames, stride_d, v, stream);
  else LaunchElementwiseKind<KIND, true>(x, frames, dim, stride_f, v, stream);
}

}  // namespace

void LaunchLayerElementwise(int kind, float *x, int frames, int dim, int64_t stride_f, int64_t stride_d, const float *v,
                            hipStream_t stream) {
  if (frames <= 0 || dim <= 0) return;
  switch (kind) {
    case PK_NNET_ADD_LAYER: LaunchElementwiseLayout<PK_NNET_ADD_LAYER>(x, frames, dim, stride_f, stride_d, v, stream); break;
    case PK_NNET_MUL_LAYER: LaunchElementwiseLayout<PK_NNET_MUL_LAYER>(x, frames, dim, stride_f, stride_d, v, stream); break;
    case PK_MI355_NNET_SIGMOID_LAYER: LaunchElementwiseLayout<PK_MI355_NNET_SIGMOID_LAYER>(x, frames, dim, stride_f, stride_d, v, stream); break;
    default: LaunchElementwiseLayout<PK_MI355_NNET_TANH_LAYER>(x, frames, dim, stride_f, stride_d, v, stream); break;
  }
}

void LaunchPnorm(const float *x, int frames, int in_dim, int out_dim, int64_t stride_f, int64_t stride_d, float *out,
                 int64_t out_ld, int out_pad, hipStream_t stream) {
  if (frames <= 0 || out_dim <= 0) return;
  const int G = in_dim / out_dim;
  if (stride_f == 1) {
    const bool vec = frames % 4 == 0 && stride_d % 4 == 0 && out_ld % 4 == 0 && Aligned16(x) && Aligned16(out);
    const int per = vec ? 4 : 1;
    const int lines = (out_pad + kLayerWaves - 1) / kLayerWaves;
    dim3 grid((frames + 64 * per - 1) / (64 * per), lines < kMaxGridY ? lines : kMaxGridY);
    if (vec) hipLaunchKernelGGL((PnormPanelKernel<4>), grid, dim3(kLayerThreads), 0, stream, x, frames, G, out_dim, out_pad, stride_d, out, out_ld);
    else hipLaunchKernelGGL((PnormPanelKernel<1>), grid, dim3(kLayerThreads), 0, stream, x, frames, G, out_dim, out_pad, stride_d, out, out_ld);
  } else {
    const int64_t n = (int64_t)frames * out_dim;
    hipLaunchKernelGGL(PnormRowsKernel, dim3((unsigned)((n + kLayerThreads - 1) / kLayerThreads)), dim3(kLayerThreads), 0, stream, x, frames, G,
                       out_dim, stride_f, out, out_ld);
  }
}

}  // namespace pkmi
