// time_splice.hip -- the time-splice layer, kind 9, for gfx950 (pk_layers.h): between two affine
// layers of the fp32 executor the activations are feature-major panels [dim][ld] with the frames contiguous, and the layer
// is n in_dim row copies, each shifted by its offset.  One HBM-bound pass, 4 in_dim bytes read and 4 n in_dim written per
// frame (the n shifted reads of a row meet in L2).  No LDS, no scratch.
#include <hip/hip_runtime.h>

#include "pk_layers.h"

namespace pkmi {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kSpliceThreads = 256;
constexpr int kSpliceWaves = kSpliceThreads / 64;      // a workgroup: 4 output rows (one per wave) x 64 lanes x VEC frames
constexpr int kMaxGridY = 32768;

// x [in_dim][ld] -> out [out_pad][out_ld].  A thread owns VEC consecutive frames j0 .. of one output row -- VEC = 4: one
// 16-byte store, which the launcher picks when `out` and out_ld allow it --, a wave 64 of those runs (256 frames), and
// walks the output rows at stride 4 gridDim.y.  Output row o = c in_dim + d reads row d at columns j + o_c: the source is
// only dword-aligned (o_c mod 4 floats off), so it is read dword by dword; where a thread's four columns would leave
// [0, rows) each is clamped on its own.  Rows [out_dim, out_pad) receive zeros.
template <int VEC>
__global__ __launch_bounds__(kSpliceThreads) void TimeSpliceKernel(const float *__restrict__ x, int64_t ld, int rows, int in_dim,
                                                                   const int32_t *__restrict__ offsets, int out_dim, int out_pad,
                                                                   float *__restrict__ out, int64_t out_ld) {
  const int j0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * VEC;
  if (j0 >= rows) return;
  const bool whole = j0 + VEC <= rows;
  for (int o = blockIdx.y * kSpliceWaves + (threadIdx.x >> 6); o < out_pad; o += gridDim.y * kSpliceWaves) {
    float s[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) s[c] = 0.0f;
    if (o < out_dim) {
      const int c = o / in_dim, d = o - c * in_dim;          // (wave-uniform)
      const int first = j0 + offsets[c];
      const float *p = x + (int64_t)d * ld;
      if (first >= 0 && first + VEC <= rows) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) s[k] = p[first + k];
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const int j = first + k;
          s[k] = p[j < 0 ? 0 : j >= rows ? rows - 1 : j];
        }
      }
    }
    float *q = out + (int64_t)o * out_ld + j0;
    if (VEC == 4 && whole) {
      f32x4 t;
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] = s[k];
      *reinterpret_cast<f32x4 *>(q) = t;
    } else {
      for (int k = 0; k < VEC && j0 + k < rows; ++k) q[k] = s[k];
    }
  }
}

}  // namespace

void LaunchTimeSplice(const float *x, int64_t ld, int rows, int in_dim, const int32_t *offsets_dev, int n, float *out,
                      int64_t out_ld, int out_pad, hipStream_t stream) {
  if (rows <= 0 || in_dim <= 0 || n <= 0) return;
  const bool vec = out_ld % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  const int per = vec ? 4 : 1;
  const int lines = (out_pad + kSpliceWaves - 1) / kSpliceWaves;
  dim3 grid((rows + 64 * per - 1) / (64 * per), lines < kMaxGridY ? lines : kMaxGridY);
  if (vec)
    hipLaunchKernelGGL((TimeSpliceKernel<4>), grid, dim3(kSpliceThreads), 0, stream, x, ld, rows, in_dim, offsets_dev, n * in_dim, out_pad, out, out_ld);
  else
    hipLaunchKernelGGL((TimeSpliceKernel<1>), grid, dim3(kSpliceThreads), 0, stream, x, ld, rows, in_dim, offsets_dev, n * in_dim, out_pad, out, out_ld);
}

}  // namespace pkmi
