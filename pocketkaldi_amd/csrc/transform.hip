// transform.hip -- TransformKernel: the feature transform, Kaldi's splice-feats | transform-feats and the per-utterance
// transform-feats (include/pk_mi355.h states the rule).  It stands between the normalisation (or
// DeltaKernel) and FeatureLayoutKernel on a batch made by pk_mi355_transform_batch_create: rows [sum T][Dp] in, rows
// [sum T][rows] out, never in place.  One kernel serves both stages: the matrix table has a stride, 0 when every
// utterance reads the same matrix (the global stage), else utterance u reads matrix u.
//
// Lane = output feature.  One wavefront (a workgroup of its own) per (utterance, run of G = kTransformFrames frames,
// block of 64 outputs):
//   Stage: the G + L + R input rows the run's outputs read (frames t0 - L .. t0 + G - 1 + R, each clamped into the
//     utterance's own rows: the edge rule is applied here, once) go to LDS as they lie, s_x[row][d], the lanes striding
//     over d -- coalesced loads.  The workgroup is this one wave and every branch around the staging is uniform over
//     it, so the __syncthreads() that orders the staging against the reads is one no wave waits at alone.
//   Apply: the host's pkxf::TransformApply (pk_transform.h) instantiated on a run of G frames held in registers: per k
//     ONE load of the lane's matrix entry (the matrix lies transposed and padded, [k][ldo]: a wave's read of one k is
//     one contiguous run, the lanes past `rows` read the padding's zeros) and G LDS reads at a wave-uniform address
//     (a broadcast, free of bank conflicts), G products and G adds -- k ascending for every frame, the offset last:
//     each output's own chain is the host's, operation for operation.  No MFMA, no fma (the pragma below, and
//     -ffp-contract=off).  Then G stores of the block.
// Every address is formed from t clamped into [0, T), d < Dp and o inside the padded matrix: a load past the
// utterance's rows is never issued, so a poisoned neighbour is never read; a lane past `rows` stores nothing; a run
// that starts behind the utterance's last frame goes on before it touches memory, so a frameless utterance costs its
// waves' launch only.
#include <hip/hip_runtime.h>

#include "pk_transform_kernel.h"

#pragma clang fp contract(off)

namespace pkmi {

namespace {

constexpr int kG = kTransformFrames;

// The run of G frames of one output that a lane holds: what TransformApply's float is on the host.
struct FrameRun {
  float v[kG];
  __device__ explicit FrameRun(float x) {
#pragma unroll
    for (int f = 0; f < kG; ++f) v[f] = x;
  }
  __device__ FrameRun() {}
};
__device__ inline FrameRun operator*(float s, const FrameRun &x) {
  FrameRun p;
#pragma unroll
  for (int f = 0; f < kG; ++f) p.v[f] = s * x.v[f];
  return p;
}
__device__ inline FrameRun operator+(const FrameRun &a, const FrameRun &b) {
  FrameRun r;
#pragma unroll
  for (int f = 0; f < kG; ++f) r.v[f] = a.v[f] + b.v[f];
  return r;
}

__global__ __launch_bounds__(64) void TransformKernel(const float *__restrict__ in, UttLayout utts, int num_utts, int Dp, int L, int R, int rows,
                                                      int affine, const float *__restrict__ mt, int64_t mat_stride, float *__restrict__ out) {
  extern __shared__ float s_x[];                      // [kG + L + R][Dp]
  const int lane = threadIdx.x;
  const int t0 = blockIdx.x * kG;
  const int o = blockIdx.y * 64 + lane;               // < ldo: inside the padded matrix
  const int ldo = (rows + 63) / 64 * 64;
  const int W = L + R + 1, staged = kG + L + R;
  for (int u = blockIdx.z; u < num_utts; u += gridDim.z) {          // (uniform over the wave, which is the workgroup)
    const int T = utts.num_frames[u];
    if (t0 >= T) continue;
    const float *x = in + utts.raw_base[u] * Dp;
    const float *m = mt + (int64_t)u * mat_stride + o;
    __syncthreads();                                  // (a second utterance of this wave: the last one's reads are done)
    for (int r = 0; r < staged; ++r) {
      const int t = t0 - L + r;
      const float *row = x + (int64_t)(t < 0 ? 0 : t < T ? t : T - 1) * Dp;
      for (int d = lane; d < Dp; d += 64) s_x[r * Dp + d] = row[d];
    }
    __syncthreads();
    const FrameRun acc = pkxf::TransformApply<FrameRun>(W, Dp, affine != 0, [&](int k) { return m[(int64_t)k * ldo]; }, [&](int j, int d) {
      FrameRun v;
#pragma unroll
      for (int f = 0; f < kG; ++f) v.v[f] = s_x[(f + j) * Dp + d];
      return v;
    });
    if (o < rows) {
      float *y = out + utts.raw_base[u] * rows + o;
#pragma unroll
      for (int f = 0; f < kG; ++f)
        if (t0 + f < T) y[(int64_t)(t0 + f) * rows] = acc.v[f];
    }
  }
}

}  // namespace

void LaunchTransform(const float *in, const UttLayout &utts, int num_utts, int max_frames, const TransformStage &s, float *out, hipStream_t stream) {
  if (num_utts <= 0 || max_frames <= 0 || s.in_dim <= 0 || s.rows <= 0) return;
  const dim3 grid((max_frames + kG - 1) / kG, (s.rows + 63) / 64, num_utts < 65535 ? num_utts : 65535);
  hipLaunchKernelGGL(TransformKernel, grid, dim3(64), TransformLds(s), stream, in, utts, num_utts, s.in_dim, s.left, s.right, s.rows, s.affine ? 1 : 0,
                     s.mt, s.mat_stride, out);
}

}  // namespace pkmi
