// delta.hip -- DeltaKernel: delta features, Kaldi's add-deltas (include/pk_mi355.h states the rule; DESIGN.md section
// 21).  It stands between the normalisation (NormKernel, OnlineCmvnKernel, CmvnChainKernel, or the raw rows in mode
// none) and FeatureLayoutKernel on a batch made by pk_mi355_deltas_batch_create: rows [sum T][Db] in, rows
// [sum T][(order + 1) Db] out, never in place.
//
// Shaped like NormKernel: lane = feature, so per frame the wave reads ONE contiguous run of up to 64 floats and writes
// order + 1 of them.  One wavefront per (utterance, run of kDeltaFrames frames, block of 64 base features):
//   Stage: the G + 2 M rows the run's outputs read (M = order * window, frames t0 - M .. t0 + G - 1 + M, each clamped
//     into the utterance's own rows: the edge rule is applied here, once) go to LDS as lane-private columns --
//     s_x[row][lane], which every lane writes and reads at its own lane only, so the wave needs no barrier and the
//     accesses are free of bank conflicts.  The loads are independent and are issued a group at a time.
//   Apply: for every block i the host's pkdelta::DeltaApply (pk_delta.h), instantiated on a run of G frames held in
//     registers: per tap ONE wave-uniform scale from the device table (a scalar load; a zero scale skips the tap for
//     the whole wave) and G products and adds per lane, j ascending for every frame -- each output's own chain is the
//     host's, operation for operation.  Then G coalesced stores of the block.
// Every address is formed from t clamped into [0, T) and d clamped into [d0, Db): a load past the utterance's rows or
// past feature Db - 1 is never issued, so a poisoned neighbour is never read; a lane past Db shadows the block's first
// feature and stores nothing; a run that starts behind the utterance's last frame returns before it touches memory.
#include <hip/hip_runtime.h>

#include "pk_delta_kernel.h"

namespace pkmi {

namespace {

constexpr int kG = kDeltaFrames;

// The run of G frames of one column that a lane holds: what DeltaApply's float is on the host.
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

__global__ __launch_bounds__(64) void DeltaKernel(const float *__restrict__ in, UttLayout utts, int num_utts, int Db, int order, int window,
                                                  const float *__restrict__ scales, float *__restrict__ out) {
  extern __shared__ float s_x[];                      // [kG + 2 M][64]
  const int lane = threadIdx.x;
  const int t0 = blockIdx.x * kG;
  const int d0 = blockIdx.y * 64;
  const bool live = d0 + lane < Db;
  const int d = live ? d0 + lane : d0;
  const int M = order * window, L = 2 * M + 1;
  const int64_t F = (int64_t)(order + 1) * Db;
  for (int u = blockIdx.z; u < num_utts; u += gridDim.z) {          // (uniform over the wave)
    const int T = utts.num_frames[u];
    if (t0 >= T) continue;
    const float *x = in + utts.raw_base[u] * Db + d;
    float *y = out + utts.raw_base[u] * F + d;
    const int rows = kG + 2 * M;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) {
      const int t = t0 - M + r;
      s_x[r * 64 + lane] = x[(int64_t)(t < 0 ? 0 : t < T ? t : T - 1) * Db];
    }
    for (int i = 0; i <= order; ++i) {
      const FrameRun acc = pkdelta::DeltaApply<FrameRun>(scales + i * L + M, i * window, [&](int j) {
        FrameRun r;
#pragma unroll
        for (int f = 0; f < kG; ++f) r.v[f] = s_x[(f + M + j) * 64 + lane];
        return r;
      });
      if (live) {
#pragma unroll
        for (int f = 0; f < kG; ++f)
          if (t0 + f < T) y[(int64_t)(t0 + f) * F + (int64_t)i * Db] = acc.v[f];
      }
    }
  }
}

}  // namespace

void LaunchDelta(const float *in, const UttLayout &utts, int num_utts, int max_frames, int base_dim, const pk_mi355_deltas_spec_t &spec,
                 const float *d_scales, float *out, hipStream_t stream) {
  if (num_utts <= 0 || max_frames <= 0 || base_dim <= 0) return;
  const dim3 grid((max_frames + kG - 1) / kG, (base_dim + 63) / 64, num_utts < 65535 ? num_utts : 65535);
  const size_t lds = sizeof(float) * 64 * (size_t)(kG + 2 * pkdelta::Reach(spec));
  hipLaunchKernelGGL(DeltaKernel, grid, dim3(64), lds, stream, in, utts, num_utts, base_dim, spec.order, spec.window, d_scales, out);
}

}  // namespace pkmi
