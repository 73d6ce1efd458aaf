// features.hip -- FeatureLayoutKernel: features the caller already has, frame-major [sum T][D], become the padded
// feature-major operand Yt[D][ldy] of the spliced first layer, for every utterance of a call in one launch
// (pk_score.h; the host side is capi_batch.hip).
//
// A pure copy: frame t of utterance u goes to column pad_base[u] + L + t, frame 0 into the L columns in front of it
// and frame T - 1 into the R columns behind (the clamp of am.cc:73-75 done once at write time, as CmvnKernel does it).
// No arithmetic touches a value, so every bit pattern arrives unchanged (NaN payloads, -0.0, subnormals).
//
// One 256-thread workgroup per (utterance, tile of 64 frames); the features are walked in blocks of 64.  A block of the
// tile goes through LDS so that both sides of the transpose are coalesced: it is read in runs that are contiguous in
// memory (for D <= 64 the whole tile is ONE span of 64 D floats) and written with lane = frame, 256 contiguous bytes
// per wave and feature row.  The LDS tile's leading dimension is odd (65): ds_write_b32 / ds_read_b32 bank modulo 32,
// and lane = frame then walks 64 different banks' worth of addresses instead of one.  Plain dword accesses only: an
// utterance's first row is 4-byte aligned and no better.  Workgroups never wait on each other.
#include <hip/hip_runtime.h>

#include "pk_score.h"

namespace pkmi {

namespace {

constexpr int kFlTile = 64;             // frames per workgroup, features per block
constexpr int kFlLd = kFlTile + 1;      // odd leading dimension of the LDS tile
constexpr int kFlThreads = 256;

__global__ __launch_bounds__(kFlThreads) void FeatureLayoutKernel(const uint32_t *__restrict__ feats, UttLayout utts, int num_utts,
                                                                  int D, int left, int right, uint32_t *__restrict__ yt, int64_t ldy) {
  __shared__ uint32_t tile[kFlTile * kFlLd];            // [frame][feature of the block]
  const int tid = threadIdx.x;
  const int t0 = blockIdx.x * kFlTile;
  for (int u = blockIdx.y; u < num_utts; u += gridDim.y) {          // (every condition below is uniform over the workgroup)
    const int T = utts.num_frames[u];
    if (t0 >= T) continue;
    const int nt = T - t0 < kFlTile ? T - t0 : kFlTile;             // frames of this tile
    const uint32_t *src = feats + (utts.raw_base[u] + t0) * D;
    uint32_t *col0 = yt + utts.pad_base[u];                         // the utterance's first column (its left pad)
    for (int d0 = 0; d0 < D; d0 += kFlTile) {
      const int nd = D - d0 < kFlTile ? D - d0 : kFlTile;           // features of this block
      if (D <= kFlTile) {
        for (int i = tid; i < nt * D; i += kFlThreads) {            // one contiguous span
          const int f = i / D, d = i - f * D;
          tile[f * kFlLd + d] = src[i];
        }
      } else {
        for (int i = tid; i < nt * kFlTile; i += kFlThreads) {      // runs of nd floats, one per frame
          const int f = i >> 6, d = i & 63;
          if (d < nd) tile[f * kFlLd + d] = src[(int64_t)f * D + d0 + d];
        }
      }
      __syncthreads();
      const int f = tid & 63;                                       // lane = frame
      if (f < nt)
        for (int d = tid >> 6; d < nd; d += kFlThreads / 64) col0[(int64_t)(d0 + d) * ldy + left + t0 + f] = tile[f * kFlLd + d];
      if (t0 == 0)                                                  // this workgroup holds frame 0: the left pad
        for (int i = tid; i < nd * left; i += kFlThreads) {
          const int d = i / left, p = i - d * left;
          col0[(int64_t)(d0 + d) * ldy + p] = tile[d];
        }
      if (t0 + nt == T)                                             // ... frame T - 1: the right pad
        for (int i = tid; i < nd * right; i += kFlThreads) {
          const int d = i / right, p = i - d * right;
          col0[(int64_t)(d0 + d) * ldy + left + T + p] = tile[(nt - 1) * kFlLd + d];
        }
      __syncthreads();
    }
  }
}

}  // namespace

void LaunchFeatureLayout(const float *feats, const UttLayout &utts, int num_utts, int max_frames, int dim, int left, int right,
                         float *yt, int64_t ldy, hipStream_t stream) {
  if (num_utts <= 0 || max_frames <= 0 || dim <= 0) return;
  const dim3 grid((max_frames + kFlTile - 1) / kFlTile, num_utts < 65535 ? num_utts : 65535);
  hipLaunchKernelGGL(FeatureLayoutKernel, grid, dim3(kFlThreads), 0, stream, reinterpret_cast<const uint32_t *>(feats), utts, num_utts,
                     dim, left, right, reinterpret_cast<uint32_t *>(yt), ldy);
}

}  // namespace pkmi
