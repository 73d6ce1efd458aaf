// features.hip -- FeatureLayoutKernel: features the caller already has, frame-major [sum T][D], become the padded
// feature-major operand Yt[D][ldy] of the spliced first layer, for every utterance of a call in one launch
// (pk_score.h; the host side is capi_batch.hip).  Further down: CmvnChainKernel, the
// sliding-window CMVN on raw rows of any feature dimension, which runs in front of it.
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

#include "pk_norm.h"
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

// ------------------------------------------------------------------ CMVN at any dimension
//
// CmvnChainKernel: raw rows [sum T][D] -> normalised rows [sum T][D], both frame-major; FeatureLayoutKernel then lays the
// result out.  cmvn.cc is elementwise in the feature index, so this is CmvnKernel's chain (pk_norm.h's sliding steps) with
// any number of lanes: one wavefront per (utterance, block of 64 features), lane = feature, serial over t.  Per frame the
// wave reads and writes ONE contiguous run of up to 64 floats; the frame that leaves the window (t - 600) is read raw
// from the input, which is why the kernel cannot run in place.  Frames are taken kChainAhead at a time and the loads of
// the next group are issued before the chain of the current one -- the rows and the two table entries of each of its
// frames (wave-uniform: scalar loads) -- so the chain waits on its own f64 adds, not on memory.
// Every address is formed from t clamped into [0, T) and d clamped into [d0, D): a load past the utterance's rows
// or past feature D - 1 is never issued; a lane past D shadows the block's first feature and stores nothing.
constexpr int kChainAhead = 8;

__global__ __launch_bounds__(64) void CmvnChainKernel(const float *__restrict__ raw, UttLayout utts, int num_utts, int D,
                                                      const float *__restrict__ g, const CmvnTables *__restrict__ tab,
                                                      float *__restrict__ out) {
  const int d0 = blockIdx.x * 64;
  const bool live = d0 + (int)threadIdx.x < D;
  const int d = live ? d0 + threadIdx.x : d0;
  const float gd = g[d];
  for (int u = blockIdx.y; u < num_utts; u += gridDim.y) {          // (uniform over the wave)
    const int T = utts.num_frames[u];
    if (T <= 0) continue;
    const float *x = raw + utts.raw_base[u] * D + d;
    float *y = out + utts.raw_base[u] * D + d;
    auto row = [&](int t) { return (int64_t)(t < 0 ? 0 : t < T ? t : T - 1) * D; };
    float cur[kChainAhead], old[kChainAhead], nxt[kChainAhead], nold[kChainAhead];
    float al[kChainAhead], ns[kChainAhead], nal[kChainAhead], nns[kChainAhead];     // alpha, neg_scale of the group's frames
#pragma unroll
    for (int k = 0; k < kChainAhead; ++k) {                         // (T >= 1; no frame has left yet; k < 600)
      cur[k] = x[row(k)]; old[k] = 0.0f;
      al[k] = tab->alpha[k]; ns[k] = tab->neg_scale[k];
    }
    float s = 0.0f;
    for (int t0 = 0; t0 < T; t0 += kChainAhead) {
#pragma unroll
      for (int k = 0; k < kChainAhead; ++k) {                       // the next group's loads, ahead of this group's chain
        const int t = t0 + kChainAhead + k;
        const int tt = t < kCmvnWindow ? t : kCmvnWindow - 1;
        nxt[k] = x[row(t)];
        nold[k] = x[row(t - kCmvnWindow)];
        nal[k] = tab->alpha[tt]; nns[k] = tab->neg_scale[tt];
      }
#pragma unroll
      for (int k = 0; k < kChainAhead; ++k) {
        const int t = t0 + k;
        if (t < T) {
          s = pknorm::SlidingSum(s, cur[k], old[k], t >= kCmvnWindow);
          const float v = pknorm::SlidingApply(cur[k], s, al[k], ns[k], gd, t + 1 < kCmvnWindow);
          if (live) y[(int64_t)t * D] = v;
        }
      }
#pragma unroll
      for (int k = 0; k < kChainAhead; ++k) { cur[k] = nxt[k]; old[k] = nold[k]; al[k] = nal[k]; ns[k] = nns[k]; }
    }
  }
}

}  // namespace

void LaunchCmvnChain(const float *raw, const UttLayout &utts, int num_utts, int dim, const float *d_global, const CmvnTables *d_cmvn_tab,
                     float *out, hipStream_t stream) {
  if (num_utts <= 0 || dim <= 0) return;
  const dim3 grid((dim + 63) / 64, num_utts < 65535 ? num_utts : 65535);
  hipLaunchKernelGGL(CmvnChainKernel, grid, dim3(64), 0, stream, raw, utts, num_utts, dim, d_global, d_cmvn_tab, out);
}

void LaunchFeatureLayout(const float *feats, const UttLayout &utts, int num_utts, int max_frames, int dim, int left, int right,
                         float *yt, int64_t ldy, hipStream_t stream) {
  if (num_utts <= 0 || max_frames <= 0 || dim <= 0) return;
  const dim3 grid((max_frames + kFlTile - 1) / kFlTile, num_utts < 65535 ? num_utts : 65535);
  hipLaunchKernelGGL(FeatureLayoutKernel, grid, dim3(kFlThreads), 0, stream, reinterpret_cast<const uint32_t *>(feats), utts, num_utts,
                     dim, left, right, reinterpret_cast<uint32_t *>(yt), ldy);
}

}  // namespace pkmi
