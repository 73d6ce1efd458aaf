// resample.hip -- ResampleKernel: polyphase windowed-sinc conversion of PCM at 8 .. 96 kHz to 16 kHz (pk_resample.h,
// DESIGN.md section 11).  One launch serves the single-wave entry, the batch scorer and the online scorer through a
// per-item plan.
//
// A 256-thread workgroup belongs to one item (blockIdx.y) and converts tiles of kResampleTile consecutive outputs,
// tile blockIdx.x, blockIdx.x + gridDim.x, ...  It stages the item's table in LDS once and, per tile, the input span
// the tile's windows cover, zero padding written there for every sample outside the item's valid range.  Each output
// is then one thread's sum over its window, in ascending tap order: rounded product, rounded add, from +0.0f -- the
// order is fixed per output sample, so a result does not depend on tiling, batching or chunking.
//
// Traffic: 4 B read per input sample, 4 B written per output (the table comes from L2 once per workgroup).
// LDS: a weight row has stride max_taps | 1 floats (odd), so that neighbouring phases start on different banks;
// with one phase (32, 48, 96 kHz) every lane reads the same weight (a broadcast) and input addresses Q apart.
#include <hip/hip_runtime.h>

#include "pk_resample.h"

namespace pkmi {

__global__ __launch_bounds__(kResampleThreads) void ResampleKernel(const ResampleItem *__restrict__ items) {
  extern __shared__ __align__(16) float lds[];
  const ResampleItem it = items[blockIdx.y];
  const int P = it.P, Q = it.Q, taps = it.max_taps, wstride = taps | 1;
  const int64_t num_out = it.j1 - it.j0;
  const int64_t tiles = (num_out + kResampleTile - 1) / kResampleTile;
  if ((int64_t)blockIdx.x >= tiles) return;            // (uniform: before any barrier)
  float *w_s = lds;                                    // [P][wstride]
  int32_t *first_s = reinterpret_cast<int32_t *>(w_s + (size_t)P * wstride);
  int32_t *count_s = first_s + P;
  float *x_s = reinterpret_cast<float *>(count_s + P); // [span]
  const int tid = threadIdx.x;

  for (int i = tid; i < P * taps; i += kResampleThreads) {
    const int p = i / taps, k = i - p * taps;
    w_s[p * wstride + k] = it.weights[i];
  }
  for (int p = tid; p < P; p += kResampleThreads) {
    // a window outside [min_first, max_end) would leave the staged span: such a phase contributes nothing
    const int f = it.first[p], c = it.count[p];
    const bool ok = c >= 0 && c <= taps && f >= it.min_first && f + c <= it.max_end;
    first_s[p] = f;
    count_s[p] = ok ? c : 0;
  }

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t ja = it.j0 + tile * kResampleTile;
    const int64_t jb = ja + kResampleTile < it.j1 ? ja + kResampleTile : it.j1;
    // the span of the tile's windows: inputs [lo, hi)
    const int64_t ua = ja / P;
    const int pa = (int)(ja - ua * P), nj = (int)(jb - ja);
    const int64_t lo = ua * Q + it.min_first;
    const int64_t hi = (jb - 1) / P * Q + it.max_end;
    const int span = hi - lo < (int64_t)it.span ? (int)(hi - lo) : it.span;
    __syncthreads();                                   // the table is staged; the previous tile's reads are done
    for (int s = tid; s < span; s += kResampleThreads) {
      const int64_t g = lo + s - it.x0;                // index into the item's staged samples
      x_s[s] = (g >= 0 && g < it.n_valid) ? it.x[g] : 0.0f;
    }
    __syncthreads();
    for (int t = tid; t < nj; t += kResampleThreads) {   // output j = ja + t: unit ua + du, phase p (32-bit from here on)
      const int pp = pa + t, du = pp / P, p = pp - du * P;
      const int base = first_s[p] - it.min_first + du * Q;   // >= 0 by the definition of lo
      const int c = count_s[p];
      const float *wp = w_s + p * wstride;
      float acc = 0.0f;
      if (base >= 0 && base + c <= span) {
        const float *xp = x_s + base;
        for (int k = 0; k < c; ++k) acc = __fadd_rn(acc, __fmul_rn(wp[k], xp[k]));
      }
      it.y[ja - it.j0 + t] = acc;
    }
  }
}

void LaunchResample(const ResampleItem *d_items, int num_items, int64_t max_tiles, size_t lds_bytes, hipStream_t stream) {
  if (num_items <= 0 || max_tiles <= 0) return;
  // enough workgroups to fill the chip a few times over; an item with more tiles walks them with the grid's stride
  const int64_t per_item = (4096 + num_items - 1) / num_items;
  const unsigned gx = (unsigned)(max_tiles < per_item ? max_tiles : per_item);
  hipLaunchKernelGGL(ResampleKernel, dim3(gx, (unsigned)num_items), dim3(kResampleThreads), lds_bytes, stream, d_items);
}

// LDS beyond the 64 KiB a launch gets without asking: raised once per process (the largest table + span is ~108 KiB).
int ResampleAllowLds(size_t lds_bytes) {
  if (lds_bytes <= 65536) return 0;
  return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(ResampleKernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_bytes);
}

}  // namespace pkmi
