// stream.hip -- the online scorer's kernels, which carry a slot's state from one step to the next, and their launchers
// (pk_score.h; the host object is capi_stream.hip).
//
// The reference pipeline is causal: frame t of fbank reads samples [160 t, 160 t + 400) only
// (fbank.cc:35-42, 193-245); online CMVN (cmvn.cc:35-71) is a running window sum rounded to float after every frame,
// so that float vector and the raw frames still inside the 600-frame window are its whole state; the splice
// (am.cc:65-88) needs R frames of look-ahead and clamps at frame 0 and at the last frame only.  Every frame's
// log-likelihoods therefore equal the whole-utterance batch scorer's, bit for bit, whatever the chunk sizes.
#include <hip/hip_runtime.h>

#include "pk_score.h"

using namespace pkhost;

namespace {

constexpr int kWave = 64;

// One workgroup per slot: segment = carried tail + pushed samples -> wave staging; the samples from 160 m on (those of
// frames not yet complete) -> the slot's other tail buffer.
__global__ __launch_bounds__(256) void StreamAssembleKernel(const StreamRec *__restrict__ recs, const float *__restrict__ upload,
                                                            float *__restrict__ tails, float *__restrict__ wave) {
  const StreamRec r = recs[blockIdx.x];
  const int seg = r.tail_len + r.new_len;
  const int keep = kFrameShift * r.m;
  const float *src = tails + ((int64_t)r.slot * 2 + r.tail_par) * kTailCap;
  float *dst = tails + ((int64_t)r.slot * 2 + (r.tail_par ^ 1)) * kTailCap;
  for (int i = threadIdx.x; i < seg; i += blockDim.x) {
    const float v = i < r.tail_len ? src[i] : upload[r.new_off + i - r.tail_len];
    wave[r.woff + i] = v;
    if (i >= keep) dst[i - keep] = v;
  }
}

// One wavefront per slot.  Lane = feature for the serial chain, exactly CmvnKernel's arithmetic (frontend.hip): one
// f32 add while the window fills, widen / two fp64 adds / narrow once it slides (cmvn.cc:44-70), then the smoothing
// with the global sums and the 1/count scale of the global frame index (cmvn.cc:73-101, CmvnTables).  The step's raw
// rows are turned into CMVN'd rows in place.  Then lane = column: the slot's region of the spliced operand.
__global__ __launch_bounds__(kWave) void StreamCmvnKernel(const StreamRec *__restrict__ recs, float *__restrict__ rows,
                                                          const float *__restrict__ g, const CmvnTables *__restrict__ tab,
                                                          float *__restrict__ sums, float *__restrict__ raw_hist,
                                                          float *__restrict__ hist, int hist_len, int left, int right,
                                                          float *__restrict__ yt, int64_t ldy) {
  const StreamRec r = recs[blockIdx.x];
  const int lane = threadIdx.x;
  const int d = lane < kNumBins ? lane : 0;          // lanes 40..63 shadow feature 0 and store nothing
  float *x = rows + r.raw_base * kNumBins;
  float *rh = raw_hist + (int64_t)r.slot * kCmvnWindow * kNumBins;
  float *hh = hist + (int64_t)r.slot * hist_len * kNumBins;
  if (r.m > 0) {
    float s = r.n_old > 0 ? sums[r.slot * kNumBins + d] : 0.0f;
    const float gd = g[d];
#pragma unroll 8
    for (int i = 0; i < r.m; ++i) {
      const int t = r.n_old + i;
      const int h = t % kCmvnWindow;                 // x[t - 600] leaves the window from the slot x[t] takes
      const float xv = x[i * kNumBins + d];
      double acc = s;                                // cmvn.cc:44-52
      acc += xv;
      if (t >= kCmvnWindow) acc += -1.0 * static_cast<double>(rh[h * kNumBins + d]);     // cmvn.cc:58-64
      s = static_cast<float>(acc);                   // cmvn.cc:66-70
      const int tt = t < kCmvnWindow ? t : kCmvnWindow - 1;
      float st = s;
      if (t + 1 < kCmvnWindow) st += tab->alpha[tt] * gd;                                 // cmvn.cc:73-92
      float y = xv;
      y += tab->neg_scale[tt] * st;                                                       // cmvn.cc:94-101
      if (lane < kNumBins) {
        rh[h * kNumBins + d] = xv;
        x[i * kNumBins + d] = y;
      }
    }
    if (lane < kNumBins) sums[r.slot * kNumBins + d] = s;
  }
  __syncthreads();
  // Columns a - L .. b + R - 1 (then zeros up to the region's end): frame f from this step's rows (f >= n_old) or from
  // the slot's history of the last L + R CMVN'd frames.  Clamped at frame 0 and, once closed, at the last frame.
  const int n = r.n_old + r.m;
  const int real = r.b - r.a + left + right;
  for (int c = lane; c < r.cols; c += kWave) {
    float *dst = yt + r.col_base + c;
    if (c >= real) {                               // the region's padding columns (rows nobody reads)
      for (int k = 0; k < kNumBins; ++k) dst[(int64_t)k * ldy] = 0.0f;
      continue;
    }
    int f = r.a - left + c;
    f = f < 0 ? 0 : f;
    if (r.closed && f > n - 1) f = n - 1;          // open: f <= b + R - 1 <= n - 1 already
    const float *src = f >= r.n_old ? x + (int64_t)(f - r.n_old) * kNumBins : hh + (int64_t)(f % hist_len) * kNumBins;
    for (int k = 0; k < kNumBins; ++k) dst[(int64_t)k * ldy] = src[k];
  }
  __syncthreads();
  // the last L + R CMVN'd frames, for the next step's left context (the reads above are done)
  const int f0 = n - hist_len > r.n_old ? n - hist_len : r.n_old;
  for (int i = lane; i < (n - f0) * kNumBins; i += kWave) {
    const int f = f0 + i / kNumBins, k = i % kNumBins;
    hh[(int64_t)(f % hist_len) * kNumBins + k] = x[(int64_t)(f - r.n_old) * kNumBins + k];
  }
}

}  // namespace

// ================================================================== launchers (pk_score.h)

namespace pkmi {

void LaunchStreamAssemble(const StreamRec *recs, int n, const float *upload, float *tails, float *wave, hipStream_t stream) {
  hipLaunchKernelGGL(StreamAssembleKernel, dim3(n), dim3(256), 0, stream, recs, upload, tails, wave);
}

void LaunchStreamCmvn(const StreamRec *recs, int n, float *rows, const float *g, const CmvnTables *tab, float *sums,
                      float *raw_hist, float *hist, int hist_len, int left, int right, float *yt, int64_t ldy, hipStream_t stream) {
  hipLaunchKernelGGL(StreamCmvnKernel, dim3(n), dim3(kWave), 0, stream, recs, rows, g, tab, sums, raw_hist, hist, hist_len,
                     left, right, yt, ldy);
}

}  // namespace pkmi
