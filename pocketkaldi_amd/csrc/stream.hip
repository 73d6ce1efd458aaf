// stream.hip -- the online scorer's kernels, which carry a slot's state from one step to the next, and their launchers
// (pk_score.h; the host object is capi_stream.hip).
//
// The reference pipeline is causal: frame t of fbank reads samples [160 t, 160 t + 400) only
// (fbank.cc:35-42, 193-245); online CMVN (cmvn.cc:35-71) is a running window sum rounded to float after every frame,
// so that float vector and the raw frames still inside the 600-frame window are its whole state; the splice
// (am.cc:65-88) needs R frames of look-ahead and clamps at frame 0 and at the last frame only.  Every frame's
// log-likelihoods therefore equal the whole-utterance batch scorer's, bit for bit, whatever the chunk sizes.
//
// Feature slots enter behind the front-end: RAW rows are copied to where FbankKernel would have
// written them (StreamRawRowsKernel) and StreamCmvnKernel runs on them unchanged; NORMALIZED frames of any dimension
// are laid out by StreamFeatureLayoutKernel, which carries the left context in two history buffers used in turn.
// Under a normalisation spec other than the sliding rule audio and RAW rows go through
// StreamNormKernel and StreamFeatureLayoutKernel instead of StreamCmvnKernel / StreamCmvnChainKernel.
#include <hip/hip_runtime.h>

#include "pk_norm_kernel.h"
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
// The chain restates pknorm::SlidingSum and SlidingApply (pk_norm.h); DESIGN.md section 23 says why.
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

// ------------------------------------------------------------------ feature slots

// One workgroup per record: a RAW slot's pushed rows go from the upload staging to where FbankKernel would have written
// them, the slot's raw rows of the step; StreamCmvnKernel then finds them there.  A copy through uint32_t.
__global__ __launch_bounds__(256) void StreamRawRowsKernel(const StreamRec *__restrict__ recs, const uint32_t *__restrict__ upload,
                                                           uint32_t *__restrict__ rows) {
  const StreamRec r = recs[blockIdx.x];
  if (r.kind != PK_MI355_FEATS_RAW) return;
  const uint32_t *src = upload + r.new_off;
  uint32_t *dst = rows + r.raw_base * kNumBins;
  for (int i = threadIdx.x; i < r.m * kNumBins; i += blockDim.x) dst[i] = src[i];
}

constexpr int kSflTile = 64;            // columns per workgroup, features per block
constexpr int kSflLd = kSflTile + 1;    // odd leading dimension of the LDS tile (features.hip tells why)
constexpr int kSflThreads = 256;

// NORMALIZED slots: what StreamCmvnKernel's column loop does, without the arithmetic and for any D, shaped after
// FeatureLayoutKernel (features.hip).  One 256-thread workgroup per (record, tile of 64 columns of the slot's region);
// the features are walked in blocks of 64 through an LDS tile: a column's features are read as one run contiguous in
// memory (neighbouring columns are neighbouring frames, so for D <= 64 the runs join), and written with lane = column,
// 256 contiguous bytes per wave and feature row.  Column c of the region holds frame a - L + c, clamped to frame 0 and
// to frame n - 1 (an open slot's last column is frame b + R - 1 <= n - 1 already: the clamp binds once it is closed);
// the columns from (b - a) + L + R on are zero.  Frame f comes from the step's new frames when f >= n_old, otherwise from
// the slot's history: the ring [f % hist_len][D] of buffer hist_par, read only for f < n_old, so only when n_old > 0,
// and f >= a - L >= n_old - R - L lies inside it.
//
// The history is handed on without workgroups talking to each other: every workgroup of the slot reads buffer hist_par,
// and the slot's first workgroup writes frames [max(n - hist_len, 0), n) -- the new ones, and those of the old ring that
// survive -- into the OTHER buffer, which nobody reads in this launch.  The host flips hist_par when m > 0; with m == 0
// (a flush served from history alone) nothing is written and nothing flips.  A pure copy through uint32_t: NaN payloads,
// -0.0 and subnormals arrive as they were.  Plain dword accesses, __syncthreads() only; every condition around a
// barrier is uniform over the workgroup.
__global__ __launch_bounds__(kSflThreads) void StreamFeatureLayoutKernel(const StreamRec *__restrict__ recs, int num_recs,
                                                                         const uint32_t *__restrict__ upload, uint32_t *__restrict__ hist,
                                                                         int hist_len, int D, int left, int right,
                                                                         uint32_t *__restrict__ yt, int64_t ldy) {
  __shared__ uint32_t tile[kSflTile * kSflLd];          // [column][feature of the block]
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * kSflTile;
  for (int k = blockIdx.y; k < num_recs; k += gridDim.y) {
    const StreamRec r = recs[k];
    const int n = r.n_old + r.m;
    const uint32_t *fresh = upload + r.row_off;                                            // frames n_old .. n - 1, [m][D]
    const uint32_t *old = hist + ((int64_t)r.slot * 2 + r.hist_par) * hist_len * D;        // frames below n_old
    if (blockIdx.x == 0 && r.m > 0) {
      uint32_t *next = hist + ((int64_t)r.slot * 2 + (r.hist_par ^ 1)) * hist_len * D;
      const int f0 = n - hist_len > 0 ? n - hist_len : 0;
      for (int i = tid; i < (n - f0) * D; i += kSflThreads) {
        const int j = i / D, d = i - j * D, f = f0 + j;
        const uint32_t *src = f >= r.n_old ? fresh + (int64_t)(f - r.n_old) * D : old + (int64_t)(f % hist_len) * D;
        next[(int64_t)(f % hist_len) * D + d] = src[d];
      }
    }
    if (c0 >= r.cols) continue;                                                            // past the slot's region (or no rows)
    const int nc = r.cols - c0 < kSflTile ? r.cols - c0 : kSflTile;                        // columns of this tile
    const int real = r.b - r.a + left + right;
    uint32_t *col0 = yt + r.col_base + c0;
    for (int d0 = 0; d0 < D; d0 += kSflTile) {
      const int nd = D - d0 < kSflTile ? D - d0 : kSflTile;                                // features of this block
      const int w = D <= kSflTile ? D : kSflTile;                                          // (D <= 64: one block, nd == D)
      for (int i = tid; i < nc * w; i += kSflThreads) {
        const int c = i / w, d = i - c * w;
        if (d >= nd) continue;
        uint32_t v = 0;
        if (c0 + c < real) {
          int f = r.a - left + c0 + c;
          f = f < 0 ? 0 : f;
          f = f > n - 1 ? n - 1 : f;
          const uint32_t *src = f >= r.n_old ? fresh + (int64_t)(f - r.n_old) * D : old + (int64_t)(f % hist_len) * D;
          v = src[d0 + d];
        }
        tile[c * kSflLd + d] = v;
      }
      __syncthreads();
      const int c = tid & 63;                                                              // lane = column
      if (c < nc)
        for (int d = tid >> 6; d < nd; d += kSflThreads / 64) col0[(int64_t)(d0 + d) * ldy + c] = tile[c * kSflLd + d];
      __syncthreads();
    }
  }
}

// RAW slots at a feature dimension other than 40: StreamCmvnKernel's chain with any number of
// lanes, through pknorm::SlidingSum and SlidingApply (pk_norm.h).
// One wavefront per (record, block of 64 features), lane = feature; NORMALIZED records and records that brought no
// frames return at once.  RAW records bring pushed rows, audio records of a front-end spec the
// rows FbankAnyKernel has just written.  The slot's m fresh rows are normalised IN PLACE where they lie in the upload
// staging ([m][D] at row_off): the raw values the window needs later are kept in the slot's ring raw_hist[slot][600][D], the
// running sums in sums[slot][D], exactly as StreamCmvnKernel keeps them at 40.  StreamFeatureLayoutKernel then lays the
// record out as it does a NORMALIZED one.  A lane owns its feature's column of the rows, the ring and the sums, so
// no two lanes (and no two waves) touch one address.  Frames are taken kSChainAhead at a time, the next group's loads
// (rows, ring entries, and the two table entries of each frame) issued before the current group's chain and stores: the
// ring positions and rows of the two groups differ (600 is far more than 2 kSChainAhead).  Addresses are formed from i clamped into [0, m) and d clamped into [d0, D).
constexpr int kSChainAhead = 8;

__global__ __launch_bounds__(kWave) void StreamCmvnChainKernel(const StreamRec *__restrict__ recs, int D, float *upload,
                                                               const float *__restrict__ g, const CmvnTables *__restrict__ tab,
                                                               float *__restrict__ sums, float *raw_hist) {
  const StreamRec r = recs[blockIdx.x];
  if (r.kind == PK_MI355_FEATS_NORMALIZED || r.m <= 0) return;
  const int d0 = blockIdx.y * kWave;
  const bool live = d0 + (int)threadIdx.x < D;
  const int d = live ? d0 + threadIdx.x : d0;
  float *x = upload + r.row_off + d;
  float *rh = raw_hist + (int64_t)r.slot * kCmvnWindow * D + d;
  const int m = r.m;
  auto row = [&](int i) { return (int64_t)(i < m ? i : m - 1) * D; };
  auto ring = [&](int i) { return (int64_t)((r.n_old + (i < m ? i : m - 1)) % kCmvnWindow) * D; };
  float s = r.n_old > 0 ? sums[(int64_t)r.slot * D + d] : 0.0f;
  const float gd = g[d];
  float cur[kSChainAhead], old[kSChainAhead], nxt[kSChainAhead], nold[kSChainAhead];
  float al[kSChainAhead], ns[kSChainAhead], nal[kSChainAhead], nns[kSChainAhead];   // alpha, neg_scale of the group's frames
  auto entry = [&](int i) { return r.n_old + i < kCmvnWindow ? r.n_old + i : kCmvnWindow - 1; };
#pragma unroll
  for (int k = 0; k < kSChainAhead; ++k) {
    cur[k] = x[row(k)];
    old[k] = r.n_old + k >= kCmvnWindow ? rh[ring(k)] : 0.0f;      // (the ring is read only once the window slides)
    al[k] = tab->alpha[entry(k)]; ns[k] = tab->neg_scale[entry(k)];
  }
  for (int i0 = 0; i0 < m; i0 += kSChainAhead) {
#pragma unroll
    for (int k = 0; k < kSChainAhead; ++k) {                        // the next group's loads, ahead of this group's chain
      const int i = i0 + kSChainAhead + k;
      nxt[k] = x[row(i)];
      nold[k] = r.n_old + i >= kCmvnWindow ? rh[ring(i)] : 0.0f;
      nal[k] = tab->alpha[entry(i)]; nns[k] = tab->neg_scale[entry(i)];
    }
#pragma unroll
    for (int k = 0; k < kSChainAhead; ++k) {
      const int i = i0 + k;
      if (i < m) {
        const int t = r.n_old + i;
        const float xv = cur[k];
        s = pknorm::SlidingSum(s, xv, old[k], t >= kCmvnWindow);
        const float v = pknorm::SlidingApply(xv, s, al[k], ns[k], gd, t + 1 < kCmvnWindow);
        if (live) {
          rh[ring(i)] = xv;
          x[row(i)] = v;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kSChainAhead; ++k) { cur[k] = nxt[k]; old[k] = nold[k]; al[k] = nal[k]; ns[k] = nns[k]; }
  }
  if (live) sums[(int64_t)r.slot * D + d] = s;
}

// Audio and RAW slots of a scorer whose normalisation spec is `speaker` or online CMVN, in
// StreamCmvnChainKernel's place and shape: one wavefront per (record, block of 64 features), lane = feature, the slot's m
// fresh rows normalised IN PLACE at rows + row_off; StreamFeatureLayoutKernel then lays the record out.  A lane owns
// its feature's column of the rows, of the ring and of the two pairs of sums.
//   Both modes: total[slot] gains every frame's value and square (pknorm::StatsAdd), t ascending -- the utterance
//     rule's order, so the record of a whole slot is the batch scorer's norm_stats of the whole input.
//   speaker: y = NormApply(x, the slot's finalised offset and scale).
//   online CMVN: the batch kernel's steps (norm.hip; here through pknorm::MakeOnlinePrior and WindowStep) with the
//     state carried from step to step -- the window sums in
//     win[slot], the raw rows still inside the window in ring[slot][t % W] (frame t - W leaves from the position frame
//     t takes).  Frames are taken kSNormAhead at a time, the next group's rows and ring entries loaded into registers
//     ahead of the current group's chain and handed to it through LDS (lane-private columns: no barrier).  A ring entry
//     that this very launch writes (t - W >= n_old: a window shorter than the step) is not loaded ahead: the chain reads
//     it where it needs it, behind the lane's own store.  The ring positions a group writes and the positions loaded
//     ahead for the next group differ: they could meet only for W <= 2 kSNormAhead - 1, where the entry is this launch's.
// Addresses are formed from i clamped into [0, m) and d clamped into [d0, D).
constexpr int kSNormAhead = 8;

__global__ __launch_bounds__(kWave) void StreamNormKernel(const StreamRec *__restrict__ recs, int D, float *rows, pkmi::StreamNormState st) {
  __shared__ float s_cur[kSNormAhead][kWave], s_old[kSNormAhead][kWave];
  const StreamRec r = recs[blockIdx.x];
  if (r.kind == PK_MI355_FEATS_NORMALIZED || r.m <= 0) return;
  const int lane = threadIdx.x;
  const int d0 = blockIdx.y * kWave;
  const bool live = d0 + lane < D;
  const int d = live ? d0 + lane : d0;
  const bool vars = st.norm_vars != 0;
  const int m = r.m, W = st.window;
  float *x = rows + r.row_off + d;
  double *tot = st.total + (int64_t)r.slot * 2 * D + d;
  double t0s = r.n_old > 0 ? tot[0] : 0.0, t1s = r.n_old > 0 ? tot[D] : 0.0;
  auto row = [&](int i) { return (int64_t)(i < m ? i : m - 1) * D; };
  if (st.mode == PK_MI355_NORM_SPEAKER) {
    const float *tab = st.table + (int64_t)r.slot * 2 * D;
    const float offs = tab[d], scale = tab[D + d];
    float cur[kSNormAhead];
#pragma unroll
    for (int k = 0; k < kSNormAhead; ++k) cur[k] = x[row(k)];
    for (int i0 = 0; i0 < m; i0 += kSNormAhead) {
      float nxt[kSNormAhead];
#pragma unroll
      for (int k = 0; k < kSNormAhead; ++k) nxt[k] = x[row(i0 + kSNormAhead + k)];
#pragma unroll
      for (int k = 0; k < kSNormAhead; ++k)
        if (i0 + k < m) {
          pknorm::StatsAdd(t0s, t1s, cur[k]);
          if (live) x[row(i0 + k)] = pknorm::NormApply(cur[k], offs, scale, vars);
        }
#pragma unroll
      for (int k = 0; k < kSNormAhead; ++k) cur[k] = nxt[k];
    }
    if (live) { tot[0] = t0s; tot[D] = t1s; }
    return;
  }
  const double *rec = st.spk + (int64_t)r.slot * 2 * (D + 1);
  __builtin_assume(rec != nullptr);     // pk_mi355_stream_norm_set_online_cmvn allocates st.spk before any slot runs
  const pknorm::OnlinePrior p =
      pknorm::MakeOnlinePrior(W, st.speaker_frames, st.global_frames, st.global_frames > 0 ? st.glob : nullptr, rec, D, d);
  double *win = st.win + (int64_t)r.slot * 2 * D + d;
  float *rh = st.ring + (int64_t)r.slot * W * D + d;
  double S0 = r.n_old > 0 ? win[0] : 0.0, S1 = r.n_old > 0 ? win[D] : 0.0;
  auto ring = [&](int i) { return (int64_t)((r.n_old + (i < m ? i : m - 1)) % W) * D; };
  // frame t - W of fresh frame i was stored by an earlier launch: its ring entry may be loaded ahead
  auto settled = [&](int i) { return i < m && r.n_old + i >= W && i < W; };
  float cur[kSNormAhead], old[kSNormAhead];
#pragma unroll
  for (int k = 0; k < kSNormAhead; ++k) { cur[k] = x[row(k)]; old[k] = settled(k) ? rh[ring(k)] : 0.0f; }
  for (int i0 = 0; i0 < m; i0 += kSNormAhead) {
#pragma unroll
    for (int k = 0; k < kSNormAhead; ++k) { s_cur[k][lane] = cur[k]; s_old[k][lane] = old[k]; }
#pragma unroll
    for (int k = 0; k < kSNormAhead; ++k) {                          // the next group's loads, ahead of this group's chain
      const int i = i0 + kSNormAhead + k;
      cur[k] = x[row(i)];
      old[k] = settled(i) ? rh[ring(i)] : 0.0f;
    }
    const int n = m - i0 < kSNormAhead ? m - i0 : kSNormAhead;
#pragma unroll 1
    for (int k = 0; k < n; ++k) {
      const int i = i0 + k, t = r.n_old + i;
      const float xt = s_cur[k][lane];
      pknorm::StatsAdd(t0s, t1s, xt);
      if (t >= W) pknorm::WindowStep(S0, S1, xt, i < W ? s_old[k][lane] : rh[ring(i)], true);
      else pknorm::WindowStep(S0, S1, xt, 0.0f, false);                  // (i >= W above: this launch's own store)
      float offs, scale;
      pknorm::OnlineCmvnFinalize(S0, S1, static_cast<double>(t + 1), p, vars, &offs, &scale);
      if (live) {
        rh[ring(i)] = xt;
        x[row(i)] = pknorm::NormApply(xt, offs, scale, vars);
      }
    }
  }
  if (live) { win[0] = S0; win[D] = S1; tot[0] = t0s; tot[D] = t1s; }
}

}  // namespace

// ================================================================== launchers (pk_score.h)

namespace pkmi {

void LaunchStreamNorm(const StreamRec *recs, int n, int dim, float *rows, const StreamNormState &st, hipStream_t stream) {
  if (n <= 0 || dim <= 0) return;
  hipLaunchKernelGGL(StreamNormKernel, dim3(n, (dim + kWave - 1) / kWave), dim3(kWave), 0, stream, recs, dim, rows, st);
}

void LaunchStreamAssemble(const StreamRec *recs, int n, const float *upload, float *tails, float *wave, hipStream_t stream) {
  hipLaunchKernelGGL(StreamAssembleKernel, dim3(n), dim3(256), 0, stream, recs, upload, tails, wave);
}

void LaunchStreamCmvn(const StreamRec *recs, int n, float *rows, const float *g, const CmvnTables *tab, float *sums,
                      float *raw_hist, float *hist, int hist_len, int left, int right, float *yt, int64_t ldy, hipStream_t stream) {
  hipLaunchKernelGGL(StreamCmvnKernel, dim3(n), dim3(kWave), 0, stream, recs, rows, g, tab, sums, raw_hist, hist, hist_len,
                     left, right, yt, ldy);
}

void LaunchStreamRawRows(const StreamRec *recs, int n, const float *upload, float *rows, hipStream_t stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(StreamRawRowsKernel, dim3(n), dim3(256), 0, stream, recs, reinterpret_cast<const uint32_t *>(upload),
                     reinterpret_cast<uint32_t *>(rows));
}

void LaunchStreamCmvnChain(const StreamRec *recs, int n, int dim, float *upload, const float *g, const CmvnTables *tab, float *sums,
                           float *raw_hist, hipStream_t stream) {
  if (n <= 0 || dim <= 0) return;
  hipLaunchKernelGGL(StreamCmvnChainKernel, dim3(n, (dim + kWave - 1) / kWave), dim3(kWave), 0, stream, recs, dim, upload, g, tab, sums,
                     raw_hist);
}

void LaunchStreamFeatureLayout(const StreamRec *recs, int n, int max_cols, const float *upload, float *hist, int hist_len, int dim,
                               int left, int right, float *yt, int64_t ldy, hipStream_t stream) {
  if (n <= 0 || dim <= 0) return;
  // (a slot without rows still has its history written: one tile at least)
  const dim3 grid(max_cols > kSflTile ? (max_cols + kSflTile - 1) / kSflTile : 1, n < 65535 ? n : 65535);
  hipLaunchKernelGGL(StreamFeatureLayoutKernel, grid, dim3(kSflThreads), 0, stream, recs, n, reinterpret_cast<const uint32_t *>(upload),
                     reinterpret_cast<uint32_t *>(hist), hist_len, dim, left, right, reinterpret_cast<uint32_t *>(yt), ldy);
}

}  // namespace pkmi
