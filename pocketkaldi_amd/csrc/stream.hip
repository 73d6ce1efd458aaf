// stream.hip -- the online scorer (pk_mi355_stream_*): live PCM pushed in chunks per slot, and every step scores, for
// every slot, the frames that became final since the last step.  Host C++ over the HIP runtime, and the kernels that
// carry a slot's state from one step to the next.
//
// The reference pipeline is causal: frame t of fbank reads samples [160 t, 160 t + 400) only
// (fbank.cc:35-42, 193-245); online CMVN (cmvn.cc:35-71) is a running window sum rounded to float after every frame,
// so that float vector and the raw frames still inside the 600-frame window are its whole state; the splice
// (am.cc:65-88) needs R frames of look-ahead and clamps at frame 0 and at the last frame only.  Every frame's
// log-likelihoods therefore equal the whole-utterance batch scorer's, bit for bit, whatever the chunk sizes.
//
// One step:
//   1. StreamAssembleKernel: each slot's segment (the samples it carried from earlier steps, then those pushed since)
//      into the wave staging, one "utterance" of the UttLayout; the samples past the step's last frame become the
//      slot's carried tail (two buffers per slot, used in turn).
//   2. FbankKernel (LaunchFbank), unchanged: raw frames n_old .. n_old + m - 1 of every slot.
//   3. StreamCmvnKernel: the CMVN chain continued from the carried window sum at the global frame index, the new
//      frames into the slot's raw history; then the first layer's feature-major operand for the rows being scored,
//      with the real neighbouring frames (edge replication only at frame 0 and, once closed, at the last frame).
//   4. RunLayers (fp32), rows laid out slot after slot, the first layer's column shift >= 0 by construction.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "pk_host.h"

using namespace pkmi;
using namespace pkhost;

namespace {

constexpr int kWave = 64;
constexpr int kTailCap = kFrameLength;     // a carried tail holds at most 399 samples (fewer than one frame's 400)

// One slot's share of a step (device array, one entry per slot taking part).
struct StreamRec {
  int32_t slot;
  int32_t tail_len;    // samples carried from earlier steps (global samples 160 n_old ...)
  int32_t new_len;     // samples pushed since the last step
  int32_t tail_par;    // the slot's tail buffer that holds the carried samples (the step writes the other one)
  int32_t n_old;       // CMVN frames computed before this step
  int32_t m;           // frames this step computes: n_old .. n_old + m - 1
  int32_t a, b;        // rows scored: frames [a, b)
  int32_t closed;      // 1: the right edge is the last frame (am.cc:73-75)
  int32_t cols;        // columns of the slot's region of Yt: RoundUp(b - a, 4) + L + R (0: no rows)
  int64_t woff;        // first sample of the segment in the wave staging
  int64_t new_off;     // first pushed sample in the upload staging
  int64_t raw_base;    // first row of the slot's new frames in the step's raw rows
  int64_t col_base;    // first column of the slot's region of Yt
};

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

enum SlotState { kFree = 0, kOpen = 1, kClosed = 2 };

struct Slot {
  int state = kFree;
  int n = 0;               // CMVN frames computed
  int a = 0;               // frames scored (the next row to score)
  int tail_len = 0;
  int tail_par = 0;
  std::vector<float> pending;   // pushed since the last step
  // the last step's rows of this slot
  int last_first = 0, last_count = 0;
  int64_t last_out = 0;
  bool last_flushed = false;     // the last step was the slot's final one
};

}  // namespace

struct pk_mi355_stream {
  pk_mi355_am *am = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  int max_streams = 0;
  int64_t max_step_samples = 0;
  int64_t pending_total = 0;
  std::vector<Slot> slots;
  int hist_len = 1;                   // max(L + R, 1)
  int64_t max_frames = 0, max_rows = 0, max_cols = 0, chunk = 0, zero_span = 0, ldy = 0, wave_cap = 0;
  FrontendTables *d_tables = nullptr;
  float *d_global = nullptr;
  CmvnTables *d_cmvn_tab = nullptr;
  // per-slot state in HBM
  float *d_tails = nullptr;           // [slots][2][kTailCap]
  float *d_sums = nullptr;            // [slots][40]
  float *d_raw_hist = nullptr;        // [slots][600][40]
  float *d_hist = nullptr;            // [slots][hist_len][40]
  // per-step staging
  float *h_upload = nullptr, *d_upload = nullptr;    // pushed samples, page-locked -> HBM
  float *d_wave = nullptr;            // segments
  float *d_rows = nullptr;            // raw -> CMVN'd rows of the step's new frames
  char *h_meta = nullptr, *d_meta = nullptr;          // records, UttLayout arrays, column shifts
  size_t meta_bytes = 0;
  float *d_yt = nullptr;              // [40][ldy]
  float *d_ll = nullptr;              // [max_cols][num_pdfs]
  ExecBufs exec;
  hipEvent_t ev_staged = nullptr;     // the last step's uploads have left the page-locked buffers
  bool staged = false;
};

namespace {

int SlotIndex(const pk_mi355_stream *s, int slot) {
  if (!s) return Fail(PK_MI355_E_INVALID, "null stream");
  if (slot < 0 || slot >= s->max_streams) return Fail(PK_MI355_E_INVALID, "slot %d out of range [0, %d)", slot, s->max_streams);
  return 0;
}

}  // namespace

namespace pkhost {
const pk_mi355_am *StreamModel(const pk_mi355_stream *s) { return s->am; }
int StreamSlots(const pk_mi355_stream *s) { return s->max_streams; }
hipStream_t StreamHipStream(const pk_mi355_stream *s) { return s->stream; }
const float *StreamLoglikBase(const pk_mi355_stream *s) { return s->d_ll; }
bool StreamSlotFlushed(const pk_mi355_stream *s, int slot) { return slot >= 0 && slot < s->max_streams && s->slots[slot].last_flushed; }
}  // namespace pkhost

extern "C" {

pk_mi355_stream_t *pk_mi355_stream_create(pk_mi355_am_t *am, const float *global_stats41, int max_streams,
                                          int64_t max_step_samples) {
  if (!am) { Fail(PK_MI355_E_INVALID, "null model"); return nullptr; }
  if (am->precision != PK_MI355_PRECISION_F32) {
    Fail(PK_MI355_E_INVALID, "the online scorer runs f32 models only (the f16 modes' calibration and range verdict are per batch)");
    return nullptr;
  }
  if (!am->finalized) { Fail(PK_MI355_E_STATE, "model not finalized"); return nullptr; }
  if (am->feat_dim != kNumBins) { Fail(PK_MI355_E_INVALID, "the front-end produces %d-dim features, the model expects %d", kNumBins, am->feat_dim); return nullptr; }
  if (!global_stats41 || max_streams <= 0 || max_step_samples <= 0 || max_step_samples > (int64_t)1 << 30) {
    Fail(PK_MI355_E_INVALID, "bad stream capacity");
    return nullptr;
  }
  if (UseDevice(am->device)) return nullptr;
  pk_mi355_stream *s = new pk_mi355_stream();
  s->am = am;
  s->device = am->device;
  s->max_streams = max_streams;
  s->max_step_samples = max_step_samples;
  s->slots.resize(max_streams);
  const int pad = am->left + am->right;
  s->hist_len = std::max(pad, 1);
  // a slot's segment holds at most 399 carried samples and its pushes; its rows are its new frames and the (at most R)
  // frames held back for look-ahead, padded to four
  s->wave_cap = max_step_samples + (int64_t)max_streams * kTailCap;
  s->max_frames = s->wave_cap / kFrameShift + max_streams;
  s->max_rows = s->max_frames + (int64_t)max_streams * (am->right + 3);
  s->max_cols = RoundUp(s->max_rows + (int64_t)max_streams * pad, kTileF16);
  s->chunk = std::min<int64_t>(262144, s->max_cols);
  s->zero_span = RoundUp((int64_t)max_streams * pad + 2 * kTile, 256);
  s->ldy = RoundUp(s->max_cols, s->chunk) + 256 + s->zero_span;
  const int64_t groups = s->max_cols / 4 + kTileF16;
  s->meta_bytes = RoundUp(sizeof(StreamRec) * max_streams, 256) + RoundUp((sizeof(int64_t) * 2 + sizeof(int32_t)) * max_streams, 256) +
                  sizeof(int32_t) * groups;
  FrontendTables host;
  bool ok = BuildFrontendTables(&host) == 0;
  auto chk = [&](hipError_t e) { if (e != hipSuccess && ok) { ok = false; Fail(PK_MI355_E_DEVICE, "stream_create: %s", hipGetErrorString(e)); } };
  if (!ok) Fail(PK_MI355_E_INVALID, "front-end table construction failed");
  chk(hipStreamCreate(&s->stream));
  chk(hipEventCreateWithFlags(&s->ev_staged, hipEventDisableTiming));
  chk(hipMalloc(&s->d_tables, sizeof(FrontendTables)));
  if (ok) chk(hipMemcpy(s->d_tables, &host, sizeof(FrontendTables), hipMemcpyHostToDevice));
  chk(hipMalloc(&s->d_global, sizeof(float) * (kNumBins + 1)));
  if (ok) chk(hipMemcpy(s->d_global, global_stats41, sizeof(float) * (kNumBins + 1), hipMemcpyHostToDevice));
  CmvnTables ctab;
  BuildCmvnTables(global_stats41[kNumBins], &ctab);
  chk(hipMalloc(&s->d_cmvn_tab, sizeof(CmvnTables)));
  if (ok) chk(hipMemcpy(s->d_cmvn_tab, &ctab, sizeof(CmvnTables), hipMemcpyHostToDevice));
  chk(hipMalloc(&s->d_tails, sizeof(float) * max_streams * 2 * kTailCap));
  chk(hipMalloc(&s->d_sums, sizeof(float) * max_streams * kNumBins));
  chk(hipMalloc(&s->d_raw_hist, sizeof(float) * max_streams * kCmvnWindow * kNumBins));
  chk(hipMalloc(&s->d_hist, sizeof(float) * max_streams * s->hist_len * kNumBins));
  chk(hipHostMalloc(reinterpret_cast<void **>(&s->h_upload), sizeof(float) * max_step_samples, hipHostMallocDefault));
  chk(hipMalloc(&s->d_upload, sizeof(float) * max_step_samples));
  chk(hipMalloc(&s->d_wave, sizeof(float) * s->wave_cap));
  chk(hipMalloc(&s->d_rows, sizeof(float) * s->max_frames * kNumBins));
  chk(hipHostMalloc(reinterpret_cast<void **>(&s->h_meta), s->meta_bytes, hipHostMallocDefault));
  chk(hipMalloc(&s->d_meta, s->meta_bytes));
  chk(hipMalloc(&s->d_yt, sizeof(float) * s->ldy * kNumBins));
  if (ok) chk(hipMemset(s->d_yt, 0, sizeof(float) * s->ldy * kNumBins));   // the zero span at the end of feature row 0
  chk(hipMalloc(&s->d_ll, sizeof(float) * s->max_cols * am->num_pdfs));
  if (ok && AllocExec(am, s->chunk, &s->exec)) ok = false;
  if (!ok) { pk_mi355_stream_destroy(s); return nullptr; }
  return s;
}

void pk_mi355_stream_destroy(pk_mi355_stream_t *s) {
  if (!s) return;
  hipSetDevice(s->device);
  if (s->stream) hipStreamSynchronize(s->stream);
  FreeExec(&s->exec);
  hipFree(s->d_tables); hipFree(s->d_global); hipFree(s->d_cmvn_tab);
  hipFree(s->d_tails); hipFree(s->d_sums); hipFree(s->d_raw_hist); hipFree(s->d_hist);
  hipFree(s->d_upload); hipFree(s->d_wave); hipFree(s->d_rows); hipFree(s->d_meta); hipFree(s->d_yt); hipFree(s->d_ll);
  if (s->h_upload) hipHostFree(s->h_upload);
  if (s->h_meta) hipHostFree(s->h_meta);
  if (s->ev_staged) hipEventDestroy(s->ev_staged);
  if (s->stream) hipStreamDestroy(s->stream);
  delete s;
}

int pk_mi355_stream_open(pk_mi355_stream_t *s, int slot) {
  int rc = SlotIndex(s, slot);
  if (rc) return rc;
  Slot &z = s->slots[slot];
  if (z.state != kFree) return Fail(PK_MI355_E_STATE, "slot %d is %s", slot, z.state == kOpen ? "open" : "closed and not yet flushed by a step");
  z.state = kOpen;
  z.n = z.a = z.tail_len = 0;
  z.pending.clear();
  return 0;
}

int pk_mi355_stream_push(pk_mi355_stream_t *s, int slot, const float *samples, int num_samples) {
  int rc = SlotIndex(s, slot);
  if (rc) return rc;
  Slot &z = s->slots[slot];
  if (z.state != kOpen) return Fail(PK_MI355_E_STATE, "slot %d is not open", slot);
  if (num_samples < 0 || (num_samples > 0 && !samples)) return Fail(PK_MI355_E_INVALID, "bad samples");
  if (s->pending_total + num_samples > s->max_step_samples)
    return Fail(PK_MI355_E_INVALID, "push of %d samples exceeds the step capacity (%lld pending of %lld)", num_samples,
                (long long)s->pending_total, (long long)s->max_step_samples);
  z.pending.insert(z.pending.end(), samples, samples + num_samples);
  s->pending_total += num_samples;
  return 0;
}

int pk_mi355_stream_push_i16(pk_mi355_stream_t *s, int slot, const int16_t *samples, int num_samples) {
  int rc = SlotIndex(s, slot);
  if (rc) return rc;
  if (num_samples < 0 || (num_samples > 0 && !samples)) return Fail(PK_MI355_E_INVALID, "bad samples");
  std::vector<float> f(samples, samples + num_samples);    // exact: 16-bit integers
  return pk_mi355_stream_push(s, slot, f.data(), num_samples);
}

int pk_mi355_stream_close(pk_mi355_stream_t *s, int slot) {
  int rc = SlotIndex(s, slot);
  if (rc) return rc;
  Slot &z = s->slots[slot];
  if (z.state != kOpen) return Fail(PK_MI355_E_STATE, "slot %d is not open", slot);
  z.state = kClosed;
  return 0;
}

int pk_mi355_stream_step(pk_mi355_stream_t *s, float prob_scale, int sync) {
  if (!s) return Fail(PK_MI355_E_INVALID, "null stream");
  int rc = UseDevice(s->device);
  if (rc) return rc;
  pk_mi355_am *am = s->am;
  const int L = am->left, R = am->right, pad = L + R, N = am->num_pdfs;
  bool any = false;
  for (const Slot &z : s->slots) any = any || z.state != kFree;
  if (!any) return Fail(PK_MI355_E_STATE, "step with no open slot");
  if (s->staged) HIP_TRY(hipEventSynchronize(s->ev_staged));   // the page-locked staging is free again
  s->staged = false;
  for (Slot &z : s->slots) { z.last_count = 0; z.last_flushed = false; }   // a step's rows are readable until the next step
  // ---- the step's plan, on the host
  StreamRec *recs = reinterpret_cast<StreamRec *>(s->h_meta);
  char *lay_base = s->h_meta + RoundUp(sizeof(StreamRec) * s->max_streams, 256);
  std::vector<int> who, flushed;                      // slots taking part; closed slots with nothing left
  int64_t woff = 0, upl = 0, raw = 0, out = 0, col = 0;
  int max_m = 0;
  int32_t shift = 0;
  std::vector<std::pair<int64_t, int32_t>> spans;    // (end row, column shift) per slot with rows
  for (int slot = 0; slot < s->max_streams; ++slot) {
    const Slot &z = s->slots[slot];
    if (z.state == kFree) continue;
    const bool closed = z.state == kClosed;
    const int new_len = (int)z.pending.size();
    const int seg = z.tail_len + new_len;
    const int m = pk_mi355_num_frames(seg);
    const int n = z.n + m;
    const int b = closed ? n : std::max(z.a, n - R);    // open: R frames of look-ahead held back
    if (new_len == 0 && m == 0 && b == z.a) {
      if (closed) flushed.push_back(slot);
      continue;
    }
    StreamRec &r = recs[who.size()];
    r.slot = slot; r.tail_len = z.tail_len; r.new_len = new_len; r.tail_par = z.tail_par;
    r.n_old = z.n; r.m = m; r.a = z.a; r.b = b; r.closed = closed ? 1 : 0;
    r.woff = woff; r.new_off = upl; r.raw_base = raw;
    r.col_base = 0; r.cols = 0;
    if (b > z.a) {
      // Rows slot after slot, each padded to four; the slot's columns a - L .. b + R - 1 in a region of RoundUp(b - a, 4)
      // + L + R columns.  The column of row j is j + (the number of earlier slots with rows) x (L + R): never negative.
      // (The batch scorer's compact rows pad the rows but not the columns: their shift goes negative when L + R < 3.)
      shift = (int32_t)(col - out);
      if (shift < 0 || shift + kTile > s->zero_span)
        return Fail(PK_MI355_E_INVALID, "internal: column shift %d outside [0, %lld]", shift, (long long)(s->zero_span - kTile));
      r.col_base = col;
      r.cols = (int)RoundUp(b - z.a, 4) + pad;
      out += RoundUp(b - z.a, 4);
      col += r.cols;
      spans.push_back({out, shift});
    }
    woff += seg; upl += new_len; raw += m;
    max_m = std::max(max_m, m);
    who.push_back(slot);
  }
  if (woff > s->wave_cap || raw > s->max_frames || RoundUp(out, kTileF16) > s->max_cols || col > s->max_cols)
    return Fail(PK_MI355_E_INVALID, "internal: step exceeds the stream's capacity");
  // the plan holds: consume every pushed sample, advance the slots
  for (size_t k = 0; k < who.size(); ++k) {
    const StreamRec &r = recs[k];
    Slot &z = s->slots[r.slot];
    if (r.new_len) memcpy(s->h_upload + r.new_off, z.pending.data(), sizeof(float) * r.new_len);
    z.pending.clear();
    z.tail_len = r.tail_len + r.new_len - kFrameShift * r.m;
    z.tail_par ^= 1;
    z.n = r.n_old + r.m;
    z.a = r.b;
    z.last_first = r.a; z.last_count = r.b - r.a;
    if (z.state == kClosed) { z.state = kFree; z.last_flushed = true; }   // flushed: the slot may be opened again
  }
  for (int slot : flushed) { s->slots[slot].state = kFree; s->slots[slot].last_flushed = true; }
  s->pending_total = 0;
  {
    int64_t o = 0;
    for (size_t k = 0; k < who.size(); ++k) {
      Slot &z = s->slots[recs[k].slot];
      z.last_out = o;
      o += RoundUp(z.last_count, 4);
    }
  }
  const int K = (int)who.size();
  if (K == 0) return sync ? pk_mi355_stream_synchronize(s) : 0;
  // UttLayout arrays and the column shift of every group of four rows (the groups past the last row keep the last shift)
  int64_t *h_woff = reinterpret_cast<int64_t *>(lay_base);
  int64_t *h_rawb = h_woff + s->max_streams;
  int32_t *h_T = reinterpret_cast<int32_t *>(h_rawb + s->max_streams);
  int32_t *h_shift4 = reinterpret_cast<int32_t *>(s->h_meta + (s->meta_bytes - sizeof(int32_t) * (s->max_cols / 4 + kTileF16)));
  for (int k = 0; k < K; ++k) { h_woff[k] = recs[k].woff; h_rawb[k] = recs[k].raw_base; h_T[k] = recs[k].m; }
  const int64_t total_rows = out;
  const int64_t groups = total_rows > 0 ? RoundUp(total_rows, kTileF16) / 4 + kTileF16 / 4 : 0;
  {
    int64_t g = 0;
    for (const auto &sp : spans)
      for (; g < sp.first / 4; ++g) h_shift4[g] = sp.second;
    for (; g < groups; ++g) h_shift4[g] = shift;
  }
  // ---- uploads (one for the samples, one for the plan) and the launches, all on the stream
  if (upl) HIP_TRY(hipMemcpyAsync(s->d_upload, s->h_upload, sizeof(float) * upl, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(s->d_meta, s->h_meta, s->meta_bytes, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipEventRecord(s->ev_staged, s->stream));
  s->staged = true;
  const StreamRec *d_recs = reinterpret_cast<const StreamRec *>(s->d_meta);
  const char *d_lay = s->d_meta + (lay_base - s->h_meta);
  const int64_t *d_woff = reinterpret_cast<const int64_t *>(d_lay);
  const int64_t *d_rawb = d_woff + s->max_streams;
  const int32_t *d_T = reinterpret_cast<const int32_t *>(d_rawb + s->max_streams);
  const int32_t *d_shift4 = reinterpret_cast<const int32_t *>(s->d_meta + (s->meta_bytes - sizeof(int32_t) * (s->max_cols / 4 + kTileF16)));
  hipLaunchKernelGGL(StreamAssembleKernel, dim3(K), dim3(256), 0, s->stream, d_recs, s->d_upload, s->d_tails, s->d_wave);
  UttLayout lay{d_woff, d_T, d_rawb, d_rawb};
  LaunchFbank(s->d_wave, nullptr, lay, K, max_m, s->d_tables, s->d_rows, s->stream);
  hipLaunchKernelGGL(StreamCmvnKernel, dim3(K), dim3(kWave), 0, s->stream, d_recs, s->d_rows, s->d_global, s->d_cmvn_tab,
                     s->d_sums, s->d_raw_hist, s->d_hist, s->hist_len, L, R, s->d_yt, s->ldy);
  for (int64_t c0 = 0; c0 < total_rows; c0 += s->chunk) {
    const int rows = (int)std::min<int64_t>(s->chunk, total_rows - c0);
    rc = RunLayers(am, s->exec, s->d_yt + c0, s->ldy, kNumBins, rows, true, prob_scale, s->d_ll + c0 * N, N, s->stream,
                   nullptr, nullptr, s->d_yt + (s->ldy - s->zero_span), d_shift4 + c0 / 4);
    if (rc) return rc;
  }
  hipError_t le = hipGetLastError();
  if (le != hipSuccess) return Fail(PK_MI355_E_DEVICE, "stream step launch failed: %s", hipGetErrorString(le));
  if (sync) return pk_mi355_stream_synchronize(s);
  return 0;
}

int pk_mi355_stream_synchronize(pk_mi355_stream_t *s) {
  if (!s) return Fail(PK_MI355_E_INVALID, "null stream");
  HIP_TRY(hipStreamSynchronize(s->stream));
  return 0;
}

const float *pk_mi355_stream_loglik_device(const pk_mi355_stream_t *s, int slot, int *first_frame, int *count) {
  if (first_frame) *first_frame = 0;
  if (count) *count = 0;
  if (SlotIndex(s, slot)) return nullptr;
  const Slot &z = s->slots[slot];
  if (first_frame) *first_frame = z.last_first;
  if (count) *count = z.last_count;
  return z.last_count > 0 ? s->d_ll + z.last_out * s->am->num_pdfs : nullptr;
}

int pk_mi355_stream_fetch(pk_mi355_stream_t *s, int slot, pk_decodable_t *out, int *first_frame) {
  int rc = SlotIndex(s, slot);
  if (rc) return rc;
  if (!out) return Fail(PK_MI355_E_INVALID, "null decodable");
  if ((rc = UseDevice(s->device))) return rc;
  int count = 0, first = 0;
  const float *src = pk_mi355_stream_loglik_device(s, slot, &first, &count);
  const int N = s->am->num_pdfs;
  if (first_frame) *first_frame = first;
  out->am = s->am;
  out->log_prob.ncol = 0; out->log_prob.nrow = 0; out->log_prob.data = nullptr;
  if (count == 0) return 0;
  float *host = static_cast<float *>(malloc(sizeof(float) * (size_t)count * N));
  if (!host) return Fail(PK_MI355_E_INVALID, "out of host memory");
  hipError_t e = hipMemcpyAsync(host, src, sizeof(float) * (size_t)count * N, hipMemcpyDeviceToHost, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) { free(host); return Fail(PK_MI355_E_DEVICE, "stream fetch: %s", hipGetErrorString(e)); }
  out->log_prob.ncol = count; out->log_prob.nrow = N; out->log_prob.data = host;
  return 0;
}

}  // extern "C"
