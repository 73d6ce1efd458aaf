// norm.hip -- NormKernel: per-utterance and per-speaker mean and variance normalisation of raw rows, Kaldi's
// AccCmvnStats followed by ApplyCmvn (include/pk_mi355.h states the rule).  It takes
// CmvnChainKernel's place (features.hip) in front of FeatureLayoutKernel when a batch scorer has a normalisation spec
// other than the sliding rule.  OnlineCmvnKernel, further down, is Kaldi's online CMVN in the same place (section 20).
//
// Shaped like the chain: one wavefront per (utterance, block of 64 features), lane = feature, so per frame the wave
// reads ONE contiguous run of up to 64 floats.
//   Phase 1 (utterance mode): serial over t, two independent f64 chains per lane (the sum and the sum of squares; a
//     float's square is exact in double, so the order of the adds is all that matters, and it is Kaldi's: t ascending).
//     Frames are taken kNormAhead at a time and the next group's rows are loaded before the current group's adds.  A
//     group's adds take a small part of one memory round trip, so what the wave waits on is the latency of its own
//     loads, and the time falls with the rows it keeps in flight (measured at 8 and 32: DESIGN.md section 19).  The
//     wave writes its sums into the utterance's record
//     [2][D + 1]; the block that holds feature 0 also writes the count and the 0 behind the sums of squares.
//   Phase 2: pknorm::NormFinalize per lane, the host's lines (pk_norm.h) -- a double divide and sqrt, which give the
//     host's bits here (tail.hip relies on the same).  Speaker mode reads the finalised float table instead.
//   Phase 3: the utterance's rows again (they are in L2 for all but the longest utterances), normalised rows out.
// Never in place: the caller keeps the raw rows (fetch_fbank).
// Every address is formed from t clamped into [0, T) and d clamped into [d0, D): a load past the utterance's rows or
// past feature D - 1 is never issued, so a poisoned neighbour is never read; a lane past D shadows the block's first
// feature and stores nothing.
#include <hip/hip_runtime.h>

#include "pk_norm_kernel.h"

namespace pkmi {

namespace {

constexpr int kNormAhead = 32;     // rows in flight per wave: the loops wait on memory latency, not on their adds

__global__ __launch_bounds__(64) void NormKernel(const float *__restrict__ raw, UttLayout utts, int num_utts, int D, int mode,
                                                 int norm_means, int norm_vars, const float *__restrict__ table,
                                                 double *__restrict__ stats, float *__restrict__ out) {
  const int d0 = blockIdx.x * 64;
  const bool live = d0 + (int)threadIdx.x < D;
  const int d = live ? d0 + threadIdx.x : d0;
  const bool vars = norm_vars != 0;
  for (int u = blockIdx.y; u < num_utts; u += gridDim.y) {          // (uniform over the wave)
    const int T = utts.num_frames[u];
    double *rec = stats + (int64_t)u * 2 * (D + 1);                 // (formed, not touched, in speaker mode)
    if (T <= 0) {
      if (mode == PK_MI355_NORM_UTTERANCE) {                        // the record of no frames: zeros
        if (live) { rec[d] = 0.0; rec[D + 1 + d] = 0.0; }
        if (d0 == 0 && threadIdx.x == 0) { rec[D] = 0.0; rec[2 * D + 1] = 0.0; }
      }
      continue;
    }
    const float *x = raw + utts.raw_base[u] * D + d;
    float *y = out + utts.raw_base[u] * D + d;
    auto row = [&](int t) { return (int64_t)(t < T ? t : T - 1) * D; };
    float cur[kNormAhead], nxt[kNormAhead];
    float offs, scale;
    if (mode == PK_MI355_NORM_UTTERANCE) {
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int k = 0; k < kNormAhead; ++k) cur[k] = x[row(k)];
      for (int t0 = 0; t0 < T; t0 += kNormAhead) {
#pragma unroll
        for (int k = 0; k < kNormAhead; ++k) nxt[k] = x[row(t0 + kNormAhead + k)];     // ahead of this group's adds
#pragma unroll
        for (int k = 0; k < kNormAhead; ++k)
          if (t0 + k < T) pknorm::StatsAdd(s0, s1, cur[k]);
#pragma unroll
        for (int k = 0; k < kNormAhead; ++k) cur[k] = nxt[k];
      }
      if (live) { rec[d] = s0; rec[D + 1 + d] = s1; }
      if (d0 == 0 && threadIdx.x == 0) { rec[D] = static_cast<double>(T); rec[2 * D + 1] = 0.0; }
      pknorm::NormFinalize(s0, s1, static_cast<double>(T), norm_means != 0, vars, &offs, &scale);
    } else {
      const float *tab = table + (int64_t)u * 2 * D;
      offs = tab[d];
      scale = tab[D + d];
    }
#pragma unroll
    for (int k = 0; k < kNormAhead; ++k) cur[k] = x[row(k)];
    for (int t0 = 0; t0 < T; t0 += kNormAhead) {
#pragma unroll
      for (int k = 0; k < kNormAhead; ++k) nxt[k] = x[row(t0 + kNormAhead + k)];
#pragma unroll
      for (int k = 0; k < kNormAhead; ++k)
        if (live && t0 + k < T) y[(int64_t)(t0 + k) * D] = pknorm::NormApply(cur[k], offs, scale, vars);
#pragma unroll
      for (int k = 0; k < kNormAhead; ++k) cur[k] = nxt[k];
    }
  }
}

// OnlineCmvnKernel: Kaldi's OnlineCmvn over whole utterances (include/pk_mi355.h states the rule; DESIGN.md section
// 20).  The same shape: one wavefront per (utterance, block of 64 features), lane = feature, serial over t.  Per frame
// a lane adds x[t] to its two f64 window sums, takes x[t - W] out of them (after the additions), and runs the host's
// pknorm::OnlineCmvnFinalize -- the smoothing by the speaker's and the global record while the window is not full,
// then NormFinalize -- and NormApply.  Rows t and t - W are loaded a group of kNormAhead frames ahead of the chain,
// into registers, and handed to the chain through LDS: every lane writes and reads its own column of the two
// [kNormAhead][64] arrays only, so the wave needs no barrier, and the chain's loop stays rolled (the finalisation
// holds several f64 divisions and a square root; kNormAhead unrolled copies of it would not fit the instruction cache).
// Never in place: frame t - W is read raw.  Addresses are clamped as in NormKernel; the records are read at d < D.
// The prior fill and the window step restate pknorm::MakeOnlinePrior and WindowStep (pk_norm.h).
__global__ __launch_bounds__(64) void OnlineCmvnKernel(const float *__restrict__ raw, UttLayout utts, int num_utts, int D, int W,
                                                       int speaker_frames, int global_frames, int norm_vars,
                                                       const double *__restrict__ glob, const double *__restrict__ spk,
                                                       float *__restrict__ out) {
  __shared__ float s_cur[kNormAhead][64], s_old[kNormAhead][64];
  const int lane = threadIdx.x;
  const int d0 = blockIdx.x * 64;
  const bool live = d0 + lane < D;
  const int d = live ? d0 + lane : d0;
  const bool vars = norm_vars != 0;
  pknorm::OnlinePrior p;
  p.window = static_cast<double>(W);
  p.speaker_frames = static_cast<double>(speaker_frames);
  p.global_frames = glob ? static_cast<double>(global_frames) : 0.0;
  p.global_count = glob ? glob[D] : 0.0;
  p.glob0 = glob ? glob[d] : 0.0;
  p.glob1 = glob ? glob[D + 1 + d] : 0.0;
  for (int u = blockIdx.y; u < num_utts; u += gridDim.y) {          // (uniform over the wave)
    const int T = utts.num_frames[u];
    if (T <= 0) continue;
    const double *rec = spk ? spk + (int64_t)u * 2 * (D + 1) : nullptr;
    p.speaker_count = rec ? rec[D] : 0.0;
    p.spk0 = rec ? rec[d] : 0.0;
    p.spk1 = rec ? rec[D + 1 + d] : 0.0;
    const float *x = raw + utts.raw_base[u] * D + d;
    float *y = out + utts.raw_base[u] * D + d;
    auto row = [&](int t) { return (int64_t)(t < 0 ? 0 : t < T ? t : T - 1) * D; };
    float cur[kNormAhead], old[kNormAhead];
#pragma unroll
    for (int k = 0; k < kNormAhead; ++k) { cur[k] = x[row(k)]; old[k] = x[row(k - W)]; }
    double S0 = 0.0, S1 = 0.0;
    for (int t0 = 0; t0 < T; t0 += kNormAhead) {
#pragma unroll
      for (int k = 0; k < kNormAhead; ++k) { s_cur[k][lane] = cur[k]; s_old[k][lane] = old[k]; }
#pragma unroll
      for (int k = 0; k < kNormAhead; ++k) {                         // the next group, ahead of this group's chain
        cur[k] = x[row(t0 + kNormAhead + k)];
        old[k] = x[row(t0 + kNormAhead + k - W)];
      }
      const int n = T - t0 < kNormAhead ? T - t0 : kNormAhead;
#pragma unroll 1
      for (int k = 0; k < n; ++k) {
        const int t = t0 + k;
        const float xt = s_cur[k][lane];
        const double v = static_cast<double>(xt);
        S0 = S0 + v;
        S1 = S1 + v * v;
        if (t >= W) {
          const double o = static_cast<double>(s_old[k][lane]);
          S0 = S0 - o;
          S1 = S1 - o * o;
        }
        float offs, scale;
        pknorm::OnlineCmvnFinalize(S0, S1, static_cast<double>(t + 1), p, vars, &offs, &scale);
        if (live) y[(int64_t)t * D] = pknorm::NormApply(xt, offs, scale, vars);
      }
    }
  }
}

}  // namespace

void LaunchOnlineCmvn(const float *raw, const UttLayout &utts, int num_utts, int dim, const pk_mi355_online_cmvn_spec_t &spec,
                      const double *glob, const double *spk, float *out, hipStream_t stream) {
  if (num_utts <= 0 || dim <= 0) return;
  const dim3 grid((dim + 63) / 64, num_utts < 65535 ? num_utts : 65535);
  hipLaunchKernelGGL(OnlineCmvnKernel, grid, dim3(64), 0, stream, raw, utts, num_utts, dim, spec.cmn_window, spec.speaker_frames,
                     spec.global_frames, spec.norm_vars, spec.global_frames > 0 ? glob : nullptr, spk, out);
}

void LaunchNorm(const float *raw, const UttLayout &utts, int num_utts, int dim, int mode, bool norm_means, bool norm_vars,
                const float *table, double *stats, float *out, hipStream_t stream) {
  if (num_utts <= 0 || dim <= 0) return;
  const dim3 grid((dim + 63) / 64, num_utts < 65535 ? num_utts : 65535);
  hipLaunchKernelGGL(NormKernel, grid, dim3(64), 0, stream, raw, utts, num_utts, dim, mode, norm_means ? 1 : 0, norm_vars ? 1 : 0, table,
                     stats, out);
}

}  // namespace pkmi
