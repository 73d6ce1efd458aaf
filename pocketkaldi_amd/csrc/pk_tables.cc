// pk_tables.cc -- host construction of the front-end constant tables and of the resampler's polyphase table.
// Compile: g++ -O2 -ffp-contract=off (no -march): float expressions must round
// exactly where the reference's do.  See pk_tables.h / pk_resample.h for what each table is.
#include "pk_tables.h"
#include "pk_files.h"
#include "pk_frontend.h"
#include "pk_logf.h"
#include "pk_resample.h"

#include <math.h>
#include <cmath>
#include <string.h>

#include <algorithm>
#include <vector>

namespace pkmi {

namespace {

// srfft.cc:37-39 full-precision 2*pi; fbank.cc:18-20 truncated 2*pi.
const double kTwoPiFull = 6.283185307179586476925286766559005;
const double kTwoPiTrunc = 6.28318530718;

struct Block { int off, logm; };

// srfft.cc:224-237: a transform of 2^logm points at `off` recurses into
// (off, logm-1), (off + m/2, logm-2), (off + 3m/4, logm-2).
void Enumerate(int off, int logm, std::vector<Block> *out) {
  if (logm <= 0) return;
  out->push_back({off, logm});
  if (logm >= 2) {
    int m = 1 << logm;
    Enumerate(off, logm - 1, out);
    Enumerate(off + m / 2, logm - 2, out);
    Enumerate(off + 3 * (m / 4), logm - 2, out);
  }
}

float MelScale(float freq) {  // fbank.h:30-32
  return 1127.0f * logf(1.0f + freq / 700.0f);
}

}  // namespace

int BuildFrontendTables(FrontendTables *t) {
  memset(t, 0, sizeof(*t));
  static const double logf_tab[kLogfTableDoubles] = PK_LOGF_TABLE_INIT;
  memcpy(t->logf_tab, logf_tab, sizeof(logf_tab));

  // ---- Hamming window, fbank.cc:249-256 (float angle step, float cos, the
  // 0.54 - 0.46 * c expression in double, one rounding to float)
  float a = kTwoPiTrunc / (kFrameLength - 1);
  for (int i = 0; i < kFrameLength; ++i) {
    float i_fl = static_cast<float>(i);
    t->window[i] = 0.54 - 0.46 * cosf(a * i_fl);
  }

  // ---- split-radix block schedule
  std::vector<Block> blocks;
  Enumerate(0, kLogCplx, &blocks);
  std::stable_sort(blocks.begin(), blocks.end(), [](const Block &x, const Block &y) {
    return x.logm != y.logm ? x.logm > y.logm : x.off < y.off;
  });
  if (static_cast<int>(blocks.size()) > kMaxBlocks) return -1;
  int pos = 0;
  for (int p = 0; p < kNumPasses; ++p) {
    int logm = kLogCplx - p;
    t->pass_start[p] = pos;
    for (const Block &b : blocks)
      if (b.logm == logm) t->blk_off[pos++] = b.off;
  }
  t->pass_start[kNumPasses] = pos;

  // ---- butterfly coefficient tables, srfft.cc:64-91
  int woff = 0;
  for (int logm = 4; logm <= kLogCplx; ++logm) {
    int m = 1 << logm, m4 = m / 4, m8 = m / 8;
    t->tw_off[logm] = woff;
    float *base = t->tw + woff;
    for (int n = 1; n < m4; ++n) {
      if (n == m8) continue;
      float ang = n * kTwoPiFull / m;
      float c = cosf(ang), s = sinf(ang);
      base[0 * m4 + n] = c;
      base[1 * m4 + n] = -(s + c);
      base[2 * m4 + n] = s - c;
      ang = 3 * n * kTwoPiFull / m;
      c = cosf(ang);
      s = sinf(ang);
      base[3 * m4 + n] = c;
      base[4 * m4 + n] = -(s + c);
      base[5 * m4 + n] = s - c;
    }
    woff += 6 * m4;
  }
  if (woff != kTwFloats) return -2;

  // ---- bit reversal (what srfft.cc:239-265 realises)
  for (int i = 0; i < kFftCplx; ++i) {
    int r = 0, v = i;
    for (int bit = 0; bit < kLogCplx; ++bit) { r = (r << 1) | (v & 1); v >>= 1; }
    t->bitrev[i] = r;
  }

  // ---- real post-pass twiddle, srfft.cc:384-394: iterated float complex product
  float ang1 = static_cast<float>(kTwoPiFull / kFftSize * -1);
  float root_re = cosf(ang1), root_im = sinf(ang1);
  float kre = 1.0f, kim = 0.0f;
  t->post_re[0] = kre;
  t->post_im[0] = kim;
  for (int k = 1; k <= kFftCplx / 2; ++k) {
    float tmp = (kre * root_re) - (kim * root_im);
    kim = kre * root_im + kim * root_re;
    kre = tmp;
    t->post_re[k] = kre;
    t->post_im[k] = kim;
  }

  // ---- mel triangles, fbank.cc:103-163
  float sample_freq = kSampleRate;
  int num_fft_bins = kFftSize / 2;
  float fft_bin_width = sample_freq / kFftSize;
  float mel_low = MelScale(20);
  float mel_high = MelScale(kSampleRate / 2);
  float mel_delta = (mel_high - mel_low) / (kNumBins + 1);
  t->mel_maxlen = 0;
  int packed = 0;
  for (int bin = 0; bin < kNumBins; ++bin) {
    float left = mel_low + bin * mel_delta;
    float center = mel_low + (bin + 1) * mel_delta;
    float right = mel_low + (bin + 2) * mel_delta;
    int first = -1, last = -1;
    std::vector<float> w(num_fft_bins, 0.0f);
    for (int i = 0; i < num_fft_bins; ++i) {
      float freq = fft_bin_width * i;
      float mel = MelScale(freq);
      if (mel > left && mel < right) {
        w[i] = (mel <= center) ? (mel - left) / (center - left)
                               : (right - mel) / (right - center);
        if (first < 0) first = i;
        last = i;
      }
    }
    if (first < 0 || last <= first) return -3;
    int len = last + 1 - first;
    if (len > kMelMaxLen) return -4;
    t->mel_off[bin] = first;
    t->mel_len[bin] = len;
    t->mel_maxlen = std::max(t->mel_maxlen, len);
    if (packed + len > kMelPacked) return -5;
    t->mel_base[bin] = packed;
    for (int j = 0; j < len; ++j) t->mel_packed[packed + j] = w[first + j];
    packed += len;
  }

  // ---- the packed LDS image of the kernels
  FrontendLdsImage &L = t->lds;
  memcpy(L.logf_tab, t->logf_tab, sizeof(L.logf_tab));
  memcpy(L.window, t->window, sizeof(L.window));
  memcpy(L.tw, t->tw, sizeof(L.tw));
  memcpy(L.post_re, t->post_re, sizeof(L.post_re));
  memcpy(L.post_im, t->post_im, sizeof(L.post_im));
  // the mel stage in product order (pk_tables.h: kMelProducts)
  memset(L.mel_wprod, 0, sizeof(L.mel_wprod));
  memset(L.mel_pgrp, 0, sizeof(L.mel_pgrp));
  int prod = 0;
  for (int b = 0; b < kNumBins; ++b) {
    const int len = t->mel_len[b], padded = (len + 3) / 4 * 4;
    // (a padding tap reads a power-spectrum slot behind the triangle: it must exist -- pw[] has kFftCplx + 4 of them)
    if (prod + padded > kMelProducts || padded > kMelMaxPadded || t->mel_off[b] + padded > kFftCplx + 4) return -6;
    L.mel_pbase[b] = (short)prod;
    L.mel_plen[b] = (short)padded;
    for (int j = 0; j < len; ++j) L.mel_wprod[prod + j] = t->mel_packed[t->mel_base[b] + j];
    for (int j = 0; j < padded; j += 4) L.mel_pgrp[(prod + j) / 4] = (short)(t->mel_off[b] + j);
    prod += padded;
  }
  for (int i = 0; i <= kLogCplx; ++i) L.tw_off[i] = (short)t->tw_off[i];
  for (int i = 0; i <= kNumPasses; ++i) L.pass_start[i] = (short)t->pass_start[i];
  for (int i = 0; i <= kMaxBlocks; ++i) {
    if (t->blk_off[i] < 0 || t->blk_off[i] > 255) return -1;
    L.blk_off[i] = (unsigned char)t->blk_off[i];
  }
  for (int i = 0; i < kFftCplx; ++i) L.bitrev[i] = (unsigned char)t->bitrev[i];
  return 0;
}

void BuildCmvnTables(float global_count_f, CmvnTables *t) {
  const double global_count = global_count_f;
  for (int i = 0; i < kCmvnWindow; ++i) {
    float cnt = static_cast<float>(i + 1);
    float alpha = 0.0f;
    const double count = cnt;
    if (count < kCmvnWindow) {                       // cmvn.cc:80-91
      double from_global = kCmvnWindow - count;
      if (from_global > kCmvnGlobalFrames) from_global = kCmvnGlobalFrames;
      alpha = static_cast<float>(from_global / global_count);
      cnt += alpha * global_count_f;                 // the count element of the float axpy
    }
    const float scale = static_cast<float>(1 / static_cast<double>(cnt));   // cmvn.cc:99
    t->alpha[i] = alpha;
    t->neg_scale[i] = -scale;
  }
}

// ------------------------------------------------------------------ the front-end at a specification (pk_frontend.h)

int BuildFrontendAnyTables(const pk_mi355_frontend_spec_t *spec, FrontendAnyTables *t) {
  using pkhost::Fail;
  if (!spec) return Fail(PK_MI355_E_INVALID, "null argument");
  const pk_mi355_frontend_spec_t &s = *spec;
  if (s.kind != PK_MI355_FRONTEND_FBANK && s.kind != PK_MI355_FRONTEND_MFCC)
    return Fail(PK_MI355_E_INVALID, "front-end spec: unknown kind %d (0 fbank, 1 MFCC)", s.kind);
  if (s.window != PK_MI355_WINDOW_HAMMING && s.window != PK_MI355_WINDOW_POVEY)
    return Fail(PK_MI355_E_INVALID, "front-end spec: unknown window %d (0 Hamming, 1 Povey)", s.window);
  const int B = s.num_mel_bins;
  if (B < kAnyMinBins || B > kAnyMaxBins)
    return Fail(PK_MI355_E_INVALID, "front-end spec: num_mel_bins %d is outside %d .. %d", B, kAnyMinBins, kAnyMaxBins);
  const bool mfcc = s.kind == PK_MI355_FRONTEND_MFCC;
  if (mfcc && (s.num_ceps < 1 || s.num_ceps > B))
    return Fail(PK_MI355_E_INVALID, "front-end spec: num_ceps %d is outside 1 .. num_mel_bins = %d", s.num_ceps, B);
  if (!mfcc && s.num_ceps != 0) return Fail(PK_MI355_E_INVALID, "front-end spec: num_ceps must be 0 for fbank (got %d)", s.num_ceps);
  if (!std::isfinite(s.low_freq) || s.low_freq < 0) return Fail(PK_MI355_E_INVALID, "front-end spec: low_freq %g is negative or not finite", (double)s.low_freq);
  if (!std::isfinite(s.high_freq)) return Fail(PK_MI355_E_INVALID, "front-end spec: high_freq %g is not finite", (double)s.high_freq);
  if (mfcc && (!std::isfinite(s.cepstral_lifter) || s.cepstral_lifter < 0))
    return Fail(PK_MI355_E_INVALID, "front-end spec: cepstral_lifter %g is negative or not finite", (double)s.cepstral_lifter);
  const float high = s.high_freq > 0.0f ? s.high_freq : kAnyNyquist + s.high_freq;      // Kaldi: <= 0 is an offset from Nyquist
  if (high > kAnyNyquist || !(high > s.low_freq))
    return Fail(PK_MI355_E_INVALID, "front-end spec: high_freq resolves to %g Hz: it must be above low_freq = %g and at most %g",
                (double)high, (double)s.low_freq, (double)kAnyNyquist);

  std::vector<FrontendAnyTables> own;      // (t == null: the check alone; 70 KiB, so not on the stack)
  if (!t) { own.resize(1); t = own.data(); }
  memset(t, 0, sizeof(*t));
  t->kind = s.kind; t->num_bins = B; t->num_ceps = mfcc ? s.num_ceps : 0; t->dim = mfcc ? s.num_ceps : B;

  // ---- window: the reference's float angle step (fbank.cc:249-256).  Hamming as BuildFrontendTables forms it (float
  // cosine, the expression in double); Povey in double throughout.  One rounding to float.
  const float a = kTwoPiTrunc / (kFrameLength - 1);
  for (int i = 0; i < kFrameLength; ++i) {
    const float i_fl = static_cast<float>(i);
    if (s.window == PK_MI355_WINDOW_HAMMING) t->lds.window[i] = 0.54 - 0.46 * cosf(a * i_fl);
    else t->lds.window[i] = pow(0.5 - 0.5 * cos(static_cast<double>(a) * i), 0.85);
  }

  // ---- mel triangles, fbank.cc:103-163 with B bins over the spec's band; a bin needs one tap (Kaldi's condition)
  const float sample_freq = kSampleRate;
  const int num_fft_bins = kFftSize / 2;
  const float fft_bin_width = sample_freq / kFftSize;
  // The band's edges: the reference writes MelScale(20) and MelScale(8000) with constants, which its compiler folds with
  // a correctly rounded logarithm -- one ulp above the C library's logf at 20 Hz.  So the edges take the logarithm in
  // double, rounded to float once (what the fold gives, at every band); the FFT bins' mel values below are computed at
  // run time in the reference too, with the C library's logf.
  auto edge_mel = [](float freq) { return 1127.0f * static_cast<float>(log(static_cast<double>(1.0f + freq / 700.0f))); };
  const float mel_low = edge_mel(s.low_freq);
  const float mel_high = edge_mel(high);
  const float mel_delta = (mel_high - mel_low) / (B + 1);
  int taps = 0;
  for (int bin = 0; bin < B; ++bin) {
    const float left = mel_low + bin * mel_delta;
    const float center = mel_low + (bin + 1) * mel_delta;
    const float right = mel_low + (bin + 2) * mel_delta;
    int first = -1, last = -1;
    float w[kFftSize / 2];
    for (int i = 0; i < num_fft_bins; ++i) {
      const float freq = fft_bin_width * i;
      const float mel = MelScale(freq);
      w[i] = 0.0f;
      if (mel > left && mel < right) {
        w[i] = (mel <= center) ? (mel - left) / (center - left) : (right - mel) / (right - center);
        if (first < 0) first = i;
        last = i;
      }
    }
    if (first < 0)
      return Fail(PK_MI355_E_INVALID, "front-end spec: mel bin %d of %d over %g .. %g Hz has an empty triangle (no FFT bin inside it): "
                  "fewer bins or a wider band", bin, B, (double)s.low_freq, (double)high);
    const int len = last + 1 - first;
    if (taps + len > kAnyMaxTaps) return Fail(PK_MI355_E_INVALID, "internal: front-end spec with more than %d mel taps", kAnyMaxTaps);
    t->mel_off[bin] = first;
    t->lds.mel_base[bin] = (short)taps;
    t->lds.mel_len[bin] = (short)len;
    for (int j = 0; j < len; ++j) {
      t->lds.mel_w[taps + j] = w[first + j];
      t->lds.mel_tap[taps + j] = (short)(first + j);
    }
    taps += len;
  }
  t->num_taps = taps;

  // ---- DCT and lifter (Kaldi's definitions), in double, one rounding
  for (int k = 0; k < kAnyMaxBins; ++k) t->lifter[k] = 1.0f;
  if (mfcc) {
    for (int k = 0; k < s.num_ceps; ++k) {
      for (int b = 0; b < B; ++b)
        t->dct_t[b * kAnyMaxBins + k] = k == 0 ? sqrt(1.0 / B) : sqrt(2.0 / B) * cos(M_PI / B * (b + 0.5) * k);
      const double Q = s.cepstral_lifter;
      if (Q != 0) t->lifter[k] = 1.0 + 0.5 * Q * sin(M_PI * k / Q);
    }
  }
  return 0;
}

// ------------------------------------------------------------------ resampler (pk_resample.h)

int BuildResampleTable(int rate, ResampleTable *t) {
  if (rate < kResampleMinRate || rate > kResampleMaxRate) return -1;
  if (rate == kResampleOutRate) {                      // the identity (no filter: callers copy)
    t->rate = rate; t->Q = t->P = t->max_taps = 1;
    t->min_first = 0; t->max_end = 1;
    t->first.assign(1, 0); t->count.assign(1, 1); t->weights.assign(1, 1.0f);
    return 0;
  }
  const int fi = rate, fo = kResampleOutRate;
  int a = fi, b = fo;
  while (b) { const int r = a % b; a = b; b = r; }
  const int Q = fi / a, P = fo / a;
  if ((int64_t)P * 12 > kResampleMaxEntries) return -1;   // (a window of 2 w fi >= 12.1 samples holds at least 12 taps)
  const double fc = 0.99 * 0.5 * std::min(fi, fo);
  const double Z = 6.0;
  const double w = Z / (2 * fc);
  std::vector<int32_t> first(P), count(P);
  int max_taps = 0;
  for (int p = 0; p < P; ++p) {
    const double tau = (double)p / fo;
    // the taps: the integers i with |i / fi - tau| < w (strict); scanned over a range that certainly holds them
    const int lo = (int)floor((tau - w) * fi) - 2, hi = (int)ceil((tau + w) * fi) + 2;
    int f = 0, c = 0;
    for (int i = lo; i <= hi; ++i)
      if (fabs((double)i / fi - tau) < w) {
        if (c == 0) f = i;
        ++c;
      }
    first[p] = f;
    count[p] = c;
    max_taps = std::max(max_taps, c);
  }
  if ((int64_t)P * max_taps > kResampleMaxEntries) return -1;
  t->rate = rate; t->Q = Q; t->P = P; t->max_taps = max_taps;
  t->first.swap(first);
  t->count.swap(count);
  t->weights.assign((size_t)P * max_taps, 0.0f);
  t->min_first = t->first[0];
  t->max_end = t->first[0] + t->count[0];
  for (int p = 0; p < P; ++p) {
    const double tau = (double)p / fo;
    t->min_first = std::min(t->min_first, t->first[p]);
    t->max_end = std::max(t->max_end, t->first[p] + t->count[p]);
    for (int k = 0; k < t->count[p]; ++k) {
      const double d = (double)(t->first[p] + k) / fi - tau;
      const double x = 2 * fc * d;
      const double sinc = x == 0 ? 1.0 : sin(M_PI * x) / (M_PI * x);
      const double window = 0.5 * (1 + cos(2 * M_PI * fc * d / Z));
      t->weights[(size_t)p * max_taps + k] = (float)(2 * fc * sinc * window / fi);   // double throughout, one rounding
    }
  }
  return 0;
}

int64_t ResampleNumFinal(const ResampleTable &t, int64_t n) {
  if (n <= 0) return 0;
  // every window of a unit below u0 ends below u0 Q + max_end - Q <= n: the search starts there
  int64_t j = (n > t.max_end ? (n - t.max_end) / t.Q : 0) * t.P;
  for (;; ++j) {
    const int64_t u = j / t.P;
    const int p = (int)(j - u * t.P);
    if (t.first[p] + u * t.Q + t.count[p] - 1 >= n) break;
  }
  return std::min(j, ResampleNumOutput(t, n));
}

}  // namespace pkmi

// ------------------------------------------------------------------ the resampler's host entries (no device)

namespace {
int BuildOrFail(int rate, pkmi::ResampleTable *t) {
  if (pkmi::BuildResampleTable(rate, t))
    return pkhost::Fail(PK_MI355_E_INVALID, "sample rate %d is not supported: 8000 .. 96000 Hz with a polyphase table of at most %d entries",
                        rate, pkmi::kResampleMaxEntries);
  return 0;
}
}  // namespace

extern "C" {

int pk_mi355_resample_plan(int rate, int *Q, int *P, int *max_taps) {
  pkmi::ResampleTable t;
  if (int rc = BuildOrFail(rate, &t)) return rc;
  if (Q) *Q = t.Q;
  if (P) *P = t.P;
  if (max_taps) *max_taps = t.max_taps;
  return 0;
}

int pk_mi355_resample_table(int rate, int32_t *first, int32_t *count, float *weights) {
  pkmi::ResampleTable t;
  if (int rc = BuildOrFail(rate, &t)) return rc;
  if (first) memcpy(first, t.first.data(), sizeof(int32_t) * t.P);
  if (count) memcpy(count, t.count.data(), sizeof(int32_t) * t.P);
  if (weights) memcpy(weights, t.weights.data(), sizeof(float) * t.weights.size());
  return 0;
}

int64_t pk_mi355_resample_num_output(int rate, int64_t n) {
  pkmi::ResampleTable t;
  if (int rc = BuildOrFail(rate, &t)) return rc;
  if (n < 0) return pkhost::Fail(PK_MI355_E_INVALID, "negative sample count");
  return pkmi::ResampleNumOutput(t, n);
}

// ------------------------------------------------------------------ the front-end spec's host entries (no device)

int pk_mi355_frontend_check(const pk_mi355_frontend_spec_t *spec) { return pkmi::BuildFrontendAnyTables(spec, nullptr); }

int pk_mi355_frontend_dim(const pk_mi355_frontend_spec_t *spec) {
  if (int rc = pkmi::BuildFrontendAnyTables(spec, nullptr)) return rc;
  return spec->kind == PK_MI355_FRONTEND_MFCC ? spec->num_ceps : spec->num_mel_bins;
}

int pk_mi355_frontend_default(pk_mi355_frontend_spec_t *spec) {      // fbank.h:10, fbank.cc:116-117, :249-256
  if (!spec) return pkhost::Fail(PK_MI355_E_INVALID, "null argument");
  *spec = pk_mi355_frontend_spec_t{PK_MI355_FRONTEND_FBANK, pkmi::kNumBins, 0, PK_MI355_WINDOW_HAMMING, 20.0f, 0.0f, 0.0f};
  return 0;
}

int pk_mi355_frontend_tables(const pk_mi355_frontend_spec_t *spec, float *window, int32_t *mel_off, int32_t *mel_len, float *mel_weights,
                             float *dct, float *lifter) {
  std::vector<pkmi::FrontendAnyTables> tv(1);
  pkmi::FrontendAnyTables &t = tv[0];
  if (int rc = pkmi::BuildFrontendAnyTables(spec, &t)) return rc;
  if (window) memcpy(window, t.lds.window, sizeof(t.lds.window));
  for (int b = 0; b < t.num_bins; ++b) {
    if (mel_off) mel_off[b] = t.mel_off[b];
    if (mel_len) mel_len[b] = t.lds.mel_len[b];
  }
  if (mel_weights) memcpy(mel_weights, t.lds.mel_w, sizeof(float) * t.num_taps);
  for (int k = 0; k < t.num_ceps; ++k) {
    if (dct) for (int b = 0; b < t.num_bins; ++b) dct[k * t.num_bins + b] = t.dct_t[b * pkmi::kAnyMaxBins + k];
    if (lifter) lifter[k] = t.lifter[k];
  }
  return 0;
}

}  // extern "C"
