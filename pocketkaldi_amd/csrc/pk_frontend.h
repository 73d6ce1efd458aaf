// pk_frontend.h -- the front-end at a specification: log-mel fbank with any number of bins over
// any band, MFCC on top of it.  The per-spec tables the host builds (pk_tables.cc) and the launcher of FbankAnyKernel
// (frontend.hip).  Kept apart from pk_tables.h / pk_kernels.h: those are part of what gemm.hip is compiled from.
#ifndef PK_FRONTEND_H_
#define PK_FRONTEND_H_

#include <stddef.h>
#include <stdint.h>

#include "../../include/pk_mi355.h"
#include "pk_tables.h"
#ifdef __HIP__
#include "pk_kernels.h"
#endif

namespace pkmi {

constexpr int kAnyMinBins = 3;
constexpr int kAnyMaxBins = 128;       // two bins (and two cepstra) per lane
// A frequency lies strictly inside at most two neighbouring triangles, and the triangles cover FFT bins 0..255 only
// (fbank.cc:133): no spec has more than 512 taps (checked when the tables are built).
constexpr int kAnyMaxTaps = 512;
constexpr float kAnyNyquist = 0.5f * kSampleRate;

// What FbankAnyKernel keeps in LDS beside FbankKernel's FFT and logf tables, copied flat in 16-byte pieces.
struct alignas(16) FrontendAnyLds {
  float window[kFrameLength];          // the spec's window
  float mel_w[kAnyMaxTaps];            // tap weights, bin after bin, no padding
  short mel_tap[kAnyMaxTaps];          // the FFT bin of tap i
  short mel_base[kAnyMaxBins];         // first tap of bin b
  short mel_len[kAnyMaxBins];          // its taps (>= 1)
};
static_assert(sizeof(FrontendAnyLds) % 16 == 0, "copied in 16-byte pieces");

struct FrontendAnyTables {
  FrontendAnyLds lds;
  int32_t kind, num_bins, num_ceps, dim, num_taps;
  int32_t mel_off[kAnyMaxBins];        // first FFT bin of bin b (the host entries report it; the kernel reads lds.mel_tap)
  float lifter[kAnyMaxBins];           // 1.0f where there is none
  float dct_t[kAnyMaxBins * kAnyMaxBins];   // MFCC: dct[k][b] at [b * kAnyMaxBins + k]: lane k reads consecutive addresses
};

// 0, or PK_MI355_E_INVALID with the field named in the fail text.  t may be null (the check alone).  Host only.
int BuildFrontendAnyTables(const pk_mi355_frontend_spec_t *spec, FrontendAnyTables *t);

#ifdef __HIP__   // (pk_tables.cc is plain C++)
// The spec's features for a batch: PCM -> rows raw[(raw_base[u] + t) * dim + d], LaunchFbank's contract at the spec's
// dimension.  d_tables: FbankKernel's (FFT schedule, twiddles, logf); d_any: the spec's.  dim = any.dim (host copy).
void LaunchFbankAny(const float *wave_f32, const int16_t *wave_i16, const UttLayout &utts, int num_utts, int max_frames,
                    const FrontendTables *d_tables, const FrontendAnyTables *d_any, int dim, float *raw, hipStream_t stream);
#endif

}  // namespace pkmi

#endif  // PK_FRONTEND_H_
