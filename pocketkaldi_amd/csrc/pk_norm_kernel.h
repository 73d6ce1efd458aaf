// pk_norm_kernel.h -- the launchers of NormKernel and OnlineCmvnKernel (norm.hip, DESIGN.md sections 19 and 20), for
// capi_batch.hip, and of StreamNormKernel (stream.hip), for capi_stream.hip.  Kept out of pk_kernels.h: that header is
// part of the hash that ties the GEMM profiles to the GEMM's sources.  Internal.
#ifndef PK_NORM_KERNEL_H_
#define PK_NORM_KERNEL_H_

#include <hip/hip_runtime.h>

#include "pk_kernels.h"
#include "pk_norm.h"

namespace pkmi {

// Raw rows [sum T][dim] -> normalised rows `out` of the same shape (never in place), utterance u's rows from raw_base[u]
// on; LaunchFeatureLayout then lays `out` out.  mode: PK_MI355_NORM_UTTERANCE or _SPEAKER.
// UTTERANCE: stats [num_utts][2][dim + 1] doubles receives every utterance's record (one without frames: zeros).
// SPEAKER: table [num_utts][2][dim] floats holds the offsets and the scales (pknorm::FinalizeSpeakerStats).
// One wavefront per (utterance, block of 64 features).  The caller has checked every base and count against the buffers.
void LaunchNorm(const float *raw, const UttLayout &utts, int num_utts, int dim, int mode, bool norm_means, bool norm_vars,
                const float *table, double *stats, float *out, hipStream_t stream);

// Online CMVN on the same rows, in LaunchNorm's place: raw rows -> `out` (never in place).
// glob: the global record [2][dim + 1] doubles on the device (read only when spec.global_frames > 0).  spk: null, or
// [num_utts][2][dim + 1] doubles, utterance u's speaker record (a count of 0: no prior).  The caller has checked the
// spec, the counts, every base and count against the buffers.
void LaunchOnlineCmvn(const float *raw, const UttLayout &utts, int num_utts, int dim, const pk_mi355_online_cmvn_spec_t &spec,
                      const double *glob, const double *spk, float *out, hipStream_t stream);

// ---- the online scorer's normalisation at a spec (stream.hip)
struct StreamRec;                       // pk_score.h

// What StreamNormKernel reads and carries, per stream object.  mode: PK_MI355_NORM_SPEAKER (the slot's finalised table)
// or pknorm::kNormOnlineCmvn (the window state, the ring of raw rows, the two records).
struct StreamNormState {
  int mode, norm_vars;
  int window, speaker_frames, global_frames;      // online CMVN's spec
  const double *glob;       // [2][dim + 1]: the global record (read only when global_frames > 0)
  const double *spk;        // [slots][2][dim + 1]: the slots' speaker records (a count of 0: no prior)
  const float *table;       // [slots][2][dim]: mode speaker's offsets and scales
  double *win;              // [slots][2][dim]: the window sums S0, S1 behind the slot's last frame
  double *total;            // [slots][2][dim]: the sums and sums of squares of all frames since the slot was opened
  float *ring;              // [slots][window][dim]: the raw rows still inside the window, frame t at t % window
};
// The audio and RAW records among the n given have their m fresh rows, [m][dim] at rows + row_off, normalised in place
// (NORMALIZED records and records without fresh rows return at once); LaunchStreamFeatureLayout then lays them out.  One
// wavefront per (record, block of 64 features).  The caller has checked every base and count against the buffers.
void LaunchStreamNorm(const StreamRec *recs, int n, int dim, float *rows, const StreamNormState &st, hipStream_t stream);

}  // namespace pkmi

#endif  // PK_NORM_KERNEL_H_
