// pk_norm_kernel.h -- the launcher of NormKernel (norm.hip), for capi_batch.hip.  Kept out of
// pk_kernels.h: that header is part of the hash that ties the GEMM profiles to the GEMM's sources.  Internal.
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

}  // namespace pkmi

#endif  // PK_NORM_KERNEL_H_
