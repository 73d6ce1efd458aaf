// pk_delta_kernel.h -- the launcher of DeltaKernel (delta.hip), for capi_batch.hip.  Kept out of
// pk_kernels.h: that header is part of the hash that ties the GEMM profiles to the GEMM's sources.  Internal.
#ifndef PK_DELTA_KERNEL_H_
#define PK_DELTA_KERNEL_H_

#include <hip/hip_runtime.h>

#include "pk_delta.h"
#include "pk_kernels.h"

namespace pkmi {

constexpr int kDeltaFrames = 32;        // G: output frames per wavefront

// Rows in [sum T][base_dim] -> rows out [sum T][(order + 1) base_dim] (never in place), utterance u's rows from
// raw_base[u] on in both; LaunchFeatureLayout then lays `out` out.  d_scales: the spec's table (pkdelta::BuildScales) on
// the device.  One wavefront per (utterance, run of kDeltaFrames frames, block of 64 base features).  The caller has
// checked the spec, every base and count against the buffers.
void LaunchDelta(const float *in, const UttLayout &utts, int num_utts, int max_frames, int base_dim, const pk_mi355_deltas_spec_t &spec,
                 const float *d_scales, float *out, hipStream_t stream);

}  // namespace pkmi

#endif  // PK_DELTA_KERNEL_H_
