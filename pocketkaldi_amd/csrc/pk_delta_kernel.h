// pk_delta_kernel.h -- the launchers of DeltaKernel (delta.hip), for capi_batch.hip, and of
// StreamDeltaKernel, for capi_stream.hip.  Kept out of pk_kernels.h: that header is part of the
// hash that ties the GEMM profiles to the GEMM's sources.  Internal.
#ifndef PK_DELTA_KERNEL_H_
#define PK_DELTA_KERNEL_H_

#include <hip/hip_runtime.h>

#include "pk_delta.h"
#include "pk_kernels.h"
#include "pk_score.h"       // StreamRec

namespace pkmi {

constexpr int kDeltaFrames = 32;        // G: output frames per wavefront

// Rows in [sum T][base_dim] -> rows out [sum T][(order + 1) base_dim] (never in place), utterance u's rows from
// raw_base[u] on in both; LaunchFeatureLayout then lays `out` out.  d_scales: the spec's table (pkdelta::BuildScales) on
// the device.  One wavefront per (utterance, run of kDeltaFrames frames, block of 64 base features).  The caller has
// checked the spec, every base and count against the buffers.
void LaunchDelta(const float *in, const UttLayout &utts, int num_utts, int max_frames, int base_dim, const pk_mi355_deltas_spec_t &spec,
                 const float *d_scales, float *out, hipStream_t stream);

// StreamDeltaKernel (delta.hip), between the normaliser and StreamFeatureLayoutKernel of a step of
// a deltas stream object.  recs[k]: the step's record of a slot (audio or RAW: m fresh normalised base rows [m][base_dim]
// at rows + row_off, n_old base frames before them, ring_par; NORMALIZED records are skipped).  lrecs[k]: the record the
// layout launch will see for the same slot -- n_old = nd, the delta frames final before the step, m = the delta frames
// [nd, nd + m) this launch makes final, written as rows [m][(order + 1) base_dim] at rows + lrecs[k].row_off (the delta
// staging: never where the base rows lie).  ring: [slots][2][2 M][base_dim], M = order * window; buffer ring_par holds
// the base frames [max(n_old - 2 M, 0), n_old), the other one receives [max(n - 2 M, 0), n) when m > 0 (the host then
// flips the bit).  max_new: the most delta frames any record makes final.  One wavefront per (record, run of
// kDeltaFrames delta frames, block of 64 base features).  The caller has checked every base and count against the buffers.
void LaunchStreamDelta(const StreamRec *recs, const StreamRec *lrecs, int n, int max_new, int base_dim, const pk_mi355_deltas_spec_t &spec,
                       const float *d_scales, float *rows, float *ring, hipStream_t stream);

}  // namespace pkmi

#endif  // PK_DELTA_KERNEL_H_
