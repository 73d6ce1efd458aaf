// pk_transform_kernel.h -- the launchers of TransformKernel (transform.hip), for capi_batch.hip,
// and of StreamTransformKernel, for capi_stream.hip.  Kept out of pk_kernels.h: that header is part of the hash that ties the GEMM profiles to the GEMM's sources.  Internal.
#ifndef PK_TRANSFORM_KERNEL_H_
#define PK_TRANSFORM_KERNEL_H_

#include <hip/hip_runtime.h>

#include "pk_kernels.h"     // UttLayout
#include "pk_score.h"       // StreamRec
#include "pk_transform.h"

namespace pkmi {

constexpr int kTransformFrames = 16;    // G: output frames per wavefront
// The widest model a live slot's own matrix is accepted for: the stage's G rows of feat_dim floats fill 64 KiB of LDS.
constexpr int kMaxSlotTransformDim = 1024;

// One stage of the transform.  Rows in [sum T][in_dim] -> rows out [sum T][rows] (never in place), utterance u's rows
// from raw_base[u] on in both.  Frame t of an utterance reads its frames clamp(t - left .. t + right, 0, T - 1).
// mt: matrices in pkxf::PackTransposed's layout, [cols][Ldo(rows)] each, cols = (left + right + 1) * in_dim + (affine ?
// 1 : 0); utterance u reads the matrix at mt + u * mat_stride floats -- stride 0: every utterance the same one.
struct TransformStage {
  int in_dim, left, right, rows;
  bool affine;
  const float *mt;
  int64_t mat_stride;
};
// Dynamic LDS of a launch: the (G + left + right) staged rows.  The widest accepted spec (in_dim 512, left + right 16)
// takes exactly 64 KiB.
inline size_t TransformLds(const TransformStage &s) { return sizeof(float) * (size_t)(kTransformFrames + s.left + s.right) * s.in_dim; }
// One wavefront per (utterance, run of kTransformFrames frames, block of 64 outputs).  The caller has checked the spec
// (pkxf::CheckSpec's limits), every base and count against the buffers.
void LaunchTransform(const float *in, const UttLayout &utts, int num_utts, int max_frames, const TransformStage &stage, float *out,
                     hipStream_t stream);

// StreamTransformKernel (transform.hip), between the normaliser (or StreamDeltaKernel) and
// StreamFeatureLayoutKernel of a step of a transform stream object.  irecs[k]: the record of a slot as the stage in
// front left it (audio or RAW: m fresh input rows [m][in_dim] at rows + row_off, n_old input frames before them;
// NORMALIZED records are skipped).  orecs[k]: the record the next stage will see for the same slot -- n_old = nx, the
// transform frames final before the step, m = the frames [nx, nx + m) this launch makes final, written as rows
// [m][stage.rows] at rows + orecs[k].row_off (a staging of this stage's own: never where the input rows lie).
// ring: [slots][2][max(C, 1)][in_dim], C = left + right; the buffer that bit 0 of irecs[k].xf_bits names holds the input
// frames [max(n_old - C, 0), n_old), the other one receives [max(n - C, 0), n) when m > 0 and C > 0 (the host then flips
// the bit).  per_slot: the slots' own stage (left = right = 0, in_dim = rows, the ring never read): the matrix of slot s
// lies at stage.mt + s * stage.mat_stride, bits 1-2 of irecs[k].xf_bits say whether it is linear or affine, and a slot
// without one has its rows copied as bits; stage.affine is not read.  Else every record reads stage.mt.
// max_new: the most frames any record makes final.  One wavefront per (record, run of kTransformFrames transform
// frames, block of 64 outputs).  The caller has checked the spec, every base and count against the buffers.
void LaunchStreamTransform(const StreamRec *irecs, const StreamRec *orecs, int n, int max_new, const TransformStage &stage, bool per_slot,
                           float *rows, float *ring, hipStream_t stream);

}  // namespace pkmi

#endif  // PK_TRANSFORM_KERNEL_H_
