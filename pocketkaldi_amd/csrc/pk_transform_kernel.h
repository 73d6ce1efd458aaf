// pk_transform_kernel.h -- the launcher of TransformKernel (transform.hip), for capi_batch.hip.
// Kept out of pk_kernels.h: that header is part of the hash that ties the GEMM profiles to the GEMM's sources.  Internal.
#ifndef PK_TRANSFORM_KERNEL_H_
#define PK_TRANSFORM_KERNEL_H_

#include <hip/hip_runtime.h>

#include "pk_kernels.h"     // UttLayout
#include "pk_transform.h"

namespace pkmi {

constexpr int kTransformFrames = 16;    // G: output frames per wavefront

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

}  // namespace pkmi

#endif  // PK_TRANSFORM_KERNEL_H_
