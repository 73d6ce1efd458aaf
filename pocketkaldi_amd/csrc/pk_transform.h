// pk_transform.h -- feature transforms (Kaldi's splice-feats | transform-feats and per-utterance transform-feats;
// include/pk_mi355.h states the rule): the spec's check, the per-output chain and the layout the
// kernel reads a matrix in.  Plain C++: no HIP header; pk_transform.cc is compiled by g++ like pk_delta.cc, so it also
// builds into a stand-alone program that runs under the host sanitizers (tests/cpp/transform_test.cc).  transform.hip
// includes this header for TransformApply: the kernel and the host run the same lines.  Internal, like pk_delta.h.
#ifndef PK_TRANSFORM_H_
#define PK_TRANSFORM_H_

#include <stddef.h>
#include <stdint.h>

#include "pk_norm.h"        // PK_NORM_HD, include/pk_mi355.h

namespace pkxf {

constexpr int kMaxContext = 16;         // left, right, and their sum
constexpr int kMaxInDim = 512;
constexpr int kMaxRows = 2048;

inline bool HasMatrix(const pk_mi355_transform_spec_t &s) { return s.matrix != nullptr; }
inline int Window(const pk_mi355_transform_spec_t &s) { return s.left_context + s.right_context + 1; }
inline int K(const pk_mi355_transform_spec_t &s) { return Window(s) * s.in_dim; }
inline bool Affine(const pk_mi355_transform_spec_t &s) { return s.cols == K(s) + 1; }      // (a checked spec with a matrix)
inline int OutDim(const pk_mi355_transform_spec_t &s) { return HasMatrix(s) ? s.rows : s.in_dim; }

// pk_mi355_transform_check
int CheckSpec(const pk_mi355_transform_spec_t *spec);
// The first entry of m [n] that is not finite, or -1.
int64_t FirstNonFinite(const float *m, int64_t n);

// The layout TransformKernel reads a matrix in: transposed and padded, [cols][ldo] with ldo = rows rounded up to 64 and
// zeros in the padding -- with lane = output, a wave's read of one k is one coalesced run, and the lanes past `rows`
// read zeros.  PackTransposed: m [rows][cols] row-major -> out [cols][Ldo(rows)].
inline int Ldo(int rows) { return (rows + 63) / 64 * 64; }
void PackTransposed(const float *m, int rows, int cols, float *out);

// One output: the chain of include/pk_mi355.h.  W = L + R + 1 window frames of Dp features; m(k): the output's matrix
// entry k (k = W * Dp: the offset); x(j, d): feature d of window frame j (frame clamp(t + j - L, 0, T - 1)).  k
// ascending, a rounded product and a rounded add (built with -ffp-contract=off), no tap skipped, the offset last.
// V: float on the host; in TransformKernel a run of frames of the output, every frame's chain being these lines.
template <class V, class Mat, class Load>
PK_NORM_HD inline V TransformApply(int W, int Dp, bool affine, Mat m, Load x) {
  V acc = V(0.0f);
  for (int j = 0; j < W; ++j)
    for (int d = 0; d < Dp; ++d) {
      const V p = m(j * Dp + d) * x(j, d);
      acc = acc + p;
    }
  if (affine) acc = acc + V(m(W * Dp));
  return acc;
}

}  // namespace pkxf

#endif  // PK_TRANSFORM_H_
