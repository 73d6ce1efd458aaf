// pk_transform.h -- feature transforms (Kaldi's splice-feats | transform-feats and per-utterance transform-feats;
// include/pk_mi355.h states the rule): the spec's check, the per-output chain and the layout the
// kernel reads a matrix in.  Plain C++: no HIP header; pk_transform.cc is compiled by g++ like pk_delta.cc, so it also
// builds into a stand-alone program that runs under the host sanitizers (tests/cpp/transform_test.cc).  transform.hip
// includes this header for TransformApply: the kernel and the host run the same lines.  Below them what a live slot adds
// (DESIGN.md section 26): the frame accounting of one step, the choice between a step's fresh rows and the slot's ring --
// which StreamTransformKernel compiles too -- and a host streaming apply for the stand-alone test
// (tests/cpp/stream_transform_test.cc).  Internal, like pk_delta.h.
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

// ------------------------------------------------------------------ a live slot
// One step of a slot's frame accounting.  nin: the transform's input frames final after the step's pushes (normalised
// base frames, or behind deltas the nd1 of pkdelta::StreamDeltaAdvance); nx: transform frames final before it; a: rows
// scored before it; Rt: the spec's right context; R: the model's.  Transform frames [nx, nx1) become final (an open slot
// holds Rt input frames back, a closed one none); rows [a, b) are scored (an open slot holds R transform frames back).
struct StreamTransformCounts { int nx1, b; };
inline StreamTransformCounts StreamTransformAdvance(int nin, int nx, int a, int Rt, int R, bool closed) {
  const int nx1 = closed ? nin : (nin - Rt > nx ? nin - Rt : nx);
  const int b = closed ? nx1 : (nx1 - R > a ? nx1 - R : a);
  return StreamTransformCounts{nx1, b};
}

// Where input frame f of a slot lies during a step that found nin_old input frames final: among the step's fresh rows
// (row f - nin_old), or in the slot's ring of the last C = left_context + right_context frames (entry f mod C; asked
// only when C > 0 and f >= nin_old - C).
struct StreamTransformSource { bool fresh; int row; };
PK_NORM_HD inline StreamTransformSource StreamTransformPick(int f, int nin_old, int C) {
  return f >= nin_old ? StreamTransformSource{true, f - nin_old} : StreamTransformSource{false, f % C};
}

// The live rule on the host (test-only, internal; tests/cpp/stream_transform_test.cc holds it to
// pk_mi355_transform_apply on the whole matrix): what StreamTransformKernel does for one slot, with the same
// accounting, the same pick and a ring of exactly C frames.  Push(x, m, closed, out): m input rows [m][in_dim]; appends
// the rows [.][OutDim] that became final to *out and returns how many.  Nothing may be pushed after closed.  The spec
// has been checked and its matrix outlives the object.
class StreamTransformHost {
 public:
  explicit StreamTransformHost(const pk_mi355_transform_spec_t &spec);
  ~StreamTransformHost();
  StreamTransformHost(const StreamTransformHost &) = delete;
  StreamTransformHost &operator=(const StreamTransformHost &) = delete;
  int Push(const float *x, int m, bool closed, float *out);      // out: room for m + right_context rows
  int frames() const { return nin_; }
  int final_frames() const { return nx_; }

 private:
  pk_mi355_transform_spec_t spec_;
  int C_, nin_ = 0, nx_ = 0, par_ = 0;
  float *ring_[2];                // two buffers of exactly C * in_dim floats each, used in turn
};

}  // namespace pkxf

#endif  // PK_TRANSFORM_H_
