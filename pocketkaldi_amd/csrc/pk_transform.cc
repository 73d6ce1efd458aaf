// pk_transform.cc -- feature transforms on the host (pk_transform.h): the check, the matrix layout
// the kernel reads and the whole rule for one matrix; the streaming apply of a live slot (section 26).  No HIP: g++ builds
// it, into the library and into tests/cpp/transform_test.cc and tests/cpp/stream_transform_test.cc.
#include "pk_transform.h"

#include <math.h>
#include <string.h>

#include "pk_files.h"

namespace pkxf {

using pkhost::Fail;

int64_t FirstNonFinite(const float *m, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!isfinite(m[i])) return i;
  return -1;
}

int CheckSpec(const pk_mi355_transform_spec_t *spec) {
  if (!spec) return Fail(PK_MI355_E_INVALID, "null argument");
  const pk_mi355_transform_spec_t &s = *spec;
  if (s.left_context < 0 || s.left_context > kMaxContext)
    return Fail(PK_MI355_E_INVALID, "transform spec: left_context %d is outside [0, %d]", s.left_context, kMaxContext);
  if (s.right_context < 0 || s.right_context > kMaxContext)
    return Fail(PK_MI355_E_INVALID, "transform spec: right_context %d is outside [0, %d]", s.right_context, kMaxContext);
  if (s.left_context + s.right_context > kMaxContext)
    return Fail(PK_MI355_E_INVALID, "transform spec: left_context %d + right_context %d is above %d", s.left_context, s.right_context, kMaxContext);
  if (s.in_dim < 1 || s.in_dim > kMaxInDim) return Fail(PK_MI355_E_INVALID, "transform spec: in_dim %d is outside [1, %d]", s.in_dim, kMaxInDim);
  if (!s.matrix) {
    if (s.rows != 0 || s.cols != 0 || s.left_context != 0 || s.right_context != 0)
      return Fail(PK_MI355_E_INVALID, "transform spec: a null matrix goes with rows = cols = left_context = right_context = 0 only "
                  "(got rows %d, cols %d, left_context %d, right_context %d)", s.rows, s.cols, s.left_context, s.right_context);
    return 0;
  }
  if (s.rows < 1 || s.rows > kMaxRows) return Fail(PK_MI355_E_INVALID, "transform spec: rows %d is outside [1, %d]", s.rows, kMaxRows);
  const int k = K(s);
  if (s.cols != k && s.cols != k + 1)
    return Fail(PK_MI355_E_INVALID, "transform spec: cols %d is neither %d = (left_context + right_context + 1) * in_dim (linear) nor %d (affine)",
                s.cols, k, k + 1);
  const int64_t bad = FirstNonFinite(s.matrix, (int64_t)s.rows * s.cols);
  if (bad >= 0)
    return Fail(PK_MI355_E_INVALID, "transform spec: matrix entry at row %d, column %d is not finite", (int)(bad / s.cols), (int)(bad % s.cols));
  return 0;
}

void PackTransposed(const float *m, int rows, int cols, float *out) {
  const int ldo = Ldo(rows);
  for (int k = 0; k < cols; ++k) {
    for (int o = 0; o < rows; ++o) out[(size_t)k * ldo + o] = m[(size_t)o * cols + k];
    for (int o = rows; o < ldo; ++o) out[(size_t)k * ldo + o] = 0.0f;
  }
}

StreamTransformHost::StreamTransformHost(const pk_mi355_transform_spec_t &spec) : spec_(spec), C_(spec.left_context + spec.right_context) {
  for (int p = 0; p < 2; ++p) ring_[p] = new float[(size_t)C_ * spec_.in_dim];
}

StreamTransformHost::~StreamTransformHost() {
  for (int p = 0; p < 2; ++p) delete[] ring_[p];
}

int StreamTransformHost::Push(const float *x, int m, bool closed, float *out) {
  const int nin_old = nin_, nin = nin_ + m, Dp = spec_.in_dim, C = C_, L = spec_.left_context;
  const StreamTransformCounts c = StreamTransformAdvance(nin, nx_, 0, spec_.right_context, 0, closed);
  const float *old = ring_[par_];
  auto frame = [&](int f) {               // f in [max(nin_old - C, 0), nin)
    const StreamTransformSource s = StreamTransformPick(f, nin_old, C);
    return s.fresh ? x + (size_t)s.row * Dp : old + (size_t)s.row * Dp;
  };
  auto clamped = [&](int t) { return frame(t < 0 ? 0 : t > nin - 1 ? nin - 1 : t); };
  if (!HasMatrix(spec_)) {                // rows pass as bits
    for (int t = nx_; t < c.nx1; ++t) memcpy(out + (size_t)(t - nx_) * Dp, frame(t), sizeof(float) * Dp);
  } else {
    const int W = Window(spec_);
    const bool affine = Affine(spec_);
    const size_t rows = (size_t)spec_.rows, cols = (size_t)spec_.cols;
    for (int t = nx_; t < c.nx1; ++t)
      for (size_t o = 0; o < rows; ++o) {
        const float *mrow = spec_.matrix + o * cols;
        out[(size_t)(t - nx_) * rows + o] =
            TransformApply<float>(W, Dp, affine, [&](int k) { return mrow[k]; }, [&](int j, int d) { return clamped(t + j - L)[d]; });
      }
  }
  if (m > 0 && C > 0) {                   // frames [max(nin - C, 0), nin) to the other buffer, which nothing above reads
    float *next = ring_[par_ ^ 1];
    for (int f = nin - C > 0 ? nin - C : 0; f < nin; ++f) memcpy(next + (size_t)(f % C) * Dp, frame(f), sizeof(float) * Dp);
    par_ ^= 1;
  }
  const int made = c.nx1 - nx_;
  nin_ = nin; nx_ = c.nx1;
  return made;
}

}  // namespace pkxf

extern "C" {

int pk_mi355_transform_check(const pk_mi355_transform_spec_t *spec) { return pkxf::CheckSpec(spec); }

int pk_mi355_transform_out_dim(const pk_mi355_transform_spec_t *spec) {
  if (int rc = pkxf::CheckSpec(spec)) return rc;
  return pkxf::OutDim(*spec);
}

int pk_mi355_transform_apply(const pk_mi355_transform_spec_t *spec, const float *x, int num_frames, float *y) {
  using namespace pkxf;
  if (int rc = CheckSpec(spec)) return rc;
  if (num_frames < 0) return pkhost::Fail(PK_MI355_E_INVALID, "bad shape (%d frames)", num_frames);
  if (num_frames > 0 && (!x || !y)) return pkhost::Fail(PK_MI355_E_INVALID, "null argument");
  if (num_frames > 0 && x == y) return pkhost::Fail(PK_MI355_E_INVALID, "transform: the output may not be the input");
  const size_t T = (size_t)num_frames, Dp = (size_t)spec->in_dim;
  if (!HasMatrix(*spec)) {
    if (T > 0) memcpy(y, x, sizeof(float) * T * Dp);
    return 0;
  }
  const int L = spec->left_context, W = Window(*spec);
  const bool affine = Affine(*spec);
  const size_t rows = (size_t)spec->rows, cols = (size_t)spec->cols;
  for (size_t t = 0; t < T; ++t)
    for (size_t o = 0; o < rows; ++o) {
      const float *m = spec->matrix + o * cols;
      y[t * rows + o] = TransformApply<float>(W, spec->in_dim, affine, [&](int k) { return m[k]; }, [&](int j, int d) {
        const int64_t tt = (int64_t)t + j - L;
        return x[(size_t)(tt < 0 ? 0 : tt >= (int64_t)T ? (int64_t)T - 1 : tt) * Dp + d];
      });
    }
  return 0;
}

}  // extern "C"
