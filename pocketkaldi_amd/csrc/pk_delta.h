// pk_delta.h -- delta features (Kaldi's add-deltas; include/pk_mi355.h states the rule): the
// spec's check, the scale table and the per-element apply step.  Plain C++: no HIP header; pk_delta.cc is compiled by g++
// like pk_norm.cc, so it also builds into a stand-alone program that runs under the host sanitizers
// (tests/cpp/delta_test.cc).  delta.hip includes this header for DeltaApply: the kernel and the host run the same
// lines.  Below them what a live slot adds: the frame accounting of one step, the choice between
// a step's fresh rows and the slot's ring -- which StreamDeltaKernel compiles too -- and a host streaming apply for the
// stand-alone test (tests/cpp/stream_delta_test.cc).  Internal, like pk_norm.h.
#ifndef PK_DELTA_H_
#define PK_DELTA_H_

#include <stdint.h>

#include "pk_norm.h"        // PK_NORM_HD, include/pk_mi355.h

namespace pkdelta {

constexpr int kMaxOrder = 3;
constexpr int kMaxWindow = 8;
constexpr int kMaxReach = kMaxOrder * kMaxWindow;                 // M of the highest block, at most
constexpr int kMaxRowLen = 2 * kMaxReach + 1;
constexpr int kMaxTable = (kMaxOrder + 1) * kMaxRowLen;           // floats of the largest scale table

// The scale table of a checked spec: [order + 1][2 * order * window + 1] floats, row i holding its 2 i window + 1 scales
// centred (entry j of block i at column order * window + j), zeros around them.
inline int Reach(const pk_mi355_deltas_spec_t &s) { return s.order * s.window; }
inline int RowLen(const pk_mi355_deltas_spec_t &s) { return 2 * Reach(s) + 1; }

// pk_mi355_deltas_check
int CheckSpec(const pk_mi355_deltas_spec_t *spec);
// Kaldi's DeltaFeatures constructor, in float (the spec has been checked); table: (order + 1) * RowLen floats.
void BuildScales(const pk_mi355_deltas_spec_t &spec, float *table);

// One output element: block i of one frame of one column.  centre: the block's scale for j = 0 (its row of the table
// plus order * window); M = i * window; x(j): the column's value at frame clamp(t + j, 0, T - 1).  j ascending, a
// rounded product and a rounded add (built with -ffp-contract=off), taps whose scale is zero skipped.
// V: float on the host; in DeltaKernel a run of frames of the column, every frame's chain being these lines.
template <class V, class Load>
PK_NORM_HD inline V DeltaApply(const float *centre, int M, Load x) {
  V acc = V(0.0f);
  for (int j = -M; j <= M; ++j) {
    const float s = centre[j];
    if (s != 0.0f) {
      const V p = s * x(j);
      acc = acc + p;
    }
  }
  return acc;
}

// ------------------------------------------------------------------ a live slot
// One step of a slot's frame accounting.  n: normalised base frames after the step's pushes; nd: delta frames final
// before it; a: rows scored before it; M = order * window; R: the model's right context.  Delta frames [nd, nd1) become
// final (an open slot holds M base frames back, a closed one none); rows [a, b) are scored (an open slot holds R delta
// frames back).
struct StreamDeltaCounts { int nd1, b; };
inline StreamDeltaCounts StreamDeltaAdvance(int n, int nd, int a, int M, int R, bool closed) {
  const int nd1 = closed ? n : (n - M > nd ? n - M : nd);
  const int b = closed ? nd1 : (nd1 - R > a ? nd1 - R : a);
  return StreamDeltaCounts{nd1, b};
}

// Where normalised base frame f of a slot lies during a step that found n_old frames computed: among the step's fresh
// rows (row f - n_old), or in the slot's ring of the last 2 M frames (entry f mod 2 M; only f >= n_old - 2 M is there).
struct StreamDeltaSource { bool fresh; int row; };
PK_NORM_HD inline StreamDeltaSource StreamDeltaPick(int f, int n_old, int M) {
  return f >= n_old ? StreamDeltaSource{true, f - n_old} : StreamDeltaSource{false, f % (2 * M)};
}

// The live rule on the host (test-only, internal; tests/cpp/stream_delta_test.cc holds it to pk_mi355_deltas_apply on
// the whole matrix): what StreamDeltaKernel does for one slot, with the same accounting, the same pick and a ring of
// exactly 2 M frames.  Push(x, m, closed, out): m normalised base rows [m][Db]; appends the rows [.][(order + 1) Db]
// that became final to *out and returns how many.  Nothing may be pushed after closed.
class StreamDeltaHost {
 public:
  StreamDeltaHost(const pk_mi355_deltas_spec_t &spec, int base_dim);
  ~StreamDeltaHost();
  StreamDeltaHost(const StreamDeltaHost &) = delete;
  StreamDeltaHost &operator=(const StreamDeltaHost &) = delete;
  int Push(const float *x, int m, bool closed, float *out);      // out: room for m + M rows
  int frames() const { return n_; }
  int final_frames() const { return nd_; }

 private:
  pk_mi355_deltas_spec_t spec_;
  int Db_, M_, n_ = 0, nd_ = 0, par_ = 0;
  float table_[kMaxTable];
  float *ring_[2];                // two buffers of exactly 2 M * Db floats each, used in turn
};

}  // namespace pkdelta

#endif  // PK_DELTA_H_
