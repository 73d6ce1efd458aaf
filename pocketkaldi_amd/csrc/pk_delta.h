// pk_delta.h -- delta features (Kaldi's add-deltas; include/pk_mi355.h states the rule): the
// spec's check, the scale table and the per-element apply step.  Plain C++: no HIP header; pk_delta.cc is compiled by g++
// like pk_norm.cc, so it also builds into a stand-alone program that runs under the host sanitizers
// (tests/cpp/delta_test.cc).  delta.hip includes this header for DeltaApply: the kernel and the host run the same
// lines.  Internal, like pk_norm.h.
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

}  // namespace pkdelta

#endif  // PK_DELTA_H_
