// pk_norm.h -- the normalisation spec of a batch scorer (include/pk_mi355.h): its check, the
// finalisation of a statistics record into the (offset, scale) pair NormKernel applies, and the rule on the host.
// Plain C++: no HIP header; pk_norm.cc is compiled by g++ like pk_files.cc, so it also builds into a stand-alone program
// that runs under the host sanitizers (tests/cpp/norm_test.cc).  norm.hip includes this header for NormFinalize: the
// kernel and the host run the same lines.  Internal, like pk_host.h.
#ifndef PK_NORM_H_
#define PK_NORM_H_

#include <math.h>
#include <stdint.h>

#include "../../include/pk_mi355.h"

#if defined(__HIPCC__)
#define PK_NORM_HD __host__ __device__
#else
#define PK_NORM_HD
#endif

namespace pknorm {

constexpr double kVarFloor = 1e-20;      // Kaldi's ApplyCmvn

// One column's sums and count -> what the apply step adds and multiplies by.  All in double; one rounding to float each.
// (A NaN variance fails the comparison and stays NaN.)
PK_NORM_HD inline void NormFinalize(double s0, double s1, double n, bool norm_means, bool norm_vars, float *offs_f, float *scale_f) {
  const double mean = norm_means ? s0 / n : 0.0;
  double scale = 1.0, offset = -mean;
  if (norm_vars) {
    double var = s1 / n - mean * mean;
    if (var < kVarFloor) var = kVarFloor;
    scale = 1.0 / sqrt(var);
    offset = -(mean * scale);
  }
  *offs_f = (float)offset;
  *scale_f = (float)scale;
}

// y = norm_vars ? (x * scale) + offset : x + offset, a rounded product and a rounded add (built with -ffp-contract=off)
PK_NORM_HD inline float NormApply(float x, float offs_f, float scale_f, bool norm_vars) {
  if (!norm_vars) return x + offs_f;
  const float p = x * scale_f;
  return p + offs_f;
}

// pk_mi355_norm_check
int CheckSpec(const pk_mi355_norm_spec_t *spec);
// true for the modes whose kernel reads the switches
inline bool UsesStats(int mode) { return mode == PK_MI355_NORM_UTTERANCE || mode == PK_MI355_NORM_SPEAKER; }
// Speaker records [num_utts][2][dim + 1] -> table [num_utts][2][dim] (row 0 the offsets, row 1 the scales).  Every count
// is checked first (PK_MI355_E_INVALID naming the utterance); nothing is written when one is bad.
int FinalizeSpeakerStats(const double *stats, int num_utts, int dim, bool norm_means, bool norm_vars, float *table);

}  // namespace pknorm

#endif  // PK_NORM_H_
