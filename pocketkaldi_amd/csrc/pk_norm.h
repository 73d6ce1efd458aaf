// pk_norm.h -- the normalisation spec of a batch scorer (include/pk_mi355.h): its check, the
// finalisation of a statistics record into the (offset, scale) pair NormKernel applies, and the rule on the host.
// Plain C++: no HIP header; pk_norm.cc is compiled by g++ like pk_files.cc, so it also builds into a stand-alone program
// that runs under the host sanitizers (tests/cpp/norm_test.cc).  Also here: online CMVN and
// its check.  Internal, like pk_host.h.  Each per-frame step of a rule is stated here once, and compiled by (DESIGN.md
// section 23, which also says which kernels restate a step, and why):
//   StatsAdd, NormFinalize, NormApply: pk_norm.cc, NormKernel (norm.hip), StreamNormKernel (stream.hip)
//   WindowStep, MakeOnlinePrior, OnlineCmvnFinalize: pk_norm.cc, StreamNormKernel (OnlineCmvnKernel: the last only)
//   SlidingSum, SlidingApply: CmvnKernel (frontend.hip), CmvnChainKernel, StreamCmvnChainKernel, tests/cpp/norm_test.cc
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

// One frame's value and square into a column's statistics, in double; the callers walk t ascending (AccCmvnStats).
PK_NORM_HD inline void StatsAdd(double &s0, double &s1, float x) {
  const double v = (double)x;
  s0 = s0 + v;
  s1 = s1 + v * v;
}

// ---- The sliding rule (cmvn.cc:35-101), one frame of one column.  The window decisions arrive as booleans: slid is
// t >= 600 (frame t - 600 leaves), smooth is t + 1 < 600; alpha and neg_scale are CmvnTables' entries of frame
// min(t, 599) (pk_tables.h), g the column's global sum.  The window sum behind frame t: widen, add, subtract, narrow.
PK_NORM_HD inline float SlidingSum(float s, float x, float old, bool slid) {
  double acc = s;                                 // cmvn.cc:44-52
  acc += x;
  if (slid) acc += -1.0 * (double)old;            // cmvn.cc:58-64
  return (float)acc;                              // cmvn.cc:66-70
}

// y_t from x_t and the window sum behind frame t: rounded products and rounded adds (built with -ffp-contract=off)
PK_NORM_HD inline float SlidingApply(float x, float s, float alpha, float neg_scale, float g, bool smooth) {
  float st = s;
  if (smooth) st += alpha * g;                    // cmvn.cc:73-92 (count < window)
  float y = x;
  y += neg_scale * st;                            // cmvn.cc:94-101
  return y;
}

// ---- Online CMVN (include/pk_mi355.h)
constexpr int kNormOnlineCmvn = 4;       // what a batch's norm.mode holds under pk_mi355_norm_set_online_cmvn (no public mode: pk_mi355_norm_check refuses it)
constexpr int kMaxCmnWindow = 6000;

// What smooths a window that is not full yet, for one column: the spec's frame limits and the two records' entries.
struct OnlinePrior {
  double window;           // W
  double speaker_frames, speaker_count, spk0, spk1;     // speaker_count 0: no speaker prior
  double global_frames, global_count, glob0, glob1;     // global_frames 0: no global prior
};

// The prior of column d from the records [2][D + 1]; a null glob or spk is "no global prior", "no speaker prior".  Every
// caller (LaunchOnlineCmvn, StreamNormKernel, the host entry) passes glob exactly when global_frames > 0: one condition.
PK_NORM_HD inline OnlinePrior MakeOnlinePrior(int W, int speaker_frames, int global_frames, const double *glob, const double *spk,
                                              int D, int d) {
  OnlinePrior p;
  p.window = (double)W;
  p.speaker_frames = (double)speaker_frames;
  p.global_frames = glob ? (double)global_frames : 0.0;
  p.global_count = glob ? glob[D] : 0.0;
  p.glob0 = glob ? glob[d] : 0.0;
  p.glob1 = glob ? glob[D + 1 + d] : 0.0;
  p.speaker_count = spk ? spk[D] : 0.0;
  p.spk0 = spk ? spk[d] : 0.0;
  p.spk1 = spk ? spk[D + 1 + d] : 0.0;
  return p;
}

// Steps 1 and 2 of the rule, one frame of one column: both additions of x[t], then, once slid (t >= W), both subtractions.
PK_NORM_HD inline void WindowStep(double &S0, double &S1, float x, float old, bool slid) {
  StatsAdd(S0, S1, x);
  if (slid) {
    const double o = (double)old;
    S0 = S0 - o;
    S1 = S1 - o * o;
  }
}

// Steps 3 to 5 of the rule for one frame of one column: the window's sums S0, S1 behind frame t and seen = t + 1 ->
// what the apply step adds and multiplies by.
PK_NORM_HD inline void OnlineCmvnFinalize(double S0, double S1, double seen, const OnlinePrior &p, bool norm_vars, float *offs_f, float *scale_f) {
  double s0 = S0, s1 = S1, n = seen < p.window ? seen : p.window;
  if (n < p.window) {
    if (p.speaker_count > 0.0) {
      double c = p.window - n;
      if (p.speaker_frames < c) c = p.speaker_frames;
      if (p.speaker_count < c) c = p.speaker_count;
      if (c > 0.0) {
        const double f = c / p.speaker_count;
        const double a0 = f * p.spk0, a1 = f * p.spk1, an = f * p.speaker_count;
        s0 = s0 + a0;
        s1 = s1 + a1;
        n = n + an;
      }
    }
    if (n < p.window && p.global_frames > 0.0) {
      double c = p.window - n;
      if (p.global_frames < c) c = p.global_frames;
      const double f = c / p.global_count;
      const double a0 = f * p.glob0, a1 = f * p.glob1, an = f * p.global_count;
      s0 = s0 + a0;
      s1 = s1 + a1;
      n = n + an;
    }
  }
  NormFinalize(s0, s1, n, true, norm_vars, offs_f, scale_f);
}

// pk_mi355_online_cmvn_check
int CheckOnlineSpec(const pk_mi355_online_cmvn_spec_t *spec, const double *global_stats, int dim);
// Speaker records [num_utts][2][dim + 1] of online CMVN: every count finite and not negative (0: no prior), else
// PK_MI355_E_INVALID naming the utterance.
int CheckOnlineSpeakerCounts(const double *stats, int num_utts, int dim);

// pk_mi355_norm_check
int CheckSpec(const pk_mi355_norm_spec_t *spec);
// true for the modes whose kernel reads the switches
inline bool UsesStats(int mode) { return mode == PK_MI355_NORM_UTTERANCE || mode == PK_MI355_NORM_SPEAKER; }
// Speaker records [num_utts][2][dim + 1] -> table [num_utts][2][dim] (row 0 the offsets, row 1 the scales).  Every count
// is checked first (PK_MI355_E_INVALID naming the utterance); nothing is written when one is bad.
int FinalizeSpeakerStats(const double *stats, int num_utts, int dim, bool norm_means, bool norm_vars, float *table);

}  // namespace pknorm

#endif  // PK_NORM_H_
