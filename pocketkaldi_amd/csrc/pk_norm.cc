// pk_norm.cc -- the normalisation spec on the host (pk_norm.h): the check, the speaker records'
// finalisation and the whole rule for one matrix; and online CMVN: its check and the whole rule for
// one matrix.  No HIP: g++ builds it, into the library and into tests/cpp/norm_test.cc and online_cmvn_test.cc.
#include "pk_norm.h"

#include <cmath>
#include <vector>

#include "pk_files.h"

namespace pknorm {

using pkhost::Fail;

int CheckSpec(const pk_mi355_norm_spec_t *spec) {
  if (!spec) return Fail(PK_MI355_E_INVALID, "null argument");
  const pk_mi355_norm_spec_t &s = *spec;
  if (s.mode < PK_MI355_NORM_SLIDING || s.mode > PK_MI355_NORM_SPEAKER)
    return Fail(PK_MI355_E_INVALID, "norm spec: unknown mode %d (0 sliding, 1 none, 2 utterance, 3 speaker)", s.mode);
  if (s.mode == PK_MI355_NORM_NONE) return 0;
  if (s.norm_means != 0 && s.norm_means != 1) return Fail(PK_MI355_E_INVALID, "norm spec: norm_means %d is neither 0 nor 1", s.norm_means);
  if (s.norm_vars != 0 && s.norm_vars != 1) return Fail(PK_MI355_E_INVALID, "norm spec: norm_vars %d is neither 0 nor 1", s.norm_vars);
  if (s.mode == PK_MI355_NORM_SLIDING) {
    if (!s.norm_means) return Fail(PK_MI355_E_INVALID, "norm spec: norm_means must be 1 in mode sliding (the sliding rule is a mean normalisation)");
    if (s.norm_vars) return Fail(PK_MI355_E_INVALID, "norm spec: norm_vars must be 0 in mode sliding (the sliding rule has no variance)");
    return 0;
  }
  if (!s.norm_means && !s.norm_vars)
    return Fail(PK_MI355_E_INVALID, "norm spec: norm_means and norm_vars are both 0 in mode %s: use mode none",
                s.mode == PK_MI355_NORM_UTTERANCE ? "utterance" : "speaker");
  return 0;
}

int FinalizeSpeakerStats(const double *stats, int num_utts, int dim, bool norm_means, bool norm_vars, float *table) {
  if (num_utts > 0 && (!stats || !table)) return Fail(PK_MI355_E_INVALID, "null argument");
  if (dim <= 0) return Fail(PK_MI355_E_INVALID, "speaker statistics: dimension %d", dim);
  const size_t rec = 2 * ((size_t)dim + 1);
  for (int u = 0; u < num_utts; ++u) {
    const double n = stats[u * rec + dim];
    if (!std::isfinite(n) || !(n > 0.0))
      return Fail(PK_MI355_E_INVALID, "speaker statistics of utterance %d: the count %g is not positive and finite", u, n);
  }
  for (int u = 0; u < num_utts; ++u) {
    const double *s0 = stats + u * rec, *s1 = s0 + dim + 1;
    float *offs = table + (size_t)u * 2 * dim, *scale = offs + dim;
    for (int d = 0; d < dim; ++d) NormFinalize(s0[d], s1[d], s0[dim], norm_means, norm_vars, &offs[d], &scale[d]);
  }
  return 0;
}

int CheckOnlineSpec(const pk_mi355_online_cmvn_spec_t *spec, const double *global_stats, int dim) {
  if (!spec) return Fail(PK_MI355_E_INVALID, "null argument");
  const pk_mi355_online_cmvn_spec_t &s = *spec;
  if (s.cmn_window < 1 || s.cmn_window > kMaxCmnWindow)
    return Fail(PK_MI355_E_INVALID, "online cmvn spec: cmn_window %d is outside [1, %d]", s.cmn_window, kMaxCmnWindow);
  if (s.speaker_frames < 0) return Fail(PK_MI355_E_INVALID, "online cmvn spec: speaker_frames %d is negative", s.speaker_frames);
  if (s.global_frames < 0) return Fail(PK_MI355_E_INVALID, "online cmvn spec: global_frames %d is negative", s.global_frames);
  if (s.norm_vars != 0 && s.norm_vars != 1) return Fail(PK_MI355_E_INVALID, "online cmvn spec: norm_vars %d is neither 0 nor 1", s.norm_vars);
  if (s.global_frames > 0) {
    if (!global_stats) return Fail(PK_MI355_E_INVALID, "online cmvn spec: global_frames %d needs the global statistics", s.global_frames);
    if (dim <= 0) return Fail(PK_MI355_E_INVALID, "online cmvn: dimension %d", dim);
    const double n = global_stats[dim];
    if (!std::isfinite(n) || !(n > 0.0))
      return Fail(PK_MI355_E_INVALID, "online cmvn spec: global_frames %d with global statistics whose count %g is not positive and finite", s.global_frames, n);
  }
  return 0;
}

int CheckOnlineSpeakerCounts(const double *stats, int num_utts, int dim) {
  if (num_utts > 0 && !stats) return Fail(PK_MI355_E_INVALID, "null argument");
  if (dim <= 0) return Fail(PK_MI355_E_INVALID, "speaker statistics: dimension %d", dim);
  const size_t rec = 2 * ((size_t)dim + 1);
  for (int u = 0; u < num_utts; ++u) {
    const double n = stats[u * rec + dim];
    if (!std::isfinite(n) || n < 0.0)
      return Fail(PK_MI355_E_INVALID, "speaker statistics of utterance %d: the count %g is negative or not finite", u, n);
  }
  return 0;
}

}  // namespace pknorm

extern "C" {

int pk_mi355_online_cmvn_check(const pk_mi355_online_cmvn_spec_t *spec, const double *global_stats, int dim) {
  return pknorm::CheckOnlineSpec(spec, global_stats, dim);
}

int pk_mi355_online_cmvn_apply(const pk_mi355_online_cmvn_spec_t *spec, const float *x, int num_frames, int dim, const double *global_stats,
                               const double *speaker_stats, float *y, double *state_out) {
  using namespace pknorm;
  if (int rc = CheckOnlineSpec(spec, global_stats, dim)) return rc;
  if (num_frames < 0 || dim <= 0) return Fail(PK_MI355_E_INVALID, "bad shape (%d frames of %d features)", num_frames, dim);
  if (num_frames > 0 && (!x || !y)) return Fail(PK_MI355_E_INVALID, "null argument");
  if (speaker_stats)
    if (int rc = CheckOnlineSpeakerCounts(speaker_stats, 1, dim)) return rc;
  const size_t T = (size_t)num_frames, D = (size_t)dim, W = (size_t)spec->cmn_window;
  const bool vars = spec->norm_vars != 0;
  const double *glob = spec->global_frames > 0 ? global_stats : nullptr;       // (checked above: not null when asked for)
  std::vector<double> state(2 * (D + 1), 0.0);
  for (size_t d = 0; d < D; ++d) {
    const OnlinePrior p = MakeOnlinePrior(spec->cmn_window, spec->speaker_frames, spec->global_frames, glob, speaker_stats, dim, (int)d);
    double S0 = 0.0, S1 = 0.0;
    for (size_t t = 0; t < T; ++t) {
      WindowStep(S0, S1, x[t * D + d], t >= W ? x[(t - W) * D + d] : 0.0f, t >= W);
      float offs, scale;
      OnlineCmvnFinalize(S0, S1, (double)(t + 1), p, vars, &offs, &scale);
      y[t * D + d] = NormApply(x[t * D + d], offs, scale, vars);
    }
    state[d] = S0;
    state[D + 1 + d] = S1;
  }
  state[D] = (double)num_frames;
  if (state_out) for (size_t i = 0; i < state.size(); ++i) state_out[i] = state[i];
  return 0;
}

int pk_mi355_norm_check(const pk_mi355_norm_spec_t *spec) { return pknorm::CheckSpec(spec); }

int pk_mi355_norm_apply(const pk_mi355_norm_spec_t *spec, const float *x, int num_frames, int dim, const double *stats, float *y,
                        double *stats_out) {
  using namespace pknorm;
  if (int rc = CheckSpec(spec)) return rc;
  if (spec->mode == PK_MI355_NORM_SLIDING) return Fail(PK_MI355_E_INVALID, "norm spec: mode sliding is pk_mi355_cmvn_apply's rule, not this entry's");
  if (num_frames < 0 || dim <= 0) return Fail(PK_MI355_E_INVALID, "bad shape (%d frames of %d features)", num_frames, dim);
  if (num_frames > 0 && (!x || !y)) return Fail(PK_MI355_E_INVALID, "null argument");
  if (spec->mode == PK_MI355_NORM_SPEAKER && !stats) return Fail(PK_MI355_E_INVALID, "mode speaker needs a statistics record");
  const size_t T = (size_t)num_frames, D = (size_t)dim;
  if (spec->mode == PK_MI355_NORM_NONE) {
    for (size_t i = 0; i < T * D; ++i) y[i] = x[i];
    return 0;
  }
  const bool means = spec->norm_means != 0, vars = spec->norm_vars != 0;
  std::vector<float> table(2 * D);
  if (spec->mode == PK_MI355_NORM_SPEAKER) {
    if (int rc = FinalizeSpeakerStats(stats, 1, dim, means, vars, table.data())) return rc;
  } else {
    std::vector<double> rec(2 * (D + 1), 0.0);
    for (size_t t = 0; t < T; ++t)
      for (size_t d = 0; d < D; ++d) StatsAdd(rec[d], rec[D + 1 + d], x[t * D + d]);
    rec[D] = (double)num_frames;
    if (stats_out) for (size_t i = 0; i < rec.size(); ++i) stats_out[i] = rec[i];
    if (T == 0) return 0;
    for (size_t d = 0; d < D; ++d) NormFinalize(rec[d], rec[D + 1 + d], rec[D], means, vars, &table[d], &table[D + d]);
  }
  for (size_t t = 0; t < T; ++t)
    for (size_t d = 0; d < D; ++d) y[t * D + d] = NormApply(x[t * D + d], table[d], table[D + d], vars);
  return 0;
}

}  // extern "C"
