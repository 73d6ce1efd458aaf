// norm_example.cc -- audio into a model that was trained with per-utterance mean and variance normalisation: an 80-bin
// Povey-window fbank front-end in front of an 80-dim model, pocketkaldi::BatchScorer::SetNorm(NormSpec::Utterance(true,
// true)) (include/pocketkaldi_amd.hpp).  The model is frontend_example.cc's (L = 2, R = 1, one
// affine layer of 16 pdfs and a softmax, the same weights), so that the test can build it too.  It prints the frames and
// the 64-bit FNV-1a of the normalised rows', of the statistics record's and of the log-likelihood rows' bytes; then it
// scores the wave again in mode speaker on the record it fetched, which must give the same rows bit for bit.
//
//   norm_example <16 kHz wav>
//   norm_example --link-only        (exits before touching the GPU)
// Built and run by tests/test_cpp_norm.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "pocketkaldi_amd.hpp"

static float Weight(uint32_t k) { return ((float)((k * 2654435761u) >> 16) / 65536.0f - 0.5f) * 0.05f; }

static unsigned long long Fnv(const void *data, size_t bytes) {
  unsigned long long h = 14695981039346656037ull;
  const unsigned char *p = static_cast<const unsigned char *>(data);
  for (size_t i = 0; i < bytes; ++i) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

int main(int argc, char **argv) {
  if (argc >= 2 && strcmp(argv[1], "--link-only") == 0) {
    printf("%s\n", pk_mi355_version());
    return 0;
  }
  if (argc < 2) {
    fprintf(stderr, "usage: %s wave.wav\n", argv[0]);
    return 64;
  }
  const pocketkaldi::FrontendSpec spec = pocketkaldi::FrontendSpec::Fbank(80);
  const int D = spec.dim(), L = 2, R = 1, N = 16;
  {   // a spec the library refuses says which field
    pocketkaldi::NormSpec bad = pocketkaldi::NormSpec::Utterance(false, false);
    if (bad.Check().ok() || bad.Check().what().find("use mode none") == std::string::npos || !pocketkaldi::NormSpec().Check().ok()) {
      fprintf(stderr, "a spec without either switch was not refused by name\n");
      return 1;
    }
  }
  pk_vector_t wave = {0, nullptr};
  if (pk_mi355_16kpcm_read(argv[1], &wave) != 0) {
    fprintf(stderr, "wave: %s\n", pk_mi355_last_error());
    return 1;
  }
  pocketkaldi::AcousticModel am;
  pocketkaldi::Status st;
  {
    const int in = D * (L + R + 1);
    std::vector<float> W((size_t)N * in), b(N), prior(N, 1.0f / N);
    for (size_t k = 0; k < W.size(); ++k) W[k] = Weight((uint32_t)k);
    for (int k = 0; k < N; ++k) b[k] = Weight(1000003u + k);
    st = am.AddLinear(in, N, W.data(), b.data());
    if (st.ok()) st = am.AddLayer(PK_NNET_SOFTMAX_LAYER);
    if (st.ok()) st = am.Finalize(prior, L, R, std::vector<int32_t>());
    if (!st.ok() || am.feat_dim() != D) {
      fprintf(stderr, "model: %s\n", st.what().c_str());
      return 1;
    }
  }
  std::vector<float> global(D + 1, 0.0f);          // the sliding rule's statistics: the object needs some, this program's modes read none
  global[D] = 1.0f;
  pocketkaldi::BatchScorer scorer(am.handle(), spec, global.data(), D + 1, 1, wave.dim + 1);
  if (!scorer.last_status().ok()) {
    fprintf(stderr, "create: %s\n", scorer.last_status().what().c_str());
    return 1;
  }
  st = scorer.SetNorm(pocketkaldi::NormSpec::Utterance(true, true));
  if (st.ok()) st = scorer.SetWaves(&wave, 1);
  if (st.ok()) st = scorer.Score(0.1f);
  if (!st.ok()) {
    fprintf(stderr, "score: %s\n", st.what().c_str());
    return 1;
  }
  const int T = scorer.NumFrames(0);
  std::vector<float> rows((size_t)T * D), again((size_t)T * D);
  std::vector<double> record;
  pk_decodable_t out, out2;
  st = scorer.FetchNormalized(0, rows.data());
  if (st.ok()) st = scorer.NormStats(0, &record);
  if (st.ok()) st = scorer.Fetch(0, &out);
  if (!st.ok() || out.log_prob.ncol != T || out.log_prob.nrow != N || record[D] != (double)T) {
    fprintf(stderr, "fetch: %s\n", st.what().c_str());
    return 1;
  }
  printf("frames %d dim %d\n", T, D);
  printf("normalized %016llx\n", Fnv(rows.data(), sizeof(float) * rows.size()));
  printf("stats %016llx\n", Fnv(record.data(), sizeof(double) * record.size()));
  printf("loglik %016llx\n", Fnv(out.log_prob.data, sizeof(float) * (size_t)T * N));
  // the same wave as its own speaker: the utterance call's bits; the records are consumed by one Score
  st = scorer.SetNorm(pocketkaldi::NormSpec::Speaker(true, true));
  if (st.ok()) st = scorer.SetWaves(&wave, 1);
  if (st.ok() && scorer.Score(0.1f).code() != PK_MI355_E_STATE) st = pocketkaldi::Status(PK_MI355_E_STATE, "mode speaker scored without statistics");
  if (st.ok()) st = scorer.SetSpeakerStats(record.data(), 1);
  if (st.ok()) st = scorer.Score(0.1f);
  if (st.ok()) st = scorer.FetchNormalized(0, again.data());
  if (st.ok()) st = scorer.Fetch(0, &out2);
  if (!st.ok() || memcmp(rows.data(), again.data(), sizeof(float) * rows.size()) != 0 ||
      memcmp(out.log_prob.data, out2.log_prob.data, sizeof(float) * (size_t)T * N) != 0) {
    fprintf(stderr, "mode speaker on the utterance's own record differs: %s\n", st.what().c_str());
    return 1;
  }
  if (scorer.Score(0.1f).code() != PK_MI355_E_STATE || scorer.NormStats(0, &record).code() != PK_MI355_E_STATE) {
    fprintf(stderr, "the speaker records were not consumed\n");
    return 1;
  }
  pk_decodable_destroy(&out);
  pk_decodable_destroy(&out2);
  free(wave.data);
  printf("norm_example ok\n");
  return 0;
}
