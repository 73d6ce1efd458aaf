// frontend_example.cc -- audio into a model that is not the reference's 40-bin fbank: an 80-bin Povey-window fbank
// front-end (pocketkaldi::FrontendSpec::Fbank(80), Kaldi's defaults) in front of an 80-dim model, through
// pocketkaldi::BatchScorer's front-end constructor with the 81 statistics of a Kaldi global CMVN file
// (include/pocketkaldi_amd.hpp).  The model is a small one made in memory (L = 2, R = 1, one affine layer of 16 pdfs and
// a softmax; weight k is ((k * 2654435761 mod 2^32) >> 16) / 65536 - 0.5, scaled by 0.05), so that the test can build
// the same model.  It prints the frames and the 64-bit FNV-1a of the feature rows' and of the log-likelihood rows' bytes;
// pocketkaldi::Frontend::Compute on the same wave must give the batch's feature rows.
//
//   frontend_example <16 kHz wav> <global-cmvn-stats file>
//   frontend_example --link-only        (exits before touching the GPU)
// Built and run by tests/test_cpp_frontend.py.
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
  if (argc < 3) {
    fprintf(stderr, "usage: %s wave.wav global-cmvn-stats\n", argv[0]);
    return 64;
  }
  const pocketkaldi::FrontendSpec spec = pocketkaldi::FrontendSpec::Fbank(80);
  const int D = spec.dim(), L = 2, R = 1, N = 16;
  if (D != 80 || !spec.Check().ok()) {
    fprintf(stderr, "spec: %s\n", pk_mi355_last_error());
    return 1;
  }
  {   // a spec the library refuses says which field
    pocketkaldi::FrontendSpec bad = pocketkaldi::FrontendSpec::Mfcc(23, 24);
    if (bad.Check().ok() || bad.dim() >= 0 || bad.Check().what().find("num_ceps") == std::string::npos) {
      fprintf(stderr, "a 24-of-23 MFCC spec was not refused by name\n");
      return 1;
    }
  }
  std::vector<float> stats;
  int rows = 0, cols = 0;
  pocketkaldi::Status st = pocketkaldi::ArkReader::ReadObject(argv[2], &stats, &rows, &cols);
  if (!st.ok() || rows != 2 || cols != D + 1) {
    fprintf(stderr, "statistics: %s (%d x %d)\n", st.what().c_str(), rows, cols);
    return 1;
  }
  pk_vector_t wave = {0, nullptr};
  if (pk_mi355_16kpcm_read(argv[1], &wave) != 0) {
    fprintf(stderr, "wave: %s\n", pk_mi355_last_error());
    return 1;
  }
  pocketkaldi::AcousticModel am;
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
  {   // the dimensions must agree, and the refusal names both
    pocketkaldi::BatchScorer wrong(am.handle(), pocketkaldi::FrontendSpec::Mfcc(23, 13), stats.data(), D + 1, 1, wave.dim + 1);
    if (wrong.last_status().ok() || wrong.last_status().what().find("13") == std::string::npos ||
        wrong.last_status().what().find("80") == std::string::npos) {
      fprintf(stderr, "a 13-dim front-end on an 80-dim model: %s\n", wrong.last_status().what().c_str());
      return 1;
    }
  }
  pocketkaldi::BatchScorer scorer(am.handle(), spec, stats.data(), D + 1, 1, wave.dim + 1);
  if (!scorer.last_status().ok()) {
    fprintf(stderr, "create: %s\n", scorer.last_status().what().c_str());
    return 1;
  }
  st = scorer.SetWaves(&wave, 1);
  if (st.ok()) st = scorer.Score(0.1f);
  if (!st.ok()) {
    fprintf(stderr, "score: %s\n", st.what().c_str());
    return 1;
  }
  const int T = scorer.NumFrames(0);
  std::vector<float> rows_batch((size_t)T * D);
  st = scorer.FetchFeatures(0, rows_batch.data());
  pocketkaldi::Frontend frontend(spec);
  pk_matrix_t feats = {0, 0, nullptr};
  frontend.Compute(&wave, &feats);
  if (!st.ok() || !frontend.last_status().ok() || feats.ncol != T || feats.nrow != D ||
      memcmp(feats.data, rows_batch.data(), sizeof(float) * rows_batch.size()) != 0) {
    fprintf(stderr, "Frontend::Compute and the batch's rows differ (%d x %d against %d x %d)\n", feats.ncol, feats.nrow, T, D);
    return 1;
  }
  pk_decodable_t out;
  st = scorer.Fetch(0, &out);
  if (!st.ok() || out.log_prob.ncol != T || out.log_prob.nrow != N) {
    fprintf(stderr, "fetch: %s\n", st.what().c_str());
    return 1;
  }
  printf("frames %d dim %d\n", T, D);
  printf("features %016llx\n", Fnv(feats.data, sizeof(float) * (size_t)T * D));
  printf("loglik %016llx\n", Fnv(out.log_prob.data, sizeof(float) * (size_t)T * N));
  pk_decodable_destroy(&out);
  free(feats.data);
  free(wave.data);
  printf("frontend_example ok\n");
  return 0;
}
