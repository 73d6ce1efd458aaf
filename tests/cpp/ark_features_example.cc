// ark_features_example.cc -- raw features from a Kaldi archive, normalised on the GPU at the model's own dimension:
// every entry of the archive (pocketkaldi::ArkReader) goes, 10 frames a step, as PK_MI355_FEATS_RAW through a
// features-only pocketkaldi::OnlineScorer made with the D + 1 statistics of a Kaldi global CMVN file
// (ArkReader::ReadObject; include/pocketkaldi_amd.hpp).  The model is a small one made in memory at the archive's
// dimension D (L = 2, R = 1, one affine layer of 16 pdfs and a softmax; weight k is ((k * 2654435761 mod 2^32) >> 16) /
// 65536 - 0.5, scaled by 0.05), so that the test can build the same model.  It prints per entry the key, the frames
// and the 64-bit FNV-1a of the log-likelihood rows' bytes.
//
//   ark_features_example <feats.ark | feats.scp> <global-cmvn-stats file>
//   ark_features_example --link-only        (exits before touching the GPU)
// Built and run by tests/test_cpp_ark_features.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pocketkaldi_amd.hpp"

static float Weight(uint32_t k) { return ((float)((k * 2654435761u) >> 16) / 65536.0f - 0.5f) * 0.05f; }

int main(int argc, char **argv) {
  if (argc >= 2 && strcmp(argv[1], "--link-only") == 0) {
    printf("%s\n", pk_mi355_version());
    return 0;
  }
  if (argc < 3) {
    fprintf(stderr, "usage: %s feats.ark global-cmvn-stats\n", argv[0]);
    return 64;
  }
  std::vector<float> stats;
  int rows = 0, cols = 0;
  pocketkaldi::Status st = pocketkaldi::ArkReader::ReadObject(argv[2], &stats, &rows, &cols);
  if (!st.ok() || rows != 2 || cols < 2) {
    fprintf(stderr, "statistics: %s (%d x %d)\n", st.what().c_str(), rows, cols);
    return 1;
  }
  const int D = cols - 1, L = 2, R = 1, N = 16;            // row 0: D sums, then the count
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
  const int chunk = 10;
  pocketkaldi::OnlineScorer scorer(pocketkaldi::OnlineScorer::kFeaturesOnly, am.handle(), stats.data(), D + 1, 1, chunk);
  if (!scorer.last_status().ok()) {
    fprintf(stderr, "create: %s\n", scorer.last_status().what().c_str());
    return 1;
  }
  {   // the 41-float entry refuses this model unless it is 40-dim
    pocketkaldi::OnlineScorer old(pocketkaldi::OnlineScorer::kFeaturesOnly, am.handle(), stats.data(), 1, chunk);
    if (old.last_status().ok() != (D == 40)) {
      fprintf(stderr, "the 41-float entry: unexpected verdict at D = %d\n", D);
      return 1;
    }
  }
  pocketkaldi::ArkReader reader(argv[1]);
  if (!reader.last_status().ok()) {
    fprintf(stderr, "open: %s\n", reader.last_status().what().c_str());
    return 1;
  }
  int entries = 0;
  while (reader.Next()) {
    const pk_matrix_t m = reader.Matrix();
    if (m.ncol > 0 && m.nrow != D) {
      fprintf(stderr, "%s: %d-dim features, the statistics are %d-dim\n", reader.Key().c_str(), m.nrow, D);
      return 1;
    }
    unsigned long long h = 14695981039346656037ull;
    int T = 0;
    st = scorer.OpenFeatures(0, PK_MI355_FEATS_RAW);
    for (int pos = 0; st.ok(); pos += chunk) {
      const bool last = pos >= m.ncol;
      if (!last) st = scorer.PushFeatures(0, m.data + (size_t)pos * D, std::min(chunk, m.ncol - pos));
      else st = scorer.Close(0);
      if (st.ok()) st = scorer.Step(0.1f);
      if (!st.ok()) break;
      pk_decodable_t out;
      int first = 0;
      st = scorer.Fetch(0, &out, &first);
      if (!st.ok()) break;
      if (out.log_prob.ncol > 0 && first != T) {
        fprintf(stderr, "%s: rows from frame %d, %d expected\n", reader.Key().c_str(), first, T);
        return 1;
      }
      const unsigned char *p = reinterpret_cast<const unsigned char *>(out.log_prob.data);
      for (size_t i = 0; i < sizeof(float) * (size_t)out.log_prob.ncol * out.log_prob.nrow; ++i) h = (h ^ p[i]) * 1099511628211ull;
      T += out.log_prob.ncol;
      pk_decodable_destroy(&out);
      if (last) break;
    }
    if (!st.ok()) {
      fprintf(stderr, "%s: %s\n", reader.Key().c_str(), st.what().c_str());
      return 1;
    }
    printf("entry %s frames %d loglik %016llx\n", reader.Key().c_str(), T, h);
    ++entries;
  }
  if (!reader.last_status().ok()) {
    fprintf(stderr, "read: %s\n", reader.last_status().what().c_str());
    return 1;
  }
  printf("entries: %d\nark_features_example ok\n", entries);
  return 0;
}
