// layer_kinds_example.cc -- an nnet2-style p-norm model through include/pocketkaldi_amd.hpp:
// Linear 24 -> 40, p-norm -> 10 (groups of 4), Normalize, Linear 10 -> 8, a scale (PK_NNET_MUL_LAYER, nnet2's
// FixedScaleComponent) and Softmax on 6-dim features with two frames of left and one of right context.  Weights follow
// frontend_example.cc's rule (W entry k: 8 Weight(k), the second layer's from 2000003 on; biases from 1000003 and 3000017
// on; scale entry k: 1 + 4 Weight(4000037 + k)), feature entry i of 37 frames: 40 Weight(6000011 + i), so that the test
// can build everything too.  It scores the one utterance and prints row 17 and the 64-bit FNV-1a of all rows' bytes.
//
//   layer_kinds_example
//   layer_kinds_example --link-only        (exits before touching the GPU)
// Built and run by tests/test_gpu_layer_kinds.py.
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
  const int D = 6, L = 2, R = 1, in = D * (L + R + 1), H = 40, O = 10, N = 8, T = 37;
  pocketkaldi::AcousticModel am;
  pocketkaldi::Status st;
  {   // what the library refuses says why
    pocketkaldi::AcousticModel bad;
    st = bad.AddPnorm(H, 7);
    if (st.ok() || st.what().find("input width 40 is not a multiple of the output width 7") == std::string::npos) {
      fprintf(stderr, "a p-norm 40 -> 7 was not refused by name: %s\n", st.what().c_str());
      return 1;
    }
    st = bad.AddVectorLayer(PK_NNET_MUL_LAYER, std::vector<float>());
    if (st.ok()) {
      fprintf(stderr, "an empty scale was not refused\n");
      return 1;
    }
  }
  std::vector<float> W1((size_t)H * in), b1(H), W2((size_t)N * O), b2(N), scale(N), prior(N, 1.0f / N);
  for (size_t k = 0; k < W1.size(); ++k) W1[k] = 8.0f * Weight((uint32_t)k);
  for (int k = 0; k < H; ++k) b1[k] = Weight(1000003u + k);
  for (size_t k = 0; k < W2.size(); ++k) W2[k] = 8.0f * Weight(2000003u + (uint32_t)k);
  for (int k = 0; k < N; ++k) b2[k] = Weight(3000017u + k);
  for (int k = 0; k < N; ++k) scale[k] = 1.0f + 4.0f * Weight(4000037u + k);
  st = am.AddLinear(in, H, W1.data(), b1.data());
  if (st.ok()) st = am.AddPnorm(H, O);
  if (st.ok()) st = am.AddLayer(PK_NNET_NORMALIZE_LAYER);
  if (st.ok()) st = am.AddLinear(O, N, W2.data(), b2.data());
  if (st.ok()) st = am.AddVectorLayer(PK_NNET_MUL_LAYER, scale);
  if (st.ok()) st = am.AddLayer(PK_NNET_SOFTMAX_LAYER);
  if (st.ok()) st = am.Finalize(prior, L, R, std::vector<int32_t>());
  if (!st.ok() || am.feat_dim() != D || am.num_pdfs() != N) {
    fprintf(stderr, "model: %s\n", st.what().c_str());
    return 1;
  }
  std::vector<float> feats((size_t)T * D);
  for (size_t i = 0; i < feats.size(); ++i) feats[i] = 40.0f * Weight(6000011u + (uint32_t)i);
  pk_matrix_t frames = {T, D, feats.data()}, loglik = {0, 0, nullptr};
  am.Compute(&frames, &loglik);
  if (loglik.ncol != T || loglik.nrow != N || !loglik.data) {
    fprintf(stderr, "compute: %s\n", pk_mi355_last_error());
    return 1;
  }
  printf("frames %d pdfs %d\n", T, N);
  printf("row 17:");
  for (int k = 0; k < N; ++k) printf(" %.9g", loglik.data[(size_t)17 * N + k]);
  printf("\n");
  printf("loglik %016llx\n", Fnv(loglik.data, sizeof(float) * (size_t)T * N));
  free(loglik.data);
  printf("layer_kinds_example ok\n");
  return 0;
}
