// time_splice_example.cc -- a small TDNN through include/pocketkaldi_amd.hpp: on 6-dim features with
// two frames of left and one of right context, Linear 24 -> 40, p-norm -> 10, Normalize, a time-splice {-1, 2}, Linear
// 20 -> 34, ReLU, a time-splice {-3, 3}, Linear 68 -> 12, tanh, Linear 12 -> 7, Softmax.  The time-splice layers consume
// 4 frames on the left and 5 on the right.  Weights follow layer_kinds_example.cc's rule (W entry k of linear layer l:
// 8 Weight(l 1000003 + k), bias entry k: Weight(500009 + l 1000003 + k)), feature entry i of 37 frames:
// 40 Weight(6000011 + i), so that the test can build everything too.  It scores the one utterance and prints rows 0, 17
// and 36 and the 64-bit FNV-1a of all rows' bytes.
//
//   time_splice_example
//   time_splice_example --link-only        (exits before touching the GPU)
// Built and run by tests/test_gpu_time_splice.py.
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

static pocketkaldi::Status AddLinear(pocketkaldi::AcousticModel *am, int l, int in, int out) {
  std::vector<float> W((size_t)out * in), b(out);
  for (size_t k = 0; k < W.size(); ++k) W[k] = 8.0f * Weight((uint32_t)l * 1000003u + (uint32_t)k);
  for (int k = 0; k < out; ++k) b[k] = Weight(500009u + (uint32_t)l * 1000003u + (uint32_t)k);
  return am->AddLinear(in, out, W.data(), b.data());
}

int main(int argc, char **argv) {
  if (argc >= 2 && strcmp(argv[1], "--link-only") == 0) {
    printf("%s\n", pk_mi355_version());
    return 0;
  }
  const int D = 6, L = 2, R = 1, N = 7, T = 37;
  pocketkaldi::AcousticModel am;
  pocketkaldi::Status st;
  {   // what the library refuses says why
    pocketkaldi::AcousticModel bad;
    st = bad.AddTimeSplice(10, {-1, 2, 2});
    if (st.ok() || st.what().find("offset 2 (index 2) follows 2") == std::string::npos) {
      fprintf(stderr, "offsets out of order were not refused by name: %s\n", st.what().c_str());
      return 1;
    }
    st = bad.AddTimeSplice(10, std::vector<int32_t>());
    if (st.ok()) {
      fprintf(stderr, "an empty offset list was not refused\n");
      return 1;
    }
  }
  st = AddLinear(&am, 0, D * (L + R + 1), 40);
  if (st.ok()) st = am.AddPnorm(40, 10);
  if (st.ok()) st = am.AddLayer(PK_NNET_NORMALIZE_LAYER);
  if (st.ok()) st = am.AddTimeSplice(10, {-1, 2});
  if (st.ok()) st = AddLinear(&am, 1, 20, 34);
  if (st.ok()) st = am.AddLayer(PK_NNET_RELU_LAYER);
  if (st.ok()) st = am.AddTimeSplice(34, {-3, 3});
  if (st.ok()) st = AddLinear(&am, 2, 68, 12);
  if (st.ok()) st = am.AddLayer(PK_MI355_NNET_TANH_LAYER);
  if (st.ok()) st = AddLinear(&am, 3, 12, N);
  if (st.ok()) st = am.AddLayer(PK_NNET_SOFTMAX_LAYER);
  if (st.ok()) st = am.Finalize(std::vector<float>(N, 1.0f / N), L, R, std::vector<int32_t>());
  int lh = -1, rh = -1;
  if (st.ok()) st = am.TimeContext(&lh, &rh);
  if (!st.ok() || am.feat_dim() != D || am.num_pdfs() != N || lh != 4 || rh != 5) {
    fprintf(stderr, "model: %s (time context %d, %d)\n", st.what().c_str(), lh, rh);
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
  printf("frames %d pdfs %d context %d %d\n", T, N, lh, rh);
  for (int t : {0, 17, 36}) {
    printf("row %d:", t);
    for (int k = 0; k < N; ++k) printf(" %.9g", loglik.data[(size_t)t * N + k]);
    printf("\n");
  }
  printf("loglik %016llx\n", Fnv(loglik.data, sizeof(float) * (size_t)T * N));
  free(loglik.data);
  printf("time_splice_example ok\n");
  return 0;
}
