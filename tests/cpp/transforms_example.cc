// transforms_example.cc -- audio into a model that was trained on compute-mfcc-feats | apply-cmvn | splice-feats
// --left-context=3 --right-context=3 | transform-feats final.mat | transform-feats trans.ark (LDA+MLLT+SAT): a 13-of-23
// MFCC front-end, pocketkaldi::BatchScorer with a TransformSpec of 91 -> 40 affine (include/pocketkaldi_amd.hpp,
// DESIGN.md section 25), per-utterance mean and variance normalisation and one per-utterance 40 x 41 matrix in front of
// a 40-dim model.  L = 2, R = 1, one affine layer of 16 pdfs and a softmax with frontend_example.cc's weight rule; the
// matrices follow the same rule (global entry k: 20 Weight(5000011 + k); per-utterance entry k: 20 Weight(7000003 + k),
// plus 1 on the diagonal), so that the test can build everything too.  It prints the frames and the 64-bit FNV-1a of the
// front-end's rows', of the first layer's input rows' and of the log-likelihood rows' bytes; the first layer's input
// must be TransformSpec::Apply twice over the normalised front-end rows, bit for bit.
//
//   transforms_example <16 kHz wav>
//   transforms_example --link-only        (exits before touching the GPU)
// Built and run by tests/test_gpu_recognize_transforms.py.
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
  const pocketkaldi::FrontendSpec spec = pocketkaldi::FrontendSpec::Mfcc(23, 13);
  const int Db = spec.dim(), ctx = 3, K = (2 * ctx + 1) * Db, D = 40, L = 2, R = 1, N = 16;
  std::vector<float> global_m((size_t)D * (K + 1)), utt_m((size_t)D * (D + 1));
  for (size_t k = 0; k < global_m.size(); ++k) global_m[k] = 20.0f * Weight(5000011u + (uint32_t)k);
  for (size_t k = 0; k < utt_m.size(); ++k) utt_m[k] = 20.0f * Weight(7000003u + (uint32_t)k) + (k / (D + 1) == k % (D + 1) ? 1.0f : 0.0f);
  const pocketkaldi::TransformSpec transform(global_m.data(), D, K + 1, Db, ctx, ctx);
  const pocketkaldi::TransformSpec per_utt(utt_m.data(), D, D + 1, D);
  {   // a spec the library refuses says which field
    pocketkaldi::TransformSpec bad(global_m.data(), D, K + 1, Db, ctx, ctx + 1);
    if (bad.Check().ok() || bad.Check().what().find("cols 92") == std::string::npos || !transform.Check().ok() || transform.out_dim() != D) {
      fprintf(stderr, "92 columns at a window of 8 were not refused by name\n");
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
  std::vector<float> global(Db + 1, 0.0f);         // the sliding rule's statistics: the object needs some, this program's mode reads none
  global[Db] = 1.0f;
  {   // statistics at the model's dimension instead of the front-end's are refused with both numbers
    pocketkaldi::BatchScorer wrong(am.handle(), spec, nullptr, transform, std::vector<float>(D + 1, 1.0f).data(), D + 1, 1, wave.dim + 1);
    if (wrong.last_status().ok() || wrong.last_status().what().find("14") == std::string::npos) {
      fprintf(stderr, "statistics of 41 entries were not refused: %s\n", wrong.last_status().what().c_str());
      return 1;
    }
  }
  pocketkaldi::BatchScorer scorer(am.handle(), spec, nullptr, transform, global.data(), Db + 1, 1, wave.dim + 1);
  if (!scorer.last_status().ok() || scorer.BaseDim() != Db || scorer.InDim() != Db || scorer.FeatDim() != D) {
    fprintf(stderr, "create: %s\n", scorer.last_status().what().c_str());
    return 1;
  }
  st = scorer.SetNorm(pocketkaldi::NormSpec::Utterance(true, true));
  if (st.ok()) st = scorer.SetWaves(&wave, 1);
  if (st.ok()) st = scorer.SetUttTransforms(utt_m.data(), D + 1, 1);
  if (st.ok()) st = scorer.Score(0.1f);
  if (!st.ok()) {
    fprintf(stderr, "score: %s\n", st.what().c_str());
    return 1;
  }
  const int T = scorer.NumFrames(0);
  std::vector<float> base((size_t)T * Db), rows((size_t)T * D), normalized((size_t)T * Db), mid, host;
  pk_decodable_t out;
  st = scorer.FetchFeatures(0, base.data());
  if (st.ok()) st = scorer.FetchNormalized(0, rows.data());
  if (st.ok()) st = scorer.Fetch(0, &out);
  if (!st.ok() || out.log_prob.ncol != T || out.log_prob.nrow != N) {
    fprintf(stderr, "fetch: %s\n", st.what().c_str());
    return 1;
  }
  // the same rows on the host: the norm's rule, then the transform's rule twice
  pocketkaldi::NormSpec utt = pocketkaldi::NormSpec::Utterance(true, true);
  if (pk_mi355_norm_apply(&utt, base.data(), T, Db, nullptr, normalized.data(), nullptr) != 0 || !transform.Apply(normalized.data(), T, &mid).ok() ||
      !per_utt.Apply(mid.data(), T, &host).ok() || host.size() != rows.size() || memcmp(host.data(), rows.data(), sizeof(float) * rows.size()) != 0) {
    fprintf(stderr, "the first layer's input is not the host rule's: %s\n", pk_mi355_last_error());
    return 1;
  }
  printf("frames %d base %d dim %d\n", T, Db, D);
  printf("features %016llx\n", Fnv(base.data(), sizeof(float) * base.size()));
  printf("transformed %016llx\n", Fnv(rows.data(), sizeof(float) * rows.size()));
  printf("loglik %016llx\n", Fnv(out.log_prob.data, sizeof(float) * (size_t)T * N));
  pk_decodable_destroy(&out);
  free(wave.data);
  printf("transforms_example ok\n");
  return 0;
}
