// online_transforms_example.cc -- live audio into a model that was trained on compute-mfcc-feats | apply-cmvn |
// splice-feats | transform-feats final.mat, with a speaker's own 40 x 41 matrix (fMLLR) behind it: transforms_example.cc's
// stages with pocketkaldi::OnlineScorer in the batch scorer's place (include/pocketkaldi_amd.hpp).
// The wave goes in 100 ms at a step under the sliding-window CMVN; a live slot looks right_context + R = 4 frames ahead,
// the step after Close() flushes them.  The rows of all steps together must be pocketkaldi::BatchScorer's on the whole
// wave under the same matrices, bit for bit.  It prints the frames and the 64-bit FNV-1a of the log-likelihood rows' bytes.
//
//   online_transforms_example <16 kHz wav>
//   online_transforms_example --link-only        (exits before touching the GPU)
// Built and run by tests/test_cpp_stream_transforms.py and tests/test_gpu_online_recognizer_transforms.py.
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
  const int Db = spec.dim(), Lt = 3, Rt = 3, D = 40, K = (Lt + Rt + 1) * Db, L = 2, R = 1, N = 16, chunk = 1600;
  std::vector<float> lda((size_t)D * (K + 1)), fmllr((size_t)D * (D + 1));
  for (size_t k = 0; k < lda.size(); ++k) lda[k] = Weight(2000003u + (uint32_t)k) * 4.0f;
  for (size_t k = 0; k < fmllr.size(); ++k) fmllr[k] = Weight(3000017u + (uint32_t)k) + (k / (D + 1) == k % (D + 1) ? 1.0f : 0.0f);
  const pocketkaldi::TransformSpec transform(lda.data(), D, K + 1, Db, Lt, Rt);
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
  std::vector<float> global(Db + 1, 0.0f);         // the sliding rule's statistics: means 0, count 1
  global[Db] = 1.0f;
  // the yardstick: the batch scorer on the whole wave, the speaker's matrix handed over for the call
  pocketkaldi::BatchScorer batch(am.handle(), spec, nullptr, transform, global.data(), Db + 1, 1, wave.dim + 1);
  st = batch.last_status();
  if (st.ok()) st = batch.SetWaves(&wave, 1);
  if (st.ok()) st = batch.SetUttTransforms(fmllr.data(), D + 1, 1);
  if (st.ok()) st = batch.Score(0.1f);
  pk_decodable_t want;
  if (st.ok()) st = batch.Fetch(0, &want);
  if (!st.ok()) {
    fprintf(stderr, "batch: %s\n", st.what().c_str());
    return 1;
  }
  const int T = batch.NumFrames(0);
  {   // statistics at the model's dimension instead of the front-end's are refused with both numbers
    pocketkaldi::OnlineScorer wrong(am.handle(), spec, nullptr, transform, std::vector<float>(D + 1, 1.0f).data(), D + 1, 1, chunk);
    if (wrong.last_status().ok() || wrong.last_status().what().find("14") == std::string::npos) {
      fprintf(stderr, "statistics of 41 entries were not refused: %s\n", wrong.last_status().what().c_str());
      return 1;
    }
  }
  pocketkaldi::OnlineScorer live(am.handle(), spec, nullptr, transform, global.data(), Db + 1, 1, chunk);
  if (!live.last_status().ok() || live.BaseDim() != Db || live.InDim() != Db || live.FeatDim() != D) {
    fprintf(stderr, "create: %s\n", live.last_status().what().c_str());
    return 1;
  }
  std::vector<float> rows;
  st = live.Open(0);
  if (st.ok()) st = live.SetSlotTransform(0, fmllr.data(), D + 1);
  int pushed = 0, next = 0;
  bool closed = false;
  while (st.ok() && !closed) {
    const int n = wave.dim - pushed < chunk ? wave.dim - pushed : chunk;
    st = live.Push(0, wave.data + pushed, n);
    pushed += n;
    if (st.ok() && pushed == wave.dim) {
      st = live.Close(0);
      closed = true;
    }
    if (st.ok()) st = live.Step(0.1f);
    pk_decodable_t out;
    int first = 0;
    if (st.ok()) st = live.Fetch(0, &out, &first);
    if (!st.ok()) break;
    const int count = out.log_prob.ncol;
    const int frames = pk_mi355_num_frames(pushed);
    // an open slot has scored the frames below n - Rt - R; the flush brings the rest
    if ((count > 0 && first != next) || next + count != (closed ? T : (frames - Rt - R > 0 ? frames - Rt - R : 0))) {
      fprintf(stderr, "after %d samples: rows [%d, %d), expected them to start at %d\n", pushed, first, first + count, next);
      return 1;
    }
    if (count > 0) rows.insert(rows.end(), out.log_prob.data, out.log_prob.data + (size_t)count * N);
    next += count;
    pk_decodable_destroy(&out);
  }
  if (!st.ok()) {
    fprintf(stderr, "live: %s\n", st.what().c_str());
    return 1;
  }
  // (once its first transform frame is computed a slot keeps the matrix it has)
  if (live.SetSlotTransform(0, fmllr.data(), D + 1).ok()) {
    fprintf(stderr, "a matrix for a slot that is not open was not refused\n");
    return 1;
  }
  if (want.log_prob.ncol != T || rows.size() != (size_t)T * N || memcmp(rows.data(), want.log_prob.data, sizeof(float) * rows.size()) != 0) {
    fprintf(stderr, "the live rows are not the batch scorer's\n");
    return 1;
  }
  printf("frames %d base %d dim %d\n", T, Db, D);
  printf("loglik %016llx\n", Fnv(rows.data(), sizeof(float) * rows.size()));
  pk_decodable_destroy(&want);
  free(wave.data);
  printf("online_transforms_example ok\n");
  return 0;
}
