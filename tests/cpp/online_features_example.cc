// online_features_example.cc -- live features instead of live audio: the WAV's log-mel fbank (pk_mi355_fbank_compute
// stands for a front-end of the caller's) is pushed 10 frames a step, as PK_MI355_FEATS_RAW, through a features-only
// pocketkaldi::OnlineScorer and a pocketkaldi::OnlineDecoder (include/pocketkaldi_amd.hpp).  It prints the partial
// hypothesis after every step and at the end the lines tests/cpp/gpu_decode_example.cc prints for the whole utterance
// (frames, hyp, weight, loglikelihood_per_frame).  With a recognizer configuration as fourth argument the same frames
// also go through pocketkaldi::OnlineRecognizer::OpenFeatures / PushFeatures, and its sentence is printed.
//
//   online_features_example <model.conf> <utterance.wav> <graph.fst> [recognizer.conf]
//   online_features_example --link-only        (exits before touching the GPU)
// Built and run by tests/test_cpp_online_features.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "pocketkaldi_amd.hpp"

int main(int argc, char **argv) {
  if (argc >= 2 && strcmp(argv[1], "--link-only") == 0) {
    printf("%s\n", pk_mi355_version());
    return 0;
  }
  if (argc < 4) {
    fprintf(stderr, "usage: %s model.conf utterance.wav graph.fst [recognizer.conf]\n", argv[0]);
    return 64;
  }
  pk_mi355_am_t *am = nullptr;
  float cmvn41[41];
  if (pk_mi355_load(argv[1], PK_MI355_PRECISION_F32, &am, cmvn41) != 0) {
    fprintf(stderr, "pk_mi355_load: %s\n", pk_mi355_last_error());
    return 1;
  }
  pocketkaldi::Fst fst;
  pocketkaldi::Status st = fst.Read(argv[3]);
  if (!st.ok()) {
    fprintf(stderr, "Fst::Read: %s\n", st.what().c_str());
    return 1;
  }
  pk_vector_t wave = {0, nullptr};
  pk_matrix_t fbank = {0, 0, nullptr};                  // {ncol = T, nrow = 40}: frame-major
  if (pk_mi355_16kpcm_read(argv[2], &wave) != 0 || pk_mi355_fbank_compute(&wave, &fbank) != 0) {
    fprintf(stderr, "front-end: %s\n", pk_mi355_last_error());
    return 1;
  }
  const int chunk = 10;                                 // frames per step: 100 ms
  const int total = fbank.ncol, dim = fbank.nrow;
  int rc = 0, T = 0;
  std::string hyp;
  float weight = 0.0f, per_frame = 0.0f;
  {
    pocketkaldi::OnlineScorer scorer(pocketkaldi::OnlineScorer::kFeaturesOnly, am, cmvn41, 1, chunk);
    pocketkaldi::OnlineDecoder decoder(&fst, am, 1);
    if (!scorer.last_status().ok() || !decoder.last_status().ok()) {
      fprintf(stderr, "create: %s%s\n", scorer.last_status().what().c_str(), decoder.last_status().what().c_str());
      return 1;
    }
    if (scorer.FeatDim() != dim || scorer.Open(0).ok() || scorer.SlotKind(0) != -1) {   // (no audio on this object)
      fprintf(stderr, "a features-only scorer of %d-dim frames was expected\n", dim);
      return 1;
    }
    st = scorer.OpenFeatures(0, PK_MI355_FEATS_RAW);
    if (st.ok()) st = decoder.Open(0);
    for (int pos = 0; st.ok(); pos += chunk) {
      const bool last = pos >= total;
      if (!last) st = scorer.PushFeatures(0, fbank.data + (size_t)pos * dim, std::min(chunk, total - pos));
      else st = scorer.Close(0);
      if (st.ok()) st = scorer.Step(0.1f);
      if (st.ok()) st = decoder.Advance(&scorer);
      if (!st.ok()) break;
      pk_decodable_t rows;
      int first = 0;
      if (scorer.Fetch(0, &rows, &first).ok()) {
        T += rows.log_prob.ncol;
        pk_decodable_destroy(&rows);
      }
      if (last) break;
      float cost = 0.0f;
      std::string partial;
      for (int w : decoder.Partial(0, &cost)) partial += "w" + std::to_string(w) + " ";
      printf("partial %d frames: %s(%.9g)\n", std::min(pos + chunk, total), partial.c_str(), cost);
    }
    if (!st.ok()) {
      fprintf(stderr, "step: %s\n", st.what().c_str());
      return 1;
    }
    if (scorer.SlotKind(0) != PK_MI355_FEATS_RAW) return 1;
    int ok = 0;
    for (int w : decoder.Result(0, &weight, &ok)) hyp += "w" + std::to_string(w) + " ";
    if (!hyp.empty()) per_frame = weight / T;
    rc = ok ? 0 : 5;
  }
  printf("frames: %d\nhyp: %s\nweight: %.9g\nloglikelihood_per_frame: %.9g\n", T, hyp.c_str(), weight, per_frame);
  if (argc >= 5) {
    pocketkaldi::OnlineRecognizer recognizer;
    st = recognizer.Load(argv[4], 1, 160 * chunk);
    if (st.ok()) st = recognizer.OpenFeatures(0);       // raw fbank
    for (int pos = 0; st.ok() && pos < total; pos += chunk) {
      st = recognizer.PushFeatures(0, fbank.data + (size_t)pos * dim, std::min(chunk, total - pos));
      if (st.ok()) st = recognizer.Step();
    }
    if (st.ok()) st = recognizer.Close(0);
    if (st.ok()) st = recognizer.Step();
    pocketkaldi::Recognizer::Utterance result;
    if (st.ok()) st = recognizer.Result(0, &result);
    if (!st.ok()) {
      fprintf(stderr, "recognizer: %s\n", st.what().c_str());
      return 1;
    }
    printf("recognizer_hyp: %s\nrecognizer_loglikelihood_per_frame: %.9g\n", result.hyp.c_str(), result.loglikelihood_per_frame);
  }
  free(wave.data);
  free(fbank.data);
  pk_mi355_am_destroy(am);
  if (rc == 0) printf("online_features_example ok\n");
  return rc;
}
