// gpu_decode_example.cc -- pk_process (pocketkaldi.cc:176-248) with BOTH halves on the GPU:
//   pk_read_audio                -> pk_mi355_16kpcm_read                          (pocketkaldi.cc:166-174)
//   Fbank / CMVN / NNET          -> pk_mi355_process_acoustic                     (:189-218)
//   decoder.Decode / BestPath    -> pocketkaldi::Decoder (include/pocketkaldi_amd.hpp, pk_mi355_decoder_*)
//   std::reverse(hyp.words())    -> spoken order, loglikelihood_per_frame = weight / T  (:225-239)
// Prints what tests/cpp/process_example.cc prints, so the two outputs can be compared line for line.
//
//   gpu_decode_example <model.conf> <utterance.wav> <graph.fst> [--reference-softmax]
//   gpu_decode_example --link-only        (exits before touching the GPU)
// Built and run by tests/test_cpp_decode.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pocketkaldi_amd.hpp"

int main(int argc, char **argv) {
  if (argc >= 2 && strcmp(argv[1], "--link-only") == 0) {
    pocketkaldi::Fst fst;
    printf("%s\n", pk_mi355_version());
    return fst.handle() == nullptr ? 0 : 1;
  }
  if (argc < 4) {
    fprintf(stderr, "usage: %s model.conf utterance.wav graph.fst [--reference-softmax]\n", argv[0]);
    return 64;
  }
  pk_mi355_am_t *am = nullptr;
  float cmvn41[41];
  if (pk_mi355_load(argv[1], PK_MI355_PRECISION_F32, &am, cmvn41) != 0) {             // pk_load, :72-144
    fprintf(stderr, "pk_mi355_load: %s\n", pk_mi355_last_error());
    return 1;
  }
  if (argc >= 5 && strcmp(argv[4], "--reference-softmax") == 0) pk_mi355_am_set_softmax(am, PK_MI355_SOFTMAX_REFERENCE);
  pocketkaldi::Fst fst;
  pocketkaldi::Status st = fst.Read(argv[3]);
  if (!st.ok()) {
    fprintf(stderr, "Fst::Read: %s\n", st.what().c_str());
    return 1;
  }
  pk_vector_t cmvn = {41, cmvn41};
  pk_vector_t wave = {0, nullptr};
  if (pk_mi355_16kpcm_read(argv[2], &wave) != 0) {
    fprintf(stderr, "pk_mi355_16kpcm_read: %s\n", pk_mi355_last_error());
    return 1;
  }
  int rc = 0, T = 0;
  std::string hyp;
  float weight = 0.0f, per_frame = 0.0f;
  if (wave.dim > 0) {                                                                 // :180-184
    pk_decodable_t decodable;
    if (pk_mi355_process_acoustic(am, &cmvn, &wave, 0.1f, &decodable, /*verbose=*/1) != 0) {
      fprintf(stderr, "process_acoustic: %s\n", pk_mi355_last_error());
      return 1;
    }
    T = decodable.log_prob.ncol;
    pocketkaldi::Decoder decoder(&fst, am);
    const bool ok = decoder.Decode(&decodable);
    if (!decoder.last_status().ok()) {
      fprintf(stderr, "Decoder: %s\n", decoder.last_status().what().c_str());
      return 1;
    }
    pocketkaldi::Decoder::Hypothesis h = decoder.BestPath();
    std::vector<int> words = h.words();
    std::reverse(words.begin(), words.end());                                        // :226-227
    for (int w : words) hyp += "w" + std::to_string(w) + " ";
    weight = h.weight();
    if (!words.empty()) per_frame = weight / T;                                       // :239
    pk_decodable_destroy(&decodable);                                                 // :247
    rc = ok ? 0 : 5;
  }
  printf("frames: %d\nhyp: %s\nweight: %.9g\nloglikelihood_per_frame: %.9g\n", T, hyp.c_str(), weight, per_frame);
  free(wave.data);
  pk_mi355_am_destroy(am);
  if (rc == 0) printf("gpu_decode_example ok\n");
  return rc;
}
