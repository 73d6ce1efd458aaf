// stream_example.cc -- pk_process on live audio: the WAV is pushed in 100 ms chunks through pocketkaldi::OnlineScorer
// and pocketkaldi::OnlineDecoder (include/pocketkaldi_amd.hpp); after every step the partial hypothesis is printed,
// and at the end the lines tests/cpp/gpu_decode_example.cc prints for the whole utterance (frames, hyp, weight,
// loglikelihood_per_frame, pocketkaldi.cc:225-239).
//
//   stream_example <model.conf> <utterance.wav> <graph.fst>
//   stream_example --link-only        (exits before touching the GPU)
// Built and run by tests/test_cpp_stream.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pocketkaldi_amd.hpp"

int main(int argc, char **argv) {
  if (argc >= 2 && strcmp(argv[1], "--link-only") == 0) {
    printf("%s\n", pk_mi355_version());
    return 0;
  }
  if (argc < 4) {
    fprintf(stderr, "usage: %s model.conf utterance.wav graph.fst\n", argv[0]);
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
  if (pk_mi355_16kpcm_read(argv[2], &wave) != 0) {
    fprintf(stderr, "pk_mi355_16kpcm_read: %s\n", pk_mi355_last_error());
    return 1;
  }
  const int chunk = 1600;                               // 100 ms
  int rc = 0, T = 0;
  std::string hyp;
  float weight = 0.0f, per_frame = 0.0f;
  {
    pocketkaldi::OnlineScorer scorer(am, cmvn41, 1, chunk);
    pocketkaldi::OnlineDecoder decoder(&fst, am, 1);
    if (!scorer.last_status().ok() || !decoder.last_status().ok()) {
      fprintf(stderr, "create: %s%s\n", scorer.last_status().what().c_str(), decoder.last_status().what().c_str());
      return 1;
    }
    scorer.Open(0);
    decoder.Open(0);
    for (int pos = 0; ; pos += chunk) {
      const bool last = pos >= wave.dim;
      if (!last) st = scorer.Push(0, wave.data + pos, std::min(chunk, wave.dim - pos));
      else st = scorer.Close(0);
      if (st.ok()) st = scorer.Step(0.1f);
      if (st.ok()) st = decoder.Advance(&scorer);
      if (!st.ok()) {
        fprintf(stderr, "step: %s\n", st.what().c_str());
        return 1;
      }
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
      printf("partial %d ms: %s(%.9g)\n", (pos + chunk) / 16, partial.c_str(), cost);
    }
    int ok = 0;
    for (int w : decoder.Result(0, &weight, &ok)) hyp += "w" + std::to_string(w) + " ";
    if (!hyp.empty()) per_frame = weight / T;
    rc = ok ? 0 : 5;
  }
  printf("frames: %d\nhyp: %s\nweight: %.9g\nloglikelihood_per_frame: %.9g\n", T, hyp.c_str(), weight, per_frame);
  free(wave.data);
  pk_mi355_am_destroy(am);
  if (rc == 0) printf("stream_example ok\n");
  return rc;
}
