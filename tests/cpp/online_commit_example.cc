// online_commit_example.cc -- tests/cpp/stream_example.cc with the online decoder's commit mode on
// (pocketkaldi::OnlineDecoder::SetCommit): the WAV in 100 ms chunks through pocketkaldi::OnlineScorer and
// pocketkaldi::OnlineDecoder; after every step the partial hypothesis is printed as stream_example prints it, followed
// by the number of its words that are committed (OnlineDecoder::Committed) -- they must be the partial's first words
// and never fewer than before -- and at the end the same four lines (frames, hyp, weight, loglikelihood_per_frame).
//
//   online_commit_example <model.conf> <utterance.wav> <graph.fst>
//   online_commit_example --link-only        (exits before touching the GPU)
// Built and run by tests/test_cpp_online_commit.py, which compares the lines with stream_example's.
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
    if (!(st = decoder.SetCommit(true)).ok()) {
      fprintf(stderr, "SetCommit: %s\n", st.what().c_str());
      return 1;
    }
    scorer.Open(0);
    decoder.Open(0);
    if (decoder.SetCommit(false).code() != PK_MI355_E_STATE) {        // the mode is the object's: not while a slot is open
      fprintf(stderr, "SetCommit with a slot open was not refused\n");
      return 1;
    }
    size_t stable_before = 0;
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
      const std::vector<int> words = decoder.Partial(0, &cost);
      for (int w : words) partial += "w" + std::to_string(w) + " ";
      int arcs = 0, frames = 0;
      int64_t in_use = 0, peak = 0, capacity = 0;
      const std::vector<int> stable = decoder.Committed(0, &arcs, &frames);
      if (stable.size() > words.size() || !std::equal(stable.begin(), stable.end(), words.begin()) ||
          stable.size() < stable_before || frames > arcs || frames > T ||
          !decoder.TraceStats(0, &in_use, &peak, &capacity).ok() || in_use > peak || peak > capacity) {
        fprintf(stderr, "committed: not a growing prefix of the partial hypothesis\n");
        return 1;
      }
      stable_before = stable.size();
      printf("partial %d ms: %s(%.9g) stable %d words %d arcs\n", (pos + chunk) / 16, partial.c_str(), cost, (int)stable.size(), arcs);
    }
    int ok = 0;
    for (int w : decoder.Result(0, &weight, &ok)) hyp += "w" + std::to_string(w) + " ";
    if (!hyp.empty()) per_frame = weight / T;
    rc = ok ? 0 : 5;
  }
  printf("frames: %d\nhyp: %s\nweight: %.9g\nloglikelihood_per_frame: %.9g\n", T, hyp.c_str(), weight, per_frame);
  free(wave.data);
  pk_mi355_am_destroy(am);
  if (rc == 0) printf("online_commit_example ok\n");
  return rc;
}
