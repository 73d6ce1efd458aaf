// online_endpoint_example.cc -- tests/cpp/online_recognize_example.cc with endpointing on
// (pocketkaldi::OnlineRecognizer::SetEndpointing): one wave fed as live audio, 100 ms at a time, cut into utterances
// where an endpoint rule fires.  One line per utterance, "<file>[<start s>-<end s>]\t<sentence>\t<llpf>", as
// python -m pocketkaldi_amd.recognize --online --endpoint-silence prints them.
//
//   online_endpoint_example <model-file> <utterance.wav> <silence pdfs, e.g. 0,1,2> [must,trail_s,relcost,len_s ...]
//   online_endpoint_example --link-only          (exits before touching the GPU)
// Without rules the usual five (pk_mi355_endpoint_default_rules).  Built by tests/test_cpp_online_endpoint.py.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pocketkaldi_amd.hpp"

static int Failed(const pocketkaldi::Status &status) {
  printf("pocketkaldi: %s\n", status.what().c_str());
  return 1;
}

int main(int argc, char **argv) {
  if (argc >= 2 && strcmp(argv[1], "--link-only") == 0) {
    pocketkaldi::OnlineRecognizer recognizer;
    const std::vector<pk_mi355_endpoint_rule_t> rules = pocketkaldi::OnlineDecoder::DefaultEndpointRules();
    printf("%s\n", pk_mi355_version());
    // (host only: the second of the usual rules fires after half a second of silence behind speech)
    const bool fires = rules.size() == 5 && pk_mi355_endpoint_eval(rules.data(), 5, 80, 50, 1.0f) == 2 &&
                       pk_mi355_endpoint_eval(rules.data(), 5, 80, 49, 1.0f) == 0;
    return recognizer.handle() == nullptr && recognizer.Utterances(0).empty() && fires ? 0 : 1;
  }
  if (argc < 4) {
    puts("Usage: online_endpoint_example <model-file> <input-file.wav> <silence pdfs> [must,trail_s,relcost,len_s ...]");
    return 1;
  }
  std::vector<int32_t> silence;
  for (char *p = strtok(argv[3], ","); p; p = strtok(nullptr, ",")) silence.push_back(atoi(p));
  std::vector<pk_mi355_endpoint_rule_t> rules;
  for (int i = 4; i < argc; ++i) {
    int must = 0;
    float trail = 0.0f, cost = 0.0f, len = 0.0f;
    if (sscanf(argv[i], "%d,%f,%f,%f", &must, &trail, &cost, &len) != 4) {
      printf("pocketkaldi: bad rule %s\n", argv[i]);
      return 1;
    }
    rules.push_back(pk_mi355_endpoint_rule_t{must, static_cast<int>(lround(trail * 100.0)), cost, static_cast<int>(lround(len * 100.0))});
  }
  if (rules.empty()) rules = pocketkaldi::OnlineDecoder::DefaultEndpointRules();
  pk_vector_t wave = {0, nullptr};
  if (pk_mi355_16kpcm_read(argv[2], &wave) != 0) {
    printf("pocketkaldi: %s\n", pk_mi355_last_error());
    return 1;
  }
  const int chunk = 1600;                                                            // 100 ms at 16 kHz
  pocketkaldi::OnlineRecognizer recognizer;
  pocketkaldi::Status status = recognizer.Load(argv[1], 1, chunk);
  if (!status.ok()) return Failed(status);
  if (!(status = recognizer.SetEndpointing(silence, rules)).ok()) return Failed(status);
  if (!(status = recognizer.Open(0)).ok()) return Failed(status);
  if (recognizer.SetEndpointing(silence, rules).code() != PK_MI355_E_STATE) {        // the mode is the object's
    puts("pocketkaldi: SetEndpointing with a slot open was not refused");
    return 1;
  }
  for (int at = 0; at < wave.dim; at += chunk) {
    const int n = wave.dim - at < chunk ? wave.dim - at : chunk;
    if (!(status = recognizer.Push(0, wave.data + at, n)).ok() || !(status = recognizer.Step()).ok()) return Failed(status);
  }
  if (!(status = recognizer.Close(0)).ok() || !(status = recognizer.Step()).ok()) return Failed(status);
  int frames = 0;
  for (const pocketkaldi::OnlineRecognizer::Piece &p : recognizer.Utterances(0)) {
    if (p.info.first_frame != frames) {
      puts("pocketkaldi: the utterances do not follow each other");
      return 1;
    }
    frames += p.info.num_frames;
    printf("%s[%.2f-%.2f]\t%s\t%f\n", argv[2], p.info.first_frame / 100.0, frames / 100.0, p.hyp.c_str(),
           p.info.loglikelihood_per_frame);
  }
  free(wave.data);
  return 0;
}
