// online_frontend_example.cc -- live audio to text for a model that is not the reference's 40-bin fbank (DESIGN.md
// section 18), through the C++ mirror: an 80-bin Povey-window fbank front-end (pocketkaldi::FrontendSpec::Fbank(80),
// Kaldi's defaults) in front of an 80-dim model whose model file carries 81 CMVN statistics.
//   pk_load                      -> pocketkaldi::OnlineRecognizer::Load(model file, spec, ...)
//   pk_read_audio                -> pk_mi355_16kpcm_read
//   pk_process                   -> Open, Push 100 ms at a time with a Step after each, Close, Step, Result
//   printf("%s\t%s\t%f\n", ...)  -> the same line                                  (main.cc:28)
// The partial hypotheses go to stderr as they change.  A spec of another dimension than the model's is refused with both
// numbers named, which the example shows first.
//
//   online_frontend_example <model-file> <utterance.wav>
//   online_frontend_example --link-only         (exits before touching the GPU)
// Built and run by tests/test_cpp_online_frontend.py, which compares the line with python -m pocketkaldi_amd.recognize
// --frontend num_mel_bins=80,window=povey on the same files.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "pocketkaldi_amd.hpp"

static int Failed(const pocketkaldi::Status &status) {
  printf("pocketkaldi: %s\n", status.what().c_str());                                // main.cc:10-15
  return 1;
}

int main(int argc, char **argv) {
  if (argc >= 2 && strcmp(argv[1], "--link-only") == 0) {
    pocketkaldi::OnlineRecognizer recognizer;
    printf("%s\n", pk_mi355_version());
    return recognizer.handle() == nullptr && pocketkaldi::FrontendSpec::Fbank(80).dim() == 80 ? 0 : 1;
  }
  if (argc < 3) {
    puts("Usage: online_frontend_example <model-file> <input-file.wav>");
    return 1;
  }
  pk_vector_t wave = {0, nullptr};
  if (pk_mi355_16kpcm_read(argv[2], &wave) != 0) {
    printf("pocketkaldi: %s\n", pk_mi355_last_error());
    return 1;
  }
  const int chunk = 1600;                                                            // 100 ms at 16 kHz
  pocketkaldi::OnlineRecognizer recognizer;
  pocketkaldi::Status status = recognizer.Load(argv[1], pocketkaldi::FrontendSpec::Mfcc(23, 13), 1, chunk);
  if (status.ok() || status.what().find("13") == std::string::npos || status.what().find("80") == std::string::npos) {
    printf("a 13-dim spec in front of the 80-dim model was not refused by its numbers: %s\n", status.what().c_str());
    return 1;
  }
  const pocketkaldi::FrontendSpec spec = pocketkaldi::FrontendSpec::Fbank(80);
  if (!(status = recognizer.Load(argv[1], spec, 1, chunk)).ok()) return Failed(status);
  if (pk_mi355_stream_feat_dim(recognizer.stream()) != spec.dim()) return 1;
  if (!(status = recognizer.Open(0)).ok()) return Failed(status);
  std::string shown;
  for (int at = 0; at < wave.dim; at += chunk) {
    const int n = wave.dim - at < chunk ? wave.dim - at : chunk;
    if (!(status = recognizer.Push(0, wave.data + at, n)).ok() || !(status = recognizer.Step()).ok()) return Failed(status);
    const std::string partial = recognizer.Partial(0);
    if (partial != shown) fprintf(stderr, "%s\t%.2f\t%s\n", argv[2], (at + n) / 16000.0, partial.c_str());
    shown = partial;
  }
  if (!(status = recognizer.Close(0)).ok() || !(status = recognizer.Step()).ok()) return Failed(status);
  pocketkaldi::Recognizer::Utterance utt;
  if (!(status = recognizer.Result(0, &utt)).ok()) return Failed(status);
  printf("%s\t%s\t%f\n", argv[2], utt.hyp.c_str(), utt.loglikelihood_per_frame);
  free(wave.data);
  return 0;
}
