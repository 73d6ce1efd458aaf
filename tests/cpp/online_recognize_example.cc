// online_recognize_example.cc -- the reference's command-line program (main.cc:17-80) for one wave fed as live audio,
// through the C++ mirror:
//   pk_load                      -> pocketkaldi::OnlineRecognizer::Load            (pocketkaldi.cc:72-144)
//   pk_read_audio                -> pk_mi355_16kpcm_read                           (:166-174)
//   pk_process                   -> Open, Push 100 ms at a time with a Step after each, Close, Step, Result  (:176-248)
//   printf("%s\t%s\t%f\n", ...)  -> the same line                                  (main.cc:28)
//
//   online_recognize_example <model-file> <utterance.wav> [--reference-softmax]
//   online_recognize_example --link-only         (exits before touching the GPU)
// Built and run by tests/test_gpu_online_recognizer.py, which compares the line with python -m pocketkaldi_amd.recognize's.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pocketkaldi_amd.hpp"

static int Failed(const pocketkaldi::Status &status) {
  printf("pocketkaldi: %s\n", status.what().c_str());                                // main.cc:10-15
  return 1;
}

int main(int argc, char **argv) {
  if (argc >= 2 && strcmp(argv[1], "--link-only") == 0) {
    pocketkaldi::OnlineRecognizer recognizer;
    printf("%s\n", pk_mi355_version());
    return recognizer.handle() == nullptr && !recognizer.Finished(0) ? 0 : 1;
  }
  if (argc < 3) {
    puts("Usage: online_recognize_example <model-file> <input-file.wav> [--reference-softmax]");
    return 1;
  }
  pk_vector_t wave = {0, nullptr};
  if (pk_mi355_16kpcm_read(argv[2], &wave) != 0) {
    printf("pocketkaldi: %s\n", pk_mi355_last_error());
    return 1;
  }
  const int chunk = 1600;                                                            // 100 ms at 16 kHz
  pocketkaldi::OnlineRecognizer recognizer;
  pocketkaldi::Status status = recognizer.Load(argv[1], 1, chunk);
  if (!status.ok()) return Failed(status);
  if (argc >= 4 && strcmp(argv[3], "--reference-softmax") == 0) pk_mi355_am_set_softmax(recognizer.am(), PK_MI355_SOFTMAX_REFERENCE);
  if (!(status = recognizer.Open(0)).ok()) return Failed(status);
  for (int at = 0; at < wave.dim; at += chunk) {
    const int n = wave.dim - at < chunk ? wave.dim - at : chunk;
    if (!(status = recognizer.Push(0, wave.data + at, n)).ok() || !(status = recognizer.Step()).ok()) return Failed(status);
  }
  if (!(status = recognizer.Close(0)).ok() || !(status = recognizer.Step()).ok()) return Failed(status);
  pocketkaldi::Recognizer::Utterance utt;
  if (!(status = recognizer.Result(0, &utt)).ok()) return Failed(status);
  printf("%s\t%s\t%f\n", argv[2], utt.hyp.c_str(), utt.loglikelihood_per_frame);
  free(wave.data);
  return 0;
}
