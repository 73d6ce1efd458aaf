// recognize_example.cc -- the reference's command-line program (main.cc:17-80) for one wave, through the C++ mirror:
//   pk_load                      -> pocketkaldi::Recognizer::Load                  (pocketkaldi.cc:72-144)
//   pk_read_audio                -> pk_mi355_16kpcm_read                           (:166-174)
//   pk_process                   -> pocketkaldi::Recognizer::Process               (:176-248)
//   printf("%s\t%s\t%f\n", ...)  -> the same line                                  (main.cc:28)
//
//   recognize_example <model-file> <utterance.wav> [--reference-softmax]
//   recognize_example --link-only         (exits before touching the GPU)
// Built and run by tests/test_gpu_recognizer.py, which compares the line with python -m pocketkaldi_amd.recognize's.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pocketkaldi_amd.hpp"

int main(int argc, char **argv) {
  if (argc >= 2 && strcmp(argv[1], "--link-only") == 0) {
    pocketkaldi::Recognizer recognizer;
    pocketkaldi::SymbolTable symbols;
    printf("%s\n", pk_mi355_version());
    return recognizer.handle() == nullptr && symbols.size() == 0 ? 0 : 1;
  }
  if (argc < 3) {
    puts("Usage: recognize_example <model-file> <input-file.wav> [--reference-softmax]");
    return 1;
  }
  pk_vector_t wave = {0, nullptr};
  if (pk_mi355_16kpcm_read(argv[2], &wave) != 0) {
    printf("pocketkaldi: %s\n", pk_mi355_last_error());                              // main.cc:10-15
    return 1;
  }
  pocketkaldi::Recognizer recognizer;
  pocketkaldi::Status status = recognizer.Load(argv[1], PK_MI355_PRECISION_F32, 1, wave.dim > 0 ? wave.dim : 1);
  if (!status.ok()) {
    printf("pocketkaldi: %s\n", status.what().c_str());
    return 1;
  }
  if (argc >= 4 && strcmp(argv[3], "--reference-softmax") == 0) pk_mi355_am_set_softmax(recognizer.am(), PK_MI355_SOFTMAX_REFERENCE);
  std::vector<pocketkaldi::Recognizer::Utterance> utts;
  status = recognizer.Process(&wave, 1, &utts);
  if (!status.ok()) {
    printf("pocketkaldi: %s\n", status.what().c_str());
    return 1;
  }
  printf("%s\t%s\t%f\n", argv[2], utts[0].hyp.c_str(), utts[0].loglikelihood_per_frame);
  free(wave.data);
  return 0;
}
