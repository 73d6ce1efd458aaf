// online_norm_example.cc -- audio into a model that was trained on apply-cmvn-online's features: an 80-bin Povey-window
// fbank front-end in front of an 80-dim model, pocketkaldi::BatchScorer::SetNorm(OnlineCmvnSpec(...), global statistics)
// (include/pocketkaldi_amd.hpp).  The model is norm_example.cc's.  The global record says 300
// frames of mean 10 and variance 4 in every column, the speaker record 37 frames of mean 12 and variance 2.  It prints
// the frames and the 64-bit FNV-1a of the normalised rows' and of the log-likelihood rows' bytes, without and with the
// speaker record; the rows must equal pk_mi355_online_cmvn_apply's on the front-end's rows bit for bit.  Then the same wave
// goes through a pocketkaldi::OnlineScorer under the same spec (SetNorm, SetSpeakerStats, NormStats), 100 ms a step: its
// log-likelihood rows must be the batch scorer's bit for bit.
//
//   online_norm_example <16 kHz wav>
//   online_norm_example --link-only        (exits before touching the GPU)
// Built and run by tests/test_cpp_online_cmvn.py.
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

static std::vector<double> Record(int D, double mean, double var, double n) {
  std::vector<double> s(2 * (static_cast<size_t>(D) + 1), 0.0);
  for (int d = 0; d < D; ++d) {
    s[d] = mean * n;
    s[D + 1 + d] = (mean * mean + var) * n;
  }
  s[D] = n;
  return s;
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
  const pocketkaldi::FrontendSpec spec = pocketkaldi::FrontendSpec::Fbank(80);
  const int D = spec.dim(), L = 2, R = 1, N = 16;
  const pocketkaldi::OnlineCmvnSpec norm(8, 3, 2, true);
  const std::vector<double> glob = Record(D, 10.0, 4.0, 300.0), spk = Record(D, 12.0, 2.0, 37.0);
  {   // a spec the library refuses says which field
    pocketkaldi::OnlineCmvnSpec bad(0);
    if (bad.Check(glob.data(), D).ok() || bad.Check(glob.data(), D).what().find("cmn_window") == std::string::npos ||
        norm.Check(nullptr, D).ok() || !norm.Check(glob.data(), D).ok() || !pocketkaldi::OnlineCmvnSpec().Check(glob.data(), D).ok()) {
      fprintf(stderr, "the specs were not checked as expected\n");
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
  std::vector<float> sliding(D + 1, 0.0f);         // the sliding rule's statistics: the object needs some, online CMVN reads none
  sliding[D] = 1.0f;
  pocketkaldi::BatchScorer scorer(am.handle(), spec, sliding.data(), D + 1, 1, wave.dim + 1);
  if (!scorer.last_status().ok()) {
    fprintf(stderr, "create: %s\n", scorer.last_status().what().c_str());
    return 1;
  }
  if (scorer.SetNorm(norm, nullptr).code() != PK_MI355_E_INVALID) {
    fprintf(stderr, "global_frames without global statistics was not refused\n");
    return 1;
  }
  st = scorer.SetNorm(norm, glob.data());
  pocketkaldi::OnlineScorer live(am.handle(), spec, sliding.data(), D + 1, 1, 1600);
  if (!live.last_status().ok() || live.SetNorm(pocketkaldi::NormSpec::Utterance()).code() != PK_MI355_E_INVALID) {
    fprintf(stderr, "the online scorer: %s\n", live.last_status().what().c_str());
    return 1;
  }
  if (st.ok()) st = live.SetNorm(norm, glob.data());
  for (int speaker = 0; speaker < 2 && st.ok(); ++speaker) {
    if (speaker) st = scorer.SetSpeakerStats(spk.data(), 1);
    if (st.ok()) st = scorer.SetWaves(&wave, 1);
    if (st.ok()) st = scorer.Score(0.1f);
    if (!st.ok()) break;
    const int T = scorer.NumFrames(0);
    std::vector<float> raw((size_t)T * D), rows((size_t)T * D), want((size_t)T * D);
    pk_decodable_t out;
    st = scorer.FetchFeatures(0, raw.data());
    if (st.ok()) st = scorer.FetchNormalized(0, rows.data());
    if (st.ok()) st = scorer.Fetch(0, &out);
    if (st.ok()) st = pocketkaldi::Status::FromLast(pk_mi355_online_cmvn_apply(&norm, raw.data(), T, D, glob.data(), speaker ? spk.data() : nullptr,
                                                                               want.data(), nullptr));
    if (!st.ok() || out.log_prob.ncol != T || out.log_prob.nrow != N) break;
    if (memcmp(rows.data(), want.data(), sizeof(float) * rows.size()) != 0) {
      fprintf(stderr, "the scorer's rows are not the host rule's (speaker %d)\n", speaker);
      return 1;
    }
    if (!speaker) printf("frames %d dim %d\n", T, D);
    printf("normalized %d %016llx\n", speaker, Fnv(rows.data(), sizeof(float) * rows.size()));
    printf("loglik %d %016llx\n", speaker, Fnv(out.log_prob.data, sizeof(float) * (size_t)T * N));
    // the same wave live, 100 ms a step, under the same spec: the batch scorer's rows bit for bit, and the slot's record
    std::vector<float> live_rows;
    st = live.Open(0);
    if (st.ok() && speaker) st = live.SetSpeakerStats(0, spk.data());
    for (int pos = 0; st.ok(); pos += 1600) {
      const bool last = pos >= wave.dim;
      st = last ? live.Close(0) : live.Push(0, wave.data + pos, wave.dim - pos < 1600 ? wave.dim - pos : 1600);
      if (st.ok()) st = live.Step(0.1f);
      pk_decodable_t part;
      int first = 0;
      if (st.ok()) st = live.Fetch(0, &part, &first);
      if (!st.ok()) break;
      if (part.log_prob.ncol > 0) {
        if (first * N != (int)live_rows.size()) st = pocketkaldi::Status(PK_MI355_E_STATE, "the live rows do not continue");
        live_rows.insert(live_rows.end(), part.log_prob.data, part.log_prob.data + (size_t)part.log_prob.ncol * N);
      }
      pk_decodable_destroy(&part);
      if (last) break;
    }
    std::vector<double> record;
    if (st.ok()) st = live.NormStats(0, &record);
    if (!st.ok() || live_rows.size() != (size_t)T * N || memcmp(live_rows.data(), out.log_prob.data, sizeof(float) * live_rows.size()) != 0 ||
        record[D] != (double)T) {
      fprintf(stderr, "the live rows are not the batch scorer's (speaker %d): %s\n", speaker, st.what().c_str());
      return 1;
    }
    pk_decodable_destroy(&out);
  }
  if (!st.ok()) {
    fprintf(stderr, "score: %s\n", st.what().c_str());
    return 1;
  }
  free(wave.data);
  printf("online_norm_example ok\n");
  return 0;
}
