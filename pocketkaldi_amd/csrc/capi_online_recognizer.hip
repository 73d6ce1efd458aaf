// capi_online_recognizer.hip -- pk_load + a live pk_process (pocketkaldi.cc:72-248) as one object: model file -> graph,
// symbol table, acoustic model, online scorer and online decoder (alignment on); PCM chunks per slot -> partial text
// while a slot is live, sentence and log-likelihood per frame at its end.  Nothing here computes: the scorer and the
// decoder are the library's own entries, wired slot for slot, and every knob of theirs stays theirs
// (pk_mi355_online_recognizer_am / _stream / _decoder hand them out).  The file-loading half is capi_recognizer.hip's.
#include <string>
#include <vector>

#include "pk_host.h"

using namespace pkhost;

struct pk_mi355_online_recognizer : RecognizerFiles {
  pk_mi355_am_t *am = nullptr;
  pk_mi355_stream_t *stream = nullptr;
  pk_mi355_online_decoder_t *decoder = nullptr;
  int max_streams = 0;
  std::vector<char> live, closed, finished;  // per slot: opened here; closed, its flush still to come; its result is final
  std::vector<std::string> partial, hyp;     // per slot: the text after the last step; a finished slot's sentence
  std::vector<std::string> stable;           // per slot: the committed words' text after the last step ("": mode off)
  std::vector<size_t> stable_words;          // per slot: how many of the decoder's committed words stable[slot] holds
  std::vector<float> per_frame;
};

namespace {

// The text of every slot this object opened, after a step; a slot whose close the step flushed becomes finished.
int Refresh(pk_mi355_online_recognizer *r) {
  std::vector<int> words;
  for (int slot = 0; slot < r->max_streams; ++slot) {
    if (!r->live[slot]) continue;
    const int count = pk_mi355_online_decoder_partial(r->decoder, slot, nullptr, 0, nullptr);
    if (count < 0) return count;
    // Per step: the newly committed words are appended to the stable text, and only the tail's words are joined anew.
    const std::vector<int> *committed = OnlineDecoderCommittedWords(r->decoder, slot);
    if (!committed) return Fail(PK_MI355_E_INVALID, "online recognizer: slot %d is not the decoder's", slot);
    if (committed->size() < r->stable_words[slot]) { r->stable[slot].clear(); r->stable_words[slot] = 0; }   // (the slot ended)
    std::string more;
    int rc = JoinWords(r->symtab, committed->data() + r->stable_words[slot], (int)(committed->size() - r->stable_words[slot]), &more);
    if (rc) return rc;
    if (!more.empty()) r->stable[slot] += (r->stable[slot].empty() ? "" : " ") + more;
    r->stable_words[slot] = committed->size();
    OnlineDecoderTailWords(r->decoder, slot, &words);
    if ((int)(committed->size() + words.size()) != count) return Fail(PK_MI355_E_DEVICE, "online recognizer: slot %d: word counts differ", slot);
    if ((rc = JoinWords(r->symtab, words.data(), (int)words.size(), &more))) return rc;
    r->partial[slot] = r->stable[slot] + (!r->stable[slot].empty() && !more.empty() ? " " : "") + more;
    if (!r->closed[slot]) continue;
    float weight = 0.0f;
    int ok = 0;
    const int final_count = pk_mi355_online_decoder_result(r->decoder, slot, nullptr, 0, &weight, &ok);
    if (final_count < 0) return final_count;
    r->live[slot] = 0; r->closed[slot] = 0; r->finished[slot] = 1;
    r->hyp[slot].clear();
    r->per_frame[slot] = 0.0f;
    if (!ok || final_count == 0) continue;             // pocketkaldi.cc:240-243: no words, "" and 0.0f
    r->hyp[slot] = r->partial[slot];                   // (the partial after the final advance is the final result)
    r->per_frame[slot] = weight / pk_mi355_online_decoder_num_frames(r->decoder, slot);     // :239
  }
  return 0;
}

int CheckSlot(const pk_mi355_online_recognizer *r, int slot) {
  if (!r) return Fail(PK_MI355_E_INVALID, "null online recognizer");
  if (slot < 0 || slot >= r->max_streams) return Fail(PK_MI355_E_INVALID, "slot %d out of range [0, %d)", slot, r->max_streams);
  return 0;
}

}  // namespace

extern "C" {

void pk_mi355_online_recognizer_destroy(pk_mi355_online_recognizer_t *r) {
  if (!r) return;
  pk_mi355_online_decoder_destroy(r->decoder);   // (waits for its last call, which reads the scorer's rows)
  pk_mi355_stream_destroy(r->stream);
  pk_mi355_am_destroy(r->am);
  FreeRecognizerFiles(r);
  delete r;
}

pk_mi355_online_recognizer_t *pk_mi355_online_recognizer_load(const char *config_path, int max_streams, int64_t max_step_samples,
                                                              int64_t trace_capacity) {
  if (!config_path) { Fail(PK_MI355_E_INVALID, "null path"); return nullptr; }
  if (max_streams <= 0 || max_step_samples <= 0 || trace_capacity < 0) { Fail(PK_MI355_E_INVALID, "bad online recognizer capacity"); return nullptr; }
  pk_mi355_online_recognizer *r = new pk_mi355_online_recognizer();
  auto failed = [&]() { pk_mi355_online_recognizer_destroy(r); return nullptr; };
  if (LoadRecognizerFiles(config_path, r)) return failed();
  float stats[kCmvnStats];
  if (pk_mi355_load(config_path, PK_MI355_PRECISION_F32, &r->am, stats)) return failed();
  if (!(r->stream = pk_mi355_stream_create(r->am, stats, max_streams, max_step_samples))) return failed();
  if (!(r->decoder = pk_mi355_online_decoder_create(r->fst, r->am, max_streams, trace_capacity))) return failed();
  if (pk_mi355_online_decoder_set_alignment(r->decoder, 1)) return failed();
  r->max_streams = max_streams;
  r->live.assign(max_streams, 0); r->closed.assign(max_streams, 0); r->finished.assign(max_streams, 0);
  r->partial.assign(max_streams, std::string()); r->hyp.assign(max_streams, std::string());
  r->stable.assign(max_streams, std::string());
  r->stable_words.assign(max_streams, 0);
  r->per_frame.assign(max_streams, 0.0f);
  return r;
}

pk_mi355_am_t *pk_mi355_online_recognizer_am(pk_mi355_online_recognizer_t *r) {
  if (!r) { Fail(PK_MI355_E_INVALID, "null online recognizer"); return nullptr; }
  return r->am;
}
pk_mi355_stream_t *pk_mi355_online_recognizer_stream(pk_mi355_online_recognizer_t *r) {
  if (!r) { Fail(PK_MI355_E_INVALID, "null online recognizer"); return nullptr; }
  return r->stream;
}
pk_mi355_online_decoder_t *pk_mi355_online_recognizer_decoder(pk_mi355_online_recognizer_t *r) {
  if (!r) { Fail(PK_MI355_E_INVALID, "null online recognizer"); return nullptr; }
  return r->decoder;
}
const pk_mi355_symtab_t *pk_mi355_online_recognizer_symtab(const pk_mi355_online_recognizer_t *r) {
  if (!r) { Fail(PK_MI355_E_INVALID, "null online recognizer"); return nullptr; }
  return r->symtab;
}

int pk_mi355_online_recognizer_open(pk_mi355_online_recognizer_t *r, int slot) {
  return pk_mi355_online_recognizer_open_rate(r, slot, pkmi::kSampleRate);
}

int pk_mi355_online_recognizer_open_rate(pk_mi355_online_recognizer_t *r, int slot, int rate) {
  int rc = CheckSlot(r, slot);
  if (rc) return rc;
  // (asked first: a scorer slot, once open, could not be taken back if the decoder then refused its own)
  if (OnlineDecoderSlotOpen(r->decoder, slot)) return Fail(PK_MI355_E_STATE, "online recognizer: slot %d is open in the decoder", slot);
  if ((rc = pk_mi355_stream_open_rate(r->stream, slot, rate)) || (rc = pk_mi355_online_decoder_open(r->decoder, slot))) return rc;
  r->live[slot] = 1; r->closed[slot] = 0; r->finished[slot] = 0;
  r->partial[slot].clear(); r->hyp[slot].clear(); r->stable[slot].clear();
  r->stable_words[slot] = 0;
  r->per_frame[slot] = 0.0f;
  return 0;
}

int pk_mi355_online_recognizer_push(pk_mi355_online_recognizer_t *r, int slot, const float *samples, int num_samples) {
  if (!r) return Fail(PK_MI355_E_INVALID, "null online recognizer");
  return pk_mi355_stream_push(r->stream, slot, samples, num_samples);
}

int pk_mi355_online_recognizer_push_i16(pk_mi355_online_recognizer_t *r, int slot, const int16_t *samples, int num_samples) {
  if (!r) return Fail(PK_MI355_E_INVALID, "null online recognizer");
  return pk_mi355_stream_push_i16(r->stream, slot, samples, num_samples);
}

int pk_mi355_online_recognizer_close(pk_mi355_online_recognizer_t *r, int slot) {
  int rc = CheckSlot(r, slot);
  if (rc) return rc;
  if ((rc = pk_mi355_stream_close(r->stream, slot))) return rc;
  r->closed[slot] = 1;
  return 0;
}

int pk_mi355_online_recognizer_step(pk_mi355_online_recognizer_t *r) {
  if (!r) return Fail(PK_MI355_E_INVALID, "null online recognizer");
  int rc = pk_mi355_stream_step(r->stream, 0.1f, 0);
  if (rc) return rc;
  // What the advance returns is returned.  A slot's verdict (capacity, a closure that did not settle) comes after
  // every slot's result was fetched, so the text is refreshed whatever it said: the other slots go on.
  rc = pk_mi355_online_decoder_advance(r->decoder, r->stream, 1);
  if (!rc) return Refresh(r);
  const std::string said = LastError();                  // (the refresh's getters may say something of their own)
  Refresh(r);
  return Fail(rc, "%s", said.c_str());
}

const char *pk_mi355_online_recognizer_partial(const pk_mi355_online_recognizer_t *r, int slot) {
  if (CheckSlot(r, slot)) return nullptr;
  return r->partial[slot].c_str();
}

const char *pk_mi355_online_recognizer_stable(const pk_mi355_online_recognizer_t *r, int slot) {
  if (CheckSlot(r, slot)) return nullptr;
  return r->stable[slot].c_str();
}

int pk_mi355_online_recognizer_finished(const pk_mi355_online_recognizer_t *r, int slot) {
  int rc = CheckSlot(r, slot);
  if (rc) return rc;
  return r->finished[slot];
}

const char *pk_mi355_online_recognizer_hyp(const pk_mi355_online_recognizer_t *r, int slot) {
  if (CheckSlot(r, slot)) return nullptr;
  if (!r->finished[slot]) { Fail(PK_MI355_E_STATE, "online recognizer: slot %d is not finished", slot); return nullptr; }
  return r->hyp[slot].c_str();
}

float pk_mi355_online_recognizer_loglikelihood_per_frame(const pk_mi355_online_recognizer_t *r, int slot) {
  if (CheckSlot(r, slot)) return NAN;
  if (!r->finished[slot]) { Fail(PK_MI355_E_STATE, "online recognizer: slot %d is not finished", slot); return NAN; }
  return r->per_frame[slot];
}

}  // extern "C"
