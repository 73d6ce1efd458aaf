// capi_online_recognizer.hip -- pk_load + a live pk_process (pocketkaldi.cc:72-248) as one object: model file -> graph,
// symbol table, acoustic model, online scorer and online decoder (alignment on); PCM chunks per slot -> partial text
// while a slot is live, sentence and log-likelihood per frame at its end.  Nothing here computes: the scorer and the
// decoder are the library's own entries, wired slot for slot, and every knob of theirs stays theirs
// (pk_mi355_online_recognizer_am / _stream / _decoder hand them out).  The file-loading half is capi_recognizer.hip's.
#include <string>
#include <utility>
#include <vector>

#include "pk_score.h"

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
  // pk_mi355_online_recognizer_set_endpointing: a slot's stream is cut into utterances where a rule fires.  Per slot the
  // pieces since it was opened, and the frames they hold (the next piece's first_frame)
  bool endpointing = false;
  struct Piece {
    pk_mi355_utterance_t info;
    std::string hyp;
    std::vector<int> words;
    std::vector<pk_mi355_word_t> segments;
  };
  std::vector<std::vector<Piece>> pieces;
  std::vector<int> piece_first;
};

namespace {

// The decoder slot's finished utterance as the slot's next piece (rule: what ended it, 0 for the stream's end).  Text
// and per-frame figure by pk_process's rules (pocketkaldi.cc:239-243); segment frames are relative to first_frame.
int Snapshot(pk_mi355_online_recognizer *r, int slot, int rule) {
  pk_mi355_online_recognizer::Piece p;
  float weight = 0.0f;
  int ok = 0;
  const int count = pk_mi355_online_decoder_result(r->decoder, slot, nullptr, 0, &weight, &ok);
  if (count < 0) return count;
  p.words.resize(count);
  if (count) pk_mi355_online_decoder_result(r->decoder, slot, p.words.data(), count, nullptr, nullptr);
  const int frames = pk_mi355_online_decoder_num_frames(r->decoder, slot);
  if (frames < 0) return frames;
  const int segs = pk_mi355_online_decoder_word_segments(r->decoder, slot, nullptr, 0);
  if (segs < 0) return segs;
  p.segments.resize(segs);
  if (segs) pk_mi355_online_decoder_word_segments(r->decoder, slot, p.segments.data(), segs);
  float per_frame = 0.0f;
  if (ok && count > 0) {
    const int rc = JoinWords(r->symtab, p.words.data(), count, &p.hyp);
    if (rc) return rc;
    per_frame = weight / frames;
  }
  p.info = pk_mi355_utterance_t{r->piece_first[slot], frames, rule, ok, count, segs, weight, per_frame};
  r->piece_first[slot] += frames;
  r->pieces[slot].push_back(std::move(p));
  return 0;
}

// After a step's advance and refresh, with endpointing on: every live slot that is not closing and whose endpoint rule
// fired ends its utterance now (one finish call for all of them), becomes a piece and starts the next utterance at the
// scorer's next row.  The scorer's slot is not touched: CMVN, context and resampler run on.
int CutAtEndpoints(pk_mi355_online_recognizer *r) {
  std::vector<int> cut, rules;
  for (int slot = 0; slot < r->max_streams; ++slot) {
    if (!r->live[slot] || r->closed[slot]) continue;
    const int rule = pk_mi355_online_decoder_endpoint(r->decoder, slot, nullptr);
    if (rule < 0) return rule;
    if (rule > 0) { cut.push_back(slot); rules.push_back(rule); }
  }
  if (cut.empty()) return 0;
  int rc = pk_mi355_online_decoder_finish(r->decoder, cut.data(), (int)cut.size(), 1);
  if (rc) return rc;
  for (size_t i = 0; i < cut.size(); ++i) {
    const int slot = cut[i];
    if ((rc = Snapshot(r, slot, rules[i])) || (rc = pk_mi355_online_decoder_open(r->decoder, slot))) return rc;
    r->partial[slot].clear(); r->stable[slot].clear();      // the next piece's text starts empty
    r->stable_words[slot] = 0;
  }
  return 0;
}

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

// Refresh, and with endpointing on the stream's last piece of every slot that it found finished.
int RefreshAndClose(pk_mi355_online_recognizer *r) {
  if (!r->endpointing) return Refresh(r);
  const std::vector<char> was_live = r->live;
  int rc = Refresh(r);
  for (int slot = 0; slot < r->max_streams && !rc; ++slot)
    if (was_live[slot] && r->finished[slot]) rc = Snapshot(r, slot, 0);
  return rc;
}

// A getter's piece: slot and index in range.
const pk_mi355_online_recognizer::Piece *PieceOf(const pk_mi355_online_recognizer *r, int slot, int i) {
  if (!r) { Fail(PK_MI355_E_INVALID, "null online recognizer"); return nullptr; }
  if (slot < 0 || slot >= r->max_streams) { Fail(PK_MI355_E_INVALID, "slot %d out of range [0, %d)", slot, r->max_streams); return nullptr; }
  if (i < 0 || i >= (int)r->pieces[slot].size()) {
    Fail(PK_MI355_E_INVALID, "online recognizer: slot %d has %d utterances, not %d", slot, (int)r->pieces[slot].size(), i);
    return nullptr;
  }
  return &r->pieces[slot][i];
}

int CheckSlot(const pk_mi355_online_recognizer *r, int slot) {
  if (!r) return Fail(PK_MI355_E_INVALID, "null online recognizer");
  if (slot < 0 || slot >= r->max_streams) return Fail(PK_MI355_E_INVALID, "slot %d out of range [0, %d)", slot, r->max_streams);
  return 0;
}

// open_scorer(): the scorer's own open entry for the slot, audio or features.
template <class OpenScorer>
int OpenSlot(pk_mi355_online_recognizer_t *r, int slot, OpenScorer open_scorer) {
  int rc = CheckSlot(r, slot);
  if (rc) return rc;
  // (asked first: a scorer slot, once open, could not be taken back if the decoder then refused its own)
  if (OnlineDecoderSlotOpen(r->decoder, slot)) return Fail(PK_MI355_E_STATE, "online recognizer: slot %d is open in the decoder", slot);
  if ((rc = open_scorer()) || (rc = pk_mi355_online_decoder_open(r->decoder, slot))) return rc;
  r->live[slot] = 1; r->closed[slot] = 0; r->finished[slot] = 0;
  r->partial[slot].clear(); r->hyp[slot].clear(); r->stable[slot].clear();
  r->stable_words[slot] = 0;
  r->per_frame[slot] = 0.0f;
  r->pieces[slot].clear();
  r->piece_first[slot] = 0;
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

}  // extern "C"

namespace {
// spec null: the reference's model file and front-end; otherwise a model of the spec's dimension (deltas, xform: as
// capi_recognizer.hip's LoadRecognizer).  The online scorer runs f32 models only.
pk_mi355_online_recognizer_t *LoadOnlineRecognizer(int required, const char *config_path, const pk_mi355_frontend_spec_t *spec,
                                                   const pk_mi355_deltas_spec_t *deltas, const pk_mi355_transform_spec_t *xform, int max_streams,
                                                   int64_t max_step_samples, int64_t trace_capacity) {
  if (!CheckLoadArgs(config_path, required, spec, deltas, xform, max_streams, max_step_samples, trace_capacity, "bad online recognizer capacity"))
    return nullptr;
  pk_mi355_online_recognizer *r = new pk_mi355_online_recognizer();
  auto failed = [&]() { pk_mi355_online_recognizer_destroy(r); return nullptr; };
  if (LoadRecognizerFiles(config_path, r, spec != nullptr)) return failed();
  float stats[kMaxCmvnStats];
  CreateRequest req;
  if (LoadModelAndStats(config_path, PK_MI355_PRECISION_F32, spec, deltas, xform, max_streams, max_step_samples, &r->am, stats, &req)) return failed();
  req.live = true;
  if (!(r->stream = CheckedStream(r->am, req))) return failed();
  if (!(r->decoder = pk_mi355_online_decoder_create(r->fst, r->am, max_streams, trace_capacity))) return failed();
  if (pk_mi355_online_decoder_set_alignment(r->decoder, 1)) return failed();
  r->max_streams = max_streams;
  r->live.assign(max_streams, 0); r->closed.assign(max_streams, 0); r->finished.assign(max_streams, 0);
  r->partial.assign(max_streams, std::string()); r->hyp.assign(max_streams, std::string());
  r->stable.assign(max_streams, std::string());
  r->stable_words.assign(max_streams, 0);
  r->per_frame.assign(max_streams, 0.0f);
  r->pieces.assign(max_streams, std::vector<pk_mi355_online_recognizer::Piece>());
  r->piece_first.assign(max_streams, 0);
  return r;
}
}  // namespace

extern "C" {

pk_mi355_online_recognizer_t *pk_mi355_online_recognizer_load(const char *config_path, int max_streams, int64_t max_step_samples,
                                                              int64_t trace_capacity) {
  return LoadOnlineRecognizer(0, config_path, nullptr, nullptr, nullptr, max_streams, max_step_samples, trace_capacity);
}

pk_mi355_online_recognizer_t *pk_mi355_frontend_online_recognizer_load(const char *config_path, const pk_mi355_frontend_spec_t *spec,
                                                                       int max_streams, int64_t max_step_samples, int64_t trace_capacity) {
  return LoadOnlineRecognizer(kNeedFrontend, config_path, spec, nullptr, nullptr, max_streams, max_step_samples, trace_capacity);
}

pk_mi355_online_recognizer_t *pk_mi355_deltas_online_recognizer_load(const char *config_path, const pk_mi355_frontend_spec_t *frontend_spec,
                                                                     const pk_mi355_deltas_spec_t *deltas_spec, int max_streams,
                                                                     int64_t max_step_samples, int64_t trace_capacity) {
  return LoadOnlineRecognizer(kNeedFrontend | kNeedDeltas, config_path, frontend_spec, deltas_spec, nullptr, max_streams, max_step_samples,
                              trace_capacity);
}

pk_mi355_online_recognizer_t *pk_mi355_transform_online_recognizer_load(const char *config_path, const pk_mi355_frontend_spec_t *frontend_spec,
                                                                        const pk_mi355_deltas_spec_t *deltas_spec,
                                                                        const pk_mi355_transform_spec_t *transform_spec, int max_streams,
                                                                        int64_t max_step_samples, int64_t trace_capacity) {
  return LoadOnlineRecognizer(kNeedFrontend | kNeedTransform, config_path, frontend_spec, deltas_spec, transform_spec, max_streams, max_step_samples,
                              trace_capacity);
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
  return OpenSlot(r, slot, [&] { return pk_mi355_stream_open_rate(r->stream, slot, rate); });
}

int pk_mi355_online_recognizer_open_features(pk_mi355_online_recognizer_t *r, int slot, int kind) {
  return OpenSlot(r, slot, [&] { return pk_mi355_stream_open_features(r->stream, slot, kind); });
}

int pk_mi355_online_recognizer_push_features(pk_mi355_online_recognizer_t *r, int slot, const float *frames, int num_frames) {
  if (!r) return Fail(PK_MI355_E_INVALID, "null online recognizer");
  return pk_mi355_stream_push_features(r->stream, slot, frames, num_frames);
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
  if (!rc) {
    if ((rc = RefreshAndClose(r)) || !r->endpointing) return rc;
    return CutAtEndpoints(r);
  }
  const std::string said = LastError();                  // (the refresh's getters may say something of their own)
  RefreshAndClose(r);
  if (r->endpointing) CutAtEndpoints(r);                 // (the other slots go on, cuts included)
  return Fail(rc, "%s", said.c_str());
}

int pk_mi355_online_recognizer_set_endpointing(pk_mi355_online_recognizer_t *r, const int32_t *silence_pdfs, int num_silence,
                                               const pk_mi355_endpoint_rule_t *rules, int num_rules) {
  if (!r) return Fail(PK_MI355_E_INVALID, "null online recognizer");
  for (int slot = 0; slot < r->max_streams; ++slot)
    if (r->live[slot]) return Fail(PK_MI355_E_STATE, "online recognizer: slot %d is open (set_endpointing needs every slot closed)", slot);
  const int rc = pk_mi355_online_decoder_set_endpointing(r->decoder, silence_pdfs, num_silence, rules, num_rules);
  if (rc) return rc;
  r->endpointing = num_rules > 0;
  return 0;
}

int pk_mi355_online_recognizer_num_utterances(const pk_mi355_online_recognizer_t *r, int slot) {
  const int rc = CheckSlot(r, slot);
  if (rc) return rc;
  return (int)r->pieces[slot].size();
}

int pk_mi355_online_recognizer_utterance(const pk_mi355_online_recognizer_t *r, int slot, int i, pk_mi355_utterance_t *out) {
  const pk_mi355_online_recognizer::Piece *p = PieceOf(r, slot, i);
  if (!p) return PK_MI355_E_INVALID;
  if (out) *out = p->info;
  return 0;
}

const char *pk_mi355_online_recognizer_utterance_hyp(const pk_mi355_online_recognizer_t *r, int slot, int i) {
  const pk_mi355_online_recognizer::Piece *p = PieceOf(r, slot, i);
  return p ? p->hyp.c_str() : nullptr;
}

int pk_mi355_online_recognizer_utterance_words(const pk_mi355_online_recognizer_t *r, int slot, int i, int *words, int max) {
  const pk_mi355_online_recognizer::Piece *p = PieceOf(r, slot, i);
  if (!p) return PK_MI355_E_INVALID;
  for (int k = 0; words && k < (int)p->words.size() && k < max; ++k) words[k] = p->words[k];
  return (int)p->words.size();
}

int pk_mi355_online_recognizer_utterance_word_segments(const pk_mi355_online_recognizer_t *r, int slot, int i,
                                                       pk_mi355_word_t *out, int max) {
  const pk_mi355_online_recognizer::Piece *p = PieceOf(r, slot, i);
  if (!p) return PK_MI355_E_INVALID;
  for (int k = 0; out && k < (int)p->segments.size() && k < max; ++k) out[k] = p->segments[k];
  return (int)p->segments.size();
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
