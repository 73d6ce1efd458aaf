// capi_recognizer.hip -- pk_load + pk_process (pocketkaldi.cc:72-248) as one object: model file -> graph, symbol
// table, acoustic model, batch scorer and decoder (alignment on); waves -> sentence and log-likelihood per frame.
// Nothing here computes: the scorer and the decoder are the library's own entries, and every knob of theirs stays
// theirs (pk_mi355_recognizer_am / _batch / _decoder hand them out).
#include <string>
#include <vector>

#include "pk_score.h"

using namespace pkhost;

namespace pkhost {

int LoadRecognizerFiles(const char *config_path, RecognizerFiles *r, bool any_stats) {
  // pk_load's order (pocketkaldi.cc:81-131): fst, cmvn_stats, the AcousticModel keys, symbol_table.  Keys and host-side
  // files first, so that a model file that cannot work is refused before the device is touched.
  std::string path;
  ModelConfig conf;
  if (ConfigPath(config_path, "fst", &path) || !(r->fst = pk_mi355_fst_read(path.c_str()))) return pk_mi355_last_error_code();
  int rc = any_stats ? ReadModelConfigStats(config_path, kMaxCmvnStats, &conf) : ReadModelConfig(config_path, &conf);
  if (rc) return rc;
  if (ConfigPath(config_path, "symbol_table", &path) || !(r->symtab = pk_mi355_symtab_read(path.c_str())))
    return pk_mi355_last_error_code();
  const int symbols = pk_mi355_symtab_size(r->symtab);
  for (int a = 0; a < r->fst->num_arcs; ++a)       // pk_symboltable_get asserts this when the word is looked up
    if (r->fst->arcs[a].olabel >= symbols)
      return Fail(PK_MI355_E_INVALID, "%s: arc %d of the graph has output label %d, the symbol table has %d symbols", config_path, a,
                  r->fst->arcs[a].olabel, symbols);
  return 0;
}

void FreeRecognizerFiles(RecognizerFiles *f) {
  pk_mi355_symtab_destroy(f->symtab);
  pk_mi355_fst_destroy(f->fst);
  f->symtab = nullptr; f->fst = nullptr;
}

int LoadModelAndStats(const char *config_path, int precision, const pk_mi355_frontend_spec_t *frontend, const pk_mi355_deltas_spec_t *deltas,
                      const pk_mi355_transform_spec_t *xform, int units, int64_t capacity, pk_mi355_am_t **am, float *stats, CreateRequest *r) {
  int stats_len = 0;
  *r = CreateRequest{stats, 0, !frontend, units, capacity, true, false, frontend, deltas, xform};
  if (!frontend) return pk_mi355_load(config_path, precision, am, stats);      // (41 statistics by that entry's contract)
  // a transform's scorer holds the statistics to its base dimension; deltas put them at feat_dim / (order + 1)
  const int rc = xform    ? LoadStatsBlocks(config_path, precision, 0, am, stats, kMaxCmvnStats, &stats_len)
                 : deltas ? LoadStatsBlocks(config_path, precision, deltas->order + 1, am, stats, kMaxCmvnStats, &stats_len)
                          : pk_mi355_load_stats(config_path, precision, am, stats, kMaxCmvnStats, &stats_len);
  r->stats_len = stats_len;
  return rc;
}

int JoinWords(const pk_mi355_symtab_t *symtab, const int *words, int count, std::string *text) {
  text->clear();
  for (int i = 0; i < count; ++i) {
    const char *word = pk_mi355_symtab_get(symtab, words[i]);
    if (!word) return pk_mi355_last_error_code();  // (cannot happen: load has checked every olabel)
    if (i) *text += ' ';                           // (:232-238: a space after every word, the last one dropped by pk_strlcpy)
    *text += word;
  }
  return 0;
}

}  // namespace pkhost

struct pk_mi355_recognizer : RecognizerFiles {
  pk_mi355_am_t *am = nullptr;
  pk_mi355_batch_t *batch = nullptr;
  pk_mi355_decoder_t *decoder = nullptr;
  bool have = false;                       // results of a process call are readable
  std::vector<std::string> hyp;            // per utterance of the last process
  std::vector<float> per_frame;
};

extern "C" {

void pk_mi355_recognizer_destroy(pk_mi355_recognizer_t *r) {
  if (!r) return;
  pk_mi355_decoder_destroy(r->decoder);    // (waits for its last call, which reads the batch's rows)
  pk_mi355_batch_destroy(r->batch);
  pk_mi355_am_destroy(r->am);
  FreeRecognizerFiles(r);
  delete r;
}

}  // extern "C"

namespace {
// spec null: the reference's model file and front-end; otherwise a model of the spec's dimension
// deltas (with a spec only): the model's features are (order + 1) x the spec's, the statistics at the spec's dimension
// xform (with a spec only): the model's features are the transform's output, the statistics at the spec's dimension
pk_mi355_recognizer_t *LoadRecognizer(int required, const char *config_path, const pk_mi355_frontend_spec_t *spec, const pk_mi355_deltas_spec_t *deltas,
                                      const pk_mi355_transform_spec_t *xform, int precision, int max_utts, int64_t max_total_samples,
                                      int64_t trace_capacity) {
  if (!CheckLoadArgs(config_path, required, spec, deltas, xform, max_utts, max_total_samples, trace_capacity, "bad recognizer capacity")) return nullptr;
  pk_mi355_recognizer *r = new pk_mi355_recognizer();
  auto failed = [&]() { pk_mi355_recognizer_destroy(r); return nullptr; };
  if (LoadRecognizerFiles(config_path, r, spec != nullptr)) return failed();
  float stats[kMaxCmvnStats];
  CreateRequest req;
  if (LoadModelAndStats(config_path, precision, spec, deltas, xform, max_utts, max_total_samples, &r->am, stats, &req)) return failed();
  if (!(r->batch = CheckedBatch(r->am, req))) return failed();
  if (!(r->decoder = pk_mi355_decoder_create(r->fst, r->am, max_utts, trace_capacity))) return failed();
  if (pk_mi355_decoder_set_alignment(r->decoder, 1)) return failed();
  return r;
}
}  // namespace

extern "C" {

pk_mi355_recognizer_t *pk_mi355_recognizer_load(const char *config_path, int precision, int max_utts, int64_t max_total_samples,
                                                int64_t trace_capacity) {
  return LoadRecognizer(0, config_path, nullptr, nullptr, nullptr, precision, max_utts, max_total_samples, trace_capacity);
}

pk_mi355_recognizer_t *pk_mi355_frontend_recognizer_load(const char *config_path, const pk_mi355_frontend_spec_t *spec, int precision,
                                                         int max_utts, int64_t max_total_samples, int64_t trace_capacity) {
  return LoadRecognizer(kNeedFrontend, config_path, spec, nullptr, nullptr, precision, max_utts, max_total_samples, trace_capacity);
}

pk_mi355_recognizer_t *pk_mi355_deltas_recognizer_load(const char *config_path, const pk_mi355_frontend_spec_t *frontend_spec,
                                                       const pk_mi355_deltas_spec_t *deltas_spec, int precision, int max_utts,
                                                       int64_t max_total_samples, int64_t trace_capacity) {
  return LoadRecognizer(kNeedFrontend | kNeedDeltas, config_path, frontend_spec, deltas_spec, nullptr, precision, max_utts, max_total_samples,
                        trace_capacity);
}

pk_mi355_recognizer_t *pk_mi355_transform_recognizer_load(const char *config_path, const pk_mi355_frontend_spec_t *frontend_spec,
                                                          const pk_mi355_deltas_spec_t *deltas_spec, const pk_mi355_transform_spec_t *transform_spec,
                                                          int precision, int max_utts, int64_t max_total_samples, int64_t trace_capacity) {
  return LoadRecognizer(kNeedFrontend | kNeedTransform, config_path, frontend_spec, deltas_spec, transform_spec, precision, max_utts, max_total_samples,
                        trace_capacity);
}

pk_mi355_am_t *pk_mi355_recognizer_am(pk_mi355_recognizer_t *r) {
  if (!r) { Fail(PK_MI355_E_INVALID, "null recognizer"); return nullptr; }
  return r->am;
}
pk_mi355_batch_t *pk_mi355_recognizer_batch(pk_mi355_recognizer_t *r) {
  if (!r) { Fail(PK_MI355_E_INVALID, "null recognizer"); return nullptr; }
  return r->batch;
}
pk_mi355_decoder_t *pk_mi355_recognizer_decoder(pk_mi355_recognizer_t *r) {
  if (!r) { Fail(PK_MI355_E_INVALID, "null recognizer"); return nullptr; }
  return r->decoder;
}
const pk_mi355_symtab_t *pk_mi355_recognizer_symtab(const pk_mi355_recognizer_t *r) {
  if (!r) { Fail(PK_MI355_E_INVALID, "null recognizer"); return nullptr; }
  return r->symtab;
}

int pk_mi355_recognizer_process(pk_mi355_recognizer_t *r, const pk_vector_t *waves, int n) {
  return pk_mi355_recognizer_process_rates(r, waves, nullptr, n);
}

}  // extern "C"

namespace {
// pk_process behind the batch's set_* call (`set`: the call that hands the n utterances over): score, decode, collect.
template <class Set>
int ProcessWith(pk_mi355_recognizer *r, int n, Set set) {
  r->have = false;
  int rc;
  if ((rc = set()) || (rc = pk_mi355_batch_score(r->batch, 0.1f, 0)) || (rc = pk_mi355_decoder_decode_batch(r->decoder, r->batch, 1)))
    return rc;
  r->hyp.assign(n, std::string());
  r->per_frame.assign(n, 0.0f);
  std::vector<int> words;
  for (int u = 0; u < n; ++u) {
    float weight = 0.0f;
    int ok = 0;
    const int count = pk_mi355_decoder_result(r->decoder, u, nullptr, 0, &weight, &ok);
    if (count < 0) return count;
    if (!ok || count == 0) continue;                 // pocketkaldi.cc:240-243: no words, "" and 0.0f
    words.resize(count);
    pk_mi355_decoder_result(r->decoder, u, words.data(), count, &weight, &ok);
    if ((rc = JoinWords(r->symtab, words.data(), count, &r->hyp[u]))) return rc;
    r->per_frame[u] = weight / pk_mi355_batch_num_frames(r->batch, u);     // :239
  }
  r->have = true;
  return 0;
}
}  // namespace

extern "C" {

int pk_mi355_recognizer_process_rates(pk_mi355_recognizer_t *r, const pk_vector_t *waves, const int *rates, int n) {
  if (!r || n < 0 || (n > 0 && !waves)) return Fail(PK_MI355_E_INVALID, "bad process arguments");
  pk_vector_t none = {0, nullptr};
  return ProcessWith(r, n, [&] { return pk_mi355_resample_set_waves(r->batch, n ? waves : &none, rates, n); });
}

int pk_mi355_recognizer_process_features(pk_mi355_recognizer_t *r, const pk_matrix_t *feats, int n, int kind) {
  if (!r || n < 0 || (n > 0 && !feats)) return Fail(PK_MI355_E_INVALID, "bad process arguments");
  return ProcessWith(r, n, [&] { return pk_mi355_features_set(r->batch, feats, n, kind); });
}

const char *pk_mi355_recognizer_hyp(const pk_mi355_recognizer_t *r, int utt) {
  if (!r) { Fail(PK_MI355_E_INVALID, "null recognizer"); return nullptr; }
  if (!r->have) { Fail(PK_MI355_E_STATE, "recognizer: nothing processed"); return nullptr; }
  if (utt < 0 || utt >= (int)r->hyp.size()) { Fail(PK_MI355_E_INVALID, "bad utterance index"); return nullptr; }
  return r->hyp[utt].c_str();
}

float pk_mi355_recognizer_loglikelihood_per_frame(const pk_mi355_recognizer_t *r, int utt) {
  if (!r) { Fail(PK_MI355_E_INVALID, "null recognizer"); return NAN; }
  if (!r->have) { Fail(PK_MI355_E_STATE, "recognizer: nothing processed"); return NAN; }
  if (utt < 0 || utt >= (int)r->hyp.size()) { Fail(PK_MI355_E_INVALID, "bad utterance index"); return NAN; }
  return r->per_frame[utt];
}

}  // extern "C"
