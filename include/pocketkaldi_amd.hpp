// pocketkaldi_amd.hpp -- header-only C++ host mirror of the reference's classes for the
// acoustic-scoring path, over the C ABI of libpk_mi355.so (include/pk_mi355.h).
//
// Same names, argument meaning and ownership rules as the reference, so code written against
// pocketkaldi's headers reads the same:
//
//   pocketkaldi::Fbank::Compute(const pk_vector_t*, pk_matrix_t*)        src/fbank.h:47-53
//   pocketkaldi::CMVN(global_stats, raw).GetFrame(t, pk_vector_t*)       src/cmvn.h:17-26
//   pocketkaldi::AcousticModel::Read / num_pdfs / TransitionIdToPdfId    src/am.h:23-52
//   pocketkaldi::AcousticModel::Compute(frames, loglikelihood)           src/am.h:35
//   pk_decodable_init/_destroy/_loglikelihood/_islastframe               src/decodable.h:20-41
//   pocketkaldi::Fst::Read / CountArcs                                   src/fst.h
//   pocketkaldi::Decoder(fst, am).Decode(pk_decodable_t*) / BestPath()   src/decoder.h (on the GPU)
//   pocketkaldi::Decoder::SetAlignment / Alignment / WordSegments        per-frame arcs and costs, word times
//   pocketkaldi::SymbolTable::Read / size / Get                          src/symbol_table.h
//   pocketkaldi::Recognizer::Load / Process                              pk_load + pk_process, src/pocketkaldi.cc:72-248
//   pocketkaldi::OnlineScorer(am, stats, ...).Push / Step / Fetch        live PCM, frames scored as they become final
//   pocketkaldi::OnlineDecoder(fst, am, ...).Advance / Partial / Result  the search over them, partial text while live
//
// Error behaviour: the reference reports load errors through Status and treats misuse as
// assert(); here load / device errors surface as pocketkaldi::Status (ok() / what()), and the
// void compute members throw nothing -- they leave the output empty and set Status, readable
// through last_status().  No exception crosses the C ABI.
#ifndef POCKETKALDI_AMD_HPP_
#define POCKETKALDI_AMD_HPP_

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "pk_mi355.h"

namespace pocketkaldi {

// src/status.h:37-100, reduced to what this path needs.
class Status {
 public:
  Status() : code_(0) {}
  Status(int code, const std::string &msg) : code_(code), msg_(msg) {}
  static Status OK() { return Status(); }
  static Status FromLast(int code) { return code == 0 ? Status() : Status(code, pk_mi355_last_error()); }
  bool ok() const { return code_ == 0; }
  int code() const { return code_; }
  const std::string &what() const { return msg_; }

 private:
  int code_;
  std::string msg_;
};

// src/fbank.h:47-53
class Fbank {
 public:
  // wave: 16 kHz mono sample values as pk_16kpcm_read produces them; fbank_feature is
  // resized (realloc) to {nrow = 40, ncol = T} like src/fbank.cc:267-276.
  void Compute(const pk_vector_t *wave, pk_matrix_t *fbank_feature) {
    status_ = Status::FromLast(pk_mi355_fbank_compute(wave, fbank_feature));
  }
  const Status &last_status() const { return status_; }

 private:
  Status status_;
};

// src/cmvn.h:17-26.  The reference computes frame by frame and asserts sequential access
// (src/cmvn.cc:38); here all frames are produced on the first GetFrame() and served from a
// host copy, so any access order works.
class CMVN {
 public:
  CMVN(const pk_vector_t *global_stats, const pk_matrix_t *raw_feats)
      : global_stats_(global_stats), raw_(raw_feats), done_(false) {
    out_.ncol = out_.nrow = 0;
    out_.data = nullptr;
  }
  ~CMVN() { free(out_.data); }
  CMVN(const CMVN &) = delete;
  CMVN &operator=(const CMVN &) = delete;

  void GetFrame(int frame, pk_vector_t *feats) {
    if (!done_) {
      status_ = Status::FromLast(pk_mi355_cmvn_apply(global_stats_, raw_, &out_));
      done_ = true;
    }
    if (!status_.ok() || frame < 0 || frame >= out_.ncol) return;
    if (feats->dim != out_.nrow) {   // pk_vector_copy resizes (src/vector.cc)
      feats->data = static_cast<float *>(realloc(feats->data, sizeof(float) * out_.nrow));
      feats->dim = out_.nrow;
    }
    memcpy(feats->data, out_.data + static_cast<size_t>(frame) * out_.nrow, sizeof(float) * out_.nrow);
  }
  // all frames at once: {nrow = 40, ncol = T}, owned by this object
  const pk_matrix_t *AllFrames() {
    pk_vector_t dummy = {0, nullptr};
    GetFrame(-1, &dummy);
    return &out_;
  }
  const Status &last_status() const { return status_; }

 private:
  const pk_vector_t *global_stats_;
  const pk_matrix_t *raw_;
  pk_matrix_t out_;
  bool done_;
  Status status_;
};

// src/am.h:23-52 (+ the Nnet it owns, src/nnet.h:88-104)
class AcousticModel {
 public:
  AcousticModel() : am_(pk_mi355_am_create()) {}
  ~AcousticModel() { pk_mi355_am_destroy(am_); }
  AcousticModel(const AcousticModel &) = delete;
  AcousticModel &operator=(const AcousticModel &) = delete;

  // AcousticModel::Read (src/am.cc:23-63) with the Configuration already resolved to paths
  // and integers (keys nnet, prior, left_context, right_context, num_pdfs, tid2pdf).
  Status Read(const std::string &nnet, const std::string &prior, const std::string &tid2pdf,
              int left_context, int right_context, int num_pdfs) {
    return Status::FromLast(pk_mi355_am_read(am_, nnet.c_str(), prior.c_str(),
                                             tid2pdf.empty() ? nullptr : tid2pdf.c_str(),
                                             left_context, right_context, num_pdfs));
  }
  // In-memory construction (what Nnet::ReadLayer does per layer, src/nnet.cc:80-130)
  Status AddLinear(int in_dim, int out_dim, const float *W, const float *b) {
    return Status::FromLast(pk_mi355_am_add_linear(am_, in_dim, out_dim, W, b));
  }
  Status AddLayer(int layer_type) { return Status::FromLast(pk_mi355_am_add_layer(am_, layer_type)); }
  // PK_NNET_ADD_LAYER / PK_NNET_MUL_LAYER with their vector; the 2-norm of groups of in_dim / out_dim features
  Status AddVectorLayer(int kind, const std::vector<float> &v) {
    return Status::FromLast(pk_mi355_am_add_vector_layer(am_, kind, static_cast<int>(v.size()), v.data()));
  }
  Status AddPnorm(int in_dim, int out_dim) { return Status::FromLast(pk_mi355_am_add_pnorm(am_, in_dim, out_dim)); }
  // PK_MI355_NNET_TIME_SPLICE_LAYER: in_dim -> offsets.size() * in_dim, y[t][c in_dim + d] = x[t + offsets[c]][d]
  Status AddTimeSplice(int in_dim, const std::vector<int32_t> &offsets) {
    return Status::FromLast(pk_mi355_am_add_time_splice(am_, in_dim, offsets.data(), static_cast<int>(offsets.size())));
  }
  // what the time-splice layers consume together on the left and on the right ((0, 0) without any; after Finalize)
  Status TimeContext(int *left, int *right) const { return Status::FromLast(pk_mi355_am_time_context(am_, left, right)); }
  Status Finalize(const std::vector<float> &prior, int left_context, int right_context,
                  const std::vector<int32_t> &tid2pdf) {
    return Status::FromLast(pk_mi355_am_finalize(am_, prior.data(), static_cast<int>(prior.size()),
                                                 left_context, right_context,
                                                 tid2pdf.empty() ? nullptr : tid2pdf.data(),
                                                 static_cast<int>(tid2pdf.size())));
  }

  int TransitionIdToPdfId(int transition_id) const { return pk_mi355_am_transition_to_pdf(am_, transition_id); }
  int num_pdfs() const { return pk_mi355_am_num_pdfs(am_); }
  int feat_dim() const { return pk_mi355_am_feat_dim(am_); }   // 0 until the model is finalized

  // src/am.cc:90-115: frames {nrow = feat_dim, ncol = T} -> loglikelihood {nrow = num_pdfs,
  // ncol = T} = log(max(p, 1e-20)) - log prior  (no acoustic scale; pk_decodable_init applies it)
  void Compute(const pk_matrix_t *frames, pk_matrix_t *loglikelihood) {
    pk_decodable_t d;
    pk_decodable_init(&d, am_, 1.0f, frames);
    free(loglikelihood->data);
    *loglikelihood = d.log_prob;   // ownership moves to the caller, as with pk_matrix_t in the reference
  }

  pk_mi355_am_t *handle() const { return am_; }

 private:
  pk_mi355_am_t *am_;
};

// src/fst.h: the decoding graph, read on the host (Fst::Read, src/fst.cc:29-92)
class Fst {
 public:
  Fst() : fst_(nullptr) {}
  ~Fst() { pk_mi355_fst_destroy(fst_); }
  Fst(const Fst &) = delete;
  Fst &operator=(const Fst &) = delete;

  Status Read(const std::string &path) {
    pk_mi355_fst_destroy(fst_);
    fst_ = pk_mi355_fst_read(path.c_str());
    return fst_ ? Status() : Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  int start_state() const { return pk_mi355_fst_start(fst_); }
  int num_states() const { return pk_mi355_fst_num_states(fst_); }
  int num_arcs() const { return pk_mi355_fst_num_arcs(fst_); }
  // Fst::CountArcs (src/fst.cc:94-110)
  int CountArcs(int state) const {
    int first = 0, count = 0;
    return pk_mi355_fst_arc_range(fst_, state, &first, &count) == 0 ? count : 0;
  }
  const pk_mi355_fst_t *handle() const { return fst_; }

 private:
  pk_mi355_fst_t *fst_;
};

// src/decoder.h: Decoder::Decode + BestPath on the GPU (one utterance per call; pk_mi355_decoder_decode_batch
// decodes a whole scored batch).  The graph's device copy is made for `am` (its tid2pdf maps the ilabels).
class Decoder {
 public:
  // src/decoder.h:34-40
  class Hypothesis {
   public:
    Hypothesis(const std::vector<int> &words, float weight) : words_(words), weight_(weight) {}
    // The reference's order: last word first (pk_process reverses it, src/pocketkaldi.cc:226-227)
    const std::vector<int> &words() const { return words_; }
    float weight() const { return weight_; }

   private:
    std::vector<int> words_;
    float weight_;
  };

  Decoder(const Fst *fst, pk_mi355_am_t *am) : d_(pk_mi355_decoder_create(fst->handle(), am, 1, 0)) {
    if (!d_) status_ = Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  ~Decoder() { pk_mi355_decoder_destroy(d_); }
  Decoder(const Decoder &) = delete;
  Decoder &operator=(const Decoder &) = delete;

  Status SetBeam(float beam, int max_active) { return Status::FromLast(pk_mi355_decoder_set_beam(d_, beam, max_active)); }
  // From the next Decode on: the backtrace is compacted as it fills (pk_mi355_decoder_set_trace_gc); same results
  Status SetTraceGc(bool on) { return Status::FromLast(pk_mi355_decoder_set_trace_gc(d_, on ? 1 : 0)); }
  // Backtrace use of the last Decode (pk_mi355_decoder_trace_stats), for sizing trace_capacity
  Status TraceStats(int64_t *peak_records, int64_t *slice_records, int *compactions) const {
    return Status::FromLast(pk_mi355_decoder_trace_stats(d_, 0, peak_records, slice_records, compactions));
  }

  // Decoder::Decode (src/decoder.cc:39-77): true when tokens survive the last frame.  A device or capacity
  // failure returns false and sets last_status().
  bool Decode(pk_decodable_t *decodable) {
    if (!d_) return false;
    status_ = Status::FromLast(pk_mi355_decoder_decode(d_, decodable, 1, 1));
    if (!status_.ok()) return false;
    int ok = 0;
    pk_mi355_decoder_result(d_, 0, nullptr, 0, nullptr, &ok);
    return ok != 0;
  }

  // Decoder::BestPath (src/decoder.cc:304-339) of the last Decode
  Hypothesis BestPath() const {
    float weight = 0.0f;
    const int n = d_ && status_.ok() ? pk_mi355_decoder_result(d_, 0, nullptr, 0, &weight, nullptr) : 0;
    if (n <= 0) return Hypothesis(std::vector<int>(), 0.0f);
    std::vector<int> words(n);
    pk_mi355_decoder_result(d_, 0, words.data(), n, &weight, nullptr);
    std::reverse(words.begin(), words.end());
    return Hypothesis(words, weight);
  }

  // From the next Decode on: the frame-by-frame alignment of the best path is kept (pk_mi355_decoder_set_alignment)
  Status SetAlignment(bool on) { return Status::FromLast(pk_mi355_decoder_set_alignment(d_, on ? 1 : 0)); }
  // Per frame of the last Decode: the best path's emitting arc, its transition-id and its acoustic cost (any pointer
  // may be null).  Returns the frames aligned, or a negative code (alignment off: PK_MI355_E_STATE).
  int Alignment(std::vector<int32_t> *arc_ids, std::vector<int32_t> *trans_ids, std::vector<float> *acoustic_cost) const {
    const int n = pk_mi355_decoder_alignment(d_, 0, nullptr, nullptr, nullptr, 0);
    if (n < 0) return n;
    if (arc_ids) arc_ids->resize(n);
    if (trans_ids) trans_ids->resize(n);
    if (acoustic_cost) acoustic_cost->resize(n);
    return pk_mi355_decoder_alignment(d_, 0, arc_ids ? arc_ids->data() : nullptr, trans_ids ? trans_ids->data() : nullptr,
                                      acoustic_cost ? acoustic_cost->data() : nullptr, n);
  }
  // The word segments of the last Decode's best path, in spoken order (empty on failure: see the C entry)
  std::vector<pk_mi355_word_t> WordSegments() const {
    const int n = pk_mi355_decoder_word_segments(d_, 0, nullptr, 0);
    std::vector<pk_mi355_word_t> out(n > 0 ? n : 0);
    if (n > 0) pk_mi355_decoder_word_segments(d_, 0, out.data(), n);
    return out;
  }

  const Status &last_status() const { return status_; }

 private:
  pk_mi355_decoder_t *d_;
  Status status_;
};

// src/symbol_table.h: the word list (pk_symboltable_read / pk_symboltable_get, src/symbol_table.cc:23-79)
class SymbolTable {
 public:
  SymbolTable() : st_(nullptr) {}
  ~SymbolTable() { pk_mi355_symtab_destroy(st_); }
  SymbolTable(const SymbolTable &) = delete;
  SymbolTable &operator=(const SymbolTable &) = delete;

  Status Read(const std::string &path) {
    pk_mi355_symtab_destroy(st_);
    st_ = pk_mi355_symtab_read(path.c_str());
    return st_ ? Status() : Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  int size() const { return st_ ? pk_mi355_symtab_size(st_) : 0; }
  // nullptr outside [0, size()), where the reference asserts
  const char *Get(int symbol_id) const { return st_ ? pk_mi355_symtab_get(st_, symbol_id) : nullptr; }

 private:
  pk_mi355_symtab_t *st_;
};

// Audio as people have it: a WAV file of any rate and up to 8 channels, and its conversion to
// the 16 kHz the recognizer hears, on the GPU.
// ReadWave: channel `channel` of the file into *samples (sample values as pk_mi355_16kpcm_read gives them) and its rate.
inline Status ReadWave(const std::string &path, int channel, std::vector<float> *samples, int *rate) {
  pk_vector_t v = {0, nullptr};
  const int rc = pk_mi355_wave_read(path.c_str(), channel, &v, rate, nullptr);
  if (rc == 0) samples->assign(v.data, v.data + v.dim);
  free(v.data);
  return Status::FromLast(rc);
}
// Resample: samples at `rate` Hz -> 16 kHz (pk_mi355_resample; 16000 is the identity)
inline Status Resample(const std::vector<float> &wave, int rate, std::vector<float> *out) {
  pk_vector_t in = {(int)wave.size(), const_cast<float *>(wave.data())}, v = {0, nullptr};
  const int rc = pk_mi355_resample(&in, rate, &v);
  if (rc == 0) out->assign(v.data, v.data + v.dim);
  free(v.data);
  return Status::FromLast(rc);
}

// pk_t + pk_load + pk_process (src/pocketkaldi.h, src/pocketkaldi.cc:72-248): model file and waves to text.
class Recognizer {
 public:
  // pk_utterance_t's results (src/pocketkaldi.h): hyp and loglikelihood_per_frame
  struct Utterance {
    std::string hyp;
    float loglikelihood_per_frame;
  };

  Recognizer() : r_(nullptr) {}
  ~Recognizer() { pk_mi355_recognizer_destroy(r_); }
  Recognizer(const Recognizer &) = delete;
  Recognizer &operator=(const Recognizer &) = delete;

  Status Load(const std::string &model_file, int precision = PK_MI355_PRECISION_F32, int max_utts = 1,
              int64_t max_total_samples = 16000 * 60, int64_t trace_capacity = 0) {
    pk_mi355_recognizer_destroy(r_);
    r_ = pk_mi355_recognizer_load(model_file.c_str(), precision, max_utts, max_total_samples, trace_capacity);
    return r_ ? Status() : Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // A model of the spec's feature dimension (a FrontendSpec; pk_mi355_frontend_recognizer_load)
  Status Load(const std::string &model_file, const pk_mi355_frontend_spec_t &spec, int precision = PK_MI355_PRECISION_F32,
              int max_utts = 1, int64_t max_total_samples = 16000 * 60, int64_t trace_capacity = 0) {
    pk_mi355_recognizer_destroy(r_);
    r_ = pk_mi355_frontend_recognizer_load(model_file.c_str(), &spec, precision, max_utts, max_total_samples, trace_capacity);
    return r_ ? Status() : Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // A model of (order + 1) x the spec's feature dimension, deltas behind the normalisation (a FrontendSpec and a
  // DeltaSpec; pk_mi355_deltas_recognizer_load)
  Status Load(const std::string &model_file, const pk_mi355_frontend_spec_t &spec, const pk_mi355_deltas_spec_t &deltas,
              int precision = PK_MI355_PRECISION_F32, int max_utts = 1, int64_t max_total_samples = 16000 * 60, int64_t trace_capacity = 0) {
    pk_mi355_recognizer_destroy(r_);
    r_ = pk_mi355_deltas_recognizer_load(model_file.c_str(), &spec, &deltas, precision, max_utts, max_total_samples, trace_capacity);
    return r_ ? Status() : Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // A model of the transform's output dimension, the transform behind the normalisation and (deltas not null) the deltas
  // (pk_mi355_transform_recognizer_load)
  Status Load(const std::string &model_file, const pk_mi355_frontend_spec_t &spec, const pk_mi355_deltas_spec_t *deltas,
              const pk_mi355_transform_spec_t &transform, int precision = PK_MI355_PRECISION_F32, int max_utts = 1,
              int64_t max_total_samples = 16000 * 60, int64_t trace_capacity = 0) {
    pk_mi355_recognizer_destroy(r_);
    r_ = pk_mi355_transform_recognizer_load(model_file.c_str(), &spec, deltas, &transform, precision, max_utts, max_total_samples, trace_capacity);
    return r_ ? Status() : Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // pk_process for n waves at once; out (may be null) receives one Utterance per wave.  rates (may be null: 16000
  // throughout): the sample rate of every wave; the others are converted on the GPU (pk_mi355_recognizer_process_rates)
  Status Process(const pk_vector_t *waves, int n, std::vector<Utterance> *out, const int *rates = nullptr) {
    const int rc = rates ? pk_mi355_recognizer_process_rates(r_, waves, rates, n) : pk_mi355_recognizer_process(r_, waves, n);
    return Collect(rc, n, out);
  }
  // The same from features: feats[u] is utterance u's [T][feat_dim] matrix (nrow = feat_dim, ncol = T), kind
  // PK_MI355_FEATS_RAW (40-dim log-mel fbank, the CMVN is applied) or PK_MI355_FEATS_NORMALIZED
  Status ProcessFeatures(const pk_matrix_t *feats, int n, int kind, std::vector<Utterance> *out) {
    return Collect(pk_mi355_recognizer_process_features(r_, feats, n, kind), n, out);
  }
  // The owned objects: beam, trace gc, softmax mode, calibration and the result getters are their entries
  pk_mi355_am_t *am() const { return pk_mi355_recognizer_am(r_); }
  pk_mi355_batch_t *batch() const { return pk_mi355_recognizer_batch(r_); }
  pk_mi355_decoder_t *decoder() const { return pk_mi355_recognizer_decoder(r_); }
  const pk_mi355_symtab_t *symbols() const { return pk_mi355_recognizer_symtab(r_); }
  pk_mi355_recognizer_t *handle() const { return r_; }

 private:
  Status Collect(int rc, int n, std::vector<Utterance> *out) {
    if (rc != 0) return Status::FromLast(rc);
    if (out) {
      out->clear();
      for (int u = 0; u < n; ++u) {
        const char *hyp = pk_mi355_recognizer_hyp(r_, u);
        out->push_back(Utterance{hyp ? hyp : "", pk_mi355_recognizer_loglikelihood_per_frame(r_, u)});
      }
    }
    return Status();
  }
  pk_mi355_recognizer_t *r_;
};

// Online scoring of live streams (pk_mi355_stream_*): PCM pushed per slot in chunks; every
// Step() scores the frames that became final since the last one, bit for bit what the whole wave gives.  A slot may
// take features instead (OpenFeatures / PushFeatures): the rows are then the batch scorer's on
// the whole feature matrix.
class OnlineScorer {
 public:
  enum FeaturesOnlyTag { kFeaturesOnly };
  OnlineScorer(pk_mi355_am_t *am, const float *global_stats41, int max_streams, int64_t max_step_samples)
      : s_(pk_mi355_stream_create(am, global_stats41, max_streams, max_step_samples)) {
    if (!s_) status_ = Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // The front-end at a spec of the model's feature dimension (a FrontendSpec; pk_mi355_frontend_stream_create, DESIGN.md
  // section 18): stats_len = that + 1.  Audio slots at any rate and feature slots of both kinds, as on the object above.
  OnlineScorer(pk_mi355_am_t *am, const pk_mi355_frontend_spec_t &spec, const float *global_stats, int stats_len, int max_streams,
               int64_t max_step_samples)
      : s_(pk_mi355_frontend_stream_create(am, &spec, global_stats, stats_len, max_streams, max_step_samples)) {
    if (!s_) status_ = Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // Without a front-end (pk_mi355_features_stream_create): a model of any feature dimension, feature slots only,
  // capacity in frames.  global_stats41 may be null; given (40-dim models) it enables PK_MI355_FEATS_RAW.
  OnlineScorer(FeaturesOnlyTag, pk_mi355_am_t *am, const float *global_stats41, int max_streams, int64_t max_step_frames)
      : s_(pk_mi355_features_stream_create(am, global_stats41, max_streams, max_step_frames)) {
    if (!s_) status_ = Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // The same with statistics at the model's own dimension (pk_mi355_features_stream_create_stats, DESIGN.md section
  // 15): global_stats holds feat_dim sums, then the count, stats_len = feat_dim + 1; RAW slots at any dimension.
  OnlineScorer(FeaturesOnlyTag, pk_mi355_am_t *am, const float *global_stats, int stats_len, int max_streams, int64_t max_step_frames)
      : s_(pk_mi355_features_stream_create_stats(am, global_stats, stats_len, max_streams, max_step_frames)) {
    if (!s_) status_ = Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // Deltas behind the normalisation (a DeltaSpec; pk_mi355_deltas_stream_create): a model of
  // (order + 1) x the front-end's dimension; the front-end, the statistics (stats_len = BaseDim() + 1), the normalisation
  // and RAW slots are at BaseDim().  A live slot looks order * window + R frames ahead.
  OnlineScorer(pk_mi355_am_t *am, const pk_mi355_frontend_spec_t &spec, const pk_mi355_deltas_spec_t &deltas, const float *global_stats,
               int stats_len, int max_streams, int64_t max_step_samples)
      : s_(pk_mi355_deltas_stream_create(am, &deltas, &spec, global_stats, stats_len, max_streams, max_step_samples)) {
    if (!s_) status_ = Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // The same without a front-end: feature slots only, capacity in frames; global_stats (BaseDim() sums, then the count) may
  // be null.
  OnlineScorer(FeaturesOnlyTag, pk_mi355_am_t *am, const pk_mi355_deltas_spec_t &deltas, const float *global_stats, int stats_len,
               int max_streams, int64_t max_step_frames)
      : s_(pk_mi355_deltas_stream_create(am, &deltas, nullptr, global_stats, stats_len, max_streams, max_step_frames)) {
    if (!s_) status_ = Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // A transform in front of the splice, behind the deltas when `deltas` is not null (a pk_mi355_transform_spec_t;
  // pk_mi355_transform_stream_create): a model of the transform's output dimension; the front-end, the
  // statistics (stats_len = BaseDim() + 1), the normalisation and RAW slots are at BaseDim() = InDim() / (order + 1).  A live
  // slot looks order * window + right_context + R frames ahead.
  OnlineScorer(pk_mi355_am_t *am, const pk_mi355_frontend_spec_t &spec, const pk_mi355_deltas_spec_t *deltas,
               const pk_mi355_transform_spec_t &transform, const float *global_stats, int stats_len, int max_streams, int64_t max_step_samples)
      : s_(pk_mi355_transform_stream_create(am, &transform, deltas, &spec, global_stats, stats_len, max_streams, max_step_samples)) {
    if (!s_) status_ = Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // The same without a front-end: feature slots only, capacity in frames; global_stats (BaseDim() sums, then the count) may
  // be null.
  OnlineScorer(FeaturesOnlyTag, pk_mi355_am_t *am, const pk_mi355_deltas_spec_t *deltas, const pk_mi355_transform_spec_t &transform,
               const float *global_stats, int stats_len, int max_streams, int64_t max_step_frames)
      : s_(pk_mi355_transform_stream_create(am, &transform, deltas, nullptr, global_stats, stats_len, max_streams, max_step_frames)) {
    if (!s_) status_ = Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  ~OnlineScorer() { pk_mi355_stream_destroy(s_); }
  OnlineScorer(const OnlineScorer &) = delete;
  OnlineScorer &operator=(const OnlineScorer &) = delete;

  Status Open(int slot) { return Status::FromLast(pk_mi355_stream_open(s_, slot)); }
  // The slot's pushes are samples at `rate` Hz (8 .. 96 kHz), converted on the GPU step by step
  Status Open(int slot, int rate) { return Status::FromLast(pk_mi355_stream_open_rate(s_, slot, rate)); }
  int Rate(int slot) const { return pk_mi355_stream_rate(s_, slot); }
  Status Push(int slot, const float *samples, int num_samples) {
    return Status::FromLast(pk_mi355_stream_push(s_, slot, samples, num_samples));
  }
  Status PushI16(int slot, const int16_t *samples, int num_samples) {
    return Status::FromLast(pk_mi355_stream_push_i16(s_, slot, samples, num_samples));
  }
  // The slot takes features of `kind` (PK_MI355_FEATS_NORMALIZED or PK_MI355_FEATS_RAW): frames of FeatDim() floats
  Status OpenFeatures(int slot, int kind = PK_MI355_FEATS_NORMALIZED) {
    return Status::FromLast(pk_mi355_stream_open_features(s_, slot, kind));
  }
  Status PushFeatures(int slot, const float *frames, int num_frames) {
    return Status::FromLast(pk_mi355_stream_push_features(s_, slot, frames, num_frames));
  }
  int FeatDim() const { return pk_mi355_stream_feat_dim(s_); }
  // the dimension in front of the deltas (the front-end's, the statistics', a RAW slot's frames); FeatDim() on a scorer without deltas
  int BaseDim() const { return pk_mi355_stream_base_dim(s_); }
  // the width of the rows the transform reads; FeatDim() on a scorer without a transform
  int InDim() const { return pk_mi355_stream_in_dim(s_); }
  // A scorer with a transform: the open slot's own [FeatDim()][cols] matrix, cols = FeatDim() (linear) or FeatDim() + 1
  // (affine), before its first transform frame is computed; it lasts until the slot is opened again.
  Status SetSlotTransform(int slot, const float *matrix, int cols) {
    return Status::FromLast(pk_mi355_stream_transform_set_slot(s_, slot, matrix, pk_mi355_stream_feat_dim(s_), cols));
  }
  // -1: audio, else the PK_MI355_FEATS_* kind the slot was last opened with
  int SlotKind(int slot) const { return pk_mi355_stream_slot_kind(s_, slot); }
  // The normalisation of the audio and RAW slots, while no slot is in use: a NormSpec of mode sliding,
  // none or speaker, or an OnlineCmvnSpec with its global statistics (2 x (BaseDim() + 1) doubles; null with global_frames = 0).
  Status SetNorm(const pk_mi355_norm_spec_t &spec) { return Status::FromLast(pk_mi355_stream_norm_set(s_, &spec)); }
  Status SetNorm(const pk_mi355_online_cmvn_spec_t &spec, const double *global_stats) {
    return Status::FromLast(pk_mi355_stream_norm_set_online_cmvn(s_, &spec, global_stats));
  }
  // the speaker's 2 x (BaseDim() + 1) record of an open slot, before its first frame is computed
  Status SetSpeakerStats(int slot, const double *stats) { return Status::FromLast(pk_mi355_stream_norm_set_speaker_stats(s_, slot, stats)); }
  // the 2 x (BaseDim() + 1) record of all frames of the slot since it was opened
  Status NormStats(int slot, std::vector<double> *out) {
    out->assign(2 * (static_cast<size_t>(pk_mi355_stream_base_dim(s_)) + 1), 0.0);
    return Status::FromLast(pk_mi355_stream_norm_fetch_stats(s_, slot, out->data()));
  }
  Status Close(int slot) { return Status::FromLast(pk_mi355_stream_close(s_, slot)); }
  // Synchronous: the rows are ready on return.
  Status Step(float prob_scale) { return Status::FromLast(pk_mi355_stream_step(s_, prob_scale, 1)); }
  // The rows the last Step() scored for slot, as a host decodable ({ncol = count, nrow = num_pdfs}; release with
  // pk_decodable_destroy) and the global index of its first frame.
  Status Fetch(int slot, pk_decodable_t *out, int *first_frame) {
    return Status::FromLast(pk_mi355_stream_fetch(s_, slot, out, first_frame));
  }

  const Status &last_status() const { return status_; }
  pk_mi355_stream_t *handle() const { return s_; }

 private:
  pk_mi355_stream_t *s_;
  Status status_;
};

// A front-end specification (pk_mi355_frontend_spec_t): log-mel fbank with any number of bins
// over any band, or MFCC on top of it.  The defaults are the reference's front-end; Kaldi's usual MFCC is
// FrontendSpec::Mfcc(23, 13).  Nothing is checked here: the library refuses a bad spec wherever one is used.
struct FrontendSpec : pk_mi355_frontend_spec_t {
  FrontendSpec() { pk_mi355_frontend_default(this); }
  static FrontendSpec Fbank(int num_mel_bins, int window = PK_MI355_WINDOW_POVEY, float low_freq = 20.0f, float high_freq = 0.0f) {
    FrontendSpec s;
    s.num_mel_bins = num_mel_bins; s.window = window; s.low_freq = low_freq; s.high_freq = high_freq;
    return s;
  }
  static FrontendSpec Mfcc(int num_mel_bins, int num_ceps, int window = PK_MI355_WINDOW_POVEY, float low_freq = 20.0f,
                           float high_freq = 0.0f, float cepstral_lifter = 22.0f) {
    FrontendSpec s = Fbank(num_mel_bins, window, low_freq, high_freq);
    s.kind = PK_MI355_FRONTEND_MFCC; s.num_ceps = num_ceps; s.cepstral_lifter = cepstral_lifter;
    return s;
  }
  Status Check() const { return Status::FromLast(pk_mi355_frontend_check(this)); }
  int dim() const { return pk_mi355_frontend_dim(this); }      // negative: the spec is refused
};

// Fbank at a spec: wave (16 kHz sample values) -> features {nrow = spec.dim(), ncol = T}, resized like Fbank::Compute's.
class Frontend {
 public:
  explicit Frontend(const FrontendSpec &spec) : spec_(spec) {}
  void Compute(const pk_vector_t *wave, pk_matrix_t *features) {
    status_ = Status::FromLast(pk_mi355_frontend_compute(&spec_, wave, features));
  }
  const FrontendSpec &spec() const { return spec_; }
  const Status &last_status() const { return status_; }

 private:
  FrontendSpec spec_;
  Status status_;
};

// A normalisation specification (pk_mi355_norm_spec_t): the sliding rule (the default), none, or
// Kaldi's apply-cmvn per utterance or per speaker, with or without variance.  Nothing is checked here: the library
// refuses a bad spec wherever one is used.
struct NormSpec : pk_mi355_norm_spec_t {
  NormSpec() { mode = PK_MI355_NORM_SLIDING; norm_means = 1; norm_vars = 0; }
  static NormSpec None() { NormSpec s; s.mode = PK_MI355_NORM_NONE; return s; }
  static NormSpec Utterance(bool means = true, bool vars = false) { return Make(PK_MI355_NORM_UTTERANCE, means, vars); }
  static NormSpec Speaker(bool means = true, bool vars = false) { return Make(PK_MI355_NORM_SPEAKER, means, vars); }
  Status Check() const { return Status::FromLast(pk_mi355_norm_check(this)); }

 private:
  static NormSpec Make(int mode, bool means, bool vars) {
    NormSpec s;
    s.mode = mode; s.norm_means = means ? 1 : 0; s.norm_vars = vars ? 1 : 0;
    return s;
  }
};

// Online CMVN (pk_mi355_online_cmvn_spec_t): Kaldi's OnlineCmvn at its defaults.  Nothing is
// checked here: the library refuses a bad spec wherever one is used.
struct OnlineCmvnSpec : pk_mi355_online_cmvn_spec_t {
  explicit OnlineCmvnSpec(int window = 600, int spk_frames = 600, int glob_frames = 200, bool vars = false) {
    cmn_window = window; speaker_frames = spk_frames; global_frames = glob_frames; norm_vars = vars ? 1 : 0;
  }
  // global_stats: 2 x (dim + 1) doubles, or null when global_frames is 0
  Status Check(const double *global_stats, int dim) const { return Status::FromLast(pk_mi355_online_cmvn_check(this, global_stats, dim)); }
};

// Delta features (pk_mi355_deltas_spec_t): Kaldi's add-deltas at its defaults.  Nothing is checked
// here: the library refuses a bad spec wherever one is used.
struct DeltaSpec : pk_mi355_deltas_spec_t {
  explicit DeltaSpec(int order_ = 2, int window_ = 2) { order = order_; window = window_; }
  Status Check() const { return Status::FromLast(pk_mi355_deltas_check(this)); }
  int dim(int base_dim) const { return pk_mi355_deltas_dim(this, base_dim); }      // negative: the spec or the dimension is refused
  // the rule on the host: x [T][base_dim] -> out [T][dim(base_dim)]
  Status Apply(const float *x, int num_frames, int base_dim, std::vector<float> *out) const {
    const int d = dim(base_dim);
    if (d < 0) return Status::FromLast(d);
    out->assign(static_cast<size_t>(num_frames > 0 ? num_frames : 0) * d, 0.0f);
    return Status::FromLast(pk_mi355_deltas_apply(this, x, num_frames, base_dim, out->data()));
  }
};

// A feature transform (pk_mi355_transform_spec_t): Kaldi's splice-feats | transform-feats.  The
// matrix [rows][cols], row-major, is copied; pass none (in_dim alone) for a scorer that takes per-utterance matrices
// only.  Nothing is checked here: the library refuses a bad spec wherever one is used.
struct TransformSpec : pk_mi355_transform_spec_t {
  TransformSpec(const float *m, int rows_, int cols_, int in_dim_, int left = 0, int right = 0) : keep_(m, m + static_cast<size_t>(rows_) * cols_) {
    left_context = left; right_context = right; in_dim = in_dim_; rows = rows_; cols = cols_; matrix = keep_.data();
  }
  explicit TransformSpec(int in_dim_) { left_context = right_context = 0; in_dim = in_dim_; rows = cols = 0; matrix = nullptr; }
  TransformSpec(const TransformSpec &o) : pk_mi355_transform_spec_t(o), keep_(o.keep_) { matrix = o.matrix ? keep_.data() : nullptr; }
  TransformSpec &operator=(const TransformSpec &) = delete;
  Status Check() const { return Status::FromLast(pk_mi355_transform_check(this)); }
  int out_dim() const { return pk_mi355_transform_out_dim(this); }      // negative: the spec is refused
  // the rule on the host: x [T][in_dim] -> out [T][out_dim()]
  Status Apply(const float *x, int num_frames, std::vector<float> *out) const {
    const int d = out_dim();
    if (d < 0) return Status::FromLast(d);
    out->assign(static_cast<size_t>(num_frames > 0 ? num_frames : 0) * d, 0.0f);
    return Status::FromLast(pk_mi355_transform_apply(this, x, num_frames, out->data()));
  }

 private:
  std::vector<float> keep_;
};

// The batched, device-resident scorer (pk_mi355_batch_*): PCM of many utterances -> log-likelihood rows.
class BatchScorer {
 public:
  // the reference's front-end: a 40-dim model and its 41 statistics
  BatchScorer(pk_mi355_am_t *am, const float *global_stats41, int max_utts, int64_t max_total_samples)
      : b_(pk_mi355_batch_create(am, global_stats41, max_utts, max_total_samples)) {
    if (!b_) status_ = Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // a front-end at a spec of the model's feature dimension (pk_mi355_frontend_batch_create): stats_len = that + 1
  BatchScorer(pk_mi355_am_t *am, const FrontendSpec &spec, const float *global_stats, int stats_len, int max_utts,
              int64_t max_total_samples)
      : b_(pk_mi355_frontend_batch_create(am, &spec, global_stats, stats_len, max_utts, max_total_samples)) {
    if (!b_) status_ = Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // deltas behind the normalisation (pk_mi355_deltas_batch_create): a model of deltas.dim(spec.dim()) features, the
  // front-end, the statistics (stats_len = spec.dim() + 1) and the normalisation at BaseDim() = spec.dim()
  BatchScorer(pk_mi355_am_t *am, const FrontendSpec &spec, const DeltaSpec &deltas, const float *global_stats, int stats_len, int max_utts,
              int64_t max_total_samples)
      : b_(pk_mi355_deltas_batch_create(am, &deltas, &spec, global_stats, stats_len, max_utts, max_total_samples)) {
    if (!b_) status_ = Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // a transform in front of the splice, behind the deltas when `deltas` is not null (pk_mi355_transform_batch_create): a
  // model of transform.out_dim() features; the front-end, the statistics (stats_len = spec.dim() + 1) and the
  // normalisation at BaseDim() = spec.dim()
  BatchScorer(pk_mi355_am_t *am, const FrontendSpec &spec, const DeltaSpec *deltas, const TransformSpec &transform, const float *global_stats,
              int stats_len, int max_utts, int64_t max_total_samples)
      : b_(pk_mi355_transform_batch_create(am, &transform, deltas, &spec, global_stats, stats_len, max_utts, max_total_samples)) {
    if (!b_) status_ = Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  ~BatchScorer() { pk_mi355_batch_destroy(b_); }
  BatchScorer(const BatchScorer &) = delete;
  BatchScorer &operator=(const BatchScorer &) = delete;

  Status SetWaves(const pk_vector_t *waves, int num_utts) { return Status::FromLast(pk_mi355_batch_set_waves(b_, waves, num_utts)); }
  // utterance u sampled at rates[u] Hz, converted on the GPU on the way in
  Status SetWaves(const pk_vector_t *waves, const int *rates, int num_utts) {
    return Status::FromLast(pk_mi355_resample_set_waves(b_, waves, rates, num_utts));
  }
  Status Score(float prob_scale) { return Status::FromLast(pk_mi355_batch_score(b_, prob_scale, 1)); }
  int NumFrames(int utt) const { return pk_mi355_batch_num_frames(b_, utt); }
  int FeatDim() const { return pk_mi355_features_dim(b_); }
  // the dimension in front of the deltas (the front-end's, the statistics'); FeatDim() on a scorer without deltas
  int BaseDim() const { return pk_mi355_deltas_base_dim(b_); }
  // the width of the rows the transform reads; FeatDim() on a scorer without one
  int InDim() const { return pk_mi355_transform_in_dim(b_); }
  // a scorer with a transform: [num_utts][FeatDim()][cols] floats, cols = FeatDim() or FeatDim() + 1 (the offset last),
  // applied behind the global matrix and consumed by the next Score
  Status SetUttTransforms(const float *mats, int cols, int num_utts) {
    return Status::FromLast(pk_mi355_transform_set_utt(b_, mats, FeatDim(), cols, num_utts));
  }
  // utterance utt's rows as a host decodable ({ncol = T, nrow = num_pdfs}; release with pk_decodable_destroy)
  Status Fetch(int utt, pk_decodable_t *out) { return Status::FromLast(pk_mi355_batch_fetch(b_, utt, out)); }
  // the front-end's rows, [T][BaseDim()] floats
  Status FetchFeatures(int utt, float *out) { return Status::FromLast(pk_mi355_batch_fetch_fbank(b_, utt, out)); }
  // what the first layer reads, [T][FeatDim()] floats
  Status FetchNormalized(int utt, float *out) { return Status::FromLast(pk_mi355_batch_fetch_cmvn(b_, utt, out)); }
  // The normalisation between the front-end and the first layer; it holds until it is set again.
  Status SetNorm(const NormSpec &spec) { return Status::FromLast(pk_mi355_norm_set(b_, &spec)); }
  // Online CMVN instead; global_stats: 2 x (BaseDim() + 1) doubles, or null with global_frames = 0.
  Status SetNorm(const OnlineCmvnSpec &spec, const double *global_stats) {
    return Status::FromLast(pk_mi355_norm_set_online_cmvn(b_, &spec, global_stats));
  }
  // mode speaker (required) and online CMVN (optional): [num_utts][2][BaseDim() + 1] doubles, consumed by the next Score
  Status SetSpeakerStats(const double *stats, int num_utts) { return Status::FromLast(pk_mi355_norm_set_speaker_stats(b_, stats, num_utts)); }
  // the 2 x (BaseDim() + 1) record the last Score computed for utterance utt in mode utterance
  Status NormStats(int utt, std::vector<double> *out) {
    out->assign(2 * (static_cast<size_t>(BaseDim()) + 1), 0.0);
    return Status::FromLast(pk_mi355_norm_fetch_stats(b_, utt, out->data()));
  }

  const Status &last_status() const { return status_; }
  pk_mi355_batch_t *handle() const { return b_; }

 private:
  pk_mi355_batch_t *b_;
  Status status_;
};

// Kaldi archives and script files of float matrices (pk_mi355_ark_*), entry by entry:
//   ArkReader r("scp:feats.scp");  while (r.Next()) use(r.Key(), r.Matrix());  if (!r.last_status().ok()) ...
class ArkReader {
 public:
  // spec: "ark:<path>", "scp:<path>" or a bare path (a ".scp" suffix means a script file)
  explicit ArkReader(const std::string &spec) : h_(pk_mi355_ark_open(spec.c_str())) {
    if (!h_) status_ = Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  ~ArkReader() { pk_mi355_ark_close(h_); }
  ArkReader(const ArkReader &) = delete;
  ArkReader &operator=(const ArkReader &) = delete;

  // True: there is a current entry.  False: the end, or an error (last_status() tells which).
  bool Next() {
    if (!h_) return false;
    const int rc = pk_mi355_ark_next(h_);
    if (rc < 0) status_ = Status::FromLast(rc);
    return rc == 1;
  }
  std::string Key() const { return pk_mi355_ark_key(h_); }
  // {nrow = the feature dimension, ncol = frames}, memory [frames][dim]; valid until the next call on this reader
  pk_matrix_t Matrix() const {
    pk_matrix_t m = {0, 0, nullptr};
    if (h_) pk_mi355_ark_matrix(h_, &m);
    return m;
  }
  // One keyless object ("path" or "path:offset": a global CMVN statistics file, say), row-major into *values
  static Status ReadObject(const std::string &rxfilename, std::vector<float> *values, int *rows, int *cols) {
    pk_mi355_ark_t *h = pk_mi355_ark_read_object(rxfilename.c_str());
    if (!h) return Status(pk_mi355_last_error_code(), pk_mi355_last_error());
    pk_matrix_t m = {0, 0, nullptr};
    pk_mi355_ark_matrix(h, &m);
    values->assign(m.data, m.data + static_cast<size_t>(m.ncol) * m.nrow);
    *rows = m.ncol;
    *cols = m.nrow;
    pk_mi355_ark_close(h);
    return Status();
  }
  const Status &last_status() const { return status_; }

 private:
  pk_mi355_ark_t *h_;
  Status status_;
};

// The search of pk_process frame by frame across calls (pk_mi355_online_decoder_*): Advance() after every
// OnlineScorer::Step(), Partial() while the stream is live, Result() once its slot is finished.
class OnlineDecoder {
 public:
  OnlineDecoder(const Fst *fst, pk_mi355_am_t *am, int max_streams)
      : d_(pk_mi355_online_decoder_create(fst->handle(), am, max_streams, 0)) {
    if (!d_) status_ = Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  ~OnlineDecoder() { pk_mi355_online_decoder_destroy(d_); }
  OnlineDecoder(const OnlineDecoder &) = delete;
  OnlineDecoder &operator=(const OnlineDecoder &) = delete;

  Status Open(int slot) { return Status::FromLast(pk_mi355_online_decoder_open(d_, slot)); }
  Status Advance(OnlineScorer *scorer) { return Status::FromLast(pk_mi355_online_decoder_advance(d_, scorer->handle(), 1)); }
  // words in spoken order
  std::vector<int> Partial(int slot, float *cost) const {
    const int n = pk_mi355_online_decoder_partial(d_, slot, nullptr, 0, cost);
    std::vector<int> w(n > 0 ? n : 0);
    if (n > 0) pk_mi355_online_decoder_partial(d_, slot, w.data(), n, cost);
    return w;
  }
  std::vector<int> Result(int slot, float *weight, int *ok) const {
    const int n = pk_mi355_online_decoder_result(d_, slot, nullptr, 0, weight, ok);
    std::vector<int> w(n > 0 ? n : 0);
    if (n > 0) pk_mi355_online_decoder_result(d_, slot, w.data(), n, weight, ok);
    return w;
  }
  // While no slot is open: every trace record also keeps its arc's acoustic cost (pk_mi355_online_decoder_set_alignment)
  Status SetAlignment(bool on) { return Status::FromLast(pk_mi355_online_decoder_set_alignment(d_, on ? 1 : 0)); }
  // Per frame of the slot's current path (partial while live): the emitting arc, its transition-id and its acoustic
  // cost (any pointer may be null).  Returns the frames aligned, or a negative code (alignment off: PK_MI355_E_STATE).
  int Alignment(int slot, std::vector<int32_t> *arc_ids, std::vector<int32_t> *trans_ids, std::vector<float> *acoustic_cost) const {
    const int n = pk_mi355_online_decoder_alignment(d_, slot, nullptr, nullptr, nullptr, 0);
    if (n < 0) return n;
    if (arc_ids) arc_ids->resize(n);
    if (trans_ids) trans_ids->resize(n);
    if (acoustic_cost) acoustic_cost->resize(n);
    return pk_mi355_online_decoder_alignment(d_, slot, arc_ids ? arc_ids->data() : nullptr, trans_ids ? trans_ids->data() : nullptr,
                                             acoustic_cost ? acoustic_cost->data() : nullptr, n);
  }
  // The frames the slot has decoded
  int NumFrames(int slot) const { return pk_mi355_online_decoder_num_frames(d_, slot); }
  // The word segments of the slot's current path (acoustic_cost is NaN with alignment off)
  std::vector<pk_mi355_word_t> WordSegments(int slot) const {
    const int n = pk_mi355_online_decoder_word_segments(d_, slot, nullptr, 0);
    std::vector<pk_mi355_word_t> out(n > 0 ? n : 0);
    if (n > 0) pk_mi355_online_decoder_word_segments(d_, slot, out.data(), n);
    return out;
  }
  // While no slot is open: the arcs all of a slot's tokens share leave the device for a host list at the end of every
  // launch, so a stream may be longer than the arena (pk_mi355_online_decoder_set_commit).  No result changes.
  Status SetCommit(bool on) { return Status::FromLast(pk_mi355_online_decoder_set_commit(d_, on ? 1 : 0)); }
  // The words of the committed prefix of the slot's path; its arcs and emitting arcs (either pointer may be null)
  std::vector<int> Committed(int slot, int *num_arcs, int *num_frames) const {
    const int n = pk_mi355_online_decoder_committed(d_, slot, nullptr, 0, num_arcs, num_frames);
    std::vector<int> w(n > 0 ? n : 0);
    if (n > 0) pk_mi355_online_decoder_committed(d_, slot, w.data(), n, num_arcs, num_frames);
    return w;
  }
  // The slot's backtrace arena: records in use after its last launch, the most since Open(), the capacity
  Status TraceStats(int slot, int64_t *in_use, int64_t *peak, int64_t *capacity) const {
    return Status::FromLast(pk_mi355_online_decoder_trace_stats(d_, slot, in_use, peak, capacity));
  }
  // While no slot is open: after every advance each slot gets an endpoint record -- the silence (frames whose pdf is in
  // silence_pdfs) that ends its best partial path, and its best final token's cost relative to its best token's -- on
  // which `rules` are tried (pk_mi355_online_decoder_set_endpointing).  No rules: off.
  Status SetEndpointing(const std::vector<int32_t> &silence_pdfs, const std::vector<pk_mi355_endpoint_rule_t> &rules) {
    return Status::FromLast(pk_mi355_online_decoder_set_endpointing(d_, silence_pdfs.data(), static_cast<int>(silence_pdfs.size()),
                                                                    rules.data(), static_cast<int>(rules.size())));
  }
  static std::vector<pk_mi355_endpoint_rule_t> DefaultEndpointRules() {
    std::vector<pk_mi355_endpoint_rule_t> rules(pk_mi355_endpoint_default_rules(nullptr, 0));
    pk_mi355_endpoint_default_rules(rules.data(), static_cast<int>(rules.size()));
    return rules;
  }
  // The slot's record after its last advance (out may be null).  Returns 1 + the first rule that fires, 0 for none, or
  // a negative code (the mode is off: PK_MI355_E_STATE).
  int Endpoint(int slot, pk_mi355_endpoint_t *out) const { return pk_mi355_online_decoder_endpoint(d_, slot, out); }
  // End the open slots now, with no new frame: Result() is then BestPath over the frames decoded so far, and the slots
  // can be opened again.
  Status Finish(const std::vector<int> &slots) {
    return Status::FromLast(pk_mi355_online_decoder_finish(d_, slots.data(), static_cast<int>(slots.size()), 1));
  }
  const Status &last_status() const { return status_; }
  pk_mi355_online_decoder_t *handle() const { return d_; }

 private:
  pk_mi355_online_decoder_t *d_;
  Status status_;
};

// pk_load + a live pk_process (pk_mi355_online_recognizer_*): PCM pushed per slot in chunks, Step() after every round
// of pushes, Partial() while a slot is live; Close(), one more Step(), then Result().
class OnlineRecognizer {
 public:
  OnlineRecognizer() : r_(nullptr) {}
  ~OnlineRecognizer() { pk_mi355_online_recognizer_destroy(r_); }
  OnlineRecognizer(const OnlineRecognizer &) = delete;
  OnlineRecognizer &operator=(const OnlineRecognizer &) = delete;

  Status Load(const std::string &model_file, int max_streams = 1, int64_t max_step_samples = 16000 * 8,
              int64_t trace_capacity = 0) {
    pk_mi355_online_recognizer_destroy(r_);
    r_ = pk_mi355_online_recognizer_load(model_file.c_str(), max_streams, max_step_samples, trace_capacity);
    return r_ ? Status() : Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // A model of the spec's feature dimension (a FrontendSpec; pk_mi355_frontend_online_recognizer_load)
  Status Load(const std::string &model_file, const pk_mi355_frontend_spec_t &spec, int max_streams = 1,
              int64_t max_step_samples = 16000 * 8, int64_t trace_capacity = 0) {
    pk_mi355_online_recognizer_destroy(r_);
    r_ = pk_mi355_frontend_online_recognizer_load(model_file.c_str(), &spec, max_streams, max_step_samples, trace_capacity);
    return r_ ? Status() : Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // A model of (order + 1) x the spec's feature dimension, deltas behind the normalisation (a FrontendSpec and a
  // DeltaSpec; pk_mi355_deltas_online_recognizer_load)
  Status Load(const std::string &model_file, const pk_mi355_frontend_spec_t &spec, const pk_mi355_deltas_spec_t &deltas, int max_streams = 1,
              int64_t max_step_samples = 16000 * 8, int64_t trace_capacity = 0) {
    pk_mi355_online_recognizer_destroy(r_);
    r_ = pk_mi355_deltas_online_recognizer_load(model_file.c_str(), &spec, &deltas, max_streams, max_step_samples, trace_capacity);
    return r_ ? Status() : Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  // A model of the transform's output dimension, the transform behind the normalisation and (deltas not null) the deltas
  // (pk_mi355_transform_online_recognizer_load).  A slot's own matrix:
  // pk_mi355_stream_transform_set_slot on stream() once the slot is open.
  Status Load(const std::string &model_file, const pk_mi355_frontend_spec_t &spec, const pk_mi355_deltas_spec_t *deltas,
              const pk_mi355_transform_spec_t &transform, int max_streams = 1, int64_t max_step_samples = 16000 * 8, int64_t trace_capacity = 0) {
    pk_mi355_online_recognizer_destroy(r_);
    r_ = pk_mi355_transform_online_recognizer_load(model_file.c_str(), &spec, deltas, &transform, max_streams, max_step_samples, trace_capacity);
    return r_ ? Status() : Status(pk_mi355_last_error_code(), pk_mi355_last_error());
  }
  Status Open(int slot) { return Status::FromLast(pk_mi355_online_recognizer_open(r_, slot)); }
  Status Open(int slot, int rate) { return Status::FromLast(pk_mi355_online_recognizer_open_rate(r_, slot, rate)); }
  Status Push(int slot, const float *samples, int num_samples) {
    return Status::FromLast(pk_mi355_online_recognizer_push(r_, slot, samples, num_samples));
  }
  Status PushI16(int slot, const int16_t *samples, int num_samples) {
    return Status::FromLast(pk_mi355_online_recognizer_push_i16(r_, slot, samples, num_samples));
  }
  // The slot takes 40-dim features instead of audio (raw log-mel fbank by default), [num_frames][40] per push
  Status OpenFeatures(int slot, int kind = PK_MI355_FEATS_RAW) {
    return Status::FromLast(pk_mi355_online_recognizer_open_features(r_, slot, kind));
  }
  Status PushFeatures(int slot, const float *frames, int num_frames) {
    return Status::FromLast(pk_mi355_online_recognizer_push_features(r_, slot, frames, num_frames));
  }
  Status Close(int slot) { return Status::FromLast(pk_mi355_online_recognizer_close(r_, slot)); }
  Status Step() { return Status::FromLast(pk_mi355_online_recognizer_step(r_)); }
  // The slot's current hypothesis as text ("" on misuse); valid until the next Step()
  std::string Partial(int slot) const {
    const char *text = pk_mi355_online_recognizer_partial(r_, slot);
    return text ? text : "";
  }
  // The words of Partial(slot) that are final now ("" unless pk_mi355_online_decoder_set_commit(decoder(), 1) was called)
  std::string Stable(int slot) const {
    const char *text = pk_mi355_online_recognizer_stable(r_, slot);
    return text ? text : "";
  }
  bool Finished(int slot) const { return pk_mi355_online_recognizer_finished(r_, slot) == 1; }
  // A finished slot's hyp and loglikelihood_per_frame; PK_MI355_E_STATE before that
  Status Result(int slot, Recognizer::Utterance *out) const {
    const char *hyp = pk_mi355_online_recognizer_hyp(r_, slot);
    if (!hyp) return Status(pk_mi355_last_error_code(), pk_mi355_last_error());
    if (out) *out = Recognizer::Utterance{hyp, pk_mi355_online_recognizer_loglikelihood_per_frame(r_, slot)};
    return Status();
  }
  // While no slot is open: every Step() ends the utterance of each live slot whose endpoint rule fired and starts the next
  // one at the scorer's next row (pk_mi355_online_recognizer_set_endpointing).  No rules: off.
  Status SetEndpointing(const std::vector<int32_t> &silence_pdfs, const std::vector<pk_mi355_endpoint_rule_t> &rules) {
    return Status::FromLast(pk_mi355_online_recognizer_set_endpointing(r_, silence_pdfs.data(), static_cast<int>(silence_pdfs.size()),
                                                                       rules.data(), static_cast<int>(rules.size())));
  }
  // One utterance of a slot's stream: frames [first_frame, first_frame + num_frames), rule = 1 + the rule that ended it
  // (0: the stream's end); segment frames are relative to first_frame
  struct Piece {
    pk_mi355_utterance_t info;
    std::string hyp;
    std::vector<int> words;
    std::vector<pk_mi355_word_t> segments;
  };
  // The utterances since Open(slot), in order; the last one (rule 0) is there once the slot is finished
  std::vector<Piece> Utterances(int slot) const {
    const int n = pk_mi355_online_recognizer_num_utterances(r_, slot);
    std::vector<Piece> out(n > 0 ? n : 0);
    for (int i = 0; i < n; ++i) {
      Piece &p = out[i];
      if (pk_mi355_online_recognizer_utterance(r_, slot, i, &p.info) != 0) continue;
      const char *hyp = pk_mi355_online_recognizer_utterance_hyp(r_, slot, i);
      p.hyp = hyp ? hyp : "";
      p.words.resize(p.info.num_words);
      p.segments.resize(p.info.num_word_segments);
      if (!p.words.empty()) pk_mi355_online_recognizer_utterance_words(r_, slot, i, p.words.data(), p.info.num_words);
      if (!p.segments.empty())
        pk_mi355_online_recognizer_utterance_word_segments(r_, slot, i, p.segments.data(), p.info.num_word_segments);
    }
    return out;
  }
  // The owned objects: beam, softmax mode and the other result getters (words, alignment, word segments) are their entries
  pk_mi355_am_t *am() const { return pk_mi355_online_recognizer_am(r_); }
  pk_mi355_stream_t *stream() const { return pk_mi355_online_recognizer_stream(r_); }
  pk_mi355_online_decoder_t *decoder() const { return pk_mi355_online_recognizer_decoder(r_); }
  const pk_mi355_symtab_t *symbols() const { return pk_mi355_online_recognizer_symtab(r_); }
  pk_mi355_online_recognizer_t *handle() const { return r_; }

 private:
  pk_mi355_online_recognizer_t *r_;
};

// Utterance sharding for N GPUs (one process per GPU, a full weight replica each, no data-path collective): which rank
// scores which utterance of a list.  The reference scores a ragged list one WAV after another (src/main.cc:34-46, every
// length from src/fbank.cc:35-42); balancing by FRAMES -- longest first, each utterance to the rank with the fewest
// frames so far, ties to the lower rank -- keeps the slowest rank within a fraction of a percent of the mean where
// `u mod N` leaves several percent.  A pure function of the frame counts: every rank computes the same map without
// talking.  (The Python twin is pocketkaldi_amd.dist.partition_by_frames.)
inline std::vector<std::vector<int> > PartitionByFrames(const std::vector<int> &frames, int world) {
  std::vector<int> order(frames.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = static_cast<int>(i);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return frames[a] > frames[b]; });
  std::vector<long long> load(world > 0 ? world : 0, 0);
  std::vector<std::vector<int> > shards(load.size());
  for (size_t i = 0; i < order.size() && !load.empty(); ++i) {
    const int r = static_cast<int>(std::min_element(load.begin(), load.end()) - load.begin());   // (first minimum = lower rank)
    shards[r].push_back(order[i]);
    load[r] += frames[order[i]];
  }
  for (size_t r = 0; r < shards.size(); ++r) std::sort(shards[r].begin(), shards[r].end());
  return shards;
}

}  // namespace pocketkaldi

#endif  // POCKETKALDI_AMD_HPP_
