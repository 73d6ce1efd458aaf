// capi_decoder.hip -- the decoder core (pk_decode.h: what the batch and the online decoder share) and the batch
// decoder, pk_mi355_decoder_*: whole utterances, host log-likelihoods or a scored batch's rows on the device, in one
// call; optionally per-utterance backtrace slices with garbage collection and the best path's alignment.  The kernels
// are decode.hip's.
#include <algorithm>
#include <vector>

#include "pk_decode.h"

using namespace pkhost;

// ================================================================== decoder core

namespace {

template <typename T>
int Upload(T **dst, const std::vector<T> &src, size_t min_count = 1) {
  const size_t n = std::max(src.size(), min_count);
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(dst), sizeof(T) * n));
  if (!src.empty()) HIP_TRY(hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
  return 0;
}

}  // namespace

namespace pkhost {

int CheckCoreInputs(const pk_mi355_fst *f, const pk_mi355_am *am) {
  if (!f || !am) return Fail(PK_MI355_E_INVALID, "null graph or model");
  if (!am->finalized) return Fail(PK_MI355_E_STATE, "model not finalized");
  return 0;
}

int CreateCore(DecoderCore *c, const pk_mi355_fst *f, const pk_mi355_am *am, int max_utts, int64_t trace_cap) {
  c->device = am->device; c->am = am;
  const int S = f->num_states;
  const int N = am->num_pdfs;
  if (N <= 0 || N > kMaxDecPdfs) return Fail(PK_MI355_E_INVALID, "decoder: num_pdfs %d outside [1, %d]", N, kMaxDecPdfs);
  GraphSplit g;
  int rc = SplitGraph(*f, am->tid2pdf, N, &g);
  if (rc) return rc;
  c->max_utts = max_utts; c->num_states = S; c->start = f->start; c->num_pdfs = N;
  c->trace_cap = trace_cap;
  if (c->trace_cap > (int64_t)INT32_MAX) return Fail(PK_MI355_E_INVALID, "decoder: trace_capacity above 2^31 - 1");
  // a SplitArc is uploaded as the int4 the kernels read: x = next state, y = pdf, z = weight bits, w = original arc id
  static_assert(sizeof(SplitArc) == sizeof(int4) && offsetof(SplitArc, next) == offsetof(int4, x) &&
                offsetof(SplitArc, pdf) == offsetof(int4, y) && offsetof(SplitArc, weight_bits) == offsetof(int4, z) &&
                offsetof(SplitArc, arc) == offsetof(int4, w), "SplitArc is laid out as int4");
  static_assert(kMaxSplitArcs == kEpsBit - 1, "candidate ids: an arc's index, the top bit for epsilon arcs");
  SplitArc *e_arc = nullptr, *n_arc = nullptr;
  rc = Upload(&e_arc, g.e_arc);
  c->e_arc = reinterpret_cast<int4 *>(e_arc);
  if (!rc) rc = Upload(&n_arc, g.n_arc);
  c->n_arc = reinterpret_cast<int4 *>(n_arc);
  if (rc || (rc = Upload(&c->e_off, g.e_off)) || (rc = Upload(&c->n_off, g.n_off)) || (rc = Upload(&c->e_src, g.e_src)) ||
      (rc = Upload(&c->n_src, g.n_src)) || (rc = Upload(&c->final_w, f->final_w)))
    return rc;
  LabelsOf(*f, &c->labels);
  const size_t per = (size_t)S * max_utts;
  HIP_TRY(hipMalloc(&c->key, sizeof(uint64_t) * per));
  HIP_TRY(hipMemset(c->key, 0xFF, sizeof(uint64_t) * per));
  HIP_TRY(hipMalloc(&c->tr, sizeof(int) * per));
  HIP_TRY(hipMalloc(&c->mark, sizeof(int) * per));
  HIP_TRY(hipMemset(c->mark, 0, sizeof(int) * per));
  HIP_TRY(hipMalloc(&c->touched, sizeof(int) * per));
  HIP_TRY(hipMalloc(&c->nxt, sizeof(int) * per));
  HIP_TRY(hipMalloc(&c->lists, sizeof(Tok) * per * 4));
  HIP_TRY(hipMalloc(&c->rec, sizeof(int2) * (size_t)c->trace_cap));
  // The best paths of one call are disjoint chains of that call's trace records, so an arena of trace_capacity
  // entries always holds them all.
  HIP_TRY(hipMalloc(&c->path, sizeof(int) * (size_t)c->trace_cap));
  HIP_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&c->done, hipEventDisableTiming));
  return 0;
}

void FreeCore(DecoderCore *c) {
  hipFree(c->e_arc); hipFree(c->n_arc);
  hipFree(c->e_off); hipFree(c->n_off); hipFree(c->e_src); hipFree(c->n_src); hipFree(c->final_w);
  hipFree(c->key); hipFree(c->tr); hipFree(c->mark); hipFree(c->touched); hipFree(c->nxt); hipFree(c->lists);
  hipFree(c->rec); hipFree(c->path);
  hipFree(c->d_ll);                             // (UploadLoglik's)
  if (c->done) hipEventDestroy(c->done);
  if (c->own_stream) hipStreamDestroy(c->own_stream);
}

int SetBeam(DecoderCore *c, float beam, int max_active) {
  if (!(beam >= 0.0f) || max_active <= 0) return Fail(PK_MI355_E_INVALID, "beam must be >= 0 and max_active > 0");
  c->beam = beam;
  c->max_active = max_active;
  return 0;
}

DecArgs ArgsOf(const DecoderCore *c, const float *ll, int n) {
  DecArgs A = {};
  A.e_off = c->e_off; A.e_arc = c->e_arc; A.e_src = c->e_src;
  A.n_off = c->n_off; A.n_arc = c->n_arc; A.n_src = c->n_src;
  A.final_w = c->final_w;
  A.num_states = c->num_states; A.start = c->start; A.num_pdfs = c->num_pdfs;
  A.ll = ll; A.num_utts = n;
  const size_t per = (size_t)c->num_states * c->max_utts;
  A.key = c->key; A.tr = c->tr; A.mark = c->mark; A.touched = c->touched; A.nxt = c->nxt;
  A.la = c->lists; A.lb = c->lists + per; A.fa = c->lists + 2 * per; A.fb = c->lists + 3 * per;
  A.rec = c->rec; A.path = c->path;
  A.beam = c->beam; A.max_active = c->max_active;
  A.max_rounds = c->num_states + 2;    // Bellman-Ford bound: more rounds only under a negative epsilon cycle
  return A;
}

int CheckLoglik(const DecoderCore *c, const pk_matrix_t &m, const char *what, int i) {
  if (m.ncol < 0 || (m.ncol > 0 && (m.nrow != c->num_pdfs || !m.data)))
    return Fail(PK_MI355_E_INVALID, "%s %d: log_prob is {ncol %d, nrow %d}, nrow %d expected", what, i, m.ncol, m.nrow,
                c->num_pdfs);
  return 0;
}

int UploadLoglik(DecoderCore *c, const pk_decodable_t *src, int n) {
  int64_t total = 0;
  for (int i = 0; i < n; ++i) total += (int64_t)src[i].log_prob.ncol * c->num_pdfs;
  if ((size_t)total > c->d_ll_floats) {
    if (c->d_ll) hipFree(c->d_ll);
    c->d_ll = nullptr;
    c->d_ll_floats = 0;
    HIP_TRY(hipMalloc(&c->d_ll, sizeof(float) * (size_t)total));
    c->d_ll_floats = (size_t)total;
  }
  int64_t at = 0;
  for (int i = 0; i < n; ++i) {
    const pk_matrix_t &m = src[i].log_prob;
    const int64_t count = (int64_t)m.ncol * c->num_pdfs;
    if (count > 0)
      HIP_TRY(hipMemcpyAsync(c->d_ll + at, m.data, sizeof(float) * (size_t)count, hipMemcpyHostToDevice, c->own_stream));
    at += count;
  }
  return 0;
}
}  // namespace pkhost

// ================================================================== batch decoder

struct pk_mi355_decoder : DecoderCore {
  bool trace_gc = false;                        // set_trace_gc: how the next call uses the arena
  unsigned long long *counters = nullptr;       // [0] records used; [1] (as int) path entries used
  int path_cap = 0;
  UttResult *d_res = nullptr;
  int64_t *d_off = nullptr;
  int *d_T = nullptr;
  pk_mi355_batch_t *batch = nullptr;            // decode_batch: the scored batch (its range verdict)
  // results of the last call
  bool pending = false, have = false;
  int num_utts = 0;
  bool call_gc = false;                         // the last call: trace-gc mode, its slice (records per utterance),
  int64_t call_slice = 0, call_records = 0;     // and with the mode off the records it used in all
  std::vector<UttResult> res;
  std::vector<int32_t> h_path;
  std::vector<int> h_T;
  std::vector<int64_t> h_off;
  // alignment (set_alignment): the mode of the next call and of the last one; the device table and buffers, made at
  // the first enable (d_ali and d_ac: at the first call that needs them, Launch)
  bool alignment = false, call_align = false;
  int *d_arc_pdf = nullptr;
  int64_t *d_frame_off = nullptr;
  AlignResult *d_align = nullptr;
  int *d_ali = nullptr;
  float *d_ac = nullptr;
  size_t d_ali_frames = 0;
  std::vector<int64_t> h_frame_off;               // the last call's prefix sum of T (num_utts + 1 entries)
  std::vector<AlignResult> h_align;
  std::vector<int32_t> h_ali;
  std::vector<float> h_ac;
};

namespace {

constexpr int64_t kDefaultTrace = int64_t(1) << 27;   // tokens of backtrace storage per call when the caller says 0

int CreateDecoder(pk_mi355_decoder *d, const pk_mi355_fst *f, const pk_mi355_am *am, int max_utts, int64_t trace_capacity) {
  int rc = CreateCore(d, f, am, max_utts, trace_capacity > 0 ? trace_capacity : kDefaultTrace);
  if (rc) return rc;
  d->path_cap = (int)d->trace_cap;
  HIP_TRY(hipMalloc(&d->counters, sizeof(unsigned long long) * 2));
  HIP_TRY(hipMalloc(&d->d_res, sizeof(UttResult) * max_utts));
  HIP_TRY(hipMalloc(&d->d_off, sizeof(int64_t) * max_utts));
  HIP_TRY(hipMalloc(&d->d_T, sizeof(int) * max_utts));
  return 0;
}

void FreeDecoder(pk_mi355_decoder *d) {         // (after its last call: pk_mi355_decoder_destroy)
  hipFree(d->counters); hipFree(d->d_res); hipFree(d->d_off); hipFree(d->d_T);
  hipFree(d->d_arc_pdf); hipFree(d->d_frame_off); hipFree(d->d_align);   // set_alignment's
  hipFree(d->d_ali); hipFree(d->d_ac);                                   // Launch's
  FreeCore(d);
}

// The device pointer where the last call's paths lie: with trace gc on GatherPathsKernel has moved them to the front of
// the record arena.
const int *CallPaths(const pk_mi355_decoder *d) { return d->call_gc ? reinterpret_cast<const int *>(d->rec) : d->path; }

// Queue one decode of num_utts utterances whose log-likelihoods lie at ll + off[u] (T[u] frames each) on `stream`.
int Launch(pk_mi355_decoder *d, const float *ll, const std::vector<int64_t> &off, const std::vector<int> &T,
           hipStream_t stream) {
  const int n = (int)T.size();
  if (d->pending) HIP_TRY(hipEventSynchronize(d->done));   // the previous call's work areas are about to be reused
  d->pending = false; d->have = false; d->num_utts = n;
  d->h_T = T;
  d->h_off = off;
  d->call_gc = d->trace_gc;
  d->call_slice = d->call_gc ? d->trace_cap / std::max(n, 1) : d->trace_cap;
  d->call_records = 0;
  d->call_align = d->alignment;
  if (d->call_align) {                                         // the frames of the call, one utterance after the other
    d->h_frame_off.assign(n + 1, 0);
    for (int u = 0; u < n; ++u) d->h_frame_off[u + 1] = d->h_frame_off[u] + T[u];
    const size_t frames = (size_t)d->h_frame_off[n];
    if (frames > d->d_ali_frames) {
      if (d->d_ali) hipFree(d->d_ali);
      if (d->d_ac) hipFree(d->d_ac);
      d->d_ali = nullptr; d->d_ac = nullptr; d->d_ali_frames = 0;
      HIP_TRY(hipMalloc(&d->d_ali, sizeof(int) * frames));
      HIP_TRY(hipMalloc(&d->d_ac, sizeof(float) * frames));
      d->d_ali_frames = frames;
    }
  }
  if (n > 0) {
    HIP_TRY(hipMemcpyAsync(d->d_off, d->h_off.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d->d_T, d->h_T.data(), sizeof(int) * n, hipMemcpyHostToDevice, stream));
    if (d->call_align)
      HIP_TRY(hipMemcpyAsync(d->d_frame_off, d->h_frame_off.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(d->counters, 0, sizeof(unsigned long long) * 2, stream));
    DecArgs A = ArgsOf(d, ll, n);
    A.ll_off = d->d_off; A.T = d->d_T;
    A.res = d->d_res;
    if (d->call_gc) {                                          // a slice of the arena and of the path arena per utterance
      A.rec_cap = d->call_slice;
      LaunchDecode(A, true, stream);
      LaunchGatherPaths(d->d_res, n, d->path, reinterpret_cast<int *>(d->rec), stream);
    } else {
      A.rec_cap = d->trace_cap; A.rec_top = d->counters;       // one arena and one path arena shared by the call
      A.path_cap = d->path_cap; A.path_top = reinterpret_cast<int *>(d->counters + 1);
      LaunchDecode(A, false, stream);
    }
    if (d->call_align) {
      AlignArgs G = {};
      G.res = d->d_res;
      G.path = CallPaths(d);
      G.path_cap = (int)d->trace_cap;
      G.arc_pdf = d->d_arc_pdf; G.num_arcs = (int)d->labels.ilabel.size();
      G.ll = ll; G.ll_off = d->d_off; G.T = d->d_T; G.frame_off = d->d_frame_off;
      G.num_pdfs = d->num_pdfs; G.num_utts = n;
      G.ali = d->d_ali; G.ac = d->d_ac; G.out = d->d_align;
      LaunchAlign(G, stream);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return Fail(PK_MI355_E_DEVICE, "decode launch: %s", hipGetErrorString(e));
  }
  HIP_TRY(hipEventRecord(d->done, stream));
  d->pending = true;
  return 0;
}

int Collect(pk_mi355_decoder *d) {
  if (!d->pending) return d->have ? 0 : Fail(PK_MI355_E_STATE, "decoder: nothing decoded");
  int rc = UseDevice(d->device);
  if (rc) return rc;
  d->pending = false;
  HIP_TRY(hipEventSynchronize(d->done));
  if (d->batch) {                                    // the score call's range verdict: its results are withheld
    pk_mi355_batch_t *b = d->batch;
    d->batch = nullptr;
    if ((rc = pk_mi355_batch_synchronize(b))) return rc;
  }
  const int n = d->num_utts;
  d->res.resize(n);
  if (n) HIP_TRY(hipMemcpy(d->res.data(), d->d_res, sizeof(UttResult) * n, hipMemcpyDeviceToHost));
  int used = 0;
  for (const auto &r : d->res) used = std::max(used, r.path_off + r.path_len);
  if ((int64_t)used > d->trace_cap) return Fail(PK_MI355_E_DEVICE, "decoder: corrupt result");
  d->h_path.resize(used);
  if (used) HIP_TRY(hipMemcpy(d->h_path.data(), CallPaths(d), sizeof(int) * used, hipMemcpyDeviceToHost));
  if (!d->call_gc) {
    unsigned long long records = 0;
    if (n) HIP_TRY(hipMemcpy(&records, d->counters, sizeof(records), hipMemcpyDeviceToHost));
    d->call_records = (int64_t)std::min(records, (unsigned long long)d->trace_cap);   // (a failed bump overshoots)
  }
  if (d->call_align) {
    const size_t frames = n ? (size_t)d->h_frame_off[n] : 0;
    d->h_align.resize(n); d->h_ali.resize(frames); d->h_ac.resize(frames);
    if (n) HIP_TRY(hipMemcpy(d->h_align.data(), d->d_align, sizeof(AlignResult) * n, hipMemcpyDeviceToHost));
    if (frames) {
      HIP_TRY(hipMemcpy(d->h_ali.data(), d->d_ali, sizeof(int) * frames, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(d->h_ac.data(), d->d_ac, sizeof(float) * frames, hipMemcpyDeviceToHost));
    }
  }
  for (int u = 0; u < n; ++u) {
    const UttResult &r = d->res[u];
    if (r.status == PK_MI355_E_CAPACITY && d->call_gc)
      return Fail(PK_MI355_E_CAPACITY, "decoder: utterance %d: backtrace storage exhausted after compaction (a slice of %lld "
                  "records: trace_capacity %lld over the call's %d utterances; raise it, or decode fewer utterances per call)",
                  u, (long long)d->call_slice, (long long)d->trace_cap, n);
    if (r.status == PK_MI355_E_CAPACITY)
      return Fail(PK_MI355_E_CAPACITY, "decoder: utterance %d: backtrace storage exhausted (trace_capacity %lld: raise it, "
                  "or decode fewer utterances per call)", u, (long long)d->trace_cap);
    if (r.status == PK_MI355_E_INVALID)
      return Fail(PK_MI355_E_INVALID, "decoder: utterance %d: negative epsilon cycle (the closure did not settle)", u);
    if (r.path_off < 0 || r.path_len < 0 || r.path_off + r.path_len > used)
      return Fail(PK_MI355_E_DEVICE, "decoder: utterance %d: corrupt result", u);
    if (d->call_align && (d->h_align[u].status || (d->h_align[u].frames != 0 && d->h_align[u].frames != d->h_T[u])))
      return Fail(PK_MI355_E_DEVICE, "decoder: utterance %d: corrupt result (the best path's emitting arcs are not its %d frames)",
                  u, d->h_T[u]);
  }
  d->have = true;
  return 0;
}

}  // namespace

extern "C" {

pk_mi355_decoder_t *pk_mi355_decoder_create(const pk_mi355_fst_t *fst, const pk_mi355_am_t *am, int max_utts,
                                            int64_t trace_capacity) {
  if (CheckCoreInputs(fst, am)) return nullptr;
  if (max_utts <= 0 || trace_capacity < 0) { Fail(PK_MI355_E_INVALID, "bad decoder capacity"); return nullptr; }
  if (UseDevice(am->device)) return nullptr;
  pk_mi355_decoder *d = new pk_mi355_decoder();
  if (CreateDecoder(d, fst, am, max_utts, trace_capacity)) {
    FreeDecoder(d);
    delete d;
    return nullptr;
  }
  return d;
}

void pk_mi355_decoder_destroy(pk_mi355_decoder_t *d) {
  if (!d) return;
  if (!UseDevice(d->device)) {
    if (d->pending) hipEventSynchronize(d->done);
    FreeDecoder(d);
  }
  delete d;
}

int pk_mi355_decoder_set_beam(pk_mi355_decoder_t *d, float beam, int max_active) {
  if (!d) return Fail(PK_MI355_E_INVALID, "null decoder");
  return SetBeam(d, beam, max_active);
}

int pk_mi355_decoder_set_trace_gc(pk_mi355_decoder_t *d, int enable) {
  if (!d) return Fail(PK_MI355_E_INVALID, "null decoder");
  d->trace_gc = enable != 0;
  return 0;
}

int pk_mi355_decoder_set_alignment(pk_mi355_decoder_t *d, int enable) {
  if (!d) return Fail(PK_MI355_E_INVALID, "null decoder");
  if (enable && !d->d_arc_pdf) {                  // the first enable: the emitting flag and pdf of every arc, by arc id
    int rc = UseDevice(d->device);
    if (rc) return rc;
    const std::vector<int32_t> &tid2pdf = d->am->tid2pdf;
    std::vector<int> arc_pdf(d->labels.ilabel.size());
    for (size_t a = 0; a < arc_pdf.size(); ++a) {
      const int il = d->labels.ilabel[a];           // (CreateDecoder has checked every ilabel against the model)
      arc_pdf[a] = il == 0 ? -1 : tid2pdf.empty() ? il : tid2pdf[il];
    }
    if (!d->d_frame_off) HIP_TRY(hipMalloc(&d->d_frame_off, sizeof(int64_t) * d->max_utts));
    if (!d->d_align) HIP_TRY(hipMalloc(&d->d_align, sizeof(AlignResult) * d->max_utts));
    if ((rc = Upload(&d->d_arc_pdf, arc_pdf))) {
      if (d->d_arc_pdf) hipFree(d->d_arc_pdf);
      d->d_arc_pdf = nullptr;
      return rc;
    }
  }
  d->alignment = enable != 0;
  return 0;
}

int pk_mi355_decoder_decode_batch(pk_mi355_decoder_t *d, pk_mi355_batch_t *b, int sync) {
  if (!d || !b) return Fail(PK_MI355_E_INVALID, "null decoder or batch");
  if (!BatchScored(b)) return Fail(PK_MI355_E_STATE, "batch not scored");
  if (BatchModel(b) != d->am)        // the pdf map the graph was checked and mapped with is that model's
    return Fail(PK_MI355_E_INVALID, "decoder: the batch was scored with another model than the decoder was created for");
  const int n = pk_mi355_batch_num_utts(b);
  if (n > d->max_utts) return Fail(PK_MI355_E_INVALID, "decoder: %d utterances, capacity %d", n, d->max_utts);
  int rc = UseDevice(d->device);
  if (rc) return rc;
  std::vector<int64_t> off(n);
  std::vector<int> T(n);
  const float *base = n ? pk_mi355_batch_loglik_device(b, 0) : nullptr;
  for (int u = 0; u < n; ++u) {
    T[u] = pk_mi355_batch_num_frames(b, u);
    off[u] = pk_mi355_batch_loglik_device(b, u) - base;
  }
  d->batch = nullptr;
  if ((rc = Launch(d, base, off, T, (hipStream_t)pk_mi355_batch_stream(b)))) return rc;
  d->batch = b;
  return sync ? Collect(d) : 0;
}

int pk_mi355_decoder_decode(pk_mi355_decoder_t *d, const pk_decodable_t *utts, int num_utts, int sync) {
  if (!d || (num_utts > 0 && !utts) || num_utts < 0) return Fail(PK_MI355_E_INVALID, "bad decode arguments");
  if (num_utts > d->max_utts) return Fail(PK_MI355_E_INVALID, "decoder: %d utterances, capacity %d", num_utts, d->max_utts);
  int rc = UseDevice(d->device);
  if (rc) return rc;
  if (d->pending) HIP_TRY(hipEventSynchronize(d->done));   // d_ll may still be read by the previous call
  std::vector<int64_t> off(num_utts);
  std::vector<int> T(num_utts);
  int64_t total = 0;
  for (int u = 0; u < num_utts; ++u) {
    const pk_matrix_t &m = utts[u].log_prob;
    if ((rc = CheckLoglik(d, m, "decoder: utterance", u))) return rc;
    off[u] = total;
    T[u] = m.ncol;
    total += (int64_t)m.ncol * d->num_pdfs;
  }
  if ((rc = UploadLoglik(d, utts, num_utts))) return rc;
  d->batch = nullptr;
  if ((rc = Launch(d, d->d_ll, off, T, d->own_stream))) return rc;
  return sync ? Collect(d) : 0;
}

int pk_mi355_decoder_synchronize(pk_mi355_decoder_t *d) {
  if (!d) return Fail(PK_MI355_E_INVALID, "null decoder");
  return Collect(d);
}

static int CheckResult(const pk_mi355_decoder_t *d, int utt) {
  if (!d) return Fail(PK_MI355_E_INVALID, "null decoder");
  if (!d->have) return Fail(PK_MI355_E_STATE, "decoder: no results (synchronize first)");
  if (utt < 0 || utt >= d->num_utts) return Fail(PK_MI355_E_INVALID, "bad utterance index");
  return 0;
}

int pk_mi355_decoder_result(const pk_mi355_decoder_t *d, int utt, int *words, int max_words, float *weight, int *ok) {
  int rc = CheckResult(d, utt);
  if (rc) return rc;
  const UttResult &r = d->res[utt];
  if (weight) *weight = r.weight;
  if (ok) *ok = r.ok;
  return PathWords(d->labels.olabel, d->h_path.data() + r.path_off, r.path_len, words, max_words);
}

int pk_mi355_decoder_best_path_arcs(const pk_mi355_decoder_t *d, int utt, int32_t *arcs, int max_arcs) {
  int rc = CheckResult(d, utt);
  if (rc) return rc;
  const UttResult &r = d->res[utt];
  for (int i = 0; i < r.path_len && i < max_arcs; ++i) arcs[i] = d->h_path[r.path_off + i];
  return r.path_len;
}

static int CheckAligned(const pk_mi355_decoder_t *d, int utt) {
  int rc = CheckResult(d, utt);
  if (rc) return rc;
  if (!d->call_align) return Fail(PK_MI355_E_STATE, "decoder: the call ran with alignment off (pk_mi355_decoder_set_alignment)");
  return 0;
}

int pk_mi355_decoder_alignment(const pk_mi355_decoder_t *d, int utt, int32_t *arc_ids, int32_t *trans_ids, float *acoustic_cost,
                               int max_frames) {
  int rc = CheckAligned(d, utt);
  if (rc) return rc;
  const int frames = d->h_align[utt].frames;
  const int64_t at = d->h_frame_off[utt];
  for (int t = 0; t < frames && t < max_frames; ++t) {
    const int arc = d->h_ali[at + t];
    if (arc_ids) arc_ids[t] = arc;
    if (trans_ids) trans_ids[t] = (arc >= 0 && arc < (int)d->labels.ilabel.size()) ? d->labels.ilabel[arc] : 0;
    if (acoustic_cost) acoustic_cost[t] = d->h_ac[at + t];
  }
  return frames;
}

int pk_mi355_decoder_word_segments(const pk_mi355_decoder_t *d, int utt, pk_mi355_word_t *out, int max) {
  int rc = CheckAligned(d, utt);
  if (rc) return rc;
  const UttResult &r = d->res[utt];
  static const float none = 0.0f;                   // (a call without any frame: still "given", and never read)
  const float *ac = d->h_ac.empty() ? &none : d->h_ac.data() + d->h_frame_off[utt];
  return WordSegments(d->labels, d->h_path.data() + r.path_off, r.path_len, ac, d->h_align[utt].frames, out, max);
}

int pk_mi355_decoder_active_bound(const pk_mi355_decoder_t *d, int utt) {
  int rc = CheckResult(d, utt);
  if (rc) return rc;
  return d->res[utt].active_bound;
}

int pk_mi355_decoder_trace_stats(const pk_mi355_decoder_t *d, int utt, int64_t *peak_records, int64_t *slice_records,
                                 int *compactions) {
  int rc = CheckResult(d, utt);
  if (rc) return rc;
  const UttResult &r = d->res[utt];
  if (peak_records) *peak_records = d->call_gc ? (int64_t)r.peak : d->call_records;
  if (slice_records) *slice_records = d->call_slice;
  if (compactions) *compactions = d->call_gc ? r.compactions : 0;
  return 0;
}

}  // extern "C"
