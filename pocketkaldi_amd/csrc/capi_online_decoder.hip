// capi_online_decoder.hip -- the online decoder, pk_mi355_online_decoder_*: slots that are opened, advanced by chunks
// of log-likelihoods (the host's, or an online scorer's rows on the device) and closed; a slot's tokens and backtrace
// live on the device between calls.  Over the decoder core (pk_decode.h); the kernel is decode.hip's.
#include <vector>

#include "pk_decode.h"

using namespace pkhost;

// What the host keeps of one slot.  A committing slot's path is committed ++ path: the arcs that left the device for
// good, then the best token's tail.  Host memory grows by 4 bytes per committed arc, 8 with alignment.
struct Slot {
  int open = 0, fresh = 1, finished = 0;
  char aligned = 0, committing = 0;             // opened with the alignment / the commit mode on
  OnlineResult res = {};                        // after synchronize
  std::vector<int32_t> path;                    // the arcs of res's path
  std::vector<float> path_ac;                   // aligned only: the acoustic cost of every arc of path
  std::vector<int32_t> committed;
  std::vector<float> committed_ac;              // aligned only
  std::vector<int> committed_words;             // the words (olabel != 0) of committed, kept as the arcs arrive
  int committed_frames = 0;                     // the emitting arcs among committed
  int64_t in_use = 0, peak = 0;                 // records in the arena after the last launch; the most since open
  int committed_run = 0;                        // endpointing: the silent emitting arcs that end committed (epsilons skipped)
  pk_mi355_endpoint_t ep = {};                  // endpointing: the record after the slot's last advance

  void ClearCommitted() { committed.clear(); committed_ac.clear(); committed_words.clear(); committed_frames = 0; committed_run = 0; }
};

// The core's work areas are one per slot, its arenas cap records per slot.
struct pk_mi355_online_decoder : DecoderCore {
  int max_streams = 0;
  int64_t cap = 0;
  // one allocation, fetched in one copy: max_streams results, then as many states, then as many commit lengths
  OnlineResult *d_results = nullptr;
  OnlineState *d_state = nullptr;
  int *d_commit = nullptr;
  int *d_remap = nullptr;
  OnlineCall *d_calls = nullptr;
  bool align = false;                           // pk_mi355_online_decoder_set_alignment
  float *d_rec_ac = nullptr, *d_path_ac = nullptr;   // cap floats per slot each, from the first enable
  bool commit = false;                          // pk_mi355_online_decoder_set_commit
  // pk_mi355_online_decoder_set_endpointing: the rules, the arcs' kind on the host (0 epsilon, 1 emitting, 2 emitting a
  // silence pdf) and, from the first enable, the arcs' pdfs, the silence mask and one record per slot on the device
  bool endpoint = false;
  std::vector<pk_mi355_endpoint_rule_t> rules;
  std::vector<char> arc_kind;
  int *d_arc_pdf = nullptr;
  uint32_t *d_silence = nullptr;
  EndpointRecord *d_endpoint = nullptr;
  std::vector<EndpointRecord> ep_fetched;       // d_endpoint as copied back
  std::vector<Slot> slots;
  std::vector<char> fetched;                    // d_results' allocation as copied back; the last call's slots are read from it
  std::vector<int32_t> got;                     // a slot's path slice as copied back
  std::vector<float> got_ac;
  std::vector<int> last_slots;                  // slots of the last call
  bool pending = false;
};

namespace {

size_t OnlineBlockBytes(int max_streams) { return (sizeof(OnlineResult) + sizeof(OnlineState) + sizeof(int)) * max_streams; }

int OnlineCollect(pk_mi355_online_decoder *o);

int OnlineLaunch(pk_mi355_online_decoder *o, const float *ll, const std::vector<OnlineCall> &calls, hipStream_t stream) {
  // With the commit mode on, what the last call committed exists only in its slots' path slices and commit lengths,
  // which this launch overwrites: a call that was never synchronized is collected first.  What it says of a slot
  // (capacity, ...) was that advance's to report and stays readable in the slot's result; a device failure is returned.
  if (o->pending && o->commit) {
    const int rc = OnlineCollect(o);
    if (rc == PK_MI355_E_DEVICE) return rc;
  }
  if (o->pending) HIP_TRY(hipEventSynchronize(o->done));
  o->pending = false;
  o->last_slots.clear();
  for (const auto &c : calls) o->last_slots.push_back(c.slot);
  const int n = (int)calls.size();
  if (n > 0) {
    HIP_TRY(hipMemcpyAsync(o->d_calls, calls.data(), sizeof(OnlineCall) * n, hipMemcpyHostToDevice, stream));
    // (frames, arenas and results are per slot: the calls, and o->cap entries of rec and path each)
    DecArgs A = ArgsOf(o, ll, n);
    A.rec_cap = o->cap; A.remap = o->d_remap;
    if (o->align) { A.rec_ac = o->d_rec_ac; A.path_ac = o->d_path_ac; }
    if (o->commit) A.commit_len = o->d_commit;
    LaunchOnlineDecode(A, o->d_calls, o->d_state, o->d_results, n, stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return Fail(PK_MI355_E_DEVICE, "online decode launch: %s", hipGetErrorString(e));
    if (o->endpoint) {                                   // the endpoint records of the call's slots, from what the launch left
      EndpointArgs E;
      E.calls = o->d_calls; E.states = o->d_state; E.results = o->d_results; E.n = n;
      E.la = A.la; E.lb = A.lb; E.num_states = o->num_states; E.final_w = o->final_w;
      E.path = o->path; E.cap = o->cap; E.commit_len = o->commit ? o->d_commit : nullptr;
      E.arc_pdf = o->d_arc_pdf; E.num_arcs = (int)o->labels.ilabel.size();
      E.silence = o->d_silence; E.num_pdfs = o->num_pdfs;
      E.out = o->d_endpoint;
      LaunchEndpoint(E, stream);
      e = hipGetLastError();
      if (e != hipSuccess) return Fail(PK_MI355_E_DEVICE, "endpoint launch: %s", hipGetErrorString(e));
    }
  }
  for (const auto &c : calls) {
    Slot &s = o->slots[c.slot];
    s.fresh = 0;
    if (c.final_) { s.finished = 1; s.open = 0; }
  }
  HIP_TRY(hipEventRecord(o->done, stream));
  o->pending = true;
  return 0;
}

int OnlineCollect(pk_mi355_online_decoder *o) {
  if (!o->pending) return 0;
  int rc = UseDevice(o->device);
  if (rc) return rc;
  o->pending = false;
  HIP_TRY(hipEventSynchronize(o->done));
  if (o->last_slots.empty()) return 0;
  // Only the call's slots take their record: a slot opened again since its last launch keeps the cleared record that
  // open gave it, whatever the device still holds of its previous utterance.
  o->fetched.resize(OnlineBlockBytes(o->max_streams));
  HIP_TRY(hipMemcpy(o->fetched.data(), o->d_results, o->fetched.size(), hipMemcpyDeviceToHost));
  const OnlineResult *results = reinterpret_cast<const OnlineResult *>(o->fetched.data());
  const OnlineState *states = reinterpret_cast<const OnlineState *>(results + o->max_streams);
  const int *commits = reinterpret_cast<const int *>(states + o->max_streams);
  if (o->endpoint) {
    o->ep_fetched.resize(o->max_streams);
    HIP_TRY(hipMemcpy(o->ep_fetched.data(), o->d_endpoint, sizeof(EndpointRecord) * o->max_streams, hipMemcpyDeviceToHost));
  }
  int first_bad = -1, first_bad_ep = -1;
  for (int slot : o->last_slots) {
    Slot &s = o->slots[slot];
    s.res = results[slot];
    const OnlineResult &r = s.res;
    const int nc = s.committing ? commits[slot] : 0;            // newly committed arcs, ahead of the tail in the slice
    if (r.path_len < 0 || nc < 0 || (int64_t)nc + r.path_len > o->cap)
      return Fail(PK_MI355_E_DEVICE, "online decoder: slot %d: corrupt result", slot);
    // (the mode-off kernel keeps no maximum inside a launch: there the peak is sampled at the end of each launch only)
    s.in_use = (int64_t)std::min<unsigned long long>(states[slot].top, (unsigned long long)o->cap);
    s.peak = std::max(s.peak, std::max(s.in_use, (int64_t)(s.committing ? states[slot].peak : 0)));
    const int len = nc + r.path_len;
    o->got.resize(len);
    if (len)
      HIP_TRY(hipMemcpy(o->got.data(), o->path + (int64_t)slot * o->cap, sizeof(int32_t) * len, hipMemcpyDeviceToHost));
    s.committed.insert(s.committed.end(), o->got.begin(), o->got.begin() + nc);
    for (int i = 0; i < nc; ++i) {                       // the host's per-step work: the new arcs, not the whole prefix
      const int32_t arc = o->got[i];
      if (arc < 0 || arc >= (int32_t)o->labels.olabel.size()) continue;
      if (o->labels.olabel[arc] != 0) s.committed_words.push_back(o->labels.olabel[arc]);
      s.committed_frames += o->labels.ilabel[arc] != 0;
      if (o->endpoint && o->arc_kind[arc]) s.committed_run = o->arc_kind[arc] == 2 ? s.committed_run + 1 : 0;
    }
    s.path.assign(o->got.begin() + nc, o->got.end());
    if (s.aligned) {
      o->got_ac.resize(len);
      if (len)
        HIP_TRY(hipMemcpy(o->got_ac.data(), o->d_path_ac + (int64_t)slot * o->cap, sizeof(float) * len, hipMemcpyDeviceToHost));
      s.committed_ac.insert(s.committed_ac.end(), o->got_ac.begin(), o->got_ac.begin() + nc);
      s.path_ac.assign(o->got_ac.begin() + nc, o->got_ac.end());
    }
    // no path at all, whatever was committed earlier: a slot that ended, or one that finished without a final token
    if (r.status || !r.ok || !r.has_path) s.ClearCommitted();
    if (r.status && first_bad < 0) first_bad = slot;
    if (o->endpoint) {
      const EndpointRecord &e = o->ep_fetched[slot];
      s.ep = pk_mi355_endpoint_t{};
      if (e.status && !r.status && first_bad_ep < 0) first_bad_ep = slot;
      if (e.valid && !e.status && !r.status && r.ok) {
        s.ep.valid = 1;
        s.ep.frames = r.frames;
        s.ep.trailing_silence_frames = e.tail_silence + (e.tail_open ? s.committed_run : 0);
        s.ep.num_final = e.num_final;
        s.ep.best_cost = e.best_cost; s.ep.final_cost = e.final_cost; s.ep.relative_cost = e.relative_cost;
        s.ep.rule = pk_mi355_endpoint_eval(o->rules.data(), (int)o->rules.size(), s.ep.frames, s.ep.trailing_silence_frames,
                                           s.ep.relative_cost);
      }
    }
  }
  if (first_bad < 0 && first_bad_ep >= 0)
    return Fail(PK_MI355_E_DEVICE, "online decoder: slot %d: the endpoint scan met an arc or a length out of range", first_bad_ep);
  if (first_bad >= 0) {
    const OnlineResult &r = o->slots[first_bad].res;
    if (r.status == PK_MI355_E_CAPACITY)
      return Fail(PK_MI355_E_CAPACITY, "online decoder: slot %d: backtrace storage exhausted after compaction (%lld records "
                  "per slot)", first_bad, (long long)o->cap);
    if (r.status == PK_MI355_E_DEVICE)
      return Fail(PK_MI355_E_DEVICE, "online decoder: slot %d: inconsistent backtrace records at the commit", first_bad);
    return Fail(PK_MI355_E_INVALID, "online decoder: slot %d: negative epsilon cycle (the closure did not settle)", first_bad);
  }
  return 0;
}

// A slot's path (or its costs) as every getter sees it: the tail alone, or committed ++ tail put together in `joined`.
template <typename T>
const std::vector<T> &Joined(const std::vector<T> &committed, const std::vector<T> &tail, std::vector<T> *joined) {
  if (committed.empty()) return tail;
  *joined = committed;
  joined->insert(joined->end(), tail.begin(), tail.end());
  return *joined;
}

// The words of the slot's path: those of the committed prefix as they were kept, then the tail's.
int OnlineWords(const pk_mi355_online_decoder *o, int slot, int *words, int max_words) {
  const Slot &s = o->slots[slot];
  const int c = (int)s.committed_words.size();
  for (int i = 0; words && i < c && i < max_words; ++i) words[i] = s.committed_words[i];
  const bool room = words && c < max_words;
  return c + PathWords(o->labels.olabel, s.path.data(), (int)s.path.size(), room ? words + c : nullptr,
                       room ? max_words - c : 0);
}

int OnlineSlot(const pk_mi355_online_decoder *o, int slot) {
  if (!o) return Fail(PK_MI355_E_INVALID, "null online decoder");
  if (slot < 0 || slot >= o->max_streams) return Fail(PK_MI355_E_INVALID, "slot %d out of range [0, %d)", slot, o->max_streams);
  return 0;
}

// A getter's slot: in range, and no call in flight.
int OnlineReady(const pk_mi355_online_decoder *o, int slot) {
  int rc = OnlineSlot(o, slot);
  if (rc) return rc;
  if (o->pending) return Fail(PK_MI355_E_STATE, "online decoder: synchronize first");
  return 0;
}

// The slot's current path as frames (PathFrames): 0 for a slot without a path.
int OnlineFrames(const pk_mi355_online_decoder *o, int slot, int32_t *arc_ids, int32_t *trans_ids, float *ac, int max_frames) {
  const Slot &s = o->slots[slot];
  const OnlineResult &r = s.res;
  if (!r.has_path || !r.ok || r.status) return 0;
  if (!s.aligned) return Fail(PK_MI355_E_STATE, "online decoder: slot %d was decoded with alignment off", slot);
  std::vector<int32_t> joined;
  std::vector<float> joined_ac;
  const auto &p = Joined(s.committed, s.path, &joined);
  const auto &pa = Joined(s.committed_ac, s.path_ac, &joined_ac);
  if (pa.size() != p.size()) return Fail(PK_MI355_E_DEVICE, "online decoder: slot %d: path and costs differ in length", slot);
  return PathFrames(o->labels, p.data(), pa.data(), (int)p.size(), r.frames, arc_ids, trans_ids, ac, max_frames);
}

}  // namespace

namespace pkhost {
bool OnlineDecoderSlotOpen(const pk_mi355_online_decoder *o, int slot) {
  return o && slot >= 0 && slot < o->max_streams && o->slots[slot].open != 0;
}
const std::vector<int> *OnlineDecoderCommittedWords(const pk_mi355_online_decoder *o, int slot) {
  return o && slot >= 0 && slot < o->max_streams ? &o->slots[slot].committed_words : nullptr;
}
void OnlineDecoderTailWords(const pk_mi355_online_decoder *o, int slot, std::vector<int> *words) {
  words->clear();
  if (!o || slot < 0 || slot >= o->max_streams) return;
  const auto &p = o->slots[slot].path;
  words->resize(PathWords(o->labels.olabel, p.data(), (int)p.size(), nullptr, 0));
  PathWords(o->labels.olabel, p.data(), (int)p.size(), words->data(), (int)words->size());
}
}  // namespace pkhost

extern "C" {

pk_mi355_online_decoder_t *pk_mi355_online_decoder_create(const pk_mi355_fst_t *fst, const pk_mi355_am_t *am, int max_streams,
                                                          int64_t trace_capacity) {
  if (CheckCoreInputs(fst, am)) return nullptr;
  if (max_streams <= 0 || trace_capacity < 0) { Fail(PK_MI355_E_INVALID, "bad online decoder capacity"); return nullptr; }
  const int64_t cap = trace_capacity > 0 ? trace_capacity : (int64_t)1 << 20;
  if (cap * max_streams > (int64_t)INT32_MAX) { Fail(PK_MI355_E_INVALID, "online decoder: max_streams x trace_capacity above 2^31 - 1"); return nullptr; }
  if (UseDevice(am->device)) return nullptr;
  pk_mi355_online_decoder *o = new pk_mi355_online_decoder();
  o->max_streams = max_streams;
  o->cap = cap;
  bool ok = CreateCore(o, fst, am, max_streams, cap * max_streams) == 0;
  auto chk = [&](hipError_t e) { if (e != hipSuccess && ok) { ok = false; Fail(PK_MI355_E_DEVICE, "online_decoder_create: %s", hipGetErrorString(e)); } };
  static_assert(sizeof(OnlineResult) % alignof(OnlineState) == 0, "the states follow the results in one allocation");
  if (ok) chk(hipMalloc(&o->d_results, OnlineBlockBytes(max_streams)));
  if (ok) chk(hipMemset(o->d_results, 0, OnlineBlockBytes(max_streams)));
  if (ok) {
    o->d_state = reinterpret_cast<OnlineState *>(o->d_results + max_streams);
    o->d_commit = reinterpret_cast<int *>(o->d_state + max_streams);
  }
  if (ok) chk(hipMalloc(&o->d_remap, sizeof(int) * cap * max_streams));
  if (ok) chk(hipMalloc(&o->d_calls, sizeof(OnlineCall) * max_streams));
  if (!ok) { pk_mi355_online_decoder_destroy(o); return nullptr; }
  o->slots.assign(max_streams, Slot{});
  return o;
}

void pk_mi355_online_decoder_destroy(pk_mi355_online_decoder_t *o) {
  if (!o) return;
  if (!UseDevice(o->device)) {
    if (o->pending) hipEventSynchronize(o->done);
    hipFree(o->d_results); hipFree(o->d_remap); hipFree(o->d_calls);
    hipFree(o->d_rec_ac); hipFree(o->d_path_ac);
    hipFree(o->d_arc_pdf); hipFree(o->d_silence); hipFree(o->d_endpoint);
    FreeCore(o);
  }
  delete o;
}

int pk_mi355_online_decoder_set_beam(pk_mi355_online_decoder_t *o, float beam, int max_active) {
  if (!o) return Fail(PK_MI355_E_INVALID, "null online decoder");
  return SetBeam(o, beam, max_active);
}

int pk_mi355_online_decoder_set_alignment(pk_mi355_online_decoder_t *o, int enable) {
  if (!o) return Fail(PK_MI355_E_INVALID, "null online decoder");
  for (int slot = 0; slot < o->max_streams; ++slot)     // one launch serves every slot: the mode is the object's
    if (o->slots[slot].open) return Fail(PK_MI355_E_STATE, "online decoder: slot %d is open (set_alignment needs every slot closed)", slot);
  int rc = UseDevice(o->device);
  if (rc) return rc;
  // A call still in flight ends first.  What it says of a slot (capacity, a closure that did not settle) was that
  // advance's to report and stays readable in the slot's result: only a device failure stops the mode change.
  if ((rc = OnlineCollect(o)) == PK_MI355_E_DEVICE) return rc;
  if (enable && !o->d_rec_ac) {
    const size_t bytes = sizeof(float) * (size_t)o->cap * o->max_streams;
    float *rec_ac = nullptr, *path_ac = nullptr;
    hipError_t e = hipMalloc(&rec_ac, bytes);
    if (e == hipSuccess && (e = hipMalloc(&path_ac, bytes)) != hipSuccess) hipFree(rec_ac);
    if (e != hipSuccess) return Fail(PK_MI355_E_DEVICE, "online_decoder_set_alignment: %s", hipGetErrorString(e));
    o->d_rec_ac = rec_ac; o->d_path_ac = path_ac;
  }
  o->align = enable != 0;                                // (a finished slot keeps its results, and the mode it was opened with)
  return 0;
}

int pk_mi355_online_decoder_set_commit(pk_mi355_online_decoder_t *o, int enable) {
  if (!o) return Fail(PK_MI355_E_INVALID, "null online decoder");
  for (int slot = 0; slot < o->max_streams; ++slot)     // one launch serves every slot: the mode is the object's
    if (o->slots[slot].open) return Fail(PK_MI355_E_STATE, "online decoder: slot %d is open (set_commit needs every slot closed)", slot);
  int rc = UseDevice(o->device);
  if (rc) return rc;
  if ((rc = OnlineCollect(o)) == PK_MI355_E_DEVICE) return rc;      // (as set_alignment: a call in flight ends first)
  o->commit = enable != 0;                               // (a finished slot keeps its results, and the mode it was opened with)
  return 0;
}

int pk_mi355_online_decoder_set_endpointing(pk_mi355_online_decoder_t *o, const int32_t *silence_pdfs, int num_silence,
                                            const pk_mi355_endpoint_rule_t *rules, int num_rules) {
  if (!o) return Fail(PK_MI355_E_INVALID, "null online decoder");
  if (num_silence < 0 || num_rules < 0 || (num_silence > 0 && !silence_pdfs) || (num_rules > 0 && !rules))
    return Fail(PK_MI355_E_INVALID, "online decoder: bad endpointing arguments");
  for (int i = 0; i < num_silence; ++i)
    if (silence_pdfs[i] < 0 || silence_pdfs[i] >= o->num_pdfs)
      return Fail(PK_MI355_E_INVALID, "online decoder: silence pdf %d outside [0, %d)", (int)silence_pdfs[i], o->num_pdfs);
  for (int i = 0; i < num_rules; ++i) {
    if (rules[i].min_trailing_silence_frames < 0 || rules[i].min_utterance_frames < 0)
      return Fail(PK_MI355_E_INVALID, "online decoder: endpoint rule %d: negative frame count", i);
    if (rules[i].max_relative_cost != rules[i].max_relative_cost)
      return Fail(PK_MI355_E_INVALID, "online decoder: endpoint rule %d: max_relative_cost is NaN", i);
  }
  for (int slot = 0; slot < o->max_streams; ++slot)     // one launch serves every slot: the mode is the object's
    if (o->slots[slot].open) return Fail(PK_MI355_E_STATE, "online decoder: slot %d is open (set_endpointing needs every slot closed)", slot);
  int rc = UseDevice(o->device);
  if (rc) return rc;
  if ((rc = OnlineCollect(o)) == PK_MI355_E_DEVICE) return rc;      // (as set_alignment: a call in flight ends first)
  if (num_rules == 0) { o->endpoint = false; o->rules.clear(); return 0; }
  const size_t words = ((size_t)o->num_pdfs + 31) / 32;
  std::vector<uint32_t> mask(words, 0u);
  for (int i = 0; i < num_silence; ++i) mask[silence_pdfs[i] >> 5] |= 1u << (silence_pdfs[i] & 31);
  const std::vector<int32_t> &tid2pdf = o->am->tid2pdf;
  const size_t num_arcs = o->labels.ilabel.size();
  std::vector<int> arc_pdf(num_arcs);
  std::vector<char> kind(num_arcs);
  for (size_t a = 0; a < num_arcs; ++a) {
    const int il = o->labels.ilabel[a];                  // (CreateCore has checked every ilabel against the model)
    arc_pdf[a] = il == 0 ? -1 : tid2pdf.empty() ? il : tid2pdf[il];
    const int p = arc_pdf[a];
    kind[a] = p < 0 ? 0 : (p < o->num_pdfs && ((mask[p >> 5] >> (p & 31)) & 1u)) ? 2 : 1;
  }
  if (!o->d_endpoint) {                                  // the first enable
    int *d_arc_pdf = nullptr;
    uint32_t *d_silence = nullptr;
    EndpointRecord *d_endpoint = nullptr;
    hipError_t e = hipMalloc(&d_arc_pdf, sizeof(int) * std::max<size_t>(num_arcs, 1));
    if (e == hipSuccess) e = hipMalloc(&d_silence, sizeof(uint32_t) * std::max<size_t>(words, 1));
    if (e == hipSuccess) e = hipMalloc(&d_endpoint, sizeof(EndpointRecord) * o->max_streams);
    if (e == hipSuccess) e = hipMemset(d_endpoint, 0, sizeof(EndpointRecord) * o->max_streams);
    if (e == hipSuccess && num_arcs) e = hipMemcpy(d_arc_pdf, arc_pdf.data(), sizeof(int) * num_arcs, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      hipFree(d_arc_pdf); hipFree(d_silence); hipFree(d_endpoint);
      return Fail(PK_MI355_E_DEVICE, "online_decoder_set_endpointing: %s", hipGetErrorString(e));
    }
    o->d_arc_pdf = d_arc_pdf; o->d_silence = d_silence; o->d_endpoint = d_endpoint;
  }
  if (words) HIP_TRY(hipMemcpy(o->d_silence, mask.data(), sizeof(uint32_t) * words, hipMemcpyHostToDevice));
  o->arc_kind.swap(kind);
  o->rules.assign(rules, rules + num_rules);
  o->endpoint = true;                                    // (a finished slot keeps its results)
  return 0;
}

int pk_mi355_online_decoder_endpoint(const pk_mi355_online_decoder_t *o, int slot, pk_mi355_endpoint_t *out) {
  int rc = OnlineReady(o, slot);
  if (rc) return rc;
  if (!o->endpoint) return Fail(PK_MI355_E_STATE, "online decoder: endpointing is off (pk_mi355_online_decoder_set_endpointing)");
  const Slot &s = o->slots[slot];
  const bool live = s.open && !s.fresh && !s.finished;
  if (out) *out = live ? s.ep : pk_mi355_endpoint_t{};
  return live ? s.ep.rule : 0;
}

int pk_mi355_online_decoder_finish(pk_mi355_online_decoder_t *o, const int *slots, int n, int sync) {
  if (!o || n < 0 || (n > 0 && !slots)) return Fail(PK_MI355_E_INVALID, "bad finish arguments");
  int rc = UseDevice(o->device);
  if (rc) return rc;
  std::vector<char> seen(o->max_streams, 0);
  std::vector<OnlineCall> calls(n);
  for (int i = 0; i < n; ++i) {
    const int slot = slots[i];
    if ((rc = OnlineSlot(o, slot))) return rc;
    if (!o->slots[slot].open) return Fail(PK_MI355_E_STATE, "online decoder: slot %d is not open", slot);
    if (seen[slot]) return Fail(PK_MI355_E_INVALID, "online decoder: slot %d twice in one call", slot);
    seen[slot] = 1;
    calls[i] = OnlineCall{slot, 0, 1, o->slots[slot].fresh, 0};      // no new frame: the closing launch alone
  }
  // (OnlineLaunch waits for a pending advance -- and collects it with commit on -- before it queues this one)
  if ((rc = OnlineLaunch(o, o->d_ll, calls, o->own_stream))) return rc;
  return sync ? OnlineCollect(o) : 0;
}

int pk_mi355_online_decoder_open(pk_mi355_online_decoder_t *o, int slot) {
  int rc = OnlineSlot(o, slot);
  if (rc) return rc;
  if (o->slots[slot].open) return Fail(PK_MI355_E_STATE, "online decoder: slot %d is open", slot);
  if ((rc = OnlineCollect(o))) return rc;       // a result of the slot's last utterance is replaced
  Slot fresh;
  fresh.open = 1; fresh.aligned = o->align; fresh.committing = o->commit;
  o->slots[slot] = fresh;
  return 0;
}

int pk_mi355_online_decoder_advance_host(pk_mi355_online_decoder_t *o, const int *slots, const pk_decodable_t *chunks,
                                         const int *final_, int n, int sync) {
  if (!o || n < 0 || (n > 0 && (!slots || !chunks))) return Fail(PK_MI355_E_INVALID, "bad advance arguments");
  int rc = UseDevice(o->device);
  if (rc) return rc;
  std::vector<char> seen(o->max_streams, 0);
  int64_t total = 0;
  std::vector<OnlineCall> calls(n);
  for (int i = 0; i < n; ++i) {
    const int slot = slots[i];
    if ((rc = OnlineSlot(o, slot))) return rc;
    if (!o->slots[slot].open) return Fail(PK_MI355_E_STATE, "online decoder: slot %d is not open", slot);
    if (seen[slot]) return Fail(PK_MI355_E_INVALID, "online decoder: slot %d twice in one call", slot);
    seen[slot] = 1;
    const pk_matrix_t &m = chunks[i].log_prob;
    if ((rc = CheckLoglik(o, m, "online decoder: chunk", i))) return rc;
    calls[i] = OnlineCall{slot, m.ncol, final_ && final_[i] ? 1 : 0, o->slots[slot].fresh, total};
    total += (int64_t)m.ncol * o->num_pdfs;
  }
  if (o->pending) HIP_TRY(hipEventSynchronize(o->done));     // d_ll may still be read by the previous call
  if ((rc = UploadLoglik(o, chunks, n))) return rc;
  if ((rc = OnlineLaunch(o, o->d_ll, calls, o->own_stream))) return rc;
  return sync ? OnlineCollect(o) : 0;
}

int pk_mi355_online_decoder_advance(pk_mi355_online_decoder_t *o, pk_mi355_stream_t *s, int sync) {
  if (!o || !s) return Fail(PK_MI355_E_INVALID, "null online decoder or stream");
  if (StreamModel(s) != o->am)
    return Fail(PK_MI355_E_INVALID, "online decoder: the stream scores with another model than the decoder was created for");
  if (StreamSlots(s) > o->max_streams) return Fail(PK_MI355_E_INVALID, "online decoder: the stream has more slots than the decoder");
  int rc = UseDevice(o->device);
  if (rc) return rc;
  std::vector<OnlineCall> calls;
  const float *base = StreamLoglikBase(s);
  for (int slot = 0; slot < StreamSlots(s); ++slot) {
    if (!o->slots[slot].open) continue;
    int first = 0, count = 0;
    const float *p = pk_mi355_stream_loglik_device(s, slot, &first, &count);
    const bool fin = StreamSlotFlushed(s, slot);
    if (count == 0 && !fin) continue;
    calls.push_back(OnlineCall{slot, count, fin ? 1 : 0, o->slots[slot].fresh, count ? (int64_t)(p - base) : 0});
  }
  if ((rc = OnlineLaunch(o, base, calls, StreamHipStream(s)))) return rc;
  return sync ? OnlineCollect(o) : 0;
}

int pk_mi355_online_decoder_synchronize(pk_mi355_online_decoder_t *o) {
  if (!o) return Fail(PK_MI355_E_INVALID, "null online decoder");
  return OnlineCollect(o);
}

int pk_mi355_online_decoder_partial(const pk_mi355_online_decoder_t *o, int slot, int *words, int max_words, float *cost) {
  int rc = OnlineReady(o, slot);
  if (rc) return rc;
  if (cost) *cost = o->slots[slot].res.weight;
  return OnlineWords(o, slot, words, max_words);
}

int pk_mi355_online_decoder_result(const pk_mi355_online_decoder_t *o, int slot, int *words, int max_words, float *weight,
                                   int *ok) {
  int rc = OnlineReady(o, slot);
  if (rc) return rc;
  if (!o->slots[slot].finished || !o->slots[slot].res.final_) return Fail(PK_MI355_E_STATE, "online decoder: slot %d is not finished", slot);
  if (weight) *weight = o->slots[slot].res.weight;
  if (ok) *ok = o->slots[slot].res.ok;
  return OnlineWords(o, slot, words, max_words);
}

int pk_mi355_online_decoder_best_path_arcs(const pk_mi355_online_decoder_t *o, int slot, int32_t *arcs, int max_arcs) {
  int rc = OnlineReady(o, slot);
  if (rc) return rc;
  std::vector<int32_t> joined;
  const auto &p = Joined(o->slots[slot].committed, o->slots[slot].path, &joined);
  for (int i = 0; i < (int)p.size() && i < max_arcs; ++i) arcs[i] = p[i];
  return (int)p.size();
}

int pk_mi355_online_decoder_word_segments(const pk_mi355_online_decoder_t *o, int slot, pk_mi355_word_t *out, int max) {
  int rc = OnlineReady(o, slot);
  if (rc) return rc;
  std::vector<int32_t> joined;
  const auto &p = Joined(o->slots[slot].committed, o->slots[slot].path, &joined);
  if (!o->align || !o->slots[slot].aligned)             // (the rows are gone, and no cost was kept: no acoustic cost)
    return WordSegments(o->labels, p.data(), (int)p.size(), nullptr, 0, out, max);
  std::vector<float> ac(std::max(o->slots[slot].res.frames, 1));                    // the costs kept with the trace
  const int frames = OnlineFrames(o, slot, nullptr, nullptr, ac.data(), (int)ac.size());
  if (frames < 0) return frames;
  return WordSegments(o->labels, p.data(), (int)p.size(), ac.data(), frames, out, max);
}

int pk_mi355_online_decoder_alignment(const pk_mi355_online_decoder_t *o, int slot, int32_t *arc_ids, int32_t *trans_ids,
                                      float *acoustic_cost, int max_frames) {
  int rc = OnlineReady(o, slot);
  if (rc) return rc;
  if (!o->align) return Fail(PK_MI355_E_STATE, "online decoder: alignment is off (pk_mi355_online_decoder_set_alignment)");
  return OnlineFrames(o, slot, arc_ids, trans_ids, acoustic_cost, max_frames);
}

int pk_mi355_online_decoder_committed(const pk_mi355_online_decoder_t *o, int slot, int *words, int max_words, int *num_arcs,
                                      int *num_frames) {
  int rc = OnlineReady(o, slot);
  if (rc) return rc;
  const auto &cw = o->slots[slot].committed_words;
  if (num_arcs) *num_arcs = (int)o->slots[slot].committed.size();
  if (num_frames) *num_frames = o->slots[slot].committed_frames;
  for (int i = 0; words && i < (int)cw.size() && i < max_words; ++i) words[i] = cw[i];
  return (int)cw.size();
}

int pk_mi355_online_decoder_trace_stats(const pk_mi355_online_decoder_t *o, int slot, int64_t *in_use, int64_t *peak,
                                        int64_t *capacity) {
  int rc = OnlineReady(o, slot);
  if (rc) return rc;
  if (o->slots[slot].fresh) return Fail(PK_MI355_E_STATE, "online decoder: slot %d has not been advanced since it was opened", slot);
  if (in_use) *in_use = o->slots[slot].in_use;
  if (peak) *peak = o->slots[slot].peak;
  if (capacity) *capacity = o->cap;
  return 0;
}

int pk_mi355_online_decoder_num_frames(const pk_mi355_online_decoder_t *o, int slot) {
  int rc = OnlineReady(o, slot);
  if (rc) return rc;
  return o->slots[slot].res.frames;
}

int pk_mi355_online_decoder_active_bound(const pk_mi355_online_decoder_t *o, int slot) {
  int rc = OnlineReady(o, slot);
  if (rc) return rc;
  return o->slots[slot].res.active_bound;
}

}  // extern "C"
