// pk_decode.h -- what crosses between the decoder's kernels (decode.hip) and its two host objects
// (capi_decoder.hip, capi_online_decoder.hip), and what those two share: the decoder core (internal).
#ifndef PK_DECODE_H_
#define PK_DECODE_H_

#include "pk_host.h"

namespace pkmi {

// ------------------------------------------------------------------ kernel arguments and results (decode.hip)

constexpr int kMaxDecPdfs = 16384;                 // one frame's log-likelihood row in LDS: 64 KiB at most
constexpr uint32_t kEpsBit = 0x80000000u;          // candidate id of an epsilon arc (loses ties to an emitting one)

struct Tok {        // one token: its state, cost and trace record (-1: the start token)
  int state;
  float cost;
  int trace;
  int pad;
};

struct UttResult {
  int status;       // 0, PK_MI355_E_CAPACITY, PK_MI355_E_INVALID
  int ok;           // Decode()'s return (decoder.cc:77)
  float weight;     // Hypothesis::weight()
  int path_off;     // arc ids of the best path in the path arena, start to end
  int path_len;
  int active_bound; // largest per-frame count of touched states
  int peak;         // trace-gc mode: the most records the utterance's slice held (taken before every compaction)
  int compactions;  // trace-gc mode: how often the slice was compacted
};

struct DecArgs {
  // graph, split into emitting and epsilon CSR lists (arc order kept).  Arcs: x = next state, y = pdf
  // (ilabel mapped through the model's tid2pdf at create), z = weight bits, w = original arc id.
  const int *e_off; const int4 *e_arc; const int *e_src;
  const int *n_off; const int4 *n_arc; const int *n_src;
  const float *final_w;
  int num_states, start, num_pdfs;
  // log-likelihoods: utterance u's frame t is ll + ll_off[u] + t * num_pdfs
  const float *ll; const int64_t *ll_off; const int *T;
  int num_utts;
  // per-utterance work areas (stride num_states entries)
  uint64_t *key; int *tr; int *mark; int *touched; int *nxt; Tok *la; Tok *lb; Tok *fa; Tok *fb;
  // backtrace arena and best-path arena, rec_cap entries of each per utterance or slot.  Read by
  //   DecodeKernel<false>: rec, path, rec_cap (one of each for the call), path_cap, the bump counters rec_top / path_top
  //   DecodeKernel<true>:  rec, path (the remap scratch until the path is written), rec_cap; the slice's top is in LDS
  //   OnlineDecodeKernel:  rec, path, rec_cap, remap (the slot's top is its OnlineState's); rec_ac and path_ac, both or
  //     neither, with alignment (<true, .>); commit_len with commit (<., true>): what each holds is said at the kernel
  int2 *rec; int64_t rec_cap; unsigned long long *rec_top;
  int *path; int path_cap; int *path_top;
  float beam; int max_active; int max_rounds;
  UttResult *res;
  int *remap; float *rec_ac; float *path_ac; int *commit_len;
};

struct AlignResult {
  int status;       // 0, or PK_MI355_E_DEVICE: the path's emitting arcs are not the utterance's frames
  int frames;       // frames aligned
};

struct AlignArgs {
  const UttResult *res;
  const int *path; int path_cap;        // the call's paths (path_off / path_len of res index it) and its entries
  const int *arc_pdf; int num_arcs;     // by original arc id: the pdf, -1 for an epsilon arc
  const float *ll; const int64_t *ll_off; const int *T; const int64_t *frame_off;
  int num_pdfs, num_utts;
  int *ali; float *ac;                  // per frame of the call: utterance u's frame t at frame_off[u] + t
  AlignResult *out;
};

struct OnlineState {
  int nL, par;            // tokens of the current list and which of the slot's two list buffers holds them
  int ok, status;         // N2 / capacity / closure verdicts: a slot that ended stays ended
  int active, frames;     // largest touched count; frames decoded
  int started, peak;      // peak: the commit mode's kernel only -- the most the arena held since open
  unsigned long long top; // records used in the slot's arena
};

struct OnlineResult {
  int status, ok, final_, path_len;
  float weight;           // final: Hypothesis::weight(); partial: the best token's cost
  int active_bound, frames, has_path;
};

struct OnlineCall {       // one slot of a launch
  int slot, T, final_, fresh;
  int64_t ll_off;
};

struct EndpointRecord {   // what EndpointKernel says of one slot after a launch (pk_mi355_online_decoder_set_endpointing)
  int valid;              // 0: the slot finished, ended or holds no token -- nothing else is meaningful
  int status;             // 0, or PK_MI355_E_DEVICE: an arc id or a length of the slot's path is out of range
  int num_final;          // tokens whose cost + final weight is not INFINITY
  int tail_silence;       // emitting arcs of the scanned path after its last non-silent emitting arc
  int tail_open;          // the scanned path has no non-silent emitting arc
  int tail_frames;        // emitting arcs of the scanned path
  float best_cost, final_cost, relative_cost;
  int pad;
};

struct EndpointArgs {
  const OnlineCall *calls; const OnlineState *states; const OnlineResult *results;   // of the decode launch before it
  int n;
  const Tok *la, *lb; int num_states;                  // the slots' two token lists (DecArgs), stride num_states
  const float *final_w;
  const int *path; int64_t cap; const int *commit_len; // the slots' path slices; commit_len: null with commit off
  const int *arc_pdf; int num_arcs;                    // by original arc id: the pdf, -1 for an epsilon arc
  const uint32_t *silence; int num_pdfs;               // bit p of the mask: pdf p is silence
  EndpointRecord *out;                                 // per slot
};

// ------------------------------------------------------------------ launchers (decode.hip)
// One workgroup per utterance (slot) of A.num_utts (n); a frame's log-likelihood row is the dynamic LDS.

// DecodeKernel<trace_gc>: the whole utterances of one batch call
void LaunchDecode(const DecArgs &A, bool trace_gc, hipStream_t stream);
// after LaunchDecode with trace_gc: the n best paths from their slices of `path` to the front of `out`
void LaunchGatherPaths(UttResult *res, int n, const int *path, int *out, hipStream_t stream);
// after the decode (and the gather) on the same stream: the frame of every emitting arc of the best paths
void LaunchAlign(const AlignArgs &A, hipStream_t stream);
// the new frames of n slots (calls; states and results are per slot): OnlineDecodeKernel<A.rec_ac && A.path_ac, A.commit_len>
void LaunchOnlineDecode(const DecArgs &A, const OnlineCall *calls, OnlineState *states, OnlineResult *results, int n,
                        hipStream_t stream);
// after LaunchOnlineDecode on the same stream, over the same calls: EndpointKernel, one record per slot of the call
void LaunchEndpoint(const EndpointArgs &E, hipStream_t stream);

}  // namespace pkmi

namespace pkhost {

// ------------------------------------------------------------------ decoder core (capi_decoder.hip)
// What the batch and the online decoder both are: the graph on the device, one set of work areas per slot, the
// backtrace and path arenas, the upload buffer of host log-likelihoods, a stream and the event of the last call.
// Where a call's frames, results and arena slices are is the owner's.
struct DecoderCore {
  int device = 0;
  const pk_mi355_am *am = nullptr;              // the model the graph's ilabels were checked against
  int max_utts = 0, num_states = 0, start = 0, num_pdfs = 0;   // max_utts: utterances per call, or slots
  float beam = 16.0f;
  int max_active = 30000;
  int64_t trace_cap = 0;                        // entries of rec and of path
  // device graph
  int *e_off = nullptr, *e_src = nullptr, *n_off = nullptr, *n_src = nullptr;
  int4 *e_arc = nullptr, *n_arc = nullptr;
  float *final_w = nullptr;
  // work areas
  uint64_t *key = nullptr;
  int *tr = nullptr, *mark = nullptr, *touched = nullptr, *nxt = nullptr;
  Tok *lists = nullptr;
  int2 *rec = nullptr;
  int *path = nullptr;
  float *d_ll = nullptr;                        // host decodables uploaded here
  size_t d_ll_floats = 0;
  hipStream_t own_stream = nullptr;
  hipEvent_t done = nullptr;                    // the owner's last call
  ArcLabels labels;                             // the graph's labels and weights by original arc id (words, segments)
};

// The create entries' first checks: a graph, and a finalized model.
int CheckCoreInputs(const pk_mi355_fst *f, const pk_mi355_am *am);
// On the selected device (am's).  On failure the caller still calls FreeCore.
int CreateCore(DecoderCore *c, const pk_mi355_fst *f, const pk_mi355_am *am, int max_utts, int64_t trace_cap);
void FreeCore(DecoderCore *c);                  // (the owner has waited for its last call)
int SetBeam(DecoderCore *c, float beam, int max_active);
// What every launch over c's graph and work areas shares (n utterances or slots, log-likelihoods at ll); the caller
// adds where its frames, backtrace arena, paths and results are.
DecArgs ArgsOf(const DecoderCore *c, const float *ll, int n);
// One host log-likelihood matrix against the model (`what`: the caller's name for item i).
int CheckLoglik(const DecoderCore *c, const pk_matrix_t &m, const char *what, int i);
// Checked host log-likelihoods into d_ll, one after the other (item i at the sum of the sizes before it), queued on
// own_stream.  The caller has waited for the last call that read d_ll.
int UploadLoglik(DecoderCore *c, const pk_decodable_t *src, int n);

}  // namespace pkhost

#endif  // PK_DECODE_H_
