// decode.hip -- the search half of pk_process (Decoder::Decode + BestPath, decoder.cc:39-339) on the GPU,
// batched: one workgroup per utterance decodes the whole utterance in ONE launch, frame after frame,
// synchronising only with __syncthreads() (no workgroup waits on another).  The graph's reader and its split into
// the arc lists below are host-only: pk_files.cc.
//
// Semantics (DESIGN.md "Decoder"): the reference's float / double arithmetic operation for operation;
// order-independent where the reference depends on iteration order:
//   * emitting candidates are kept when <= R0 (the bound from the best token's arcs, decoder.cc:244-262),
//     and only tokens <= F (the exact non-emitting cutoff) form the next frame's list;
//   * ties on a state go to the lowest candidate id (64-bit atomicMin of (ordered cost bits << 32) | id);
//   * when max-active binds, the cutoff is the EXACT max_active-th smallest cost (radix select), not the
//     reference's 200-cost sample (decoder.cc:137-168);
//   * N1: a NaN log-likelihood decodes as -inf; N2: a frame that starts without a token of finite cost ends the
//     utterance with ok = 0 (where the reference dereferences a null best_tok).
// Compiled with -ffp-contract=off and no fast-math (build.py), like every other translation unit.
#include <math.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "pk_host.h"

using namespace pkhost;

namespace {

constexpr int kDecThreads = 512;
constexpr int kDecWaves = kDecThreads / 64;
constexpr int kMaxDecPdfs = 16384;                 // one frame's log-likelihood row in LDS: 64 KiB at most
constexpr uint32_t kEpsBit = 0x80000000u;          // candidate id of an epsilon arc (loses ties to an emitting one)
constexpr uint32_t kStartId = 0x7FFFFFFFu;         // the start token's id (never resolved: it has no arc)
constexpr uint64_t kEmpty = ~0ull;
constexpr int64_t kDefaultTrace = int64_t(1) << 27;   // tokens of backtrace storage per call when the caller says 0

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
  // backtrace arena and best-path arena.  DecodeKernel<false>: shared by the call, with their capacities and bump
  // counters; DecodeKernel<true>: a slice of rec_cap entries of each per utterance (no counter: the top lives in LDS);
  // OnlineDecodeKernel: rec and path only, a slice per slot (its capacity is a kernel argument, its top the slot's state)
  int2 *rec; int64_t rec_cap; unsigned long long *rec_top;
  int *path; int path_cap; int *path_top;
  float beam; int max_active; int max_rounds;
  UttResult *res;
};

__device__ __forceinline__ uint32_t OrdBits(float c) {
  const uint32_t u = __float_as_uint(c);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float OrdFloat(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
__device__ __forceinline__ uint64_t Pack(float c, uint32_t id) { return (uint64_t(OrdBits(c)) << 32) | id; }
// keys are changed by atomics (performed at L2): read them past the L1
__device__ __forceinline__ uint64_t LoadKey(const uint64_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct Shared {
  int scan[kDecWaves];
  int cnt_touched, cnt_nxt, fail;
  unsigned long long base;
  double dred[kDecWaves];
  uint64_t ured[kDecWaves];
  int hist[256];
  int sel;
  // one chunk of source tokens of a load-balanced expansion
  int excl[kDecThreads];
  int first[kDecThreads];
};

// exclusive scan of one int per thread; *total = the sum (all threads)
__device__ int BlockScan(Shared &sh, int v, int *total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) sh.scan[w] = x;
  __syncthreads();
  int before = 0, all = 0;
  for (int i = 0; i < kDecWaves; ++i) {
    const int s = sh.scan[i];
    if (i < w) before += s;
    all += s;
  }
  __syncthreads();
  *total = all;
  return before + x - v;
}

__device__ double BlockMinD(Shared &sh, double v) {
  for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d, 64));
  if ((threadIdx.x & 63) == 0) sh.dred[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = sh.dred[0];
  for (int i = 1; i < kDecWaves; ++i) r = fmin(r, sh.dred[i]);
  __syncthreads();
  return r;
}

__device__ uint64_t BlockMinU(Shared &sh, uint64_t v) {
  for (int d = 32; d >= 1; d >>= 1) {
    const uint64_t o = __shfl_xor(v, d, 64);
    v = o < v ? o : v;
  }
  if ((threadIdx.x & 63) == 0) sh.ured[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t r = sh.ured[0];
  for (int i = 1; i < kDecWaves; ++i) r = sh.ured[i] < r ? sh.ured[i] : r;
  __syncthreads();
  return r;
}

// The k-th smallest (1-based) ordered cost of list[0..n): four 8-bit radix passes over an LDS histogram.
__device__ uint32_t SelectKth(Shared &sh, const Tok *list, int n, int k) {
  uint32_t prefix = 0, mask = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = threadIdx.x; i < 256; i += kDecThreads) sh.hist[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kDecThreads) {
      const uint32_t o = OrdBits(list[i].cost);
      if ((o & mask) == prefix) atomicAdd(&sh.hist[(o >> shift) & 255], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int acc = 0, b = 0;
      for (; b < 255; ++b) {
        if (acc + sh.hist[b] >= k) break;
        acc += sh.hist[b];
      }
      sh.sel = b;
      sh.cnt_nxt = k - acc;      // rank inside the chosen bin (scratch; cnt_nxt is reset before use)
    }
    __syncthreads();
    prefix |= uint32_t(sh.sel) << shift;
    mask |= 255u << shift;
    k = sh.cnt_nxt;
    __syncthreads();
  }
  return prefix;
}

// Load-balanced walk over the arcs of src[0..n) (CSR off/arcs), skipping tokens whose cost > cut.
// fn(token index j, csr arc index a) for every arc; lanes walk the flattened arc range chunk by chunk.
template <typename Fn>
__device__ void ForArcs(Shared &sh, const Tok *src, int n, float cut, const int *off, Fn fn) {
  for (int c0 = 0; c0 < n; c0 += kDecThreads) {
    const int j = c0 + threadIdx.x;
    int cnt = 0, first = 0;
    if (j < n) {
      const Tok t = src[j];
      if (!(t.cost > cut)) {
        first = off[t.state];
        cnt = off[t.state + 1] - first;
      }
    }
    int total;
    const int ex = BlockScan(sh, cnt, &total);
    sh.excl[threadIdx.x] = ex;
    sh.first[threadIdx.x] = first;
    __syncthreads();
    const int m = min(kDecThreads, n - c0);
    for (int e = threadIdx.x; e < total; e += kDecThreads) {
      int lo = 0, hi = m - 1;                        // the last token whose exclusive offset is <= e
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sh.excl[mid] <= e) lo = mid; else hi = mid - 1;
      }
      fn(c0 + lo, sh.first[lo] + (e - sh.excl[lo]));
    }
    __syncthreads();
  }
}

// The backtrace arena that trace records go to: the call's shared one (DecodeKernel<false>), an utterance's slice of it
// (DecodeKernel<true>) or a slot's own (OnlineDecodeKernel).
struct Arena {
  int2 *rec;                    // (previous record, original arc id)
  int64_t cap;
  unsigned long long *top;      // records used
};

// One utterance's (slot's) decoding state for the duration of a launch.
struct Work {
  uint64_t *key; int *tr, *mark, *touched, *nxt;    // state table, trace index, frontier mark, touched / improved states
  Tok *L, *Lnext, *fa, *fb;                         // this frame's tokens, the next frame's, the closure's two frontiers
  Arena arena;
  int nL;                                           // tokens in L
  int status, ok, active;                           // failure code; N2's verdict; largest per-frame count of touched states
  int frames, par;                                  // online only: frames decoded; which list buffer L is
};

__device__ __forceinline__ Work WorkOf(const DecArgs &A, int u, const Arena &arena) {
  const size_t at = (size_t)A.num_states * u;
  Work w;
  w.key = A.key + at;
  w.tr = A.tr + at; w.mark = A.mark + at; w.touched = A.touched + at; w.nxt = A.nxt + at;
  w.L = A.la + at; w.Lnext = A.lb + at; w.fa = A.fa + at; w.fb = A.fb + at;
  w.arena = arena;
  w.nL = 0; w.status = 0; w.ok = 1; w.active = 0; w.frames = 0; w.par = 0;
  return w;
}

// Give each winner of touched-or-improved states a trace record and write it as a token into out[].
// states[0..n): the states; arcs/srcs: the CSR the winners' ids index (emitting or epsilon);
// only winners <= F are kept.  Returns the number written (all threads), or -1 when the arena is full.
__device__ int Resolve(Shared &sh, const DecArgs &A, const Arena &R, const int *states, int n, float F, bool eps,
                       uint64_t *key, int *tr, int *mark, Tok *out) {
  int written = 0;
  for (int c0 = 0; c0 < n; c0 += kDecThreads) {
    const int i = c0 + threadIdx.x;
    int need = 0, s = 0, prev = -1, arc = -1;
    float c = 0.f;
    if (i < n) {
      s = states[i];
      if (eps) mark[s] = 0;
      const uint64_t k = LoadKey(&key[s]);
      c = OrdFloat(uint32_t(k >> 32));
      const uint32_t id = uint32_t(k);
      if (!(c > F) && id != kStartId) {
        need = 1;
        if (eps) {
          const int a = int(id & ~kEpsBit);
          prev = tr[A.n_src[a]];
          arc = A.n_arc[a].w;
        } else {
          prev = tr[A.e_src[id]];
          arc = A.e_arc[id].w;
        }
      }
    }
    int total;
    const int ex = BlockScan(sh, need, &total);
    if (threadIdx.x == 0) sh.base = total ? atomicAdd(R.top, (unsigned long long)total) : 0ull;
    __syncthreads();
    const unsigned long long base = sh.base;
    __syncthreads();
    if (base + (unsigned long long)total > (unsigned long long)R.cap) return -1;
    if (need) {
      const int r = int(base) + ex;
      R.rec[r] = make_int2(prev, arc);
      Tok t;
      t.state = s; t.cost = c; t.trace = r; t.pad = 0;
      out[written + ex] = t;
    }
    written += total;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < written; i += kDecThreads) tr[out[i].state] = out[i].trace;
  __syncthreads();
  return written;
}

// The frame step, shared by the whole-utterance and the online kernel: InitDecoding when the first frame index t is
// -1, then frames t .. T - 1 of ll (ProcessEmitting, ProcessNonemitting, the next token list).  before(L, nL) runs
// ahead of every emitting frame: nothing for DecodeKernel<false>, the trace compaction for DecodeKernel<true> and
// OnlineDecodeKernel.
template <typename Before>
__device__ __forceinline__ void DecodeFrames(Shared &sh, float *s_ll, const DecArgs &A, Work &w, const float *ll, int t,
                                             int T, Before before) {
  uint64_t *key = w.key;
  int *tr = w.tr, *mark = w.mark, *touched = w.touched, *nxt = w.nxt;
  Tok *L = w.L, *Lnext = w.Lnext, *fa = w.fa, *fb = w.fb;
  int status = w.status, ok = w.ok, active = w.active;
  int nL = w.nL, nT = 0, nF = 0;
  float F = INFINITY;

  // InitDecoding (decoder.cc:79-97): the start token, cost 0, then the epsilon closure with an infinite cutoff
  if (t < 0) {
    if (threadIdx.x == 0) {
      key[A.start] = Pack(0.0f, kStartId);
      touched[0] = A.start;
      tr[A.start] = -1;
      Tok tk;
      tk.state = A.start; tk.cost = 0.0f; tk.trace = -1; tk.pad = 0;
      fa[0] = tk;
    }
    nT = 1;
    nF = 1;
    __syncthreads();
  }

  for (; t < T; ++t) {
    if (t >= 0) {
      before(L, nL);
      // ---- ProcessEmitting (decoder.cc:226-301)
      // N1: a NaN log-likelihood decodes as -inf (fmaxf returns the operand that is not NaN), its candidates as +inf
      for (int p = threadIdx.x; p < A.num_pdfs; p += kDecThreads)
        s_ll[p] = fmaxf(ll[(size_t)t * A.num_pdfs + p], -INFINITY);
      // GetCutoff (:132-182): best token (lowest state on equal cost), exact max-active cutoff
      uint64_t bk = kEmpty;
      for (int i = threadIdx.x; i < nL; i += kDecThreads) {
        const uint64_t k = (uint64_t(OrdBits(L[i].cost)) << 32) | uint32_t(L[i].state);
        bk = k < bk ? k : bk;
      }
      bk = BlockMinU(sh, bk);
      const float best = OrdFloat(uint32_t(bk >> 32));
      const int best_state = int(uint32_t(bk));
      // N2: no token of finite cost (or none at all: the beam emptied) -- the reference's best_tok stays null
      if (!(best < INFINITY)) { ok = 0; break; }
      const double beam_cutoff = (double)best + (double)A.beam;
      float adaptive_beam = A.beam, weight_cutoff = (float)beam_cutoff;
      if (nL > A.max_active) {
        const double kth = (double)OrdFloat(SelectKth(sh, L, nL, A.max_active));
        if (kth < beam_cutoff) {
          adaptive_beam = (float)(kth - (double)best + (double)0.5f);
          weight_cutoff = (float)kth;
        }
      }
      // R0: the bound from the best token's arcs (:244-262)
      double r0 = INFINITY;
      for (int a = A.e_off[best_state] + threadIdx.x; a < A.e_off[best_state + 1]; a += kDecThreads) {
        const int4 arc = A.e_arc[a];
        const float c = (best + __int_as_float(arc.z)) + (-s_ll[arc.y]);
        r0 = fmin(r0, (double)c + (double)adaptive_beam);
      }
      __syncthreads();                                 // (s_ll complete before the block reductions' barriers matter)
      r0 = BlockMinD(sh, r0);
      if (threadIdx.x == 0) sh.cnt_touched = 0;
      __syncthreads();
      // every candidate <= R0 into the state table
      double cmin = INFINITY;
      ForArcs(sh, L, nL, weight_cutoff, A.e_off, [&](int j, int a) {
        const int4 arc = A.e_arc[a];
        const float c = (L[j].cost + __int_as_float(arc.z)) + (-s_ll[arc.y]);
        cmin = fmin(cmin, (double)c);
        if ((double)c > r0) return;
        const uint64_t k = Pack(c, uint32_t(a));
        const uint64_t old = atomicMin((unsigned long long *)&key[arc.x], (unsigned long long)k);
        if (old == kEmpty) touched[atomicAdd(&sh.cnt_touched, 1)] = arc.x;
      });
      cmin = BlockMinD(sh, cmin);
      nT = sh.cnt_touched;
      F = (float)(cmin + (double)adaptive_beam);       // the non-emitting cutoff ProcessEmitting returns
      nF = Resolve(sh, A, w.arena, touched, nT, F, false, key, tr, mark, fa);
      if (nF < 0) { status = PK_MI355_E_CAPACITY; break; }
    }
    // ---- ProcessNonemitting (decoder.cc:186-222): frontier by frontier to the fixed point, bounded
    int rounds = 0;
    while (nF > 0) {
      if (rounds >= A.max_rounds) { status = PK_MI355_E_INVALID; break; }
      if (threadIdx.x == 0) { sh.cnt_nxt = 0; sh.cnt_touched = nT; }
      __syncthreads();
      ForArcs(sh, fa, nF, INFINITY, A.n_off, [&](int j, int a) {
        const int4 arc = A.n_arc[a];
        const float c = fa[j].cost + __int_as_float(arc.z);
        if (c > F) return;
        const uint64_t k = Pack(c, uint32_t(a) | kEpsBit);
        const uint64_t old = atomicMin((unsigned long long *)&key[arc.x], (unsigned long long)k);
        if (k < old) {
          if (old == kEmpty) touched[atomicAdd(&sh.cnt_touched, 1)] = arc.x;
          if (atomicExch(&mark[arc.x], 1) == 0) nxt[atomicAdd(&sh.cnt_nxt, 1)] = arc.x;
        }
      });
      const int nN = sh.cnt_nxt;
      nT = sh.cnt_touched;
      __syncthreads();
      nF = Resolve(sh, A, w.arena, nxt, nN, F, true, key, tr, mark, fb);
      if (nF < 0) { status = PK_MI355_E_CAPACITY; break; }
      Tok *x = fa; fa = fb; fb = x;
      ++rounds;
    }
    if (status) break;
    active = max(active, nT);
    // the next frame's tokens: the touched states <= F; every touched entry of the table is reset
    int written = 0;
    for (int c0 = 0; c0 < nT; c0 += kDecThreads) {
      const int i = c0 + threadIdx.x;
      int keep = 0, s = 0;
      float c = 0.f;
      if (i < nT) {
        s = touched[i];
        c = OrdFloat(uint32_t(LoadKey(&key[s]) >> 32));
        keep = !(c > F);
      }
      int total;
      const int ex = BlockScan(sh, keep, &total);
      if (keep) {
        Tok tk;
        tk.state = s; tk.cost = c; tk.trace = tr[s]; tk.pad = 0;
        Lnext[written + ex] = tk;
      }
      written += total;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nT; i += kDecThreads) key[touched[i]] = kEmpty;
    nT = 0;
    nL = written;
    { Tok *x = L; L = Lnext; Lnext = x; }
    w.par ^= 1;
    if (t >= 0) ++w.frames;
    __syncthreads();
  }
  if (status) {                                        // leave the work areas clean for the next call
    for (int i = threadIdx.x; i < nT; i += kDecThreads) {
      key[touched[i]] = kEmpty;
      mark[touched[i]] = 0;
    }
  }
  w.L = L; w.Lnext = Lnext; w.nL = nL; w.status = status; w.ok = ok; w.active = active;
}

// The token whose path is the result (its index in w.L to every thread, or -1) and the hypothesis' weight.
// fin: BestPath (decoder.cc:304-339), min (double)cost + final over the final tokens, != INFINITY; otherwise the
// partial hypothesis, the bare cost.  Lowest state on a tie in both.
__device__ __forceinline__ int BestToken(Shared &sh, const DecArgs &A, const Work &w, bool fin, float *weight) {
  const Tok *L = w.L;
  double bc = INFINITY;
  int bi = -1;
  for (int i = threadIdx.x; i < w.nL; i += kDecThreads) {
    const double c = (double)L[i].cost + (fin ? (double)A.final_w[L[i].state] : 0.0);
    if (c != INFINITY && (c < bc || (c == bc && bi >= 0 && L[i].state < L[bi].state))) { bc = c; bi = i; }
  }
  const double m = BlockMinD(sh, bc);
  uint64_t cand = (bi >= 0 && bc == m) ? ((uint64_t(uint32_t(L[bi].state)) << 32) | uint32_t(bi)) : kEmpty;
  cand = BlockMinU(sh, cand);
  bi = cand == kEmpty ? -1 : int(uint32_t(cand));
  float wt = (float)m;
  if (fin && bi >= 0) wt += A.final_w[L[bi].state];    // final() counted twice, as the reference does (:338-339)
  *weight = wt;
  return bi;
}

// The path walk of one lane: count the records from `trace` back to the start, then fill path[0..len) back to front.
__device__ __forceinline__ int PathLen(const Arena &R, int trace) {
  int len = 0;
  for (int x = trace; x >= 0 && len <= R.cap; x = R.rec[x].x) ++len;
  return len;
}
__device__ __forceinline__ void FillPath(const Arena &R, int trace, int *path, int len) {
  for (int x = trace; x >= 0 && len > 0; x = R.rec[x].x) path[--len] = R.rec[x].y;
}

// Mark the records reachable from the list's tokens, renumber them in creation order with an exclusive scan (a
// record's predecessor is always older, so one forward pass remaps every `prev`), move them down, and rewrite the
// tokens' trace (and the state table's, which the next emitting step reads).  Changes where records live, never a
// result.
__device__ void CompactTrace(Shared &sh, int2 *rec, int *remap, unsigned long long *top, Tok *L, int nL, int *tr) {
  const int n = (int)*top;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += kDecThreads) remap[i] = 0;
  __syncthreads();
  for (int j = threadIdx.x; j < nL; j += kDecThreads)
    for (int x = L[j].trace; x >= 0 && atomicExch(&remap[x], 1) == 0;) x = rec[x].x;
  __syncthreads();
  int base = 0;
  for (int c0 = 0; c0 < n; c0 += kDecThreads) {
    const int i = c0 + threadIdx.x;
    const int alive = i < n ? __hip_atomic_load(&remap[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;   // set by atomics
    int2 r = make_int2(-1, -1);
    if (alive) r = rec[i];
    int total;
    const int ex = BlockScan(sh, alive, &total);    // (its barriers: every read of this chunk is done)
    if (i < n) remap[i] = alive ? base + ex : -1;
    __syncthreads();
    if (alive) {
      r.x = r.x >= 0 ? remap[r.x] : -1;            // older: remapped in this chunk or an earlier one
      rec[base + ex] = r;
    }
    base += total;
    __syncthreads();
  }
  for (int j = threadIdx.x; j < nL; j += kDecThreads) {
    const int x = L[j].trace;
    if (x >= 0) {
      L[j].trace = remap[x];
      tr[L[j].state] = remap[x];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) *top = (unsigned long long)base;
  __syncthreads();
}

// kGc = false: the call's shared arena and path arena, their bump counters in HBM; nothing is reclaimed.
// kGc = true (pk_mi355_decoder_set_trace_gc): utterance u owns entries [u * rec_cap, (u + 1) * rec_cap) of rec and of
// path, its top lives in LDS, and the slice is compacted when more than half full before an emitting frame, as the
// online kernel does.  Until the best path is written the utterance's slice of path is the compaction's remap scratch
// (one int per record); no counter of the call is touched.
template <bool kGc>
__global__ void __launch_bounds__(kDecThreads) DecodeKernel(DecArgs A) {
  extern __shared__ float s_ll[];
  __shared__ Shared sh;
  __shared__ unsigned long long s_top;                 // kGc only
  const int u = blockIdx.x;
  if (u >= A.num_utts) return;
  Work w;
  int peak = 0, compactions = 0;
  if constexpr (kGc) {
    if (threadIdx.x == 0) s_top = 0;
    __syncthreads();
    const int64_t at = (int64_t)u * A.rec_cap;
    w = WorkOf(A, u, Arena{A.rec + at, A.rec_cap, &s_top});
    int *remap = A.path + at;
    DecodeFrames(sh, s_ll, A, w, A.ll + A.ll_off[u], -1, A.T[u], [&](Tok *L, int nL) {
      const unsigned long long top = s_top;
      peak = max(peak, (int)top);
      if (top > (unsigned long long)(A.rec_cap / 2)) {
        CompactTrace(sh, w.arena.rec, remap, &s_top, L, nL, w.tr);
        ++compactions;
      }
    });
    peak = (int)min((unsigned long long)A.rec_cap, max((unsigned long long)peak, s_top));   // (a failed bump overshoots)
  } else {
    w = WorkOf(A, u, Arena{A.rec, A.rec_cap, A.rec_top});
    DecodeFrames(sh, s_ll, A, w, A.ll + A.ll_off[u], -1, A.T[u], [](Tok *, int) {});
  }
  float weight = 0.f;
  int bi = -1;
  if (!w.status && w.ok) bi = BestToken(sh, A, w, true, &weight);
  if (threadIdx.x == 0) {
    UttResult r;
    r.status = w.status; r.ok = (w.status || w.nL == 0) ? 0 : w.ok; r.weight = 0.f;
    r.path_off = 0; r.path_len = 0; r.active_bound = w.active; r.peak = peak; r.compactions = compactions;
    if (!w.status && r.ok && bi >= 0) {
      r.weight = weight;
      const int len = PathLen(w.arena, w.L[bi].trace);
      if constexpr (kGc) {                             // a chain of the slice's records: it fits the slice of path
        if (len > A.rec_cap) {                         // (cannot happen: PathLen stops counting at cap + 1)
          r.status = PK_MI355_E_CAPACITY;
          r.ok = 0;
        } else {
          r.path_off = int((int64_t)u * A.rec_cap); r.path_len = len;
          FillPath(w.arena, w.L[bi].trace, A.path + r.path_off, len);
        }
      } else {
        const int off = atomicAdd(A.path_top, len);    // the call's shared path arena
        if (off + len > A.path_cap) {                  // (cannot happen: see CreateDecoder)
          r.status = PK_MI355_E_CAPACITY;
          r.ok = 0;
        } else {
          r.path_off = off; r.path_len = len;
          FillPath(w.arena, w.L[bi].trace, A.path + off, len);
        }
      }
    }
    A.res[u] = r;
  }
}

// After DecodeKernel<true> the best paths lie one per slice of the path arena.  Moved together, in utterance order, to
// the front of `out` (the record arena, dead once every path is written: at most trace_capacity ints of its
// 2 x trace_capacity), so that the host fetches one prefix as it does with the mode off.  One workgroup per utterance.
__global__ void __launch_bounds__(256) GatherPathsKernel(UttResult *res, int n, const int *path, int *out) {
  const int u = blockIdx.x;
  if (u >= n) return;
  int off = 0;
  for (int v = 0; v < u; ++v) off += res[v].path_len;
  const int from = res[u].path_off, len = res[u].path_len;
  for (int i = threadIdx.x; i < len; i += blockDim.x) out[off + i] = path[from + i];
  __syncthreads();
  if (threadIdx.x == 0) res[u].path_off = off;
}

// ================================================================== alignment (pk_mi355_decoder_set_alignment)
// After the decode (and, with trace gc, after GatherPathsKernel) on the same stream: the frame of every emitting arc of
// the best path.  One workgroup per utterance walks the path's arc ids in chunks of the block size; an exclusive scan
// over "this arc emits" with a base carried from chunk to chunk numbers the frames.  Per frame t it writes the arc id
// and the acoustic cost -N1(ll[t][pdf]).  An utterance that failed, ended with ok = 0 or has no path writes nothing.

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

__global__ void __launch_bounds__(kDecThreads) AlignKernel(AlignArgs A) {
  __shared__ Shared sh;
  __shared__ int s_bad;
  const int u = blockIdx.x;
  if (u >= A.num_utts) return;
  const UttResult r = A.res[u];
  const int T = A.T[u];
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  const bool active = !r.status && r.ok && r.path_len > 0;
  const bool inside = r.path_off >= 0 && (int64_t)r.path_off + r.path_len <= (int64_t)A.path_cap;
  int base = 0;
  if (active && inside) {
    const int *path = A.path + r.path_off;
    const float *ll = A.ll + A.ll_off[u];
    const int64_t at = A.frame_off[u];
    for (int c0 = 0; c0 < r.path_len; c0 += kDecThreads) {
      const int i = c0 + threadIdx.x;
      int arc = -1, pdf = -1;
      if (i < r.path_len) {
        arc = path[i];
        if (arc >= 0 && arc < A.num_arcs) pdf = A.arc_pdf[arc];
        else s_bad = 1;
      }
      const int emits = pdf >= 0 && pdf < A.num_pdfs;
      int total;
      const int t = base + BlockScan(sh, emits, &total);
      if (emits && t < T) {
        A.ali[at + t] = arc;
        A.ac[at + t] = -fmaxf(ll[(size_t)t * A.num_pdfs + pdf], -INFINITY);   // N1: a NaN log-likelihood counts as -inf
      }
      base += total;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool good = active && inside && !s_bad && base == T;
    AlignResult o;
    o.status = active && !good ? PK_MI355_E_DEVICE : 0;
    o.frames = good ? base : 0;
    A.out[u] = o;
  }
}

// ================================================================== online decoding (pk_mi355_online_decoder_*)
// DecodeFrames, resumable: a slot's token list, its count and buffer, ok / status, the largest touched count, the
// frames decoded and its trace-arena top live in HBM between launches.  One workgroup per slot with new frames;
// InitDecoding on the slot's first launch, BestPath only once the slot is closed.  Each slot has an arena of its own
// (A.rec and A.path hold `cap` entries per slot); when it is more than half full before an emitting frame the
// reachable records are compacted (CompactTrace).  The compaction, the frame count and the list-buffer parity are all
// this kernel adds to the frame step: DecodeKernel<false> instantiates it with an empty `before` and never reads them.

struct OnlineState {
  int nL, par;            // tokens of the current list and which of the slot's two list buffers holds them
  int ok, status;         // N2 / capacity / closure verdicts: a slot that ended stays ended
  int active, frames;     // largest touched count; frames decoded
  int started, pad;
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

__global__ void __launch_bounds__(kDecThreads) OnlineDecodeKernel(DecArgs A, const OnlineCall *calls, OnlineState *states,
                                                                    OnlineResult *results, int *remap_all, int64_t cap) {
  extern __shared__ float s_ll[];
  __shared__ Shared sh;
  const OnlineCall call = calls[blockIdx.x];
  const int u = call.slot;
  OnlineState st = states[u];
  if (call.fresh) {
    st.nL = 0; st.par = 0; st.ok = 1; st.status = 0; st.active = 0; st.frames = 0; st.started = 0; st.pad = 0; st.top = 0;
  }
  __shared__ unsigned long long s_top;
  if (threadIdx.x == 0) s_top = st.top;
  __syncthreads();
  Work w = WorkOf(A, u, Arena{A.rec + (int64_t)u * cap, cap, &s_top});   // the slot's own arena
  int *remap = remap_all + (int64_t)u * cap;
  if (st.par) { Tok *x = w.L; w.L = w.Lnext; w.Lnext = x; }
  w.nL = st.nL; w.status = st.status; w.ok = st.ok; w.active = st.active; w.frames = st.frames; w.par = st.par;
  if (!w.status && w.ok)
    DecodeFrames(sh, s_ll, A, w, A.ll + call.ll_off, st.started ? 0 : -1, call.T, [&](Tok *L, int nL) {
      if (s_top > (unsigned long long)(cap / 2)) CompactTrace(sh, w.arena.rec, remap, &s_top, L, nL, w.tr);
    });
  // the path of the best token: BestPath's once the slot is closed, the partial hypothesis' otherwise
  const bool fin = call.final_ != 0;
  float weight = 0.f;
  int bi = -1;
  if (!w.status && w.ok) bi = BestToken(sh, A, w, fin, &weight);
  if (threadIdx.x == 0) {
    OnlineResult r;
    r.status = w.status; r.final_ = fin ? 1 : 0;
    r.ok = (w.status || w.nL == 0) ? 0 : w.ok;
    r.weight = 0.f; r.path_len = 0; r.has_path = 0;
    r.active_bound = w.active; r.frames = w.frames;
    if (!w.status && r.ok && bi >= 0) {
      r.weight = weight;
      r.path_len = PathLen(w.arena, w.L[bi].trace);
      FillPath(w.arena, w.L[bi].trace, A.path + (int64_t)u * cap, r.path_len);
      r.has_path = 1;
    }
    results[u] = r;
    st.nL = w.nL; st.par = w.par; st.ok = w.ok; st.status = w.status; st.active = w.active; st.frames = w.frames;
    st.started = 1; st.top = s_top;
    states[u] = st;
  }
}
}  // namespace

// ================================================================== host objects

struct pk_mi355_decoder {
  int device = 0;
  const pk_mi355_am *am = nullptr;              // the model the graph's ilabels were checked against
  int max_utts = 0, num_states = 0, start = 0, num_pdfs = 0;
  float beam = 16.0f;
  int max_active = 30000;
  int64_t trace_cap = 0;
  bool trace_gc = false;                        // set_trace_gc: how the next call uses the arena
  // device graph
  int *e_off = nullptr, *e_src = nullptr, *n_off = nullptr, *n_src = nullptr;
  int4 *e_arc = nullptr, *n_arc = nullptr;
  float *final_w = nullptr;
  // work areas
  uint64_t *key = nullptr;
  int *tr = nullptr, *mark = nullptr, *touched = nullptr, *nxt = nullptr;
  Tok *lists = nullptr;
  int2 *rec = nullptr;
  unsigned long long *counters = nullptr;       // [0] records used; [1] (as int) path entries used
  int *path = nullptr;
  int path_cap = 0;
  UttResult *d_res = nullptr;
  float *d_ll = nullptr;                        // host decodables uploaded here
  size_t d_ll_floats = 0;
  int64_t *d_off = nullptr;
  int *d_T = nullptr;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;                 // where the last call was queued
  hipEvent_t done = nullptr;
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
  ArcLabels labels;                             // the graph's labels and weights by original arc id (words, segments)
  // alignment (set_alignment): the mode of the next call and of the last one; the device table and buffers, made at
  // the first enable
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

void FreeDecoderDevice(pk_mi355_decoder *d) {
  void *ptrs[] = {d->e_off, d->e_src, d->n_off, d->n_src, d->e_arc, d->n_arc, d->final_w, d->key, d->tr, d->mark,
                  d->touched, d->nxt, d->lists, d->rec, d->counters, d->path, d->d_res, d->d_ll, d->d_off, d->d_T,
                  d->d_arc_pdf, d->d_frame_off, d->d_align, d->d_ali, d->d_ac};
  for (void *p : ptrs) if (p) hipFree(p);
  if (d->done) hipEventDestroy(d->done);
  if (d->own_stream) hipStreamDestroy(d->own_stream);
}

template <typename T>
int Upload(T **dst, const std::vector<T> &src, size_t min_count = 1) {
  const size_t n = std::max(src.size(), min_count);
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(dst), sizeof(T) * n));
  if (!src.empty()) HIP_TRY(hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
  return 0;
}

int CreateDecoder(pk_mi355_decoder *d, const pk_mi355_fst *f, const pk_mi355_am *am, int max_utts, int64_t trace_capacity) {
  const int S = f->num_states;
  const int N = am->num_pdfs;
  if (N <= 0 || N > kMaxDecPdfs) return Fail(PK_MI355_E_INVALID, "decoder: num_pdfs %d outside [1, %d]", N, kMaxDecPdfs);
  GraphSplit g;
  int rc = SplitGraph(*f, am->tid2pdf, N, &g);
  if (rc) return rc;
  d->max_utts = max_utts; d->num_states = S; d->start = f->start; d->num_pdfs = N;
  d->trace_cap = trace_capacity > 0 ? trace_capacity : kDefaultTrace;
  if (d->trace_cap > (int64_t)INT32_MAX) return Fail(PK_MI355_E_INVALID, "decoder: trace_capacity above 2^31 - 1");
  // a SplitArc is uploaded as the int4 the kernels read: x = next state, y = pdf, z = weight bits, w = original arc id
  static_assert(sizeof(SplitArc) == sizeof(int4) && offsetof(SplitArc, next) == offsetof(int4, x) &&
                offsetof(SplitArc, pdf) == offsetof(int4, y) && offsetof(SplitArc, weight_bits) == offsetof(int4, z) &&
                offsetof(SplitArc, arc) == offsetof(int4, w), "SplitArc is laid out as int4");
  static_assert(kMaxSplitArcs == kEpsBit - 1, "candidate ids: an arc's index, the top bit for epsilon arcs");
  SplitArc *e_arc = nullptr, *n_arc = nullptr;
  rc = Upload(&e_arc, g.e_arc);
  d->e_arc = reinterpret_cast<int4 *>(e_arc);
  if (!rc) rc = Upload(&n_arc, g.n_arc);
  d->n_arc = reinterpret_cast<int4 *>(n_arc);
  if (rc || (rc = Upload(&d->e_off, g.e_off)) || (rc = Upload(&d->n_off, g.n_off)) || (rc = Upload(&d->e_src, g.e_src)) ||
      (rc = Upload(&d->n_src, g.n_src)) || (rc = Upload(&d->final_w, f->final_w)))
    return rc;
  LabelsOf(*f, &d->labels);
  const size_t per = (size_t)S * max_utts;
  HIP_TRY(hipMalloc(&d->key, sizeof(uint64_t) * per));
  HIP_TRY(hipMemset(d->key, 0xFF, sizeof(uint64_t) * per));
  HIP_TRY(hipMalloc(&d->tr, sizeof(int) * per));
  HIP_TRY(hipMalloc(&d->mark, sizeof(int) * per));
  HIP_TRY(hipMemset(d->mark, 0, sizeof(int) * per));
  HIP_TRY(hipMalloc(&d->touched, sizeof(int) * per));
  HIP_TRY(hipMalloc(&d->nxt, sizeof(int) * per));
  HIP_TRY(hipMalloc(&d->lists, sizeof(Tok) * per * 4));
  HIP_TRY(hipMalloc(&d->rec, sizeof(int2) * (size_t)d->trace_cap));
  // The best paths of one call are disjoint chains of that call's trace records, so an arena of trace_capacity
  // entries always holds them all.
  HIP_TRY(hipMalloc(&d->path, sizeof(int) * (size_t)d->trace_cap));
  d->path_cap = (int)d->trace_cap;
  HIP_TRY(hipMalloc(&d->counters, sizeof(unsigned long long) * 2));
  HIP_TRY(hipMalloc(&d->d_res, sizeof(UttResult) * max_utts));
  HIP_TRY(hipMalloc(&d->d_off, sizeof(int64_t) * max_utts));
  HIP_TRY(hipMalloc(&d->d_T, sizeof(int) * max_utts));
  HIP_TRY(hipStreamCreateWithFlags(&d->own_stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&d->done, hipEventDisableTiming));
  return 0;
}

// What every launch over d's graph and work areas shares (n utterances or slots, log-likelihoods at ll); the caller
// adds where its frames, backtrace arena, paths and results are.
DecArgs ArgsOf(const pk_mi355_decoder *d, const float *ll, int n) {
  DecArgs A = {};
  A.e_off = d->e_off; A.e_arc = d->e_arc; A.e_src = d->e_src;
  A.n_off = d->n_off; A.n_arc = d->n_arc; A.n_src = d->n_src;
  A.final_w = d->final_w;
  A.num_states = d->num_states; A.start = d->start; A.num_pdfs = d->num_pdfs;
  A.ll = ll; A.num_utts = n;
  const size_t per = (size_t)d->num_states * d->max_utts;
  A.key = d->key; A.tr = d->tr; A.mark = d->mark; A.touched = d->touched; A.nxt = d->nxt;
  A.la = d->lists; A.lb = d->lists + per; A.fa = d->lists + 2 * per; A.fb = d->lists + 3 * per;
  A.rec = d->rec; A.path = d->path;
  A.beam = d->beam; A.max_active = d->max_active;
  A.max_rounds = d->num_states + 2;    // Bellman-Ford bound: more rounds only under a negative epsilon cycle
  return A;
}

// One host log-likelihood matrix against the model (`what`: the caller's name for item i).
int CheckLoglik(const pk_mi355_decoder *d, const pk_matrix_t &m, const char *what, int i) {
  if (m.ncol < 0 || (m.ncol > 0 && (m.nrow != d->num_pdfs || !m.data)))
    return Fail(PK_MI355_E_INVALID, "%s %d: log_prob is {ncol %d, nrow %d}, nrow %d expected", what, i, m.ncol, m.nrow,
                d->num_pdfs);
  return 0;
}

// Checked host log-likelihoods into d_ll, one after the other (item i at the sum of the sizes before it), queued on
// own_stream.  The caller has waited for the last call that read d_ll.
int UploadLoglik(pk_mi355_decoder *d, const pk_decodable_t *src, int n) {
  int64_t total = 0;
  for (int i = 0; i < n; ++i) total += (int64_t)src[i].log_prob.ncol * d->num_pdfs;
  if ((size_t)total > d->d_ll_floats) {
    if (d->d_ll) hipFree(d->d_ll);
    d->d_ll = nullptr;
    d->d_ll_floats = 0;
    HIP_TRY(hipMalloc(&d->d_ll, sizeof(float) * (size_t)total));
    d->d_ll_floats = (size_t)total;
  }
  int64_t at = 0;
  for (int i = 0; i < n; ++i) {
    const pk_matrix_t &m = src[i].log_prob;
    const int64_t count = (int64_t)m.ncol * d->num_pdfs;
    if (count > 0)
      HIP_TRY(hipMemcpyAsync(d->d_ll + at, m.data, sizeof(float) * (size_t)count, hipMemcpyHostToDevice, d->own_stream));
    at += count;
  }
  return 0;
}

// Queue one decode of num_utts utterances whose log-likelihoods lie at ll + off[u] (T[u] frames each) on `stream`.
int Launch(pk_mi355_decoder *d, const float *ll, const std::vector<int64_t> &off, const std::vector<int> &T,
           hipStream_t stream) {
  const int n = (int)T.size();
  if (d->pending) HIP_TRY(hipEventSynchronize(d->done));   // the previous call's work areas are about to be reused
  d->pending = false; d->have = false; d->num_utts = n;
  d->h_T = T;
  d->h_off = off;
  d->stream = stream;
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
      hipLaunchKernelGGL(DecodeKernel<true>, dim3(n), dim3(kDecThreads), sizeof(float) * d->num_pdfs, stream, A);
      hipLaunchKernelGGL(GatherPathsKernel, dim3(n), dim3(256), 0, stream, d->d_res, n, d->path, reinterpret_cast<int *>(d->rec));
    } else {
      A.rec_cap = d->trace_cap; A.rec_top = d->counters;       // one arena and one path arena shared by the call
      A.path_cap = d->path_cap; A.path_top = reinterpret_cast<int *>(d->counters + 1);
      hipLaunchKernelGGL(DecodeKernel<false>, dim3(n), dim3(kDecThreads), sizeof(float) * d->num_pdfs, stream, A);
    }
    if (d->call_align) {
      AlignArgs G = {};
      G.res = d->d_res;
      // (with trace gc on GatherPathsKernel has moved the paths to the front of the record arena)
      G.path = d->call_gc ? reinterpret_cast<const int *>(d->rec) : d->path;
      G.path_cap = (int)d->trace_cap;
      G.arc_pdf = d->d_arc_pdf; G.num_arcs = (int)d->labels.ilabel.size();
      G.ll = ll; G.ll_off = d->d_off; G.T = d->d_T; G.frame_off = d->d_frame_off;
      G.num_pdfs = d->num_pdfs; G.num_utts = n;
      G.ali = d->d_ali; G.ac = d->d_ac; G.out = d->d_align;
      hipLaunchKernelGGL(AlignKernel, dim3(n), dim3(kDecThreads), 0, stream, G);
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
  // (with trace gc on GatherPathsKernel has moved the paths to the front of the record arena)
  const int *paths = d->call_gc ? reinterpret_cast<const int *>(d->rec) : d->path;
  if (used) HIP_TRY(hipMemcpy(d->h_path.data(), paths, sizeof(int) * used, hipMemcpyDeviceToHost));
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
  if (!fst || !am) { Fail(PK_MI355_E_INVALID, "null graph or model"); return nullptr; }
  if (!am->finalized) { Fail(PK_MI355_E_STATE, "model not finalized"); return nullptr; }
  if (max_utts <= 0 || trace_capacity < 0) { Fail(PK_MI355_E_INVALID, "bad decoder capacity"); return nullptr; }
  if (UseDevice(am->device)) return nullptr;
  pk_mi355_decoder *d = new pk_mi355_decoder();
  d->device = am->device;
  d->am = am;
  if (CreateDecoder(d, fst, am, max_utts, trace_capacity)) {
    FreeDecoderDevice(d);
    delete d;
    return nullptr;
  }
  return d;
}

void pk_mi355_decoder_destroy(pk_mi355_decoder_t *d) {
  if (!d) return;
  if (!UseDevice(d->device)) {
    if (d->pending) hipEventSynchronize(d->done);
    FreeDecoderDevice(d);
  }
  delete d;
}

int pk_mi355_decoder_set_beam(pk_mi355_decoder_t *d, float beam, int max_active) {
  if (!d) return Fail(PK_MI355_E_INVALID, "null decoder");
  if (!(beam >= 0.0f) || max_active <= 0) return Fail(PK_MI355_E_INVALID, "beam must be >= 0 and max_active > 0");
  d->beam = beam;
  d->max_active = max_active;
  return 0;
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

// ================================================================== online decoder (host)

struct pk_mi355_online_decoder {
  pk_mi355_decoder dec;                         // graph, work areas (one per slot), arenas (cap records per slot)
  int max_streams = 0;
  int64_t cap = 0;
  OnlineState *d_state = nullptr;
  OnlineResult *d_results = nullptr;
  int *d_remap = nullptr;
  OnlineCall *d_calls = nullptr;
  std::vector<int> open_, fresh, finished;      // per slot
  std::vector<OnlineResult> res;                // per slot, after synchronize
  std::vector<std::vector<int32_t>> paths;      // per slot: the arcs of res[slot]'s path
  std::vector<int> last_slots;                  // slots of the last call
  bool pending = false;
};

namespace {

int OnlineLaunch(pk_mi355_online_decoder *o, const float *ll, const std::vector<OnlineCall> &calls, hipStream_t stream) {
  pk_mi355_decoder *d = &o->dec;
  if (o->pending) HIP_TRY(hipEventSynchronize(d->done));
  o->pending = false;
  o->last_slots.clear();
  for (const auto &c : calls) o->last_slots.push_back(c.slot);
  const int n = (int)calls.size();
  if (n > 0) {
    HIP_TRY(hipMemcpyAsync(o->d_calls, calls.data(), sizeof(OnlineCall) * n, hipMemcpyHostToDevice, stream));
    // (frames, arenas and results are per slot: the calls, and o->cap entries of rec and path each)
    hipLaunchKernelGGL(OnlineDecodeKernel, dim3(n), dim3(kDecThreads), sizeof(float) * d->num_pdfs, stream, ArgsOf(d, ll, n),
                       o->d_calls, o->d_state, o->d_results, o->d_remap, o->cap);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return Fail(PK_MI355_E_DEVICE, "online decode launch: %s", hipGetErrorString(e));
  }
  for (const auto &c : calls) {
    o->fresh[c.slot] = 0;
    if (c.final_) { o->finished[c.slot] = 1; o->open_[c.slot] = 0; }
  }
  HIP_TRY(hipEventRecord(d->done, stream));
  o->pending = true;
  return 0;
}

int OnlineCollect(pk_mi355_online_decoder *o) {
  if (!o->pending) return 0;
  int rc = UseDevice(o->dec.device);
  if (rc) return rc;
  o->pending = false;
  HIP_TRY(hipEventSynchronize(o->dec.done));
  if (o->last_slots.empty()) return 0;
  HIP_TRY(hipMemcpy(o->res.data(), o->d_results, sizeof(OnlineResult) * o->max_streams, hipMemcpyDeviceToHost));
  int first_bad = -1;
  for (int slot : o->last_slots) {
    const OnlineResult &r = o->res[slot];
    if (r.path_len < 0 || r.path_len > o->cap) return Fail(PK_MI355_E_DEVICE, "online decoder: slot %d: corrupt result", slot);
    o->paths[slot].resize(r.path_len);
    if (r.path_len)
      HIP_TRY(hipMemcpy(o->paths[slot].data(), o->dec.path + (int64_t)slot * o->cap, sizeof(int32_t) * r.path_len,
                        hipMemcpyDeviceToHost));
    if (r.status && first_bad < 0) first_bad = slot;
  }
  if (first_bad >= 0) {
    const OnlineResult &r = o->res[first_bad];
    if (r.status == PK_MI355_E_CAPACITY)
      return Fail(PK_MI355_E_CAPACITY, "online decoder: slot %d: backtrace storage exhausted after compaction (%lld records "
                  "per slot)", first_bad, (long long)o->cap);
    return Fail(PK_MI355_E_INVALID, "online decoder: slot %d: negative epsilon cycle (the closure did not settle)", first_bad);
  }
  return 0;
}

int OnlineWords(const pk_mi355_online_decoder *o, int slot, int *words, int max_words) {
  return PathWords(o->dec.labels.olabel, o->paths[slot].data(), (int)o->paths[slot].size(), words, max_words);
}

int OnlineSlot(const pk_mi355_online_decoder *o, int slot) {
  if (!o) return Fail(PK_MI355_E_INVALID, "null online decoder");
  if (slot < 0 || slot >= o->max_streams) return Fail(PK_MI355_E_INVALID, "slot %d out of range [0, %d)", slot, o->max_streams);
  return 0;
}

}  // namespace

extern "C" {

pk_mi355_online_decoder_t *pk_mi355_online_decoder_create(const pk_mi355_fst_t *fst, const pk_mi355_am_t *am, int max_streams,
                                                          int64_t trace_capacity) {
  if (!fst || !am) { Fail(PK_MI355_E_INVALID, "null graph or model"); return nullptr; }
  if (!am->finalized) { Fail(PK_MI355_E_STATE, "model not finalized"); return nullptr; }
  if (max_streams <= 0 || trace_capacity < 0) { Fail(PK_MI355_E_INVALID, "bad online decoder capacity"); return nullptr; }
  const int64_t cap = trace_capacity > 0 ? trace_capacity : (int64_t)1 << 20;
  if (cap * max_streams > (int64_t)INT32_MAX) { Fail(PK_MI355_E_INVALID, "online decoder: max_streams x trace_capacity above 2^31 - 1"); return nullptr; }
  if (UseDevice(am->device)) return nullptr;
  pk_mi355_online_decoder *o = new pk_mi355_online_decoder();
  o->dec.device = am->device;
  o->dec.am = am;
  o->max_streams = max_streams;
  o->cap = cap;
  bool ok = CreateDecoder(&o->dec, fst, am, max_streams, cap * max_streams) == 0;
  auto chk = [&](hipError_t e) { if (e != hipSuccess && ok) { ok = false; Fail(PK_MI355_E_DEVICE, "online_decoder_create: %s", hipGetErrorString(e)); } };
  if (ok) chk(hipMalloc(&o->d_state, sizeof(OnlineState) * max_streams));
  if (ok) chk(hipMemset(o->d_state, 0, sizeof(OnlineState) * max_streams));
  if (ok) chk(hipMalloc(&o->d_results, sizeof(OnlineResult) * max_streams));
  if (ok) chk(hipMemset(o->d_results, 0, sizeof(OnlineResult) * max_streams));
  if (ok) chk(hipMalloc(&o->d_remap, sizeof(int) * cap * max_streams));
  if (ok) chk(hipMalloc(&o->d_calls, sizeof(OnlineCall) * max_streams));
  if (!ok) { pk_mi355_online_decoder_destroy(o); return nullptr; }
  o->open_.assign(max_streams, 0); o->fresh.assign(max_streams, 1); o->finished.assign(max_streams, 0);
  o->res.assign(max_streams, OnlineResult{});
  o->paths.assign(max_streams, {});
  return o;
}

void pk_mi355_online_decoder_destroy(pk_mi355_online_decoder_t *o) {
  if (!o) return;
  if (!UseDevice(o->dec.device)) {
    if (o->pending) hipEventSynchronize(o->dec.done);
    FreeDecoderDevice(&o->dec);
    hipFree(o->d_state); hipFree(o->d_results); hipFree(o->d_remap); hipFree(o->d_calls);
  }
  delete o;
}

int pk_mi355_online_decoder_set_beam(pk_mi355_online_decoder_t *o, float beam, int max_active) {
  if (!o) return Fail(PK_MI355_E_INVALID, "null online decoder");
  return pk_mi355_decoder_set_beam(&o->dec, beam, max_active);
}

int pk_mi355_online_decoder_open(pk_mi355_online_decoder_t *o, int slot) {
  int rc = OnlineSlot(o, slot);
  if (rc) return rc;
  if (o->open_[slot]) return Fail(PK_MI355_E_STATE, "online decoder: slot %d is open", slot);
  if ((rc = OnlineCollect(o))) return rc;       // a result of the slot's last utterance is replaced
  o->open_[slot] = 1; o->fresh[slot] = 1; o->finished[slot] = 0;
  o->res[slot] = OnlineResult{};
  o->paths[slot].clear();
  return 0;
}

int pk_mi355_online_decoder_advance_host(pk_mi355_online_decoder_t *o, const int *slots, const pk_decodable_t *chunks,
                                         const int *final_, int n, int sync) {
  if (!o || n < 0 || (n > 0 && (!slots || !chunks))) return Fail(PK_MI355_E_INVALID, "bad advance arguments");
  pk_mi355_decoder *d = &o->dec;
  int rc = UseDevice(d->device);
  if (rc) return rc;
  std::vector<char> seen(o->max_streams, 0);
  int64_t total = 0;
  std::vector<OnlineCall> calls(n);
  for (int i = 0; i < n; ++i) {
    const int slot = slots[i];
    if ((rc = OnlineSlot(o, slot))) return rc;
    if (!o->open_[slot]) return Fail(PK_MI355_E_STATE, "online decoder: slot %d is not open", slot);
    if (seen[slot]) return Fail(PK_MI355_E_INVALID, "online decoder: slot %d twice in one call", slot);
    seen[slot] = 1;
    const pk_matrix_t &m = chunks[i].log_prob;
    if ((rc = CheckLoglik(d, m, "online decoder: chunk", i))) return rc;
    calls[i] = OnlineCall{slot, m.ncol, final_ && final_[i] ? 1 : 0, o->fresh[slot], total};
    total += (int64_t)m.ncol * d->num_pdfs;
  }
  if (o->pending) HIP_TRY(hipEventSynchronize(d->done));     // d_ll may still be read by the previous call
  if ((rc = UploadLoglik(d, chunks, n))) return rc;
  if ((rc = OnlineLaunch(o, d->d_ll, calls, d->own_stream))) return rc;
  return sync ? OnlineCollect(o) : 0;
}

int pk_mi355_online_decoder_advance(pk_mi355_online_decoder_t *o, pk_mi355_stream_t *s, int sync) {
  if (!o || !s) return Fail(PK_MI355_E_INVALID, "null online decoder or stream");
  if (StreamModel(s) != o->dec.am)
    return Fail(PK_MI355_E_INVALID, "online decoder: the stream scores with another model than the decoder was created for");
  if (StreamSlots(s) > o->max_streams) return Fail(PK_MI355_E_INVALID, "online decoder: the stream has more slots than the decoder");
  int rc = UseDevice(o->dec.device);
  if (rc) return rc;
  std::vector<OnlineCall> calls;
  const float *base = StreamLoglikBase(s);
  for (int slot = 0; slot < StreamSlots(s); ++slot) {
    if (!o->open_[slot]) continue;
    int first = 0, count = 0;
    const float *p = pk_mi355_stream_loglik_device(s, slot, &first, &count);
    const bool fin = StreamSlotFlushed(s, slot);
    if (count == 0 && !fin) continue;
    calls.push_back(OnlineCall{slot, count, fin ? 1 : 0, o->fresh[slot], count ? (int64_t)(p - base) : 0});
  }
  if ((rc = OnlineLaunch(o, base, calls, StreamHipStream(s)))) return rc;
  return sync ? OnlineCollect(o) : 0;
}

int pk_mi355_online_decoder_synchronize(pk_mi355_online_decoder_t *o) {
  if (!o) return Fail(PK_MI355_E_INVALID, "null online decoder");
  return OnlineCollect(o);
}

int pk_mi355_online_decoder_partial(const pk_mi355_online_decoder_t *o, int slot, int *words, int max_words, float *cost) {
  int rc = OnlineSlot(o, slot);
  if (rc) return rc;
  if (o->pending) return Fail(PK_MI355_E_STATE, "online decoder: synchronize first");
  if (cost) *cost = o->res[slot].weight;
  return OnlineWords(o, slot, words, max_words);
}

int pk_mi355_online_decoder_result(const pk_mi355_online_decoder_t *o, int slot, int *words, int max_words, float *weight,
                                   int *ok) {
  int rc = OnlineSlot(o, slot);
  if (rc) return rc;
  if (o->pending) return Fail(PK_MI355_E_STATE, "online decoder: synchronize first");
  if (!o->finished[slot] || !o->res[slot].final_) return Fail(PK_MI355_E_STATE, "online decoder: slot %d is not finished", slot);
  if (weight) *weight = o->res[slot].weight;
  if (ok) *ok = o->res[slot].ok;
  return OnlineWords(o, slot, words, max_words);
}

int pk_mi355_online_decoder_best_path_arcs(const pk_mi355_online_decoder_t *o, int slot, int32_t *arcs, int max_arcs) {
  int rc = OnlineSlot(o, slot);
  if (rc) return rc;
  if (o->pending) return Fail(PK_MI355_E_STATE, "online decoder: synchronize first");
  const auto &p = o->paths[slot];
  for (int i = 0; i < (int)p.size() && i < max_arcs; ++i) arcs[i] = p[i];
  return (int)p.size();
}

int pk_mi355_online_decoder_word_segments(const pk_mi355_online_decoder_t *o, int slot, pk_mi355_word_t *out, int max) {
  int rc = OnlineSlot(o, slot);
  if (rc) return rc;
  if (o->pending) return Fail(PK_MI355_E_STATE, "online decoder: synchronize first");
  const auto &p = o->paths[slot];
  return WordSegments(o->dec.labels, p.data(), (int)p.size(), nullptr, 0, out, max);   // (the rows are gone: no acoustic cost)
}

int pk_mi355_online_decoder_active_bound(const pk_mi355_online_decoder_t *o, int slot) {
  int rc = OnlineSlot(o, slot);
  if (rc) return rc;
  if (o->pending) return Fail(PK_MI355_E_STATE, "online decoder: synchronize first");
  return o->res[slot].active_bound;
}

}  // extern "C"
