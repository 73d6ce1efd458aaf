// decode.hip -- the search half of pk_process (Decoder::Decode + BestPath, decoder.cc:39-339) on the GPU,
// batched: one workgroup per utterance decodes the whole utterance in ONE launch, frame after frame,
// synchronising only with __syncthreads() (no workgroup waits on another).  Device code and its launchers only
// (pk_decode.h): the host objects are capi_decoder.hip and capi_online_decoder.hip; the graph's reader and its split
// into the arc lists below are host-only: pk_files.cc.
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

#include "pk_decode.h"

using namespace pkhost;

namespace {

constexpr int kDecThreads = 512;
constexpr int kDecWaves = kDecThreads / 64;
constexpr uint32_t kStartId = 0x7FFFFFFFu;         // the start token's id (never resolved: it has no arc)
constexpr uint64_t kEmpty = ~0ull;

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
  float *ac;                    // kAc only: a record's acoustic cost, parallel to rec (null otherwise, never read)
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
// kAc (pk_mi355_online_decoder_set_alignment): the record also keeps its acoustic cost, -s_ll[pdf of the winning arc]
// (s_ll: the frame's row as staged, N1 applied -- the bits AlignKernel writes), 0 for an epsilon arc.
template <bool kAc>
__device__ int Resolve(Shared &sh, const float *s_ll, const DecArgs &A, const Arena &R, const int *states, int n, float F,
                       bool eps, uint64_t *key, int *tr, int *mark, Tok *out) {
  int written = 0;
  for (int c0 = 0; c0 < n; c0 += kDecThreads) {
    const int i = c0 + threadIdx.x;
    int need = 0, s = 0, prev = -1, arc = -1;
    float c = 0.f;
    [[maybe_unused]] float ac = 0.0f;
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
          if constexpr (kAc) ac = -s_ll[A.e_arc[id].y];
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
      if constexpr (kAc) R.ac[r] = ac;
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
template <bool kAc, typename Before>
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
      nF = Resolve<kAc>(sh, s_ll, A, w.arena, touched, nT, F, false, key, tr, mark, fa);
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
      nF = Resolve<kAc>(sh, s_ll, A, w.arena, nxt, nN, F, true, key, tr, mark, fb);
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
// kAc: the records' acoustic costs beside their arcs (path_ac is not read otherwise)
template <bool kAc>
__device__ __forceinline__ void FillPath(const Arena &R, int trace, int *path, [[maybe_unused]] float *path_ac, int len) {
  for (int x = trace; x >= 0 && len > 0; x = R.rec[x].x) {
    path[--len] = R.rec[x].y;
    if constexpr (kAc) path_ac[len] = R.ac[x];
  }
}

// The trace compaction, three passes.  Count: every token walks from its record towards the root adding 1 to remap[x]
// and goes on only where it was the first to arrive, so remap[x] = (reachable children of x) + (tokens at x) and every
// reachable record is visited by one walker.  Rank: the reachable records are numbered in creation order with a chunked
// exclusive scan (a record's predecessor is always older, so one forward pass remaps every `prev`).  Move: they go
// down to their rank, and the tokens' trace (and the state table's, which the next emitting step reads) is rewritten.
// Changes where records live, never a result.  kAc: R.ac[i] moves wherever rec[i] does.
// kCommit = false, the compaction inside a launch: every reachable record stays (b = 0); remap is trusted, nothing is
// checked, path and path_ac are not read, and 0 is returned.
// kCommit = true, the commit mode's end of a launch (pk_mi355_online_decoder_set_commit): with one root and no token at
// the start (trace < 0), b = the lowest index that either carries a count >= 2 or is a token's own record is the last
// record every path shares: a predecessor is always older and compaction keeps creation order, so everything off the
// trunk -- a descendant of the first branching record -- has a higher index than it, and the reachable records below b
// ARE the trunk, in path order.  Those go, in that order, to path[0, nc) (their costs to path_ac with kAc); the rest
// moves down, b to index 0 with prev = -1.  Otherwise b = 0 and this is the plain compaction.  Every index read from
// memory is checked against the arena's top before it is used.  Returns nc (all threads), or -1 when the records are
// inconsistent.
constexpr int kCommitNone = 1, kCommitBad = 2;       // sh.fail: a token at the start; an index out of range

template <bool kAc, bool kCommit>
__device__ int CompactTrace(Shared &sh, const Arena &R, int *remap, Tok *L, int nL, int *tr, [[maybe_unused]] int *path,
                            [[maybe_unused]] float *path_ac) {
  int2 *rec = R.rec;
  const unsigned long long top = *R.top;
  __syncthreads();
  if constexpr (kCommit) {
    if (top > (unsigned long long)R.cap) return -1;
  }
  const int n = (int)top;
  for (int i = threadIdx.x; i < n; i += kDecThreads) remap[i] = 0;
  if constexpr (kCommit) {
    if (threadIdx.x == 0) { sh.cnt_nxt = 0; sh.fail = 0; sh.sel = 0; }   // roots; flags; nc
  }
  __syncthreads();
  [[maybe_unused]] uint64_t lo = kEmpty;
  for (int j = threadIdx.x; j < nL; j += kDecThreads) {
    int x = L[j].trace;
    if constexpr (kCommit) {
      if (x < 0) { atomicOr(&sh.fail, kCommitNone); continue; }
      if (x >= n) { atomicOr(&sh.fail, kCommitBad); continue; }
      lo = min(lo, (uint64_t)x);
    }
    while (x >= 0 && atomicAdd(&remap[x], 1) == 0) {
      const int p = rec[x].x;
      if constexpr (kCommit) {
        if (p < 0) atomicAdd(&sh.cnt_nxt, 1);
        else if (p >= x) { atomicOr(&sh.fail, kCommitBad); break; }     // (older, so in range; and the walk ends)
      }
      x = p;
    }
  }
  __syncthreads();
  int b = 0;
  if constexpr (kCommit) {
    for (int i = threadIdx.x; i < n; i += kDecThreads)
      if (__hip_atomic_load(&remap[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 2) { lo = min(lo, (uint64_t)i); break; }
    lo = BlockMinU(sh, lo);
    const int flags = sh.fail;
    if (flags & kCommitBad) return -1;
    if (sh.cnt_nxt == 1 && !flags && lo != kEmpty) b = (int)lo;
  }
  int base = 0;
  for (int c0 = 0; c0 < n; c0 += kDecThreads) {
    const int i = c0 + threadIdx.x;
    const int alive = i < n ? __hip_atomic_load(&remap[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0 : 0;   // set by atomics
    int2 r = make_int2(-1, -1);
    [[maybe_unused]] float ac = 0.0f;
    if (alive) {
      r = rec[i];
      if constexpr (kAc) ac = R.ac[i];
    }
    int total;
    const int g = base + BlockScan(sh, alive, &total);   // rank among the reachable: trunk first, b at nc
                                                         // (its barriers: every read of this chunk is done)
    int nc = 0;
    if constexpr (kCommit) {
      if (alive && i == b) sh.sel = g;
      __syncthreads();
      nc = i >= b ? sh.sel : 0;
    }
    if (i < n) remap[i] = (alive && i >= b) ? g - nc : -1;
    __syncthreads();
    if (alive) {
      if (kCommit && i < b) {
        path[g] = r.y;
        if constexpr (kAc) path_ac[g] = ac;
      } else {
        r.x = (!(kCommit && i == b) && r.x >= 0) ? remap[r.x] : -1;   // older: remapped in this chunk or an earlier one
        rec[g - nc] = r;
        if constexpr (kAc) R.ac[g - nc] = ac;
      }
    }
    base += total;
    __syncthreads();
  }
  const int nc = kCommit ? sh.sel : 0;
  for (int j = threadIdx.x; j < nL; j += kDecThreads) {
    const int x = L[j].trace;
    if (x >= 0) {
      L[j].trace = remap[x];
      tr[L[j].state] = remap[x];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) *R.top = (unsigned long long)(base - nc);
  __syncthreads();
  return nc;
}

// What DecodeKernel<true> and OnlineDecodeKernel run before an emitting frame: a slice more than half full is compacted.
template <bool kAc>
__device__ __forceinline__ bool CompactIfHalfFull(Shared &sh, const Arena &R, int *remap, Tok *L, int nL, int *tr) {
  if (*R.top <= (unsigned long long)(R.cap / 2)) return false;
  CompactTrace<kAc, false>(sh, R, remap, L, nL, tr, nullptr, nullptr);
  return true;
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
    w = WorkOf(A, u, Arena{A.rec + at, A.rec_cap, &s_top, nullptr});
    int *remap = A.path + at;
    DecodeFrames<false>(sh, s_ll, A, w, A.ll + A.ll_off[u], -1, A.T[u], [&](Tok *L, int nL) {
      peak = max(peak, (int)s_top);
      compactions += CompactIfHalfFull<false>(sh, w.arena, remap, L, nL, w.tr);
    });
    peak = (int)min((unsigned long long)A.rec_cap, max((unsigned long long)peak, s_top));   // (a failed bump overshoots)
  } else {
    w = WorkOf(A, u, Arena{A.rec, A.rec_cap, A.rec_top, nullptr});
    DecodeFrames<false>(sh, s_ll, A, w, A.ll + A.ll_off[u], -1, A.T[u], [](Tok *, int) {});
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
          FillPath<false>(w.arena, w.L[bi].trace, A.path + r.path_off, nullptr, len);
        }
      } else {
        const int off = atomicAdd(A.path_top, len);    // the call's shared path arena
        if (off + len > A.path_cap) {                  // (cannot happen: see CreateDecoder)
          r.status = PK_MI355_E_CAPACITY;
          r.ok = 0;
        } else {
          r.path_off = off; r.path_len = len;
          FillPath<false>(w.arena, w.L[bi].trace, A.path + off, nullptr, len);
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
// (A.rec, A.path and A.remap hold cap = A.rec_cap entries per slot); when it is more than half full before an emitting
// frame the reachable records are compacted (CompactTrace).  The compaction, the frame count and the list-buffer parity
// are all this kernel adds to the frame step: DecodeKernel<false> instantiates it with an empty `before` and never
// reads them.
// kAc (pk_mi355_online_decoder_set_alignment): A.rec_ac and A.path_ac, `cap` floats per slot, run parallel to the slot's
// records and path -- a frame's acoustic cost is kept when the frame is decoded, since its row is void afterwards.
// kCommit (pk_mi355_online_decoder_set_commit): the slot's path slice ends the launch with A.commit_len[slot] newly
// committed arcs followed by the result's path_len arcs of the best token's tail, and st.peak is kept.
// A mode that is off reads none of its pointers and writes neither A.commit_len nor st.peak.

template <bool kAc, bool kCommit>
__global__ void __launch_bounds__(kDecThreads) OnlineDecodeKernel(DecArgs A, const OnlineCall *calls, OnlineState *states,
                                                                    OnlineResult *results) {
  extern __shared__ float s_ll[];
  __shared__ Shared sh;
  const OnlineCall call = calls[blockIdx.x];
  const int u = call.slot;
  const int64_t cap = A.rec_cap, at = (int64_t)u * cap;      // the slot's own arena, and where its slices begin
  OnlineState st = states[u];
  if (call.fresh) {
    st.nL = 0; st.par = 0; st.ok = 1; st.status = 0; st.active = 0; st.frames = 0; st.started = 0; st.peak = 0; st.top = 0;
  }
  __shared__ unsigned long long s_top;
  if (threadIdx.x == 0) s_top = st.top;
  __syncthreads();
  Work w = WorkOf(A, u, Arena{A.rec + at, cap, &s_top, kAc ? A.rec_ac + at : nullptr});
  int *remap = A.remap + at;
  int *path = A.path + at;
  [[maybe_unused]] float *path_ac = kAc ? A.path_ac + at : nullptr;
  [[maybe_unused]] unsigned long long peak = (unsigned long long)st.peak;   // kCommit: the most the arena held since open
  if (st.par) { Tok *x = w.L; w.L = w.Lnext; w.Lnext = x; }
  w.nL = st.nL; w.status = st.status; w.ok = st.ok; w.active = st.active; w.frames = st.frames; w.par = st.par;
  if (!w.status && w.ok)
    DecodeFrames<kAc>(sh, s_ll, A, w, A.ll + call.ll_off, st.started ? 0 : -1, call.T, [&](Tok *L, int nL) {
      [[maybe_unused]] const unsigned long long top = s_top;
      if (CompactIfHalfFull<kAc>(sh, w.arena, remap, L, nL, w.tr)) {
        if constexpr (kCommit) peak = max(peak, top);
      }
    });
  const bool fin = call.final_ != 0;
  // kCommit: the arcs every token's path shares, but the last, leave the arena for the front of the slot's path (not in
  // the launch that finishes the slot, and not for a slot that has ended); the best token's tail follows them below
  int nc = 0;
  if constexpr (kCommit) {
    peak = max(peak, s_top);
    if (!w.status && w.ok && !fin && w.nL > 0) {
      nc = CompactTrace<kAc, true>(sh, w.arena, remap, w.L, w.nL, w.tr, path, path_ac);
      if (nc < 0) { w.status = PK_MI355_E_DEVICE; nc = 0; }
    }
  }
  // the path of the best token: BestPath's once the slot is closed, the partial hypothesis' otherwise
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
      const int len = PathLen(w.arena, w.L[bi].trace);
      // kCommit: the committed arcs and the tail are distinct records reachable before the commit, so together they fit
      // the slice; with nc = 0 the check is vacuous (a chain of the arena's records), and it is not compiled
      if (kCommit && (int64_t)nc + len > cap) {
        w.status = r.status = PK_MI355_E_DEVICE;
        r.ok = 0; r.weight = 0.f;
        nc = 0;
      } else {
        r.path_len = len;
        FillPath<kAc>(w.arena, w.L[bi].trace, path + nc, kAc ? path_ac + nc : nullptr, len);
        r.has_path = 1;
      }
    }
    if constexpr (kCommit) {
      A.commit_len[u] = nc;
      st.peak = (int)min((unsigned long long)cap, max(peak, s_top));        // (a failed bump overshoots)
    }
    results[u] = r;
    st.nL = w.nL; st.par = w.par; st.ok = w.ok; st.status = w.status; st.active = w.active; st.frames = w.frames;
    st.started = 1; st.top = s_top;
    states[u] = st;
  }
}

// ================================================================== endpointing (pk_mi355_online_decoder_set_endpointing)
// After OnlineDecodeKernel on the same stream, over the same calls, one workgroup per call entry: what the endpoint
// rules need of a slot that is still live (its launch was not final, status == 0, ok, nL > 0); any other slot gets
// valid = 0.  A kernel of its own, so that the decode kernels' code is the same with the mode on, off or never built.
//   * relative cost: over the slot's token list as the decode launch left it, m_best = min (double)cost and
//     m_fin = min (double)cost + (double)final over the tokens where that sum is not INFINITY (BestPath's test);
//     relative_cost = (float)(m_fin - m_best), +inf without a final token.
//   * trailing silence: over the best token's path as the decode launch wrote it (behind the newly committed arcs with
//     commit on), in chunks of the workgroup's width: a wave ballots "emits" and "emits a non-silence pdf", its lane 0
//     leaves (emitting arcs, has a non-silent one, emitting arcs after the last non-silent one) in LDS, and every thread
//     folds the waves in path order into the carry (frames, silence run, still open).
// Every arc id is checked against the table before it indexes it, and the slice's lengths against the slot's capacity.
__global__ void __launch_bounds__(kDecThreads) EndpointKernel(EndpointArgs E) {
  __shared__ Shared sh;
  __shared__ int s_wave[kDecWaves][3];
  __shared__ int s_bad;
  if ((int)blockIdx.x >= E.n) return;
  const OnlineCall call = E.calls[blockIdx.x];
  const int u = call.slot;
  const OnlineState st = E.states[u];
  const OnlineResult r = E.results[u];
  EndpointRecord o;
  o.valid = 0; o.status = 0; o.num_final = 0; o.tail_silence = 0; o.tail_open = 0; o.tail_frames = 0;
  o.best_cost = 0.f; o.final_cost = 0.f; o.relative_cost = 0.f; o.pad = 0;
  const bool live = !call.final_ && !st.status && st.ok && st.nL > 0 && st.nL <= E.num_states;
  if (!live) {                                          // (the same verdict in every thread)
    if (threadIdx.x == 0) E.out[u] = o;
    return;
  }
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  // ---- the best token and the best final token
  const Tok *L = (st.par ? E.lb : E.la) + (size_t)E.num_states * u;
  double m_best = INFINITY, m_fin = INFINITY;
  int finals = 0;
  for (int i = threadIdx.x; i < st.nL; i += kDecThreads) {
    const Tok tk = L[i];
    if (tk.state < 0 || tk.state >= E.num_states) { s_bad = 1; continue; }
    const double c = (double)tk.cost;
    m_best = fmin(m_best, c);
    const double f = c + (double)E.final_w[tk.state];
    if (f != INFINITY) { m_fin = fmin(m_fin, f); ++finals; }
  }
  m_best = BlockMinD(sh, m_best);
  m_fin = BlockMinD(sh, m_fin);
  int num_final;
  BlockScan(sh, finals, &num_final);
  // ---- the silence at the end of the best token's path
  const int nc = E.commit_len ? E.commit_len[u] : 0;
  const bool inside = nc >= 0 && r.path_len >= 0 && (int64_t)nc + r.path_len <= E.cap;
  int frames = 0, run = 0, open = 1;
  if (inside) {
    const int *path = E.path + (int64_t)u * E.cap + nc;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int c0 = 0; c0 < r.path_len; c0 += kDecThreads) {
      const int i = c0 + threadIdx.x;
      int pdf = -1;
      if (i < r.path_len) {
        const int arc = path[i];
        if (arc >= 0 && arc < E.num_arcs) pdf = E.arc_pdf[arc];
        else s_bad = 1;
      }
      const int emits = pdf >= 0;
      int silent = 0;
      if (emits) {
        if (pdf < E.num_pdfs) silent = (E.silence[pdf >> 5] >> (pdf & 31)) & 1u;
        else s_bad = 1;
      }
      const unsigned long long em = __ballot(emits), nm = __ballot(emits && !silent);
      if (lane == 0) {
        // (the lanes above the last non-silent one: bits last + 1 .. 63)
        const int last = nm ? 63 - __clzll((long long)nm) : -1;
        const unsigned long long after = last < 0 ? em : last == 63 ? 0ull : em & (~0ull << (last + 1));
        s_wave[wv][0] = __popcll(em);
        s_wave[wv][1] = nm != 0;
        s_wave[wv][2] = __popcll(after);
      }
      __syncthreads();
      for (int k = 0; k < kDecWaves; ++k) {
        frames += s_wave[k][0];
        if (s_wave[k][1]) { run = s_wave[k][2]; open = 0; }
        else run += s_wave[k][2];
      }
      __syncthreads();
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (!inside || s_bad) {
      o.status = PK_MI355_E_DEVICE;
    } else {
      o.valid = 1;
      o.num_final = num_final;
      o.tail_silence = run; o.tail_open = open; o.tail_frames = frames;
      o.best_cost = (float)m_best;
      o.final_cost = num_final ? (float)m_fin : INFINITY;
      o.relative_cost = num_final ? (float)(m_fin - m_best) : INFINITY;
    }
    E.out[u] = o;
  }
}
}  // namespace

// ================================================================== launchers (pk_decode.h)

namespace pkmi {

void LaunchDecode(const DecArgs &A, bool trace_gc, hipStream_t stream) {
  if (trace_gc)
    hipLaunchKernelGGL(DecodeKernel<true>, dim3(A.num_utts), dim3(kDecThreads), sizeof(float) * A.num_pdfs, stream, A);
  else
    hipLaunchKernelGGL(DecodeKernel<false>, dim3(A.num_utts), dim3(kDecThreads), sizeof(float) * A.num_pdfs, stream, A);
}

void LaunchGatherPaths(UttResult *res, int n, const int *path, int *out, hipStream_t stream) {
  hipLaunchKernelGGL(GatherPathsKernel, dim3(n), dim3(256), 0, stream, res, n, path, out);
}

void LaunchAlign(const AlignArgs &A, hipStream_t stream) {
  hipLaunchKernelGGL(AlignKernel, dim3(A.num_utts), dim3(kDecThreads), 0, stream, A);
}

void LaunchOnlineDecode(const DecArgs &A, const OnlineCall *calls, OnlineState *states, OnlineResult *results, int n,
                        hipStream_t stream) {
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(n), dim3(kDecThreads), sizeof(float) * A.num_pdfs, stream, A, calls, states, results);
  };
  if (A.commit_len) {
    if (A.rec_ac && A.path_ac) launch(OnlineDecodeKernel<true, true>); else launch(OnlineDecodeKernel<false, true>);
  } else {
    if (A.rec_ac && A.path_ac) launch(OnlineDecodeKernel<true, false>); else launch(OnlineDecodeKernel<false, false>);
  }
}

void LaunchEndpoint(const EndpointArgs &E, hipStream_t stream) {
  hipLaunchKernelGGL(EndpointKernel, dim3(E.n), dim3(kDecThreads), 0, stream, E);
}

}  // namespace pkmi
