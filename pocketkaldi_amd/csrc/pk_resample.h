// pk_resample.h -- sample-rate conversion to 16 kHz: the polyphase table (built on the host, pk_tables.cc, no HIP),
// the per-item plan of ResampleKernel and its launcher (resample.hip).  DESIGN.md section 11 states the rule.
//
// Output rate fo = 16000, input rate fi, g = gcd(fi, fo), Q = fi / g input samples per unit, P = fo / g phases.
// Output j = u P + p reads the count[p] inputs from base = first[p] + u Q on:
//     y[j] = sum over k < count[p], ascending, of weight[p][k] * x[base + k]      (fp32, from +0.0f, product then add)
// with x outside [0, N_in) read as +0.0f.  N_out = floor(N_in P / Q).
#ifndef PK_RESAMPLE_H_
#define PK_RESAMPLE_H_

#include <stdint.h>

#include <vector>

namespace pkmi {

constexpr int kResampleOutRate = 16000;
constexpr int kResampleMinRate = 8000, kResampleMaxRate = 96000;
constexpr int kResampleMaxEntries = 16384;   // P x max_taps: a 64 KiB table, staged in LDS beside an input span
constexpr int kResampleTile = 1024;          // outputs of one item a workgroup converts between two barriers
constexpr int kResampleThreads = 256;

struct ResampleTable {
  int rate = 0, Q = 0, P = 0, max_taps = 0;
  int min_first = 0, max_end = 0;            // min first[p] and max first[p] + count[p]: every window lies in [u Q + min_first, u Q + max_end)
  std::vector<int32_t> first, count;         // [P]
  std::vector<float> weights;                // [P][max_taps], rows zero-padded behind count[p]
  // the longest input span a tile of kResampleTile outputs reads (what the kernel stages per tile)
  int Span() const { return ((kResampleTile - 1) / P + 1) * Q + (max_end - min_first); }
};

// 0, or -1 for a rate outside [8000, 96000] or whose table exceeds kResampleMaxEntries (rate 16000: Q = P = 1 and one
// tap of weight one -- callers copy instead).  Pure host code, no HIP; weights in double, rounded to float once.
int BuildResampleTable(int rate, ResampleTable *t);
// floor(n P / Q) in 64-bit integers
inline int64_t ResampleNumOutput(const ResampleTable &t, int64_t n) { return n <= 0 ? 0 : n * t.P / t.Q; }
// The outputs that are final once n inputs have arrived: the first j whose window does not end below n
// (base + count[p] - 1 >= n); never more than ResampleNumOutput.
int64_t ResampleNumFinal(const ResampleTable &t, int64_t n);

// One item of a launch: outputs [j0, j1) of a signal whose samples [x0, x0 + n_valid) lie at x[0 .. n_valid).
// Samples outside that range read as +0.0f.  y[0] receives output j0.
struct ResampleItem {
  const float *x;
  int64_t x0;
  int64_t n_valid;
  int64_t j0, j1;
  float *y;
  // the item's table, in device memory: first[P], count[P], weights[P][max_taps]
  const int32_t *first;
  const int32_t *count;
  const float *weights;
  int32_t Q, P, max_taps, min_first, max_end;
  int32_t span;                              // LDS floats this item's tiles need (ResampleTable::Span)
};

#ifdef __HIPCC__
// d_items: num_items plans in device memory; max_tiles: the most tiles any item has; lds_bytes: the largest item's
// table + span.  The host has checked every plan and table entry (capi_resample.hip).
void LaunchResample(const ResampleItem *d_items, int num_items, int64_t max_tiles, size_t lds_bytes, hipStream_t stream);
// LDS bytes of one item's workgroup: weights (row stride max_taps | 1), first, count, span
inline size_t ResampleLdsBytes(int P, int max_taps, int span) {
  return sizeof(float) * ((size_t)P * (max_taps | 1) + (size_t)span) + sizeof(int32_t) * 2 * (size_t)P;
}
// a launch whose LDS exceeds 64 KiB must be allowed first (hipFuncSetAttribute); returns the hipError_t as int
int ResampleAllowLds(size_t lds_bytes);
#endif

}  // namespace pkmi

#ifdef __HIPCC__
namespace pkhost {

// A rate's table in device memory.
struct DeviceResampleTable {
  pkmi::ResampleTable host;
  int32_t *d_first = nullptr, *d_count = nullptr;
  float *d_weights = nullptr;
};

// What an object that converts audio owns (capi_resample.hip): the tables of the rates it has met, built on first use
// and kept, and the plan buffers of a launch (page-locked and device).  One host thread at a time, like its owner.
struct Resampler {
  std::vector<DeviceResampleTable *> tables;
  pkmi::ResampleItem *h_items = nullptr, *d_items = nullptr;
  int items_cap = 0;
  hipEvent_t uploaded = nullptr;     // the last launch's plan has left h_items
  size_t lds_allowed = 65536;

  // PK_MI355_E_INVALID (naming the rate) for an unsupported rate
  int Table(int rate, const DeviceResampleTable **out);
  // a plan over table t with the table fields filled in
  static pkmi::ResampleItem Item(const DeviceResampleTable &t, const float *x, int64_t x0, int64_t n_valid, int64_t j0, int64_t j1,
                                 float *y);
  // checks every plan, uploads them and launches on `stream` (nothing for an empty list)
  int Run(const std::vector<pkmi::ResampleItem> &items, hipStream_t stream);
  void Free();
};

}  // namespace pkhost
#endif

#endif  // PK_RESAMPLE_H_
