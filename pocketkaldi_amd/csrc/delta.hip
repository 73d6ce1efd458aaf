// delta.hip -- DeltaKernel: delta features, Kaldi's add-deltas (include/pk_mi355.h states the rule; DESIGN.md section
// 21).  It stands between the normalisation (NormKernel, OnlineCmvnKernel, CmvnChainKernel, or the raw rows in mode
// none) and FeatureLayoutKernel on a batch made by pk_mi355_deltas_batch_create: rows [sum T][Db] in, rows
// [sum T][(order + 1) Db] out, never in place.
//
// Shaped like NormKernel: lane = feature, so per frame the wave reads ONE contiguous run of up to 64 floats and writes
// order + 1 of them.  One wavefront per (utterance, run of kDeltaFrames frames, block of 64 base features):
//   Stage: the G + 2 M rows the run's outputs read (M = order * window, frames t0 - M .. t0 + G - 1 + M, each clamped
//     into the utterance's own rows: the edge rule is applied here, once) go to LDS as lane-private columns --
//     s_x[row][lane], which every lane writes and reads at its own lane only, so the wave needs no barrier and the
//     accesses are free of bank conflicts.  The loads are independent and are issued a group at a time.
//   Apply: for every block i the host's pkdelta::DeltaApply (pk_delta.h), instantiated on a run of G frames held in
//     registers: per tap ONE wave-uniform scale from the device table (a scalar load; a zero scale skips the tap for
//     the whole wave) and G products and adds per lane, j ascending for every frame -- each output's own chain is the
//     host's, operation for operation.  Then G coalesced stores of the block.
// Every address is formed from t clamped into [0, T) and d clamped into [d0, Db): a load past the utterance's rows or
// past feature Db - 1 is never issued, so a poisoned neighbour is never read; a lane past Db shadows the block's first
// feature and stores nothing; a run that starts behind the utterance's last frame returns before it touches memory.
//
// StreamDeltaKernel, further down, is the same stage and apply for a live slot of a stream made by
// pk_mi355_deltas_stream_create: the frames below the step's fresh rows come from the slot's ring.
#include <hip/hip_runtime.h>

#include "pk_delta_kernel.h"

namespace pkmi {

namespace {

constexpr int kG = kDeltaFrames;

// The run of G frames of one column that a lane holds: what DeltaApply's float is on the host.
struct FrameRun {
  float v[kG];
  __device__ explicit FrameRun(float x) {
#pragma unroll
    for (int f = 0; f < kG; ++f) v[f] = x;
  }
  __device__ FrameRun() {}
};
__device__ inline FrameRun operator*(float s, const FrameRun &x) {
  FrameRun p;
#pragma unroll
  for (int f = 0; f < kG; ++f) p.v[f] = s * x.v[f];
  return p;
}
__device__ inline FrameRun operator+(const FrameRun &a, const FrameRun &b) {
  FrameRun r;
#pragma unroll
  for (int f = 0; f < kG; ++f) r.v[f] = a.v[f] + b.v[f];
  return r;
}

__global__ __launch_bounds__(64) void DeltaKernel(const float *__restrict__ in, UttLayout utts, int num_utts, int Db, int order, int window,
                                                  const float *__restrict__ scales, float *__restrict__ out) {
  extern __shared__ float s_x[];                      // [kG + 2 M][64]
  const int lane = threadIdx.x;
  const int t0 = blockIdx.x * kG;
  const int d0 = blockIdx.y * 64;
  const bool live = d0 + lane < Db;
  const int d = live ? d0 + lane : d0;
  const int M = order * window, L = 2 * M + 1;
  const int64_t F = (int64_t)(order + 1) * Db;
  for (int u = blockIdx.z; u < num_utts; u += gridDim.z) {          // (uniform over the wave)
    const int T = utts.num_frames[u];
    if (t0 >= T) continue;
    const float *x = in + utts.raw_base[u] * Db + d;
    float *y = out + utts.raw_base[u] * F + d;
    const int rows = kG + 2 * M;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) {
      const int t = t0 - M + r;
      s_x[r * 64 + lane] = x[(int64_t)(t < 0 ? 0 : t < T ? t : T - 1) * Db];
    }
    for (int i = 0; i <= order; ++i) {
      const FrameRun acc = pkdelta::DeltaApply<FrameRun>(scales + i * L + M, i * window, [&](int j) {
        FrameRun r;
#pragma unroll
        for (int f = 0; f < kG; ++f) r.v[f] = s_x[(f + M + j) * 64 + lane];
        return r;
      });
      if (live) {
#pragma unroll
        for (int f = 0; f < kG; ++f)
          if (t0 + f < T) y[(int64_t)(t0 + f) * F + (int64_t)i * Db] = acc.v[f];
      }
    }
  }
}

// The deltas of a live slot: DeltaKernel's stage and apply, with the frames below the step's
// fresh rows taken from the slot's ring.  One wavefront per (record, run of G of the record's newly final delta frames,
// block of 64 base features), lane = feature.  Delta frame t reads the normalised base frames clamp(t + j, 0, n - 1):
// frame f from the step's fresh rows when f >= n_old, else from ring entry f mod 2 M of buffer ring_par
// (pkdelta::StreamDeltaPick, the host's line) -- read only for f < n_old, so only when n_old > 0, and f >= nd - M >=
// n_old - 2 M lies inside it.  While the slot is open t + M <= n - 1 for every frame that becomes final, so the upper
// clamp binds for them only once it is closed; for the frames of a run past the record's last new one it merely keeps
// the address inside the slot's own rows (their results are not stored).
//
// The ring is handed on as StreamFeatureLayoutKernel hands its history on: every wave of a slot reads buffer ring_par;
// the slot's first run (per block of features) writes frames [max(n - 2 M, 0), n) -- the fresh ones and those of the old
// ring that survive -- into the OTHER buffer, which no wave reads in this launch.  The host flips the bit when m > 0;
// with m == 0 (a flush from the ring alone) nothing is written and nothing flips.  No wave waits on another.
// Every address is formed from f clamped into [0, n) and d clamped into [d0, Db); a lane past Db shadows the block's
// first feature and stores nothing; a run past the record's last new delta frame returns before it touches memory
// (the first run, once it has handed the ring on).
__global__ __launch_bounds__(64) void StreamDeltaKernel(const StreamRec *__restrict__ recs, const StreamRec *__restrict__ lrecs, int num_recs, int Db,
                                                        int order, int window, const float *__restrict__ scales, float *rows, float *ring) {
  extern __shared__ float s_x[];                      // [kG + 2 M][64]
  const int lane = threadIdx.x;
  const int d0 = blockIdx.y * 64;
  const bool live = d0 + lane < Db;
  const int d = live ? d0 + lane : d0;
  const int M = order * window, L = 2 * M + 1;
  const int64_t F = (int64_t)(order + 1) * Db;
  const int k0 = blockIdx.x * kG;                     // the run's first frame among a record's new ones
  for (int k = blockIdx.z; k < num_recs; k += gridDim.z) {          // (uniform over the wave, as every `continue` below)
    // (the fields this kernel needs, one by one: a whole record is 96 bytes of scalar registers, and there are two)
    if (recs[k].kind == PK_MI355_FEATS_NORMALIZED) continue;
    const int slot = recs[k].slot, ring_par = recs[k].ring_par, m = recs[k].m;
    const int n_old = recs[k].n_old, n = n_old + m;
    const int nd = lrecs[k].n_old, made = lrecs[k].m;   // delta frames [nd, nd + made) become final
    const float *fresh = rows + recs[k].row_off + d;
    const float *old = ring + ((int64_t)slot * 2 + ring_par) * (2 * M) * Db + d;
    auto frame = [&](int f) {                         // f in [max(n_old - 2 M, 0), n)
      const pkdelta::StreamDeltaSource s = pkdelta::StreamDeltaPick(f, n_old, M);
      return (s.fresh ? fresh : old)[(int64_t)s.row * Db];
    };
    if (blockIdx.x == 0 && m > 0) {
      float *next = ring + ((int64_t)slot * 2 + (ring_par ^ 1)) * (2 * M) * Db + d;
      for (int f = n - 2 * M > 0 ? n - 2 * M : 0; f < n; ++f) {
        const float v = frame(f);
        if (live) next[(int64_t)(f % (2 * M)) * Db] = v;
      }
    }
    if (k0 >= made) continue;
    const int t0 = nd + k0;
    const int staged = kG + 2 * M;
#pragma unroll 8
    for (int q = 0; q < staged; ++q) {
      const int t = t0 - M + q;
      s_x[q * 64 + lane] = frame(t < 0 ? 0 : t < n ? t : n - 1);
    }
    float *y = rows + lrecs[k].row_off + d;
    for (int i = 0; i <= order; ++i) {
      const FrameRun acc = pkdelta::DeltaApply<FrameRun>(scales + i * L + M, i * window, [&](int j) {
        FrameRun v;
#pragma unroll
        for (int f = 0; f < kG; ++f) v.v[f] = s_x[(f + M + j) * 64 + lane];
        return v;
      });
      if (live) {
#pragma unroll
        for (int f = 0; f < kG; ++f)
          if (k0 + f < made) y[(int64_t)(k0 + f) * F + (int64_t)i * Db] = acc.v[f];
      }
    }
  }
}

}  // namespace

void LaunchStreamDelta(const StreamRec *recs, const StreamRec *lrecs, int n, int max_new, int base_dim, const pk_mi355_deltas_spec_t &spec,
                       const float *d_scales, float *rows, float *ring, hipStream_t stream) {
  if (n <= 0 || base_dim <= 0) return;
  // (a record without new delta frames still hands its ring on: one run at least)
  const dim3 grid(max_new > kG ? (max_new + kG - 1) / kG : 1, (base_dim + 63) / 64, n < 65535 ? n : 65535);
  const size_t lds = sizeof(float) * 64 * (size_t)(kG + 2 * pkdelta::Reach(spec));
  hipLaunchKernelGGL(StreamDeltaKernel, grid, dim3(64), lds, stream, recs, lrecs, n, base_dim, spec.order, spec.window, d_scales, rows, ring);
}

void LaunchDelta(const float *in, const UttLayout &utts, int num_utts, int max_frames, int base_dim, const pk_mi355_deltas_spec_t &spec,
                 const float *d_scales, float *out, hipStream_t stream) {
  if (num_utts <= 0 || max_frames <= 0 || base_dim <= 0) return;
  const dim3 grid((max_frames + kG - 1) / kG, (base_dim + 63) / 64, num_utts < 65535 ? num_utts : 65535);
  const size_t lds = sizeof(float) * 64 * (size_t)(kG + 2 * pkdelta::Reach(spec));
  hipLaunchKernelGGL(DeltaKernel, grid, dim3(64), lds, stream, in, utts, num_utts, base_dim, spec.order, spec.window, d_scales, out);
}

}  // namespace pkmi
