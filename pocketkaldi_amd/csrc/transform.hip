// transform.hip -- TransformKernel: the feature transform, Kaldi's splice-feats | transform-feats and the per-utterance
// transform-feats (include/pk_mi355.h states the rule).  It stands between the normalisation (or
// DeltaKernel) and FeatureLayoutKernel on a batch made by pk_mi355_transform_batch_create: rows [sum T][Dp] in, rows
// [sum T][rows] out, never in place.  One kernel serves both stages: the matrix table has a stride, 0 when every
// utterance reads the same matrix (the global stage), else utterance u reads matrix u.
//
// Lane = output feature.  One wavefront (a workgroup of its own) per (utterance, run of G = kTransformFrames frames,
// block of 64 outputs):
//   Stage: the G + L + R input rows the run's outputs read (frames t0 - L .. t0 + G - 1 + R, each clamped into the
//     utterance's own rows: the edge rule is applied here, once) go to LDS as they lie, s_x[row][d], the lanes striding
//     over d -- coalesced loads.  The workgroup is this one wave and every branch around the staging is uniform over
//     it, so the __syncthreads() that orders the staging against the reads is one no wave waits at alone.
//   Apply: the host's pkxf::TransformApply (pk_transform.h) instantiated on a run of G frames held in registers: per k
//     ONE load of the lane's matrix entry (the matrix lies transposed and padded, [k][ldo]: a wave's read of one k is
//     one contiguous run, the lanes past `rows` read the padding's zeros) and G LDS reads at a wave-uniform address
//     (a broadcast, free of bank conflicts), G products and G adds -- k ascending for every frame, the offset last:
//     each output's own chain is the host's, operation for operation.  No MFMA, no fma (the pragma below, and
//     -ffp-contract=off).  Then G stores of the block.
// Every address is formed from t clamped into [0, T), d < Dp and o inside the padded matrix: a load past the
// utterance's rows is never issued, so a poisoned neighbour is never read; a lane past `rows` stores nothing; a run
// that starts behind the utterance's last frame goes on before it touches memory, so a frameless utterance costs its
// waves' launch only.
//
// StreamTransformKernel, further down, is the same stage and apply for a live slot of a stream made by
// pk_mi355_transform_stream_create: the frames below the step's fresh rows come from the slot's
// ring.  The run of frames a lane holds, the apply and the store are one device function that both kernels call.
#include <hip/hip_runtime.h>

#include "pk_transform_kernel.h"

#pragma clang fp contract(off)

namespace pkmi {

namespace {

constexpr int kG = kTransformFrames;

// The run of G frames of one output that a lane holds: what TransformApply's float is on the host.
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

// The apply and the store of one cell, shared by both kernels: s_x holds the run's staged rows, [kG + W - 1][Dp], row f +
// j being window frame j of the run's frame f; m: the lane's column of the padded transposed matrix; y: the lane's
// output of the run's first frame; the run's first `count` frames are stored, by the lanes below `rows`.
__device__ inline void ApplyRun(const float *s_x, int W, int Dp, bool affine, const float *m, int ldo, int rows, int o, float *y, int count) {
  const FrameRun acc = pkxf::TransformApply<FrameRun>(W, Dp, affine, [&](int k) { return m[(int64_t)k * ldo]; }, [&](int j, int d) {
    FrameRun v;
#pragma unroll
    for (int f = 0; f < kG; ++f) v.v[f] = s_x[(f + j) * Dp + d];
    return v;
  });
  if (o < rows) {
#pragma unroll
    for (int f = 0; f < kG; ++f)
      if (f < count) y[(int64_t)f * rows] = acc.v[f];
  }
}

__global__ __launch_bounds__(64) void TransformKernel(const float *__restrict__ in, UttLayout utts, int num_utts, int Dp, int L, int R, int rows,
                                                      int affine, const float *__restrict__ mt, int64_t mat_stride, float *__restrict__ out) {
  extern __shared__ float s_x[];                      // [kG + L + R][Dp]
  const int lane = threadIdx.x;
  const int t0 = blockIdx.x * kG;
  const int o = blockIdx.y * 64 + lane;               // < ldo: inside the padded matrix
  const int ldo = (rows + 63) / 64 * 64;
  const int W = L + R + 1, staged = kG + L + R;
  for (int u = blockIdx.z; u < num_utts; u += gridDim.z) {          // (uniform over the wave, which is the workgroup)
    const int T = utts.num_frames[u];
    if (t0 >= T) continue;
    const float *x = in + utts.raw_base[u] * Dp;
    const float *m = mt + (int64_t)u * mat_stride + o;
    __syncthreads();                                  // (a second utterance of this wave: the last one's reads are done)
    for (int r = 0; r < staged; ++r) {
      const int t = t0 - L + r;
      const float *row = x + (int64_t)(t < 0 ? 0 : t < T ? t : T - 1) * Dp;
      for (int d = lane; d < Dp; d += 64) s_x[r * Dp + d] = row[d];
    }
    __syncthreads();
    ApplyRun(s_x, W, Dp, affine != 0, m, ldo, rows, o, out + (utts.raw_base[u] + t0) * rows + o, T - t0);
  }
}

// The transform of a live slot: TransformKernel's stage and apply, with the frames below the
// step's fresh rows taken from the slot's ring.  One wavefront (a workgroup of its own) per (record, run of G of the
// record's newly final transform frames, block of 64 outputs), lane = output.  Transform frame t reads the input frames
// clamp(t + j, 0, n - 1), j = -L .. R: frame f from the step's fresh rows when f >= n_old, else from ring entry f mod C
// of the buffer bit 0 of xf_bits names (pkxf::StreamTransformPick, the host's line) -- read only for f < n_old, so only
// when n_old > 0, and f >= nx - L >= n_old - C lies inside it.  While the slot is open t + R <= n - 1 for every frame
// that becomes final, so the upper clamp binds for them only once it is closed; for the frames of a run past the
// record's last new one it merely keeps the address inside the slot's own rows (their results are not stored).
//
// The ring is handed on as StreamDeltaKernel hands its ring on: every wave of a slot reads the buffer the bit names;
// the slot's first run (of the first block of outputs) writes frames [max(n - C, 0), n) -- the fresh ones and those of
// the old ring that survive -- into the OTHER buffer, which no wave reads in this launch.  The host flips the bit when
// m > 0; with m == 0 (a flush from the ring alone) or C == 0 nothing is written.  No wave waits on another.
// per_slot: the slots' own stage, C == 0 (the ring is never read), the matrix table indexed by the record's slot; a slot
// without a matrix has its rows copied through LDS as bits.
// Every address is formed from f clamped into [0, n), d < Dp and o inside the padded matrix; a lane past `rows` stores
// nothing; a run past the record's last new frame returns before it touches memory (the first run, once it has handed
// the ring on).
__global__ __launch_bounds__(64) void StreamTransformKernel(const StreamRec *__restrict__ irecs, const StreamRec *__restrict__ orecs, int num_recs,
                                                            int Dp, int L, int R, int rows, int affine, int per_slot, const float *__restrict__ mt,
                                                            int64_t mat_stride, float *io, float *ring) {
  extern __shared__ float s_x[];                      // [kG + L + R][Dp]
  const int lane = threadIdx.x;
  const int o = blockIdx.y * 64 + lane;               // < ldo: inside the padded matrix
  const int ldo = (rows + 63) / 64 * 64;
  const int C = L + R, W = C + 1, staged = kG + C, ring_len = C > 0 ? C : 1;
  const int k0 = blockIdx.x * kG;                     // the run's first frame among a record's new ones
  for (int k = blockIdx.z; k < num_recs; k += gridDim.z) {          // (uniform over the wave, which is the workgroup, as every `continue` below)
    if (irecs[k].kind == PK_MI355_FEATS_NORMALIZED) continue;
    const int slot = irecs[k].slot, bits = irecs[k].xf_bits, par = bits & 1, mat = bits >> 1;
    const int n_old = irecs[k].n_old, m_in = irecs[k].m, n = n_old + m_in;
    const int nx = orecs[k].n_old, made = orecs[k].m;   // transform frames [nx, nx + made) become final
    const float *fresh = io + irecs[k].row_off;
    const float *old = ring + ((int64_t)slot * 2 + par) * ring_len * Dp;
    auto frame = [&](int f) {                         // f in [max(n_old - C, 0), n)
      const pkxf::StreamTransformSource s = pkxf::StreamTransformPick(f, n_old, C);
      return (s.fresh ? fresh : old) + (int64_t)s.row * Dp;
    };
    if (blockIdx.x == 0 && blockIdx.y == 0 && m_in > 0 && C > 0) {
      float *next = ring + ((int64_t)slot * 2 + (par ^ 1)) * ring_len * Dp;
      for (int f = n - C > 0 ? n - C : 0; f < n; ++f) {
        const float *row = frame(f);
        for (int d = lane; d < Dp; d += 64) next[(int64_t)(f % C) * Dp + d] = row[d];
      }
    }
    if (k0 >= made) continue;
    const int t0 = nx + k0;
    __syncthreads();                                  // (a second record of this wave: the last one's reads are done)
    for (int q = 0; q < staged; ++q) {
      const int t = t0 - L + q;
      const float *row = frame(t < 0 ? 0 : t < n ? t : n - 1);
      for (int d = lane; d < Dp; d += 64) s_x[q * Dp + d] = row[d];
    }
    __syncthreads();
    float *y = io + orecs[k].row_off + (int64_t)k0 * rows + o;
    if (per_slot && mat == kSlotMatNone) {            // (Dp == rows, C == 0: row f of the LDS is frame f)
      if (o < rows)
        for (int f = 0; f < kG && f < made - k0; ++f) y[(int64_t)f * rows] = s_x[f * Dp + o];
      continue;
    }
    const float *m = mt + (per_slot ? (int64_t)slot * mat_stride : 0) + o;
    ApplyRun(s_x, W, Dp, per_slot ? mat == kSlotMatAffine : affine != 0, m, ldo, rows, o, y, made - k0);
  }
}

}  // namespace

void LaunchStreamTransform(const StreamRec *irecs, const StreamRec *orecs, int n, int max_new, const TransformStage &s, bool per_slot, float *rows,
                           float *ring, hipStream_t stream) {
  if (n <= 0 || s.in_dim <= 0 || s.rows <= 0) return;
  // (a record without new transform frames still hands its ring on: one run at least)
  const dim3 grid(max_new > kG ? (max_new + kG - 1) / kG : 1, (s.rows + 63) / 64, n < 65535 ? n : 65535);
  hipLaunchKernelGGL(StreamTransformKernel, grid, dim3(64), TransformLds(s), stream, irecs, orecs, n, s.in_dim, s.left, s.right, s.rows,
                     s.affine ? 1 : 0, per_slot ? 1 : 0, s.mt, s.mat_stride, rows, ring);
}

void LaunchTransform(const float *in, const UttLayout &utts, int num_utts, int max_frames, const TransformStage &s, float *out, hipStream_t stream) {
  if (num_utts <= 0 || max_frames <= 0 || s.in_dim <= 0 || s.rows <= 0) return;
  const dim3 grid((max_frames + kG - 1) / kG, (s.rows + 63) / 64, num_utts < 65535 ? num_utts : 65535);
  hipLaunchKernelGGL(TransformKernel, grid, dim3(64), TransformLds(s), stream, in, utts, num_utts, s.in_dim, s.left, s.right, s.rows, s.affine ? 1 : 0,
                     s.mt, s.mat_stride, out);
}

}  // namespace pkmi
