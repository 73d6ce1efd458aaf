// pk_f16_layout.h -- the operand contract of the fp16 matrix-core GEMMs, once: how a value is split, where it lies
// in a row, and how a half-slab of rows lies in LDS.  Shared by the kernels that read or write operands
// (gemm_f16.hip) and by the host code that packs the weights (capi_model.hip).
#ifndef PK_F16_LAYOUT_H_
#define PK_F16_LAYOUT_H_

#include <hip/hip_runtime.h>
#include <math.h>

#include "pk_kernels.h"

namespace pkmi {

// ---- a value.  x = hi + lo with hi = fp16(x), lo = fp16(x - hi)  (x - hi is exact in fp32).  fp16 saturates at
// 65504; the split clamps instead of overflowing.
struct SplitOut {
  _Float16 hi, lo;
};
__host__ __device__ __forceinline__ SplitOut Split(float v) {
  v = fminf(fmaxf(v, -65504.0f), 65504.0f);
  SplitOut s;
  s.hi = static_cast<_Float16>(v);
  s.lo = static_cast<_Float16>(v - static_cast<float>(s.hi));
  return s;
}

// ---- a row.  The (hi, lo) pairs are interleaved in chunks of 8 k's: [hi k0..7][lo k0..7][hi k8..15][lo ...], so
// the 64 bytes one k16 step needs of a row are contiguous.  A row of K values is 2 K halves long.
constexpr int kChunk = 8, kChunkLog2 = 3;
constexpr int kLoHalves = kChunk;             // a lo half lies this many halves behind its hi half
// where the hi half of logical k lies in the row that starts at `row`
template <class T>
__host__ __device__ __forceinline__ constexpr T *HiPtr(T *row, int k) { return row + (k >> kChunkLog2) * (2 * kChunk) + (k & (kChunk - 1)); }
// byte offset in a row of the hi halves of columns w g .. w g + w - 1, w = 2 or 4 (they share a chunk).  Not a
// template, and not HiPtr of w g: either spelling changes the instruction stream of the GEMM epilogues.
__host__ __device__ __forceinline__ constexpr int HiByteOfGroup(int g, int w) {
  return (g >> (w == 2 ? 2 : 1)) * (4 * kChunk) + (g & (w == 2 ? 3 : 1)) * (2 * w);
}

// ---- a half-slab: k16 of the 256 X rows, then of the 256 W rows of a tile, 64 bytes per row.
constexpr int kT = kTileF16;                  // 256: tile edge
constexpr int kStepK = 16;                    // k per half-slab = one MFMA k16 step
constexpr int kOperandBytes = kT * 64;        // one operand of one half-slab: 256 rows x 64 B
constexpr int kHalfSlabBytes = 2 * kOperandBytes;   // X rows, then W rows: 32 KiB
constexpr int kRingF16 = 4;

// LDS row (0..255) of the W tile -> column n of the tile, per MFMA form.  32 x 32 x 16: within each block of 64
// columns sub-tile y of a wave owns columns 2 i' + y, stored as 32 consecutive LDS rows.  16 x 16 x 32: tile y owns
// columns 4 j + y, stored as 16 consecutive rows.
__host__ __device__ __forceinline__ constexpr int WRowToCol(int row) { return (row & ~63) + 2 * (row & 31) + ((row >> 5) & 1); }
__host__ __device__ __forceinline__ constexpr int WRowToCol16(int row) { return (row & ~63) + 4 * (row & 15) + ((row >> 4) & 3); }

// XOR swizzle: byte offset of logical 16-byte position q of LDS row `row`; the four positions of a 64-byte row are
// [k0..7 hi][k0..7 lo][k8..15 hi][k8..15 lo].  The twist of a row is (row >> 2) & 3 for the 32 x 32 form and its
// Gray code for the 16 x 16 form (why: gemm_f16.hip, GemmF16K32Kernel).  A DMA lane applies the same twist to the
// SOURCE position it fetches (gemm_f16.hip: q).
__host__ __device__ __forceinline__ constexpr int Gray2(int c) { return c ^ (c >> 1); }
__host__ __device__ __forceinline__ constexpr int SwzOff(int row, int q) { return row * 64 + ((q ^ ((row >> 2) & 3)) << 4); }
__host__ __device__ __forceinline__ constexpr int SwzOff16(int row, int q) { return row * 64 + ((q ^ Gray2((row >> 2) & 3)) << 4); }

}  // namespace pkmi

#endif  // PK_F16_LAYOUT_H_
