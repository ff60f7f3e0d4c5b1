// What the Shampoo kernels (shampoo.hip) share: the fp32 matrix instruction, the LDS layout of a
// 64 x 64 block and the tile products on it.
//
// v_mfma_f32_16x16x4_f32: lane (c = lane & 15, g = lane >> 4) gives A[c][g] and B[g][c] of a
// 16 x 4 by 4 x 16 product and holds C[4 g + v][c], v = 0..3.  A 64-long reduction is 16 of them.
// Which four reduction indices one instruction takes is free as long as both operands agree, and
// here lane group g takes 16 kk + 4 g + v in instruction (kk, v).  Then
//   * an operand read along a ROW of its matrix is one 16-byte LDS read for four instructions
//     (elements 16 kk + 4 g .. + 3 of row c), and
//   * an operand read along a COLUMN is a 4-byte read of row 16 kk + 4 g + v, column c.
// With the row stride SH_S = 68 floats (68 = 4 mod 64 banks) the 16 lanes of a group of the row
// read start at banks 4 c and cover all 64 once; the column read falls on bank
// 4 (4 g + v) + c = 16 g + c (+ const): 64 lanes, 64 banks.  Unpadded (stride 64) every lane of a
// row read would start at the same bank.  An accumulator is stored as four 4-byte writes of rows
// 4 g + v, the column read's pattern.
#pragma once
#include "optim_device.h"

namespace dtr {

constexpr int SH_S = SH_BLOCK + 4;        // LDS row stride of a block, in floats
constexpr int SH_MAT = SH_BLOCK * SH_S;   // floats of one block in LDS

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// The four values lane (c, g) feeds to instructions (k0 / 16, 0..3) for tile t of M: along the
// rows of M (the tile's 16 rows are M's rows) or along its columns.
template <bool COL>
__device__ __forceinline__ f32x4 sh_operand(const float* __restrict__ M, int t, int k0, int c, int g) {
  if constexpr (COL) {
    const float* p = M + (k0 + 4 * g) * SH_S + 16 * t + c;
    return f32x4{p[0], p[SH_S], p[2 * SH_S], p[3 * SH_S]};
  } else {
    return *reinterpret_cast<const f32x4*>(M + (16 * t + c) * SH_S + k0 + 4 * g);
  }
}

// acc[b] = tile (ti, tj + b) of op(A) op(B) over the first kp (a multiple of 16) reduction
// indices, b < NB: the A operand is loaded once for NB column tiles.
//   ACOL 0, BROW 0: A B      ACOL 0, BROW 1: A B^T      ACOL 1, BROW 0: A^T B
template <bool ACOL, bool BROW, int NB>
__device__ __forceinline__ void sh_tiles(const float* __restrict__ A, const float* __restrict__ B,
                                         int ti, int tj, int kp, int c, int g, f32x4 (&acc)[NB]) {
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < kp; k0 += 16) {
    const f32x4 a = sh_operand<ACOL>(A, ti, k0, c, g);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const f32x4 bv = sh_operand<!BROW>(B, tj + b, k0, c, g);
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[b] = mfma4(a[v], bv[v], acc[b]);
    }
  }
}

// The accumulator of tile (ti, tj) into the LDS block M.
__device__ __forceinline__ void sh_store_tile(float* __restrict__ M, int ti, int tj, int c, int g,
                                              const f32x4& acc) {
  float* p = M + (16 * ti + 4 * g) * SH_S + 16 * tj + c;
#pragma unroll
  for (int v = 0; v < 4; ++v) p[v * SH_S] = acc[v];
}

// Sum of a workgroup's per-thread fp32 sums: widened, the wave's shuffles and the NW waves left
// to right in fp64 through red[NW] (one order; the caller keeps red's uses a barrier apart).
template <int NW>
__device__ __forceinline__ double sh_block_sum(float s, double* red) {
  const double w = wave_sum_f64((double)s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  double tot = red[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) tot += red[i];
  return tot;
}

}  // namespace dtr
