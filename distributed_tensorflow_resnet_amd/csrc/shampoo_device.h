// What the Shampoo kernels (shampoo.hip, soap.hip) share: the fp32 matrix instruction, the LDS
// layout of a 64 x 64 block, the tile products on it and the passes that stage a block.
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

constexpr int SH_THREADS = 256;   // the staging passes' default workgroup (stats, precondition)

// The 1-based step count of the launches: t = *gstep - *start + 1 (start may be null: 0).
__device__ __forceinline__ long long sh_step(const long long* __restrict__ gstep,
                                             const long long* __restrict__ start) {
  return *gstep - (start ? *start : 0ll) + 1;
}

// g' = s g of block b into Gs: all 64 x 64 entries, zero outside the live r x k.  16-byte loads
// where every row of the block starts on a 16-byte boundary and k is a multiple of 4, scalar
// loads of the block's own elements otherwise.  NT threads.
template <int NT = SH_THREADS>
__device__ __forceinline__ void sh_stage_grad(const float* __restrict__ grad, const ShampooBlock& b,
                                              float s, float* __restrict__ Gs) {
  const bool vec = ((b.offset | (long long)b.K | (long long)b.k) & 3) == 0;
  for (int q = threadIdx.x; q < SH_BLOCK * 16; q += NT) {
    const int i = q >> 4, j4 = (q & 15) << 2;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (i < b.r && j4 < b.k) {
      const float* p = grad + b.offset + (long long)i * b.K + j4;
      if (vec) {
        v = *reinterpret_cast<const f32x4*>(p);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (j4 + u < b.k) v[u] = p[u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = s * v[u];
    }
    *reinterpret_cast<f32x4*>(Gs + i * SH_S + j4) = v;
  }
}

// A whole state slot [64][64] into an LDS block.
template <int NT = SH_THREADS>
__device__ __forceinline__ void sh_stage_slot(const float* __restrict__ slot, float* __restrict__ M) {
  for (int q = threadIdx.x; q < SH_BLOCK * 16; q += NT) {
    const int i = q >> 4, j4 = (q & 15) << 2;
    *reinterpret_cast<f32x4*>(M + i * SH_S + j4) =
        *reinterpret_cast<const f32x4*>(slot + i * SH_BLOCK + j4);
  }
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
