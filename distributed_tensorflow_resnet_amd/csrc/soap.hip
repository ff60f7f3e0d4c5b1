// SOAP (Vyas et al. 2024): Adam in the eigenbasis of Shampoo's statistics, as a variant of the
// blocked Shampoo of shampoo.hip -- the same block table, the same statistics launch, no matrix
// root.  Per 64 x 64 block of a conv kernel (live size r x k), with G the block of g' = s g,
// t the 1-based step count and b1, b2, eps adamw's coefficients:
//   L' = sb2 L + c G G^T,  Rt' = sb2 Rt + c G^T G                      (shampoo_stats, unchanged)
//   when t % every == 0, for (S, Q) in ((L', QL), (Rt', QR)):  Q <- the orthonormal factor of the
//     Householder QR of S Q, its columns signed so that diag(R) >= 0   (one orthogonal iteration;
//     order and sign of the columns carry over, which V below relies on)
//   M' = b1 M + (1 - b1) G                                  (original space, the momentum buffer)
//   G~ = QL^T G QR,  M~ = QL^T M' QR,  V' = b2 V + (1 - b2) G~ G~      (V: rotated space)
//   N  = QL (M~ / (sqrt(V') + eps)) QR^T                               (the direction buffer)
//   w' = (w - alpha N) - (lr wd_s) w,  alpha = lr sqrt(1 - b2^t) / (1 - b1^t)
// and every other tensor takes adamw's element step.  The bases start as the identity on the
// live part; products by the identity are exact on the matrix cores, and the element arithmetic
// is written out (soap_adam_elem: contraction off, the fmas explicit) with the roundings
// adam.hip's adam_elem compiles to on both of its paths,
//   m' = fma(b1, m, (1 - b1) g'),  v' = fma(b2, v, (1 - b2) (g' g')),  q = m' / (sqrtf(v') + eps),
//   w' = fma(-(lr wd), w, fma(-alpha, q, w))
// so until the first refresh the step is adamw's bit for bit.  (adam_elem itself, inlined into
// this file's walk, is contracted differently from element to element.)
// Three launches after shampoo_stats:
//   soap_refresh      one workgroup of 8 waves per (block, side); all leave at once unless
//                     t % every == 0, read from the step word, so a captured graph replays it.
//                     S and Q are staged into LDS and A = S Q is formed on the matrix cores by
//                     waves 0..3: wave w holds column tile w of A in its accumulators, lane
//                     (c, g) the rows 16 q + 4 g + e of column 16 w + c.  Waves 4..7 hold, in the
//                     same layout, W = I, which becomes Q^T = H_{n-1} .. H_0: the QR runs on the
//                     augmented [A | W] in REGISTERS, 16 per thread, each thread owning a quarter
//                     of one column.  Column j's owner publishes it through a double-buffered
//                     64-float LDS vector -- the one barrier of a column step -- and every
//                     thread then forms the reflector for itself (the column's norm: fp32 over a
//                     thread's rows, fp64 over the four lane groups, the same bits in every
//                     thread), takes v^T (its column) over its quarter plus two shuffles, and
//                     updates its quarter.  A column whose norm is not > 0 skips its reflector
//                     (H = I), so a rank-deficient statistic still gives an orthonormal Q.  The
//                     live part of the slot is overwritten by the signed transpose of W unless
//                     something is not finite, which adds 1 to *fail.
//   soap_rotate_adam  one workgroup of 8 waves per block; G, M', QL, QR and two scratch blocks
//                     in LDS (6 x 17 KB).  M' is formed while staging and written back.
//                     QL^T G and QL^T M' -> barrier -> (.) QR for both in the accumulators, where
//                     V is read, updated and stored and N~ formed, N~ into G's block -> barrier ->
//                     QL N~ -> barrier -> (.) QR^T from the accumulators to the direction buffer.
//                     Only the live r x k elements of a block are read or written.
//   soap_update_pack  a FlatWalk launch of adam_update_pack's shape: alpha N for a rotated
//                     segment, soap_adam_elem for the others.  ohwi_pack follows.
#include "shampoo_device.h"

namespace dtr {

constexpr int SOAP_THREADS = 512, SOAP_WAVES = SOAP_THREADS / 64;
constexpr int SOAP_LDS6 = 6 * SH_MAT * (int)sizeof(float);   // 104,448 B: one workgroup per CU
static_assert(SOAP_LDS6 <= 163840, "LDS");

// The sum over the four lane groups of a wave (lanes c, c + 16, c + 32, c + 48), in fp64: the
// same tree, so the same bits, in all four.
__device__ __forceinline__ double soap_group_sum(float s) {
  double d = (double)s;
  d += __shfl_xor(d, 16, 64);
  d += __shfl_xor(d, 32, 64);
  return d;
}

// adam_elem's decoupled step, the roundings written out.
__device__ __forceinline__ float soap_moment1(float m, float gp, const AdamCoef& c) {
#pragma clang fp contract(off)
  return __builtin_fmaf(c.b1, m, c.omb1 * gp);
}

__device__ __forceinline__ float soap_moment2(float v, float gp, const AdamCoef& c) {
#pragma clang fp contract(off)
  return __builtin_fmaf(c.b2, v, c.omb2 * (gp * gp));
}

__device__ __forceinline__ float soap_quotient(float m, float v, const AdamCoef& c) {
  return m / (sqrtf(v) + c.eps);
}

__device__ __forceinline__ float soap_descend(float w, float q, float alpha, float lrwd) {
  return __builtin_fmaf(-lrwd, w, __builtin_fmaf(-alpha, q, w));
}

__device__ __forceinline__ void soap_adam_elem(float& w, float g, float& m, float& v, float s,
                                               float lrwd, float alpha, const AdamCoef& c) {
#pragma clang fp contract(off)
  const float gp = g * s;
  m = soap_moment1(m, gp, c);
  v = soap_moment2(v, gp, c);
  w = soap_descend(w, soap_quotient(m, v, c), alpha, lrwd);
}

// ---------------------------------------------------------------------------------- refresh
__global__ void __launch_bounds__(SOAP_THREADS)
soap_refresh_kernel(const ShampooBlock* __restrict__ tab, const float* __restrict__ L,
                    const float* __restrict__ Rt, float* QL, float* QR,
                    const long long* __restrict__ gstep, const long long* __restrict__ start,
                    int every, int* __restrict__ fail) {
#pragma clang fp contract(off)
  if (sh_step(gstep, start) % every != 0) return;   // the same word for every thread
  __shared__ __attribute__((aligned(16))) float Ss[SH_MAT];
  __shared__ __attribute__((aligned(16))) float Qs[SH_MAT];
  __shared__ __attribute__((aligned(16))) float vb[2][SH_BLOCK];
  __shared__ float sgn[SH_BLOCK];
  __shared__ int bad;
  const ShampooBlock b = tab[blockIdx.x];
  const bool right = blockIdx.y != 0;
  const int n = right ? b.k : b.r, nt = (n + 15) >> 4, np = 16 * nt;
  const float* __restrict__ S = (right ? Rt : L) + (long long)b.slot * (SH_BLOCK * SH_BLOCK);
  float* P = (right ? QR : QL) + (long long)b.slot * (SH_BLOCK * SH_BLOCK);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, cc = lane & 15, g = lane >> 4;
  sh_stage_slot<SOAP_THREADS>(S, Ss);
  sh_stage_slot<SOAP_THREADS>(P, Qs);
  if (tid == 0) bad = 0;
  lds_barrier();
  // the thread's quarter column: rows 16 q + 4 g + e of column `col` of A (waves 0..3) or W
  const bool isA = wave < 4;
  const int ct = wave & 3, col = 16 * ct + cc;
  f32x4 a[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    a[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (isA) {
      if (q < nt && ct < nt) {   // uniform per wave
        f32x4 acc[1];
        sh_tiles<false, false, 1>(Ss, Qs, q, ct, np, cc, g, acc);
        a[q] = acc[0];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) a[q][e] = (16 * q + 4 * g + e == col && col < n) ? 1.f : 0.f;
    }
  }
  bool nf = false;
  for (int j = 0; j < n; ++j) {
    float* vj = vb[j & 1];
    if (isA && col == j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(vj + 16 * q + 4 * g) = a[q];
    }
    lds_barrier();   // column j is published; the other buffer is free for column j + 1
    f32x4 x[4];
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      x[q] = *reinterpret_cast<const f32x4*>(vj + 16 * q + 4 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (16 * q + 4 * g + e < j) x[q][e] = 0.f;
        ss = __builtin_fmaf(x[q][e], x[q][e], ss);
      }
    }
    const float x0 = vj[j];
    const float nrm = (float)sqrt(soap_group_sum(ss));
    if (!(nrm > 0.f)) {   // a zero column (H = I), or NaN: uniform over the workgroup
      nf = nf || nrm != 0.f;
      if (tid == 0) sgn[j] = 1.f;
      continue;
    }
    // H = I - v v^T / den with v = x - beta e_j, beta = -sign(x0) ||x||: H x = beta e_j = R[j][j] e_j
    const float beta = x0 >= 0.f ? -nrm : nrm;
    const float v0 = x0 - beta;
    const float den = -beta * v0;   // ||x|| (|x0| + ||x||) > 0
    if (tid == 0) sgn[j] = beta < 0.f ? -1.f : 1.f;
    if (isA && 16 * ct + 15 <= j) continue;   // (uniform per wave) these columns are done
    float w = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (16 * q + 4 * g + e == j) x[q][e] = v0;
        w = __builtin_fmaf(x[q][e], a[q][e], w);
      }
    }
    const float f = (float)soap_group_sum(w) / den;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int e = 0; e < 4; ++e) a[q][e] = __builtin_fmaf(-f, x[q][e], a[q][e]);
    }
  }
  if (!isA) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int e = 0; e < 4; ++e) nf = nf || !(fabsf(a[q][e]) <= 3.0e38f);
    }
  }
  if (nf) bad = 1;
  lds_barrier();   // the signs and the flag
  if (bad) {       // the old basis stays
    if (tid == 0 && fail) atomicAdd(fail, 1);
    return;
  }
  // Q[col][i] = sgn[i] W[i][col]: four consecutive elements of row `col` per store
  if (!isA && col < n) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i0 = 16 * q + 4 * g;
      if (i0 >= n) continue;
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = i0 + e < n ? a[q][e] * sgn[i0 + e] : 0.f;
      float* p = P + col * SH_BLOCK + i0;
      if (i0 + 4 <= n) {
        *reinterpret_cast<f32x4*>(p) = o;
      } else {
        for (int e = 0; e < 4 && i0 + e < n; ++e) p[e] = o[e];
      }
    }
  }
}

void soap_refresh(const ShampooBlock* tab, int nblocks, int sides, const float* L, const float* Rt,
                  float* QL, float* QR, const long long* gstep, const long long* start, int every,
                  int* fail, hipStream_t st) {
  if (nblocks <= 0) return;
  hipLaunchKernelGGL(soap_refresh_kernel, dim3(nblocks, sides), dim3(SOAP_THREADS), 0, st, tab, L,
                     Rt, QL, QR, gstep, start, every, fail);
  DTR_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------- rotate
// g' = s g and M' = fma(b1, M, (1 - b1) g') of block b into Gs and Ms (zero outside the live
// r x k), M' also back to the momentum buffer: sh_stage_grad's walk.
__device__ __forceinline__ void soap_stage_moment(const float* __restrict__ grad,
                                                  float* __restrict__ mom, const ShampooBlock& b,
                                                  float s, const AdamCoef& c,
                                                  float* __restrict__ Gs, float* __restrict__ Ms) {
#pragma clang fp contract(off)
  const bool vec = ((b.offset | (long long)b.K | (long long)b.k) & 3) == 0;
  for (int q = threadIdx.x; q < SH_BLOCK * 16; q += SOAP_THREADS) {
    const int i = q >> 4, j4 = (q & 15) << 2;
    f32x4 gv = {0.f, 0.f, 0.f, 0.f}, mv = {0.f, 0.f, 0.f, 0.f};
    if (i < b.r && j4 < b.k) {
      const long long e0 = b.offset + (long long)i * b.K + j4;
      if (vec) {
        gv = *reinterpret_cast<const f32x4*>(grad + e0);
        mv = *reinterpret_cast<const f32x4*>(mom + e0);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (j4 + u < b.k) {
            gv[u] = grad[e0 + u];
            mv[u] = mom[e0 + u];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        gv[u] = gv[u] * s;
        mv[u] = soap_moment1(mv[u], gv[u], c);
      }
      if (vec) {
        *reinterpret_cast<f32x4*>(mom + e0) = mv;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (j4 + u < b.k) mom[e0 + u] = mv[u];
      }
    }
    *reinterpret_cast<f32x4*>(Gs + i * SH_S + j4) = gv;
    *reinterpret_cast<f32x4*>(Ms + i * SH_S + j4) = mv;
  }
}

__global__ void __launch_bounds__(SOAP_THREADS)
soap_rotate_adam_kernel(const float* __restrict__ grad, const ShampooBlock* __restrict__ tab,
                        const float* __restrict__ QL, const float* __restrict__ QR,
                        float* __restrict__ mom, float* __restrict__ vbuf,
                        float* __restrict__ dir, AdamCoef c, float grad_scale) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Gs = reinterpret_cast<float*>(smem);   // g', later N~
  float* Ms = Gs + SH_MAT;                      // M'
  float* Ls = Ms + SH_MAT;                      // QL
  float* Rs = Ls + SH_MAT;                      // QR
  float* T1 = Rs + SH_MAT;                      // QL^T G, later QL N~
  float* T2 = T1 + SH_MAT;                      // QL^T M'
  const ShampooBlock b = tab[blockIdx.x];
  soap_stage_moment(grad, mom, b, grad_scale, c, Gs, Ms);
  sh_stage_slot<SOAP_THREADS>(QL + (long long)b.slot * (SH_BLOCK * SH_BLOCK), Ls);
  sh_stage_slot<SOAP_THREADS>(QR + (long long)b.slot * (SH_BLOCK * SH_BLOCK), Rs);
  lds_barrier();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, cc = lane & 15, g = lane >> 4;
  const int ntr = (b.r + 15) >> 4, ntk = (b.k + 15) >> 4, ntile = ntr * ntk;
  f32x4 acc[1];
  for (int u = wave; u < 2 * ntile; u += SOAP_WAVES) {   // QL^T G and QL^T M' (uniform per wave)
    const bool second = u >= ntile;
    const int w = second ? u - ntile : u, ti = w / ntk, tj = w - ti * ntk;
    sh_tiles<true, false, 1>(Ls, second ? Ms : Gs, ti, tj, 16 * ntr, cc, g, acc);
    sh_store_tile(second ? T2 : T1, ti, tj, cc, g, acc[0]);
  }
  lds_barrier();   // G is read
  for (int u = wave; u < ntile; u += SOAP_WAVES) {   // G~, M~; V' and N~ in the accumulators
    const int ti = u / ntk, tj = u - ti * ntk;
    f32x4 gt[1], mt[1];
    sh_tiles<false, false, 1>(T1, Rs, ti, tj, 16 * ntk, cc, g, gt);
    sh_tiles<false, false, 1>(T2, Rs, ti, tj, 16 * ntk, cc, g, mt);
    const int col = 16 * tj + cc;
    f32x4 nt4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = 16 * ti + 4 * g + v;
      if (row < b.r && col < b.k) {
        float* pv = vbuf + b.offset + (long long)row * b.K + col;
        const float vn = soap_moment2(*pv, gt[0][v], c);
        *pv = vn;
        nt4[v] = soap_quotient(mt[0][v], vn, c);
      }
    }
    sh_store_tile(Gs, ti, tj, cc, g, nt4);
  }
  lds_barrier();   // N~ is complete, T1 and T2 are read
  for (int u = wave; u < ntile; u += SOAP_WAVES) {   // QL N~
    const int ti = u / ntk, tj = u - ti * ntk;
    sh_tiles<false, false, 1>(Ls, Gs, ti, tj, 16 * ntr, cc, g, acc);
    sh_store_tile(T1, ti, tj, cc, g, acc[0]);
  }
  lds_barrier();
  for (int u = wave; u < ntile; u += SOAP_WAVES) {   // N = (QL N~) QR^T, the live part out
    const int ti = u / ntk, tj = u - ti * ntk;
    sh_tiles<false, true, 1>(T1, Rs, ti, tj, 16 * ntk, cc, g, acc);
    const int col = 16 * tj + cc;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = 16 * ti + 4 * g + v;
      if (row < b.r && col < b.k) dir[b.offset + (long long)row * b.K + col] = acc[0][v];
    }
  }
}

void soap_rotate_adam(const float* grad, const ShampooBlock* tab, int nblocks, const float* QL,
                      const float* QR, float* mom, float* v, float* dir, float beta1, float beta2,
                      float epsilon, float grad_scale, hipStream_t st) {
  if (nblocks <= 0) return;
  hipLaunchKernelGGL(soap_rotate_adam_kernel, dim3(nblocks), dim3(SOAP_THREADS), SOAP_LDS6, st,
                     grad, tab, QL, QR, mom, v, dir, adam_coef(beta1, beta2, epsilon), grad_scale);
  DTR_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------- update
// FlatWalk's step: a rotated segment takes soap_descend along N (its m and v are
// soap_rotate_adam's), every other one soap_adam_elem.
struct SoapStep {
  const float* __restrict__ g;
  float* __restrict__ m;
  float* __restrict__ v;
  const float* __restrict__ dir;
  const float* __restrict__ wd_seg;
  const int* __restrict__ pre_seg;
  AdamCoef c;
  float grad_scale, lr, alpha;
  static constexpr bool update = true;

  __device__ __forceinline__ void operator()(int sgi, long e0, f32x4& wv) const {
    const float wd = wd_seg[sgi];
    const float lrwd = lr * wd;
    if (pre_seg[sgi] != 0) {
      const f32x4 dv = ld4<false>(dir + e0);
#pragma unroll
      for (int j = 0; j < 4; ++j) wv[j] = soap_descend(wv[j], dv[j], alpha, lrwd);
      return;
    }
    const f32x4 gv = ld4<false>(g + e0);
    f32x4 mv = ld4<true>(m + e0);
    f32x4 vv = ld4<true>(v + e0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float wj = wv[j], mj = mv[j], vj = vv[j];
      soap_adam_elem(wj, gv[j], mj, vj, grad_scale, lrwd, alpha, c);
      wv[j] = wj;
      mv[j] = mj;
      vv[j] = vj;
    }
    st4<true>(m + e0, mv);
    st4<true>(v + e0, vv);
  }

  __device__ __forceinline__ void operator()(int sgi, long e, float& wj) const {
    const float lrwd = lr * wd_seg[sgi];
    if (pre_seg[sgi] != 0) {
      wj = soap_descend(wj, dir[e], alpha, lrwd);
      return;
    }
    float mj = m[e], vj = v[e];
    soap_adam_elem(wj, g[e], mj, vj, grad_scale, lrwd, alpha, c);
    m[e] = mj;
    v[e] = vj;
  }
};

__global__ void __launch_bounds__(256)
soap_pack_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                 float* __restrict__ v, const float* __restrict__ dir, long n, LrSchedule sched,
                 const long long* __restrict__ gstep, const long long* __restrict__ start,
                 AdamCoef c, float grad_scale, const ParamSeg* __restrict__ segs, int nseg,
                 const float* __restrict__ wd_seg, const int* __restrict__ pre_seg,
                 bf16* __restrict__ bf, float* __restrict__ lr_out, float* __restrict__ adam_out) {
  __shared__ ParamSeg sseg[SEG_LDS_MAX];
  __shared__ float rate_s[2];
  if (threadIdx.x == 0) {
    const long long step = gstep ? *gstep : 0ll;
    const float lr = lr_at(sched, (long)step);
    const BiasCorrection b = bias_correction(step, start, c);
    const float alpha = b.alpha(lr);
    rate_s[0] = lr;
    rate_s[1] = alpha;
    if (blockIdx.x == 0) {
      if (lr_out) *lr_out = lr;
      if (adam_out) {
        adam_out[0] = lr;
        adam_out[1] = alpha;
        adam_out[2] = (float)b.t;
      }
    }
  }
  const FlatWalk walk(sseg, segs, nseg, true);   // the table and the two rates
  walk.run(w, n, bf, SoapStep{g, m, v, dir, wd_seg, pre_seg, c, grad_scale, rate_s[0], rate_s[1]});
}

void soap_update_pack(float* master, const float* grad, float* m, float* v, const float* dir,
                      long n, const LrSchedule& s, const long long* gstep,
                      const long long* start_step, float beta1, float beta2, float epsilon,
                      float grad_scale, const ParamSeg* segs, int nseg, const float* wd_seg,
                      const int* pre_seg, bf16* bf, float* lr_out, float* adam_out,
                      hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(soap_pack_kernel, dim3(flat_blocks(n)), dim3(256), 0, st, master, grad, m, v,
                     dir, n, s, gstep, start_step, adam_coef(beta1, beta2, epsilon), grad_scale,
                     segs, nseg, wd_seg, pre_seg, bf, lr_out, adam_out);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
