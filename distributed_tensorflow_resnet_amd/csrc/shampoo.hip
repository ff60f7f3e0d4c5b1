// Blocked Shampoo (Gupta, Koren, Singer 2018; Anil et al. 2020) with SGD grafting.  A conv
// master tensor in HWIO order is the row-major R x K matrix M (R = kh kw C, K = out), cut into
// ceil(R / 64) x ceil(K / 64) blocks of live size r x k (ragged at the edges).  Per block, with
// G the block of g' = s g, t the 1-based step count and `every` the refresh interval:
//   L' = b2 L + c G G^T (r x r),  Rt' = b2 Rt + c G^T G (k x k)      (b2 = 1: c = 1, the sum)
//   when t % every == 0, for A in (L', Rt'):
//     lam = ||A||_F,  D = A + eps lam I,  z = 5 / (2 ||D||_F),  X = z^(1/4) I,  Mk = z D
//     at most 32 times:  stop if max|Mk - I| < 1e-5;  T = (5 I - Mk) / 4;
//                        Mk = T^4 Mk (T2 = T T, T4 = T2 T2, T4 Mk);  X = X T
//     the root is X ~ D^(-1/4); ending at max|Mk - I| >= 1e-2 or not finite the block keeps its
//     old root and counts as failed
//   U = PL G PR with the roots as they stand (the identity until the first refresh)
// Per tensor c = ||g'||_F / ||U||_F (1 where a norm is not > 0) and the update is mom's with
// c U in place of the gradient.  All matrix arithmetic is fp32 on v_mfma_f32_16x16x4_f32;
// shampoo_device.h has the operand layout.  State: L, Rt, PL, PR as [slot][64][64] fp32, zero
// outside the live part.  Five launches over the host's block table (train/layout.py):
//   shampoo_stats         one workgroup (4 waves) per block: g' staged once into LDS, G G^T from
//                         its rows and G^T G from its columns.  G G^T is symmetric bit for bit (the
//                         same products in the same order), so an accumulator column is stored as
//                         a row of L: 16-byte stores.  The first workgroup clears the failure
//                         counter of a refresh step.
//   shampoo_roots         one workgroup of 8 waves per (block, side); all of them leave at once
//                         unless t % every == 0, read from the step word, so a captured graph
//                         replays it.  Mk, X, T and a scratch block stay in LDS (4 x 17 KB).  A
//                         wave owns one 16-row tile against two column tiles (64 live rows: 8
//                         units, one per wave): X T and T T -> barrier -> T4 = T2 T2 over T ->
//                         barrier -> T4 Mk -> barrier -> Mk', T' and the residual from the
//                         accumulators -> barrier: four per iteration, the exit uniform.  A live
//                         size n is padded to 16 ceil(n / 16) with the identity in Mk and T, which
//                         the live part never meets; only the live part of X is written back.
//   shampoo_precondition  one workgroup per block: T1 = PL G and U = T1 PR through LDS, then one
//                         pass in the staging pass's element order that writes U to dir and sums
//                         g'^2 and U^2 -- the same order for both, so U == g' gives equal sums.
//   shampoo_graft         one wave per tensor: its blocks' partials in table order, c.
//   shampoo_update_pack   a FlatWalk launch: sgd_pack_kernel's roundings with c U in place of s g
//                         for a preconditioned segment.  ohwi_pack follows.
// Sums are fp32 per thread and fp64 from the wave on, in one order; no float atomics.  Products
// by the identity are exact, so before the first refresh U == g', c == 1 and the step is mom's.
#include "shampoo_device.h"

namespace dtr {

constexpr int SH_WAVES = SH_THREADS / 64;                        // stats, precondition
constexpr int SHR_THREADS = 512, SHR_WAVES = SHR_THREADS / 64;   // roots
constexpr int SH_LDS4 = 4 * SH_MAT * (int)sizeof(float);         // four blocks: 69,632 B
constexpr int SH_MAX_ITERS = 32;
constexpr float SH_TOL = 1e-5f, SH_FAIL = 1e-2f;
static_assert(SH_LDS4 + 256 <= 163840, "LDS");

// ---------------------------------------------------------------------------------- stats
// S' = b2 S + c acc for the 4 elements (row, col .. col + 3) of a statistics slot, live size n.
__device__ __forceinline__ void sh_stat_row4(float* __restrict__ S, int row, int col, int n,
                                             float b2, float c, const f32x4& acc) {
  if (row >= n || col >= n) return;
  float* p = S + row * SH_BLOCK + col;
  if (col + 4 <= n) {
    f32x4 o = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int v = 0; v < 4; ++v) o[v] = b2 * o[v] + c * acc[v];
    *reinterpret_cast<f32x4*>(p) = o;
  } else {
    for (int v = 0; v < 4 && col + v < n; ++v) p[v] = b2 * p[v] + c * acc[v];
  }
}

__global__ void __launch_bounds__(SH_THREADS)
shampoo_stats_kernel(const float* __restrict__ grad, const ShampooBlock* __restrict__ tab,
                     float* __restrict__ L, float* __restrict__ Rt, float b2, float c,
                     float grad_scale, const long long* __restrict__ gstep,
                     const long long* __restrict__ start, int every, int* __restrict__ fail) {
  __shared__ __attribute__((aligned(16))) float Gs[SH_MAT];
  if (fail && blockIdx.x == 0 && threadIdx.x == 0 && sh_step(gstep, start) % every == 0) *fail = 0;
  const ShampooBlock b = tab[blockIdx.x];
  sh_stage_grad(grad, b, grad_scale, Gs);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, cc = lane & 15, g = lane >> 4;
  const int ntr = (b.r + 15) >> 4, ntk = (b.k + 15) >> 4;
  float* __restrict__ Ls = L + (long long)b.slot * (SH_BLOCK * SH_BLOCK);
  float* __restrict__ Rs = Rt + (long long)b.slot * (SH_BLOCK * SH_BLOCK);
  for (int u = wave; u < ntr * ntr + ntk * ntk; u += SH_WAVES) {   // uniform per wave
    f32x4 acc[1];
    if (u < ntr * ntr) {          // G G^T: both operands along the rows of Gs
      const int ti = u / ntr, tj = u - ti * ntr;
      sh_tiles<false, true, 1>(Gs, Gs, ti, tj, 16 * ntk, cc, g, acc);
      // lane: C[16 ti + 4 g + v][16 tj + c] == C[16 tj + c][16 ti + 4 g + v]
      sh_stat_row4(Ls, 16 * tj + cc, 16 * ti + 4 * g, b.r, b2, c, acc[0]);
    } else {                      // G^T G: both along its columns
      const int w = u - ntr * ntr, ti = w / ntk, tj = w - ti * ntk;
      sh_tiles<true, false, 1>(Gs, Gs, ti, tj, 16 * ntr, cc, g, acc);
      sh_stat_row4(Rs, 16 * tj + cc, 16 * ti + 4 * g, b.k, b2, c, acc[0]);
    }
  }
}

void shampoo_stats(const float* grad, const ShampooBlock* tab, int nblocks, float* L, float* Rt,
                   float beta2, float grad_scale, const long long* gstep, const long long* start,
                   int every, int* fail, hipStream_t st) {
  if (nblocks <= 0) return;
  const float c = beta2 == 1.f ? 1.f : (float)(1.0 - (double)beta2);
  hipLaunchKernelGGL(shampoo_stats_kernel, dim3(nblocks), dim3(SH_THREADS), 0, st, grad, tab, L,
                     Rt, beta2, c, grad_scale, gstep, start, every, fail);
  DTR_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------- roots
__device__ __forceinline__ float sh_dev(float m, bool diag) {
  const float d = fabsf(m - (diag ? 1.f : 0.f));
  return d <= 3.0e38f ? d : __builtin_inff();   // NaN and inf alike
}

__device__ __forceinline__ float sh_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ void __launch_bounds__(SHR_THREADS)
shampoo_roots_kernel(const ShampooBlock* __restrict__ tab, const float* __restrict__ L,
                     const float* __restrict__ Rt, float* __restrict__ PL, float* __restrict__ PR,
                     const long long* __restrict__ gstep, const long long* __restrict__ start,
                     int every, float eps, int* __restrict__ fail) {
  if (sh_step(gstep, start) % every != 0) return;   // the same word for every thread
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Mk = reinterpret_cast<float*>(smem);
  float* X = Mk + SH_MAT;
  float* T = X + SH_MAT;
  float* Sc = T + SH_MAT;
  double* red = reinterpret_cast<double*>(Sc + SH_MAT);   // [2][8]
  float* redf = reinterpret_cast<float*>(red + 2 * SHR_WAVES);   // [8]
  const ShampooBlock b = tab[blockIdx.x];
  const bool right = blockIdx.y != 0;
  const int n = right ? b.k : b.r, nt = (n + 15) >> 4, np = 16 * nt;
  const float* __restrict__ A = (right ? Rt : L) + (long long)b.slot * (SH_BLOCK * SH_BLOCK);
  float* __restrict__ P = (right ? PR : PL) + (long long)b.slot * (SH_BLOCK * SH_BLOCK);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, cc = lane & 15, g = lane >> 4;
  // A (zero outside its live part) into Mk, lam = ||A||_F
  float ss = 0.f;
  for (int q = tid; q < np * 16; q += SHR_THREADS) {
    const int i = q >> 4, j4 = (q & 15) << 2;
    if (j4 < np) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(A + i * SH_BLOCK + j4);
      *reinterpret_cast<f32x4*>(Mk + i * SH_S + j4) = v;
#pragma unroll
      for (int u = 0; u < 4; ++u) ss = __builtin_fmaf(v[u], v[u], ss);
    }
  }
  const float lam = (float)sqrt(sh_block_sum<SHR_WAVES>(ss, red));
  // D = A + eps lam I on the live diagonal; z = 5 / (2 ||D||_F).  (Every pass from here on
  // walks the np x np elements in one thread assignment: a thread meets its own stores.)
  const float ridge = eps * lam;
  ss = 0.f;
  for (int q = tid; q < np * np; q += SHR_THREADS) {
    const int i = q / np, j = q - i * np;
    float d = Mk[i * SH_S + j];
    if (i == j && i < n) {
      d += ridge;
      Mk[i * SH_S + j] = d;
    }
    ss = __builtin_fmaf(d, d, ss);
  }
  const float z = 2.5f / (float)sqrt(sh_block_sum<SHR_WAVES>(ss, red + SHR_WAVES));
  const float zq = sqrtf(sqrtf(z));
  // Mk = z D, X = z^(1/4) I, T = (5 I - Mk) / 4; the padding carries the identity in Mk and T
  float dev = 0.f;
  for (int q = tid; q < np * np; q += SHR_THREADS) {
    const int i = q / np, j = q - i * np;
    const bool diag = i == j;
    const float m = diag && i >= n ? 1.f : z * Mk[i * SH_S + j];
    Mk[i * SH_S + j] = m;
    X[i * SH_S + j] = diag ? zq : 0.f;
    T[i * SH_S + j] = ((diag ? 5.f : 0.f) - m) * 0.25f;
    dev = fmaxf(dev, sh_dev(m, diag));
  }
  dev = sh_wave_max(dev);
  if (lane == 0) redf[wave] = dev;
  lds_barrier();
  float res = redf[0];
#pragma unroll
  for (int w = 1; w < SHR_WAVES; ++w) res = fmaxf(res, redf[w]);
  // the wave's unit: tile row ti against the column tiles tj0, tj0 + 1 (nt <= 4: at most 8 units)
  const int hp = (nt + 1) >> 1;
  const bool active = wave < nt * hp;
  const int ti = active ? wave / hp : 0, tj0 = active ? 2 * (wave - ti * hp) : 0;
  const bool two = tj0 + 1 < nt;
  for (int it = 0; it < SH_MAX_ITERS && res >= SH_TOL && res <= 3.0e38f; ++it) {   // uniform
    f32x4 ax[2], as[2];
    if (active) {
      if (two) {
        sh_tiles<false, false, 2>(X, T, ti, tj0, np, cc, g, ax);
        sh_tiles<false, false, 2>(T, T, ti, tj0, np, cc, g, as);
      } else {
        f32x4 a1[1];
        sh_tiles<false, false, 1>(X, T, ti, tj0, np, cc, g, a1);
        ax[0] = a1[0];
        sh_tiles<false, false, 1>(T, T, ti, tj0, np, cc, g, a1);
        as[0] = a1[0];
      }
      sh_store_tile(Sc, ti, tj0, cc, g, as[0]);                 // T2 (nothing reads Sc now)
      if (two) sh_store_tile(Sc, ti, tj0 + 1, cc, g, as[1]);
    }
    lds_barrier();   // every read of X and T is done, T2 is complete
    if (active) {
      sh_store_tile(X, ti, tj0, cc, g, ax[0]);                  // X = X T
      if (two) sh_store_tile(X, ti, tj0 + 1, cc, g, ax[1]);
      if (two) {
        sh_tiles<false, false, 2>(Sc, Sc, ti, tj0, np, cc, g, as);
      } else {
        f32x4 a1[1];
        sh_tiles<false, false, 1>(Sc, Sc, ti, tj0, np, cc, g, a1);
        as[0] = a1[0];
      }
      sh_store_tile(T, ti, tj0, cc, g, as[0]);                  // T4 over T
      if (two) sh_store_tile(T, ti, tj0 + 1, cc, g, as[1]);
    }
    lds_barrier();   // T4 is complete
    if (active) {
      if (two) {
        sh_tiles<false, false, 2>(T, Mk, ti, tj0, np, cc, g, as);
      } else {
        f32x4 a1[1];
        sh_tiles<false, false, 1>(T, Mk, ti, tj0, np, cc, g, a1);
        as[0] = a1[0];
      }
    }
    lds_barrier();   // every read of T4 and Mk is done
    dev = 0.f;
    if (active) {
#pragma unroll
      for (int bb = 0; bb < 2; ++bb) {
        if (bb == 0 || two) {
          const int col = 16 * (tj0 + bb) + cc;
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int row = 16 * ti + 4 * g + v;
            const float m = as[bb][v];
            Mk[row * SH_S + col] = m;
            T[row * SH_S + col] = ((row == col ? 5.f : 0.f) - m) * 0.25f;
            dev = fmaxf(dev, sh_dev(m, row == col));
          }
        }
      }
    }
    dev = sh_wave_max(dev);
    if (lane == 0) redf[wave] = dev;
    lds_barrier();
    res = redf[0];
#pragma unroll
    for (int w = 1; w < SHR_WAVES; ++w) res = fmaxf(res, redf[w]);
  }
  if (!(res < SH_FAIL)) {   // not converged, or not finite: the old root stays
    if (tid == 0 && fail) atomicAdd(fail, 1);
    return;
  }
  for (int q = tid; q < n * n; q += SHR_THREADS) {
    const int i = q / n, j = q - i * n;
    P[i * SH_BLOCK + j] = X[i * SH_S + j];
  }
}

void shampoo_roots(const ShampooBlock* tab, int nblocks, int sides, const float* L, const float* Rt,
                   float* PL, float* PR, const long long* gstep, const long long* start, int every,
                   float epsilon, int* fail, hipStream_t st) {
  if (nblocks <= 0) return;
  const int lds = SH_LDS4 + 2 * SHR_WAVES * (int)sizeof(double) + SHR_WAVES * (int)sizeof(float);
  hipLaunchKernelGGL(shampoo_roots_kernel, dim3(nblocks, sides), dim3(SHR_THREADS), lds, st, tab, L,
                     Rt, PL, PR, gstep, start, every, epsilon, fail);
  DTR_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------- direction
__global__ void __launch_bounds__(SH_THREADS)
shampoo_precondition_kernel(const float* __restrict__ grad, const ShampooBlock* __restrict__ tab,
                            const float* __restrict__ PL, const float* __restrict__ PR,
                            float* __restrict__ dir, double* __restrict__ part, float grad_scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Gs = reinterpret_cast<float*>(smem);
  float* Ps = Gs + SH_MAT;    // PL, later U
  float* Qs = Ps + SH_MAT;    // PR
  float* Ts = Qs + SH_MAT;    // PL G
  double* red = reinterpret_cast<double*>(Ts + SH_MAT);   // [2][4]
  const ShampooBlock b = tab[blockIdx.x];
  sh_stage_grad(grad, b, grad_scale, Gs);
  sh_stage_slot(PL + (long long)b.slot * (SH_BLOCK * SH_BLOCK), Ps);
  sh_stage_slot(PR + (long long)b.slot * (SH_BLOCK * SH_BLOCK), Qs);
  lds_barrier();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, cc = lane & 15, g = lane >> 4;
  const int ntr = (b.r + 15) >> 4, ntk = (b.k + 15) >> 4;
  f32x4 acc[1];
  for (int u = wave; u < ntr * ntk; u += SH_WAVES) {   // T1 = PL G
    const int ti = u / ntk, tj = u - ti * ntk;
    sh_tiles<false, false, 1>(Ps, Gs, ti, tj, 16 * ntr, cc, g, acc);
    sh_store_tile(Ts, ti, tj, cc, g, acc[0]);
  }
  lds_barrier();   // PL is read, T1 complete
  for (int u = wave; u < ntr * ntk; u += SH_WAVES) {   // U = T1 PR, over PL's block
    const int ti = u / ntk, tj = u - ti * ntk;
    sh_tiles<false, false, 1>(Ts, Qs, ti, tj, 16 * ntk, cc, g, acc);
    sh_store_tile(Ps, ti, tj, cc, g, acc[0]);
  }
  lds_barrier();
  // U out and both sums, element for element in one order
  const bool vec = ((b.offset | (long long)b.K | (long long)b.k) & 3) == 0;
  float sg = 0.f, su = 0.f;
  for (int q = threadIdx.x; q < SH_BLOCK * 16; q += SH_THREADS) {
    const int i = q >> 4, j4 = (q & 15) << 2;
    if (i < b.r && j4 < b.k) {
      const f32x4 gv = *reinterpret_cast<const f32x4*>(Gs + i * SH_S + j4);
      const f32x4 uv = *reinterpret_cast<const f32x4*>(Ps + i * SH_S + j4);
      float* p = dir + b.offset + (long long)i * b.K + j4;
      if (vec) *reinterpret_cast<f32x4*>(p) = uv;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (j4 + u < b.k) {
          if (!vec) p[u] = uv[u];
          sg = __builtin_fmaf(gv[u], gv[u], sg);
          su = __builtin_fmaf(uv[u], uv[u], su);
        }
      }
    }
  }
  const double tg = sh_block_sum<SH_WAVES>(sg, red);
  const double tu = sh_block_sum<SH_WAVES>(su, red + SH_WAVES);
  if (threadIdx.x == 0) {
    part[2 * (long long)blockIdx.x] = tg;
    part[2 * (long long)blockIdx.x + 1] = tu;
  }
}

void shampoo_precondition(const float* grad, const ShampooBlock* tab, int nblocks, const float* PL,
                          const float* PR, float* dir, double* part, float grad_scale,
                          hipStream_t st) {
  if (nblocks <= 0) return;
  const int lds = SH_LDS4 + 2 * SH_WAVES * (int)sizeof(double);
  hipLaunchKernelGGL(shampoo_precondition_kernel, dim3(nblocks), dim3(SH_THREADS), lds, st, grad,
                     tab, PL, PR, dir, part, grad_scale);
  DTR_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------- grafting
__global__ void __launch_bounds__(64)
shampoo_graft_kernel(const double* __restrict__ part, const ShampooTensor* __restrict__ ttab,
                     int nseg, float* __restrict__ out) {
  const ShampooTensor t = ttab[blockIdx.x];
  const LarsSeg ls{t.block0, t.nblocks, 0};
  double s0, s1;
  seg_part_sums(part, ls, s0, s1);
  if (threadIdx.x == 0) {
    const double gn = sqrt(s0), un = sqrt(s1);
    out[t.seg] = gn > 0.0 && un > 0.0 ? (float)(gn / un) : 1.f;
    out[nseg + t.seg] = (float)gn;
    out[2 * nseg + t.seg] = (float)un;
  }
}

void shampoo_graft(const double* part, const ShampooTensor* ttab, int ntensors, int nseg,
                   float* out, hipStream_t st) {
  if (ntensors <= 0) return;
  hipLaunchKernelGGL(shampoo_graft_kernel, dim3(ntensors), dim3(64), 0, st, part, ttab, nseg, out);
  DTR_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------- update
// SgdStep<false>'s update with momentum, written out with the roundings sgd_pack_kernel has on
// its two paths (tests/golden/optim_bits.json pins them; muon.hip's MuonAuxStep has the story):
//   four elements: gv = fma(wd, w, d);  one element: gv = wd w + d, both products rounded;
//   then acc = fma(momentum, m, gv), w' = fma(-lr, acc, w)
// with d = s g, or c U (one rounding) for a preconditioned segment.
struct ShampooStep {
  const float* __restrict__ g;
  float* __restrict__ mom;
  const float* __restrict__ dir;
  const int* __restrict__ pre_seg;
  const float* __restrict__ graft;
  float lr, momentum, wd, grad_scale;
  static constexpr bool update = true;

  __device__ __forceinline__ void tail(float gv, float& m, float& w) const {
    m = __builtin_fmaf(momentum, m, gv);
    w = __builtin_fmaf(-lr, m, w);
  }

  __device__ __forceinline__ void operator()(int sgi, long e0, f32x4& wv) const {
#pragma clang fp contract(off)
    const bool pre = pre_seg[sgi] != 0;
    const f32x4 dv = ld4<false>((pre ? dir : g) + e0);
    const float s = pre ? graft[sgi] : grad_scale;
    f32x4 mv = ld4<false>(mom + e0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = dv[j] * s;
      float mj = mv[j], wj = wv[j];
      tail(__builtin_fmaf(wd, wj, d), mj, wj);
      mv[j] = mj;
      wv[j] = wj;
    }
    st4<false>(mom + e0, mv);
  }

  __device__ __forceinline__ void operator()(int sgi, long e, float& wj) const {
#pragma clang fp contract(off)
    const bool pre = pre_seg[sgi] != 0;
    const float dec = wd * wj;
    const float d = (pre ? dir[e] : g[e]) * (pre ? graft[sgi] : grad_scale);
    float mj = mom[e];
    tail(dec + d, mj, wj);
    mom[e] = mj;
  }
};

__global__ void __launch_bounds__(256)
shampoo_pack_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ mom,
                    const float* __restrict__ dir, long n, LrSchedule sched,
                    const long long* __restrict__ gstep, float momentum, float wd,
                    float grad_scale, const ParamSeg* __restrict__ segs, int nseg,
                    const int* __restrict__ pre_seg, const float* __restrict__ graft,
                    bf16* __restrict__ bf, float* __restrict__ lr_out) {
  __shared__ ParamSeg sseg[SEG_LDS_MAX];
  __shared__ float lr_s;
  if (threadIdx.x == 0) {
    const float lr = lr_at(sched, gstep ? (long)*gstep : 0L);
    lr_s = lr;
    if (lr_out && blockIdx.x == 0) *lr_out = lr;
  }
  const FlatWalk walk(sseg, segs, nseg, true);   // the table and the rate
  walk.run(w, n, bf, ShampooStep{g, mom, dir, pre_seg, graft, lr_s, momentum, wd, grad_scale});
}

void shampoo_update_pack(float* master, const float* grad, float* mom, const float* dir, long n,
                         const LrSchedule& s, const long long* gstep, float momentum, float wd,
                         float grad_scale, const ParamSeg* segs, int nseg, const int* pre_seg,
                         const float* graft, bf16* bf, float* lr_out, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(shampoo_pack_kernel, dim3(flat_blocks(n)), dim3(256), 0, st, master, grad, mom,
                     dir, n, s, gstep, momentum, wd, grad_scale, segs, nseg, pre_seg, graft, bf,
                     lr_out);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
