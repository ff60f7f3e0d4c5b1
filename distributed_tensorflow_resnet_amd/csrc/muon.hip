// Muon (Jordan et al. 2024): momentum, then the momentum matrix of every conv kernel is
// orthogonalised by a quintic Newton-Schulz iteration before it moves the weight.  A conv
// master tensor in HWIO order is the row-major R x K matrix M (R = kh kw C, K = out).  With
// s the gradient's scale, mu the momentum and (a, b, c) = (3.4445, -4.7750, 2.0315):
//   g' = s g,  m' = mu m + g',  u = g' + mu m' (Nesterov) or m'
//   X  = bf16(u / (||u||_F + 1e-7)), oriented short x long (X = M^T if K <= R, else M)
//   steps times:  A = bf16(X X^T),  B = bf16(b A + c (A A)),  X = bf16(a X + B X)
//   O  = X in M's orientation;   w' = (w - (lr wd) w) - (lr q) O,  q = sqrt(max(1, K / R))
// Every other trainable tensor takes SgdStep<false>'s update at the rate lr * aux_scale.
//
// Launch 1, muon_orthogonalize: ONE workgroup of 512 threads (8 waves) per conv tensor, the
// whole iteration on chip.  It covers a short side <= 64 and a long side <= 576
// (muon_covers): every conv kernel of the CIFAR networks.
//   * Pass 1 reads g and m (scalar, coalesced), stores m' and sums u^2 per thread in fp32;
//     the thread sums are added in fp64 by the wave's shuffles and over the eight waves left
//     to right: no atomics, one order, so two launches and two ranks give the same bits.
//     Pass 2 forms u again from g and the m' just stored (the same roundings) and stages X0.
//   * LDS holds TWO bf16 copies of X.  X[s][l + 8] (long side contiguous) feeds X X^T: both
//     MFMA operands are rows of it, 16 bytes per lane; the 8 elements of row padding turn the
//     row stride into 16 m + 4 dwords, so the 16 rows of an operand fall on 16 different
//     bank groups (unpadded, 576 elements are 288 dwords and the rows alternate between two).
//     XT[l][SP] (short side contiguous) feeds B X as its B operand, again 16 bytes per lane.
//     The accumulator of B X holds 4 consecutive short-side elements of one long-side
//     column, so the new X goes back to XT as ONE 8-byte store and to X as four 2-byte
//     stores.  64 x 576: 74,752 + 73,728 B, plus 8 KB for A and B, which share a buffer.
//     profiles/muon.md has the reasoning and the options that were not built.
//   * A and B are symmetric: A[i][j] and A[j][i] are the same products added in the same
//     order, and so are B's.  That is used three times -- the second operand of A A and of
//     B X is read along rows, and an accumulator column is stored as a row (8 bytes).
//   * Zero padding: the short side is padded to SP (a multiple of 32: it is the reduction
//     length of A A and B X) and the long side to LP (a multiple of 32: X X^T's).  All of LDS
//     that is read is cleared first; zero rows and columns stay zero through the iteration
//     and the write-out walks the tensor's own elements only.
//   * Work split.  X X^T: a unit is one 16-row tile of A against TWO column tiles (three
//     operand loads per two MFMAs); 64 rows give 8 units, one per wave, 2 x 18 MFMAs each.
//     A A: one tile per wave and round (16 tiles at s = 64), the results held in registers
//     across the barrier behind which B overwrites A.  B X: a wave owns 16 long-side columns
//     at a time (36 blocks over 8 waves), keeps all of B in registers (at most 8 operands)
//     and updates its columns of XT in place: every store depends on all of the wave's
//     operand loads, so nothing it reads is overwritten early.  64 x 576: 288 + 32 + 288
//     MFMAs and four barriers per step.
//   * grad is only read; O goes out as fp32 to dir at the tensor's offset.
// Launch 2, muon_update_pack: a FlatWalk launch in lion_update_pack's shape.  muon_seg[segment]
// != 0: the weight update above from dir, contraction off, one rounding per operation; the
// other segments take SgdStep<false>'s update at lr * aux_scale with sgd_pack_kernel's own
// roundings (MuonAuxStep), bit for bit what `mom` gives them.  ohwi_pack follows.
#include "muon_device.h"

namespace dtr {

constexpr int MUON_SHORT = 64, MUON_LONG = 576;   // muon_covers
constexpr int MUON_THREADS = 512, MUON_WAVES = MUON_THREADS / 64;
constexpr int MUON_XPAD = 8;                      // elements of padding per row of X
constexpr int MUON_X_B = MUON_SHORT * (MUON_LONG + MUON_XPAD) * 2;
constexpr int MUON_XT_B = MUON_LONG * MUON_SHORT * 2;
constexpr int MUON_AB_B = MUON_SHORT * MUON_SHORT * 2;
constexpr int MUON_LDS = MUON_X_B + MUON_XT_B + MUON_AB_B + MUON_WAVES * 8;
static_assert(MUON_LDS <= 163840, "LDS");

bool muon_covers(int R, int K) {
  const int s = R < K ? R : K, l = R < K ? K : R;
  return s >= 1 && s <= MUON_SHORT && l <= MUON_LONG;
}

// Element (short i, long c) of XT.
__device__ __forceinline__ int xt_at(int c, int i, int SP) { return c * SP + i; }

// The Newton-Schulz steps for ST 16-row tiles of the short side; SP = 32 * KS.
template <int ST>
__device__ __forceinline__ void muon_iterate(bf16* __restrict__ X, bf16* __restrict__ XT,
                                             bf16* __restrict__ AB, int XS, int LP, int steps) {
  constexpr int KS = (ST + 1) / 2, SP = 32 * KS, HP = (ST + 1) / 2;
  constexpr int T2 = (ST * ST + MUON_WAVES - 1) / MUON_WAVES;   // A A tiles per wave
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  for (int it = 0; it < steps; ++it) {
    // A = bf16(X X^T): rows ti of A against the column tiles tj0, tj0 + 1
    for (int u = wave; u < ST * HP; u += MUON_WAVES) {
      const int ti = u / HP, tj0 = 2 * (u - ti * HP);
      const bool two = tj0 + 1 < ST;
      const bf16* pa = X + (ti * 16 + c) * XS + 8 * g;
      const bf16* pb0 = X + (tj0 * 16 + c) * XS + 8 * g;
      const bf16* pb1 = two ? pb0 + 16 * XS : pb0;
      f32x4 acc0 = {}, acc1 = {};
      for (int k = 0; k < LP; k += 32) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(pa + k);
        acc0 = mfma16(a, *reinterpret_cast<const bf16x8*>(pb0 + k), acc0);
        if (two) acc1 = mfma16(a, *reinterpret_cast<const bf16x8*>(pb1 + k), acc1);
      }
      // lane: A[ti 16 + 4 g + i][tj 16 + c], stored as row tj 16 + c (A is symmetric)
      const bf16x4 h0 = {(bf16)acc0[0], (bf16)acc0[1], (bf16)acc0[2], (bf16)acc0[3]};
      *reinterpret_cast<bf16x4*>(AB + (tj0 * 16 + c) * SP + ti * 16 + 4 * g) = h0;
      if (two) {
        const bf16x4 h1 = {(bf16)acc1[0], (bf16)acc1[1], (bf16)acc1[2], (bf16)acc1[3]};
        *reinterpret_cast<bf16x4*>(AB + ((tj0 + 1) * 16 + c) * SP + ti * 16 + 4 * g) = h1;
      }
    }
    lds_barrier();
    // B = bf16(b A + c (A A)), in registers until every wave has read A
    bf16x4 bv[T2];
#pragma unroll
    for (int r = 0; r < T2; ++r) {
      const int t = wave + r * MUON_WAVES;
      if (t < ST * ST) {
        const int ti = t / ST, tj = t - ti * ST;
        f32x4 acc = {};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          acc = mfma16(*reinterpret_cast<const bf16x8*>(AB + (ti * 16 + c) * SP + ks * 32 + 8 * g),
                       *reinterpret_cast<const bf16x8*>(AB + (tj * 16 + c) * SP + ks * 32 + 8 * g),
                       acc);
        const bf16x4 av = *reinterpret_cast<const bf16x4*>(AB + (tj * 16 + c) * SP + ti * 16 + 4 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) bv[r][i] = (bf16)(NS_B * (float)av[i] + NS_C * acc[i]);
      }
    }
    lds_barrier();
#pragma unroll
    for (int r = 0; r < T2; ++r) {
      const int t = wave + r * MUON_WAVES;
      if (t < ST * ST) {
        const int ti = t / ST, tj = t - ti * ST;
        *reinterpret_cast<bf16x4*>(AB + (tj * 16 + c) * SP + ti * 16 + 4 * g) = bv[r];
      }
    }
    lds_barrier();
    // X = bf16(a X + B X): all of B in registers, 16 long-side columns at a time, in place
    bf16x8 breg[ST][KS];
#pragma unroll
    for (int rt = 0; rt < ST; ++rt)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        breg[rt][ks] = *reinterpret_cast<const bf16x8*>(AB + (rt * 16 + c) * SP + ks * 32 + 8 * g);
    for (int cb = wave; cb < LP / 16; cb += MUON_WAVES) {
      const int col = cb * 16 + c;
      bf16x8 xk[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        xk[ks] = *reinterpret_cast<const bf16x8*>(XT + xt_at(col, ks * 32 + 8 * g, SP));
      f32x4 acc[ST];
#pragma unroll
      for (int rt = 0; rt < ST; ++rt) {
        const bf16x4 x0 = *reinterpret_cast<const bf16x4*>(XT + xt_at(col, rt * 16 + 4 * g, SP));
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[rt][i] = NS_A * (float)x0[i];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) acc[rt] = mfma16(breg[rt][ks], xk[ks], acc[rt]);
      }
#pragma unroll
      for (int rt = 0; rt < ST; ++rt) {
        const bf16x4 h = {(bf16)acc[rt][0], (bf16)acc[rt][1], (bf16)acc[rt][2], (bf16)acc[rt][3]};
        *reinterpret_cast<bf16x4*>(XT + xt_at(col, rt * 16 + 4 * g, SP)) = h;
#pragma unroll
        for (int i = 0; i < 4; ++i) X[(rt * 16 + 4 * g + i) * XS + col] = h[i];
      }
    }
    lds_barrier();
  }
}

__global__ void __launch_bounds__(MUON_THREADS)
muon_orthogonalize_kernel(const float* __restrict__ grad, float* __restrict__ mom,
                          float* __restrict__ dir, const MuonTensor* __restrict__ tab, float mu,
                          int nesterov, int steps, float grad_scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* X = reinterpret_cast<bf16*>(smem);
  bf16* XT = reinterpret_cast<bf16*>(smem + MUON_X_B);
  bf16* AB = reinterpret_cast<bf16*>(smem + MUON_X_B + MUON_XT_B);
  double* red = reinterpret_cast<double*>(smem + MUON_X_B + MUON_XT_B + MUON_AB_B);
  const MuonTensor t = tab[blockIdx.x];
  const int tid = threadIdx.x, R = t.R, K = t.K, n = R * K;
  const bool tr = t.transpose != 0;   // X = M^T: short index = column of M
  const int s = tr ? K : R, l = tr ? R : K;
  const int ST = (s + 15) / 16, SP = 32 * ((ST + 1) / 2), LP = (l + 31) & ~31, XS = LP + MUON_XPAD;
  const float* __restrict__ g = grad + t.offset;
  float* __restrict__ m = mom + t.offset;
  // pass 1: m' and the thread's share of ||u||^2
  float ss = 0.f;
  for (int e = tid; e < n; e += MUON_THREADS) {
    float mj = m[e], u;
    muon_moment(g[e], mj, grad_scale, mu, nesterov, u);
    m[e] = mj;
    ss += u * u;
  }
  const double ws = wave_sum_f64((double)ss);
  if ((tid & 63) == 0) red[tid >> 6] = ws;
  // everything of LDS that the iteration reads, cleared in 16-byte stores
  const f32x4 z = {};
  for (int i = tid; i < ST * 16 * XS / 8; i += MUON_THREADS) reinterpret_cast<f32x4*>(X)[i] = z;
  for (int i = tid; i < LP * SP / 8; i += MUON_THREADS) reinterpret_cast<f32x4*>(XT)[i] = z;
  for (int i = tid; i < ST * 16 * SP / 8; i += MUON_THREADS) reinterpret_cast<f32x4*>(AB)[i] = z;
  __syncthreads();   // (global too: pass 2 reads m' where this thread stored it, but be plain)
  double tot = red[0];
#pragma unroll
  for (int w = 1; w < MUON_WAVES; ++w) tot += red[w];
  const float den = sqrtf((float)tot) + 1e-7f;
  // pass 2: X0 = bf16(u / (||u|| + 1e-7)) into both copies
  for (int e = tid; e < n; e += MUON_THREADS) {
    float mj = m[e], u;
    if (nesterov) {
#pragma clang fp contract(off)
      const float gp = grad_scale * g[e];
      const float tt = mu * mj;
      u = gp + tt;
    } else {
      u = mj;
    }
    const int r = e / K, k = e - r * K;
    const int i = tr ? k : r, c = tr ? r : k;
    const bf16 x = (bf16)(u / den);
    X[i * XS + c] = x;
    XT[xt_at(c, i, SP)] = x;
  }
  lds_barrier();
  switch (ST) {   // uniform over the workgroup
    case 1: muon_iterate<1>(X, XT, AB, XS, LP, steps); break;
    case 2: muon_iterate<2>(X, XT, AB, XS, LP, steps); break;
    case 3: muon_iterate<3>(X, XT, AB, XS, LP, steps); break;
    default: muon_iterate<4>(X, XT, AB, XS, LP, steps); break;
  }
  float* __restrict__ o = dir + t.offset;
  for (int e = tid; e < n; e += MUON_THREADS) {
    const int r = e / K, k = e - r * K;
    o[e] = (float)X[(tr ? k : r) * XS + (tr ? r : k)];
  }
}

void muon_orthogonalize(const float* grad, float* mom, float* dir, const MuonTensor* tab,
                        int ntensors, float momentum, int nesterov, int steps, float grad_scale,
                        hipStream_t st) {
  if (ntensors <= 0) return;
  hipLaunchKernelGGL(muon_orthogonalize_kernel, dim3(ntensors), dim3(MUON_THREADS), MUON_LDS, st,
                     grad, mom, dir, tab, momentum, nesterov, steps, grad_scale);
  DTR_CHECK_LAUNCH();
}

__device__ __forceinline__ void muon_elem(float& w, float d, float lrwd, float lrq) {
#pragma clang fp contract(off)
  const float dec = lrwd * w;
  const float kept = w - dec;
  const float step = lrq * d;
  w = kept - step;
}

// SgdStep<false>'s update with momentum for the other segments, written out with the roundings
// that sgd_pack_kernel has on its two paths (tests/golden/optim_bits.json pins them), so that
// such a tensor moves exactly as under `mom`: left to the compiler, this kernel contracted
// g' + wd w the other way round (fma(s, g, wd w)), one ulp off in about 2 % of the elements.
//   four elements: gv = fma(wd, w, s g);  one element: gv = wd w + s g, both products rounded;
//   then acc = fma(momentum, m, gv), w' = fma(-rate, acc, w).
struct MuonAuxStep {
  const float* __restrict__ g;
  float* __restrict__ mom;
  float rate, momentum, wd, grad_scale;

  __device__ __forceinline__ void tail(float gv, float& m, float& w) const {
    m = __builtin_fmaf(momentum, m, gv);
    w = __builtin_fmaf(-rate, m, w);
  }

  __device__ __forceinline__ void operator()(long e0, f32x4& wv) const {
#pragma clang fp contract(off)
    const f32x4 gv = ld4<false>(g + e0);
    f32x4 mv = ld4<false>(mom + e0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float sg = gv[j] * grad_scale;
      float mj = mv[j], wj = wv[j];
      tail(__builtin_fmaf(wd, wj, sg), mj, wj);
      mv[j] = mj;
      wv[j] = wj;
    }
    st4<false>(mom + e0, mv);
  }

  __device__ __forceinline__ void operator()(long e, float& wj) const {
#pragma clang fp contract(off)
    const float dec = wd * wj;
    const float sg = g[e] * grad_scale;
    float mj = mom[e];
    tail(dec + sg, mj, wj);
    mom[e] = mj;
  }
};

// FlatWalk's step: a muon segment moves along dir, any other takes MuonAuxStep at lr_aux.
struct MuonStep {
  const float* __restrict__ dir;
  const int* __restrict__ muon_seg;
  const float* __restrict__ q_seg;
  MuonAuxStep aux;
  float lr, wd;
  static constexpr bool update = true;

  __device__ __forceinline__ void operator()(int sgi, long e0, f32x4& wv) const {
    if (muon_seg[sgi]) {
      const f32x4 dv = ld4<false>(dir + e0);
      const float lrwd = lr * wd, lrq = lr * q_seg[sgi];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float wj = wv[j];
        muon_elem(wj, dv[j], lrwd, lrq);
        wv[j] = wj;
      }
    } else {
      aux(e0, wv);
    }
  }

  __device__ __forceinline__ void operator()(int sgi, long e, float& wj) const {
    if (muon_seg[sgi]) muon_elem(wj, dir[e], lr * wd, lr * q_seg[sgi]);
    else aux(e, wj);
  }
};

__global__ void __launch_bounds__(256)
muon_pack_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ mom,
                 const float* __restrict__ dir, long n, LrSchedule sched,
                 const long long* __restrict__ gstep, float momentum, float wd, float aux_scale,
                 float grad_scale, const ParamSeg* __restrict__ segs, int nseg,
                 const int* __restrict__ muon_seg, const float* __restrict__ q_seg,
                 bf16* __restrict__ bf, float* __restrict__ lr_out) {
  __shared__ ParamSeg sseg[SEG_LDS_MAX];
  __shared__ float lr_s;
  if (threadIdx.x == 0) {
    const float lr = lr_at(sched, gstep ? (long)*gstep : 0L);
    lr_s = lr;
    if (lr_out && blockIdx.x == 0) *lr_out = lr;
  }
  const FlatWalk walk(sseg, segs, nseg, true);   // the table and the rate
  const float lr = lr_s;
  walk.run(w, n, bf,
           MuonStep{dir, muon_seg, q_seg,
                    MuonAuxStep{g, mom, lr * aux_scale, momentum, wd, grad_scale},
                    lr, wd});
}

void muon_update_pack(float* master, const float* grad, float* mom, const float* dir, long n,
                      const LrSchedule& s, const long long* gstep, float momentum, float wd,
                      float aux_scale, float grad_scale, const ParamSeg* segs, int nseg,
                      const int* muon_seg, const float* q_seg, bf16* bf, float* lr_out,
                      hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(muon_pack_kernel, dim3(flat_blocks(n)), dim3(256), 0, st, master, grad, mom,
                     dir, n, s, gstep, momentum, wd, aux_scale, grad_scale, segs, nseg, muon_seg,
                     q_seg, bf, lr_out);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
