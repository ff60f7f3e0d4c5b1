// Persistent small-batch CIFAR step, the backward: the dgrad chain with its BatchNorm
// backwards and the 52 weight gradients in one launch, plus the two small kernels that
// go with it (the head's batch folds, the comm stream's bucket wait).  The design, the
// hand-off protocol and the device primitives are in prn_device.h.
#include "prn_device.h"

namespace dtr {

namespace {

// =====================================================================================
// backward
// =====================================================================================
// (dgrad weights for w_prefetch / w_store: see WLoad)
__device__ __forceinline__ WLoad wl_dgrad(const bf16* src, int co, int ci, int ks) {
  const int K = ks * ks * co;
  return WLoad{src, ci, K, kpad_of(K), 1, ci, co, __frcp_rn((float)(K / 8)), __builtin_ctz(co / 8),
               __builtin_ctz(ci)};
}

// Stride-2 dgrad into output stage SO (high resolution, parity-class-major pixels), slice
// k, from the output gradient of CO channels at resolution R_SO / 2 in the halo `hal`
// (slice rows RS_SO / 2 + 2 halo rows):
//   3x3 (PROJ = false): dx(2i+a, 2j+b) = sum over taps r = a+1 (mod 2), s = b+1 (mod 2)
//     of dy(i + di, j + dj) W[r][s], di = (a + 1 - r) / 2 -- 1, 2, 2 or 4 taps per class;
//   1x1 (PROJ): dx(2i, 2j) = dy(i, j) Wp (class 0 only).
// Weights [ci][k = tap * CO + co].  A wave's pixel blocks all lie in one class.
template <int SO, int P, int CO, bool PROJ>
__device__ __forceinline__ void dgrad_s2_acc(f32x4 (&acc)[8], const bf16* hal, const bf16* wl,
                                             int kslice, int wave, int lane) {
  using G = Stg<SO, P>;
  lane = opaque_v(lane);
  static_assert(G::CLS, "class-major output");
  if (!wave_active<SO, P>(wave)) return;
  constexpr int RL = G::R / 2, RSL = G::RS / 2, W2L = RL + 2, UL = CO / 8;
  constexpr int KP = kpad_of(PROJ ? CO : 9 * CO);
  const int fr = lane & 15, fq = lane >> 4;
  int pb0, cb0;
  tile_of<SO, P>(wave, 0, pb0, cb0);
  const int cls = (pb0 * 16) / (G::NPX / 4);
  const int ca = cls >> 1, cbit = cls & 1;
  if (PROJ && cls != 0) return;
  int il[G::PBW], jl[G::PBW];
#pragma unroll
  for (int i = 0; i < G::PBW; ++i) {
    int pb, cb, h, w;
    tile_of<SO, P>(wave, i * G::CBW, pb, cb);
    canon<SO, P>(kslice, pb * 16 + fr, h, w);
    il[i] = (h >> 1) - kslice * RSL + 1;   // local halo row of dy(i, .)
    jl[i] = (w >> 1) + 1;
  }
  const int nr = PROJ ? 1 : (ca ? 2 : 1), ns = PROJ ? 1 : (cbit ? 2 : 1);
  for (int ri = 0; ri < nr; ++ri) {
    const int r = PROJ ? 0 : (ca ? 2 * ri : 1), di = PROJ ? 0 : (ca ? 1 - ri : 0);
    for (int si = 0; si < ns; ++si) {
      const int s = PROJ ? 0 : (cbit ? 2 * si : 1), dj = PROJ ? 0 : (cbit ? 1 - si : 0);
      const int tap = PROJ ? 0 : r * 3 + s;
#pragma unroll
      for (int kk = 0; kk < CO / 32; ++kk) {
        const int c = kk * 32 + fq * 8;
        const int k = tap * CO + c;
        bf16x8 av[G::CBW];
#pragma unroll
        for (int j = 0; j < G::CBW; ++j) av[j] = lds16(wl + ((cb0 + j) * 16 + fr) * KP + k);
#pragma unroll
        for (int i = 0; i < G::PBW; ++i) {
          const int hr = il[i] + di, hc = jl[i] + dj;
          const bf16x8 b = lds16(hal + haddr<UL>(hr * W2L + hc, hc, c));
#pragma unroll
          for (int j = 0; j < G::CBW; ++j) acc[i * G::CBW + j] = mfma16(av[j], b, acc[i * G::CBW + j]);
        }
      }
    }
  }
}

// The slice's own rows of a halo (rows 1..RS) -> the image tensor (write-through 16-B
// stores): publishes a tensor some time after it was staged, from LDS, without holding
// its registers live in between.
template <int S, int P>
__device__ __forceinline__ void halo_to_global(const bf16* hal, bf16* img_base, int kslice) {
  using G = Stg<S, P>;
  constexpr int UNITS = G::RS * G::R * G::U;
  for (int q = threadIdx.x; q < UNITS; q += PT) {
    const int row = q / (G::R * G::U), rem = q - row * G::R * G::U;
    const int col = rem / G::U, u = rem - col * G::U;
    const int lr = row + 1, lc = col + 1;
    st_sc1_b128(img_base, ((long)(kslice * G::RS + row) * G::R + col) * G::C + u * 8,
                lds16(hal + haddr<G::U>(lr * G::W2 + lc, lc, u * 8)));
  }
}

__device__ __forceinline__ void bn_prefetch_bwd(const PrnBn& bn, int C, BnRegs& r) {
  const int c = threadIdx.x;
  if (c < C) {
    r.g = ldg(bn.gamma + c);
    r.mean = ldg(bn.mean + c);
    r.rstd = ldg(bn.rstd + c);
    r.scale = ldg(bn.scale + c);
    r.shift = ldg(bn.shift + c);
  }
}

// the forward table (scale, shift, mean, rstd) of a BN the forward launch finalized,
// into registers before a wait / from registers into LDS [4][64] as (scale, shift,
// -mean*rstd, rstd): the backward's xhat = x*rstd + (-mean*rstd), one fma
__device__ __forceinline__ void bn_prefetch_tab(const PrnBn& bn, int C, BnRegs& r) {
  const int c = threadIdx.x;
  if (c < C) {
    r.scale = ldg(bn.scale + c);
    r.shift = ldg(bn.shift + c);
    r.mean = ldg(bn.mean + c);
    r.rstd = ldg(bn.rstd + c);
  }
}
__device__ __forceinline__ void tab_store(const BnRegs& r, int C, float* tbl) {
  const int c = threadIdx.x;
  if (c < C) {
    tbl[c] = r.scale;
    tbl[64 + c] = r.shift;
    tbl[128 + c] = -r.mean * r.rstd;
    tbl[192 + c] = r.rstd;
  }
}

// backward BN: sums (sum g, sum g*xhat) -> coefficient table [a, k0, k1, scale, shift] x 64
// with dh = a g - b - c xhat (bn_bwd_apply's formula) refactored as a g + k0 + k1 x:
// k1 = -c rstd, k0 = c mean rstd - b (two fmas per element); workgroup 0 writes
// dgamma / dbeta.  Ends with a barrier.
__device__ __forceinline__ void bn_bwd_table(const PrnBn& bn, const BnRegs& pr, int C, float M,
                                             float* tbl) {
  const int c = threadIdx.x;
  if (c < C) {
    double d1, d2;
    acc_read(bn.bacc, C, c, d1, d2);
    const float sg = (float)d1, sgx = (float)d2;
    const float a = pr.g * pr.rstd;
    const float b = a * sg / M, cc = a * sgx / M;
    tbl[c] = a;
    tbl[64 + c] = cc * pr.mean * pr.rstd - b;
    tbl[128 + c] = -cc * pr.rstd;
    tbl[192 + c] = pr.scale;
    tbl[256 + c] = pr.shift;
    if (blockIdx.x == 0) {   // (write-through: the overlap mode's comm stream reads them
      st_sc1_f32(bn.dbeta + c, sg);   //  while this launch still runs)
      st_sc1_f32(bn.dgamma + c, sgx);
    }
  }
  __syncthreads();
}

// the forward table of a BN the forward launch finalized (backward launch: read back)
__device__ __forceinline__ void bn_load_table(const PrnBn& bn, int C, float* tbl) {
  const int c = threadIdx.x;
  if (c < C) {
    const float rs = ldg(bn.rstd + c);
    tbl[c] = ldg(bn.scale + c);
    tbl[64 + c] = ldg(bn.shift + c);
    tbl[128 + c] = -ldg(bn.mean + c) * rs;   // (tab_store's layout)
    tbl[192 + c] = rs;
  }
}

// one value of the BN-backward output a g + k0 + k1 x, g = da [x*scale+shift > 0]
// (bn_bwd_table's coefficients cf)
__device__ __forceinline__ float bwd1(float da, float xf, const float* cf, int c) {
  const float gg = fmaf(xf, cf[192 + c], cf[256 + c]) > 0.f ? da : 0.f;
  return fmaf(cf[128 + c], xf, fmaf(cf[c], gg, cf[64 + c]));
}
// 8 values (+ add)
__device__ __forceinline__ bf16x8 bwd8(bf16x8 da, bf16x8 x, bf16x8 add, bool has_add,
                                       const float* cf, int c0) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float r = bwd1((float)da[j], (float)x[j], cf, c0 + j);
    if (has_add) r += (float)add[j];
    o[j] = (bf16)r;
  }
  return o;
}

// Backward: slice workgroup 0 republishes every completed barrier as a count on its own
// line (bar + PRN_READY): the ~190 weight-gradient workgroups poll that line instead of
// the arrival shards the slices' atomics go to.
// after a backward arrive workgroup 0 also counts a finished bucket of BatchNorm gradients
// (x.mark), ordered after the arrive's drain of its write-through dgamma / dbeta stores
// (thread 0's wave issued them, and drains in either arrive before thread 0 goes on)
__device__ __forceinline__ void mark_bwd(Ctx& x) {
  if (x.mark != nullptr) {
    if (threadIdx.x == 0) __hip_atomic_fetch_add(x.mark, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x.mark = nullptr;
  }
}
// backward arrive without BN sums in front of it
__device__ __forceinline__ void arrive_bwd(Ctx& x) {
  grid_arrive(x.a->bar + PRN_BWD, x.a->shards);
  mark_bwd(x);
}
__device__ __forceinline__ bool wait_bwd(Ctx& x) {
  ++x.nbar;
  const bool ok = grid_wait(x.a->bar, PRN_BWD, x.nbar, x.slices, x.a->shards, x.a->err, x.m.flag);
  if (ok && blockIdx.x == 0 && threadIdx.x == 0)
    __hip_atomic_store(x.a->bar + PRN_READY, x.nbar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return ok;
}

// sums of g = da [xs*scale+shift > 0] and g * xhat with the forward table tb, then the
// arrive at the backward barrier (bn_sums_arrive); probe tag `tag` (0: none) once the atomics are issued
template <int S, int P>
__device__ __forceinline__ void bwd_sums_arrive(Ctx& x, const bf16x4 (&da)[8], const bf16x4 (&xs)[8],
                                                const float* tb, int bi, int tag, int wave, int lane) {
  lane = opaque_v(lane);
  bn_sums<S, P>([&](int t, int r, float& s1, float& s2) {
    int pb, cb;
    tile_of<S, P>(wave, t, pb, cb);
    const int c = cb * 16 + 4 * (lane >> 4) + r;
    const float xf = (float)xs[t][r];
    const float gg = (xf * tb[c] + tb[64 + c] > 0.f) ? (float)da[t][r] : 0.f;
    s1 = gg;
    s2 = gg * fmaf(xf, tb[192 + c], tb[128 + c]);   // (tb[128] = -mean * rstd)
  }, x.m.red, ld_const(x.a->bns + (bi)).bacc, wave, lane);
  if (tag) probe(x, tag);
  bn_sums_arrive<P>(x.a->bar + PRN_BWD, x.a->shards, wave);
  mark_bwd(x);
}

// dh = a g - b - c xhat (+ add) with the backward coefficient table cf
template <int S, int P, bool ADD>
__device__ __forceinline__ void bwd_apply(bf16x4 (&out)[8], const bf16x4 (&da)[8],
                                          const bf16x4 (&xs)[8], const bf16x4 (&add)[8],
                                          const float* cf, int wave, int lane) {
  lane = opaque_v(lane);
  if (!wave_active<S, P>(wave)) return;
#pragma unroll
  for (int t = 0; t < Stg<S, P>::TPW; ++t) {
    int pb, cb;
    tile_of<S, P>(wave, t, pb, cb);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = cb * 16 + 4 * (lane >> 4) + r;
      float o = bwd1((float)da[t][r], (float)xs[t][r], cf, c);
      if (ADD) o += (float)add[t][r];
      out[t][r] = (bf16)o;
    }
  }
}

// The halo of a BN-backward output (stage S) for the next dgrad: own values from
// registers; the neighbour rows recomputed here from what the neighbours published
// before the barrier -- da (their dgrad output; nullptr: the per-channel constant dpc,
// the pooled head's gradient), the BN input xsrc (saved by the forward) and the residual
// gradient add (nullptr: none) -- with the coefficient table cf.  The loads are issued
// (bwd_nbr_issue) right after the barrier wait, before the BN-backward combine, so the
// two round trips overlap.
struct NbrBwd {
  bf16x8 dv, xv, av;
};
template <int S, int P>
__device__ __forceinline__ void bwd_nbr_issue(const Nbr<S, P>& nb, const bf16* da,
                                              const bf16* xsrc, const bf16* add, NbrBwd& q) {
  if ((int)threadIdx.x < Nbr<S, P>::UNITS && nb.ok) {
    q.dv = da ? ld_sc1_b128(da, nb.gofs) : bf16x8{};
    q.xv = ldg(reinterpret_cast<const bf16x8*>(xsrc + nb.gofs));
    q.av = add ? ld_sc1_b128(add, nb.gofs) : bf16x8{};
  }
}
template <int S, int P>
__device__ __forceinline__ void bwd_halo(Ctx& x, bf16* hal, const bf16x4 (&own)[8],
                                         const Nbr<S, P>& nb, NbrBwd& q, const float* dpc,
                                         bool has_add, const float* cf, int wave, int lane) {
  bf16x8 nv = {};
  if ((int)threadIdx.x < Nbr<S, P>::UNITS && nb.ok) {
    if (dpc) {
#pragma unroll
      for (int j = 0; j < 8; ++j) q.dv[j] = (bf16)dpc[nb.u * 8 + j];
    }
    nv = bwd8(q.dv, q.xv, q.av, has_add, cf, nb.u * 8);
  }
  to_halo<S, P, 0>(hal, own, nullptr, nullptr, nb, nv, x.kslice, wave, lane);
}

// One block's backward: dout (stage S) in registers and its halo in HB, the saved BN2
// input `hs` in registers, conv2's dgrad weights in W1, BN2's forward table in x.ftr;
// out: dx (input stage) in `dout`, its halo in HB, and for the previous block `Bn`
// (has_prev false: none) its conv2 dgrad weights (`next_w2`) in W1, its BN2 input in `hs`, its
// BN2 forward table in x.ftr.  Every global load on the critical path is issued a phase
// ahead (before a barrier wait, or before the halo work).
template <int S, int STR, bool PROJ, int P>
__device__ __forceinline__ bool block_bwd(Ctx& x, bf16x4 (&dout)[8], bf16x4 (&hs)[8],
                                          const WLoad& next_w2, bool has_prev,
                                          const PrnBlock& Bn, const PrnBlock& B) {
  constexpr int SI = STR == 2 ? S - 1 : S;
  using GI = Stg<SI, P>;
  using G = Stg<S, P>;
  const PrnArgs& a = *x.a;
  const int wave = opaque_s(x.wave), lane = opaque_v(x.lane);
  const long img_o = (long)x.img * G::R * G::R * G::C;
  const long img_i = (long)x.img * GI::R * GI::R * GI::C;
  probe(x, 100 + S);
  bf16x4 xs[8];
  load_regs<SI, P>(xs, B.x + img_i, x.kslice, wave, lane);     // BN1 input (used after a barrier)
  tab_store(x.ftr, G::C, x.m.tbl);
  __syncthreads();
  probe(x, 1);
  f32x4 acc[8];
  zero_acc(acc);
  conv_acc<S, P, G::C, 3, 1, true>(acc, x.m.hb, x.m.w1, x.kslice, wave, lane, x.m.red);
  bf16x4 da[8];
  round_acc<S, P, false>(da, acc, da);
  probe(x, 3);
  if constexpr (P > 1)   // only the neighbouring slices read it, only its border rows
    publish<S, P, 1>(da, B.da2 + img_o, x.kslice, wave, lane);
  if constexpr (P > 1) probe(x, 20);
  bwd_sums_arrive<S, P>(x, da, hs, x.m.tbl, B.bn2, 4, wave, lane);
  // dout for the conv2 / projection weight gradients and the neighbours' residual rows:
  // stored after this arrive and the next phase's prefetches (its drain overlaps the
  // wait), drained by the next arrive; from its halo in HB as whole 16-B units (the
  // fragments' 8-B write-through stores left partial lines: bs128 0.749 -> 0.733 ms,
  // bs16 0.557 -> 0.550)
  {
    const WLoad L1 = wl_dgrad(B.w1b, G::C, GI::C, 3);
    WLoad LP{};
    if (PROJ) LP = wl_dgrad(B.wpb, G::C, GI::C, 1);
    bf16x8 w1r[nreg(conv_units(G::C, GI::C, 3))], wpr[1];
    w_prefetch(L1, w1r);
    w_prefetch(LP, wpr);
    bn_prefetch_bwd(ld_const(a.bns + (B.bn2)), G::C, x.bnr);
    bn_prefetch_tab(ld_const(a.bns + (B.bn1)), GI::C, x.ftr);
    halo_to_global<S, P>(x.m.hb, B.dout + img_o, x.kslice);
    probe(x, 5);
    if (!wait_bwd(x)) return false;
    probe(x, 6);
    const Nbr<S, P> nb(x.kslice);
    NbrBwd q;
    bwd_nbr_issue<S, P>(nb, B.da2 + img_o, B.h1 + img_o, nullptr, q);
    bn_bwd_table(ld_const(a.bns + (B.bn2)), x.bnr, G::C, (float)a.N * G::R * G::R, x.m.tbl2);
    bf16x4 dh[8];
    bwd_apply<S, P, false>(dh, da, hs, dh, x.m.tbl2, wave, lane);
    bwd_halo<S, P>(x, x.m.ha, dh, nb, q, nullptr, false, x.m.tbl2, wave, lane);
    tab_store(x.ftr, GI::C, x.m.tbl);
    w_store(L1, w1r, x.m.w1);
    w_store(LP, wpr, x.m.w2);
  }
  __syncthreads();
  probe(x, 8);
  zero_acc(acc);
  if constexpr (STR == 2) {
    dgrad_s2_acc<SI, P, G::C, false>(acc, x.m.ha, x.m.w1, x.kslice, wave, lane);
    dgrad_s2_acc<SI, P, G::C, true>(acc, x.m.hb, x.m.w2, x.kslice, wave, lane);
  } else {
    conv_acc<S, P, G::C, 3, 1, true>(acc, x.m.ha, x.m.w1, x.kslice, wave, lane, x.m.red);
    if constexpr (PROJ) conv_acc<S, P, G::C, 1, 1, false>(acc, x.m.hb, x.m.w2, x.kslice, wave, lane, x.m.red);
  }
  round_acc<SI, P, false>(da, acc, da);
  probe(x, 9);
  if constexpr (P > 1)   // only the neighbouring slices read it, only its border rows
    publish<SI, P, 1>(da, B.da1 + img_i, x.kslice, wave, lane);
  if constexpr (P > 1) probe(x, 21);
  bwd_sums_arrive<SI, P>(x, da, xs, x.m.tbl, B.bn1, 10, wave, lane);
  // dh1 for the conv1 weight gradient, from its halo (HA, intact until the next block
  // stages its own): stored after this arrive, drained by the next one
  halo_to_global<S, P>(x.m.ha, B.dh1 + img_o, x.kslice);
  probe(x, 11);
  bf16x8 w2r[nreg(conv_units(G::C, G::C, 3))];
  w_prefetch(next_w2, w2r);
  bn_prefetch_bwd(ld_const(a.bns + (B.bn1)), GI::C, x.bnr);
  if (has_prev) bn_prefetch_tab(ld_const(a.bns + (Bn.bn2)), GI::C, x.ftr);
  if (!wait_bwd(x)) return false;
  probe(x, 12);
  const Nbr<SI, P> nb(x.kslice);
  NbrBwd q;
  bwd_nbr_issue<SI, P>(nb, B.da1 + img_i, B.x + img_i, PROJ ? nullptr : B.dout + img_o, q);
  bn_bwd_table(ld_const(a.bns + (B.bn1)), x.bnr, GI::C, (float)a.N * GI::R * GI::R, x.m.tbl2);
  probe(x, 13);
  // a stage's first block is the last one the backward reaches: its BN1 gradient completes
  // the stage's BatchNorm gradients (overlap mode: counted on the stage's bucket line)
  if (PROJ && a.overlap && blockIdx.x == 0 && a.bucket_of_stage[S] >= 0)
    x.mark = a.bar + PRN_BUCKET + a.bucket_of_stage[S] * PRN_LINE;
  if constexpr (PROJ) bwd_apply<SI, P, false>(dout, da, xs, dout, x.m.tbl2, wave, lane);
  else bwd_apply<SI, P, true>(dout, da, xs, dout, x.m.tbl2, wave, lane);
  probe(x, 14);
  if (has_prev) load_regs<SI, P>(hs, Bn.h1 + img_i, x.kslice, wave, lane);   // previous block's BN2 input
  // the halo of dx for the previous block's conv2 dgrad (its neighbour rows: this block's
  // published da1, the saved block input, and -- identity blocks -- the published dout)
  bwd_halo<SI, P>(x, x.m.hb, dout, nb, q, nullptr, !PROJ, x.m.tbl2, wave, lane);
  probe(x, 15);
  w_store(next_w2, w2r, x.m.w1);   // visible after the next block's first __syncthreads
  return true;
}

// ---- weight-gradient items ---------------------------------------------------------------
// dW[co][tap][ci] = sum_{images, p} dy[p][co] * A[p @ tap][ci], A = relu(bn(x)) (or x):
// per image, dy [Ro^2][CO] and the A halo [(Ri+2)^2][CI] go to LDS pixel-major; MFMA
// fragments by the transposed read ds_read_b64_tr_b16 (conv_wgrad_direct.hip's scheme);
// waves = WT tile groups x (8 / WT) pixel slices, summed in LDS in a fixed order.
template <int CO, int CI, int KSZ, int STR, int RO, int WT>
__device__ __forceinline__ void wgrad_item(const PrnItem& it, char* smem, int wave, int lane, bool wt) {
  constexpr int RI = RO * STR, W2 = RI + 2, OFF = KSZ == 1 ? 1 : 0;
  constexpr int KN = KSZ * KSZ * CI, NB = (KN + 15) / 16, MB = CO / 16;
  constexpr int TILES = MB * NB, TPW = TILES / WT, WKS = NW / WT;
  constexpr int KSI = RO * RO / 32, KPW = KSI / WKS;   // k-steps per image / per wave
  static_assert(TILES % WT == 0 && KSI % WKS == 0 && TPW <= 36, "wgrad tiles");
  static_assert(NB % TPW == 0, "a wave's tiles share one output-channel block");
  bf16* dys = reinterpret_cast<bf16*>(smem);                    // [RO*RO][CO]
  bf16* hal = dys + RO * RO * CO;                               // [W2*W2][CI]
  float* tb = reinterpret_cast<float*>(hal + W2 * W2 * CI);     // [2][64]
  const int tid = threadIdx.x;
  wave = opaque_s(wave);
  lane = opaque_v(lane);
  const int tg = wave % WT, kq = wave / WT;
  const int gq = lane >> 4, li = lane & 15, qr = li >> 2, pc = li & 3;
  if (it.scale != nullptr && tid < CI) {
    tb[tid] = ldg(it.scale + tid);
    tb[64 + tid] = ldg(it.shift + tid);
  }
  f32x4 acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // operands of image n + 1 are loaded into registers while image n's MFMAs run
  constexpr int DU = RO * RO * CO / 8, CU = CI / 8, XU = W2 * W2 * CU;
  constexpr int ND = (DU + PT - 1) / PT, NX = (XU + PT - 1) / PT;
  bf16x8 rd[ND], rx[NX];
  auto fetch = [&](int n) {
#pragma unroll
    for (int i = 0; i < ND; ++i) {
      const int q = tid + i * PT;
      if (q < DU) rd[i] = ld_sc1_b128(it.dy, (long)n * RO * RO * CO + q * 8);
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int q = tid + i * PT, pix = q / CU, u = q - pix * CU;
      const int hr = pix / W2, hc = pix - hr * W2;
      rx[i] = bf16x8{};
      if (q < XU && hr >= 1 && hr <= RI && hc >= 1 && hc <= RI)
        rx[i] = ldg(reinterpret_cast<const bf16x8*>(it.x + (((long)n * RI + hr - 1) * RI + hc - 1) * CI + u * 8));
    }
  };
  const int nend = it.img0 + it.nimg;
  fetch(it.img0);
  for (int n = it.img0; n < nend; ++n) {
    __syncthreads();   // the previous image's operands are dead; tb written
#pragma unroll
    for (int i = 0; i < ND; ++i) {
      const int q = tid + i * PT;
      if (q < DU) *reinterpret_cast<bf16x8*>(dys + q * 8) = rd[i];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int q = tid + i * PT, pix = q / CU, u = q - pix * CU;
      const int hr = pix / W2, hc = pix - hr * W2;
      if (q < XU) {
        bf16x8 v = rx[i];
        if (it.scale != nullptr && hr >= 1 && hr <= RI && hc >= 1 && hc <= RI)
          v = affine_relu8(v, tb + u * 8, tb + 64 + u * 8);
        *reinterpret_cast<bf16x8*>(hal + pix * CI + u * 8) = v;
      }
    }
    __syncthreads();
    if (n + 1 < nend) fetch(n + 1);
#pragma unroll 1
    for (int kk = 0; kk < KPW; ++kk) {
      const int ks = kq * KPW + kk;
      const int r1 = ks * 32 + 4 * gq + qr, r2 = r1 + 16;     // output pixels of this lane
      int hp[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int p = e ? r2 : r1, oh = p / RO, ow = p - oh * RO;
        hp[e] = (oh * STR + OFF) * W2 + ow * STR + OFF;
      }
      const int mbw = (tg * TPW) / NB;                            // this wave's channel block
      bf16x8 af;
      {
        const s16x4 lo = lds_read_tr16(dys + r1 * CO + mbw * 16 + 4 * pc);
        const s16x4 hi = lds_read_tr16(dys + r2 * CO + mbw * 16 + 4 * pc);
        af = __builtin_bit_cast(bf16x8, (s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
      }
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const int nb = (tg * TPW + t) % NB;
        const int col = nb * 16 + 4 * pc;                         // (tap, ci) of this lane's address
        int tap = col / CI;
        const int ci = col - tap * CI;
        tap = tap < KSZ * KSZ ? tap : KSZ * KSZ - 1;
        const int toff = (tap / KSZ) * W2 + tap % KSZ;
        const s16x4 lo = lds_read_tr16(hal + (hp[0] + toff) * CI + ci);
        const s16x4 hi = lds_read_tr16(hal + (hp[1] + toff) * CI + ci);
        const bf16x8 bfr =
            __builtin_bit_cast(bf16x8, (s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
        acc[t] = mfma16(af, bfr, acc[t]);
      }
    }
  }
  // fixed-order tree sum of the WKS pixel slices (slice kq += slice kq + h, h = WKS/2 .. 1;
  // each level writes a fresh LDS region, so one barrier per level), then the slab
  float* red = reinterpret_cast<float*>(smem);
  static_assert((WKS - 1) * TILES * 64 * 16 <= OFF_MISC, "wgrad reduction LDS");
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int h = WKS / 2; h >= 1; h /= 2) {
    if (kq >= h && kq < 2 * h)
#pragma unroll
      for (int t = 0; t < TPW; ++t)
        *reinterpret_cast<f32x4*>(red + (((base + kq - h) * TILES + tg * TPW + t) * 64 + lane) * 4) = acc[t];
    __syncthreads();
    if (kq < h)
#pragma unroll
      for (int t = 0; t < TPW; ++t)
        acc[t] += *reinterpret_cast<const f32x4*>(red + (((base + kq) * TILES + tg * TPW + t) * 64 + lane) * 4);
    base += h;
  }
  if (kq == 0) {
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int tile = tg * TPW + t, mb = tile / NB, nb = tile - mb * NB;
      const int n = nb * 16 + li;
      if (n < KN) {
        if (wt) {   // overlap mode: read by the comm stream while the launch runs
#pragma unroll
          for (int i = 0; i < 4; ++i) st_sc1_f32(it.part + (long)(mb * 16 + 4 * gq + i) * KN + n, acc[t][i]);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) stg(it.part + (long)(mb * 16 + 4 * gq + i) * KN + n, acc[t][i]);
        }
      }
    }
  }
  __syncthreads();
}

constexpr int PRN_KINDS = 9;
// LDS of the weight-gradient role per kind: dy + halo + table
__host__ __device__ constexpr int wg_lds(int co, int ci, int str, int ro) {
  return ro * ro * co * 2 + (ro * str + 2) * (ro * str + 2) * ci * 2 + 512;
}

__device__ __forceinline__ void run_item(const PrnItem& it, char* smem, int wave, int lane, bool wt) {
  switch (it.kind) {
    case 0: wgrad_item<16, 16, 3, 1, 32, 1>(it, smem, wave, lane, wt); break;   // stage-0 3x3
    case 1: wgrad_item<32, 32, 3, 1, 16, 2>(it, smem, wave, lane, wt); break;   // stage-1 3x3
    case 2: wgrad_item<64, 64, 3, 1, 8, 8>(it, smem, wave, lane, wt); break;    // stage-2 3x3
    case 3: wgrad_item<32, 16, 3, 2, 16, 2>(it, smem, wave, lane, wt); break;   // 3x3/2 16->32
    case 4: wgrad_item<64, 32, 3, 2, 8, 8>(it, smem, wave, lane, wt); break;    // 3x3/2 32->64
    case 5: wgrad_item<16, 16, 1, 1, 32, 1>(it, smem, wave, lane, wt); break;   // 1x1 16->16
    case 6: wgrad_item<32, 16, 1, 2, 16, 2>(it, smem, wave, lane, wt); break;   // 1x1/2 16->32
    case 7: wgrad_item<64, 32, 1, 2, 8, 8>(it, smem, wave, lane, wt); break;    // 1x1/2 32->64
    case 8: wgrad_item<16, 8, 3, 1, 32, 1>(it, smem, wave, lane, wt); break;    // stem 8->16
    default: break;
  }
}


}  // namespace

// The slice role of the backward launch: the dgrad chain with its BatchNorm backwards
// (returns false when a barrier wait timed out).
template <int P>
__device__ __forceinline__ bool prn_bwd_slices(const PrnArgs& a, char* smem, int wave, int lane) {
  const int nsl = a.N * P;
  const int tid = threadIdx.x;
  Ctx x;
  x.a = &a;
  x.m = carve(smem);
  x.img = blockIdx.x / P;
  x.kslice = blockIdx.x % P;
  x.wave = wave;
  x.lane = lane;
  x.nbar = 0;
  x.slices = (unsigned)nsl;
  x.pc = 0;
  x.mark = nullptr;
  probe(x, 0);
  const int nb = a.nblocks;
  const PrnBlock& BL = ld_const(a.blocks + (nb - 1));
  {   // the last block's conv2 dgrad weights (stage 2: 64 x 576)
    const WLoad L = wl_dgrad(BL.w2b, 64, 64, 3);
    bf16x8 r[nreg(conv_units(64, 64, 3))];
    w_prefetch(L, r);
    w_store(L, r, x.m.w1);
  }
  // ---- final BN backward: sums of g = dpool * relu'(bn(XL)), one barrier, then
  //      dXL = a g - b - c xhat and its halo ----
  using G2 = Stg<2, P>;
  bf16x4 dout[8], hs[8];
  {
    const int fb = 2 * nb;
    const long img_o = (long)x.img * 64 * 64;
    bf16x4 xs[8];
    load_regs<2, P>(xs, BL.out + img_o, x.kslice, wave, lane);
    float* dps = x.m.tbl + 256;   // this image's dpool row
    bn_load_table(ld_const(a.bns + (fb)), 64, x.m.tbl);
    if (tid < 64) dps[tid] = a.dpool[(long)x.img * 64 + tid];
    __syncthreads();
    bf16x4 dp[8];
#pragma unroll
    for (int t = 0; t < G2::TPW; ++t) {
      int pb, cb;
      tile_of<2, P>(wave, t, pb, cb);
#pragma unroll
      for (int r = 0; r < 4; ++r) dp[t][r] = (bf16)dps[(cb * 16 + 4 * (lane >> 4) + r) & 63];
    }
    bwd_sums_arrive<2, P>(x, dp, xs, x.m.tbl, fb, 0, wave, lane);
    bn_prefetch_bwd(ld_const(a.bns + (fb)), 64, x.bnr);
    bn_prefetch_tab(ld_const(a.bns + (BL.bn2)), 64, x.ftr);
    if (!wait_bwd(x)) return false;
    const Nbr<2, P> nb(x.kslice);
    NbrBwd q;
    bwd_nbr_issue<2, P>(nb, nullptr, BL.out + img_o, nullptr, q);
    bn_bwd_table(ld_const(a.bns + (fb)), x.bnr, 64, (float)a.N * 64, x.m.tbl2);
    bwd_apply<2, P, false>(dout, dp, xs, dout, x.m.tbl2, wave, lane);
    load_regs<2, P>(hs, BL.h1 + img_o, x.kslice, wave, lane);
    bwd_halo<2, P>(x, x.m.hb, dout, nb, q, dps, false, x.m.tbl2, wave, lane);
  }
  // ---- blocks, last to first (straight-line stages, as in the forward) ----
  const int nps = nb / 3;
  auto run = [&](auto tag, int bi) -> bool {
    constexpr int S = decltype(tag)::S, STR = decltype(tag)::STR;
    constexpr bool PROJ = decltype(tag)::PROJ;
    WLoad n2{};
    const bool hp = bi > 0;
    const PrnBlock Bp = ld_const(a.blocks + (hp ? bi - 1 : bi));
    if (hp) n2 = wl_dgrad(Bp.w2b, 16 << Bp.stage, 16 << Bp.stage, 3);
    return block_bwd<S, STR, PROJ, P>(x, dout, hs, n2, hp, Bp, ld_const(a.blocks + (bi)));
  };
  for (int bi = nb - 1; bi > 2 * nps; --bi)
    if (!run(BlkTag<2, 1, false>{}, bi)) return false;
  if (!run(BlkTag<2, 2, true>{}, 2 * nps)) return false;
  for (int bi = 2 * nps - 1; bi > nps; --bi)
    if (!run(BlkTag<1, 1, false>{}, bi)) return false;
  if (!run(BlkTag<1, 2, true>{}, nps)) return false;
  for (int bi = nps - 1; bi > 0; --bi)
    if (!run(BlkTag<0, 1, false>{}, bi)) return false;
  if (!run(BlkTag<0, 1, true>{}, 0)) return false;
  probe(x, 200);
  // ---- the stem output's gradient: published for the stem's weight gradient ----
  if constexpr (P == 1) {   // from its halo (block_bwd's dout store)
    __syncthreads();
    halo_to_global<0, P>(x.m.hb, a.dx0 + (long)x.img * 1024 * 16, x.kslice);
  } else {
    publish<0, P>(dout, a.dx0 + (long)x.img * 1024 * 16, x.kslice, wave, lane);
  }
  arrive_bwd(x);
  if (blockIdx.x == 0) wait_bwd(x);   // publishes the stem item's readiness
  return true;
}

// The head's batch folds in one workgroup, launched on the main stream right after the
// backward launch: the loss / precision / bias-gradient folds of
// softmax_xent_reduce_kernel (head.hip, same thread mapping and order) and the dense
// weight gradient pooled^T x dlogits (bf16 operands staged in LDS, fp32 sums over the
// images in order).  These were a side-stream softmax_xent_reduce + conv_wgrad pair
// whose fork and join events cost ~11 us per step between the launches.  (Run by the
// backward launch's first weight-gradient workgroup instead, this code perturbed the
// register allocation of the whole backward kernel: 76 -> 272 B of scratch per lane,
// +55 us per step.)
__device__ void prn_head_fold(const PrnArgs& a, char* smem, int tid) {
  const int N = a.N, ld = a.kpad, classes = a.classes;
  // every operand into LDS with one round of 16-byte loads: the fp32 gradient rows and
  // the per-image (loss, correct) pairs and in-top-k flags of the softmax workspace, pooled
  // [N][64] and dlogits [N][ld] (bf16); rows of 64 and ld (% 16) elements are whole 16-B
  // chunks, the pair block goes in 8-byte pieces, the flags one by one
  float* red = reinterpret_cast<float*>(smem);           // [4][64]
  float* sw = red + 256;                                  // [N][ld] + [N][2] + [N]
  bf16* sp = reinterpret_cast<bf16*>(sw + ((N * ld + 3 * N + 3) & ~3));   // 16-B aligned
  bf16* sd = sp + N * 64;
  for (int i = tid; i < N * ld / 4; i += PT)
    reinterpret_cast<f32x4*>(sw)[i] = ldg(reinterpret_cast<const f32x4*>(a.ws) + i);
  for (int i = tid; i < N; i += PT)
    reinterpret_cast<float2*>(sw + N * ld)[i] = ldg(reinterpret_cast<const float2*>(a.ws + N * ld) + i);
  if (a.topk_out != nullptr)
    for (int i = tid; i < N; i += PT) sw[N * ld + 2 * N + i] = ldg(a.ws + N * ld + 2 * N + i);
  for (int i = tid; i < N * 8; i += PT)
    reinterpret_cast<uint4*>(sp)[i] = ldg(reinterpret_cast<const uint4*>(a.pooled) + i);
  for (int i = tid; i < N * ld / 8; i += PT)
    reinterpret_cast<uint4*>(sd)[i] = ldg(reinterpret_cast<const uint4*>(a.dlogits) + i);
  __syncthreads();
  const int lane = tid & 63, q = tid >> 6;
  if (q < 4) {   // bias gradient: thread (class, row slice q) sums rows q, q + 4, ...
    float t = 0.f;
    if (lane < classes) {
#pragma unroll 8
      for (int r = q; r < N; r += 4) t += sw[r * ld + lane];
    }
    red[q * 64 + lane] = t;
  } else if (q == 4) {   // loss and precision
    const float* rs = sw + N * ld;
    float l = 0.f, k = 0.f;
    for (int r = lane; r < N; r += 64) {
      l += rs[2 * r];
      k += rs[2 * r + 1];
    }
    l = wave_sum(l);
    k = wave_sum(k);
    if (lane == 0) {
      stg(a.loss_sum, l);
      stg(a.correct, k);
    }
    if (a.topk_out != nullptr) {   // uniform
      const float* rk = rs + 2 * N;
      float k5 = 0.f;
      for (int r = lane; r < N; r += 64) k5 += rk[r];
      k5 = wave_sum(k5);
      if (lane == 0) stg(a.topk_out, k5);
    }
  }
  // dense weight gradient: thread (f = tid % 64, image chunk tid / 64 of 8) holds 16
  // classes' sums in registers over its images (the dlogits row is a broadcast LDS read),
  // the 8 chunk partials are added in chunk order through LDS.  (One thread per output
  // over all images ran 10-14 us: ~2.5k LDS instructions queued on this one CU.)
  static_assert(PT == 512, "8 image chunks of 64 threads");
  float* part = reinterpret_cast<float*>(sd + ((N * ld + 7) & ~7));   // [8][64][16]
  {
    const int f = tid & 63, c = tid >> 6;
    const int n0 = (N * c) >> 3, n1 = (N * (c + 1)) >> 3;
    for (int k0 = 0; k0 < classes; k0 += 16) {   // ld % 16 == 0: k0 + 15 < ld
      float acc[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[j] = 0.f;
      for (int n = n0; n < n1; ++n) {
        const float x = (float)sp[n * 64 + f];
        const bf16* drow = sd + n * ld + k0;
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] += x * (float)drow[j];
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) part[(c * 64 + f) * 16 + j] = acc[j];
      __syncthreads();
      for (int o = tid; o < 64 * 16; o += PT) {
        const int ff = o >> 4, j = o & 15;
        if (k0 + j < classes) {
          float t = part[ff * 16 + j];
#pragma unroll
          for (int cc = 1; cc < 8; ++cc) t += part[(cc * 64 + ff) * 16 + j];
          stg(a.dense_grad + ff * classes + k0 + j, t);   // HWIO [64][classes]
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  if (q == 0 && lane < classes)
    stg(a.dbias + lane, red[lane] + red[64 + lane] + red[128 + lane] + red[192 + lane]);
}

template <int P>
__global__ void __launch_bounds__(PT, 1) prn_bwd_kernel(PrnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  if ((int)blockIdx.x < a.N * P && !prn_bwd_slices<P>(a, smem, wave, lane)) return;
  // ---- weight-gradient items from one queue in readiness order: the workgroups beyond
  //      the slices from the start, every slice once its dgrad chain is done (the last
  //      items -- the first stage and the stem -- only become ready at the very end) ----
  int* flag = reinterpret_cast<int*>(smem + OFF_MISC);
  int* slot = flag + 1;
  for (;;) {
    __syncthreads();   // the previous item's LDS and the slot word are free
    if (tid == 0)
      *slot = (int)__hip_atomic_fetch_add(a.bar + PRN_QUEUE, 1u, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int i = __builtin_amdgcn_readfirstlane(*slot);
    if (i >= a.nitems) {
      if (a.probe != nullptr && tid == 0)   // diagnostics: when the last workgroup ran out of items
        __hip_atomic_fetch_max(a.probe + 8191, (long long)wall_clock64(), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    const PrnItem& it = ld_const(a.items + i);
    if (!count_wait<8>(a.bar, PRN_READY, (unsigned)it.ready, a.err, flag)) return;
    run_item(it, smem, wave, lane, a.overlap != 0);
    if (a.overlap && it.bucket >= 0) {   // the slab's write-through stores drained, then counted
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0)
        __hip_atomic_fetch_add(a.bar + PRN_BUCKET + it.bucket * PRN_LINE, 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// comm-stream bucket wait (overlap mode): lane 0 polls the bucket line (bounded)
__global__ void __launch_bounds__(64) prn_bucket_wait_kernel(unsigned* bar, int bucket, unsigned target,
                                                            int* err) {
  if (threadIdx.x != 0) return;
  const unsigned* ctr = bar + PRN_BUCKET + bucket * PRN_LINE;
  const long long t0 = wall_clock64();
  while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
    __builtin_amdgcn_s_sleep(4);
    if (wall_clock64() - t0 > kSpinTicks) {
      __hip_atomic_store(err, 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
  }
}

__global__ void __launch_bounds__(PT, 1) prn_head_kernel(PrnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  prn_head_fold(a, smem, threadIdx.x);
}

// ---- host ------------------------------------------------------------------------------
int prn_item_kind(int cin, int cout, int ksize, int stride) {
  if (cin == 8 && cout == 16 && ksize == 3 && stride == 1) return 8;
  if (ksize == 3 && stride == 1 && cin == cout) return cin == 16 ? 0 : cin == 32 ? 1 : cin == 64 ? 2 : -1;
  if (ksize == 3 && stride == 2) return cin == 16 && cout == 32 ? 3 : cin == 32 && cout == 64 ? 4 : -1;
  if (ksize == 1 && stride == 1 && cin == 16 && cout == 16) return 5;
  if (ksize == 1 && stride == 2) return cin == 16 && cout == 32 ? 6 : cin == 32 && cout == 64 ? 7 : -1;
  return -1;
}

static_assert(wg_lds(16, 16, 1, 32) <= LDS_TOTAL && wg_lds(32, 16, 2, 16) <= LDS_TOTAL &&
                  wg_lds(16, 8, 1, 32) <= LDS_TOTAL,
              "weight-gradient LDS");

static size_t prn_head_lds(int N, int kpad) {
  return 1024 + 32 + (size_t)N * ((64 + kpad) * sizeof(bf16) + (kpad + 3) * sizeof(float)) +
         8 * 64 * 16 * sizeof(float);
}

long prn_bwd_resident(int P) {
  return P == 1 ? resident_blocks(prn_bwd_kernel<1>, LDS_TOTAL)
         : P == 2 ? resident_blocks(prn_bwd_kernel<2>, LDS_TOTAL)
                  : resident_blocks(prn_bwd_kernel<4>, LDS_TOTAL);
}

std::string prn_check(int N, int P, int P_fwd, int nblocks, int classes, int kpad) {
  if (!prn_supported(N, P, nblocks, classes, kpad) || !prn_supported(N, P_fwd, nblocks, classes, kpad))
    return "unsupported shape (slices 1/2/4, N x slices <= 256, 3n blocks, classes <= kpad <= 64)";
  const int cus = cu_count();
  if (N * P_fwd > cus) return "forward grid (N x slices) exceeds the CUs";
  if (N * P + 1 > cus) return "backward grid (N x slices + weight-gradient workgroups) exceeds the CUs";
  if (N > 240 || prn_head_lds(N, kpad) > LDS_TOTAL) return "head folds: batch too large for LDS";
  // co-residency: every workgroup of a grid must be resident at once (grid barriers)
  const long rf = prn_fwd_resident(P_fwd), rb = prn_bwd_resident(P);
  if (rf < 0 || rb < 0) return "occupancy query failed";
  if (rf < (long)N * P_fwd) return "forward grid not co-resident (occupancy API)";
  if (rb < (long)N * P + 1) return "backward grid not co-resident (occupancy API)";
  return "";
}

void prn_head(const PrnArgs& a, hipStream_t s) {
  if (!prn_supported(a.N, a.P, a.nblocks, a.classes, a.kpad) || a.N > 240 || !a.dense_grad ||
      !a.loss_sum || !a.correct || !a.dbias)
    throw std::invalid_argument("prn_head: unsupported shape or missing outputs");
  const size_t lds = prn_head_lds(a.N, a.kpad);
  if (lds > LDS_TOTAL) throw std::invalid_argument("prn_head: batch too large for LDS");
  hipLaunchKernelGGL(prn_head_kernel, dim3(1), dim3(PT), lds, s, a);
  DTR_CHECK_LAUNCH();
}

void prn_bucket_wait(unsigned* bar, int bucket, unsigned target, int* err, hipStream_t s) {
  if (bucket < 0 || bucket >= PRN_NBUCKET || bar == nullptr || err == nullptr)
    throw std::invalid_argument("prn_bucket_wait: bucket 0..2, bar and err required");
  hipLaunchKernelGGL(prn_bucket_wait_kernel, dim3(1), dim3(64), 0, s, bar, bucket, target, err);
  DTR_CHECK_LAUNCH();
}

void prn_backward(const PrnArgs& a, int wgrad_wgs, hipStream_t s) {
  if (!prn_supported(a.N, a.P, a.nblocks, a.classes, a.kpad))
    throw std::invalid_argument("prn_backward: unsupported shape");
  const int grid = a.N * a.P + std::max(1, wgrad_wgs);
  if (grid > cu_count())
    throw std::invalid_argument("prn_backward: the grid must be co-resident (<= one per CU)");
  PrnArgs b = a;
  b.probe = g_prn_probe;
  b.shards = prn_shards(a.N, a.P);
  if (a.P == 1) hipLaunchKernelGGL(prn_bwd_kernel<1>, dim3(grid), dim3(PT), LDS_TOTAL, s, b);
  else if (a.P == 2) hipLaunchKernelGGL(prn_bwd_kernel<2>, dim3(grid), dim3(PT), LDS_TOTAL, s, b);
  else hipLaunchKernelGGL(prn_bwd_kernel<4>, dim3(grid), dim3(PT), LDS_TOTAL, s, b);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
