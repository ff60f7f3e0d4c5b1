// Persistent small-batch CIFAR step, the training forward: the whole forward with the
// head (dense, softmax cross-entropy, dense dgrad, pool gradient) in one launch.  The
// design, the hand-off protocol and the device primitives are in prn_device.h.
#include "prn_device.h"
#include "xent_row.h"

namespace dtr {

namespace {

// =====================================================================================
// forward
// =====================================================================================
__device__ __forceinline__ bool wait_fwd(Ctx& x) {
  ++x.nbar;
  if (x.a->fault_bar == (int)x.nbar && blockIdx.x == 0) {   // tests: a lost workgroup
    if (threadIdx.x == 0) __hip_atomic_store(x.a->err, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return false;
  }
  return grid_wait(x.a->bar, PRN_FWD, x.nbar, x.slices, x.a->shards, x.a->err, x.m.flag);
}

// the slice's sums of v and v^2 into BatchNorm bi's accumulators, then the arrive at the
// forward barrier (bn_sums_arrive); probe tag `tag` (0: none) once the atomics are issued
template <int S, int P>
__device__ __forceinline__ void fwd_sums_arrive(Ctx& x, const bf16x4 (&v)[8], int bi, int tag,
                                                int wave, int lane) {
  bn_sums<S, P>([&](int t, int r, float& s1, float& s2) {
    const float f = (float)v[t][r];
    s1 = f;
    s2 = f * f;
  }, x.m.red, ld_const(x.a->bns + (bi)).acc, wave, lane);
  if (tag) probe(x, tag);
  bn_sums_arrive<P>(x.a->bar + PRN_FWD, x.a->shards, wave);
}

// BN + ReLU of the published raw tensor `src` (stage S, this image) into halo `hal`: own
// values from registers, neighbour rows from src (sc1 loads issued first), table from
// the BN's accumulators (bnr prefetched).  Ends with a barrier.
template <int S, int P>
__device__ __forceinline__ void fwd_bn_halo(Ctx& x, bf16* hal, const bf16x4 (&v)[8],
                                            const bf16* src, int bi, int wave, int lane) {
  using G = Stg<S, P>;
  const PrnArgs& a = *x.a;
  const Nbr<S, P> nb(x.kslice);
  bf16x8 nv = {};
  if ((int)threadIdx.x < Nbr<S, P>::UNITS && nb.ok) nv = ld_sc1_b128(src, nb.gofs);
  bn_fwd_table(ld_const(a.bns + (bi)), x.bnr, G::C, (double)a.N * G::R * G::R, a.eps, a.momentum,
               a.update_moving, x.m.tbl);
  if ((int)threadIdx.x < Nbr<S, P>::UNITS && nb.ok)
    nv = affine_relu8(nv, x.m.tbl + nb.u * 8, x.m.tbl + 64 + nb.u * 8);
  to_halo<S, P, 1>(hal, v, x.m.tbl, x.m.tbl + 64, nb, nv, x.kslice, wave, lane);
}

// One building block, output stage S; STR 2: transition (input stage S-1, projection);
// PROJ with STR 1: stage-0 block 0 (1x1 stride-1 projection).  On entry W1 (W2) hold
// conv1's (the projection's) weights and x.bnr the block's BN1 parameters; on exit the
// next block's.
template <int S, int STR, bool PROJ, int P>
__device__ __forceinline__ bool block_fwd(Ctx& x, bf16x4 (&xr)[8], int bi_next,
                                          const WLoad& next_w1, const WLoad& next_wp,
                                          const PrnBlock& B) {
  constexpr int SI = STR == 2 ? S - 1 : S;
  using GI = Stg<SI, P>;
  using G = Stg<S, P>;
  const PrnArgs& a = *x.a;
  const int wave = opaque_s(x.wave), lane = opaque_v(x.lane);
  const long img_o = (long)x.img * G::R * G::R * G::C;
  const long img_i = (long)x.img * GI::R * GI::R * GI::C;
  probe(x, 100 + S);
  // BN1 + ReLU of the block input -> halo A (input stage)
  fwd_bn_halo<SI, P>(x, x.m.ha, xr, B.x + img_i, B.bn1, wave, lane);
  probe(x, 1);
  __syncthreads();
  probe(x, 2);
  bf16x4 pr[8], hr[8];
  f32x4 acc[8];
  if constexpr (PROJ) {
    zero_acc(acc);
    conv_acc<S, P, GI::C, 1, STR, false>(acc, x.m.ha, x.m.w2, x.kslice, wave, lane, x.m.red);
    round_acc<S, P, false>(pr, acc, pr);
  }
  zero_acc(acc);
  conv_acc<S, P, GI::C, 3, STR, false>(acc, x.m.ha, x.m.w1, x.kslice, wave, lane, x.m.red);
  round_acc<S, P, false>(hr, acc, hr);
  probe(x, 3);
  // Inside this launch only the neighbouring slices read the saved tensor, and only its
  // border rows: those are published before the arrive; the rest (read by the backward
  // launch) is stored after it, its drain overlapping the barrier wait.
  if constexpr (P > 1) publish<S, P, 1>(hr, B.h1 + img_o, x.kslice, wave, lane);
  if constexpr (P > 1) probe(x, 20);
  fwd_sums_arrive<S, P>(x, hr, B.bn2, 4, wave, lane);
  publish<S, P, P == 1 ? 0 : 2, true>(hr, B.h1 + img_o, x.kslice, wave, lane);
  probe(x, 5);
  {
    bf16x8 w2r[nreg(conv_units(G::C, G::C, 3))];
    const WLoad L2 = wl_fwd(B.w2f, G::C, G::C, 3);
    w_prefetch(L2, w2r);
    bn_prefetch_fwd(ld_const(a.bns + (B.bn2)), G::C, x.bnr);
    if (!wait_fwd(x)) return false;
    probe(x, 6);
    // BN2 + ReLU -> halo A, conv2 (+ residual)
    fwd_bn_halo<S, P>(x, x.m.ha, hr, B.h1 + img_o, B.bn2, wave, lane);
    w_store(L2, w2r, x.m.w1);
  }
  __syncthreads();
  probe(x, 8);
  zero_acc(acc);
  conv_acc<S, P, G::C, 3, 1, false>(acc, x.m.ha, x.m.w1, x.kslice, wave, lane, x.m.red);
  if constexpr (PROJ) round_acc<S, P, true>(xr, acc, pr);
  else round_acc<S, P, true>(xr, acc, xr);
  probe(x, 9);
  if constexpr (P > 1) publish<S, P, 1>(xr, B.out + img_o, x.kslice, wave, lane);
  if constexpr (P > 1) probe(x, 21);
  fwd_sums_arrive<S, P>(x, xr, bi_next, 10, wave, lane);
  publish<S, P, P == 1 ? 0 : 2, true>(xr, B.out + img_o, x.kslice, wave, lane);
  probe(x, 11);
  bf16x8 w1r[nreg_next_fwd<S>()], wpr[1];
  w_prefetch(next_w1, w1r);
  w_prefetch(next_wp, wpr);
  bn_prefetch_fwd(ld_const(a.bns + (bi_next)), G::C, x.bnr);   // the next BN normalizes this output
  if (!wait_fwd(x)) return false;
  probe(x, 12);
  w_store(next_w1, w1r, x.m.w1);   // visible after the next block's first __syncthreads
  w_store(next_wp, wpr, x.m.w2);
  return true;
}

template <int P>
__device__ __forceinline__ void prn_forward_body(const PrnArgs& a, char* smem) {
  Ctx x;
  x.a = &a;
  x.m = carve(smem);
  x.img = blockIdx.x / P;
  x.kslice = blockIdx.x % P;
  x.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  x.lane = threadIdx.x & 63;
  x.nbar = 0;
  x.slices = (unsigned)(a.N * P);
  x.pc = 0;
  x.mark = nullptr;
  const int tid = threadIdx.x;
  probe(x, 0);

  // ---- stem: 3x3 8 -> 16 on the 32x32 image (no BN before it): the slice's rows plus
  //      one halo row above and below straight from the input ----
  stem_fill<P, false>(a, x.img, x.m.ha, x.m.w1, x.kslice);
  __syncthreads();
  const PrnBlock& B0 = ld_const(a.blocks + (0));
  bf16x4 xr[8];
  {
    f32x4 acc[8];
    zero_acc(acc);
    conv_acc<0, P, 8, 3, 1, false>(acc, x.m.ha, x.m.w1, x.kslice, x.wave, x.lane, x.m.red);
    round_acc<0, P, false>(xr, acc, xr);
    if constexpr (P > 1) publish<0, P, 1>(xr, B0.x + (long)x.img * 1024 * 16, x.kslice, x.wave, x.lane);
    fwd_sums_arrive<0, P>(x, xr, B0.bn1, 0, x.wave, x.lane);
    publish<0, P, P == 1 ? 0 : 2, true>(xr, B0.x + (long)x.img * 1024 * 16, x.kslice, x.wave, x.lane);
    const WLoad L1 = wl_fwd(B0.w1f, 16, 16, 3);
    WLoad LP{};
    if (B0.wpf) LP = wl_fwd(B0.wpf, 16, 16, 1);
    bf16x8 w1r[nreg(conv_units(16, 16, 3))], wpr[1];
    w_prefetch(L1, w1r);
    w_prefetch(LP, wpr);
    bn_prefetch_fwd(ld_const(a.bns + (B0.bn1)), 16, x.bnr);
    if (!wait_fwd(x)) return;
    w_store(L1, w1r, x.m.w1);
    w_store(LP, wpr, x.m.w2);
  }

  // ---- blocks: per stage a transition block then identity blocks (straight-line
  //      stages, no per-block switch: one register allocation region per variant).
  //      (Every failed wait returns from here directly: routed through a helper that
  //      reports it as a bool, the same dispatch allocated 40-50 more VGPRs.  The
  //      next-block lookup is written here and in prn_infer_body, not in a shared
  //      helper: through one, by struct or by out-parameters, the block loop's register
  //      assignment changed and the batch-128 forward measured 1-3 us slower.) ----
  const int nps = a.nblocks / 3;   // blocks per stage
  auto run = [&](auto tag, int bi) -> bool {
    constexpr int S = decltype(tag)::S, STR = decltype(tag)::STR;
    constexpr bool PROJ = decltype(tag)::PROJ;
    const PrnBlock& B = ld_const(a.blocks + (bi));
    const bool last = bi + 1 == a.nblocks;
    const int bnx = last ? 2 * a.nblocks : ld_const(a.blocks + (bi + 1)).bn1;
    WLoad n1{}, np{};
    if (!last) {
      const PrnBlock& Bn = ld_const(a.blocks + (bi + 1));
      const int so = Bn.stage, si = Bn.stride == 2 ? so - 1 : so;
      n1 = wl_fwd(Bn.w1f, 16 << so, 16 << si, 3);
      if (Bn.wpf) np = wl_fwd(Bn.wpf, 16 << so, 16 << si, 1);
    }
    return block_fwd<S, STR, PROJ, P>(x, xr, bnx, n1, np, B);
  };
  if (!run(BlkTag<0, 1, true>{}, 0)) return;
  for (int bi = 1; bi < nps; ++bi)
    if (!run(BlkTag<0, 1, false>{}, bi)) return;
  if (!run(BlkTag<1, 2, true>{}, nps)) return;
  for (int bi = nps + 1; bi < 2 * nps; ++bi)
    if (!run(BlkTag<1, 1, false>{}, bi)) return;
  if (!run(BlkTag<2, 2, true>{}, 2 * nps)) return;
  for (int bi = 2 * nps + 1; bi < 3 * nps; ++bi)
    if (!run(BlkTag<2, 1, false>{}, bi)) return;

  // ---- head (head.hip head_fused numerics): final BN + ReLU, the slice's average-pool
  //      sums (fp64 atomics per image), one barrier; then slice 0 of each image: dense,
  //      softmax cross-entropy row, dense dgrad, pool gradient ----
  probe(x, 200);
  const int fb = 2 * a.nblocks;
  const int dunits = 64 * a.kpad / 8;
  bf16x8 dwv = {};
  if (x.kslice == 0 && tid < dunits) dwv = *reinterpret_cast<const bf16x8*>(a.dense_w + tid * 8);
  bn_fwd_table(ld_const(a.bns + (fb)), x.bnr, 64, (double)a.N * 64, a.eps, a.momentum, a.update_moving, x.m.tbl);
  {
    const float v = pool_sums<P>(xr, x.m.tbl, x.m.red, x.wave, x.lane);
    if (tid < 64) atomic_add_g(a.pool_acc + (long)x.img * 64 + tid, (double)v);
  }
  grid_arrive(a.bar + PRN_FWD, a.shards);
  if (!wait_fwd(x)) return;
  if (x.kslice != 0) return;
  float* pool_s = x.m.tbl2;          // [0, 64) pooled, [64, 128) dp, [128, 192) g
  float* wd = reinterpret_cast<float*>(x.m.w1);   // dense weights as fp32 [64][kpad]
  if (tid < dunits)
#pragma unroll
    for (int j = 0; j < 8; ++j) wd[tid * 8 + j] = (float)dwv[j];
  if (tid < 64) {
    const bf16 pb = (bf16)((float)ld_sc1_d(a.pool_acc + (long)x.img * 64 + tid) / 64.f);
    a.pooled[(long)x.img * 64 + tid] = pb;
    pool_s[tid] = (float)pb;
  }
  __syncthreads();
  if (x.wave == 0) {
    const int lane = x.lane;
    const int y = a.labels[x.img];
    float z = -INFINITY;
    if (lane < a.classes) {
      float acc = 0.f;
#pragma unroll 8
      for (int c = 0; c < 64; ++c) acc += pool_s[c] * wd[c * a.kpad + lane];
      z = acc + a.dense_b[lane];
    }
    const float zy = __shfl(z, (y >= 0 && y < a.classes) ? y : 0, 64);
    const int yb = a.labels_b ? a.labels_b[x.img] : -1;   // mixup: partner label, the row's lam
    const float lam = a.mix_lam ? a.mix_lam[x.img] : 1.f;
    const float zyb = __shfl(z, (yb >= 0 && yb < a.classes) ? yb : 0, 64);
    const XentRow r = xent_row<1>([&](int) { return z; }, lane, a.classes, y, zy,
                                  a.label_smoothing, a.topk, yb, zyb, lam);
    float g = 0.f;
    if (lane < a.classes) g = r.grad(r.prob(z), lane == y, lane == yb, a.grad_scale);
    if (lane < a.kpad) {
      const bf16 gb = (bf16)g;
      a.dlogits[(long)x.img * a.kpad + lane] = gb;
      a.ws[(long)x.img * a.kpad + lane] = g;
      pool_s[128 + lane] = (float)gb;
    }
    if (lane == 0) {
      float* rs = a.ws + (long)a.N * a.kpad + 2 * x.img;
      rs[0] = r.loss;
      rs[1] = r.top1;
      if (a.topk > 0) a.ws[(long)a.N * a.kpad + 2L * a.N + x.img] = r.topk;
    }
  }
  __syncthreads();
  if (tid < 64) {
    float d = 0.f;
    for (int k = 0; k < a.kpad; ++k) d += pool_s[128 + k] * wd[tid * a.kpad + k];
    const float db = (float)(bf16)d;
    a.dpool[(long)x.img * 64 + tid] = (float)(bf16)(db * (1.f / 64.f));
  }
}

}  // namespace

template <int P>
__global__ void __launch_bounds__(PT, 1) prn_fwd_kernel(PrnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  prn_forward_body<P>(a, smem);
}

// ---- host ------------------------------------------------------------------------------
long long* g_prn_probe = nullptr;
void prn_set_probe(long long* p) { g_prn_probe = p; }

int device_cus() { return cu_count(); }
std::vector<uint32_t> device_cu_mask() { return cu_mask_words(); }

size_t prn_lds_bytes() { return LDS_TOTAL; }
int prn_bar_words() { return PRN_BAR_WORDS; }
int prn_acc_rep() { return PRN_ACC_REP; }

bool prn_supported(int N, int P, int nblocks, int classes, int kpad) {
  return N >= 1 && (P == 1 || P == 2 || P == 4) && N * P <= 256 && nblocks >= 3 && nblocks % 3 == 0 &&
         classes >= 1 && classes <= kpad && kpad <= 64 && kpad % 16 == 0;
}

// Arrival shards of a launch whose barriers N x P slices arrive at.  Auto (tune -1): 64
// (about two arrivals per line) when 128 or more slices of at most half an image each
// arrive together, else 8 -- more lines cost every poll (one load per line) and pay only
// where the arrivals cluster.  Same-process A/B, step ms, 8 / 32 / 64 shards (scripts/
// tune_ab.py): bs16 0.5573 / 0.5592 / 0.5598, bs32 0.5764 / 0.5710 / 0.5676, bs64 0.6439
// / 0.6434 / 0.6409, bs128 (one slice per image) 0.7332 / 0.7323 / 0.7351.
int prn_shards(int N, int P) {
  const long t = tune(T_PRN_SHARDS);
  if (t == 1 || t == 8 || t == 16 || t == 32 || t == 64) return (int)t;
  return N * P >= 128 && P >= 2 ? 64 : 8;
}

long prn_fwd_resident(int P) {
  return P == 1 ? resident_blocks(prn_fwd_kernel<1>, LDS_TOTAL)
         : P == 2 ? resident_blocks(prn_fwd_kernel<2>, LDS_TOTAL)
                  : resident_blocks(prn_fwd_kernel<4>, LDS_TOTAL);
}

void prn_forward(const PrnArgs& a, hipStream_t s) {
  if (!prn_supported(a.N, a.P, a.nblocks, a.classes, a.kpad) || a.N * a.P > cu_count())
    throw std::invalid_argument("prn_forward: unsupported shape (N x P <= CUs, 3n blocks, <= 64 classes)");
  PrnArgs b = a;
  b.probe = g_prn_probe;
  b.shards = prn_shards(a.N, a.P);
  if (a.P == 1) hipLaunchKernelGGL(prn_fwd_kernel<1>, dim3(a.N), dim3(PT), LDS_TOTAL, s, b);
  else if (a.P == 2) hipLaunchKernelGGL(prn_fwd_kernel<2>, dim3(a.N * 2), dim3(PT), LDS_TOTAL, s, b);
  else hipLaunchKernelGGL(prn_fwd_kernel<4>, dim3(a.N * 4), dim3(PT), LDS_TOTAL, s, b);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
