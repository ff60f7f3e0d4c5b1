// Persistent CIFAR inference forward (moving-average BatchNorm): the whole network in
// one launch.  The device primitives, and the pieces shared with the training forward
// (stem fill, next-block lookup, pool partials), are in prn_device.h.
//
// One workgroup per image (the P = 1 geometry), the whole network in one pass: without
// batch statistics nothing crosses images, so there is no grid barrier, no atomic and no
// tensor published between workgroups -- only the logits (and optionally the pooled
// features) are stored.  A block is: BN1 + ReLU of the register-held input -> halo A,
// projection + conv1, BN2 + ReLU -> halo A, conv2 + residual (fp32, then one bf16
// rounding).  Four workgroup barriers per block order the halo / weight / table reuse:
//   (B) halo A, W1 / W2 and the table are written    -> the convs read them
//   (C) conv1 is done with halo A and W1              -> BN2's halo fill, conv2's weights
//   (E) halo A and W1 are written                     -> conv2 reads them
//   (F) conv2 is done with halo A and W1              -> the next block's fill and weights
// The next weights (conv2's during conv1, the next block's during conv2) and the next
// BatchNorm's four parameter vectors are loaded into registers before each conv and
// stored to LDS after the barrier behind it, so their memory round trip runs under the
// MFMA work.  The two tables alternate (BN1: tbl, BN2: tbl2): wave 0 writes the next one
// right after its conv, before the barrier that also frees the halo.
#include "prn_device.h"

namespace dtr {

namespace {

__device__ __forceinline__ void bn_prefetch_infer(const PrnBn& bn, int C, BnRegs& r) {
  const int c = threadIdx.x;
  if (c < C) {
    r.g = ldg(bn.gamma + c);
    r.b = ldg(bn.beta + c);
    r.mm = ldg(bn.mmean + c);
    r.mv = ldg(bn.mvar + c);
  }
}
// (scale, shift) table [2][64] from the moving statistics: bn_eval_kernel's expressions
__device__ __forceinline__ void bn_infer_table(const BnRegs& r, int C, float eps, float* tbl) {
  const int c = threadIdx.x;
  if (c < C) {
    const float sc = r.g * rsqrtf(r.mv + eps);
    tbl[c] = sc;
    tbl[64 + c] = r.b - r.mm * sc;
  }
}

constexpr int DENSE_KP = 64 + 8;   // dense weight row in LDS (padded: rows spread over banks)
static_assert(128 * DENSE_KP * 2 <= HALO_B, "dense weights fit halo B's region");

// One building block (block_fwd's variants).  On entry tbl holds BN1's table and W1 (W2)
// conv1's (the projection's) weights, both stored since barrier (F) of the step before;
// on exit the next block's (the final BN's table after the last block).
template <int S, int STR, bool PROJ>
__device__ __forceinline__ void block_infer(const PrnInferArgs& a, const Smem& m, bf16x4 (&xr)[8],
                                            BnRegs& bnr, int bi_next, const WLoad& next_w1,
                                            const WLoad& next_wp, const PrnBlock& B, int wave_,
                                            int lane_) {
  constexpr int SI = STR == 2 ? S - 1 : S;
  using GI = Stg<SI, 1>;
  using G = Stg<S, 1>;
  const int wave = opaque_s(wave_), lane = opaque_v(lane_);
  bf16x4 pr[8], hr[8];
  f32x4 acc[8];
  {
    const Nbr<SI, 1> nb(0);   // (one slice: rows -1 and R are the conv's zero padding)
    to_halo<SI, 1, 1>(m.ha, xr, m.tbl, m.tbl + 64, nb, bf16x8{}, 0, wave, lane);
    bf16x8 w2r[nreg(conv_units(G::C, G::C, 3))];
    const WLoad L2 = wl_fwd(B.w2f, G::C, G::C, 3);
    w_prefetch(L2, w2r);
    bn_prefetch_infer(ld_const(a.bns + (B.bn2)), G::C, bnr);
    __syncthreads();   // (B)
    if constexpr (PROJ) {
      zero_acc(acc);
      conv_acc<S, 1, GI::C, 1, STR, false>(acc, m.ha, m.w2, 0, wave, lane, m.red);
      round_acc<S, 1, false>(pr, acc, pr);
    }
    zero_acc(acc);
    conv_acc<S, 1, GI::C, 3, STR, false>(acc, m.ha, m.w1, 0, wave, lane, m.red);
    round_acc<S, 1, false>(hr, acc, hr);
    bn_infer_table(bnr, G::C, a.eps, m.tbl2);
    __syncthreads();   // (C)
    w_store(L2, w2r, m.w1);
  }
  const Nbr<S, 1> nb(0);
  to_halo<S, 1, 1>(m.ha, hr, m.tbl2, m.tbl2 + 64, nb, bf16x8{}, 0, wave, lane);
  bf16x8 w1r[nreg_next_fwd<S>()], wpr[1];
  w_prefetch(next_w1, w1r);
  w_prefetch(next_wp, wpr);
  bn_prefetch_infer(ld_const(a.bns + (bi_next)), G::C, bnr);   // the next BN normalizes this output
  __syncthreads();   // (E)
  zero_acc(acc);
  conv_acc<S, 1, G::C, 3, 1, false>(acc, m.ha, m.w1, 0, wave, lane, m.red);
  if constexpr (PROJ) round_acc<S, 1, true>(xr, acc, pr);
  else round_acc<S, 1, true>(xr, acc, xr);
  bn_infer_table(bnr, G::C, a.eps, m.tbl);
  __syncthreads();   // (F)
  w_store(next_w1, w1r, m.w1);
  w_store(next_wp, wpr, m.w2);
}

__device__ __forceinline__ void prn_infer_body(const PrnInferArgs& a, char* smem) {
  const Smem m = carve(smem);
  const int img = blockIdx.x, tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  bf16* dw = m.hb;   // dense weights [kpad][DENSE_KP] (halo B's region: unused here)
  BnRegs bnr;
  const PrnBlock& B0 = ld_const(a.blocks + (0));

  // ---- stem: 3x3 8 -> 16 on the 32x32 image (no BN before it) ----
  bf16x4 xr[8];
  {
    stem_fill<1, true>(a, img, m.ha, m.w1, 0);
    // the dense weights (any kpad <= 128: 8 units per class row, looped)
    for (int q = tid; q < a.kpad * 8; q += PT)
      *reinterpret_cast<bf16x8*>(dw + (q >> 3) * DENSE_KP + (q & 7) * 8) =
          ldg(reinterpret_cast<const bf16x8*>(a.dense_w + q * 8));
    const WLoad L1 = wl_fwd(B0.w1f, 16, 16, 3);
    WLoad LP{};
    if (B0.wpf) LP = wl_fwd(B0.wpf, 16, 16, 1);
    bf16x8 w1r[nreg(conv_units(16, 16, 3))], wpr[1];
    w_prefetch(L1, w1r);
    w_prefetch(LP, wpr);
    bn_prefetch_infer(ld_const(a.bns + (B0.bn1)), 16, bnr);
    __syncthreads();
    f32x4 acc[8];
    zero_acc(acc);
    conv_acc<0, 1, 8, 3, 1, false>(acc, m.ha, m.w1, 0, wave, lane, m.red);
    round_acc<0, 1, false>(xr, acc, xr);
    bn_infer_table(bnr, 16, a.eps, m.tbl);
    __syncthreads();
    w_store(L1, w1r, m.w1);
    w_store(LP, wpr, m.w2);
  }

  // ---- blocks (prn_forward_body's dispatch: one straight-line region per variant) ----
  const int nps = a.nblocks / 3;
  auto run = [&](auto tag, int bi) {
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
    block_infer<S, STR, PROJ>(a, m, xr, bnr, bnx, n1, np, B, wave, lane);
  };
  run(BlkTag<0, 1, true>{}, 0);
  for (int bi = 1; bi < nps; ++bi) run(BlkTag<0, 1, false>{}, bi);
  run(BlkTag<1, 2, true>{}, nps);
  for (int bi = nps + 1; bi < 2 * nps; ++bi) run(BlkTag<1, 1, false>{}, bi);
  run(BlkTag<2, 2, true>{}, 2 * nps);
  for (int bi = 2 * nps + 1; bi < 3 * nps; ++bi) run(BlkTag<2, 1, false>{}, bi);

  // ---- head: final BN + ReLU (its table is in tbl), the 8x8 mean in fp32 rounded to bf16
  //      (bnrelu_avgpool's rounding point), dense in fp32 from the bf16 weights + bias ----
  float* pool_s = m.tbl2;
  const float v = pool_sums<1>(xr, m.tbl, m.red, wave, lane);
  if (tid < 64) {
    const bf16 pb = (bf16)(v / 64.f);
    pool_s[tid] = (float)pb;
    if (a.pooled != nullptr) stg(a.pooled + (long)img * 64 + tid, pb);
  }
  __syncthreads();
  for (int k = tid; k < a.kpad; k += PT) {   // class columns, looped (kpad up to 128)
    float z = 0.f;
    if (k < a.classes) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bf16x8 w = lds16(dw + k * DENSE_KP + j * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += pool_s[j * 8 + e] * (float)w[e];
      }
      z = acc + ldg(a.dense_b + k);
    }
    stg(a.logits + (long)img * a.kpad + k, z);
  }
}

}  // namespace

__global__ void __launch_bounds__(PT, 1) prn_infer_kernel(PrnInferArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  prn_infer_body(a, smem);
}

// ---- host ------------------------------------------------------------------------------
bool prn_infer_supported(int nblocks, int classes, int kpad) {
  return nblocks >= 3 && nblocks % 3 == 0 && classes >= 1 && classes <= kpad && kpad <= 128 &&
         kpad % 16 == 0;
}

// (no grid limit: the workgroups do not wait for each other, so N > CUs is more workgroups)
void prn_infer(const PrnInferArgs& a, hipStream_t s) {
  if (!prn_infer_supported(a.nblocks, a.classes, a.kpad) || a.N < 1)
    throw std::invalid_argument("prn_infer: unsupported shape (3n blocks, classes <= kpad <= 128, kpad % 16 == 0)");
  if (!a.blocks || !a.bns || !a.x_in || !a.stem_w || !a.dense_w || !a.dense_b || !a.logits)
    throw std::invalid_argument("prn_infer: missing pointer");
  hipLaunchKernelGGL(prn_infer_kernel, dim3(a.N), dim3(PT), LDS_TOTAL, s, a);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
