// RMSProp in the form of TF 1.12's tf.train.RMSPropOptimizer (the ApplyRMSProp /
// ApplyCenteredRMSProp kernels; timm's `rmsproptf`): momentum, epsilon INSIDE the square root,
// no bias correction, an optional centered denominator.  With g^ the complete mean gradient,
// s the gradient's scale (1, or clip.hip's clip_scale slot), wd_s the decay of the element's
// tensor and lr the schedule's rate,
//   g'   = s * g^ (+ wd_s * w                 in l2 mode)
//   ms'  = rho * ms + (1 - rho) * (g' * g')
//   mg'  = rho * mg + (1 - rho) * g'          (centered only)
//   d    = ms' + eps                          (centered: (ms' - mg' * mg') + eps)
//   mom' = momentum * mom + (lr * g') / sqrt(d)
//   w'   = w - mom' (- (lr * wd_s) * w, the old w, in decoupled mode)
// as ONE streaming launch over the flat fp32 master, gradient, mom (the momentum buffer), ms and
// -- centered only -- mg: optim_device.h's FlatWalk, in adam_update_pack's shape, with RmsStep
// as its step (16-byte loads of g, ms, mom [, mg] and stores of ms, mom [, mg] beside the walk's
// w and bf16 copy).  ohwi_pack follows, with its global_step += 1, as after adam_update_pack.
// ms starts from ones (TF's `rms` slot), mg and mom from zeros: the host's to arrange.
// The decay of a segment is wd_seg[segment] (train/layout.py adam_decay_table); the decay mode
// is uniform over the launch.  One lane per workgroup evaluates lr (lr_at) ahead of the loads,
// and the rate rides the barrier that publishes the segment table.  Nothing is read by the host.
// Per element everything is fp32 with floating-point contraction off in the helper: each
// product, sum, difference, square root and quotient is rounded exactly once, as written
// (sqrtf and / are the correctly rounded ones adam.hip uses; tests/rmsprop_oracle.py counts
// them).  1 - rho comes rounded once from fp64 on the host (adam_coef: b1 = rho, b2 = momentum).
// With g = mom = 0 and no decay the quotient is 0 / sqrt(d) = 0 (d >= eps > 0 is the binding's
// to check), so w and mom are left bit for bit and ms' is the one rounding of rho * ms.  A NaN
// gradient shows in its own element's ms', mom' and w' (and mg'), and nowhere else.
// CENTERED is a template parameter: the plain kernel carries no third stream in registers or
// code and never touches mg (a null pointer will do).
// ms, mg and mom are touched once per step by this kernel alone and are read and written
// non-temporally (NT; profiles/rmsprop.md has the A/B against plain accesses, the build with
// -DDTR_RMSPROP_NT=0: 151 -> 138 us plain and 185 -> 164 us centered at ImageNet ResNet-50's
// 25.5 M elements, about the spread at CIFAR's 0.76 M); w and the bf16 copy, which the next
// forward reads, keep ordinary stores.
#include "optim_device.h"

namespace dtr {

#ifndef DTR_RMSPROP_NT
#define DTR_RMSPROP_NT 1          // -DDTR_RMSPROP_NT=0: the A/B build of profiles/rmsprop.md
#endif
constexpr bool RMSPROP_NT = DTR_RMSPROP_NT != 0;   // non-temporal ms / mg / mom accesses

// c: adam_coef(rho, momentum, eps), so c.b1 = rho, c.omb1 = 1 - rho, c.b2 = momentum.
template <bool CENTERED>
__device__ __forceinline__ void rms_elem(float& w, float g, float& ms, float& mg, float& mom,
                                         float s, float wd, float lr, float lrwd,
                                         const AdamCoef& c, bool decoupled) {
#pragma clang fp contract(off)
  float gp = s * g;
  if (!decoupled) {
    const float l2 = wd * w;
    gp = gp + l2;
  }
  const float g2 = gp * gp;
  const float s1 = c.b1 * ms, s2 = c.omb1 * g2;
  ms = s1 + s2;
  float d = ms;
  if constexpr (CENTERED) {
    const float a1 = c.b1 * mg, a2 = c.omb1 * gp;
    mg = a1 + a2;
    const float mg2 = mg * mg;
    d = ms - mg2;
  }
  d = d + c.eps;
  const float num = lr * gp;
  const float q = num / sqrtf(d);
  const float carried = c.b2 * mom;
  mom = carried + q;
  float wn = w - mom;
  if (decoupled) {
    const float dec = lrwd * w;
    wn = wn - dec;
  }
  w = wn;
}

// FlatWalk's step: what rmsprop keeps beside w.
template <bool CENTERED, bool NT>
struct RmsStep {
  const float* __restrict__ g;
  float* __restrict__ ms;
  float* __restrict__ mg;     // CENTERED only; never touched otherwise
  float* __restrict__ mom;
  const float* __restrict__ wd_seg;
  AdamCoef c;
  float grad_scale, lr;
  bool dec;
  static constexpr bool update = true;

  __device__ __forceinline__ void operator()(int sgi, long e0, f32x4& wv) const {
    const f32x4 gv = ld4<false>(g + e0);
    f32x4 sv = ld4<NT>(ms + e0);
    f32x4 mv = ld4<NT>(mom + e0);
    f32x4 av = {0.f, 0.f, 0.f, 0.f};
    if constexpr (CENTERED) av = ld4<NT>(mg + e0);
    const float wd = wd_seg[sgi];
    const float lrwd = lr * wd;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float wj = wv[j], sj = sv[j], aj = av[j], mj = mv[j];
      rms_elem<CENTERED>(wj, gv[j], sj, aj, mj, grad_scale, wd, lr, lrwd, c, dec);
      wv[j] = wj;
      sv[j] = sj;
      mv[j] = mj;
      if constexpr (CENTERED) av[j] = aj;
    }
    st4<NT>(ms + e0, sv);
    st4<NT>(mom + e0, mv);
    if constexpr (CENTERED) st4<NT>(mg + e0, av);
  }

  __device__ __forceinline__ void operator()(int sgi, long e, float& wj) const {
    const float wd = wd_seg[sgi];
    float sj = ms[e], mj = mom[e], aj = 0.f;
    if constexpr (CENTERED) aj = mg[e];
    rms_elem<CENTERED>(wj, g[e], sj, aj, mj, grad_scale, wd, lr, lr * wd, c, dec);
    ms[e] = sj;
    mom[e] = mj;
    if constexpr (CENTERED) mg[e] = aj;
  }
};

template <bool CENTERED, bool CLIP, bool NT>
__global__ void __launch_bounds__(256)
rmsprop_pack_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ ms,
                    float* __restrict__ mg, float* __restrict__ mom, long n, LrSchedule sched,
                    const long long* __restrict__ gstep, AdamCoef c, float grad_scale,
                    const float* __restrict__ clip, int decoupled,
                    const ParamSeg* __restrict__ segs, int nseg,
                    const float* __restrict__ wd_seg, bf16* __restrict__ bf,
                    float* __restrict__ lr_out) {
  __shared__ ParamSeg sseg[SEG_LDS_MAX];
  __shared__ float lr_s;
  if constexpr (CLIP) grad_scale = clip[1];
  if (threadIdx.x == 0) {
    const float lr = lr_at(sched, gstep ? (long)*gstep : 0L);
    lr_s = lr;
    if (lr_out && blockIdx.x == 0) *lr_out = lr;
  }
  const FlatWalk walk(sseg, segs, nseg, true);   // the table and the rate
  walk.run(w, n, bf, RmsStep<CENTERED, NT>{g, ms, mg, mom, wd_seg, c, grad_scale, lr_s,
                                           decoupled != 0});   // (the mode: uniform)
}

template <bool CENTERED, bool CLIP>
static void rmsprop_launch(float* master, const float* grad, float* ms, float* mg, float* mom,
                           long n, const LrSchedule& s, const long long* gstep,
                           const AdamCoef& c, float grad_scale, const float* clip, int decoupled,
                           const ParamSeg* segs, int nseg, const float* wd_seg, bf16* bf,
                           float* lr_out, hipStream_t st) {
  hipLaunchKernelGGL((rmsprop_pack_kernel<CENTERED, CLIP, RMSPROP_NT>), dim3(flat_blocks(n)),
                     dim3(256), 0, st, master, grad, ms, mg, mom, n, s, gstep, c,
                     CLIP ? 1.f : grad_scale, clip, decoupled, segs, nseg, wd_seg, bf, lr_out);
}

void rmsprop_update_pack(float* master, const float* grad, float* ms, float* mg, float* mom,
                         long n, const LrSchedule& s, const long long* gstep, float rho,
                         float momentum, float epsilon, float grad_scale, const float* clip,
                         int centered, int decoupled, const ParamSeg* segs, int nseg,
                         const float* wd_seg, bf16* bf, float* lr_out, hipStream_t st) {
  if (n <= 0) return;
  const AdamCoef c = adam_coef(rho, momentum, epsilon);
  auto go = centered ? (clip ? rmsprop_launch<true, true> : rmsprop_launch<true, false>)
                     : (clip ? rmsprop_launch<false, true> : rmsprop_launch<false, false>);
  go(master, grad, ms, mg, mom, n, s, gstep, c, grad_scale, clip, decoupled, segs, nseg, wd_seg,
     bf, lr_out, st);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
