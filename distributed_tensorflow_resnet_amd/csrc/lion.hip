// Lion (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms"): the update is the
// sign of an interpolated momentum.  With g^ the complete mean gradient, s the gradient's
// scale (1, or clip.hip's clip_scale slot), wd_s the decay of the element's tensor and lr the
// schedule's rate,
//   g' = s * g^
//   c  = b1 * m + (1 - b1) * g'
//   u  = 1 if c > 0, -1 if c < 0, else c     (+-0 stays 0 and a NaN stays a NaN)
//   w' = (w - lr * u) - (lr * wd_s) * w      (the old w: the decay is decoupled, as adamw's)
//   m' = b2 * m + (1 - b2) * g'
// as ONE streaming launch over the flat fp32 master, gradient and m (the momentum buffer, the
// only state): optim_device.h's FlatWalk, in adam_update_pack's shape, with LionStep as its
// step (16-byte loads of g and m and stores of m beside the walk's w and bf16 copy).
// ohwi_pack follows, with its global_step += 1, as after adam_update_pack.
// The decay of a segment is wd_seg[segment] (train/layout.py adam_decay_table).  One lane per
// workgroup evaluates lr (lr_at) ahead of the loads, and the rate rides the barrier that
// publishes the segment table.  Nothing is read by the host.
// Per element everything is fp32 with floating-point contraction off in the helper: each
// product, sum and difference is rounded exactly once, as written (tests/lion_oracle.py counts
// them).  There is no square root, no division and no bias correction; 1 - b1 and 1 - b2 come
// rounded once from fp64 on the host (adam_coef; its epsilon is unused here).  lr * u is exact
// (u is +-1 or 0), so every element whose c is not 0 moves by exactly lr before the decay.
// With g = m = 0 and no decay c = 0, u = 0 and w, m are left bit for bit.
// m is touched once per step by this kernel alone and is read and written non-temporally (NT;
// profiles/lion.md has the A/B against plain accesses: 127 -> 120 us at ImageNet ResNet-50's
// 25.5 M elements, no difference at CIFAR's 0.76 M); w and the bf16 copy, which the next
// forward reads, keep ordinary stores.
#include "optim_device.h"

namespace dtr {

#ifndef DTR_LION_NT
#define DTR_LION_NT 1             // -DDTR_LION_NT=0: the A/B build of profiles/lion.md
#endif
constexpr bool LION_NT = DTR_LION_NT != 0;   // non-temporal m accesses

__device__ __forceinline__ void lion_elem(float& w, float g, float& m, float s, float lr,
                                          float lrwd, const AdamCoef& c) {
#pragma clang fp contract(off)
  const float gp = s * g;
  const float c1 = c.b1 * m, c2 = c.omb1 * gp;
  const float ci = c1 + c2;
  const float u = ci > 0.f ? 1.f : ci < 0.f ? -1.f : ci;
  const float m1 = c.b2 * m, m2 = c.omb2 * gp;
  m = m1 + m2;
  const float step = lr * u;
  const float moved = w - step;
  const float dec = lrwd * w;
  w = moved - dec;
}

// FlatWalk's step: what lion keeps beside w.
template <bool NT>
struct LionStep {
  const float* __restrict__ g;
  float* __restrict__ m;
  const float* __restrict__ wd_seg;
  AdamCoef c;
  float grad_scale, lr;
  static constexpr bool update = true;

  __device__ __forceinline__ void operator()(int sgi, long e0, f32x4& wv) const {
    const f32x4 gv = ld4<false>(g + e0);
    f32x4 mv = ld4<NT>(m + e0);
    const float lrwd = lr * wd_seg[sgi];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float wj = wv[j], mj = mv[j];
      lion_elem(wj, gv[j], mj, grad_scale, lr, lrwd, c);
      wv[j] = wj;
      mv[j] = mj;
    }
    st4<NT>(m + e0, mv);
  }

  __device__ __forceinline__ void operator()(int sgi, long e, float& wj) const {
    float mj = m[e];
    lion_elem(wj, g[e], mj, grad_scale, lr, lr * wd_seg[sgi], c);
    m[e] = mj;
  }
};

template <bool CLIP, bool NT>
__global__ void __launch_bounds__(256)
lion_pack_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                 long n, LrSchedule sched, const long long* __restrict__ gstep, AdamCoef c,
                 float grad_scale, const float* __restrict__ clip,
                 const ParamSeg* __restrict__ segs, int nseg, const float* __restrict__ wd_seg,
                 bf16* __restrict__ bf, float* __restrict__ lr_out) {
  __shared__ ParamSeg sseg[SEG_LDS_MAX];
  __shared__ float lr_s;
  if constexpr (CLIP) grad_scale = clip[1];
  if (threadIdx.x == 0) {
    const float lr = lr_at(sched, gstep ? (long)*gstep : 0L);
    lr_s = lr;
    if (lr_out && blockIdx.x == 0) *lr_out = lr;
  }
  const FlatWalk walk(sseg, segs, nseg, true);   // the table and the rate
  walk.run(w, n, bf, LionStep<NT>{g, m, wd_seg, c, grad_scale, lr_s});
}

void lion_update_pack(float* master, const float* grad, float* m, long n, const LrSchedule& s,
                      const long long* gstep, float beta1, float beta2, float grad_scale,
                      const float* clip, const ParamSeg* segs, int nseg, const float* wd_seg,
                      bf16* bf, float* lr_out, hipStream_t st) {
  if (n <= 0) return;
  const AdamCoef c = adam_coef(beta1, beta2, 0.f);
  if (clip)
    hipLaunchKernelGGL((lion_pack_kernel<true, LION_NT>), dim3(flat_blocks(n)), dim3(256), 0, st,
                       master, grad, m, n, s, gstep, c, 1.f, clip, segs, nseg, wd_seg, bf, lr_out);
  else
    hipLaunchKernelGGL((lion_pack_kernel<false, LION_NT>), dim3(flat_blocks(n)), dim3(256), 0, st,
                       master, grad, m, n, s, gstep, c, grad_scale, clip, segs, nseg, wd_seg, bf,
                       lr_out);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
