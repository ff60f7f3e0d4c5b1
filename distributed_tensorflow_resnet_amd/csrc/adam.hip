// AdamW (Adam with decoupled weight decay, Loshchilov & Hutter 2019; the Adam part in the
// form of tf.train.AdamOptimizer, whose epsilon sits outside the bias correction): with g^
// the complete mean gradient, s the gradient's scale (1, or clip.hip's clip_scale slot),
// wd_s the decay of the element's tensor and t = global_step - adam_start_step + 1,
//   g'    = s * g^ (+ wd_s * w              in l2 mode)
//   m'    = b1 * m + (1 - b1) * g'
//   v'    = b2 * v + (1 - b2) * g' * g'
//   alpha = lr * sqrt(1 - b2^t) / (1 - b1^t)
//   w'    = w - alpha * m' / (sqrt(v') + eps) (- lr * wd_s * w, the old w, in decoupled mode)
// as ONE streaming launch over the flat fp32 master, gradient and the two moment buffers
// (the first moment lives in the momentum buffer): optim_device.h's FlatWalk, in
// sgd_update_pack's shape, with AdamStep as its step (16-byte loads of g, m, v and stores of
// m, v beside the walk's w and bf16 copy).  ohwi_pack follows, with its global_step += 1, as
// after sgd_update_pack.
// The decay of a segment is wd_seg[segment] (train/layout.py adam_decay_table), as LARS
// reads trust[]; the decay mode is uniform over the launch.
// Bias correction (optim_device.h bias_correction): one lane per workgroup evaluates lr
// (lr_at) and alpha ahead of the loads, and both ride the barrier that publishes the segment
// table.  t is a 64-bit integer; the square root and the quotient are fp64, and the result is
// rounded to fp32 once: within one fp32 ulp of the correctly rounded value.  Nothing is read
// by the host.
// Per element everything is fp32, each product, sum, square root and quotient rounded at
// most once (sqrtf and / are correctly rounded; tests/adam_oracle.py counts them).  1 - b1
// and 1 - b2 come rounded once from fp64 on the host.  With g = m = v = 0 and no decay the
// quotient is 0 / eps = 0 and w is left bit for bit (eps > 0 is the binding's to check).
// m and v are touched once per step by this kernel alone and are read and written
// non-temporally (NT; profiles/adam.md has the A/B against plain accesses: 163 -> 142 us at
// ImageNet ResNet-50's 25.5 M elements, no difference at CIFAR's 0.76 M); w and the bf16
// copy, which the next forward reads, keep ordinary stores.
#include "optim_device.h"

namespace dtr {

#ifndef DTR_ADAM_NT
#define DTR_ADAM_NT 1             // -DDTR_ADAM_NT=0: the A/B build of profiles/adam.md
#endif
constexpr bool ADAM_NT = DTR_ADAM_NT != 0;   // non-temporal m / v accesses

__device__ __forceinline__ void adam_elem(float& w, float g, float& m, float& v, float s,
                                          float wd, float lrwd, float alpha, const AdamCoef& c,
                                          bool decoupled) {
  float gp = g * s;
  if (!decoupled) gp += wd * w;
  m = c.b1 * m + c.omb1 * gp;
  v = c.b2 * v + c.omb2 * (gp * gp);
  const float q = m / (sqrtf(v) + c.eps);
  float wn = w - alpha * q;
  if (decoupled) wn -= lrwd * w;
  w = wn;
}

// FlatWalk's step: what adam keeps beside w.
template <bool NT>
struct AdamStep {
  const float* __restrict__ g;
  float* __restrict__ m;
  float* __restrict__ v;
  const float* __restrict__ wd_seg;
  AdamCoef c;
  float grad_scale, lr, alpha;
  bool dec;
  static constexpr bool update = true;

  __device__ __forceinline__ void operator()(int sgi, long e0, f32x4& wv) const {
    const f32x4 gv = ld4<false>(g + e0);
    f32x4 mv = ld4<NT>(m + e0);
    f32x4 vv = ld4<NT>(v + e0);
    const float wd = wd_seg[sgi];
    const float lrwd = lr * wd;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float wj = wv[j], mj = mv[j], vj = vv[j];
      adam_elem(wj, gv[j], mj, vj, grad_scale, wd, lrwd, alpha, c, dec);
      wv[j] = wj;
      mv[j] = mj;
      vv[j] = vj;
    }
    st4<NT>(m + e0, mv);
    st4<NT>(v + e0, vv);
  }

  __device__ __forceinline__ void operator()(int sgi, long e, float& wj) const {
    const float wd = wd_seg[sgi];
    float mj = m[e], vj = v[e];
    adam_elem(wj, g[e], mj, vj, grad_scale, wd, lr * wd, alpha, c, dec);
    m[e] = mj;
    v[e] = vj;
  }
};

template <bool CLIP, bool NT>
__global__ void __launch_bounds__(256)
adam_pack_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                 float* __restrict__ v, long n, LrSchedule sched,
                 const long long* __restrict__ gstep, const long long* __restrict__ start,
                 AdamCoef c, float grad_scale, const float* __restrict__ clip, int decoupled,
                 const ParamSeg* __restrict__ segs, int nseg, const float* __restrict__ wd_seg,
                 bf16* __restrict__ bf, float* __restrict__ lr_out, float* __restrict__ adam_out) {
  __shared__ ParamSeg sseg[SEG_LDS_MAX];
  __shared__ float rate_s[2];
  if constexpr (CLIP) grad_scale = clip[1];
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
  walk.run(w, n, bf, AdamStep<NT>{g, m, v, wd_seg, c, grad_scale, rate_s[0], rate_s[1],
                                  decoupled != 0});   // (the mode: uniform over the launch)
}

void adam_update_pack(float* master, const float* grad, float* m, float* v, long n,
                      const LrSchedule& s, const long long* gstep, const long long* start_step,
                      float beta1, float beta2, float epsilon, float grad_scale,
                      const float* clip, int decoupled, const ParamSeg* segs, int nseg,
                      const float* wd_seg, bf16* bf, float* lr_out, float* adam_out,
                      hipStream_t st) {
  if (n <= 0) return;
  const AdamCoef c = adam_coef(beta1, beta2, epsilon);
  if (clip)
    hipLaunchKernelGGL((adam_pack_kernel<true, ADAM_NT>), dim3(flat_blocks(n)), dim3(256), 0, st,
                       master, grad, m, v, n, s, gstep, start_step, c, 1.f, clip, decoupled, segs,
                       nseg, wd_seg, bf, lr_out, adam_out);
  else
    hipLaunchKernelGGL((adam_pack_kernel<false, ADAM_NT>), dim3(flat_blocks(n)), dim3(256), 0, st,
                       master, grad, m, v, n, s, gstep, start_step, c, grad_scale, clip, decoupled,
                       segs, nseg, wd_seg, bf, lr_out, adam_out);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
