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
// (the first moment lives in the momentum buffer), in sgd_update_pack's shape: 256 threads,
// at most 4096 workgroups, four consecutive elements per thread and trip (16-byte loads of
// w, g, m, v; 16-byte stores of w, m, v; an 8-byte store of the bf16 HWIO copy), the
// parameter segment tracked incrementally from the LDS copy of the table.  ohwi_pack
// follows, with its global_step += 1, as after sgd_update_pack.
// The decay of a segment is wd_seg[segment] (train/layout.py adam_decay_table), as LARS
// reads trust[]; the decay mode is uniform over the launch.
// Bias correction: one lane per workgroup evaluates lr (lr_at) and alpha ahead of the
// loads, and both ride the barrier that publishes the segment table.  t is a 64-bit
// integer; 1 - b^t is -expm1(t * log(b)) in fp64 (no cancellation at small t; b = 0 gives
// exactly 1), the square root and the quotient are fp64, and the result is rounded to fp32
// once: within one fp32 ulp of the correctly rounded value.  Nothing is read by the host.
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

struct AdamCoef {
  float b1, omb1, b2, omb2, eps;
};

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

template <bool NT>
__device__ __forceinline__ f32x4 adam_ld4(const float* p) {
  if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
  else return *reinterpret_cast<const f32x4*>(p);
}

template <bool NT>
__device__ __forceinline__ void adam_st4(float* p, f32x4 x) {
  if constexpr (NT) __builtin_nontemporal_store(x, reinterpret_cast<f32x4*>(p));
  else *reinterpret_cast<f32x4*>(p) = x;
}

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
    long long t = step - (start ? *start : 0ll) + 1;
    if (t < 1) t = 1;
    const double c1 = -expm1((double)t * log((double)c.b1));
    const double c2 = -expm1((double)t * log((double)c.b2));
    const float alpha = (float)((double)lr * sqrt(c2) / c1);
    rate_s[0] = lr;
    rate_s[1] = alpha;
    if (blockIdx.x == 0) {
      if (lr_out) *lr_out = lr;
      if (adam_out) {
        adam_out[0] = lr;
        adam_out[1] = alpha;
        adam_out[2] = (float)t;
      }
    }
  }
  const ParamSeg* S = segs;
  if (nseg <= SEG_LDS_MAX) {
    for (int i = threadIdx.x; i < nseg; i += blockDim.x) sseg[i] = segs[i];
    S = sseg;
  }
  __syncthreads();   // the table and the two rates
  const float lr = rate_s[0], alpha = rate_s[1];
  const bool dec = decoupled != 0;   // uniform over the launch
  const long nv = (n + 3) / 4;
  const long stride = (long)gridDim.x * blockDim.x;
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= nv) return;
  int sgi = find_seg(S, nseg, i * 4);
  for (; i < nv; i += stride) {
    const long e0 = i * 4;
    while (sgi + 1 < nseg && S[sgi + 1].offset <= e0) ++sgi;
    const ParamSeg& sg = S[sgi];
    const bool whole = e0 + 4 <= n && e0 + 4 <= sg.offset + sg.numel;
    if (whole) {
      f32x4 wv = *reinterpret_cast<const f32x4*>(w + e0);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + e0);
      f32x4 mv = adam_ld4<NT>(m + e0);
      f32x4 vv = adam_ld4<NT>(v + e0);
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
      adam_st4<NT>(m + e0, mv);
      adam_st4<NT>(v + e0, vv);
      *reinterpret_cast<f32x4*>(w + e0) = wv;
      if (bf && sg.bf_hwio >= 0) {
        if (sg.kpad == sg.K && ((e0 - sg.offset) & 3) == 0) {
          bf16x4 h = {(bf16)wv[0], (bf16)wv[1], (bf16)wv[2], (bf16)wv[3]};
          *reinterpret_cast<bf16x4*>(bf + sg.bf_hwio + (e0 - sg.offset)) = h;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) write_hwio(sg, e0 + j, wv[j], bf);
        }
      }
    } else {   // a vector straddling a segment end (e.g. a 10-class bias) or the tail
      for (int j = 0; j < 4 && e0 + j < n; ++j) {
        const long e = e0 + j;
        const int sj_i = find_seg(S, nseg, e);
        const ParamSeg& sj = S[sj_i];
        const float wd = wd_seg[sj_i];
        float wj = w[e], mj = m[e], vj = v[e];
        adam_elem(wj, g[e], mj, vj, grad_scale, wd, lr * wd, alpha, c, dec);
        m[e] = mj;
        v[e] = vj;
        w[e] = wj;
        if (bf) write_hwio(sj, e, wj, bf);
      }
    }
  }
}

void adam_update_pack(float* master, const float* grad, float* m, float* v, long n,
                      const LrSchedule& s, const long long* gstep, const long long* start_step,
                      float beta1, float beta2, float epsilon, float grad_scale,
                      const float* clip, int decoupled, const ParamSeg* segs, int nseg,
                      const float* wd_seg, bf16* bf, float* lr_out, float* adam_out,
                      hipStream_t st) {
  if (n <= 0) return;
  long blocks = ((n + 3) / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  const AdamCoef c{beta1, (float)(1.0 - (double)beta1), beta2, (float)(1.0 - (double)beta2),
                   epsilon};
  if (clip)
    hipLaunchKernelGGL((adam_pack_kernel<true, ADAM_NT>), dim3((unsigned)blocks), dim3(256), 0, st,
                       master, grad, m, v, n, s, gstep, start_step, c, 1.f, clip, decoupled, segs,
                       nseg, wd_seg, bf, lr_out, adam_out);
  else
    hipLaunchKernelGGL((adam_pack_kernel<false, ADAM_NT>), dim3((unsigned)blocks), dim3(256), 0,
                       st, master, grad, m, v, n, s, gstep, start_step, c, grad_scale, clip,
                       decoupled, segs, nseg, wd_seg, bf, lr_out, adam_out);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
