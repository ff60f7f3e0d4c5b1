// LAMB (You et al. 2020, "Large Batch Optimization for Deep Learning", Algorithm 2 with bias
// correction, in the form of TF-Addons' LAMB: epsilon after the square root of the corrected
// second moment, phi the identity, no clamp): adamw's direction at a per-tensor rate.  With
// g^ the complete mean gradient, s the gradient's scale (1, or clip.hip's clip_scale slot),
// wd_s the decay of the element's tensor and t = global_step - adam_start_step + 1,
//   g' = s * g^ (+ wd_s * w             in l2 mode)
//   m' = b1 * m + (1 - b1) * g'
//   v' = b2 * v + (1 - b2) * g' * g'
//   r  = (m' * k1) / (sqrtf(v' * k2) + eps)      k1 = 1 / (1 - b1^t),  k2 = 1 / (1 - b2^t)
//   u  = r (+ wd_s * w                  in decoupled mode)
//   trust_s = ||w_s|| / ||u_s||  for an adapted tensor with both norms > 0, else exactly 1
//   w' = w - (lr * trust_s) * u
// The norm of u exists only after the moments are updated and before any weight moves, so
// the step is three launches over the flat fp32 master, gradient and the two moment buffers:
//   lamb_moments_norms  one workgroup per LARS_CHUNK elements of one tensor (lars.hip's chunk
//                table): reads w, g, m, v, stores m' and v' in place, and writes the chunk's
//                sums of w^2 and u^2 to part[chunk].  Head / body / tail as lars_norms
//                (chunk_span), the stores included: no workgroup touches an element of a
//                neighbouring tensor.  A thread adds at most 18 squares in fp32; the wave
//                shuffles, the four waves (block_sum_f64), the chunks, the square roots and
//                the ratio are fp64.  No atomics, a fixed order.
//   lamb_trust   one wave per tensor: its chunks' partials added in chunk order
//                (seg_part_sums), the two norms and the trust ratio (lars_trust's rule).
//   lamb_update_pack  the FlatWalk with LambApply as its step: reads w, m', v', forms u again
//                with the same helper and the same k1, k2 -- evaluated again from the same
//                integers, never read from a slot another workgroup writes -- and writes w
//                and the bf16 HWIO copy.  ohwi_pack follows, with its global_step += 1, as
//                after adam_update_pack.
// The walks, the reductions, AdamCoef and bias_correction are optim_device.h's; this file
// has u, its application and the closing formula of the trust ratio.
// u is recomputed rather than kept: a scratch buffer would cost the same bytes, and the
// gradient buffer stays untouched (the update launch does not read it at all).
// k1 and k2: one lane per workgroup, from the fp64 bias correction, each rounded to fp32
// once.  Nothing is read by the host, so a captured graph replays the step.
// Per element everything is fp32 with floating-point contraction off in the helper: each
// product, sum, square root and quotient is rounded exactly once, and both passes form the
// same bits of u (tests/lamb_oracle.py counts the roundings).  With g = m = v = 0 and no
// decay u = 0 / eps = 0: the tensor's |u| is 0, its trust 1 and w is left bit for bit.
// m' and v' are stored and read back non-temporally, as in adam.hip.
#include "optim_device.h"

namespace dtr {

constexpr bool LAMB_NT = true;   // non-temporal m / v accesses (profiles/adam.md)

// MOMENTS: m and v are the old moments and are updated from g first (the norm pass);
// otherwise they are m' and v' already (the update pass) and g, s are unused.  Returns u.
template <bool MOMENTS>
__device__ __forceinline__ float lamb_elem(float w, float g, float& m, float& v, float s,
                                           float wd, float k1, float k2, const AdamCoef& c,
                                           bool decoupled) {
#pragma clang fp contract(off)
  if constexpr (MOMENTS) {
    float gp = s * g;
    if (!decoupled) gp = gp + wd * w;
    const float m1 = c.b1 * m, m2 = c.omb1 * gp;
    m = m1 + m2;
    const float v1 = c.b2 * v, g2 = gp * gp;
    const float v2 = c.omb2 * g2;
    v = v1 + v2;
  }
  const float num = m * k1;
  const float den = sqrtf(v * k2) + c.eps;
  float u = num / den;
  if (decoupled) {
    const float d = wd * w;
    u = u + d;
  }
  return u;
}

__device__ __forceinline__ float lamb_apply(float w, float rate, float u) {
#pragma clang fp contract(off)
  const float p = rate * u;
  return w - p;
}

template <bool CLIP, bool NT>
__global__ void __launch_bounds__(256)
lamb_moments_norms_kernel(const float* __restrict__ w, const float* __restrict__ g,
                          float* __restrict__ m, float* __restrict__ v,
                          const long long* __restrict__ gstep,
                          const long long* __restrict__ start_step, AdamCoef c, float grad_scale,
                          const float* __restrict__ clip, int decoupled,
                          const ParamSeg* __restrict__ segs, const LarsSeg* __restrict__ lsegs,
                          const int* __restrict__ blk_seg, const float* __restrict__ wd_seg,
                          double* __restrict__ part) {
  __shared__ float k_s[2];
  if constexpr (CLIP) grad_scale = clip[1];
  const int tid = threadIdx.x;
  const int si = blk_seg[blockIdx.x];
  const ChunkSpan ch = chunk_span(segs[si].offset, segs[si].numel,
                                  (long long)blockIdx.x - lsegs[si].chunk0, LARS_CHUNK);
  const float wd = wd_seg[si];
  const bool dec = decoupled != 0;                // uniform over the launch
  f32x4 a[4], b[4], mm[4], vv[4];                 // 16 loads in flight (nvec <= 4 * 256)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = tid + j * 256;
    a[j] = b[j] = mm[j] = vv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (k < ch.nvec) {
      a[j] = *reinterpret_cast<const f32x4*>(w + ch.body0 + 4ll * k);
      b[j] = *reinterpret_cast<const f32x4*>(g + ch.body0 + 4ll * k);
      mm[j] = ld4<NT>(m + ch.body0 + 4ll * k);
      vv[j] = ld4<NT>(v + ch.body0 + 4ll * k);
    }
  }
  if (tid == 0) {
    const BiasCorrection bc = bias_correction(gstep ? *gstep : 0ll, start_step, c);
    k_s[0] = bc.k1();
    k_s[1] = bc.k2();
  }
  __syncthreads();   // k1, k2
  const float k1 = k_s[0], k2 = k_s[1];
  float sw = 0.f, su = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = tid + j * 256;
    if (k < ch.nvec) {   // (no store outside the body; the zeros of the other slots add nothing)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float mi = mm[j][i], vi = vv[j][i];
        const float u = lamb_elem<true>(a[j][i], b[j][i], mi, vi, grad_scale, wd, k1, k2, c, dec);
        mm[j][i] = mi;
        vv[j][i] = vi;
        sw += a[j][i] * a[j][i];
        su += u * u;
      }
      st4<NT>(m + ch.body0 + 4ll * k, mm[j]);
      st4<NT>(v + ch.body0 + 4ll * k, vv[j]);
    }
  }
  if (tid < ch.head) {
    const long long e = ch.start + tid;
    const float x = w[e];
    float mi = m[e], vi = v[e];
    const float u = lamb_elem<true>(x, g[e], mi, vi, grad_scale, wd, k1, k2, c, dec);
    m[e] = mi;
    v[e] = vi;
    sw += x * x;
    su += u * u;
  }
  if (tid < ch.tail) {
    const long long e = ch.tail0 + tid;
    const float x = w[e];
    float mi = m[e], vi = v[e];
    const float u = lamb_elem<true>(x, g[e], mi, vi, grad_scale, wd, k1, k2, c, dec);
    m[e] = mi;
    v[e] = vi;
    sw += x * x;
    su += u * u;
  }
  block_sum_f64<2>({sw, su}, part);
}

void lamb_moments_norms(const float* master, const float* grad, float* m, float* v,
                        const long long* gstep, const long long* start_step, float beta1,
                        float beta2, float epsilon, float grad_scale, const float* clip,
                        int decoupled, const ParamSeg* segs, const LarsSeg* lsegs,
                        const int* blk_seg, int nblocks, const float* wd_seg, double* part,
                        hipStream_t st) {
  if (nblocks <= 0) return;
  const AdamCoef c = adam_coef(beta1, beta2, epsilon);
  if (clip)
    hipLaunchKernelGGL((lamb_moments_norms_kernel<true, LAMB_NT>), dim3((unsigned)nblocks),
                       dim3(256), 0, st, master, grad, m, v, gstep, start_step, c, 1.f, clip,
                       decoupled, segs, lsegs, blk_seg, wd_seg, part);
  else
    hipLaunchKernelGGL((lamb_moments_norms_kernel<false, LAMB_NT>), dim3((unsigned)nblocks),
                       dim3(256), 0, st, master, grad, m, v, gstep, start_step, c, grad_scale,
                       clip, decoupled, segs, lsegs, blk_seg, wd_seg, part);
  DTR_CHECK_LAUNCH();
}

__global__ void __launch_bounds__(64)
lamb_trust_kernel(const double* __restrict__ part, const LarsSeg* __restrict__ lsegs,
                  float* __restrict__ trust, float* __restrict__ wn, float* __restrict__ un) {
  const int si = blockIdx.x;
  const LarsSeg ls = lsegs[si];
  double sw, su;
  seg_part_sums(part, ls, sw, su);
  if (threadIdx.x == 0) {
    const double w_n = sqrt(sw), u_n = sqrt(su);
    float t = 1.f;
    if (!ls.skip && w_n > 0.0 && u_n > 0.0) t = (float)(w_n / u_n);
    trust[si] = t;
    wn[si] = (float)w_n;
    un[si] = (float)u_n;
  }
}

void lamb_trust(const double* part, const LarsSeg* lsegs, int nseg, float* trust, float* wn,
                float* un, hipStream_t st) {
  if (nseg <= 0) return;
  hipLaunchKernelGGL(lamb_trust_kernel, dim3((unsigned)nseg), dim3(64), 0, st, part, lsegs, trust,
                     wn, un);
  DTR_CHECK_LAUNCH();
}

// FlatWalk's step: u from the stored m' and v', applied at the segment's rate.
template <bool NT>
struct LambApply {
  const float* __restrict__ m;
  const float* __restrict__ v;
  const float* __restrict__ wd_seg;
  const float* __restrict__ trust;
  AdamCoef c;
  float lr, k1, k2;
  bool dec;
  static constexpr bool update = true;

  __device__ __forceinline__ void operator()(int sgi, long e0, f32x4& wv) const {
    const f32x4 mv = ld4<NT>(m + e0);
    const f32x4 vv = ld4<NT>(v + e0);
    const float wd = wd_seg[sgi];
    const float rate = lr * trust[sgi];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float mj = mv[j], vj = vv[j];
      const float u = lamb_elem<false>(wv[j], 0.f, mj, vj, 1.f, wd, k1, k2, c, dec);
      wv[j] = lamb_apply(wv[j], rate, u);
    }
  }

  __device__ __forceinline__ void operator()(int sgi, long e, float& wj) const {
    float mj = m[e], vj = v[e];
    const float u = lamb_elem<false>(wj, 0.f, mj, vj, 1.f, wd_seg[sgi], k1, k2, c, dec);
    wj = lamb_apply(wj, lr * trust[sgi], u);
  }
};

template <bool NT>
__global__ void __launch_bounds__(256)
lamb_pack_kernel(float* __restrict__ w, const float* __restrict__ m, const float* __restrict__ v,
                 long n, LrSchedule sched, const long long* __restrict__ gstep,
                 const long long* __restrict__ start_step, AdamCoef c, int decoupled,
                 const ParamSeg* __restrict__ segs, int nseg, const float* __restrict__ wd_seg,
                 const float* __restrict__ trust, bf16* __restrict__ bf,
                 float* __restrict__ lr_out, float* __restrict__ adam_out) {
  __shared__ ParamSeg sseg[SEG_LDS_MAX];
  __shared__ float rate_s[3];
  if (threadIdx.x == 0) {
    const long long step = gstep ? *gstep : 0ll;
    const float lr = lr_at(sched, (long)step);
    const BiasCorrection b = bias_correction(step, start_step, c);
    rate_s[0] = lr;
    rate_s[1] = b.k1();
    rate_s[2] = b.k2();
    if (blockIdx.x == 0) {
      if (lr_out) *lr_out = lr;
      if (adam_out) {   // adam_update_pack's slot: {lr, alpha, t}
        adam_out[0] = lr;
        adam_out[1] = b.alpha(lr);
        adam_out[2] = (float)b.t;
      }
    }
  }
  const FlatWalk walk(sseg, segs, nseg, true);   // the table, the rate and k1, k2
  walk.run(w, n, bf, LambApply<NT>{m, v, wd_seg, trust, c, rate_s[0], rate_s[1], rate_s[2],
                                   decoupled != 0});   // (the mode: uniform over the launch)
}

void lamb_update_pack(float* master, const float* m, const float* v, long n,
                      const LrSchedule& s, const long long* gstep, const long long* start_step,
                      float beta1, float beta2, float epsilon, int decoupled,
                      const ParamSeg* segs, int nseg, const float* wd_seg, const float* trust,
                      bf16* bf, float* lr_out, float* adam_out, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL((lamb_pack_kernel<LAMB_NT>), dim3(flat_blocks(n)), dim3(256), 0, st, master,
                     m, v, n, s, gstep, start_step, adam_coef(beta1, beta2, epsilon), decoupled,
                     segs, nseg, wd_seg, trust, bf, lr_out, adam_out);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
