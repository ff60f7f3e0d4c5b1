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
//                sums of w^2 and u^2 to part[chunk].  Head / body / tail as lars_norms (scalars
//                up to the first 16-byte boundary, float4s, scalars), the stores included: no
//                workgroup touches an element of a neighbouring tensor.  A thread adds at
//                most 18 squares in fp32; the wave shuffles, the four waves, the chunks, the
//                square roots and the ratio are fp64.  No atomics, a fixed order.
//   lamb_trust   one wave per tensor: its chunks' partials added in chunk order, the two
//                norms and the trust ratio (lars_trust's shape and rule).
//   lamb_update_pack  sgd_update_pack's shape (256 threads, at most 4096 workgroups, four
//                elements per thread and trip, the segment table in LDS): reads w, m', v',
//                forms u again with the same helper and the same k1, k2 -- evaluated again from
//                the same integers, never read from a slot another workgroup writes -- and
//                writes w and the bf16 HWIO copy.  ohwi_pack follows, with its
//                global_step += 1, as after adam_update_pack.
// u is recomputed rather than kept: a scratch buffer would cost the same bytes, and the
// gradient buffer stays untouched (the update launch does not read it at all).
// k1 and k2: one lane per workgroup, in fp64 as adam.hip evaluates alpha (1 - b^t as
// -expm1(t * log b), t a 64-bit integer), each rounded to fp32 once.  Nothing is read by the
// host, so a captured graph replays the step.
// Per element everything is fp32 with floating-point contraction off in the helper: each
// product, sum, square root and quotient is rounded exactly once, and both passes form the
// same bits of u (tests/lamb_oracle.py counts the roundings).  With g = m = v = 0 and no
// decay u = 0 / eps = 0: the tensor's |u| is 0, its trust 1 and w is left bit for bit.
// m' and v' are stored and read back non-temporally, as in adam.hip.
#include "optim_device.h"

namespace dtr {

struct LambCoef {
  float b1, omb1, b2, omb2, eps;
};

constexpr bool LAMB_NT = true;   // non-temporal m / v accesses (profiles/adam.md)

// MOMENTS: m and v are the old moments and are updated from g first (the norm pass);
// otherwise they are m' and v' already (the update pass) and g, s are unused.  Returns u.
template <bool MOMENTS>
__device__ __forceinline__ float lamb_elem(float w, float g, float& m, float& v, float s,
                                           float wd, float k1, float k2, const LambCoef& c,
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

// t = max(1, step - start + 1); k[0] = 1 / (1 - b1^t), k[1] = 1 / (1 - b2^t), fp64 rounded once
__device__ __forceinline__ long long lamb_bias(const long long* gstep, const long long* start,
                                               const LambCoef& c, float* k, double* c12) {
  const long long step = gstep ? *gstep : 0ll;
  long long t = step - (start ? *start : 0ll) + 1;
  if (t < 1) t = 1;
  const double c1 = -expm1((double)t * log((double)c.b1));
  const double c2 = -expm1((double)t * log((double)c.b2));
  k[0] = (float)(1.0 / c1);
  k[1] = (float)(1.0 / c2);
  if (c12) {
    c12[0] = c1;
    c12[1] = c2;
  }
  return t;
}

template <bool NT>
__device__ __forceinline__ f32x4 lamb_ld4(const float* p) {
  if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
  else return *reinterpret_cast<const f32x4*>(p);
}

template <bool NT>
__device__ __forceinline__ void lamb_st4(float* p, f32x4 x) {
  if constexpr (NT) __builtin_nontemporal_store(x, reinterpret_cast<f32x4*>(p));
  else *reinterpret_cast<f32x4*>(p) = x;
}

__device__ __forceinline__ double lamb_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool CLIP, bool NT>
__global__ void __launch_bounds__(256)
lamb_moments_norms_kernel(const float* __restrict__ w, const float* __restrict__ g,
                          float* __restrict__ m, float* __restrict__ v,
                          const long long* __restrict__ gstep,
                          const long long* __restrict__ start_step, LambCoef c, float grad_scale,
                          const float* __restrict__ clip, int decoupled,
                          const ParamSeg* __restrict__ segs, const LarsSeg* __restrict__ lsegs,
                          const int* __restrict__ blk_seg, const float* __restrict__ wd_seg,
                          double* __restrict__ part) {
  __shared__ double red[4][2];
  __shared__ float k_s[2];
  if constexpr (CLIP) grad_scale = clip[1];
  const int tid = threadIdx.x;
  const int si = blk_seg[blockIdx.x];
  const long long off = segs[si].offset, numel = segs[si].numel;
  const long long ch = (long long)blockIdx.x - lsegs[si].chunk0;
  // this chunk: [start, end) inside the segment -- never an element of a neighbour
  const long long start = off + ch * LARS_CHUNK;
  const long long rest = numel - ch * LARS_CHUNK;
  const long long end = start + (rest < LARS_CHUNK ? rest : (long long)LARS_CHUNK);
  // scalars up to the first 16-byte boundary, float4s, scalars after the last whole one
  long long body0 = (start + 3) & ~3ll;
  if (body0 > end) body0 = end;
  const int head = (int)(body0 - start);          // < 4
  const int nvec = (int)((end - body0) >> 2);     // <= LARS_CHUNK / 4 = 4 * 256
  const long long tail0 = body0 + 4ll * nvec;
  const int tail = (int)(end - tail0);            // < 4
  const float wd = wd_seg[si];
  const bool dec = decoupled != 0;                // uniform over the launch
  f32x4 a[4], b[4], mm[4], vv[4];                 // 16 loads in flight
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = tid + j * 256;
    a[j] = b[j] = mm[j] = vv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (k < nvec) {
      a[j] = *reinterpret_cast<const f32x4*>(w + body0 + 4ll * k);
      b[j] = *reinterpret_cast<const f32x4*>(g + body0 + 4ll * k);
      mm[j] = lamb_ld4<NT>(m + body0 + 4ll * k);
      vv[j] = lamb_ld4<NT>(v + body0 + 4ll * k);
    }
  }
  if (tid == 0) lamb_bias(gstep, start_step, c, k_s, nullptr);
  __syncthreads();   // k1, k2
  const float k1 = k_s[0], k2 = k_s[1];
  float sw = 0.f, su = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = tid + j * 256;
    if (k < nvec) {   // (no store outside the body; the zeros of the other slots add nothing)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float mi = mm[j][i], vi = vv[j][i];
        const float u = lamb_elem<true>(a[j][i], b[j][i], mi, vi, grad_scale, wd, k1, k2, c, dec);
        mm[j][i] = mi;
        vv[j][i] = vi;
        sw += a[j][i] * a[j][i];
        su += u * u;
      }
      lamb_st4<NT>(m + body0 + 4ll * k, mm[j]);
      lamb_st4<NT>(v + body0 + 4ll * k, vv[j]);
    }
  }
  if (tid < head) {
    const long long e = start + tid;
    const float x = w[e];
    float mi = m[e], vi = v[e];
    const float u = lamb_elem<true>(x, g[e], mi, vi, grad_scale, wd, k1, k2, c, dec);
    m[e] = mi;
    v[e] = vi;
    sw += x * x;
    su += u * u;
  }
  if (tid < tail) {
    const long long e = tail0 + tid;
    const float x = w[e];
    float mi = m[e], vi = v[e];
    const float u = lamb_elem<true>(x, g[e], mi, vi, grad_scale, wd, k1, k2, c, dec);
    m[e] = mi;
    v[e] = vi;
    sw += x * x;
    su += u * u;
  }
  const double dw = lamb_wave_sum((double)sw), du = lamb_wave_sum((double)su);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = dw;
    red[tid >> 6][1] = du;
  }
  __syncthreads();
  if (tid == 0) {
    part[2 * (long long)blockIdx.x] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    part[2 * (long long)blockIdx.x + 1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
  }
}

static LambCoef lamb_coef(float beta1, float beta2, float epsilon) {
  return LambCoef{beta1, (float)(1.0 - (double)beta1), beta2, (float)(1.0 - (double)beta2),
                  epsilon};
}

void lamb_moments_norms(const float* master, const float* grad, float* m, float* v,
                        const long long* gstep, const long long* start_step, float beta1,
                        float beta2, float epsilon, float grad_scale, const float* clip,
                        int decoupled, const ParamSeg* segs, const LarsSeg* lsegs,
                        const int* blk_seg, int nblocks, const float* wd_seg, double* part,
                        hipStream_t st) {
  if (nblocks <= 0) return;
  const LambCoef c = lamb_coef(beta1, beta2, epsilon);
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
  __shared__ double sh[64][2];
  const int lane = threadIdx.x;
  const int si = blockIdx.x;
  const LarsSeg ls = lsegs[si];
  double sw = 0.0, su = 0.0;
  // 64 partials at a time through LDS (coalesced loads), added by one lane in chunk order
  for (int c0 = 0; c0 < ls.nchunks; c0 += 64) {
    const int c = c0 + lane;
    if (c < ls.nchunks) {
      sh[lane][0] = part[2 * (ls.chunk0 + c)];
      sh[lane][1] = part[2 * (ls.chunk0 + c) + 1];
    }
    __syncthreads();
    if (lane == 0) {
      const int n = min(64, ls.nchunks - c0);
      for (int j = 0; j < n; ++j) {
        sw += sh[j][0];
        su += sh[j][1];
      }
    }
    __syncthreads();
  }
  if (lane == 0) {
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

template <bool NT>
__global__ void __launch_bounds__(256)
lamb_pack_kernel(float* __restrict__ w, const float* __restrict__ m, const float* __restrict__ v,
                 long n, LrSchedule sched, const long long* __restrict__ gstep,
                 const long long* __restrict__ start_step, LambCoef c, int decoupled,
                 const ParamSeg* __restrict__ segs, int nseg, const float* __restrict__ wd_seg,
                 const float* __restrict__ trust, bf16* __restrict__ bf,
                 float* __restrict__ lr_out, float* __restrict__ adam_out) {
  __shared__ ParamSeg sseg[SEG_LDS_MAX];
  __shared__ float rate_s[3];
  if (threadIdx.x == 0) {
    const float lr = lr_at(sched, gstep ? (long)*gstep : 0L);
    double c12[2];
    const long long t = lamb_bias(gstep, start_step, c, rate_s + 1, c12);
    rate_s[0] = lr;
    if (blockIdx.x == 0) {
      if (lr_out) *lr_out = lr;
      if (adam_out) {   // adam_update_pack's slot: {lr, alpha, t}
        adam_out[0] = lr;
        adam_out[1] = (float)((double)lr * sqrt(c12[1]) / c12[0]);
        adam_out[2] = (float)t;
      }
    }
  }
  const ParamSeg* S = segs;
  if (nseg <= SEG_LDS_MAX) {
    for (int i = threadIdx.x; i < nseg; i += blockDim.x) sseg[i] = segs[i];
    S = sseg;
  }
  __syncthreads();   // the table, the rate and k1, k2
  const float lr = rate_s[0], k1 = rate_s[1], k2 = rate_s[2];
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
      const f32x4 mv = lamb_ld4<NT>(m + e0);
      const f32x4 vv = lamb_ld4<NT>(v + e0);
      const float wd = wd_seg[sgi];
      const float rate = lr * trust[sgi];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float mj = mv[j], vj = vv[j];
        const float u = lamb_elem<false>(wv[j], 0.f, mj, vj, 1.f, wd, k1, k2, c, dec);
        wv[j] = lamb_apply(wv[j], rate, u);
      }
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
        float mj = m[e], vj = v[e];
        const float u = lamb_elem<false>(w[e], 0.f, mj, vj, 1.f, wd_seg[sj_i], k1, k2, c, dec);
        const float wj = lamb_apply(w[e], lr * trust[sj_i], u);
        w[e] = wj;
        if (bf) write_hwio(sj, e, wj, bf);
      }
    }
  }
}

void lamb_update_pack(float* master, const float* m, const float* v, long n,
                      const LrSchedule& s, const long long* gstep, const long long* start_step,
                      float beta1, float beta2, float epsilon, int decoupled,
                      const ParamSeg* segs, int nseg, const float* wd_seg, const float* trust,
                      bf16* bf, float* lr_out, float* adam_out, hipStream_t st) {
  if (n <= 0) return;
  long blocks = ((n + 3) / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL((lamb_pack_kernel<LAMB_NT>), dim3((unsigned)blocks), dim3(256), 0, st, master,
                     m, v, n, s, gstep, start_step, lamb_coef(beta1, beta2, epsilon), decoupled,
                     segs, nseg, wd_seg, trust, bf, lr_out, adam_out);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
