// Device code shared by the optimizer kernels (optim.hip, lars.hip): the learning-rate
// schedule, the segment search and the flat SGD-momentum update + HWIO re-pack.
#pragma once
#include "common.h"
#include "kernels.h"
#include "optim.h"

namespace dtr {

// Cosine / polynomial decay (optim.h LrSchedule; the step-0 quirk and the fp32 warm-up are
// lr_at's).  fp64 from the two 64-bit differences on, rounded to fp32 once: the chain's
// relative error is a few 2^-53 (sinpi and the products; the general power as
// exp(power * log q) adds power * |log q| * 2^-53, |log q| < 44 for any 64-bit D), far
// inside an fp32 half-ulp, so the result is the correctly rounded rate except on a
// rounding boundary.  sinpi(q / 2)^2 is 0.5 (1 + cos(pi p)) at p = 1 - q without the
// cancellation at the end of the run; its argument is in (0, 1/2], so no large-argument
// reduction is pulled in.  One lane per workgroup evaluates it, ahead of the update loops'
// loads: inlined it leaves the four optimizer kernels' VGPR counts where they were and
// costs fewer SGPR spills in sgd_tiles than a call does (profiles/lr_schedules.md).
__device__ __forceinline__ float lr_decay_curve(int kind, long long t, long long warm_steps,
                                                long long decay_steps, float peak, float end,
                                                float power) {
  const double q = (double)(decay_steps - t) / (double)(decay_steps - warm_steps);
  double f;
  if (kind == LR_COSINE) {
    const double sn = sinpi(0.5 * q);
    f = sn * sn;
  } else if (power == 1.f) {
    f = q;
  } else if (power == 2.f) {
    f = q * q;
  } else {
    f = exp((double)power * log(q));   // q in (0, 1]
  }
  return (float)((double)end + ((double)peak - (double)end) * f);
}

__device__ __forceinline__ float lr_decay_at(const LrSchedule& s, long step) {
  if (step <= 0) return s.init;
  const long t = step - 1;
  if (t < s.warm_steps) return s.warm_from + (s.warm_to - s.warm_from) * (float)t / (float)s.warm_steps;
  if (t >= s.decay_steps) return s.end;
  return lr_decay_curve(s.kind, t, s.warm_steps, s.decay_steps, s.warm_to, s.end, s.power);
}

__device__ __forceinline__ float lr_piecewise_at(const LrSchedule& s, long step) {
  // The reference's hook feeds the rate computed after the *previous* run:
  // step 0 uses the initial value from begin(); step t>0 uses f(t-1).
  if (step <= 0) return s.init;
  const long t = step - 1;
  if (t < s.warm_steps) return s.warm_from + (s.warm_to - s.warm_from) * (float)t / (float)s.warm_steps;
  for (int i = 0; i < s.nb; ++i)
    if (t < s.bound[i]) return s.val[i];
  return s.val[s.nb];
}

// The rate of `step`: the branch on the kind is uniform over the launch.
__device__ __forceinline__ float lr_at(const LrSchedule& s, long step) {
  return s.kind != LR_PIECEWISE ? lr_decay_at(s, step) : lr_piecewise_at(s, step);
}

constexpr int SEG_LDS_MAX = 640;   // segment tables cached in LDS up to this size (30 KB)

__device__ __forceinline__ int find_seg(const ParamSeg* segs, int nseg, long e) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].offset <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}


// HWIO bf16 copy of element e (contiguous with e: the master IS HWIO order).
__device__ __forceinline__ void write_hwio(const ParamSeg& sg, long e, float w, bf16* bf) {
  if (sg.bf_hwio < 0) return;
  const long local = e - sg.offset;
  if (sg.kpad == sg.K) {
    bf[sg.bf_hwio + local] = (bf16)w;
  } else {
    const long row = local / sg.K, co = local - row * sg.K;
    bf[sg.bf_hwio + row * sg.kpad + co] = (bf16)w;
  }
}

// The update itself: 4 consecutive elements per thread (16-B loads / stores of
// w, grad, momentum; an 8-B store of the HWIO bf16 copy) with the parameter
// segment tracked incrementally per thread (elements only move forward) instead
// of a binary search per element.  The OHWI copy (a transpose) is ohwi_pack's.
// LARS: the rate of an element is lr * trust[its segment] (lars.hip); `sseg` is the
// calling kernel's LDS copy of the segment table (SEG_LDS_MAX entries).
// CLIP: the gradient's scale is read from the device slot clip[1] (clip.hip's clip_scale)
// in place of the host grad_scale.
template <bool LARS, bool CLIP = false>
__device__ __forceinline__ void
sgd_pack_body(ParamSeg* sseg, float* __restrict__ w, const float* __restrict__ g,
              float* __restrict__ mom, long n, const LrSchedule& sched,
              const long long* __restrict__ gstep, float momentum, float wd, float grad_scale,
              int use_momentum, const ParamSeg* __restrict__ segs, int nseg,
              const float* __restrict__ trust, bf16* __restrict__ bf, float* __restrict__ lr_out,
              int update, const float* __restrict__ clip = nullptr) {
  if constexpr (CLIP) grad_scale = clip[1];
  // the segment table in LDS: one coalesced round trip per block instead of a binary
  // search of dependent global loads per thread (~8 for ResNet-50's 161 tensors)
  // a decay schedule's rate (fp64) is evaluated by one lane and rides the table's barrier
  __shared__ float lr_s;
  const bool decay = update && sched.kind != LR_PIECEWISE;   // uniform over the launch
  if (decay && threadIdx.x == 0) lr_s = lr_decay_at(sched, gstep ? (long)*gstep : 0L);
  const ParamSeg* S = segs;
  if (nseg <= SEG_LDS_MAX) {
    for (int i = threadIdx.x; i < nseg; i += blockDim.x) sseg[i] = segs[i];
    __syncthreads();
    S = sseg;
  } else if (decay) {
    __syncthreads();   // (no table to publish: the barrier is the rate's alone)
  }
  const float lr = !update ? 0.f : decay ? lr_s : lr_piecewise_at(sched, gstep ? (long)*gstep : 0L);
  if (update && lr_out && blockIdx.x == 0 && threadIdx.x == 0) *lr_out = lr;
  const long nv = (n + 3) / 4;
  const long stride = (long)gridDim.x * blockDim.x;
  long v = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (v >= nv) return;
  int sgi = find_seg(S, nseg, v * 4);
  for (; v < nv; v += stride) {
    const long e0 = v * 4;
    while (sgi + 1 < nseg && S[sgi + 1].offset <= e0) ++sgi;
    const ParamSeg& sg = S[sgi];
    const bool whole = e0 + 4 <= n && e0 + 4 <= sg.offset + sg.numel;
    if (whole) {
      f32x4 wv = *reinterpret_cast<const f32x4*>(w + e0);
      if (update) {
        float rate = lr;
        if constexpr (LARS) rate = lr * trust[sgi];
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + e0) * grad_scale + wd * wv;
        if (use_momentum) {
          const f32x4 acc = momentum * *reinterpret_cast<const f32x4*>(mom + e0) + gv;
          *reinterpret_cast<f32x4*>(mom + e0) = acc;
          wv -= rate * acc;
        } else {
          wv -= rate * gv;
        }
        *reinterpret_cast<f32x4*>(w + e0) = wv;
      }
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
        float wj = w[e];
        if (update) {
          float rate = lr;
          if constexpr (LARS) rate = lr * trust[sj_i];
          const float gj = g[e] * grad_scale + wd * wj;
          if (use_momentum) {
            const float acc = momentum * mom[e] + gj;
            mom[e] = acc;
            wj -= rate * acc;
          } else {
            wj -= rate * gj;
          }
          w[e] = wj;
        }
        if (bf) write_hwio(sj, e, wj, bf);
      }
    }
  }
}

}  // namespace dtr
