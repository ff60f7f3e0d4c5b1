// Device code shared by the optimizer kernels (optim.hip, lars.hip, clip.hip, adam.hip,
// lamb.hip).  The control flow exists once, here; the files keep their arithmetic:
//   lr_at            the learning-rate schedule;
//   FlatWalk         the flat streaming walk over the master + HWIO re-pack of the *_pack
//                    kernels, over a per-optimizer step (SgdStep here, adam.hip's, lamb.hip's);
//   chunk_span, block_sum_f64   a chunk of one tensor as head / float4 body / tail, and the
//                    fp64 reduction of a workgroup's sums into part[] (the *_norms kernels);
//   seg_part_sums    a tensor's chunk partials added in chunk order (the *_trust kernels);
//   AdamCoef, bias_correction, ld4 / st4, flat_blocks   what adam.hip and lamb.hip share.
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

// ...of the four elements from e0 on, all of segment sg: one 8-byte store where the copy's
// rows are not padded and the four sit on an 8-byte boundary of it.
__device__ __forceinline__ void store_hwio4(const ParamSeg& sg, long e0, const f32x4& wv, bf16* bf) {
  if (sg.bf_hwio < 0) return;
  if (sg.kpad == sg.K && ((e0 - sg.offset) & 3) == 0) {
    bf16x4 h = {(bf16)wv[0], (bf16)wv[1], (bf16)wv[2], (bf16)wv[3]};
    *reinterpret_cast<bf16x4*>(bf + sg.bf_hwio + (e0 - sg.offset)) = h;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) write_hwio(sg, e0 + j, wv[j], bf);
  }
}

// The flat streaming walk of the *_pack kernels: 256 threads, at most 4096 workgroups
// (flat_blocks), 4 consecutive elements per thread and trip -- a 16-byte load and store of w,
// an 8-byte store of the HWIO bf16 copy -- with the parameter segment tracked incrementally
// per thread (elements only move forward) instead of a binary search per element.  The OHWI
// copy (a transpose) is ohwi_pack's.
// The constructor puts the segment table into `sseg`, the kernel's LDS copy (SEG_LDS_MAX
// entries): one coalesced round trip per block instead of a binary search of dependent global
// loads per thread (~8 for ResNet-50's 161 tensors), and its barrier.  What one lane of the
// kernel wrote to LDS before it (a rate) is published by that barrier; `rides` says that there
// is such a value, so a table too long for LDS still gets the barrier.
// run() takes the optimizer's step: step(sgi, e0, f32x4& w) updates w and loads, updates and
// stores whatever else it keeps for the four elements at e0 of segment sgi, step(sgi, e,
// float& w) does so for the one element e.  With step.update == 0 nothing but the copy moves
// (sgd_update_pack's pack-only mode).  The test of it stands here, around the call, not in the
// step: sgd_pack's arithmetic on the scalar path compiles differently otherwise
// (tests/test_optim_bits_gpu.py).
struct FlatWalk {
  const ParamSeg* S;
  int nseg;
  long threads;   // blockDim.x, read once: read again behind the barrier it is a vector load
                  // that every workgroup waits for before its first trip (profiles/optim_walk.md)

  __device__ __forceinline__ FlatWalk(ParamSeg* sseg, const ParamSeg* __restrict__ segs, int nseg_,
                                      bool rides)
      : S(segs), nseg(nseg_), threads(blockDim.x) {
    const bool fits = nseg <= SEG_LDS_MAX;
    if (fits) {
      for (int i = threadIdx.x; i < nseg; i += (int)threads) sseg[i] = segs[i];
      S = sseg;
    }
    if (fits || rides) __syncthreads();   // (no table to publish: the barrier is the rides' alone)
  }

  template <class Step>
  __device__ __forceinline__ void run(float* __restrict__ w, long n, bf16* __restrict__ bf,
                                      const Step& step) const {
    const long nv = (n + 3) / 4;
    const long stride = gridDim.x * threads;
    long v = blockIdx.x * threads + threadIdx.x;
    if (v >= nv) return;
    int sgi = find_seg(S, nseg, v * 4);
    for (; v < nv; v += stride) {
      const long e0 = v * 4;
      while (sgi + 1 < nseg && S[sgi + 1].offset <= e0) ++sgi;
      const ParamSeg& sg = S[sgi];
      const bool whole = e0 + 4 <= n && e0 + 4 <= sg.offset + sg.numel;
      if (whole) {
        f32x4 wv = *reinterpret_cast<const f32x4*>(w + e0);
        if (step.update) {
          step(sgi, e0, wv);
          *reinterpret_cast<f32x4*>(w + e0) = wv;
        }
        if (bf) store_hwio4(sg, e0, wv, bf);
      } else {   // a vector straddling a segment end (e.g. a 10-class bias) or the tail
        for (int j = 0; j < 4 && e0 + j < n; ++j) {
          const long e = e0 + j;
          const int sj = find_seg(S, nseg, e);
          float wj = w[e];
          if (step.update) {
            step(sj, e, wj);
            w[e] = wj;
          }
          if (bf) write_hwio(S[sj], e, wj, bf);
        }
      }
    }
  }
};

// SGD with momentum for V = f32x4 (the four elements at e) or float (the one): 16-byte or
// scalar loads / stores of grad and momentum.  LARS: the rate of an element is
// lr * trust[its segment] (lars.hip).
template <bool LARS>
struct SgdStep {
  const float* __restrict__ g;
  float* __restrict__ mom;
  const float* __restrict__ trust;
  float lr, momentum, wd, grad_scale;
  int use_momentum, update;

  template <class V>
  __device__ __forceinline__ void operator()(int sgi, long e, V& wv) const {
    float rate = lr;
    if constexpr (LARS) rate = lr * trust[sgi];
    const V gv = *reinterpret_cast<const V*>(g + e) * grad_scale + wd * wv;
    if (use_momentum) {
      const V acc = momentum * *reinterpret_cast<const V*>(mom + e) + gv;
      *reinterpret_cast<V*>(mom + e) = acc;
      wv -= rate * acc;
    } else {
      wv -= rate * gv;
    }
  }
};

// The body of sgd_pack, lars_sgd_pack and sgd_clip_pack.  `sseg` is the calling kernel's LDS
// copy of the segment table (SEG_LDS_MAX entries).  CLIP: the gradient's scale is read from
// the device slot clip[1] (clip.hip's clip_scale) in place of the host grad_scale.
template <bool LARS, bool CLIP = false>
__device__ __forceinline__ void
sgd_pack_body(ParamSeg* sseg, float* __restrict__ w, const float* __restrict__ g,
              float* __restrict__ mom, long n, const LrSchedule& sched,
              const long long* __restrict__ gstep, float momentum, float wd, float grad_scale,
              int use_momentum, const ParamSeg* __restrict__ segs, int nseg,
              const float* __restrict__ trust, bf16* __restrict__ bf, float* __restrict__ lr_out,
              int update, const float* __restrict__ clip = nullptr) {
  if constexpr (CLIP) grad_scale = clip[1];
  // a decay schedule's rate (fp64) is evaluated by one lane and rides the table's barrier;
  // the piecewise rate is cheap enough for every thread
  __shared__ float lr_s;
  const bool decay = update && sched.kind != LR_PIECEWISE;   // uniform over the launch
  if (decay && threadIdx.x == 0) lr_s = lr_decay_at(sched, gstep ? (long)*gstep : 0L);
  const FlatWalk walk(sseg, segs, nseg, decay);
  const float lr = !update ? 0.f : decay ? lr_s : lr_piecewise_at(sched, gstep ? (long)*gstep : 0L);
  if (update && lr_out && blockIdx.x == 0 && threadIdx.x == 0) *lr_out = lr;
  walk.run(w, n, bf, SgdStep<LARS>{g, mom, trust, lr, momentum, wd, grad_scale, use_momentum, update});
}

// Chunk c (of `chunk` elements) of the segment [off, off + numel): [start, tail0 + tail) inside
// the segment -- never an element of a neighbour -- as `head` (< 4) scalars up to the first
// 16-byte boundary, `nvec` float4s from body0 on and `tail` (< 4) scalars from tail0 on.
struct ChunkSpan {
  long long start, body0, tail0;
  int head, nvec, tail;
};

__device__ __forceinline__ ChunkSpan chunk_span(long long off, long long numel, long long c,
                                                int chunk) {
  ChunkSpan s;
  s.start = off + c * chunk;
  const long long rest = numel - c * chunk;
  const long long end = s.start + (rest < chunk ? rest : (long long)chunk);
  s.body0 = (s.start + 3) & ~3ll;
  if (s.body0 > end) s.body0 = end;
  s.head = (int)(s.body0 - s.start);
  s.nvec = (int)((end - s.body0) >> 2);
  s.tail0 = s.body0 + 4ll * s.nvec;
  s.tail = (int)(end - s.tail0);
  return s;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The N sums of a 256-thread workgroup into part[N * workgroup + i]: each thread's fp32 sum
// widened, the wave's shuffles and the four waves, left to right, in fp64.  All the wave sums
// come before the first LDS store: with a store in between, the compiler pairs the callers'
// fp32 sums differently and contracts other products into them (lamb_moments_norms' partials
// moved in the last bits; tests/test_optim_bits_gpu.py).
template <int N>
__device__ __forceinline__ void block_sum_f64(const float (&s)[N], double* __restrict__ part) {
  __shared__ double red[4][N];
  const int tid = threadIdx.x;
  double d[N];
#pragma unroll
  for (int i = 0; i < N; ++i) d[i] = wave_sum_f64((double)s[i]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[tid >> 6][i] = d[i];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i)
      part[N * (long long)blockIdx.x + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
  }
}

// One wave per tensor: its chunks' two partials (block_sum_f64<2>'s), 64 at a time through
// LDS (coalesced loads), added by one lane in chunk order.  The sums are lane 0's.
__device__ __forceinline__ void seg_part_sums(const double* __restrict__ part, const LarsSeg& ls,
                                              double& s0, double& s1) {
  __shared__ double sh[64][2];
  const int lane = threadIdx.x;
  s0 = s1 = 0.0;
  for (int c0 = 0; c0 < ls.nchunks; c0 += 64) {
    const int c = c0 + lane;
    if (c < ls.nchunks) {
      sh[lane][0] = part[2 * (ls.chunk0 + c)];
      sh[lane][1] = part[2 * (ls.chunk0 + c) + 1];
    }
    __syncthreads();
    if (lane == 0) {
      const int m = min(64, ls.nchunks - c0);
      for (int j = 0; j < m; ++j) {
        s0 += sh[j][0];
        s1 += sh[j][1];
      }
    }
    __syncthreads();
  }
}

// Adam's coefficients as adam.hip and lamb.hip take them: 1 - b1 and 1 - b2 rounded once from
// fp64 on the host.
struct AdamCoef {
  float b1, omb1, b2, omb2, eps;
};

inline AdamCoef adam_coef(float beta1, float beta2, float epsilon) {
  return AdamCoef{beta1, (float)(1.0 - (double)beta1), beta2, (float)(1.0 - (double)beta2),
                  epsilon};
}

// Bias correction at global step `step`: t = max(1, step - start + 1), c1 = 1 - b1^t and
// c2 = 1 - b2^t as -expm1(t * log b) in fp64 (no cancellation at small t; b = 0 gives exactly 1).
// The rates derived from it are fp64 expressions rounded to fp32 once.
struct BiasCorrection {
  long long t;
  double c1, c2;
  __device__ __forceinline__ float alpha(float lr) const { return (float)((double)lr * sqrt(c2) / c1); }
  __device__ __forceinline__ float k1() const { return (float)(1.0 / c1); }
  __device__ __forceinline__ float k2() const { return (float)(1.0 / c2); }
};

__device__ __forceinline__ BiasCorrection bias_correction(long long step,
                                                          const long long* __restrict__ start,
                                                          const AdamCoef& c) {
  long long t = step - (start ? *start : 0ll) + 1;
  if (t < 1) t = 1;
  return {t, -expm1((double)t * log((double)c.b1)), -expm1((double)t * log((double)c.b2))};
}

// 16-byte accesses; NT: non-temporal, for the moments, which one kernel touches once per step
// (profiles/adam.md).
template <bool NT>
__device__ __forceinline__ f32x4 ld4(const float* p) {
  if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
  else return *reinterpret_cast<const f32x4*>(p);
}

template <bool NT>
__device__ __forceinline__ void st4(float* p, f32x4 x) {
  if constexpr (NT) __builtin_nontemporal_store(x, reinterpret_cast<f32x4*>(p));
  else *reinterpret_cast<f32x4*>(p) = x;
}

// Workgroups of a FlatWalk launch over n elements.
inline unsigned flat_blocks(long n) {
  const long blocks = ((n + 3) / 4 + 255) / 256;
  return (unsigned)(blocks > 4096 ? 4096 : blocks < 1 ? 1 : blocks);
}

}  // namespace dtr
