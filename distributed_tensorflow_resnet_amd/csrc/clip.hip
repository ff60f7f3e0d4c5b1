// Global gradient-norm clipping (tf.clip_by_global_norm) on the device: with g^ the
// complete mean gradient (reduced, all-reduced, the s2d stem's mapped back; before decay)
//   norm  = sqrt(sum over all trainables of g^^2)
//   scale = 1 if norm <= c,  c / norm if norm > c,  NaN if the sum is not finite
//   acc   = momentum * acc + scale * g^ + wd * w,  w -= lr * acc   (sgd: without acc)
// The gradient buffer is not rescaled, and the decay term is not clipped (TF, whose cost
// holds the decay, would clip g^ + wd * w; LARS's g^ makes the same choice).  Three
// launches over the flat fp32 gradient:
//   grad_sqnorm   one workgroup per CLIP_CHUNK elements: its sum of squares into
//                 part[chunk].  The base is 16-byte aligned and the chunk a multiple of 4,
//                 so only the last chunk has a ragged tail; nothing at or past n is read.
//                 No float atomics and a fixed summation order: bit-reproducible;
//   clip_scale    one wave: the partials added in chunk order, norm and scale into the
//                 two-float slot {norm, scale};
//   sgd_clip_pack sgd_pack's update and HWIO re-pack with the gradient scaled by slot[1]
//                 in place of the host grad_scale; ohwi_pack follows as after sgd_pack.
// optim_device.h has the fp64 reduction of a workgroup (block_sum_f64) and sgd_pack_body, the
// SGD step over the flat walk; clip_scale keeps its own loop over the partials, which
// prefetches (one sum per chunk, thousands of chunks in one wave).
// c = inf measures only: every finite norm is <= inf, so the scale is exactly 1.
// Accumulation widths: a thread adds at most 17 squares in fp32 (4 float4s and one tail
// scalar; lars_norms' bound of 18 covers it); from there on everything is fp64 -- the wave
// shuffles, the four waves, the chunks, the square root and the quotient, each rounded to
// fp32 once.  With u = 2^-24: a thread's sum is within 18 u of exact (one rounding per
// square, at most 17 for the additions, all terms non-negative), the fp64 part adds less
// than 2^-40 relative, so norm is within ~9 u (1 + O(u)) + u for its rounding and scale
// within ~10 u of the exact values (tests/clip_oracle.py derives the bounds the tests use,
// with room).  A square overflows fp32 beyond |g| ~ 1.8e19: such a step reports NaN.
#include "optim_device.h"

namespace dtr {

// (no head and a fixed alignment: its own three lines in place of chunk_span)
__global__ void __launch_bounds__(256)
grad_sqnorm_kernel(const float* __restrict__ g, long long n, double* __restrict__ part) {
  const int tid = threadIdx.x;
  const long long start = (long long)blockIdx.x * CLIP_CHUNK;   // a multiple of 4: aligned
  const long long rest = n - start;                             // > 0 (grid = ceil(n / chunk))
  const int cnt = (int)(rest < CLIP_CHUNK ? rest : (long long)CLIP_CHUNK);
  const int nvec = cnt >> 2;                     // whole float4s, <= 4 * 256
  const long long tail0 = start + 4ll * nvec;
  const int tail = cnt - 4 * nvec;               // < 4, non-zero in the last chunk only
  f32x4 a[4];                                    // 4 loads in flight, then the adds
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = tid + j * 256;
    a[j] = f32x4{0.f, 0.f, 0.f, 0.f};            // (adding the zeros is exact)
    if (k < nvec) a[j] = *reinterpret_cast<const f32x4*>(g + start + 4ll * k);
  }
  float t = 0.f;
  if (tid < tail) t = g[tail0 + tid];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s += a[j][i] * a[j][i];
  }
  s += t * t;
  block_sum_f64<1>({s}, part);
}

int clip_chunks(long long n) { return n <= 0 ? 0 : (int)((n + CLIP_CHUNK - 1) / CLIP_CHUNK); }

void grad_sqnorm(const float* grad, long long n, double* part, hipStream_t st) {
  const int nblocks = clip_chunks(n);
  if (nblocks <= 0) return;
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, grad, n, part);
  DTR_CHECK_LAUNCH();
}

__global__ void __launch_bounds__(64)
clip_scale_kernel(const double* __restrict__ part, int nchunks, float c, float* __restrict__ out) {
  __shared__ double sh[64];
  const int lane = threadIdx.x;
  double ss = 0.0;
  // 64 partials at a time through LDS (coalesced loads), added by one lane in chunk order;
  // the next 64 are loaded while these are added (6238 chunks for ImageNet ResNet-50)
  double nxt = lane < nchunks ? part[lane] : 0.0;
  for (int c0 = 0; c0 < nchunks; c0 += 64) {
    sh[lane] = nxt;
    const int n1 = c0 + 64 + lane;
    nxt = n1 < nchunks ? part[n1] : 0.0;
    __syncthreads();
    if (lane == 0) {
      const int m = min(64, nchunks - c0);
      for (int j = 0; j < m; ++j) ss += sh[j];
    }
    __syncthreads();
  }
  if (lane == 0) {
    const double norm = sqrt(ss);                // NaN / inf of a blown-up step stay visible
    double scale = 1.0;
    if (!__builtin_isfinite(ss)) scale = __builtin_nan("");
    else if (norm > (double)c) scale = (double)c / norm;
    out[0] = (float)norm;
    out[1] = (float)scale;
  }
}

void clip_scale(const double* part, int nchunks, float c, float* out, hipStream_t st) {
  hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(64), 0, st, part, nchunks, c, out);
  DTR_CHECK_LAUNCH();
}

__global__ void __launch_bounds__(256)
sgd_clip_pack_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ mom,
                     long n, LrSchedule sched, const long long* __restrict__ gstep,
                     float momentum, float wd, const float* __restrict__ clip, int use_momentum,
                     const ParamSeg* __restrict__ segs, int nseg, bf16* __restrict__ bf,
                     float* __restrict__ lr_out) {
  __shared__ ParamSeg sseg[SEG_LDS_MAX];
  sgd_pack_body<false, true>(sseg, w, g, mom, n, sched, gstep, momentum, wd, 1.f, use_momentum,
                             segs, nseg, nullptr, bf, lr_out, 1, clip);
}

void sgd_clip_update_pack(float* master, const float* grad, float* mom, long n,
                          const LrSchedule& s, const long long* gstep, float momentum, float wd,
                          const float* clip, int use_momentum, const ParamSeg* segs, int nseg,
                          bf16* bf, float* lr_out, hipStream_t st) {
  hipLaunchKernelGGL(sgd_clip_pack_kernel, dim3(flat_blocks(n)), dim3(256), 0, st, master, grad,
                     mom, n, s, gstep, momentum, wd, clip, use_momentum, segs, nseg, bf, lr_out);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
