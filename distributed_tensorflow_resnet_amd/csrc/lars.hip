// LARS (layer-wise adaptive rate scaling; You, Gitman, Ginsburg 2017, in the form of
// tf.contrib.opt.LARSOptimizer): per trainable tensor s,
//   g^    = grad * grad_scale
//   trust = eeta * ||w_s|| / (||g^_s|| + wd * ||w_s|| + epsilon)   (1 for a skipped tensor
//                                                                   or a zero norm)
//   g'    = g^ + wd * w,  accum = momentum * accum + g',  w -= (lr * trust) * accum
// as three launches over the flat fp32 master and gradient:
//   lars_norms   one workgroup per LARS_CHUNK elements of one tensor (host-built chunk
//                table): its two sums of squares into part[chunk].  No float atomics and
//                a fixed summation order, so the norms are bit-reproducible;
//   lars_trust   one wave per tensor: its chunks' partials added in chunk order, the two
//                norms and the trust ratio;
//   lars_sgd_pack  sgd_pack's update and HWIO re-pack at the rate lr * trust[segment];
//                ohwi_pack follows as after sgd_pack.
// The control flow is optim_device.h's: chunk_span and block_sum_f64 (lars_norms),
// seg_part_sums (lars_trust), sgd_pack_body's SgdStep<LARS> over the FlatWalk (lars_sgd_pack).
// Its own are the squares, the closing formula of the trust ratio and the launchers.
// Accumulation widths: a thread adds at most 18 squares in fp32 (4 float4s of the aligned
// body, one head and one tail scalar); from there on everything is fp64 -- the wave
// shuffles, the four waves, the chunks, the square roots and the ratio, which is rounded
// to fp32 once.  With u = 2^-24: a thread's sum is within 18 u of exact (one rounding
// per square, at most 17 for the additions, all terms non-negative), the fp64 part adds
// less than 2^-40 relative, so ||.|| is within ~9 u (1 + O(u)) and trust within ~19 u of
// the exact ratio (tests/lars_oracle.py derives the bounds the tests use, with room).
#include "optim_device.h"

namespace dtr {

__global__ void __launch_bounds__(256)
lars_norms_kernel(const float* __restrict__ w, const float* __restrict__ g,
                  const ParamSeg* __restrict__ segs, const LarsSeg* __restrict__ lsegs,
                  const int* __restrict__ blk_seg, double* __restrict__ part) {
  const int tid = threadIdx.x;
  const int si = blk_seg[blockIdx.x];
  const ChunkSpan ch = chunk_span(segs[si].offset, segs[si].numel,
                                  (long long)blockIdx.x - lsegs[si].chunk0, LARS_CHUNK);
  float sw = 0.f, sg = 0.f;
  f32x4 a[4], b[4];                               // 8 loads in flight (nvec <= 4 * 256)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = tid + j * 256;
    a[j] = b[j] = f32x4{0.f, 0.f, 0.f, 0.f};      // (adding the zeros is exact)
    if (k < ch.nvec) {
      a[j] = *reinterpret_cast<const f32x4*>(w + ch.body0 + 4ll * k);
      b[j] = *reinterpret_cast<const f32x4*>(g + ch.body0 + 4ll * k);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sw += a[j][i] * a[j][i];
      sg += b[j][i] * b[j][i];
    }
  }
  if (tid < ch.head) {
    const float x = w[ch.start + tid], y = g[ch.start + tid];
    sw += x * x;
    sg += y * y;
  }
  if (tid < ch.tail) {
    const float x = w[ch.tail0 + tid], y = g[ch.tail0 + tid];
    sw += x * x;
    sg += y * y;
  }
  block_sum_f64<2>({sw, sg}, part);
}

void lars_norms(const float* master, const float* grad, const ParamSeg* segs,
                const LarsSeg* lsegs, const int* blk_seg, int nblocks, double* part,
                hipStream_t st) {
  if (nblocks <= 0) return;
  hipLaunchKernelGGL(lars_norms_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, master, grad,
                     segs, lsegs, blk_seg, part);
  DTR_CHECK_LAUNCH();
}

__global__ void __launch_bounds__(64)
lars_trust_kernel(const double* __restrict__ part, const LarsSeg* __restrict__ lsegs, float eeta,
                  float wd, float epsilon, float grad_scale, float* __restrict__ trust,
                  float* __restrict__ wn, float* __restrict__ gn) {
  const int si = blockIdx.x;
  const LarsSeg ls = lsegs[si];
  double sw, sg;
  seg_part_sums(part, ls, sw, sg);
  if (threadIdx.x == 0) {
    const double w_n = sqrt(sw), g_n = fabs((double)grad_scale) * sqrt(sg);
    float t = 1.f;
    if (!ls.skip && w_n > 0.0 && g_n > 0.0)
      t = (float)((double)eeta * w_n / (g_n + (double)wd * w_n + (double)epsilon));
    trust[si] = t;
    wn[si] = (float)w_n;
    gn[si] = (float)g_n;
  }
}

void lars_trust(const double* part, const LarsSeg* lsegs, int nseg, float eeta, float wd,
                float epsilon, float grad_scale, float* trust, float* wn, float* gn,
                hipStream_t st) {
  if (nseg <= 0) return;
  hipLaunchKernelGGL(lars_trust_kernel, dim3((unsigned)nseg), dim3(64), 0, st, part, lsegs, eeta,
                     wd, epsilon, grad_scale, trust, wn, gn);
  DTR_CHECK_LAUNCH();
}

__global__ void __launch_bounds__(256)
lars_sgd_pack_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ mom,
                     long n, LrSchedule sched, const long long* __restrict__ gstep,
                     float momentum, float wd, float grad_scale,
                     const ParamSeg* __restrict__ segs, int nseg,
                     const float* __restrict__ trust, bf16* __restrict__ bf,
                     float* __restrict__ lr_out) {
  __shared__ ParamSeg sseg[SEG_LDS_MAX];
  sgd_pack_body<true>(sseg, w, g, mom, n, sched, gstep, momentum, wd, grad_scale, 1, segs, nseg,
                      trust, bf, lr_out, 1);
}

void lars_update_pack(float* master, const float* grad, float* mom, long n, const LrSchedule& s,
                      const long long* gstep, float momentum, float wd, float grad_scale,
                      const ParamSeg* segs, int nseg, const float* trust, bf16* bf,
                      float* lr_out, hipStream_t st) {
  hipLaunchKernelGGL(lars_sgd_pack_kernel, dim3(flat_blocks(n)), dim3(256), 0, st, master, grad,
                     mom, n, s, gstep, momentum, wd, grad_scale, segs, nseg, trust, bf, lr_out);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
