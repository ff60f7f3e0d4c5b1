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
//   lars_sgd_pack  sgd_pack's update and HWIO re-pack at the rate lr * trust[segment]
//                (optim_device.h); ohwi_pack follows as after sgd_pack.
// Accumulation widths: a thread adds at most 18 squares in fp32 (4 float4s of the aligned
// body, one head and one tail scalar); from there on everything is fp64 -- the wave
// shuffles, the four waves, the chunks, the square roots and the ratio, which is rounded
// to fp32 once.  With u = 2^-24: a thread's sum is within 18 u of exact (one rounding
// per square, at most 17 for the additions, all terms non-negative), the fp64 part adds
// less than 2^-40 relative, so ||.|| is within ~9 u (1 + O(u)) and trust within ~19 u of
// the exact ratio (tests/lars_oracle.py derives the bounds the tests use, with room).
#include "optim_device.h"

namespace dtr {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(256)
lars_norms_kernel(const float* __restrict__ w, const float* __restrict__ g,
                  const ParamSeg* __restrict__ segs, const LarsSeg* __restrict__ lsegs,
                  const int* __restrict__ blk_seg, double* __restrict__ part) {
  __shared__ double red[4][2];
  const int tid = threadIdx.x;
  const int si = blk_seg[blockIdx.x];
  const long long off = segs[si].offset, numel = segs[si].numel;
  const long long c = (long long)blockIdx.x - lsegs[si].chunk0;
  // this chunk: [start, end) inside the segment -- never an element of a neighbour
  const long long start = off + c * LARS_CHUNK;
  const long long rest = numel - c * LARS_CHUNK;
  const long long end = start + (rest < LARS_CHUNK ? rest : (long long)LARS_CHUNK);
  // scalars up to the first 16-byte boundary, float4s, scalars after the last whole one
  long long body0 = (start + 3) & ~3ll;
  if (body0 > end) body0 = end;
  const int head = (int)(body0 - start);          // < 4
  const int nvec = (int)((end - body0) >> 2);     // <= LARS_CHUNK / 4 = 4 * 256
  const long long tail0 = body0 + 4ll * nvec;
  const int tail = (int)(end - tail0);            // < 4
  float sw = 0.f, sg = 0.f;
  f32x4 a[4], b[4];                               // 8 loads in flight
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = tid + j * 256;
    a[j] = b[j] = f32x4{0.f, 0.f, 0.f, 0.f};      // (adding the zeros is exact)
    if (k < nvec) {
      a[j] = *reinterpret_cast<const f32x4*>(w + body0 + 4ll * k);
      b[j] = *reinterpret_cast<const f32x4*>(g + body0 + 4ll * k);
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
  if (tid < head) {
    const float x = w[start + tid], y = g[start + tid];
    sw += x * x;
    sg += y * y;
  }
  if (tid < tail) {
    const float x = w[tail0 + tid], y = g[tail0 + tid];
    sw += x * x;
    sg += y * y;
  }
  const double dw = wave_sum_f64((double)sw), dg = wave_sum_f64((double)sg);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = dw;
    red[tid >> 6][1] = dg;
  }
  __syncthreads();
  if (tid == 0) {
    part[2 * (long long)blockIdx.x] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    part[2 * (long long)blockIdx.x + 1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
  }
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
  __shared__ double sh[64][2];
  const int lane = threadIdx.x;
  const int si = blockIdx.x;
  const LarsSeg ls = lsegs[si];
  double sw = 0.0, sg = 0.0;
  // 64 partials at a time through LDS (coalesced loads), added by one lane in chunk order
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
        sw += sh[j][0];
        sg += sh[j][1];
      }
    }
    __syncthreads();
  }
  if (lane == 0) {
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
  long blocks = ((n + 3) / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(lars_sgd_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, master, grad,
                     mom, n, s, gstep, momentum, wd, grad_scale, segs, nseg, trust, bf, lr_out);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
