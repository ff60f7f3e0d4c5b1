// AugMix (Hendrycks et al. 2020) on the step's uint8 batch buffer: one launch IN FRONT of the
// input launch, in RandAugment's place (one policy at a time), with RandAugment's integer ops
// (randaug_device.h).  data/augmix.py is the specification this must equal bit for bit.
//
// Per image: `width` chains, each starting from the original o and 1..3 ops long, give c_i;
//   acc = sum_i w_i c_i                  w_i Q8, sum w_i == 256, so acc <= 65280 (16 bits)
//   out = ((65536 - m) (o << 8) + m acc + 2^23) >> 24      m Q16 in 0..65536; below 2^32
// The weights and m come from one entry of a host-made table (Dirichlet / Beta samples in
// fixed point: no sampler, no float here).  The draw is keyed (seed ^ salt, global_step, n);
// sub-hashes give the table entry, each chain's depth and each (chain, slot)'s op and sign.
// Every operand of the draw is uniform over the workgroup.
//
// One workgroup per image, two instantiations:
//   CHW 32x32 (the CIFAR records): 256 threads.  LDS holds the original and two working
//     copies (3 x 3 KB); a chain re-stages the original LDS to LDS.  The accumulator never
//     touches memory: thread t owns bytes 12 t .. 12 t + 11 of the image and keeps their 12 Q8
//     sums in registers across the chains.  The final blend reads the original's 12 bytes from
//     LDS; four neighbouring lanes trade their 3 + 3 + 3 + 3 result words with cross-lane
//     reads into three 16-B stores.
//   HWC H x W (the ImageNet crops): 1024 threads, one copy in dynamic LDS (150,528 B of 160 KB
//     at 224x224: no room for the original beside it, let alone an accumulator).  Each chain
//     re-stages the original from the input buffer with 16-B loads; the moving ops alternate
//     between LDS and the image's slot of the OUTPUT buffer, which is free until the final
//     write.  The Q8 accumulator is a uint16 workspace in global memory, 32 B per 16 image
//     bytes: the first chain stores it without reading it, the last chain does not store it
//     but blends with the original (16-B load) and writes the output.  Staging, accumulate
//     and final write all give vector v to thread v % 1024, so a thread only ever re-reads
//     what it wrote itself: a chain that ended in the output slot is accumulated by the
//     thread that then overwrites that vector, and by every thread before the next chain's
//     first barrier, behind which the slot is written again.
// No float, no global atomics, no inline assembly, plain C++ stores.
//
// Three-view fan-out for the Jensen-Shannon loss (AmFan, the `_fan` kernels; data/augmix.py
// augmix_fanout): B stored images become 3B outputs.  Workgroup p reads source image p % B
// wherever the kernels above read "the original".  p < B is the clean view: a straight 16-B
// copy, its log rows -1.  p >= B runs the chains keyed on the OUTPUT position p (seed,
// global_step, p), so one image's two views differ and a resumed run continues the sequence;
// its thread 0 also writes labels[p] = labels[p % B] (slots < B are only read).  The HWC
// workspace and the output slot stay keyed on p.  Without AmFan the launch is the kernel, the
// arguments and the bits it was.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"
#include "randaug_device.h"

namespace dtr {

namespace {

constexpr unsigned long long AM_SALT = 0x4155474D495821ull;   // "AUGMIX!"
constexpr int AM_MAX_DEPTH = 3, AM_LOG_ROW = (1 + AM_MAX_DEPTH) * 2;

__device__ __forceinline__ unsigned am_blend(unsigned o, unsigned acc, unsigned m) {
  return ((65536u - m) * (o << 8) + m * acc + (1u << 23)) >> 24;
}

// image n's hash, its table entry, chain i's depth and slot k's (op, sign); thread 0 logs
struct AmDraw {
  unsigned long long h, hc;
  int* row;   // chain i's log row, or null
  __device__ __forceinline__ AmDraw(unsigned long long seed, const long long* gstep, int n) {
    const unsigned long long step = gstep ? (unsigned long long)*gstep : 0ull;
    h = ra_splitmix(ra_splitmix(seed ^ AM_SALT) ^
                    ra_splitmix(step * 0x100000001B3ull + (unsigned long long)n));
    hc = 0;
    row = nullptr;
  }
  __device__ __forceinline__ int entry(const AugMix& am) const {
    return (int)((unsigned)h % (unsigned)am.mix_len);
  }
  __device__ __forceinline__ int chain(int i, int n, const AugMix& am) {
    hc = ra_splitmix(h ^ ((unsigned long long)(i + 1) << 8));
    const int depth = am.depth > 0 ? am.depth : 1 + (int)((unsigned)hc % 3u);
    row = am.log && threadIdx.x == 0 ? am.log + ((long)n * am.width + i) * AM_LOG_ROW : nullptr;
    if (row) {
      row[0] = depth;
      row[1] = entry(am);
#pragma unroll
      for (int k = 2 * depth + 2; k < AM_LOG_ROW; ++k) row[k] = -1;
    }
    return depth;
  }
  __device__ __forceinline__ void slot(int k, const AugMix& am, int& op, int& sign) const {
    const unsigned long long hk = ra_splitmix(hc ^ (unsigned long long)(k + 1));
    const unsigned idx = (unsigned)hk % (unsigned)am.op_len;
    op = (int)((am.op_nibbles >> (4 * idx)) & 15ull);
    sign = (int)((hk >> 32) & 1ull);
    if (row) {
      row[2 + 2 * k] = op;
      row[3 + 2 * k] = sign;
    }
  }
};

struct AmFan {
  int B;         // source images; the grid has 3 B workgroups
  int* labels;   // [3 B], the first B given
};

// the clean view's log rows, and the views' labels (workgroup-uniform p)
__device__ __forceinline__ void am_fan_side(const AmFan& fan, const AugMix& am, int p) {
  if (p < fan.B) {
    if (am.log && threadIdx.x < am.width * AM_LOG_ROW)
      am.log[(long)p * am.width * AM_LOG_ROW + threadIdx.x] = -1;
  } else if (threadIdx.x == 0 && fan.labels) {
    fan.labels[p] = fan.labels[p % fan.B];
  }
}

template <bool FAN>
__device__ __forceinline__ void
augmix_chw_body(const uint8_t* __restrict__ in, uint8_t* out, unsigned long long seed,
                const long long* __restrict__ gstep, const AugMix& am, const AmFan& fan) {
  constexpr int H = 32, W = 32, NV = 3 * H * W / 16;
  __shared__ uint4 orig[NV];
  __shared__ uint4 buf[2][NV];
  __shared__ RaScratch s;
  const int n = blockIdx.x, tid = threadIdx.x;
  const int src = FAN ? n % fan.B : n;   // the stored image this output comes from
  if (FAN) {
    am_fan_side(fan, am, n);
    if (n < fan.B) {   // the clean view (workgroup-uniform)
      if (tid < NV)
        reinterpret_cast<uint4*>(out)[(long)n * NV + tid] =
            reinterpret_cast<const uint4*>(in)[(long)src * NV + tid];
      return;
    }
  }
  if (tid < NV) orig[tid] = reinterpret_cast<const uint4*>(in)[(long)src * NV + tid];
  AmDraw draw(seed, gstep, n);
  const int* e = am.mix + (long)draw.entry(am) * (am.width + 1);
  const unsigned m = (unsigned)e[am.width];
  unsigned acc[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) acc[j] = 0u;
#pragma unroll 1
  for (int i = 0; i < am.width; ++i) {
    if (tid < NV) buf[0][tid] = orig[tid];   // thread tid's own vector of the original
    __syncthreads();
    const int depth = draw.chain(i, n, am);
    int cur = 0;
#pragma unroll 1
    for (int k = 0; k < depth; ++k) {
      int op, sign;
      draw.slot(k, am, op, sign);
      if (ra_op<RaCHW, 256>(op, sign, reinterpret_cast<uint8_t*>(buf[cur]),
                            reinterpret_cast<uint8_t*>(buf[cur ^ 1]), H, W, s, am.tables))
        cur ^= 1;
    }
    const unsigned* c = reinterpret_cast<const unsigned*>(buf[cur]) + 3 * tid;
    const unsigned w = (unsigned)e[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const unsigned q = c[j];
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[4 * j + b] += w * ((q >> (8 * b)) & 255u);
    }
    __syncthreads();   // the next chain's staging overwrites buf[0]
  }
  const unsigned* o = reinterpret_cast<const unsigned*>(orig) + 3 * tid;
  unsigned r[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const unsigned q = o[j];
    r[j] = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      r[j] |= am_blend((q >> (8 * b)) & 255u, acc[4 * j + b], m) << (8 * b);
  }
  // lanes 4 g .. 4 g + 3 hold words 12 g .. 12 g + 11 of the image, three each; lane 4 g + j
  // (j < 3) collects words 4 j .. 4 j + 3 of those and stores them as vector 3 g + j
  const int lane = tid & 63, base = lane & ~3, j4 = (lane & 3) * 4;
  unsigned v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int d = min(j4 + q, 11), src = base + d / 3, loc = d % 3;
    const unsigned a0 = __shfl(r[0], src, 64), a1 = __shfl(r[1], src, 64),
                   a2 = __shfl(r[2], src, 64);
    v[q] = loc == 0 ? a0 : loc == 1 ? a1 : a2;
  }
  if ((lane & 3) < 3)
    reinterpret_cast<uint4*>(out)[(long)n * NV + (tid >> 2) * 3 + (lane & 3)] =
        make_uint4(v[0], v[1], v[2], v[3]);
}

__global__ void __launch_bounds__(256)
augmix_chw_kernel(const uint8_t* __restrict__ in, uint8_t* out, unsigned long long seed,
                  const long long* __restrict__ gstep, AugMix am) {
  augmix_chw_body<false>(in, out, seed, gstep, am, AmFan{});
}
__global__ void __launch_bounds__(256)
augmix_chw_fan_kernel(const uint8_t* __restrict__ in, uint8_t* out, unsigned long long seed,
                      const long long* __restrict__ gstep, AugMix am, AmFan fan) {
  augmix_chw_body<true>(in, out, seed, gstep, am, fan);
}

extern __shared__ uint4 am_dyn[];   // RaScratch, then the image

template <bool FAN>
__device__ __forceinline__ void
augmix_hwc_body(const uint8_t* __restrict__ in, uint8_t* out, int H, int W,
                unsigned long long seed, const long long* __restrict__ gstep, const AugMix& am,
                const AmFan& fan) {
  RaScratch& s = *reinterpret_cast<RaScratch*>(am_dyn);
  uint8_t* lds = reinterpret_cast<uint8_t*>(am_dyn) + sizeof(RaScratch);
  const int n = blockIdx.x, tid = threadIdx.x;
  const int nvec = 3 * H * W / 16;
  // the original: the stored image this output comes from (re-staged by every chain)
  const uint4* gin = reinterpret_cast<const uint4*>(in) + (long)(FAN ? n % fan.B : n) * nvec;
  uint8_t* g = out + (long)n * nvec * 16;   // this image's slot of the output: the other home
  if (FAN) {
    am_fan_side(fan, am, n);
    if (n < fan.B) {   // the clean view (workgroup-uniform)
      for (int v = tid; v < nvec; v += 1024) reinterpret_cast<uint4*>(g)[v] = gin[v];
      return;
    }
  }
  // 16 uint16 sums per image vector (null at width 1, where nothing is carried)
  uint4* ws = am.acc ? reinterpret_cast<uint4*>(am.acc + (long)n * nvec * 16) : nullptr;
  AmDraw draw(seed, gstep, n);
  const int* e = am.mix + (long)draw.entry(am) * (am.width + 1);
  const unsigned m = (unsigned)e[am.width];
#pragma unroll 1
  for (int i = 0; i < am.width; ++i) {
    for (int v = tid; v < nvec; v += 1024) reinterpret_cast<uint4*>(lds)[v] = gin[v];
    __syncthreads();
    const int depth = draw.chain(i, n, am);
    bool in_lds = true;
#pragma unroll 1
    for (int k = 0; k < depth; ++k) {
      int op, sign;
      draw.slot(k, am, op, sign);
      const bool moved = in_lds ? ra_op<RaHWC, 1024>(op, sign, lds, g, H, W, s, am.tables)
                                : ra_op<RaHWC, 1024>(op, sign, g, lds, H, W, s, am.tables);
      if (moved) in_lds = !in_lds;
    }
    const uint4* src = reinterpret_cast<const uint4*>(in_lds ? lds : g);
    const unsigned w = (unsigned)e[i];
    const bool first = i == 0, last = i == am.width - 1;
    for (int v = tid; v < nvec; v += 1024) {
      const uint4 q = src[v];
      const unsigned c[4] = {q.x, q.y, q.z, q.w};
      unsigned a[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};   // two uint16 sums per word
      if (!first) {
        const uint4 lo = ws[2 * v], hi = ws[2 * v + 1];
        a[0] = lo.x, a[1] = lo.y, a[2] = lo.z, a[3] = lo.w;
        a[4] = hi.x, a[5] = hi.y, a[6] = hi.z, a[7] = hi.w;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {   // bytes 2 j and 2 j + 1 of the vector; neither sum
        const unsigned two = c[j >> 1] >> (16 * (j & 1));   // passes 65280, so no carry
        a[j] += w * (two & 255u) + ((w * ((two >> 8) & 255u)) << 16);
      }
      if (!last) {
        ws[2 * v] = make_uint4(a[0], a[1], a[2], a[3]);
        ws[2 * v + 1] = make_uint4(a[4], a[5], a[6], a[7]);
      } else {
        const uint4 oq = gin[v];
        const unsigned o[4] = {oq.x, oq.y, oq.z, oq.w};
        unsigned r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          r[j] = 0u;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const unsigned sum = (a[2 * j + (b >> 1)] >> (16 * (b & 1))) & 65535u;
            r[j] |= am_blend((o[j] >> (8 * b)) & 255u, sum, m) << (8 * b);
          }
        }
        reinterpret_cast<uint4*>(g)[v] = make_uint4(r[0], r[1], r[2], r[3]);
      }
    }
  }
}

__global__ void __launch_bounds__(1024)
augmix_hwc_kernel(const uint8_t* __restrict__ in, uint8_t* out, int H, int W,
                  unsigned long long seed, const long long* __restrict__ gstep, AugMix am) {
  augmix_hwc_body<false>(in, out, H, W, seed, gstep, am, AmFan{});
}
__global__ void __launch_bounds__(1024)
augmix_hwc_fan_kernel(const uint8_t* __restrict__ in, uint8_t* out, int H, int W,
                      unsigned long long seed, const long long* __restrict__ gstep, AugMix am,
                      AmFan fan) {
  augmix_hwc_body<true>(in, out, H, W, seed, gstep, am, fan);
}

}  // namespace

void augmix_check(const void* in, const void* out, int N, int H, int W, int hwc,
                  const AugMix& am, int fan_B) {
  if (fan_B < 0 || (fan_B > 0 && N != 3 * fan_B))
    throw std::invalid_argument("augmix: the three-view fan-out writes N == 3 * fan_B outputs");
  if (!in || !out || !am.tables || !am.mix)
    throw std::invalid_argument("augmix: null buffer or table");
  if (reinterpret_cast<uintptr_t>(in) % 16 || reinterpret_cast<uintptr_t>(out) % 16)
    throw std::invalid_argument("augmix: both batch buffers must be 16-byte aligned");
  // the output slot is a chain's working home while the input is still being re-staged
  const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
  const uintptr_t bytes = (uintptr_t)(N > 0 ? N : 0) * 3u * (uintptr_t)(H > 0 ? H : 0) *
                          (uintptr_t)(W > 0 ? W : 0);
  const uintptr_t in_bytes = fan_B > 0 ? bytes / 3u : bytes;   // the fan-out reads B images
  if (a == b || (a < b + bytes && b < a + in_bytes))
    throw std::invalid_argument("augmix: needs an output buffer of its own, not overlapping "
                                "the input");
  if (am.width < 1 || am.width > 4) throw std::invalid_argument("augmix: width must be in 1..4");
  if (am.depth != -1 && (am.depth < 1 || am.depth > AM_MAX_DEPTH))
    throw std::invalid_argument("augmix: depth must be -1 (drawn) or in 1..3");
  if (am.op_len < 1 || am.op_len > 16)
    throw std::invalid_argument("augmix: the op table needs 1..16 entries");
  for (int i = 0; i < am.op_len; ++i)
    if (((am.op_nibbles >> (4 * i)) & 15ull) > 13ull)
      throw std::invalid_argument("augmix: op ids must be in 0..13");
  if (am.table_len != RA_TABLE_LEN)
    throw std::invalid_argument("augmix: the parameter table has 64 entries (randaug_tables)");
  if (am.mix_len < 1 || am.mix_len > (1 << 24))
    throw std::invalid_argument("augmix: the mixing table needs 1..2^24 entries");
  if (N < 1 || N > (1 << 20)) throw std::invalid_argument("augmix: need 1 <= N <= 2^20");
  if (!hwc) {
    if (H != 32 || W != 32) throw std::invalid_argument("augmix: the CHW kernel is for 32x32");
    return;
  }
  if (H < 1 || W < 1 || H >= 4096 || W >= 4096 || (3L * H * W) % 16)
    throw std::invalid_argument("augmix: HWC needs 1 <= H, W < 4096 and 3 * H * W % 16 == 0");
  if (3L * H * W + (long)sizeof(RaScratch) > RA_LDS_MAX)
    throw std::invalid_argument("augmix: the image and its scratch do not fit 160 KB of LDS");
  if (am.width > 1 && (!am.acc || reinterpret_cast<uintptr_t>(am.acc) % 16))
    throw std::invalid_argument("augmix: HWC with more than one chain needs a 16-byte aligned "
                                "uint16 workspace [N][3 H W]");
  // above the 64 KB a workgroup gets by default: asked for once per process, here, so that
  // it has happened when the op is made and no launch (or graph capture) has to
  // (each kernel when it is first asked for: a run without the fan-out never touches its kernel)
  const auto lds_attr = [](const void* kernel) {
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RA_LDS_MAX);
  };
  hipError_t attr;
  if (fan_B > 0) {
    static const hipError_t fan = lds_attr(reinterpret_cast<const void*>(augmix_hwc_fan_kernel));
    attr = fan;
  } else {
    static const hipError_t plain = lds_attr(reinterpret_cast<const void*>(augmix_hwc_kernel));
    attr = plain;
  }
  if (attr != hipSuccess)
    throw std::runtime_error(std::string("augmix: cannot get 160 KB of LDS: ") +
                             hipGetErrorString(attr));
}

void augmix(const uint8_t* in, uint8_t* out, int N, int H, int W, int hwc,
            unsigned long long seed, const long long* gstep, const AugMix& am, hipStream_t s,
            int fan_B, int* labels) {
  augmix_check(in, out, N, H, W, hwc, am, fan_B);
  const AmFan fan{fan_B, labels};
  const size_t lds = sizeof(RaScratch) + 3 * (size_t)H * W;
  if (!hwc) {
    if (fan_B)
      hipLaunchKernelGGL(augmix_chw_fan_kernel, dim3(N), dim3(256), 0, s, in, out, seed, gstep,
                         am, fan);
    else
      hipLaunchKernelGGL(augmix_chw_kernel, dim3(N), dim3(256), 0, s, in, out, seed, gstep, am);
  } else if (fan_B) {
    hipLaunchKernelGGL(augmix_hwc_fan_kernel, dim3(N), dim3(1024), lds, s, in, out, H, W, seed,
                       gstep, am, fan);
  } else {
    hipLaunchKernelGGL(augmix_hwc_kernel, dim3(N), dim3(1024), lds, s, in, out, H, W, seed,
                       gstep, am);
  }
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
