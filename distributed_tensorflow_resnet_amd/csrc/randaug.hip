// RandAugment (Cubuk et al. 2020) on the step's uint8 batch buffer: one launch of its own IN
// FRONT of the input launch, which then reads the augmented buffer instead of the uploaded one.
// The ops are defined on 0..255 pixels, so they cannot run behind the standardising input
// launch as Random Erasing does; no input kernel changes.
//
// One workgroup per image, and the image stays on chip for its whole chain of ops.
// data/randaug.py is the specification this must equal for every input, bit for bit: integers
// only -- every real number (sin, cos, 0.3 m / 30, ...) was evaluated on the host into the 64
// int32 of randaug_tables, so no float, trig, sqrt or real division runs here.  The draw is
// per image, keyed like the crops with (seed, global_step, n) under a salt of its own; every
// operand is uniform over the workgroup, so the chain is a loop over num_ops with a switch and
// no divergence.  global_step is read from the device word: a captured graph replays with
// fresh draws.  The allowed op ids travel in the kernel arguments, 4 bits each.
//
// Two instantiations of one op set:
//   CHW 32x32 (the CIFAR records): 256 threads, two 3 KB images in LDS.  Ops that read other
//     positions than the one they write (the five gathers, Sharpness) go from one to the other.
//   HWC H x W (the ImageNet crops): 1024 threads, the image staged once with 16-B loads into
//     dynamic LDS (150,528 B at 224x224 -- no room for a second copy).  The moving ops
//     alternate between LDS and the image's slot of the OUTPUT buffer in global memory: the
//     same workgroup wrote it, so the barrier's wait on its stores orders the read-back.
// Pointwise and LUT ops run in place, wherever the image lives.  At the end the image is
// copied out with 16-B stores if it is still in LDS.
//
// Statistics: a 3x256 uint32 histogram by LDS atomic adds and a 256-bin exclusive prefix sum by
// one wave per channel with cross-lane adds (Equalize); channel min/max (AutoContrast) and the
// grey sum (Contrast) as integer wave reductions plus a small LDS combine -- exact sums, no
// fp32.  Brightness, Contrast, Posterize, Solarize, AutoContrast and Equalize all end as a
// 3x256 byte LUT in LDS applied 16 bytes per thread.  No inline assembly, plain C++ stores.
// The ops themselves are in randaug_device.h, which augmix.hip shares.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"
#include "randaug_device.h"

namespace dtr {

namespace {

constexpr unsigned long long RA_SALT = 0x52414E44415547ull;   // "RANDAUG"

// image n's hash and op slot k's (op, sign); thread 0 logs the pair
struct RaDraw {
  unsigned long long h;
  __device__ __forceinline__ RaDraw(unsigned long long seed, const long long* gstep, int n) {
    const unsigned long long step = gstep ? (unsigned long long)*gstep : 0ull;
    h = ra_splitmix(ra_splitmix(seed ^ RA_SALT) ^
                    ra_splitmix(step * 0x100000001B3ull + (unsigned long long)n));
  }
  __device__ __forceinline__ void slot(int k, int n, const RandAug& ra, int& op, int& sign) {
    const unsigned long long hk = ra_splitmix(h ^ (unsigned long long)(k + 1));
    const unsigned idx = (unsigned)hk % (unsigned)ra.op_len;
    op = (int)((ra.op_nibbles >> (4 * idx)) & 15ull);
    sign = (int)((hk >> 32) & 1ull);
    if (ra.log && threadIdx.x == 0) {
      ra.log[(n * ra.num_ops + k) * 2] = op;
      ra.log[(n * ra.num_ops + k) * 2 + 1] = sign;
    }
  }
};

__global__ void __launch_bounds__(256)
randaug_chw_kernel(const uint8_t* __restrict__ in, uint8_t* out, unsigned long long seed,
                   const long long* __restrict__ gstep, RandAug ra) {
  constexpr int H = 32, W = 32, NV = 3 * H * W / 16;
  __shared__ uint4 buf[2][NV];
  __shared__ RaScratch s;
  const int n = blockIdx.x, tid = threadIdx.x;
  if (tid < NV) buf[0][tid] = reinterpret_cast<const uint4*>(in)[(long)n * NV + tid];
  __syncthreads();
  RaDraw draw(seed, gstep, n);
  int cur = 0;
#pragma unroll 1
  for (int k = 0; k < ra.num_ops; ++k) {
    int op, sign;
    draw.slot(k, n, ra, op, sign);
    if (ra_op<RaCHW, 256>(op, sign, reinterpret_cast<uint8_t*>(buf[cur]),
                          reinterpret_cast<uint8_t*>(buf[cur ^ 1]), H, W, s, ra.tables))
      cur ^= 1;
  }
  if (tid < NV) reinterpret_cast<uint4*>(out)[(long)n * NV + tid] = buf[cur][tid];
}

extern __shared__ uint4 ra_dyn[];   // RaScratch, then the image

__global__ void __launch_bounds__(1024)
randaug_hwc_kernel(const uint8_t* __restrict__ in, uint8_t* out, int H, int W,
                   unsigned long long seed, const long long* __restrict__ gstep, RandAug ra) {
  RaScratch& s = *reinterpret_cast<RaScratch*>(ra_dyn);
  uint8_t* lds = reinterpret_cast<uint8_t*>(ra_dyn) + sizeof(RaScratch);
  const int n = blockIdx.x, tid = threadIdx.x;
  const int nvec = 3 * H * W / 16;
  const uint4* gin = reinterpret_cast<const uint4*>(in) + (long)n * nvec;
  uint8_t* g = out + (long)n * nvec * 16;   // this image's slot of the output: the other home
  for (int i = tid; i < nvec; i += 1024) reinterpret_cast<uint4*>(lds)[i] = gin[i];
  __syncthreads();
  RaDraw draw(seed, gstep, n);
  bool in_lds = true;
#pragma unroll 1
  for (int k = 0; k < ra.num_ops; ++k) {
    int op, sign;
    draw.slot(k, n, ra, op, sign);
    const bool moved = in_lds ? ra_op<RaHWC, 1024>(op, sign, lds, g, H, W, s, ra.tables)
                              : ra_op<RaHWC, 1024>(op, sign, g, lds, H, W, s, ra.tables);
    if (moved) in_lds = !in_lds;
  }
  if (in_lds)
    for (int i = tid; i < nvec; i += 1024)
      reinterpret_cast<uint4*>(g)[i] = reinterpret_cast<const uint4*>(lds)[i];
}

}  // namespace

void randaug_check(const void* in, const void* out, int N, int H, int W, int hwc,
                   const RandAug& ra) {
  if (!in || !out || !ra.tables) throw std::invalid_argument("randaug: null buffer or table");
  if (reinterpret_cast<uintptr_t>(in) % 16 || reinterpret_cast<uintptr_t>(out) % 16)
    throw std::invalid_argument("randaug: both batch buffers must be 16-byte aligned");
  if (in == out) throw std::invalid_argument("randaug: needs an output buffer of its own");
  if (ra.num_ops < 1 || ra.num_ops > 3)
    throw std::invalid_argument("randaug: num_ops must be in 1..3");
  if (ra.op_len < 1 || ra.op_len > 16)
    throw std::invalid_argument("randaug: the op table needs 1..16 entries");
  for (int i = 0; i < ra.op_len; ++i)
    if (((ra.op_nibbles >> (4 * i)) & 15ull) > 13ull)
      throw std::invalid_argument("randaug: op ids must be in 0..13");
  if (ra.table_len != RA_TABLE_LEN)
    throw std::invalid_argument("randaug: the parameter table has 64 entries (randaug_tables)");
  if (N < 1 || N > (1 << 20)) throw std::invalid_argument("randaug: need 1 <= N <= 2^20");
  if (!hwc) {
    if (H != 32 || W != 32) throw std::invalid_argument("randaug: the CHW kernel is for 32x32");
    return;
  }
  if (H < 1 || W < 1 || H >= 4096 || W >= 4096 || (3L * H * W) % 16)
    throw std::invalid_argument("randaug: HWC needs 1 <= H, W < 4096 and 3 * H * W % 16 == 0");
  if (3L * H * W + (long)sizeof(RaScratch) > RA_LDS_MAX)
    throw std::invalid_argument("randaug: the image and its scratch do not fit 160 KB of LDS");
  // above the 64 KB a workgroup gets by default: asked for once per process, here, so that
  // it has happened when the op is made and no launch (or graph capture) has to
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void*>(randaug_hwc_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, RA_LDS_MAX);
  if (attr != hipSuccess)
    throw std::runtime_error(std::string("randaug: cannot get 160 KB of LDS: ") +
                             hipGetErrorString(attr));
}

void randaug(const uint8_t* in, uint8_t* out, int N, int H, int W, int hwc,
             unsigned long long seed, const long long* gstep, const RandAug& ra, hipStream_t s) {
  randaug_check(in, out, N, H, W, hwc, ra);
  if (!hwc) {
    hipLaunchKernelGGL(randaug_chw_kernel, dim3(N), dim3(256), 0, s, in, out, seed, gstep, ra);
  } else {
    const size_t lds = sizeof(RaScratch) + 3 * (size_t)H * W;
    hipLaunchKernelGGL(randaug_hwc_kernel, dim3(N), dim3(1024), lds, s, in, out, H, W, seed,
                       gstep, ra);
  }
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
