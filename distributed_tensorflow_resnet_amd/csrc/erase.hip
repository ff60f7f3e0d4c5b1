// Random Erasing (Zhong et al. 2020; zero fill: Cutout, DeVries & Taylor 2017) on the step's
// input buffer: one launch of its own behind the input launch, so it composes with every
// input kernel (unmixed, mixup, CutMix) and none of them changes.
//
// One 256-thread workgroup per image.  The workgroup evaluates its image's draw --
// data/cifar.py erase_draw is the specification this must equal for every input: integers
// only, keyed like the crops with (seed, global_step, n) under a salted and hashed seed, the
// box size read from a host-made table (eh << 16 | ew, erase_table), so no sampler, sqrt or log
// runs here -- and returns at once when the draw is off.  Every operand of the draw is uniform
// over the workgroup; global_step is read from the device word, as the input kernels read it,
// so the launch replays under a captured graph with fresh boxes.
//
// The threads then walk the eh * ew pixels of the box.  A pixel is ONE vector store of the
// whole padded pixel: 16 B in the NHWC layout with 8 channels, 8 B (the pixel's 4-channel
// group) in the space-to-depth stem layout S[y>>1][x>>1][((y&1)*2 + (x&1))*4 + c].  The first
// three channels get the fill (0, or a value of the host-made noise table picked by a hash
// of the placement hash and the element, rounded to bf16 once), every padding channel exactly
// 0.  Nothing outside the box is read or written: no atomics, no LDS, plain C++ vector stores.
// erase_table only makes entries with eh < H and ew < W (torchvision's acceptance test).  The
// draw itself is defined for every box that fits, 1 <= eh <= H and 1 <= ew <= W (a hand-made
// table may hold a full row, column or image: the modulus H - eh + 1 is then 1 and the corner
// 0), here as in erase_draw.  An entry that does not fit counts as "off", so a bad table
// cannot write out of bounds (erase_draw raises for it instead).
#include <stdexcept>

#include "common.h"
#include "kernels.h"

namespace dtr {

namespace {

constexpr unsigned long long ERASE_SALT = 0x455241534521ull;   // "ERASE!"

__device__ __forceinline__ unsigned long long erase_splitmix(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

template <bool S2D>
__global__ void __launch_bounds__(256)
erase_boxes_kernel(bf16* __restrict__ x, int H, int W, unsigned long long seed,
                   const long long* __restrict__ gstep, Erase er) {
  const int n = blockIdx.x, tid = threadIdx.x;
  const unsigned long long step = gstep ? (unsigned long long)*gstep : 0ull;
  const unsigned long long h = erase_splitmix(
      erase_splitmix(seed ^ ERASE_SALT) ^
      erase_splitmix(step * 0x100000001B3ull + (unsigned long long)n));
  int on = (unsigned)(h >> 40) < er.thresh;
  int eh = 0, ew = 0, y0 = 0, x0 = 0;
  unsigned long long h2 = 0;
  if (on) {
    const int e = er.table[(unsigned)h % (unsigned)er.table_len];
    eh = (e >> 16) & 0xFFFF;
    ew = e & 0xFFFF;
    on = eh >= 1 && ew >= 1 && eh <= H && ew <= W;   // entry 0: this image is not erased
    if (on) {
      h2 = erase_splitmix(h ^ ERASE_SALT);
      y0 = (int)((unsigned)h2 % (unsigned)(H - eh + 1));
      x0 = (int)((unsigned)(h2 >> 32) % (unsigned)(W - ew + 1));
    } else {
      eh = ew = 0;
    }
  }
  if (er.log && tid < 5) {
    const int v = tid == 0 ? on : tid == 1 ? y0 : tid == 2 ? x0 : tid == 3 ? eh : ew;
    er.log[n * 5 + tid] = v;
  }
  if (!on) return;
  const int area = eh * ew;
  for (int i = tid; i < area; i += 256) {
    const int dy = i / ew;
    const int y = y0 + dy, xx = x0 + (i - dy * ew);
    bf16 c[3] = {(bf16)0.f, (bf16)0.f, (bf16)0.f};
    if (er.noise) {
      const unsigned long long key = (unsigned long long)(y * W + xx) * 4ull;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        c[k] = (bf16)er.noise[erase_splitmix(h2 ^ (key + k)) % (unsigned long long)er.noise_len];
    }
    if (S2D) {
      const bf16x4 r = {c[0], c[1], c[2], (bf16)0.f};
      const long q = ((long)n * (H >> 1) + (y >> 1)) * (long)(W >> 1) + (xx >> 1);
      *reinterpret_cast<bf16x4*>(x + q * 16 + ((y & 1) * 2 + (xx & 1)) * 4) = r;
    } else {
      bf16x8 r = {};
      r[0] = c[0];
      r[1] = c[1];
      r[2] = c[2];
      *reinterpret_cast<bf16x8*>(x + (((long)n * H + y) * (long)W + xx) * 8) = r;
    }
  }
}

}  // namespace

void erase_boxes_check(const void* x, int N, int H, int W, int Cpad, int s2d, const Erase& er) {
  if (!x || !er.table) throw std::invalid_argument("erase_boxes: null buffer or table");
  if (reinterpret_cast<uintptr_t>(x) % 16)
    throw std::invalid_argument("erase_boxes: the input buffer must be 16-byte aligned");
  if (N < 1 || H < 2 || W < 2 || H >= (1 << 15) || W >= (1 << 15))
    throw std::invalid_argument("erase_boxes: need N >= 1 and 2 <= H, W < 2^15");
  if (Cpad != 8)   // (s2d: the 16-channel rows the Cpad-8 stem operand is packed into)
    throw std::invalid_argument("erase_boxes: only for input buffers with Cpad 8");
  if (s2d && ((H | W) & 1)) throw std::invalid_argument("erase_boxes: s2d needs even H, W");
  if (er.table_len < 1) throw std::invalid_argument("erase_boxes: empty table");
  if (er.thresh > (1u << 24)) throw std::invalid_argument("erase_boxes: thresh must be in [0, 2^24]");
  if (er.noise && er.noise_len < 1) throw std::invalid_argument("erase_boxes: empty noise table");
}

void erase_boxes(bf16* x, int N, int H, int W, int Cpad, int s2d, unsigned long long seed,
                 const long long* gstep, const Erase& er, hipStream_t s) {
  erase_boxes_check(x, N, H, W, Cpad, s2d, er);
  if (s2d)
    hipLaunchKernelGGL(erase_boxes_kernel<true>, dim3(N), dim3(256), 0, s, x, H, W, seed, gstep,
                       er);
  else
    hipLaunchKernelGGL(erase_boxes_kernel<false>, dim3(N), dim3(256), 0, s, x, H, W, seed, gstep,
                       er);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
