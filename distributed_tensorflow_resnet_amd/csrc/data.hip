// On-device input pipeline pieces.
//
// cifar_augment reproduces the reference CIFAR training preprocessing
// (resnet_cifar_main.py:201-216: pad to 40x40, random 32x32 crop, random
// left-right flip, tf.image.per_image_standardization) and the eval path
// (cifar_input.py:71-76: standardization only) on raw CIFAR-binary uint8 images
// ([N][3][32][32], the record layout of resnet_cifar_main.py:173-198), writing
// bf16 NHWC with the channel dim zero-padded to Cpad (the stem conv consumes 8
// channels so every 16-B fragment is one tap).  Crop/flip randomness comes from
// a counter-based hash of (seed, global_step, image) read on the device, so the
// augmentation is part of the captured hipGraph and replays with fresh crops.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"
#include "data.h"

namespace dtr {

__device__ __forceinline__ unsigned long long splitmix(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// ---- mixup (Zhang et al. 2018): x = lam * x_n + (1 - lam) * x_m, m = (n + shift) % N ---
// One draw per step, shared by the rank's batch: data/cifar.py mixup_draw is the
// specification this must equal for every input (integers only; the salted seed keeps it
// off the crop hashes).  lam = table[index], a host-made table of Beta(alpha, alpha) draws
// (mixup_table), so no sampler runs here.  Every operand is uniform over the grid.  The
// arguments are data.h's Mixup; a null table launches the kernels' unmixed instantiation.
struct MixDraw {
  unsigned index, shift;
};

__device__ __forceinline__ unsigned long long mix_hash(unsigned long long seed,
                                                       unsigned long long step) {
  return splitmix(splitmix(seed ^ 0x4D4958555021ull) ^ splitmix(step * 0x100000001B3ull));
}

__device__ __forceinline__ MixDraw mix_draw_of(unsigned long long h, int batch, int table_len) {
  MixDraw d;
  d.index = (unsigned)h % (unsigned)table_len;
  d.shift = batch >= 2 ? 1u + (unsigned)(h >> 32) % (unsigned)(batch - 1) : 0u;
  return d;
}

__device__ __forceinline__ MixDraw mixup_draw(unsigned long long seed, unsigned long long step,
                                              int batch, int table_len) {
  return mix_draw_of(mix_hash(seed, step), batch, table_len);
}

// ---- CutMix (Yun et al. 2019): x = box ? x_m : x_n, one box per step ---------------------
// data/cifar.py cutmix_draw is the specification: the same {index, shift}; a salted rehash of
// the same hash decides, against Mixup::cut_thresh (of 2^24), whether the step pastes or
// blends, and places the box; its size is cut_table[index] (ch << 16 | cw, made on the host
// from a Beta draw, so no sqrt runs here).  lam = (H*W - area) / (H*W), one correctly rounded
// fp32 division (this file is built without fast-math).  In a CutMix step the fp32 table is
// not read.  Every operand is uniform over the grid.
enum { MIX_OFF = 0, MIX_BLEND = 1, MIX_CUT = 2 };   // the input kernels' MIX template argument

struct CutBox {
  int cut, y0, y1, x0, x1;
  __device__ __forceinline__ bool has(int y, int x) const {
    return y >= y0 && y < y1 && x >= x0 && x < x1;
  }
};

// the step's draw with CutMix on: the mode, the box and lam; `log` (one thread of the grid)
// also writes mix_log and cut_log
__device__ __forceinline__ MixDraw cutmix_draw(const Mixup& mx, unsigned long long seed,
                                               unsigned long long step, int batch, int H, int W,
                                               bool log, CutBox& b, float& lam) {
  const unsigned long long h = mix_hash(seed, step);
  const MixDraw d = mix_draw_of(h, batch, mx.table_len);
  const unsigned long long h2 = splitmix(h ^ 0x4355544D4958ull);
  b = CutBox{};
  int area = 0, cy = 0, cx = 0;
  b.cut = (unsigned)(h2 >> 40) < mx.cut_thresh;
  if (b.cut) {
    const int e = mx.cut_table[d.index];
    const int ch2 = ((e >> 16) & 0xFFFF) >> 1, cw2 = (e & 0xFFFF) >> 1;
    cy = (int)(((unsigned)h2 & 0xFFFFu) % (unsigned)H);
    cx = (int)(((unsigned)(h2 >> 16) & 0xFFFFu) % (unsigned)W);
    b.y0 = max(cy - ch2, 0);
    b.y1 = min(cy + ch2, H);
    b.x0 = max(cx - cw2, 0);
    b.x1 = min(cx + cw2, W);
    area = (b.y1 - b.y0) * (b.x1 - b.x0);
    lam = (float)(H * W - area) / (float)(H * W);
  } else {
    lam = mx.table[d.index];
  }
  if (log) {
    if (mx.mix_log) {
      mx.mix_log[0] = (int)d.index;
      mx.mix_log[1] = (int)d.shift;
    }
    if (mx.cut_log) {
      const int v[8] = {b.cut, b.y0, b.y1, b.x0, b.x1, area, cy, cx};
#pragma unroll
      for (int i = 0; i < 8; ++i) mx.cut_log[i] = v[i];
    }
  }
  return d;
}

// One workgroup per image: the 3 KB record is staged in LDS with 16-B loads, every
// thread keeps its 4 output pixels' 3 channels in registers across the
// per-image statistics, and writes each pixel as ONE 16-B NHWC row (3 channels +
// zero padding).  Optionally zeroes a buffer in the same launch (the step's
// BatchNorm accumulators), so the step needs no separate memset.
//
// cifar_augment_image is the body shared by cifar_augment_kernel (record n of a
// batch buffer) and cifar_augment_resident_kernel (a record the workgroup picks
// from the resident split): `src` is the image's 3072-B record, `step` the value
// the crop/flip hash is keyed with.  MIX: the workgroup also stages `src_b`, the record
// of batch position m, standardises it with position m's own crop/flip hash -- the two
// fp32 images are exactly what the unmixed body produces for n and m -- and writes
// bf16(lam * a + (1.f - lam) * b): blended in fp32, rounded once.  MIX == MIX_CUT: the same
// launch with CutMix; in a step with box.cut the pixel is bf16(box.has(y, x) ? b : a), a
// select, so every output pixel is bit for bit the unmixed body's for n or for m.
//
// cifar_crop_stats: the staged record `im` -> this thread's PPT pixels x 3 channels of
// batch position n's crop, the image's mean and 1 / adjusted std.  `red`: 8 floats of
// this call's own.  One barrier inside.
__device__ __forceinline__ void cifar_crop_stats(const uint8_t* im, int n, int pad,
                                                 unsigned long long seed,
                                                 unsigned long long step, int train,
                                                 int* crop_log, float* red, float (&v)[4][3],
                                                 float& mean, float& inv) {
  constexpr int H = 32, W = 32, HW = H * W, CHW = 3 * HW, PPT = HW / 256;
  const int tid = threadIdx.x;
  int oy = pad, ox = pad, flip = 0;
  if (train) {
    const unsigned long long h = splitmix(seed ^ splitmix(step * 0x100000001B3ull + n));
    oy = (int)(h % (2 * pad + 1));
    ox = (int)((h >> 16) % (2 * pad + 1));
    flip = (int)((h >> 32) & 1);
  }
  if (crop_log && tid == 0) {
    crop_log[n * 3 + 0] = oy;
    crop_log[n * 3 + 1] = ox;
    crop_log[n * 3 + 2] = flip;
  }
  // pixel (y,x) of the crop = padded-image pixel (y+oy, x'+ox), x' = flip ? W-1-x : x
  float s = 0.f, q = 0.f;
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int p = tid + k * 256;
    const int y = p / W, x = p - y * W;
    const int xs = flip ? (W - 1 - x) : x;
    const int py = y + oy - pad, px = xs + ox - pad;
    const bool in = py >= 0 && py < H && px >= 0 && px < W;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[k][c] = in ? (float)im[c * HW + py * W + px] : 0.f;
      s += v[k][c];
      q += v[k][c] * v[k][c];
    }
  }
  s = wave_sum(s);
  q = wave_sum(q);
  if ((tid & 63) == 0) {
    red[tid >> 6] = s;
    red[4 + (tid >> 6)] = q;
  }
  __syncthreads();
  const float tot = red[0] + red[1] + red[2] + red[3];
  const float totq = red[4] + red[5] + red[6] + red[7];
  const float nel = (float)CHW;
  mean = tot / nel;
  const float var = fmaxf(totq / nel - mean * mean, 0.f);
  const float adj = fmaxf(sqrtf(var), rsqrtf(nel));
  inv = 1.f / adj;
}

// im / im_b: 3072 B each (im_b only with MIX); red: 8 floats (16 with MIX)
template <int CPAD, int MIX>
__device__ __forceinline__ void cifar_augment_image(const uint8_t* __restrict__ src,
                                                    const uint8_t* __restrict__ src_b,
                                                    bf16* __restrict__ out, int n, int m,
                                                    float lam, const CutBox& box, int pad,
                                                    unsigned long long seed,
                                                    unsigned long long step, int train,
                                                    int* crop_log, uint8_t* im, uint8_t* im_b,
                                                    float* red) {
  constexpr int HW = 32 * 32, CHW = 3 * HW, PPT = HW / 256;
  const int tid = threadIdx.x;
  if (tid < CHW / 16) {
    reinterpret_cast<uint4*>(im)[tid] = reinterpret_cast<const uint4*>(src)[tid];
    if (MIX) reinterpret_cast<uint4*>(im_b)[tid] = reinterpret_cast<const uint4*>(src_b)[tid];
  }
  __syncthreads();
  float v[PPT][3], mean, inv;
  cifar_crop_stats(im, n, pad, seed, step, train, crop_log, red, v, mean, inv);
  float vb[PPT][3], mean_b = 0.f, inv_b = 0.f;
  if (MIX) cifar_crop_stats(im_b, m, pad, seed, step, train, nullptr, red + 8, vb, mean_b, inv_b);
  bf16* o = out + (long)n * HW * CPAD;
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int p = tid + k * 256;
    const bool paste = MIX == MIX_CUT && box.cut && box.has(p >> 5, p & 31);
    bf16x8 r = {};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = (v[k][c] - mean) * inv;
      if (MIX) {
        const float b = (vb[k][c] - mean_b) * inv_b;
        if (MIX == MIX_CUT && box.cut)
          r[c] = (bf16)(paste ? b : a);
        else
          r[c] = (bf16)(lam * a + (1.f - lam) * b);
      } else {
        r[c] = (bf16)a;
      }
    }
    *reinterpret_cast<bf16x8*>(o + (long)p * CPAD) = r;
  }
}

// the step's draw, and batch position n's side outputs (thread 0 of workgroup n)
template <int MIX>
__device__ __forceinline__ MixDraw mix_side_outputs(const Mixup& mx, unsigned long long seed,
                                                    unsigned long long step, int n, int batch,
                                                    float& lam, CutBox& box) {
  if (MIX == MIX_CUT) {   // 32x32: the CIFAR launches
    const MixDraw d =
        cutmix_draw(mx, seed, step, batch, 32, 32, threadIdx.x == 0 && n == 0, box, lam);
    if (threadIdx.x == 0) mx.mix_lam[n] = lam;
    return d;
  }
  const MixDraw d = mixup_draw(seed, step, batch, mx.table_len);
  lam = mx.table[d.index];
  if (threadIdx.x == 0) {
    mx.mix_lam[n] = lam;
    if (mx.mix_log && n == 0) {
      mx.mix_log[0] = (int)d.index;
      mx.mix_log[1] = (int)d.shift;
    }
  }
  return d;
}

// workgroup n of the host-fed launch; im: 3072 B (6144 with MIX), red: 8 floats (16)
template <int CPAD, int MIX>
__device__ __forceinline__ void cifar_augment_wg(const uint8_t* __restrict__ img,
                                                 bf16* __restrict__ out, int pad,
                                                 unsigned long long seed, const long long* gstep,
                                                 int train, int* crop_log, uint4* __restrict__ zero,
                                                 long zero_vec, const Mixup& mx, uint8_t* im,
                                                 float* red) {
  constexpr int CHW = 3 * 32 * 32;
  const int n = blockIdx.x, tid = threadIdx.x;
  for (long i = blockIdx.x * 256L + tid; i < zero_vec; i += (long)gridDim.x * 256)
    zero[i] = make_uint4(0u, 0u, 0u, 0u);
  const unsigned long long step = (train && gstep) ? (unsigned long long)*gstep : 0ull;
  int m = n;
  float lam = 1.f;
  CutBox box = {};
  if (MIX) {
    const MixDraw d = mix_side_outputs<MIX>(mx, seed, step, n, (int)gridDim.x, lam, box);
    m = (int)(((unsigned)n + d.shift) % gridDim.x);
    if (tid == 0) mx.labels_b[n] = mx.labels[m];
  }
  cifar_augment_image<CPAD, MIX>(img + (long)n * CHW, img + (long)m * CHW, out, n, m, lam, box,
                                 pad, seed, step, train, crop_log, im, im + (MIX ? CHW : 0), red);
}

template <int CPAD>
__global__ void __launch_bounds__(256)
cifar_augment_kernel(const uint8_t* __restrict__ img, bf16* __restrict__ out, int pad,
                     unsigned long long seed, const long long* gstep, int train, int* crop_log,
                     uint4* __restrict__ zero, long zero_vec) {
  __shared__ __attribute__((aligned(16))) uint8_t im[3 * 32 * 32];
  __shared__ float red[8];
  cifar_augment_wg<CPAD, MIX_OFF>(img, out, pad, seed, gstep, train, crop_log, zero, zero_vec,
                                  Mixup{}, im, red);
}

// the same launch with mixup (a kernel of its own: the unmixed one keeps its code and budget)
template <int CPAD>
__global__ void __launch_bounds__(256)
cifar_mixup_kernel(const uint8_t* __restrict__ img, bf16* __restrict__ out, int pad,
                   unsigned long long seed, const long long* gstep, int train, int* crop_log,
                   uint4* __restrict__ zero, long zero_vec, Mixup mx) {
  __shared__ __attribute__((aligned(16))) uint8_t im[2 * 3 * 32 * 32];
  __shared__ float red[16];
  cifar_augment_wg<CPAD, MIX_BLEND>(img, out, pad, seed, gstep, train, crop_log, zero, zero_vec,
                                    mx, im, red);
}

// the same launch with mixup and CutMix, switched per step (a kernel of its own again: the
// mixup-only one keeps its code and budget)
template <int CPAD>
__global__ void __launch_bounds__(256)
cifar_cutmix_kernel(const uint8_t* __restrict__ img, bf16* __restrict__ out, int pad,
                    unsigned long long seed, const long long* gstep, int train, int* crop_log,
                    uint4* __restrict__ zero, long zero_vec, Mixup mx) {
  __shared__ __attribute__((aligned(16))) uint8_t im[2 * 3 * 32 * 32];
  __shared__ float red[16];
  cifar_augment_wg<CPAD, MIX_CUT>(img, out, pad, seed, gstep, train, crop_log, zero, zero_vec, mx,
                                  im, red);
}

// ---- device-resident split: the workgroup picks its own record ----------------------
// Batch position n of step `step` reads record resident_record(...) of the split: each
// epoch (S = (records / world) / batch steps, the tail dropped) is one keyed permutation
// of the record indices, cut into disjoint rank shards.  The permutation is a balanced
// 4-round Feistel network over 2*hb bits with cycle walking; data/cifar.py
// resident_index is the specification this must equal for every input.  Unshuffled
// (the evaluator), a single rank also visits the tail batch, whose positions past the
// end read the batch's first record.  Every operand is uniform over the workgroup.
__device__ __forceinline__ unsigned resident_feistel(unsigned long long key, unsigned x, int hb) {
  const unsigned mask = (1u << hb) - 1u;
  unsigned L = x >> hb, R = x & mask;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned F =
        (unsigned)splitmix(key ^ ((unsigned long long)(r + 1) << 40) ^ (unsigned long long)R) & mask;
    const unsigned t = L ^ F;
    L = R;
    R = t;
  }
  return (L << hb) | R;
}

__device__ __forceinline__ int resident_record(unsigned long long step, int n, int batch,
                                               int records, int rank, int world, int shuffle,
                                               unsigned long long key_seed) {
  const unsigned ur = (unsigned)records, ub = (unsigned)batch;
  const unsigned S = (ur / (unsigned)world) / ub;               // host: S >= 1
  const unsigned per_rank = S * ub;
  // unshuffled on one rank: the epoch also has the tail batch
  const unsigned steps = (!shuffle && world == 1) ? (ur + ub - 1u) / ub : S;
  unsigned long long epoch;
  unsigned k;
  if ((step >> 32) == 0) {   // the usual case: one 32-bit division
    const unsigned s32 = (unsigned)step;
    epoch = s32 / steps;
    k = s32 - (unsigned)epoch * steps;
  } else {
    epoch = step / steps;
    k = (unsigned)(step - epoch * steps);
  }
  const unsigned first = (unsigned)rank * per_rank + k * ub;    // the batch's first position
  unsigned p = first + (unsigned)n;
  if (p >= ur) p = first < ur ? first : 0u;                     // tail batch (unshuffled)
  if (!shuffle) return (int)p;
  const unsigned r1 = ur - 1u;
  const int bits = r1 ? 32 - __builtin_clz(r1) : 0;
  const int hb = bits > 1 ? (bits + 1) >> 1 : 1;
  const unsigned long long key = splitmix(key_seed ^ splitmix(epoch));
  unsigned x = p;
  do {
    x = resident_feistel(key, x, hb);
  } while (x >= ur);   // p < records and the network is a bijection: the walk returns
  return (int)x;
}

// workgroup n of the resident launch; im: 3072 B (6144 with MIX), red: 8 floats (16)
template <int MIX>
__device__ __forceinline__ void cifar_resident_wg(
    const uint8_t* __restrict__ records_u8, const int* __restrict__ labels_all,
    bf16* __restrict__ out, int* __restrict__ labels_out, const long long* pos, int records,
    int rank, int world, int shuffle, unsigned long long key_seed, int pad,
    unsigned long long seed, int train, int* crop_log, int* idx_log, uint4* __restrict__ zero,
    long zero_vec, const Mixup& mx, uint8_t* im, float* red) {
  constexpr int CHW = 3 * 32 * 32;
  const int n = blockIdx.x, tid = threadIdx.x;
  // the one global read the record address waits for; the same value in every lane
  const unsigned long long raw = pos ? (unsigned long long)*pos : 0ull;
  for (long i = blockIdx.x * 256L + tid; i < zero_vec; i += (long)gridDim.x * 256)
    zero[i] = make_uint4(0u, 0u, 0u, 0u);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)raw);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(raw >> 32));
  const unsigned long long step = ((unsigned long long)hi << 32) | lo;
  const int idx = resident_record(step, n, (int)gridDim.x, records, rank, world, shuffle, key_seed);
  if (tid == 0) {
    labels_out[n] = labels_all[idx];
    if (idx_log) idx_log[n] = idx;
  }
  int m = n, idx_b = idx;
  float lam = 1.f;
  CutBox box = {};
  if (MIX) {   // the partner's record: position m's own pick
    const MixDraw d = mix_side_outputs<MIX>(mx, seed, step, n, (int)gridDim.x, lam, box);
    m = (int)(((unsigned)n + d.shift) % gridDim.x);
    idx_b = resident_record(step, m, (int)gridDim.x, records, rank, world, shuffle, key_seed);
    if (tid == 0) mx.labels_b[n] = labels_all[idx_b];
  }
  cifar_augment_image<8, MIX>(records_u8 + (long)idx * CHW, records_u8 + (long)idx_b * CHW, out, n,
                              m, lam, box, pad, seed, step, train, crop_log, im,
                              im + (MIX ? CHW : 0), red);
}

__global__ void __launch_bounds__(256)
cifar_augment_resident_kernel(const uint8_t* __restrict__ records_u8,
                              const int* __restrict__ labels_all, bf16* __restrict__ out,
                              int* __restrict__ labels_out, const long long* pos, int records,
                              int rank, int world, int shuffle, unsigned long long key_seed,
                              int pad, unsigned long long seed, int train, int* crop_log,
                              int* idx_log, uint4* __restrict__ zero, long zero_vec) {
  __shared__ __attribute__((aligned(16))) uint8_t im[3 * 32 * 32];
  __shared__ float red[8];
  cifar_resident_wg<MIX_OFF>(records_u8, labels_all, out, labels_out, pos, records, rank, world,
                             shuffle, key_seed, pad, seed, train, crop_log, idx_log, zero, zero_vec,
                             Mixup{}, im, red);
}

__global__ void __launch_bounds__(256)
cifar_mixup_resident_kernel(const uint8_t* __restrict__ records_u8,
                            const int* __restrict__ labels_all, bf16* __restrict__ out,
                            int* __restrict__ labels_out, const long long* pos, int records,
                            int rank, int world, int shuffle, unsigned long long key_seed, int pad,
                            unsigned long long seed, int train, int* crop_log, int* idx_log,
                            uint4* __restrict__ zero, long zero_vec, Mixup mx) {
  __shared__ __attribute__((aligned(16))) uint8_t im[2 * 3 * 32 * 32];
  __shared__ float red[16];
  cifar_resident_wg<MIX_BLEND>(records_u8, labels_all, out, labels_out, pos, records, rank, world,
                               shuffle, key_seed, pad, seed, train, crop_log, idx_log, zero,
                               zero_vec, mx, im, red);
}

__global__ void __launch_bounds__(256)
cifar_cutmix_resident_kernel(const uint8_t* __restrict__ records_u8,
                             const int* __restrict__ labels_all, bf16* __restrict__ out,
                             int* __restrict__ labels_out, const long long* pos, int records,
                             int rank, int world, int shuffle, unsigned long long key_seed, int pad,
                             unsigned long long seed, int train, int* crop_log, int* idx_log,
                             uint4* __restrict__ zero, long zero_vec, Mixup mx) {
  __shared__ __attribute__((aligned(16))) uint8_t im[2 * 3 * 32 * 32];
  __shared__ float red[16];
  cifar_resident_wg<MIX_CUT>(records_u8, labels_all, out, labels_out, pos, records, rank, world,
                             shuffle, key_seed, pad, seed, train, crop_log, idx_log, zero, zero_vec,
                             mx, im, red);
}

// Generic-shape fallback (any H, W, Cpad): one element per thread iteration.
__global__ void __launch_bounds__(256)
cifar_augment_generic_kernel(const uint8_t* __restrict__ img, bf16* __restrict__ out, int H,
                             int W, int Cpad, int pad, unsigned long long seed,
                             const long long* gstep, int train, int* crop_log,
                             uint4* __restrict__ zero, long zero_vec) {
  __shared__ float red[8];
  const int n = blockIdx.x, tid = threadIdx.x;
  for (long i = blockIdx.x * 256L + tid; i < zero_vec; i += (long)gridDim.x * 256)
    zero[i] = make_uint4(0u, 0u, 0u, 0u);
  const int HW = H * W, CHW = 3 * HW;
  const uint8_t* src = img + (long)n * CHW;
  int oy = pad, ox = pad, flip = 0;
  if (train) {
    const unsigned long long step = gstep ? (unsigned long long)*gstep : 0ull;
    const unsigned long long h = splitmix(seed ^ splitmix(step * 0x100000001B3ull + n));
    oy = (int)(h % (2 * pad + 1));
    ox = (int)((h >> 16) % (2 * pad + 1));
    flip = (int)((h >> 32) & 1);
  }
  if (crop_log && tid == 0) {
    crop_log[n * 3 + 0] = oy;
    crop_log[n * 3 + 1] = ox;
    crop_log[n * 3 + 2] = flip;
  }
  auto val = [&](int p, int c) -> float {
    const int y = p / W, x = p - y * W;
    const int xs = flip ? (W - 1 - x) : x;
    const int py = y + oy - pad, px = xs + ox - pad;
    if (py < 0 || py >= H || px < 0 || px >= W) return 0.f;
    return (float)src[c * HW + py * W + px];
  };
  float s = 0.f, q = 0.f;
  for (int i = tid; i < CHW; i += 256) {
    const float v = val(i / 3, i % 3);
    s += v;
    q += v * v;
  }
  s = wave_sum(s);
  q = wave_sum(q);
  if ((tid & 63) == 0) {
    red[tid >> 6] = s;
    red[4 + (tid >> 6)] = q;
  }
  __syncthreads();
  const float tot = red[0] + red[1] + red[2] + red[3];
  const float totq = red[4] + red[5] + red[6] + red[7];
  const float nel = (float)CHW;
  const float mean = tot / nel;
  const float var = fmaxf(totq / nel - mean * mean, 0.f);
  const float adj = fmaxf(sqrtf(var), rsqrtf(nel));
  const float inv = 1.f / adj;
  bf16* o = out + (long)n * HW * Cpad;
  for (int i = tid; i < HW * Cpad; i += 256) {
    const int p = i / Cpad, c = i - p * Cpad;
    o[i] = (bf16)(c < 3 ? (val(p, c) - mean) * inv : 0.f);
  }
}

// the mixup arguments of an input launch (`host_fed`: the partner labels come from `labels`)
static Mixup mix_args(const char* op, const Mixup& mix, bool host_fed, int train) {
  if (!mix.table) {
    if (mix.cut_thresh)
      throw std::invalid_argument(std::string(op) + ": cut_thresh > 0 needs the mixup arguments");
    return Mixup{};
  }
  if (!train)
    throw std::invalid_argument(std::string(op) + ": mixup and CutMix are training augmentations");
  if (mix.table_len < 1 || !mix.labels_b || !mix.mix_lam || (host_fed && !mix.labels))
    throw std::invalid_argument(std::string(op) + ": mixup needs a table of >= 1 entries, " +
                                (host_fed ? "labels, " : "") + "labels_b and mix_lam");
  if (mix.cut_thresh > (1u << 24))
    throw std::invalid_argument(std::string(op) + ": cut_thresh is out of 2^24");
  if (mix.cut_thresh && !mix.cut_table)
    throw std::invalid_argument(std::string(op) + ": cut_thresh > 0 needs a cut_table");
  return mix;
}

void cifar_augment(const uint8_t* img, bf16* out, int N, int H, int W, int Cpad, int pad,
                   unsigned long long seed, const long long* gstep, int train, int* crop_log,
                   void* zero, long zero_bytes, hipStream_t s, const Mixup& mix) {
  if (zero_bytes % 16) throw std::invalid_argument("cifar_augment: zero_bytes % 16 != 0");
  uint4* z = reinterpret_cast<uint4*>(zero);
  const long zv = zero ? zero_bytes / 16 : 0;
  const Mixup mx = mix_args("cifar_augment", mix, true, train);
  if (mx.table && !(H == 32 && W == 32 && Cpad == 8))
    throw std::invalid_argument("cifar_augment: mixup only for 32x32 images with Cpad 8");
  if (mx.cut_thresh)
    hipLaunchKernelGGL(cifar_cutmix_kernel<8>, dim3(N), dim3(256), 0, s, img, out, pad, seed,
                       gstep, train, crop_log, z, zv, mx);
  else if (mx.table)
    hipLaunchKernelGGL(cifar_mixup_kernel<8>, dim3(N), dim3(256), 0, s, img, out, pad, seed,
                       gstep, train, crop_log, z, zv, mx);
  else if (H == 32 && W == 32 && Cpad == 8)
    hipLaunchKernelGGL(cifar_augment_kernel<8>, dim3(N), dim3(256), 0, s, img, out, pad, seed,
                       gstep, train, crop_log, z, zv);
  else
    hipLaunchKernelGGL(cifar_augment_generic_kernel, dim3(N), dim3(256), 0, s, img, out, H, W,
                       Cpad, pad, seed, gstep, train, crop_log, z, zv);
  DTR_CHECK_LAUNCH();
}

void cifar_augment_resident(const uint8_t* records_u8, const int* labels_all, bf16* out,
                            int* labels_out, const long long* pos, int N, int H, int W, int Cpad,
                            long records, int rank, int world, int shuffle,
                            unsigned long long key_seed, int pad, unsigned long long seed,
                            int train, int* crop_log, int* idx_log, void* zero, long zero_bytes,
                            hipStream_t s, const Mixup& mix) {
  cifar_augment_resident_check(N, H, W, Cpad, records, rank, world, zero_bytes);
  if (!records_u8 || !labels_all || !out || !labels_out || !pos)
    throw std::invalid_argument("cifar_augment_resident: null buffer");
  if (reinterpret_cast<uintptr_t>(records_u8) % 16)
    throw std::invalid_argument("cifar_augment_resident: records not 16-B aligned");
  const Mixup mx = mix_args("cifar_augment_resident", mix, false, train);
  if (mx.cut_thresh)
    hipLaunchKernelGGL(cifar_cutmix_resident_kernel, dim3(N), dim3(256), 0, s, records_u8,
                       labels_all, out, labels_out, pos, (int)records, rank, world,
                       shuffle ? 1 : 0, key_seed, pad, seed, train, crop_log, idx_log,
                       reinterpret_cast<uint4*>(zero), zero ? zero_bytes / 16 : 0, mx);
  else if (mx.table)
    hipLaunchKernelGGL(cifar_mixup_resident_kernel, dim3(N), dim3(256), 0, s, records_u8,
                       labels_all, out, labels_out, pos, (int)records, rank, world,
                       shuffle ? 1 : 0, key_seed, pad, seed, train, crop_log, idx_log,
                       reinterpret_cast<uint4*>(zero), zero ? zero_bytes / 16 : 0, mx);
  else
    hipLaunchKernelGGL(cifar_augment_resident_kernel, dim3(N), dim3(256), 0, s, records_u8,
                       labels_all, out, labels_out, pos, (int)records, rank, world,
                       shuffle ? 1 : 0, key_seed, pad, seed, train, crop_log, idx_log,
                       reinterpret_cast<uint4*>(zero), zero ? zero_bytes / 16 : 0);
  DTR_CHECK_LAUNCH();
}

void cifar_augment_resident_check(int N, int H, int W, int Cpad, long records, int rank,
                                  int world, long zero_bytes) {
  if (H != 32 || W != 32 || Cpad != 8)
    throw std::invalid_argument("cifar_augment_resident: only 32x32 images with Cpad 8");
  if (N < 1 || world < 1) throw std::invalid_argument("cifar_augment_resident: batch, world >= 1");
  if (rank < 0 || rank >= world) throw std::invalid_argument("cifar_augment_resident: rank >= world");
  if (records >= (1L << 31)) throw std::invalid_argument("cifar_augment_resident: records >= 2^31");
  if (records < (long)N * world)
    throw std::invalid_argument("cifar_augment_resident: records < batch * world");
  if (zero_bytes % 16) throw std::invalid_argument("cifar_augment_resident: zero_bytes % 16 != 0");
}

__global__ void pad_channels_kernel(const float* __restrict__ x, bf16* __restrict__ out, long npix,
                                    int C, int Cpad) {
  const long total = npix * Cpad;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long p = i / Cpad;
    const int c = (int)(i - p * Cpad);
    out[i] = (bf16)(c < C ? x[p * C + c] : 0.f);
  }
}

void nhwc_pad_channels(const float* x, bf16* out, long npix, int C, int Cpad, hipStream_t s) {
  long blocks = (npix * Cpad + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(pad_channels_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, out, npix,
                     C, Cpad);
  DTR_CHECK_LAUNCH();
}

// Gaussian-ish synthetic activations (sum of 4 uniforms, unit variance) in
// NHWC with the padded channels kept zero.
__global__ void synth_kernel(bf16* out, long npix, int C, int Cpad, unsigned long long seed) {
  const long total = npix * Cpad;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cpad);
    float v = 0.f;
    if (c < C) {
      const unsigned long long h = splitmix(seed + (unsigned long long)i);
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) s += (float)((h >> (16 * k)) & 0xFFFF) * (1.f / 65535.f);
      v = (s - 2.f) * 1.7320508f;
    }
    out[i] = (bf16)v;
  }
}

void synthetic_images(bf16* out, long npix, int C, int Cpad, unsigned long long seed,
                      hipStream_t s) {
  long blocks = (npix * Cpad + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(synth_kernel, dim3((unsigned)blocks), dim3(256), 0, s, out, npix, C, Cpad,
                     seed);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr

namespace dtr {

// ImageNet real-data feed (resnet_imagenet_main.py:122-192 with VGG preprocessing,
// vgg_preprocessing.py:284-333): CPU workers decode the JPEG, do the
// aspect-preserving resize and the random (train) / central (eval) 224x224 crop
// and ship the crop as uint8 HWC -- 4x fewer host->device bytes than float32.
// This kernel does the rest on the device: the random left-right flip (hash of
// (seed, global_step, image), like cifar_augment), the per-channel mean
// subtraction (R,G,B = 123.68, 116.78, 103.94, vgg_preprocessing.py:37-39) and the
// bf16 NHWC packing with the channel dim padded to 8 (one 16-B row per pixel,
// the stem conv's operand layout).  Optionally clears a buffer in the same launch
// (the step's BatchNorm accumulators).  One thread per output pixel.
// MIX (mixup, above): the thread also reads its pixel of the partner crop m = (n + shift)
// % N, from the same batch buffer and with position m's own flip, and writes
// bf16(lam * a + (1.f - lam) * b) of the two mean-subtracted fp32 values, rounded once.
template <bool MIX>
__global__ void __launch_bounds__(256)
imagenet_u8_pack_kernel(const uint8_t* __restrict__ img, bf16* __restrict__ out, int H, int W,
                        unsigned long long seed, const long long* gstep, int train,
                        uint4* __restrict__ zero, long zero_vec, long npix, int s2d, int N,
                        Mixup mx) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < zero_vec; i += (long)gridDim.x * 256)
    zero[i] = make_uint4(0u, 0u, 0u, 0u);
  const long p = blockIdx.x * 256L + threadIdx.x;
  if (p >= npix) return;
  const long HW = (long)H * W;
  const long n = p / HW;
  const int rem = (int)(p - n * HW);
  const int y = rem / W, x = rem - y * W;
  const unsigned long long step = (train && gstep) ? (unsigned long long)*gstep : 0ull;
  int flip = 0;
  if (train)
    flip = (int)((splitmix(seed ^ splitmix(step * 0x100000001B3ull + (unsigned long long)n)) >> 32) & 1);
  const int xs = flip ? W - 1 - x : x;
  const uint8_t* src = img + ((n * H + y) * (long)W + xs) * 3;
  float f0 = (float)src[0] - 123.68f, f1 = (float)src[1] - 116.78f, f2 = (float)src[2] - 103.94f;
  if (MIX) {
    const MixDraw d = mixup_draw(seed, step, N, mx.table_len);
    const float lam = mx.table[d.index];
    const long m = (long)(((unsigned)n + d.shift) % (unsigned)N);
    const int flip_b =
        (int)((splitmix(seed ^ splitmix(step * 0x100000001B3ull + (unsigned long long)m)) >> 32) & 1);
    const int xb = flip_b ? W - 1 - x : x;
    const uint8_t* sb = img + ((m * H + y) * (long)W + xb) * 3;
    f0 = lam * f0 + (1.f - lam) * ((float)sb[0] - 123.68f);
    f1 = lam * f1 + (1.f - lam) * ((float)sb[1] - 116.78f);
    f2 = lam * f2 + (1.f - lam) * ((float)sb[2] - 103.94f);
    if (rem == 0) {   // the image's first pixel writes its side outputs
      mx.labels_b[n] = mx.labels[m];
      mx.mix_lam[n] = lam;
      if (mx.mix_log && n == 0) {
        mx.mix_log[0] = (int)d.index;
        mx.mix_log[1] = (int)d.shift;
      }
    }
  }
  const bf16 c0 = (bf16)f0, c1 = (bf16)f1, c2 = (bf16)f2;
  if (s2d) {   // space-to-depth stem operand [N][H/2][W/2][16] (stem_s2d_pack below)
    bf16x4 r = {c0, c1, c2, (bf16)0.f};
    const long q = (n * (H >> 1) + (y >> 1)) * (long)(W >> 1) + (x >> 1);
    *reinterpret_cast<bf16x4*>(out + q * 16 + ((y & 1) * 2 + (x & 1)) * 4) = r;
    return;
  }
  bf16x8 r = {};
  r[0] = c0;
  r[1] = c1;
  r[2] = c2;
  *reinterpret_cast<bf16x8*>(out + p * 8) = r;
}

// The mixed launch with CutMix (a kernel of its own: the two above keep their code).  The box
// is in the flipped image's coordinates, before the space-to-depth packing.  In a CutMix step
// the thread reads only the one source pixel it writes -- the partner's inside the box, with
// the partner's own flip, its own outside; in a mixup step it blends as the kernel above.
__global__ void __launch_bounds__(256)
imagenet_u8_cutmix_kernel(const uint8_t* __restrict__ img, bf16* __restrict__ out, int H, int W,
                          unsigned long long seed, const long long* gstep, int train,
                          uint4* __restrict__ zero, long zero_vec, long npix, int s2d, int N,
                          Mixup mx) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < zero_vec; i += (long)gridDim.x * 256)
    zero[i] = make_uint4(0u, 0u, 0u, 0u);
  const long p = blockIdx.x * 256L + threadIdx.x;
  if (p >= npix) return;
  const long HW = (long)H * W;
  const long n = p / HW;
  const int rem = (int)(p - n * HW);
  const int y = rem / W, x = rem - y * W;
  const unsigned long long step = (train && gstep) ? (unsigned long long)*gstep : 0ull;
  CutBox box;
  float lam;
  const MixDraw d = cutmix_draw(mx, seed, step, N, H, W, p == 0, box, lam);
  const long m = (long)(((unsigned)n + d.shift) % (unsigned)N);
  const bool paste = box.cut && box.has(y, x);
  const long own = paste ? m : n;   // the image of the one pixel a CutMix step reads
  const int flip =
      (int)((splitmix(seed ^ splitmix(step * 0x100000001B3ull + (unsigned long long)own)) >> 32) & 1);
  const int xs = flip ? W - 1 - x : x;
  const uint8_t* src = img + ((own * H + y) * (long)W + xs) * 3;
  float f0 = (float)src[0] - 123.68f, f1 = (float)src[1] - 116.78f, f2 = (float)src[2] - 103.94f;
  if (!box.cut) {
    const int flip_b =
        (int)((splitmix(seed ^ splitmix(step * 0x100000001B3ull + (unsigned long long)m)) >> 32) & 1);
    const int xb = flip_b ? W - 1 - x : x;
    const uint8_t* sb = img + ((m * H + y) * (long)W + xb) * 3;
    f0 = lam * f0 + (1.f - lam) * ((float)sb[0] - 123.68f);
    f1 = lam * f1 + (1.f - lam) * ((float)sb[1] - 116.78f);
    f2 = lam * f2 + (1.f - lam) * ((float)sb[2] - 103.94f);
  }
  if (rem == 0) {   // the image's first pixel writes its side outputs
    mx.labels_b[n] = mx.labels[m];
    mx.mix_lam[n] = lam;
  }
  const bf16 c0 = (bf16)f0, c1 = (bf16)f1, c2 = (bf16)f2;
  if (s2d) {
    bf16x4 r = {c0, c1, c2, (bf16)0.f};
    const long q = (n * (H >> 1) + (y >> 1)) * (long)(W >> 1) + (x >> 1);
    *reinterpret_cast<bf16x4*>(out + q * 16 + ((y & 1) * 2 + (x & 1)) * 4) = r;
    return;
  }
  bf16x8 r = {};
  r[0] = c0;
  r[1] = c1;
  r[2] = c2;
  *reinterpret_cast<bf16x8*>(out + p * 8) = r;
}

void imagenet_u8_pack(const uint8_t* img, bf16* out, int N, int H, int W,
                      unsigned long long seed, const long long* gstep, int train, void* zero,
                      long zero_bytes, int s2d, hipStream_t s, const Mixup& mix) {
  if (zero_bytes % 16 != 0) throw std::invalid_argument("imagenet_u8_pack: zero_bytes % 16");
  if (s2d && ((H | W) & 1)) throw std::invalid_argument("imagenet_u8_pack: s2d needs even H, W");
  const Mixup mx = mix_args("imagenet_u8_pack", mix, true, train);
  const long npix = (long)N * H * W;
  const int grid = (int)((npix + 255) / 256);
  if (mx.cut_thresh && (H >= (1 << 15) || W >= (1 << 15) || (long)H * W > (1L << 24)))
    throw std::invalid_argument("imagenet_u8_pack: CutMix needs H, W < 2^15 and H * W <= 2^24");
  if (mx.cut_thresh)
    hipLaunchKernelGGL(imagenet_u8_cutmix_kernel, dim3(grid), dim3(256), 0, s, img, out, H, W,
                       seed, gstep, train, reinterpret_cast<uint4*>(zero),
                       zero ? zero_bytes / 16 : 0, npix, s2d, N, mx);
  else if (mx.table)
    hipLaunchKernelGGL(imagenet_u8_pack_kernel<true>, dim3(grid), dim3(256), 0, s, img, out, H, W,
                       seed, gstep, train, reinterpret_cast<uint4*>(zero),
                       zero ? zero_bytes / 16 : 0, npix, s2d, N, mx);
  else
    hipLaunchKernelGGL(imagenet_u8_pack_kernel<false>, dim3(grid), dim3(256), 0, s, img, out, H, W,
                       seed, gstep, train, reinterpret_cast<uint4*>(zero),
                       zero ? zero_bytes / 16 : 0, npix, s2d, N, mx);
  DTR_CHECK_LAUNCH();
}

// Space-to-depth ImageNet stem.  The 7x7 / stride-2 conv (TF fixed padding 3) over
// a 224x224x3 image equals a 4x4 / stride-1 conv (padding 2 before, 1 after) over
// the 112x112x16 space-to-depth image S[q][p][(rh*2 + rw)*4 + c] = X[2q+rh][2p+rw][c]
// (c = 3 zero): out(o) = sum_th S(o - 2 + th) reads rows 2o - 4 + 2th + rh, i.e.
// tap kh = 2th + rh - 1 of the 7x7 filter (kh = -1 is a zero row).  K = 4*4*16 = 256
// instead of 7*7*8 = 392 (57 % of the MACs real instead of 37 %), stride-1 gathers of
// 32-B pixel rows, and a weight gradient of 256 columns (two 128-wide tiles instead of
// four, the last 94 % empty).  The fp32 master weight stays the 7x7x3 HWIO of the
// checkpoint; these two kernels map it to the bf16 4x4x16 OHWI operand and the 4x4x16
// HWIO weight gradient back.
__global__ void stem_s2d_pack_kernel(const float* __restrict__ w7, bf16* __restrict__ w4, int K) {
  const int i = blockIdx.x * 256 + threadIdx.x;   // [K][4][4][16]
  if (i >= K * 256) return;
  const int o = i >> 8, r = i & 255;
  const int th = r >> 6, tw = (r >> 4) & 3, ch = r & 15;
  const int kh = 2 * th + (ch >> 3) - 1, kw = 2 * tw + ((ch >> 2) & 1) - 1, c = ch & 3;
  float v = 0.f;
  if (c < 3 && kh >= 0 && kh < 7 && kw >= 0 && kw < 7) v = w7[((kh * 7 + kw) * 3 + c) * K + o];
  w4[i] = (bf16)v;
}

__global__ void stem_s2d_grad_kernel(const float* __restrict__ g4, float* __restrict__ g7, int K) {
  const int i = blockIdx.x * 256 + threadIdx.x;   // [7][7][3][K]
  if (i >= 147 * K) return;
  const int o = i % K, t = i / K;
  const int c = t % 3, tap = t / 3;
  const int kh = tap / 7 + 1, kw = tap % 7 + 1;   // +1: row / column of the 8x8 grid
  const int ch = ((kh & 1) * 2 + (kw & 1)) * 4 + c;
  g7[i] = g4[(((kh >> 1) * 4 + (kw >> 1)) * 16 + ch) * K + o];
}

void stem_s2d_pack(const float* w7, bf16* w4, int K, hipStream_t s) {
  hipLaunchKernelGGL(stem_s2d_pack_kernel, dim3(K), dim3(256), 0, s, w7, w4, K);
  DTR_CHECK_LAUNCH();
}

void stem_s2d_grad(const float* g4, float* g7, int K, hipStream_t s) {
  hipLaunchKernelGGL(stem_s2d_grad_kernel, dim3((147 * K + 255) / 256), dim3(256), 0, s, g4, g7, K);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
