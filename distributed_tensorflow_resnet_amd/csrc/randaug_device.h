// What randaug.hip and augmix.hip share: the 14 integer ops of data/randaug.py on one image
// held by one workgroup (layout L, T threads), their statistics and the draw's hash.
//
// Statistics: a 3x256 uint32 histogram by LDS atomic adds and a 256-bin exclusive prefix sum by
// one wave per channel with cross-lane adds (Equalize); channel min/max (AutoContrast) and the
// grey sum (Contrast) as integer wave reductions plus a small LDS combine -- exact sums, no
// fp32.  Brightness, Contrast, Posterize, Solarize, AutoContrast and Equalize all end as a
// 3x256 byte LUT in LDS applied 16 bytes per thread.  No inline assembly, plain C++ stores.
#pragma once
#include "common.h"

namespace dtr {

constexpr int RA_FILL = 128;
// randaug_tables: [5 ops 1..5][2 signs][6] Q16 coefficients, [2 signs] Q16 blend factor, the
// Posterize mask, the Solarize threshold
constexpr int RA_T_GEO = 0, RA_T_BLEND = 60, RA_T_POST = 62, RA_T_SOL = 63, RA_TABLE_LEN = 64;
constexpr int RA_LDS_MAX = 160 * 1024;   // gfx950: LDS of one CU, all of it one workgroup's

struct alignas(16) RaScratch {
  unsigned hist[3 * 256];   // histogram, then its exclusive prefix sums
  unsigned red[16 * 8];     // per-wave partials of the reductions
  unsigned last[4];         // Equalize: the count of each channel's last non-zero bin
  uint8_t lut[3 * 256];     // at a 16-B offset
};

struct RaCHW {   // planar [3][H][W]; a 16-B vector lies in one plane (H * W % 16 == 0)
  static __device__ __forceinline__ int at(int c, int p, int HW) { return c * HW + p; }
  static __device__ __forceinline__ int chan(int vec, int k, int HW) { return vec * 16 / HW; }
};
struct RaHWC {   // interleaved [H][W][3]; byte 16 vec + k is channel (vec + k) % 3
  static __device__ __forceinline__ int at(int c, int p, int HW) { return p * 3 + c; }
  static __device__ __forceinline__ int chan(int vec, int k, int HW) {
    return (vec % 3 + k % 3) % 3;
  }
};

__device__ __forceinline__ unsigned long long ra_splitmix(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ int ra_blend(int D, int p, int F) {
  const int v = (D * (65536 - F) + p * F + 32768) >> 16;   // >> floors
  return min(max(v, 0), 255);
}

__device__ __forceinline__ int ra_grey(int r, int g, int b) {
  return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
}

// the sum of v over the workgroup, in every thread (two barriers)
template <int T>
__device__ __forceinline__ unsigned ra_block_sum(unsigned v, unsigned* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned r = 0;
#pragma unroll
  for (int w = 0; w < T / 64; ++w) r += red[w];
  __syncthreads();
  return r;
}

// the maxima of v[0..5] over the workgroup, in every thread (two barriers)
template <int T>
__device__ __forceinline__ void ra_block_max6(int (&v)[6], unsigned* red) {
#pragma unroll
  for (int j = 0; j < 6; ++j) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[j] = max(v[j], __shfl_xor(v[j], o, 64));
    if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * 8 + j] = (unsigned)v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    int r = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) r = max(r, (int)red[w * 8 + j]);
    v[j] = r;
  }
  __syncthreads();
}

// Equalize's statistics: s.hist becomes each channel's exclusive prefix sums, s.last the
// count of its last non-zero bin.  Wave c scans channel c: four bins per lane, then a
// cross-lane inclusive scan of the lane totals.
template <class L, int T>
__device__ __forceinline__ void ra_histogram(const uint8_t* img, int HW, RaScratch& s) {
  const int tid = threadIdx.x;
  for (int i = tid; i < 3 * 256; i += T) s.hist[i] = 0u;
  __syncthreads();
  for (int p = tid; p < HW; p += T) {
#pragma unroll
    for (int c = 0; c < 3; ++c) atomicAdd(&s.hist[c * 256 + img[L::at(c, p, HW)]], 1u);
  }
  __syncthreads();
  if (tid < 3 * 64) {
    const int c = tid >> 6, lane = tid & 63;
    uint4* bins = reinterpret_cast<uint4*>(&s.hist[c * 256 + lane * 4]);
    const uint4 q = *bins;
    const unsigned tot = q.x + q.y + q.z + q.w;
    unsigned inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    const unsigned base = inc - tot;
    int last = q.w ? lane * 4 + 3 : q.z ? lane * 4 + 2 : q.y ? lane * 4 + 1 : q.x ? lane * 4 : -1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
    if (last >= 0 && (last >> 2) == lane)
      s.last[c] = (last & 3) == 3 ? q.w : (last & 3) == 2 ? q.z : (last & 3) == 1 ? q.y : q.x;
    *bins = make_uint4(base, base + q.x, base + q.x + q.y, base + q.x + q.y + q.z);
  }
  __syncthreads();
}

// img[i] = lut[channel of i][img[i]] for the whole image, 16 bytes per thread, in place
template <class L, int T>
__device__ __forceinline__ void ra_apply_lut(uint8_t* img, int HW, const uint8_t* lut) {
  uint4* v = reinterpret_cast<uint4*>(img);
  const int nvec = 3 * HW / 16;
  for (int i = threadIdx.x; i < nvec; i += T) {
    const uint4 q = v[i];
    unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned r = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b)
        r |= (unsigned)lut[L::chan(i, j * 4 + b, HW) * 256 + ((w[j] >> (8 * b)) & 255u)]
             << (8 * b);
      w[j] = r;
    }
    v[i] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// One op on the image at `img` (H x W, layout L).  Ops that read other positions than the one
// they write put their result into `other` and return true: the image has moved.  Every path
// ends with a barrier that also waits for this workgroup's global stores.
template <class L, int T>
__device__ __forceinline__ bool ra_op(int op, int sign, uint8_t* img, uint8_t* other, int H,
                                      int W, RaScratch& s, const int* __restrict__ tab) {
  const int tid = threadIdx.x, HW = H * W;
  const int F = tab[RA_T_BLEND + sign];
  bool moved = false;
  switch (op) {
    case 1: case 2: case 3: case 4: case 5: {   // inverse-mapped nearest-neighbour gather
      const int* k = tab + RA_T_GEO + ((op - 1) * 2 + sign) * 6;
      const int a = k[0], b = k[1], c = k[2], d = k[3], e = k[4], f = k[5];
      for (int p = tid; p < HW; p += T) {
        const int y = p / W, x = p - y * W;
        const int u = 2 * x - (W - 1), v = 2 * y - (H - 1);
        const int sx = (a * u + b * v + c + (W << 16)) >> 17;
        const int sy = (d * u + e * v + f + (H << 16)) >> 17;
        const bool in = (unsigned)sx < (unsigned)W && (unsigned)sy < (unsigned)H;
        const int sp = in ? sy * W + sx : 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const uint8_t got = img[L::at(ch, sp, HW)];
          other[L::at(ch, p, HW)] = in ? got : (uint8_t)RA_FILL;
        }
      }
      moved = true;
      break;
    }
    case 7: {   // Color: towards / away from the pixel's own grey
      for (int p = tid; p < HW; p += T) {
        const int r = img[L::at(0, p, HW)], g = img[L::at(1, p, HW)], b = img[L::at(2, p, HW)];
        const int D = ra_grey(r, g, b);
        img[L::at(0, p, HW)] = (uint8_t)ra_blend(D, r, F);
        img[L::at(1, p, HW)] = (uint8_t)ra_blend(D, g, F);
        img[L::at(2, p, HW)] = (uint8_t)ra_blend(D, b, F);
      }
      break;
    }
    case 9: {   // Sharpness: towards / away from the 3x3 smooth [[1,1,1],[1,5,1],[1,1,1]] / 13
      for (int p = tid; p < HW; p += T) {
        const int y = p / W, x = p - y * W;
        const bool inner = y >= 1 && y < H - 1 && x >= 1 && x < W - 1;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int v = img[L::at(ch, p, HW)];
          int D = v;   // a border pixel is its own degenerate
          if (inner) {
            int sum = 4 * v;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
              for (int dx = -1; dx <= 1; ++dx) sum += img[L::at(ch, p + dy * W + dx, HW)];
            D = (sum + 6) / 13;
          }
          other[L::at(ch, p, HW)] = (uint8_t)ra_blend(D, v, F);
        }
      }
      moved = true;
      break;
    }
    case 6: case 8: case 10: case 11: case 12: case 13: {   // a 3x256 LUT, applied in place
      int mean = 0, mm[6] = {0, 0, 0, 0, 0, 0};
      if (op == 8) {   // Contrast: the image's mean grey, rounded half up
        unsigned sum = 0;
        for (int p = tid; p < HW; p += T)
          sum += (unsigned)ra_grey(img[L::at(0, p, HW)], img[L::at(1, p, HW)],
                                   img[L::at(2, p, HW)]);
        sum = ra_block_sum<T>(sum, s.red);
        mean = (int)((2u * sum + (unsigned)HW) / (2u * (unsigned)HW));
      } else if (op == 12) {   // AutoContrast: 255 - min and max per channel
        for (int p = tid; p < HW; p += T) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const int v = img[L::at(ch, p, HW)];
            mm[ch] = max(mm[ch], 255 - v);
            mm[3 + ch] = max(mm[3 + ch], v);
          }
        }
        ra_block_max6<T>(mm, s.red);
      } else if (op == 13) {
        ra_histogram<L, T>(img, HW, s);
      }
      const int post = tab[RA_T_POST], sol = tab[RA_T_SOL];
      for (int i = tid; i < 3 * 256; i += T) {
        const int ch = i >> 8, p = i & 255;
        int r = p;
        if (op == 6) {
          r = ra_blend(0, p, F);
        } else if (op == 8) {
          r = ra_blend(mean, p, F);
        } else if (op == 10) {
          r = p & post;
        } else if (op == 11) {
          r = p >= sol ? 255 - p : p;
        } else if (op == 12) {
          const int lo = 255 - (ch == 0 ? mm[0] : ch == 1 ? mm[1] : mm[2]);
          const int hi = ch == 0 ? mm[3] : ch == 1 ? mm[4] : mm[5];
          if (hi > lo) r = min(255, (max(p - lo, 0) * 510 + (hi - lo)) / (2 * (hi - lo)));
        } else {   // Equalize (PIL / TF): step 0 leaves the channel as it is
          const unsigned step = ((unsigned)HW - s.last[ch]) / 255u;
          if (step) r = (int)min(255u, (s.hist[i] + step / 2u) / step);
        }
        s.lut[i] = (uint8_t)r;
      }
      __syncthreads();
      ra_apply_lut<L, T>(img, HW, s.lut);
      break;
    }
    default:   // 0, Identity (the ids are checked when the op is made)
      break;
  }
  __syncthreads();
  return moved;
}

}  // namespace dtr
