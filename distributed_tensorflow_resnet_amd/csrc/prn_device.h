// Persistent small-batch CIFAR step: the whole forward in one launch, the whole
// backward (with its weight gradients) in one more.
//
// Why: at the per-rank batches of the strong-scaling headline config (global batch 128
// over 4-8 GPUs = 16-32 images per rank) every CIFAR conv is a few MFMA microseconds
// wrapped in a ~1.5 us kernel boundary plus a global-memory round trip of its operands
// (profiles/cifar_direct_conv_phases.md); ~110 dependent launches set the step time.
// Here each image is split into P row slices and one 512-thread workgroup owns one slice
// for the whole network (resnet_model_official.py:217-278, building_block :94-130):
//   * the slice's activations stay on-chip between layers: a conv's fp32 accumulators
//     are rounded to bf16 in registers, the next BatchNorm + ReLU is applied from the
//     registers straight into an LDS halo, and the next conv reads its B operand there;
//   * a 3x3 conv needs one halo row from each neighbouring slice: the forward reads it
//     from the tensor the neighbour publishes anyway (the activations saved for the
//     backward, stored write-through before the barrier) and applies BN + ReLU itself;
//     the backward recomputes the neighbour's BN-backward output rows from what the
//     neighbour published before the barrier (its dgrad output) plus saved tensors;
//   * BatchNorm's batch statistics are the only cross-slice dependency: each workgroup
//     adds its slice's per-channel sums into fp64 replicas with memory-side atomics
//     (exact: fp32 partials summed in fp64, so the result does not depend on the order),
//     one grid barrier, then every workgroup reads the sums -- one round trip;
//   * the next layer's weights are prefetched into registers by waves 1-7 between the
//     barrier's arrive and its wait (wave 0 polls), then stored to LDS;
//   * MFMA orientation D[channel][pixel] = W[channel][k] x Act[k][pixel]
//     (v_mfma_f32_16x16x32_bf16): a lane's accumulator holds 4 consecutive channels of
//     one pixel, i.e. one 8-byte NHWC store / LDS write after the bf16 rounding;
//   * pixels are kept in a "canonical" order per slice: parity-class-major on the 32x32
//     and 16x16 maps, so every stride-2 dgrad tile (sub-pixel decomposition: 1, 2, 2 or
//     4 taps per output parity class) is made of pixels of one class.
// In the backward launch the workgroups beyond the N x P slices compute the 52 weight
// gradients (dW = sum_p dy x im2col(relu(bn(x)))) per image group into fp32 slabs: they
// take items from one queue in readiness order (the slices join once their dgrad chain
// is done), each as soon as the readiness count says its dy is published; the existing
// deterministic grouped reduce sums the slabs afterwards (which workgroup ran an item
// does not change its slab: bitwise deterministic).
//
// Hand-off protocol (MI355X_MICROARCH.md, "Valid forms" row 1): every byte another
// workgroup reads inside the launch (published tensors) is stored write-through (sc1),
// every wave drains (s_waitcnt vmcnt(0)) before its workgroup's lane 0 adds to the
// barrier counter, consumers poll the counter with relaxed agent loads and read the bytes
// with sc1 loads.  BN sums are memory-side atomics, read with sc1 loads after the
// barrier.  Every spin is bounded (2 s of wall clock): a timed-out wait sets *err and the
// workgroup exits.  The grid must be co-resident: one workgroup per CU, grid <= CUs.
//
// This header is internal to the three launches' translation units -- prn_fwd.hip (the
// training forward), prn_bwd.hip (the backward, its weight-gradient items, the head folds
// and the bucket wait) and prn_infer.hip (the inference forward) -- and holds what more
// than one of them uses: geometry, load / store flavours, the grid barrier, weight
// staging, the convolution on the LDS halo, the BN sums, the LDS carve-up, and the pieces
// the two forwards share (stem fill, next-block lookup, pool partials).
#pragma once
#include <algorithm>
#include <stdexcept>

#include "common.h"
#include "kernels.h"

namespace dtr {

namespace {

constexpr int PT = PRN_THREADS;
constexpr int NW = PT / 64;                  // waves per workgroup
constexpr long long kSpinTicks = 200000000;  // 2 s at 100 MHz

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---- geometry ---------------------------------------------------------------------
template <int S, int P>
struct Stg {                                  // stage S: R x R maps, C channels, P slices
  static constexpr int R = 32 >> S, C = 16 << S, U = C / 8, W2 = R + 2;
  static constexpr int RS = R / P, HR = RS + 2;          // rows per slice, halo rows
  static constexpr int NPX = R * RS;                     // pixels per slice
  static constexpr int NPB = NPX / 16, NCB = C / 16;     // 16-pixel / 16-channel blocks
  static constexpr int WPB = NPB >= NW ? 1 : NW / NPB;   // waves per pixel block
  static constexpr int PBW = NPB >= NW ? NPB / NW : 1;   // pixel blocks per wave
  static constexpr int CBW = NCB / WPB > 0 ? NCB / WPB : 1;   // channel blocks per wave
  static constexpr int TPW = PBW * CBW;                  // 16x16 tiles per wave
  static constexpr int NT = NPB * NCB;                   // 16x16 output tiles
  static constexpr bool ALL = NT >= NW;                  // every wave holds tiles
  static constexpr bool CLS = R > 8;                     // parity-class-major pixel order
  static_assert(RS >= 2 && (!CLS || RS % 2 == 0) && NPX % 16 == 0 && TPW <= 8, "slices");
  static_assert(!CLS || (NPB / 4) % PBW == 0, "a wave's pixel blocks lie in one class");
};

// slice k's canonical pixel p -> image (h, w): parity-class-major on 32x32 / 16x16
// (class, class row, class column), row-major on 8x8
template <int S, int P>
__device__ __forceinline__ void canon(int k, int p, int& h, int& w) {
  using G = Stg<S, P>;
  if constexpr (G::CLS) {
    constexpr int Q = G::NPX / 4, H2 = G::R / 2;
    const int cls = p / Q, idx = p - cls * Q, il = idx / H2;
    h = k * G::RS + 2 * il + (cls >> 1);
    w = 2 * (idx - il * H2) + (cls & 1);
  } else {
    h = k * G::RS + p / G::R;
    w = p % G::R;
  }
}

// this wave's tile t -> (pixel block, channel block); a wave is idle (no tiles) when the
// slice has fewer tiles than waves and its channel block is past the last
template <int S, int P>
__device__ __forceinline__ void tile_of(int wave, int t, int& pb, int& cb) {
  using G = Stg<S, P>;
  pb = (wave / G::WPB) * G::PBW + t / G::CBW;
  cb = (wave % G::WPB) * G::CBW + t % G::CBW;
}
template <int S, int P>
__device__ __forceinline__ bool wave_active(int wave) {
  using G = Stg<S, P>;
  return G::ALL || (wave % G::WPB) * G::CBW < G::NCB;
}

// LDS halo element offset: local pixel `pix` (row-major in the HR x W2 slice halo,
// column lc), channel c (multiple of 4) of a U-unit (8 channels per 16-B unit) image;
// units XOR-swizzled by the column so a fragment's 16 pixel lanes spread over banks
// (Not on the 32x32 map, U = 2: its fragments are parity-class-major, so their 16 lanes
// share the column parity and the swizzle bit -- it moved no lane to another bank, and
// without it a halo read is one add on a per-pixel-block base instead of five VALU ops.)
template <int U>
__device__ __forceinline__ int haddr(int pix, int lc, int c) {
  if constexpr (U == 2) return pix * 16 + c;
  return (pix * U + ((c >> 3) ^ (lc & (U - 1)))) * 8 + (c & 7);
}

// Descriptor tables (blocks, BatchNorms, weight-gradient items) are read-only for the
// whole launch: read them through the constant address space, i.e. scalar loads into
// SGPRs via the scalar cache.  Through a generic pointer the compiler issues vector
// loads, waits a full memory round trip for each pointer it needs and then builds
// buffer descriptors from VGPRs in readfirstlane loops.
#define DTR_CONST_AS __attribute__((address_space(4)))
template <typename T>
__device__ __forceinline__ T ld_const(const T* p) {
#if __HIP_DEVICE_COMPILE__
  return *(const DTR_CONST_AS T*)p;
#else
  return *p;   // (host pass: never called)
#endif
}

// Global loads / stores through pointers read from the descriptor tables: the compiler
// cannot infer their address space and emits flat instructions, which also count in
// lgkmcnt -- every LDS barrier (s_waitcnt lgkmcnt(0)) after one then waits for a memory
// round trip.  These casts make them global_load / global_store.
template <typename T>
__device__ __forceinline__ T ldg(const T* p) {
#if __HIP_DEVICE_COMPILE__
  return *(const __attribute__((address_space(1))) T*)p;
#else
  return *p;
#endif
}
template <typename T>
__device__ __forceinline__ void stg(T* p, T v) {
#if __HIP_DEVICE_COMPILE__
  *(__attribute__((address_space(1))) T*)p = v;
#else
  *p = v;
#endif
}

// 4-byte write-through store (global_store_dword ... sc1): read by another agent-scope
// consumer before this kernel ends (overlap mode)
__device__ __forceinline__ void st_sc1_f32(float* p, float v) {
#if __HIP_DEVICE_COMPILE__
  __hip_atomic_store((__attribute__((address_space(1))) float*)p, v, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
#else
  *p = v;
#endif
}

__device__ __forceinline__ bf16x8 lds16(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }

__device__ __forceinline__ double ld_sc1_d(const double* p) {
#if __HIP_DEVICE_COMPILE__
  return __hip_atomic_load((const __attribute__((address_space(1))) double*)p, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}
// memory-side fp64 add (global_atomic_add_f64, no return)
__device__ __forceinline__ void atomic_add_g(double* p, double v) {
#if __HIP_DEVICE_COMPILE__
  __builtin_amdgcn_global_atomic_fadd_f64((__attribute__((address_space(1))) double*)p, v);
#else
  *p += v;
#endif
}
// a wave-uniform pointer, stated as such (SGPRs): a buffer descriptor built from VGPRs
// costs a readfirstlane waterfall loop around every buffer instruction
template <typename T>
__device__ __forceinline__ T* uniform_ptr(T* p) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return reinterpret_cast<T*>(((unsigned long long)hi << 32) | lo);
}

// 8-byte write-through store of 4 bf16 / 16-byte sc1 load (buffer ops with the sc1 bit);
// `base` is wave-uniform
__device__ __forceinline__ void st_sc1_b64(bf16* base, long elem, bf16x4 v) {
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(base), 0, 0x7fffffff, 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), rs, (int)(elem * 2), 0, 16);
}
// the same store without sc1 (write-back L2): tensors only a later launch reads
__device__ __forceinline__ void st_wb_b64(bf16* base, long elem, bf16x4 v) {
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(base), 0, 0x7fffffff, 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), rs, (int)(elem * 2), 0, 0);
}
__device__ __forceinline__ void st_sc1_b128(bf16* base, long elem, bf16x8 v) {
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(base), 0, 0x7fffffff, 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, (int)(elem * 2), 0, 16);
}
__device__ __forceinline__ bf16x8 ld_sc1_b128(const bf16* base, long elem) {
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(const_cast<bf16*>(base)), 0,
                                                    0x7fffffff, 0x00020000);
  return __builtin_bit_cast(bf16x8, (u32x4)__builtin_amdgcn_raw_buffer_load_b128(rs, (int)(elem * 2), 0, 16));
}

// Opaque copies of the lane / wave ids: every per-tile address is derived from them
// inside each phase instead of being hoisted to the kernel entry and kept live across
// the whole network (which spilled hundreds of registers).
__device__ __forceinline__ int opaque_v(int v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ int opaque_s(int v) {
  asm volatile("" : "+s"(v));
  return v;
}

// ---- grid barrier ---------------------------------------------------------------------
// Arrival counters sharded over up to PRN_SHARDS cache lines: workgroup b adds to line
// b % shards (8 or 64, prn_shards; with 8, one XCD per line under round-robin placement),
// and the waiters poll all lines with ONE load, one lane per line.  One shared counter serialises its arrivals at the memory side (~12 ns
// each) and its pollers contend with them: microbench/bn_barrier.hip, profiles/bn_barrier.md
// -- a BN barrier (sums, drain, arrive, wait, sums read) at 128 workgroups 3.94 -> 2.72 us,
// at 256 8.85 -> 4.86 us, at 64 2.31 -> 2.07 us.
constexpr int PRN_SHARDS = 64, PRN_LINE = 32;   // (max shards) 32 words = one 128-B line per shard
// bar layout (words): forward shards at PRN_FWD + 32 s, backward shards at PRN_BWD + 32 s,
// the backward readiness count at PRN_READY, the weight-gradient item queue at PRN_QUEUE
// (each on its own line; PRN_BAR_WORDS in all, zeroed every step)
constexpr int PRN_FWD = 0, PRN_BWD = PRN_SHARDS * PRN_LINE, PRN_READY = 2 * PRN_SHARDS * PRN_LINE,
              PRN_QUEUE = PRN_READY + PRN_LINE, PRN_BUCKET = PRN_QUEUE + PRN_LINE,
              PRN_NBUCKET = 3, PRN_BAR_WORDS = PRN_BUCKET + PRN_NBUCKET * PRN_LINE;
constexpr unsigned PRN_BUCKET_RELEASED = 0x40000000u;   // a timed-out launch releases the waiters

// a timed-out wait: flag the error and release the comm stream's bucket waiters (they
// would otherwise wait for counts the exiting workgroups never reach)
__device__ __forceinline__ void prn_fail(unsigned* bar, int* err) {
  __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int b = 0; b < PRN_NBUCKET; ++b)
    __hip_atomic_store(bar + PRN_BUCKET + b * PRN_LINE, PRN_BUCKET_RELEASED, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// Every wave drains its stores / atomics, then lane 0 arrives on its shard.  The caller
// issues its prefetches (waves 1-7) and waits (grid_wait).  This is the arrive of the
// barriers without BN sums in front of them (the forward's pool sums, the backward's last
// publish) and, at 2 and 4 slices per image, of every BN barrier; at one slice per image
// the BN sums arrive themselves (bn_sums_arrive) without this second workgroup barrier.
__device__ __forceinline__ void grid_arrive(unsigned* bar, int shards) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0)
    __hip_atomic_fetch_add(bar + (blockIdx.x % shards) * PRN_LINE, 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// Wait until barrier k (1-based) of `nsl` arriving workgroups is complete: shard s holds
// k x (the arrivers b < nsl with b % 8 == s).  Lanes 0-7 of wave 0 poll their shard every
// 64 clocks.  Returns false when the wait timed out (*err set): the caller exits.
__device__ __forceinline__ bool grid_wait(unsigned* base, int off, unsigned k, unsigned nsl,
                                          int shards, int* err, int* flag) {
  unsigned* bar = base + off;
  if ((int)threadIdx.x < shards) {
    const unsigned sh = threadIdx.x;
    const unsigned target = k * ((nsl + shards - 1 - sh) >> __builtin_ctz(shards));   // (1 or 8)
    const unsigned* p = bar + sh * PRN_LINE;
    const long long t0 = wall_clock64();
    int ok = 1;
    for (;;) {
      const bool done = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target;
      if (__builtin_amdgcn_ballot_w64(!done) == 0) break;   // every shard complete
      __builtin_amdgcn_s_sleep(1);
      if (wall_clock64() - t0 > kSpinTicks) {
        if (sh == 0) prn_fail(base, err);
        ok = 0;
        break;
      }
    }
    if (sh == 0) *flag = ok;
  }
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(*flag) != 0;   // uniform: no divergent region after
}

// Wait until the single counter `ctr` reaches `target` (the weight-gradient workgroups on
// the readiness line; they poll 8x less often: ~190 pollers on one line slow its writer).
template <int SLEEP = 8>
__device__ __forceinline__ bool count_wait(unsigned* base, int off, unsigned target, int* err,
                                           int* flag) {
  if (threadIdx.x == 0) {
    const unsigned* ctr = base + off;
    const long long t0 = wall_clock64();
    int ok = 1;
    while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(SLEEP);
      if (wall_clock64() - t0 > kSpinTicks) {
        prn_fail(base, err);
        ok = 0;
        break;
      }
    }
    *flag = ok;
  }
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(*flag) != 0;
}

// ---- weights: global -> registers (waves 1-7) -> LDS -----------------------------------
struct WLoad {
  const bf16* src;
  int rows, K, KP;      // LDS rows x K (padded row KP; columns [K, KP - 8) zero)
  int dgrad, cin, cout; // dgrad: rows = ci of HWIO [tap][ci][co], k = tap * cout + co
  // unit u -> (row, 16-B column j) without integer division (the shapes are runtime
  // values -- the next block's -- and a 32-bit division by one is ~20 VALU per unit,
  // ~40 % of the forward's VALU): row = (u + 1/2) x (8 / K) in fp32 (exact: u < 2^13 and
  // the quotient's fraction is >= 1/144 away from an integer); cout / 8 is a power of 2
  float inv_upr;
  int cu_shift, ci_shift;   // log2(cout / 8), log2(cin): the dgrad's HWIO offsets as shifts
};
__device__ __forceinline__ int wl_row(const WLoad& L, int u) {
  return (int)(((float)u + 0.5f) * L.inv_upr);
}

// (the thread id is taken opaque in both: otherwise each stage loop hoists the per-thread
// addresses of every weight unit out of its loop and keeps them live across the blocks --
// the backward kernels' VGPR spills)
template <int NR>
__device__ __forceinline__ void w_prefetch(const WLoad& L, bf16x8 (&r)[NR]) {
  const int t = opaque_v((int)threadIdx.x) - 64;
  if (t < 0 || L.src == nullptr) return;
  const int upr = L.K / 8, units = L.rows * upr;
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int u = t + i * (PT - 64);
    if (u < units) {
      int off;   // (< 2^31: weights of <= 64 x 576)
      if (L.dgrad) {   // HWIO [tap][ci = row][co]: ((tap * cin + row) * cout + co
        const int row = wl_row(L, u), j = u - __umul24(row, upr);
        const int tap = j >> L.cu_shift;
        off = ((((tap << L.ci_shift) + row) << L.cu_shift) + (j - (tap << L.cu_shift))) * 8;
      } else {         // rows of K contiguous: unit u is at u x 8
        off = u * 8;
      }
      r[i] = ldg(reinterpret_cast<const bf16x8*>(L.src + off));
    }
  }
}

template <int NR>
__device__ __forceinline__ void w_store(const WLoad& L, const bf16x8 (&r)[NR], bf16* wl) {
  if (L.src == nullptr) return;
  const int tid = opaque_v((int)threadIdx.x), t = tid - 64;
  const int upr = L.K / 8, units = L.rows * upr;
  if (t >= 0) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int u = t + i * (PT - 64);
      if (u < units) {   // row * KP + j * 8 = u * 8 + row * (KP - K)
        const int row = wl_row(L, u);
        *reinterpret_cast<bf16x8*>(wl + u * 8 + __umul24(row, L.KP - L.K)) = r[i];
      }
    }
  }
  const int pad = (L.KP - 8 - L.K) / 8;   // zero columns up to the last k-step (0-3)
  for (int q = tid; q < L.rows * pad; q += PT) {
    const int row = pad == 1 ? q : pad == 2 ? q >> 1 : q / pad, j = upr + (q - row * pad);
    *reinterpret_cast<bf16x8*>(wl + row * L.KP + j * 8) = bf16x8{};
  }
}

// 16-B weight units of a conv, and the prefetch registers waves 1-7 need for them
__host__ __device__ constexpr int conv_units(int co, int ci, int ks) { return co * ks * ks * ci / 8; }
__host__ __device__ constexpr int nreg(int units) { return (units + PT - 65) / (PT - 64); }
__host__ __device__ constexpr int cmax(int a, int b) { return a > b ? a : b; }

__host__ __device__ constexpr int kpad_of(int K) { return ((K + 31) / 32) * 32 + 8; }

__device__ __forceinline__ WLoad wl_fwd(const bf16* src, int co, int ci, int ks) {
  const int K = ks * ks * ci;
  return WLoad{src, co, K, kpad_of(K), 0, ci, co, __frcp_rn((float)(K / 8)), __builtin_ctz(co / 8),
               __builtin_ctz(ci)};
}

// ---- convolutions on the LDS halo ------------------------------------------------------
// acc[t] += sum_k W[channel][k] * Act[k][pixel] over this wave's tiles of output stage SO,
// slice k.  The input halo (CI channels, resolution R_SO * STR, slice rows RS_SO * STR
// plus one halo row above and below) holds image row hi at local row hi - k*RSI + 1.
// Forward (FLIP = false): tap (r, s) of output pixel (h, w) reads input (h*STR + r - PAD,
// w*STR + s - PAD), PAD = 1 for 3x3 (TF fixed padding), 0 for 1x1.
// Stride-1 dgrad (FLIP = true, 3x3): input (h + 1 - r, w + 1 - s) of the output gradient.
// Weights in LDS: [channel][k = tap * CI + ci] rows of KP.
// When the slice has fewer output tiles than waves (stage 3 at 4 slices: 4 tiles), the
// idle waves take half of each tile's k-steps (SPLIT) and their partial sums are added
// through the LDS scratch `xred` (two barriers; every wave calls this function).
template <int SO, int P, int CI, int KSZ, int STR, bool FLIP>
__device__ __forceinline__ void conv_acc(f32x4 (&acc)[8], const bf16* hal, const bf16* wl,
                                         int kslice, int wave, int lane, float* xred) {
  using G = Stg<SO, P>;
  lane = opaque_v(lane);
  constexpr int RI = G::R * STR, RSI = G::RS * STR, W2I = RI + 2, UI = CI >= 8 ? CI / 8 : 1;
  constexpr int K = KSZ * KSZ * CI, KS = (K + 31) / 32, KP = kpad_of(K);
  constexpr int PAD = KSZ == 3 ? 1 : 0;
  constexpr bool SPLIT = !G::ALL && KS >= 4 && NW % G::NT == 0;
  constexpr int WPT = SPLIT ? NW / G::NT : 1;   // waves per tile
  static_assert(!SPLIT || (G::TPW == 1 && G::NT * 256 * (WPT - 1) <= 8 * 128), "split scratch");
  int kh = 0;
  if constexpr (SPLIT) {
    kh = wave / G::NT;
    wave = wave % G::NT;
  } else if (!wave_active<SO, P>(wave)) {
    return;
  }
  const int fr = lane & 15, fq = lane >> 4;
  int hb[G::PBW], hcb[G::PBW];
#pragma unroll
  for (int i = 0; i < G::PBW; ++i) {
    int pb, cb, h, w;
    tile_of<SO, P>(wave, i * G::CBW, pb, cb);
    canon<SO, P>(kslice, pb * 16 + fr, h, w);
    const int lr = FLIP ? h - kslice * RSI + 2 : h * STR - PAD - kslice * RSI + 1;
    hcb[i] = FLIP ? w + 2 : w * STR - PAD + 1;
    hb[i] = lr * W2I + hcb[i];
  }
  int cb0, pb0;
  tile_of<SO, P>(wave, 0, pb0, cb0);
#pragma unroll
  for (int ks = kh; ks < KS; ks += WPT) {
    const int k = ks * 32 + fq * 8;
    int tap = k / CI;
    const int c = k - tap * CI;
    tap = tap < KSZ * KSZ ? tap : KSZ * KSZ - 1;   // padded k: zero weights
    const int tr = FLIP ? -(tap / KSZ) : tap / KSZ;
    const int ts = FLIP ? -(tap % KSZ) : tap % KSZ;
    bf16x8 a[G::CBW];
#pragma unroll
    for (int j = 0; j < G::CBW; ++j) a[j] = lds16(wl + ((cb0 + j) * 16 + fr) * KP + k);
#pragma unroll
    for (int i = 0; i < G::PBW; ++i) {
      const bf16x8 b = lds16(hal + haddr<UI>(hb[i] + tr * W2I + ts, hcb[i] + ts, c));
#pragma unroll
      for (int j = 0; j < G::CBW; ++j) acc[i * G::CBW + j] = mfma16(a[j], b, acc[i * G::CBW + j]);
    }
  }
  if constexpr (SPLIT) {   // partial sums of waves kh > 0 -> the tile's kh = 0 wave
    if (kh > 0) *reinterpret_cast<f32x4*>(xred + ((kh - 1) * G::NT + wave) * 256 + lane * 4) = acc[0];
    __syncthreads();
    if (kh == 0) {
#pragma unroll
      for (int j = 1; j < WPT; ++j)
        acc[0] += *reinterpret_cast<const f32x4*>(xred + ((j - 1) * G::NT + wave) * 256 + lane * 4);
    }
    __syncthreads();   // (xred is the BN sums' scratch next)
  }
}

// ---- register tensors (bf16x4 per tile: 4 channels of one pixel) ------------------------
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[8]) {
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// image NHWC element offset of this lane's tile-t values
template <int S, int P>
__device__ __forceinline__ int gofs(int kslice, int wave, int lane, int t) {
  using G = Stg<S, P>;
  int pb, cb, h, w;
  tile_of<S, P>(wave, t, pb, cb);
  canon<S, P>(kslice, pb * 16 + (lane & 15), h, w);
  return (h * G::R + w) * G::C + cb * 16 + 4 * (lane >> 4);
}

template <int S, int P>
__device__ __forceinline__ void load_regs(bf16x4 (&v)[8], const bf16* img_base, int kslice,
                                          int wave, int lane) {
  lane = opaque_v(lane);
  if (!wave_active<S, P>(wave)) return;
#pragma unroll
  for (int t = 0; t < Stg<S, P>::TPW; ++t)
    v[t] = ldg(reinterpret_cast<const bf16x4*>(img_base + gofs<S, P>(kslice, wave, lane, t)));
}

// write-through (sc1) stores: these tensors are read by other workgroups in the launch.
// ROWS 1: only the slice's first and last rows (what the neighbouring slices read inside
// the launch), 2: only the rows between them, 0: all.  WB: write-back stores instead (the
// forward's saved tensors past the border rows: only the backward launch reads them).
template <int S, int P, int ROWS = 0, bool WB = false>
__device__ __forceinline__ void publish(const bf16x4 (&v)[8], bf16* img_base, int kslice,
                                        int wave, int lane) {
  using G = Stg<S, P>;
  lane = opaque_v(lane);
  if (!wave_active<S, P>(wave)) return;
#pragma unroll
  for (int t = 0; t < G::TPW; ++t) {
    int pb, cb, h, w;
    tile_of<S, P>(wave, t, pb, cb);
    canon<S, P>(kslice, pb * 16 + (lane & 15), h, w);
    const int lr = h - kslice * G::RS;
    const bool border = lr == 0 || lr == G::RS - 1;
    if (ROWS == 0 || (ROWS == 1) == border) {
      if constexpr (WB) st_wb_b64(img_base, (h * G::R + w) * G::C + cb * 16 + 4 * (lane >> 4), v[t]);
      else st_sc1_b64(img_base, (h * G::R + w) * G::C + cb * 16 + 4 * (lane >> 4), v[t]);
    }
  }
}

// ---- halos -------------------------------------------------------------------------------
// Neighbour halo rows: 2 rows x R pixels x U units (always 128 units) -- thread t < 128
// handles unit t: row sel = t / (R U) (0: image row k*RS - 1, 1: row (k+1)*RS), column,
// unit.  `ok` is false outside the image (the conv's zero padding).
template <int S, int P>
struct Nbr {
  static constexpr int UNITS = 2 * Stg<S, P>::R * Stg<S, P>::U;
  static_assert(UNITS <= PT, "neighbour units");
  int sel, col, u, gofs;   // gofs: image element offset of the unit
  bool ok;
  __device__ __forceinline__ Nbr(int kslice) {
    using G = Stg<S, P>;
    const int t = threadIdx.x;
    sel = t / (G::R * G::U);
    const int rem = t - sel * G::R * G::U;
    col = rem / G::U;
    u = rem - col * G::U;
    const int gr = sel ? (kslice + 1) * G::RS : kslice * G::RS - 1;
    ok = t < UNITS && gr >= 0 && gr < G::R;
    gofs = (gr * G::R + col) * G::C + u * 8;
  }
};

// own values (this wave's tiles; MODE 1: BN + ReLU with the LDS table sc/sh, 0: as is)
// -> halo rows 1..RS; the neighbour units `nv` (already transformed; zero where !ok)
// -> rows 0 and RS + 1; the left / right border columns -> zero
template <int S, int P, int MODE>
__device__ __forceinline__ void to_halo(bf16* hal, const bf16x4 (&v)[8], const float* sc,
                                        const float* sh, const Nbr<S, P>& nb, bf16x8 nv,
                                        int kslice, int wave, int lane) {
  using G = Stg<S, P>;
  lane = opaque_v(lane);
  const int fr = lane & 15, fq = lane >> 4;
  if (wave_active<S, P>(wave)) {
    // (MODE 1) this lane's 4 channels of each of the wave's channel blocks, read once: the
    // halo stores below may alias the table for the compiler, which re-read it per tile
    f32x4 scv[G::CBW], shv[G::CBW];
    if constexpr (MODE == 1) {
#pragma unroll
      for (int j = 0; j < G::CBW; ++j) {
        int pb, cb;
        tile_of<S, P>(wave, j, pb, cb);
        scv[j] = *reinterpret_cast<const f32x4*>(sc + cb * 16 + 4 * fq);
        shv[j] = *reinterpret_cast<const f32x4*>(sh + cb * 16 + 4 * fq);
      }
    }
#pragma unroll
    for (int t = 0; t < G::TPW; ++t) {
      int pb, cb, h, w;
      tile_of<S, P>(wave, t, pb, cb);
      canon<S, P>(kslice, pb * 16 + fr, h, w);
      const int c0 = cb * 16 + 4 * fq;
      bf16x4 o = v[t];
      if constexpr (MODE == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          o[r] = (bf16)fmaxf((float)v[t][r] * scv[t % G::CBW][r] + shv[t % G::CBW][r], 0.f);
      }
      const int lr = h - kslice * G::RS + 1;
      *reinterpret_cast<bf16x4*>(hal + haddr<G::U>(lr * G::W2 + w + 1, w + 1, c0)) = o;
    }
  }
  if ((int)threadIdx.x < Nbr<S, P>::UNITS) {
    const int lr = nb.sel ? G::RS + 1 : 0, lc = nb.col + 1;
    *reinterpret_cast<bf16x8*>(hal + haddr<G::U>(lr * G::W2 + lc, lc, nb.u * 8)) = nb.ok ? nv : bf16x8{};
  }
  // left / right border columns of every halo row
  for (int q = threadIdx.x; q < 2 * G::HR * G::U; q += PT) {
    const int b = q / G::U, u = q - b * G::U;
    const int lr = b >> 1, lc = (b & 1) ? G::R + 1 : 0;
    *reinterpret_cast<bf16x8*>(hal + haddr<G::U>(lr * G::W2 + lc, lc, u * 8)) = bf16x8{};
  }
}

// Sum over the 16 lanes of a DPP row (the 16 pixel lanes of an MFMA fragment): quad
// swaps, then the half-row and row mirrors -- VALU-latency DPP moves instead of the
// LDS-latency ds_bpermute chain __shfl_xor compiles to.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);   // row_half_mirror
  v += dpp_mov<0x140>(v);   // row_mirror
  return v;
}
// row16_sum of N independent values, level by level: each value goes through the same
// four adds in the same order, but the N chains are written interleaved, so a level's
// DPP moves issue back to back instead of every value waiting out its own four-deep chain
template <int N>
__device__ __forceinline__ void row16_sum_n(float (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_mov<0xB1>(v[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_mov<0x4E>(v[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_mov<0x141>(v[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_mov<0x140>(v[i]);
}

// fp64 accumulator replicas per BatchNorm of the persistent kernels (the per-layer
// kernels use BN_ACC_REP; the engine sizes every BN's block for the larger count).  Each
// workgroup adds into replica blockIdx % REP; after the barrier every workgroup reads all
// REP replicas of its channels.  Same-box A/B, step ms bs128 / bs16
// (profiles/cifar_persist_variants.md): 1 replica 1.058 / 0.657 (same-address atomics
// serialise), 2: 0.887 / 0.594, 4: 0.850 / 0.595, 8: 0.862 / 0.597, 16: 0.879 / 0.627
// (the combine's reads grow).
constexpr int PRN_ACC_REP = 4;

// Per-channel sums over this slice of two per-value quantities f(t, r, x1, x2), added to
// a BN's fp64 accumulator replicas acc [PRN_ACC_REP][2][C] (memory-side atomics; exact, so
// order-independent); the caller follows it with the workgroup's arrive at the grid
// barrier, bn_sums_arrive (a probe stamp may stand between the two).
// The fp32 addition tree is fixed (the step's outputs are bitwise reproducible across
// builds): per thread over its tiles with equal t % CBW in ascending t; over the 16 pixel
// lanes in row16_sum's order; over the waves that hold the channel in ascending wave
// order from 0.f.
//   * the 2 CBW 4 lane-sum chains run interleaved (row16_sum_n);
//   * lanes fr == 0 write their 4 consecutive channels of a sum as one 16-byte LDS store
//     into `red` [8 waves][128]: a wave's row holds sum 1 of channel c at c and sum 2 at
//     C + c (the four fq lanes of a store cover 64 contiguous bytes: no bank conflict);
//   * after ONE workgroup barrier, lane i < 2C of wave 0 folds entry i over the waves
//     (C = 64: lane c folds c and 64 + c, so that wave 0 alone holds every atomic): the
//     chain's LDS loads are all issued before its adds, then one fp64 atomic per entry.
// The hand-off to the arrive.  At one slice per image (P = 1) no wave has stored anything
// since the last arrive that it has not had a whole phase to complete (the forward's
// saved tensors and the backward's dout / dh1 go out right after the previous arrive), so
// every wave drains (s_waitcnt vmcnt(0)) BEFORE the one workgroup barrier; after it only
// wave 0 has global operations in flight -- the atomics -- and it drains itself and its
// lane 0 adds to the barrier counter: the protocol's order (all of the workgroup's stores
// and atomics complete, then the counter add) holds without the second workgroup barrier
// of grid_arrive, and waves 1-7 go on to their prefetches while wave 0 folds.  `red` is
// safe to reuse: its next writer (the next sums, a split conv's partials, the pool sums)
// runs after the grid_wait that follows, whose __syncthreads wave 0 joins only after its
// fold's reads.  At P > 1 every wave's border-row publish is issued right before the
// sums; draining it in front of the workgroup barrier would expose its round trip, so the
// sums are followed by grid_arrive (drain, barrier, add).
template <int S, int P, typename F>
__device__ __forceinline__ void bn_sums(F f, float* red, double* acc, int wave, int lane) {
  using G = Stg<S, P>;
  constexpr int C = G::C;
  constexpr int SPT = 2 * C > 64 ? 2 : 1, NTH = 2 * C / SPT;   // entries per lane, lanes
  constexpr int NCH = NW / G::WPB;                              // waves per channel
  constexpr bool SELF = P == 1;                                 // wave 0 arrives by itself
  lane = opaque_v(lane);
  const int fr = lane & 15, fq = lane >> 4;
  if (wave_active<S, P>(wave)) {
    float s[2 * G::CBW * 4];   // [sum][channel block j][r]
#pragma unroll
    for (int i = 0; i < 2 * G::CBW * 4; ++i) s[i] = 0.f;
#pragma unroll
    for (int t = 0; t < G::TPW; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float a, b;
        f(t, r, a, b);
        s[(t % G::CBW) * 4 + r] += a;
        s[(G::CBW + t % G::CBW) * 4 + r] += b;
      }
    row16_sum_n(s);
    if (fr == 0) {
      int pb, cb0;
      tile_of<S, P>(wave, 0, pb, cb0);
#pragma unroll
      for (int j = 0; j < G::CBW; ++j) {
        float* q = red + wave * 128 + (cb0 + j) * 16 + 4 * fq;
        *reinterpret_cast<f32x4*>(q) = f32x4{s[j * 4], s[j * 4 + 1], s[j * 4 + 2], s[j * 4 + 3]};
        *reinterpret_cast<f32x4*>(q + C) = f32x4{s[(G::CBW + j) * 4], s[(G::CBW + j) * 4 + 1],
                                                 s[(G::CBW + j) * 4 + 2], s[(G::CBW + j) * 4 + 3]};
      }
    }
  }
  if constexpr (SELF) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x < NTH) {
    float ld[SPT][NCH];
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
      const int i = threadIdx.x + k * NTH;
      const int grp = ((i & (C - 1)) / 16) / G::CBW;   // waves w with w % WPB == grp hold the channel
#pragma unroll
      for (int q = 0; q < NCH; ++q) ld[k][q] = red[(grp + q * G::WPB) * 128 + i];
    }
    double* p = acc + (long)(blockIdx.x % PRN_ACC_REP) * 2 * C + threadIdx.x;
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
      float v = 0.f;
#pragma unroll
      for (int q = 0; q < NCH; ++q) v += ld[k][q];
      atomic_add_g(p + k * NTH, (double)v);
    }
  }
}

// the arrive after bn_sums (see there): at P = 1 wave 0 alone, no workgroup barrier
template <int P>
__device__ __forceinline__ void bn_sums_arrive(unsigned* bar, int shards, int wave) {
  if constexpr (P == 1) {
    if (wave == 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (threadIdx.x == 0)
        __hip_atomic_fetch_add(bar + (blockIdx.x % shards) * PRN_LINE, 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
  } else {
    grid_arrive(bar, shards);
  }
}

// After the barrier: the channel's two sums from the PRN_ACC_REP replicas (sc1 loads,
// replicas added in a fixed order)
__device__ __forceinline__ void acc_read(const double* acc, int C, int c, double& s1, double& s2) {
  double a[PRN_ACC_REP], b[PRN_ACC_REP];
#pragma unroll
  for (int r = 0; r < PRN_ACC_REP; ++r) {
    a[r] = ld_sc1_d(acc + (long)r * 2 * C + c);
    b[r] = ld_sc1_d(acc + (long)r * 2 * C + C + c);
  }
  s1 = s2 = 0.0;
#pragma unroll
  for (int r = 0; r < PRN_ACC_REP; ++r) {
    s1 += a[r];
    s2 += b[r];
  }
}

// BN parameters prefetched into registers (thread c < C) before a barrier wait
struct BnRegs {
  float g, b, mean, rstd, scale, shift, mm, mv;
};
// (workgroup 0 also updates the moving averages: their old values are prefetched too,
// or its read-modify-write would put a memory round trip in front of its next arrive --
// and every workgroup waits for that one)
__device__ __forceinline__ void bn_prefetch_fwd(const PrnBn& bn, int C, BnRegs& r) {
  const int c = threadIdx.x;
  if (c < C) {
    r.g = ldg(bn.gamma + c);
    r.b = ldg(bn.beta + c);
    if (blockIdx.x == 0) {
      r.mm = ldg(bn.mmean + c);
      r.mv = ldg(bn.mvar + c);
    }
  }
}

// forward BN: sums -> scale/shift/mean/rstd table [4][64] in LDS; workgroup 0 publishes the
// batch statistics and updates the moving averages (TF FusedBatchNorm, bn_fused.h).
// Ends with a barrier.
__device__ __forceinline__ void bn_fwd_table(const PrnBn& bn, const BnRegs& pr, int C, double M,
                                             float eps, float momentum, int update_moving,
                                             float* tbl) {
  const int c = threadIdx.x;
  if (c < C) {
    double s1, s2;
    acc_read(bn.acc, C, c, s1, s2);
    const double dm = s1 / M;
    const double var = fmax(s2 / M - dm * dm, 0.0);
    const float fmu = (float)dm, fvar = (float)var;
    const float rs = rsqrtf(fvar + eps);
    const float sc = pr.g * rs;
    const float sh = pr.b - fmu * sc;
    tbl[c] = sc;
    tbl[64 + c] = sh;
    tbl[128 + c] = fmu;
    tbl[192 + c] = rs;
    if (blockIdx.x == 0) {
      stg(bn.mean + c, fmu);
      stg(bn.rstd + c, rs);
      stg(bn.scale + c, sc);
      stg(bn.shift + c, sh);
      if (update_moving) {
        const float uvar = M > 1.0 ? (float)(var * M / (M - 1.0)) : fvar;
        const float mm = pr.mm, mv = pr.mv;
        stg(bn.mmean + c, mm - (1.f - momentum) * (mm - fmu));
        stg(bn.mvar + c, mv - (1.f - momentum) * (mv - uvar));
      }
    }
  }
  __syncthreads();
}

// ---- LDS carve-up (bytes) ------------------------------------------------------------
constexpr int HALO_B = (32 + 2) * 34 * 16 * 2;            // P = 1: the whole 32x32x16 map
constexpr int W1_B = 64 * kpad_of(576) * 2;               // 64 rows x 9*64 (+pad)
constexpr int W2_B = 64 * kpad_of(32) * 2;                // projection (64 x 32 fwd / 32 x 64 dgrad)
constexpr int TBL_B = 7 * 64 * 4;
constexpr int RED_B = 8 * 128 * 4;
constexpr int MISC_B = 256;
constexpr int OFF_HA = 0, OFF_HB = OFF_HA + HALO_B, OFF_W1 = OFF_HB + HALO_B,
              OFF_W2 = OFF_W1 + W1_B, OFF_TBL = OFF_W2 + W2_B, OFF_TBL2 = OFF_TBL + TBL_B,
              OFF_RED = OFF_TBL2 + TBL_B, OFF_MISC = OFF_RED + RED_B,
              LDS_TOTAL = OFF_MISC + MISC_B;
static_assert(LDS_TOTAL <= 163840, "LDS");

struct Smem {
  bf16 *ha, *hb, *w1, *w2;
  float *tbl, *tbl2, *red;
  int* flag;
};
__device__ __forceinline__ Smem carve(char* s) {
  Smem m;
  m.ha = reinterpret_cast<bf16*>(s + OFF_HA);
  m.hb = reinterpret_cast<bf16*>(s + OFF_HB);
  m.w1 = reinterpret_cast<bf16*>(s + OFF_W1);
  m.w2 = reinterpret_cast<bf16*>(s + OFF_W2);
  m.tbl = reinterpret_cast<float*>(s + OFF_TBL);
  m.tbl2 = reinterpret_cast<float*>(s + OFF_TBL2);
  m.red = reinterpret_cast<float*>(s + OFF_RED);
  m.flag = reinterpret_cast<int*>(s + OFF_MISC);
  return m;
}

// round accumulators (+ optional bf16 residual) to bf16 registers
template <int S, int P, bool RES>
__device__ __forceinline__ void round_acc(bf16x4 (&o)[8], const f32x4 (&acc)[8], const bf16x4 (&res)[8]) {
#pragma unroll
  for (int t = 0; t < Stg<S, P>::TPW; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) o[t][r] = (bf16)(RES ? acc[t][r] + (float)res[t][r] : acc[t][r]);
}

template <int S_, int STR_, bool PROJ_>
struct BlkTag {
  static constexpr int S = S_, STR = STR_;
  static constexpr bool PROJ = PROJ_;
};

struct Ctx {
  const PrnArgs* a;
  Smem m;
  int img, kslice, wave, lane;
  unsigned nbar;     // barriers passed
  unsigned slices;   // barrier arrivals per barrier (N x P)
  int pc;            // probe stamps written
  BnRegs bnr;        // prefetched BN parameters of the next combine
  BnRegs ftr;        // backward: prefetched forward table of the next BN-backward sums
  unsigned* mark;    // overlap mode, workgroup 0: bucket line its next arrive counts on
};

// diagnostics: workgroup 0's lane 0 records (tag, wall clock) pairs (prn_set_probe)
__device__ __forceinline__ void probe(Ctx& x, int tag) {
  if (x.a->probe != nullptr) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      x.a->probe[2 * x.pc] = tag;
      x.a->probe[2 * x.pc + 1] = wall_clock64();
    }
    ++x.pc;
  }
}

// prefetch registers for the next block's conv1 after a stage-S block (stage S or S+1)
template <int S>
__host__ __device__ constexpr int nreg_next_fwd() {
  return S < 2 ? cmax(nreg(conv_units(16 << S, 16 << S, 3)), nreg(conv_units(32 << S, 16 << S, 3)))
               : nreg(conv_units(64, 64, 3));
}

// =====================================================================================
// pieces the training forward and the inference forward share
// =====================================================================================
// a 16-byte load in the calling kernel's flavour: the training forward dereferences, the
// inference forward loads through the global address space (ldg)
template <bool LDG>
__device__ __forceinline__ bf16x8 ld_b128(const bf16* p) {
  if constexpr (LDG) return ldg(reinterpret_cast<const bf16x8*>(p));
  else return *reinterpret_cast<const bf16x8*>(p);
}

// Stem operands (3x3 8 -> 16 on the 32x32 image, no BN before it): slice `kslice`'s rows
// of image `img` of a.x_in plus one halo row above and below, straight from the input ->
// halo `ha` (34 wide, zero outside the image); a.stem_w -> `w1` in rows of kpad_of(72).
// No barrier: the caller's next __syncthreads publishes both.  (Takes the kernel's argument
// struct, PrnArgs or PrnInferArgs, not the two pointers: handed the pointers, the compiler
// emitted the weight fill's `j < 9` branch differently from the code written in place.)
template <int P, bool LDG, class Args>
__device__ __forceinline__ void stem_fill(const Args& a, int img, bf16* ha, bf16* w1, int kslice) {
  using G0 = Stg<0, P>;
  const int tid = threadIdx.x;
  const bf16* src = a.x_in + (long)img * 1024 * 8;
  for (int q = tid; q < G0::HR * 34; q += PT) {
    const int lr = q / 34, lc = q - lr * 34;
    const int gr = kslice * G0::RS + lr - 1, gc = lc - 1;
    bf16x8 v = {};
    if (gr >= 0 && gr < 32 && gc >= 0 && gc < 32) v = ld_b128<LDG>(src + (gr * 32 + gc) * 8);
    *reinterpret_cast<bf16x8*>(ha + q * 8) = v;
  }
  constexpr int SKP = kpad_of(72);
  for (int q = tid; q < 16 * (SKP / 8); q += PT) {
    const int row = q / (SKP / 8), j = q - row * (SKP / 8);
    bf16x8 v = {};
    if (j < 9) v = ld_b128<LDG>(a.stem_w + row * 72 + j * 8);
    *reinterpret_cast<bf16x8*>(w1 + row * SKP + j * 8) = v;
  }
}

// Final BN + ReLU (table tbl: scale, shift) of the last block's output in registers and
// this slice's average-pool sums: every active wave's per-channel sums over its pixels
// into `red` [8 waves][128], a barrier, then thread c < 64 adds the waves that hold
// channel c in a fixed order.  Returns that sum (threads 64 and up: 0).
template <int P>
__device__ __forceinline__ float pool_sums(const bf16x4 (&xr)[8], const float* tbl, float* red,
                                           int wave_, int lane_) {
  using G2 = Stg<2, P>;
  const int wave = opaque_s(wave_), lane = opaque_v(lane_);
  if (wave_active<2, P>(wave)) {
    float s[G2::CBW][4];
#pragma unroll
    for (int j = 0; j < G2::CBW; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) s[j][r] = 0.f;
#pragma unroll
    for (int t = 0; t < G2::TPW; ++t) {
      int pb, cb;
      tile_of<2, P>(wave, t, pb, cb);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = cb * 16 + 4 * (lane >> 4) + r;
        s[t % G2::CBW][r] += fmaxf((float)xr[t][r] * tbl[c] + tbl[64 + c], 0.f);
      }
    }
#pragma unroll
    for (int j = 0; j < G2::CBW; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) s[j][r] = row16_sum(s[j][r]);
    if ((lane & 15) == 0) {
      int pb, cb0;
      tile_of<2, P>(wave, 0, pb, cb0);
#pragma unroll
      for (int j = 0; j < G2::CBW; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave * 128 + (cb0 + j) * 16 + 4 * (lane >> 4) + r] = s[j][r];
    }
  }
  __syncthreads();
  const int c = threadIdx.x;
  float v = 0.f;
  if (c < 64) {
    const int grp = (c / 16) / G2::CBW;   // waves w with w % WPB == grp hold channel c
#pragma unroll
    for (int w = 0; w < NW; ++w)
      if (w % G2::WPB == grp) v += red[w * 128 + c];
  }
  return v;
}

}  // namespace

// ---- host: shared between the translation units ----------------------------------------
// (internal to the prn_*.hip files: not part of kernels.h's public surface, not to be bound)
extern long long* g_prn_probe;      // prn_set_probe (prn_fwd.hip)
int prn_shards(int N, int P);       // arrival shards of a launch (prn_fwd.hip)
// workgroups of prn_fwd_kernel<P> / prn_bwd_kernel<P> the device keeps resident at once
// (-1: the occupancy query failed); each in its kernel's own translation unit
long prn_fwd_resident(int P);
long prn_bwd_resident(int P);

// workgroups of `kern` (PT threads, `lds` bytes) the device keeps resident at once
template <typename K>
static long resident_blocks(K kern, size_t lds) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, PT, lds) != hipSuccess) return -1;
  return (long)per_cu * cu_count();
}

}  // namespace dtr
