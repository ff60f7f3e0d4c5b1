// Muon's Newton-Schulz iteration (muon.hip's header: the same formulas and the same roundings)
// for the matrices one workgroup cannot hold: a short side s <= 1024 and a long side l <= 8192
// (muon_tiled_covers), every conv kernel of the ImageNet networks.  The operands live in a bf16
// device scratch -- per tensor X[SP][LP] (short x long, the long side contiguous), A[SP][SP] and
// B[SP][SP], SP and LP the sides rounded up to 64 -- and stay in L2 between the launches.  Every
// launch is grouped over all tiled tensors of the network and driven by a host-built work table
// (MuonWork, one record per workgroup, the longest reduction first); a kernel boundary is the
// only synchronisation between phases.  No grid barrier, no co-residency, no float atomic and
// no split-K: every output element is the sum of one workgroup in one order, so two launches
// and two ranks give the same bits.  3 + 3 * steps launches:
//   muon_tiled_moments   one workgroup per 4096-element chunk of a tensor (chunk_span): m' =
//                        mu m + s g in place, the chunk's sum of u^2 (fp32 per thread, fp64
//                        from the wave on: block_sum_f64) into part[chunk].
//   muon_tiled_stage     one workgroup per 64 x 64 tile of X, padding tiles included: adds the
//                        tensor's partials in chunk order (every workgroup of a tensor forms the
//                        same den), forms u again from g and the stored m' and writes X0 =
//                        bf16(u / den), zero where the tile leaves the tensor.  The tile goes
//                        through LDS: the fp32 rows of M are read along their contiguous side
//                        (4 bytes per lane, 256 per wave: a tensor's offset need not be 16-byte
//                        aligned) and X is written in 16-byte row pieces, transposed or not.
//   muon_tiled_syrk<EPI> C = epi(P P^T) for the upper triangle of 64 x 64 tiles; P = X
//                        (reduction LP) gives A = bf16(acc), P = A (reduction SP; A is
//                        symmetric, so A A = A A^T) gives B = bf16(b A + c acc).  Both operands
//                        are rows of P with the reduction contiguous: 16-byte global loads into
//                        registers one k-tile ahead, then into the other of two LDS stages; one
//                        LDS barrier per k-tile.  An LDS row is 64 + 8 elements = 36 dwords =
//                        16 * 2 + 4, so the 16 rows of an MFMA operand start on the 16 different
//                        4-bank groups and a 16-byte read per lane has no conflict (unpadded,
//                        32 dwords: all rows on one group).  Four waves, 32 x 32 each: four
//                        operand reads per four MFMAs.  The tile is stored twice, as it lies
//                        and mirrored (the diagonal tiles once): A[i][j] and A[j][i] are the
//                        same bits.  Both stores go through LDS -- the accumulator's four rows
//                        of one column are 2-byte stores into T and ONE 8-byte store into the
//                        transposed TT -- so both are 16-byte row stores.
//   muon_tiled_apply     X = bf16(a X + B X) in place on ONE copy of X.  A workgroup owns BN
//                        long-side columns (64 up to SP = 512, 32 above) for ALL SP rows: it
//                        loads its SP x BN panel into LDS once, and a barrier stands between
//                        that load and its first store; no workgroup reads what another writes.
//                        B's 64 x 64 tiles stream from L2 through two LDS stages as in syrk.
//                        The panel is long-side contiguous, so the MFMA's B operand (reduction
//                        along the short side) comes from ds_read_b64_tr_b16, two reads per
//                        fragment (conv_wgrad_direct.hip's scheme): lane group g gets the short
//                        rows 4 g .. 4 g + 3 and 16 + 4 g .. 16 + 4 g + 3 of a 32-row k-step,
//                        and B's fragment is read as the same two 4-element pieces.  A panel
//                        row is BN + 16 elements = 40 or 24 dwords = 8 (odd): the eight rows a
//                        half-wave reads (32 bytes each) start 8 banks apart mod 64 -- all 64
//                        banks once.  Results leave through an LDS tile as 16-byte row pieces.
//   muon_tiled_unstage   stage's tile walk backwards: X as fp32 into dir in M's orientation,
//                        the tensor's own elements only.
// Zero padding: stage writes every element of X[SP][LP]; syrk writes every tile of A and B.
// Zero rows and columns stay zero through the iteration, so the GEMM kernels have no edge
// code.  profiles/muon_tiled.md has the resource summary and the measurements.
#include "muon_device.h"

namespace dtr {

constexpr int MT = MUON_TILE;          // 64
constexpr int MT_LD = MT + 8;          // LDS row of a 64-wide bf16 tile
constexpr int MT_THREADS = 256;
constexpr int MT_XPAD = 16;            // padding of a panel row in apply

bool muon_tiled_covers(int R, int K) {
  const int s = R < K ? R : K, l = R < K ? K : R;
  return s >= 1 && s <= MUON_TILED_SHORT && l <= MUON_TILED_LONG;
}

static int apply_bn(int SP) { return SP <= 512 ? 64 : 32; }

static int apply_lds_of(int SP) {
  const int XS = apply_bn(SP) + MT_XPAD;
  return (SP * XS + 2 * MT * MT_LD + MT * XS) * 2;
}

// (a table that reaches past 512 may hold a 512 too, whose wider panel can be the larger)
int muon_tiled_apply_lds(int max_sp) {
  const int own = apply_lds_of(max_sp), wide = apply_lds_of(512);
  return max_sp > 512 && wide > own ? wide : own;
}
static_assert((1024 * (32 + MT_XPAD) + 2 * MT * MT_LD + MT * (32 + MT_XPAD)) * 2 <= 163840, "LDS");

// ------------------------------------------------------------------------------- moments
__global__ void __launch_bounds__(MT_THREADS)
muon_tiled_moments_kernel(const float* __restrict__ g, float* __restrict__ m,
                          const MuonTiledTensor* __restrict__ tab, const int* __restrict__ blk_t,
                          double* __restrict__ part, float mu, int nesterov, float scale) {
  const int tid = threadIdx.x;
  const MuonTiledTensor t = tab[blk_t[blockIdx.x]];
  const ChunkSpan ch = chunk_span(t.offset, (long long)t.R * t.K,
                                  (long long)blockIdx.x - t.chunk0, LARS_CHUNK);
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {                   // nvec <= 4 * 256
    const int k = tid + j * MT_THREADS;
    if (k < ch.nvec) {
      const long long e = ch.body0 + 4ll * k;
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + e);
      f32x4 mv = *reinterpret_cast<const f32x4*>(m + e);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float mj = mv[i], u;
        muon_moment(gv[i], mj, scale, mu, nesterov, u);
        mv[i] = mj;
        ss += u * u;
      }
      *reinterpret_cast<f32x4*>(m + e) = mv;
    }
  }
  if (tid < ch.head + ch.tail) {
    const long long e = tid < ch.head ? ch.start + tid : ch.tail0 + (tid - ch.head);
    float mj = m[e], u;
    muon_moment(g[e], mj, scale, mu, nesterov, u);
    m[e] = mj;
    ss += u * u;
  }
  block_sum_f64<1>({ss}, part);
}

void muon_tiled_moments(const float* grad, float* mom, const MuonTiledTensor* tab,
                        const int* blk_t, int nblocks, double* part, float momentum,
                        int nesterov, float grad_scale, hipStream_t st) {
  if (nblocks <= 0) return;
  hipLaunchKernelGGL(muon_tiled_moments_kernel, dim3((unsigned)nblocks), dim3(MT_THREADS), 0, st,
                     grad, mom, tab, blk_t, part, momentum, nesterov, grad_scale);
  DTR_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------ stage / unstage
// The tile walk both share: thread (tx, ty) visits 16 elements of the tile, tx along M's
// contiguous side.  il, cl: the element's short and long index inside the tile; e: its index
// in M, or -1 outside the tensor.
struct TileWalk {
  int tx, ty, i0, c0, R, K, tr;
  __device__ __forceinline__ TileWalk(const MuonTiledTensor& t, const MuonWork& w)
      : tx(threadIdx.x & 63), ty(threadIdx.x >> 6), i0(w.i * MT), c0(w.j * MT), R(t.R), K(t.K),
        tr(t.transpose) {}
  __device__ __forceinline__ int at(int it, int& il, int& cl) const {
    const int other = ty + 4 * it;
    il = tr ? tx : other;
    cl = tr ? other : tx;
    const int r = tr ? c0 + cl : i0 + il, k = tr ? i0 + il : c0 + cl;
    return r < R && k < K ? r * K + k : -1;
  }
};

__global__ void __launch_bounds__(MT_THREADS)
muon_tiled_stage_kernel(const float* __restrict__ grad, const float* __restrict__ mom,
                        const MuonTiledTensor* __restrict__ tab,
                        const MuonWork* __restrict__ work, const double* __restrict__ part,
                        bf16* __restrict__ scratch, float mu, int nesterov, float scale) {
  __shared__ __attribute__((aligned(16))) bf16 T[MT * MT_LD];
  __shared__ double sh[MT_THREADS];
  __shared__ float den_s;
  const int tid = threadIdx.x;
  const MuonWork w = work[blockIdx.x];
  const MuonTiledTensor t = tab[w.t];
  // the tensor's partials in chunk order, by one lane
  double tot = 0.0;
  for (int c0 = 0; c0 < t.nchunks; c0 += MT_THREADS) {
    if (c0 + tid < t.nchunks) sh[tid] = part[t.chunk0 + c0 + tid];
    __syncthreads();
    if (tid == 0) {
      const int n = min(MT_THREADS, t.nchunks - c0);
      for (int j = 0; j < n; ++j) tot += sh[j];
    }
    __syncthreads();
  }
  if (tid == 0) den_s = sqrtf((float)tot) + 1e-7f;
  __syncthreads();
  const float den = den_s;
  const float* __restrict__ g = grad + t.offset;
  const float* __restrict__ m = mom + t.offset;
  const TileWalk walk(t, w);
#pragma unroll 4
  for (int it = 0; it < 16; ++it) {
    int il, cl;
    const int e = walk.at(it, il, cl);
    float x = 0.f;
    if (e >= 0) {
      const float mj = m[e];
      float u = mj;
      if (nesterov) {
#pragma clang fp contract(off)
        const float gp = scale * g[e];
        const float tt = mu * mj;
        u = gp + tt;
      }
      x = u / den;
    }
    T[il * MT_LD + cl] = (bf16)x;
  }
  lds_barrier();
  bf16* __restrict__ X = scratch + t.x_off;
  for (int q = tid; q < MT * 8; q += MT_THREADS) {
    const int row = q >> 3, c8 = (q & 7) * 8;
    *reinterpret_cast<f32x4*>(X + (long long)(w.i * MT + row) * t.LP + w.j * MT + c8) =
        *reinterpret_cast<const f32x4*>(T + row * MT_LD + c8);
  }
}

void muon_tiled_stage(const float* grad, const float* mom, const MuonTiledTensor* tab,
                      const MuonWork* work, int nwork, const double* part, bf16* scratch,
                      float momentum, int nesterov, float grad_scale, hipStream_t st) {
  if (nwork <= 0) return;
  hipLaunchKernelGGL(muon_tiled_stage_kernel, dim3((unsigned)nwork), dim3(MT_THREADS), 0, st,
                     grad, mom, tab, work, part, scratch, momentum, nesterov, grad_scale);
  DTR_CHECK_LAUNCH();
}

__global__ void __launch_bounds__(MT_THREADS)
muon_tiled_unstage_kernel(const bf16* __restrict__ scratch, float* __restrict__ dir,
                          const MuonTiledTensor* __restrict__ tab,
                          const MuonWork* __restrict__ work) {
  __shared__ __attribute__((aligned(16))) bf16 T[MT * MT_LD];
  const int tid = threadIdx.x;
  const MuonWork w = work[blockIdx.x];
  const MuonTiledTensor t = tab[w.t];
  const bf16* __restrict__ X = scratch + t.x_off;
  for (int q = tid; q < MT * 8; q += MT_THREADS) {
    const int row = q >> 3, c8 = (q & 7) * 8;
    *reinterpret_cast<f32x4*>(T + row * MT_LD + c8) =
        *reinterpret_cast<const f32x4*>(X + (long long)(w.i * MT + row) * t.LP + w.j * MT + c8);
  }
  lds_barrier();
  float* __restrict__ o = dir + t.offset;
  const TileWalk walk(t, w);
#pragma unroll 4
  for (int it = 0; it < 16; ++it) {
    int il, cl;
    const int e = walk.at(it, il, cl);
    if (e >= 0) o[e] = (float)T[il * MT_LD + cl];
  }
}

void muon_tiled_unstage(const bf16* scratch, float* dir, const MuonTiledTensor* tab,
                        const MuonWork* work, int nwork, hipStream_t st) {
  if (nwork <= 0) return;
  hipLaunchKernelGGL(muon_tiled_unstage_kernel, dim3((unsigned)nwork), dim3(MT_THREADS), 0, st,
                     scratch, dir, tab, work);
  DTR_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------- syrk
// A 64-row x 64-k tile of a row-major bf16 matrix (row stride ld): this thread's two 16-byte
// pieces, global -> registers and registers -> an LDS tile of MT_LD-element rows.
struct TileRegs {
  f32x4 v[2];
  __device__ __forceinline__ void load(const bf16* __restrict__ p, int ld) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int q = threadIdx.x + h * MT_THREADS;
      v[h] = *reinterpret_cast<const f32x4*>(p + (long long)(q >> 3) * ld + (q & 7) * 8);
    }
  }
  __device__ __forceinline__ void store(bf16* s) const {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int q = threadIdx.x + h * MT_THREADS;
      *reinterpret_cast<f32x4*>(s + (q >> 3) * MT_LD + (q & 7) * 8) = v[h];
    }
  }
};

template <int EPI>
__global__ void __launch_bounds__(MT_THREADS)
muon_tiled_syrk_kernel(bf16* __restrict__ scratch, const MuonTiledTensor* __restrict__ tab,
                       const MuonWork* __restrict__ work) {
  __shared__ __attribute__((aligned(16))) bf16 S[2][2][MT * MT_LD];   // [stage][operand]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const MuonWork w = work[blockIdx.x];
  const MuonTiledTensor t = tab[w.t];
  const int ld = EPI == 0 ? t.LP : t.SP;    // P's row stride and the reduction length
  const bf16* __restrict__ P = scratch + (EPI == 0 ? t.x_off : t.a_off);
  bf16* __restrict__ C = scratch + (EPI == 0 ? t.a_off : t.b_off);
  const bf16* __restrict__ Pi = P + (long long)w.i * MT * ld;
  const bf16* __restrict__ Pj = P + (long long)w.j * MT * ld;
  const int nk = ld / MT;
  f32x4 acc[2][2] = {};
  TileRegs ri, rj;
  ri.load(Pi, ld);
  rj.load(Pj, ld);
  ri.store(S[0][0]);
  rj.store(S[0][1]);
  lds_barrier();
  for (int kt = 0; kt < nk; ++kt) {
    const int st = kt & 1;
    if (kt + 1 < nk) {
      ri.load(Pi + (kt + 1) * MT, ld);
      rj.load(Pj + (kt + 1) * MT, ld);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 a[2], b[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        a[x] = *reinterpret_cast<const bf16x8*>(S[st][0] + (wm * 32 + x * 16 + c) * MT_LD + ks * 32 + 8 * g);
        b[x] = *reinterpret_cast<const bf16x8*>(S[st][1] + (wn * 32 + x * 16 + c) * MT_LD + ks * 32 + 8 * g);
      }
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = mfma16(a[x], b[y], acc[x][y]);
    }
    if (kt + 1 < nk) {
      ri.store(S[st ^ 1][0]);
      rj.store(S[st ^ 1][1]);
    }
    lds_barrier();   // stage st is read, stage st ^ 1 is written
  }
  // lane: C[wm 32 + x 16 + 4 g + i][wn 32 + y 16 + c] of the tile
  bf16* T = S[0][0];
  bf16* TT = S[0][1];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      const int row = wm * 32 + x * 16 + 4 * g, col = wn * 32 + y * 16 + c;
      bf16x4 h;
      if constexpr (EPI == 0) {
        h = bf16x4{(bf16)acc[x][y][0], (bf16)acc[x][y][1], (bf16)acc[x][y][2], (bf16)acc[x][y][3]};
      } else {
        // A[row + i][col] read as A[col][row + i] (symmetric): one 8-byte load
        const bf16x4 av = *reinterpret_cast<const bf16x4*>(
            P + (long long)(w.j * MT + col) * ld + w.i * MT + row);
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = (bf16)(NS_B * (float)av[i] + NS_C * acc[x][y][i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) T[(row + i) * MT_LD + col] = h[i];
      *reinterpret_cast<bf16x4*>(TT + col * MT_LD + row) = h;
    }
  lds_barrier();
  for (int q = tid; q < MT * 8; q += MT_THREADS) {
    const int row = q >> 3, c8 = (q & 7) * 8;
    *reinterpret_cast<f32x4*>(C + (long long)(w.i * MT + row) * t.SP + w.j * MT + c8) =
        *reinterpret_cast<const f32x4*>(T + row * MT_LD + c8);
    if (w.i != w.j)
      *reinterpret_cast<f32x4*>(C + (long long)(w.j * MT + row) * t.SP + w.i * MT + c8) =
          *reinterpret_cast<const f32x4*>(TT + row * MT_LD + c8);
  }
}

void muon_tiled_syrk(bf16* scratch, const MuonTiledTensor* tab, const MuonWork* work, int nwork,
                     int epi, hipStream_t st) {
  if (nwork <= 0) return;
  if (epi == 0)
    hipLaunchKernelGGL(muon_tiled_syrk_kernel<0>, dim3((unsigned)nwork), dim3(MT_THREADS), 0, st,
                       scratch, tab, work);
  else
    hipLaunchKernelGGL(muon_tiled_syrk_kernel<1>, dim3((unsigned)nwork), dim3(MT_THREADS), 0, st,
                       scratch, tab, work);
  DTR_CHECK_LAUNCH();
}

// --------------------------------------------------------------------------------- apply
template <int BN>
__device__ __forceinline__ void muon_tiled_apply_body(char* smem, bf16* __restrict__ X,
                                                      const bf16* __restrict__ B, int SP, int LP) {
  constexpr int XS = BN + MT_XPAD, CH = BN / 8, NT = BN / 16;
  bf16* Xp = reinterpret_cast<bf16*>(smem);   // [SP][XS]: the panel
  bf16* Bs = Xp + SP * XS;                    // two stages of a 64 x 64 tile of B
  bf16* Os = Bs + 2 * MT * MT_LD;             // [64][XS]: a row tile of the result
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int qr = c >> 2, pc = c & 3;
  const int T = SP / MT, n = T * T;
  TileRegs rb;
  rb.load(B, SP);
  for (int q = tid; q < SP * CH; q += MT_THREADS) {
    const int row = q / CH, c8 = (q - row * CH) * 8;
    *reinterpret_cast<f32x4*>(Xp + row * XS + c8) =
        *reinterpret_cast<const f32x4*>(X + (long long)row * LP + c8);
  }
  rb.store(Bs);
  __syncthreads();   // the whole panel is loaded: every store to X comes after this
  f32x4 acc[NT];
  for (int idx = 0; idx < n; ++idx) {
    const int rt = idx / T, kt = idx - rt * T, st = idx & 1;
    if (kt == 0) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[nt][i] = NS_A * (float)Xp[(rt * MT + wave * 16 + 4 * g + i) * XS + nt * 16 + c];
    }
    if (idx + 1 < n) {
      const int rt1 = (idx + 1) / T, kt1 = idx + 1 - rt1 * T;
      rb.load(B + (long long)rt1 * MT * SP + kt1 * MT, SP);
    }
    const bf16* Bt = Bs + st * MT * MT_LD + (wave * 16 + c) * MT_LD;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      // k order of a fragment: 4 g + (0..3), then 16 + 4 g + (0..3), as the transposing read
      const bf16x4 alo = *reinterpret_cast<const bf16x4*>(Bt + ks * 32 + 4 * g);
      const bf16x4 ahi = *reinterpret_cast<const bf16x4*>(Bt + ks * 32 + 16 + 4 * g);
      const bf16x8 af = {alo[0], alo[1], alo[2], alo[3], ahi[0], ahi[1], ahi[2], ahi[3]};
      const bf16* xr = Xp + (kt * MT + ks * 32 + 4 * g + qr) * XS + 4 * pc;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const s16x4 lo = lds_read_tr16(xr + nt * 16);
        const s16x4 hi = lds_read_tr16(xr + 16 * XS + nt * 16);
        const s16x8 bv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[nt] = mfma16(af, __builtin_bit_cast(bf16x8, bv), acc[nt]);
      }
    }
    if (idx + 1 < n) rb.store(Bs + (st ^ 1) * MT * MT_LD);
    if (kt == T - 1) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          Os[(wave * 16 + 4 * g + i) * XS + nt * 16 + c] = (bf16)acc[nt][i];
    }
    lds_barrier();   // stage st is read, stage st ^ 1 and (last k-tile) Os are written
    if (kt == T - 1) {
      for (int q = tid; q < MT * CH; q += MT_THREADS) {
        const int row = q / CH, c8 = (q - row * CH) * 8;
        *reinterpret_cast<f32x4*>(X + (long long)(rt * MT + row) * LP + c8) =
            *reinterpret_cast<const f32x4*>(Os + row * XS + c8);
      }
      lds_barrier();   // Os is read before the next row tile writes it
    }
  }
}

__global__ void __launch_bounds__(MT_THREADS)
muon_tiled_apply_kernel(bf16* __restrict__ scratch, const MuonTiledTensor* __restrict__ tab,
                        const MuonWork* __restrict__ work) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const MuonWork w = work[blockIdx.x];
  const MuonTiledTensor t = tab[w.t];
  bf16* X = scratch + t.x_off + (long long)w.i * w.j;   // the block's first column
  const bf16* B = scratch + t.b_off;
  if (w.j == 64) muon_tiled_apply_body<64>(smem, X, B, t.SP, t.LP);
  else muon_tiled_apply_body<32>(smem, X, B, t.SP, t.LP);
}

void muon_tiled_apply(bf16* scratch, const MuonTiledTensor* tab, const MuonWork* work, int nwork,
                      int max_sp, hipStream_t st) {
  if (nwork <= 0) return;
  hipLaunchKernelGGL(muon_tiled_apply_kernel, dim3((unsigned)nwork), dim3(MT_THREADS),
                     muon_tiled_apply_lds(max_sp), st, scratch, tab, work);
  DTR_CHECK_LAUNCH();
}

}  // namespace dtr
