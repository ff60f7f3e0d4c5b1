"""An independent fp64 reference for the BatchNorm kernels (csrc/bn.hip) and the pooled
head (bnrelu_avgpool, avgpool_bwd in csrc/head.hip), the error bounds their tests use,
and the case tables the CPU and GPU tests share.

Everything here is plain fp64 torch on the CPU; nothing calls a kernel or ops/reference.py.
Each function takes the SAME rounded inputs the kernel sees -- bf16 tensors and fp32
per-channel vectors, widened exactly (f64()) -- so every kernel is judged in isolation:
the bound only has to cover that kernel's own arithmetic.

Bounds
------
u = 2**-24 is the unit roundoff of fp32; gam(n) = n u / (1 - n u) is the standard bound on
the relative error of a chain of n roundings (Higham, Accuracy and Stability, 3.1).  Each
bound below is a function with its derivation in the docstring; the tests call these and
use no literal tolerance.  The one measured quantity is RSTD_ULPS.
"""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

F64 = torch.float64
BF = torch.bfloat16
U32 = 2.0 ** -24
BN_TILE_ROWS = 256        # rows per tile of bn_stats / bn_bwd_reduce
FIN_BATCH = 16            # partials per thread and round of the per-channel finalize kernels
MOMENTUM, EPS = 0.997, 1.001e-5

# Largest distance, in fp32 ulps, between a finalize kernel's rstd and the oracle's rstd
# rounded correctly to fp32, plus one ulp (the division and the +eps rounding on other
# inputs).  rsqrtf's device accuracy is documented nowhere in the project, so this one
# constant is measured, on the MI355X over every finalize case of test_bn_exact_gpu.py
# (tree, chan and acc forward, and bn_relu_apply_acc).  Measured: 2 ulp, first reached by
# bn_finalize_kernel (tree) at tiles=255, last tile full, C=512, and by 74 of the 144
# tree / chan cases (the distance includes those kernels' fp32 variance error); the
# accumulator kernels, whose variance is exact to one fp32 rounding, reach 1 ulp
# (M=1003, C=256).
RSTD_ULPS = 2 + 1


def f32(v: float) -> float:
    """v rounded to fp32, as a Python float: the value a kernel's float argument holds."""
    return float(torch.tensor(v, dtype=torch.float32))


def f64(t):
    """Exact widening of a bf16 / fp32 tensor to fp64 on the CPU."""
    return t.detach().to("cpu").to(F64)


def gam(n) -> float:
    return n * U32 / (1.0 - n * U32)


def _exp(v):
    """e with 2**(e-1) <= |v| < 2**e (frexp), clamped at the smallest normal's exponent;
    frexp gives 0 for v = 0, which belongs with the subnormals: -125."""
    v = v.abs().to(F64)
    _, e = torch.frexp(v)
    return torch.where(v == 0, torch.full_like(e, -125), e).clamp(min=-125)


def ulp32(v):
    """Spacing of fp32 at |v| (of the subnormals below 2**-126)."""
    return torch.ldexp(torch.ones_like(v, dtype=F64), _exp(v) - 24)


def ulp_bf16(v):
    """Spacing of bf16 (8 significand bits) at |v|."""
    return torch.ldexp(torch.ones_like(v, dtype=F64), _exp(v) - 8)


def round_f32(v):
    """fp64 -> nearest fp32 (round to nearest even), widened again."""
    return v.to(torch.float32).to(F64)


def ulp_distance32(a, b):
    """|a - b| in units of the fp32 spacing at b (a, b fp64 holding fp32 values)."""
    return (a - b).abs() / ulp32(b)


# ---------------------------------------------------------------------------
# forward statistics
# ---------------------------------------------------------------------------
Partials = namedtuple("Partials", "mean m2 sum_abs sum_sq_dev n")


def tile_partials(x, tile_rows):
    """Per-tile Welford partials of x [M][C] (fp64): mean and M2 = sum (x - mean)**2 per
    tile and channel, [tiles][C] each; sum_abs = sum |x| and sum_sq_dev (the same M2, named
    for the bounds); n [tiles] = rows of each tile (the last holds the remainder)."""
    M, C = x.shape
    tiles = -(-M // tile_rows)
    full = M // tile_rows
    mean = torch.empty(tiles, C, dtype=F64)
    m2 = torch.empty(tiles, C, dtype=F64)
    sab = torch.empty(tiles, C, dtype=F64)
    if full:
        xt = x[:full * tile_rows].view(full, tile_rows, C)
        mu = xt.mean(1)
        mean[:full] = mu
        m2[:full] = ((xt - mu[:, None, :]) ** 2).sum(1)
        sab[:full] = xt.abs().sum(1)
    if tiles > full:
        xl = x[full * tile_rows:]
        mu = xl.mean(0)
        mean[full] = mu
        m2[full] = ((xl - mu) ** 2).sum(0)
        sab[full] = xl.abs().sum(0)
    n = torch.full((tiles,), float(tile_rows), dtype=F64)
    n[-1] = M - (tiles - 1) * tile_rows
    return Partials(mean, m2, sab, m2, n)


def pack_partials(mean, m2):
    """The kernels' layout [tiles][2][C] in fp32 (rounding each partial once)."""
    return torch.stack([mean, m2], 1).to(torch.float32).contiguous()


Final = namedtuple("Final", "mean var rstd scale shift mm mv N m2 uvar sum_n_abs_mean max_abs_mean spread_mean")


def _moving(mm, mv, mean, uvar, momentum):
    k = 1.0 - f32(momentum)        # exact in fp32 too for momentum in [0.5, 1] (Sterbenz)
    return mm - k * (mm - mean), mv - k * (mv - uvar)


def finalize(part_f32, tiles, tile_rows, M, gamma, beta, mm, mv, momentum=MOMENTUM, eps=EPS):
    """Exact (fp64) Chan combine of fp32 partials [tiles][2][C]: tile t holds
    n_t = min(tile_rows, M - t*tile_rows) rows.  N = sum n_t, mean = sum n_t m_t / N,
    M2 = sum q_t + sum n_t (m_t - mean)**2.  rstd = (M2/N + eps)**-0.5 (biased variance);
    the moving variance is fed the Bessel-corrected one, N > 1 ? M2/(N-1) : M2, as the
    kernels do; moving averages in TF's form mm - (1-momentum)(mm - mean).  gamma, beta,
    mm, mv: fp32 vectors (widened here).  Also returns the magnitudes the bounds need."""
    p = f64(part_f32).view(tiles, 2, -1)
    m, q = p[:, 0], p[:, 1]
    n = torch.full((tiles, 1), float(tile_rows), dtype=F64)
    n[-1] = M - (tiles - 1) * tile_rows
    N = float(n.sum())
    assert N == M
    mean = (n * m).sum(0) / N
    m2 = q.sum(0) + (n * (m - mean) ** 2).sum(0)
    return _finish(mean, m2, N, gamma, beta, mm, mv, momentum, eps,
                   (n * m.abs()).sum(0), m.abs().max(0).values,
                   m.max(0).values - m.min(0).values)


def _finish(mean, m2, N, gamma, beta, mm, mv, momentum, eps, snm, mam, spread):
    var = m2 / N
    rstd = (var + f32(eps)) ** -0.5
    scale = f64(gamma) * rstd
    shift = f64(beta) - mean * scale
    uvar = m2 / (N - 1) if N > 1 else m2
    mm2, mv2 = _moving(f64(mm), f64(mv), mean, uvar, momentum)
    return Final(mean, var, rstd, scale, shift, mm2, mv2, N, m2, uvar, snm, mam, spread)


def acc_sums(acc):
    """fp64 replicas [rep][2][C] -> (s1, s2), replicas added in order like bn_acc_sums."""
    a = f64(acc)
    s1, s2 = torch.zeros_like(a[0, 0]), torch.zeros_like(a[0, 1])
    for r in range(a.shape[0]):
        s1 = s1 + a[r, 0]
        s2 = s2 + a[r, 1]
    return s1, s2


def finalize_acc(acc, M, gamma, beta, mm, mv, momentum=MOMENTUM, eps=EPS):
    """The same from accumulator replicas [rep][2][C] of sum y, sum y**2:
    mean = s1/M, var = max(s2/M - mean**2, 0).  The subtraction is done in extended
    precision so that the oracle's own cancellation stays far below one fp32 ulp."""
    s1, s2 = acc_sums(acc)
    mean = s1 / M
    m_l = s1.numpy().astype(np.longdouble) / M
    v_l = s2.numpy().astype(np.longdouble) / M - m_l * m_l
    var = torch.from_numpy(np.maximum(v_l, 0).astype(np.float64))
    return _finish(mean, var * M, float(M), gamma, beta, mm, mv, momentum, eps,
                   s1.abs(), mean.abs(), torch.zeros_like(mean))


# ---------------------------------------------------------------------------
# bounds: forward
# ---------------------------------------------------------------------------
def stats_chain(C, rows=BN_TILE_ROWS):
    """Longest addition chain of bn_stats_kernel / bn_bwd_reduce_kernel for one tile:
    a thread owns one 8-channel group of every rows_per_iter-th row (rows_per_iter =
    256 / (C/8)) and adds them serially, ceil(rows / rows_per_iter) terms; the LDS pass
    then adds the rows_per_iter per-thread sums serially."""
    rpi = 256 // (C // 8)
    return -(-rows // rpi) + rpi


def stats_mean_bound(C, part):
    """|mean_kernel - mean| per tile and channel.  The bf16 inputs are exact in fp32; the
    sum takes stats_chain(C) additions and one division follows: gam(chain + 1) * sum|x| / n."""
    return gam(stats_chain(C) + 1) * part.sum_abs / part.n[:, None]


def stats_m2_bound(C, part):
    """|M2_kernel - M2| per tile and channel.  The kernel's second pass is about ITS fp32
    mean mu = mean + d, |d| <= stats_mean_bound: sum (x - mu)**2 = M2 + n d**2 exactly
    (sum (x - mean) = 0).  Each term costs three roundings (x - mu, the square, and its
    sum), the chain stats_chain(C) more, all terms non-negative:
    gam(chain + 3) (M2 + n d**2) + n d**2."""
    d = stats_mean_bound(C, part)
    nd2 = part.n[:, None] * d * d
    return gam(stats_chain(C) + 3) * (part.sum_sq_dev + nd2) + nd2


def fin_depth(variant, tiles):
    """Longest chain of the forward finalize kernels, read from the code.
    'chan' (bn_finalize_chan_kernel): a thread adds FIN_BATCH partials of the first round
    and one per 256 tiles past the first FIN_BATCH * 256; then 6 wave-shuffle levels and a
    2-level sum of the 4 waves.
    'tree' (bn_finalize_kernel): a thread folds ceil(tiles / 256) partials with wcombine,
    then 8 LDS tree levels: that many Welford combines in sequence."""
    if variant == "chan":
        return FIN_BATCH + max(0, -(-(tiles - FIN_BATCH * 256) // 256)) + 8
    assert variant == "tree"
    return -(-tiles // 256) + 8


def fin_mean_bound(variant, tiles, fin):
    """|mean_kernel - mean| per channel for the partial-tile finalize kernels.
    chan: sx = sum n_t m_t, one rounding per product, fin_depth additions, one division
      (N and the n_t are integers below 2**24, exact): gam(depth + 2) sum n_t|m_t| / N.
    tree: each wcombine computes d = mb - ma, fb = nb/n <= 1, d*fb and ma + d*fb: three
      roundings of a quantity no larger than |d| fb <= R and one of the new mean, <= A,
      with R = max_t m_t - min_t m_t and A = max_t |m_t| (every combined mean is a
      weighted average of tile means): <= u (3 R + A) per combine, carried through the
      later combines with weights (1 - fb, fb) that sum to 1; one more link of the chain
      for the second-order terms (the means that enter d are themselves perturbed):
      gam(depth + 1) (3 R + A).
    acc: s1/M in fp64 cast to fp32, one fp32 rounding and fp64 dust: gam(2) |mean|."""
    if variant == "acc":
        return gam(2) * fin.mean.abs()
    depth = fin_depth(variant, tiles)
    if variant == "chan":
        return gam(depth + 2) * fin.sum_n_abs_mean / fin.N
    return gam(depth + 1) * (3 * fin.spread_mean + fin.max_abs_mean)


def fin_m2_bound(variant, tiles, fin):
    """|M2_kernel - M2| per channel (M2 is not an output; moving_var's bound uses it).
    With d = fin_mean_bound:
    chan: sum q_t + n_t (m_t - mu)**2 about the kernel's own mean mu equals M2 + N e**2,
      |e| <= d, exactly; a term costs 4 roundings (m_t - mu, two products, + q_t) and the
      chain fin_depth more, all terms non-negative:  T = M2 + N d**2,  gam(depth + 4) T + (T - M2).
    tree: M2 = sum q_t + sum_k w_k d_k**2 over the combines k, w_k = na nb / n.  Each d_k is
      off by at most 2 d (both means), so sum w_k (d_k + e_k)**2 <= B + 4 d sqrt(B W) +
      4 d**2 W with B = sum w_k d_k**2 <= M2 and W = sum w_k <= N depth (the combines of
      one level act on disjoint rows, w_k <= min(na, nb)).  A term costs 6 roundings (d*d,
      * na, fb, * fb, two sums), a q_t passes through 2 depth sums:
      T = M2 + 4 d sqrt(M2 W) + 4 d**2 W,  gam(2 depth + 6) T + (T - M2).
    acc: var in fp64, M2 = var * M is never formed in fp32: 0."""
    if variant == "acc":
        return torch.zeros_like(fin.m2)
    d = fin_mean_bound(variant, tiles, fin)
    depth = fin_depth(variant, tiles)
    if variant == "chan":
        T = fin.m2 + fin.N * d * d
        return gam(depth + 4) * T + (T - fin.m2)
    W = fin.N * depth
    T = fin.m2 + 4 * d * torch.sqrt(fin.m2 * W) + 4 * d * d * W
    return gam(2 * depth + 6) * T + (T - fin.m2)


def fin_mm_bound(variant, tiles, fin, mm, momentum=MOMENTUM):
    """|moving_mean' - oracle|: mm - k (mm - mean), k = 1 - momentum: the subtraction k
    (exact for momentum >= 0.5, counted anyway), mm - mean, the product and the last
    subtraction, each no larger than |mm| + k(|mm| + |mean|); the mean's own error enters
    with weight k:  gam(4) (|mm| + k |mm| + k |mean|) + k fin_mean_bound."""
    k = 1.0 - f32(momentum)
    mm = f64(mm).abs()
    return gam(4) * (mm + k * mm + k * fin.mean.abs()) + k * fin_mean_bound(variant, tiles, fin)


def fin_mv_bound(variant, tiles, fin, mv, momentum=MOMENTUM):
    """|moving_var' - oracle|: as fin_mm_bound with uvar = M2/(N-1) (one more rounding, the
    division; in acc mode the cast of var*M/(M-1)), whose error is fin_m2_bound/(N-1):
    gam(5) (|mv| + k |mv| + k uvar) + k fin_m2_bound / max(N-1, 1)."""
    k = 1.0 - f32(momentum)
    mv = f64(mv).abs()
    return (gam(5) * (mv + k * mv + k * fin.uvar)
            + k * fin_m2_bound(variant, tiles, fin) / max(fin.N - 1, 1))


def rstd_bound(fin):
    """RSTD_ULPS fp32 ulps of the oracle's rstd (the measured constant above)."""
    return RSTD_ULPS * ulp32(fin.rstd)


def scale_bound(gamma, rstd_k):
    """scale = gamma * rstd in one fp32 product of the kernel's OWN rstd: 1 ulp."""
    return ulp32(f64(gamma) * f64(rstd_k))


def shift_bound(beta, mean_k, scale_k):
    """shift = beta - mean * scale from the kernel's own mean and scale: a product and a
    subtraction (one rounding when contracted), 1 ulp each."""
    ms = f64(mean_k) * f64(scale_k)
    return ulp32(ms) + ulp32(f64(beta) - ms)


def eval_reference(gamma, beta, mm, mv, eps=EPS):
    """bn_eval: scale = gamma rsqrt(mv + eps), shift = beta - mm scale (fp64)."""
    rstd = (f64(mv) + f32(eps)) ** -0.5
    scale = f64(gamma) * rstd
    return scale, f64(beta) - f64(mm) * scale


def eval_scale_bound(gamma, mv, eps=EPS):
    """bn_eval's scale: mv + eps (one rounding: half an ulp of rsqrt's argument is a
    quarter ulp of its value, counted as one), rsqrtf (RSTD_ULPS, which includes that
    rounding on the finalize cases) and the product: (RSTD_ULPS + 2) ulps of the scale."""
    scale, _ = eval_reference(gamma, torch.zeros_like(gamma), torch.zeros_like(gamma), mv, eps)
    return (RSTD_ULPS + 2) * ulp32(scale)


# ---------------------------------------------------------------------------
# apply / pool
# ---------------------------------------------------------------------------
def ambiguous(x, scale, shift):
    """(pre, mag, amb): fp64 pre = x*scale + shift, mag = |x*scale| + |shift| and the
    AMBIGUOUS-MASK set |pre| <= 2**-23 mag: a correct fp32 evaluation, contracted to an fma
    (one rounding) or not (two), is within 2 u mag = 2**-23 mag of pre and may land on
    either side of zero there; outside the set its sign is that of pre."""
    xs = x * scale
    pre = xs + shift
    mag = xs.abs() + shift.abs()
    return pre, mag, pre.abs() <= 2.0 ** -23 * mag


K_APPLY = 2 + 1        # x*scale, + shift; +1: gam(k) <= (k+1) u
K_BWD_APPLY = 7 + 1    # x - mean, * rstd, c*xhat, a*g, - b, - c*xhat, + add; +1 as above
K_POOL_BWD = 2 + 1     # 1/HW, dp * inv


def bf16_out_bound(r, S, k):
    """|out - r| <= 1/2 ulp_bf16(r) + k u S for an output rounded once to bf16 from an fp32
    value v whose expression makes k - 1 roundings, each of an intermediate no larger
    than S, the sum of the magnitudes of the expression's terms: |v - r| <= gam(k-1) S <=
    k u S, and the rounding to bf16 adds half a bf16 ulp.  (Where k u S carries r across a
    power of two the half ulp is that of v's binade; then k u S exceeds a whole bf16 ulp
    of r and the first-order count, which charges every rounding at its full size and
    no contraction, has that room.)"""
    return 0.5 * ulp_bf16(r) + k * U32 * S


def apply(x, scale, shift):
    """relu(x*scale + shift) in fp64; returns (y, S, amb) with S = |x*scale| + |shift|.
    On the ambiguous set y is within 2**-23 S of 0 either way, which K_APPLY u S covers."""
    pre, mag, amb = ambiguous(x, scale, shift)
    return pre.clamp(min=0), mag, amb


def pool_chain(HW, C):
    """bnrelu_avgpool_kernel: a thread adds ceil(HW / rpi) rows, rpi = max(1, 256/(C/8)),
    the LDS pass adds rpi sums; each term carries the affine's 2 roundings and the
    division by HW is one more."""
    rpi = max(1, 256 // (C // 8))
    return -(-HW // rpi) + rpi + 3


def avgpool(x, scale, shift):
    """x [N][HW][C]: (pooled, S, amb_widen): the mean over HW of relu(x*scale+shift); S =
    mean of |x*scale| + |shift|; amb_widen = the ambiguous elements' share, mean over HW
    of 2**-23 mag on the ambiguous set (either branch of such an element is correct).
    Bound: bf16_out_bound(pooled, S, pool_chain + 1) + amb_widen."""
    pre, mag, amb = ambiguous(x, scale, shift)
    widen = (2.0 ** -23 * mag * amb).mean(1)
    return pre.clamp(min=0).mean(1), mag.mean(1), widen, amb


def avgpool_bwd(dp, HW):
    """dp [N][C] -> dp / HW broadcast to [N][HW][C]; S = |dp| / HW (K_POOL_BWD roundings:
    the kernel multiplies by fl(1/HW))."""
    r = (dp / HW)[:, None, :].expand(dp.shape[0], HW, dp.shape[1])
    return r, r.abs()


# ---------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------
BwdSums = namedtuple("BwdSums", "sg sgx abs_g abs_gx amb amb_g amb_gx n")


def _tile_sum(v, tile_rows):
    M, C = v.shape
    tiles = -(-M // tile_rows)
    pad = tiles * tile_rows - M
    if pad:
        v = torch.cat([v, torch.zeros(pad, C, dtype=v.dtype)])
    return v.view(tiles, tile_rows, C).sum(1)


def bwd_terms(dy, x, mean, rstd, scale, shift):
    """Per element (g, g xhat, amb, xhat) with the fp64 ReLU mask."""
    pre, _, amb = ambiguous(x, scale, shift)
    g = torch.where(pre > 0, dy, torch.zeros_like(dy))
    xh = (x - mean) * rstd
    return g, g * xh, amb, xh


def bwd_sums(dy, x, mean, rstd, scale, shift, tile_rows=BN_TILE_ROWS):
    """g = dy [x*scale + shift > 0], xhat = (x - mean) rstd.  Per tile and channel
    sg = sum g, sgx = sum g xhat, the sums of magnitudes abs_g, abs_gx, the ambiguous-mask
    set amb [M][C] (ambiguous()) and amb_g, amb_gx = sum over the tile's ambiguous
    elements of |dy|, |dy xhat|: a correct kernel may count or drop each of them."""
    g, gx, amb, xh = bwd_terms(dy, x, mean, rstd, scale, shift)
    ts = lambda v: _tile_sum(v, tile_rows)  # noqa: E731
    M = x.shape[0]
    tiles = -(-M // tile_rows)
    n = torch.full((tiles,), float(tile_rows), dtype=F64)
    n[-1] = M - (tiles - 1) * tile_rows
    return BwdSums(ts(g), ts(gx), ts(g.abs()), ts(gx.abs()), amb,
                   ts(dy.abs() * amb), ts((dy * xh).abs() * amb), n)


def bwd_reduce_bounds(C, s):
    """Per tile and channel (bound_sg, bound_sgx) of bn_bwd_reduce_kernel.  g is a bf16
    value, exact: sum g costs stats_chain(C) roundings; a term g*(x - mean)*rstd three
    more.  gam(chain) abs_g + amb_g  and  gam(chain + 3) abs_gx + amb_gx."""
    ch = stats_chain(C)
    return gam(ch) * s.abs_g + s.amb_g, gam(ch + 3) * s.abs_gx + s.amb_gx


def sum_partials(part_f32, tiles):
    """fp32 backward partials [tiles][2][C] -> exact (s1, s2, sum|.|, sum|.|)."""
    p = f64(part_f32).view(tiles, 2, -1)
    return p[:, 0].sum(0), p[:, 1].sum(0), p[:, 0].abs().sum(0), p[:, 1].abs().sum(0)


BwdFinal = namedtuple("BwdFinal", "dbeta dgamma coef")


def bwd_finalize(s1, s2, M, gamma, rstd):
    """From the exact sums of what the kernel is handed (sum_partials or acc_sums):
    dbeta = s1, dgamma = s2, coef = [a, a s1 / M, a s2 / M], a = gamma rstd."""
    a = f64(gamma) * f64(rstd)
    return BwdFinal(s1, s2, torch.stack([a, a * s1 / M, a * s2 / M]))


def bwd_fin_chain(variant, tiles):
    """'tile' (bn_bwd_finalize_kernel): a thread adds every 16th partial, then 16 sums are
    added serially.  'chan' (bn_bwd_finalize_chan_kernel): FIN_BATCH partials per round of
    4096, then 6 shuffle levels and a 2-level sum.  'acc': fp64 sums, one cast to fp32."""
    if variant == "tile":
        return -(-tiles // 16) + 16
    if variant == "chan":
        return -(-tiles // (FIN_BATCH * 256)) * FIN_BATCH + 8
    assert variant == "acc"
    return 1


def sum_bound(n, sum_abs):
    """A sum of fp32 terms along chains of at most n additions: gam(n) sum |terms|."""
    return gam(n) * sum_abs


def coef_bounds(fin, M, d1, d2):
    """Bounds [3][C] on coef given the bounds d1, d2 on the two sums.  a: one product,
    gam(1)|a|.  a*s/M: two more roundings and the sum's own error scaled by |a|/M:
    gam(3) |a s / M| + (1 + gam(3)) |a| d / M."""
    a = fin.coef[0].abs()
    g3 = gam(3)
    return torch.stack([gam(1) * a,
                        g3 * fin.coef[1].abs() + (1 + g3) * a * d1 / M,
                        g3 * fin.coef[2].abs() + (1 + g3) * a * d2 / M])


def bwd_apply(dy, x, mean, rstd, scale, shift, coef, add=None):
    """dx = a g - b - c xhat (+ add) per element in fp64, for both values of the ReLU
    mask: returns (dx, dx_flipped, S, amb).  dx uses the fp64 mask, dx_flipped the other
    branch (a correct kernel may produce it on the ambiguous set amb only);
    S = |a dy| + |b| + |c xhat| + |add| bounds every intermediate of either branch."""
    pre, _, amb = ambiguous(x, scale, shift)
    a, b, c = coef[0], coef[1], coef[2]
    xh = (x - mean) * rstd
    rest = -b - c * xh
    S = (a * dy).abs() + b.abs() + (c * xh).abs()
    if add is not None:
        rest = rest + add
        S = S + add.abs()
    on, off = a * dy + rest, rest.expand_as(dy)
    pos = pre > 0
    return torch.where(pos, on, off), torch.where(pos, off, on), S, amb


AMBIGUOUS_CAP = 1e-3   # at most 0.1 % of a case's elements may be ambiguous


def ambiguous_share(amb) -> float:
    return float(amb.sum()) / amb.numel()


# ---------------------------------------------------------------------------
# comparison helper
# ---------------------------------------------------------------------------
def worst(got, ref, bound, alt=None, alt_ok=None):
    """Per-element check |got - ref| <= bound (or |got - alt| <= bound where alt_ok).
    Returns None when every element passes, else a message naming the worst offender's
    index, its value, the reference and the bound."""
    got = f64(got).reshape(ref.shape)
    err = (got - ref).abs()
    ok = err <= bound
    if alt is not None:
        ok = ok | (alt_ok & ((got - alt).abs() <= bound))
    ok = ok & torch.isfinite(got)
    if bool(ok.all()):
        return None
    excess = torch.where(ok, torch.zeros_like(err), err / torch.as_tensor(bound).clamp(min=1e-300))
    excess = torch.where(torch.isfinite(excess), excess, torch.full_like(excess, math.inf))
    flat = int(excess.reshape(-1).argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ref.shape))
    b = torch.as_tensor(bound).expand(ref.shape)[idx]
    return (f"{int((~ok).sum())} of {ok.numel()} outside the bound; worst at {idx}: "
            f"got {float(got[idx])!r}, oracle {float(ref[idx])!r}, "
            f"|err| {float(err[idx]):.3e} > bound {float(b):.3e}")


# ---------------------------------------------------------------------------
# shared inputs and case tables (the CPU test checks the ambiguity cap on all of them)
# ---------------------------------------------------------------------------
def make_x(M, C, seed, hard=False):
    """x ~ 2 N(0,1) + 3 rounded to bf16 (fp64-generated); hard: per-channel means spread
    over [-40, 40] with std 0.5, where a one-pass variance would lose digits."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(M, C, dtype=F64, generator=g)
    if hard:
        x = z * 0.5 + torch.linspace(-40, 40, C, dtype=F64)
    else:
        x = z * 2 + 3
    return x.to(BF)


def make_vecs(C, seed):
    """fp32 gamma in [0.5, 1.5), beta ~ +-(0.05 + 0.1 |N|), nonzero starting moving averages.
    beta keeps away from zero: with M = 1 the variance is 0, x*scale + shift collapses to
    beta under a cancellation of ~1000 |x|, and a beta below 2**-23 of that would be a
    legitimately ambiguous ReLU mask."""
    g = torch.Generator().manual_seed(seed + 1000)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1
    beta = beta + torch.where(beta < 0, -0.05, 0.05)
    mm = torch.randn(C, generator=g) * 0.5
    mv = torch.rand(C, generator=g) + 0.5
    return gamma, beta, mm, mv


Inputs = namedtuple("Inputs", "x dy add gamma beta mm mv fin mean rstd scale shift")


@lru_cache(maxsize=4)
def real_inputs(M, C, seed, hard=False):
    """One BatchNorm's tensors for the apply / reduce tests: bf16 x, dy, add, and fp32
    mean, rstd, scale, shift from a real finalize (the oracle's, rounded to fp32) of x's
    256-row partials.  Cached and shared between tests; treat as read-only."""
    x = make_x(M, C, seed, hard)
    g = torch.Generator().manual_seed(seed + 2000)
    dy = torch.randn(M, C, dtype=F64, generator=g).to(BF)
    add = torch.randn(M, C, dtype=F64, generator=g).to(BF)
    gamma, beta, mm, mv = make_vecs(C, seed)
    p = tile_partials(f64(x), BN_TILE_ROWS)
    tiles = p.mean.shape[0]
    fin = finalize(pack_partials(p.mean, p.m2), tiles, BN_TILE_ROWS, M, gamma, beta, mm, mv)
    r32 = lambda v: v.to(torch.float32)  # noqa: E731
    return Inputs(x, dy, add, gamma, beta, mm, mv, fin, r32(fin.mean), r32(fin.rstd),
                  r32(fin.scale), r32(fin.shift))


def inputs(M, C, hard=False):
    """The input set of shape (M, C) every test shares."""
    return real_inputs(M, C, case_seed(M, C), hard)


FIN_TILE_ROWS = 4
FIN_TILES = (1, 255, 256, 257, 1023, 1024, 4096, 4097, 5003)
FIN_CS = (16, 80, 512, 520)
FIN_LAST = (FIN_TILE_ROWS, 1)          # rows of the last tile
ACC_CS = (16, 256, 264)
STATS_CASES = [(M, C) for C in (16, 64, 256, 2048) for M in (1, 255, 257, 256 * 3 + 7)]
BWD_APPLY_CASES = [(1, 16), (257, 64), (129, 2048), (65539, 256)]
# the fused apply's two grids: C <= 64 (U = 2) and, past 256*256*4 vectors, the capped U = 4
# one.  The default grid rule admits the latter only from M >= 21846 rows on (a shape like
# (4099, 512) stays on the separate finalize), hence (21859, 128): 349744 vectors.
BWD_APPLY_ACC_CASES = [(1000, 64), (21859, 128)]
APPLY_CASES = [(3, 16), (65539, 256)]
APPLY_ACC_CASES = [(4099, 512), (3, 16)]
POOL_CASES = [(3, 64, 64), (2, 49, 2048), (1, 1, 16)]
CHAIN_CASE = (769, 64)


def case_seed(*dims):
    return sum(int(d) * k for d, k in zip(dims, (1, 7919, 104729))) % (2 ** 31)


@lru_cache(maxsize=2)
def fin_source(tiles, last_rows):
    """(M, x, partials): x (bf16 values, fp64) [M][max C] behind the synthetic finalize
    partials, M = (tiles - 1) * 4 + last_rows, and its 4-row partials."""
    M = (tiles - 1) * FIN_TILE_ROWS + last_rows
    x = f64(make_x(M, max(FIN_CS), case_seed(tiles, last_rows)))
    return M, x, tile_partials(x, FIN_TILE_ROWS)


def stats_chain_propagation(part, fin):
    """How the errors of bn_stats' partials reach the statistics of the original x through
    an exact Chan combine: with |m_t' - m_t| <= d_t (stats_mean_bound) and |q_t' - q_t| <=
    e_t (stats_m2_bound), the mean moves by at most sum n_t d_t / N, and M2 = sum q_t +
    n_t (m_t - mean)**2 by at most sum e_t + n_t (2 |m_t - mean| w + w**2) with
    w = d_t + sum n_t d_t / N.  Returns (d_mean, d_m2) per channel."""
    C = part.mean.shape[1]
    d, e, n = stats_mean_bound(C, part), stats_m2_bound(C, part), part.n[:, None]
    dm = (n * d).sum(0) / fin.N
    w = d + dm
    return dm, (e + n * (2 * (part.mean - fin.mean).abs() * w + w * w)).sum(0)


def rstd_propagation(var_a, var_b, d_var, eps=EPS):
    """|f(va) - f(vb)| for f(v) = (v + eps)**-0.5 and |va - vb| <= d_var: f is convex and
    decreasing with f' = -f**3 / 2, so the difference is at most d_var f(v_min)**3 / 2,
    v_min = max(min(va, vb) - d_var, 0)."""
    vmin = (torch.minimum(var_a, var_b) - d_var).clamp(min=0)
    return 0.5 * d_var * (vmin + f32(eps)) ** -1.5


def make_acc(x64, rep, second=None):
    """fp64 replicas [rep][2][C] of sum y, sum y**2 (or of the rows of `second`) with
    UNEQUAL shares: replica r takes rows r, r + rep, ... of the first 3/4 of the rows and
    replica 0 the rest as well."""
    M, C = x64.shape
    second = x64 * x64 if second is None else second
    acc = torch.zeros(rep, 2, C, dtype=F64)
    cut = M * 3 // 4
    for r in range(rep):
        acc[r, 0], acc[r, 1] = x64[:cut][r::rep].sum(0), second[:cut][r::rep].sum(0)
    acc[0, 0] += x64[cut:].sum(0)
    acc[0, 1] += second[cut:].sum(0)
    return acc
