"""Exactly representable conv operands and an independent fp64 oracle.

Every conv kernel path accumulates bf16 products in fp32.  With small-integer (or dyadic)
operands every product and every partial sum is an integer (or a multiple of a fixed power
of two) below 2**24, hence exact in fp32 in ANY summation order: MFMA order, K-tile order,
split-K slice order, ring or register loop and parity class stop mattering, and each path
owes one bit pattern -- the exact result rounded ONCE to bf16, round-to-nearest-even (fp32
outputs owe the exact number itself).  The comparison is equality, so one wrong halo pixel,
dropped tap or mis-stored row fails it.

Operand ranges (all survive the cast to bf16 unchanged, asserted):
  activations / gradients  integers in [-3, 3]      weights   integers in [-2, 2]
  residual / accumulate    integers in [-8, 8]      bias      integers in [-8, 8]
  pre_scale in {0.5, 1, 2}, pre_shift integer in [-2, 2]  (relu(x*sc+sh): half-integers <= 8)
  wgrad scale in {1, 0.5, 0.25}

Values are random.  So that the ONE rounding is observable (|y| >= 256 needs ~7 sigma of an
i.i.d. 144-term sum) a few output columns get full-magnitude weights and a few dozen
receptive fields are sign-aligned with them on a random share of their channels: still
random integers of the same ranges, but the outputs then spread over [-6*Kdim, 6*Kdim].

The oracle is the TF fixed-padding arithmetic written out here: explicit zero pad of
(k-1)//2 before and the rest after, then a VALID conv with the stride, one fp64 matmul
per filter tap.  Nothing here imports ops/reference.py or calls a kernel.
"""
from dataclasses import dataclass
from functools import lru_cache

import torch

BF = torch.bfloat16
F64 = torch.float64
EXACT_LIMIT = 2 ** 24


# ---------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------
def pads(k):
    """TF conv2d_fixed_padding: (before, after) = ((k-1)//2, the rest)."""
    before = (k - 1) // 2
    return before, k - 1 - before


def out_size(H, k, s):
    b, e = pads(k)
    return (H + b + e - k) // s + 1


@dataclass(frozen=True)
class Case:
    """One conv launch.  mode 'fwd': y[N,Ho,Ho,K] = conv(x[N,H,H,C], w); mode 'dgrad':
    dx[N,H,H,C] from dy[N,Ho,Ho,K].  w is always HWIO [k,k,C,K]."""
    name: str
    mode: str
    N: int
    H: int
    C: int
    K: int
    k: int
    s: int
    res: bool = False       # residual add (forward)
    acc: bool = False       # accumulate onto a non-zero base
    f32: bool = False       # fp32 output (forward)
    nbias: int = 0          # bias on columns < nbias (forward)
    pre: bool = False       # relu(x*pre_scale+pre_shift) prologue (forward)
    seed: int = 0
    keep: int = 1           # weights kept on every keep-th reduction channel only
    zero_from: int = 0      # activation channels >= zero_from are zero (padded stems)

    @property
    def Ho(self):
        return out_size(self.H, self.k, self.s)

    @property
    def pad(self):
        return pads(self.k)[0]

    @property
    def cin(self):          # reduction channels / output columns of the implicit GEMM
        return self.C if self.mode == "fwd" else self.K

    @property
    def ncol(self):
        return self.K if self.mode == "fwd" else self.C

    @property
    def kdim(self):        # non-zero terms of one output's sum
        return self.k * self.k * min(self.cin, self.zero_from or self.cin)

    @property
    def out_shape(self):
        return (self.N, self.Ho, self.Ho, self.K) if self.mode == "fwd" else \
            (self.N, self.H, self.H, self.C)

    def geom(self):
        """The bindings' geometry list [N,H,W,C,Ho,Wo,K,kh,kw,stride,pad]."""
        return [self.N, self.H, self.H, self.C, self.Ho, self.Ho, self.K, self.k, self.k, self.s,
                self.pad]


# ---------------------------------------------------------------------------
# oracle: fp64, one matmul per tap over the explicitly padded tensor
# ---------------------------------------------------------------------------
def _padded(x, kh, kw):
    N, H, W, C = x.shape
    (bh, eh), (bw, ew) = pads(kh), pads(kw)
    xp = torch.zeros(N, H + bh + eh, W + bw + ew, C, dtype=F64)
    xp[:, bh:bh + H, bw:bw + W] = x
    return xp


def _tap(t, r, c, Ho, Wo, s):
    return t[:, r:r + (Ho - 1) * s + 1:s, c:c + (Wo - 1) * s + 1:s]


def conv_fwd(x, w, s):
    """x [N,H,W,C], w HWIO -> [N,Ho,Wo,K], fp64."""
    x, w = x.to(F64), w.to(F64)
    kh, kw, C, K = w.shape
    N, H, W, _ = x.shape
    Ho, Wo = out_size(H, kh, s), out_size(W, kw, s)
    xp = _padded(x, kh, kw)
    y = torch.zeros(N * Ho * Wo, K, dtype=F64)
    for r in range(kh):
        for c in range(kw):
            y += _tap(xp, r, c, Ho, Wo, s).reshape(-1, C) @ w[r, c]
    return y.view(N, Ho, Wo, K)


def conv_dgrad(dy, w, x_shape, s):
    """Gradient of conv_fwd wrt x: every tap scatters dy @ w[r,c]^T onto its strided
    positions of the padded input; the pad is cropped."""
    dy, w = dy.to(F64), w.to(F64)
    kh, kw, C, K = w.shape
    N, H, W, _ = x_shape
    Ho, Wo = dy.shape[1], dy.shape[2]
    (bh, _), (bw, _) = pads(kh), pads(kw)
    dxp = _padded(torch.zeros(N, H, W, C, dtype=F64), kh, kw)
    flat = dy.reshape(-1, K)
    for r in range(kh):
        for c in range(kw):
            _tap(dxp, r, c, Ho, Wo, s).add_((flat @ w[r, c].t()).view(N, Ho, Wo, C))
    return dxp[:, bh:bh + H, bw:bw + W].contiguous()


def conv_wgrad(dy, x, k, s):
    """Gradient of conv_fwd wrt w, HWIO [k,k,C,K]."""
    dy, x = dy.to(F64), x.to(F64)
    N, H, W, C = x.shape
    Ho, Wo, K = dy.shape[1], dy.shape[2], dy.shape[3]
    xp = _padded(x, k, k)
    flat = dy.reshape(-1, K)
    dw = torch.zeros(k, k, C, K, dtype=F64)
    for r in range(k):
        for c in range(k):
            dw[r, c] = _tap(xp, r, c, Ho, Wo, s).reshape(-1, C).t() @ flat
    return dw


def prologue(x, sc, sh):
    return torch.relu(x.to(F64) * sc.to(F64) + sh.to(F64))


def crop_hwio(dw, k_valid, c_valid):
    return dw[:, :, :c_valid, :k_valid].contiguous()


# ---------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------
def gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int64)


def choice(g, values, n):
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), (n,), generator=g)]


def assert_bf16_exact(t, what):
    t = t.to(F64)
    assert torch.equal(t.to(BF).to(F64), t), f"{what}: not exactly representable in bf16"


def guard(nterms, a, b, *extras):
    """The exactness condition: nterms * max|a| * max|b| + sum max|extras| < 2**24, so every
    partial sum in every order is exact in fp32.  Returns the bound."""
    bound = nterms * float(a.abs().max()) * float(b.abs().max())
    bound += sum(float(e.abs().max()) for e in extras if e is not None)
    assert bound < EXACT_LIMIT, f"exactness guard: {bound} >= 2**24"
    return bound


def _sources(case, p, q, r, c):
    """Operand pixel that filter tap (r, c) pairs with output pixel (p, q), or None."""
    if case.mode == "fwd":
        h, w = p * case.s + r - case.pad, q * case.s + c - case.pad
        return (h, w) if 0 <= h < case.H and 0 <= w < case.H else None
    hn, wn = p + case.pad - r, q + case.pad - c
    if hn % case.s or wn % case.s:
        return None
    ho, wo = hn // case.s, wn // case.s
    return (ho, wo) if 0 <= ho < case.Ho and 0 <= wo < case.Ho else None


def _plant(case, g, a, w, plants=96, hot=2):
    """Full-magnitude weights on `hot` output columns; `plants` receptive fields (each the
    fullest of 8 random output pixels: borders and stride-2 parity classes see fewer taps)
    aligned with one of them on a random share of their channels (module docstring)."""
    cols = torch.randperm(case.ncol, generator=g)[:hot].tolist()
    for j in cols:
        sl = w[:, :, :, j] if case.mode == "fwd" else w[:, :, j, :]
        # +-2, one in eight +-1: with +-2 alone every aligned sum would be even, and an
        # even integer below 512 is never rounded
        mag = 2 - (ints(g, sl.shape, 0, 7) == 0).to(torch.int64)
        sl.copy_(mag * (2 * ints(g, sl.shape, 0, 1) - 1))
    P = case.out_shape[1]
    taps = [(r, c) for r in range(case.k) for c in range(case.k)]
    # few enough that the planted fields of a small image do not overwrite each other
    for _ in range(min(plants, max(4, case.N * P * P // 4))):
        n = int(ints(g, (1,), 0, case.N - 1))
        best = []
        for p, q in ints(g, (8, 2), 0, P - 1).tolist():
            srcs = [(t, _sources(case, p, q, *t)) for t in taps]
            srcs = [(t, src) for t, src in srcs if src is not None]
            if len(srcs) > len(best):
                best = srcs
        j = cols[int(ints(g, (1,), 0, hot - 1))]
        share = 0.7 + 0.3 * float(torch.rand(1, generator=g))
        for (r, c), src in best:
            wv = w[r, c, :, j] if case.mode == "fwd" else w[r, c, j, :]
            pick = torch.rand(wv.shape, generator=g) < share
            vec = a[n, src[0], src[1]]
            vec[pick] = (3 * torch.sign(wv))[pick]


@lru_cache(maxsize=4)
def operands(case):
    """fp64 CPU operands of a Case: a (x or dy), w (HWIO) and whichever of sc, sh, res,
    base, bias the case asks for; 'want' is the exact result (fp64) and 'bound' the
    guard's bound.  Treat the returned tensors as read-only (they are cached)."""
    g = gen(1000 + case.seed)
    a_shape = (case.N, case.H, case.H, case.C) if case.mode == "fwd" else \
        (case.N, case.Ho, case.Ho, case.K)
    a = ints(g, a_shape, -3, 3)
    w = ints(g, (case.k, case.k, case.C, case.K), -2, 2)
    _plant(case, g, a, w)
    if case.keep > 1:
        mask = torch.arange(case.cin) % case.keep == 0
        w = w * (mask.view(1, 1, -1, 1) if case.mode == "fwd" else mask.view(1, 1, 1, -1))
    if case.zero_from:
        a[..., case.zero_from:] = 0
    o = {"a": a.to(F64), "w": w.to(F64)}
    eff = o["a"]
    if case.pre:
        o["sc"] = choice(g, [0.5, 1.0, 2.0], case.C)
        o["sh"] = ints(g, (case.C,), -2, 2).to(F64)
        eff = prologue(o["a"], o["sc"], o["sh"])
    if case.mode == "fwd":
        want = conv_fwd(eff, o["w"], case.s)
    else:
        want = conv_dgrad(o["a"], o["w"], (case.N, case.H, case.H, case.C), case.s)
    if case.nbias:
        o["bias"] = ints(g, (case.nbias,), -8, 8).to(F64)
        want[..., :case.nbias] += o["bias"]
    if case.res:
        o["res"] = ints(g, case.out_shape, -8, 8).to(F64)
        want = want + o["res"]
    if case.acc:
        o["base"] = ints(g, case.out_shape, -8, 8).to(F64)
        want = want + o["base"]
    for name, t in o.items():
        assert_bf16_exact(t, f"{case.name}: {name}")
    assert_bf16_exact(eff, f"{case.name}: prologue output")
    o["bound"] = guard(case.kdim, eff, o["w"], o.get("bias"), o.get("res"), o.get("base"))
    o["want"] = want
    return o


# ---------------------------------------------------------------------------
# what the one rounding does to an exact result
# ---------------------------------------------------------------------------
def rounding_census(want):
    """(values that bf16 rounds at all, exact ties where round-to-nearest-even and
    round-half-away-from-zero give different bit patterns) of an exact fp64 tensor."""
    f = want.to(torch.float32)
    assert torch.equal(f.to(F64), want), "not exact in fp32"
    bits = f.view(torch.int32)
    low = bits & 0xFFFF
    rounded = int((low != 0).sum())
    # a tie has exactly the half bit set; RNE keeps an even bf16 mantissa (truncates) where
    # half-away increments it
    ties = int(((low == 0x8000) & (((bits >> 16) & 1) == 0)).sum())
    return rounded, ties


# ---------------------------------------------------------------------------
# the GPU cases (tests/test_exact_conv_gpu.py runs them, test_exact_conv_cpu.py checks the
# guard and the rounding census of each)
# ---------------------------------------------------------------------------
def _both(name, *geo, **kw):
    return [Case(f"{name}-fwd", "fwd", *geo, **kw), Case(f"{name}-dgrad", "dgrad", *geo, **kw)]


# (tile, full/partial) of the generic implicit GEMM: geometry N, H, C, K, k, s.  C == K so
# one geometry reaches the same tile forward and backward; the partial cases have M no
# multiple of the row tile and odd H with stride 2.  The 16- and 32-column tiles take
# exactly 16 / 32 columns and the 128x128 tile needs Ncol % 128 == 0 (launch_mode), so
# only the 64-column tiles have partial columns: Ncol 48, and 80 = one full + one partial.
TILE_CASES = {
    (64, 16): _both("t64x16-full", 2, 32, 16, 16, 3, 1) + _both("t64x16-part", 3, 9, 16, 16, 3, 2),
    (128, 16): _both("t128x16-full", 32, 32, 16, 16, 1, 1) +
    _both("t128x16-part", 35, 61, 16, 16, 3, 2),
    (256, 16): _both("t256x16-full", 128, 32, 16, 16, 3, 1) +
    _both("t256x16-part", 137, 31, 16, 16, 1, 1),
    (64, 32): _both("t64x32-full", 2, 16, 32, 32, 3, 1) + _both("t64x32-part", 3, 9, 32, 32, 3, 2),
    (128, 32): _both("t128x32-full", 128, 16, 32, 32, 1, 1) +
    _both("t128x32-part", 35, 61, 32, 32, 3, 2),
    (64, 64): _both("t64x64-full", 1, 8, 64, 64, 3, 1) + _both("t64x64-part", 3, 9, 48, 48, 3, 2) +
    [Case("t64x64-part48-fwd", "fwd", 3, 9, 32, 48, 3, 2),
     Case("t64x64-part80-fwd", "fwd", 3, 9, 32, 80, 1, 1),
     Case("t64x64-part80-dgrad", "dgrad", 3, 9, 80, 32, 3, 2)],
    # Kdim = 64: the single-buffer (nbuf1_kt) loop
    (128, 64): _both("t128x64-full", 32, 32, 64, 64, 1, 1) +
    _both("t128x64-part", 35, 31, 48, 48, 3, 1),
    (128, 128): _both("t128x128-full", 16, 16, 128, 128, 1, 1) +
    _both("t128x128-part", 21, 14, 128, 128, 3, 1) +
    [Case("t128x128-nbuf1-fwd", "fwd", 16, 16, 64, 128, 1, 1),
     Case("t128x128-nbuf1-dgrad", "dgrad", 16, 16, 128, 64, 1, 1)],
}

# epilogue / prologue options on a small tile (64x32) and on 128x128
OPTION_CASES = [
    Case("opt-res-small", "fwd", 2, 9, 32, 32, 3, 1, res=True, seed=1),
    Case("opt-res-128", "fwd", 21, 14, 64, 128, 3, 1, res=True, seed=2),
    Case("opt-acc-small", "fwd", 2, 9, 32, 32, 3, 1, acc=True, seed=3),
    Case("opt-acc-128", "fwd", 21, 14, 64, 128, 3, 1, acc=True, seed=4),
    Case("opt-acc-small-dgrad", "dgrad", 2, 9, 32, 32, 3, 1, acc=True, seed=5),
    Case("opt-acc-128-dgrad", "dgrad", 21, 14, 128, 64, 3, 1, acc=True, seed=6),
    Case("opt-f32-small", "fwd", 2, 9, 32, 32, 3, 1, f32=True, seed=7),
    Case("opt-f32-128", "fwd", 21, 14, 64, 128, 3, 1, f32=True, acc=True, seed=8),
    # the dense layer: 1x1, H = 1, 64 -> 16 with 10 classes
    Case("opt-bias-dense", "fwd", 37, 1, 64, 16, 1, 1, f32=True, nbias=10, seed=9),
    Case("opt-bias-128", "fwd", 4099, 1, 64, 128, 1, 1, f32=True, nbias=100, seed=10),
    Case("opt-bias-bf16", "fwd", 37, 1, 64, 16, 1, 1, nbias=10, res=True, seed=11),
    Case("opt-pre-small", "fwd", 2, 9, 32, 32, 3, 1, pre=True, seed=12),
    Case("opt-pre-small-s2", "fwd", 2, 9, 32, 32, 3, 2, pre=True, res=True, seed=13),
    Case("opt-pre-128", "fwd", 21, 14, 64, 128, 3, 1, pre=True, seed=14),
    Case("opt-pre-128-res", "fwd", 65, 15, 64, 128, 3, 2, pre=True, res=True, seed=15),
]

# an under-filled FAST grid: 13 x 8 tiles of 64x64, 72 K tiles
SPLITK_CASES = _both("splitk", 16, 7, 512, 512, 3, 1, seed=20) + \
    [Case("splitk-pre-fwd", "fwd", 16, 7, 512, 512, 3, 1, pre=True, seed=21)]

PARITY_CASES = [Case(f"parity-k{k}-h{H}{'-acc' if acc else ''}", "dgrad", 2, H, 32, 64, k, 2,
                     acc=acc, seed=30 + H + k)
                for k in (1, 3) for H in (8, 9) for acc in (False, True)]

# the smallest N at which each class of the ring tests still takes the ring loop (128-row
# tiles: M >= 4096 for 128 columns, >= 32768 for 64), channels cut to what the class needs
RING_CASES = [
    Case("ring-fwd-3x3", "fwd", 21, 14, 64, 128, 3, 1, res=True, seed=40),
    Case("ring-fwd-3x3-s2", "fwd", 21, 27, 64, 128, 3, 2, res=True, seed=41),
    Case("ring-fwd-1x1", "fwd", 21, 14, 320, 256, 1, 1, seed=42),
    Case("ring-fwd-1x1-s2", "fwd", 84, 13, 320, 128, 1, 2, seed=43),
    Case("ring-fwd-splitk", "fwd", 84, 7, 256, 128, 3, 1, seed=44),
    Case("ring-dgrad-3x3", "dgrad", 21, 14, 128, 64, 3, 1, acc=True, seed=45),
    Case("ring-dgrad-3x3-s2", "dgrad", 84, 14, 128, 128, 3, 2, acc=True, seed=46),
    Case("ring-dgrad-3x3-s2-odd", "dgrad", 84, 13, 128, 128, 3, 2, seed=47),
    Case("ring-dgrad-1x1-splitk", "dgrad", 84, 7, 128, 1024, 1, 1, seed=48),
    Case("ring-fwd-3x3-n64", "fwd", 42, 28, 64, 64, 3, 1, res=True, seed=49),
    Case("ring-fwd-1x1-n64", "fwd", 42, 28, 320, 64, 1, 1, seed=50),
    Case("ring-dgrad-3x3-n64", "dgrad", 42, 28, 64, 64, 3, 1, acc=True, seed=51),
    Case("ring-dgrad-1x1-n64", "dgrad", 42, 28, 64, 256, 1, 1, seed=52),
]
RING_SPLITK = {"ring-fwd-splitk", "ring-dgrad-1x1-splitk"}

# direct 3x3 kernels: (channels @ width), one image and an odd image count
DIRECT_CASES = [c for ch, H in ((16, 32), (32, 16), (64, 8)) for N in (1, 3) for c in
                _both(f"direct-{ch}at{H}-n{N}", N, H, ch, ch, 3, 1, seed=60 + N) +
                [Case(f"direct-{ch}at{H}-n{N}-pre-res", "fwd", N, H, ch, ch, 3, 1, pre=True,
                      res=True, seed=62 + N),
                 Case(f"direct-{ch}at{H}-n{N}-acc", "dgrad", N, H, ch, ch, 3, 1, acc=True,
                      seed=64 + N)]]

# stems: 3 real channels padded to 8, non-zero weights against the zero channels
STEM_CASES = [Case("stem-cifar", "fwd", 2, 32, 8, 16, 3, 1, zero_from=3, seed=70),
              Case("stem-imagenet", "fwd", 1, 17, 8, 64, 7, 2, zero_from=3, seed=71)]


def conv_cases():
    out = [c for cases in TILE_CASES.values() for c in cases]
    return out + OPTION_CASES + SPLITK_CASES + PARITY_CASES + RING_CASES + DIRECT_CASES + \
        STEM_CASES


# ---------------------------------------------------------------------------
# fused BN-backward prologue (direct dgrad `abwd`, streaming bnd1x1 mode 1)
# ---------------------------------------------------------------------------
def bn_backward_operands(seed, shape, C):
    """Operands of dh = a*g - b - c*xhat (+ add), g = da * [x*scale+shift > 0], xhat =
    (x - mean) * rstd, with mean / shift integers and rstd / scale / a / b / c powers of
    two: every term is a multiple of 1/4 of magnitude < 32, so dh is exact under any
    contraction and exactly representable in bf16 (asserted)."""
    g = gen(2000 + seed)
    o = {"da": ints(g, shape, -3, 3).to(F64), "x": ints(g, shape, -3, 3).to(F64),
         "add": ints(g, shape, -8, 8).to(F64),
         "mean": ints(g, (C,), -2, 2).to(F64), "rstd": choice(g, [0.5, 1.0, 2.0], C),
         "scale": choice(g, [0.5, 1.0, 2.0], C), "shift": ints(g, (C,), -2, 2).to(F64),
         "coef": torch.cat([choice(g, [0.5, 1.0, 2.0], C), choice(g, [1.0, 2.0, 4.0], C),
                            choice(g, [0.5, 1.0], C)])}
    return o


def bn_backward_apply(o, grad, with_add):
    """The exact dh for a gradient tensor `grad` (da itself, or an exact dgrad)."""
    C = o["mean"].numel()
    a, b, c = o["coef"][:C], o["coef"][C:2 * C], o["coef"][2 * C:]
    gg = grad * ((o["x"] * o["scale"] + o["shift"]) > 0).to(F64)
    dh = a * gg - b - c * (o["x"] - o["mean"]) * o["rstd"]
    return dh + o["add"] if with_add else dh


ABWD_CASES = [(16, 32, 1), (16, 32, 3), (32, 16, 2), (64, 8, 1), (64, 8, 3)]   # C, H, N


@lru_cache(maxsize=2)
def abwd_operands(C, H, N, with_add):
    o = dict(bn_backward_operands(C * 100 + N * 2 + with_add, (N, H, H, C), C))
    o["w"] = ints(gen(2500 + C + N), (3, 3, C, C), -2, 2).to(F64)
    o["dh"] = bn_backward_apply(o, o["da"], with_add)
    for name in ("da", "x", "add", "w", "dh"):
        assert_bf16_exact(o[name], f"abwd {name}")
    o["bound"] = guard(9 * C, o["dh"], o["w"])
    o["want"] = conv_dgrad(o["dh"], o["w"], (N, H, H, C), 1)
    return o


# streaming 1x1 kernels: (M, C, K) = (rows, output columns, reduction channels); the
# smallest covered widths, and row counts that are an odd number of row tiles (the
# kernels take whole row tiles only: the bindings reject any other M, which the GPU
# test asserts)
BNF_CASES = [(96, 64, 64), (160, 256, 64), (48, 256, 128), (80, 512, 256)]
BND_CASES = [(96, 64, 64), (160, 128, 64), (96, 256, 64), (80, 256, 128)]


@lru_cache(maxsize=2)
def bnf_operands(M, C, K, pre):
    case = Case(f"bnf-{M}-{C}-{K}", "fwd", M, 1, K, C, 1, 1, res=True, pre=pre, seed=101 + pre)
    return case, operands(case)


@lru_cache(maxsize=2)
def bnd_operands(M, C, K, with_add):
    """bnd1x1 mode 1 rounds twice on purpose: the dgrad g = dz W^T is rounded to bf16 (the
    same bits the implicit-GEMM dgrad stores) before the BN backward is applied and rounded
    again.  The exact test therefore keeps weights on every second reduction channel only,
    so |g| <= 6 * K / 2 <= 256 for K <= 64 is an integer bf16 holds exactly (K = 128: every
    fourth, asserted) and the final rounding is the only one that acts."""
    keep = 2 if K <= 64 else 4
    case = Case(f"bnd-{M}-{C}-{K}", "dgrad", M, 1, C, K, 1, 1, keep=keep, seed=90 + with_add)
    ops = operands(case)
    g = ops["want"].reshape(M, C)
    assert_bf16_exact(g, "bnd1x1: intermediate dgrad")
    o = dict(bn_backward_operands(3000 + M + C + K + with_add, (M, C), C))
    o["dz"], o["w"] = ops["a"].reshape(M, K), ops["w"].reshape(C, K)
    o["want"] = bn_backward_apply(o, g, with_add)
    o["bound"] = guard(1, 4 * g.abs().max().view(1) + 64, torch.ones(1))
    return o


# ---------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class WCase:
    name: str
    N: int
    H: int
    C: int
    K: int
    k: int
    s: int
    pre: bool
    path: str        # 'generic' | 'ring' | 'direct'
    seed: int = 0

    @property
    def Ho(self):
        return out_size(self.H, self.k, self.s)

    def geom(self):
        return [self.N, self.H, self.H, self.C, self.Ho, self.Ho, self.K, self.k, self.k, self.s,
                pads(self.k)[0]]


WGRAD_CASES = [WCase(f"{n}{'-pre' if pre else ''}", *geo, pre, path, seed)
               for pre in (False, True) for seed, (n, path, geo) in enumerate([
                   ("wg-generic", "generic", (3, 15, 32, 48, 3, 1)),
                   ("wg-generic-s2", "generic", (5, 23, 24, 16, 3, 2)),
                   ("wg-ring", "ring", (4, 14, 64, 128, 3, 1)),
                   ("wg-ring-s2", "ring", (6, 27, 72, 128, 3, 2)),
                   ("wg-direct-16", "direct", (2, 32, 16, 16, 3, 1)),
                   ("wg-direct-32", "direct", (3, 16, 32, 32, 3, 1)),
                   ("wg-direct-64", "direct", (17, 8, 64, 64, 3, 1))])]


@lru_cache(maxsize=2)
def wgrad_operands(wc):
    """x, dy, optional prologue, and the exact HWIO gradient 'want' (fp64, unscaled)."""
    g = gen(4000 + wc.seed + 50 * wc.pre)
    o = {"x": ints(g, (wc.N, wc.H, wc.H, wc.C), -3, 3).to(F64),
         "dy": ints(g, (wc.N, wc.Ho, wc.Ho, wc.K), -3, 3).to(F64)}
    eff = o["x"]
    if wc.pre:
        o["sc"] = choice(g, [0.5, 1.0, 2.0], wc.C)
        o["sh"] = ints(g, (wc.C,), -2, 2).to(F64)
        eff = prologue(o["x"], o["sc"], o["sh"])
    o["base"] = ints(g, (wc.k, wc.k, wc.C, wc.K), -8, 8).to(F64)
    for name, t in o.items():
        assert_bf16_exact(t, f"{wc.name}: {name}")
    assert_bf16_exact(eff, f"{wc.name}: prologue output")
    # the reduction runs over the N*Ho*Wo output pixels
    o["bound"] = guard(wc.N * wc.Ho * wc.Ho, eff, o["dy"], o["base"])
    o["want"] = conv_wgrad(o["dy"], eff, wc.k, wc.s)
    return o
