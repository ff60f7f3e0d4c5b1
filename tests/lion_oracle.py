"""An independent fp64 reference for the Lion kernel (csrc/lion.hip lion_update_pack) and the
bounds its tests use.  Like tests/adam_oracle.py it is plain fp64 / index arithmetic; nothing
calls the kernel or the host mirrors of it, and no tolerance is tuned to what the kernel gives.

Semantics (per element; s the gradient's scale, wd the decay of the element's tensor;
coefficients as the fp32 values the kernel receives, 1 - b as the fp32 rounding of the fp64
difference, which is what the host passes):
    g' = s * g
    c  = b1 * m + (1 - b1) * g'
    u  = 1 if c > 0, -1 if c < 0, else c     (+-0 stays 0, a NaN stays a NaN)
    w' = (w - lr * u) - (lr * wd) * w        (the old w)
    m' = b2 * m + (1 - b2) * g'

Bounds
------
u32 = 2**-24 (fp32 unit roundoff), as in optim_oracle.  The kernel evaluates every product,
sum and difference in fp32 with contraction off: each rounds once, by at most u32 relative to
its result.  |x| below is the fp64 reference's value; every bound carries the factor
(1 + 4 u32), which covers the second-order terms.

g':  Eg = u32 |s g|: one product; exactly 0 for s = 1.
c:   Bc = 3 u32 (|b1 m| + |(1 - b1) g'|) + (1 - b1) Eg.  Two products and a sum (3 roundings,
     each result no larger than the sum of the two magnitudes), plus g''s error through its
     coefficient.
m':  Bm = 3 u32 (|b2 m| + |(1 - b2) g'|) + (1 - b2) Eg, likewise.
u:   an fp32 evaluation of c lies within Bc of c_ref, so for |c_ref| > Bc it has c_ref's sign:
     the element is `decided`.  c_ref = 0 has Bc = 0 (both terms are 0; the test data has no
     exact cancellation of non-zero terms, asserted) and the kernel's c is 0 too.  Every other
     element is undecided: either sign is a correct evaluation.  lr * u is exact for u = +-1, 0.
w':  with p = (lr wd) w:  Bw = 2 u32 |p| + 2 u32 (|w| + |lr u| + |p|).  lr * wd rounds once and
     its product with w once (2 u32 |p|); the two differences round once each, each result no
     larger than the sum of the three magnitudes.  For an undecided element the bound is
     applied around both candidates w - lr - p and w + lr - p.
An element with g = m = 0 and wd = 0 has every bound but 2 u32 |w| equal to 0; the tests ask
more of it (w bit for bit unchanged).  A NaN in g or m gives NaN in that element's c, w' and
m' and in no other; check() asks exactly that.
"""
import torch

import optim_oracle as oo

U32 = oo.U32
UNDECIDED_MAX = 1e-3   # the share of a test's elements that may be undecided (a condition on
#                        the test data, asserted on the oracle alone: not a tolerance)


def lion_inputs(n, seed):
    """Seeded normal w, g, m; g and m at magnitudes 1e-3 to 1 (the tests' data)."""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 10.0 ** (-3.0 * torch.rand(n, generator=gen))
    m = torch.randn(n, generator=gen) * 10.0 ** (-3.0 * torch.rand(n, generator=gen))
    return w, g, m


class LionRef(tuple):
    """(w', m', Bw, Bm, Bc, decided), and as the attribute `u` the reference's sign(c_ref), which
    check() needs for the other candidate of an undecided element."""
    u = None


def lion_reference(w, g, m, seg_arr, wd_seg, lr, b1, b2, scale):
    """One Lion step in fp64 over the flat buffers (the first sum(numel) elements).  seg_arr:
    the ParamSeg table (contiguous segments), wd_seg: the per-segment decay; the coefficients
    are rounded to fp32 here, as the kernel's float arguments are.  Returns (w', m', Bw, Bm,
    Bc, decided): the new state for u = sign(c_ref), the per-element bounds of a correct fp32
    evaluation (module docstring) and the mask |c_ref| > Bc."""
    n = int(seg_arr[-1]["offset"] + seg_arr[-1]["numel"])
    numel = torch.tensor([int(r["numel"]) for r in seg_arr], device=w.device)
    assert int(numel.sum()) == n and len(wd_seg) == len(seg_arr) and all(
        int(a["offset"] + a["numel"]) == int(b["offset"]) for a, b in zip(seg_arr, seg_arr[1:]))
    w, g, m = (x[:n].double() for x in (w, g, m))
    lr, b1, b2, scale = (oo.f32(x) for x in (lr, b1, b2, scale))
    omb1, omb2 = oo.f32(1.0 - b1), oo.f32(1.0 - b2)
    wd = torch.repeat_interleave(
        torch.tensor([oo.f32(x) for x in wd_seg], dtype=torch.float64, device=w.device), numel)
    u32, so = U32, 1.0 + 4.0 * U32
    gp = scale * g
    Eg = u32 * gp.abs() if scale != 1.0 else torch.zeros_like(gp)
    c1, c2 = b1 * m, omb1 * gp
    c = c1 + c2
    Bc = (3 * u32 * (c1.abs() + c2.abs()) + omb1 * Eg) * so
    m1, m2 = b2 * m, omb2 * gp
    m_new = m1 + m2
    Bm = (3 * u32 * (m1.abs() + m2.abs()) + omb2 * Eg) * so
    decided = c.abs() > Bc
    # c_ref = 0 only where both of its terms are: no exact cancellation in the data
    assert bool(((c1 == 0) & (c2 == 0))[c == 0].all())
    one = torch.ones_like(c)
    u = torch.where(c > 0, one, torch.where(c < 0, -one, c))
    p = (lr * wd) * w
    w_new = (w - lr * u) - p
    Bw = (2 * u32 * p.abs() + 2 * u32 * (w.abs() + (lr * u).abs() + p.abs())) * so
    ref = LionRef((w_new, m_new, Bw, Bm, Bc, decided))
    ref.u = u
    return ref


def undecided_share(ref) -> float:
    """The share of finite elements whose sign a correct fp32 evaluation may get either way
    (c_ref != 0 and |c_ref| <= Bc)."""
    w_new, m_new, Bw, Bm, Bc, decided = ref
    fin = torch.isfinite(m_new) & torch.isfinite(w_new)
    und = fin & ~decided & (Bc > 0)
    return float(und.sum()) / max(1, int(fin.sum()))


def assert_decidable(ref, what=""):
    """The condition on a test's data, on the oracle alone."""
    share = undecided_share(ref)
    assert share <= UNDECIDED_MAX, (what, share)
    return share


def check(w_k, m_k, ref, lr, what=""):
    """The kernel's (or a backend's) w', m' against the reference: within Bw, Bm; for an
    undecided element within Bw of either candidate; NaN exactly where the reference has one.
    Returns the worst err / bound of (w, m)."""
    w_ref, m_ref, Bw, Bm, Bc, decided = ref
    n = w_ref.numel()
    w_k, m_k = w_k[:n].double(), m_k[:n].double()
    lr = oo.f32(lr)
    nan = torch.isnan(m_ref)
    assert torch.equal(torch.isnan(m_k), nan), (what, "NaNs of m")
    assert torch.equal(torch.isnan(w_k), torch.isnan(w_ref)), (what, "NaNs of w")
    ok = ~nan
    em = (m_k - m_ref).abs()
    bad = (ok & ~(em <= Bm)).nonzero().flatten()
    assert bad.numel() == 0, (what, "m", bad[:8].tolist(), float(em[ok].max()))
    und = ok & ~decided & (Bc > 0)
    ew = (w_k - w_ref).abs()
    # undecided: the other candidate w + lr u - p moved the other way, 2 lr from the reference's
    other = w_ref + 2 * lr * ref.u
    ew = torch.where(und, torch.minimum(ew, (w_k - other).abs()), ew)
    bad = (ok & ~(ew <= Bw)).nonzero().flatten()
    assert bad.numel() == 0, (what, "w", bad[:8].tolist(), float(ew[ok].max()))
    worst = (float((ew / Bw.clamp_min(1e-300))[ok].max()), float((em / Bm.clamp_min(1e-300))[ok].max()))
    return worst
