"""An independent fp64 reference for the LAMB kernels (csrc/lamb.hip: lamb_moments_norms,
lamb_trust, lamb_update_pack) and the bounds their tests use.  Like tests/lars_oracle.py and
tests/adam_oracle.py it is plain fp64 / index arithmetic (the bias corrections in mpmath);
nothing calls the kernels or the host mirrors of them, and no tolerance is tuned to what the
kernels give.

Semantics (per element; s the gradient's scale, wd the decay of the element's tensor, t >= 1
the step count of the bias correction; coefficients as the fp32 values the kernels receive,
1 - b as the fp32 rounding of the fp64 difference):
    g' = s * g (+ wd * w                in "l2" mode)
    m' = b1 * m + (1 - b1) * g'
    v' = b2 * v + (1 - b2) * g' * g'
    r  = (m' * k1) / (sqrt(v' * k2) + eps)     k1 = 1 / (1 - b1^t),  k2 = 1 / (1 - b2^t)
    u  = r (+ wd * w                    in "decoupled" mode)
per tensor:
    trust = |w| / |u|  if adapted and |w| > 0 and |u| > 0, else 1
    w'    = w - (lr * trust) * u

Bounds
------
u_ = 2**-24 (fp32 unit roundoff; written u_ here because u is the direction).  The helper's
fp32 operations each round once (contraction is off in it), by at most u_ relative to their
result; sqrtf and / are correctly rounded.  |x| below is the fp64 reference's value; every
bound carries a (1 + O(u_)) factor that the spare units cover.

The helper's roundings, counted: g' 1 (l2: 3), m' 3, v' 4, m' * k1 1, v' * k2 1, the square
root 1, + eps 1, the quotient 1, and in decoupled mode wd * w 1 and the last sum 1: 15 in
either mode's longest chain, plus k1 and k2, each within one fp32 ulp of the correctly
rounded value (an fp64 chain rounded once): 3 u_ relative of the exact one.  Were no inner
sum to cancel, u would be within that count times u_ (|r| + |wd w|).  But m' (and in l2 mode
g') is itself a sum that can cancel, which no multiple of u_ |r| covers; so the count is
propagated term by term, each sum against the magnitudes of its two terms:

g':  Eg = 3 u_ (|s g| + |wd w|) in l2 mode (two products and a sum, each result no larger
     than the sum of the magnitudes), u_ |s g| in decoupled mode (one product).
m':  Bm = 3 u_ (|b1 m| + |(1 - b1) g'|) + (1 - b1) Eg.
v':  Bv = 4 u_ (b2 v + (1 - b2) g'^2) + (1 - b2) (2 |g'| Eg + Eg^2).  (adam_oracle's two.)
a = m' k1:     Ea = k1 Bm + 4 u_ |a|   (k1's 3 u_ and the product's rounding).
x = v' k2:     Ex = k2 Bv + 4 u_ x.
q = sqrt(x):   Eq = Ex / q + u_ q   (|sqrt(a) - sqrt(b)| <= |a - b| / sqrt(b); x = 0 only when
               both terms of v' are 0, and then Bv = 0 and the kernel's x is 0 too: Eq = 0).
d = q + eps:   Ed = Eq + u_ d.
r = a / d:     Er = (Ea + |r| Ed) / (d - Ed) + u_ |r|   (as adam_oracle's quotient; d - Ed > 0
               is asserted).
u = r + wd w:  Eu = Er + u_ |wd w| + 2 u_ (|r| + |wd w|)   (the product, the sum -- whose
               result is no larger than the two magnitudes -- and one spare; decoupled mode.
               l2: Eu = Er).  This is "the count times 2**-24 (|r| + |wd w|)" with the inner
               cancellations carried: the sum r + wd w can cancel, so the bound is absolute.

sums of squares (per chunk and per tensor):  the kernel adds fl(u_k^2) as lars_norms adds its
     squares: at most 18 fp32 terms a thread, fp64 from there: SS_REL = 20 u_ relative to the
     sum of the kernel's own squares (lars_oracle).  u_k^2 is within D = 2 |u| Eu + Eu^2 of u^2:
     Bss_u = sum D + SS_REL (sum u^2 + sum D);   Bss_w = SS_REL sum w^2   (w is exact).
norms:  |w| within NORM_REL = 11 u_ relative (lars_oracle).  |u| = sqrt(ss_u): with rho =
     Bss_u / ss_u (asserted < 1/2), the fp64 root is within rho (1 + rho) / 2 relative
     (1 / (1 + sqrt(1 - rho)) <= (1 + rho) / 2 on [0, 1/2]), and the slot is rounded to
     fp32 once: Bun = |u| (rho (1 + rho) / 2 + u_).
trust:  the fp64 quotient of two roots within 10 u_ and rho' = rho (1 + rho) / 2, rounded to
     fp32 once: relative (10 u_ + rho') / (1 - rho') + 2 u_ (the rounding and one spare) =:
     TR.  A skipped tensor and a norm that is not > 0 give exactly 1.
w':  the kernel's rate fl(lr * trust_k) is within TR + u_ of lr * trust; the product with u_k
     rounds once, the difference once (its result no larger than |w| + |rate u|), one spare:
     Bw = rate Eu + |rate u| (TR + 3 u_) + 2 u_ (|w| + |rate u|).
An element with g = m = v = 0 and wd = 0 has u = 0 exactly; a tensor of them has |u| = 0 and
trust 1, and the tests ask that its w is left bit for bit.
"""
import mpmath
import numpy as np
import torch

import optim_oracle as oo

U32 = oo.U32
SS_REL = 20 * U32       # lars_oracle's, derived there
NORM_REL = 11 * U32
MP = mpmath.mp.clone()
MP.dps = 60


def _k_mp(t, b):
    b = MP.mpf(oo.f32(b))
    return 1 / (1 - b ** int(t))


def bias_reference(t, b1, b2):
    """(k1, k2) = (1 / (1 - b1^t), 1 / (1 - b2^t)) from the fp32 coefficients at 60 digits,
    each rounded to fp32 once.  The device's fp64 chain can differ by one fp32 ulp, and only
    next to a rounding boundary."""
    out = []
    for b in (b1, b2):
        x = _k_mp(t, b)
        with MP.workprec(24):
            out.append(float(+x))
    return tuple(out)


def ulp(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))


def _expand(vals, numel, device):
    return torch.repeat_interleave(torch.tensor(list(vals), dtype=torch.float64, device=device),
                                   numel)


def lamb_direction_reference(w, g, m, v, seg_arr, wd_seg, t, b1, b2, eps, scale, mode):
    """Stage 1 per element in fp64 over the flat buffers (the first sum(numel) elements).
    Returns (m', v', u, Bm, Bv, Eu): the new moments, the direction and the per-element bounds
    of a correct fp32 evaluation (module docstring)."""
    assert mode in ("decoupled", "l2") and t >= 1
    n = int(seg_arr[-1]["offset"] + seg_arr[-1]["numel"])
    numel = torch.tensor([int(r["numel"]) for r in seg_arr], device=w.device)
    assert int(numel.sum()) == n and len(wd_seg) == len(seg_arr) and all(
        int(a["offset"] + a["numel"]) == int(b["offset"]) for a, b in zip(seg_arr, seg_arr[1:]))
    w, g, m, v = (x[:n].double() for x in (w, g, m, v))
    b1, b2, eps, scale = (oo.f32(x) for x in (b1, b2, eps, scale))
    omb1, omb2 = oo.f32(1.0 - b1), oo.f32(1.0 - b2)
    k1, k2 = float(_k_mp(t, b1)), float(_k_mp(t, b2))
    wd = _expand([oo.f32(x) for x in wd_seg], numel, w.device)
    u_ = U32
    gs = scale * g
    dec = wd * w
    if mode == "l2":
        gp = gs + dec
        Eg = 3 * u_ * (gs.abs() + dec.abs())
    else:
        gp = gs
        Eg = u_ * gs.abs()
    m1, m2 = b1 * m, omb1 * gp
    m_new = m1 + m2
    Bm = 3 * u_ * (m1.abs() + m2.abs()) + omb1 * Eg
    v1, v2 = b2 * v, omb2 * gp * gp
    v_new = v1 + v2
    Bv = 4 * u_ * (v1.abs() + v2) + omb2 * (2 * gp.abs() * Eg + Eg * Eg)
    a = m_new * k1
    Ea = k1 * Bm + 4 * u_ * a.abs()
    x = v_new * k2
    Ex = k2 * Bv + 4 * u_ * x
    q = x.sqrt()
    assert bool((Bv[q == 0] == 0).all())
    Eq = torch.where(q > 0, Ex / q.clamp_min(1e-300), torch.zeros_like(q)) + u_ * q
    d = q + eps
    Ed = Eq + u_ * d
    assert bool((d - Ed > 0).all())
    r = a / d
    Er = (Ea + r.abs() * Ed) / (d - Ed) + u_ * r.abs()
    if mode == "decoupled":
        u = r + dec
        Eu = Er + u_ * dec.abs() + 2 * u_ * (r.abs() + dec.abs())
    else:
        u = r
        Eu = Er
    return m_new, v_new, u, Bm, Bv, Eu


def sums_reference(w, u, Eu, bounds):
    """(sum w^2, sum u^2, Bss_w, Bss_u) over each [a, b) of `bounds` (chunks or tensors), as
    lists of floats."""
    w, u = w.double(), u.double()
    D = 2 * u.abs() * Eu + Eu * Eu
    out = [], [], [], []
    for a, b in bounds:
        ssw, ssu, sd = (float(x[a:b].sum()) for x in (w * w, u * u, D))
        for lst, val in zip(out, (ssw, ssu, SS_REL * ssw, sd + SS_REL * (ssu + sd))):
            lst.append(val)
    return out


def chunk_bounds(seg_arr, chunk):
    """[a, b) of every lamb_moments_norms workgroup, in grid order."""
    out = []
    for r in seg_arr:
        o, n = int(r["offset"]), int(r["numel"])
        out += [(o + c, min(o + c + chunk, o + n)) for c in range(0, n, chunk)]
    return out


def trust_reference(ssw, ssu, Bssu, skip):
    """Per tensor (wn, un, trust, Bun, TR): the norms, the trust ratio, the absolute bound of
    the |u| slot and the relative bound of the trust slot (0 where it is exactly 1)."""
    wn, un, trust, Bun, TR = [], [], [], [], []
    for a, b, Bb, sk in zip(ssw, ssu, Bssu, skip):
        x, y = float(np.sqrt(a)), float(np.sqrt(b))
        rho = Bb / b if b > 0 else 0.0
        assert rho < 0.5 and (b > 0 or Bb == 0)
        rp = rho * (1 + rho) / 2
        wn.append(x)
        un.append(y)
        Bun.append(y * (rp + U32))
        if sk or not x > 0 or not y > 0:
            trust.append(1.0)
            TR.append(0.0)
        else:
            trust.append(x / y)
            TR.append((10 * U32 + rp) / (1 - rp) + 2 * U32)
    return wn, un, trust, Bun, TR


def lamb_reference(w, g, m, v, seg_arr, wd_seg, skip, lr, t, b1, b2, eps, scale, mode):
    """One LAMB step in fp64.  Returns a dict: the new state w, m, v, the direction u, the
    per-element bounds Bw, Bm, Bv, Eu, and per tensor ssw, ssu, Bssw, Bssu, wn, un, trust,
    Bun, TR (lists)."""
    m_new, v_new, u, Bm, Bv, Eu = lamb_direction_reference(w, g, m, v, seg_arr, wd_seg, t, b1, b2,
                                                           eps, scale, mode)
    n = u.numel()
    w = w[:n].double()
    segs = [(int(r["offset"]), int(r["offset"] + r["numel"])) for r in seg_arr]
    ssw, ssu, Bssw, Bssu = sums_reference(w, u, Eu, segs)
    wn, un, trust, Bun, TR = trust_reference(ssw, ssu, Bssu, skip)
    numel = torch.tensor([b - a for a, b in segs], device=w.device)
    rate = oo.f32(lr) * _expand(trust, numel, w.device)
    tr = _expand(TR, numel, w.device)
    step = rate * u
    w_new = w - step
    Bw = rate * Eu + step.abs() * (tr + 3 * U32) + 2 * U32 * (w.abs() + step.abs())
    return dict(w=w_new, m=m_new, v=v_new, u=u, Bw=Bw, Bm=Bm, Bv=Bv, Eu=Eu, ssw=ssw, ssu=ssu,
                Bssw=Bssw, Bssu=Bssu, wn=wn, un=un, trust=trust, Bun=Bun, TR=TR)
