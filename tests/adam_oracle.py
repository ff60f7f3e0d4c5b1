"""An independent fp64 reference for the AdamW kernel (csrc/adam.hip adam_update_pack) and
the bounds its tests use.  Like tests/optim_oracle.py it is plain fp64 / index arithmetic
(the bias-corrected rate in mpmath, as tests/lr_decay_oracle.py does its curve); nothing
calls the kernel or the host mirrors of it, and no tolerance is tuned to what the kernel gives.

Semantics (per element; s the gradient's scale, wd the decay of the element's tensor,
t >= 1 the step count of the bias correction; coefficients as the fp32 values the kernel
receives, 1 - b as the fp32 rounding of the fp64 difference, which is what the host passes):
    g'    = s * g (+ wd * w                   in "l2" mode)
    m'    = b1 * m + (1 - b1) * g'
    v'    = b2 * v + (1 - b2) * g' * g'
    alpha = lr * sqrt(1 - b2^t) / (1 - b1^t)
    w'    = w - alpha * m' / (sqrt(v') + eps) (- lr * wd * w, the old w, in "decoupled" mode)

Bounds
------
u = 2**-24 (fp32 unit roundoff), as in optim_oracle.  The kernel's fp32 products, sums,
square root and quotient each round once, by at most u relative to their result (fewer
roundings where the compiler contracts a product and a sum into an fma); sqrtf and / are
correctly rounded.  |x| below is the fp64 reference's value; every bound carries a (1 + O(u))
factor that the spare units cover.

g':  Eg = 3 u (|s g| + |wd w|).  l2: two products and a sum, each result no larger than
     |s g| + |wd w| (3 roundings); decoupled: one product.
m':  Bm = 3 u (|b1 m| + |(1 - b1) g'|) + (1 - b1) Eg.  Two products and a sum (3 roundings,
     each result <= the sum of the two magnitudes), plus g''s error through its coefficient.
v':  Bv = 4 u (b2 v + (1 - b2) g'^2) + (1 - b2) (2 |g'| Eg + Eg^2).  The square, two products
     and a sum: at most 3 roundings on either term's path, and one spare; g''s error through
     the square ((g' + e)^2 - g'^2 = 2 g' e + e^2).
r = sqrt(v'):  Er = Bv / r + u r.  |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <=
     |a - b| / sqrt(b) with b the reference's v'; one rounding.  v' = 0 only when both of its
     terms are 0, and then Bv = 0 and the kernel's v' is 0 too: Er = 0.
d = r + eps:  Ed = Er + u d.
q = m' / d:  Eq = (Bm + |q| Ed) / (d - Ed) + u |q|.  The two partial derivatives 1 / d and
     -m' / d^2 carry the errors of m' and d, made rigorous for finite errors:
     |m_k / d_k - m / d| = |(m_k - m) d - m (d_k - d)| / (d d_k) <= (Bm d + |m| Ed) / (d (d - Ed));
     one rounding of the quotient.  (d - Ed > 0 for the tests' data; asserted.)
alpha:  the kernel's alpha is within one fp32 ulp of the correctly rounded value (an fp64
     chain rounded once; alpha_reference below), so within 3 u relative of the exact one.
w':  Bw = |alpha| Eq + 4 u |alpha q| + 3 u |lr wd w| + 2 u (|w| + |alpha q| + |lr wd w|).
     alpha * q: alpha's 3 u and the product's rounding; decoupled: lr * wd (one rounding),
     times w (one), and one spare; the two differences, each result no larger than the sum of
     the three magnitudes.
An element with g = m = v = 0 and wd = 0 has every bound but 2 u |w| equal to 0; the tests ask
more of it (w bit for bit unchanged).
"""
import math

import mpmath
import numpy as np
import torch

import optim_oracle as oo

U32 = oo.U32
MP = mpmath.mp.clone()
MP.dps = 60


def _alpha_mp(lr, t, b1, b2):
    lr, b1, b2 = (MP.mpf(oo.f32(x)) for x in (lr, b1, b2))
    return lr * MP.sqrt(1 - b2 ** int(t)) / (1 - b1 ** int(t))


def alpha_reference(lr, t, b1, b2) -> float:
    """lr * sqrt(1 - b2^t) / (1 - b1^t) from the fp32 coefficients at 60 digits, rounded to
    fp32 once.  The device's fp64 chain (a few 2**-53 relative) can differ from it only by
    one fp32 ulp, and only next to a rounding boundary."""
    x = _alpha_mp(lr, t, b1, b2)
    with MP.workprec(24):
        r = float(+x)
    assert r == 0.0 or abs(r) > 2.0 ** -120
    return r


def ulp(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))


def adam_reference(w, g, m, v, seg_arr, wd_seg, lr, t, b1, b2, eps, scale, mode):
    """One AdamW step in fp64 over the flat buffers (the first sum(numel) elements).
    seg_arr: the ParamSeg table (contiguous segments), wd_seg: the per-segment decay; the
    coefficients are rounded to fp32 here, as the kernel's float arguments are.  Returns
    (w', m', v', Bw, Bm, Bv, alpha): the new state, the per-element bounds of a correct fp32
    evaluation (module docstring) and the exact alpha (fp64)."""
    assert mode in ("decoupled", "l2") and t >= 1
    n = int(seg_arr[-1]["offset"] + seg_arr[-1]["numel"])
    numel = torch.tensor([int(r["numel"]) for r in seg_arr], device=w.device)
    assert int(numel.sum()) == n and len(wd_seg) == len(seg_arr) and all(
        int(a["offset"] + a["numel"]) == int(b["offset"]) for a, b in zip(seg_arr, seg_arr[1:]))
    w, g, m, v = (x[:n].double() for x in (w, g, m, v))
    lr, b1, b2, eps, scale = (oo.f32(x) for x in (lr, b1, b2, eps, scale))
    omb1, omb2 = oo.f32(1.0 - b1), oo.f32(1.0 - b2)
    wd = torch.repeat_interleave(
        torch.tensor([oo.f32(x) for x in wd_seg], dtype=torch.float64, device=w.device), numel)
    alpha = float(_alpha_mp(lr, t, b1, b2))
    u = U32
    gs = scale * g
    dec = wd * w
    if mode == "l2":
        gp = gs + dec
        Eg = 3 * u * (gs.abs() + dec.abs())
    else:
        gp = gs
        Eg = 3 * u * gs.abs()
    m1, m2 = b1 * m, omb1 * gp
    m_new = m1 + m2
    Bm = 3 * u * (m1.abs() + m2.abs()) + omb1 * Eg
    v1, v2 = b2 * v, omb2 * gp * gp
    v_new = v1 + v2
    Bv = 4 * u * (v1.abs() + v2) + omb2 * (2 * gp.abs() * Eg + Eg * Eg)
    r = v_new.sqrt()
    Er = torch.where(r > 0, Bv / r.clamp_min(1e-300), torch.zeros_like(r)) + u * r
    assert bool((Bv[r == 0] == 0).all())
    d = r + eps
    Ed = Er + u * d
    assert bool((d - Ed > 0).all())
    q = m_new / d
    Eq = (Bm + q.abs() * Ed) / (d - Ed) + u * q.abs()
    step = alpha * q
    lrdec = lr * dec if mode == "decoupled" else torch.zeros_like(w)
    w_new = w - step - lrdec
    Bw = (abs(alpha) * Eq + 4 * u * step.abs() + 3 * u * lrdec.abs()
          + 2 * u * (w.abs() + step.abs() + lrdec.abs()))
    return w_new, m_new, v_new, Bw, Bm, Bv, alpha


def adam_closed_form_first_step(g, lr, b1, b2, eps):
    """w - w' of the step t = 1 from zero moments without decay: m' = (1 - b1) g, v' =
    (1 - b2) g^2 and alpha = lr sqrt(1 - b2) / (1 - b1), so with eps outside the correction
    (tf.train.AdamOptimizer's form)
    lr sqrt(1 - b2) g / (sqrt(1 - b2) |g| + eps) = lr g / (|g| + eps / sqrt(1 - b2))."""
    g = g.double()
    return lr * g / (g.abs() + eps / math.sqrt(1.0 - b2))
