"""An independent fp64 reference for the RMSProp kernel (csrc/rmsprop.hip rmsprop_update_pack)
and the bounds its tests use.  Like tests/lion_oracle.py it is plain fp64 / index arithmetic;
nothing calls the kernel or the host mirrors of it, and no tolerance is tuned to what the kernel
gives.

Semantics (TF 1.12 ApplyRMSProp / ApplyCenteredRMSProp per element; s the gradient's scale, wd
the decay of the element's tensor; coefficients as the fp32 values the kernel receives, 1 - rho
as the fp32 rounding of the fp64 difference, which is what the host passes):
    g'   = s * g (+ wd * w                    in "l2" mode)
    ms'  = rho * ms + (1 - rho) * (g' * g')
    mg'  = rho * mg + (1 - rho) * g'          (centered only)
    d    = ms' + eps                          (centered: (ms' - mg' * mg') + eps)
    mom' = momentum * mom + (lr * g') / sqrt(d)
    w'   = w - mom' (- (lr * wd) * w, the old w, in "decoupled" mode)

Bounds
------
u = 2**-24 (fp32 unit roundoff), as in optim_oracle.  The kernel evaluates every product, sum,
difference, square root and quotient in fp32 with contraction off: each rounds once, by at most
u relative to its result; sqrtf and / are the correctly rounded ones of csrc/adam.hip, so the
per-operation bound of tests/adam_oracle.py ("sqrtf and / are correctly rounded": one u each)
carries over.  |x| below is the fp64 reference's value.  The bounds are first order in u; every
one carries the factor (1 + 64 u), which covers the second-order terms of the at most 16
roundings on any path ((1 + u)^16 - 1 - 16 u < 128 u^2).

g':   decoupled: Eg = u |s g| (one product; exactly 0 for s = 1).
      l2: Eg = 2 u (|s g| + |wd w|): two products, and a sum no larger than the two magnitudes.
g'^2: Eq2 = 2 |g'| Eg + Eg^2 + u g'^2.  (g' + e)^2 - g'^2 = 2 g' e + e^2; one rounding.
ms':  Bms = 3 u (rho ms + (1 - rho) g'^2) + (1 - rho) (2 |g'| Eg + Eg^2).  The path of the
      second term has three roundings (square, product, sum), the first's two; g''s error
      through the square and its coefficient.  Both terms are non-negative for ms >= 0.
mg':  Bmg = 3 u (|rho mg| + |(1 - rho) g'|) + (1 - rho) Eg.  Two products and a sum.
mg'^2:  Em2 = 2 |mg'| Bmg + Bmg^2 + u mg'^2.
d:    plain:    Ed = Bms + u (ms' + eps).  One sum.
      centered: Ed = Bms + Em2 + u (|ms'| + |mg'^2|) + u (|ms'| + |mg'^2| + eps).  The
      difference ms' - mg'^2 CANCELS: its rounding and the errors of its operands are bounded
      by the operands' magnitudes |ms'| + |mg'^2|, not by the result.  The test data keeps it
      well conditioned: ms' >= 4 mg'^2 for every element of the reference (assert_conditioned:
      a condition on the data, asserted on the oracle alone), so d >= 3/4 ms'.
r = sqrt(d):  Er = Ed / r + u r.  |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <=
      |a - b| / sqrt(b) with b the reference's d; one rounding.  (d - Ed > 0 asserted.)
num = lr * g':  En = |lr| Eg + u |num|.  lr is the fp32 rate the kernel reports (lr_out).
q = num / r:  Eq = (En + |q| Er) / (r - Er) + u |q|.  |n_k / r_k - n / r| =
      |(n_k - n) r - n (r_k - r)| / (r r_k) <= (En r + |n| Er) / (r (r - Er)); one rounding.
      (r - Er > 0 asserted.)
mom': Bmom = 2 u |momentum mom| + u |q| + Eq.  A product, and a sum no larger than
      |momentum mom| + |q|.
w':   Bw = Bmom + u (|w| + |mom'|)  (+ 2 u |p| + u (|w| + |mom'| + |p|) with p = (lr wd) w in
      decoupled mode: lr * wd rounds once, its product with w once, and the second difference).
An element with g = mom = 0 and wd = 0 has Bmom = 0; the tests ask more of it (w and mom bit for
bit unchanged, ms' the one rounding of rho * ms).  A NaN in g gives NaN in that element's ms',
mg', mom' and w' and in no other; check() asks exactly that.  There is no undecided class: every
element is held to its bound.
"""
import torch

import optim_oracle as oo

U32 = oo.U32
SO = 1.0 + 64.0 * U32


def rmsprop_inputs(n, seed, wd_max=0.3):
    """Seeded test data: normal w; g and mom at magnitudes 1e-3 to 1; mg at 1e-3 to 0.3; and
    ms = 4 mg^2 + 4 (|g| + wd_max |w|)^2 (1 + rand), so that for every rho in [0.5, 1), scale
    in [0, 1] and decay <= wd_max the updated state keeps ms' >= 4 mg'^2:
    mg'^2 <= rho mg^2 + (1 - rho) g'^2 (convexity) and |g'| <= |g| + wd_max |w| give
    ms' - 4 mg'^2 >= rho (ms - 4 mg^2) - 3 (1 - rho) g'^2 >= (4 rho - 3 (1 - rho)) g'^2 > 0."""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 10.0 ** (-3.0 * torch.rand(n, generator=gen))
    mom = torch.randn(n, generator=gen) * 10.0 ** (-3.0 * torch.rand(n, generator=gen))
    mg = 0.3 * torch.randn(n, generator=gen).clamp(-1, 1) * 10.0 ** (-2.5 * torch.rand(n, generator=gen))
    gmax = g.abs() + wd_max * w.abs()
    ms = 4 * mg * mg + 4 * gmax * gmax * (1 + torch.rand(n, generator=gen))
    return w, g, ms, mg, mom


class RmsRef(dict):
    """{"w", "ms", "mg", "mom"}: the new state (mg None when plain); {"Bw", "Bms", "Bmg",
    "Bmom"}: the per-element bounds; "d", "mg2": the denominator's terms."""


def rmsprop_reference(w, g, ms, mg, mom, seg_arr, wd_seg, lr, rho, momentum, eps, scale,
                      centered, mode):
    """One RMSProp step in fp64 over the flat buffers (the first sum(numel) elements).  seg_arr:
    the ParamSeg table (contiguous segments), wd_seg: the per-segment decay; the coefficients
    are rounded to fp32 here, as the kernel's float arguments are.  mg is ignored unless
    centered.  Returns an RmsRef (module docstring)."""
    assert mode in ("l2", "decoupled")
    n = int(seg_arr[-1]["offset"] + seg_arr[-1]["numel"])
    numel = torch.tensor([int(r["numel"]) for r in seg_arr], device=w.device)
    assert int(numel.sum()) == n and len(wd_seg) == len(seg_arr) and all(
        int(a["offset"] + a["numel"]) == int(b["offset"]) for a, b in zip(seg_arr, seg_arr[1:]))
    w, g, ms, mom = (x[:n].double() for x in (w, g, ms, mom))
    lr, rho, momentum, eps, scale = (oo.f32(x) for x in (lr, rho, momentum, eps, scale))
    omr = oo.f32(1.0 - rho)
    wd = torch.repeat_interleave(
        torch.tensor([oo.f32(x) for x in wd_seg], dtype=torch.float64, device=w.device), numel)
    u = U32
    zero = torch.zeros_like(w)
    gs = scale * g
    dec = wd * w
    if mode == "l2":
        gp = gs + dec
        Eg = 2 * u * (gs.abs() + dec.abs())
    else:
        gp = gs
        Eg = u * gs.abs() if scale != 1.0 else zero
    g2 = gp * gp
    s1, s2 = rho * ms, omr * g2
    ms_new = s1 + s2
    Bms = 3 * u * (s1.abs() + s2) + omr * (2 * gp.abs() * Eg + Eg * Eg)
    if centered:
        mg = mg[:n].double()
        a1, a2 = rho * mg, omr * gp
        mg_new = a1 + a2
        Bmg = 3 * u * (a1.abs() + a2.abs()) + omr * Eg
        mg2 = mg_new * mg_new
        Em2 = 2 * mg_new.abs() * Bmg + Bmg * Bmg + u * mg2
        d0 = ms_new - mg2
        mag = ms_new.abs() + mg2          # the cancelling difference: by its operands
        d = d0 + eps
        Ed = Bms + Em2 + u * mag + u * (mag + eps)
    else:
        mg_new, Bmg, mg2 = None, None, zero
        d = ms_new + eps
        Ed = Bms + u * (ms_new.abs() + eps)
    fin = torch.isfinite(d)
    assert bool((d - Ed > 0)[fin].all()), "d within its own error of 0"
    r = d.sqrt()
    Er = Ed / r + u * r
    assert bool((r - Er > 0)[fin].all())
    num = lr * gp
    En = abs(lr) * Eg + u * num.abs()
    q = num / r
    Eq = (En + q.abs() * Er) / (r - Er) + u * q.abs()
    c = momentum * mom
    mom_new = c + q
    Bmom = 2 * u * c.abs() + u * q.abs() + Eq
    w_new = w - mom_new
    Bw = Bmom + u * (w.abs() + mom_new.abs())
    if mode == "decoupled":
        p = (lr * wd) * w
        w_new = w_new - p
        Bw = Bw + 2 * u * p.abs() + u * (w.abs() + mom_new.abs() + p.abs())
    ref = RmsRef(w=w_new, ms=ms_new, mg=mg_new, mom=mom_new, Bw=Bw * SO, Bms=Bms * SO,
                 Bmg=Bmg * SO if centered else None, Bmom=Bmom * SO, d=d, mg2=mg2)
    return ref


def assert_conditioned(ref, what=""):
    """The condition on a centered test's data, on the oracle alone: ms' >= 4 mg'^2 for every
    (finite) element, so the cancelling difference keeps at least 3/4 of ms'.  Returns the
    smallest ms' / mg'^2."""
    assert ref["mg"] is not None, what
    ms, mg2 = ref["ms"], ref["mg2"]
    fin = torch.isfinite(ms) & torch.isfinite(mg2)
    bad = (fin & ~(ms >= 4 * mg2)).nonzero().flatten()
    assert bad.numel() == 0, (what, "ms' < 4 mg'^2", bad[:8].tolist())
    return float((ms / mg2.clamp_min(1e-300))[fin].min())


def check(w_k, ms_k, mg_k, mom_k, ref, what=""):
    """The kernel's (or a backend's) w', ms', mg', mom' against the reference: each within its
    bound, NaN exactly where the reference has one; every element counts.  mg_k is ignored for
    a plain reference.  Returns the worst err / bound per buffer as a dict."""
    n = ref["w"].numel()
    nan = torch.isnan(ref["ms"])
    worst = {}
    for key, x_k in (("ms", ms_k), ("mg", mg_k), ("mom", mom_k), ("w", w_k)):
        x_ref, B = ref[key], ref["B" + key]
        if x_ref is None:
            continue
        x_k = x_k[:n].double()
        assert torch.equal(torch.isnan(x_ref), nan), (what, key, "the reference's NaNs")
        assert torch.equal(torch.isnan(x_k), nan), (what, "NaNs of " + key)
        ok = ~nan
        err = (x_k - x_ref).abs()
        bad = (ok & ~(err <= B)).nonzero().flatten()
        assert bad.numel() == 0, (what, key, bad[:8].tolist(),
                                  float((err / B.clamp_min(1e-300))[ok].max()))
        worst[key] = float((err / B.clamp_min(1e-300))[ok].max())
    return worst
