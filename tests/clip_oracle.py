"""An independent fp64 reference for the clipping kernels (csrc/clip.hip: grad_sqnorm,
clip_scale, sgd_clip_update_pack) and the bounds their tests use.  Like tests/lars_oracle.py
it is plain fp64 arithmetic, and no tolerance is tuned to what the kernels give.

Semantics (c as the fp32 value the kernel receives; g^ the complete mean gradient):
    ss    = sum over [0, n) of g^^2,  norm = sqrt(ss)
    scale = 1 if norm <= c,  c / norm if norm > c,  NaN if ss is not finite
    acc   = momentum * acc + scale * g^ + wd * w,  w -= lr * acc      (the gradient stays)

Bounds
------
u = 2**-24 (fp32 unit roundoff), as in optim_oracle.

chunk partials and their sum, SS_REL = 20 u relative:
  a grad_sqnorm thread adds at most 17 squares in fp32 (4 float4s of a 4096-element chunk
  and one tail scalar; 18, lars_norms' count, is used): one rounding per square and at most
  17 for the additions, every term non-negative, so each partial sum is <= the thread's
  exact sum and the thread's result is within 18 u (1 + O(u)) of it.  Everything after
  that -- the 6 shuffle levels, the 4 waves, the chunks in chunk order -- is fp64:
  (9 + chunks) 2**-53, below 2**-40 for any gradient under 2**25 elements.  20 u leaves
  room for both and for the second-order terms.  All terms being non-negative, the bound
  holds for every partial and for their sum alike.

norm, NORM_REL = 11 u relative:
  the square root halves the relative error of its argument (10 u (1 + O(u))); the fp64
  square root adds ~2**-53; the result is rounded to fp32 once (u).

scale, SCALE_REL = 12 u relative when norm > c:
  c / norm in fp64 with norm within 10 u (1 + O(u)): the quotient is within 10 u
  (1 + O(u)), the fp64 division adds ~2**-53, one rounding to fp32 (u): 11 u, and one
  spare.  When norm <= c the scale is exactly 1; the tests keep c at least a factor 2 from
  the norm, far outside the 10 u in which the comparison itself could go either way.
  c = inf: every finite norm compares <= inf, exactly 1.

update: optim_oracle.sgd_reference with grad_scale = the fp32 scale the kernel wrote, and
  its own bound B: the kernel does the same six fp32 operations with that very number.
"""
import math

import optim_oracle as oo

U32 = oo.U32
SS_REL = 20 * U32
NORM_REL = 11 * U32
SCALE_REL = 12 * U32
CHUNK = 4096


def sumsq_reference(g, n):
    """(per-chunk fp64 sums of squares as a list, their total) over g[:n]."""
    sq = g[:n].double() ** 2
    parts = [float(sq[o:o + CHUNK].sum()) for o in range(0, n, CHUNK)]
    return parts, float(sq.sum())


def scale_reference(ss: float, c: float):
    """(norm, scale) in fp64 from the exact sum of squares and the fp32 clip value."""
    if not math.isfinite(ss):
        return math.sqrt(ss) if ss == math.inf else math.nan, math.nan
    norm = math.sqrt(ss)
    return norm, (c / norm if norm > c else 1.0)


def check_norm_scale(norm_k: float, scale_k: float, ss: float, c: float, what=""):
    """The kernel's fp32 (norm, scale) against the fp64 values of `ss` and clip value c."""
    norm, scale = scale_reference(ss, oo.f32(c))
    assert abs(norm_k - norm) <= NORM_REL * norm, (what, "norm", norm_k, norm)
    if scale == 1.0:
        assert scale_k == 1.0, (what, "scale of an unclipped step", scale_k, norm, c)
    else:
        assert abs(scale_k - scale) <= SCALE_REL * scale, (what, "scale", scale_k, scale)
    return norm, scale
