"""An independent fp64 reference for the LARS kernels (csrc/lars.hip: lars_norms,
lars_trust, lars_update_pack) and the bounds their tests use.  Like tests/optim_oracle.py
it is plain fp64 / index arithmetic, and no tolerance is tuned to what the kernels give.

Semantics (per trainable tensor s; coefficients as the fp32 values the kernels receive):
    g^     = g * grad_scale
    wn, gn = ||w_s||, ||g^_s||
    trust  = eeta * wn / (gn + wd * wn + epsilon)   if adapted and wn > 0 and gn > 0, else 1
    g'     = g^ + wd * w,  acc = momentum * acc + g',  w -= (lr * trust) * acc

Bounds
------
u = 2**-24 (fp32 unit roundoff), as in optim_oracle.

sum of squares, SS_REL = 20 u relative:
  a lars_norms thread adds at most 18 squares in fp32 (4 float4s of a 4096-element chunk's
  aligned body, one head and one tail scalar): one rounding per square and at most 17 for
  the additions, every term non-negative, so each partial sum is <= the thread's exact sum
  and the thread's result is within 18 u (1 + O(u)) of it.  Everything after that -- the
  6 shuffle levels, the 4 waves, the chunks of a segment in chunk order -- is fp64:
  (9 + chunks) 2**-53, below 2**-40 for any tensor under 2**25 elements.  20 u leaves room
  for both and for the second-order terms.

norms, NORM_REL = 11 u relative:
  the square root halves the relative error of its argument (10 u (1 + O(u))); the fp64
  square root and product with |grad_scale| add ~2**-52; the result is rounded to fp32
  once for wn[] / gn[] (u).

trust, TRUST_REL = 22 u relative:
  in fp64, eeta * wn / (gn + wd * wn + epsilon): the numerator carries wn's 10 u; the
  denominator is a sum of non-negative terms each within 10 u (epsilon exactly), so within
  10 u; the quotient within 20 u (1 + O(u)); fp64 arithmetic ~2**-50; one rounding to fp32
  (u): 21 u, and one spare.  A skipped tensor and a zero norm give exactly 1.

update: w' within  B + |lr * trust * acc| * (TRUST_REL + u),  acc within B:
  B is sgd_reference's bound evaluated with the rate lr * trust_ref: the kernel does the
  same six fp32 operations with its own rate r = fl(lr * trust_kernel), which is within
  (TRUST_REL + u) of lr * trust_ref (the trust bound and the rounding of the product); the
  difference enters w' through the one product r * acc.  acc does not depend on the rate.
"""
import numpy as np
import torch

import optim_oracle as oo

U32 = oo.U32
SS_REL = 20 * U32
NORM_REL = 11 * U32
TRUST_REL = 22 * U32
RATE_REL = TRUST_REL + U32


def lars_norms_reference(w, g, seg_arr, grad_scale):
    """Per segment (sum w^2, sum g^2) and (wn, gn) in fp64, as lists."""
    w, g = w.double(), g.double()
    ssw, ssg = [], []
    for r in seg_arr:
        o, m = int(r["offset"]), int(r["numel"])
        ssw.append(float((w[o:o + m] ** 2).sum()))
        ssg.append(float((g[o:o + m] ** 2).sum()))
    wn = [float(np.sqrt(x)) for x in ssw]
    gn = [abs(grad_scale) * float(np.sqrt(x)) for x in ssg]
    return ssw, ssg, wn, gn


def trust_reference(wn, gn, skip, eeta, wd, epsilon):
    return [1.0 if (sk or a <= 0 or b <= 0) else eeta * a / (b + wd * a + epsilon)
            for a, b, sk in zip(wn, gn, skip)]


def lars_reference(w, g, mom, seg_arr, skip, lr, momentum, wd, grad_scale, eeta, epsilon):
    """One LARS step in fp64 over the flat buffers (the first sum(numel) elements).
    Returns (w', acc, Bw, Bacc, wn, gn, trust): the new weights and accumulator, the
    per-element error bounds of a correct fp32 evaluation (module docstring) and the
    per-segment norms and trust ratios."""
    n = int(seg_arr[-1]["offset"] + seg_arr[-1]["numel"])
    w, g, mom = w[:n], g[:n], mom[:n]
    _, _, wn, gn = lars_norms_reference(w, g, seg_arr, grad_scale)
    trust = trust_reference(wn, gn, skip, eeta, wd, epsilon)
    numel = torch.tensor([int(r["numel"]) for r in seg_arr], device=w.device)
    assert int(numel.sum()) == n and all(
        int(a["offset"] + a["numel"]) == int(b["offset"]) for a, b in zip(seg_arr, seg_arr[1:]))
    tv = torch.repeat_interleave(torch.tensor(trust, dtype=torch.float64, device=w.device), numel)
    w_new, acc, B = oo.sgd_reference(w, g, mom, lr * tv, momentum, wd, grad_scale, True)
    Bw = B + (lr * tv * acc).abs() * RATE_REL
    return w_new, acc, Bw, B, wn, gn, trust
