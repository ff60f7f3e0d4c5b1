"""An independent fp64 reference for the weight EMA (csrc/ema.hip ema_update, and the CPU
backend's fp32 torch twin) and the bound its tests use.  Like tests/optim_oracle.py and
tests/lars_oracle.py it is plain fp64 arithmetic, and the tolerance is derived, not fitted
to what the kernel gives.

Semantics (per element; k = the number of completed steps, `decay` the fp64 flag value):
    om     = max(1 - decay, 9 / (10 + k))   with warm-up, else 1 - decay
    shadow = shadow - om * (shadow - master)
which is TF's  shadow -= (1 - d) * (shadow - var),  d = min(decay, (1 + k) / (10 + k)).

Bound
-----
u = 2**-24 (fp32 unit roundoff).  s, m are the fp32 inputs, taken exactly.

om, OM_REL = 2 u relative:
  without warm-up the kernel uses the one fp32 value the host passes, fl(1 - decay): one
  rounding of the fp64 difference, u.  With warm-up it forms fl(9 / fl(10 + k)): the
  int64 -> fp32 conversion rounds once (u; exact below 2**24) and the IEEE division once
  (u), 2 u (1 + O(u)) together; the max of two values each within 2 u of its exact
  counterpart is within 2 u of the exact max.

update, B = |om (s - m)| (2 u + OM_REL) + u |r|,  r = s - om (s - m) exact:
  unfused, d = fl(s - m) (u), p = fl(om_k d) (u), result fl(s - p) (u of the result): the
  product carries the rounding of the difference, its own and om's error, (2 u + OM_REL)
  relative to |om (s - m)|, and the last subtraction rounds once relative to the value it
  returns.  Fused (an FMA for the product and the subtraction) drops the product's
  rounding, so the same expression covers it.  The tests use 2 B: room for the
  second-order terms (products of two roundings) and for |r| being taken at the reference
  instead of the computed value.
"""
import numpy as np
import torch

U32 = 2.0 ** -24
OM_REL = 2 * U32
ROOM = 2.0


def f32(x):
    return float(np.float32(x))


def om_reference(decay, k, warm):
    """The exact (fp64) rate 1 - d_k of step count k."""
    om = 1.0 - float(decay)
    return max(om, 9.0 / (10.0 + float(k))) if warm else om


def ema_reference(shadow, master, decay, k, warm):
    """One EMA update in fp64 from fp32 (or fp64) tensors.  Returns (shadow', bound): the
    exact result and the per-element error bound of a correct fp32 evaluation, room
    included (module docstring)."""
    s, m = shadow.double(), master.double()
    om = om_reference(decay, k, warm)
    p = om * (s - m)
    r = s - p
    return r, ROOM * (p.abs() * (2 * U32 + OM_REL) + U32 * r.abs())


def ema_recurrence(shadow0, masters, decay, warm, k0=0):
    """shadow after len(masters) updates; update j (0-based) sees masters[j] and k = k0 + j + 1
    (the step's global_step += 1 precedes it)."""
    s = float(shadow0)
    for j, m in enumerate(masters):
        s -= om_reference(decay, k0 + j + 1, warm) * (s - float(m))
    return s
