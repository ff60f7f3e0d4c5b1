"""An independent reference for the cosine and polynomial learning-rate decay
(csrc/optim_device.h lr_decay_at, train/schedule.py LRSchedule.at), and the steps and
schedules at which the tests compare them.

The decay is computed in its textbook form -- 0.5 * (1 + cos(pi * p)) and (1 - p)**power with
p = (t - W) / (D - W) -- in mpmath at 60 digits, from the fp32-rounded parameters (the values
a kernel's float arguments hold), and rounded to fp32 once, directly from the 60-digit value.
The kernel and the host mirror use the rewritten sin(pi q / 2)**2 in fp64: nothing is shared.

Tolerance (derived, not measured).  The fp64 chain -- one quotient, sinpi or a product or
exp(power * log q), one difference, one fma or product and sum -- has a relative error of a few
2**-53 (~1e-16; the general power adds power * |log q| * 2**-53, below 1e-14 here), against
an fp32 half-ulp of 2**-24 (6e-8).  So its fp32 rounding can differ from the correctly rounded
value only when the exact value lies within ~1e-14 relative of a rounding boundary, and then
by one ulp: device and mirror must each be within ONE fp32 ulp of the oracle.  From t = D on
the rate is exactly float32(end); for t < W it is the fp32 warm-up expression, operation by
operation (numpy float32 arithmetic is IEEE, like the device's), exactly.
"""
import mpmath
import numpy as np

from distributed_tensorflow_resnet_amd.train.schedule import decay_lr_schedule

MP = mpmath.mp.clone()
MP.dps = 60


def f32(x: float) -> float:
    return float(np.float32(x))


def _round_f32(x) -> float:
    """The 60-digit x rounded to fp32 in one rounding (to nearest even; the rates here
    are far above fp32's subnormals)."""
    with MP.workprec(24):
        r = float(+x)   # unary plus rounds to the working precision
    assert r == 0.0 or abs(r) > 2.0 ** -120
    return r


def in_warmup(s, step: int) -> bool:
    return step >= 1 and step - 1 < s.warm_steps


def lr_oracle(s, step: int) -> float:
    """The fp32 rate of training step `step` (the value of global_step when it starts)."""
    peak, end, w0 = f32(s.warm_to), f32(s.end), f32(s.warm_from)
    W, D = int(s.warm_steps), int(s.decay_steps)
    if step < 1:
        return w0 if W > 0 else peak          # f(0)
    t = step - 1
    if t < W:
        a, b = np.float32(w0), np.float32(peak)
        return float(a + (b - a) * np.float32(t) / np.float32(W))
    if t >= D:
        return end
    p = MP.mpf(t - W) / MP.mpf(D - W)
    if s.decay == "cosine":
        F = (1 + MP.cos(MP.pi * p)) / 2
    else:
        assert s.decay == "poly"
        F = (1 - p) ** MP.mpf(f32(s.power))
    return _round_f32(MP.mpf(end) + (MP.mpf(peak) - MP.mpf(end)) * F)


def ulp(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))


def check_rate(s, step: int, got: float, what="") -> float:
    """`got` (an fp32 value) against the oracle as the module docstring derives; returns
    the oracle's rate."""
    ref = lr_oracle(s, step)
    if in_warmup(s, step) or step < 1 or step - 1 >= s.decay_steps:
        assert got == ref, (what, step, got, ref)
    else:
        assert abs(got - ref) <= ulp(ref), (what, step, got, ref, (got - ref) / ulp(ref))
    return ref


def steps_of(W: int, D: int):
    """The steps at which a decay schedule can go wrong (the device looks at step - 1)."""
    s = {0, 1, 2, (W + D) // 2, 2 ** 31 + 5}
    s |= {W - 1, W, W + 1, W + 2}
    s |= {D - 1, D, D + 1, D + 2, D + 3}
    return sorted(x for x in s if x >= 0)


def _mk(decay, W, D, power=2.0, peak=0.1, end=0.0, warm_from=0.01):
    return decay_lr_schedule(decay, peak, D, warm_steps=W, warm_from=warm_from if W else 0.0,
                             end=end, power=power)


def cases():
    """{name: (schedule, steps)}.  Rates that are not fp32 numbers; a non-zero end in some."""
    out = {}
    for W, D in ((0, 5), (2, 7), (6240, 112590)):
        out[f"cosine_{W}_{D}"] = (_mk("cosine", W, D, peak=0.1 if D < 100 else 0.4 * 1.1,
                                      end=0.0 if W else 0.001), steps_of(W, D))
        for power in (1.0, 2.0, 0.5, 3.0):
            out[f"poly{power:g}_{W}_{D}"] = (_mk("poly", W, D, power, peak=0.3,
                                                 end=0.0 if power != 3.0 else 0.0007),
                                             steps_of(W, D))
    # the cancellation case: 1 + cos(pi p) at p = 1 - 1e-6 (t = D - 1)
    W, D = 1000, 1000 + 10 ** 6
    for name, sch in (("cosine", _mk("cosine", W, D)),
                      ("cosine_end", _mk("cosine", W, D, end=1e-5)),
                      ("poly2", _mk("poly", W, D)), ("poly0.5", _mk("poly", W, D, 0.5))):
        out[f"{name}_cancel"] = (sch, [D - 2, D - 1, D, D + 1])
    # differences that do not fit 32 bits
    D = 2 ** 33
    big = [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 32 + 2, 2 ** 31 + 5, D - 1, D, D + 1, D + 2]
    out["cosine_2^33"] = (_mk("cosine", 0, D), big)
    out["poly2_2^33"] = (_mk("poly", 0, D, end=0.002), big)
    out["poly3_warm_2^33"] = (_mk("poly", 2 ** 32 - 7, D, 3.0), [1, 2 ** 31 + 5] + big)
    return out
