"""Learning-rate schedules: an optional linear warm-up, then the reference's piecewise-constant
steps or a cosine / polynomial decay, evaluated on the device by the optimizer kernels
(csrc/optim.h LrSchedule, csrc/optim_device.h lr_at) and mirrored on the host.  Pure Python:
importable without torch or the native module.

Cosine and polynomial decay (`decay` "cosine" / "poly"; W = warm_steps, D = decay_steps, the
peak is warm_to).  The reference's step-0 quirk is kept: training step s uses f(s - 1) and
step 0 uses init = f(0).  With t = s - 1:
  t < W    warm_from + (peak - warm_from) * t / W, in fp32 (the warm-up of every kind)
  t >= D   exactly end
  else     q = (D - t) / (D - W), lr = end + (peak - end) * F(q) in fp64, rounded to fp32
           once; F = sin(pi q / 2)^2 for cosine -- 0.5 (1 + cos(pi p)) at p = 1 - q without
           its cancellation at the end of the run -- and q^power for poly.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass, replace

DECAYS = ("piecewise", "cosine", "poly")


def _f32(x: float) -> float:
    """x rounded to fp32 (round to nearest even), as a Python float."""
    return struct.unpack("f", struct.pack("f", x))[0]


@dataclass
class LRSchedule:
    """LR schedule evaluated on the device (see csrc/optim.h LrSchedule)."""
    init: float
    bounds: list
    values: list
    warm_steps: int = 0
    warm_from: float = 0.0
    warm_to: float = 0.0
    decay: str = "piecewise"
    decay_steps: int = 0
    end: float = 0.0
    power: float = 2.0

    def __post_init__(self):
        if self.decay not in DECAYS:
            raise ValueError(f"lr decay must be one of {DECAYS}, got {self.decay!r}")
        if self.decay == "piecewise":
            return
        if not (isinstance(self.warm_steps, int) and isinstance(self.decay_steps, int)
                and self.decay_steps > self.warm_steps >= 0):
            raise ValueError(f"lr decay_steps must exceed the warm-up: need decay_steps > "
                             f"warm_steps >= 0, got {self.decay_steps!r} and {self.warm_steps!r}")
        if not (self.power > 0 and math.isfinite(self.power)):
            raise ValueError(f"lr poly power must be positive and finite, got {self.power!r}")
        for name in ("init", "warm_from", "warm_to", "end"):
            v = getattr(self, name)
            if not (math.isfinite(v) and v >= 0):
                raise ValueError(f"lr rates must be finite and >= 0, got {name} = {v!r}")

    def at(self, step: int) -> float:
        """Host mirror of the device formula (used by hooks/tests)."""
        if self.decay != "piecewise":
            return self._decay_at(step)
        if step <= 0:
            return self.init
        t = step - 1
        if t < self.warm_steps:
            return self.warm_from + (self.warm_to - self.warm_from) * t / self.warm_steps
        for b, v in zip(self.bounds, self.values):
            if t < b:
                return v
        return self.values[-1]

    def _decay_at(self, step: int) -> float:
        """Cosine / poly.  The rates are the fp32 values the kernels are handed, and the
        warm-up is the device's fp32 expression operation by operation (an fp64 result
        rounded to fp32 is the fp32 result for +, -, * and /)."""
        peak, end, w0 = _f32(self.warm_to), _f32(self.end), _f32(self.warm_from)
        if step <= 0:
            return _f32(self.init)
        t = step - 1
        W, D = self.warm_steps, self.decay_steps
        if t < W:
            prod = _f32(_f32(peak - w0) * _f32(float(t)))
            return _f32(w0 + _f32(prod / _f32(float(W))))
        if t >= D:
            return end
        q = float(D - t) / float(D - W)
        if self.decay == "cosine":
            f = math.sin(math.pi * (q / 2)) ** 2
        else:
            p = _f32(self.power)
            f = q if p == 1.0 else q * q if p == 2.0 else q ** p
        return _f32(end + (peak - end) * f)

    def launch_args(self) -> tuple:
        """The schedule as the optimizer launches take it, in their argument order:
        (init, warm_steps, warm_from, warm_to, bounds, values)."""
        return (self.init, self.warm_steps, self.warm_from, self.warm_to, list(self.bounds),
                list(self.values))

    def decay_args(self) -> tuple:
        """The trailing argument of the optimizer launches' decay overloads:
        (decay, decay_steps, end, power).  A piecewise schedule is launched without it."""
        return (self.decay, self.decay_steps, self.end, self.power)

    def extra_launch_args(self) -> tuple:
        """What follows an optimizer launch's own arguments: nothing for a piecewise
        schedule (the launch is recorded as it always was), else (decay_args(),)."""
        return () if self.decay == "piecewise" else (self.decay_args(),)


def cifar_lr_schedule() -> LRSchedule:
    """resnet_cifar_main.py:304-324 (begin() = 0.1)."""
    return LRSchedule(0.1, [40000, 60000, 80000], [0.1, 0.01, 0.001, 0.0001])


def imagenet_lr_schedule() -> LRSchedule:
    """resnet_imagenet_main.py:306-329: warm-up 0.1->0.4 over 6240 steps (begin()=0.4)."""
    return LRSchedule(0.4, [37440, 74880, 99840], [0.4, 0.04, 0.004, 0.0004],
                      warm_steps=6240, warm_from=0.1, warm_to=0.4)


def decay_lr_schedule(decay: str, peak: float, decay_steps: int, *, warm_steps: int = 0,
                      warm_from: float = 0.0, end: float = 0.0, power: float = 2.0) -> LRSchedule:
    """Warm-up from warm_from to peak over warm_steps, then cosine / poly decay to `end` at
    decay_steps (module docstring).  init = f(0): warm_from with a warm-up, else the peak."""
    if decay not in ("cosine", "poly"):
        raise ValueError(f"lr decay must be cosine or poly, got {decay!r}")
    return LRSchedule(warm_from if warm_steps > 0 else peak, [], [peak], warm_steps=warm_steps,
                      warm_from=warm_from, warm_to=peak, decay=decay, decay_steps=decay_steps,
                      end=end, power=power)


def scaled(s: LRSchedule, factor: float) -> LRSchedule:
    """The same schedule with its step boundaries (and warm-up length, and decay length)
    x factor."""
    if factor == 1.0:
        return s
    warm = int(round(s.warm_steps * factor))
    decay_steps = s.decay_steps
    if s.decay != "piecewise":
        decay_steps = max(warm + 1, int(round(s.decay_steps * factor)))
    return replace(s, bounds=[max(1, int(round(b * factor))) for b in s.bounds],
                   values=list(s.values), warm_steps=warm, decay_steps=decay_steps)


def lr_values_scaled(s: LRSchedule, factor: float) -> LRSchedule:
    """The same schedule with every LR value (the warm-up's ends, the peak and the decay's
    end) x factor."""
    if factor == 1.0:
        return s
    return replace(s, init=s.init * factor, bounds=list(s.bounds),
                   values=[v * factor for v in s.values], warm_from=s.warm_from * factor,
                   warm_to=s.warm_to * factor, end=s.end * factor)


def constant_lr(lr: float) -> LRSchedule:
    return LRSchedule(lr, [], [lr])


def schedule_from_flags(flags) -> LRSchedule:
    """The schedule of a run: the dataset's preset, changed by --lr_decay, --lr_peak,
    --lr_warmup_steps, --lr_warmup_from, --lr_decay_steps, --lr_end and --lr_poly_power
    (utils/flags.py; their defaults give the preset itself), before --lr_schedule_scale and
    --lr_value_scale.  Raises ValueError for values no schedule can be built from."""
    s = cifar_lr_schedule() if flags.dataset.startswith("cifar") else imagenet_lr_schedule()
    peak, warm, warm_from = flags.lr_peak, flags.lr_warmup_steps, flags.lr_warmup_from
    for name, v in (("--lr_peak", peak), ("--lr_warmup_from", warm_from),
                    ("--lr_end", flags.lr_end)):
        if v is not None and not (math.isfinite(v) and v >= 0):
            raise ValueError(f"{name} must be finite and >= 0, got {v!r}")
    power = flags.lr_poly_power
    if not (power > 0 and math.isfinite(power)):
        raise ValueError(f"--lr_poly_power must be positive and finite, got {power!r}")
    if flags.lr_decay == "piecewise":
        given = [n for n, v, d in (("--lr_decay_steps", flags.lr_decay_steps, 0),
                                   ("--lr_end", flags.lr_end, 0.0),
                                   ("--lr_poly_power", power, 2.0)) if v != d]
        if given:
            raise ValueError(f"{', '.join(given)} cannot be combined with --lr_decay piecewise: "
                             "the piecewise schedule has no decay length, end rate or power")
        if peak is not None:   # the preset's drops, relative to the new first value
            k = peak / s.values[0]
            s = replace(s, init=peak, values=[peak] + [v * k for v in s.values[1:]],
                        warm_from=s.warm_from * k, warm_to=peak if s.warm_steps else s.warm_to)
        if warm >= 0:
            s = replace(s, warm_steps=warm, warm_to=s.values[0])
        if warm_from is not None:
            s = replace(s, warm_from=warm_from)
        return s
    warm = s.warm_steps if warm < 0 else warm
    decay_steps = flags.lr_decay_steps or flags.train_steps
    if decay_steps <= warm:
        raise ValueError(f"--lr_decay_steps ({decay_steps}) must exceed the warm-up "
                         f"(--lr_warmup_steps: {warm} steps)")
    return decay_lr_schedule(flags.lr_decay, s.values[0] if peak is None else peak, decay_steps,
                             warm_steps=warm,
                             warm_from=s.warm_from if warm_from is None else warm_from,
                             end=flags.lr_end, power=power)
