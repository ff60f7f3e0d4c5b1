"""Learning-rate schedules: piecewise-constant with an optional linear warm-up, evaluated
on the device by the optimizer kernels (csrc/optim.h LrSchedule) and mirrored on the
host.  Pure Python: importable without torch or the native module."""
from __future__ import annotations

from dataclasses import dataclass


@dataclass
class LRSchedule:
    """Piecewise LR evaluated on the device (see csrc/optim.h LrSchedule)."""
    init: float
    bounds: list
    values: list
    warm_steps: int = 0
    warm_from: float = 0.0
    warm_to: float = 0.0

    def at(self, step: int) -> float:
        """Host mirror of the device formula (used by hooks/tests)."""
        if step <= 0:
            return self.init
        t = step - 1
        if t < self.warm_steps:
            return self.warm_from + (self.warm_to - self.warm_from) * t / self.warm_steps
        for b, v in zip(self.bounds, self.values):
            if t < b:
                return v
        return self.values[-1]

    def launch_args(self) -> tuple:
        """The schedule as the optimizer launches take it, in their argument order:
        (init, warm_steps, warm_from, warm_to, bounds, values)."""
        return (self.init, self.warm_steps, self.warm_from, self.warm_to, list(self.bounds),
                list(self.values))


def cifar_lr_schedule() -> LRSchedule:
    """resnet_cifar_main.py:304-324 (begin() = 0.1)."""
    return LRSchedule(0.1, [40000, 60000, 80000], [0.1, 0.01, 0.001, 0.0001])


def imagenet_lr_schedule() -> LRSchedule:
    """resnet_imagenet_main.py:306-329: warm-up 0.1->0.4 over 6240 steps (begin()=0.4)."""
    return LRSchedule(0.4, [37440, 74880, 99840], [0.4, 0.04, 0.004, 0.0004],
                      warm_steps=6240, warm_from=0.1, warm_to=0.4)


def scaled(s: LRSchedule, factor: float) -> LRSchedule:
    """The same schedule with its step boundaries (and warm-up length) x factor."""
    if factor == 1.0:
        return s
    return LRSchedule(s.init, [max(1, int(round(b * factor))) for b in s.bounds], list(s.values),
                      int(round(s.warm_steps * factor)), s.warm_from, s.warm_to)


def lr_values_scaled(s: LRSchedule, factor: float) -> LRSchedule:
    """The same schedule with every LR value (and the warm-up's ends) x factor."""
    if factor == 1.0:
        return s
    return LRSchedule(s.init * factor, list(s.bounds), [v * factor for v in s.values],
                      s.warm_steps, s.warm_from * factor, s.warm_to * factor)


def constant_lr(lr: float) -> LRSchedule:
    return LRSchedule(lr, [], [lr])
