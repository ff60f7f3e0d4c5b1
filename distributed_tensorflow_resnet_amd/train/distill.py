"""Knowledge distillation (Hinton, Vinyals, Dean 2015): a frozen teacher's logits in the
training loss.

With z the student row, t the teacher row on the same input, tau the temperature, alpha the
soft weight, and L_h / t_c the hard loss and target (label smoothing and mixup included):

    q = softmax(t / tau)     p = softmax(z)     p_tau = softmax(z / tau)
    loss = (1 - alpha) * L_h + alpha * tau^2 * sum_c q_c * (log q_c - log p_tau_c)
    g_c  = ((1 - alpha) * (p_c - t_c) + alpha * tau * (p_tau_c - q_c)) * grad_scale

GPU: the teacher is a second, inference-only Engine of its own depth (DeviceTeacher).  Its
forward is ONE prn_infer launch on the main stream between the step's input launches and
the student's forward, reading the student's x_in (after every augmentation) and writing
only the teacher logits [N][kpad]; whichever loss head the plan records reads them through
csrc/xent_row.h.  CPU: soft_loss below, in fp32 torch, with a TorchResNet teacher in eval
mode.  The teacher is not checkpointed with the student; every rank runs its own.
"""
from __future__ import annotations

import torch

from ..models.params import ParamStore
from ..models.spec import ModelSpec, build_spec
from ..ops.reference import BN_EPS
from ..utils import tensor_bundle as tb
from ..utils.checkpoint import tf_to_state

IMAGENET_REASON = ("distillation runs the teacher through the persistent CIFAR inference "
                   "forward (prn_infer): CIFAR networks only")


def check_distill(alpha, temperature, has_teacher: bool, dataset: str = "cifar10"):
    """--distill_alpha / --distill_temperature as both backends take them -> (alpha, tau).
    alpha in [0, 1] (0 = off), tau > 0; alpha > 0 needs a teacher, and a teacher a CIFAR
    student."""
    try:
        alpha, tau = float(alpha), float(temperature)
    except (TypeError, ValueError):
        raise ValueError(f"distill_alpha and distill_temperature must be numbers, got "
                         f"{alpha!r}, {temperature!r}") from None
    if not 0.0 <= alpha <= 1.0:   # NaN included
        raise ValueError(f"distill_alpha must be in [0, 1], got {alpha!r}")
    if not 0.0 < tau < float("inf"):
        raise ValueError(f"distill_temperature must be finite and > 0, got {temperature!r}")
    if alpha > 0 and not has_teacher:
        raise ValueError("distill_alpha > 0 needs a teacher (--distill_teacher_dir)")
    if has_teacher and not dataset.startswith("cifar"):
        raise ValueError(IMAGENET_REASON)
    return alpha, tau


def load_teacher(directory: str, dataset: str, resnet_size: int, num_classes: int):
    """(teacher spec, checkpoint tensors) of the latest checkpoint in `directory`."""
    prefix = tb.latest_checkpoint(directory)
    if prefix is None:
        raise FileNotFoundError(f"--distill_teacher_dir {directory!r}: no checkpoint found")
    return build_spec(dataset, resnet_size, num_classes), tb.read_bundle(prefix)


def _check_classes(student: ModelSpec, teacher: ModelSpec):
    if teacher.num_classes != student.num_classes:
        raise ValueError(f"the distillation teacher has {teacher.num_classes} classes, the "
                         f"student {student.num_classes}")


def _load(store: ParamStore, weights):
    """`weights`: checkpoint tensors by TF name, or an int seed (random weights: tests)."""
    if isinstance(weights, int):
        store.initialize(weights)
    else:
        tf_to_state(weights, store, None, strict=True)


def soft_loss(z: torch.Tensor, t: torch.Tensor, tau: float) -> torch.Tensor:
    """Per-row tau^2 * KL(softmax(t / tau) || softmax(z / tau)) in the logsumexp form of
    csrc/xent_row.h (a teacher class whose q underflowed to 0 adds exactly 0)."""
    ls = z / tau - torch.logsumexp(z / tau, 1, keepdim=True)
    lq = t / tau - torch.logsumexp(t / tau, 1, keepdim=True)
    q = torch.exp(lq)
    return tau * tau * torch.where(q > 0, q * (lq - ls), torch.zeros_like(q)).sum(1)


class TorchTeacher:
    """The CPU backend's teacher: a TorchResNet in eval mode, fp32."""

    def __init__(self, student: ModelSpec, spec: ModelSpec, weights):
        from ..models.resnet_torch import TorchResNet

        _check_classes(student, spec)
        self.store = ParamStore(spec)
        _load(self.store, weights)
        self.model = TorchResNet(spec, self.store)

    def logits(self, x: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            return self.model(x, False).detach()


class DeviceTeacher:
    """The engine's teacher: an inference-only Engine of the teacher's depth (built the way
    GPUInference builds one), its PersistInfer tables, and the logits buffer the student's
    loss head reads."""

    def __init__(self, student, spec: ModelSpec, weights):
        from .engine import Engine, constant_lr
        from .persist import PersistInfer, infer_check

        _check_classes(student.spec, spec)
        reason = infer_check(student)
        if reason:
            raise ValueError(f"distillation student: {reason}")
        self.engine = Engine(spec, student.N, weight_decay=0.0, lr_schedule=constant_lr(0.0),
                             device=student.device, use_graph=False)
        reason = infer_check(self.engine)
        if reason:
            raise ValueError(f"distillation teacher: {reason}")
        assert self.engine.kpad == student.kpad
        _load(self.engine.params, weights)
        self.engine.repack()
        self.prn = PersistInfer(self.engine)
        self.logits = torch.zeros((student.N, student.kpad), device=student.device)

    def record(self, plan, x_in, N: int):
        """The one prn_infer launch: x_in -> self.logits (nothing else is written)."""
        return self.prn.record(plan, x_in, self.logits, N, BN_EPS)
