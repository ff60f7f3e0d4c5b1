"""Knowledge distillation without a GPU: the CPU backend's formulas against the fp64 rows of
tests/distill_oracle.py, the flags, and alpha == 0 as the plain step."""
import distill_oracle as do
import kernel_resources as kr
import numpy as np
import pytest
import torch

from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.ops import reference as ref
from distributed_tensorflow_resnet_amd.train.backends import CPUBackend
from distributed_tensorflow_resnet_amd.train.distill import (TorchTeacher, check_distill, load_teacher,
                                                            soft_loss)
from distributed_tensorflow_resnet_amd.train.engine import constant_lr
from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver
from distributed_tensorflow_resnet_amd.utils.flags import build_parser


def rows(N, K):
    """Student and teacher rows (exact in fp32), labels and partner labels (never the label);
    row 1's teacher and row 2's student have one logit 80 above the rest, so some q (p_tau)
    underflow to 0 in fp32."""
    g = torch.Generator().manual_seed(K)
    z = torch.randint(-32, 33, (N, K), generator=g).float() / 8
    t = torch.randint(-32, 33, (N, K), generator=g).float() / 8
    t[1, 3] = t[1].max() + 80
    z[2, K - 2] = z[2].max() + 80
    y = torch.randint(0, K, (N,), generator=g)
    return z, t, y, (y + 1 + torch.randint(0, K - 1, (N,), generator=g)) % K


@pytest.mark.parametrize("eps,lam", [(0.0, 1.0), (0.1, 0.3)])
@pytest.mark.parametrize("alpha", [0.3, 1.0])
@pytest.mark.parametrize("tau", [1.0, 4.0])
def test_torch_formulas_match_oracle(tau, alpha, eps, lam):
    z, t, y, yb = rows(5, 10)
    z.requires_grad_(True)
    mix = {} if lam == 1.0 else {"labels_b": yb, "lam": lam}
    hard = ref.softmax_cross_entropy(z, y, eps, **mix)   # mean over the rows
    soft = soft_loss(z, t, tau)
    ((1 - alpha) * hard + alpha * soft.mean()).backward()
    r = do.distill_rows(z.detach().numpy(), t.numpy(), y.numpy(), tau, alpha, eps,
                        None if lam == 1.0 else yb.numpy(), lam)
    assert torch.isfinite(soft).all() and torch.isfinite(z.grad).all()
    got = (1 - alpha) * float(hard.detach()) + alpha * float(soft.detach().mean())
    assert abs(got - r["loss"].mean()) <= do.loss_bound(tau, alpha)
    err = np.abs(z.grad.numpy() - r["grad"] / 5) / do.grad_bound(r, tau, alpha, 1 / 5)
    assert (err <= 1.0).all(), err.max()


def _backend(**kw):
    b = CPUBackend(cifar_spec(8, 10), 4, weight_decay=1e-4, lr_schedule=constant_lr(0.1), **kw)
    g = torch.Generator().manual_seed(1)
    b.set_batch(torch.randn(4, 32, 32, 3, generator=g), torch.randint(0, 10, (4,), generator=g))
    return b


def test_cpu_backend_logs_the_combined_loss():
    tau, alpha = 4.0, 0.5
    b = _backend(distill_alpha=alpha, distill_temperature=tau, label_smoothing=0.1,
                 distill_teacher=(cifar_spec(14, 10), 3))
    assert b.distill_state() is None
    b.step()
    z, t = b.last_logits.numpy(), b.distill_state().numpy()
    assert t.shape == (4, 10) and np.abs(t).max() > 0
    r = do.distill_rows(z, t, b._y.numpy(), tau, alpha, eps=0.1)
    m = b.metrics()
    assert abs(m["cross_entropy"] - r["loss"].mean()) <= do.loss_bound(tau, alpha)
    assert (m["distill_alpha"], m["distill_temperature"]) == (alpha, tau)


def test_alpha_zero_is_the_plain_step():
    plain, off = _backend(), _backend(distill_alpha=0.0, distill_teacher=(cifar_spec(14, 10), 3))
    assert off.teacher is None   # nothing is built
    for b in (plain, off):
        b.step()
    assert torch.equal(plain.store.master, off.store.master)
    assert torch.equal(plain.mom, off.mom)
    assert plain.metrics() == off.metrics()


def test_flags_and_arguments():
    p = build_parser("cifar")
    ns = p.parse_args([])
    assert (ns.distill_alpha, ns.distill_temperature, ns.distill_teacher_dir) == (0.0, 4.0, "")
    ns = p.parse_args(["--distill_alpha", "0.5", "--distill_teacher_dir", "d",
                       "--distill_teacher_size", "14", "--distill_temperature", "2"])
    assert (ns.distill_alpha, ns.distill_temperature, ns.distill_teacher_size) == (0.5, 2.0, 14)
    for bad in (["--distill_alpha", "0.5"],                                  # no teacher
                ["--distill_alpha", "1.5", "--distill_teacher_dir", "d"],
                ["--distill_alpha", "0.5", "--distill_teacher_dir", "d", "--distill_temperature", "0"],
                ["--distill_teacher_dir", "d", "--distill_teacher_size", "15"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit):   # ImageNet students are refused
        build_parser("imagenet").parse_args(["--distill_alpha", "0.5", "--distill_teacher_dir", "d"])
    with pytest.raises(ValueError, match="CIFAR"):
        check_distill(0.5, 4.0, True, "imagenet")
    with pytest.raises(ValueError, match="classes"):
        _backend(distill_alpha=0.5, distill_teacher=(cifar_spec(14, 100), 3))


def test_teacher_from_a_checkpoint_directory(tmp_path):
    """The path the flags take: the latest checkpoint of a directory -> load_teacher ->
    the teacher's weights and moving statistics."""
    src = _backend()
    src.store.stats.uniform_(0.5, 1.5)
    Saver(str(tmp_path), 2).save(src.state_tensors(), 7)
    spec, tensors = load_teacher(str(tmp_path), "cifar10", 8, 10)
    teacher = TorchTeacher(cifar_spec(8, 10), spec, tensors)
    assert torch.equal(teacher.store.master, src.store.master)
    assert torch.equal(teacher.store.stats, src.store.stats)
    assert torch.equal(teacher.logits(src._x), src.model(src._x, False).detach())


@pytest.mark.skipif(not kr.have_compiler(), reason="no ROCm compiler")
def test_teacher_forward_keeps_the_register_budget():
    """The persistent forward with the distillation head: no VGPR spill, no scratch, the
    occupancy and VGPR budget of the plain forward at the same slice count."""
    res = kr.prn_resources()
    kd = sorted(n for n in res if "prn_fwd_kd_kernel" in n)       # sorted: 1, 2, 4 slices
    plain = sorted(n for n in res if "prn_fwd_kernel" in n)
    assert len(kd) == len(plain) == 3, sorted(res)
    for k, p in zip(kd, plain):
        assert int(res[k]["VGPRs Spill"]) == 0 and int(res[k]["ScratchSize [bytes/lane]"]) == 0
        for key in ("Occupancy [waves/SIMD]", "LDS Size [bytes/block]"):
            assert res[k][key] == res[p][key], (k, key)
