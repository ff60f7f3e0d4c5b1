"""--optimizer lion without a GPU: the oracle (tests/lion_oracle.py) on its own, the CPU
backend's update against the oracle, the flags, the checkpoint entries and the restore rules,
and the compiler's resource remarks of csrc/lion.hip."""
import os

import numpy as np
import pytest
import torch

import kernel_resources as kr
import lion_oracle as lio
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.train.backends import CPUBackend
from distributed_tensorflow_resnet_amd.train.layout import (OPT_FUSED_LION_REASON, OPTIMIZERS,
                                                              SEG_DTYPE, check_lion)
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr
from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver
from distributed_tensorflow_resnet_amd.utils.flags import build_parser


def _one_seg(n):
    seg = np.zeros(1, dtype=SEG_DTYPE)
    seg["numel"] = n
    return seg


# ---------------------------------------------------------------- the oracle on its own
def test_oracle_exact_values():
    """b1 = 0.5, b2 = 0.75, lr = 0.125 and the data are exact in fp32: the step by hand."""
    w = torch.tensor([1.0, 2.0, -3.0, 0.5])
    g = torch.tensor([0.5, -2.0, 0.0, float("nan")])
    m = torch.tensor([0.25, 1.0, 0.0, 0.0])
    ref = lio.lion_reference(w, g, m, _one_seg(4), [0.5], 0.125, 0.5, 0.75, 1.0)
    w1, m1, Bw, Bm, Bc, decided = ref
    # c = (0.375, -0.5, 0, nan)
    assert w1[:3].tolist() == [1.0 - 0.125 - 0.0625, 2.0 + 0.125 - 0.125, -3.0 + 0.1875]
    assert m1[:3].tolist() == [0.1875 + 0.125, 0.75 - 0.5, 0.0]
    assert decided[:3].tolist() == [True, True, False] and float(Bc[2]) == 0.0
    assert bool(torch.isnan(w1[3])) and bool(torch.isnan(m1[3]))
    assert lio.undecided_share(ref) == 0.0


def test_oracle_refuses_exact_cancellation():
    with pytest.raises(AssertionError):
        lio.lion_reference(torch.ones(1), torch.ones(1), -torch.ones(1), _one_seg(1), [0.0], 0.125,
                           0.5, 0.75, 1.0)


@pytest.mark.parametrize("seed", [31, 32, 34, 35])
@pytest.mark.parametrize("b1,b2,scale", [(0.9, 0.99, 1.0), (0.0, 0.5, 0.37)])
def test_oracle_undecided_share_of_the_test_data(seed, b1, b2, scale):
    """The seeds the GPU tests use: a handful in 1e5 at the most."""
    n = 100003
    w, g, m = lio.lion_inputs(n, seed)
    ref = lio.lion_reference(w, g, m, _one_seg(n), [0.1], 1e-3, b1, b2, scale)
    assert lio.assert_decidable(ref) <= 1e-4
    # an fp32 numpy evaluation, each operation rounded once, passes check()
    f = np.float32
    gp = f(scale) * g.numpy()
    c = f(b1) * m.numpy() + f(1.0 - float(f(b1))) * gp
    u = np.where(c > 0, f(1), np.where(c < 0, f(-1), c)).astype(f)
    m1 = f(b2) * m.numpy() + f(1.0 - float(f(b2))) * gp
    w1 = (w.numpy() - f(1e-3) * u) - (f(1e-3) * f(0.1)) * w.numpy()
    assert w1.dtype == f and m1.dtype == f
    worst = lio.check(torch.from_numpy(w1), torch.from_numpy(m1), ref, 1e-3)
    assert max(worst) <= 1.0
    # and a wrong sign, a missing decay or swapped betas do not
    for bad_w, bad_m in ((w.numpy() + f(1e-3) * u, m1), (w.numpy() - f(1e-3) * u, m1),
                         (w1, f(b1) * m.numpy() + f(1.0 - float(f(b1))) * gp)):
        with pytest.raises(AssertionError):
            lio.check(torch.from_numpy(bad_w.astype(f)), torch.from_numpy(bad_m.astype(f)), ref, 1e-3)


# ---------------------------------------------------------------- CPU backend against the oracle
def _seg_of(store):
    seg = np.zeros(len(store.train_slots), dtype=SEG_DTYPE)
    for r, s in zip(seg, store.train_slots):
        r["offset"], r["numel"] = s.offset, s.numel
    return seg


@pytest.mark.parametrize("skip,clip,b1", [("none", 0.0, 0.9), ("vectors", 0.0, 0.0),
                                          ("vectors", 0.05, 0.9)])
def test_cpu_backend_lion_step_matches_oracle(skip, clip, b1):
    """Two steps (the second from a non-zero m) of the backend's own fp32 gradient through the
    oracle: the CPU backend is the kernel's expressions in fp32 torch, so the kernel's bounds
    hold for it."""
    spec = cifar_spec(8)
    wd, lr, b2 = 0.05, 1e-3, 0.99
    be = CPUBackend(spec, 4, weight_decay=wd, lr_schedule=constant_lr(lr), optimizer="lion",
                    lion_beta1=b1, lion_beta2=b2, lion_decay_skip=skip, clip_grad_norm=clip)
    assert be.lion and be.adam_state() is None and be.lamb_state() is None
    seg = _seg_of(be.store)
    wd_seg = [0.0 if skip == "vectors" and len(s.shape) == 1 else wd for s in be.store.train_slots]
    assert 0.0 in wd_seg or skip == "none"
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, 32, 32, 3, generator=gen)
    y = torch.randint(0, 10, (4,), generator=gen)
    for step in range(2):
        w0, m0 = be.store.master.detach().clone(), be.mom.clone()
        be.set_batch(x, y)
        be.step()
        g = be.store.master.grad.detach()
        scale = 1.0
        if clip:
            norm, scale = be.clip_state()
            assert scale < 1.0
        ref = lio.lion_reference(w0, g, m0, seg, wd_seg, lr, b1, b2, scale)
        lio.assert_decidable(ref, f"step {step}")
        lio.check(be.store.master.detach(), be.mom, ref, lr, f"step {step}")
        # every element with a non-zero c moved by lr: far more than the bounds
        moved = (ref[0] - w0.double()).abs()
        assert float((moved / ref[2]).median()) > 1e3
        assert be.metrics()["optimizer"] == "lion" and "adam_alpha" not in be.metrics()
    assert float(be.mom.abs().max()) > 0


# ---------------------------------------------------------------- flags
@pytest.mark.parametrize("kind", ["cifar", "imagenet"])
def test_lion_flags(kind):
    f = build_parser(kind).parse_args([])
    assert (f.optimizer, f.lion_beta1, f.lion_beta2, f.lion_decay_skip) == ("mom", 0.9, 0.99, "none")
    f = build_parser(kind).parse_args(["--optimizer", "lion", "--lion_beta1", "0", "--lion_beta2",
                                       "0.5", "--lion_decay_skip", "vectors", "--clip_grad_norm",
                                       "1.0"])
    assert (f.optimizer, f.lion_beta1, f.lion_beta2, f.lion_decay_skip) == ("lion", 0.0, 0.5, "vectors")
    # a non-default --adam_* flag with lion: accepted and unused, as lars_skip is
    f = build_parser(kind).parse_args(["--optimizer", "lion", "--adam_beta1", "0.5", "--adam_decay",
                                       "l2", "--adam_trust_skip", "none"])
    assert f.optimizer == "lion" and f.adam_beta1 == 0.5
    for bad in (["--lion_beta1", "1"], ["--lion_beta1", "-0.1"], ["--lion_beta2", "1.5"],
                ["--lion_beta2", "nan"], ["--lion_beta2", "0.999999999"],   # 1 in fp32
                ["--lion_decay_skip", "biases"], ["--optimizer", "lion", "--adam_trust", "on"]):
        with pytest.raises(SystemExit):
            build_parser(kind).parse_args(bad)


def test_optimizers_and_backend_errors():
    assert "lion" in OPTIMIZERS and OPTIMIZERS[:4] == ("mom", "sgd", "lars", "adamw")
    assert "lion" in OPT_FUSED_LION_REASON
    assert check_lion(0.9, 0.99) == (0.9, 0.99)
    for kw in (dict(lion_beta1=1.0), dict(lion_beta2=-0.5), dict(lion_beta1=float("nan")),
               dict(lion_decay_skip="all"), dict(adam_trust="on")):
        with pytest.raises(ValueError):
            CPUBackend(cifar_spec(8), 4, weight_decay=1e-4, lr_schedule=constant_lr(1e-3),
                       optimizer="lion", **kw)
    be = CPUBackend(cifar_spec(8), 4, weight_decay=1e-4, lr_schedule=constant_lr(1e-3),
                    optimizer="lion", adam_beta1=0.5, adam_decay="l2")
    assert be.lion and not be.adam and be.adam_v is None


# ---------------------------------------------------------------- checkpoints
def _backend(optimizer, seed=0, **kw):
    return CPUBackend(cifar_spec(8), 4, weight_decay=1e-3, lr_schedule=constant_lr(1e-3),
                      optimizer=optimizer, seed=seed, **kw)


def _steps(be, n, seed=3):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(4, 32, 32, 3, generator=gen)
    y = torch.randint(0, 10, (4,), generator=gen)
    for _ in range(n):
        be.set_batch(x, y)
        be.step()


def test_lion_round_trip_writes_lion_slots_and_resumes_bitwise(tmp_path):
    straight = _backend("lion")
    _steps(straight, 4)
    first = _backend("lion")
    _steps(first, 2)
    t = first.state_tensors()
    train = [s.name for s in first.store.train_slots]
    stats = [s.name for s in first.store.stat_slots]
    assert set(t) == set(train) | {n + "/Lion" for n in train} | set(stats) | {"global_step"}
    assert not any(k.endswith("/Momentum") for k in t)
    s = first.store.train_slots[0]
    assert np.array_equal(t[s.name + "/Lion"].reshape(-1),
                          first.mom[s.offset:s.offset + s.numel].numpy())
    prefix = Saver(str(tmp_path)).save(t, 2)
    second = _backend("lion", seed=9)
    second.load_state(Saver.restore(prefix))
    assert second.global_step == 2 and torch.equal(second.mom, first.mom)
    _steps(second, 2)
    assert torch.equal(second.store.master, straight.store.master)
    assert torch.equal(second.mom, straight.mom)


def test_lion_restores_a_mom_checkpoint_with_zero_m_and_back(tmp_path, capsys):
    mom = _backend("mom")
    _steps(mom, 3)
    assert float(mom.mom.abs().max()) > 0
    prefix = Saver(str(tmp_path)).save(mom.state_tensors(), 3)
    be = _backend("lion", seed=9)
    be.mom.fill_(1.0)
    capsys.readouterr()
    be.load_state(Saver.restore(prefix))
    out = capsys.readouterr().out
    assert out.count("no Lion slots") == 1 and len(out.strip().splitlines()) == 1
    assert be.global_step == 3 and int(be.mom.count_nonzero()) == 0
    assert torch.equal(be.store.master, mom.store.master)
    _steps(be, 1)
    t = be.state_tensors()
    assert int(t["global_step"]) == 4 and "conv2d/kernel/Lion" in t
    # and back: a mom (or adamw) run restoring a lion checkpoint starts its own state from zero
    prefix = Saver(str(tmp_path)).save(t, 4)
    back = _backend("mom", seed=5)
    back.load_state(Saver.restore(prefix))
    assert back.global_step == 4 and int(back.mom.count_nonzero()) == 0
    assert torch.equal(back.store.master, be.store.master)
    adam = _backend("adamw", seed=5)
    adam.load_state(Saver.restore(prefix))
    assert int(adam.mom.count_nonzero()) == 0 and int(adam.adam_v.count_nonzero()) == 0
    assert adam.adam_start == 4


def test_checkpoint_entries_of_a_mom_run_are_unchanged():
    be = _backend("mom", lion_beta1=0.5, lion_decay_skip="vectors")
    _steps(be, 1)
    t = be.state_tensors()
    train = [s.name for s in be.store.train_slots]
    stats = [s.name for s in be.store.stat_slots]
    assert set(t) == set(train) | {n + "/Momentum" for n in train} | set(stats) | {"global_step"}
    assert "optimizer" not in be.metrics()


# ---------------------------------------------------------------- the kernel's resources
@pytest.mark.skipif(not kr.have_compiler(), reason="no ROCm compiler")
def test_lion_kernel_has_no_spills_and_no_scratch():
    rows = kr._resources(os.path.join(kr.CSRC, "lion.hip"))
    kernels = {n: r for n, r in rows.items() if "lion_pack_kernel" in n}
    assert len(kernels) == 2, sorted(rows)   # CLIP and plain
    for name, r in kernels.items():
        print(f"{name}: VGPRs {r['VGPRs']} SGPRs {r['TotalSGPRs']} "
              f"waves/SIMD {r['Occupancy [waves/SIMD]']}")
        assert int(r["VGPRs Spill"]) == 0, (name, r)
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
