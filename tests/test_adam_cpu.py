"""--optimizer adamw without a GPU: the oracle (tests/adam_oracle.py) against closed forms,
the CPU backend's update against the oracle, the flags, the checkpoint entries and the two
restore rules, and the per-segment decay table."""
import math

import numpy as np
import pytest
import torch

import adam_oracle as ao
import optim_oracle as oo
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.train.backends import CPUBackend
from distributed_tensorflow_resnet_amd.train.layout import (SEG_DTYPE, adam_alpha,
                                                              adam_decay_table, check_adam)
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr
from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver
from distributed_tensorflow_resnet_amd.utils.flags import build_parser


def _one_seg(n):
    seg = np.zeros(1, dtype=SEG_DTYPE)
    seg["numel"] = n
    return seg


# ---------------------------------------------------------------- oracle against closed forms
def test_oracle_first_step_closed_form():
    gen = torch.Generator().manual_seed(1)
    g = torch.randn(257, generator=gen).double() * 3
    w = torch.randn(257, generator=gen).double()
    z = torch.zeros(257, dtype=torch.float64)
    lr, b1, b2, eps = oo.f32(1e-3), oo.f32(0.9), oo.f32(0.999), oo.f32(1e-3)
    for mode in ("decoupled", "l2"):
        w1, m1, v1, *_ = ao.adam_reference(w, g, z, z, _one_seg(257), [0.0], lr, 1, b1, b2, eps,
                                           1.0, mode)
        # the oracle takes 1 - b as the fp32 value the kernel gets; the closed form is in
        # terms of that value
        omb1, omb2 = oo.f32(1.0 - b1), oo.f32(1.0 - b2)
        want = lr * math.sqrt(1 - b2) / (1 - b1) * omb1 * g / (math.sqrt(omb2) * g.abs() + eps)
        assert float(((w - w1) - want).abs().max()) < 1e-15
        # with the exact 1 - b: lr g / (|g| + eps / sqrt(1 - b2)), to the 1e-8 relative that
        # the fp32 rounding of 1 - b leaves
        closed = ao.adam_closed_form_first_step(g, lr, b1, b2, eps)
        assert float(((w - w1) - closed).abs().max()) < 1e-7 * lr
        assert float((w - w1).abs().max()) > 0.9 * lr   # |g| >> eps / sqrt(1 - b2) somewhere


def test_oracle_constant_gradient_keeps_m_hat():
    """A constant gradient: m_t = (1 - b1^t) g exactly, so m_hat = m_t / (1 - b1^t) = g and
    v_hat = g^2 for 50 steps; the step is alpha_t m_t / (sqrt(v_t) + eps)."""
    g = torch.tensor([0.5, -2.0, 3.25], dtype=torch.float64)
    w = torch.tensor([1.0, 2.0, -3.0], dtype=torch.float64)
    m = v = torch.zeros(3, dtype=torch.float64)
    b1, b2 = 0.5, 0.75        # exact in fp32, and so are 1 - b1 and 1 - b2
    for t in range(1, 51):
        w1, m, v, _, _, _, alpha = ao.adam_reference(w, g, m, v, _one_seg(3), [0.0], 0.125, t, b1,
                                                     b2, 1e-8, 1.0, "decoupled")
        c1, c2 = 1 - b1 ** t, 1 - b2 ** t
        assert float((m / c1 - g).abs().max()) < 1e-14
        assert float((v / c2 - g * g).abs().max()) < 1e-13
        assert alpha == pytest.approx(0.125 * math.sqrt(c2) / c1, rel=1e-15)
        assert float(((w - w1) - alpha * m / (v.sqrt() + oo.f32(1e-8))).abs().max()) < 1e-15
        w = w1


def test_alpha_reference_and_host_mirror():
    for b1, b2 in ((0.9, 0.999), (0.5, 0.75), (0.0, 0.99), (0.95, 0.0)):
        for t in (1, 2, 10, 1000, 2 ** 31 + 5):
            for lr in (1e-3, 0.1):
                ref = ao.alpha_reference(lr, t, b1, b2)
                got = adam_alpha(lr, t, b1, b2)
                assert abs(got - ref) <= ao.ulp(ref), (b1, b2, t, lr, got, ref)
    # t = 1: lr sqrt(1 - b2) / (1 - b1); t large: lr
    assert ao.alpha_reference(0.25, 2 ** 31 + 5, 0.9, 0.999) == 0.25
    assert ao.alpha_reference(0.25, 1, 0.5, 0.75) == 0.25


# ---------------------------------------------------------------- CPU backend against the oracle
def _seg_of(store):
    seg = np.zeros(len(store.train_slots), dtype=SEG_DTYPE)
    for r, s in zip(seg, store.train_slots):
        r["offset"], r["numel"] = s.offset, s.numel
    return seg


@pytest.mark.parametrize("mode,skip,clip", [("decoupled", "none", 0.0), ("l2", "vectors", 0.0),
                                            ("decoupled", "vectors", 0.05)])
def test_cpu_backend_adamw_step_matches_oracle(mode, skip, clip):
    """Two steps (the second from non-zero moments) of the backend's own fp32 gradient
    through the oracle: the CPU backend is the kernel's expressions in fp32 torch, so the
    kernel's bounds hold for it."""
    spec = cifar_spec(8)
    wd, lr, b1, b2, eps = 0.05, 1e-3, 0.9, 0.99, 1e-6
    be = CPUBackend(spec, 4, weight_decay=wd, lr_schedule=constant_lr(lr), optimizer="adamw",
                    adam_beta1=b1, adam_beta2=b2, adam_epsilon=eps, adam_decay=mode,
                    adam_decay_skip=skip, clip_grad_norm=clip)
    assert be.adam_state() is None
    seg = _seg_of(be.store)
    wd_seg = [0.0 if skip == "vectors" and len(s.shape) == 1 else wd for s in be.store.train_slots]
    assert 0.0 in wd_seg or skip == "none"
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, 32, 32, 3, generator=gen)
    y = torch.randint(0, 10, (4,), generator=gen)
    for step in range(2):
        w0 = be.store.master.detach().clone()
        m0, v0 = be.mom.clone(), be.adam_v.clone()
        be.set_batch(x, y)
        be.step()
        g = be.store.master.grad.detach()
        scale = 1.0
        if clip:
            norm, scale = be.clip_state()
            assert scale < 1.0 and norm == pytest.approx(float(g.double().norm()), rel=1e-6)
        w1, m1, v1, Bw, Bm, Bv, alpha = ao.adam_reference(w0, g, m0, v0, seg, wd_seg, lr, step + 1,
                                                          b1, b2, eps, scale, mode)
        t, a = be.adam_state()
        assert t == step + 1 and abs(a - alpha) <= ao.ulp(alpha)
        assert be.metrics()["adam_alpha"] == a
        for got, ref, B, name in ((be.store.master.detach(), w1, Bw, "w"), (be.mom, m1, Bm, "m"),
                                  (be.adam_v, v1, Bv, "v")):
            err = (got.double() - ref).abs()
            assert bool((err <= B).all()), (name, step, float((err / B.clamp_min(1e-300)).max()))
        # the update moved the weights by far more than the bounds
        assert float(((w1 - w0.double()).abs() / Bw).median()) > 1e3
    with pytest.raises(ValueError):
        CPUBackend(spec, 4, weight_decay=wd, lr_schedule=constant_lr(lr), optimizer="adam")


# ---------------------------------------------------------------- flags
@pytest.mark.parametrize("kind", ["cifar", "imagenet"])
def test_adam_flags(kind):
    f = build_parser(kind).parse_args([])
    assert (f.optimizer, f.adam_beta1, f.adam_beta2, f.adam_epsilon, f.adam_decay,
            f.adam_decay_skip) == ("mom", 0.9, 0.999, 1e-8, "decoupled", "none")
    f = build_parser(kind).parse_args(["--optimizer", "adamw", "--adam_beta1", "0.8",
                                       "--adam_beta2", "0", "--adam_epsilon", "1e-6",
                                       "--adam_decay", "l2", "--adam_decay_skip", "vectors",
                                       "--lars_eeta", "0.02", "--clip_grad_norm", "1.0"])
    assert (f.optimizer, f.adam_beta1, f.adam_beta2, f.adam_epsilon, f.adam_decay,
            f.adam_decay_skip) == ("adamw", 0.8, 0.0, 1e-6, "l2", "vectors")
    for bad in (["--adam_beta1", "1"], ["--adam_beta1", "-0.1"], ["--adam_beta2", "1.5"],
                ["--adam_beta2", "nan"], ["--adam_epsilon", "0"], ["--adam_epsilon", "-1e-8"],
                ["--adam_epsilon", "inf"], ["--adam_epsilon", "1e-60"],   # 0 in fp32
                ["--adam_beta2", "0.999999999"],                           # 1 in fp32
                ["--adam_decay", "adamw"], ["--adam_decay_skip", "biases"],
                ["--optimizer", "adam"]):
        with pytest.raises(SystemExit):
            build_parser(kind).parse_args(bad)


def test_check_adam_and_backend_errors():
    assert check_adam(0.9, 0.999, 1e-8) == (0.9, 0.999, 1e-8)
    for kw in (dict(adam_beta1=1.0), dict(adam_beta2=-0.5), dict(adam_epsilon=0.0),
               dict(adam_epsilon=float("nan")), dict(adam_decay="coupled"),
               dict(adam_decay_skip="all")):
        with pytest.raises(ValueError):
            CPUBackend(cifar_spec(8), 4, weight_decay=1e-4, lr_schedule=constant_lr(1e-3),
                       optimizer="adamw", **kw)


# ---------------------------------------------------------------- layout
def test_adam_decay_table():
    shapes = [(3, 3, 3, 16), (16,), (16,), (64, 10), (10,)]
    t = adam_decay_table(shapes, 5e-4, "none")
    assert t.dtype == np.float32 and t.tolist() == [float(np.float32(5e-4))] * 5
    t = adam_decay_table(shapes, 5e-4, "vectors")
    w = float(np.float32(5e-4))
    assert t.tolist() == [w, 0.0, 0.0, w, 0.0]
    with pytest.raises(ValueError):
        adam_decay_table(shapes, 5e-4, "biases")


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


def test_checkpoint_entries_of_an_adamw_run():
    be = _backend("adamw", adam_beta1=0.5, adam_beta2=0.75)
    _steps(be, 3)
    t = be.state_tensors()
    train = [s.name for s in be.store.train_slots]
    stats = [s.name for s in be.store.stat_slots]
    want = set(train) | {n + "/Adam" for n in train} | {n + "/Adam_1" for n in train} | set(stats) \
        | {"global_step", "beta1_power", "beta2_power", "adam_start_step"}
    assert set(t) == want and len(t) == 3 * len(train) + len(stats) + 4
    assert not any(k.endswith("/Momentum") for k in t)
    # TF 1.12: the power variables start at beta and are multiplied once per step
    assert t["beta1_power"].dtype == np.float32 and t["beta1_power"].shape == ()
    assert float(t["beta1_power"]) == 0.5 ** 4 and float(t["beta2_power"]) == 0.75 ** 4
    assert t["adam_start_step"].dtype == np.int64 and int(t["adam_start_step"]) == 0
    assert int(t["global_step"]) == 3
    s = be.store.train_slots[0]
    assert np.array_equal(t[s.name + "/Adam"].reshape(-1), be.mom[s.offset:s.offset + s.numel].numpy())
    assert np.array_equal(t[s.name + "/Adam_1"].reshape(-1),
                          be.adam_v[s.offset:s.offset + s.numel].numpy())
    assert float(np.abs(t[s.name + "/Adam_1"]).max()) > 0


def test_checkpoint_entries_of_a_mom_run_are_unchanged():
    be = _backend("mom")
    _steps(be, 1)
    t = be.state_tensors()
    train = [s.name for s in be.store.train_slots]
    stats = [s.name for s in be.store.stat_slots]
    assert set(t) == set(train) | {n + "/Momentum" for n in train} | set(stats) | {"global_step"}
    # CIFAR ResNet-50: the reference's 403 entries
    from distributed_tensorflow_resnet_amd.models.params import ParamStore
    from distributed_tensorflow_resnet_amd.utils.checkpoint import state_to_tf

    ps = ParamStore(cifar_spec(50))
    ps.initialize(0)
    assert len(state_to_tf(ps, torch.zeros(ps.n_train), 0)) == 403


def test_adamw_round_trip_resumes_bitwise(tmp_path):
    straight = _backend("adamw")
    _steps(straight, 4)
    first = _backend("adamw")
    _steps(first, 2)
    prefix = Saver(str(tmp_path)).save(first.state_tensors(), 2)
    second = _backend("adamw", seed=9)
    second.load_state(Saver.restore(prefix))
    assert second.global_step == 2 and second.adam_start == 0
    assert torch.equal(second.mom, first.mom) and torch.equal(second.adam_v, first.adam_v)
    _steps(second, 2)
    assert second.adam_state() == straight.adam_state() and second.adam_state()[0] == 4
    assert torch.equal(second.store.master, straight.store.master)
    assert torch.equal(second.mom, straight.mom) and torch.equal(second.adam_v, straight.adam_v)
    # a TF-written file has the slots but no adam_start_step: the count starts at 0
    tensors = {k: v for k, v in Saver.restore(prefix).items() if k != "adam_start_step"}
    third = _backend("adamw", seed=9)
    third.adam_start = 7
    third.load_state(tensors)
    assert third.adam_start == 0 and torch.equal(third.adam_v, first.adam_v)


def test_adamw_restores_a_mom_checkpoint_with_fresh_moments(tmp_path, capsys):
    mom = _backend("mom")
    _steps(mom, 3)
    assert float(mom.mom.abs().max()) > 0
    prefix = Saver(str(tmp_path)).save(mom.state_tensors(), 3)
    be = _backend("adamw", seed=9)
    be.mom.fill_(1.0)
    be.adam_v.fill_(1.0)
    be.load_state(Saver.restore(prefix))
    assert "no Adam slots" in capsys.readouterr().out
    assert be.global_step == 3 and be.adam_start == 3
    assert int(be.mom.count_nonzero()) == 0 and int(be.adam_v.count_nonzero()) == 0
    assert torch.equal(be.store.master, mom.store.master)
    _steps(be, 1)
    assert be.adam_state()[0] == 1      # the bias correction restarted with the moments
    t = be.state_tensors()
    assert int(t["adam_start_step"]) == 3 and int(t["global_step"]) == 4
    assert float(t["beta1_power"]) == float(np.float32(float(np.float32(0.9)) ** 2))
    # and back: a mom run restoring an adamw checkpoint keeps its momentum as it was (zero),
    # as for any file without /Momentum
    prefix = Saver(str(tmp_path)).save(t, 4)
    back = _backend("mom", seed=5)
    back.load_state(Saver.restore(prefix))
    assert back.global_step == 4 and int(back.mom.count_nonzero()) == 0
    assert torch.equal(back.store.master, be.store.master)
