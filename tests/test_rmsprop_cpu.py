"""--optimizer rmsprop without a GPU: the oracle (tests/rmsprop_oracle.py) on its own, the CPU
backend's update against the oracle, the flags, the checkpoint entries and the restore rules,
the driver on the CPU, and the compiler's resource remarks of csrc/rmsprop.hip."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kernel_resources as kr
import rmsprop_oracle as rmo
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.train.backends import CPUBackend
from distributed_tensorflow_resnet_amd.train.layout import (OPT_FUSED_RMSPROP_REASON, OPTIMIZERS,
                                                              SEG_DTYPE, check_rmsprop)
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr
from distributed_tensorflow_resnet_amd.utils import tensor_bundle as tb
from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver
from distributed_tensorflow_resnet_amd.utils.flags import build_parser


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one_seg(n):
    seg = np.zeros(1, dtype=SEG_DTYPE)
    seg["numel"] = n
    return seg


# ---------------------------------------------------------------- the oracle on its own
def test_oracle_exact_values():
    """rho = 0.5, momentum = 0.5, lr = 0.125 and the data are exact in fp32 and the roots are
    whole numbers: the step by hand (eps = 2^-20 is far below the figures compared)."""
    w = torch.tensor([1.0, 2.0, -3.0, 0.5])
    g = torch.tensor([4.0, -2.0, 0.0, float("nan")])
    ms = torch.tensor([2.0, 4.0, 8.0, 1.0])
    mom = torch.tensor([0.5, 0.0, 1.0, 0.0])
    eps = 2.0 ** -20
    ref = rmo.rmsprop_reference(w, g, ms, None, mom, _one_seg(4), [0.0], 0.125, 0.5, 0.5, eps,
                                1.0, False, "l2")
    # ms' = (9, 4, 4, nan); q = lr g / sqrt(ms' + eps) = (1/6, -1/8, 0)
    assert ref["ms"][:3].tolist() == [9.0, 4.0, 4.0] and ref["mg"] is None
    want_mom = torch.tensor([0.25 + 0.5 / 3.0, -0.125, 0.5], dtype=torch.float64)
    assert torch.allclose(ref["mom"][:3], want_mom, rtol=1e-6, atol=0)
    assert torch.allclose(ref["w"][:3], w[:3].double() - want_mom, rtol=1e-6, atol=0)
    assert all(bool(torch.isnan(ref[k][3])) for k in ("ms", "mom", "w"))
    # centered: mg' = 0.5 mg + 0.5 g; the denominator is ms' - mg'^2
    mg = torch.tensor([0.0, 2.0, 0.0, 0.0])
    cen = rmo.rmsprop_reference(w, g, ms, mg, mom, _one_seg(4), [0.0], 0.125, 0.5, 0.5, eps, 1.0,
                                True, "l2")
    assert cen["mg"][:3].tolist() == [2.0, 0.0, 0.0]
    assert torch.allclose(cen["d"][:3], torch.tensor([5.0, 4.0, 4.0], dtype=torch.float64),
                          rtol=1e-6, atol=0)
    assert rmo.assert_conditioned(
        rmo.rmsprop_reference(w[1:3], g[1:3], ms[1:3], mg[1:3], mom[1:3], _one_seg(2), [0.0],
                              0.125, 0.5, 0.5, eps, 1.0, True, "l2")) >= 4.0
    with pytest.raises(AssertionError):   # element 0: ms' = 9 < 4 * 4
        rmo.assert_conditioned(cen)
    # l2 puts the decay into g'; decoupled takes (lr wd) w off the old w
    l2 = rmo.rmsprop_reference(w, g, ms, None, mom, _one_seg(4), [0.5], 0.125, 0.5, 0.5, eps, 1.0,
                               False, "l2")
    assert l2["ms"][:3].tolist() == [1.0 + 0.5 * 4.5 ** 2, 2.0 + 0.5, 4.0 + 0.5 * 1.5 ** 2]
    de = rmo.rmsprop_reference(w, g, ms, None, mom, _one_seg(4), [0.5], 0.125, 0.5, 0.5, eps, 1.0,
                               False, "decoupled")
    assert torch.equal(de["ms"][:3], ref["ms"][:3])
    assert torch.allclose(de["w"][:3], ref["w"][:3] - 0.0625 * w[:3].double(), rtol=1e-12, atol=0)


def _numpy_step(w, g, ms, mg, mom, wd, lr, rho, mo, eps, scale, centered, mode):
    """An fp32 numpy evaluation, each operation rounded once, as the kernel's is written."""
    f = np.float32
    w, g, ms, mom = (x.numpy() for x in (w, g, ms, mom))
    omr = f(1.0 - float(f(rho)))
    gp = f(scale) * g
    if mode == "l2":
        gp = gp + f(wd) * w
    ms1 = f(rho) * ms + omr * (gp * gp)
    d, mg1 = ms1, None
    if centered:
        mg1 = f(rho) * mg.numpy() + omr * gp
        d = ms1 - mg1 * mg1
    d = d + f(eps)
    mom1 = f(mo) * mom + (f(lr) * gp) / np.sqrt(d)
    w1 = w - mom1
    if mode == "decoupled":
        w1 = w1 - (f(lr) * f(wd)) * w
    assert all(x.dtype == f for x in (w1, ms1, mom1))
    t = torch.from_numpy
    return t(w1), t(ms1), (t(mg1) if centered else None), t(mom1)


@pytest.mark.parametrize("seed", [41, 42, 43, 44, 45])
@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("rho,mo,eps,wd,scale,mode", [(0.9, 0.9, 1e-10, 0.05, 1.0, "l2"),
                                                      (0.5, 0.0, 1e-3, 0.3, 0.37, "decoupled")])
def test_oracle_on_the_test_data(seed, centered, rho, mo, eps, wd, scale, mode):
    """The seeds the GPU tests use: the centered denominator is well conditioned for every
    element, an fp32 evaluation passes check(), and wrong ones do not."""
    n = 100003
    w, g, ms, mg, mom = rmo.rmsprop_inputs(n, seed)
    args = (_one_seg(n), [wd], 1e-2, rho, mo, eps, scale, centered, mode)
    ref = rmo.rmsprop_reference(w, g, ms, mg, mom, *args)
    if centered:
        assert rmo.assert_conditioned(ref) >= 4.0
    good = _numpy_step(w, g, ms, mg, mom, wd, 1e-2, rho, mo, eps, scale, centered, mode)
    worst = rmo.check(*good, ref)
    assert max(worst.values()) <= 1.0 and set(worst) == {"w", "ms", "mom"} | ({"mg"} if centered
                                                                              else set())
    other = "decoupled" if mode == "l2" else "l2"
    wrong = [_numpy_step(w, g, ms, mg, mom, wd, 1e-2, rho, mo, eps, scale, centered, other),
             _numpy_step(w, g, ms, mg, mom, wd, 1e-2, rho, mo, eps, scale, not centered, mode)
             if not centered else None,
             _numpy_step(w, g, ms, mg, mom, wd, 1e-2, rho, mo, eps + 1e-2, scale, centered, mode),
             _numpy_step(w, g, ms, mg, mom, wd, 1e-2, rho, mo + 0.05, eps, scale, centered, mode)]
    for bad in wrong:
        if bad is not None:
            with pytest.raises(AssertionError):
                rmo.check(bad[0], bad[1], good[2], bad[3], ref)
    # epsilon outside the root (adamw's place) is another optimizer
    if eps >= 1e-3:
        f = np.float32
        q = (f(1e-2) * (f(scale) * g.numpy())) / (np.sqrt(ref["d"].numpy().astype(f) - f(eps)) + f(eps))
        mom_out = torch.from_numpy(f(mo) * mom.numpy() + q.astype(f))
        with pytest.raises(AssertionError):
            rmo.check(good[0], good[1], good[2], mom_out, ref)


# ---------------------------------------------------------------- CPU backend against the oracle
def _seg_of(store):
    seg = np.zeros(len(store.train_slots), dtype=SEG_DTYPE)
    for r, s in zip(seg, store.train_slots):
        r["offset"], r["numel"] = s.offset, s.numel
    return seg


@pytest.mark.parametrize("centered,mode,skip,clip,mo", [
    (False, "l2", "none", 0.0, 0.9), (True, "l2", "vectors", 0.0, 0.0),
    (False, "decoupled", "vectors", 0.05, 0.9), (True, "decoupled", "none", 0.05, 0.9)])
def test_cpu_backend_rmsprop_step_matches_oracle(centered, mode, skip, clip, mo):
    """Two steps (the second from a non-trivial state) of the backend's own fp32 gradient
    through the oracle: the CPU backend is the kernel's expressions in fp32 torch, so the
    kernel's bounds hold for it."""
    spec = cifar_spec(8)
    wd, lr, rho, eps = 0.05, 1e-3, 0.9, 1e-10
    be = CPUBackend(spec, 4, weight_decay=wd, lr_schedule=constant_lr(lr), optimizer="rmsprop",
                    rmsprop_rho=rho, rmsprop_momentum=mo, rmsprop_epsilon=eps,
                    rmsprop_centered=centered, rmsprop_wd=mode, rmsprop_decay_skip=skip,
                    clip_grad_norm=clip)
    assert be.rmsprop and be.adam_state() is None and be.lamb_state() is None
    st = be.rmsprop_state()
    assert {k: st[k] for k in ("rho", "momentum", "epsilon", "centered")} == \
        {"rho": rho, "momentum": mo, "epsilon": eps, "centered": centered}
    assert ("mg" in st) == centered and torch.equal(st["ms"], torch.ones(be.store.n_train))
    assert int(be.mom.count_nonzero()) == 0 and (not centered or int(st["mg"].count_nonzero()) == 0)
    seg = _seg_of(be.store)
    wd_seg = [0.0 if skip == "vectors" and len(s.shape) == 1 else wd for s in be.store.train_slots]
    assert 0.0 in wd_seg or skip == "none"
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, 32, 32, 3, generator=gen)
    y = torch.randint(0, 10, (4,), generator=gen)
    for step in range(2):
        w0, ms0, mom0 = be.store.master.detach().clone(), be.rms_ms.clone(), be.mom.clone()
        mg0 = be.rms_mg.clone() if centered else None
        be.set_batch(x, y)
        be.step()
        g = be.store.master.grad.detach()
        scale = 1.0
        if clip:
            norm, scale = be.clip_state()
            assert scale < 1.0
        ref = rmo.rmsprop_reference(w0, g, ms0, mg0, mom0, seg, wd_seg, lr, rho, mo, eps, scale,
                                    centered, mode)
        if centered:
            rmo.assert_conditioned(ref, f"step {step}")
        rmo.check(be.store.master.detach(), be.rms_ms, be.rms_mg, be.mom, ref, f"step {step}")
        # the update is far above the bounds
        moved = (ref["w"] - w0.double()).abs()
        assert float((moved / ref["Bw"]).median()) > 100
        assert be.metrics()["optimizer"] == "rmsprop" and "adam_alpha" not in be.metrics()
    assert float(be.mom.abs().max()) > 0 and not torch.equal(be.rms_ms, torch.ones_like(be.rms_ms))


# ---------------------------------------------------------------- flags
@pytest.mark.parametrize("kind", ["cifar", "imagenet"])
def test_rmsprop_flags(kind):
    f = build_parser(kind).parse_args([])
    assert (f.optimizer, f.rmsprop_rho, f.rmsprop_momentum, f.rmsprop_epsilon, f.rmsprop_centered,
            f.rmsprop_wd, f.rmsprop_decay_skip) == ("mom", 0.9, 0.9, 1e-10, False, "l2", "none")
    f = build_parser(kind).parse_args(["--optimizer", "rmsprop", "--rmsprop_rho", "0.5",
                                       "--rmsprop_momentum", "0", "--rmsprop_epsilon", "1.0",
                                       "--rmsprop_centered", "--rmsprop_wd", "decoupled",
                                       "--rmsprop_decay_skip", "vectors", "--clip_grad_norm", "1.0"])
    assert (f.optimizer, f.rmsprop_rho, f.rmsprop_momentum, f.rmsprop_epsilon, f.rmsprop_centered,
            f.rmsprop_wd, f.rmsprop_decay_skip) == ("rmsprop", 0.5, 0.0, 1.0, True, "decoupled",
                                                    "vectors")
    assert build_parser(kind).parse_args(["--rmsprop_centered=true"]).rmsprop_centered is True
    assert build_parser(kind).parse_args(["--rmsprop_centered",
                                          "--normsprop_centered"]).rmsprop_centered is False
    # the --adam_* and --lion_* flags with rmsprop, and --rmsprop_* with another optimizer:
    # accepted and unused
    f = build_parser(kind).parse_args(["--optimizer", "rmsprop", "--adam_beta1", "0.5",
                                       "--adam_trust_skip", "none", "--lion_beta2", "0.5"])
    assert f.optimizer == "rmsprop" and f.adam_beta1 == 0.5
    f = build_parser(kind).parse_args(["--optimizer", "lion", "--rmsprop_rho", "0.5",
                                       "--rmsprop_centered", "--rmsprop_wd", "decoupled"])
    assert f.optimizer == "lion" and f.rmsprop_rho == 0.5 and f.rmsprop_centered
    for bad in (["--rmsprop_rho", "1"], ["--rmsprop_rho", "-0.1"], ["--rmsprop_rho", "nan"],
                ["--rmsprop_momentum", "1"], ["--rmsprop_momentum", "1.5"],
                ["--rmsprop_momentum", "-1e-3"], ["--rmsprop_rho", "0.999999999"],   # 1 in fp32
                ["--rmsprop_epsilon", "0"], ["--rmsprop_epsilon", "-1e-10"],
                ["--rmsprop_epsilon", "nan"], ["--rmsprop_epsilon", "1e-60"],        # 0 in fp32
                ["--rmsprop_epsilon", "inf"], ["--rmsprop_wd", "none"],
                ["--rmsprop_decay_skip", "biases"],
                ["--optimizer", "rmsprop", "--adam_trust", "on"]):
        with pytest.raises(SystemExit):
            build_parser(kind).parse_args(bad)


def test_optimizers_and_backend_errors():
    assert OPTIMIZERS[-1] == "rmsprop" and OPTIMIZERS[:5] == ("mom", "sgd", "lars", "adamw", "lion")
    assert "rmsprop" in OPT_FUSED_RMSPROP_REASON
    assert check_rmsprop(0.9, 0.0, 1e-10) == (0.9, 0.0, 1e-10, False)
    for kw in (dict(rmsprop_rho=1.0), dict(rmsprop_momentum=-0.5), dict(rmsprop_rho=float("nan")),
               dict(rmsprop_epsilon=0.0), dict(rmsprop_epsilon=-1.0), dict(rmsprop_wd="off"),
               dict(rmsprop_decay_skip="all"), dict(adam_trust="on")):
        with pytest.raises(ValueError):
            CPUBackend(cifar_spec(8), 4, weight_decay=1e-4, lr_schedule=constant_lr(1e-3),
                       optimizer="rmsprop", **kw)
    be = CPUBackend(cifar_spec(8), 4, weight_decay=1e-4, lr_schedule=constant_lr(1e-3),
                    optimizer="rmsprop", adam_beta1=0.5, adam_decay="l2", lion_beta1=0.5)
    assert be.rmsprop and not be.adam and not be.lion and be.adam_v is None and be.rms_mg is None
    # with another optimizer the flags are unused: no state, no rmsprop_state
    be = CPUBackend(cifar_spec(8), 4, weight_decay=1e-4, lr_schedule=constant_lr(1e-3),
                    optimizer="mom", rmsprop_rho=0.5, rmsprop_centered=True)
    assert not be.rmsprop and be.rms_ms is None and be.rms_mg is None
    assert be.rmsprop_state() is None


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


@pytest.mark.parametrize("centered", [False, True])
def test_rmsprop_round_trip_writes_tf_slots_and_resumes_bitwise(tmp_path, centered):
    """Entry names and counts, the tensor-bundle round trip and a bitwise resume.  The slots
    are named in the order TF 1.12 creates them: rms, mg (centered only), momentum."""
    kw = dict(rmsprop_centered=centered)
    straight = _backend("rmsprop", **kw)
    _steps(straight, 4)
    first = _backend("rmsprop", **kw)
    _steps(first, 2)
    t = first.state_tensors()
    train = [s.name for s in first.store.train_slots]
    stats = [s.name for s in first.store.stat_slots]
    slots = ("/RMSProp", "/RMSProp_1", "/RMSProp_2")[:3 if centered else 2]
    assert set(t) == (set(train) | {n + x for n in train for x in slots} | set(stats)
                      | {"global_step"})
    assert len(t) == len(train) * (1 + len(slots)) + len(stats) + 1
    assert not any(k.endswith(("/Momentum", "/Adam", "/Lion")) for k in t)
    s = first.store.train_slots[0]
    sl = slice(s.offset, s.offset + s.numel)
    assert np.array_equal(t[s.name + "/RMSProp"].reshape(-1), first.rms_ms[sl].numpy())
    assert np.array_equal(t[s.name + slots[-1]].reshape(-1), first.mom[sl].numpy())
    if centered:
        assert np.array_equal(t[s.name + "/RMSProp_1"].reshape(-1), first.rms_mg[sl].numpy())
    assert t[s.name + "/RMSProp"].shape == tuple(s.shape)
    prefix = Saver(str(tmp_path)).save(t, 2)
    back = Saver.restore(prefix)
    assert set(back) == set(t) and all(np.array_equal(back[k], t[k]) for k in t)
    assert set(tb.read_bundle(prefix)) == set(t)
    second = _backend("rmsprop", seed=9, **kw)
    second.load_state(back)
    assert second.global_step == 2 and torch.equal(second.mom, first.mom)
    assert torch.equal(second.rms_ms, first.rms_ms)
    _steps(second, 2)
    assert torch.equal(second.store.master, straight.store.master)
    assert torch.equal(second.mom, straight.mom) and torch.equal(second.rms_ms, straight.rms_ms)
    if centered:
        assert torch.equal(second.rms_mg, straight.rms_mg)


@pytest.mark.parametrize("centered", [False, True])
def test_rmsprop_restores_a_mom_checkpoint_from_ones_and_back(tmp_path, capsys, centered):
    mom = _backend("mom")
    _steps(mom, 3)
    assert float(mom.mom.abs().max()) > 0
    prefix = Saver(str(tmp_path)).save(mom.state_tensors(), 3)
    be = _backend("rmsprop", seed=9, rmsprop_centered=centered)
    _steps(be, 1)   # a state to be reset
    assert not torch.equal(be.rms_ms, torch.ones_like(be.rms_ms))
    capsys.readouterr()
    be.load_state(Saver.restore(prefix))
    out = capsys.readouterr().out
    assert out.count("no RMSProp slots") == 1 and len(out.strip().splitlines()) == 1
    assert be.global_step == 3 and int(be.mom.count_nonzero()) == 0
    assert torch.equal(be.rms_ms, torch.ones_like(be.rms_ms))
    assert not centered or int(be.rms_mg.count_nonzero()) == 0
    assert torch.equal(be.store.master, mom.store.master)
    _steps(be, 1)
    t = be.state_tensors()
    assert int(t["global_step"]) == 4 and "conv2d/kernel/RMSProp" in t
    # and back: a mom, adamw or lion run restoring it starts its own state from zero
    prefix = Saver(str(tmp_path)).save(t, 4)
    back = _backend("mom", seed=5)
    back.load_state(Saver.restore(prefix))
    assert back.global_step == 4 and int(back.mom.count_nonzero()) == 0
    assert torch.equal(back.store.master, be.store.master)
    adam = _backend("adamw", seed=5)
    adam.load_state(Saver.restore(prefix))
    assert int(adam.mom.count_nonzero()) == 0 and int(adam.adam_v.count_nonzero()) == 0
    assert adam.adam_start == 4
    lion = _backend("lion", seed=5)
    lion.load_state(Saver.restore(prefix))
    assert int(lion.mom.count_nonzero()) == 0


@pytest.mark.parametrize("centered", [False, True])
def test_plain_and_centered_checkpoints_do_not_mix(centered):
    """<name>/RMSProp_1 is the momentum of a plain run and mg of a centered one: refused, and
    nothing of the run's state has moved."""
    src = _backend("rmsprop", rmsprop_centered=centered)
    _steps(src, 2)
    t = src.state_tensors()
    be = _backend("rmsprop", seed=9, rmsprop_centered=not centered)
    _steps(be, 1)
    before = [x.clone() for x in (be.store.master.detach(), be.mom, be.rms_ms)]
    with pytest.raises(ValueError, match="centered.*plain|plain.*centered"):
        be.load_state(t)
    for x, y in zip(before, (be.store.master.detach(), be.mom, be.rms_ms)):
        assert torch.equal(x, y)
    assert be.global_step == 1


@pytest.mark.parametrize("slots", [True, False])
def test_a_restore_that_fails_on_the_weights_leaves_the_rmsprop_state(slots):
    """The slots are loaded (or reset to ones and zeros) after the weights, as the adam and
    lion slots are: a checkpoint that passes the form check and then fails on a variable
    (here: a weight of the wrong shape) has moved none of ms, mg, mom."""
    src = _backend("rmsprop" if slots else "mom", **(dict(rmsprop_centered=True) if slots else {}))
    _steps(src, 2)
    t = dict(src.state_tensors())
    name = src.store.train_slots[-1].name
    t[name] = np.zeros(t[name].size + 1, dtype=np.float32)
    be = _backend("rmsprop", seed=9, rmsprop_centered=True)
    _steps(be, 1)
    before = [x.clone() for x in (be.mom, be.rms_ms, be.rms_mg)]
    with pytest.raises((ValueError, RuntimeError)):
        be.load_state(t)
    for x, y in zip(before, (be.mom, be.rms_ms, be.rms_mg)):
        assert torch.equal(x, y)
    # a slot of the wrong size is refused by the form check, before the weights move
    if slots:
        t = dict(src.state_tensors())
        t[name + "/RMSProp_1"] = np.zeros(3, dtype=np.float32)
        w = be.store.master.detach().clone()
        with pytest.raises(ValueError, match="RMSProp_1"):
            be.load_state(t)
        assert torch.equal(w, be.store.master.detach()) and torch.equal(before[1], be.rms_ms)


def test_the_root_through_fp64_is_the_correctly_rounded_fp32_root():
    """The CPU backend and the momentum-0 GPU test take sqrt(d) as the fp64 root rounded to
    fp32 once more; numpy's fp32 sqrt (the hardware's, correctly rounded) gives the same bits."""
    gen = torch.Generator().manual_seed(7)
    d = torch.cat([torch.rand(100003, generator=gen) * 4 + 1e-10,
                   10.0 ** (torch.rand(100003, generator=gen) * 40 - 30)])
    assert np.array_equal(d.double().sqrt().float().numpy(), np.sqrt(d.numpy()))


def test_checkpoint_entries_of_a_mom_run_are_unchanged():
    be = _backend("mom", rmsprop_rho=0.5, rmsprop_centered=True, rmsprop_decay_skip="vectors")
    _steps(be, 1)
    t = be.state_tensors()
    train = [s.name for s in be.store.train_slots]
    stats = [s.name for s in be.store.stat_slots]
    assert set(t) == set(train) | {n + "/Momentum" for n in train} | set(stats) | {"global_step"}
    assert "optimizer" not in be.metrics()


# ---------------------------------------------------------------- the driver
def test_cli_runs_two_rmsprop_steps_on_the_cpu(tmp_path):
    e = dict(os.environ)
    e.update({"CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": "", "OMP_NUM_THREADS": "2"})
    td, ld = str(tmp_path / "train"), str(tmp_path / "log")
    r = subprocess.run([sys.executable, "resnet_cifar_main.py", "--device", "cpu", "--synthetic",
                        "--resnet_size", "8", "--batch_size", "4", "--log_every", "1",
                        "--summary_every", "1", "--optimizer", "rmsprop", "--lr_decay", "cosine",
                        "--lr_peak", "1e-3", "--train_steps", "2", "--train_dir", td,
                        "--log_dir", ld],
                       cwd=ROOT, capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "optimizer: rmsprop" in r.stdout + r.stderr
    rows = [json.loads(line) for line in open(os.path.join(ld, "metrics.jsonl"))]
    assert len(rows) == 2
    for row in rows:
        assert row["optimizer"] == "rmsprop" and np.isfinite(row["cross_entropy"])
        assert "adam_alpha" not in row
    t = tb.read_bundle(tb.latest_checkpoint(td))
    assert int(t["global_step"]) == 2 and "conv2d/kernel/RMSProp_1" in t
    assert "conv2d/kernel/RMSProp_2" not in t and "conv2d/kernel/Momentum" not in t


# ---------------------------------------------------------------- the kernel's resources
@pytest.mark.skipif(not kr.have_compiler(), reason="no ROCm compiler")
def test_rmsprop_kernel_has_no_spills_and_no_scratch():
    rows = kr._resources(os.path.join(kr.CSRC, "rmsprop.hip"))
    kernels = {n: r for n, r in rows.items() if "rmsprop_pack_kernel" in n}
    assert len(kernels) == 4, sorted(rows)   # CENTERED x CLIP
    for name, r in kernels.items():
        print(f"{name}: VGPRs {r['VGPRs']} SGPRs {r['TotalSGPRs']} "
              f"waves/SIMD {r['Occupancy [waves/SIMD]']}")
        assert int(r["VGPRs Spill"]) == 0, (name, r)
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
