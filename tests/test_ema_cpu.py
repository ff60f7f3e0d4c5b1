"""--ema_decay without a GPU: the fp64 recurrence of tests/ema_oracle.py against its closed
form, the warm-up switch, the CPU backend's shadows step by step, the checkpoint names and
round trip, ema_weights, the flags, the evaluator scoring shadows or weights, and two gloo
ranks keeping identical shadows."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import ema_oracle as eo
from distributed_tensorflow_resnet_amd.models.params import ParamStore
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.train.backends import CPUBackend
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr
from distributed_tensorflow_resnet_amd.utils import tensor_bundle as tb
from distributed_tensorflow_resnet_amd.utils.checkpoint import (Saver, ema_weights, state_to_tf,
                                                                tf_to_state)
from distributed_tensorflow_resnet_amd.utils.flags import build_parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMA = "/ExponentialMovingAverage"


# ---------------------------------------------------------------- the recurrence itself
@pytest.mark.parametrize("decay", [0.5, 0.9, 0.9999])
def test_recurrence_matches_closed_form_constant_and_ramp(decay):
    om, k, s0 = 1.0 - decay, 25, 3.0
    c = -1.25
    got = eo.ema_recurrence(s0, [c] * k, decay, warm=False)
    want = c + (1.0 - om) ** k * (s0 - c)
    assert abs(got - want) <= 1e-13 * max(1.0, abs(want))
    a, b = 0.5, 0.125
    ramp = [a + b * j for j in range(1, k + 1)]
    got = eo.ema_recurrence(s0, ramp, decay, warm=False)
    want = (1.0 - om) ** k * s0 + sum(om * (1.0 - om) ** (k - j) * (a + b * j)
                                      for j in range(1, k + 1))
    assert abs(got - want) <= 1e-13 * max(1.0, abs(want))
    # with warm-up: the product form, each factor from its own step count
    got = eo.ema_recurrence(s0, [c] * k, decay, warm=True)
    keep = np.prod([1.0 - eo.om_reference(decay, j, True) for j in range(1, k + 1)])
    assert abs(got - (c + keep * (s0 - c))) <= 1e-13


def test_warmup_switches_where_the_two_rates_cross():
    # decay 0.5: 9 / (10 + k) > 0.5 up to k = 7, equal at k = 8, below from 9 on
    oms = [eo.om_reference(0.5, k, True) for k in range(0, 12)]
    assert oms[:8] == [9.0 / (10 + k) for k in range(8)] and all(o > 0.5 for o in oms[:8])
    assert oms[8:] == [0.5] * 4
    assert eo.om_reference(0.5, 0, False) == 0.5
    # TF's form: 1 - min(decay, (1 + k) / (10 + k))
    for decay in (0.5, 0.9, 0.9999):
        for k in (0, 1, 7, 8, 9, 100, 10 ** 6):
            tf_form = 1.0 - min(decay, (1.0 + k) / (10.0 + k))
            assert abs(eo.om_reference(decay, k, True) - tf_form) <= 1e-15
    # 0.9999 takes over where 9 / (10 + k) < 1e-4: k > 89990
    assert eo.om_reference(0.9999, 89989, True) > 1.0 - 0.9999
    assert eo.om_reference(0.9999, 89991, True) == 1.0 - 0.9999


# ---------------------------------------------------------------- CPU backend
def _batch(n, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, 32, 32, 3, generator=gen), torch.randint(0, 10, (n,), generator=gen)


@pytest.mark.parametrize("warm", [True, False])
def test_cpu_backend_shadow_follows_the_oracle(warm):
    be = CPUBackend(cifar_spec(8), 8, weight_decay=5e-4, lr_schedule=constant_lr(0.1),
                    ema_decay=0.5, ema_warmup=warm)
    assert torch.equal(be.ema, be.store.master.detach()) and be.ema is not be.store.master
    assert list(be.ema_state()) == [s.name for s in be.store.train_slots]
    x, y = _batch(8)
    worst = 0.0
    for step in range(12):
        prev = be.ema.clone()
        be.set_batch(x, y)
        be.step()
        ref, B = eo.ema_reference(prev, be.store.master.detach(), 0.5, step + 1, warm)
        err = (be.ema.double() - ref).abs()
        worst = max(worst, float((err / B.clamp_min(1e-300)).max()))
        assert bool((err <= B).all()), (step, float(err.max()))
    print(f"cpu backend warm={warm}: max err/bound {worst:.3f}")
    assert not torch.equal(be.ema, be.store.master.detach())   # it lags the weights


def test_cpu_backend_without_ema_keeps_nothing():
    be = CPUBackend(cifar_spec(8), 4, weight_decay=0.0, lr_schedule=constant_lr(0.1))
    assert be.ema is None and be.ema_state() is None and be.ema_decay == 0.0
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            CPUBackend(cifar_spec(8), 4, weight_decay=0.0, lr_schedule=constant_lr(0.1),
                       ema_decay=bad)


# ---------------------------------------------------------------- checkpoints
def _stores():
    a, b = ParamStore(cifar_spec(8)), ParamStore(cifar_spec(8))
    a.initialize(1)
    b.initialize(2)
    return a, b


def test_checkpoint_entries_and_round_trip(tmp_path):
    a, b = _stores()
    mom = torch.randn(a.n_train)
    off = state_to_tf(a, mom, 7)
    want = ({s.name for s in a.train_slots} | {s.name + "/Momentum" for s in a.train_slots}
            | {s.name for s in a.stat_slots} | {"global_step"})
    assert set(off) == want                      # EMA off: exactly the reference's entries
    big = ParamStore(cifar_spec(50))
    assert len(state_to_tf(big, torch.zeros(big.n_train), 0)) == 403
    on = state_to_tf(a, mom, 7, ema=b.master.detach())
    assert set(on) == want | {s.name + EMA for s in a.train_slots}
    assert len(state_to_tf(big, torch.zeros(big.n_train), 0,
                           ema=torch.zeros(big.n_train))) == 403 + len(big.train_slots)
    for k in want:
        assert np.array_equal(on[k], off[k])
    prefix = Saver(str(tmp_path)).save(on, 7)
    loaded = tb.read_bundle(prefix)
    for s in a.train_slots:                      # TF's shadow name, the variable's shape
        assert loaded[s.name + EMA].shape == tuple(s.shape)
    c = ParamStore(cifar_spec(8))
    c.initialize(5)
    m2, e2 = torch.zeros(a.n_train), torch.zeros(a.n_train)
    assert tf_to_state(loaded, c, m2, ema=e2) == 7
    assert torch.equal(c.master.detach(), a.master.detach()) and torch.equal(m2, mom)
    assert torch.equal(e2, b.master.detach())
    # a run without EMA ignores the shadows
    d = ParamStore(cifar_spec(8))
    assert tf_to_state(loaded, d, torch.zeros(a.n_train)) == 7
    assert torch.equal(d.master.detach(), a.master.detach())


def test_restore_without_shadows_starts_them_from_the_weights(tmp_path, capsys):
    a, _ = _stores()
    prefix = Saver(str(tmp_path)).save(state_to_tf(a, torch.zeros(a.n_train), 3), 3)
    be = CPUBackend(cifar_spec(8), 4, weight_decay=0.0, lr_schedule=constant_lr(0.1), seed=9,
                    ema_decay=0.9)
    capsys.readouterr()
    be.load_state(Saver.restore(prefix))
    out = [l for l in capsys.readouterr().out.splitlines() if "EMA" in l]
    assert len(out) == 1 and "restored weights" in out[0]
    assert be.global_step == 3
    assert torch.equal(be.ema, a.master.detach()) and torch.equal(be.store.master.detach(),
                                                                  a.master.detach())
    # and the backend's own checkpoint carries them back
    be2 = CPUBackend(cifar_spec(8), 4, weight_decay=0.0, lr_schedule=constant_lr(0.1), seed=4,
                     ema_decay=0.9)
    be.ema.mul_(1.5)
    be2.load_state(be.state_tensors())
    assert capsys.readouterr().out == ""
    assert torch.equal(be2.ema, be.ema)


def test_ema_weights_swaps_trainables_only_and_never_falls_back():
    a, b = _stores()
    a.stats.data.add_(0.25)
    t = state_to_tf(a, None, 4, ema=b.master.detach())
    sw = ema_weights(t, a)
    want_b = state_to_tf(b, None, 4)
    for s in a.train_slots:
        assert np.array_equal(sw[s.name], want_b[s.name])
    for s in a.stat_slots:                       # BN moving statistics stay the raw ones
        assert np.array_equal(sw[s.name], t[s.name])
    assert int(sw["global_step"]) == 4
    assert np.array_equal(t[a.train_slots[0].name],
                          state_to_tf(a, None, 4)[a.train_slots[0].name])   # input untouched
    with pytest.raises(KeyError, match="ExponentialMovingAverage"):
        ema_weights(state_to_tf(a, None, 4), a)
    del t[a.train_slots[3].name + EMA]
    with pytest.raises(KeyError, match=a.train_slots[3].name):
        ema_weights(t, a)


# ---------------------------------------------------------------- flags
@pytest.mark.parametrize("kind", ["cifar", "imagenet", "cifar_eval", "imagenet_eval"])
def test_ema_flags(kind):
    f = build_parser(kind).parse_args([])
    assert (f.ema_decay, f.ema_warmup, f.eval_ema) == (0.0, True, False)
    f = build_parser(kind).parse_args(["--ema_decay", "0.9999", "--noema_warmup", "--eval_ema"])
    assert (f.ema_decay, f.ema_warmup, f.eval_ema) == (0.9999, False, True)
    assert build_parser(kind).parse_args(["--ema_warmup=false"]).ema_warmup is False
    for bad in ("1", "1.0", "-0.1", "-1", "x"):
        with pytest.raises(SystemExit):
            build_parser(kind).parse_args([f"--ema_decay={bad}"])
    assert "0.9999" in build_parser(kind).format_help()


# ---------------------------------------------------------------- evaluator
def test_evaluator_scores_shadows_with_eval_ema_and_weights_without(tmp_path, capsys):
    from distributed_tensorflow_resnet_amd.train import driver
    from distributed_tensorflow_resnet_amd.train.evaluator import CPUInference

    spec = cifar_spec(8)
    a, b = _stores()
    a.stats.data.add_(0.125)                     # statistics of the checkpoint, not of seed 2
    ckpt = state_to_tf(a, torch.zeros(a.n_train), 11, ema=b.master.detach())
    Saver(str(tmp_path / "ema")).save(ckpt, 11)

    def argv(train_dir):
        return ["--mode", "eval", "--device", "cpu", "--synthetic", "--resnet_size", "8",
                "--train_dir", str(train_dir), "--eval_batch_size", "8",
                "--eval_batch_count", "2", "--eval_once"]

    got = {}
    for ema in (False, True):
        flags = build_parser("cifar_eval").parse_args(argv(tmp_path / "ema")
                                                        + (["--eval_ema"] if ema else []))
        capsys.readouterr()
        got[ema] = driver.run_eval(flags, spec, "cpu")
        lines = capsys.readouterr().out.splitlines()
        assert (lines[0] == "INFO:tensorflow:weights: ema") == ema
        assert not any("weights: ema" in l for l in lines[1:])
    # the models loaded directly: seed-1 weights / seed-2 weights, both on the checkpoint's stats
    b.stats.data.copy_(a.stats.detach())
    batches = driver._eval_batches_factory(flags, spec)
    for ema, store in ((False, a), (True, b)):
        m = CPUInference(spec, 8)
        m.load(state_to_tf(store, None, 11))
        tot = cor = los = 0.0
        for i, (x, y) in enumerate(batches()):
            if i >= 2:
                break
            l, c, _ = m.run(x, y)
            los, cor, tot = los + l, cor + c, tot + y.shape[0]
        assert got[ema] == [(11, cor / tot, los / tot)]
    assert got[True][0][2] != got[False][0][2]
    # a checkpoint without shadows is an error under --eval_ema, never the raw weights
    Saver(str(tmp_path / "raw")).save(state_to_tf(a, None, 2), 2)
    flags = build_parser("cifar_eval").parse_args(argv(tmp_path / "raw") + ["--eval_ema"])
    with pytest.raises(KeyError):
        driver.run_eval(flags, spec, "cpu")


# ---------------------------------------------------------------- two gloo ranks
def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    from distributed_tensorflow_resnet_amd.parallel.dist import DistContext

    ctx = DistContext(backend="gloo")
    be = CPUBackend(cifar_spec(8), 4, weight_decay=5e-4, lr_schedule=constant_lr(0.1),
                    seed=100 + rank, dist_ctx=ctx, ema_decay=0.5)    # different inits
    be.ema.add_(float(rank))                                         # ... and shadows
    be.broadcast_parameters(0)
    x, y = _batch(4, seed=10 + rank)
    for _ in range(5):
        be.set_batch(x, y)
        be.step()
    torch.save([be.ema.clone(), be.store.master.detach().clone()],
               os.path.join(out_dir, f"r{rank}.pt"))
    ctx.shutdown()


def test_two_gloo_ranks_keep_identical_shadows(tmp_path):
    mp.spawn(_rank, args=(2, _port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "r0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "r1.pt", weights_only=True)
    assert torch.equal(r0[0], r1[0]) and torch.equal(r0[1], r1[1])
    assert not torch.equal(r0[0], r0[1])
