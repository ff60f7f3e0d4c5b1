"""--clip_grad_norm without a GPU: the flag, the constructors' checks, the CPU backend's
clipped update against tests/optim_oracle.py, two gloo ranks, the hooks and the CLI, and
the compiler's resource remarks of csrc/clip.hip."""
import json
import math
import os
import socket
import subprocess
import sys
import types

import pytest
import torch
import torch.multiprocessing as mp

import clip_oracle as co
import kernel_resources as kr
import optim_oracle as oo
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.train import hooks as H
from distributed_tensorflow_resnet_amd.train.backends import CPUBackend
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr
from distributed_tensorflow_resnet_amd.utils.flags import build_parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
WD, LR, MOMENTUM = 5e-4, 0.1, 0.9
BASE_KEYS = {"global_step", "cross_entropy", "cost", "precision", "lr", "l2"}


# ---------------------------------------------------------------- flags and constructors
@pytest.mark.parametrize("kind", ["cifar", "imagenet"])
def test_clip_flag(kind):
    assert build_parser(kind).parse_args([]).clip_grad_norm == 0.0
    for text, want in (("0", 0.0), ("1.5", 1.5), ("inf", INF)):
        assert build_parser(kind).parse_args(["--clip_grad_norm", text]).clip_grad_norm == want
    for bad in ("-1", "nan", "-inf", "x"):
        with pytest.raises(SystemExit):
            build_parser(kind).parse_args([f"--clip_grad_norm={bad}"])
    with pytest.raises(SystemExit):
        build_parser(kind).parse_args(["--clip_grad_norm", "1.5", "--optimizer", "lars"])
    # off, lars is as before
    assert build_parser(kind).parse_args(["--optimizer", "lars"]).clip_grad_norm == 0.0
    assert "--clip_grad_norm" in build_parser(kind).format_help()


def _cpu(**kw):
    return CPUBackend(cifar_spec(8), 4, weight_decay=WD, lr_schedule=constant_lr(LR),
                      momentum=MOMENTUM, **kw)


def _engine(**kw):
    from distributed_tensorflow_resnet_amd.train.engine import Engine

    return Engine(cifar_spec(8), 4, weight_decay=WD, lr_schedule=constant_lr(LR), **kw)


@pytest.mark.parametrize("kw", [dict(clip_grad_norm=-1.0), dict(clip_grad_norm=float("nan")),
                                dict(clip_grad_norm=1.0, optimizer="lars"),
                                dict(clip_grad_norm=INF, optimizer="lars")])
def test_constructors_raise_the_same_error(kw):
    """The check comes before anything touches a device, so Engine raises it here too."""
    msgs = []
    for make in (_cpu, _engine):
        with pytest.raises(ValueError) as ei:
            make(**kw)
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1] and "clip_grad_norm" in msgs[0]


# ---------------------------------------------------------------- CPU backend
def _batch(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, 32, 32, 3, generator=gen), torch.randint(0, 10, (n,), generator=gen)


def _run(be, steps=3, seed=3):
    """`steps` steps on one batch; per step (w0, m0, grad, clip_state, metrics)."""
    x, y = _batch(be.N, seed)
    rows = []
    for _ in range(steps):
        w0, m0 = be.store.master.detach().clone(), be.mom.clone()
        be.set_batch(x, y)
        be.step()
        rows.append((w0, m0, be.store.master.grad.detach().clone(), be.clip_state(),
                     be.metrics()))
    return rows


def test_cpu_backend_measure_only_is_bitwise_clipping_off():
    off, on = _cpu(), _cpu(clip_grad_norm=INF)
    assert off.clip_state() is None and on.clip_state() is None   # no step yet
    r_off, r_on = _run(off), _run(on)
    assert torch.equal(off.store.master, on.store.master) and torch.equal(off.mom, on.mom)
    for (_, _, g_off, st_off, m_off), (_, _, g, st, m) in zip(r_off, r_on):
        assert st_off is None and set(m_off) == BASE_KEYS
        assert set(m) == BASE_KEYS | {"grad_norm", "clip_scale"}
        assert torch.equal(g, g_off)
        _, ss = co.sumsq_reference(g, g.numel())
        co.check_norm_scale(st[0], st[1], ss, INF, "cpu measure-only")
        assert st[1] == 1.0 and (m["grad_norm"], m["clip_scale"]) == st


def test_cpu_backend_clipped_step_matches_fp64():
    probe = _cpu(clip_grad_norm=INF)
    norm0 = _run(probe, steps=1)[0][3][0]
    be = _cpu(clip_grad_norm=norm0 / 2)
    rows = _run(be)
    # a step's results are the next step's (w0, m0); the last step's the backend's buffers
    after = [(r[0], r[1]) for r in rows[1:]] + [(be.store.master.detach(), be.mom)]
    for step, ((w0, m0, g, st, _), (w1, m1)) in enumerate(zip(rows, after)):
        _, ss = co.sumsq_reference(g, g.numel())
        _, scale = co.check_norm_scale(st[0], st[1], ss, norm0 / 2, f"cpu step {step}")
        if step == 0:   # (c is half an fp32 norm that is itself within NORM_REL of exact)
            assert abs(scale - 0.5) <= 0.5 * (co.NORM_REL + 2 * co.U32) and st[1] < 1.0
        w_ref, m_ref, B = oo.sgd_reference(w0, g, m0, oo.f32(LR), oo.f32(MOMENTUM), oo.f32(WD),
                                           st[1], True)
        assert bool(((w1.double() - w_ref).abs() <= B).all()), step
        assert bool(((m1.double() - m_ref).abs() <= B).all()), step
        assert float((w1 - w0).abs().max()) > 1e-4


def test_cpu_backend_sgd_and_nan():
    """--optimizer sgd takes the same scale without the accumulator; a non-finite gradient
    gives a NaN scale (and NaN weights: the blown-up step is not hidden)."""
    be = _cpu(clip_grad_norm=1e-3, optimizer="sgd")
    (w0, m0, g, st, _), = _run(be, steps=1)
    assert st[1] < 1.0 and torch.equal(be.mom, m0)
    w_ref, _, B = oo.sgd_reference(w0, g, m0, oo.f32(LR), 0.0, oo.f32(WD), st[1], False)
    assert bool(((be.store.master.detach().double() - w_ref).abs() <= B).all())
    for bad in (INF, float("nan")):
        be = _cpu(clip_grad_norm=1.0)
        g = torch.ones(8)
        g[3] = bad
        assert math.isnan(float(be._clip_scale(g))) and math.isnan(be.clip_state()[1])


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
    be = CPUBackend(cifar_spec(8), 4, weight_decay=WD, lr_schedule=constant_lr(LR),
                    seed=100 + rank, dist_ctx=ctx, clip_grad_norm=0.05)   # different inits
    be.broadcast_parameters(0)
    x, y = _batch(4, seed=10 + rank)                                      # ... and batches
    states = []
    for _ in range(3):
        be.set_batch(x, y)
        be.step()
        states.append(be.clip_state())
    torch.save([torch.tensor(states, dtype=torch.float64), be.store.master.detach().clone(),
                be.mom.clone()], os.path.join(out_dir, f"r{rank}.pt"))
    ctx.shutdown()


def test_two_gloo_ranks_log_the_same_norm():
    import tempfile

    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_rank, args=(2, _port(), td), nprocs=2, join=True)
        r0 = torch.load(os.path.join(td, "r0.pt"), weights_only=True)
        r1 = torch.load(os.path.join(td, "r1.pt"), weights_only=True)
    for a, b in zip(r0, r1):
        assert torch.equal(a, b)
    assert bool((r0[0][:, 0] > 0).all()) and bool((r0[0][:, 1] < 1.0).any())


# ---------------------------------------------------------------- hooks and the CLI
class _Writer:
    def __init__(self):
        self.rows = []

    def add_scalars(self, step, vals):
        self.rows.append((step, dict(vals)))

    def flush(self):
        pass


def _session(metrics):
    return types.SimpleNamespace(metrics=lambda: metrics, is_chief=True,
                                 backend=types.SimpleNamespace(), global_step=1)


@pytest.mark.parametrize("on", [False, True])
def test_hooks_carry_the_two_values_only_with_the_flag(tmp_path, capsys, on):
    m = {"global_step": 1, "cross_entropy": 2.0, "cost": 2.5, "precision": 0.25, "lr": 0.1,
         "l2": 3.0}
    if on:
        m.update(grad_norm=1.25, clip_scale=0.5)
    s = _session(m)
    w = _Writer()
    H.SummarySaverHook(w, save_steps=1).after_run(s, 1)
    assert ({"grad_norm", "clip_scale"} <= set(w.rows[0][1])) == on
    if on:
        assert w.rows[0][1]["grad_norm"] == 1.25 and w.rows[0][1]["clip_scale"] == 0.5
    path = str(tmp_path / "metrics.jsonl")
    H.JsonlMetricsHook(path, every=1).after_run(s, 1)
    row = json.loads(open(path).read())
    assert ("grad_norm" in row, "clip_scale" in row) == (on, on)
    capsys.readouterr()
    H.LoggingTensorHook(every_n_iter=1).after_run(s, 1)
    line = capsys.readouterr().out + capsys.readouterr().err
    assert (", grad norm = 1.25 (scale 0.5)" in line) == on and "lr = 0.1" in line


def _cli(args):
    e = dict(os.environ)
    e.update({"CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": "", "OMP_NUM_THREADS": "2"})
    return subprocess.run([sys.executable, "resnet_cifar_main.py", "--device", "cpu", "--synthetic",
                           "--resnet_size", "8", "--batch_size", "4", "--log_every", "1",
                           "--summary_every", "1", "--train_steps", "2"] + args,
                          cwd=ROOT, capture_output=True, text=True, timeout=600, env=e)


@pytest.mark.parametrize("clip", ["0", "0.01"])
def test_cli_metrics_jsonl(tmp_path, clip):
    td, ld = str(tmp_path / "train"), str(tmp_path / "log")
    r = _cli(["--clip_grad_norm", clip, "--train_dir", td, "--log_dir", ld])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    rows = [json.loads(line) for line in open(os.path.join(ld, "metrics.jsonl"))]
    assert len(rows) == 2
    on = clip != "0"
    for row in rows:
        assert ("grad_norm" in row, "clip_scale" in row) == (on, on)
        if on:
            assert row["grad_norm"] > 0.01 and row["clip_scale"] == pytest.approx(
                0.01 / row["grad_norm"], rel=1e-5)
    assert ("grad norm = " in r.stdout + r.stderr) == on


def test_cli_rejects_clip_with_lars(tmp_path):
    r = _cli(["--clip_grad_norm", "1", "--optimizer", "lars", "--train_dir", str(tmp_path)])
    assert r.returncode == 2 and "--clip_grad_norm" in r.stderr


# ---------------------------------------------------------------- compiler remarks
@pytest.mark.skipif(not kr.have_compiler(), reason="no ROCm compiler")
def test_clip_kernels_have_no_spills():
    rows = kr._resources(os.path.join(kr.CSRC, "clip.hip"))
    kernels = {n: r for n, r in rows.items() if "clip" in n or "sqnorm" in n}
    assert len(kernels) == 3, sorted(rows)
    for name, r in kernels.items():
        assert int(r["VGPRs Spill"]) == 0, (name, r)
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
