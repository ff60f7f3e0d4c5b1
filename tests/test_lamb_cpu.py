"""--optimizer adamw --adam_trust on (LAMB) without a GPU: the flags, the oracle's bounds
(tests/lamb_oracle.py) against an fp32 numpy emulation of csrc/lamb.hip's helper and summation
order, the CPU backend's update against the fp64 reference, and the CLI end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lamb_oracle as lmo
import optim_oracle as oo
from test_lars_gpu import TABLE_A
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.train.backends import CPUBackend
from distributed_tensorflow_resnet_amd.train.layout import (LARS_CHUNK, SEG_DTYPE,
                                                              adam_decay_table, check_adam_trust,
                                                              lamb_bias_corrections,
                                                              lamb_trust_summary)
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr
from distributed_tensorflow_resnet_amd.utils.flags import build_parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
# beta1, beta2, epsilon, wd, grad_scale: test_adam_gpu's two sets (a weight decay in both)
COEFFS = [(0.9, 0.999, 1e-8, 0.05, 1.0), (0.75, 0.95, 1e-3, 0.3, 0.5)]
STEPS = [1, 2, 1000, 2 ** 31 + 5]


# ---------------------------------------------------------------- flags
@pytest.mark.parametrize("kind", ["cifar", "imagenet"])
def test_lamb_flags(kind):
    f = build_parser(kind).parse_args([])
    assert (f.optimizer, f.adam_trust, f.adam_trust_skip) == ("mom", "off", "vectors")
    f = build_parser(kind).parse_args(["--optimizer", "adamw", "--adam_trust", "on"])
    assert (f.adam_trust, f.adam_trust_skip) == ("on", "vectors")
    f = build_parser(kind).parse_args(["--optimizer", "adamw", "--adam_trust", "on",
                                       "--adam_trust_skip", "none", "--clip_grad_norm", "1.0"])
    assert (f.adam_trust, f.adam_trust_skip) == ("on", "none")
    f = build_parser(kind).parse_args(["--optimizer", "adamw", "--adam_trust", "off",
                                       "--adam_trust_skip", "vectors"])
    assert (f.adam_trust, f.adam_trust_skip) == ("off", "vectors")
    # the skip alone is accepted and unused, as --lars_skip is without lars
    f = build_parser(kind).parse_args(["--optimizer", "mom", "--adam_trust_skip", "none"])
    assert (f.adam_trust, f.adam_trust_skip) == ("off", "none")
    for bad in (["--adam_trust", "yes"], ["--adam_trust", "1"], ["--adam_trust_skip", "biases"],
                ["--adam_trust", "on"],                            # the default optimizer is mom
                ["--optimizer", "mom", "--adam_trust", "on"],
                ["--optimizer", "sgd", "--adam_trust", "on"],
                ["--optimizer", "lars", "--adam_trust", "on"],
                ["--optimizer", "lamb"]):
        with pytest.raises(SystemExit):
            build_parser(kind).parse_args(bad)


def test_check_adam_trust_and_backend_errors():
    assert check_adam_trust("on", "none", "adamw") is True
    assert check_adam_trust("off", "vectors", "mom") is False
    kw = dict(weight_decay=1e-4, lr_schedule=constant_lr(1e-3))
    for opt in ("mom", "sgd", "lars"):
        with pytest.raises(ValueError):
            CPUBackend(cifar_spec(8), 4, optimizer=opt, adam_trust="on", **kw)
    for bad in (dict(adam_trust="maybe"), dict(adam_trust="on", adam_trust_skip="all")):
        with pytest.raises(ValueError):
            CPUBackend(cifar_spec(8), 4, optimizer="adamw", **bad, **kw)
    with pytest.raises(ValueError):
        CPUBackend(cifar_spec(8), 4, optimizer="lamb", **kw)
    be = CPUBackend(cifar_spec(8), 4, optimizer="adamw", adam_trust_skip="none", **kw)
    assert not be.lamb and be.lamb_state() is None and be.lamb_summary() is None
    assert lamb_trust_summary({}) == {}
    assert lamb_trust_summary({"a": (1, 2, 0.5), "b": (1, 2, 3.0), "c": (1, 1, 1.0)}) == \
        {"lamb_trust_min": 0.5, "lamb_trust_median": 1.0, "lamb_trust_max": 3.0}


# ---------------------------------------------------------------- the bounds, on the CPU
def test_bias_corrections_host_mirror():
    for b1, b2 in ((0.9, 0.999), (0.75, 0.95), (0.0, 0.99), (0.95, 0.0)):
        for t in STEPS + [10]:
            ref = lmo.bias_reference(t, b1, b2)
            got = lamb_bias_corrections(t, b1, b2)
            for g, r in zip(got, ref):
                assert abs(g - r) <= lmo.ulp(r), (b1, b2, t, g, r)
    assert lmo.bias_reference(2 ** 31 + 5, 0.9, 0.999) == (1.0, 1.0)
    assert lmo.bias_reference(1, 0.5, 0.75) == (2.0, 4.0)


def _emulate_helper(w, g, m, v, wd, s, k1, k2, b1, b2, eps, mode):
    """csrc/lamb.hip lamb_elem in numpy fp32: every operation rounded once, in its order."""
    b1, b2, eps, s, k1, k2 = (F(x) for x in (b1, b2, eps, s, k1, k2))
    omb1, omb2 = F(1.0 - float(b1)), F(1.0 - float(b2))
    gp = s * g
    if mode == "l2":
        gp = gp + wd * w
    m1 = b1 * m + omb1 * gp
    v1 = b2 * v + omb2 * (gp * gp)
    u = (m1 * k1) / (np.sqrt(v1 * k2) + eps)
    if mode == "decoupled":
        u = u + wd * w
    for x in (gp, m1, v1, u):
        assert x.dtype == np.float32
    return m1, v1, u


def _emulate_chunk_sum(x, a, b):
    """The kernel's sum of squares over the chunk [a, b): a scalar head up to the first
    multiple of 4, float4s (vector k to thread k % 256, in order), a scalar tail; fp32 within
    a thread in the kernel's order (body, head, tail), fp64 across the threads."""
    body0 = min((a + 3) & ~3, b)
    nvec = (b - body0) // 4
    tail0 = body0 + 4 * nvec
    acc = np.zeros(256, dtype=np.float32)
    for k in range(nvec):
        for i in range(4):
            e = x[body0 + 4 * k + i]
            acc[k % 256] = acc[k % 256] + e * e
    for tid in range(body0 - a):
        acc[tid] = acc[tid] + x[a + tid] * x[a + tid]
    for tid in range(b - tail0):
        acc[tid] = acc[tid] + x[tail0 + tid] * x[tail0 + tid]
    return float(acc.astype(np.float64).sum())


class CpuTable:
    """test_adam_gpu's Table on the CPU: O(1) values bounded away from zero, v0 = x^2."""

    def __init__(self, seed):
        specs = [s for s, _ in TABLE_A]
        self.seg, _, self.n, *_ = oo.build_seg_table(specs)
        self.shapes = [(1,) if s[0] == "vec" else (s[1], s[2], s[3], s[4]) for s in specs]
        gen = torch.Generator().manual_seed(seed)

        def rand():
            x = torch.randn(self.n, generator=gen)
            return x + 0.25 * torch.sign(x)

        self.w, self.g, self.m, x = rand(), rand(), rand(), rand()
        self.v = x * x

    def skip(self, mode):
        return [mode == "vectors" and len(s) == 1 for s in self.shapes]


@pytest.fixture(scope="module")
def cpu_table():
    T = CpuTable(31)
    assert {int(r["offset"]) % 4 for r in T.seg} == {0, 1, 2, 3}
    return T


@pytest.mark.parametrize("mode", ["decoupled", "l2"])
@pytest.mark.parametrize("ci", [0, 1])
def test_bounds_hold_for_an_fp32_emulation(cpu_table, ci, mode):
    T = cpu_table
    b1, b2, eps, wd, scale = COEFFS[ci]
    lr = 0.1
    wd_seg = adam_decay_table(T.shapes, wd, "vectors" if ci else "none")
    numel = [int(r["numel"]) for r in T.seg]
    wd_e = np.repeat(wd_seg, numel)
    skip = T.skip("vectors")
    chunks = lmo.chunk_bounds(T.seg, LARS_CHUNK)
    assert len(chunks) == sum(-(-k // LARS_CHUNK) for k in numel)
    w, g, m, v = (x.numpy() for x in (T.w, T.g, T.m, T.v))
    worst = 0.0
    for t in STEPS:
        k1, k2 = lamb_bias_corrections(t, b1, b2)
        m1, v1, u = _emulate_helper(w, g, m, v, wd_e, scale, k1, k2, b1, b2, eps, mode)
        R = lmo.lamb_reference(T.w, T.g, T.m, T.v, T.seg, wd_seg, skip, lr, t, b1, b2, eps, scale,
                               mode)
        for got, ref, B, name in ((m1, R["m"], R["Bm"], "m"), (v1, R["v"], R["Bv"], "v"),
                                  (u, R["u"], R["Eu"], "u")):
            err = (torch.from_numpy(got).double() - ref).abs()
            assert bool((err <= B).all()), (name, t, float((err / B.clamp_min(1e-300)).max()))
            worst = max(worst, float((err / B.clamp_min(1e-300)).max()))
        # the direction is far above its bound almost everywhere: the bound tests something
        assert float((R["u"].abs() / R["Eu"].clamp_min(1e-300)).median()) > 1e4
        # chunk partials in the kernel's order
        cw, cu, Bcw, Bcu = lmo.sums_reference(T.w, R["u"], R["Eu"], chunks)
        for (a, b), rw, ru, bw, bu in zip(chunks, cw, cu, Bcw, Bcu):
            assert abs(_emulate_chunk_sum(w, a, b) - rw) <= bw, (t, a, b)
            assert abs(_emulate_chunk_sum(u, a, b) - ru) <= bu, (t, a, b)
        # norms, trust and the update from the emulation's own sums
        pos = 0
        w_new = np.empty_like(w)
        for i, r in enumerate(T.seg):
            o, k = int(r["offset"]), int(r["numel"])
            nch = -(-k // LARS_CHUNK)
            sw = sum(_emulate_chunk_sum(w, a, b) for a, b in chunks[pos:pos + nch])
            su = sum(_emulate_chunk_sum(u, a, b) for a, b in chunks[pos:pos + nch])
            pos += nch
            wn, un = np.sqrt(sw), np.sqrt(su)
            tr = F(wn / un) if not skip[i] and wn > 0 and un > 0 else F(1.0)
            assert abs(float(F(un)) - R["un"][i]) <= R["Bun"][i], (t, i)
            assert abs(float(F(wn)) - R["wn"][i]) <= lmo.NORM_REL * R["wn"][i], (t, i)
            assert abs(float(tr) - R["trust"][i]) <= R["TR"][i] * R["trust"][i], (t, i)
            if skip[i]:
                assert float(tr) == 1.0 and R["trust"][i] == 1.0
            rate = F(lr) * tr
            w_new[o:o + k] = w[o:o + k] - rate * u[o:o + k]
        err = (torch.from_numpy(w_new).double() - R["w"]).abs()
        assert bool((err <= R["Bw"]).all()), (t, float((err / R["Bw"]).max()))
        assert float(((R["w"] - T.w.double()).abs() / R["Bw"]).median()) > 1e3
    print(f"emulation {mode} coeffs {ci}: worst err/bound {worst:.3f}")


def test_zero_direction_has_trust_one_and_keeps_w():
    seg = np.zeros(2, dtype=SEG_DTYPE)
    seg["offset"], seg["numel"] = [0, 5], [5, 7]
    w = torch.arange(1, 13, dtype=torch.float32)
    g = torch.cat([torch.zeros(5), torch.ones(7)])
    z = torch.zeros(12)
    R = lmo.lamb_reference(w, g, z, z, seg, [0.0, 0.0], [False, False], 0.1, 1, 0.9, 0.999, 1e-8,
                           1.0, "decoupled")
    assert R["un"][0] == 0.0 and R["trust"][0] == 1.0 and R["TR"][0] == 0.0
    assert torch.equal(R["w"][:5], w[:5].double()) and float(R["Eu"][:5].max()) == 0.0
    # first step from zero moments: r = g / (|g| + eps') ~ sign(g), so |u| = sqrt(7)
    assert R["un"][1] == pytest.approx(7 ** 0.5, rel=1e-6)
    assert R["trust"][1] == pytest.approx(float(w[5:].double().norm()) / 7 ** 0.5, rel=1e-6)


# ---------------------------------------------------------------- CPU backend against the oracle
def _seg_of(store):
    seg = np.zeros(len(store.train_slots), dtype=SEG_DTYPE)
    for r, s in zip(seg, store.train_slots):
        r["offset"], r["numel"] = s.offset, s.numel
    return seg


@pytest.mark.parametrize("mode", ["decoupled", "l2"])
@pytest.mark.parametrize("skip", ["vectors", "none"])
def test_cpu_backend_lamb_step_matches_fp64(skip, mode):
    """Two steps (the second from non-zero moments) of the backend's own fp32 gradient through
    the fp64 reference: the CPU backend is the kernels' expressions in fp32 torch (its sums
    of squares in fp64), so the kernels' bounds hold for it."""
    spec = cifar_spec(8)
    wd, lr, b1, b2, eps = 0.05, 1e-3, 0.9, 0.99, 1e-6
    be = CPUBackend(spec, 4, weight_decay=wd, lr_schedule=constant_lr(lr), optimizer="adamw",
                    adam_beta1=b1, adam_beta2=b2, adam_epsilon=eps, adam_decay=mode,
                    adam_trust="on", adam_trust_skip=skip)
    assert be.lamb and be.lamb_state() is None and be.lamb_summary() is None
    seg = _seg_of(be.store)
    wd_seg = [wd] * len(seg)
    skips = [skip == "vectors" and len(s.shape) == 1 for s in be.store.train_slots]
    assert any(skips) == (skip == "vectors")
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, 32, 32, 3, generator=gen)
    y = torch.randint(0, 10, (4,), generator=gen)
    for step in range(2):
        w0 = be.store.master.detach().clone()
        m0, v0 = be.mom.clone(), be.adam_v.clone()
        be.set_batch(x, y)
        be.step()
        g = be.store.master.grad.detach()
        R = lmo.lamb_reference(w0, g, m0, v0, seg, wd_seg, skips, lr, step + 1, b1, b2, eps, 1.0,
                               mode)
        for got, ref, B, name in ((be.store.master.detach(), R["w"], R["Bw"], "w"),
                                  (be.mom, R["m"], R["Bm"], "m"), (be.adam_v, R["v"], R["Bv"], "v")):
            err = (got.double() - ref).abs()
            assert bool((err <= B).all()), (name, step, float((err / B.clamp_min(1e-300)).max()))
        st = be.lamb_state()
        for i, s in enumerate(be.store.train_slots):
            wn, un, tr = st[s.name]
            assert abs(wn - R["wn"][i]) <= lmo.NORM_REL * R["wn"][i]
            assert abs(un - R["un"][i]) <= R["Bun"][i]
            assert abs(tr - R["trust"][i]) <= R["TR"][i] * R["trust"][i]
            if skips[i]:
                assert tr == 1.0
        adapted = [st[s.name][2] for s, sk in zip(be.store.train_slots, skips) if not sk]
        # (BN betas start at zero: |w| = 0 and trust 1 even when adapted)
        rank2 = sum(len(s.shape) > 1 for s in be.store.train_slots)
        assert sum(t != 1.0 for t in adapted) >= rank2
        # the update moved the weights by far more than the bounds
        assert float(((R["w"] - w0.double()).abs() / R["Bw"]).median()) > 1e3
        sm = be.lamb_summary()
        assert 0 < sm["lamb_trust_min"] <= sm["lamb_trust_median"] <= sm["lamb_trust_max"]
        assert sm["lamb_trust_min"] == min(adapted) and sm["lamb_trust_max"] == max(adapted)
        assert be.adam_state()[0] == step + 1


def test_lamb_and_adamw_checkpoints_are_interchangeable():
    def backend(trust, seed=0):
        return CPUBackend(cifar_spec(8), 4, weight_decay=1e-3, lr_schedule=constant_lr(1e-3),
                          optimizer="adamw", seed=seed, adam_trust=trust)

    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, 32, 32, 3, generator=gen)
    y = torch.randint(0, 10, (4,), generator=gen)
    a = backend("on")
    for _ in range(2):
        a.set_batch(x, y)
        a.step()
    t = a.state_tensors()
    plain = backend("off")
    for _ in range(2):
        plain.set_batch(x, y)
        plain.step()
    assert set(t) == set(plain.state_tensors())          # no entry of its own
    b = backend("off", seed=9)
    b.load_state(t)
    assert b.global_step == 2 and b.adam_start == 0
    assert torch.equal(b.mom, a.mom) and torch.equal(b.adam_v, a.adam_v)
    c = backend("on", seed=9)
    c.load_state(plain.state_tensors())
    assert torch.equal(c.adam_v, plain.adam_v) and torch.equal(c.store.master, plain.store.master)
    c.set_batch(x, y)
    c.step()
    assert c.adam_state()[0] == 3 and c.lamb_state() is not None


# ---------------------------------------------------------------- the CLI
def test_cli_lamb_logs_trust_ratios(tmp_path):
    e = dict(os.environ)
    e.update({"CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": "", "OMP_NUM_THREADS": "2"})
    td, ld = str(tmp_path / "train"), str(tmp_path / "log")
    r = subprocess.run([sys.executable, "resnet_cifar_main.py", "--device", "cpu", "--synthetic",
                        "--resnet_size", "8", "--batch_size", "4", "--log_every", "1",
                        "--summary_every", "1", "--optimizer", "adamw", "--adam_trust", "on",
                        "--train_steps", "3", "--train_dir", td, "--log_dir", ld],
                       cwd=ROOT, capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "lamb trust min/median/max" in r.stdout + r.stderr
    rows = [json.loads(line) for line in open(os.path.join(ld, "metrics.jsonl"))]
    assert len(rows) == 3
    for row in rows:
        assert 0 < row["lamb_trust_min"] <= row["lamb_trust_median"] <= row["lamb_trust_max"]
        assert "adam_alpha" in row and "lars_trust_min" not in row
