"""The Lion kernel (csrc/lion.hip lion_update_pack) launched directly on synthetic parameter
tables, and the engine's lion optimizer on both plans, against the fp64 reference and the
derived bounds of tests/lion_oracle.py.  g and m are seeded normals at magnitudes 1e-3 to 1;
every test first asserts, on the oracle alone, that at most 1e-3 of its elements have a sign
an fp32 evaluation may get either way.  Every decided element moves by lr, far above its
bound: a wrong sign, swapped betas, a missing decay or a decay of the new w fails."""
import numpy as np
import pytest
import torch

import lion_oracle as lio
import optim_oracle as oo
from test_adam_gpu import CLIP_SLOT, COSINE, _check_lr, _check_wbf, _sa, _st
from test_lamb_gpu import _recorded_calls
from test_lars_gpu import SEVEN, TABLE_A, V
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule
from distributed_tensorflow_resnet_amd.train.layout import (OPT_FUSED_LION_REASON,
                                                              adam_decay_table)

pytestmark = pytest.mark.gpu

# beta1, beta2, wd, grad_scale
COEFFS = [(0.9, 0.99, 0.05, 1.0), (0.0, 0.5, 0.3, 0.5)]
STEPS = [0, 3, 12, 2 ** 31 + 7]   # step 0, SEVEN's warm-up, past it, past 2^31


@pytest.fixture(scope="module")
def nat(gpu):
    import distributed_tensorflow_resnet_amd as dtr

    return dtr.native(required=True)


class Table:
    """A synthetic table with lion_oracle.lion_inputs' data; the segments in `zero` have
    g = m = 0, the elements in `nan` a NaN gradient."""

    def __init__(self, specs, gpu, seed, zero=(), nan=()):
        (self.seg, self.names, self.n, self.bf_total, tile0, self.tiles) = oo.build_seg_table(specs)
        self.gpu, self.nseg = gpu, len(self.seg)
        self.shapes = [(1,) if s[0] == "vec" else (s[1], s[2], s[3], s[4]) for s in specs]
        self.segs_d = torch.from_numpy(self.seg.view(np.uint8).copy()).to(gpu)
        self.tile0_d = torch.from_numpy(tile0).to(gpu)
        w, g, m = lio.lion_inputs(self.n, seed)
        self.zero_mask = torch.zeros(self.n, dtype=torch.bool)
        for i in zero:
            o, k = int(self.seg[i]["offset"]), int(self.seg[i]["numel"])
            self.zero_mask[o:o + k] = True
        g[self.zero_mask] = 0.0
        m[self.zero_mask] = 0.0
        for e in nan:
            g[e] = float("nan")
        self.w0, self.g, self.m0 = (t.to(gpu) for t in (w, g, m))
        self.zero_mask = self.zero_mask.to(gpu)

    def wd_table(self, wd, skip):
        return adam_decay_table(self.shapes, wd, skip)

    def fresh(self):
        return (self.w0.clone(), self.m0.clone(),
                torch.zeros(self.bf_total, dtype=torch.bfloat16, device=self.gpu))


def _launch(nat, T, sched, gstep_v, coeff, wd_seg, clip_on):
    """lion_update_pack + ohwi_pack on fresh buffers; returns (w, m, wbf, lr)."""
    b1, b2, _, gs = coeff
    gpu = T.gpu
    w, m, wbf = T.fresh()
    gstep = torch.tensor([gstep_v], dtype=torch.int64, device=gpu)
    lr_out = torch.full((1,), 7.0, device=gpu)
    clip = torch.tensor(CLIP_SLOT, device=gpu) if clip_on else None
    wd_d = torch.from_numpy(wd_seg).to(gpu)
    extra = () if sched.decay == "piecewise" else (sched.decay_args(),)
    # (with a clip slot the host grad_scale must be ignored: a wrong one is handed in)
    nat.lion_update_pack(w.data_ptr(), T.g.data_ptr(), m.data_ptr(), T.n, *_sa(sched),
                         gstep.data_ptr(), b1, b2, 55.0 if clip_on else gs,
                         clip.data_ptr() if clip_on else 0, T.segs_d.data_ptr(), T.nseg,
                         wd_d.data_ptr(), wbf.data_ptr(), lr_out.data_ptr(), *extra, _st())
    nat.ohwi_pack(w.data_ptr(), T.segs_d.data_ptr(), T.tile0_d.data_ptr(), T.nseg, T.tiles,
                  wbf.data_ptr(), gstep.data_ptr(), _st())
    torch.cuda.synchronize()
    assert int(gstep) == gstep_v + 1
    if clip_on:
        assert tuple(clip.tolist()) == tuple(oo.f32(c) for c in CLIP_SLOT)
    return w, m, wbf, float(lr_out)


def _full(nat, T, sched, gstep_v, coeff, skip, clip_on, what):
    """One launch against the oracle: the undecided share first (the oracle alone; c does not
    depend on the rate), then lr_out, w', m' and the bf16 copy."""
    b1, b2, wd, gs = coeff
    wd_seg = T.wd_table(wd, skip)
    scale = CLIP_SLOT[1] if clip_on else gs
    lio.assert_decidable(lio.lion_reference(T.w0, T.g, T.m0, T.seg, wd_seg, sched.init, b1, b2,
                                            scale), what)
    w, m, wbf, lr = _launch(nat, T, sched, gstep_v, coeff, wd_seg, clip_on)
    _check_lr(sched, gstep_v, lr)
    ref = lio.lion_reference(T.w0, T.g, T.m0, T.seg, wd_seg, lr, b1, b2, scale)
    worst = lio.check(w, m, ref, lr, what)
    print(f"{what} max err/bound: w {worst[0]:.3f} m {worst[1]:.3f}")
    _check_wbf(T.seg, w, wbf, what)
    return w, m, wbf


# ---------------------------------------------------------------- (a) synthetic tables
@pytest.fixture(scope="module")
def table_a(gpu):
    """A 10-element bias whose float4 straddles a segment end, tensor ends off the multiples
    of 4, a padded-K bf16 copy, tensors without a copy, n % 4 != 0; 2e4 elements."""
    T = Table([s for s, _ in TABLE_A], gpu, seed=31)
    offs = [int(r["offset"]) for r in T.seg]
    assert {o % 4 for o in offs} == {0, 1, 2, 3} and T.n % 4 != 0
    assert any(int(r["numel"]) == 10 and int(r["offset"]) % 4 for r in T.seg)
    assert any(int(r["kpad"]) != int(r["K"]) and r["bf_hwio"] >= 0 for r in T.seg)
    assert any(r["bf_hwio"] < 0 for r in T.seg)
    return T


@pytest.mark.parametrize("clip_on", [False, True])
@pytest.mark.parametrize("skip", ["none", "vectors"])
@pytest.mark.parametrize("ci", [0, 1])
def test_lion_kernel_against_fp64(gpu, nat, table_a, ci, skip, clip_on):
    T = table_a
    if skip == "vectors":
        tab = T.wd_table(1.0, skip).tolist()
        assert 0.0 in tab and 1.0 in tab
    for sched in (SEVEN, COSINE):
        for gstep_v in STEPS:
            a = _full(nat, T, sched, gstep_v, COEFFS[ci], skip, clip_on,
                      f"table A {sched.decay} step={gstep_v}")
    b = _full(nat, T, COSINE, STEPS[-1], COEFFS[ci], skip, clip_on, "again")
    for x, y in zip(a, b):   # a second identical launch: bit-equal
        assert torch.equal(x, y)


# ---------------------------------------------------------------- (b) exact cases
@pytest.mark.parametrize("wd", [0.0, 0.25])
def test_lion_zero_elements_are_exact(gpu, nat, wd):
    zero = {1, 4, 7, 13}   # a conv, a 5-vector, the kpad > K conv, the 10-class dense
    T = Table([s for s, _ in TABLE_A], gpu, seed=32, zero=zero)
    assert int(T.zero_mask.sum()) > 1000
    coeff = (0.9, 0.99, wd, 1.0)
    wd_seg = T.wd_table(wd, "none")
    lio.assert_decidable(lio.lion_reference(T.w0, T.g, T.m0, T.seg, wd_seg, SEVEN.init, 0.9, 0.99,
                                            1.0))
    w, m, wbf, lr = _launch(nat, T, SEVEN, 12, coeff, wd_seg, False)
    z = T.zero_mask
    assert int(m[z].count_nonzero()) == 0
    if wd == 0.0:
        assert torch.equal(w[z], T.w0[z])       # bit for bit
    else:                                       # exactly w - (lr wd) w, each rounded once
        lrwd = torch.tensor(lr, device=gpu) * torch.tensor(wd, device=gpu)
        assert lrwd.dtype == torch.float32
        assert torch.equal(w[z], T.w0[z] - lrwd * T.w0[z])
        assert not torch.equal(w[z], T.w0[z])
    assert not torch.equal(w[~z], T.w0[~z])
    ref = lio.lion_reference(T.w0, T.g, T.m0, T.seg, wd_seg, lr, 0.9, 0.99, 1.0)
    lio.check(w, m, ref, lr, f"zero blocks wd={wd}")
    _check_wbf(T.seg, w, wbf)


def test_lion_nan_gradient_stays_in_its_element(gpu, nat):
    specs = [s for s, _ in TABLE_A]
    seg = oo.build_seg_table(specs)[0]
    # inside a float4 of a conv, in the straddling 10-vector, the last element (the tail)
    n = int(seg[-1]["offset"] + seg[-1]["numel"])
    nan = [int(seg[3]["offset"]) + 6, int(seg[8]["offset"]) + 3, n - 1]
    T = Table(specs, gpu, seed=35, nan=nan)
    wd_seg = T.wd_table(0.05, "none")
    lio.assert_decidable(lio.lion_reference(T.w0, T.g, T.m0, T.seg, wd_seg, SEVEN.init,
                                            *COEFFS[0][:2], 1.0))
    w, m, wbf, lr = _launch(nat, T, SEVEN, 12, COEFFS[0], wd_seg, False)
    want = torch.zeros(T.n, dtype=torch.bool, device=gpu)
    want[nan] = True
    assert torch.equal(torch.isnan(w), want) and torch.equal(torch.isnan(m), want)
    ref = lio.lion_reference(T.w0, T.g, T.m0, T.seg, wd_seg, lr, *COEFFS[0][:2], 1.0)
    lio.check(w, m, ref, lr, "NaN gradient")


# ---------------------------------------------------------------- (c) table and grid extremes
def test_lion_long_tables(gpu, nat):
    """More than 640 segments: the update reads the segment table from global memory."""
    specs = []
    for i in range(700):
        k = i % 4
        specs.append(("conv", 1, 1, 4, 8, 4, 8, True, True) if k == 0 else
                     ("conv", 3, 3, 4, 4, 8, 4, True, True) if k == 2 else
                     V(1 + i % 9) if k == 1 else V(1 + i % 5))
    T = Table(specs, gpu, seed=33)
    assert T.nseg == 700
    _full(nat, T, SEVEN, 12, COEFFS[0], "vectors", False, "700 segments")
    _full(nat, T, COSINE, 12, COEFFS[1], "vectors", True, "700 segments clip")


def test_lion_grid_stride(gpu, nat):
    """More float4s than 4096 x 256 threads: the update loop's second trip, and segment ends
    off the multiples of 4."""
    n = 4 * 256 * 4096 + 4099
    specs, off = [], 0
    special = {0: ("conv", 1, 1, 333, 1001, 333, 1001, False, True),
               3: ("conv", 1, 1, 129, 515, 129, 520, False, True)}
    for i in range(8):
        s = special.get(i)
        if s is None:
            size = 500003 + 1000 * i
            while (off + size) % 4 == 0:
                size += 1
            s = V(size)
        specs.append(s)
        off += s[1] * s[2] * s[3] * s[4]
    specs.append(V(n - off))
    T = Table(specs, gpu, seed=34)
    assert T.n == n and (n + 3) // 4 > 4096 * 256
    _full(nat, T, cifar_lr_schedule(), 7, COEFFS[1], "vectors", False, "grid-stride")


# ---------------------------------------------------------------- (d) the binding
def test_lion_rejects_unaligned_buffers_and_bad_betas(gpu, nat, table_a):
    T = table_a
    w, m, wbf = T.fresh()
    g = T.g.clone()
    gstep = torch.zeros(1, dtype=torch.int64, device=gpu)
    wd_d = torch.from_numpy(T.wd_table(0.1, "none")).to(gpu)

    def call(ptrs, b1=0.9, b2=0.99):
        nat.lion_update_pack(*ptrs, T.n - 4, *_sa(SEVEN), gstep.data_ptr(), b1, b2, 1.0, 0,
                             T.segs_d.data_ptr(), T.nseg, wd_d.data_ptr(), wbf.data_ptr(), 0, _st())

    base = [w.data_ptr(), g.data_ptr(), m.data_ptr()]
    for i in range(3):
        ptrs = list(base)
        ptrs[i] += 4
        with pytest.raises(ValueError):
            call(ptrs)
    for kw in (dict(b1=1.0), dict(b1=-0.1), dict(b2=1.5), dict(b2=float("nan"))):
        with pytest.raises(ValueError):
            call(base, **kw)
    torch.cuda.synchronize()
    assert torch.equal(w, T.w0) and torch.equal(m, T.m0)
    assert int(wbf.count_nonzero()) == 0


# ---------------------------------------------------------------- (e) engine
WD = 5e-4
LION = dict(lion_beta1=0.9, lion_beta2=0.95)


def _engine(spec, N, gpu, optimizer="lion", seed=0, **kw):
    kw = {**(LION if optimizer == "lion" else {}), **kw}
    eng = Engine(spec, N, weight_decay=WD, lr_schedule=cifar_lr_schedule(), optimizer=optimizer,
                 device=gpu, input_mode="nhwc", seed=seed, **kw)
    gen = torch.Generator().manual_seed(5)
    imgs = torch.randn(N, spec.image_h, spec.image_w, 3, generator=gen).to(torch.bfloat16).float()
    eng.set_batch(imgs.to(gpu), torch.randint(0, spec.num_classes, (N,), generator=gen).to(gpu))
    return eng


def _check_engine_step(eng, w0, m0, step, what):
    """The engine's own gradient through lion_reference against its master and m: the
    optimizer alone, without the convolutions' bf16 noise."""
    n = eng.params.n_train
    lr = oo.f32(oo.lr_reference(eng.sched, step))
    assert eng.metrics()["lr"] == lr
    scale = 1.0
    if eng.clip_grad_norm > 0:
        norm, scale = eng.clip_state()
        assert scale < 1.0, (norm, scale)
    wd_seg = adam_decay_table([s.shape for s in eng.params.train_slots], eng.wd,
                              eng.lion_decay_skip)
    ref = lio.lion_reference(w0, eng.grad, m0, eng.seg_arr, wd_seg, lr, eng.lion_beta1,
                             eng.lion_beta2, scale)
    lio.assert_decidable(ref, what)
    worst = lio.check(eng.params.master[:n], eng.mom[:n], ref, lr, f"{what} step {step}")
    print(f"{what} step {step}: max err/bound master {worst[0]:.3f} m {worst[1]:.3f}")
    assert eng.adam_state() is None and eng.lamb_state() is None
    m = eng.metrics()
    assert m["optimizer"] == "lion" and "adam_alpha" not in m
    assert torch.equal(eng.wbf, oo.expected_wbf(eng.seg_arr, eng.params.master, eng.wbf.numel()))


def _run_steps(eng, steps, what):
    for step in range(steps):
        w0, m0 = eng.params.master.clone(), eng.mom.clone()
        assert int(eng.gstep.item()) == step
        eng.step()
        torch.cuda.synchronize()
        assert not eng.persist_error()
        _check_engine_step(eng, w0, m0, step, what)
    assert int(eng.gstep.item()) == steps


OPT_OPS = ("grad_sqnorm", "clip_scale", "lion_update_pack", "adam_update_pack", "ohwi_pack",
           "sgd_update_pack", "sgd_clip_update_pack", "sgd_tiles", "lars_update_pack",
           "lamb_update_pack", "ema_update")


@pytest.mark.parametrize("clip", [0.0, 0.05])
@pytest.mark.parametrize("persist", [0, 1])
def test_engine_lion_step(gpu, monkeypatch, persist, clip):
    monkeypatch.setenv("DTR_TUNE", f"persist={persist}")
    eng = _engine(cifar_spec(8), 16, gpu, clip_grad_norm=clip,
                  lion_decay_skip="vectors" if clip else "none", ema_decay=0.99 if clip else 0.0)
    assert eng.persist == bool(persist) and eng.lion and not eng.adam
    assert not eng.opt_fused and eng.opt_fused_reason == OPT_FUSED_LION_REASON
    assert "lion" in eng.opt_fused_reason
    assert eng.adam_v is None and eng.adam_out is None     # one state buffer: the momentum's
    names = eng.plan.names()
    a, b = eng.seg["opt"]
    assert [n for n in names[a:b] if n in OPT_OPS] == \
        (["grad_sqnorm", "clip_scale"] if clip else []) + ["lion_update_pack", "ohwi_pack"] + \
        (["ema_update"] if clip else [])                   # the EMA op stays last
    assert not any(n in ("sgd_update_pack", "sgd_clip_update_pack", "sgd_tiles") for n in names)
    _run_steps(eng, 2, f"cifar8 persist={persist} clip={clip}")   # step 1: a non-zero m


def test_engine_lion_imagenet_s2d_stem(gpu, monkeypatch):
    monkeypatch.setenv("DTR_TUNE", "persist=0")
    eng = _engine(imagenet_spec(18, image_hw=64), 8, gpu)
    assert eng.stem_s2d
    _run_steps(eng, 1, "imagenet18 s2d")


@pytest.mark.parametrize("dtype,persist", [("fp32", "0"), ("bf16", "1")])
def test_engine_lion_takes_the_exchanged_gradient(gpu, monkeypatch, dtype, persist):
    """comm = the doubling loopback: the update is formed from the all-reduced gradient
    (2x the local one; bf16: rebuilt from the bf16 exchange)."""
    import distributed_tensorflow_resnet_amd as dtr

    monkeypatch.setenv("DTR_TUNE", f"persist={persist}")
    spec = cifar_spec(8)
    ref = _engine(spec, 16, gpu, optimizer="mom")
    eng = _engine(spec, 16, gpu, comm=dtr.native().Comm.loopback(2.0), bucket_mb=0.05,
                  allreduce_dtype=dtype)
    assert eng.persist == (persist == "1") and not eng.opt_fused
    assert torch.equal(eng.params.master, ref.params.master)
    w0, m0 = eng.params.master.clone(), eng.mom.clone()
    ref.step()
    eng.step()
    torch.cuda.synchronize()
    base = ref.grad if dtype == "fp32" else ref.grad.to(torch.bfloat16).float()
    assert torch.equal(eng.grad, 2 * base)
    _check_engine_step(eng, w0, m0, 0, f"loopback {dtype}")


def _state(eng):
    return [eng.params.master.clone(), eng.mom.clone(), eng.params.stats.clone(),
            eng.wbf.clone(), eng.gstep.clone()]


def test_engine_lion_same_seed_engines_agree_bitwise(gpu):
    a, b = _engine(cifar_spec(8), 16, gpu), _engine(cifar_spec(8), 16, gpu)
    for _ in range(5):
        a.step()
        b.step()
    torch.cuda.synchronize()
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    assert int(a.gstep.item()) == 5 and float(a.mom.abs().max()) > 0


def test_engine_lion_resume_is_bitwise(gpu, tmp_path):
    from distributed_tensorflow_resnet_amd.train.backends import GPUBackend
    from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver

    straight = _engine(cifar_spec(8), 16, gpu)
    for _ in range(6):
        straight.step()
    first = GPUBackend(_engine(cifar_spec(8), 16, gpu))
    for _ in range(3):
        first.step()
    torch.cuda.synchronize()
    tensors = first.state_tensors()
    assert "conv2d/kernel/Lion" in tensors
    assert not any(k.endswith(("/Momentum", "/Adam", "/Adam_1")) for k in tensors)
    assert "adam_start_step" not in tensors and "beta1_power" not in tensors
    prefix = Saver(str(tmp_path)).save(tensors, 3)
    second = GPUBackend(_engine(cifar_spec(8), 16, gpu, seed=9))
    second.load_state(Saver.restore(prefix))
    assert second.global_step == 3
    for _ in range(3):
        second.step()
    torch.cuda.synchronize()
    for x, y in zip(_state(straight), _state(second.engine)):
        assert torch.equal(x, y)


def test_engine_lion_restores_a_mom_checkpoint(gpu, capsys):
    from distributed_tensorflow_resnet_amd.train.backends import GPUBackend

    mom = GPUBackend(_engine(cifar_spec(8), 16, gpu, optimizer="mom"))
    for _ in range(3):
        mom.step()
    torch.cuda.synchronize()
    assert float(mom.engine.mom.abs().max()) > 0
    be = GPUBackend(_engine(cifar_spec(8), 16, gpu, seed=9))
    be.step()                                   # a non-zero m to be cleared
    capsys.readouterr()
    be.load_state(mom.state_tensors())
    assert capsys.readouterr().out.count("no Lion slots") == 1
    eng = be.engine
    assert be.global_step == 3 and int(eng.gstep.item()) == 3
    assert int(eng.mom.count_nonzero()) == 0
    assert torch.equal(eng.params.master, mom.engine.params.master)
    w0, m0 = eng.params.master.clone(), eng.mom.clone()
    be.step()
    torch.cuda.synchronize()
    _check_engine_step(eng, w0, m0, 3, "after a mom checkpoint")
    # and back: a mom run restoring the lion checkpoint keeps its own (zero) momentum
    back = GPUBackend(_engine(cifar_spec(8), 16, gpu, optimizer="mom", seed=5))
    back.load_state(be.state_tensors())
    assert back.global_step == 4 and int(back.engine.mom.count_nonzero()) == 0


def test_engine_lion_graph_replay_equals_eager(gpu):
    spec = cifar_spec(8)
    eager = _engine(spec, 16, gpu, use_graph=True)   # the same recording,
    graph = _engine(spec, 16, gpu, use_graph=True)   # stepped eagerly / replayed
    for _ in range(6):
        eager.step()
    done = graph.capture(warmup=2)
    assert graph.graph is not None
    for _ in range(6 - done):
        graph.step()
    torch.cuda.synchronize()
    assert int(graph.gstep.item()) == 6
    for x, y in zip(_state(eager), _state(graph)):
        assert torch.equal(x, y)


# ---------------------------------------------------------------- (f) other optimizers unchanged
@pytest.mark.parametrize("optimizer,persist,opt_ops", [
    ("mom", 1, ["sgd_tiles"]), ("mom", 0, ["sgd_update_pack", "ohwi_pack"]),
    ("adamw", 1, ["adam_update_pack", "ohwi_pack"])])
def test_other_optimizers_unchanged(gpu, monkeypatch, optimizer, persist, opt_ops):
    """The lion flags reach no plan but lion's: with them at other values a mom and an adamw
    engine record the same ops with the same arguments and allocate the same bytes, and the
    optimizer segment is the one they have always recorded."""
    monkeypatch.setenv("DTR_TUNE", f"persist={persist}")
    base, ops0, grown0 = _recorded_calls(gpu, monkeypatch, optimizer=optimizer, trust="off")
    other, ops1, grown1 = _recorded_calls(gpu, monkeypatch, optimizer=optimizer, trust="off",
                                          lion_beta1=0.5, lion_beta2=0.25,
                                          lion_decay_skip="vectors")
    assert len(ops0) > 10 and ops1 == ops0 and grown1 == grown0
    for eng in (base, other):
        assert not eng.lion and eng.lion_wd is None and eng.persist == bool(persist)
        names = eng.plan.names()
        assert "lion_update_pack" not in names and "lion" not in eng.opt_fused_reason
        a, b = eng.seg["opt"]
        assert [n for n in names[a:b] if n in OPT_OPS] == opt_ops
    base.step()
    torch.cuda.synchronize()
    assert "optimizer" not in base.metrics()
    with pytest.raises(ValueError):
        _engine(cifar_spec(8), 16, gpu, lion_beta2=1.0)
    with pytest.raises(ValueError):
        _engine(cifar_spec(8), 16, gpu, adam_trust="on")
