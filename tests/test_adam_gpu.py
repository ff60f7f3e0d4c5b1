"""The AdamW kernel (csrc/adam.hip adam_update_pack) launched directly on synthetic parameter
tables, and the engine's adamw optimizer on both plans, against the fp64 reference and the
derived bounds of tests/adam_oracle.py.  The data is O(1) and bounded away from zero with
v0 = x^2, so every term of the update is far above its bound: a dropped or doubled term,
swapped betas, a missing bias correction or decay in the wrong mode fails."""
import numpy as np
import pytest
import torch

import adam_oracle as ao
import lr_decay_oracle as ldo
import optim_oracle as oo
from test_lars_gpu import SEVEN, TABLE_A, V
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule
from distributed_tensorflow_resnet_amd.train.layout import adam_decay_table

pytestmark = pytest.mark.gpu

# beta1, beta2, epsilon, wd, grad_scale
COEFFS = [(0.9, 0.999, 1e-8, 0.05, 1.0), (0.75, 0.95, 1e-3, 0.3, 0.5)]
COSINE = ldo._mk("cosine", 2, 2 ** 33, peak=0.1, end=0.001)
STEPS = [1, 2, 10, 1000, 2 ** 31 + 5]
CLIP_SLOT = (123.0, 0.37)   # {norm, scale} as clip_scale leaves them


@pytest.fixture(scope="module")
def nat(gpu):
    import distributed_tensorflow_resnet_amd as dtr

    return dtr.native(required=True)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _sa(s):
    return (s.init, s.warm_steps, s.warm_from, s.warm_to, list(s.bounds), list(s.values))


class Table:
    """A synthetic table with O(1) values bounded away from zero and v0 = x^2; the segments
    in `zero` have g = m = v = 0."""

    def __init__(self, specs, gpu, seed, zero=()):
        (self.seg, self.names, self.n, self.bf_total, tile0, self.tiles) = oo.build_seg_table(specs)
        self.gpu, self.nseg = gpu, len(self.seg)
        self.shapes = [(1,) if s[0] == "vec" else (s[1], s[2], s[3], s[4]) for s in specs]
        self.segs_d = torch.from_numpy(self.seg.view(np.uint8).copy()).to(gpu)
        self.tile0_d = torch.from_numpy(tile0).to(gpu)
        gen = torch.Generator().manual_seed(seed)

        def rand():
            x = torch.randn(self.n, generator=gen)
            return x + 0.25 * torch.sign(x)

        w, g, m, x = rand(), rand(), rand(), rand()
        v = x * x
        self.zero_mask = torch.zeros(self.n, dtype=torch.bool)
        for i in zero:
            o, k = int(self.seg[i]["offset"]), int(self.seg[i]["numel"])
            self.zero_mask[o:o + k] = True
        for t in (g, m, v):
            t[self.zero_mask] = 0.0
        self.w0, self.g, self.m0, self.v0 = (t.to(gpu) for t in (w, g, m, v))
        self.zero_mask = self.zero_mask.to(gpu)

    def wd_table(self, wd, skip):
        return adam_decay_table(self.shapes, wd, skip)

    def fresh(self):
        return (self.w0.clone(), self.m0.clone(), self.v0.clone(),
                torch.zeros(self.bf_total, dtype=torch.bfloat16, device=self.gpu))


def _check_lr(sched, step, lr):
    if sched.decay != "piecewise":
        ldo.check_rate(sched, step, lr, "adam lr")
        return
    ref = oo.lr_reference(oo.f32_schedule(sched), step)
    if oo.lr_in_warmup(sched, step):
        assert abs(lr - ref) <= oo.lr_bound(sched), (step, lr, ref)
    else:
        assert lr == oo.f32(ref), (step, lr, ref)


def _launch(nat, T, sched, gstep_v, start_v, coeff, mode, wd_seg, clip_on):
    """adam_update_pack + ohwi_pack on fresh buffers; returns (w, m, v, wbf, lr, out[3])."""
    b1, b2, eps, _, gs = coeff
    gpu = T.gpu
    w, m, v, wbf = T.fresh()
    gstep = torch.tensor([gstep_v], dtype=torch.int64, device=gpu)
    start = torch.tensor([start_v], dtype=torch.int64, device=gpu)
    lr_out = torch.full((1,), 7.0, device=gpu)
    out = torch.full((3,), float("nan"), device=gpu)
    clip = torch.tensor(CLIP_SLOT, device=gpu) if clip_on else None
    wd_d = torch.from_numpy(wd_seg).to(gpu)
    extra = () if sched.decay == "piecewise" else (sched.decay_args(),)
    # (with a clip slot the host grad_scale must be ignored: a wrong one is handed in)
    nat.adam_update_pack(w.data_ptr(), T.g.data_ptr(), m.data_ptr(), v.data_ptr(), T.n,
                         *_sa(sched), gstep.data_ptr(), start.data_ptr(), b1, b2, eps,
                         55.0 if clip_on else gs, clip.data_ptr() if clip_on else 0, mode,
                         T.segs_d.data_ptr(), T.nseg, wd_d.data_ptr(), wbf.data_ptr(),
                         lr_out.data_ptr(), out.data_ptr(), *extra, _st())
    nat.ohwi_pack(w.data_ptr(), T.segs_d.data_ptr(), T.tile0_d.data_ptr(), T.nseg, T.tiles,
                  wbf.data_ptr(), gstep.data_ptr(), _st())
    torch.cuda.synchronize()
    assert int(gstep) == gstep_v + 1 and int(start) == start_v
    if clip_on:
        assert tuple(clip.tolist()) == tuple(oo.f32(c) for c in CLIP_SLOT)
    return w, m, v, wbf, float(lr_out), out.cpu().tolist()


def _check(T, got, lr, t, coeff, mode, wd_seg, scale, what):
    b1, b2, eps, _, _ = coeff
    w, m, v = got
    w_ref, m_ref, v_ref, Bw, Bm, Bv, _ = ao.adam_reference(T.w0, T.g, T.m0, T.v0, T.seg, wd_seg, lr,
                                                           t, b1, b2, eps, scale, mode)
    worst = []
    for x, ref, B, name in ((w, w_ref, Bw, "w"), (m, m_ref, Bm, "m"), (v, v_ref, Bv, "v")):
        err = (x.double() - ref).abs()
        worst.append(float((err / B.clamp_min(1e-300)).max()))
        bad = (err > B).nonzero().flatten()
        assert bad.numel() == 0, (what, name, bad[:8].tolist(), float(err.max()))
        assert bool(torch.isfinite(x).all()), (what, name)
    print(f"{what} max err/bound: w {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")


def _check_slot(out, lr, t, coeff, what):
    b1, b2 = coeff[:2]
    assert out[0] == lr and out[2] == float(np.float32(t)), (what, out)
    ref = ao.alpha_reference(lr, t, b1, b2)
    assert abs(out[1] - ref) <= ao.ulp(ref), (what, t, out[1], ref, (out[1] - ref) / ao.ulp(ref))


def _check_wbf(seg, w1, wbf, what=""):
    want = oo.expected_wbf(seg, w1, wbf.numel())
    if not torch.equal(wbf, want):
        bad = (wbf != want).nonzero().flatten()
        raise AssertionError((what, "wbf differs at", bad[:8].tolist(), bad.numel()))


def _full(nat, T, sched, gstep_v, t, coeff, mode, skip, clip_on, what):
    wd_seg = T.wd_table(coeff[3], skip)
    w, m, v, wbf, lr, out = _launch(nat, T, sched, gstep_v, gstep_v - t + 1, coeff, mode, wd_seg,
                                    clip_on)
    _check_lr(sched, gstep_v, lr)
    _check_slot(out, lr, t, coeff, what)
    _check(T, (w, m, v), lr, t, coeff, mode, wd_seg, CLIP_SLOT[1] if clip_on else coeff[4], what)
    _check_wbf(T.seg, w, wbf, what)
    return w, m, v, wbf


# ---------------------------------------------------------------- (a) synthetic tables
@pytest.fixture(scope="module")
def table_a(gpu):
    T = Table([s for s, _ in TABLE_A], gpu, seed=31)
    offs = [int(r["offset"]) for r in T.seg]
    assert {o % 4 for o in offs} == {0, 1, 2, 3} and T.n % 4 != 0
    return T


@pytest.mark.parametrize("clip_on", [False, True])
@pytest.mark.parametrize("skip", ["none", "vectors"])
@pytest.mark.parametrize("mode", ["decoupled", "l2"])
@pytest.mark.parametrize("ci", [0, 1])
def test_adam_kernel_against_fp64(gpu, nat, table_a, ci, mode, skip, clip_on):
    T = table_a
    if skip == "vectors":
        tab = T.wd_table(1.0, skip).tolist()
        assert 0.0 in tab and 1.0 in tab
    for sched in (SEVEN, COSINE):
        for t in STEPS:
            # the schedule sees global_step, the bias correction global_step - start + 1:
            # small t inside SEVEN's warm-up and first boundaries, the last past 2^31
            gstep_v = t + 2
            a = _full(nat, T, sched, gstep_v, t, COEFFS[ci], mode, skip, clip_on,
                      f"table A {sched.decay} t={t}")
    b = _full(nat, T, COSINE, STEPS[-1] + 2, STEPS[-1], COEFFS[ci], mode, skip, clip_on, "again")
    for x, y in zip(a, b):   # a second identical launch: bit-equal
        assert torch.equal(x, y)


# ---------------------------------------------------------------- (b) zero-gradient elements
@pytest.mark.parametrize("mode", ["decoupled", "l2"])
def test_adam_zero_gradient_elements_stay_bitwise(gpu, nat, mode):
    zero = {1, 4, 7, 13}   # a conv, a 5-vector, the kpad > K conv, the 10-class dense
    T = Table([s for s, _ in TABLE_A], gpu, seed=32, zero=zero)
    assert int(T.zero_mask.sum()) > 1000
    coeff = (0.9, 0.999, 1e-8, 0.0, 1.0)
    wd_seg = T.wd_table(0.0, "none")
    w, m, v, wbf, lr, out = _launch(nat, T, SEVEN, 12, 0, coeff, mode, wd_seg, False)
    z = T.zero_mask
    assert torch.equal(w[z], T.w0[z])
    assert int(m[z].count_nonzero()) == 0 and int(v[z].count_nonzero()) == 0
    assert not torch.equal(w[~z], T.w0[~z])
    for x in (w, m, v):
        assert bool(torch.isfinite(x).all())
    _check(T, (w, m, v), lr, 13, coeff, mode, wd_seg, 1.0, f"zero blocks {mode}")
    _check_wbf(T.seg, w, wbf)


# ---------------------------------------------------------------- (c) table and grid extremes
def test_adam_long_tables(gpu, nat):
    """More than 640 segments: the update reads the segment table from global memory."""
    specs = []
    for i in range(700):
        k = i % 4
        specs.append(("conv", 1, 1, 4, 8, 4, 8, True, True) if k == 0 else
                     ("conv", 3, 3, 4, 4, 8, 4, True, True) if k == 2 else
                     V(1 + i % 9) if k == 1 else V(1 + i % 5))
    T = Table(specs, gpu, seed=33)
    assert T.nseg == 700
    _full(nat, T, SEVEN, 12, 5, COEFFS[0], "decoupled", "vectors", False, "700 segments")
    _full(nat, T, COSINE, 12, 5, COEFFS[1], "l2", "vectors", True, "700 segments l2")


def test_adam_grid_stride(gpu, nat):
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
    _full(nat, T, cifar_lr_schedule(), 7, 3, COEFFS[1], "decoupled", "vectors", False, "grid-stride")


# ---------------------------------------------------------------- (d) unaligned buffers
def test_adam_rejects_unaligned_buffers_and_bad_coefficients(gpu, nat, table_a):
    T = table_a
    w, m, v, wbf = T.fresh()
    g = T.g.clone()
    gstep = torch.zeros(1, dtype=torch.int64, device=gpu)
    start = torch.zeros(1, dtype=torch.int64, device=gpu)
    wd_d = torch.from_numpy(T.wd_table(0.1, "none")).to(gpu)

    def call(ptrs, b1=0.9, b2=0.999, eps=1e-8, mode="decoupled"):
        nat.adam_update_pack(*ptrs, T.n - 4, *_sa(SEVEN), gstep.data_ptr(), start.data_ptr(), b1,
                             b2, eps, 1.0, 0, mode, T.segs_d.data_ptr(), T.nseg, wd_d.data_ptr(),
                             wbf.data_ptr(), 0, 0, _st())

    base = [w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()]
    for i in range(4):
        ptrs = list(base)
        ptrs[i] += 4
        with pytest.raises(ValueError):
            call(ptrs)
    for kw in (dict(b1=1.0), dict(b2=-0.1), dict(eps=0.0), dict(eps=float("nan")),
               dict(mode="adamw")):
        with pytest.raises(ValueError):
            call(base, **kw)
    torch.cuda.synchronize()
    assert torch.equal(w, T.w0) and torch.equal(m, T.m0) and torch.equal(v, T.v0)
    assert int(wbf.count_nonzero()) == 0


# ---------------------------------------------------------------- (e) engine
WD = 5e-4
ADAM = dict(adam_beta1=0.9, adam_beta2=0.99, adam_epsilon=1e-6)


def _engine(spec, N, gpu, optimizer="adamw", seed=0, **kw):
    kw = {**(ADAM if optimizer == "adamw" else {}), **kw}
    eng = Engine(spec, N, weight_decay=WD, lr_schedule=cifar_lr_schedule(), optimizer=optimizer,
                 device=gpu, input_mode="nhwc", seed=seed, **kw)
    gen = torch.Generator().manual_seed(5)
    imgs = torch.randn(N, spec.image_h, spec.image_w, 3, generator=gen).to(torch.bfloat16).float()
    eng.set_batch(imgs.to(gpu), torch.randint(0, spec.num_classes, (N,), generator=gen).to(gpu))
    return eng


def _check_engine_step(eng, w0, m0, v0, step, t, what):
    """The engine's own gradient through adam_reference against its master, moments and
    adam_state(): the optimizer alone, without the convolutions' bf16 noise."""
    n = eng.params.n_train
    lr = oo.f32(oo.lr_reference(eng.sched, step))
    assert eng.metrics()["lr"] == lr
    scale = 1.0
    if eng.clip_grad_norm > 0:
        norm, scale = eng.clip_state()
        assert scale < 1.0, (norm, scale)
    wd_seg = adam_decay_table([s.shape for s in eng.params.train_slots], eng.wd,
                              eng.adam_decay_skip)
    w_ref, m_ref, v_ref, Bw, Bm, Bv, _ = ao.adam_reference(
        w0, eng.grad, m0, v0, eng.seg_arr, wd_seg, lr, t, eng.adam_beta1, eng.adam_beta2,
        eng.adam_epsilon, scale, eng.adam_decay)
    worst = []
    for x, ref, B, name in ((eng.params.master[:n], w_ref, Bw, "master"), (eng.mom[:n], m_ref, Bm, "m"),
                            (eng.adam_v[:n], v_ref, Bv, "v")):
        err = (x.double() - ref).abs()
        worst.append(float((err / B.clamp_min(1e-300)).max()))
        assert bool((err <= B).all()), (what, step, name, float(err.max()))
    print(f"{what} step {step}: max err/bound master {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
    t_k, alpha = eng.adam_state()
    ref = ao.alpha_reference(lr, t, eng.adam_beta1, eng.adam_beta2)
    assert t_k == t and abs(alpha - ref) <= ao.ulp(ref), (what, t_k, alpha, ref)
    assert eng.metrics()["adam_alpha"] == alpha
    assert torch.equal(eng.wbf, oo.expected_wbf(eng.seg_arr, eng.params.master, eng.wbf.numel()))


def _run_steps(eng, steps, what):
    for step in range(steps):
        w0, m0, v0 = eng.params.master.clone(), eng.mom.clone(), eng.adam_v.clone()
        assert int(eng.gstep.item()) == step
        eng.step()
        torch.cuda.synchronize()
        assert not eng.persist_error()
        _check_engine_step(eng, w0, m0, v0, step, step + 1, what)
    assert int(eng.gstep.item()) == steps


OPT_OPS = ("grad_sqnorm", "clip_scale", "adam_update_pack", "ohwi_pack", "sgd_update_pack",
           "sgd_clip_update_pack", "sgd_tiles", "lars_update_pack")


@pytest.mark.parametrize("clip", [0.0, 0.05])
@pytest.mark.parametrize("persist", [0, 1])
def test_engine_adamw_step(gpu, monkeypatch, persist, clip):
    monkeypatch.setenv("DTR_TUNE", f"persist={persist}")
    eng = _engine(cifar_spec(8), 16, gpu, clip_grad_norm=clip,
                  adam_decay="l2" if clip else "decoupled",
                  adam_decay_skip="vectors" if clip else "none")
    assert eng.persist == bool(persist) and eng.adam
    assert not eng.opt_fused and "adamw" in eng.opt_fused_reason
    names = eng.plan.names()
    a, b = eng.seg["opt"]
    assert [n for n in names[a:b] if n in OPT_OPS] == \
        (["grad_sqnorm", "clip_scale"] if clip else []) + ["adam_update_pack", "ohwi_pack"]
    _run_steps(eng, 2, f"cifar8 persist={persist} clip={clip}")   # step 1: non-zero moments


def test_engine_adamw_imagenet_s2d_stem(gpu, monkeypatch):
    monkeypatch.setenv("DTR_TUNE", "persist=0")
    eng = _engine(imagenet_spec(18, image_hw=64), 8, gpu)
    assert eng.stem_s2d
    _run_steps(eng, 2, "imagenet18 s2d")


@pytest.mark.parametrize("dtype,persist", [("fp32", "0"), ("bf16", "1")])
def test_engine_adamw_takes_the_exchanged_gradient(gpu, monkeypatch, dtype, persist):
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
    w0, m0, v0 = eng.params.master.clone(), eng.mom.clone(), eng.adam_v.clone()
    ref.step()
    eng.step()
    torch.cuda.synchronize()
    base = ref.grad if dtype == "fp32" else ref.grad.to(torch.bfloat16).float()
    assert torch.equal(eng.grad, 2 * base)
    _check_engine_step(eng, w0, m0, v0, 0, 1, f"loopback {dtype}")


def _state(eng):
    return [eng.params.master.clone(), eng.mom.clone(), eng.adam_v.clone(),
            eng.params.stats.clone(), eng.wbf.clone(), eng.gstep.clone(), eng.adam_start.clone()]


def test_engine_adamw_same_seed_engines_agree_bitwise(gpu):
    a, b = _engine(cifar_spec(8), 16, gpu), _engine(cifar_spec(8), 16, gpu)
    for _ in range(5):
        a.step()
        b.step()
    torch.cuda.synchronize()
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    assert a.adam_state() == b.adam_state() and a.adam_state()[0] == 5


def test_engine_adamw_resume_is_bitwise(gpu, tmp_path):
    from distributed_tensorflow_resnet_amd.train.backends import GPUBackend
    from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver

    straight = _engine(cifar_spec(8), 16, gpu)
    for _ in range(4):
        straight.step()
    first = GPUBackend(_engine(cifar_spec(8), 16, gpu))
    first.engine.set_adam_start(0)
    for _ in range(2):
        first.step()
    torch.cuda.synchronize()
    tensors = first.state_tensors()
    assert int(tensors["adam_start_step"]) == 0 and "conv2d/kernel/Adam_1" in tensors
    assert not any(k.endswith("/Momentum") for k in tensors)
    prefix = Saver(str(tmp_path)).save(tensors, 2)
    second = GPUBackend(_engine(cifar_spec(8), 16, gpu, seed=9))
    second.engine.set_adam_start(99)    # overwritten by the restore
    second.load_state(Saver.restore(prefix))
    assert second.global_step == 2 and int(second.engine.adam_start.item()) == 0
    for _ in range(2):
        second.step()
    torch.cuda.synchronize()
    for x, y in zip(_state(straight), _state(second.engine)):
        assert torch.equal(x, y)
    assert second.adam_state() == straight.adam_state()


def test_engine_adamw_restores_a_mom_checkpoint(gpu):
    from distributed_tensorflow_resnet_amd.train.backends import GPUBackend

    mom = GPUBackend(_engine(cifar_spec(8), 16, gpu, optimizer="mom"))
    for _ in range(3):
        mom.step()
    torch.cuda.synchronize()
    assert float(mom.engine.mom.abs().max()) > 0
    be = GPUBackend(_engine(cifar_spec(8), 16, gpu, seed=9))
    be.step()                                   # non-zero moments to be cleared
    be.load_state(mom.state_tensors())
    eng = be.engine
    assert be.global_step == 3 and int(eng.adam_start.item()) == 3 and int(eng.gstep.item()) == 3
    assert int(eng.mom.count_nonzero()) == 0 and int(eng.adam_v.count_nonzero()) == 0
    assert torch.equal(eng.params.master, mom.engine.params.master)
    w0, m0, v0 = eng.params.master.clone(), eng.mom.clone(), eng.adam_v.clone()
    be.step()
    torch.cuda.synchronize()
    _check_engine_step(eng, w0, m0, v0, 3, 1, "after a mom checkpoint")   # t = 1 at step 3


def test_engine_adamw_graph_replay_equals_eager(gpu):
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
    assert graph.adam_state() == eager.adam_state() and graph.adam_state()[0] == 6


# ---------------------------------------------------------------- (f) a mom engine is unchanged
def test_mom_engine_is_unchanged(gpu, monkeypatch):
    monkeypatch.setenv("DTR_TUNE", "persist=1")
    eng = _engine(cifar_spec(8), 16, gpu, optimizer="mom")
    other = _engine(cifar_spec(8), 16, gpu, optimizer="mom", adam_beta1=0.5, adam_decay="l2")
    assert not eng.adam and eng.adam_state() is None
    assert eng.adam_v is None and eng.adam_start is None and eng.adam_out is None
    assert eng.opt_fused and eng.opt_fused_reason == "" and eng.persist
    assert eng.plan.names() == other.plan.names() and "adam_update_pack" not in eng.plan.names()
    eng.step()
    torch.cuda.synchronize()
    assert eng.adam_state() is None and "adam_alpha" not in eng.metrics()
    with pytest.raises(ValueError):
        _engine(cifar_spec(8), 16, gpu, optimizer="adamw", adam_epsilon=0.0)
    with pytest.raises(ValueError):
        _engine(cifar_spec(8), 16, gpu, optimizer="adamw", adam_beta2=1.0)
