"""The RMSProp kernel (csrc/rmsprop.hip rmsprop_update_pack) launched directly on synthetic
parameter tables, and the engine's rmsprop optimizer on every plan, against the fp64 reference
and the derived bounds of tests/rmsprop_oracle.py.  The synthetic data (rmsprop_inputs) keeps
the centered denominator well conditioned, ms' >= 4 mg'^2, which every centered test first
asserts on the oracle alone; every element is held to its bound."""
import numpy as np
import pytest
import torch

import optim_oracle as oo
import rmsprop_oracle as rmo
from test_adam_gpu import CLIP_SLOT, COSINE, _check_lr, _check_wbf, _sa, _st
from test_lamb_gpu import _recorded_calls
from test_lars_gpu import SEVEN, TABLE_A, V
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule
from distributed_tensorflow_resnet_amd.train.layout import (OPT_FUSED_RMSPROP_REASON,
                                                              adam_decay_table)

pytestmark = pytest.mark.gpu

# rho, momentum, epsilon, wd, grad_scale: slim's momentum with TF's epsilon, and TF's momentum
COEFFS = {0.9: (0.9, 0.9, 1e-10, 0.05, 1.0), 0.0: (0.5, 0.0, 1e-3, 0.3, 0.5)}
# (schedule, step): step 0, SEVEN's warm-up, past it, past 2^31; the device-evaluated cosine
RATES = [(SEVEN, 0), (SEVEN, 3), (SEVEN, 12), (SEVEN, 2 ** 31 + 7), (COSINE, 12),
         (COSINE, 2 ** 31 + 7)]


@pytest.fixture(scope="module")
def nat(gpu):
    import distributed_tensorflow_resnet_amd as dtr

    return dtr.native(required=True)


class Table:
    """A synthetic table with rmsprop_oracle.rmsprop_inputs' data; the segments in `zero` have
    g = mom = 0, the elements in `nan` a NaN gradient."""

    def __init__(self, specs, gpu, seed, zero=(), nan=()):
        (self.seg, self.names, self.n, self.bf_total, tile0, self.tiles) = oo.build_seg_table(specs)
        self.gpu, self.nseg = gpu, len(self.seg)
        self.shapes = [(1,) if s[0] == "vec" else (s[1], s[2], s[3], s[4]) for s in specs]
        self.segs_d = torch.from_numpy(self.seg.view(np.uint8).copy()).to(gpu)
        self.tile0_d = torch.from_numpy(tile0).to(gpu)
        w, g, ms, mg, mom = rmo.rmsprop_inputs(self.n, seed)
        self.zero_mask = torch.zeros(self.n, dtype=torch.bool)
        for i in zero:
            o, k = int(self.seg[i]["offset"]), int(self.seg[i]["numel"])
            self.zero_mask[o:o + k] = True
        g[self.zero_mask] = 0.0
        mom[self.zero_mask] = 0.0
        for e in nan:
            g[e] = float("nan")
        self.w0, self.g, self.ms0, self.mg0, self.mom0 = (t.to(gpu) for t in (w, g, ms, mg, mom))
        self.zero_mask = self.zero_mask.to(gpu)

    def wd_table(self, wd, skip):
        return adam_decay_table(self.shapes, wd, skip)

    def fresh(self):
        return (self.w0.clone(), self.ms0.clone(), self.mg0.clone(), self.mom0.clone(),
                torch.zeros(self.bf_total, dtype=torch.bfloat16, device=self.gpu))


def _launch(nat, T, sched, gstep_v, coeff, centered, mode, wd_seg, clip_on, mg_ptr=None):
    """rmsprop_update_pack + ohwi_pack on fresh buffers; returns (w, ms, mg, mom, wbf, lr).
    mg_ptr: the pointer handed in for mg instead of the fresh copy's."""
    rho, mo, eps, _, gs = coeff
    gpu = T.gpu
    w, ms, mg, mom, wbf = T.fresh()
    gstep = torch.tensor([gstep_v], dtype=torch.int64, device=gpu)
    lr_out = torch.full((1,), 7.0, device=gpu)
    clip = torch.tensor(CLIP_SLOT, device=gpu) if clip_on else None
    wd_d = torch.from_numpy(wd_seg).to(gpu)
    extra = () if sched.decay == "piecewise" else (sched.decay_args(),)
    # (with a clip slot the host grad_scale must be ignored: a wrong one is handed in)
    nat.rmsprop_update_pack(w.data_ptr(), T.g.data_ptr(), ms.data_ptr(),
                            mg.data_ptr() if mg_ptr is None else mg_ptr, mom.data_ptr(), T.n,
                            *_sa(sched), gstep.data_ptr(), rho, mo, eps, 55.0 if clip_on else gs,
                            clip.data_ptr() if clip_on else 0, int(centered), mode,
                            T.segs_d.data_ptr(), T.nseg, wd_d.data_ptr(), wbf.data_ptr(),
                            lr_out.data_ptr(), *extra, _st())
    nat.ohwi_pack(w.data_ptr(), T.segs_d.data_ptr(), T.tile0_d.data_ptr(), T.nseg, T.tiles,
                  wbf.data_ptr(), gstep.data_ptr(), _st())
    torch.cuda.synchronize()
    assert int(gstep) == gstep_v + 1
    if clip_on:
        assert tuple(clip.tolist()) == tuple(oo.f32(c) for c in CLIP_SLOT)
    return w, ms, mg, mom, wbf, float(lr_out)


def _reference(T, lr, coeff, centered, mode, wd_seg, scale):
    rho, mo, eps, _, _ = coeff
    return rmo.rmsprop_reference(T.w0, T.g, T.ms0, T.mg0, T.mom0, T.seg, wd_seg, lr, rho, mo, eps,
                                 scale, centered, mode)


def _full(nat, T, sched, gstep_v, coeff, centered, mode, skip, clip_on, what):
    """One launch against the oracle: lr_out, then w', ms', mg', mom' each within its bound
    and the bf16 copy equal to the rounding of the kernel's own w'."""
    wd_seg = T.wd_table(coeff[3], skip)
    scale = CLIP_SLOT[1] if clip_on else coeff[4]
    w, ms, mg, mom, wbf, lr = _launch(nat, T, sched, gstep_v, coeff, centered, mode, wd_seg,
                                      clip_on)
    _check_lr(sched, gstep_v, lr)
    ref = _reference(T, lr, coeff, centered, mode, wd_seg, scale)
    if centered:
        rmo.assert_conditioned(ref, what)
    else:
        assert torch.equal(mg, T.mg0), (what, "the plain kernel wrote mg")
    worst = rmo.check(w, ms, mg, mom, ref, what)
    print(f"{what} max err/bound: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    _check_wbf(T.seg, w, wbf, what)
    return w, ms, mg, mom, wbf


# ---------------------------------------------------------------- (a) synthetic tables
@pytest.fixture(scope="module")
def table_a(gpu):
    """Segments of 1, 3 and 5 elements, a 10-element bias whose float4 straddles a segment end,
    offsets off the multiples of 4, a padded-K bf16 copy, tensors without a copy, a last
    segment ending off a 16-byte boundary; 2e4 elements."""
    T = Table([s for s, _ in TABLE_A], gpu, seed=41)
    offs = [int(r["offset"]) for r in T.seg]
    assert {o % 4 for o in offs} == {0, 1, 2, 3} and T.n % 4 != 0
    assert {1, 3, 5, 10} <= {int(r["numel"]) for r in T.seg}
    assert any(int(r["numel"]) == 10 and int(r["offset"]) % 4 for r in T.seg)
    assert any(int(r["kpad"]) != int(r["K"]) and r["bf_hwio"] >= 0 for r in T.seg)
    assert any(r["bf_hwio"] < 0 for r in T.seg)
    return T


@pytest.mark.parametrize("mo", [0.0, 0.9])
@pytest.mark.parametrize("clip_on", [False, True])
@pytest.mark.parametrize("skip", ["none", "vectors"])
@pytest.mark.parametrize("mode", ["l2", "decoupled"])
@pytest.mark.parametrize("centered", [False, True])
def test_rmsprop_kernel_against_fp64(gpu, nat, table_a, centered, mode, skip, clip_on, mo):
    T = table_a
    if skip == "vectors":
        tab = T.wd_table(1.0, skip).tolist()
        assert 0.0 in tab and 1.0 in tab
    for sched, gstep_v in RATES:
        a = _full(nat, T, sched, gstep_v, COEFFS[mo], centered, mode, skip, clip_on,
                  f"table A {sched.decay} step={gstep_v}")
    b = _full(nat, T, *RATES[-1], COEFFS[mo], centered, mode, skip, clip_on, "again")
    for x, y in zip(a, b):   # a second identical launch: bit-equal
        assert torch.equal(x, y)


# ---------------------------------------------------------------- (b) exact cases
@pytest.mark.parametrize("mode", ["l2", "decoupled"])
@pytest.mark.parametrize("centered", [False, True])
def test_rmsprop_zero_elements_are_exact(gpu, nat, centered, mode):
    """g = 0, mom = 0, wd = 0: w and mom bit for bit unchanged, ms' (and mg') the single
    rounding of rho * ms (rho * mg)."""
    zero = {1, 4, 7, 13}   # a conv, a 5-vector, the kpad > K conv, the 10-class dense
    T = Table([s for s, _ in TABLE_A], gpu, seed=42, zero=zero)
    assert int(T.zero_mask.sum()) > 1000
    coeff = (0.9, 0.9, 1e-10, 0.0, 1.0)
    wd_seg = T.wd_table(0.0, "none")
    w, ms, mg, mom, wbf, lr = _launch(nat, T, SEVEN, 12, coeff, centered, mode, wd_seg, False)
    z = T.zero_mask
    rho = torch.tensor(0.9, device=gpu)
    assert rho.dtype == torch.float32
    assert torch.equal(w[z], T.w0[z]) and int(mom[z].count_nonzero()) == 0   # bit for bit
    assert torch.equal(ms[z], rho * T.ms0[z]) and not torch.equal(ms[z], T.ms0[z])
    if centered:
        assert torch.equal(mg[z], rho * T.mg0[z])
    assert not bool((w[~z] == T.w0[~z]).all()) and int(mom[~z].count_nonzero()) > 0
    ref = _reference(T, lr, coeff, centered, mode, wd_seg, 1.0)
    rmo.check(w, ms, mg, mom, ref, "zero blocks")
    _check_wbf(T.seg, w, wbf)


@pytest.mark.parametrize("mode", ["l2", "decoupled"])
@pytest.mark.parametrize("centered", [False, True])
def test_rmsprop_without_momentum_is_the_quotient_bit_for_bit(gpu, nat, table_a, centered, mode):
    """momentum = 0: mom' is (lr * g') / sqrt(d), evaluated here in fp32 torch on the host
    (correctly rounded products, sums, square root and quotient, each on its own) from the
    kernel's own ms' and mg', and w' is w - mom' (- (lr wd) w)."""
    T = table_a
    rho, _, eps, wd, _ = coeff = (0.9, 0.0, 1e-3, 0.25, 1.0)
    wd_seg = T.wd_table(wd, "none")
    w, ms, mg, mom, wbf, lr = _launch(nat, T, SEVEN, 12, coeff, centered, mode, wd_seg, False)
    f = lambda x: torch.tensor(x, dtype=torch.float32)   # noqa: E731
    w0, g = T.w0.cpu(), T.g.cpu()
    gp = g + f(wd) * w0 if mode == "l2" else g           # (s = 1: s * g is g)
    d = ms.cpu()
    if centered:
        d = d - mg.cpu() * mg.cpu()
    d = d + f(eps)
    # the correctly rounded fp32 root, whichever vector sqrt the torch build uses: the fp64
    # root rounded once more (innocuous for a square root when the wide format has at least
    # 2 * 24 + 2 bits; tests/test_rmsprop_cpu.py checks this route against numpy's fp32 sqrt)
    root = d.double().sqrt().float()
    q = (f(lr) * gp) / root
    assert q.dtype == torch.float32 and int(q.count_nonzero()) > T.n // 2
    assert torch.equal(mom.cpu(), q)
    wn = w0 - q
    if mode == "decoupled":
        wn = wn - (f(lr) * f(wd)) * w0
    assert torch.equal(w.cpu(), wn)
    # and ms' itself from the same g'
    assert torch.equal(ms.cpu(), f(rho) * T.ms0.cpu() + f(1.0 - float(f(rho))) * (gp * gp))


@pytest.mark.parametrize("clip_on", [False, True])
def test_plain_rmsprop_never_touches_mg(gpu, nat, table_a, clip_on):
    """The plain kernel's outputs depend neither on the contents of mg nor on whether there is
    one: a null pointer, the table's mg and a buffer of NaNs give the same bits, and the
    buffers handed in are left as they were."""
    T = table_a
    coeff = COEFFS[0.9]
    wd_seg = T.wd_table(coeff[3], "none")
    poison = torch.full((T.n,), float("nan"), device=gpu)
    runs = [_launch(nat, T, SEVEN, 12, coeff, False, "l2", wd_seg, clip_on, mg_ptr=p)
            for p in (None, 0, poison.data_ptr())]
    assert bool(torch.isnan(poison).all())
    for r in runs:
        assert torch.equal(r[2], T.mg0)
    for r in runs[1:]:
        for i in (0, 1, 3, 4):
            assert torch.equal(r[i], runs[0][i])
    assert bool(torch.isfinite(runs[0][0]).all())


@pytest.mark.parametrize("centered", [False, True])
def test_rmsprop_nan_gradient_stays_in_its_element(gpu, nat, centered):
    specs = [s for s, _ in TABLE_A]
    seg = oo.build_seg_table(specs)[0]
    # inside a float4 of a conv, in the straddling 10-vector, the last element (the tail)
    n = int(seg[-1]["offset"] + seg[-1]["numel"])
    nan = [int(seg[3]["offset"]) + 6, int(seg[8]["offset"]) + 3, n - 1]
    T = Table(specs, gpu, seed=45, nan=nan)
    coeff = COEFFS[0.9]
    wd_seg = T.wd_table(coeff[3], "none")
    w, ms, mg, mom, wbf, lr = _launch(nat, T, SEVEN, 12, coeff, centered, "l2", wd_seg, False)
    want = torch.zeros(T.n, dtype=torch.bool, device=gpu)
    want[nan] = True
    for x in (w, ms, mom) + ((mg,) if centered else ()):
        assert torch.equal(torch.isnan(x), want)
    ref = _reference(T, lr, coeff, centered, "l2", wd_seg, 1.0)
    if centered:
        rmo.assert_conditioned(ref)
    rmo.check(w, ms, mg, mom, ref, "NaN gradient")


# ---------------------------------------------------------------- (c) table and grid extremes
def test_rmsprop_long_tables(gpu, nat):
    """More than 640 segments: the update reads the segment table from global memory."""
    specs = []
    for i in range(700):
        k = i % 4
        specs.append(("conv", 1, 1, 4, 8, 4, 8, True, True) if k == 0 else
                     ("conv", 3, 3, 4, 4, 8, 4, True, True) if k == 2 else
                     V(1 + i % 9) if k == 1 else V(1 + i % 5))
    T = Table(specs, gpu, seed=43)
    assert T.nseg == 700
    _full(nat, T, SEVEN, 12, COEFFS[0.9], False, "l2", "vectors", False, "700 segments")
    _full(nat, T, COSINE, 12, COEFFS[0.0], True, "decoupled", "vectors", True,
          "700 segments centered clip")


def test_rmsprop_grid_stride(gpu, nat):
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
    T = Table(specs, gpu, seed=44)
    assert T.n == n and (n + 3) // 4 > 4096 * 256
    _full(nat, T, cifar_lr_schedule(), 7, COEFFS[0.0], True, "l2", "vectors", False,
          "grid-stride centered")
    _full(nat, T, cifar_lr_schedule(), 7, COEFFS[0.9], False, "decoupled", "none", False,
          "grid-stride plain")


# ---------------------------------------------------------------- (d) the binding
def test_rmsprop_rejects_unaligned_buffers_and_bad_coefficients(gpu, nat, table_a):
    T = table_a
    w, ms, mg, mom, wbf = T.fresh()
    g = T.g.clone()
    gstep = torch.zeros(1, dtype=torch.int64, device=gpu)
    wd_d = torch.from_numpy(T.wd_table(0.1, "none")).to(gpu)

    def call(ptrs, rho=0.9, mo=0.9, eps=1e-10, centered=1, mode="l2"):
        nat.rmsprop_update_pack(*ptrs, T.n - 4, *_sa(SEVEN), gstep.data_ptr(), rho, mo, eps, 1.0,
                                0, centered, mode, T.segs_d.data_ptr(), T.nseg, wd_d.data_ptr(),
                                wbf.data_ptr(), 0, _st())

    base = [w.data_ptr(), g.data_ptr(), ms.data_ptr(), mg.data_ptr(), mom.data_ptr()]
    for i in range(5):
        ptrs = list(base)
        ptrs[i] += 4
        with pytest.raises(ValueError):
            call(ptrs)
        if i != 3:   # (plain never touches mg)
            with pytest.raises(ValueError):
                call(ptrs, centered=0)
    for kw in (dict(rho=1.0), dict(rho=-0.1), dict(rho=float("nan")), dict(mo=1.0), dict(mo=1.5),
               dict(mo=-0.5), dict(mo=float("nan")), dict(eps=0.0), dict(eps=-1e-10),
               dict(eps=float("nan")), dict(eps=float("inf")), dict(mode="none")):
        for centered in (0, 1):
            with pytest.raises(ValueError):
                call(base, centered=centered, **kw)
    nomg = list(base)
    nomg[3] = 0
    with pytest.raises(ValueError):
        call(nomg)                        # centered without mg
    for i in (0, 1, 2, 4):
        ptrs = list(base)
        ptrs[i] = 0
        with pytest.raises(ValueError):
            call(ptrs, centered=0)
    torch.cuda.synchronize()
    assert torch.equal(w, T.w0) and torch.equal(ms, T.ms0) and torch.equal(mg, T.mg0)
    assert torch.equal(mom, T.mom0) and int(wbf.count_nonzero()) == 0


# ---------------------------------------------------------------- (e) engine
WD = 5e-4
N = 8
RMS = dict(rmsprop_rho=0.9, rmsprop_momentum=0.9, rmsprop_epsilon=1e-10)


def _engine(spec, gpu, optimizer="rmsprop", seed=0, n=N, **kw):
    kw = {**(RMS if optimizer == "rmsprop" else {}), **kw}
    eng = Engine(spec, n, weight_decay=WD, lr_schedule=cifar_lr_schedule(), optimizer=optimizer,
                 device=gpu, input_mode="nhwc", seed=seed, **kw)
    gen = torch.Generator().manual_seed(5)
    imgs = torch.randn(n, spec.image_h, spec.image_w, 3, generator=gen).to(torch.bfloat16).float()
    eng.set_batch(imgs.to(gpu), torch.randint(0, spec.num_classes, (n,), generator=gen).to(gpu))
    return eng


def _rms_state(eng):
    st = eng.rmsprop_state()
    return st["ms"].clone(), (st["mg"].clone() if eng.rmsprop_centered else None), eng.mom.clone()


def _check_engine_step(eng, w0, state0, step, what):
    """The engine's own gradient through rmsprop_reference against its master and state: the
    optimizer alone, without the convolutions' bf16 noise."""
    n = eng.params.n_train
    lr = oo.f32(oo.lr_reference(eng.sched, step))
    assert eng.metrics()["lr"] == lr
    scale = 1.0
    if eng.clip_grad_norm > 0:
        norm, scale = eng.clip_state()
        assert scale < 1.0, (norm, scale)
    wd_seg = adam_decay_table([s.shape for s in eng.params.train_slots], eng.wd,
                              eng.rmsprop_decay_skip)
    ms0, mg0, mom0 = state0
    ref = rmo.rmsprop_reference(w0, eng.grad, ms0, mg0, mom0, eng.seg_arr, wd_seg, lr,
                                eng.rmsprop_rho, eng.rmsprop_momentum, eng.rmsprop_epsilon, scale,
                                eng.rmsprop_centered, eng.rmsprop_wd)
    if eng.rmsprop_centered:
        rmo.assert_conditioned(ref, what)
    ms, mg, mom = _rms_state(eng)
    worst = rmo.check(eng.params.master[:n], ms, mg, mom, ref, f"{what} step {step}")
    print(f"{what} step {step}: max err/bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert eng.adam_state() is None and eng.lamb_state() is None
    m = eng.metrics()
    assert m["optimizer"] == "rmsprop" and "adam_alpha" not in m
    assert torch.equal(eng.wbf, oo.expected_wbf(eng.seg_arr, eng.params.master, eng.wbf.numel()))


def _run_steps(eng, steps, what):
    for step in range(steps):
        w0, state0 = eng.params.master.clone(), _rms_state(eng)
        assert int(eng.gstep.item()) == step
        eng.step()
        torch.cuda.synchronize()
        assert not eng.persist_error()
        _check_engine_step(eng, w0, state0, step, what)
    assert int(eng.gstep.item()) == steps


OPT_OPS = ("grad_sqnorm", "clip_scale", "rmsprop_update_pack", "lion_update_pack",
           "adam_update_pack", "ohwi_pack", "sgd_update_pack", "sgd_clip_update_pack", "sgd_tiles",
           "lars_update_pack", "lamb_update_pack", "ema_update")


@pytest.mark.parametrize("clip", [0.0, 0.05])
@pytest.mark.parametrize("persist", [0, 1])
@pytest.mark.parametrize("centered", [False, True])
def test_engine_rmsprop_step(gpu, monkeypatch, centered, persist, clip):
    monkeypatch.setenv("DTR_TUNE", f"persist={persist}")
    eng = _engine(cifar_spec(8), gpu, clip_grad_norm=clip, rmsprop_centered=centered,
                  rmsprop_wd="decoupled" if clip else "l2",
                  rmsprop_decay_skip="vectors" if clip else "none",
                  ema_decay=0.99 if clip else 0.0)
    assert eng.persist == bool(persist) and eng.rmsprop and not eng.adam and not eng.lion
    assert not eng.opt_fused and eng.opt_fused_reason == OPT_FUSED_RMSPROP_REASON
    assert "rmsprop" in eng.opt_fused_reason
    assert eng.adam_v is None and eng.adam_out is None and eng.lion_wd is None
    st = eng.rmsprop_state()
    assert {k: st[k] for k in ("rho", "momentum", "epsilon", "centered")} == \
        {"rho": 0.9, "momentum": 0.9, "epsilon": 1e-10, "centered": centered}
    assert set(st) == {"rho", "momentum", "epsilon", "centered", "ms"} | ({"mg"} if centered
                                                                          else set())
    n = eng.params.n_train
    assert st["ms"].shape == (n,) and torch.equal(st["ms"], torch.ones(n, device=gpu))  # TF: ones
    assert (eng.rms_mg is None) == (not centered)
    assert int(eng.mom.count_nonzero()) == 0 and (not centered or int(st["mg"].count_nonzero()) == 0)
    names = eng.plan.names()
    a, b = eng.seg["opt"]
    assert [x for x in names[a:b] if x in OPT_OPS] == \
        (["grad_sqnorm", "clip_scale"] if clip else []) + ["rmsprop_update_pack", "ohwi_pack"] + \
        (["ema_update"] if clip else [])                   # the EMA op stays last
    assert not any(x in ("sgd_update_pack", "sgd_clip_update_pack", "sgd_tiles") for x in names)
    _run_steps(eng, 2, f"cifar8 centered={centered} persist={persist} clip={clip}")


@pytest.mark.parametrize("centered", [False, True])
def test_engine_rmsprop_imagenet_s2d_stem(gpu, monkeypatch, centered):
    monkeypatch.setenv("DTR_TUNE", "persist=0")
    eng = _engine(imagenet_spec(18, image_hw=64), gpu, rmsprop_centered=centered)
    assert eng.stem_s2d
    _run_steps(eng, 1, f"imagenet18 s2d centered={centered}")


@pytest.mark.parametrize("dtype,persist", [("fp32", "0"), ("bf16", "1")])
def test_engine_rmsprop_takes_the_exchanged_gradient(gpu, monkeypatch, dtype, persist):
    """comm = the doubling loopback (the overlap plans): the update is formed from the
    all-reduced gradient (2x the local one; bf16: rebuilt from the bf16 exchange)."""
    import distributed_tensorflow_resnet_amd as dtr

    monkeypatch.setenv("DTR_TUNE", f"persist={persist}")
    spec = cifar_spec(8)
    ref = _engine(spec, gpu, optimizer="mom")
    eng = _engine(spec, gpu, comm=dtr.native().Comm.loopback(2.0), bucket_mb=0.05,
                  allreduce_dtype=dtype, rmsprop_centered=True)
    assert eng.persist == (persist == "1") and not eng.opt_fused
    assert "rmsprop_update_pack" in eng.plan.names()
    assert torch.equal(eng.params.master, ref.params.master)
    w0, state0 = eng.params.master.clone(), _rms_state(eng)
    ref.step()
    eng.step()
    torch.cuda.synchronize()
    base = ref.grad if dtype == "fp32" else ref.grad.to(torch.bfloat16).float()
    assert torch.equal(eng.grad, 2 * base)
    _check_engine_step(eng, w0, state0, 0, f"loopback {dtype}")


def _state(eng):
    return [eng.params.master.clone(), eng.mom.clone(), eng.rms_ms.clone(),
            eng.params.stats.clone(), eng.wbf.clone(), eng.gstep.clone()] + \
        ([eng.rms_mg.clone()] if eng.rmsprop_centered else [])


@pytest.mark.parametrize("centered", [False, True])
def test_engine_rmsprop_same_seed_engines_agree_bitwise(gpu, centered):
    a = _engine(cifar_spec(8), gpu, rmsprop_centered=centered)
    b = _engine(cifar_spec(8), gpu, rmsprop_centered=centered)
    for _ in range(3):
        a.step()
        b.step()
    torch.cuda.synchronize()
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    assert int(a.gstep.item()) == 3 and float(a.mom.abs().max()) > 0
    assert bool(torch.isfinite(a.params.master).all())


@pytest.mark.parametrize("centered", [False, True])
def test_engine_rmsprop_resume_is_bitwise(gpu, tmp_path, centered):
    from distributed_tensorflow_resnet_amd.train.backends import GPUBackend
    from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver

    kw = dict(rmsprop_centered=centered)
    straight = _engine(cifar_spec(8), gpu, **kw)
    for _ in range(6):
        straight.step()
    first = GPUBackend(_engine(cifar_spec(8), gpu, **kw))
    for _ in range(3):
        first.step()
    torch.cuda.synchronize()
    tensors = first.state_tensors()
    slots = ("/RMSProp", "/RMSProp_1", "/RMSProp_2")
    for i, s in enumerate(slots):
        assert (("conv2d/kernel" + s) in tensors) == (i < 2 or centered)
    assert not any(k.endswith(("/Momentum", "/Adam", "/Adam_1", "/Lion")) for k in tensors)
    assert "adam_start_step" not in tensors and "beta1_power" not in tensors
    prefix = Saver(str(tmp_path)).save(tensors, 3)
    second = GPUBackend(_engine(cifar_spec(8), gpu, seed=9, **kw))
    second.load_state(Saver.restore(prefix))
    assert second.global_step == 3
    assert torch.equal(second.engine.rms_ms, first.engine.rms_ms)
    for _ in range(3):
        second.step()
    torch.cuda.synchronize()
    for x, y in zip(_state(straight), _state(second.engine)):
        assert torch.equal(x, y)


def test_engine_rmsprop_restores_a_mom_checkpoint(gpu, capsys):
    from distributed_tensorflow_resnet_amd.train.backends import GPUBackend

    mom = GPUBackend(_engine(cifar_spec(8), gpu, optimizer="mom"))
    for _ in range(3):
        mom.step()
    torch.cuda.synchronize()
    assert float(mom.engine.mom.abs().max()) > 0
    be = GPUBackend(_engine(cifar_spec(8), gpu, seed=9, rmsprop_centered=True))
    be.step()                                   # a state to be reset
    capsys.readouterr()
    be.load_state(mom.state_tensors())
    assert capsys.readouterr().out.count("no RMSProp slots") == 1
    eng = be.engine
    assert be.global_step == 3 and int(eng.gstep.item()) == 3
    assert torch.equal(eng.rms_ms, torch.ones_like(eng.rms_ms))
    assert int(eng.mom.count_nonzero()) == 0 and int(eng.rms_mg.count_nonzero()) == 0
    assert torch.equal(eng.params.master, mom.engine.params.master)
    w0, state0 = eng.params.master.clone(), _rms_state(eng)
    be.step()
    torch.cuda.synchronize()
    _check_engine_step(eng, w0, state0, 3, "after a mom checkpoint")
    # and back: a mom run restoring the rmsprop checkpoint keeps its own (zero) momentum
    back = GPUBackend(_engine(cifar_spec(8), gpu, optimizer="mom", seed=5))
    back.load_state(be.state_tensors())
    assert back.global_step == 4 and int(back.engine.mom.count_nonzero()) == 0


@pytest.mark.parametrize("centered", [False, True])
def test_engine_rmsprop_refuses_the_other_form(gpu, centered):
    from distributed_tensorflow_resnet_amd.train.backends import GPUBackend

    src = GPUBackend(_engine(cifar_spec(8), gpu, rmsprop_centered=centered))
    src.step()
    torch.cuda.synchronize()
    be = GPUBackend(_engine(cifar_spec(8), gpu, seed=9, rmsprop_centered=not centered))
    before = _state(be.engine)
    with pytest.raises(ValueError, match="centered.*plain|plain.*centered"):
        be.load_state(src.state_tensors())
    for x, y in zip(before, _state(be.engine)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("centered", [False, True])
def test_engine_rmsprop_graph_replay_equals_eager(gpu, centered):
    spec = cifar_spec(8)
    eager = _engine(spec, gpu, use_graph=True, rmsprop_centered=centered)   # the same recording,
    graph = _engine(spec, gpu, use_graph=True, rmsprop_centered=centered)   # eager / replayed
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
def _device_tensors(eng):
    """{attribute: (dtype, bytes)} of every device tensor the engine holds, lists and dicts of
    tensors included."""
    out = {}

    def walk(key, v):
        if torch.is_tensor(v):
            if v.is_cuda:
                out[key] = (str(v.dtype), v.numel() * v.element_size())
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk(f"{key}[{i}]", x)
        elif isinstance(v, dict):
            for k, x in v.items():
                walk(f"{key}[{k!r}]", x)

    for k, v in vars(eng).items():
        walk(k, v)
    walk("params.master", eng.params.master)
    walk("params.stats", eng.params.stats)
    return out


@pytest.mark.parametrize("optimizer,persist,opt_ops", [
    ("mom", 1, ["sgd_tiles"]), ("mom", 0, ["sgd_update_pack", "ohwi_pack"]),
    ("adamw", 1, ["adam_update_pack", "ohwi_pack"]),
    ("adamw", 0, ["adam_update_pack", "ohwi_pack"]),
    ("lion", 1, ["lion_update_pack", "ohwi_pack"]), ("lion", 0, ["lion_update_pack", "ohwi_pack"])])
def test_other_optimizers_unchanged(gpu, monkeypatch, optimizer, persist, opt_ops):
    """The rmsprop flags reach no plan but rmsprop's: with them at other values a mom, an adamw
    and a lion engine record the same ops with the same arguments and hold the same device
    buffers as with the defaults, no ms / mg buffer exists, and the optimizer segment is the one they
    have always recorded."""
    monkeypatch.setenv("DTR_TUNE", f"persist={persist}")
    base, ops0, grown0 = _recorded_calls(gpu, monkeypatch, optimizer=optimizer, trust="off")
    other, ops1, grown1 = _recorded_calls(gpu, monkeypatch, optimizer=optimizer, trust="off",
                                          rmsprop_rho=0.5, rmsprop_momentum=0.25,
                                          rmsprop_epsilon=1.0, rmsprop_centered=True,
                                          rmsprop_wd="decoupled", rmsprop_decay_skip="vectors")
    assert len(ops0) > 10 and ops1 == ops0
    # the same device buffers, name for name and byte for byte (the allocator's own figure
    # `grown` also counts blocks of earlier engines whose release is still pending on a side
    # stream when it is read, so it depends on what ran before and is not compared)
    assert _device_tensors(base) == _device_tensors(other)
    for eng in (base, other):
        assert not eng.rmsprop and eng.persist == bool(persist)
        assert eng.rms_ms is None and eng.rms_mg is None and eng.rmsprop_wd_seg is None
        assert eng.rmsprop_state() is None
        names = eng.plan.names()
        assert "rmsprop_update_pack" not in names and "rmsprop" not in eng.opt_fused_reason
        a, b = eng.seg["opt"]
        assert [x for x in names[a:b] if x in OPT_OPS] == opt_ops
    base.step()
    torch.cuda.synchronize()
    assert base.metrics().get("optimizer") in (None, "lion")
    with pytest.raises(ValueError):
        _engine(cifar_spec(8), gpu, rmsprop_rho=1.0)
    with pytest.raises(ValueError):
        _engine(cifar_spec(8), gpu, rmsprop_epsilon=0.0)
    with pytest.raises(ValueError):
        _engine(cifar_spec(8), gpu, adam_trust="on")
