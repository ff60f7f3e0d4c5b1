"""Global gradient-norm clipping on the device (csrc/clip.hip: grad_sqnorm, clip_scale,
sgd_clip_update_pack) launched directly, and the engine's clip_grad_norm on both plans,
against the fp64 reference and the derived bounds of tests/clip_oracle.py.  Every other
chunk is scaled by 1000 and the floats behind the gradient are inf, so an element read from
the wrong place or from past the end breaks a partial."""
import math

import numpy as np
import pytest
import torch

import clip_oracle as co
import optim_oracle as oo
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.train.engine import (Engine, LRSchedule,
                                                              cifar_lr_schedule)

pytestmark = pytest.mark.gpu

CHUNK = co.CHUNK
LENGTHS = [1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 5, 65 * 4096 + 1]
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def nat(gpu):
    import distributed_tensorflow_resnet_amd as dtr

    n = dtr.native(required=True)
    assert n.CLIP_CHUNK == CHUNK
    return n


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gradient(n, gpu, seed):
    """randn over [0, n), every other chunk x 1000, 8 floats of inf behind it."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.full((n + 8,), INF)
    g[:n] = torch.randn(n, generator=gen)
    for c in range(1, -(-n // CHUNK), 2):
        g[c * CHUNK:min(n, (c + 1) * CHUNK)] *= 1000.0
    return g.to(gpu)


def _launch(nat, g, n, c):
    """grad_sqnorm + clip_scale on NaN-poisoned outputs (one spare element each, which must
    stay NaN); returns (part, [norm, scale]) on the host."""
    nch = nat.clip_chunks(n)
    assert nch == -(-n // CHUNK)
    part = torch.full((nch + 1,), NAN, dtype=torch.float64, device=g.device)
    out = torch.full((3,), NAN, device=g.device)
    assert g.data_ptr() % 16 == 0
    nat.grad_sqnorm(g.data_ptr(), n, part.data_ptr(), _st())
    nat.clip_scale(part.data_ptr(), nch, c, out.data_ptr(), _st())
    torch.cuda.synchronize()
    part, out = part.cpu(), out.cpu()
    assert math.isnan(float(part[nch])) and math.isnan(float(out[2]))
    return part[:nch], out[:2]


@pytest.mark.parametrize("n", LENGTHS)
def test_clip_kernels_against_fp64(gpu, nat, n):
    g = _gradient(n, gpu, seed=31 + n % 7)
    parts, ss = co.sumsq_reference(g, n)
    assert len(parts) == -(-n // CHUNK) and (n < 65 * 4096 or len(parts) > 64)
    part, out = _launch(nat, g, n, INF)
    for i, ref in enumerate(parts):
        got = float(part[i])
        assert abs(got - ref) <= co.SS_REL * ref, ("partial", n, i, got, ref)
    norm, _ = co.check_norm_scale(float(out[0]), float(out[1]), ss, INF, f"n={n} c=inf")
    assert float(out[1]) == 1.0
    norm_k = float(out[0])
    worst = 0.0
    for c, clipped in ((2.0 * norm, False), (norm / 3.0, True)):
        part2, out2 = _launch(nat, g, n, c)
        assert torch.equal(part2, part) and float(out2[0]) == norm_k   # bit-reproducible
        _, scale = co.check_norm_scale(float(out2[0]), float(out2[1]), ss, c, f"n={n} c={c}")
        assert (scale != 1.0) == clipped and (float(out2[1]) == 1.0) == (not clipped)
        if clipped:
            worst = abs(float(out2[1]) - scale) / (co.SCALE_REL * scale)
            part3, out3 = _launch(nat, g, n, c)
            assert torch.equal(part3, part2) and torch.equal(out3, out2)
    print(f"n={n}: norm err/bound {abs(norm_k - norm) / (co.NORM_REL * norm):.3f}, "
          f"scale err/bound {worst:.3f}")


def test_clip_zero_gradient(gpu, nat):
    n = 4096 + 7
    g = torch.full((n + 8,), INF, device=gpu)
    g[:n] = 0.0
    part, out = _launch(nat, g, n, 0.5)
    assert float(part.abs().sum()) == 0.0
    assert float(out[0]) == 0.0 and float(out[1]) == 1.0


@pytest.mark.parametrize("bad", [INF, NAN])
@pytest.mark.parametrize("c", [1.0, INF])
def test_clip_non_finite_gradient_gives_nan_scale(gpu, nat, bad, c):
    """One inf / NaN inside [0, n): the scale is NaN (data only, nothing faults)."""
    n = 2 * 4096 + 5
    g = _gradient(n, gpu, seed=5)
    g[4096 + 17] = bad
    part, out = _launch(nat, g, n, c)
    assert math.isfinite(float(part[0])) and not math.isfinite(float(part[1]))
    assert math.isnan(float(out[1]))
    assert (math.isinf(float(out[0])) if bad == INF else math.isnan(float(out[0])))


def test_clip_bindings_reject_bad_arguments(gpu, nat):
    g = _gradient(64, gpu, seed=1)
    part = torch.zeros(2, dtype=torch.float64, device=gpu)
    out = torch.zeros(2, device=gpu)
    with pytest.raises(ValueError):
        nat.grad_sqnorm(g.data_ptr() + 4, 8, part.data_ptr(), _st())
    for c in (0.0, -1.0, NAN):
        with pytest.raises(ValueError):
            nat.clip_scale(part.data_ptr(), 1, c, out.data_ptr(), _st())
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(part)) == 0 and int(torch.count_nonzero(out)) == 0


# ---------------------------------------------------------------- the clipped update
SEVEN = LRSchedule(0.3, [10, 20, 35, 50, 80, 81, 1000],
                   [0.3, 0.2, 0.1, 0.05, 0.02, 0.01, 0.005, 0.001],
                   warm_steps=5, warm_from=0.01, warm_to=0.3)


def V(n):
    return ("vec", 1, 1, 1, n, 1, 1, False, False)


# vectors at unaligned offsets, a conv with kpad > K, tensors of one chunk + 1 and more
TABLE = [V(3), ("conv", 3, 3, 3, 16, 8, 16, True, False), V(1),
         ("conv", 1, 1, 64, 64, 64, 64, True, True), V(5), V(CHUNK + 1), V(7),
         ("conv", 1, 1, 16, 24, 16, 32, True, True), V(10), V(2 * CHUNK + 5),
         ("dense", 1, 1, 64, 10, 64, 16, True, True), V(3)]


def _dev(arr, gpu):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).to(gpu)


def _sa(s):
    return (s.init, s.warm_steps, s.warm_from, s.warm_to, list(s.bounds), list(s.values))


@pytest.mark.parametrize("use_momentum", [1, 0])
def test_clipped_update_equals_host_scaled_update(gpu, nat, use_momentum):
    """sgd_clip_update_pack with the device scale == sgd_update_pack with that fp32 scale
    as its host grad_scale: weights, momentum and both bf16 copies, bit for bit."""
    seg, _, n, bf_total, tile0, tiles = oo.build_seg_table(TABLE)
    assert {int(r["offset"]) % 4 for r in seg} == {0, 1, 2, 3} and n % 4 != 0
    assert any(int(r["kpad"]) > int(r["K"]) for r in seg)
    segs_d, tile0_d = _dev(seg, gpu), torch.from_numpy(tile0).to(gpu)
    gen = torch.Generator().manual_seed(41)
    w0, g, m0 = (torch.randn(n, generator=gen).to(gpu) for _ in range(3))
    momentum, wd, step = 0.9, 2e-4, 36
    _, ss = co.sumsq_reference(g, n)
    c = math.sqrt(ss) / 3.0
    nch = nat.clip_chunks(n)
    part = torch.full((nch,), NAN, dtype=torch.float64, device=gpu)
    slot = torch.full((2,), NAN, device=gpu)
    nat.grad_sqnorm(g.data_ptr(), n, part.data_ptr(), _st())
    nat.clip_scale(part.data_ptr(), nch, c, slot.data_ptr(), _st())
    torch.cuda.synchronize()
    norm_k, scale_k = slot.cpu().tolist()
    _, scale = co.check_norm_scale(norm_k, scale_k, ss, c, "table")
    assert scale < 0.5

    def run(clipped):
        w, mom = w0.clone(), m0.clone()
        wbf = torch.zeros(bf_total, dtype=torch.bfloat16, device=gpu)
        gstep = torch.tensor([step], dtype=torch.int64, device=gpu)
        lr_out = torch.full((1,), 7.0, device=gpu)
        head = (w.data_ptr(), g.data_ptr(), mom.data_ptr(), n, *_sa(SEVEN), gstep.data_ptr(),
                momentum, wd)
        tail = (use_momentum, segs_d.data_ptr(), len(seg), wbf.data_ptr(), lr_out.data_ptr())
        if clipped:
            nat.sgd_clip_update_pack(*head, slot.data_ptr(), *tail, _st())
        else:
            nat.sgd_update_pack(*head, scale_k, *tail, 1, _st())
        nat.ohwi_pack(w.data_ptr(), segs_d.data_ptr(), tile0_d.data_ptr(), len(seg), tiles,
                      wbf.data_ptr(), gstep.data_ptr(), _st())
        torch.cuda.synchronize()
        assert int(gstep) == step + 1
        return w, mom, wbf, lr_out

    a, b = run(True), run(False)
    for x, y, what in zip(a, b, ("w", "mom", "wbf", "lr")):
        assert torch.equal(x, y), what
    w, mom, wbf, lr_out = a
    assert torch.equal(slot.cpu(), torch.tensor([norm_k, scale_k]))   # the slot is only read
    # ...and both are the fp64 update with that scale, within optim_oracle's bound
    lr = float(lr_out)
    assert lr == oo.f32(oo.lr_reference(oo.f32_schedule(SEVEN), step))
    w_ref, m_ref, B = oo.sgd_reference(w0, g, m0, lr, oo.f32(momentum), oo.f32(wd), scale_k,
                                       bool(use_momentum))
    assert bool(((w.double() - w_ref).abs() <= B).all())
    assert bool(((mom.double() - m_ref).abs() <= B).all())
    assert use_momentum or torch.equal(mom, m0)
    assert torch.equal(wbf, oo.expected_wbf(seg, w, bf_total))
    assert float((w - w0).abs().max()) > 1e-3


# ---------------------------------------------------------------- engine
WD = 5e-4
CLIP_OPS = ("grad_sqnorm", "clip_scale", "sgd_clip_update_pack")


def _engine(spec, N, gpu, monkeypatch, tune="", seed=0, **kw):
    monkeypatch.setenv("DTR_TUNE", tune)
    eng = Engine(spec, N, weight_decay=WD, lr_schedule=cifar_lr_schedule(), device=gpu,
                 input_mode="nhwc", seed=seed, **kw)
    gen = torch.Generator().manual_seed(5)
    imgs = torch.randn(N, spec.image_h, spec.image_w, 3, generator=gen).to(torch.bfloat16).float()
    eng.set_batch(imgs.to(gpu), torch.randint(0, spec.num_classes, (N,), generator=gen).to(gpu))
    return eng


def _state(eng):
    return [eng.params.master.clone(), eng.mom.clone(), eng.params.stats.clone(),
            eng.wbf.clone(), eng.gstep.clone()]


def _check_clipped_step(eng, w0, m0, step, what):
    """clip_state() against the fp64 norm of the engine's own gradient, and the weights
    and momentum against the fp64 update with the scale the device formed."""
    n = eng.params.n_train
    norm_k, scale_k = eng.clip_state()
    _, ss = co.sumsq_reference(eng.grad, n)
    norm, scale = co.check_norm_scale(norm_k, scale_k, ss, eng.clip_grad_norm, what)
    lr = oo.f32(oo.lr_reference(eng.sched, step))
    m = eng.metrics()
    assert m["lr"] == lr and m["grad_norm"] == norm_k and m["clip_scale"] == scale_k
    w_ref, m_ref, B = oo.sgd_reference(w0[:n], eng.grad[:n], m0[:n], lr, oo.f32(eng.momentum),
                                       oo.f32(eng.wd), scale_k, True)
    ew = (eng.params.master[:n].double() - w_ref).abs()
    em = (eng.mom[:n].double() - m_ref).abs()
    print(f"{what} step {step}: norm {norm_k:.6g} scale {scale_k:.6g}, max err/bound master "
          f"{float((ew / B.clamp_min(1e-300)).max()):.3f} mom "
          f"{float((em / B.clamp_min(1e-300)).max()):.3f}")
    assert bool((ew <= B).all()), (what, step, float(ew.max()))
    assert bool((em <= B).all()), (what, step, float(em.max()))
    assert torch.equal(eng.wbf, oo.expected_wbf(eng.seg_arr, eng.params.master, eng.wbf.numel()))
    return norm, scale


@pytest.mark.parametrize("persist", [0, 1])
@pytest.mark.parametrize("N", [4, 8])
def test_engine_measure_only_is_bitwise_clipping_off(gpu, monkeypatch, persist, N):
    """clip_grad_norm=inf (default one-launch optimizer tuned on, so the flag turns it off)
    against clipping off on the generic optimizer branch (opt_fused=0)."""
    spec = cifar_spec(8)
    off = _engine(spec, N, gpu, monkeypatch, f"persist={persist},opt_fused=0")
    on = _engine(spec, N, gpu, monkeypatch, f"persist={persist}", clip_grad_norm=INF)
    for e in (off, on):
        assert e.persist == bool(persist) and not e.opt_fused
    assert off.clip_state() is None and off.opt_fused_reason == ""
    assert on.opt_fused_reason.startswith("clip_grad_norm:")
    assert set(off.metrics()) == {"global_step", "cross_entropy", "cost", "precision", "lr", "l2"}
    # op for op the plan without the flag, the two launches in front of the update aside
    names_off, names_on = off.plan.names(), on.plan.names()
    assert not [x for x in names_off if x in CLIP_OPS]
    assert len(names_on) == len(names_off) + 2
    a, b = on.seg["opt"]
    assert [x for x in names_on[a:b] if x in CLIP_OPS + ("sgd_update_pack", "sgd_tiles",
                                                         "ohwi_pack")] == \
        list(CLIP_OPS) + ["ohwi_pack"]
    assert [("sgd_update_pack" if x == "sgd_clip_update_pack" else x)
            for x in names_on if x not in CLIP_OPS[:2]] == names_off
    for step in range(3):
        off.step()
        on.step()
        torch.cuda.synchronize()
        assert not on.persist_error() and not off.persist_error()
        norm_k, scale_k = on.clip_state()
        _, ss = co.sumsq_reference(on.grad, on.params.n_train)
        co.check_norm_scale(norm_k, scale_k, ss, INF, f"measure-only step {step}")
        assert scale_k == 1.0 and norm_k > 0
        assert torch.equal(on.grad, off.grad)
    for x, y in zip(_state(on), _state(off)):
        assert torch.equal(x, y)
    assert int(on.gstep.item()) == 3


@pytest.mark.parametrize("persist", [0, 1])
@pytest.mark.parametrize("N", [4, 8])
def test_engine_clipped_step(gpu, monkeypatch, persist, N):
    """c = half the first step's measured norm: the first step clips by ~0.5."""
    spec = cifar_spec(8)
    probe = _engine(spec, N, gpu, monkeypatch, f"persist={persist}", clip_grad_norm=INF)
    probe.step()
    norm0, _ = probe.clip_state()
    g0 = probe.grad.clone()
    eng = _engine(spec, N, gpu, monkeypatch, f"persist={persist}", clip_grad_norm=norm0 / 2)
    assert eng.persist == bool(persist) and not eng.opt_fused
    for step in range(3):
        w0, m0 = eng.params.master.clone(), eng.mom.clone()
        eng.step()
        torch.cuda.synchronize()
        assert not eng.persist_error()
        _, scale = _check_clipped_step(eng, w0, m0, step, f"cifar8 N={N} persist={persist}")
        if step == 0:
            # (c is half an fp32 norm that is itself within NORM_REL of the exact one)
            assert abs(scale - 0.5) <= 0.5 * (co.NORM_REL + 2 * co.U32)
            assert torch.equal(eng.grad, g0)   # the gradient buffer is not rescaled
    assert int(eng.gstep.item()) == 3


def test_engine_clip_imagenet_s2d_stem(gpu, monkeypatch):
    """The s2d stem's gradient is mapped back in front of the norm."""
    eng = _engine(imagenet_spec(18, image_hw=64), 2, gpu, monkeypatch, "persist=0",
                  clip_grad_norm=1e-3)
    assert eng.stem_s2d and not eng.persist
    w0, m0 = eng.params.master.clone(), eng.mom.clone()
    eng.step()
    torch.cuda.synchronize()
    _, scale = _check_clipped_step(eng, w0, m0, 0, "imagenet18 s2d")
    assert scale < 1.0


def test_engine_clip_same_seed_engines_agree_bitwise(gpu, monkeypatch):
    a = _engine(cifar_spec(8), 8, gpu, monkeypatch, clip_grad_norm=0.05)
    b = _engine(cifar_spec(8), 8, gpu, monkeypatch, clip_grad_norm=0.05)
    clipped = 0
    for _ in range(5):
        a.step()
        b.step()
        sa, sb = a.clip_state(), b.clip_state()
        assert sa == sb
        clipped += sa[1] < 1.0
    torch.cuda.synchronize()
    assert clipped > 0
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)


def test_engine_clip_rejects_bad_values(gpu, monkeypatch):
    for bad in (-1.0, NAN):
        with pytest.raises(ValueError):
            _engine(cifar_spec(8), 4, gpu, monkeypatch, clip_grad_norm=bad)
    with pytest.raises(ValueError):
        _engine(cifar_spec(8), 4, gpu, monkeypatch, clip_grad_norm=1.0, optimizer="lars")
