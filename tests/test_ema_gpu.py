"""The weight-EMA kernel (csrc/ema.hip ema_update) launched directly, and the engine's shadows
on the per-layer and persistent plans, against the fp64 reference and the derived bound of
tests/ema_oracle.py; the recording, determinism and resume, hipGraph replay, and the
evaluator on EMA weights."""
import numpy as np
import pytest
import torch

import ema_oracle as eo
from distributed_tensorflow_resnet_amd.models.params import ParamStore
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule
from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver, ema_weights, state_to_tf

pytestmark = pytest.mark.gpu

MAX_BLOCKS = 4096                       # ema.hip's grid cap; a workgroup covers 1024 floats a trip
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 256 * 4 * 3 + 7, MAX_BLOCKS * 1024 + 5]
GUARD = 8
WD = 5e-4


@pytest.fixture(scope="module")
def nat(gpu):
    import distributed_tensorflow_resnet_amd as dtr

    return dtr.native(required=True)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _values(n, seed, gpu):
    """O(1) values bounded away from zero, every other 1024-block scaled 1000x."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=gen)
    x = x + 0.25 * torch.sign(x)
    scale = torch.where((torch.arange(n) // 1024) % 2 == 1, 1000.0, 1.0)
    return (x * scale).to(gpu)


# ---------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("n", SIZES)
def test_ema_update_kernel(nat, gpu, n):
    guard = torch.tensor([float.fromhex("0x1.234p5")] * GUARD, device=gpu)
    master0 = torch.cat([_values(n, 1, gpu), guard])
    shadow0 = torch.cat([_values(n, 2, gpu), -guard])
    worst = 0.0
    for decay in (0.5, 0.9999):
        omd = eo.f32(1.0 - decay)
        for k in (0, 7, 8, 10 ** 6):
            for warm in (1, 0):
                master, shadow = master0.clone(), shadow0.clone()
                gstep = torch.tensor([k], dtype=torch.int64, device=gpu)
                nat.ema_update(master.data_ptr(), shadow.data_ptr(), n, gstep.data_ptr(), omd,
                               warm, _st())
                torch.cuda.synchronize()
                ref, B = eo.ema_reference(shadow0[:n], master0[:n], decay, k, bool(warm))
                err = (shadow[:n].double() - ref).abs()
                worst = max(worst, float((err / B.clamp_min(1e-300)).max()))
                assert bool((err <= B).all()), (n, decay, k, warm, float(err.max()))
                assert torch.equal(shadow[n:], shadow0[n:])          # guard words untouched
                assert torch.equal(master, master0) and int(gstep.item()) == k
                # it moved: towards the master by the rate of this k
                assert not torch.equal(shadow[:n], shadow0[:n])
    print(f"n={n}: max err/bound {worst:.3f}")


def test_ema_update_rejects_misaligned_bases(nat, gpu):
    m, s = torch.zeros(64, device=gpu), torch.zeros(64, device=gpu)
    g = torch.zeros(1, dtype=torch.int64, device=gpu)
    for dm, ds in ((4, 0), (0, 4), (8, 8)):
        with pytest.raises(ValueError, match="16-byte"):
            nat.ema_update(m.data_ptr() + dm, s.data_ptr() + ds, 16, g.data_ptr(), 0.5, 1, _st())
    with pytest.raises(ValueError, match="16-byte"):
        nat.Plan().ema_update(m.data_ptr() + 4, s.data_ptr(), 16, g.data_ptr(), 0.5, 1)
    torch.cuda.synchronize()
    assert not m.any() and not s.any()


# ---------------------------------------------------------------- engine
def _engine(spec, N, gpu, seed=0, **kw):
    eng = Engine(spec, N, weight_decay=WD, lr_schedule=cifar_lr_schedule(), device=gpu,
                 input_mode="nhwc", seed=seed, **kw)
    gen = torch.Generator().manual_seed(5)
    imgs = torch.randn(N, spec.image_h, spec.image_w, 3, generator=gen).to(torch.bfloat16).float()
    eng.set_batch(imgs.to(gpu), torch.randint(0, spec.num_classes, (N,), generator=gen).to(gpu))
    return eng


def _state(eng):
    return [eng.params.master.clone(), eng.mom.clone(), eng.params.stats.clone(),
            eng.gstep.clone()]


CASES = {"cifar8-layers": (lambda: cifar_spec(8), 16, "persist=0", {}),
         "cifar8-persist": (lambda: cifar_spec(8), 16, "persist=1", {}),
         "imagenet18": (lambda: imagenet_spec(18, image_hw=64), 8, "persist=0", {}),
         "imagenet18-lars": (lambda: imagenet_spec(18, image_hw=64), 8, "persist=0",
                             dict(optimizer="lars", lars_eeta=0.01, lars_epsilon=1e-6))}


@pytest.mark.parametrize("case", list(CASES))
def test_engine_shadow_follows_the_oracle_and_only_observes(gpu, monkeypatch, case):
    mk, N, tune, kw = CASES[case]
    monkeypatch.setenv("DTR_TUNE", tune)
    eng = _engine(mk(), N, gpu, ema_decay=0.5, **kw)
    off = _engine(mk(), N, gpu, **kw)
    assert eng.persist == (tune == "persist=1") and off.ema is None and off.ema_state() is None
    n = eng.params.n_train
    assert eng.ema.shape == (n,) and torch.equal(eng.ema, eng.params.master)
    assert eng.ema.data_ptr() != eng.params.master.data_ptr()
    worst = 0.0
    for step in range(12):
        prev = eng.ema.clone()
        eng.step()
        off.step()
        torch.cuda.synchronize()
        assert not eng.persist_error()
        k = int(eng.gstep.item())
        assert k == step + 1
        ref, B = eo.ema_reference(prev, eng.params.master.detach(), 0.5, k, True)
        err = (eng.ema.double() - ref).abs()
        worst = max(worst, float((err / B.clamp_min(1e-300)).max()))
        assert bool((err <= B).all()), (case, step, float(err.max()))
    print(f"{case}: max err/bound {worst:.3f}")
    for a, b in zip(_state(eng), _state(off)):      # the EMA is a pure observer
        assert torch.equal(a, b)
    assert not torch.equal(eng.ema, eng.params.master)
    views = eng.ema_state()
    assert list(views) == [s.name for s in eng.params.train_slots]
    s = eng.params.train_slots[1]
    assert views[s.name].shape == tuple(s.shape)
    assert views[s.name].data_ptr() == eng.ema.data_ptr() + 4 * s.offset


def test_engine_shadow_on_the_persistent_overlap_plan(gpu, monkeypatch):
    """comm = the doubling loopback: buckets updated on the comm stream beside the backward,
    the EMA launch on the main stream behind the join (the stream check passes at build)."""
    import distributed_tensorflow_resnet_amd as dtr

    monkeypatch.setenv("DTR_TUNE", "persist=1")
    mk = lambda **kw: _engine(cifar_spec(8), 16, gpu, bucket_mb=0.05,   # noqa: E731
                              comm=dtr.native().Comm.loopback(2.0), **kw)
    eng, off = mk(ema_decay=0.5), mk()
    assert eng.persist and eng.persist_overlap and off.persist_overlap
    names = eng.plan.names()
    a, b = eng.seg["opt"]
    assert names.count("ema_update") == 1 and a <= names.index("ema_update") < b
    assert eng.plan.op_streams()[names.index("ema_update")] == 0
    for step in range(4):
        prev = eng.ema.clone()
        eng.step()
        off.step()
        torch.cuda.synchronize()
        assert not eng.persist_error()
        ref, B = eo.ema_reference(prev, eng.params.master.detach(), 0.5, step + 1, True)
        assert bool(((eng.ema.double() - ref).abs() <= B).all()), step
    for x, y in zip(_state(eng), _state(off)):
        assert torch.equal(x, y)


def test_engine_rejects_a_decay_outside_0_1(gpu):
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError, match="ema_decay"):
            _engine(cifar_spec(8), 16, gpu, ema_decay=bad)


@pytest.mark.parametrize("tune", ["persist=0", "persist=1"])
def test_recording_adds_one_op_inside_opt(gpu, monkeypatch, tune):
    monkeypatch.setenv("DTR_TUNE", tune)
    spec = cifar_spec(8)
    parent = _engine(spec, 16, gpu)                    # as every caller built it so far
    off = _engine(spec, 16, gpu, ema_decay=0.0)
    on = _engine(spec, 16, gpu, ema_decay=0.9999, ema_warmup=False)
    assert off.plan.names() == parent.plan.names() and off.seg == parent.seg
    assert "ema_update" not in off.plan.names()
    names = on.plan.names()
    assert on.plan.size() == off.plan.size() + 1 and names.count("ema_update") == 1
    i = names.index("ema_update")
    a, b = on.seg["opt"]
    assert a <= i < b and names[:i] + names[i + 1:] == off.plan.names()
    assert on.plan.op_streams()[i] == 0                # main stream, after every join
    assert i < on.recorded.t_opt_end < b               # inside the timed optimizer phase
    last_update = max(j for j, nm in enumerate(names[a:b], a)
                      if nm in ("sgd_update_pack", "ohwi_pack", "sgd_tiles"))
    assert i > last_update                             # behind the update and the step increment
    if "gsum" in on.seg:
        ga, gb = on.seg["gsum"]
        assert "ema_update" not in names[ga:gb]
        prev = on.ema.clone()
        on.forward_backward()                          # gradient without update: shadows stay
        torch.cuda.synchronize()
        assert torch.equal(on.ema, prev)


def test_same_seed_engines_and_resume_are_bitwise(gpu, tmp_path):
    from distributed_tensorflow_resnet_amd.train.backends import GPUBackend

    spec = cifar_spec(8)
    a, b = _engine(spec, 16, gpu, ema_decay=0.5), _engine(spec, 16, gpu, ema_decay=0.5)
    for _ in range(10):
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.ema, b.ema)
    first = GPUBackend(_engine(spec, 16, gpu, ema_decay=0.5))
    for _ in range(5):
        first.step()
    torch.cuda.synchronize()
    tensors = first.state_tensors()
    name = first.engine.params.train_slots[0].name
    assert np.array_equal(tensors[name + "/ExponentialMovingAverage"],
                          first.engine.ema_state()[name].cpu().numpy())
    prefix = Saver(str(tmp_path)).save(tensors, 5)
    second = GPUBackend(_engine(spec, 16, gpu, seed=9, ema_decay=0.5))
    second.load_state(Saver.restore(prefix))
    assert second.global_step == 5 and torch.equal(second.engine.ema, first.engine.ema)
    for _ in range(5):
        second.step()
    torch.cuda.synchronize()
    for x, y in zip(_state(a) + [a.ema], _state(second.engine) + [second.engine.ema]):
        assert torch.equal(x, y)
    # a checkpoint without shadows: they start from the restored weights
    third = GPUBackend(_engine(spec, 16, gpu, seed=3, ema_decay=0.5))
    third.load_state({k: v for k, v in tensors.items() if not k.endswith("MovingAverage")})
    assert torch.equal(third.engine.ema, first.engine.params.master)


def test_graph_replay_gives_the_eager_shadows(gpu):
    spec = cifar_spec(8)
    eager = _engine(spec, 16, gpu, ema_decay=0.5, use_graph=True)   # the same recording,
    graph = _engine(spec, 16, gpu, ema_decay=0.5, use_graph=True)   # stepped eagerly / replayed
    for _ in range(6):
        eager.step()
    done = graph.capture(warmup=2)
    assert graph.graph is not None
    for _ in range(6 - done):
        graph.step()
    torch.cuda.synchronize()
    assert int(graph.gstep.item()) == 6
    assert torch.equal(graph.ema, eager.ema) and torch.equal(graph.params.master,
                                                             eager.params.master)


def test_gpu_inference_on_ema_weights(gpu):
    from distributed_tensorflow_resnet_amd.train.evaluator import GPUInference

    spec = cifar_spec(8)
    a, b = ParamStore(spec), ParamStore(spec)
    a.initialize(1)
    b.initialize(2)
    a.stats.data.add_(0.125)
    ckpt = state_to_tf(a, None, 3, ema=b.master.detach())
    gen = torch.Generator().manual_seed(11)
    x = torch.randint(0, 256, (16, 3, 32, 32), generator=gen, dtype=torch.uint8)
    y = torch.randint(0, 10, (16,), generator=gen)
    inf = GPUInference(spec, 16, device=gpu, ema=True)
    inf.load(ckpt)
    loss, correct, probs = inf.run(x, y)
    direct = GPUInference(spec, 16, device=gpu)           # master := the shadows, directly
    direct.engine.params.master.data.copy_(b.master.detach())
    direct.engine.params.stats.data.copy_(a.stats.detach())
    direct.engine.repack()
    loss_d, correct_d, probs_d = direct.run(x, y)
    assert torch.equal(probs, probs_d) and (loss, correct) == (loss_d, correct_d)
    assert torch.equal(inf.plan.logits, direct.plan.logits)
    raw = GPUInference(spec, 16, device=gpu)
    raw.load(ckpt)
    assert not torch.equal(raw.run(x, y)[2], probs)       # the raw weights score differently
    with pytest.raises(KeyError):
        inf.load(state_to_tf(a, None, 3))
    assert ema_weights(ckpt, a)["global_step"] == 3
