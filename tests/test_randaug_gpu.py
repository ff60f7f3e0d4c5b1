"""csrc/randaug.hip against its specification (data/randaug.py), bit for bit: every op alone in
both layouts, chains that move the image between its two homes, the binding's refusals, and the
launch in front of the input launch on the engine's plans (eager, overlap, graph replay)."""
import functools

import numpy as np
import pytest
import torch

from test_randaug_cpu import images

import distributed_tensorflow_resnet_amd as dtr
from distributed_tensorflow_resnet_amd.data import randaug as ra
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.train.engine import (Engine, cifar_lr_schedule,
                                                            imagenet_lr_schedule)

pytestmark = pytest.mark.gpu

SEED = 4321
LAYOUTS = {"chw32": (0, 3, 32, 32), "hwc64x48": (1, 2, 64, 48), "hwc224": (1, 2, 224, 224)}
GATHER, POINT = set(range(1, 6)), {6, 7, 8, 10, 11, 12, 13}


@functools.lru_cache(maxsize=None)
def _batch(hwc, N, H, W, first):
    """N images, image n of kind (first + n) % 4 of test_randaug_cpu.images."""
    x = np.stack([images(H, W)[(first + n) % 4] for n in range(N)])
    return np.ascontiguousarray(x if hwc else x.transpose(0, 3, 1, 2))


def _launch(gpu, x, hwc, step, num_ops, ops, m=9):
    nat, N = dtr.native(required=True), x.shape[0]
    H, W = x.shape[1:3] if hwc else x.shape[2:]
    src = torch.from_numpy(x).to(gpu)
    dst = torch.zeros_like(src)
    tab = torch.from_numpy(ra.randaug_tables(m, H, W)).to(gpu)
    log = torch.full((N, num_ops, 2), -7, dtype=torch.int32, device=gpu)
    gstep = torch.tensor([step], dtype=torch.int64, device=gpu)
    nat.randaug(src.data_ptr(), dst.data_ptr(), N, H, W, int(hwc), SEED, gstep.data_ptr(),
                num_ops, tab.data_ptr(), tab.numel(), list(ops), log.data_ptr(), 0)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), log.cpu().numpy()


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("op", range(14), ids=ra.RA_OPS)
def test_each_op_equals_the_spec(gpu, op, layout):
    hwc, N, H, W = LAYOUTS[layout]
    signs = set()
    for i, step in enumerate((0, 1, 2 ** 32 + 3)):
        x = _batch(hwc, N, H, W, i)
        got, log = _launch(gpu, x, hwc, step, 1, [op])
        want, wlog = ra.randaug_batch(x, "hwc" if hwc else "chw", SEED, step, 1, 9, [op])
        assert np.array_equal(log, wlog) and (log[:, 0, 0] == op).all(), step
        assert np.array_equal(got, want), (step, np.argwhere(got != want)[:4])
        signs |= set(log[:, 0, 1].tolist())
    assert signs == {0, 1}


@pytest.mark.parametrize("layout", ["chw32", "hwc224"])
def test_chains_equal_the_spec(gpu, layout):
    hwc, _, H, W = LAYOUTS[layout]
    pairs = set()
    for num_ops, steps in ((2, (0, 5, 9)), (3, (0, 1, 56))):
        for i, step in enumerate(steps):
            x = _batch(hwc, 2, H, W, i)
            got, log = _launch(gpu, x, hwc, step, num_ops, range(14))
            want, wlog = ra.randaug_batch(x, "hwc" if hwc else "chw", SEED, step, num_ops, 9)
            assert np.array_equal(log, wlog), (num_ops, step)
            assert np.array_equal(got, want), (num_ops, step, log.tolist())
            pairs |= {(a, b) for row in log[:, :, 0].tolist() for a, b in zip(row, row[1:])}
    for A, B in ((GATHER, GATHER), (GATHER, POINT), (POINT, GATHER), ({9}, GATHER)):
        assert any(a in A and b in B for a, b in pairs)   # the steps were picked for these


def test_refusals(gpu):
    nat = dtr.native(required=True)
    buf = torch.zeros(2 * 3 * 256 * 256 + 64, dtype=torch.uint8, device=gpu)
    tab = torch.from_numpy(ra.randaug_tables(9, 32, 32)).to(gpu)
    a, b = buf.data_ptr(), buf.data_ptr() + 3 * 256 * 256
    good = dict(img=a, out=b, N=1, H=32, W=32, hwc=0, num_ops=2, tl=64, ops=[0, 13])
    for bad in (dict(img=0), dict(out=0), dict(img=a + 4), dict(out=b + 8), dict(num_ops=0),
                dict(num_ops=4), dict(ops=[]), dict(ops=[14]), dict(tl=63), dict(H=31),
                dict(hwc=1, H=256, W=256)):
        k = {**good, **bad}
        with pytest.raises(ValueError):
            nat.randaug(k["img"], k["out"], k["N"], k["H"], k["W"], k["hwc"], SEED, 0,
                        k["num_ops"], tab.data_ptr(), k["tl"], k["ops"], 0, 0)


@functools.lru_cache(maxsize=None)
def _records(n):
    g = torch.Generator().manual_seed(7)
    return (torch.randint(0, 256, (n, 3, 32, 32), generator=g, dtype=torch.uint8),
            torch.randint(0, 10, (n,), generator=g, dtype=torch.int32))


def _engine(monkeypatch, gpu, tune, N=4, **kw):
    monkeypatch.setenv("DTR_TUNE", tune)
    eng = Engine(cifar_spec(8), N, weight_decay=2e-4, lr_schedule=cifar_lr_schedule(),
                 device=gpu, input_mode="cifar_u8", data_seed=SEED, seed=3, **kw)
    eng.set_batch(*_records(N))
    assert eng.persist == (tune == "persist=1")
    return eng


def _same(a, b):
    torch.cuda.synchronize()
    assert not a.persist_error() and not b.persist_error()
    return all(torch.equal(x, y) for x, y in ((a.params.master, b.params.master), (a.mom, b.mom),
                                              (a.params.stats, b.params.stats),
                                              (a.gstep, b.gstep)))


def _follow(eng, off, records, layout, steps=2, first=0):
    # each step: eng's x_in equals that of `off` fed the spec's augmented records
    for step in range(first, first + steps):
        want, wlog = ra.randaug_batch(records[0].numpy(), layout, SEED, step, 2, 9)
        off.set_batch(torch.from_numpy(want), records[1])
        eng.step()
        off.step()
        torch.cuda.synchronize()
        assert not eng.persist_error() and not off.persist_error()
        assert torch.equal(eng.x_in.view(torch.int16), off.x_in.view(torch.int16)), step
        assert np.array_equal(eng.randaug_state(), wlog), step


@pytest.mark.parametrize("extra", [{}, dict(mixup_alpha=0.4, erase_prob=1.0)], ids=["plain", "mix"])
@pytest.mark.parametrize("tune", ["persist=0", "persist=1"])
def test_engine_step_augments_in_front_of_the_input_launch(gpu, monkeypatch, tune, extra):
    eng = _engine(monkeypatch, gpu, tune, randaug_num_ops=2, **extra)
    off = _engine(monkeypatch, gpu, tune, **extra)
    assert eng.randaug_state() is None and off.img_ra is None and off.randaug_log is None
    names = eng.plan.names()
    i = names.index("randaug")
    assert names[i + 1] == "cifar_augment" and eng.plan.op_streams()[i] == 0
    assert names[:i] + names[i + 1:] == off.plan.names()
    _follow(eng, off, _records(4), "chw")
    if extra:   # the mix and the erased boxes are what they are without RandAugment
        assert eng.mix_state() == off.mix_state()
        assert np.array_equal(eng.erase_state(), off.erase_state())


def test_engine_step_on_the_persistent_overlap_plan(gpu, monkeypatch):
    eng, off = (_engine(monkeypatch, gpu, "persist=1", N=16, bucket_mb=0.05, randaug_num_ops=k,
                        comm=dtr.native().Comm.loopback(2.0)) for k in (2, 0))
    assert eng.persist_overlap and off.persist_overlap
    names = eng.plan.names()
    i = names.index("randaug")
    assert names[i + 1] == "cifar_augment" and eng.recorded.op_buffers[i] == {"input"}
    assert names[:i] + names[i + 1:] == off.plan.names()
    _follow(eng, off, _records(16), "chw")


def test_imagenet_engine_step(gpu):
    spec = imagenet_spec(0, num_classes=10, image_hw=64, block="bottleneck", layers=[1, 1, 1, 1])
    g = torch.Generator().manual_seed(9)
    rec = (torch.randint(0, 256, (2, 64, 64, 3), generator=g, dtype=torch.uint8),
           torch.randint(0, 10, (2,), generator=g, dtype=torch.int32))
    eng, off = (Engine(spec, 2, weight_decay=1e-4, lr_schedule=imagenet_lr_schedule(),
                       device=gpu, input_mode="imagenet_u8", data_seed=SEED, seed=3,
                       randaug_num_ops=k) for k in (2, 0))
    eng.set_batch(*rec)
    assert eng.plan.names()[eng.plan.names().index("randaug") + 1] == "imagenet_u8_pack"
    _follow(eng, off, rec, "hwc")


@pytest.mark.parametrize("tune", ["persist=0", "persist=1"])
def test_zero_ops_is_bitwise_the_default(gpu, monkeypatch, tune):
    plain = _engine(monkeypatch, gpu, tune)
    zero = _engine(monkeypatch, gpu, tune, randaug_num_ops=0, randaug_magnitude=30,
                   randaug_ops="Rotate")
    assert zero.img_ra is None and zero.randaug_tab is None and zero.randaug_log is None
    assert zero.plan.size() == plain.plan.size() and zero.plan.names() == plain.plan.names()
    for _ in range(3):
        plain.step()
        zero.step()
    assert _same(plain, zero) and zero.randaug_state() is None


def test_graph_replay_draws_fresh_ops(gpu, monkeypatch):
    eng = _engine(monkeypatch, gpu, "persist=1", randaug_num_ops=2, use_graph=True)
    off = _engine(monkeypatch, gpu, "persist=1")
    done = eng.capture(warmup=2)
    for _ in range(done):
        off.step()
    logs = []
    for step in range(done, done + 3):
        _follow(eng, off, _records(4), "chw", steps=1, first=step)
        logs.append(eng.randaug_state().tolist())
    assert eng.graph is not None and logs[0] != logs[1] != logs[2] != logs[0]
    eager = _engine(monkeypatch, gpu, "persist=1", randaug_num_ops=2)
    for _ in range(done + 3):
        eager.step()
    assert _same(eng, eager)
