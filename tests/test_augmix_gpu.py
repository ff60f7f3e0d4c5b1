"""csrc/augmix.hip against its specification (data/augmix.py), byte for byte and log for log:
both layouts, every width and depth, op lists that leave a chain in either home, hand-made
table entries, and the launch in front of the input launch on the engine's plans."""
import functools

import numpy as np
import pytest
import torch

from test_randaug_cpu import images

import distributed_tensorflow_resnet_amd as dtr
from distributed_tensorflow_resnet_amd.data import augmix as am
from distributed_tensorflow_resnet_amd.data import randaug as ra
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.train.engine import (Engine, cifar_lr_schedule,
                                                            imagenet_lr_schedule)

pytestmark = pytest.mark.gpu

SEED = 4321
# 224x224 is the LDS limit and, like every HWC shape, the global other-home and workspace path
LAYOUTS = {"chw32": (0, 5, 32, 32), "hwc16": (1, 3, 16, 16), "hwc24x40": (1, 3, 24, 40),
           "hwc224": (1, 2, 224, 224)}
# the paper's nine; one moving op beside an in-place one, so that chains end in either home
# after odd and even counts of moves; Identity only
OP_LISTS = ("augmix", "Rotate,Solarize", "Identity")


@functools.lru_cache(maxsize=None)
def _batch(hwc, N, H, W):
    x = np.stack([images(H, W)[n % 4] for n in range(N)])
    return np.ascontiguousarray(x if hwc else x.transpose(0, 3, 1, 2))


class _Launch:
    """One set of device buffers, launched repeatedly: nothing is cleared in between."""

    def __init__(self, gpu, x, hwc, width, depth, ops, mix):
        self.N, (self.H, self.W) = x.shape[0], x.shape[1:3] if hwc else x.shape[2:]
        self.hwc, self.width, self.depth, self.ops = hwc, width, depth, [int(i) for i in ops]
        self.src = torch.from_numpy(x).to(gpu)
        self.dst = torch.full_like(self.src, 99)
        self.tab = torch.from_numpy(ra.randaug_tables(9, self.H, self.W)).to(gpu)
        self.mix = torch.from_numpy(np.ascontiguousarray(mix, dtype=np.int32)).to(gpu)
        self.acc = torch.full((self.N, 3 * self.H * self.W), -1, dtype=torch.int16, device=gpu)
        self.log = torch.full((self.N, width, 4, 2), -7, dtype=torch.int32, device=gpu)
        self.gstep = torch.zeros(1, dtype=torch.int64, device=gpu)

    def __call__(self, step):
        self.gstep.fill_(step)
        dtr.native(required=True).augmix(
            self.src.data_ptr(), self.dst.data_ptr(), self.N, self.H, self.W, int(self.hwc), SEED,
            self.gstep.data_ptr(), self.width, self.depth, self.tab.data_ptr(), self.tab.numel(),
            self.mix.data_ptr(), self.mix.numel(), self.ops,
            self.acc.data_ptr() if self.hwc and self.width > 1 else 0, self.log.data_ptr(), 0)
        torch.cuda.synchronize()
        return self.dst.cpu().numpy(), self.log.cpu().numpy()


def test_refuses_overlapping_buffers_and_a_missing_workspace(gpu):
    one = _Launch(gpu, _batch(1, 3, 16, 16), 1, 3, 1, [0], am.augmix_tables(3, 1.0, SEED))
    one(0)
    one.acc = torch.zeros(0, dtype=torch.int16)   # data_ptr() == 0: three chains need it
    with pytest.raises(ValueError, match="workspace"):
        one(0)
    one.width = 1   # one chain carries nothing, but the output lies inside the input
    one.dst = one.src.view(-1)[16:]
    with pytest.raises(ValueError, match="overlapping"):
        one(0)


def _spec(x, hwc, step, width, depth, ops, mix):
    H, W = x.shape[1:3] if hwc else x.shape[2:]
    return am.augmix_batch(x, "hwc" if hwc else "chw", SEED, step, width, depth, op_table=ops,
                           tables=ra.randaug_tables(9, H, W), mix_table=mix)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("depth", [1, 3, -1])
@pytest.mark.parametrize("width", [1, 3, 4])
def test_launch_equals_the_spec(gpu, width, depth, layout):
    hwc, N, H, W = LAYOUTS[layout]
    x, mix = _batch(hwc, N, H, W), am.augmix_tables(width, 1.0, SEED)
    for names in OP_LISTS:
        ops = am.augmix_op_table(names)
        launch, logs = _Launch(gpu, x, hwc, width, depth, ops, mix), []
        for step in (3, 2 ** 32 + 5):   # two steps on the same buffers
            got, log = launch(step)
            want, wlog = _spec(x, hwc, step, width, depth, ops, mix)
            assert np.array_equal(log, wlog), (names, step)
            assert np.array_equal(got, want), (names, step, np.argwhere(got != want)[:4])
            logs.append(log)
        assert not np.array_equal(logs[0], logs[1]), names
        if names == "Identity":
            assert np.array_equal(got, x)


@pytest.mark.parametrize("layout", ["chw32", "hwc24x40"])
def test_hand_made_entries_keep_or_replace_the_original(gpu, layout):
    hwc, N, H, W = LAYOUTS[layout]
    x, ops = _batch(hwc, N, H, W), am.augmix_op_table("Rotate,Solarize")
    mix = np.array([[100, 56, 100, 0], [0, 256, 0, 65536]], dtype=np.int32)
    got, log = _Launch(gpu, x, hwc, 3, 2, ops, mix)(1)
    want, wlog = _spec(x, hwc, 1, 3, 2, ops, mix)
    assert np.array_equal(log, wlog) and np.array_equal(got, want)
    entry = log[:, 0, 0, 1]
    assert set(entry.tolist()) == {0, 1}   # the step was picked for this
    for n in range(N):   # m = 0: the original; m = 65536, one weight of 256: chain 1 alone
        alone = ra.randaug_image(x[n] if hwc else x[n].transpose(1, 2, 0),
                                 [tuple(p) for p in log[n, 1, 1:3]], ra.randaug_tables(9, H, W))
        other = alone if hwc else alone.transpose(2, 0, 1)
        assert np.array_equal(got[n], other if entry[n] else x[n]), n


def _engine(kind, gpu, N, overlap=False, **kw):
    g = torch.Generator().manual_seed(7)
    if overlap:
        kw.update(bucket_mb=0.05, comm=dtr.native().Comm.loopback(2.0))
    if kind == "cifar":
        rec = torch.randint(0, 256, (N, 3, 32, 32), generator=g, dtype=torch.uint8)
        eng = Engine(cifar_spec(8), N, weight_decay=2e-4, lr_schedule=cifar_lr_schedule(),
                     device=gpu, input_mode="cifar_u8", data_seed=SEED, seed=3, **kw)
    else:
        spec = imagenet_spec(0, num_classes=10, image_hw=64, block="bottleneck",
                             layers=[1, 1, 1, 1])
        rec = torch.randint(0, 256, (N, 64, 64, 3), generator=g, dtype=torch.uint8)
        eng = Engine(spec, N, weight_decay=1e-4, lr_schedule=imagenet_lr_schedule(),
                     device=gpu, input_mode="imagenet_u8", data_seed=SEED, seed=3, **kw)
    labels = torch.randint(0, 10, (N,), generator=g, dtype=torch.int32)
    eng.set_batch(rec, labels)
    return eng, rec.numpy(), labels


# kind, DTR_TUNE, N, graph, overlap, the input launch
PLANS = {"persistent": ("cifar", "persist=1", 4, False, False, "cifar_augment"),
         "graph": ("cifar", "persist=1", 4, True, False, "cifar_augment"),
         "per-layer-imagenet": ("imagenet", "persist=0", 2, False, False, "imagenet_u8_pack"),
         "overlap": ("cifar", "persist=1", 16, False, True, "cifar_augment")}


@pytest.mark.parametrize("plan", list(PLANS))
def test_engine_step_feeds_the_input_launch_the_augmix_batch(gpu, monkeypatch, plan):
    kind, tune, N, graph, overlap, feed = PLANS[plan]
    monkeypatch.setenv("DTR_TUNE", tune)
    eng, rec, labels = _engine(kind, gpu, N, overlap, augmix_width=3, use_graph=graph)
    zero = _engine(kind, gpu, N, overlap, augmix_width=0, augmix_depth=2, augmix_ops="Rotate")[0]
    off = _engine(kind, gpu, N, overlap)[0]
    assert eng.persist == (kind == "cifar") and eng.persist_overlap == overlap
    assert eng.augmix_state() is None
    assert zero.img_am is None and zero.augmix_mix is None and zero.augmix_acc is None
    assert zero.plan.names() == off.plan.names()
    names = eng.plan.names()
    i = names.index("augmix")
    assert names[i + 1] == feed and names[:i] + names[i + 1:] == off.plan.names()
    assert eng.plan.op_streams()[i] == 0 and (eng.augmix_acc is not None) == (kind == "imagenet")
    if overlap:
        assert eng.recorded.op_buffers[i] == {"input"}
    first = eng.capture(warmup=2) if graph else 0   # replays draw afresh from the step word
    assert (eng.graph is not None) == graph
    for _ in range(first):
        off.step()
    for step in range(first, first + 3):
        # `off`, fed the specification's batch, must hand its network the same input
        want, wlog = am.augmix_batch(rec, "chw" if kind == "cifar" else "hwc", SEED, step, 3)
        off.set_batch(torch.from_numpy(want), labels)
        eng.step()
        off.step()
        torch.cuda.synchronize()
        assert not eng.persist_error() and not off.persist_error()
        assert torch.equal(eng.x_in.view(torch.int16), off.x_in.view(torch.int16)), step
        assert np.array_equal(eng.img_am.cpu().numpy(), want), step
        assert np.array_equal(eng.augmix_state(), wlog), step
    draw = am.augmix_draw(SEED, first + 2, 0, 3, -1, am.augmix_op_table())
    assert np.array_equal(eng.augmix_state()[0], am.augmix_log(draw))
    assert eng.metrics()["augmix"] == "w3-s3"


@pytest.mark.parametrize("mode,hw", [("cifar_resident", 32), ("nhwc", 32), ("cifar_u8", 40)])
def test_engine_refuses_input_modes_without_a_32x32_or_hwc_uint8_batch(gpu, mode, hw):
    with pytest.raises(ValueError, match="augmix_width"):
        Engine(cifar_spec(8, image_hw=hw), 4, weight_decay=2e-4,
               lr_schedule=cifar_lr_schedule(), device=gpu, input_mode=mode, augmix_width=3)
