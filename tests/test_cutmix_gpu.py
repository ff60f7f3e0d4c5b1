"""CutMix on the device: the three mixed input launches (cifar_augment,
cifar_augment_resident, imagenet_u8_pack) at their third arity against the host specification
data.cifar.cutmix_draw, re-derived in tests/cutmix_oracle.py, and against their own unmixed
output -- a pasted image is bit for bit a composition of two unmixed ones -- and the engine's
plans (per-layer, fused head, persistent) against autograd, the two-label fp64 row oracle,
resume and graph replay.

The steps of every case are chosen by evaluating the specification on the host, and the choice
is asserted: a box clipped at a border, a strictly interior one, an empty one (lam exactly 1)
and one with odd ch / cw are all among them."""
import functools

import numpy as np
import pytest
import torch
import cutmix_oracle as co
import mixup_oracle as mo

import distributed_tensorflow_resnet_amd as dtr
from distributed_tensorflow_resnet_amd.data import cifar
from distributed_tensorflow_resnet_amd.models.params import ParamStore
from distributed_tensorflow_resnet_amd.models.resnet_torch import TorchResNet
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.train.backends import GPUBackend
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule
from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SEED, KEY_SEED = 4321, 11
ONE, HALF = 2 ** 24, 2 ** 23
TABLE = [0.25, 0.75, 0.5, 0.125, 0.875, 0.375, 0.625]   # the fp32 lam table; exact in fp32
CUTS = [(0, 0), (32, 32), (16, 16), (9, 20), (1, 1), (31, 5), (32, 1)]    # (ch, cw), 32 x 32
CUTS_IMNET = [(0, 0), (12, 20), (6, 10), (5, 9), (1, 1), (11, 3), (12, 1)]   # 12 x 20
BIG_STEP = 2 ** 32 + 3


def _entries(cuts):
    return [co.entry(ch, cw) for ch, cw in cuts]


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _records(n, seed=0):
    """Random CIFAR-shaped records + labels (host, shared, never modified)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (n, 3, 32, 32), generator=g, dtype=torch.uint8),
            torch.randint(0, 10, (n,), generator=g, dtype=torch.int32))


@functools.lru_cache(maxsize=None)
def _case_steps(N, H, W, cuts):
    """Steps whose CutMix draw (thresh 2^24) is of each kind, found on the host: the first
    step of every kind, and a step past 2^32.  -> sorted steps; the kinds are asserted."""
    entries = _entries(cuts)
    kinds = {}
    for step in range(4000):
        d = co.draw(SEED, step, N, len(entries), H, W, entries, ONE)
        ch, cw = cuts[d["index"]]
        full = (2 * (ch // 2)) * (2 * (cw // 2))
        if (ch, cw) == (0, 0):
            assert d["area"] == 0 and d["lam"] == np.float32(1.0)
            kinds.setdefault("empty", step)
        if 0 < d["area"] < full:
            kinds.setdefault("clipped", step)
        if d["area"] > 0 and d["y0"] > 0 and d["y1"] < H and d["x0"] > 0 and d["x1"] < W:
            assert d["area"] == full
            kinds.setdefault("interior", step)
        if d["area"] > 0 and (ch % 2 or cw % 2):
            kinds.setdefault("odd", step)
        if float(d["lam"]) != (H * W - d["area"]) / (H * W):
            kinds.setdefault("rounded", step)    # the fp32 quotient is not exact
    assert {"empty", "clipped", "interior", "odd"} <= set(kinds), kinds
    if H * W & (H * W - 1):
        assert "rounded" in kinds
    return tuple(sorted(set(kinds.values()) | {BIG_STEP}))


class _Mix:
    """The side buffers of one mixed input launch, with the CutMix ones."""

    def __init__(self, table, cuts, N, gpu):
        self.table = torch.tensor(table, dtype=torch.float32, device=gpu)
        self.labels_b = torch.full((N,), -7, dtype=torch.int32, device=gpu)
        self.lam = torch.full((N,), -7.0, device=gpu)
        self.log = torch.full((2,), -7, dtype=torch.int32, device=gpu)
        self.cut_table = torch.tensor(_entries(cuts), dtype=torch.int32, device=gpu)
        self.cut_log = torch.full((8,), -7, dtype=torch.int32, device=gpu)

    def mix_args(self, *labels):
        return (self.table.data_ptr(), self.table.numel(), *labels, self.labels_b.data_ptr(),
                self.lam.data_ptr(), self.log.data_ptr())

    def args(self, thresh, *labels):
        return (*self.mix_args(*labels), self.cut_table.data_ptr(), thresh,
                self.cut_log.data_ptr())


def _gstep(step, gpu):
    return torch.tensor([step], dtype=torch.int64, device=gpu)


def _check_side_outputs(mix, labels, step, N, H, W, cuts, thresh):
    """mix_lam, labels_b, mix_log and cut_log against the specification -> (draw, partner)."""
    entries = _entries(cuts)
    d = cifar.cutmix_draw(SEED, step, N, len(entries), H, W, entries, thresh)
    want = co.draw(SEED, step, N, len(entries), H, W, entries, thresh)
    assert all(d[k] == v for k, v in want.items()), step
    assert mix.log.tolist() == [d["index"], d["shift"]], step
    partner = (np.arange(N) + d["shift"]) % N
    assert mix.labels_b.tolist() == labels.cpu().numpy()[partner].tolist(), step
    if d["cut"]:
        assert mix.cut_log.tolist() == [1, d["y0"], d["y1"], d["x0"], d["x1"], d["area"],
                                        d["cy"], d["cx"]], step
        lam = d["lam"]
    else:
        assert mix.cut_log.tolist() == [0] * 8, step
        lam = np.float32(TABLE[d["index"]])
    # bit-equal: the one correctly rounded fp32 quotient
    assert mix.lam.cpu().numpy().view(np.int32).tolist() == \
        [int(np.float32(lam).view(np.int32))] * N, step
    return d, partner


def _pasted(plain, d):
    """The composition of the unmixed launch's bits [N, H, W, C] the CutMix step must equal."""
    return torch.from_numpy(co.paste(_bits(plain).cpu().numpy(), d["shift"],
                                     (d["y0"], d["y1"], d["x0"], d["x1"])))


# ---------------------------------------------------------------- 1. input ops
def _augment(gpu, img, labels, step, thresh=None, mixup=False, hw=32, train=1, cut_table=True):
    """cifar_augment: the old arity, the mixup arity or (thresh given) the CutMix arity."""
    nat, N = dtr.native(required=True), img.shape[0]
    out = torch.full((N, hw, hw, 8), 7.0, dtype=BF, device=gpu)
    crops = torch.zeros((N, 3), dtype=torch.int32, device=gpu)
    mix = _Mix(TABLE, CUTS, N, gpu)
    extra = ()
    if thresh is not None:
        extra = list(mix.args(thresh, labels.data_ptr()))
        if not cut_table:
            extra[-3] = 0
    elif mixup:
        extra = mix.mix_args(labels.data_ptr())
    nat.cifar_augment(img.data_ptr(), out.data_ptr(), N, hw, hw, 8, 4, SEED,
                      _gstep(step, gpu).data_ptr(), train, crops.data_ptr(), 0, 0, *extra, _st())
    torch.cuda.synchronize()
    return out, crops, mix


def test_cifar_augment_cutmix(gpu):
    N = 5
    img, labels = (t.to(gpu) for t in _records(N))
    for step in _case_steps(N, 32, 32, tuple(CUTS)):
        plain, crops, _ = _augment(gpu, img, labels, step)
        cut, crops_c, mix = _augment(gpu, img, labels, step, ONE)
        d, partner = _check_side_outputs(mix, labels, step, N, 32, 32, CUTS, ONE)
        assert d["cut"] and torch.equal(crops, crops_c)
        # outside the box the unmixed bits of n, inside those of the partner
        assert torch.equal(_bits(cut).cpu(), _pasted(plain, d)), step
        assert torch.all(cut[..., 3:] == 0)
        if d["area"] == 0:
            assert torch.equal(_bits(cut), _bits(plain)) and mix.lam.tolist() == [1.0] * N
        # thresh 0 through the new arity is the mixup arity's launch
        off, _, mix0 = _augment(gpu, img, labels, step, 0)
        blend, _, mix1 = _augment(gpu, img, labels, step, mixup=True)
        assert torch.equal(_bits(off), _bits(blend)), step
        assert torch.equal(mix0.lam, mix1.lam) and torch.equal(mix0.log, mix1.log)
        assert torch.equal(mix0.labels_b, mix1.labels_b)
        assert mix0.cut_log.tolist() == [-7] * 8    # not the CutMix kernel: never written


def test_cifar_augment_switches_per_step(gpu):
    N = 5
    img, labels = (t.to(gpu) for t in _records(N))
    entries = _entries(CUTS)
    modes = [co.draw(SEED, s, N, 7, 32, 32, entries, HALF)["cut"] for s in range(64)]
    steps = ([s for s in range(64) if modes[s]][:4] + [s for s in range(64) if not modes[s]][:4])
    assert len(steps) == 8   # four steps of either mode
    for step in sorted(steps):
        out, _, mix = _augment(gpu, img, labels, step, HALF)
        d, partner = _check_side_outputs(mix, labels, step, N, 32, 32, CUTS, HALF)
        assert d["cut"] == modes[step]
        if d["cut"]:
            plain, _, _ = _augment(gpu, img, labels, step)
            assert torch.equal(_bits(out).cpu(), _pasted(plain, d)), step
        else:   # today's mixup launch, bit for bit
            blend, _, _ = _augment(gpu, img, labels, step, mixup=True)
            assert torch.equal(_bits(out), _bits(blend)), step


def test_refusals(gpu):
    img, labels = (t.to(gpu) for t in _records(3))
    _augment(gpu, img, labels, 0, ONE)
    with pytest.raises(ValueError):   # evaluation never pastes
        _augment(gpu, img, labels, 0, ONE, train=0)
    with pytest.raises(ValueError):   # a threshold without a table
        _augment(gpu, img, labels, 0, ONE, cut_table=False)
    _augment(gpu, img, labels, 0, 0, cut_table=False)   # threshold 0: no table needed
    for bad in (-1, ONE + 1):
        with pytest.raises(ValueError):
            _augment(gpu, img, labels, 0, bad)
    g = torch.Generator().manual_seed(1)
    img16 = torch.randint(0, 256, (3, 3, 16, 16), generator=g, dtype=torch.uint8).to(gpu)
    _augment(gpu, img16, labels, 0, hw=16)   # unmixed: the generic kernel runs
    with pytest.raises(ValueError):
        _augment(gpu, img16, labels, 0, ONE, hw=16)
    # the mixup arguments are still needed (labels_b, mix_lam)
    nat, mix = dtr.native(required=True), _Mix(TABLE, CUTS, 3, gpu)
    out = torch.empty((3, 32, 32, 8), dtype=BF, device=gpu)
    with pytest.raises(ValueError):
        nat.cifar_augment(img.data_ptr(), out.data_ptr(), 3, 32, 32, 8, 4, SEED, 0, 1, 0, 0, 0,
                          0, 0, 0, 0, 0, 0, mix.cut_table.data_ptr(), ONE, 0, _st())
    rec, lab = (t.to(gpu) for t in _records(64, seed=2))
    with pytest.raises(ValueError):
        _resident(gpu, rec, lab, 0, 0, 1, ONE, train=0)
    with pytest.raises(ValueError):
        _resident(gpu, rec, lab, 0, 0, 1, ONE, cut_table=False)
    img8 = torch.zeros((3, 12, 20, 3), dtype=torch.uint8, device=gpu)
    out8 = torch.empty((3, 12, 20, 8), dtype=BF, device=gpu)
    mixi = _Mix(TABLE, CUTS_IMNET, 3, gpu)
    for train, args in ((0, mixi.args(ONE, labels.data_ptr())),
                        (1, (*mixi.mix_args(labels.data_ptr()), 0, ONE, 0))):
        with pytest.raises(ValueError):
            nat.imagenet_u8_pack(img8.data_ptr(), out8.data_ptr(), 3, 12, 20, SEED, 0, train, 0, 0,
                                 0, *args, _st())
    torch.cuda.synchronize()


def _resident(gpu, rec, lab, step, rank, world, thresh=None, mixup=False, N=5, train=1,
              cut_table=True):
    nat = dtr.native(required=True)
    out = torch.full((N, 32, 32, 8), 7.0, dtype=BF, device=gpu)
    labels = torch.zeros(N, dtype=torch.int32, device=gpu)
    idx = torch.zeros(N, dtype=torch.int32, device=gpu)
    mix = _Mix(TABLE, CUTS, N, gpu)
    extra = ()
    if thresh is not None:
        extra = list(mix.args(thresh))
        if not cut_table:
            extra[-3] = 0
    elif mixup:
        extra = mix.mix_args()
    nat.cifar_augment_resident(rec.data_ptr(), lab.data_ptr(), out.data_ptr(), labels.data_ptr(),
                               _gstep(step, gpu).data_ptr(), N, 32, 32, 8, rec.shape[0], rank,
                               world, 1, KEY_SEED, 4, SEED, train, 0, idx.data_ptr(), 0, 0,
                               *extra, _st())
    torch.cuda.synchronize()
    return out, labels, idx, mix


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_cifar_augment_resident_cutmix(gpu, rank, world):
    N, records = 5, 64
    rec, lab = (t.to(gpu) for t in _records(records, seed=2))
    for step in _case_steps(N, 32, 32, tuple(CUTS)):
        plain, labels, idx, _ = _resident(gpu, rec, lab, step, rank, world)
        want = cifar.resident_batch(KEY_SEED, step, N, records, rank, world)
        assert np.array_equal(idx.cpu().numpy(), want)
        cut, labels_c, idx_c, mix = _resident(gpu, rec, lab, step, rank, world, ONE)
        assert torch.equal(labels, labels_c) and torch.equal(idx, idx_c)
        d, partner = _check_side_outputs(mix, labels, step, N, 32, 32, CUTS, ONE)
        assert d["cut"]
        assert torch.equal(_bits(cut).cpu(), _pasted(plain, d)), step
        assert torch.all(cut[..., 3:] == 0)
        off, _, _, mix0 = _resident(gpu, rec, lab, step, rank, world, 0)
        blend, _, _, mix1 = _resident(gpu, rec, lab, step, rank, world, mixup=True)
        assert torch.equal(_bits(off), _bits(blend)), step
        assert torch.equal(mix0.lam, mix1.lam) and torch.equal(mix0.labels_b, mix1.labels_b)
    # switching: a mixup step is the mixup launch, a CutMix step the composition
    entries = _entries(CUTS)
    modes = [co.draw(SEED, s, N, 7, 32, 32, entries, HALF)["cut"] for s in range(8)]
    assert len(set(modes)) == 2
    for step in range(8):
        out, labels, _, mix = _resident(gpu, rec, lab, step, rank, world, HALF)
        d, _ = _check_side_outputs(mix, labels, step, N, 32, 32, CUTS, HALF)
        if d["cut"]:
            plain, _, _, _ = _resident(gpu, rec, lab, step, rank, world)
            assert torch.equal(_bits(out).cpu(), _pasted(plain, d)), step
        else:
            blend, _, _, _ = _resident(gpu, rec, lab, step, rank, world, mixup=True)
            assert torch.equal(_bits(out), _bits(blend)), step


@pytest.mark.parametrize("s2d", [0, 1])
def test_imagenet_u8_pack_cutmix(gpu, s2d):
    nat = dtr.native(required=True)
    N, H, W = 3, 12, 20   # H * W = 240: the lam quotient rounds
    g = torch.Generator().manual_seed(4)
    img = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).to(gpu)
    labels = torch.tensor([3, 1, 4], dtype=torch.int32, device=gpu)
    shape = (N, H // 2, W // 2, 16) if s2d else (N, H, W, 8)

    def run(step, thresh=None, mixup=False):
        out = torch.full(shape, 7.0, dtype=BF, device=gpu)
        mix = _Mix(TABLE, CUTS_IMNET, N, gpu)
        extra = (mix.args(thresh, labels.data_ptr()) if thresh is not None else
                 mix.mix_args(labels.data_ptr()) if mixup else ())
        nat.imagenet_u8_pack(img.data_ptr(), out.data_ptr(), N, H, W, SEED,
                             _gstep(step, gpu).data_ptr(), 1, 0, 0, s2d, *extra, _st())
        torch.cuda.synchronize()
        return out, mix

    def nhwc(out):   # either layout -> bf16 [N, H, W, 4] (channel 3 is padding)
        if s2d:
            return out.view(N, H // 2, W // 2, 2, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(N, H, W, 4)
        assert torch.all(out[..., 3:] == 0)
        return out[..., :4]

    steps = _case_steps(N, H, W, tuple(CUTS_IMNET))
    for step in steps:
        plain, _ = run(step)
        cut, mix = run(step, ONE)
        d, partner = _check_side_outputs(mix, labels, step, N, H, W, CUTS_IMNET, ONE)
        assert d["cut"]
        assert torch.equal(_bits(nhwc(cut)).cpu(), _pasted(nhwc(plain), d)), step
        assert torch.all(nhwc(cut)[..., 3] == 0)
        off, mix0 = run(step, 0)
        blend, mix1 = run(step, mixup=True)
        assert torch.equal(_bits(off), _bits(blend)), step
        assert torch.equal(mix0.lam, mix1.lam) and torch.equal(mix0.labels_b, mix1.labels_b)
    entries = _entries(CUTS_IMNET)
    modes = [co.draw(SEED, s, N, 7, H, W, entries, HALF)["cut"] for s in range(8)]
    assert len(set(modes)) == 2
    for step in range(8):
        out, mix = run(step, HALF)
        d, _ = _check_side_outputs(mix, labels, step, N, H, W, CUTS_IMNET, HALF)
        if d["cut"]:
            assert torch.equal(_bits(nhwc(out)).cpu(), _pasted(nhwc(run(step)[0]), d)), step
        else:
            assert torch.equal(_bits(out), _bits(run(step, mixup=True)[0])), step


# ---------------------------------------------------------------- 2. engine
PLANS = {"unfused": "persist=0,fused_head=0", "head_fused": "persist=0,fused_head=1",
         "persistent1": "persist=1,persist_slices=1", "persistent2": "persist=1,persist_slices=2",
         "persistent4": "persist=1,persist_slices=4"}
N_ENG = 4


def _engine(monkeypatch, gpu, tune, N=N_ENG, mode="cifar_u8", **kw):
    monkeypatch.setenv("DTR_TUNE", tune)
    kw.setdefault("use_graph", False)
    eng = Engine(cifar_spec(8), N, weight_decay=2e-4, lr_schedule=cifar_lr_schedule(), device=gpu,
                 input_mode=mode, data_seed=SEED, seed=3, **kw)
    if mode == "cifar_u8":
        eng.set_batch(*_records(N, seed=7))
    return eng


def _spec_state(step, N, mixup_alpha, cutmix_alpha, prob=0.5):
    """What Engine.mix_state() and the metrics must report for `step` -> (state, area)."""
    entries = cifar.cutmix_table(cutmix_alpha, SEED, 32, 32)
    thresh = cifar.cutmix_thresh(mixup_alpha, cutmix_alpha, prob)
    d = co.draw(SEED, step, N, len(entries), 32, 32, entries, thresh)
    if d["cut"]:
        return {"mode": "cutmix", "lam": float(d["lam"]), "shift": d["shift"],
                "box": (d["y0"], d["y1"], d["x0"], d["x1"])}, d["area"]
    lam = float(cifar.mixup_table(mixup_alpha, SEED)[d["index"]])
    return {"mode": "mixup", "lam": lam, "shift": d["shift"], "box": None}, None


@pytest.mark.parametrize("plan", list(PLANS))
def test_engine_cutmix_step_matches_autograd_and_oracle(gpu, monkeypatch, plan):
    """One CutMix step: the input is the paste of the unmixed launch's images, the head's rows
    are the two-label fp64 oracle's at the area-adjusted lam, and the gradient is fp32
    autograd's on the step's own pasted input (the mixup test's bound, 5e-2)."""
    N, K = N_ENG, 10
    eng = _engine(monkeypatch, gpu, PLANS[plan], cutmix_alpha=1.0)
    assert eng.persist == plan.startswith("persistent")
    if eng.persist:
        assert eng.prn.P == int(plan[-1])
    else:
        assert eng._head_fused == (plan == "head_fused")
    assert eng.cut_thresh == ONE and len(eng.mix_head_ptrs()) == 2
    want, area = _spec_state(0, N, 0.0, 1.0)
    assert want["mode"] == "cutmix" and 0 < area < 1024   # step 0 of this seed: a real box
    lam, shift = want["lam"], want["shift"]
    partner = (np.arange(N) + shift) % N
    ya = eng.labels.cpu().numpy().copy()
    eng.forward_backward(_st())
    torch.cuda.synchronize()
    assert not eng.persist_error()
    assert eng.mix_state() == want and eng.mixup_state() == (lam, shift)
    yb = eng.labels_b.cpu().numpy()
    assert yb.tolist() == ya[partner].tolist() and eng.mix_lam.tolist() == [lam] * N
    m = eng.metrics(reduce=False)
    assert (m["mixup_lam"], m["mix_mode"], m["cutmix_area"]) == (lam, 1, area)
    # the pasted input, bit for bit
    nat = dtr.native(required=True)
    plain = torch.empty_like(eng.x_in)
    nat.cifar_augment(eng.img_u8.data_ptr(), plain.data_ptr(), N, 32, 32, 8, 4, SEED,
                      _gstep(0, gpu).data_ptr(), 1, 0, 0, 0, _st())
    torch.cuda.synchronize()
    d = dict(zip(("y0", "y1", "x0", "x1"), want["box"]), shift=shift)
    assert torch.equal(_bits(eng.x_in).cpu(), _pasted(plain, d))
    assert not torch.equal(_bits(eng.x_in), _bits(plain))
    # head rows vs the oracle, from the head's own pooled features
    s = eng.params.slot("dense/kernel")
    w = eng.params.master[s.offset:s.offset + s.numel].view(s.shape).to(BF).double().cpu()
    b = eng.params.master[eng.params.slot("dense/bias").offset:][:K].double().cpu()
    z = (eng.pooled.double().cpu() @ w + b).numpy()
    rows, _, grad = mo.mixed_xent(z, ya, yb, lam, 0.0)
    kp = eng.kpad
    ws = eng.xent_ws.double().cpu().numpy()
    np.testing.assert_allclose(ws[N * kp:N * kp + 2 * N].reshape(N, 2)[:, 0], rows,
                               rtol=1e-4, atol=1e-4)
    assert abs(eng.scalars[0].item() / N - rows.mean()) < 1e-4
    assert _rel(eng.dlogits[:, :K], grad / eng.global_batch) < 1e-2
    # the whole step against autograd on the pasted input
    store = ParamStore(eng.spec, device=gpu)
    store.master.copy_(eng.params.master)
    store.stats.copy_(eng.params.stats)
    model = TorchResNet(eng.spec, store, emulate_bf16=True)
    x = eng.x_in[..., :3].float()
    xent, _ = model.loss(model(x, True), torch.from_numpy(ya).to(gpu), 2e-4,
                         labels_b=torch.from_numpy(yb).to(gpu), lam=lam)
    xent.backward()
    g_err = _rel(eng.grad, store.master.grad.detach())
    print(f"{plan}: loss/N {eng.scalars[0].item() / N:.5f} vs {xent.item():.5f}, gradient rel "
          f"{g_err:.3e}")
    assert abs(eng.scalars[0].item() / N - xent.item()) < 1e-2 * max(1.0, xent.item())
    assert g_err < 5e-2


def _state(eng):
    torch.cuda.synchronize()
    assert not eng.persist_error()
    return {"master": eng.params.master.clone(), "mom": eng.mom.clone(),
            "stats": eng.params.stats.clone(), "gstep": eng.gstep.clone()}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("mixup", [0.0, 0.2])
@pytest.mark.parametrize("tune", ["persist=0", "persist=1"])
def test_engine_zero_cutmix_alpha_is_bitwise_the_default(gpu, monkeypatch, tune, mixup):
    res = []
    for kw in ({}, {"cutmix_alpha": 0.0, "mix_switch_prob": 0.5}, {"cutmix_alpha": 1.0}):
        eng = _engine(monkeypatch, gpu, tune, mixup_alpha=mixup, **kw)
        assert eng.persist == (tune == "persist=1")
        assert (eng.cut_table is None) == (not kw.get("cutmix_alpha"))
        assert (eng.mix_table is None) == (not mixup and not kw.get("cutmix_alpha"))
        for _ in range(3):
            eng.step()
        res.append(_state(eng))
        m = eng.metrics(reduce=False)
        assert ("mix_mode" in m) == (eng.mix_table is not None) == (eng.mix_state() is not None)
        if not kw.get("cutmix_alpha"):
            assert "cutmix_area" not in m and m.get("mix_mode", 0) == 0
    assert _same(res[0], res[1])
    assert not _same(res[0], res[2])   # and pasting is visible in the weights


def _resident_engine(monkeypatch, gpu, **kw):
    return _engine(monkeypatch, gpu, "persist=1", N=8, mode="cifar_resident",
                   resident=_records(64, seed=2), shuffle_seed=KEY_SEED, mixup_alpha=0.2,
                   cutmix_alpha=1.0, mix_switch_prob=0.5, **kw)


def test_resident_cutmix_resume_and_determinism(gpu, monkeypatch, tmp_path):
    want_states = [_spec_state(s, 8, 0.2, 1.0) for s in range(6)]
    assert {w["mode"] for w, _ in want_states} == {"mixup", "cutmix"}   # these six steps switch
    straight, twin = _resident_engine(monkeypatch, gpu), _resident_engine(monkeypatch, gpu)
    for step in range(6):
        straight.step()
        twin.step()
        st, area = want_states[step]
        assert straight.mix_state() == st
        m = straight.metrics(reduce=False)
        assert m["mixup_lam"] == st["lam"] and m["mix_mode"] == int(st["mode"] == "cutmix")
        assert m.get("cutmix_area") == area
    want = _state(straight)
    assert _same(_state(twin), want)                # two same-seed engines
    first = _resident_engine(monkeypatch, gpu)
    for _ in range(3):
        first.step()
    torch.cuda.synchronize()
    prefix = Saver(str(tmp_path)).save(GPUBackend(first).state_tensors(), 3)
    second = GPUBackend(_resident_engine(monkeypatch, gpu))
    second.load_state(Saver.restore(prefix))
    for _ in range(3):
        second.step()
    assert _same(_state(second.engine), want)       # resume continues the sequence
    assert second.mix_state() == want_states[-1][0]


def test_cutmix_under_graph_replay(gpu, monkeypatch):
    eager = _resident_engine(monkeypatch, gpu)
    for _ in range(6):
        eager.step()
    eng = _resident_engine(monkeypatch, gpu, use_graph=True)
    done = eng.capture(warmup=2)
    states = []
    for _ in range(6 - done):
        eng.step()
        states.append(eng.mix_state())
    assert eng.graph is not None
    assert _same(_state(eng), _state(eager))
    assert states == [_spec_state(s, 8, 0.2, 1.0)[0] for s in range(done, 6)]
    assert len({s["mode"] for s in states}) == 2   # both modes are replayed


def test_input_modes_without_an_input_launch_refuse_cutmix(gpu, monkeypatch):
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _engine(monkeypatch, gpu, "", cutmix_alpha=bad)
    with pytest.raises(ValueError):
        _engine(monkeypatch, gpu, "", cutmix_alpha=1.0, mixup_alpha=0.2, mix_switch_prob=1.5)
    with pytest.raises(ValueError, match="input launch"):
        _engine(monkeypatch, gpu, "", mode="nhwc", cutmix_alpha=1.0)
    _engine(monkeypatch, gpu, "", mode="nhwc", cutmix_alpha=0.0)
    # the eval plans never paste: built on a pasting engine, they score a batch as one without
    eng = _engine(monkeypatch, gpu, "", cutmix_alpha=1.0)
    plain = _engine(monkeypatch, gpu, "")
    x, y = _records(N_ENG, seed=7)
    a = eng.build_eval_plan(N_ENG).run(x, y)
    b = plain.build_eval_plan(N_ENG).run(x, y)
    assert a[0] == b[0] and a[1] == b[1]
