"""Mixup on the device: the input kernels (cifar_augment, cifar_augment_resident,
imagenet_u8_pack) against the host specification data.cifar.mixup_draw and against their own
unmixed output, every loss head against the fp64 definitions of tests/mixup_oracle.py, and
the engine's plans (per-layer, fused head, persistent) against autograd, resume and graph
replay.

Op-level logits are randint(-32, 33) / 8, exact in fp32, so order and ties are exact and the
counts are compared exactly; the tolerances are test_label_smoothing_gpu's for the same
kernels and outputs, the image bound is test_kernels_gpu.test_cifar_augment's."""
import functools

import numpy as np
import pytest
import torch
import mixup_oracle as mo
import xent_oracle as xo
from test_label_smoothing_cpu import tie_rows

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
STEPS = [0, 1, 7, 2 ** 32 + 3]
TABLE = [0.25, 0.75, 0.5, 0.125, 0.875, 0.375, 0.625]   # hand-made; exact in fp32
MEANS = torch.tensor([123.68, 116.78, 103.94])


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


class _Mix:
    """The side buffers of one mixed input launch."""

    def __init__(self, table, N, gpu):
        self.table = torch.tensor(table, dtype=torch.float32, device=gpu)
        self.labels_b = torch.full((N,), -7, dtype=torch.int32, device=gpu)
        self.lam = torch.full((N,), -7.0, device=gpu)
        self.log = torch.full((2,), -7, dtype=torch.int32, device=gpu)

    def args(self, *labels):
        return (self.table.data_ptr(), self.table.numel(), *labels, self.labels_b.data_ptr(),
                self.lam.data_ptr(), self.log.data_ptr())


def _gstep(step, gpu):
    return torch.tensor([step], dtype=torch.int64, device=gpu)


def _augment(gpu, img, labels, step, table=None, hw=32):
    """cifar_augment through the binding: old arity without a table.  -> (out, crops, mix)."""
    nat, N = dtr.native(required=True), img.shape[0]
    out = torch.full((N, hw, hw, 8), 7.0, dtype=BF, device=gpu)
    crops = torch.zeros((N, 3), dtype=torch.int32, device=gpu)
    mix = _Mix(table, N, gpu) if table is not None else None
    extra = mix.args(labels.data_ptr()) if mix else ()
    nat.cifar_augment(img.data_ptr(), out.data_ptr(), N, hw, hw, 8, 4, SEED,
                      _gstep(step, gpu).data_ptr(), 1, crops.data_ptr(), 0, 0, *extra, _st())
    torch.cuda.synchronize()
    return out, crops, mix


def _check_side_outputs(mix, labels, step, N, table):
    idx, shift = cifar.mixup_draw(SEED, step, N, len(table))
    assert mix.log.tolist() == [idx, shift], step
    partner = (np.arange(N) + shift) % N
    assert mix.labels_b.tolist() == labels.cpu().numpy()[partner].tolist(), step
    assert mix.lam.tolist() == [table[idx]] * N, step
    return partner, table[idx]


# ---------------------------------------------------------------- 1. input ops
def test_cifar_augment_mixup(gpu):
    N = 5
    img, labels = (t.to(gpu) for t in _records(N))
    for step in STEPS:
        plain, crops, _ = _augment(gpu, img, labels, step)
        # device == specification; the side outputs
        mixed, crops_m, mix = _augment(gpu, img, labels, step, TABLE)
        partner, lam = _check_side_outputs(mix, labels, step, N, TABLE)
        assert torch.equal(crops, crops_m)
        # lam = 1: the unmixed kernel's bits; lam = 0: the partner's unmixed bits
        ones, _, _ = _augment(gpu, img, labels, step, [1.0] * 7)
        assert torch.equal(_bits(ones), _bits(plain)), step
        zeros, _, _ = _augment(gpu, img, labels, step, [0.0] * 7)
        assert torch.equal(_bits(zeros), _bits(plain[torch.from_numpy(partner).to(gpu)])), step
        # lam = 0.3 against the fp32 host blend of augment_cpu's images of the same crops
        blend, _, _ = _augment(gpu, img, labels, step, [0.3] * 7)
        crop_u8 = torch.zeros(N, 3, 32, 32, dtype=torch.uint8)
        for n in range(N):
            oy, ox, flip = crops[n].tolist()
            padded = torch.zeros(3, 40, 40, dtype=torch.uint8)
            padded[:, 4:36, 4:36] = img[n].cpu()
            c = padded[:, oy:oy + 32, ox:ox + 32]
            crop_u8[n] = c.flip(2) if flip else c
        host = cifar.augment_cpu(crop_u8, train=False)
        lam3 = float(np.float32(0.3))
        for n in range(N):
            want = mo.blend(host[n].numpy(), host[partner[n]].numpy(), lam3)
            err = _rel(blend[n, :, :, :3], want)
            assert err < 1e-2, (step, n, err)
            assert torch.all(blend[n, :, :, 3:] == 0)
    # a null table is the old-arity call
    nat = dtr.native(required=True)
    out = torch.empty_like(plain)
    nat.cifar_augment(img.data_ptr(), out.data_ptr(), N, 32, 32, 8, 4, SEED,
                      _gstep(STEPS[-1], gpu).data_ptr(), 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, _st())
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(plain))


def test_generic_shape_kernel_refuses_mixup(gpu):
    g = torch.Generator().manual_seed(1)
    img = torch.randint(0, 256, (3, 3, 16, 16), generator=g, dtype=torch.uint8).to(gpu)
    labels = torch.zeros(3, dtype=torch.int32, device=gpu)
    _augment(gpu, img, labels, 0, hw=16)   # unmixed: the generic kernel runs
    with pytest.raises(ValueError):
        _augment(gpu, img, labels, 0, TABLE, hw=16)
    img32 = _records(3)[0].to(gpu)
    nat, mix = dtr.native(required=True), _Mix(TABLE, 3, gpu)
    out = torch.empty((3, 32, 32, 8), dtype=BF, device=gpu)
    for bad in ((mix.table.data_ptr(), 7, 0, mix.labels_b.data_ptr(), mix.lam.data_ptr(), 0),
                (mix.table.data_ptr(), 7, labels.data_ptr(), 0, mix.lam.data_ptr(), 0),
                (mix.table.data_ptr(), 0, labels.data_ptr(), mix.labels_b.data_ptr(),
                 mix.lam.data_ptr(), 0)):
        with pytest.raises(ValueError):
            nat.cifar_augment(img32.data_ptr(), out.data_ptr(), 3, 32, 32, 8, 4, SEED, 0, 1, 0, 0,
                              0, *bad, _st())


def _resident(gpu, rec, lab, step, rank, world, table=None, N=5):
    nat = dtr.native(required=True)
    out = torch.full((N, 32, 32, 8), 7.0, dtype=BF, device=gpu)
    labels = torch.zeros(N, dtype=torch.int32, device=gpu)
    idx = torch.zeros(N, dtype=torch.int32, device=gpu)
    mix = _Mix(table, N, gpu) if table is not None else None
    nat.cifar_augment_resident(rec.data_ptr(), lab.data_ptr(), out.data_ptr(), labels.data_ptr(),
                               _gstep(step, gpu).data_ptr(), N, 32, 32, 8, rec.shape[0], rank,
                               world, 1, KEY_SEED, 4, SEED, 1, 0, idx.data_ptr(), 0, 0,
                               *(mix.args() if mix else ()), _st())
    torch.cuda.synchronize()
    return out, labels, idx, mix


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_cifar_augment_resident_mixup(gpu, rank, world):
    N, records = 5, 64
    rec, lab = (t.to(gpu) for t in _records(records, seed=2))
    for step in STEPS:
        plain, labels, idx, _ = _resident(gpu, rec, lab, step, rank, world)
        want = cifar.resident_batch(KEY_SEED, step, N, records, rank, world)
        assert np.array_equal(idx.cpu().numpy(), want)
        mixed, labels_m, idx_m, mix = _resident(gpu, rec, lab, step, rank, world, TABLE)
        assert torch.equal(labels, labels_m) and torch.equal(idx, idx_m)
        partner, lam = _check_side_outputs(mix, labels, step, N, TABLE)
        ones, _, _, _ = _resident(gpu, rec, lab, step, rank, world, [1.0] * 7)
        assert torch.equal(_bits(ones), _bits(plain)), step
        # lam = 0 pins the partner's record and its crop / flip
        zeros, _, _, _ = _resident(gpu, rec, lab, step, rank, world, [0.0] * 7)
        assert torch.equal(_bits(zeros), _bits(plain[torch.from_numpy(partner).to(gpu)])), step
        # lam = 0.3: the blend of the two unmixed images, up to the inputs' own bf16 rounding
        blend, _, _, _ = _resident(gpu, rec, lab, step, rank, world, [0.3] * 7)
        lam3 = float(np.float32(0.3))
        pf = plain.float().cpu().numpy()
        err = _rel(blend, mo.blend(pf, pf[partner], lam3))
        assert err < 1e-2, (step, err)


@pytest.mark.parametrize("s2d", [0, 1])
def test_imagenet_u8_pack_mixup(gpu, s2d):
    nat = dtr.native(required=True)
    N, H, W = 3, 8, 8
    g = torch.Generator().manual_seed(4)
    img = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).to(gpu)
    labels = torch.tensor([3, 1, 4], dtype=torch.int32, device=gpu)
    shape = (N, H // 2, W // 2, 16) if s2d else (N, H, W, 8)

    def run(step, table=None, old_arity=False):
        out = torch.full(shape, 7.0, dtype=BF, device=gpu)
        mix = _Mix(table, N, gpu) if table is not None else None
        extra = mix.args(labels.data_ptr()) if mix else (() if old_arity else (0,) * 6)
        nat.imagenet_u8_pack(img.data_ptr(), out.data_ptr(), N, H, W, SEED,
                             _gstep(step, gpu).data_ptr(), 1, 0, 0, s2d, *extra, _st())
        torch.cuda.synchronize()
        return out, mix

    def nhwc3(out):   # either layout -> [N, H, W, 3] fp32 on the host
        o = out.float().cpu()
        if s2d:
            o = o.view(N, H // 2, W // 2, 2, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(N, H, W, 4)
        return o[..., :3]

    ref = img.float().cpu() - MEANS
    for step in STEPS:
        plain, _ = run(step, old_arity=True)
        assert torch.equal(_bits(run(step)[0]), _bits(plain))   # a null table
        mixed, mix = run(step, TABLE)
        partner, lam = _check_side_outputs(mix, labels, step, N, TABLE)
        ones, _ = run(step, [1.0] * 7)
        assert torch.equal(_bits(ones), _bits(plain)), step
        zeros, _ = run(step, [0.0] * 7)
        assert torch.equal(nhwc3(zeros), nhwc3(plain)[partner]), step
        # the fp32 images the kernel blends: the crop or its mirror image, by the unmixed output
        a = []
        for n in range(N):
            flipped = not torch.equal(nhwc3(plain)[n], ref[n].to(BF).float())
            a.append(ref[n].flip(1) if flipped else ref[n])
            assert torch.equal(nhwc3(plain)[n], a[n].to(BF).float())
        blend, _ = run(step, [0.3] * 7)
        lam3 = float(np.float32(0.3))
        for n in range(N):
            err = _rel(nhwc3(blend)[n], mo.blend(a[n].numpy(), a[partner[n]].numpy(), lam3))
            assert err < 1e-2, (step, n, err)
        if not s2d:
            assert torch.all(blend[..., 3:] == 0)


# ---------------------------------------------------------------- 2. loss heads
LAMS = [0.0, 0.3, 0.5, 1.0]
SHAPES = [(3, 10, 16), (5, 65, 80), (5, 1000, 1000)]   # VPL 1, 4 (classes % 64 = 1), 16


def _head_batch(N, K, ld, gpu, finite):
    g = torch.Generator().manual_seed(1000 * N + K)
    z = torch.randint(-32, 33, (N, K), generator=g).float() / 8
    ya = torch.randint(0, K, (N,), generator=g)
    tz, ty, _ = tie_rows(K)
    if finite:
        keep = np.isfinite(tz).all(axis=1)
        tz, ty = tz[keep], ty[keep]
    z = torch.cat([z, torch.from_numpy(tz)])
    ya = torch.cat([ya, torch.from_numpy(ty)])
    n = z.shape[0]
    yb = torch.randint(0, K, (n,), generator=g)
    yb[1] = ya[1]                                        # one row with ya == yb (lam 0.3)
    lam = torch.tensor([LAMS[i % 4] for i in range(n)])
    logits = torch.zeros(n, ld)
    logits[:, :K] = z
    return logits.to(gpu), ya.to(gpu), yb.to(gpu), lam.to(gpu), z.numpy()


def _native_xent(logits, ya, K, gs, extra, mix=None, use_ws=True):
    nat, dev = dtr.native(required=True), logits.device
    N, ld = logits.shape
    o = {"loss": torch.zeros(1, device=dev), "correct": torch.zeros(1, device=dev),
         "dlogits": torch.empty((N, ld), device=dev, dtype=BF), "dbias": torch.empty(K, device=dev),
         "probs": torch.zeros((N, ld), device=dev), "topk": torch.zeros(1, device=dev),
         "ws": torch.zeros(nat.softmax_xent_ws_floats(N, ld), device=dev)}
    keep = [ya.to(torch.int32).contiguous()]
    args = [logits.data_ptr(), ld, keep[0].data_ptr(), N, K, o["loss"].data_ptr(),
            o["correct"].data_ptr(), o["dlogits"].data_ptr(), o["dbias"].data_ptr(), gs,
            o["probs"].data_ptr(), o["ws"].data_ptr() if use_ws else 0,
            extra[0], extra[1], o["topk"].data_ptr()]
    if mix is not None:
        keep += [mix[0].to(torch.int32).contiguous(), mix[1].float().contiguous()]
        args += [keep[1].data_ptr(), keep[2].data_ptr()]
    nat.softmax_xent(*args, _st())
    torch.cuda.synchronize()
    return o


def _check_head(o, plain, z, ya, yb, lam, K, ld, eps, use_ws):
    n = z.shape[0]
    ya, yb, lam = ya.cpu().numpy(), yb.cpu().numpy(), lam.cpu().numpy().astype(np.float64)
    rows, p, grad = mo.mixed_xent(z, ya, yb, lam, eps)
    yd = mo.dominant(ya, yb, lam)
    top1 = float((z.argmax(axis=1) == yd).sum())
    top5 = float(xo.in_top_k(z, yd, 5).sum())
    got = {k: o[k].item() for k in ("loss", "correct", "topk")}
    dl_err = _rel(o["dlogits"][:, :K], grad / n)
    print(f"K={K} eps={eps}: loss/n {got['loss'] / n:.7f} vs {rows.mean():.7f}, top1 "
          f"{got['correct']} vs {top1}, top5 {got['topk']} vs {top5}, dlogits rel {dl_err:.2e}")
    assert got["correct"] == top1
    assert got["topk"] == top5
    assert abs(got["loss"] / n - rows.mean()) < 1e-4
    assert dl_err < 1e-2
    assert torch.all(o["dlogits"][:, K:] == 0)
    np.testing.assert_allclose(o["dbias"].cpu().numpy(), (grad / n).sum(axis=0), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(o["probs"][:, :K].cpu().numpy(), p, rtol=1e-4, atol=1e-6)
    # rows with lam == 1 are the plain call's rows, bit for bit
    one = torch.from_numpy(lam == 1.0).to(o["dlogits"].device)
    assert one.any() and not one.all()
    assert torch.equal(_bits(o["dlogits"][one]), _bits(plain["dlogits"][one]))
    assert torch.equal(o["probs"], plain["probs"])
    if use_ws:
        g_rows = lambda d: d["ws"][:n * ld].view(n, ld)   # noqa: E731
        per_row = lambda d: d["ws"][n * ld:n * ld + 2 * n].view(n, 2)   # noqa: E731
        assert torch.equal(g_rows(o)[one], g_rows(plain)[one])
        assert torch.equal(per_row(o)[one], per_row(plain)[one])
        np.testing.assert_allclose(per_row(o)[:, 0].cpu().numpy(), rows, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("N,K,ld", SHAPES)
def test_softmax_xent_rows_mixup_matches_fp64(gpu, N, K, ld, eps):
    logits, ya, yb, lam, z = _head_batch(N, K, ld, gpu, finite=True)
    gs = 1.0 / z.shape[0]
    o = _native_xent(logits, ya, K, gs, (eps, 5), (yb, lam))
    plain = _native_xent(logits, ya, K, gs, (eps, 5))
    _check_head(o, plain, z, ya, yb, lam, K, ld, eps, True)
    # the inf / nan rows: only the counts are defined
    logits, ya, yb, lam, z = _head_batch(N, K, ld, gpu, finite=False)
    o = _native_xent(logits, ya, K, gs, (eps, 5), (yb, lam))
    yd = mo.dominant(ya.cpu().numpy(), yb.cpu().numpy(), lam.cpu().numpy())
    assert o["topk"].item() == float(xo.in_top_k(z, yd, 5).sum())
    # null mix pointers are the call without them; one of the two alone is refused
    zero = torch.zeros(z.shape[0], device=gpu)
    with pytest.raises(ValueError):
        dtr.native(required=True).softmax_xent(
            logits.data_ptr(), ld, zero.data_ptr(), z.shape[0], K, 0, 0, 0, 0, gs, 0, 0, eps, 0, 0,
            zero.data_ptr(), 0, _st())


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_softmax_xent_single_workgroup_mixup_matches_fp64(gpu, eps):
    N, K, ld = 5, 10, 16
    logits, ya, yb, lam, z = _head_batch(N, K, ld, gpu, finite=True)
    gs = 1.0 / z.shape[0]
    o = _native_xent(logits, ya, K, gs, (eps, 5), (yb, lam), use_ws=False)
    plain = _native_xent(logits, ya, K, gs, (eps, 5), use_ws=False)
    _check_head(o, plain, z, ya, yb, lam, K, ld, eps, False)


# ---------------------------------------------------------------- 3. engine
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


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("plan", list(PLANS))
def test_engine_mixed_step_matches_autograd_and_oracle(gpu, monkeypatch, plan, eps):
    """One mixed step: the gradient against fp32 autograd on the blended input the step's own
    input launch produced and the two-label loss (test_engine_smoothed_step_matches_autograd's
    bounds), and the head's rows against the fp64 oracle on the logits of its pooled features,
    at every lam of LAMS (the table is overwritten in place; the draw's index is any)."""
    N, K = N_ENG, 10
    eng = _engine(monkeypatch, gpu, PLANS[plan], label_smoothing=eps, mixup_alpha=0.2)
    assert eng.persist == plan.startswith("persistent")
    if eng.persist:
        assert eng.prn.P == int(plan[-1])
    else:
        assert eng._head_fused == (plan == "head_fused")
    idx, shift = cifar.mixup_draw(SEED, 0, N, eng.mix_table.numel())
    partner = (np.arange(N) + shift) % N
    ya = eng.labels.cpu().numpy().copy()
    ya[partner[0]] = ya[0]                   # one row with ya == yb
    eng.labels.copy_(torch.from_numpy(ya))
    s = eng.params.slot("dense/kernel")
    for lam in LAMS + [None]:                # None: the table's own value
        if lam is not None:
            eng.mix_table.fill_(lam)
            lam = float(np.float32(lam))         # the value the device holds
        else:
            eng.mix_table.copy_(torch.from_numpy(cifar.mixup_table(0.2, SEED)))
            lam = float(eng.mix_table[idx].item())
        eng.forward_backward(_st())
        torch.cuda.synchronize()
        assert not eng.persist_error()
        assert eng.mixup_state() == (lam, shift)
        yb = eng.labels_b.cpu().numpy()
        assert yb.tolist() == ya[partner].tolist() and eng.mix_lam.tolist() == [lam] * N
        # head rows vs the oracle, from the head's own pooled features
        w = eng.params.master[s.offset:s.offset + s.numel].view(s.shape).to(BF).double().cpu()
        b = eng.params.master[eng.params.slot("dense/bias").offset:][:K].double().cpu()
        z = (eng.pooled.double().cpu() @ w + b).numpy()
        rows, _, grad = mo.mixed_xent(z, ya, yb, lam, eps)
        kp = eng.kpad
        ws = eng.xent_ws.double().cpu().numpy()
        np.testing.assert_allclose(ws[N * kp:N * kp + 2 * N].reshape(N, 2)[:, 0], rows,
                                   rtol=1e-4, atol=1e-4)
        assert abs(eng.scalars[0].item() / N - rows.mean()) < 1e-4
        dl_err = _rel(eng.dlogits[:, :K], grad / eng.global_batch)
        yd = mo.dominant(ya, yb, lam)
        print(f"{plan} lam={lam}: loss/N {eng.scalars[0].item() / N:.6f} vs {rows.mean():.6f}, "
              f"dlogits rel {dl_err:.2e}")
        assert dl_err < 1e-2
        srt = np.sort(z, axis=1)
        if (srt[:, -1] - srt[:, -2]).min() > 1e-3:   # top-1 of the dominant label (no near tie)
            assert eng.scalars[1].item() == float((z.argmax(axis=1) == yd).sum())
    # the whole step against autograd (lam: the table's own value)
    store = ParamStore(eng.spec, device=gpu)
    store.master.copy_(eng.params.master)
    store.stats.copy_(eng.params.stats)
    model = TorchResNet(eng.spec, store, emulate_bf16=True)
    x = eng.x_in[..., :3].float()
    xent, _ = model.loss(model(x, True), torch.from_numpy(ya).to(gpu), 2e-4, label_smoothing=eps,
                         labels_b=torch.from_numpy(yb).to(gpu), lam=lam)
    xent.backward()
    g_err = _rel(eng.grad, store.master.grad.detach())
    print(f"{plan}: loss/N {eng.scalars[0].item() / N:.5f} vs {xent.item():.5f}, gradient rel "
          f"{g_err:.3e}")
    assert abs(eng.scalars[0].item() / N - xent.item()) < 1e-2 * max(1.0, xent.item())
    assert g_err < 5e-2
    assert eng.metrics(reduce=False)["mixup_lam"] == lam
    # the blended input is the blend of the unmixed launch's images
    plain, _, _ = _augment(gpu, eng.img_u8, eng.labels, 0)
    pf = plain.float().cpu().numpy()
    assert _rel(eng.x_in, mo.blend(pf, pf[partner], lam)) < 1e-2


def _state(eng):
    torch.cuda.synchronize()
    assert not eng.persist_error()
    return {"master": eng.params.master.clone(), "mom": eng.mom.clone(),
            "stats": eng.params.stats.clone(), "gstep": eng.gstep.clone()}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("tune", ["persist=0", "persist=1"])
def test_engine_zero_alpha_is_bitwise_the_default(gpu, monkeypatch, tune):
    res = []
    for kw in ({}, {"mixup_alpha": 0.0}, {"mixup_alpha": 0.2}):
        eng = _engine(monkeypatch, gpu, tune, **kw)
        assert (eng.mix_table is None) == (not kw.get("mixup_alpha"))
        for _ in range(3):
            eng.step()
        res.append(_state(eng))
        assert ("mixup_lam" in eng.metrics(reduce=False)) == bool(kw.get("mixup_alpha"))
        assert (eng.mixup_state() is None) == (not kw.get("mixup_alpha"))
    assert _same(res[0], res[1])
    assert not _same(res[0], res[2])   # and mixing is visible in the weights


def _resident_engine(monkeypatch, gpu, **kw):
    return _engine(monkeypatch, gpu, "persist=1", N=8, mode="cifar_resident",
                   resident=_records(64, seed=2), shuffle_seed=KEY_SEED, mixup_alpha=0.2, **kw)


def test_resident_mixup_resume_and_determinism(gpu, monkeypatch, tmp_path):
    straight = _resident_engine(monkeypatch, gpu)
    lams = []
    for _ in range(6):
        straight.step()
        lams.append(straight.mixup_state())
    want = _state(straight)
    table = cifar.mixup_table(0.2, SEED)
    draws = [cifar.mixup_draw(SEED, s, 8, len(table)) for s in range(6)]
    assert lams == [(float(table[i]), sh) for i, sh in draws]
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
    assert second.engine.mixup_state() == lams[-1]


def test_mixup_under_graph_replay(gpu, monkeypatch):
    eager = _resident_engine(monkeypatch, gpu)
    for _ in range(6):
        eager.step()
    eng = _resident_engine(monkeypatch, gpu, use_graph=True)
    done = eng.capture(warmup=2)
    lams = []
    for _ in range(6 - done):
        eng.step()
        lams.append(eng.metrics(reduce=False)["mixup_lam"])
    assert eng.graph is not None
    assert _same(_state(eng), _state(eager))
    table = cifar.mixup_table(0.2, SEED)
    assert lams == [float(table[cifar.mixup_draw(SEED, s, 8, len(table))[0]])
                    for s in range(done, 6)]
    assert len(set(lams)) > 1   # a fresh draw in every replay


def test_input_modes_without_an_input_launch_refuse_mixup(gpu, monkeypatch):
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _engine(monkeypatch, gpu, "", mixup_alpha=bad)
    with pytest.raises(ValueError, match="input launch"):
        _engine(monkeypatch, gpu, "", mode="nhwc", mixup_alpha=0.2)
    _engine(monkeypatch, gpu, "", mode="nhwc", mixup_alpha=0.0)
    # the eval plans never mix: built on a mixing engine, they score a batch as one without
    eng = _engine(monkeypatch, gpu, "", mixup_alpha=0.2)
    plain = _engine(monkeypatch, gpu, "")
    x, y = _records(N_ENG, seed=7)
    a = eng.build_eval_plan(N_ENG).run(x, y)
    b = plain.build_eval_plan(N_ENG).run(x, y)
    assert a[0] == b[0] and a[1] == b[1]
