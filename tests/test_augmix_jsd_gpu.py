"""AugMix's Jensen-Shannon loss on the device: every `_jsd` row producer against the fp64 oracle
on the same logits, the fan-out launch against data/augmix.py, engine steps on every plan.
Bounds (profiles/augmix_jsd.md): 4 x the fp32 torch implementation's worst error against the
oracle (1.35e-7 on a loss relative to max(1, |loss|), 4.0e-6 on N x gradient); bf16 dlogits add
half a bf16 ulp.  Where the logits are the head's own fp32 dot products (head_fused, the engine)
the oracle reads them recomputed in fp64, and a first-order term for their rounding is added:
|dz| <= 64 * 2^-24 * sum |pooled * w|."""
import jsd_oracle as jo
import numpy as np
import pytest
import torch
from test_augmix_jsd_cpu import KINDS, W, triples

import distributed_tensorflow_resnet_amd as dtr
from distributed_tensorflow_resnet_amd.data.augmix import (augmix_fanout, augmix_op_table,
                                                           augmix_tables)
from distributed_tensorflow_resnet_amd.data.randaug import randaug_tables
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
LOSS_TOL, GRAD_TOL = 4 * 1.35e-7, 4 * 4.0e-6
SHAPES = [(1, 10), (2, 10), (5, 100), (3, 1000)]
C, HW = 64, 64   # head_fused's head
OFF = (0, 0, 0, 0.0, 1.0, 0, 0.0)   # the trailing arguments with every option off


def _xent(z, y, K, eps, tail, use_ws):
    # [N, K] logits, padded as the engine pads them; labels [B] or [N]
    nat, dev, N, ld = dtr.native(required=True), torch.device("cuda", 0), len(z), (K + 15) // 16 * 16
    z = torch.cat([z, torch.full((N, ld - K), 7.0)], 1).contiguous().to(dev)
    y = torch.cat([y, torch.full((N - len(y),), -5)]).to(torch.int32).to(dev)
    o = {k: torch.zeros(n, device=dev) for k, n in (("loss", 1), ("correct", 1), ("dbias", K), ("topk", 1))}
    o["dlogits"] = torch.empty((N, ld), device=dev, dtype=BF)
    o["ws"] = torch.zeros(nat.softmax_xent_ws_floats(N, ld), device=dev)
    nat.softmax_xent(z.data_ptr(), ld, y.data_ptr(), N, K, o["loss"].data_ptr(),
                     o["correct"].data_ptr(), o["dlogits"].data_ptr(), o["dbias"].data_ptr(),
                     1.0 / N, 0, o["ws"].data_ptr() if use_ws else 0, eps, 5, o["topk"].data_ptr(),
                     *tail, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {k: v for k, v in o.items() if use_ws or k != "ws"}


def _logits(pooled, w, bias):
    # fp64 logits of bf16 pooled features and dense weights, and the bound dz on their fp32 sums
    pw = pooled.double()[:, :, None] * w.double()[None]
    return (pw.sum(1) + bias.double()).cpu().numpy(), (64 * 2.0 ** -24 * pw.abs().sum(1)).cpu().numpy()


def _head_fused(B, K, kind, eps, tail, gpu):
    # unit-variance accumulators; spread: one logit of two views stands about 120 above the rest
    nat, N, ld = dtr.native(required=True), 3 * B, (K + 15) // 16 * 16
    g = torch.Generator().manual_seed(K + B)
    x, w = torch.randn(N, HW, C, generator=g), torch.zeros(C, ld)
    w[:, :K] = torch.randint(-4, 5, (C, K), generator=g).float() / 8
    if kind == "identical":
        x = x[:B].repeat(3, 1, 1)
    if kind == "spread":
        x[0, :, 0], x[B, :, 1], w[0, 1], w[1, 2] = 10.0, 10.0, 12.0, 12.0
    bias = torch.randint(-8, 9, (K,), generator=g).float() / 8
    y = torch.randint(0, K, (N,), generator=g).to(torch.int32).to(gpu)
    rep = max(nat.bn_acc_rep(), nat.prn_acc_rep())
    acc = torch.zeros(rep, 2, C, dtype=torch.float64)
    acc[0, 1] = N * HW   # mean 0, variance 1
    x, w, bias, acc = x.to(BF).to(gpu), w.to(BF).to(gpu), bias.to(gpu), acc.to(gpu)
    bn = [acc, torch.ones(C, device=gpu)] + [torch.zeros(C, device=gpu) for _ in range(7)]
    o = {"pooled": torch.zeros((N, C), device=gpu, dtype=BF), "dlogits": x.new_empty((N, ld)),
         "ws": torch.zeros(nat.softmax_xent_ws_floats(N, ld), device=gpu),
         "dact": torch.zeros((N, HW, C), device=gpu, dtype=BF), "bacc": torch.zeros_like(acc)}
    nat.head_fused(x.data_ptr(), [t.data_ptr() for t in bn], 0.997, 1e-5, 0, w.data_ptr(),
                   bias.data_ptr(), y.data_ptr(), [N, HW, C, K, ld], 1.0 / N,
                   [t.data_ptr() for t in o.values()], eps, 5, *tail,
                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o["z"], o["dz"] = _logits(o["pooled"], w[:, :K], bias)
    return o, y.cpu().numpy()


def _check(o, r, K, dz=None):
    # per-row loss, flags (exact) and gradient rows of a producer's outputs against oracle r
    N, ld = o["dlogits"].shape
    first = np.zeros(N)   # first order in dz: a clean row's loss moves by sum N |g| dz of its triple
    zerr = 0.0   # ... and |d (N g_ic) / dz| <= (3 + 5 w) p_ic summed over the triple's logits
    if dz is not None:
        first = np.tile((np.abs(r["grad"]) * N * dz).sum(1).reshape(3, -1).sum(0), 3)
        zerr = (3 + 5 * W) * r["p"] * dz.max() / N
    lbound, lerr, gerr = LOSS_TOL * np.maximum(1, np.abs(r["loss"])) + first, 0.0, 0.0
    if "ws" in o:
        rs = o["ws"][N * ld:N * ld + 2 * N].view(N, 2).double().cpu().numpy()
        rk = o["ws"][N * ld + 2 * N:N * ld + 3 * N].double().cpu().numpy()
        assert (rs[:, 1] == r["top1"]).all() and (rk == r["topk"]).all()
        lerr = (np.abs(rs[:, 0] - r["loss"]) / lbound).max()
        g32 = o["ws"][:N * ld].view(N, ld)[:, :K].double().cpu().numpy()
        gerr = (np.abs(g32 - r["grad"]) / (GRAD_TOL / N + zerr)).max()
    if "loss" in o:
        assert o["correct"].item() == r["top1"].sum() and o["topk"].item() == r["topk"].sum()
        assert abs(o["loss"].item() - r["loss"].sum()) <= lbound[:N // 3].sum()
    dl = o["dlogits"].double().cpu().numpy()
    assert np.isfinite(dl).all() and (dl[:, K:] == 0).all()
    g = np.abs(r["grad"])
    half_ulp = np.where(g > 0, 2.0 ** (np.floor(np.log2(np.maximum(g, 1e-300))) - 8), 0.0)
    derr = (np.abs(dl[:, :K] - r["grad"]) / (GRAD_TOL / N + half_ulp + zerr)).max()
    print(f"ratio to bound: row loss {lerr:.3f}, fp32 grad {gerr:.3f}, dlogits {derr:.3f}")
    assert max(lerr, gerr, derr) <= 1


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("producer,B,K", [(p, B, K) for p in ("rows", "single", "head_fused")
                                          for B, K in SHAPES if p != "head_fused" or K <= 64])
def test_producers_match_the_oracle(gpu, producer, B, K, kind, eps):
    if producer == "head_fused":
        o, y = _head_fused(B, K, kind, eps, OFF[:5] + (B, W), gpu)
        assert kind != "spread" or (torch.softmax(torch.from_numpy(o["z"]).float(), 1) == 0).any()
        _check({k: o[k] for k in ("ws", "dlogits")}, jo.jsd_head(o["z"], y, B, W, eps), K, o["dz"])
        return
    z, y = triples(B, K, kind)
    o = _xent(z, y, K, eps, OFF[:5] + (B, W), use_ws=producer == "rows")
    _check(o, jo.jsd_head(z.numpy(), y.numpy(), B, W, eps), K)
    if kind == "identical":   # JSD 0: the clean gradient is the hard one, the views' is 0
        hard = jo.jsd_head(z.numpy(), y.numpy(), B, 0.0, eps)["loss"]
        assert abs(o["loss"].item() - hard.sum()) <= \
            (LOSS_TOL * np.maximum(1, hard[:B])).sum() + B * 3 * W * LOSS_TOL
        assert o["dlogits"][B:].float().abs().max().item() <= GRAD_TOL / (3 * B)


@pytest.mark.parametrize("producer", ["rows", "single"])
def test_other_triples_are_untouched(gpu, producer):
    z, y = triples(2, 10, "random")
    z2 = z.clone()
    z2[[1, 3, 5]] += torch.randn(3, 10, generator=torch.Generator().manual_seed(9))   # triple 1
    a, b = (_xent(v, y, 10, 0.1, OFF[:5] + (2, W), producer == "rows") for v in (z, z2))
    rows = lambda t: t.view(-1)[:96].view(6, 16)[[0, 2, 4]]   # noqa: E731  (triple 0's gradient rows)
    assert torch.equal(rows(a["dlogits"]), rows(b["dlogits"])) and not torch.equal(a["dlogits"], b["dlogits"])
    if producer == "rows":   # the fp32 rows, then {loss, top-1} per row
        assert torch.equal(rows(a["ws"]), rows(b["ws"]))
        assert torch.equal(a["ws"][96:108].view(6, 2)[[0, 2, 4]], b["ws"][96:108].view(6, 2)[[0, 2, 4]])


@pytest.mark.parametrize("producer", ["rows", "single", "head_fused"])
def test_without_jsd_the_call_is_bitwise_the_old_one(gpu, producer):
    if producer == "head_fused":
        old, new = (_head_fused(2, 10, "random", 0.1, t, gpu)[0] for t in ((), OFF))
    else:
        z, y = triples(2, 10, "random")
        old, new = (_xent(z, y.repeat(3), 10, 0.1, t, producer == "rows") for t in ((), OFF))
    for k in old:
        if k not in ("z", "dz"):
            assert torch.equal(old[k], new[k]), k


@pytest.mark.parametrize("layout,B,H,Wd", [("chw", 1, 32, 32), ("chw", 3, 32, 32),
                                           ("hwc", 3, 16, 24), ("hwc", 1, 224, 224)])
def test_fanout_is_the_specification(gpu, layout, B, H, Wd):
    nat, N, width, seed, step = dtr.native(required=True), 3 * B, 2, 5, 11
    rng, shape = np.random.default_rng(B + H), (B, 3, H, Wd) if layout == "chw" else (B, H, Wd, 3)
    x, y = rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 10, B).astype(np.int32)
    tables, mix = randaug_tables(9, H, Wd), augmix_tables(width, 1.0, seed)
    want, wlab, wlog = augmix_fanout(x, y, layout, seed, step, width, tables=tables, mix_table=mix)
    xin, tab, mixd = (torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (x, tables, mix))
    out = torch.zeros((N,) + shape[1:], dtype=torch.uint8, device=gpu)
    labels = torch.from_numpy(np.concatenate([y, np.full(2 * B, -1, np.int32)])).to(gpu)
    log = torch.zeros((N, width, 4, 2), dtype=torch.int32, device=gpu)
    acc, gstep = torch.zeros((N, 3 * H * Wd), dtype=torch.int16, device=gpu), torch.tensor([step], device=gpu)
    nat.augmix(xin.data_ptr(), out.data_ptr(), N, H, Wd, int(layout == "hwc"), seed,
               gstep.data_ptr(), width, -1, tab.data_ptr(), tab.numel(), mixd.data_ptr(),
               mixd.numel(), [int(i) for i in augmix_op_table()], acc.data_ptr(), log.data_ptr(),
               B, labels.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == w).all() for t, w in ((out, want), (labels, wlab), (log, wlog)))


@pytest.mark.parametrize("dense_scale", [1.0, 256.0])
def test_engine_step_on_every_plan(gpu, monkeypatch, dense_scale):
    # dense_scale 256 spreads the logits until some p_ic underflow to 0 on every plan's head
    B, K, eps, losses = 2, 10, 0.1, {}
    g, labels = torch.Generator().manual_seed(0), torch.tensor([3, 8])
    imgs = torch.randint(0, 256, (B, 3, 32, 32), generator=g, dtype=torch.uint8)
    for plan, tune in (("persistent", "persist=1"), ("head_fused", "persist=0,fused_head=1"),
                       ("unfused", "persist=0,fused_head=0")):
        monkeypatch.setenv("DTR_TUNE", tune)
        eng = Engine(cifar_spec(8), B, weight_decay=2e-4, lr_schedule=cifar_lr_schedule(), device=gpu,
                     use_graph=False, label_smoothing=eps, augmix_width=2, augmix_jsd=True)
        assert eng.N == 3 * B and eng.persist == (plan == "persistent"), eng.persist_reason
        assert eng.persist or eng._head_fused == (plan == "head_fused")
        eng.params.view("dense/kernel").mul_(dense_scale)
        eng.repack()
        eng.set_batch(imgs, labels)
        eng.forward_backward(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert not eng.persist_error()
        want, wlab, _ = augmix_fanout(imgs.numpy(), labels.numpy(), "chw", eng.data_seed, 0, 2)
        assert (eng.img_am.cpu().numpy() == want).all() and (eng.labels.cpu().numpy() == wlab).all()
        zs, dz = _logits(eng.pooled, eng.params.view("dense/kernel").to(BF), eng.params.view("dense/bias"))
        assert bool((torch.softmax(torch.from_numpy(zs).float(), 1) == 0).any()) == (dense_scale > 1)
        o = {"dlogits": eng.dlogits.view(3 * B, eng.kpad), "loss": eng.scalars[0:1],
             "correct": eng.scalars[1:2], "topk": eng.scalars[5:6]}
        _check(o, jo.jsd_head(zs, labels.numpy(), B, 12.0, eps), K, dz)
        m = losses[plan] = eng.metrics(reduce=False)
        assert m["augmix"] == "w2-s3-jsd12"
    v = [m["cross_entropy"] for m in losses.values()]
    print(v)   # bf16 activations, rounded differently per path: 2^-10 relative
    assert dense_scale > 1 or max(v) - min(v) <= 1e-3 * max(v)
