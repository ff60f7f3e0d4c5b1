"""Label smoothing and top-5 precision on the device: every loss head (softmax_xent's
single-workgroup and row-parallel kernels, head_fused, the persistent forward's head and
the two folds) against the fp64 definitions of tests/xent_oracle.py, then through the
engine's three training plans and its two eval plans.

Op-level logits are randint(-32, 33) / 8, exact in fp32, so order and ties are exact and
the counts are compared exactly.  The tolerances are test_head_pool_xent's.  The
constructed top-5 rows of test_label_smoothing_cpu.py are appended to every batch; the two
of them with z[y] = inf / nan make the batch loss nan by definition, so they take part in
the top-5 count (`full` call) and the loss / gradient comparisons run on the batch without
them (`finite` call)."""
import numpy as np
import pytest
import torch
import xent_oracle as xo
from test_label_smoothing_cpu import tie_rows

import distributed_tensorflow_resnet_amd as dtr
from distributed_tensorflow_resnet_amd.models.params import ParamStore
from distributed_tensorflow_resnet_amd.models.resnet_torch import TorchResNet
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.ops import functional as fn
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SHAPES = [(5, 10, 16), (6, 100, 112), (7, 1000, -(-1000 // 16) * 16)]   # VPL 1, 4, 16


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _batch(N, K, ld, gpu, finite):
    g = torch.Generator().manual_seed(1000 * N + K)
    z = torch.randint(-32, 33, (N, K), generator=g).float() / 8
    y = torch.randint(0, K, (N,), generator=g)
    # top-1: row 0's label is its maximum; rows 1 and 2 have a tied maximum at classes 3 and
    # K - 2, labelled with the second (not the first argmax) and with the first
    y[0] = int(z[0].numpy().argmax())
    z[1:3, 3] = z[1:3, K - 2] = 5.0
    y[1], y[2] = K - 2, 3
    tz, ty, _ = tie_rows(K)
    if finite:
        keep = np.isfinite(tz).all(axis=1)
        tz, ty = tz[keep], ty[keep]
    z = torch.cat([z, torch.from_numpy(tz)])
    y = torch.cat([y, torch.from_numpy(ty)])
    logits = torch.zeros(z.shape[0], ld)
    logits[:, :K] = z
    return logits.to(gpu), y.to(gpu), z.numpy(), y.numpy()


def _native_xent(logits, labels, K, gs, extra, use_ws=True):
    """softmax_xent through the binding itself.  extra = () is the call as it was written
    before the smoothing arguments existed; (eps, topk) adds them.  Without a workspace the
    single-workgroup kernel runs.  Returns the outputs (and the workspace) as a dict."""
    nat, dev = dtr.native(required=True), logits.device
    N, ld = logits.shape
    o = {"loss": torch.zeros(1, device=dev), "correct": torch.zeros(1, device=dev),
         "dlogits": torch.empty((N, ld), device=dev, dtype=BF), "dbias": torch.empty(K, device=dev),
         "probs": torch.zeros((N, ld), device=dev), "topk": torch.zeros(1, device=dev),
         "ws": torch.zeros(nat.softmax_xent_ws_floats(N, ld), device=dev)}
    lab = labels.to(torch.int32).contiguous()
    args = [logits.data_ptr(), ld, lab.data_ptr(), N, K, o["loss"].data_ptr(),
            o["correct"].data_ptr(), o["dlogits"].data_ptr(), o["dbias"].data_ptr(), gs,
            o["probs"].data_ptr(), o["ws"].data_ptr() if use_ws else 0]
    if extra:
        args += [extra[0], extra[1], o["topk"].data_ptr()]
    nat.softmax_xent(*args, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return o


def _check_against_oracle(o, z, y, K, ld, eps):
    n = z.shape[0]
    rows, p, grad = xo.smoothed_xent(z, y, eps)
    top1 = float((z.argmax(axis=1) == y).sum())   # np.argmax: the first maximum
    top5 = float(xo.in_top_k(z, y, 5).sum())
    got = {k: v.item() for k, v in o.items() if k in ("loss", "correct", "topk")}
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
    assert torch.all(o["probs"][:, K:] == 0)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("N,K,ld", SHAPES)
def test_softmax_xent_rows_matches_fp64(gpu, N, K, ld, eps):
    logits, labels, z, y = _batch(N, K, ld, gpu, finite=True)
    assert logits.shape[0] % 4 != 0   # a partial last workgroup of the 4-rows-per-group kernel
    o = _native_xent(logits, labels, K, 1.0 / z.shape[0], (eps, 5))
    _check_against_oracle(o, z, y, K, ld, eps)
    # the inf / nan rows: only the counts are defined
    logits, labels, z, y = _batch(N, K, ld, gpu, finite=False)
    o = _native_xent(logits, labels, K, 1.0 / z.shape[0], (eps, 5))
    assert o["topk"].item() == float(xo.in_top_k(z, y, 5).sum())
    # ops.functional: the sixth element appears with topk > 0 only
    out = fn.softmax_xent(logits, labels, K, 1.0, label_smoothing=eps, topk=5)
    assert len(out) == 6 and out[5].item() == o["topk"].item()
    assert len(fn.softmax_xent(logits, labels, K, 1.0, label_smoothing=eps)) == 5


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_softmax_xent_single_workgroup_matches_fp64(gpu, eps):
    """No workspace: softmax_xent() dispatches to softmax_xent_kernel (one workgroup)."""
    N, K, ld = SHAPES[0]
    logits, labels, z, y = _batch(N, K, ld, gpu, finite=True)
    o = _native_xent(logits, labels, K, 1.0 / z.shape[0], (eps, 5), use_ws=False)
    _check_against_oracle(o, z, y, K, ld, eps)
    logits, labels, z, y = _batch(N, K, ld, gpu, finite=False)
    o = _native_xent(logits, labels, K, 1.0 / z.shape[0], (eps, 5), use_ws=False)
    assert o["topk"].item() == float(xo.in_top_k(z, y, 5).sum())


@pytest.mark.parametrize("use_ws", [True, False])
@pytest.mark.parametrize("N,K,ld", SHAPES)
def test_zero_smoothing_is_bitwise_the_plain_call(gpu, N, K, ld, use_ws):
    """Loss, correct count, dlogits, workspace rows, dbias and probs at smoothing 0 (with the
    top-5 count on) against the call without the new arguments."""
    logits, labels, z, _ = _batch(N, K, ld, gpu, finite=True)
    n = z.shape[0]
    old = _native_xent(logits, labels, K, 1.0 / n, (), use_ws)
    new = _native_xent(logits, labels, K, 1.0 / n, (0.0, 5), use_ws)
    for k in ("loss", "correct", "dlogits", "dbias", "probs"):
        assert torch.equal(old[k], new[k]), k
    assert torch.equal(old["ws"][:n * ld + 2 * n], new["ws"][:n * ld + 2 * n])
    assert not old["ws"][n * ld + 2 * n:].any()   # without topk the flag column is not written
    plain = fn.softmax_xent(logits, labels, K, 1.0 / n, want_probs=True)
    if use_ws:
        for a, k in zip(plain, ("loss", "correct", "dlogits", "dbias", "probs")):
            assert torch.equal(a, old[k]), k


def test_binding_rejects_bad_arguments(gpu):
    logits, labels, z, _ = _batch(5, 10, 16, gpu, finite=True)
    for extra in ((1.0, 5), (-0.1, 5), (0.1, -1)):
        with pytest.raises(ValueError):
            _native_xent(logits, labels, 10, 1.0, extra)


# ---- engine ----------------------------------------------------------------------------
N_ENG = 16
PLANS = {"unfused": "persist=0,fused_head=0", "head_fused": "persist=0,fused_head=1",
         "persistent4": "persist=1,persist_slices=4", "persistent1": "persist=1,persist_slices=1"}


def _engine(monkeypatch, gpu, tune, spec=None, N=N_ENG, **kw):
    monkeypatch.setenv("DTR_TUNE", tune)
    spec = spec or cifar_spec(8)
    eng = Engine(spec, N, weight_decay=2e-4, lr_schedule=cifar_lr_schedule(), device=gpu,
                 input_mode="nhwc", use_graph=False, **kw)
    g = torch.Generator().manual_seed(0)
    imgs = torch.randn(N, spec.image_h, spec.image_w, 3, generator=g).to(BF).float().to(gpu)
    labels = torch.randint(0, spec.num_classes, (N,), generator=g).to(gpu)
    eng.set_batch(imgs, labels)
    return eng, imgs, labels


@pytest.mark.parametrize("plan", list(PLANS))
def test_engine_smoothed_step_matches_autograd(gpu, monkeypatch, plan):
    eps, N, K = 0.1, N_ENG, 10
    eng, imgs, labels = _engine(monkeypatch, gpu, PLANS[plan], label_smoothing=eps)
    assert eng.persist == plan.startswith("persistent")
    if eng.persist:
        assert eng.prn.P == int(plan[-1])
    else:
        assert eng._head_fused == (plan == "head_fused")
    store = ParamStore(eng.spec, device=gpu)
    store.master.copy_(eng.params.master)
    store.stats.copy_(eng.params.stats)
    eng.forward_backward(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not eng.persist_error()
    model = TorchResNet(eng.spec, store, emulate_bf16=True)
    xent, _ = model.loss(model(imgs, True), labels, 2e-4, label_smoothing=eps)
    xent.backward()
    xent, g_ref = xent.item(), store.master.grad.detach()
    g_err = _rel(eng.grad, g_ref)
    print(f"{plan}: loss/N {eng.scalars[0].item() / N:.5f} vs {xent:.5f}, gradient rel {g_err:.3e}")
    assert abs(eng.scalars[0].item() / N - xent) < 1e-2 * max(1.0, xent)
    assert g_err < 5e-2
    # top-5: in_top_k of the engine's own logits; the fused and persistent heads keep none,
    # so their order is read from p_c = ws[i][c] / grad_scale + t_c (monotone in z_c)
    y = labels.cpu().numpy()
    kp = eng.kpad
    ws = eng.xent_ws.double().cpu().numpy()
    flags = ws[N * kp + 2 * N:N * kp + 3 * N]
    if plan == "unfused":
        order = eng.logits[:, :K].double().cpu().numpy()
        keep = np.ones(N, dtype=bool)
    else:
        t = np.full((N, K), eps / K)
        t[np.arange(N), y] += 1.0 - eps
        order = ws[:N * kp].reshape(N, kp)[:, :K] * eng.global_batch + t
        py = order[np.arange(N), y][:, None]
        near = np.abs(order - py) <= 1e-5 * np.abs(py)
        near[np.arange(N), y] = False
        keep = ~near.any(axis=1)
    print(f"{plan}: rows left out {int((~keep).sum())}, top-5 count {eng.scalars[5].item()}")
    assert (~keep).sum() <= 1
    want = xo.in_top_k(order, y, 5)
    assert (flags[keep] == want[keep]).all()
    assert set(flags.tolist()) <= {0.0, 1.0}
    assert eng.scalars[5].item() == flags.sum()
    m = eng.metrics(reduce=False, top5=True)
    assert m["precision_top5"] == flags.sum() / N and m["precision"] <= m["precision_top5"]
    assert set(m) - set(eng.metrics(reduce=False)) == {"precision_top5"}


@pytest.mark.parametrize("tune", ["persist=0", "persist=1"])
def test_engine_zero_smoothing_is_bitwise_the_default(gpu, monkeypatch, tune):
    res = []
    for kw in ({}, {"label_smoothing": 0.0}):
        eng, _, _ = _engine(monkeypatch, gpu, tune, **kw)
        for _ in range(3):
            eng.step()
        torch.cuda.synchronize()
        assert not eng.persist_error()
        res.append((eng.params.master.clone(), eng.mom.clone(), eng.params.stats.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("persist", [False, True])
@pytest.mark.parametrize("classes", [10, 100])
def test_eval_plans_top5_and_unsmoothed_loss(gpu, monkeypatch, classes, persist):
    """Both eval plans, attached to a training engine built with smoothing 0.1."""
    spec = cifar_spec(8, num_classes=classes)
    eng, imgs, labels = _engine(monkeypatch, gpu, "", spec=spec, N=8, label_smoothing=0.1)
    ev = eng.build_eval_plan(8, persist=persist)
    assert ev.kind == ("persistent" if persist else "per-layer")
    loss, correct, probs = ev.run(imgs, labels, raw_u8=False)
    torch.cuda.synchronize()
    z = ev.logits[:, :classes].double().cpu().numpy()
    y = labels.cpu().numpy()
    plain, _, _ = xo.smoothed_xent(z, y, 0.0)
    smooth, _, _ = xo.smoothed_xent(z, y, 0.1)
    print(f"classes {classes} persist {persist}: loss/n {loss / 8:.6f}, unsmoothed "
          f"{plain.mean():.6f}, smoothed {smooth.mean():.6f}, top5 {ev.top5}")
    assert abs(loss / 8 - plain.mean()) < 1e-4
    assert abs(smooth.mean() - plain.mean()) > 1e-3
    assert ev.top5 == float(xo.in_top_k(z, y, 5).sum())
    assert correct == float((z.argmax(axis=1) == y).sum())
