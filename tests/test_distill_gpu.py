"""Knowledge distillation on the device: every row producer that takes a teacher row
(softmax_xent's row-parallel and single-workgroup kernels, head_fused, and through the
engine the persistent forward's head) against the fp64 rows and the derived bounds of
tests/distill_oracle.py; rows without a teacher against the calls as they were, bit for bit;
and the engine's teacher launch against the teacher's own inference plan.

Row 1's teacher and row 2's student have one logit about 80 above the rest, so some q_c
(p_tau_c) underflow to 0.  Worst observed ratios to the bound: profiles/distill.md."""
import distill_oracle as do
import numpy as np
import pytest
import torch
import xent_oracle as xo
from test_distill_cpu import rows

import distributed_tensorflow_resnet_amd as dtr
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule
from distributed_tensorflow_resnet_amd.train.evaluator import GPUInference

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
N = 5          # not a multiple of the 4 rows a workgroup of the row-parallel kernel owns
C, HW = 64, 64   # head_fused's head
SHAPES = {10: 16, 64: 64, 100: 112}   # classes -> kpad
PRODUCERS = [(p, K) for K in SHAPES for p in ("rows", "single", "head_fused")
             if p != "head_fused" or SHAPES[K] <= 64]
VARIANTS = {"plain": (0.0, 1.0), "smooth_mixed": (0.1, 0.3)}   # eps, lam (yb != y)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _rows(K, ld, gpu):
    z, t, y, yb = rows(N, K)
    pad = lambda a: torch.cat([a, torch.full((N, ld - K), 7.0)], 1).contiguous().to(gpu)  # noqa: E731
    return pad(z), pad(t), y.to(torch.int32).to(gpu), yb.to(torch.int32).to(gpu)


def _tail(mix, kd):
    """The ops' trailing arguments: () as before mixup, the mixup pair, or pair + teacher."""
    if kd is None:
        return list(mix) if mix else []
    return list(mix or (0, 0)) + [kd[0].data_ptr() if kd[0] is not None else 0, kd[1], kd[2]]


def _xent(z, y, K, eps, mix, kd, use_ws):
    nat, dev = dtr.native(required=True), z.device
    ld = z.shape[1]
    o = {"loss": torch.zeros(1, device=dev), "correct": torch.zeros(1, device=dev),
         "dlogits": torch.empty((N, ld), device=dev, dtype=BF), "dbias": torch.empty(K, device=dev),
         "topk": torch.zeros(1, device=dev),
         "ws": torch.zeros(nat.softmax_xent_ws_floats(N, ld), device=dev)}
    nat.softmax_xent(z.data_ptr(), ld, y.data_ptr(), N, K, o["loss"].data_ptr(),
                     o["correct"].data_ptr(), o["dlogits"].data_ptr(), o["dbias"].data_ptr(),
                     1.0 / N, 0, o["ws"].data_ptr() if use_ws else 0, eps, 5, o["topk"].data_ptr(),
                     *_tail(mix, kd), _st())
    torch.cuda.synchronize()
    o["z"] = z[:, :K].double().cpu().numpy()
    if not use_ws:
        del o["ws"]
    return o


def _head_fused(zrows, y, K, eps, mix, kd):
    """head_fused at C = 64, HW = 64: unit-variance accumulators, image 2's channel 0 and the
    dense weight [0][K - 2] raised so that its logit K - 2 stands about 80 above the rest.
    The student logits are recomputed in fp64 from the bf16 pooled features it writes."""
    nat, dev = dtr.native(required=True), zrows.device
    ld = zrows.shape[1]
    g = torch.Generator().manual_seed(K + 1)
    x = torch.randn(N, HW, C, generator=g)
    x[2, :, 0] = 10.0
    w = torch.zeros(C, ld)
    w[:, :K] = torch.randint(-4, 5, (C, K), generator=g).float() / 8
    w[0, K - 2] = 8.0
    bias = torch.randint(-8, 9, (K,), generator=g).float() / 8
    rep = max(nat.bn_acc_rep(), nat.prn_acc_rep())
    acc = torch.zeros(rep, 2, C, dtype=torch.float64)
    acc[0, 1] = N * HW   # mean 0, variance 1
    x, w, bias, acc = x.to(BF).to(dev), w.to(BF).to(dev), bias.to(dev), acc.to(dev)
    ones, zeros = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    st = [torch.zeros(C, device=dev) for _ in range(6)]   # mmean, mvar, mean, rstd, scale, shift
    o = {"pooled": torch.zeros((N, C), device=dev, dtype=BF),
         "dlogits": torch.empty((N, ld), device=dev, dtype=BF),
         "ws": torch.zeros(nat.softmax_xent_ws_floats(N, ld), device=dev),
         "dact": torch.zeros((N, HW, C), device=dev, dtype=BF),
         "bacc": torch.zeros(rep, 2, C, dtype=torch.float64, device=dev)}
    nat.head_fused(x.data_ptr(), [acc.data_ptr(), ones.data_ptr(), zeros.data_ptr()] +
                   [s.data_ptr() for s in st], 0.997, 1e-5, 0, w.data_ptr(), bias.data_ptr(),
                   y.data_ptr(), [N, HW, C, K, ld], 1.0 / N,
                   [o[k].data_ptr() for k in ("pooled", "dlogits", "ws", "dact", "bacc")],
                   eps, 5, *_tail(mix, kd), _st())
    torch.cuda.synchronize()
    o["z"] = (o["pooled"].double() @ w[:, :K].double() + bias.double()).cpu().numpy()
    rs = o["ws"][N * ld:N * ld + 2 * N].view(N, 2)
    o["loss"], o["correct"] = rs[:, 0].sum().view(1), rs[:, 1].sum().view(1)
    o["topk"] = o["ws"][N * ld + 2 * N:N * ld + 3 * N].sum().view(1)
    return o


def _produce(producer, z, y, K, eps, mix, kd):
    if producer == "head_fused":
        return _head_fused(z, y, K, eps, mix, kd)
    return _xent(z, y, K, eps, mix, kd, use_ws=producer == "rows")


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("alpha", [0.3, 1.0])
@pytest.mark.parametrize("tau", [1.0, 4.0])
@pytest.mark.parametrize("producer,K", PRODUCERS)
def test_rows_match_fp64(gpu, producer, K, tau, alpha, variant):
    ld = SHAPES[K]
    eps, lam = VARIANTS[variant]
    z, t, y, yb = _rows(K, ld, gpu)
    lamv = torch.full((N,), lam, device=gpu)
    mix = None if lam == 1.0 else (yb.data_ptr(), lamv.data_ptr())
    o = _produce(producer, z, y, K, eps, mix, (t, alpha, 1.0 / tau))
    zs, yn, ybn = o["z"], y.cpu().numpy(), yb.cpu().numpy()
    if producer == "head_fused":
        assert zs[2, K - 2] - np.delete(zs[2], K - 2).max() > 60
    r = do.distill_rows(zs, t[:, :K].double().cpu().numpy(), yn, tau, alpha, eps,
                        None if mix is None else ybn, lam)
    yd = yn if lam >= 0.5 else ybn   # precision: against the (dominant) label
    assert o["correct"].item() == float((zs.argmax(axis=1) == yd).sum())
    assert o["topk"].item() == float(xo.in_top_k(zs, yd, 5).sum())
    worst = {}
    lb = do.loss_bound(tau, alpha)
    worst["loss"] = abs(o["loss"].item() - r["loss"].sum()) / (N * lb)
    if "ws" in o:
        rows = o["ws"][N * ld:N * ld + 2 * N].view(N, 2)[:, 0].double().cpu().numpy()
        assert np.isfinite(rows).all()
        worst["row loss"] = (np.abs(rows - r["loss"]) / lb).max()
        g32 = o["ws"][:N * ld].view(N, ld)[:, :K].double().cpu().numpy()
        assert np.isfinite(g32).all()
        worst["grad"] = (np.abs(g32 - r["grad"] / N) / do.grad_bound(r, tau, alpha, 1 / N)).max()
    dl = o["dlogits"].double().cpu().numpy()
    assert np.isfinite(dl).all() and np.isfinite(o["loss"].item())
    assert (dl[:, K:] == 0).all()
    worst["dlogits"] = (np.abs(dl[:, :K] - r["grad"] / N) /
                        do.grad_bound(r, tau, alpha, 1 / N, bf16=True)).max()
    print(f"{producer} K={K} tau={tau} alpha={alpha} {variant}: ratio to bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("producer,K", PRODUCERS)
def test_rows_without_a_teacher_are_bitwise_the_old_call(gpu, producer, K, variant):
    ld = SHAPES[K]
    eps, lam = VARIANTS[variant]
    z, _, y, yb = _rows(K, ld, gpu)
    lamv = torch.full((N,), lam, device=gpu)
    mix = None if lam == 1.0 else (yb.data_ptr(), lamv.data_ptr())
    old = _produce(producer, z, y, K, eps, mix, None)
    new = _produce(producer, z, y, K, eps, mix, (None, 0.0, 0.25))
    for k in old:
        if k != "z":
            assert torch.equal(old[k], new[k]), k


# ---- engine ----------------------------------------------------------------------------
N_ENG = 16
PLANS = {"persistent": "persist=1", "head_fused": "persist=0,fused_head=1",
         "unfused": "persist=0,fused_head=0"}
TAU, ALPHA, EPS, SEED = 4.0, 0.5, 0.1, 3


def _engine(monkeypatch, gpu, tune, **kw):
    monkeypatch.setenv("DTR_TUNE", tune)
    spec = cifar_spec(8)
    eng = Engine(spec, N_ENG, weight_decay=2e-4, lr_schedule=cifar_lr_schedule(), device=gpu,
                 input_mode="nhwc", use_graph=kw.pop("use_graph", False), **kw)
    g = torch.Generator().manual_seed(0)
    imgs = torch.randn(N_ENG, 32, 32, 3, generator=g).to(BF).float().to(gpu)
    labels = torch.randint(0, 10, (N_ENG,), generator=g).to(gpu)
    eng.set_batch(imgs, labels)
    return eng, labels


@pytest.fixture(scope="module")
def teacher_logits(gpu):
    """The ResNet-14 teacher's own inference plan (GPUInference's engine, persistent eval
    plan), filled on first use with the engine's x_in; computed once."""
    cache = {}

    def get(x_in):
        if not cache:
            inf = GPUInference(cifar_spec(14), N_ENG, device=gpu)
            inf.engine.params.initialize(SEED)
            inf.engine.repack()
            ev = inf.engine.build_eval_plan(N_ENG, persist=True)
            ev.run(x_in, torch.zeros(N_ENG, dtype=torch.int32, device=gpu), raw_u8=False)
            torch.cuda.synchronize()
            cache["t"] = ev.logits.clone()
        return cache["t"]
    return get


@pytest.mark.parametrize("plan", list(PLANS))
def test_engine_step_matches_oracle(gpu, monkeypatch, teacher_logits, plan):
    eng, labels = _engine(monkeypatch, gpu, PLANS[plan], label_smoothing=EPS,
                          distill_alpha=ALPHA, distill_temperature=TAU,
                          distill_teacher=(cifar_spec(14), SEED))
    assert eng.persist == (plan == "persistent"), eng.persist_reason
    if not eng.persist:
        assert eng._head_fused == (plan == "head_fused")
    assert eng.plan.names().count("prn_infer") == 1
    assert eng.distill_state() is None
    eng.forward_backward(_st())
    torch.cuda.synchronize()
    assert not eng.persist_error()
    assert torch.equal(eng.teacher.logits, teacher_logits(eng.x_in))   # same kernel, same bits
    K, kp = 10, eng.kpad
    w = eng.params.view("dense/kernel").to(BF).double()
    zs = (eng.pooled.double() @ w + eng.params.view("dense/bias").double()).cpu().numpy()
    t = eng.teacher.logits[:, :K].double().cpu().numpy()
    r = do.distill_rows(zs, t, labels.cpu().numpy(), TAU, ALPHA, EPS)
    loss = eng.scalars[0].item()
    dl = eng.dlogits.view(N_ENG, kp)[:, :K].double().cpu().numpy()
    ratio = (np.abs(dl - r["grad"] / N_ENG) /
             do.grad_bound(r, TAU, ALPHA, 1 / N_ENG, bf16=True)).max()
    lratio = abs(loss - r["loss"].sum()) / (N_ENG * do.loss_bound(TAU, ALPHA))
    print(f"{plan}: loss/N {loss / N_ENG:.6f} vs {r['loss'].mean():.6f} (ratio {lratio:.3f}), "
          f"dlogits ratio to bound {ratio:.3f}")
    assert np.isfinite(loss) and lratio <= 1.0 and ratio <= 1.0
    m = eng.metrics(reduce=False)
    assert (m["distill_alpha"], m["distill_temperature"]) == (ALPHA, TAU)
    assert m["cross_entropy"] == loss / N_ENG


@pytest.mark.parametrize("tune", ["persist=1", "persist=0"])
def test_engine_alpha_zero_is_the_plain_plan(gpu, monkeypatch, tune):
    plain, _ = _engine(monkeypatch, gpu, tune)
    off, _ = _engine(monkeypatch, gpu, tune, distill_alpha=0.0,
                     distill_teacher=(cifar_spec(14), SEED))
    assert off.teacher is None and off.distill_state() is None
    assert off.plan.names() == plain.plan.names() and "prn_infer" not in off.plan.names()


def test_engine_graph_replays(gpu, monkeypatch):
    """Several replays of the captured step against the same recording stepped eagerly."""
    kw = dict(distill_alpha=ALPHA, distill_teacher=(cifar_spec(14), SEED), use_graph=True)
    eager, _ = _engine(monkeypatch, gpu, "persist=0", **dict(kw))
    graph, _ = _engine(monkeypatch, gpu, "persist=0", **dict(kw))
    for _ in range(5):
        eager.step()
    done = graph.capture(warmup=2)
    assert graph.graph is not None
    for _ in range(5 - done):
        graph.step()
    torch.cuda.synchronize()
    assert int(graph.gstep.item()) == 5
    want = eager.distill_state()
    assert want.shape == (N_ENG, 10) and want.abs().max() > 0
    assert torch.equal(graph.distill_state(), want)
    assert torch.equal(graph.params.master, eager.params.master)
