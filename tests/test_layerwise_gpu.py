"""One training step of either engine, chained as in production, checked tensor by tensor
and layer by layer against the teacher-forced oracle (tests/forced_oracle.py).

The older whole-step tests (test_engine_gpu.py, test_persist_gpu.py, test_golden_gpu.py)
compare with free-running oracles, whose forward drifts from the engine's through every
training-mode BatchNorm: they can only bound the norm of the whole gradient (5e-2; at depth
20 and 50 the fp32-vs-bf16 noise of 30-110 %), so one wrong tensor -- a projection's BN, the
dense bias, a halo row missing from one wgrad -- passes.  Here the oracle re-synchronises on
the engine's own saved activations (stem_out, pool_out, X, H1, H2, pooled), its backward is
the engine's linear chain at the engine's point, and every trainable tensor t is held to

    err_t = rel(engine, exact) <= 2 * noise_t + 1e-3,   noise_t = rel(emulated, exact)

(exact: fp64, nothing rounded; emulated: fp32 with activation gradients rounded to bf16 where
the engine stores them).  noise_t is measured on every run against the reference alone; the
engine and the emulation are independent realisations of the same roundings (sqrt 2), plus
MFMA / split-K summation order.  Reference-only maxima of noise_t over the tensors, on
activations of a free-running bf16-emulating forward (CPU, N = 16, seed 0): depth 8 0.9 %,
depth 20 1.5 %, depth 50 2.2 % (BatchNorm beta / gamma of the first blocks, where the most
roundings have accumulated).

Forward: each saved tensor against the exact oracle's one-layer-ahead prediction from the
previous saved tensors, rel <= 2 * rel(bf16(pred), pred) + 1e-4 -- what bf16 storage of one
layer costs, not a bound cumulated over the network; each BatchNorm's batch mean / rstd
against the oracle's from the same saved input (the tolerances of
test_conv_fused_prologue_epilogue), and the updated moving statistics per BatchNorm.

The oracle runs on the CPU in fp64: CIFAR ResNet-50 at N = 16 is about 4 GFLOP, a fraction of
a second per mode, and fp64 convolutions are not a path the GPU libraries serve well.  BN
gamma / beta and the dense bias are moved off their initial 1 / 0 / 0 (a gradient formula that
drops gamma is invisible at gamma = 1).
"""
from dataclasses import dataclass

import pytest
import torch

import forced_oracle as fo
from distributed_tensorflow_resnet_amd.models.params import ParamStore
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule

pytestmark = pytest.mark.gpu


@dataclass
class Case:
    id: str
    spec_fn: object
    N: int
    persist: int
    slices: int = -1          # tune persist_slices (-1 auto)
    P: tuple = None           # expected (forward, backward) slices of the persistent step
    smooth: float = 0.0
    declined: str = ""        # tune persist=1, but the persistent step does not cover the case


def _bottleneck():
    return imagenet_spec(0, image_hw=64, block="bottleneck", layers=[1, 1, 1, 1])


CASES = [
    Case("persist-rn8-n16-p4", lambda: cifar_spec(8), 16, 1, 4, (4, 4)),
    Case("persist-rn8-n16-p2", lambda: cifar_spec(8), 16, 1, 2, (2, 2)),
    Case("persist-rn8-n16-p1", lambda: cifar_spec(8), 16, 1, 1, (1, 1)),
    Case("persist-rn8-n40-p4", lambda: cifar_spec(8), 40, 1, 4, (4, 4)),
    Case("persist-rn20-n16-p4", lambda: cifar_spec(20), 16, 1, 4, (4, 4)),
    Case("persist-rn20-n32-p2", lambda: cifar_spec(20), 32, 1, 2, (2, 2)),
    Case("persist-rn50-n16-p4", lambda: cifar_spec(50), 16, 1, 4, (4, 4)),
    # one slice per image in both launches, chosen by the engine: split-32 slab sums
    Case("persist-rn8-n128-auto", lambda: cifar_spec(8), 128, 1, -1, (1, 1)),
    # the smoothed head of the persistent step (kpad 16) ...
    Case("persist-rn8-n16-p4-smooth", lambda: cifar_spec(8), 16, 1, 4, (4, 4), smooth=0.1),
    # ... and at 100 classes (kpad 112), which the persistent kernels and the one-launch head
    # decline (kpad <= 64): asked for the persistent step, the engine must take the
    # launch-per-layer plan with the 8-launch smoothed head
    Case("persist-declined-rn8-c100-smooth", lambda: cifar_spec(8, num_classes=100), 16, 1, 4,
         smooth=0.1, declined="kpad <= 64"),
    Case("layers-rn20-n16", lambda: cifar_spec(20), 16, 0),              # direct convs, deep
    Case("layers-imagenet18-n8", lambda: imagenet_spec(18, image_hw=64), 8, 0),
    Case("layers-bottleneck-n8", _bottleneck, 8, 0),                     # 1x1 streaming, H2
]


@dataclass
class Result:
    case: Case
    spec: object
    store: object
    loss: float
    grad: torch.Tensor
    stats: torch.Tensor
    saved: dict
    bn: dict
    exact: fo.Step
    emu: fo.Step


@pytest.fixture(scope="module", params=CASES, ids=[c.id for c in CASES])
def res(request, gpu):
    """One engine forward_backward of the case and both oracle modes forced on what it
    saved; computed once per case and only read by the tests."""
    case = request.param
    spec, N = case.spec_fn(), case.N
    g = torch.Generator(device="cpu").manual_seed(0)
    imgs = torch.randn(N, spec.image_h, spec.image_w, 3, generator=g).to(torch.bfloat16).float()
    labels = torch.randint(0, spec.num_classes, (N,), generator=g)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("DTR_TUNE", f"persist={case.persist},persist_slices={case.slices}")
        eng = Engine(spec, N, weight_decay=2e-4, lr_schedule=cifar_lr_schedule(), device=gpu,
                     input_mode="nhwc", use_graph=False, label_smoothing=case.smooth)
        assert eng.persist == (case.persist == 1 and not case.declined), eng.persist_reason
        if eng.persist:
            assert (eng.prn.P_fwd, eng.prn.P) == case.P
        elif case.declined:
            assert case.declined in eng.persist_reason and eng.kpad == 112
        for s in eng.params.train_slots:
            if s.kind in ("gamma", "beta", "dense_bias"):
                eng.params.view(s.name).add_((0.1 * torch.randn(s.shape, generator=g)).to(gpu))
        eng.repack()
        master, stats0 = eng.params.master.detach().cpu(), eng.params.stats.detach().cpu()
        eng.set_batch(imgs.to(gpu), labels.to(gpu))
        eng.forward_backward(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert not eng.persist_error()

    def host(t):
        return t.detach().float().cpu()

    saved = {"stem_out": host(eng.stem_out), "pooled": host(eng.pooled)}
    if spec.maxpool:
        saved["pool_out"] = host(eng.pool_out)
    for i, b in enumerate(spec.blocks):
        saved[f"H1[{i}]"] = host(eng.H1[i])
        if len(b.convs) == 3:
            saved[f"H2[{i}]"] = host(eng.H2[i])
        saved[f"X[{i + 1}]"] = host(eng.X[i + 1])
    assert set(saved) == set(fo.point_names(spec))
    bn = {name: (host(e.mean), host(e.rstd)) for name, e in eng.bns.items()}
    out = {mode: fo.run(spec, master, stats0, imgs, labels, mode=mode, saved=saved,
                        label_smoothing=case.smooth) for mode in ("exact", "emulated")}
    return Result(case, spec, ParamStore(spec), eng.scalars[0].item() / N, host(eng.grad),
                  host(eng.params.stats), saved, bn, out["exact"], out["emulated"])


def test_every_gradient_tensor_within_twice_the_bf16_noise(res):
    """Backward, per tensor, no slot skipped: err_t <= 2 * noise_t + 1e-3; the loss to 1e-3;
    the updated moving statistics of every BatchNorm to 1e-4."""
    rows = fo.per_tensor(res.store, res.grad, res.exact.grad, res.emu.grad)
    assert len(rows) == len(res.store.train_slots)
    ratio = max(rows, key=lambda r: r[0] / max(r[1], 1e-30))
    print(f"{res.case.id}: max err_t/noise_t {ratio[0] / max(ratio[1], 1e-30):.3f} ({ratio[2]}: err "
          f"{ratio[0]:.5f} noise {ratio[1]:.5f}); max noise_t {max(r[1] for r in rows):.5f}; "
          f"max err_t {max(r[0] for r in rows):.5f}; loss {res.loss:.6f} vs {res.exact.loss:.6f}")
    bad = fo.violations(rows)
    for over, e, n, name in bad[:5]:
        print(f"  {name}: err_t {e:.5f} noise_t {n:.5f} ({over:.2f} x the bound)")
    assert not bad, bad[:5]
    assert torch.isfinite(res.grad).all()
    assert abs(res.loss - res.exact.loss) <= 1e-3 * abs(res.exact.loss)
    worst = max((fo.rel(res.stats[s.offset:s.offset + s.numel],
                        res.exact.stats[s.offset:s.offset + s.numel]), s.name)
                for s in res.store.stat_slots)
    print(f"  worst moving statistic: {worst}")
    assert fo.rel(res.stats, res.exact.stats) < 1e-4
    for s in res.store.stat_slots:
        sl = slice(s.offset, s.offset + s.numel)
        assert fo.rel(res.stats[sl], res.exact.stats[sl]) < 1e-4, s.name


def test_every_saved_activation_is_one_layer_of_bf16_rounding_from_the_oracle(res):
    """Forward, per forced point: the saved tensor vs the exact oracle's prediction from
    the previous saved tensors, within twice what rounding the prediction to bf16 costs.
    (The head is covered by the loss and the dense gradients: the one-launch heads keep
    their logits in registers.)"""
    worst, bad = (0.0, None), []
    for k in fo.point_names(res.spec):
        got, pred = res.saved[k], res.exact.pred[k]
        err = fo.rel(got, pred)
        bound = 2 * fo.rel(pred.to(torch.bfloat16), pred) + 1e-4
        worst = max(worst, (err / bound, k))
        if not err <= bound:
            bad.append((k, err, bound))
    print(f"{res.case.id}: worst forward err / bound {worst[0]:.3f} at {worst[1]}")
    assert not bad, bad[:5]


def test_every_batchnorm_statistic_matches_the_oracle_on_the_same_input(res):
    """Each BatchNorm's batch mean and rstd vs the oracle's, from the same saved input."""
    assert set(res.bn) == set(res.exact.bn)
    w_mean = max((float((res.bn[k][0] - res.exact.bn[k][0].float()).abs().max()), k)
                 for k in res.bn)
    w_rstd = max((fo.rel(res.bn[k][1], res.exact.bn[k][1]), k) for k in res.bn)
    print(f"{res.case.id}: worst |mean - ref| {w_mean}, worst rel rstd {w_rstd}")
    for k, (mean, rstd) in res.bn.items():
        m_ref, r_ref = (t.float() for t in res.exact.bn[k])
        torch.testing.assert_close(mean, m_ref, rtol=1e-4, atol=1e-4, msg=lambda m: f"{k} mean: {m}")
        torch.testing.assert_close(rstd, r_ref, rtol=1e-3, atol=1e-4, msg=lambda m: f"{k} rstd: {m}")
