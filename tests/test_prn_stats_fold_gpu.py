"""BatchNorm statistics fold of the persistent CIFAR kernels (csrc/prn_device.h: bn_sums,
bn_sums_arrive) on the smallest network (6n+2, n = 1: three building blocks) at the tiny
batches that still reach every path of the fold:

  * batch 3, one slice per image: wave 0 arrives by itself after the fold (no second
    workgroup barrier); an odd workgroup count, so the accumulator replicas
    (blockIdx % 4) and the arrival shards get uneven shares;
  * batch 2 at two and at four slices per image (`persist_slices`): the border-row
    publish keeps the drained arrive of every wave, and stage 3 at four slices has
    fewer 16x16 tiles than waves (the `wave_active` case: idle waves write no partials).

(The persistent training step takes at most 64 padded classes, so there is no CIFAR-100
case: 100 classes pad to 112 and run the per-layer plan.)

Each case runs the persistent step and the per-layer step (`persist=0`) from the same
weights on the same seeded batch and compares every BatchNorm's published batch mean
and rstd, the moving statistics, the loss and the updated weights, with the bounds of
tests/test_persist_gpu.py:

  * mean: rel < 5e-2 + 1e-3 max|mean|, rstd: rel < 2e-2, moving statistics: rel < 1e-3
    (test_persistent_forward_matches_per_layer);
  * loss: both plans are within 1e-2 max(1, loss) of the same oracle
    (test_persistent_step_matches_autograd), so within 2e-2 max(1, loss) of each other;
  * weights: one step moves a weight by -lr (g + wd w), so the step's weight change
    differs by no more than the gradients do; each plan's gradient is within 5e-2 of the
    same oracle (test_persistent_step_matches_autograd), so the two changes are within
    1e-1 of each other.

The fold must also stay deterministic: three steps run twice from the same state give
the same bits."""
import pytest
import torch

from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule

pytestmark = pytest.mark.gpu

CASES = [(3, 1), (2, 2), (2, 4)]   # (batch, slices per image)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _engine(monkeypatch, spec, N, gpu, persist, slices=-1):
    monkeypatch.setenv("DTR_TUNE", f"persist={persist},persist_slices={slices},opt_fused=1")
    eng = Engine(spec, N, weight_decay=2e-4, lr_schedule=cifar_lr_schedule(), device=gpu,
                 input_mode="nhwc", use_graph=False)
    assert eng.persist == (persist == 1)
    return eng


def _batch(spec, N, gpu):
    g = torch.Generator(device="cpu").manual_seed(0)
    imgs = torch.randn(N, spec.image_h, spec.image_w, 3, generator=g).to(torch.bfloat16).float()
    labels = torch.randint(0, spec.num_classes, (N,), generator=g)
    return imgs.to(gpu), labels.to(gpu)


@pytest.mark.parametrize("N,slices", CASES)
def test_fold_matches_per_layer(gpu, monkeypatch, N, slices):
    spec = cifar_spec(8)
    ep = _engine(monkeypatch, spec, N, gpu, 1, slices)
    er = _engine(monkeypatch, spec, N, gpu, 0)
    assert ep.prn.P == slices
    er.params.master.copy_(ep.params.master)
    er.params.stats.copy_(ep.params.stats)
    er.repack()
    imgs, labels = _batch(spec, N, gpu)
    w0 = ep.params.master.clone()
    for e in (ep, er):
        e.set_batch(imgs, labels)
        e.step()
    torch.cuda.synchronize()
    assert not ep.persist_error()
    figs = []
    for name, bp in ep.bns.items():
        br = er.bns[name]
        figs.append((name, _rel(bp.mean, br.mean), 5e-2 + 1e-3 * br.mean.abs().max().item(),
                     _rel(bp.rstd, br.rstd)))
    lp, lr_ = ep.scalars[0].item() / N, er.scalars[0].item() / N
    d_stats = _rel(ep.params.stats, er.params.stats)
    d_w = _rel(ep.params.master - w0, er.params.master - w0)
    print(f"N={N} P={slices}: worst mean rel {max(f[1] for f in figs):.3e}, worst rstd rel "
          f"{max(f[3] for f in figs):.3e}, moving stats rel {d_stats:.3e}, loss {lp:.6f} vs "
          f"{lr_:.6f}, weight-change rel {d_w:.3e}")
    for name, dm, bound, dr in figs:
        assert dm < bound, (name, dm, bound)
        assert dr < 2e-2, (name, dr)
    assert d_stats < 1e-3
    assert abs(lp - lr_) < 2e-2 * max(1.0, lr_)
    assert d_w < 1e-1
    assert torch.isfinite(ep.params.master).all()


@pytest.mark.parametrize("N,slices", CASES)
def test_fold_is_deterministic(gpu, monkeypatch, N, slices):
    spec = cifar_spec(8)
    ep = _engine(monkeypatch, spec, N, gpu, 1, slices)
    imgs, labels = _batch(spec, N, gpu)
    ep.set_batch(imgs, labels)
    state = [t.clone() for t in (ep.params.master, ep.params.stats, ep.mom, ep.gstep)]

    def run():
        for dst, src in zip((ep.params.master, ep.params.stats, ep.mom, ep.gstep), state):
            dst.copy_(src)
        ep.repack()
        for _ in range(3):
            ep.step()
        torch.cuda.synchronize()
        assert not ep.persist_error()
        out = [ep.params.master.clone(), ep.params.stats.clone(), ep.mom.clone(),
               ep.scalars[:2].clone()]
        for bn in ep.bns.values():
            out += [bn.mean.clone(), bn.rstd.clone()]
        return out

    a, b = run(), run()
    assert int(ep.gstep.item()) == int(state[3].item()) + 3
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"tensor {i} differs between two runs from the same state"
