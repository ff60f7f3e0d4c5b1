"""The teacher-forced oracle (tests/forced_oracle.py) pinned on the CPU: forcing on its own
activations changes nothing, it agrees with the existing autograd oracle
(models/resnet_torch.py), and the per-tensor criterion test_layerwise_gpu.py asserts with it
rejects single-tensor defects that the whole-gradient criterion of the older step tests
(rel(whole gradient) < 5e-2) accepts."""
import pytest
import torch

import forced_oracle as fo
from distributed_tensorflow_resnet_amd.models.params import ParamStore
from distributed_tensorflow_resnet_amd.models.resnet_torch import TorchResNet
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.ops import reference as ref


def _bottleneck():
    return imagenet_spec(0, image_hw=64, block="bottleneck", layers=[1, 1, 1, 1])


def _setup(spec, N, seed=0, bf16_weights=False):
    store = ParamStore(spec)
    store.initialize(seed)
    g = torch.Generator().manual_seed(seed + 1)
    # gamma 1 / beta 0 / bias 0 at init: move them so their gradients are generic
    for s in store.train_slots:
        if s.kind in ("gamma", "beta", "dense_bias"):
            store.view(s.name).add_(0.05 * torch.randn(s.shape, generator=g))
    if bf16_weights:
        store.master.copy_(store.master.to(torch.bfloat16).float())
    imgs = torch.randn(N, spec.image_h, spec.image_w, 3, generator=g).to(torch.bfloat16).float()
    labels = torch.randint(0, spec.num_classes, (N,), generator=g)
    return store, imgs, labels


def _slices(store):
    return [(s.name, slice(s.offset, s.offset + s.numel)) for s in store.train_slots]


@pytest.mark.parametrize("spec_fn,N", [(lambda: cifar_spec(8), 16), (_bottleneck, 4)])
def test_forcing_on_own_activations_is_identity(spec_fn, N):
    """Free fp64 run, then forced on its own activations: the same loss, the same gradient
    in every tensor, the same statistics (1e-12).  The bottleneck ImageNet net also forces
    the max-pool output and H2."""
    spec = spec_fn()
    store, imgs, labels = _setup(spec, N)
    free = fo.run(spec, store.master, store.stats, imgs, labels, mode="exact")
    assert list(free.pred) == fo.point_names(spec)
    assert ("pool_out" in free.pred) == spec.maxpool
    forced = fo.run(spec, store.master, store.stats, imgs, labels, mode="exact",
                    saved=free.pred)
    assert abs(forced.loss - free.loss) <= 1e-12 * abs(free.loss)
    for name, sl in _slices(store):
        assert free.grad[sl].abs().max() > 0, name
        assert fo.rel(forced.grad[sl], free.grad[sl]) <= 1e-12, name
    for k in free.pred:
        assert fo.rel(forced.pred[k], free.pred[k]) <= 1e-12, k
    for k, (mean, rstd) in free.bn.items():
        assert fo.rel(forced.bn[k][0], mean) <= 1e-12 and fo.rel(forced.bn[k][1], rstd) <= 1e-12
    assert fo.rel(forced.stats, free.stats) <= 1e-12


def test_forcing_replaces_the_value_and_keeps_the_gradient_path():
    """Forced on perturbed activations the forward takes the saved values (the next
    layer's prediction moves, the forced layer's own does not) and every tensor still
    receives a gradient."""
    spec = cifar_spec(8)
    store, imgs, labels = _setup(spec, 8)
    free = fo.run(spec, store.master, store.stats, imgs, labels, mode="exact")
    saved = dict(free.pred)
    saved["H1[1]"] = saved["H1[1]"].roll(1, dims=0)   # another image's (a scale BN would undo)
    forced = fo.run(spec, store.master, store.stats, imgs, labels, mode="exact", saved=saved)
    assert fo.rel(forced.pred["H1[1]"], free.pred["H1[1]"]) <= 1e-12
    assert fo.rel(forced.pred["X[2]"], free.pred["X[2]"]) > 1e-2
    # the next forced point re-synchronises: nothing downstream of X[2] sees the change
    assert fo.rel(forced.pred["H1[2]"], free.pred["H1[2]"]) <= 1e-12
    assert abs(forced.loss - free.loss) <= 1e-12 * abs(free.loss)
    for name, sl in _slices(store):
        assert forced.grad[sl].abs().max() > 0, name


@pytest.mark.parametrize("spec_fn,N,smooth", [(lambda: cifar_spec(8), 16, 0.0),
                                              (lambda: cifar_spec(8, num_classes=100), 8, 0.1),
                                              (_bottleneck, 4, 0.0)])
def test_free_fp32_matches_torch_resnet(spec_fn, N, smooth):
    """fp32, no forcing, no gradient rounding vs TorchResNet(emulate_bf16=False) on
    bf16-representable weights (the helper always multiplies bf16 kernels): per tensor to
    fp32 rounding, and the same moving statistics."""
    spec = spec_fn()
    store, imgs, labels = _setup(spec, N, bf16_weights=True)
    got = fo.run(spec, store.master, store.stats, imgs, labels, mode="exact",
                 dtype=torch.float32, label_smoothing=smooth)
    model = TorchResNet(spec, store, emulate_bf16=False)
    xent, _ = model.loss(model(imgs, True), labels, 2e-4, smooth)
    xent.backward()
    assert abs(got.loss - xent.item()) <= 1e-5 * abs(xent.item())
    for name, sl in _slices(store):
        assert fo.rel(got.grad[sl], store.master.grad[sl]) <= 1e-5, name
    assert fo.rel(got.stats, store.stats) <= 1e-6


def test_free_emulated_matches_torch_resnet_emulation():
    """The emulated mode rounds where TorchResNet(emulate_bf16=True) does: running free it
    is the same fp32 computation."""
    spec = cifar_spec(20)
    store, imgs, labels = _setup(spec, 16)
    got = fo.run(spec, store.master, store.stats, imgs, labels, mode="emulated")
    model = TorchResNet(spec, store, emulate_bf16=True)
    xent, _ = model.loss(model(imgs, True), labels, 2e-4)
    xent.backward()
    assert abs(got.loss - xent.item()) <= 1e-6 * abs(xent.item())
    for name, sl in _slices(store):
        assert fo.rel(got.grad[sl], store.master.grad[sl]) <= 1e-6, name


# ---------------------------------------------------------------------------- mutation
@pytest.fixture(scope="module")
def standin():
    """cifar_spec(20) at N = 16 as a stand-in for an engine: activations of a free-running
    bf16-emulating forward, the gradient of the emulated oracle forced on them, and the
    exact oracle forced on the same activations.  Computed once; the tests copy."""
    spec = cifar_spec(20)
    store, imgs, labels = _setup(spec, 16)
    free = fo.run(spec, store.master, store.stats, imgs, labels, mode="emulated")
    exact = fo.run(spec, store.master, store.stats, imgs, labels, mode="exact", saved=free.pred)
    conv = spec.blocks[4].convs[1]           # a 3x3 stride-1 conv of stage 2
    emu = fo.run(spec, store.master, store.stats, imgs, labels, mode="emulated",
                 saved=free.pred, keep=(conv.name,))
    return dict(spec=spec, store=store, imgs=imgs, labels=labels, saved=free.pred,
                exact=exact, emu=emu, conv=conv)


def _new_rejects(s, g):
    return fo.violations(fo.per_tensor(s["store"], g, s["exact"].grad, s["emu"].grad))


def _old_accepts(s, g):
    """The whole-gradient criterion of test_engine_step_matches_autograd_shallow."""
    return fo.rel(g, s["emu"].grad) < 5e-2


def test_criterion_accepts_the_unmutated_standin(standin):
    s = standin
    assert _new_rejects(s, s["emu"].grad.clone()) == []
    assert _old_accepts(s, s["emu"].grad)
    rows = fo.per_tensor(s["store"], s["emu"].grad, s["exact"].grad, s["emu"].grad)
    assert len(rows) == len(s["store"].train_slots)
    print("largest noise_t:", sorted(((n, name) for _, n, name in rows), reverse=True)[:3])
    # bf16 gradient storage alone, teacher-forced: of order 1 %, not the 30-110 % of
    # free-running oracles
    assert max(n for _, n, _ in rows) < 5e-2


def test_criterion_rejects_a_scaled_bn_beta_gradient(standin):
    """A stage-2 BN's beta gradient times 1.05 (a BN-backward coefficient off by 5 %)."""
    s = standin
    name = s["spec"].blocks[4].bns[1].name + "/beta"
    sl = dict(_slices(s["store"]))[name]
    g = s["emu"].grad.clone()
    g[sl] *= 1.05
    bad = _new_rejects(s, g)
    assert [b[3] for b in bad] == [name], bad
    assert _old_accepts(s, g)


def test_criterion_rejects_a_dropped_input_row_in_one_wgrad(standin):
    """One 3x3 conv's weight gradient recomputed from an input whose bottom row is zero
    (a slice-boundary halo row dropped from a block's wgrad)."""
    s = standin
    conv = s["conv"]
    name = conv.name + "/kernel"
    sl = dict(_slices(s["store"]))[name]
    a, dy = s["emu"].kept[conv.name]
    w = s["store"].view(name).detach().clone().requires_grad_(True)

    def wgrad(x):
        (gw,) = torch.autograd.grad(ref.conv2d(x, w, conv.stride), w, dy)
        return gw.reshape(-1)

    # the recomputation is the oracle's own gradient when nothing is dropped
    assert fo.rel(wgrad(a), s["emu"].grad[sl]) < 1e-6
    a0 = a.clone()
    a0[:, -1] = 0
    g = s["emu"].grad.clone()
    g[sl] = wgrad(a0)
    bad = _new_rejects(s, g)
    assert [b[3] for b in bad] == [name], bad
    assert _old_accepts(s, g)


def test_criterion_rejects_a_dense_bias_gradient_of_other_labels(standin):
    """dense/bias's gradient from a batch in which two labels are swapped: every sample of
    class a relabelled b and the reverse, for two classes with different counts.  (The
    bias gradient is mean(softmax - onehot) over the batch, so exchanging the labels of
    two samples would not change it; exchanging two classes does.)  The two classes'
    counts differ by one sample: the smallest defect of this kind, two entries off by
    1/N -- 40 % of this tensor, 3 % of the whole gradient."""
    s = standin
    labels = s["labels"]
    counts = torch.bincount(labels, minlength=s["spec"].num_classes).tolist()
    a, b = next((i, j) for i in range(len(counts)) for j in range(i + 1, len(counts))
                if abs(counts[i] - counts[j]) == 1)
    swapped = labels.clone()
    swapped[labels == a] = b
    swapped[labels == b] = a
    other = fo.run(s["spec"], s["store"].master, s["store"].stats, s["imgs"], swapped,
                   mode="emulated", saved=s["saved"])
    sl = dict(_slices(s["store"]))["dense/bias"]
    g = s["emu"].grad.clone()
    g[sl] = other.grad[sl]
    bad = _new_rejects(s, g)
    assert [b_[3] for b_ in bad] == ["dense/bias"], bad
    assert _old_accepts(s, g)
