"""The one-launch persistent inference forward (csrc/prn_infer.hip prn_infer_kernel,
train/persist.py PersistInfer, Engine.build_eval_plan(batch, persist=True)): against the
fp32 oracle and the reference's trained graph, its exact properties (images independent,
no atomics: bit-equal rows whatever the batch), the shared loss / precision tail, that it
writes nothing the training plan owns, and how the engine selects it."""
import pytest
import torch

from distributed_tensorflow_resnet_amd.models.params import ParamStore
from distributed_tensorflow_resnet_amd.models.resnet_torch import TorchResNet
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule

import golden_files

pytestmark = pytest.mark.gpu

NIMG = 16   # training batch of the shared engines; eval images are its first rows


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _make(spec, N, gpu, seed=0):
    """test_engine_gpu.py's setup: engine + a bf16-exact random batch + an oracle store."""
    eng = Engine(spec, N, weight_decay=2e-4, lr_schedule=cifar_lr_schedule(), device=gpu,
                 input_mode="nhwc", use_graph=False)
    torch.manual_seed(seed)
    imgs = torch.randn(N, spec.image_h, spec.image_w, 3, device=gpu).to(torch.bfloat16).float()
    labels = torch.randint(0, spec.num_classes, (N,), device=gpu)
    eng.set_batch(imgs, labels)
    return eng, imgs, labels


_cache = {}


def _trained(gpu, depth, classes=10):
    """Engine after three training steps (non-trivial moving statistics), its images and
    the fp32 oracle's probabilities of the first 8 of them -- built once per network."""
    key = (depth, classes)
    if key not in _cache:
        spec = cifar_spec(depth, num_classes=classes)
        eng, imgs, labels = _make(spec, NIMG, gpu)
        for _ in range(3):
            eng.step()
        torch.cuda.synchronize()
        store = ParamStore(spec, device=gpu)
        store.master.copy_(eng.params.master)
        store.stats.copy_(eng.params.stats)
        with torch.no_grad():
            p_ref = torch.softmax(TorchResNet(spec, store)(imgs[:8], False), 1)
        _cache[key] = (spec, eng, imgs, labels, p_ref)
    return _cache[key]


def _run(eng, imgs, labels, persist, batch=None):
    ev = eng.build_eval_plan(batch or imgs.shape[0], persist=persist)
    loss, correct, probs = ev.run(imgs, labels, raw_u8=False)
    torch.cuda.synchronize()
    return ev, loss, correct, probs.clone()


# ---- 1. against the fp32 oracle -------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3, 8])
@pytest.mark.parametrize("depth", [8, 14])
def test_matches_fp32_oracle(gpu, depth, N):
    """cifar_spec(8): one block per stage, i.e. the three projection / transition variants;
    cifar_spec(14) adds the identity blocks.  Bound: test_engine_gpu.py's for this
    comparison (test_eval_plan_matches_autograd_eval)."""
    spec, eng, imgs, labels, p_ref = _trained(gpu, depth)
    ev, _, _, probs = _run(eng, imgs[:N], labels[:N], True)
    assert ev.kind == "persistent" and ev.plan.size() == 2   # prn_infer, softmax_xent
    _, _, _, probs_l = _run(eng, imgs[:N], labels[:N], False)
    err, err_l = _rel(probs, p_ref[:N]), _rel(probs_l, p_ref[:N])
    print(f"resnet{depth} N={N}: persistent {err:.3e}, per-layer {err_l:.3e} vs fp32")
    assert err < 2e-2


def test_small_moving_variance_keeps_eps(gpu):
    """The in-kernel BatchNorm table is gamma * rsqrt(moving_variance + eps), the bn_eval
    op's expression.  With the usual variances (~1) eps = 1e-5 is invisible at any bf16
    bound, so this case sets every moving variance to 3e-5 and gamma to sqrt(3e-5 + eps):
    every BN scale is then 1, as in a well-conditioned network, while a table without eps
    scales each of the 7 BatchNorms by sqrt(4/3) -- far outside the bound.  Same bound and
    oracle as above."""
    from distributed_tensorflow_resnet_amd.train.engine import BN_EPS

    spec = cifar_spec(8)
    eng, imgs, labels = _make(spec, NIMG, gpu)
    var = 3e-5
    for name in eng.bns:
        g, v = eng.params.slot(f"{name}/gamma"), eng.params.slot(f"{name}/moving_variance")
        eng.params.master[g.offset:g.offset + g.numel] = (var + BN_EPS) ** 0.5
        eng.params.stats[v.offset:v.offset + v.numel] = var
    store = ParamStore(spec, device=gpu)
    store.master.copy_(eng.params.master)
    store.stats.copy_(eng.params.stats)
    with torch.no_grad():
        p_ref = torch.softmax(TorchResNet(spec, store)(imgs[:3], False), 1)
    _, _, _, probs = _run(eng, imgs[:3], labels[:3], True)
    _, _, _, probs_l = _run(eng, imgs[:3], labels[:3], False)
    err = _rel(probs, p_ref)
    print(f"variance 3e-5: persistent {err:.3e}, per-layer {_rel(probs_l, p_ref):.3e} vs fp32")
    assert bool(torch.isfinite(probs).all())
    assert err < 2e-2


# ---- 2. CIFAR-100 -----------------------------------------------------------------------
def test_cifar100_head(gpu):
    """100 classes pad to 112 columns: past the training step's kpad <= 64, so the looped
    dense staging and class columns run; the padding columns are stored as exact zeros."""
    spec, eng, imgs, labels, p_ref = _trained(gpu, 8, classes=100)
    assert eng.kpad == 112 and not eng.nat.prn_supported(3, 1, 3, 100, 112)
    ev = eng.build_eval_plan(3, persist=True)   # must not raise
    ev.logits.fill_(1.0)
    _, _, probs = ev.run(imgs[:3], labels[:3], raw_u8=False)
    torch.cuda.synchronize()
    _, _, _, probs_l = _run(eng, imgs[:3], labels[:3], False)
    err = _rel(probs, p_ref[:3])
    print(f"cifar-100: persistent {err:.3e}, per-layer {_rel(probs_l, p_ref[:3]):.3e} vs fp32")
    assert probs.shape == (3, 100)
    assert err < 2e-2
    assert torch.equal(ev.logits[:, 100:], torch.zeros(3, 12, device=gpu))
    assert bool((ev.logits[:, :100] != 1.0).all())


# ---- 3. the reference's trained graph -----------------------------------------------------
def test_golden_graph(gpu, monkeypatch):
    """test_golden_gpu.py::test_gpu_inference_matches_reference_graph (same seed, n, inputs
    and bounds) with the persistent plan forced."""
    from distributed_tensorflow_resnet_amd.utils import frozen
    from distributed_tensorflow_resnet_amd.utils import graphdef as gd
    from distributed_tensorflow_resnet_amd.utils.tf_interp import Interpreter

    ref_pb = golden_files.frozen_pb()
    monkeypatch.setenv("DTR_TUNE", "persist_eval=1")
    torch.manual_seed(0)
    n = 64
    x = torch.randn(n, 32, 32, 3).to(torch.bfloat16).float()
    labels = torch.randint(0, 10, (n,))
    y = torch.nn.functional.one_hot(labels, 10).float()
    probs_ref, _ = Interpreter(gd.read_graph(ref_pb)).run(["Softmax", "final_dense"], {"X": x, "Y": y})
    m = frozen.FrozenModel(ref_pb, "gpu", n)
    assert m.model.eval_path == "persistent"
    probs, _ = m.predict(x, labels)
    err = ((probs.double() - probs_ref.double()).norm() / (probs_ref.double().norm() + 1e-30)).item()
    agree = (probs.argmax(1) == probs_ref.argmax(1)).float().mean().item()
    print(f"softmax rel err {err:.2e}, argmax agreement {agree:.3f}")
    assert err < 2e-2
    assert agree >= 0.95, agree


# ---- 4. exact properties ------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch(gpu):
    """Images are independent and nothing is accumulated across workgroups: a row is
    bit-equal whatever batch it is part of and wherever it stands in it."""
    spec, eng, imgs, labels, _ = _trained(gpu, 14)
    _, _, _, p3 = _run(eng, imgs[:3], labels[:3], True)
    _, _, _, p3b = _run(eng, imgs[:3], labels[:3], True)
    assert torch.equal(p3, p3b)   # two runs
    for i in range(3):
        _, _, _, p1 = _run(eng, imgs[i:i + 1], labels[i:i + 1], True)
        assert torch.equal(p1[0], p3[i]), i
    # more images than CUs: no co-residency requirement, no batch limit
    big = 300
    assert big > eng.nat.cu_count()
    rows = [0, 1, 2, 37, 149, 255, 256, 299]
    idx = torch.arange(big, device=gpu) % 3
    idx[rows] = torch.tensor([0, 1, 2, 1, 2, 0, 1, 2], device=gpu)
    _, _, _, pb = _run(eng, imgs[idx], labels[idx], True, batch=big)
    for r in rows:
        assert torch.equal(pb[r], p3[idx[r]]), r


# ---- 5. the tail ----------------------------------------------------------------------------
def test_loss_and_correct_match_the_probabilities(gpu):
    spec, eng, imgs, labels, _ = _trained(gpu, 8)
    _, loss, correct, probs = _run(eng, imgs[:8], labels[:8], True)
    y = labels[:8].long()
    top2 = probs.topk(2, 1).values
    assert bool((top2[:, 0] > top2[:, 1]).all()), "top-1 tie in the test inputs"
    want = float(-torch.log(probs.double().gather(1, y[:, None])).sum())
    assert abs(loss - want) <= 1e-5 * abs(want), (loss, want)
    assert correct == float((probs.argmax(1) == y).sum())


# ---- 6. writes nothing it does not own ------------------------------------------------------
def test_leaves_engine_state_untouched(gpu):
    spec, eng, imgs, labels, _ = _trained(gpu, 8)
    snap = lambda: ([eng.params.master.clone(), eng.params.stats.clone(), eng.X[0].clone()] +
                    [t.clone() for bn in eng.bns.values() for t in (bn.scale, bn.shift)])
    before = snap()
    _run(eng, imgs[:8], labels[:8], True)
    for a, b in zip(before, snap()):
        assert torch.equal(a, b)


def test_eval_between_training_steps_changes_nothing(gpu):
    """Two same-seed engines on the default persistent training step, one fixed batch: 2
    steps + a persistent eval of 8 other images + 2 steps == 4 straight steps, bitwise."""
    spec = cifar_spec(8)
    e1, imgs, labels = _make(spec, NIMG, gpu)
    e2, _, _ = _make(spec, NIMG, gpu)
    assert e1.persist and e2.persist, e1.persist_reason
    torch.manual_seed(7)
    other = torch.randn(8, 32, 32, 3, device=gpu).to(torch.bfloat16).float()
    for _ in range(2):
        e1.step()
    e1.build_eval_plan(8, persist=True).run(other, labels[:8], raw_u8=False)
    for _ in range(2):
        e1.step()
    for _ in range(4):
        e2.step()
    torch.cuda.synchronize()
    assert not e1.persist_error() and not e2.persist_error()
    assert torch.equal(e1.params.master, e2.params.master)
    assert torch.equal(e1.mom, e2.mom)
    assert torch.equal(e1.params.stats, e2.params.stats)


# ---- 7. selection ---------------------------------------------------------------------------
def test_selection(gpu, monkeypatch):
    from distributed_tensorflow_resnet_amd.train.evaluator import GPUInference

    spec = cifar_spec(8)
    monkeypatch.setenv("DTR_TUNE", "persist_eval=0")
    eng, imgs, labels = _make(spec, NIMG, gpu)
    assert eng.build_eval_plan(8).kind == "per-layer"
    monkeypatch.setenv("DTR_TUNE", "persist_eval=1")
    assert eng.build_eval_plan(8).kind == "persistent"
    assert eng.build_eval_plan(8) is eng.build_eval_plan(8, persist=True)
    assert eng.build_eval_plan(8, persist=False).kind == "per-layer"
    # tune persist=0 keeps meaning "the launch-per-layer engine" under the default persist_eval
    monkeypatch.setenv("DTR_TUNE", "persist=0")
    assert eng.build_eval_plan(8).kind == "per-layer"
    # an unsupported network: persist_eval=1 quietly falls back, persist=True says why
    monkeypatch.setenv("DTR_TUNE", "persist_eval=1")
    im = Engine(imagenet_spec(18), 8, weight_decay=2e-4,
                lr_schedule=cifar_lr_schedule(), device=gpu, input_mode="nhwc", use_graph=False)
    assert im.build_eval_plan(8).kind == "per-layer"
    with pytest.raises(ValueError, match="not a CIFAR network"):
        im.build_eval_plan(8, persist=True)
    # GPUInference reports the choice; its short-last-batch path gives the full batch's rows
    gi = GPUInference(spec, 8, device=gpu)
    assert gi.eval_path == "persistent"
    x, y = imgs[:8].cpu(), labels[:8].cpu()
    _, _, full = gi.run(x, y)
    full = full.clone()
    loss5, correct5, part = gi.run(x[:5], y[:5])
    assert torch.equal(part, full[:5])
    assert correct5 == float((full[:5].argmax(1).cpu() == y[:5]).sum())
    monkeypatch.setenv("DTR_TUNE", "persist_eval=0")
    assert GPUInference(spec, 8, device=gpu).eval_path == "per-layer"
