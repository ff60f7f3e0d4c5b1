"""Mixup off the GPU: the specification (data/cifar.py mixup_table / mixup_draw), the flag,
the two-label loss of ops/reference.py and one mixed step of the CPU trainer against the
fp64 definitions of tests/mixup_oracle.py."""
import numpy as np
import pytest
import torch
import mixup_oracle as mo

from distributed_tensorflow_resnet_amd.data import cifar
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.ops import reference as ref
from distributed_tensorflow_resnet_amd.train.backends import CPUBackend
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr
from distributed_tensorflow_resnet_amd.utils.flags import build_parser

SEED = 4321


@pytest.mark.parametrize("batch", [1, 2, 3, 5, 128])
def test_draw_ranges_and_determinism(batch):
    shifts = set()
    for step in list(range(200)) + [2 ** 32 + 3, 2 ** 40 + 1]:
        idx, shift = cifar.mixup_draw(SEED, step, batch, 4096)
        assert (idx, shift) == cifar.mixup_draw(SEED, step, batch, 4096)
        assert 0 <= idx < 4096
        if batch == 1:
            assert shift == 0
        else:
            assert 1 <= shift <= batch - 1
            assert all((n + shift) % batch != n for n in range(batch))
        shifts.add(shift)
    if batch >= 3:
        assert len(shifts) > 1   # the rotation changes from step to step


def test_draw_is_exact_past_32_bits_and_salted():
    hi, lo = 2 ** 32 + 3, 3
    # the 64-bit step takes part: the draw is not that of the step's low word
    draws = [cifar.mixup_draw(SEED, s, 128, 4096) for s in (lo, hi, hi + 1)]
    assert len(set(draws)) == 3
    # written out: splitmix(splitmix(seed ^ salt) ^ splitmix(step * P mod 2^64))
    m64 = (1 << 64) - 1
    h = cifar.splitmix(cifar.splitmix(SEED ^ 0x4D4958555021) ^
                       cifar.splitmix((hi * 0x100000001B3) & m64))
    assert cifar.mixup_draw(SEED, hi, 5, 7) == ((h & 0xFFFFFFFF) % 7, 1 + (h >> 32) % 4)
    # not the crop hash of any image of that step
    crops = {cifar.splitmix(SEED ^ cifar.splitmix((hi * 0x100000001B3 + n) & m64))
             for n in range(128)}
    assert h not in crops
    for bad in ((-1, 4, 8), (0, 0, 8), (0, 4, 0)):
        with pytest.raises(ValueError):
            cifar.mixup_draw(SEED, *bad)


def test_table_is_the_numpy_beta_draw():
    t = cifar.mixup_table(0.2, 7)
    want = np.random.Generator(np.random.PCG64(7)).beta(0.2, 0.2, 4096).astype(np.float32)
    assert t.dtype == np.float32 and t.shape == (4096,)
    assert np.array_equal(t, want)
    assert (t >= 0).all() and (t <= 1).all()
    assert cifar.mixup_table(1.0, 7, 16).shape == (16,)
    assert not np.array_equal(t, cifar.mixup_table(0.2, 8))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            cifar.mixup_table(bad, 7)


@pytest.mark.parametrize("kind", ["cifar", "imagenet"])
def test_flag(kind):
    assert build_parser(kind).parse_args([]).mixup_alpha == 0.0
    assert build_parser(kind).parse_args(["--mixup_alpha", "0.2"]).mixup_alpha == 0.2
    for bad in ("-0.1", "nan", "inf", "x"):
        with pytest.raises(SystemExit):
            build_parser(kind).parse_args([f"--mixup_alpha={bad}"])
    with pytest.raises(SystemExit):
        build_parser(kind).parse_args(["--mixup_alpha", "0.2", "--synthetic"])
    assert build_parser(kind).parse_args(["--mixup_alpha", "0", "--synthetic"]).synthetic


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_reference_two_label_loss_matches_fp64(eps):
    g = torch.Generator().manual_seed(3)
    N, K = 6, 10
    z = (torch.randn(N, K, generator=g) * 3).requires_grad_(True)
    ya = torch.randint(0, K, (N,), generator=g)
    yb = torch.randint(0, K, (N,), generator=g)
    yb[0] = ya[0]
    lam = torch.tensor([0.0, 0.3, 0.5, 1.0, 0.3, 0.7])
    loss = ref.softmax_cross_entropy(z, ya, eps, yb, lam)
    loss.backward()
    rows, _, grad = mo.mixed_xent(z.detach().numpy(), ya.numpy(), yb.numpy(), lam.numpy(), eps)
    np.testing.assert_allclose(loss.item(), rows.mean(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(z.grad.numpy(), grad / N, rtol=1e-4, atol=1e-6)
    # lam = 1 is the one-label loss
    np.testing.assert_allclose(ref.softmax_cross_entropy(z, ya, eps, yb, 1.0).item(),
                               ref.softmax_cross_entropy(z, ya, eps).item(), rtol=1e-6)
    with pytest.raises(ValueError):
        ref.softmax_cross_entropy(z, ya, eps, yb)


def _trainer(**kw):
    return CPUBackend(cifar_spec(8), 4, weight_decay=2e-4, lr_schedule=constant_lr(0.1), **kw)


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(4, 32, 32, 3, generator=g), torch.randint(0, 10, (4,), generator=g)


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_cpu_trainer_mixed_step_matches_oracle(eps):
    x, y = _batch(5)
    be = _trainer(mixup_alpha=0.4, data_seed=SEED, label_smoothing=eps)
    assert be.mixup_state() is None
    be.set_batch(x, y)
    be.step()
    table = cifar.mixup_table(0.4, SEED)
    idx, shift = cifar.mixup_draw(SEED, 0, 4, len(table))
    lam, got_shift = be.mixup_state()
    assert (lam, got_shift) == (float(table[idx]), shift) and 0.0 < lam < 1.0
    m = be.metrics(top5=True)
    assert m["mixup_lam"] == lam
    yb = y.numpy()[(np.arange(4) + shift) % 4]
    logits = be.last_logits.numpy()
    rows, _, grad = mo.mixed_xent(logits, y.numpy(), yb, lam, eps)
    np.testing.assert_allclose(m["cross_entropy"], rows.mean(), rtol=1e-4, atol=1e-6)
    plain, _, _ = mo.mixed_xent(logits, y.numpy(), y.numpy(), 1.0, eps)
    assert abs(rows.mean() - plain.mean()) > 1e-3   # the second label is visible in the loss
    s = be.store.slot("dense/bias")
    db = be.store.master.grad[s.offset:s.offset + s.numel].numpy()
    np.testing.assert_allclose(db, (grad / 4).sum(axis=0), rtol=1e-4, atol=1e-6)
    yd = mo.dominant(y.numpy(), yb, lam)
    assert m["precision"] == float((logits.argmax(axis=1) == yd).mean())
    # the logits are those of the blended input: a second trainer fed the blend, unmixed
    xb = torch.from_numpy(mo.blend(x.numpy(), x.numpy()[(np.arange(4) + shift) % 4], lam)).float()
    plain_be = _trainer(label_smoothing=eps)
    plain_be.set_batch(xb, y)
    plain_be.step()
    np.testing.assert_allclose(plain_be.last_logits.numpy(), logits, rtol=1e-4, atol=1e-5)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _trainer(mixup_alpha=bad)


def test_cpu_trainer_zero_alpha_is_the_default():
    x, y = _batch(6)
    a, b = _trainer(), _trainer(mixup_alpha=0.0)
    for be in (a, b):
        be.set_batch(x, y)
        be.step()
    assert torch.equal(a.store.master, b.store.master)
    assert torch.equal(a.mom, b.mom)
    assert a.metrics(top5=True) == b.metrics(top5=True) and "mixup_lam" not in b.metrics()
