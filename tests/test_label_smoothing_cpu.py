"""Label smoothing and top-5 precision off the GPU: the flag, the fp32 oracles of
ops/reference.py against the fp64 definitions of tests/xent_oracle.py, and the CPU trainer."""
import numpy as np
import pytest
import torch
import xent_oracle as xo

from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.ops import reference as ref
from distributed_tensorflow_resnet_amd.train.backends import CPUBackend
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr
from distributed_tensorflow_resnet_amd.utils.flags import build_parser


def tie_rows(K=10):
    """The constructed top-5 rows: (logits [R, K], labels [R], expected in-top-5 [R])."""
    assert K >= 8
    rows, labels, want = [], [], []

    def add(z, y, w):
        r = np.full(K, -4.0, dtype=np.float32)
        r[:len(z)] = z
        rows.append(r)
        labels.append(y)
        want.append(w)

    add([9, 8, 7, 6, 5, 4, 3, 2], 4, True)        # label strictly 5th
    add([9, 8, 7, 6, 5, 4, 3, 2], 5, False)       # label strictly 6th
    add([9, 8, 7, 6, 5, 5, 5, 2], 6, True)        # tied with the 5th and the 6th
    add([1, 1, 1, 1, 1, 1, 1, 1], 7, True)        # (all-equal row, below)
    rows[-1][:] = 1.0
    add([9, 8, 7, 6, 5, 4, 3, np.inf], 7, False)  # z[y] = inf
    add([9, 8, 7, 6, 5, 4, 3, np.nan], 7, False)  # z[y] = nan
    return np.stack(rows), np.array(labels), np.array(want)


@pytest.mark.parametrize("kind", ["cifar", "imagenet"])
def test_flag(kind):
    assert build_parser(kind).parse_args([]).label_smoothing == 0.0
    assert build_parser(kind).parse_args(["--label_smoothing", "0.1"]).label_smoothing == 0.1
    for bad in ("1.0", "-0.1", "1.5"):
        with pytest.raises(SystemExit):
            build_parser(kind).parse_args([f"--label_smoothing={bad}"])


@pytest.mark.parametrize("N,K", [(5, 10), (6, 100)])
def test_reference_loss_matches_fp64(N, K):
    g = torch.Generator().manual_seed(N * K)
    z = (torch.randn(N, K, generator=g) * 3).requires_grad_(True)
    y = torch.randint(0, K, (N,), generator=g)
    loss = ref.softmax_cross_entropy(z, y, label_smoothing=0.1)
    loss.backward()
    rows, _, grad = xo.smoothed_xent(z.detach().numpy(), y.numpy(), 0.1)
    np.testing.assert_allclose(loss.item(), rows.mean(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(z.grad.numpy(), grad / N, rtol=1e-4, atol=1e-6)
    # eps = 0 stays the plain cross-entropy
    assert torch.equal(ref.softmax_cross_entropy(z, y),
                       torch.nn.functional.cross_entropy(z, y, reduction="mean"))
    with pytest.raises(ValueError):
        ref.softmax_cross_entropy(z, y, label_smoothing=1.0)


def test_reference_in_top_k():
    z, y, want = tie_rows()
    got = ref.in_top_k(torch.from_numpy(z), torch.from_numpy(y), 5)
    assert got.tolist() == want.tolist()
    assert xo.in_top_k(z, y, 5).tolist() == want.tolist()
    # K = 3 < 5: every finite row is in, wherever the label ranks
    z3 = torch.tensor([[3.0, 2.0, 1.0], [1.0, 2.0, 3.0], [0.0, 0.0, 0.0]])
    for label in range(3):
        assert ref.in_top_k(z3, torch.full((3,), label), 5).all()
    assert not ref.in_top_k(torch.tensor([[0.0, float("inf"), 1.0]]), torch.tensor([1]), 5).any()
    # a label outside the classes is never in
    assert not ref.in_top_k(z3, torch.tensor([3, -1, 7]), 5).any()


def _trainer(**kw):
    return CPUBackend(cifar_spec(8), 4, weight_decay=2e-4, lr_schedule=constant_lr(0.1), **kw)


def test_cpu_trainer_smoothed_step():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 32, 32, 3, generator=g)
    y = torch.randint(0, 10, (4,), generator=g)
    be = _trainer(label_smoothing=0.1)
    be.set_batch(x, y)
    be.step()
    m = be.metrics(top5=True)
    # the new key is asked for; a plain call keeps the keys it has always had
    assert set(m) - set(be.metrics()) == {"precision_top5"}
    assert sorted(be.metrics()) == ["cost", "cross_entropy", "global_step", "l2", "lr",
                                    "precision"]
    logits = be.last_logits.numpy()
    rows, _, _ = xo.smoothed_xent(logits, y.numpy(), 0.1)
    np.testing.assert_allclose(m["cross_entropy"], rows.mean(), rtol=1e-4, atol=1e-6)
    plain, _, _ = xo.smoothed_xent(logits, y.numpy(), 0.0)
    assert abs(rows.mean() - plain.mean()) > 1e-3   # the smoothing is visible in the loss
    assert m["precision_top5"] == xo.in_top_k(logits, y.numpy(), 5).mean()
    assert 0.0 <= m["precision"] <= m["precision_top5"] <= 1.0
    with pytest.raises(ValueError):
        _trainer(label_smoothing=1.0)


def test_cpu_trainer_zero_smoothing_is_the_default():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(4, 32, 32, 3, generator=g)
    y = torch.randint(0, 10, (4,), generator=g)
    a, b = _trainer(), _trainer(label_smoothing=0.0)
    for be in (a, b):
        be.set_batch(x, y)
        be.step()
    assert torch.equal(a.store.master, b.store.master)
    assert torch.equal(a.mom, b.mom)
    assert a.metrics(top5=True) == b.metrics(top5=True)
