"""AugMix's Jensen-Shannon loss without a GPU: train/jsd.py against the fp64 oracle (the errors
printed here are the base of the device bounds, profiles/augmix_jsd.md), fan-out, flags."""
import jsd_oracle as jo
import numpy as np
import pytest
import torch

from distributed_tensorflow_resnet_amd.data.augmix import augmix_batch, augmix_fanout
from distributed_tensorflow_resnet_amd.train.jsd import jsd_grad, jsd_loss
from distributed_tensorflow_resnet_amd.utils.flags import build_parser

W = 12.0
KINDS = ("random", "identical", "spread")


def triples(B, C, kind, seed=0):
    """[3B, C] fp32 logits, [B] labels.  identical: JSD 0; spread: some p_ic underflow to 0 in fp32."""
    g = torch.Generator().manual_seed(seed + 7 * B + C)
    z = torch.randn(3 * B, C, generator=g) * 3
    if kind == "identical":
        z = z[:B].repeat(3, 1)
    if kind == "spread":
        z = z * 27
        z[0, 1 % C] = 80.0    # the clean view's own peak ...
        z[B, 2 % C] = 80.0    # ... and another class in a view: a large, finite JSD
    y = torch.randint(0, C, (B,), generator=g)
    return z.contiguous(), y


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,C", [(1, 10), (2, 10), (5, 100), (3, 1000)])
def test_torch_loss_and_gradients_match_the_oracle(B, C, kind, eps):
    z, y = triples(B, C, kind)
    r = jo.jsd_head(z.numpy(), y.numpy(), B, W, eps)
    assert np.isfinite(r["loss"]).all() and np.isfinite(r["grad"]).all()
    if kind == "spread":
        assert (torch.softmax(z, 1) == 0).any()
    if kind == "identical":
        hard = jo.jsd_head(z.numpy(), y.numpy(), B, 0.0, eps)
        assert abs(r["mean"] - hard["mean"]) < 1e-12
        assert np.abs(r["grad"] - hard["grad"]).max() < 1e-12
    zt = z.clone().requires_grad_(True)
    loss = jsd_loss(zt, y, B, W, eps)
    loss.backward()
    e_loss = abs(loss.item() - r["mean"]) / max(1.0, abs(r["mean"]))
    e_auto = np.abs(zt.grad.double().numpy() - r["grad"]).max() * 3 * B
    closed = jsd_grad(z, y, B, W, eps)
    e_closed = np.abs(closed.double().numpy() - r["grad"]).max() * 3 * B
    print(f"fp32 loss err {e_loss:.2e} (of max(1, loss)), N x grad err {e_auto:.2e}, closed {e_closed:.2e}")
    assert e_loss < 2e-5 and e_auto < 2e-4 and e_closed < 2e-4
    assert torch.allclose(closed, zt.grad, atol=2e-4 / (3 * B), rtol=0)


@pytest.mark.parametrize("layout,shape", [("chw", (3, 32, 32)), ("hwc", (16, 24, 3))])
def test_fanout_specification(layout, shape):
    B, y = 3, np.array([4, 0, 9], dtype=np.int32)
    x = np.random.default_rng(1).integers(0, 256, (B,) + shape, dtype=np.uint8)
    out, lab, log = augmix_fanout(x, y, layout, 5, 11, width=2)
    assert out.shape == (3 * B,) + shape and (out[:B] == x).all() and (log[:B] == -1).all()
    assert (lab == np.tile(y, 3)).all()
    # position p is the stored image p % B through the chains keyed on p
    want, wlog = augmix_batch(np.concatenate([x, x, x]), layout, 5, 11, width=2)
    assert (out[B:] == want[B:]).all() and (log[B:] == wlog[B:]).all()
    assert (out[B:2 * B] != out[2 * B:]).any()   # the two views of an image differ


@pytest.mark.parametrize("extra,reason", [
    ([], "augmix_width"),
    (["--augmix_width", "3", "--mixup_alpha", "0.2"], "mixup_alpha"),
    (["--augmix_width", "3", "--cutmix_alpha", "1.0"], "cutmix_alpha"),
    (["--augmix_width", "3", "--erase_prob", "0.25"], "erase_prob"),
    (["--augmix_width", "3", "--distill_alpha", "0.5", "--distill_teacher_dir", "t"], "distill_alpha"),
    (["--augmix_width", "3", "--augmix_jsd_weight", "-1"], "augmix_jsd_weight"),
    (["--augmix_width", "3"], None),   # accepted
])
def test_flags(capsys, extra, reason):
    p = build_parser("cifar")
    if reason is None:
        assert p.parse_args(["--augmix_jsd"] + extra).augmix_jsd_weight == 12.0
        return
    with pytest.raises(SystemExit):
        p.parse_args(["--augmix_jsd"] + extra)
    assert reason in capsys.readouterr().err
