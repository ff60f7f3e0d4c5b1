"""AugMix's integer specification (data/augmix.py): its mix against the real-valued one, its
tables, the flags, and the CPU backend.

The mix's bound is derived, not measured: out is the exact integer expression
((65536 - m) * 256 * o + m * sum w_i c_i) / 2**24 rounded half up, and the fp64 reference
evaluates the same value without error (every factor is a dyadic rational, every product and
sum fits 53 bits), so they differ by at most 0.5."""
import numpy as np
import pytest
import torch

from test_randaug_cpu import images

from distributed_tensorflow_resnet_amd.data import augmix as am
from distributed_tensorflow_resnet_amd.data import randaug as ra
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.train.backends import CPUBackend
from distributed_tensorflow_resnet_amd.train.layout import check_augmix
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr
from distributed_tensorflow_resnet_amd.utils.flags import build_parser


@pytest.mark.parametrize("depth", [1, 3, -1])
@pytest.mark.parametrize("width", [1, 3, 4])
def test_integer_mix_is_the_rounded_real_mix(width, depth):
    H, W = 24, 40
    tables, mix = ra.randaug_tables(9, H, W), am.augmix_tables(width, 1.0, 5)
    ops = am.augmix_op_table()
    depths = set()
    for n, img in enumerate(images(H, W) * 3):
        index, chains = am.augmix_draw(5, 7, n, width, depth, ops)
        depths |= {len(c) for c in chains}
        got = am.augmix_image(img, chains, mix[index], tables).astype(np.float64)
        m = mix[index, -1] / 65536.0
        want = (1.0 - m) * img + m * sum(
            (w / 256.0) * ra.randaug_image(img, c, tables) for w, c in zip(mix[index], chains))
        assert np.abs(got - want).max() <= 0.5
    assert depths == ({depth} if depth > 0 else {1, 2, 3})


@pytest.mark.parametrize("alpha", [0.3, 1.0])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_table_entries_are_exact_fixed_point(width, alpha):
    t = am.augmix_tables(width, alpha, 11)
    assert t.shape == (am.AM_TABLE_LEN, width + 1) and t.dtype == np.int32
    assert (t[:, :width].sum(axis=1) == 256).all() and (t[:, :width] >= 0).all()
    assert t[:, width].min() >= 0 and t[:, width].max() <= 65536
    assert np.array_equal(t, am.augmix_tables(width, alpha, 11))
    assert not np.array_equal(t, am.augmix_tables(width, alpha, 12))


def test_identity_only_returns_the_input():
    x = np.stack(images(16, 16)).transpose(0, 3, 1, 2)
    out, log = am.augmix_batch(x, "chw", 3, 9, width=4, op_table=am.augmix_op_table("Identity"))
    assert np.array_equal(out, x) and (log[:, :, 1:, 0] <= 0).all()


def test_check_augmix_and_flags(capsys):
    nine = tuple(sorted(ra.RA_OPS.index(n) for n in am.AM_OPS))
    got = check_augmix(3, -1, 3, 1.0, "augmix")
    assert got[:4] == (3, -1, 3, 1.0)
    assert tuple(sorted(got[4])) == nine == (1, 2, 3, 4, 5, 10, 11, 12, 13)
    assert check_augmix(0, 2, 10, 0.5, "all", randaug_num_ops=2)[4] == tuple(range(14))
    for bad in ((5,), (-1,), (2.0,), (3, 0), (3, 4), (3, -2), (3, -1, 11), (3, -1, -1),
                (3, -1, 3, 0.0), (3, -1, 3, float("inf")), (3, -1, 3, 1.0, "Blur"),
                (3, -1, 3, 1.0, 7), (3, -1, 3, 1.0, "augmix", 2)):
        with pytest.raises(ValueError):
            check_augmix(*bad)
    p = build_parser("cifar")
    ns = p.parse_args([])
    assert (ns.augmix_width, ns.augmix_depth, ns.augmix_severity, ns.augmix_alpha,
            ns.augmix_ops) == (0, -1, 3, 1.0, "augmix")
    p.parse_args(["--augmix_width", "0", "--augmix_depth", "3", "--randaug_num_ops", "2"])
    for argv in (["--augmix_width", "3", "--randaug_num_ops", "2"],
                 ["--augmix_width", "3", "--synthetic"],
                 ["--augmix_width", "3", "--resident_data"],
                 ["--augmix_width", "5"], ["--augmix_width", "3", "--augmix_alpha", "0"],
                 ["--augmix_width", "3", "--augmix_depth", "0"],
                 ["--augmix_width", "0", "--augmix_ops", "Blur"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    assert "augmix" in capsys.readouterr().err


def test_cpu_backend_applies_the_spec():
    g = torch.Generator().manual_seed(7)
    x = torch.randint(0, 256, (4, 3, 32, 32), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 10, (4,), generator=g, dtype=torch.int32)
    on, off = (CPUBackend(cifar_spec(8), 4, weight_decay=2e-4, lr_schedule=constant_lr(0.1),
                          data_seed=21, augmix_width=w, augmix_depth=2) for w in (3, 0))
    assert off.augmix_mix is None and off.augmix_state() is None
    want, log = am.augmix_batch(x.numpy(), "chw", 21, 0, 3, 2)
    assert (want != x.numpy()).any()
    on.set_batch(x, y)
    off.set_batch(torch.from_numpy(want), y)
    assert torch.equal(on._x, off._x) and np.array_equal(on.augmix_state(), log)
    imagenet = imagenet_spec(0, num_classes=10, image_hw=64, block="bottleneck",
                             layers=[1, 1, 1, 1])
    for spec, kw in ((cifar_spec(8), dict(randaug_num_ops=1)), (imagenet, {})):
        with pytest.raises(ValueError, match="augmix_width"):
            CPUBackend(spec, 4, weight_decay=2e-4, lr_schedule=constant_lr(0.1), augmix_width=3,
                       **kw)
