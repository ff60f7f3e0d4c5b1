"""RandAugment's integer specification (data/randaug.py) against a plain fp64 formulation of the
same ops, its draw, and the flags.

Tolerances: the LUT ops, Identity and Translate are exact.  The four blends may differ by one
level (the integer degenerate image is rounded, |1 - f| <= 0.9).  Shear and Rotate are exact
wherever both fp64 source coordinates lie farther than 2^-7 from a rounding boundary (the Q16
coefficients are off by at most 2^-17 * 45); at most 5 % of the pixels may be that close.
The shapes are even and >= 40 on purpose: with an even size the shear offsets are k + 1/2, and
0.09 * 5.5 = 0.495 (magnitude 9) puts exactly two rows or columns on a boundary, 6.25 % of
32x32; with an odd size 0.3 * 5 = 1.5 (magnitude 30) puts four there, 10.8 % of 37x45.  Two of
48, 44 or 56 are under the cap (measured on the oracle's own coordinates: 4.2 % and 4.5 %)."""
import math

import numpy as np
import pytest

from distributed_tensorflow_resnet_amd.data import randaug as ra
from distributed_tensorflow_resnet_amd.train.layout import check_randaug
from distributed_tensorflow_resnet_amd.utils.flags import build_parser

SHAPES = [(48, 48), (44, 56)]


def images(H, W):
    """Uniform random, constant, two-level and horizontal-ramp uint8 [H, W, 3] images."""
    g = np.random.default_rng(H * 1000 + W)
    ramp = np.broadcast_to((np.arange(W) * 255 // (W - 1))[None, :, None], (H, W, 3))
    return [g.integers(0, 256, (H, W, 3)).astype(np.uint8), np.full((H, W, 3), 77, np.uint8),
            np.where(g.random((H, W, 3)) < 0.5, 40, 200).astype(np.uint8), ramp.astype(np.uint8)]


def half_up(x):
    return np.floor(np.asarray(x, dtype=np.float64) + 0.5)


def oracle(img, op, sign, m):
    """fp64 `op` from its real-valued definition -> (image, mask of pixels to compare)."""
    p = img.astype(np.float64)
    H, W, _ = p.shape
    g = -1.0 if sign else 1.0
    keep = np.ones((H, W), dtype=bool)
    f = 1.0 + g * 0.9 * m / 30.0
    if 1 <= op <= 5:
        y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64),
                           indexing="ij")
        cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
        s, th = g * 0.3 * m / 30.0, g * math.radians(30.0 * m / 30.0)
        sx, sy = {1: (x + s * (y - cy), y), 2: (x, y + s * (x - cx)),
                  3: (x - g * int(150.0 / 331.0 * W * m / 30.0), y),
                  4: (x, y - g * int(150.0 / 331.0 * H * m / 30.0)),
                  5: (math.cos(th) * (x - cx) - math.sin(th) * (y - cy) + cx,
                      math.sin(th) * (x - cx) + math.cos(th) * (y - cy) + cy)}[op]
        for v in (sx, sy):
            keep &= np.abs(v - np.floor(v) - 0.5) > 2.0 ** -7
        ix, iy = half_up(sx).astype(int), half_up(sy).astype(int)
        inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        out = np.full_like(p, 128.0)
        out[inside] = p[iy[inside], ix[inside]]
        return out, keep
    if 6 <= op <= 9:
        grey = 0.299 * p[..., 0] + 0.587 * p[..., 1] + 0.114 * p[..., 2]
        D = np.zeros_like(p)
        if op == 7:
            D = np.repeat(grey[..., None], 3, axis=2)
        elif op == 8:
            D = np.full_like(p, grey.mean())
        elif op == 9:
            D = p.copy()
            D[1:-1, 1:-1] = (sum(p[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx] for dy in (-1, 0, 1)
                                 for dx in (-1, 0, 1)) + 4 * p[1:-1, 1:-1]) / 13.0
        return half_up(np.clip(D * (1.0 - f) + p * f, 0.0, 255.0)), keep
    if op == 10:
        q = 2.0 ** float(half_up(4.0 * m / 30.0))
        return np.floor(p / q) * q, keep
    if op == 11:
        return np.where(p >= 255.0 - half_up(255.0 * m / 30.0), 255.0 - p, p), keep
    out = p.copy()
    for c in range(3 if op >= 12 else 0):
        ch = p[..., c]
        if op == 12 and ch.max() > ch.min():
            out[..., c] = half_up((ch - ch.min()) * 255.0 / (ch.max() - ch.min()))
        if op == 13:
            hist = np.bincount(img[..., c].ravel(), minlength=256).astype(np.float64)
            step = np.floor((hist.sum() - hist[hist > 0][-1]) / 255.0)
            if step > 0:
                lut = np.minimum(255.0, np.floor((np.cumsum(hist) - hist + np.floor(step / 2)) / step))
                out[..., c] = lut[img[..., c]]
    return out, keep


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("m", [1, 9, 30])
@pytest.mark.parametrize("sign", [0, 1])
@pytest.mark.parametrize("op", range(14), ids=ra.RA_OPS)
def test_spec_equals_the_fp64_formulation(op, sign, m, shape):
    tables = ra.randaug_tables(m, *shape)
    for img in images(*shape):
        got = ra.randaug_image(img, [(op, sign)], tables).astype(np.float64)
        want, keep = oracle(img, op, sign, m)
        assert 1.0 - keep.mean() <= (0.05 if op in (1, 2, 5) else 0.0)
        assert np.abs(got - want)[keep].max() <= (1.0 if 6 <= op <= 9 else 0.0)


def test_draw():
    tab = ra.randaug_op_table("all")
    a = ra.randaug_draw(7, 3, 5, 3, tab)
    assert a == ra.randaug_draw(7, 3, 5, 3, tab) and a[:2] == ra.randaug_draw(7, 3, 5, 2, tab)
    assert all(ra.randaug_draw(*k, 3, tab) != a
               for k in ((8, 3, 5), (7, 4, 5), (7, 3, 6), (7, 2 ** 32 + 3, 5)))
    seen = {d for n in range(14 * 200) for d in ra.randaug_draw(7, 11, n, 1, tab)}
    assert seen == {(op, s) for op in range(14) for s in (0, 1)}
    assert all(op == 13 for s in range(5) for n in range(5)
               for op, _ in ra.randaug_draw(7, s, n, 2, [13]))


def test_check_randaug_and_flags(capsys):
    assert check_randaug(2, 9, "all") == (2, 9, tuple(range(14)))
    assert check_randaug(0, 30, "rotate, Equalize") == (0, 30, (5, 13))
    for bad in ((4, 9, "all"), (-1, 9, "all"), (2.0, 9, "all"), (2, 31, "all"), (2, -1, "all"),
                (2, 9, "Blur"), (2, 9, ""), (2, 9, 3), (2, 9, ",".join(["Rotate"] * 17))):
        with pytest.raises(ValueError):
            check_randaug(*bad)
    p = build_parser("cifar")
    assert p.parse_args([]).randaug_num_ops == 0 and p.parse_args([]).randaug_magnitude == 9
    p.parse_args(["--randaug_num_ops", "0", "--randaug_magnitude", "30", "--randaug_ops",
                  "Rotate", "--synthetic", "--resident_data"])   # off: the others unused
    for argv in (["--randaug_num_ops", "2", "--synthetic"],
                 ["--randaug_num_ops", "2", "--resident_data"], ["--randaug_num_ops", "4"],
                 ["--randaug_num_ops", "1", "--randaug_magnitude", "31"],
                 ["--randaug_num_ops", "0", "--randaug_ops", "Blur"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    assert "randaug" in capsys.readouterr().err
