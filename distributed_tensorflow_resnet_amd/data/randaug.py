"""RandAugment (Cubuk et al. 2020) on the stored uint8 image: the specification.

csrc/randaug.hip must equal the functions below for every input, bit for bit.  Everything an
image goes through is integer arithmetic; whatever involves a real number (sin, cos,
0.3 * m / 30, ...) is evaluated once, here, into the small int32 table of `randaug_tables`
that both this file and the kernel read.

The ops are torchvision's RandAugment ops in its order (RA_OPS).  The draw is per image, keyed
like the crops and the erased boxes with (seed, step, n) under a salt of its own; op slot k
takes ``op_table[lo32(hk) % len(op_table)]`` and the sign bit ``(hk >> 32) & 1`` of
``hk = splitmix(h ^ (k + 1))``.  The sign negates the magnitude of ops 1-9 and is ignored by
the others.

Geometric ops (1-5) map every output pixel back to a source pixel (nearest neighbour, about
the centre ((W - 1) / 2, (H - 1) / 2), fill 128 outside).  With the doubled, centred
coordinates u = 2x - (W - 1), v = 2y - (H - 1) and six Q16 coefficients a..f per (op, sign)

    sx = (a * u + b * v + c + (W << 16)) >> 17        sy = (d * u + e * v + f + (H << 16)) >> 17

which is round-half-up of the real source coordinate (>> floors).  Blend ops (6-9) are
``clamp((D * (65536 - F) + p * F + 32768) >> 16, 0, 255)`` with the Q16 factor F and the
integer degenerate image D (ra_blend).
"""
from __future__ import annotations

import math

import numpy as np

from .cifar import _M64, splitmix

RA_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness",
          "Color", "Contrast", "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
RA_SALT = 0x52414E44415547          # "RANDAUG"
RA_FILL = 128
RA_MAX_OPS = 3
RA_MAX_MAGNITUDE = 30
# the table: [5 ops 1..5][2 signs][6] Q16 coefficients, [2 signs] Q16 blend factor, the
# Posterize mask, the Solarize threshold
RA_T_GEO, RA_T_BLEND, RA_T_POST, RA_T_SOL, RA_TABLE_LEN = 0, 60, 62, 63, 64
_Q = 65536


def _half_up(x: float) -> int:
    return int(math.floor(x + 0.5))


def randaug_tables(m: int, H: int, W: int) -> np.ndarray:
    """The int32 parameter table of magnitude bin m (0..30) for H x W images."""
    if not 0 <= int(m) <= RA_MAX_MAGNITUDE or int(m) != m:
        raise ValueError(f"randaug magnitude must be an integer in 0..30, got {m!r}")
    if not (1 <= H < 1 << 12 and 1 <= W < 1 << 12):
        raise ValueError(f"randaug needs 1 <= H, W < 4096, got {H}x{W}")
    m = int(m)
    t = np.zeros(RA_TABLE_LEN, dtype=np.int32)
    shear = 0.3 * m / 30.0
    tx = int(150.0 / 331.0 * W * m / 30.0)
    ty = int(150.0 / 331.0 * H * m / 30.0)
    theta = math.radians(30.0 * m / 30.0)
    for sign in (0, 1):
        g = -1.0 if sign else 1.0
        co, si = math.cos(g * theta), math.sin(g * theta)
        geo = {
            1: (_Q, _half_up(g * shear * _Q), 0, 0, _Q, 0),
            2: (_Q, 0, 0, _half_up(g * shear * _Q), _Q, 0),
            3: (_Q, 0, int(-g * 2 * tx) * _Q, 0, _Q, 0),
            4: (_Q, 0, 0, 0, _Q, int(-g * 2 * ty) * _Q),
            5: (_half_up(co * _Q), _half_up(-si * _Q), 0, _half_up(si * _Q), _half_up(co * _Q), 0),
        }
        for op, coef in geo.items():
            o = RA_T_GEO + ((op - 1) * 2 + sign) * 6
            t[o:o + 6] = coef
        t[RA_T_BLEND + sign] = _half_up((1.0 + g * 0.9 * m / 30.0) * _Q)
    keep = 8 - _half_up(4.0 * m / 30.0)
    t[RA_T_POST] = (0xFF << (8 - keep)) & 0xFF
    t[RA_T_SOL] = 255 - (17 * m + 1) // 2        # 255 - round-half-up(255 * m / 30)
    return t


def randaug_op_table(ops="all") -> np.ndarray:
    """The int32 list of allowed op ids: "all", a comma list of op names, or a list of ids."""
    if isinstance(ops, str):
        names = RA_OPS if ops == "all" else tuple(s.strip() for s in ops.split(","))
        lower = [n.lower() for n in RA_OPS]
        bad = [n for n in names if n.lower() not in lower]
        if bad or not names:
            raise ValueError(f"randaug_ops must be 'all' or a comma list of {RA_OPS}, got {ops!r}")
        ids = [lower.index(n.lower()) for n in names]
    else:
        ids = [int(i) for i in ops]
        if not ids or any(not 0 <= i < len(RA_OPS) for i in ids):
            raise ValueError(f"randaug op ids must be a non-empty list of 0..13, got {ops!r}")
    return np.asarray(ids, dtype=np.int32)


def randaug_draw(seed: int, step: int, n: int, num_ops: int, op_table) -> list:
    """Image n's ops at step `step`: [(op, sign)] * num_ops.  Integers only; exact for
    steps >= 2**32."""
    if step < 0 or n < 0 or not 1 <= num_ops <= RA_MAX_OPS or len(op_table) < 1:
        raise ValueError("need step >= 0, n >= 0, 1 <= num_ops <= 3 and a non-empty op table")
    h = splitmix(splitmix((seed & _M64) ^ RA_SALT) ^ splitmix((step * 0x100000001B3 + n) & _M64))
    out = []
    for k in range(num_ops):
        hk = splitmix(h ^ (k + 1))
        out.append((int(op_table[(hk & 0xFFFFFFFF) % len(op_table)]), (hk >> 32) & 1))
    return out


def ra_grey(img: np.ndarray) -> np.ndarray:
    """[H, W] integer grey of an int64 [H, W, 3] image."""
    return (19595 * img[..., 0] + 38470 * img[..., 1] + 7471 * img[..., 2] + 32768) >> 16


def ra_blend(D: np.ndarray, p: np.ndarray, F: int) -> np.ndarray:
    return np.clip((D * (_Q - F) + p * F + 32768) >> 16, 0, 255)


def _gather(img, coef):
    H, W, _ = img.shape
    a, b, c, d, e, f = (int(v) for v in coef)
    v, u = np.meshgrid(2 * np.arange(H, dtype=np.int64) - (H - 1),
                       2 * np.arange(W, dtype=np.int64) - (W - 1), indexing="ij")
    sx = (a * u + b * v + c + (W << 16)) >> 17
    sy = (d * u + e * v + f + (H << 16)) >> 17
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    out = np.full_like(img, RA_FILL)
    out[inside] = img[sy[inside], sx[inside]]
    return out


def _equalize_lut(ch: np.ndarray) -> np.ndarray:
    hist = np.bincount(ch.ravel(), minlength=256).astype(np.int64)
    step = (int(hist.sum()) - int(hist[np.nonzero(hist)[0][-1]])) // 255
    if step == 0:
        return np.arange(256, dtype=np.int64)
    before = np.cumsum(hist) - hist
    return np.minimum(255, (before + step // 2) // step)


def randaug_image(img_hwc_u8: np.ndarray, ops, tables) -> np.ndarray:
    """The uint8 [H, W, 3] image after the (op, sign) pairs of `ops`, in order."""
    img = np.asarray(img_hwc_u8).astype(np.int64)
    H, W, C = img.shape
    if C != 3 or len(tables) != RA_TABLE_LEN:
        raise ValueError("randaug_image takes an [H, W, 3] image and a randaug_tables table")
    t = [int(v) for v in tables]
    for op, sign in ops:
        F = t[RA_T_BLEND + sign]
        if op == 0:
            pass
        elif op <= 5:
            o = RA_T_GEO + ((op - 1) * 2 + sign) * 6
            img = _gather(img, t[o:o + 6])
        elif op == 6:
            img = ra_blend(np.zeros_like(img), img, F)
        elif op == 7:
            img = ra_blend(ra_grey(img)[..., None], img, F)
        elif op == 8:
            mean = (2 * int(ra_grey(img).sum()) + H * W) // (2 * H * W)
            img = ra_blend(np.full_like(img, mean), img, F)
        elif op == 9:
            D = img.copy()
            if H > 2 and W > 2:
                s = sum(img[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx]
                        for dy in (-1, 0, 1) for dx in (-1, 0, 1)) + 4 * img[1:-1, 1:-1]
                D[1:-1, 1:-1] = (s + 6) // 13
            img = ra_blend(D, img, F)
        elif op == 10:
            img = img & t[RA_T_POST]
        elif op == 11:
            img = np.where(img >= t[RA_T_SOL], 255 - img, img)
        elif op == 12:
            for c in range(3):
                lo, hi = int(img[..., c].min()), int(img[..., c].max())
                if hi > lo:
                    img[..., c] = ((img[..., c] - lo) * 510 + (hi - lo)) // (2 * (hi - lo))
        elif op == 13:
            for c in range(3):
                img[..., c] = _equalize_lut(img[..., c])[img[..., c]]
        else:
            raise ValueError(f"randaug op id must be in 0..13, got {op!r}")
    return img.astype(np.uint8)


def randaug_batch(batch_u8, layout: str, seed: int, step: int, num_ops: int = 2,
                  magnitude: int = 9, op_table=None, tables=None):
    """The augmented uint8 batch and the [N, num_ops, 2] int32 log of (op, sign).  layout "chw":
    [N, 3, H, W] (the CIFAR records), "hwc": [N, H, W, 3] (the ImageNet crops)."""
    if layout not in ("chw", "hwc"):
        raise ValueError(f"layout must be chw or hwc, got {layout!r}")
    x = np.asarray(batch_u8)
    hwc = x.transpose(0, 2, 3, 1) if layout == "chw" else x
    N, H, W, _ = hwc.shape
    op_table = randaug_op_table("all") if op_table is None else op_table
    tables = randaug_tables(magnitude, H, W) if tables is None else tables
    out = np.empty_like(hwc)
    log = np.zeros((N, num_ops, 2), dtype=np.int32)
    for n in range(N):
        ops = randaug_draw(seed, step, n, num_ops, op_table)
        log[n] = ops
        out[n] = randaug_image(hwc[n], ops, tables)
    out = out.transpose(0, 3, 1, 2) if layout == "chw" else out
    return np.ascontiguousarray(out), log
