"""AugMix (Hendrycks et al. 2020) on the stored uint8 image: the specification.

csrc/augmix.hip must equal the functions below for every input, bit for bit.  The ops are
RandAugment's (randaug.py: randaug_image with the unchanged randaug_tables of bin 3 * severity),
so everything an image goes through is integer arithmetic.  For a uint8 image o:

    c_i  = chain i's result: depth_i ops in a row, starting from o           i < width
    acc  = sum_i w_i * c_i             w_i in Q8, sum w_i == 256, so acc <= 65280 (16 bits)
    out  = ((65536 - m) * (o << 8) + m * acc + (1 << 23)) >> 24           m in Q16, 0..65536

The last line stays below 2**32 (65536 * 65280 + 2**23), so uint32 arithmetic suffices; it is
round-half-up of (1 - m) o + m sum w_i c_i.  Mixing in pixel space equals the paper's mixing
after normalisation: the weights sum to one and normalisation is affine.

No sampler runs on the device: `augmix_tables` draws Dirichlet(alpha) weights and the
Beta(alpha, alpha) factor in fp64 on the host, once, and quantises them.  The draw is per image,
keyed like the other augmentations with (seed ^ salt, step, n): h picks the table entry
``lo32(h) % len``; chain i has ``hc = splitmix(h ^ ((i + 1) << 8))`` and, when the depth is
drawn, ``depth_i = 1 + lo32(hc) % 3``; its slot k takes ``hk = splitmix(hc ^ (k + 1))``, the op
``op_table[lo32(hk) % len(op_table)]`` and the sign bit ``(hk >> 32) & 1``, as RandAugment's.

Deviations from the paper: every op has the one magnitude of its bin (the paper draws it in
[0.1, severity]); the result is rounded to uint8; there is no Jensen-Shannon consistency loss.
"""
from __future__ import annotations

import numpy as np

from .cifar import _M64, splitmix
from .randaug import randaug_image, randaug_op_table, randaug_tables

AM_SALT = 0x4155474D495821          # "AUGMIX!"
AM_TABLE_LEN = 4096
AM_MAX_WIDTH = 4
AM_MAX_DEPTH = 3
AM_MAX_SEVERITY = 10
# the paper's nine: RandAugment's ops without the four that overlap ImageNet-C (Brightness,
# Color, Contrast, Sharpness) and without Identity
AM_OPS = ("AutoContrast", "Equalize", "Posterize", "Rotate", "Solarize", "ShearX", "ShearY",
          "TranslateX", "TranslateY")


def augmix_op_table(ops="augmix") -> np.ndarray:
    """The int32 list of allowed op ids: "augmix" (the paper's nine), or what randaug_op_table
    takes ("all", a comma list of op names, a list of ids)."""
    return randaug_op_table(",".join(AM_OPS) if isinstance(ops, str) and ops == "augmix" else ops)


def augmix_tables(width: int, alpha: float = 1.0, seed: int = 0,
                  length: int = AM_TABLE_LEN) -> np.ndarray:
    """int32 [length, width + 1]: per entry the Q8 chain weights w_0..w_{width-1} and the Q16
    blend factor m, from Generator(PCG64(seed ^ salt)) in fp64.  The weights are a
    Dirichlet(alpha) sample times 256, floored, with the units that are left given to the
    largest remainders (the lower index first among equals), so every entry sums to 256
    exactly; m is a Beta(alpha, alpha) sample times 65536, rounded half up."""
    if isinstance(width, bool) or int(width) != width or not 1 <= width <= AM_MAX_WIDTH:
        raise ValueError(f"augmix width must be an integer in 1..4, got {width!r}")
    if not (alpha > 0 and np.isfinite(alpha)):
        raise ValueError(f"augmix alpha must be finite and > 0, got {alpha!r}")
    width = int(width)
    rng = np.random.Generator(np.random.PCG64((seed & _M64) ^ AM_SALT))
    p = rng.dirichlet([float(alpha)] * width, length) * 256.0
    beta = rng.beta(alpha, alpha, length)
    out = np.zeros((length, width + 1), dtype=np.int32)
    w = np.floor(p).astype(np.int64)
    for i in range(length):
        for j in np.argsort(-(p[i] - w[i]), kind="stable")[:256 - int(w[i].sum())]:
            w[i, j] += 1
    out[:, :width] = w
    out[:, width] = np.floor(beta * 65536.0 + 0.5).astype(np.int64)
    return out


def augmix_draw(seed: int, step: int, n: int, width: int, depth: int, op_table,
                table_len: int = AM_TABLE_LEN) -> tuple:
    """Image n's draw at step `step`: (table index, [[(op, sign)] * depth_i] * width).
    depth -1 draws each chain's 1..3.  Integers only; exact for steps >= 2**32."""
    if step < 0 or n < 0 or not 1 <= width <= AM_MAX_WIDTH or len(op_table) < 1 or table_len < 1:
        raise ValueError("need step >= 0, n >= 0, 1 <= width <= 4, a non-empty op table and "
                         "table_len >= 1")
    if depth != -1 and not 1 <= depth <= AM_MAX_DEPTH:
        raise ValueError(f"augmix depth must be -1 or in 1..3, got {depth!r}")
    h = splitmix(splitmix((seed & _M64) ^ AM_SALT) ^ splitmix((step * 0x100000001B3 + n) & _M64))
    chains = []
    for i in range(width):
        hc = splitmix(h ^ ((i + 1) << 8))
        ops = []
        for k in range(depth if depth > 0 else 1 + (hc & 0xFFFFFFFF) % 3):
            hk = splitmix(hc ^ (k + 1))
            ops.append((int(op_table[(hk & 0xFFFFFFFF) % len(op_table)]), (hk >> 32) & 1))
        chains.append(ops)
    return (h & 0xFFFFFFFF) % table_len, chains


def augmix_log(draw) -> np.ndarray:
    """The kernel's int32 [width, 4, 2] log of a draw: per chain {depth, table index}, then
    {op, sign} per slot, (-1, -1) for a slot that was not run."""
    index, chains = draw
    log = np.full((len(chains), 1 + AM_MAX_DEPTH, 2), -1, dtype=np.int32)
    for i, ops in enumerate(chains):
        log[i, 0] = (len(ops), index)
        log[i, 1:1 + len(ops)] = ops
    return log


def augmix_image(img_hwc_u8: np.ndarray, chains, entry, tables) -> np.ndarray:
    """The uint8 [H, W, 3] image after AugMix with the chains of augmix_draw and the table
    entry (w_0..w_{width-1}, m)."""
    o = np.asarray(img_hwc_u8)
    w, m = [int(v) for v in entry[:-1]], int(entry[-1])
    if len(w) != len(chains) or sum(w) != 256 or min(w) < 0 or not 0 <= m <= 65536:
        raise ValueError("an augmix table entry is one Q8 weight per chain, summing to 256, and "
                         f"m in 0..65536; got {list(entry)!r} for {len(chains)} chain(s)")
    acc = np.zeros(o.shape, dtype=np.int64)
    for wi, ops in zip(w, chains):
        acc += wi * randaug_image(o, ops, tables).astype(np.int64)
    out = ((65536 - m) * (o.astype(np.int64) << 8) + m * acc + (1 << 23)) >> 24
    return out.astype(np.uint8)


def augmix_batch(batch_u8, layout: str, seed: int, step: int, width: int = 3, depth: int = -1,
                 severity: int = 3, op_table=None, tables=None, mix_table=None,
                 alpha: float = 1.0):
    """The AugMix batch and the [N, width, 4, 2] int32 log (augmix_log).  layout "chw":
    [N, 3, H, W] (the CIFAR records), "hwc": [N, H, W, 3] (the ImageNet crops).  mix_table
    defaults to augmix_tables(width, alpha, seed)."""
    if layout not in ("chw", "hwc"):
        raise ValueError(f"layout must be chw or hwc, got {layout!r}")
    if isinstance(severity, bool) or int(severity) != severity or \
            not 0 <= severity <= AM_MAX_SEVERITY:
        raise ValueError(f"augmix severity must be an integer in 0..10, got {severity!r}")
    x = np.asarray(batch_u8)
    hwc = x.transpose(0, 2, 3, 1) if layout == "chw" else x
    N, H, W, _ = hwc.shape
    op_table = augmix_op_table() if op_table is None else op_table
    tables = randaug_tables(3 * int(severity), H, W) if tables is None else tables
    mix_table = augmix_tables(width, alpha, seed) if mix_table is None else np.asarray(mix_table)
    if mix_table.ndim != 2 or mix_table.shape[1] != width + 1:
        raise ValueError(f"the mixing table must be [entries, {width + 1}]")
    out = np.empty_like(hwc)
    log = np.zeros((N, width, 1 + AM_MAX_DEPTH, 2), dtype=np.int32)
    for n in range(N):
        draw = augmix_draw(seed, step, n, width, depth, op_table, len(mix_table))
        log[n] = augmix_log(draw)
        out[n] = augmix_image(hwc[n], draw[1], mix_table[draw[0]], tables)
    out = out.transpose(0, 3, 1, 2) if layout == "chw" else out
    return np.ascontiguousarray(out), log


def augmix_fanout(batch_u8, labels, layout: str, seed: int, step: int, width: int = 3,
                  depth: int = -1, severity: int = 3, op_table=None, tables=None,
                  mix_table=None, alpha: float = 1.0):
    """AugMix's three views for the Jensen-Shannon loss: B images and labels ->
    ([3B, ...] uint8, [3B] labels, [3B, width, 4, 2] log).  Position p holds source image
    p % B: p < B is a copy (the clean view; its log rows are -1), p >= B runs the chains of
    augmix_batch keyed on the OUTPUT position p, so the two views of one image differ."""
    x, y = np.asarray(batch_u8), np.asarray(labels)
    B = len(x)
    if len(y) != B:
        raise ValueError(f"{B} images but {len(y)} labels")
    rep = np.concatenate([x, x, x])
    # augmix_batch keys image n of its batch on n: positions 0..3B-1, of which B.. are kept
    out, log = augmix_batch(rep, layout, seed, step, width, depth, severity, op_table, tables,
                            mix_table, alpha)
    out[:B], log[:B] = x, -1
    return out, np.concatenate([y, y, y]), log
