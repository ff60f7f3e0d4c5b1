"""An independent reference for CutMix (Yun et al. 2019) as this project draws it: the
per-step draw written out in plain Python integers, the box-size table in fp64 and the paste.

Plain Python / numpy; nothing here calls data/cifar.py, the kernels or the engine.

  h      = mix(mix(seed ^ "MIXUP!") ^ mix(step * 0x100000001B3 mod 2^64))      (mixup's hash)
  index  = (h mod 2^32) mod table_len;  shift = 1 + (h >> 32) mod (batch - 1)  (0 for batch 1)
  h2     = mix(h ^ "CUTMIX");  cut = (h2 >> 40) < thresh                       (24 bits)
  centre = ((h2 & 0xFFFF) mod H, ((h2 >> 16) & 0xFFFF) mod W)
  box    = [cy - ch // 2, cy + ch // 2) x [cx - cw // 2, cx + cw // 2), clipped to the image
  lam    = fp32(H * W - area) / fp32(H * W), one correctly rounded fp32 division
  table  : lam' ~ Beta(alpha, alpha), r = sqrt(1 - lam') in fp64, (ch, cw) = (int(H r), int(W r))
  pixel  = partner's inside the box, own outside (a select)
"""
from fractions import Fraction

import numpy as np

M64 = (1 << 64) - 1
MIXUP_SALT = int.from_bytes(b"MIXUP!", "big")
CUTMIX_SALT = int.from_bytes(b"CUTMIX", "big")


def mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def fp32_quotient(num, den):
    """num / den (integers below 2^24) rounded once to fp32, through exact rationals."""
    q = Fraction(num, den)
    f = np.float32(float(q))
    # the candidate and its two fp32 neighbours, compared exactly: f is the nearest
    lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
    best = min((lo, f, hi), key=lambda c: abs(Fraction(float(c)) - q))
    assert best == f
    return f


def draw(seed, step, batch, table_len, H, W, entries, thresh):
    h = mix(mix((seed & M64) ^ MIXUP_SALT) ^ mix((step * 0x100000001B3) & M64))
    d = {"index": (h & 0xFFFFFFFF) % table_len,
         "shift": 1 + (h >> 32) % (batch - 1) if batch >= 2 else 0}
    h2 = mix(h ^ CUTMIX_SALT)
    d["cut"] = (h2 >> 40) < thresh
    if not d["cut"]:
        return d
    e = int(entries[d["index"]])
    ch, cw = e >> 16, e & 0xFFFF
    cy, cx = (h2 & 0xFFFF) % H, ((h2 >> 16) & 0xFFFF) % W
    y0, y1 = max(cy - ch // 2, 0), min(cy + ch // 2, H)
    x0, x1 = max(cx - cw // 2, 0), min(cx + cw // 2, W)
    area = (y1 - y0) * (x1 - x0)
    d.update(cy=cy, cx=cx, y0=y0, y1=y1, x0=x0, x1=x1, area=area,
             lam=fp32_quotient(H * W - area, H * W))
    return d


def table(lam, H, W):
    """fp32 Beta draws -> the ch << 16 | cw entries, each through Python floats (fp64)."""
    out = []
    for v in np.asarray(lam, dtype=np.float32):
        r = (1.0 - float(v)) ** 0.5
        out.append(int(H * r) << 16 | int(W * r))
    return np.array(out, dtype=np.int64)


def paste(x, shift, box):
    """x [N, H, W, ...]: position n with the box (y0, y1, x0, x1) of position (n + shift) % N."""
    x = np.asarray(x)
    y0, y1, x0, x1 = box
    out = x.copy()
    partner = np.roll(x, -shift, axis=0)
    out[:, y0:y1, x0:x1] = partner[:, y0:y1, x0:x1]
    return out


def entry(ch, cw):
    return ch << 16 | cw
