"""Random Erasing re-derived in plain Python integers and numpy on bf16 bit patterns, next to
nothing of the package: the draw (data/cifar.py erase_draw), the fill, and the erase of a whole
input buffer in either device layout.  `erase(buf, ...)` takes the buffer before the launch as
int16 bit patterns -- NHWC [N, H, W, 8] or space-to-depth [N, H/2, W/2, 16] -- and returns the
buffer after; the GPU tests compare whole buffers."""
import numpy as np

M64 = (1 << 64) - 1
SALT = 0x455241534521   # "ERASE!"
ONE = 1 << 24


def splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def crop_hash(seed, step, n):
    """The input kernels' crop / flip hash of image n (csrc/data.hip)."""
    return splitmix((seed & M64) ^ splitmix((step * 0x100000001B3 + n) & M64))


def draw_hash(seed, step, n):
    return splitmix(splitmix((seed & M64) ^ SALT) ^ splitmix((step * 0x100000001B3 + n) & M64))


def entry(eh, ew):
    return (eh << 16) | ew


def draw(seed, step, n, table, H, W, thresh):
    """-> dict(on, index, y0, x0, eh, ew, h2); all box fields 0 when off."""
    h = draw_hash(seed, step, n)
    index = (h & 0xFFFFFFFF) % len(table)
    h2 = splitmix(h ^ SALT)
    e = int(table[index])
    d = dict(on=False, index=index, y0=0, x0=0, eh=0, ew=0, h2=h2)
    if (h >> 40) >= thresh or e == 0:
        return d
    eh, ew = e >> 16, e & 0xFFFF
    assert 1 <= eh <= H and 1 <= ew <= W
    d.update(on=True, eh=eh, ew=ew, y0=(h2 & 0xFFFFFFFF) % (H - eh + 1),
             x0=(h2 >> 32) % (W - ew + 1))
    return d


def state(seed, step, N, table, H, W, thresh):
    """What the launch logs: int [N, 5] of {on, y0, x0, eh, ew}."""
    out = np.zeros((N, 5), dtype=np.int64)
    for n in range(N):
        d = draw(seed, step, n, table, H, W, thresh)
        out[n] = (int(d["on"]), d["y0"], d["x0"], d["eh"], d["ew"])
    return out


def bf16_bits(f32):
    """fp32 array -> bf16 bit patterns (uint16), round to nearest even (finite inputs)."""
    u = np.asarray(f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def fill_bits(d, y, x, W, noise):
    """The 3 image channels of erased pixel (y, x) as bf16 bit patterns."""
    if noise is None:
        return [0, 0, 0]
    idx = [splitmix(d["h2"] ^ ((y * W + x) * 4 + c)) % len(noise) for c in range(3)]
    return bf16_bits(np.asarray(noise, dtype=np.float32)[idx]).tolist()


def erase(buf, seed, step, table, H, W, thresh, noise=None, s2d=False):
    """buf: int16 bit patterns, [N, H, W, 8] or (s2d) [N, H/2, W/2, 16] -> the buffer after the
    launch.  Only the box's pixels change: 3 fill channels, the pixel's padding channels 0."""
    buf = np.asarray(buf)
    assert buf.dtype == np.int16
    N = buf.shape[0]
    assert buf.shape == ((N, H // 2, W // 2, 16) if s2d else (N, H, W, 8))
    out = buf.copy().view(np.uint16)
    for n in range(N):
        d = draw(seed, step, n, table, H, W, thresh)
        if not d["on"]:
            continue
        for y in range(d["y0"], d["y0"] + d["eh"]):
            for x in range(d["x0"], d["x0"] + d["ew"]):
                c = fill_bits(d, y, x, W, noise)
                if s2d:
                    g = ((y & 1) * 2 + (x & 1)) * 4
                    out[n, y >> 1, x >> 1, g:g + 4] = c + [0]
                else:
                    out[n, y, x] = c + [0] * 5
    return out.view(np.int16)


def box_mask(st, H, W):
    """[N, H, W] bool: the erased pixels of a state array."""
    m = np.zeros((st.shape[0], H, W), dtype=bool)
    for n, (on, y0, x0, eh, ew) in enumerate(st.tolist()):
        if on:
            m[n, y0:y0 + eh, x0:x0 + ew] = True
    return m
