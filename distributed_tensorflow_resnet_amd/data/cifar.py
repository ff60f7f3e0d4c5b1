"""CIFAR-10 / CIFAR-100 binary input pipeline.

Record layouts (resnet_cifar_main.py:150-198, cifar_input.py:25-119):
  CIFAR-10   <1 x label><3072 x pixel>               3073 bytes, files
             cifar-10-batches-bin/data_batch_{1..5}.bin, test_batch.bin
  CIFAR-100  <1 x coarse><1 x fine label><3072 x pixel>  3074 bytes (fine label
             used, label_offset=1), files cifar-100-binary/{train,test}.bin
Pixels are depth-major [3][32][32] -- exactly what the device augmentation
kernel (csrc/data.hip cifar_augment) consumes, so the GPU path ships raw uint8
records to the device and pads/crops/flips/standardizes there.  The CPU path
(augment_cpu) implements the same transform with torch ops.

Fixes reference defect #7 (CIFAR-100 training hard-coded to CIFAR-10 records).
"""
from __future__ import annotations

import glob
import os

import numpy as np
import torch

HEIGHT = WIDTH = 32
DEPTH = 3
IMAGE_BYTES = HEIGHT * WIDTH * DEPTH
NUM_IMAGES = {"train": 50000, "validation": 10000}


def record_layout(dataset: str) -> tuple[int, int, int]:
    """(label_offset, label_bytes, num_classes)."""
    if dataset == "cifar10":
        return 0, 1, 10
    if dataset == "cifar100":
        return 1, 1, 100
    raise ValueError(f"Not supported dataset {dataset}")


def get_filenames(is_training: bool, data_dir: str, dataset: str = "cifar10") -> list[str]:
    """Directory (reference layout), explicit file, or glob pattern."""
    if any(ch in data_dir for ch in "*?["):
        files = sorted(glob.glob(data_dir))
    elif os.path.isfile(data_dir):
        files = [data_dir]
    else:
        if dataset == "cifar10":
            sub = os.path.join(data_dir, "cifar-10-batches-bin")
            base = sub if os.path.isdir(sub) else data_dir
            names = ([f"data_batch_{i}.bin" for i in range(1, 6)] if is_training
                     else ["test_batch.bin"])
        else:
            sub = os.path.join(data_dir, "cifar-100-binary")
            base = sub if os.path.isdir(sub) else data_dir
            names = ["train.bin"] if is_training else ["test.bin"]
        files = [os.path.join(base, n) for n in names]
    missing = [f for f in files if not os.path.exists(f)]
    if not files or missing:
        raise FileNotFoundError(f"CIFAR data not found: {missing or data_dir}")
    return files


def load_records(files: list[str], dataset: str = "cifar10") -> tuple[np.ndarray, np.ndarray]:
    """-> images uint8 [N, 3, 32, 32] (depth-major, as stored), labels int64 [N]."""
    off, lb, _ = record_layout(dataset)
    rec = off + lb + IMAGE_BYTES
    imgs, labels = [], []
    for f in files:
        raw = np.fromfile(f, dtype=np.uint8)
        if raw.size % rec:
            raise IOError(f"{f}: size {raw.size} is not a multiple of record size {rec}")
        raw = raw.reshape(-1, rec)
        labels.append(raw[:, off].astype(np.int64))
        imgs.append(raw[:, off + lb:].reshape(-1, DEPTH, HEIGHT, WIDTH))
    return np.concatenate(imgs), np.concatenate(labels)


def write_records(path: str, images: np.ndarray, labels: np.ndarray, dataset: str = "cifar10"):
    """Write images [N,3,32,32] uint8 + labels in the binary layout (fixtures/tools)."""
    off, _, _ = record_layout(dataset)
    n = images.shape[0]
    out = np.zeros((n, off + 1 + IMAGE_BYTES), dtype=np.uint8)
    if off:
        out[:, 0] = (labels // 5).astype(np.uint8)  # coarse label placeholder
    out[:, off] = labels.astype(np.uint8)
    out[:, off + 1:] = images.reshape(n, -1)
    out.tofile(path)


def augment_cpu(img_u8: torch.Tensor, train: bool, generator: torch.Generator | None = None,
                pad: int = 4) -> torch.Tensor:
    """[N,3,H,W] uint8 -> standardized float NHWC (pad/crop/flip/standardize)."""
    x = img_u8.float().permute(0, 2, 3, 1)  # NHWC
    N, H, W, C = x.shape
    if train:
        xp = torch.zeros(N, H + 2 * pad, W + 2 * pad, C)
        xp[:, pad:pad + H, pad:pad + W] = x
        oy = torch.randint(0, 2 * pad + 1, (N,), generator=generator)
        ox = torch.randint(0, 2 * pad + 1, (N,), generator=generator)
        flip = torch.randint(0, 2, (N,), generator=generator).bool()
        out = torch.empty_like(x)
        for i in range(N):
            c = xp[i, oy[i]:oy[i] + H, ox[i]:ox[i] + W]
            out[i] = c.flip(1) if flip[i] else c
        x = out
    flat = x.reshape(N, -1)
    mean = flat.mean(1, keepdim=True)
    std = flat.std(1, unbiased=False, keepdim=True)
    adj = torch.clamp(std, min=1.0 / (flat.shape[1] ** 0.5))
    return ((flat - mean) / adj).reshape(N, H, W, C)


class CifarData:
    """In-memory CIFAR split with rank-sharded, epoch-shuffled batching."""

    def __init__(self, data_path: str, dataset: str = "cifar10", train: bool = True):
        self.dataset = dataset
        self.train = train
        self.files = get_filenames(train, data_path, dataset)
        self.images, self.labels = load_records(self.files, dataset)
        self.num_classes = record_layout(dataset)[2]

    def __len__(self):
        return self.images.shape[0]

    def batches(self, batch_size: int, *, shuffle: bool | None = None, num_epochs: int | None = None,
                seed: int = 0, rank: int = 0, world: int = 1):
        """Yield (uint8 [B,3,32,32], int64 [B]) for this rank: each epoch a fresh
        permutation (same on every rank) is split into disjoint rank shards, like
        tf.data shuffle(50000) per worker; the tail that does not fill a batch on
        every rank is dropped."""
        shuffle = self.train if shuffle is None else shuffle
        n = len(self)
        epoch = 0
        rng = np.random.default_rng(seed)
        while num_epochs is None or epoch < num_epochs:
            perm = rng.permutation(n) if shuffle else np.arange(n)
            per_rank = (n // world) // batch_size * batch_size
            mine = perm[rank * per_rank:(rank + 1) * per_rank] if world > 1 else perm
            for s in range(0, len(mine) - batch_size + 1, batch_size):
                idx = np.sort(mine[s:s + batch_size]) if not shuffle else mine[s:s + batch_size]
                yield torch.from_numpy(self.images[idx]), torch.from_numpy(self.labels[idx])
            epoch += 1


# ---------------------------------------------------------------- resident split
# The device-resident input (csrc/data.hip cifar_augment_resident_kernel) keeps the
# whole split on the GPU and lets every workgroup pick its own record.  The functions
# below are the specification of that choice: the kernel must equal resident_index for
# every input.  The order is a pure function of (key_seed, step), so a resumed run
# continues the same epoch at the same position.
_M64 = (1 << 64) - 1


def splitmix(x: int) -> int:
    """The 64-bit finalizer of csrc/data.hip (splitmix64's output function)."""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def resident_half_bits(records: int) -> int:
    """Half width of the Feistel network: its 2*hb-bit domain covers `records`."""
    return max(1, -(-(records - 1).bit_length() // 2))


def resident_key(key_seed: int, epoch: int) -> int:
    return splitmix((key_seed & _M64) ^ splitmix(epoch & _M64))


def resident_perm(key: int, p: int, records: int) -> int:
    """Position p < records -> record index: a balanced 4-round Feistel network over
    2*hb bits, walked until the output falls inside [0, records) (cycle walking keeps
    it a bijection of the records; the domain is at most 4x the record count)."""
    if not 0 <= p < records:
        raise ValueError(f"position {p} outside [0, {records})")
    hb = resident_half_bits(records)
    mask = (1 << hb) - 1
    x = p
    while True:
        left, right = x >> hb, x & mask
        for r in range(4):
            f = splitmix(key ^ ((r + 1) << 40) ^ right) & mask
            left, right = right, left ^ f
        x = (left << hb) | right
        if x < records:
            return x


def upload_resident(split, spec, device):
    """(images uint8 [M,3,32,32], labels [M]) as host arrays or tensors -> the device
    copies the resident input kernel reads: contiguous uint8 records + int32 labels."""
    images, labels = split
    images = torch.as_tensor(images)
    labels = torch.as_tensor(labels)
    if images.dtype != torch.uint8 or images.dim() != 4 or \
            tuple(images.shape[1:]) != (3, spec.image_h, spec.image_w) or \
            (spec.image_h, spec.image_w) != (32, 32):
        raise ValueError("resident split: images must be uint8 [M,3,32,32], got "
                         f"{images.dtype} {tuple(images.shape)}")
    if labels.dim() != 1 or labels.shape[0] != images.shape[0]:
        raise ValueError("resident split: one label per image")
    if not 0 < images.shape[0] < 2 ** 31:
        raise ValueError("resident split: need 0 < records < 2**31")
    return (images.to(device).contiguous(),
            labels.to(device=device, dtype=torch.int32).contiguous())


def resident_steps_per_epoch(records: int, batch: int, world: int = 1) -> int:
    """Batches per rank per epoch; the tail is dropped, as in CifarData.batches."""
    s = (records // world) // batch
    if s == 0:
        raise ValueError(f"{records} records < batch {batch} x world {world}")
    return s


def resident_index(key_seed: int, step: int, n: int, batch: int, records: int, rank: int = 0,
                   world: int = 1, shuffle: bool = True) -> int:
    """Record read by batch position `n` of step `step` on `rank`.

    Every epoch of S = (records // world) // batch steps is one permutation of the
    records, keyed by (key_seed, epoch) and the same on every rank; rank r owns its
    positions [r*S*batch, (r+1)*S*batch).  ``shuffle=False`` returns the position
    itself; a single rank then also visits the tail batch (ceil(records / batch) steps
    per epoch), whose positions at or past the end of the split read the batch's first
    record -- how the evaluator pads a short last batch."""
    if not (0 <= n < batch and 0 <= rank < world and step >= 0):
        raise ValueError("need 0 <= n < batch, 0 <= rank < world, step >= 0")
    if records >= 1 << 31:
        raise ValueError("records must be < 2**31")
    s = resident_steps_per_epoch(records, batch, world)
    per_rank = s * batch
    steps = -(-records // batch) if (not shuffle and world == 1) else s
    epoch, k = divmod(step, steps)
    first = rank * per_rank + k * batch
    p = first + n
    if p >= records:   # tail batch (unshuffled, one rank)
        p = first
    if not shuffle:
        return p
    return resident_perm(resident_key(key_seed, epoch), p, records)


def resident_batch(key_seed: int, step: int, batch: int, records: int, rank: int = 0,
                   world: int = 1, shuffle: bool = True) -> np.ndarray:
    """resident_index for n = 0..batch-1 -> int64 [batch]."""
    return np.array([resident_index(key_seed, step, n, batch, records, rank, world, shuffle)
                     for n in range(batch)], dtype=np.int64)


# ---------------------------------------------------------------- mixup
# Mixup (Zhang et al. 2018) in the input launches (csrc/data.hip): batch position n trains on
# lam * x_n + (1 - lam) * x_m with the target lam * T(y_n) + (1 - lam) * T(y_m), m = (n +
# shift) % batch.  One (lam, shift) per step for the rank's whole batch, as in the paper's
# code.  The two functions below are the specification the kernels must equal: the device
# only indexes the table and evaluates the integer draw, so no sampler runs there.
MIXUP_TABLE_LEN = 4096
_MIXUP_SALT = 0x4D4958555021   # "MIXUP!"


def mixup_table(alpha: float, seed: int, length: int = MIXUP_TABLE_LEN) -> np.ndarray:
    """`length` draws from Beta(alpha, alpha) as fp32: the lam values a run cycles through
    (computed once on the host and uploaded once).  The values depend on numpy's Beta
    sampler (Generator(PCG64(seed)).beta)."""
    if not (alpha > 0 and np.isfinite(alpha)):
        raise ValueError(f"mixup alpha must be finite and > 0, got {alpha!r}")
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.beta(alpha, alpha, length).astype(np.float32)


def mixup_draw(seed: int, step: int, batch: int, table_len: int) -> tuple[int, int]:
    """(index, shift) of step `step`: lam = table[index], the partner of batch position n is
    (n + shift) % batch.  index in [0, table_len); shift in [1, batch - 1] (a rotation
    without fixed points) for batch >= 2, 0 for batch 1.  Keyed like the crops, with the
    input kernels' seed and the 64-bit step, but the seed is salted and hashed first, so the
    draw is not the crop hash splitmix(seed ^ splitmix(step * P + n)) of any image."""
    if step < 0 or batch < 1 or table_len < 1:
        raise ValueError("need step >= 0, batch >= 1, table_len >= 1")
    h = splitmix(splitmix((seed & _M64) ^ _MIXUP_SALT) ^
                 splitmix((step * 0x100000001B3) & _M64))
    index = (h & 0xFFFFFFFF) % table_len
    shift = 1 + (h >> 32) % (batch - 1) if batch >= 2 else 0
    return index, shift


# ---------------------------------------------------------------- cutmix
# CutMix (Yun et al. 2019) in the same launches: batch position n trains on its own image with
# one box replaced by the same box of position m's image, m = (n + shift) % batch as above,
# and the two-label target at lam = 1 - area / (H * W).  One box per step for the rank's whole
# batch, as in the paper's code, in the coordinates of the augmented output image (after crop
# and flip, before the space-to-depth packing).  A pasted pixel is a select, never a blend:
# every output pixel is bit for bit a pixel of one of the two unmixed images.  With both
# augmentations on, a step is a CutMix step with probability mix_switch_prob, a mixup step
# otherwise.  The functions below are the specification the kernels must equal.
_CUTMIX_SALT = 0x4355544D4958   # "CUTMIX"
CUTMIX_THRESH_ONE = 1 << 24


def _mix_hash(seed: int, step: int) -> int:
    """The 64-bit hash mixup_draw takes (index, shift) from."""
    return splitmix(splitmix((seed & _M64) ^ _MIXUP_SALT) ^
                    splitmix((step * 0x100000001B3) & _M64))


def cutmix_table(alpha: float, seed: int, H: int, W: int,
                 length: int = MIXUP_TABLE_LEN) -> np.ndarray:
    """`length` box sizes as int32 ``ch << 16 | cw``: lam ~ Beta(alpha, alpha) (mixup_table
    under a salted seed), r = sqrt(1 - lam) in fp64, ch = int(H * r), cw = int(W * r) -- the
    paper's rand_bbox.  Computed once on the host and uploaded once, so neither a sqrt nor a
    sampler runs on the device."""
    if not (0 < H < 1 << 15 and 0 < W < 1 << 15):
        raise ValueError(f"cutmix needs 0 < H, W < 2**15, got {H}x{W}")
    lam = mixup_table(alpha, seed ^ _CUTMIX_SALT, length)
    r = np.sqrt(1.0 - lam.astype(np.float64))
    ch = (H * r).astype(np.int64)
    cw = (W * r).astype(np.int64)
    return ((ch << 16) | cw).astype(np.int32)


def cutmix_thresh(mixup_alpha: float, cutmix_alpha: float, switch_prob: float) -> int:
    """The 24-bit threshold a step's draw is compared with, in [0, 2**24]: 0 = never CutMix
    (cutmix_alpha 0), 2**24 = always (mixup_alpha 0), else round(switch_prob * 2**24)."""
    if not cutmix_alpha > 0:
        return 0
    if not mixup_alpha > 0:
        return CUTMIX_THRESH_ONE
    if not 0.0 <= switch_prob <= 1.0:
        raise ValueError(f"mix_switch_prob must be in [0, 1], got {switch_prob!r}")
    return int(round(switch_prob * CUTMIX_THRESH_ONE))


def cutmix_draw(seed: int, step: int, batch: int, table_len: int, H: int, W: int,
                cut_entry_of, thresh: int) -> dict:
    """The step's draw with CutMix: ``index``, ``shift`` exactly mixup_draw's; ``cut`` whether
    this is a CutMix step ((h2 >> 40) < thresh, h2 a salted rehash of mixup_draw's hash).  A
    CutMix step also has ``cy, cx`` (the box centre), ``y0, y1, x0, x1`` (the box, clipped to
    the image), ``area`` and ``lam`` = fp32(H*W - area) / fp32(H*W), one correctly rounded
    fp32 division; (ch, cw) come from ``cut_entry_of[index]``.  A mixup step has ``lam`` None
    (it is the fp32 table's) and the box fields 0.  Integers only, but for that quotient."""
    index, shift = mixup_draw(seed, step, batch, table_len)
    if not 0 <= thresh <= CUTMIX_THRESH_ONE:
        raise ValueError(f"thresh must be in [0, 2**24], got {thresh!r}")
    h2 = splitmix(_mix_hash(seed, step) ^ _CUTMIX_SALT)
    d = {"index": index, "shift": shift, "cut": (h2 >> 40) < thresh, "lam": None,
         "cy": 0, "cx": 0, "y0": 0, "y1": 0, "x0": 0, "x1": 0, "area": 0}
    if not d["cut"]:
        return d
    entry = int(cut_entry_of[index])
    ch, cw = (entry >> 16) & 0xFFFF, entry & 0xFFFF
    cy, cx = (h2 & 0xFFFF) % H, ((h2 >> 16) & 0xFFFF) % W
    y0, y1 = max(cy - ch // 2, 0), min(cy + ch // 2, H)
    x0, x1 = max(cx - cw // 2, 0), min(cx + cw // 2, W)
    area = (y1 - y0) * (x1 - x0)
    d.update(cy=cy, cx=cx, y0=y0, y1=y1, x0=x0, x1=x1, area=area,
             lam=np.float32(H * W - area) / np.float32(H * W))
    return d


# ---------------------------------------------------------------- random erasing
# Random Erasing (Zhong et al. 2020; with a zero fill, Cutout: DeVries & Taylor 2017) in a
# launch of its own behind the input launch (csrc/erase.hip): with probability p, batch position
# n gets one rectangle of its image overwritten by the fill.  Unlike the two mixes the draw is
# per IMAGE: keyed like the crops with (seed, step, n), under a salted and hashed seed, so it is
# no image's crop hash and no step's mix hash.  The box sizes come from a host-made table
# (torchvision's RandomErasing.get_params loop in fp64), so neither a sampler nor a sqrt nor a
# log runs on the device.  The functions below are the specification the kernel must equal.
ERASE_TABLE_LEN = 4096
ERASE_SALT = 0x455241534521           # "ERASE!"
_ERASE_NOISE_SALT = 0x4E4F495345      # "NOISE"
ERASE_THRESH_ONE = 1 << 24


def erase_table(seed: int, H: int, W: int, area_min: float = 0.02, area_max: float = 1.0 / 3.0,
                aspect_min: float = 0.3, length: int = ERASE_TABLE_LEN) -> np.ndarray:
    """`length` box sizes as int32 ``eh << 16 | ew``.  Each entry is torchvision's
    RandomErasing.get_params loop in fp64 from Generator(PCG64(seed ^ salt)): up to 10 attempts
    of area = H * W * U(area_min, area_max), log r ~ U(log aspect_min, -log aspect_min),
    eh = int(round(sqrt(area * r))), ew = int(round(sqrt(area / r))), accepted when
    1 <= eh < H and 1 <= ew < W.  Ten failures give 0: that image is not erased."""
    if not (1 < H < 1 << 15 and 1 < W < 1 << 15):
        raise ValueError(f"erasing needs 1 < H, W < 2**15, got {H}x{W}")
    if not 0.0 < area_min <= area_max <= 1.0:
        raise ValueError(f"need 0 < erase_area_min <= erase_area_max <= 1, got {area_min!r}, "
                         f"{area_max!r}")
    if not 0.0 < aspect_min <= 1.0:
        raise ValueError(f"erase_aspect_min must be in (0, 1], got {aspect_min!r}")
    rng = np.random.Generator(np.random.PCG64((seed & _M64) ^ ERASE_SALT))
    lo = float(np.log(aspect_min))
    out = np.zeros(length, dtype=np.int32)
    for i in range(length):
        for _ in range(10):
            area = H * W * rng.uniform(area_min, area_max)
            r = float(np.exp(rng.uniform(lo, abs(lo))))
            eh = int(round(float(np.sqrt(area * r))))
            ew = int(round(float(np.sqrt(area / r))))
            if 1 <= eh < H and 1 <= ew < W:
                out[i] = (eh << 16) | ew
                break
    return out


def erase_thresh(p: float) -> int:
    """The 24-bit threshold an image's draw is compared with: int(round(p * 2**24))."""
    if not 0.0 <= p <= 1.0:   # NaN included
        raise ValueError(f"erase_prob must be in [0, 1], got {p!r}")
    return int(round(p * ERASE_THRESH_ONE))


def erase_noise_table(seed: int, length: int = ERASE_TABLE_LEN) -> np.ndarray:
    """`length` fp32 standard-normal draws (Generator(PCG64(seed ^ salt)).standard_normal): the
    values a noise-filled box is made of.  Element (y, x, c) of image n's box is
    table[splitmix(h2 ^ ((y * W + x) * 4 + c)) % length] (erase_noise_index), rounded to bf16
    once on the device."""
    rng = np.random.Generator(np.random.PCG64((seed & _M64) ^ _ERASE_NOISE_SALT))
    return rng.standard_normal(length).astype(np.float32)


def erase_hash(seed: int, step: int, n: int) -> int:
    """The 64-bit hash of image n's draw: the crop hash's key form under a salted, hashed seed."""
    return splitmix(splitmix((seed & _M64) ^ ERASE_SALT) ^
                    splitmix((step * 0x100000001B3 + n) & _M64))


def erase_draw(seed: int, step: int, n: int, table_len: int, H: int, W: int, entry_of,
               thresh: int) -> dict:
    """Image n's draw at step `step`: ``on`` ((h >> 40) < thresh, and its table entry is not
    0), ``index`` into the table, the box's corner ``y0, x0`` and size ``eh, ew`` (all 0 when
    off).  ``h2`` (the placement hash, also the key of the noise fill) is returned too.
    Integers only; exact for steps >= 2**32.  erase_table only makes eh < H and ew < W; the
    draw takes every entry that fits (1 <= eh <= H, 1 <= ew <= W: a hand-made table may hold
    a full row or column) and raises for one that does not, which the kernel treats as off."""
    if step < 0 or n < 0 or table_len < 1:
        raise ValueError("need step >= 0, n >= 0, table_len >= 1")
    if not 0 <= thresh <= ERASE_THRESH_ONE:
        raise ValueError(f"thresh must be in [0, 2**24], got {thresh!r}")
    h = erase_hash(seed, step, n)
    index = (h & 0xFFFFFFFF) % table_len
    h2 = splitmix(h ^ ERASE_SALT)
    d = {"on": False, "index": index, "y0": 0, "x0": 0, "eh": 0, "ew": 0, "h2": h2}
    entry = int(entry_of[index])
    if not (h >> 40) < thresh or entry == 0:
        return d
    eh, ew = (entry >> 16) & 0xFFFF, entry & 0xFFFF
    if not (1 <= eh <= H and 1 <= ew <= W):
        raise ValueError(f"table entry {index}: box {eh}x{ew} does not fit {H}x{W}")
    d.update(on=True, y0=(h2 & 0xFFFFFFFF) % (H - eh + 1), x0=(h2 >> 32) % (W - ew + 1),
             eh=eh, ew=ew)
    return d


def erase_noise_index(h2: int, y: int, x: int, c: int, W: int, length: int) -> int:
    """Index into the noise table of channel c of pixel (y, x) of a box placed by h2."""
    return splitmix(h2 ^ ((y * W + x) * 4 + c)) % length


def synthetic_batches(batch_size: int, num_classes: int = 10, seed: int = 0):
    """Endless random uint8 CIFAR-shaped records (for --synthetic)."""
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randint(0, 256, (batch_size, DEPTH, HEIGHT, WIDTH), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, num_classes, (batch_size,), generator=g)
    while True:
        yield imgs, labels
