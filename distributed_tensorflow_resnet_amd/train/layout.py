"""Host tables of the training engine: the parameter-segment table (where every
trainable tensor and its bf16 copies live) and the work maps of the optimizer launches.
Pure arithmetic over the model spec -- numpy only, no device and no native module -- laid
out as the structs of csrc/optim.h that the kernels read."""
from __future__ import annotations

import numpy as np

WGD_DTYPE = np.dtype([
    ("part", "<u8"), ("grad", "<u8"), ("splits", "<i4"), ("K", "<i4"), ("Kv", "<i4"),
    ("taps", "<i4"), ("C", "<i4"), ("Cv", "<i4"), ("chunk0", "<i8"),
])

SEG_DTYPE = np.dtype([
    ("offset", "<i8"), ("numel", "<i8"), ("bf_ohwi", "<i8"), ("bf_hwio", "<i8"),
    ("kh", "<i4"), ("kw", "<i4"), ("C", "<i4"), ("K", "<i4"), ("cpad", "<i4"), ("kpad", "<i4"),
])

OPTW_DTYPE = np.dtype([   # csrc/optim.h OptWork
    ("part", "<u8"), ("tile0", "<i8"), ("splits", "<i4"), ("kslab", "<i4"), ("cslab", "<i4"),
    ("tiled", "<i4"), ("tr", "<i4"), ("tc", "<i4"),
])

OPT_TILE_LOADS = 2048   # a sgd_tiles workgroup's slab loads: <= 8 16-byte loads per thread

LARS_DTYPE = np.dtype([   # csrc/optim.h LarsSeg
    ("chunk0", "<i8"), ("nchunks", "<i4"), ("skip", "<i4"),
])
LARS_CHUNK = 4096         # csrc/optim.h LARS_CHUNK: elements per lars_norms workgroup
LARS_SKIPS = ("vectors", "none")


def _ceil(a, b):
    return (a + b - 1) // b


def _pow2ceil(x: int) -> int:
    return 1 << max(0, (int(x) - 1).bit_length())


def param_segments(spec, train_slots, *, cpad_in: int, kpad: int, stem_s2d: bool):
    """The parameter-segment table (SEG_DTYPE, one record per trainable slot, in slot
    order) and the element count of the bf16 weight buffer.  A conv weight gets a bf16
    OHWI copy (input channels padded to `cpad_in` below 8; none for a space-to-depth
    stem, whose operand comes from stem_s2d_pack) and, from 8 input channels up (the
    stem never needs dgrad), a bf16 HWIO copy; the dense kernel both, its classes padded
    to `kpad`.  bf_ohwi / bf_hwio are element offsets into that buffer, -1 = no copy."""
    conv_specs = {c.name: c for c in spec.all_convs()}
    seg_arr = np.zeros(len(train_slots), dtype=SEG_DTYPE)
    bf_total = 0
    for rec, s in zip(seg_arr, train_slots):
        rec["offset"], rec["numel"] = s.offset, s.numel
        rec["bf_ohwi"] = rec["bf_hwio"] = -1
        if s.kind == "conv":
            c = conv_specs[s.name.split("/")[0]]
            taps = c.kh * c.kw
            cpad = cpad_in if c.cin < 8 else c.cin
            rec["kh"], rec["kw"], rec["C"], rec["K"] = c.kh, c.kw, c.cin, c.cout
            rec["cpad"], rec["kpad"] = cpad, c.cout
            if not (stem_s2d and c.name == spec.stem.name):
                rec["bf_ohwi"] = bf_total
                bf_total += c.cout * taps * cpad
            if c.cin >= 8:
                rec["bf_hwio"] = bf_total
                bf_total += taps * c.cin * c.cout
        elif s.kind == "dense_kernel":
            F, classes = s.shape
            rec["kh"], rec["kw"], rec["C"], rec["K"] = 1, 1, F, classes
            rec["cpad"], rec["kpad"] = F, kpad
            rec["bf_ohwi"] = bf_total
            bf_total += kpad * F
            rec["bf_hwio"] = bf_total
            bf_total += F * kpad
        else:
            rec["kh"] = rec["kw"] = rec["C"] = rec["K"] = rec["cpad"] = rec["kpad"] = 1
    return seg_arr, bf_total


def opt_tile(R: int, K: int, splits: int, cslab: int, C: int, taps: int, nosplit=(64, 64)):
    """Tile (rows tap*C+ci, output channels) of a weight in the one-launch optimizer
    (csrc/optim.hip sgd_tiles_kernel): 64 x 64 without slabs; with `splits` slabs the
    tile shrinks (columns first) until its float4 slab loads fit OPT_TILE_LOADS and,
    past 8 splits (4 thread groups of 64 float4 units), until it has <= 64 units.
    Padded slab rows (cslab != C, the stem) keep all rows in one tile."""
    if splits == 0:
        return nosplit
    units_max = 64 if splits > 8 else 1 << 30
    TC = min(64, _pow2ceil(K))
    if cslab != C:
        assert R <= 64 and (taps * cslab) % 4 == 0, (R, taps, cslab)
        cols4 = taps * cslab // 4
        while TC > 1 and (TC * cols4 * splits > OPT_TILE_LOADS or TC * cols4 > units_max):
            TC //= 2
        assert TC * cols4 <= units_max, (R, K, splits, cslab)
        return R, TC
    assert C % 4 == 0, C
    TR = min(64, _pow2ceil(R))
    while (TR * TC // 4) * splits > OPT_TILE_LOADS or TR * TC // 4 > units_max:
        if TC >= TR and TC > 1:
            TC //= 2
        elif TR > 4:
            TR //= 2
        else:
            break
    assert TR * TC // 4 <= units_max, (R, K, splits)
    return TR, TC


def lars_tables(seg_arr, skip):
    """The work map of lars_norms / lars_trust (csrc/lars.hip): per parameter segment its
    first workgroup, its number of LARS_CHUNK-element chunks and whether it is skipped
    (trust = 1).  Returns the LarsSeg table (numpy, LARS_DTYPE) and blk_seg (a list: the
    segment of each lars_norms workgroup)."""
    assert len(skip) == len(seg_arr)
    tab = np.zeros(len(seg_arr), dtype=LARS_DTYPE)
    blk = []
    for i, rec in enumerate(seg_arr):
        n = -(-int(rec["numel"]) // LARS_CHUNK)
        tab[i] = (len(blk), n, int(bool(skip[i])))
        blk += [i] * n
    return tab, blk


def lars_trust_summary(state):
    """min / median / max trust ratio over a lars_state() dict (metrics.jsonl, the log)."""
    t = sorted(v[2] for v in state.values())
    if not t:
        return {}
    return {"lars_trust_min": t[0], "lars_trust_median": t[len(t) // 2], "lars_trust_max": t[-1]}


CLIP_CHUNK = 4096         # csrc/optim.h CLIP_CHUNK: elements per grad_sqnorm workgroup
OPT_FUSED_CLIP_REASON = ("clip_grad_norm: the norm is taken over the complete gradient, "
                         "before the update")


OPTIMIZERS = ("mom", "sgd", "lars", "adamw", "lion", "rmsprop")
ADAM_DECAYS = ("decoupled", "l2")
ADAM_DECAY_SKIPS = ("none", "vectors")
OPT_FUSED_ADAM_REASON = ("optimizer adamw: the one-launch optimizer is SGD-momentum; adamw takes "
                         "the generic optimizer launches")


def check_adam(beta1, beta2, epsilon, decay: str = "decoupled", decay_skip: str = "none"):
    """The adamw flags as both backends take them: (beta1, beta2, epsilon) as floats.  The
    betas are in [0, 1); epsilon > 0 (with 0 an element whose gradient is zero would be
    0 / 0) and finite."""
    try:
        b1, b2, eps = float(beta1), float(beta2), float(epsilon)
    except (TypeError, ValueError):
        raise ValueError(f"adam_beta1, adam_beta2 and adam_epsilon must be numbers, got "
                         f"{beta1!r}, {beta2!r}, {epsilon!r}") from None
    for name, b in (("adam_beta1", b1), ("adam_beta2", b2)):
        if not 0.0 <= b < 1.0:   # NaN included
            raise ValueError(f"{name} must be in [0, 1), got {b!r}")
    # (as the kernel's float argument: a positive value fp32 rounds to 0 is no epsilon)
    if not 0.0 < float(np.float32(eps)) < float("inf"):
        raise ValueError(f"adam_epsilon must be positive (and finite in fp32), got {eps!r}")
    if float(np.float32(b1)) >= 1.0 or float(np.float32(b2)) >= 1.0:
        raise ValueError(f"adam_beta1 and adam_beta2 must be below 1 in fp32, got {b1!r}, {b2!r}")
    if decay not in ADAM_DECAYS:
        raise ValueError(f"adam_decay must be one of {ADAM_DECAYS}, got {decay!r}")
    if decay_skip not in ADAM_DECAY_SKIPS:
        raise ValueError(f"adam_decay_skip must be one of {ADAM_DECAY_SKIPS}, got {decay_skip!r}")
    return b1, b2, eps


ADAM_TRUSTS = ("off", "on")
ADAM_TRUST_SKIPS = ("vectors", "none")
OPT_FUSED_LAMB_REASON = ("optimizer adamw with adam_trust on (LAMB): the trust ratio needs the "
                         "norm of the whole Adam direction, after the moments and before any "
                         "weight moves; it takes three generic launches")


def check_adam_trust(trust="off", trust_skip: str = "vectors", optimizer: str = "adamw") -> bool:
    """--adam_trust / --adam_trust_skip as both backends take them: whether layer-wise
    adaptation (LAMB, csrc/lamb.hip) is on.  `trust` is 'off' / 'on' (or a bool); 'on' needs
    the adamw optimizer; the skip is accepted and unused without it, as lars_skip is."""
    if isinstance(trust, bool):
        trust = "on" if trust else "off"
    if trust not in ADAM_TRUSTS:
        raise ValueError(f"adam_trust must be one of {ADAM_TRUSTS}, got {trust!r}")
    if trust_skip not in ADAM_TRUST_SKIPS:
        raise ValueError(f"adam_trust_skip must be one of {ADAM_TRUST_SKIPS}, got {trust_skip!r}")
    if trust == "on" and optimizer != "adamw":
        raise ValueError(f"adam_trust on is layer-wise adaptation of adamw: it cannot be combined "
                         f"with optimizer {optimizer!r}")
    return trust == "on"


OPT_FUSED_LION_REASON = ("optimizer lion: the one-launch optimizer is SGD-momentum; lion takes "
                         "the generic optimizer launches")


def check_lion(beta1, beta2, decay_skip: str = "none"):
    """The lion flags as both backends take them: (beta1, beta2) as floats, both in [0, 1)
    (in fp32 too, as the kernel's float arguments); decay_skip as adam_decay_skip."""
    try:
        b1, b2 = float(beta1), float(beta2)
    except (TypeError, ValueError):
        raise ValueError(f"lion_beta1 and lion_beta2 must be numbers, got "
                         f"{beta1!r}, {beta2!r}") from None
    for name, b in (("lion_beta1", b1), ("lion_beta2", b2)):
        if not 0.0 <= b < 1.0:   # NaN included
            raise ValueError(f"{name} must be in [0, 1), got {b!r}")
    if float(np.float32(b1)) >= 1.0 or float(np.float32(b2)) >= 1.0:
        raise ValueError(f"lion_beta1 and lion_beta2 must be below 1 in fp32, got {b1!r}, {b2!r}")
    if decay_skip not in ADAM_DECAY_SKIPS:
        raise ValueError(f"lion_decay_skip must be one of {ADAM_DECAY_SKIPS}, got {decay_skip!r}")
    return b1, b2


OPT_FUSED_RMSPROP_REASON = ("optimizer rmsprop: the one-launch optimizer is SGD-momentum; rmsprop "
                            "takes the generic optimizer launches")
RMSPROP_WDS = ("l2", "decoupled")


def check_rmsprop(rho, momentum, epsilon, centered=False, wd: str = "l2",
                  decay_skip: str = "none"):
    """The rmsprop flags as both backends take them: (rho, momentum, epsilon, centered) as
    floats and a bool.  rho and momentum are in [0, 1) (in fp32 too, as the kernel's float
    arguments); epsilon > 0 and finite in fp32 (it sits inside the square root: with 0 an
    element whose gradient and ms are zero would be 0 / 0); wd is the decay mode, decay_skip
    as adam_decay_skip.  (adam_trust on with rmsprop is check_adam_trust's to refuse.)"""
    try:
        r, mo, eps = float(rho), float(momentum), float(epsilon)
    except (TypeError, ValueError):
        raise ValueError(f"rmsprop_rho, rmsprop_momentum and rmsprop_epsilon must be numbers, "
                         f"got {rho!r}, {momentum!r}, {epsilon!r}") from None
    for name, b in (("rmsprop_rho", r), ("rmsprop_momentum", mo)):
        if not 0.0 <= b < 1.0:   # NaN included
            raise ValueError(f"{name} must be in [0, 1), got {b!r}")
    if float(np.float32(r)) >= 1.0 or float(np.float32(mo)) >= 1.0:
        raise ValueError(f"rmsprop_rho and rmsprop_momentum must be below 1 in fp32, got "
                         f"{r!r}, {mo!r}")
    if not 0.0 < float(np.float32(eps)) < float("inf"):
        raise ValueError(f"rmsprop_epsilon must be positive (and finite in fp32), got {eps!r}")
    if wd not in RMSPROP_WDS:
        raise ValueError(f"rmsprop_wd must be one of {RMSPROP_WDS}, got {wd!r}")
    if decay_skip not in ADAM_DECAY_SKIPS:
        raise ValueError(f"rmsprop_decay_skip must be one of {ADAM_DECAY_SKIPS}, got "
                         f"{decay_skip!r}")
    return r, mo, eps, bool(centered)


def lamb_bias_corrections(t: int, beta1: float, beta2: float):
    """Host mirror of the device's k1 = 1 / (1 - b1^t), k2 = 1 / (1 - b2^t) (csrc/lamb.hip):
    fp64 from the fp32 coefficients, 1 - b^t as -expm1(t * log(b)), each rounded to fp32 once."""
    import math

    def k(b):
        b = float(np.float32(b))
        return float(np.float32(1.0 / (1.0 if b == 0.0 else -math.expm1(t * math.log(b)))))

    t = max(1, int(t))
    return k(beta1), k(beta2)


def lamb_trust_summary(state):
    """min / median / max trust ratio over a lamb_state() dict (lars_trust_summary's shape)."""
    t = sorted(v[2] for v in state.values())
    if not t:
        return {}
    return {"lamb_trust_min": t[0], "lamb_trust_median": t[len(t) // 2], "lamb_trust_max": t[-1]}


def adam_decay_table(shapes, wd: float, decay_skip: str = "none"):
    """wd_seg of adam_update_pack (csrc/adam.hip): the fp32 weight decay of each parameter
    segment, in slot order.  `shapes`: the trainables' shapes.  'none' decays every
    trainable (this project's rule); 'vectors' gives every rank-1 tensor (BN gamma / beta,
    the dense bias) 0."""
    if decay_skip not in ADAM_DECAY_SKIPS:
        raise ValueError(f"adam_decay_skip must be one of {ADAM_DECAY_SKIPS}, got {decay_skip!r}")
    return np.array([0.0 if decay_skip == "vectors" and len(s) == 1 else wd for s in shapes],
                    dtype=np.float32)


def adam_alpha(lr: float, t: int, beta1: float, beta2: float) -> float:
    """Host mirror of the device's bias-corrected rate (csrc/adam.hip): lr * sqrt(1 - b2^t) /
    (1 - b1^t) in fp64 from the fp32 coefficients, 1 - b^t as -expm1(t * log(b)), rounded to
    fp32 once."""
    import math

    def om_pow(b):
        b = float(np.float32(b))
        return 1.0 if b == 0.0 else -math.expm1(t * math.log(b))

    t = max(1, int(t))
    return float(np.float32(float(np.float32(lr)) * math.sqrt(om_pow(beta2)) / om_pow(beta1)))


# input modes whose step has an input launch mixup can be built into
MIXUP_INPUT_MODES = ("cifar_u8", "cifar_resident", "imagenet_u8")


def check_mixup_alpha(alpha) -> float:
    """--mixup_alpha as both backends take it: 0 = off, else the (finite, positive)
    parameter of the Beta(alpha, alpha) the blend weights are drawn from."""
    try:
        alpha = float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f"mixup_alpha must be a number, got {alpha!r}") from None
    if not 0.0 <= alpha < float("inf"):   # negative, inf or NaN
        raise ValueError(f"mixup_alpha must be finite and >= 0, got {alpha!r}")
    return alpha


def check_cutmix_alpha(alpha) -> float:
    """--cutmix_alpha as both backends take it: 0 = off, else the (finite, positive)
    parameter of the Beta(alpha, alpha) the pasted box's area share is drawn from."""
    try:
        alpha = float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f"cutmix_alpha must be a number, got {alpha!r}") from None
    if not 0.0 <= alpha < float("inf"):   # negative, inf or NaN
        raise ValueError(f"cutmix_alpha must be finite and >= 0, got {alpha!r}")
    return alpha


def check_mix_switch_prob(p) -> float:
    """--mix_switch_prob as both backends take it: the probability, in [0, 1], that a step
    is a CutMix step when mixup and CutMix are both on."""
    try:
        p = float(p)
    except (TypeError, ValueError):
        raise ValueError(f"mix_switch_prob must be a number, got {p!r}") from None
    if not 0.0 <= p <= 1.0:   # NaN included
        raise ValueError(f"mix_switch_prob must be in [0, 1], got {p!r}")
    return p


ERASE_FILLS = ("zero", "noise")


def check_erase(prob, area_min=0.02, area_max=1.0 / 3.0, aspect_min=0.3, fill="zero",
                dataset: str = "") -> tuple:
    """--erase_prob and its sub-flags as both backends take them -> (prob, area_min, area_max,
    aspect_min, fill): prob in [0, 1] (0 = off), 0 < area_min <= area_max <= 1, aspect_min in
    (0, 1], fill zero | noise.  Noise is refused for ImageNet: those inputs are mean-subtracted
    but not scaled, so unit noise is a constant there, and zero is already the mean pixel."""
    try:
        prob, area_min, area_max, aspect_min = (float(v) for v in
                                                (prob, area_min, area_max, aspect_min))
    except (TypeError, ValueError):
        raise ValueError("erase_prob, erase_area_min, erase_area_max and erase_aspect_min must "
                         "be numbers") from None
    if not 0.0 <= prob <= 1.0:   # NaN included
        raise ValueError(f"erase_prob must be in [0, 1], got {prob!r}")
    if not 0.0 < area_min <= area_max <= 1.0:
        raise ValueError(f"need 0 < erase_area_min <= erase_area_max <= 1, got {area_min!r}, "
                         f"{area_max!r}")
    if not 0.0 < aspect_min <= 1.0:
        raise ValueError(f"erase_aspect_min must be in (0, 1], got {aspect_min!r}")
    if fill not in ERASE_FILLS:
        raise ValueError(f"erase_fill must be one of {ERASE_FILLS}, got {fill!r}")
    if fill == "noise" and str(dataset).startswith("imagenet"):
        raise ValueError("erase_fill noise is not for ImageNet: its inputs are mean-subtracted "
                         "but not scaled, so unit noise is a constant there (zero is the mean "
                         "pixel)")
    return prob, area_min, area_max, aspect_min, fill


def check_clip_grad_norm(c, optimizer: str) -> float:
    """--clip_grad_norm as both backends take it: 0 = off, a positive number or inf (inf:
    the norm is measured, the scale is exactly 1); not together with lars, whose trust
    ratio already normalises by the gradient norm."""
    try:
        c = float(c)
    except (TypeError, ValueError):
        raise ValueError(f"clip_grad_norm must be a number, got {c!r}") from None
    if not c >= 0.0:   # negative or NaN
        raise ValueError(f"clip_grad_norm must be 0 (off), positive or inf, got {c!r}")
    if c > 0 and optimizer == "lars":
        raise ValueError("clip_grad_norm cannot be combined with optimizer lars: the trust "
                         "ratio already normalises by the gradient norm")
    return c


def sgd_tiles_work(seg_arr, seg_names, slabs, gptr: int, names=None, nosplit=(64, 64)):
    """The work map of the one-launch optimizer (csrc/optim.hip sgd_tiles_kernel): per
    parameter segment its slab (split-K partials still to be summed, or none: the
    gradient is in `grad`, at device address gptr) and its first workgroup; weights with
    bf16 copies or slabs go in tiles of their HWIO master (opt_tile), other tensors in
    1024-element chunks.  `names`: only those segments get workgroups (a bucket's pack
    launch).  Returns the OptWork table (numpy, OPTW_DTYPE) and blk_seg (a list)."""
    work = np.zeros(len(seg_arr), dtype=OPTW_DTYPE)
    blk = []
    for i, (rec, name) in enumerate(zip(seg_arr, seg_names)):
        if names is not None and name not in names:
            continue
        d = slabs.get(name)
        taps, C, K = int(rec["kh"] * rec["kw"]), int(rec["C"]), int(rec["K"])
        tiled = d is not None or rec["bf_ohwi"] >= 0 or rec["bf_hwio"] >= 0
        part, splits, kslab, cslab = 0, 0, 0, 0
        if d is not None:
            part, grad, splits, kslab, Kv, dtaps, cslab, Cv = d
            assert (grad, Kv, dtaps, Cv) == (gptr + 4 * int(rec["offset"]), K, taps, C), name
            assert kslab >= K and cslab >= C and part % 16 == 0, name
        tr = tc = 0
        if tiled:
            assert taps * C * K == rec["numel"], name
            tr, tc = opt_tile(taps * C, K, splits, cslab or C, C, taps, nosplit)
            n = _ceil(taps * C, tr) * _ceil(K, tc)
        else:
            n = _ceil(int(rec["numel"]), 1024)
        work[i] = (part, len(blk), splits, kslab, cslab, int(tiled), tr, tc)
        blk += [i] * n
    assert not set(slabs) - set(seg_names), "slab without a parameter segment"
    assert names is None or not set(slabs) - set(names), "slab outside the packed segments"
    return work, blk
