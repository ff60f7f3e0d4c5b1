"""An independent reference for the optimizer kernels (csrc/optim.hip), and builders
of the synthetic tables their tests launch them on.

Everything here is plain fp64 / index arithmetic; nothing calls the kernels or the
engine's host mirrors of them (LRSchedule.at).  Every tolerance the optimizer tests
use is one of the bounds derived below; none is tuned to what the kernels give.

Bounds
------
u = 2**-24 is the unit roundoff of fp32 (round to nearest: |fl(x) - x| <= u |x|).

sgd_reference, B = 8 u (|g*grad_scale| + |wd*w| + |momentum*mom| + |w| + |lr*acc|):
  the kernel evaluates  g' = g*grad_scale + wd*w,  acc = momentum*mom + g',
  w' = w - lr*acc  in fp32: three products and three sums, six roundings at most
  (fewer where the compiler contracts a product and a sum into an fma).  Each
  rounding is at most u relative to its result, and every intermediate result is
  bounded by the sum S of the magnitudes of the terms that enter it, all of which
  are among the five terms of B.  An error made early is carried through later
  operations with a factor of at most momentum <= 1 or lr <= 1 here, so the total is
  at most 6 u S (1 + O(u)); the factor 8 leaves room for the order of contraction.
  The same B is used for w' and acc (for acc it is generous: it also holds |w|).
  The coefficients are taken as given: callers pass the fp32 values the kernel
  receives (f32()).

lr_reference, 4 u max(|warm_from|, |warm_to|, max |val|):
  in the warm-up branch the device does a subtraction, a product, a quotient and a
  sum in fp32 (the conversions of t and warm_steps are exact below 2**24), each
  result no larger than the largest rate of the schedule.  Outside warm-up the
  device returns a stored fp32 constant: float32(value) exactly.

slab sums, splits * u * sum_s |part_s|:
  a sum of `splits` fp32 numbers in any order makes at most splits - 1 roundings,
  each of a partial sum no larger than sum_s |part_s|.

l2_half_sum, (ceil(n / 131072) + 24) u sum v**2:
  512 x 256 threads each add ceil(n / 131072) squares serially, then 6 wave-shuffle
  levels and a 4-way block sum (8 additions deep), then 2 serial additions, 6 levels
  and a 4-way sum over the 512 partials (10 deep), one rounding for the square
  itself: 19 roundings on any element's path past the serial part, all terms
  non-negative, so every partial sum is <= sum v**2.  24 leaves room.
"""
import dataclasses
import math

import numpy as np
import torch

from distributed_tensorflow_resnet_amd.train.layout import (OPTW_DTYPE, SEG_DTYPE, opt_tile,
                                                              sgd_tiles_work)

U32 = 2.0 ** -24


def f32(x: float) -> float:
    """x rounded to fp32, as a Python float: the value a kernel's float argument holds."""
    return float(np.float32(x))


def sgd_reference(w, g, mom, lr, momentum, wd, grad_scale, use_momentum=True):
    """One SGD-momentum step with L2 weight decay (tf.train.MomentumOptimizer,
    non-Nesterov) in fp64.  Returns (w', acc, B): the new weights, the new accumulator
    (`mom` itself without momentum: the kernel leaves it alone) and the per-element
    bound B on a correct fp32 evaluation's error (module docstring)."""
    w, g, mom = w.double(), g.double(), mom.double()
    gs = g * grad_scale
    dec = wd * w
    gp = gs + dec
    if use_momentum:
        mm = momentum * mom
        acc = mm + gp
    else:
        mm = torch.zeros_like(w)
        acc = gp
    step = lr * acc
    w_new = w - step
    B = 8 * U32 * (gs.abs() + dec.abs() + mm.abs() + w.abs() + step.abs())
    return w_new, (acc if use_momentum else mom), B


def lr_reference(sched, step: int) -> float:
    """The learning rate of training step `step` (the value of global_step when the
    step starts) in fp64.  The reference's session hook feeds each run the rate it
    computed after the previous run from that run's global_step: step 0 gets the
    hook's begin() value, step s > 0 gets f(s - 1) with f the piecewise schedule
    (linear warm-up, then the value of the first boundary not yet reached)."""
    if step < 1:
        return float(sched.init)
    seen = step - 1          # the global_step the hook saw after the previous run
    if seen < sched.warm_steps:
        frac = seen / float(sched.warm_steps)
        return float(sched.warm_from) + (float(sched.warm_to) - float(sched.warm_from)) * frac
    passed = sum(1 for b in sched.bounds if seen >= b)   # boundaries ascend
    return float(sched.values[passed])


def f32_schedule(sched):
    """The schedule with its rates rounded to fp32: what the kernels are handed.  The
    device's rate is compared with lr_reference of this one, so the bound only has to
    cover the device's own arithmetic."""
    return dataclasses.replace(sched, init=f32(sched.init), values=[f32(v) for v in sched.values],
                               warm_from=f32(sched.warm_from), warm_to=f32(sched.warm_to))


def lr_in_warmup(sched, step: int) -> bool:
    return step >= 1 and step - 1 < sched.warm_steps


def lr_bound(sched) -> float:
    return 4 * U32 * max([abs(sched.warm_from), abs(sched.warm_to)] + [abs(v) for v in sched.values])


def lr_steps(sched):
    """The steps at which a schedule can go wrong: the start, each side of the end of
    warm-up and of every boundary (the device looks at step - 1), far past the last
    boundary, and past 2**31."""
    s = {0, 1, 2, 2 ** 31 + 5}
    w = sched.warm_steps
    s |= {w - 1, w, w + 1, w + 2}
    for b in sched.bounds:
        s |= {b - 1, b, b + 1, b + 2}
    if sched.bounds:
        s.add(sched.bounds[-1] + 1000)
    return sorted(x for x in s if x >= 0)


def expected_wbf(seg_arr, master_f32, total: int):
    """The whole bf16 weight buffer (`total` elements) both pack paths must produce from
    the fp32 master (HWIO per segment: [tap][ci][co]): per segment with bf_hwio >= 0 the
    copy [tap*C + ci][kpad] (columns >= K zero), with bf_ohwi >= 0 the copy
    [co][tap][cpad] (ci >= C zero, rows co >= K zero); zero everywhere else."""
    out = torch.zeros(total, dtype=torch.bfloat16, device=master_f32.device)
    for r in seg_arr:
        ho, oh = int(r["bf_hwio"]), int(r["bf_ohwi"])
        if ho < 0 and oh < 0:
            continue
        taps, C, K = int(r["kh"]) * int(r["kw"]), int(r["C"]), int(r["K"])
        cpad, kpad = int(r["cpad"]), int(r["kpad"])
        off = int(r["offset"])
        w = master_f32[off:off + taps * C * K].to(torch.bfloat16).view(taps, C, K)
        if ho >= 0:
            out[ho:ho + taps * C * kpad].view(taps * C, kpad)[:, :K] = w.reshape(taps * C, K)
        if oh >= 0:
            out[oh:oh + K * taps * cpad].view(K, taps, cpad)[:, :, :C] = w.permute(2, 0, 1)
    return out


def ohwi_tile_table(seg_arr):
    """ohwi_pack's work map: tile0[s] = first 64 x 64 transpose tile of segment s (a prefix
    over ceil(taps*C/64) * ceil(K/64) tiles; none without an OHWI copy) and the total."""
    tiles = [(-(-(int(r["kh"]) * int(r["kw"]) * int(r["C"])) // 64) * -(-int(r["K"]) // 64)
              if r["bf_ohwi"] >= 0 else 0) for r in seg_arr]
    tile0 = np.concatenate([[0], np.cumsum(tiles)[:-1]]).astype(np.int64)
    return tile0, int(sum(tiles))


def build_seg_table(specs, gap: int = 8):
    """A ParamSeg table (numpy, SEG_DTYPE) from a list of
    (kind, kh, kw, C, K, cpad, kpad, has_ohwi, has_hwio), kind in "conv", "dense", "vec".
    Segments are contiguous in the master in list order, kh*kw*C*K elements each; a "vec"
    is recorded like the engine records BN vectors and biases (1x1, C = K = 1, no copies).
    The bf16 copies are laid out in list order, OHWI ([kpad][taps][cpad]) before HWIO
    ([taps*C][kpad]), each starting on a multiple of 8 elements (the kernels store the
    HWIO copy 4 elements at a time) after `gap` elements that belong to nobody, so a
    store past a copy's end shows up in expected_wbf.  Returns (seg_arr, names, n,
    bf_total, ohwi_tile0, ohwi_tiles): tile0 is ohwi_pack's first-tile prefix."""
    recs, names = [], []
    off, bf = 0, 0

    def take(n):
        nonlocal bf
        start = -(-(bf + gap) // 8) * 8
        bf = start + n
        return start

    for i, (kind, kh, kw, C, K, cpad, kpad, has_ohwi, has_hwio) in enumerate(specs):
        assert kind in ("conv", "dense", "vec"), kind
        rec = np.zeros(1, dtype=SEG_DTYPE)[0]
        numel = kh * kw * C * K
        rec["offset"], rec["numel"] = off, numel
        rec["bf_ohwi"] = rec["bf_hwio"] = -1
        if kind == "vec":
            assert not has_ohwi and not has_hwio
            rec["kh"] = rec["kw"] = rec["C"] = rec["K"] = rec["cpad"] = rec["kpad"] = 1
        else:
            assert cpad >= C and kpad >= K
            rec["kh"], rec["kw"], rec["C"], rec["K"] = kh, kw, C, K
            rec["cpad"], rec["kpad"] = cpad, kpad
            if has_ohwi:
                rec["bf_ohwi"] = take(kpad * kh * kw * cpad)
            if has_hwio:
                rec["bf_hwio"] = take(kh * kw * C * kpad)
        recs.append(rec)
        names.append(f"{kind}{i}")
        off += numel
    seg_arr = np.array(recs, dtype=SEG_DTYPE)
    tile0, tiles = ohwi_tile_table(seg_arr)
    return seg_arr, names, off, bf + gap, tile0, tiles


def build_opt_work(seg_arr, names, grad_ptr: int = 0, slabs=None, only=None, nosplit=(64, 64)):
    """The OptWork table (numpy, OPTW_DTYPE) and blk_seg (list) of one sgd_tiles launch
    over a build_seg_table table, by the engine's own sgd_tiles_work (so the tile shapes
    are the ones the engine would choose: opt_tile).  slabs: {name: (part_ptr, splits,
    kslab, cslab)} for the weights whose gradient is still in split-K slabs
    [splits][kslab][taps*cslab]; only: the segments that get workgroups."""
    d = {}
    by_name = dict(zip(names, seg_arr))
    for name, (part, splits, kslab, cslab) in (slabs or {}).items():
        r = by_name[name]
        d[name] = (part, grad_ptr + 4 * int(r["offset"]), splits, kslab, int(r["K"]),
                   int(r["kh"]) * int(r["kw"]), cslab, int(r["C"]))
    work, blk = sgd_tiles_work(seg_arr, names, d, grad_ptr, only, nosplit)
    assert work.dtype == OPTW_DTYPE
    for r, ow in zip(seg_arr, work):   # what the kernel's LDS tiles and registers hold
        if ow["tiled"]:
            assert 1 <= ow["tr"] <= 64 and 1 <= ow["tc"] <= 64 and ow["tr"] * ow["tc"] <= 4096
            assert (ow["tr"], ow["tc"]) == tuple(opt_tile(
                int(r["kh"] * r["kw"] * r["C"]), int(r["K"]), int(ow["splits"]),
                int(ow["cslab"]) or int(r["C"]), int(r["C"]), int(r["kh"] * r["kw"]), nosplit))
    return work, blk


def slab_sum_reference(part, splits, kslab, cslab, taps, C, K):
    """fp64 sum of split-K slabs [splits][kslab][taps*cslab] as the HWIO gradient
    [taps*C][K], and the sum of magnitudes the error bound is made of."""
    p = part.double().view(splits, kslab, taps, cslab)[:, :K, :, :C]
    s = p.sum(0).permute(1, 2, 0).reshape(taps * C, K)
    a = p.abs().sum(0).permute(1, 2, 0).reshape(taps * C, K)
    return s, a


def l2_bound(n: int, sumsq: float) -> float:
    return (math.ceil(n / 131072) + 24) * U32 * sumsq
