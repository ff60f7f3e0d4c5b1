"""Torch-tensor front end of the native gfx950 kernels.

Every function here validates shapes/dtypes/devices on the host, allocates the
outputs with torch's caching allocator and launches the HIP kernel on the
current stream.  There is deliberately NO fallback: on a GPU box a missing
extension or a bad argument raises.  CPU code paths use ``ops.reference``.

Layout conventions: activations NHWC bf16; conv weights bf16 in
``ohwi`` = [K][kh][kw][C] (forward B operand) and ``hwio`` = [kh][kw][C][K]
(TF layout; dgrad B operand); BN statistics and all optimizer state fp32.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import native
from .reference import BN_EPS

BF16 = torch.bfloat16


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: torch.Tensor | None) -> int:
    return 0 if t is None else t.data_ptr()


def _check(t: torch.Tensor, dtype, ndim: int | None = None, name: str = "tensor"):
    if not t.is_cuda:
        raise ValueError(f"{name} must be a GPU tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name} must be {ndim}-D, got {tuple(t.shape)}")


@dataclass(frozen=True)
class ConvGeom:
    """TF ``conv2d_fixed_padding`` geometry (resnet_model_official.py:80-91)."""
    N: int
    H: int
    W: int
    C: int
    K: int
    kh: int
    kw: int
    stride: int

    @property
    def pad(self) -> int:
        return (self.kh - 1) // 2

    @property
    def Ho(self) -> int:
        return (self.H - 1) // self.stride + 1

    @property
    def Wo(self) -> int:
        return (self.W - 1) // self.stride + 1

    def as_list(self):
        return [self.N, self.H, self.W, self.C, self.Ho, self.Wo, self.K, self.kh, self.kw,
                self.stride, self.pad]


def stat_tiles(M: int, ncol: int) -> tuple[int, int]:
    """(tiles, rows per tile) of the conv epilogue's BN-stat partials."""
    bm = native().conv_gemm_bm(M, ncol)
    return (M + bm - 1) // bm, bm


def conv2d_fwd(x, w_ohwi, stride: int, *, pre_scale=None, pre_shift=None, residual=None,
               stat_part=None, bias=None, out=None, out_f32: bool = False, accumulate=False,
               fin=None, pfin=None):
    """y = conv(relu(x*pre_scale+pre_shift) if pre else x, W) [+bias] [+residual].

    ``fin=[counters, gamma, beta, mmean, mvar, mean, rstd, scale, shift, gpart, group,
    groups_only]`` (tensors or ints) finalizes the output's BN statistics inside the
    kernel (last arriver); ``pfin=[part, cnt, rows_per, M, gamma, beta, mean, rstd,
    scale, shift, mmean, mvar]`` finalizes the PRE BatchNorm in the prologue (the
    kernel is that BN's first consumer; pre_scale/pre_shift are then outputs)."""
    _check(x, BF16, 4, "x")
    _check(w_ohwi, BF16, 4, "w_ohwi")
    N, H, W, C = x.shape
    K, kh, kw, C2 = w_ohwi.shape
    if C2 != C:
        raise ValueError(f"channel mismatch x C={C} vs w C={C2}")
    g = ConvGeom(N, H, W, C, K, kh, kw, stride)
    if out is None:
        out = torch.empty((N, g.Ho, g.Wo, K), device=x.device,
                          dtype=torch.float32 if out_f32 else BF16)
    if residual is not None:
        _check(residual, BF16, 4, "residual")
        if tuple(residual.shape) != tuple(out.shape):
            raise ValueError("residual shape mismatch")
    if pre_scale is not None:
        _check(pre_scale, torch.float32, 1, "pre_scale")
        _check(pre_shift, torch.float32, 1, "pre_shift")
    if stat_part is not None:
        tiles, _ = stat_tiles(N * g.Ho * g.Wo, K)
        if stat_part.numel() < tiles * 2 * K:
            raise ValueError("stat_part too small")
    native().conv_gemm(0, x.data_ptr(), w_ohwi.data_ptr(),
                       0 if out_f32 else out.data_ptr(), out.data_ptr() if out_f32 else 0,
                       _ptr(residual), _ptr(pre_scale), _ptr(pre_shift), _ptr(bias),
                       0 if bias is None else bias.numel(), _ptr(stat_part), int(accumulate),
                       g.as_list(), [], _ptrs(fin), [], _ptrs(pfin), [], 0.997, BN_EPS, 1, _stream())
    return out


def _ptrs(lst):
    return [] if lst is None else [t.data_ptr() if torch.is_tensor(t) else int(t) for t in lst]


def conv2d_dgrad(dy, w_hwio, x_shape, stride: int, *, out=None, accumulate=False, bnb=None,
                 bfin=None, abwd=None):
    """dx = conv2d_transpose(dy, W) with TF fixed padding; w_hwio [kh][kw][C][K].

    ``bnb=(x, mean, rstd, scale, shift, part)`` additionally emits the
    BN+ReLU backward partials of dx (per tile: sum g, sum g*xhat, g = dx*[relu]).
    ``abwd=[x, add, mean, rstd, scale, shift, gamma, part, cnt, a_out, dgamma, dbeta,
    coef]``: ``dy`` is the gradient BEFORE its BatchNorm+ReLU backward, which the kernel
    applies while staging (writing the result to a_out) -- direct 3x3 kernel only."""
    _check(dy, BF16, 4, "dy")
    _check(w_hwio, BF16, 4, "w_hwio")
    N, H, W, C = x_shape
    kh, kw, C2, K = w_hwio.shape
    g = ConvGeom(N, H, W, C, K, kh, kw, stride)
    if tuple(dy.shape) != (N, g.Ho, g.Wo, K) or C2 != C:
        raise ValueError(f"dgrad shape mismatch dy={tuple(dy.shape)} geom={g}")
    if out is None:
        out = torch.empty((N, H, W, C), device=dy.device, dtype=BF16)
    bl = [] if bnb is None else [t.data_ptr() for t in bnb]
    native().conv_gemm(1, dy.data_ptr(), w_hwio.data_ptr(), out.data_ptr(), 0, 0, 0, 0, 0, 0, 0,
                       int(accumulate), g.as_list(), bl, [], _ptrs(bfin), [], _ptrs(abwd), 0.997, BN_EPS, 1,
                       _stream())
    return out


def conv2d_wgrad(dy, x, kh: int, kw: int, stride: int, *, pre_scale=None, pre_shift=None,
                 grad_hwio=None, scale: float = 1.0, accumulate=False, k_valid=None):
    """dW (fp32, TF HWIO) = sum_pixels dy (x) im2col(x); deterministic split-K."""
    _check(dy, BF16, 4, "dy")
    _check(x, BF16, 4, "x")
    N, H, W, C = x.shape
    K = dy.shape[3]
    g = ConvGeom(N, H, W, C, K, kh, kw, stride)
    if tuple(dy.shape) != (N, g.Ho, g.Wo, K):
        raise ValueError("wgrad shape mismatch")
    kv = K if k_valid is None else k_valid
    nat = native()
    splits, pps = nat.wgrad_pick_splits(g.as_list())
    part = torch.empty(splits * K * kh * kw * C, device=dy.device, dtype=torch.float32)
    if grad_hwio is None:
        grad_hwio = torch.empty((kh, kw, C, kv), device=dy.device, dtype=torch.float32)
    nat.conv_wgrad(dy.data_ptr(), x.data_ptr(), _ptr(pre_scale), _ptr(pre_shift),
                   part.data_ptr(), g.as_list(), splits, pps, _stream())
    nat.wgrad_reduce(part.data_ptr(), grad_hwio.data_ptr(), splits, K, kv, kh * kw, C, C,
                     float(scale), int(accumulate), _stream())
    return grad_hwio


def bn_finalize(stat_part, tiles, tile_rows, M, gamma, beta, moving_mean, moving_var,
                momentum=0.997, eps=BN_EPS, update_moving=True):
    C = gamma.numel()
    dev = gamma.device
    mean, rstd, scale, shift = (torch.empty(C, device=dev) for _ in range(4))
    native().bn_finalize(stat_part.data_ptr(), tiles, tile_rows, M, C, gamma.data_ptr(),
                         beta.data_ptr(), moving_mean.data_ptr(), moving_var.data_ptr(),
                         momentum, eps, int(update_moving), mean.data_ptr(), rstd.data_ptr(),
                         scale.data_ptr(), shift.data_ptr(), _stream())
    return mean, rstd, scale, shift


def bn_stats(x2d):
    """Welford partials (tiles x 2 x C) of a [M][C] bf16 tensor."""
    _check(x2d, BF16, 2, "x")
    M, C = x2d.shape
    nat = native()
    tiles = nat.bn_bwd_tiles(M, C)
    part = torch.empty(tiles * 2 * C, device=x2d.device)
    nat.bn_stats(x2d.data_ptr(), M, C, part.data_ptr(), _stream())
    return part, tiles, nat.bn_stats_tile_rows()


def bn_relu_backward(dy2d, x2d, mean, rstd, scale, shift, gamma, add=None):
    """Returns (dx, dgamma, dbeta) of y = relu(bn(x)) given dL/dy (training stats)."""
    _check(dy2d, BF16, 2, "dy")
    _check(x2d, BF16, 2, "x")
    M, C = x2d.shape
    nat = native()
    tiles = nat.bn_bwd_tiles(M, C)
    dev = x2d.device
    part = torch.empty(tiles * 2 * C, device=dev)
    dgamma = torch.empty(C, device=dev)
    dbeta = torch.empty(C, device=dev)
    coef = torch.empty(3 * C, device=dev)
    dx = torch.empty_like(x2d)
    st = _stream()
    nat.bn_bwd_reduce(dy2d.data_ptr(), x2d.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                      scale.data_ptr(), shift.data_ptr(), M, C, part.data_ptr(), st)
    nat.bn_bwd_finalize(part.data_ptr(), tiles, M, C, gamma.data_ptr(), rstd.data_ptr(),
                        dgamma.data_ptr(), dbeta.data_ptr(), coef.data_ptr(), st)
    nat.bn_bwd_apply(dy2d.data_ptr(), x2d.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                     scale.data_ptr(), shift.data_ptr(), coef.data_ptr(), _ptr(add),
                     dx.data_ptr(), M, C, st)
    return dx, dgamma, dbeta


def bn_relu_apply(x2d, scale, shift):
    _check(x2d, BF16, 2, "x")
    M, C = x2d.shape
    y = torch.empty_like(x2d)
    native().bn_relu_apply(x2d.data_ptr(), scale.data_ptr(), shift.data_ptr(), y.data_ptr(), M,
                           C, _stream())
    return y


def bnrelu_avgpool(x, scale, shift):
    _check(x, BF16, 4, "x")
    N, H, W, C = x.shape
    pooled = torch.empty((N, C), device=x.device, dtype=BF16)
    native().bnrelu_avgpool(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), pooled.data_ptr(),
                            N, H * W, C, _stream())
    return pooled


def avgpool_bwd(dpooled, H, W):
    _check(dpooled, BF16, 2, "dpooled")
    N, C = dpooled.shape
    dx = torch.empty((N, H, W, C), device=dpooled.device, dtype=BF16)
    native().avgpool_bwd(dpooled.data_ptr(), dx.data_ptr(), N, H * W, C, _stream())
    return dx


def softmax_xent(logits, labels, classes, grad_scale, want_probs=False, label_smoothing=0.0,
                 topk=0):
    """Returns (loss_sum, correct, dlogits bf16 [N][ld], dbias fp32 [classes], probs) and,
    when topk > 0, a sixth element: the number of rows whose label is in the top `topk`
    logits (tf.nn.in_top_k).  label_smoothing in [0, 1) smooths the targets to
    (1 - eps) * onehot + eps / classes."""
    _check(logits, torch.float32, 2, "logits")
    N, ld = logits.shape
    dev = logits.device
    loss = torch.zeros(1, device=dev)
    corr = torch.zeros(1, device=dev)
    ink = torch.zeros(1, device=dev) if topk > 0 else None
    dl = torch.empty((N, ld), device=dev, dtype=BF16)
    db = torch.empty(classes, device=dev)
    probs = torch.zeros((N, ld), device=dev) if want_probs else None
    labels = labels.to(device=dev, dtype=torch.int32).contiguous()
    ws = torch.empty(native().softmax_xent_ws_floats(N, ld), device=dev)
    native().softmax_xent(logits.data_ptr(), ld, labels.data_ptr(), N, classes, loss.data_ptr(),
                          corr.data_ptr(), dl.data_ptr(), db.data_ptr(), float(grad_scale),
                          _ptr(probs), ws.data_ptr(), float(label_smoothing), int(topk),
                          _ptr(ink), _stream())
    return (loss, corr, dl, db, probs, ink) if topk > 0 else (loss, corr, dl, db, probs)


def maxpool_fwd(x, k=3, stride=2):
    """TF max_pooling2d(pool k, stride, padding='SAME') on NHWC.
    Returns (y, argmax) where argmax holds the window position of the first max."""
    _check(x, BF16, 4, "x")
    N, H, W, C = x.shape
    Ho, Wo = -(-H // stride), -(-W // stride)
    pad = max((Ho - 1) * stride + k - H, 0) // 2
    y = torch.empty((N, Ho, Wo, C), device=x.device, dtype=BF16)
    am = torch.empty((N, Ho, Wo, C), device=x.device, dtype=torch.uint8)
    native().maxpool_fwd(x.data_ptr(), y.data_ptr(), am.data_ptr(),
                         [N, H, W, C, Ho, Wo, C, k, k, stride, pad], k, _stream())
    return y, am


def maxpool_bwd(argmax, dy, x_shape, k=3, stride=2):
    N, H, W, C = x_shape
    Ho, Wo = dy.shape[1], dy.shape[2]
    pad = max((Ho - 1) * stride + k - H, 0) // 2
    dx = torch.empty(x_shape, device=dy.device, dtype=BF16)
    native().maxpool_bwd(argmax.data_ptr(), dy.data_ptr(), dx.data_ptr(),
                         [N, H, W, C, Ho, Wo, C, k, k, stride, pad], k, _stream())
    return dx


def cifar_augment(img_u8, cpad=8, pad=4, seed=0, gstep=None, train=True, log_crops=False):
    """Raw CIFAR records [N,3,H,W] uint8 -> standardized bf16 NHWC (Cpad channels)."""
    if img_u8.dtype != torch.uint8 or not img_u8.is_cuda:
        raise ValueError("img must be a uint8 GPU tensor [N,3,H,W]")
    N, _, H, W = img_u8.shape
    out = torch.empty((N, H, W, cpad), device=img_u8.device, dtype=BF16)
    log = torch.zeros((N, 3), device=img_u8.device, dtype=torch.int32) if log_crops else None
    native().cifar_augment(img_u8.data_ptr(), out.data_ptr(), N, H, W, cpad, pad, seed,
                           _ptr(gstep), int(train), _ptr(log), 0, 0, _stream())
    return (out, log) if log_crops else out


def cifar_augment_resident(records_u8, labels_all, pos, batch, cpad=8, pad=4, seed=0, key_seed=0,
                           rank=0, world=1, shuffle=True, train=True, zero=None, log_crops=False,
                           log_index=False):
    """cifar_augment on a device-resident split: batch position n reads record
    data.cifar.resident_index(key_seed, pos, n, batch, records, rank, world, shuffle).

    records_u8 [M,3,32,32] uint8, labels_all [M] int32, pos [1] int64 (the step), all on
    the GPU; ``zero``: an optional buffer cleared in the same launch.  Returns (out bf16
    [batch,32,32,cpad], labels int32 [batch]) followed by the crop log [batch,3] and the
    index log [batch] (int32) when asked for."""
    if records_u8.dtype != torch.uint8 or not records_u8.is_cuda or records_u8.dim() != 4 \
            or not records_u8.is_contiguous():
        raise ValueError("records must be a contiguous uint8 GPU tensor [M,3,H,W]")
    M, _, H, W = records_u8.shape
    if labels_all.dtype != torch.int32 or not labels_all.is_cuda or labels_all.numel() != M \
            or not labels_all.is_contiguous():
        raise ValueError("labels must be a contiguous int32 GPU tensor [M]")
    if pos.dtype != torch.int64 or not pos.is_cuda or pos.numel() != 1:
        raise ValueError("pos must be an int64 GPU tensor [1]")
    dev = records_u8.device
    out = torch.empty((batch, H, W, cpad), device=dev, dtype=BF16)
    labels = torch.empty(batch, device=dev, dtype=torch.int32)
    crops = torch.zeros((batch, 3), device=dev, dtype=torch.int32) if log_crops else None
    idx = torch.zeros(batch, device=dev, dtype=torch.int32) if log_index else None
    zbytes = zero.numel() * zero.element_size() if zero is not None else 0
    native().cifar_augment_resident(records_u8.data_ptr(), labels_all.data_ptr(), out.data_ptr(),
                                    labels.data_ptr(), pos.data_ptr(), batch, H, W, cpad, M, rank,
                                    world, int(bool(shuffle)), key_seed & (2 ** 64 - 1), pad, seed,
                                    int(train), _ptr(crops), _ptr(idx), _ptr(zero), zbytes,
                                    _stream())
    res = (out, labels)
    if log_crops:
        res += (crops,)
    if log_index:
        res += (idx,)
    return res


def muon_orthogonalize(grad, mom, shapes, offsets=None, *, momentum=0.95, nesterov=True, steps=5,
                       grad_scale=1.0, out=None):
    """csrc/muon.hip's first launch on flat fp32 buffers: for every (R, K) of ``shapes`` (the
    row-major R x K matrix at the matching element of ``offsets``, default back to back) the
    momentum ``mom`` is updated in place and the Newton-Schulz-orthogonalised direction is
    written into ``out`` (default: zeros like grad) at the same offset.  One workgroup per
    matrix; a short side above 64 or a long side above 576 raises.  Returns ``out``."""
    import numpy as np

    from ..train.layout import MUON_DTYPE

    _check(grad, torch.float32, 1, "grad")
    _check(mom, torch.float32, 1, "mom")
    out = torch.zeros_like(grad) if out is None else out
    _check(out, torch.float32, 1, "out")
    if offsets is None:
        offsets = [0]
        for R, K in shapes[:-1]:
            offsets.append(offsets[-1] + R * K)
    if len(offsets) != len(shapes) or mom.numel() != grad.numel() or out.numel() != grad.numel():
        raise ValueError("one offset per shape, and grad, mom and out of one length")
    for o, (R, K) in zip(offsets, shapes):
        if o < 0 or o + R * K > grad.numel():
            raise ValueError(f"matrix {R} x {K} at {o} is outside the {grad.numel()} elements")
    tab = np.array([(o, i, R, K, int(K <= R)) for i, (o, (R, K)) in enumerate(zip(offsets, shapes))],
                   dtype=MUON_DTYPE)
    dtab = torch.from_numpy(tab.view(np.uint8).copy()).to(grad.device)
    native().muon_orthogonalize(grad.data_ptr(), mom.data_ptr(), out.data_ptr(), dtab.data_ptr(),
                                [R for R, _ in shapes], [K for _, K in shapes], float(momentum),
                                int(bool(nesterov)), int(steps), float(grad_scale), _stream())
    return out


def muon_tiled_buffers(tt, device):
    """Device copies of train/layout.py muon_tiled_tables' dict, the chunk partials and the
    bf16 scratch (X, A and B of every tensor) of the tiled muon launches."""
    import numpy as np

    from ..train.layout import MUON_TILED_DTYPE, MUON_WORK_DTYPE

    nat = native()
    assert MUON_TILED_DTYPE.itemsize == nat.muon_tiled_tensor_bytes()
    assert MUON_WORK_DTYPE.itemsize == nat.muon_work_bytes()
    raw = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(device)   # noqa: E731
    buf = {k: raw(tt[k]) for k in ("tab", "stage", "syrk_a", "syrk_b", "apply")}
    buf["n"] = {k: len(tt[k]) for k in ("stage", "syrk_a", "syrk_b", "apply", "blk")}
    buf["blk"] = torch.from_numpy(tt["blk"]).to(device)
    buf["part"] = torch.zeros(len(tt["blk"]), dtype=torch.float64, device=device)
    buf["scratch"] = torch.zeros(tt["scratch"], dtype=BF16, device=device)
    buf["max_sp"] = tt["max_sp"]
    return buf


def muon_tiled_sequence(api, buf, grad, mom, out, momentum, nesterov, steps, grad_scale, tail=()):
    """The 3 + 3 * steps tiled muon launches (csrc/muon_tiled.hip) through `api`: the native
    module (tail = the stream) or a plan being recorded (tail empty).  grad, mom and out are
    pointers.  Returns what the calls returned (a plan's op indices)."""
    n, p = buf["n"], {k: v.data_ptr() for k, v in buf.items() if torch.is_tensor(v)}
    mu, nes, gs = float(momentum), int(bool(nesterov)), float(grad_scale)
    ops = [api.muon_tiled_moments(grad, mom, p["tab"], p["blk"], n["blk"], p["part"], mu, nes, gs,
                                  *tail),
           api.muon_tiled_stage(grad, mom, p["tab"], p["stage"], n["stage"], p["part"],
                                p["scratch"], mu, nes, gs, *tail)]
    for _ in range(int(steps)):
        ops += [api.muon_tiled_syrk(p["scratch"], p["tab"], p["syrk_a"], n["syrk_a"], 0, *tail),
                api.muon_tiled_syrk(p["scratch"], p["tab"], p["syrk_b"], n["syrk_b"], 1, *tail),
                api.muon_tiled_apply(p["scratch"], p["tab"], p["apply"], n["apply"],
                                     buf["max_sp"], *tail)]
    ops.append(api.muon_tiled_unstage(p["scratch"], out, p["tab"], p["stage"], n["stage"], *tail))
    return ops


def muon_orthogonalize_tiled(grad, mom, shapes, offsets=None, *, momentum=0.95, nesterov=True,
                             steps=5, grad_scale=1.0, out=None):
    """muon_orthogonalize's contract for matrices of any covered size: a shape inside
    muon_covers goes to muon_orthogonalize's one workgroup, any other with a short side <= 1024
    and a long side <= 8192 to the tiled launches of csrc/muon_tiled.hip (grad and mom must
    then be 16-byte aligned); anything else raises.  Returns ``out``."""
    from ..train.layout import muon_covers, muon_tiled_covers, muon_tiled_tables

    _check(grad, torch.float32, 1, "grad")
    _check(mom, torch.float32, 1, "mom")
    out = torch.zeros_like(grad) if out is None else out
    _check(out, torch.float32, 1, "out")
    if offsets is None:
        offsets = [0]
        for R, K in shapes[:-1]:
            offsets.append(offsets[-1] + R * K)
    if len(offsets) != len(shapes) or mom.numel() != grad.numel() or out.numel() != grad.numel():
        raise ValueError("one offset per shape, and grad, mom and out of one length")
    if not 1 <= int(steps) <= 8 or not 0.0 <= float(momentum) < 1.0:
        raise ValueError("steps in [1, 8] and momentum in [0, 1)")
    small, big = [], []
    for i, (o, (R, K)) in enumerate(zip(offsets, shapes)):
        if R < 1 or K < 1 or o < 0 or o + R * K > grad.numel():
            raise ValueError(f"matrix {R} x {K} at {o} is outside the {grad.numel()} elements")
        if muon_covers(R, K):
            small.append((o, (R, K)))
        elif muon_tiled_covers(R, K):
            big.append((int(o), i, int(R), int(K)))
        else:
            raise ValueError(f"matrix {R} x {K}: the tiled launches take a short side <= 1024 "
                             f"and a long side <= 8192")
    if small:
        muon_orthogonalize(grad, mom, [s for _, s in small], [o for o, _ in small],
                           momentum=momentum, nesterov=nesterov, steps=steps,
                           grad_scale=grad_scale, out=out)
    if big:
        buf = muon_tiled_buffers(muon_tiled_tables(big), grad.device)
        muon_tiled_sequence(native(), buf, grad.data_ptr(), mom.data_ptr(), out.data_ptr(),
                            momentum, nesterov, steps, grad_scale, tail=(_stream(),))
    return out


def _shampoo_table(recs, device):
    """Device copy of train/layout.py shampoo_block_table(recs)'s block table, and the host one."""
    import numpy as np

    from ..train.layout import SHAMPOO_DTYPE, SHAMPOO_TENSOR_DTYPE, shampoo_block_table

    nat = native()
    assert SHAMPOO_DTYPE.itemsize == nat.shampoo_block_bytes()
    assert SHAMPOO_TENSOR_DTYPE.itemsize == nat.shampoo_tensor_bytes()
    blocks, _ = shampoo_block_table(recs)
    return torch.from_numpy(blocks.view(np.uint8).copy()).to(device), blocks


def _shampoo_state(x, nblocks, name):
    _check(x, torch.float32, 3, name)
    if tuple(x.shape) != (nblocks, 64, 64):
        raise ValueError(f"{name} must be [{nblocks}, 64, 64], got {tuple(x.shape)}")


def shampoo_roots(stat, root, sizes, *, epsilon=1e-6, step=1, every=1, fail=None):
    """csrc/shampoo.hip's roots launch on single sides: slot i of ``stat`` ([n, 64, 64] fp32,
    zero outside its live sizes[i] x sizes[i] part) is a symmetric positive semi-definite
    statistic A, and the live part of slot i of ``root`` becomes (A + epsilon ||A||_F I)^(-1/4)
    by the coupled Newton iteration -- when ``step`` (the 1-based step count, put into a step
    word on the device) is a multiple of ``every``; otherwise the launch changes nothing.  A
    slot whose iteration fails keeps its root and adds 1 to ``fail`` (int32 [1], optional).
    Returns ``root``."""
    n = len(sizes)
    _shampoo_state(stat, n, "stat")
    _shampoo_state(root, n, "root")
    if any(not 1 <= int(s) <= 64 for s in sizes):
        raise ValueError("every live size must be in [1, 64]")
    # (a block table of n x n matrices back to back: only r and the slot are read)
    recs, off = [], 0
    for i, s in enumerate(sizes):
        recs.append((off, i, int(s), int(s)))
        off += int(s) * int(s)
    dtab, _ = _shampoo_table(recs, stat.device)
    gstep = torch.tensor([int(step) - 1], dtype=torch.int64, device=stat.device)
    native().shampoo_roots(dtab.data_ptr(), n, 1, stat.data_ptr(), 0, root.data_ptr(), 0,
                           gstep.data_ptr(), 0, int(every), float(epsilon), _ptr(fail), _stream())
    return root


def shampoo_stats_precondition(grad, shapes, offsets, L, Rt, PL, PR, *, beta2=1.0, grad_scale=1.0,
                               out=None):
    """csrc/shampoo.hip's stats and precondition launches on bare tensors: every (R, K) of
    ``shapes`` is the row-major matrix at the matching element of ``offsets`` in the flat fp32
    ``grad`` (only read), cut into 64 x 64 blocks in train/layout.py shampoo_block_table's
    order; L, Rt, PL, PR are [blocks, 64, 64].  L and Rt are updated in place
    (beta2 L + c G G^T, beta2 Rt + c G^T G) and U = PL G PR is written into ``out`` (default:
    zeros like grad) at the blocks' elements.  Returns (out, part, blocks): part is the fp64
    [blocks, 2] table of each block's sums of g'^2 and U^2, blocks the host table."""
    _check(grad, torch.float32, 1, "grad")
    out = torch.zeros_like(grad) if out is None else out
    _check(out, torch.float32, 1, "out")
    if len(offsets) != len(shapes) or out.numel() != grad.numel():
        raise ValueError("one offset per shape, and grad and out of one length")
    recs = []
    for i, (o, (R, K)) in enumerate(zip(offsets, shapes)):
        if R < 1 or K < 1 or o < 0 or o + R * K > grad.numel():
            raise ValueError(f"matrix {R} x {K} at {o} is outside the {grad.numel()} elements")
        recs.append((int(o), i, int(R), int(K)))
    dtab, blocks = _shampoo_table(recs, grad.device)
    nb = len(blocks)
    for x, name in ((L, "L"), (Rt, "Rt"), (PL, "PL"), (PR, "PR")):
        _shampoo_state(x, nb, name)
    part = torch.zeros(nb, 2, dtype=torch.float64, device=grad.device)
    gstep = torch.zeros(1, dtype=torch.int64, device=grad.device)
    nat = native()
    nat.shampoo_stats(grad.data_ptr(), dtab.data_ptr(), nb, L.data_ptr(), Rt.data_ptr(),
                      float(beta2), float(grad_scale), gstep.data_ptr(), 0, 1, 0, _stream())
    nat.shampoo_precondition(grad.data_ptr(), dtab.data_ptr(), nb, PL.data_ptr(), PR.data_ptr(),
                             out.data_ptr(), part.data_ptr(), float(grad_scale), _stream())
    return out, part, blocks


def soap_refresh(stat, basis, sizes, *, step=1, every=1, fail=None):
    """csrc/soap.hip's refresh launch on single sides: slot i of ``stat`` ([n, 64, 64] fp32, zero
    outside its live sizes[i] x sizes[i] part) is a symmetric statistic S and slot i of ``basis``
    an orthonormal Q; the live part of the basis slot becomes the orthonormal factor of the
    Householder QR of S Q, columns signed so that diag(R) >= 0 -- when ``step`` (the 1-based step
    count, put into a step word on the device) is a multiple of ``every``; otherwise the launch
    changes nothing.  A slot that meets a non-finite value keeps its basis and adds 1 to ``fail``
    (int32 [1], optional).  Returns ``basis``."""
    n = len(sizes)
    _shampoo_state(stat, n, "stat")
    _shampoo_state(basis, n, "basis")
    if any(not 1 <= int(s) <= 64 for s in sizes):
        raise ValueError("every live size must be in [1, 64]")
    recs, off = [], 0   # (only r and the slot are read, as in shampoo_roots)
    for i, s in enumerate(sizes):
        recs.append((off, i, int(s), int(s)))
        off += int(s) * int(s)
    dtab, _ = _shampoo_table(recs, stat.device)
    gstep = torch.tensor([int(step) - 1], dtype=torch.int64, device=stat.device)
    native().soap_refresh(dtab.data_ptr(), n, 1, stat.data_ptr(), 0, basis.data_ptr(), 0,
                          gstep.data_ptr(), 0, int(every), _ptr(fail), _stream())
    return basis


def soap_rotate_adam(grad, mom, v, shapes, offsets, QL, QR, *, beta1=0.9, beta2=0.999,
                     epsilon=1e-8, grad_scale=1.0, out=None):
    """csrc/soap.hip's rotate launch on bare tensors: every (R, K) of ``shapes`` is the row-major
    matrix at the matching element of ``offsets`` in the flat fp32 ``grad`` (only read), ``mom``
    and ``v`` (both updated in place), cut into 64 x 64 blocks in train/layout.py
    shampoo_block_table's order; QL, QR are [blocks, 64, 64] bases.  Per block
    M' = beta1 M + (1 - beta1) G, V' = beta2 V + (1 - beta2) (QL^T G QR)^2 and
    N = QL ((QL^T M' QR) / (sqrt(V') + epsilon)) QR^T, written into ``out`` (default: zeros like
    grad) at the blocks' elements; nothing else is touched.  Returns (out, blocks): blocks is the
    host table."""
    for x, name in ((grad, "grad"), (mom, "mom"), (v, "v")):
        _check(x, torch.float32, 1, name)
    out = torch.zeros_like(grad) if out is None else out
    _check(out, torch.float32, 1, "out")
    if len(offsets) != len(shapes) or not out.numel() == grad.numel() == mom.numel() == v.numel():
        raise ValueError("one offset per shape, and grad, mom, v and out of one length")
    recs = []
    for i, (o, (R, K)) in enumerate(zip(offsets, shapes)):
        if R < 1 or K < 1 or o < 0 or o + R * K > grad.numel():
            raise ValueError(f"matrix {R} x {K} at {o} is outside the {grad.numel()} elements")
        recs.append((int(o), i, int(R), int(K)))
    dtab, blocks = _shampoo_table(recs, grad.device)
    for x, name in ((QL, "QL"), (QR, "QR")):
        _shampoo_state(x, len(blocks), name)
    native().soap_rotate_adam(grad.data_ptr(), dtab.data_ptr(), len(blocks), QL.data_ptr(),
                              QR.data_ptr(), mom.data_ptr(), v.data_ptr(), out.data_ptr(),
                              float(beta1), float(beta2), float(epsilon), float(grad_scale),
                              _stream())
    return out, blocks
