"""Bit-exact, per-element checks of every conv kernel path.

Operands are the exactly representable integers / dyadic rationals of tests/exact_conv.py,
so whatever the summation order each path owes one bit pattern: the exact fp64 oracle
rounded once to bf16 (round-to-nearest-even), or the exact number itself for fp32 outputs.
Every test asserts the dispatcher's own predicates for the path it names (nothing is skipped
when a predicate is false) and prints the path; a mismatch reports how many elements differ
and the first few (n, h, w, c) with got / want.
"""
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import exact_conv as ec
from distributed_tensorflow_resnet_amd.ops import functional as fn
from distributed_tensorflow_resnet_amd.ops.reference import BN_EPS

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@contextmanager
def tuned(**keys):
    """Set native tuning keys for a block; every key goes back to what it was."""
    nat = fn.native()
    before = {t[0]: t[3] for t in nat.tune_table()}
    try:
        for k, v in keys.items():
            nat.tune_set(k, v)
        yield
    finally:
        for k in keys:
            nat.tune_set(k, before[k])


def check(got, want, what):
    """got (GPU tensor) == want (exact fp64 CPU tensor, cast to got's dtype) elementwise."""
    torch.cuda.synchronize()
    got = got.detach().cpu()
    want = want.to(got.dtype).reshape(got.shape)
    bad = got.float() != want.float()          # NaN counts as different
    n = int(bad.sum())
    if n:
        idx = bad.nonzero()[:6].tolist()
        first = ", ".join(f"{tuple(i)}: got {float(got[tuple(i)])} want {float(want[tuple(i)])}"
                          for i in idx)
        pytest.fail(f"{what}: {n} of {got.numel()} elements differ; first {first}")


def to_gpu(case, o, gpu):
    d = {"a": o["a"].to(BF).to(gpu), "w_hwio": o["w"].to(BF).to(gpu).contiguous()}
    d["w_ohwi"] = d["w_hwio"].permute(3, 0, 1, 2).contiguous()
    for k in ("sc", "sh", "bias"):
        if k in o:
            d[k] = o[k].float().to(gpu)
    if "res" in o:
        d["res"] = o["res"].to(BF).to(gpu)
    if "base" in o:
        d["base"] = o["base"].to(torch.float32 if case.f32 else BF).to(gpu)
    return d


def launch(case, d):
    dt = torch.float32 if case.f32 else BF
    out = d["base"].clone() if case.acc else \
        torch.full(case.out_shape, float("nan"), device=d["a"].device, dtype=dt)
    if case.mode == "fwd":
        fn.conv2d_fwd(d["a"], d["w_ohwi"], case.s, pre_scale=d.get("sc"), pre_shift=d.get("sh"),
                      residual=d.get("res"), bias=d.get("bias"), out=out, out_f32=case.f32,
                      accumulate=case.acc)
    else:
        fn.conv2d_dgrad(d["a"], d["w_hwio"], (case.N, case.H, case.H, case.C), case.s, out=out,
                        accumulate=case.acc)
    return out


def rows(case, parity=True):
    """Rows of the implicit GEMM the dispatcher picks its tile for."""
    if case.mode == "fwd":
        return case.N * case.Ho * case.Ho
    if case.s == 2 and parity:
        return case.N * ((case.H + 1) // 2) ** 2
    return case.N * case.H * case.H


def tile(case, parity=True):
    nat = fn.native()
    M = rows(case, parity)
    return nat.conv_gemm_bm(M, case.ncol), nat.conv_gemm_bn(M, case.ncol)


def mode_id(case):
    return 0 if case.mode == "fwd" else 1


def generic_only(case):
    """Neither the direct nor the ring kernel takes the conv under the current tuning."""
    nat = fn.native()
    assert not nat.conv_direct_covers(mode_id(case), case.geom())
    assert not nat.conv_ring_covers(mode_id(case), case.geom())


# ---------------------------------------------------------------------------
# generic implicit GEMM: every tile, both loops
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("want_tile,case", [(t, c) for t, cs in ec.TILE_CASES.items() for c in cs],
                         ids=lambda v: v.name if isinstance(v, ec.Case) else f"{v[0]}x{v[1]}")
def test_generic_tiles(gpu, want_tile, case):
    """Forward and dgrad on each tile launch_mode can pick, full and partial, with the
    pipelined loop on and off, and the single-buffer loop (Kdim <= 64) on and off."""
    o = ec.operands(case)
    d = to_gpu(case, o, gpu)
    one_tile = (case.k * case.k * case.cin + 63) // 64 <= 1
    for pipe in (0, 1):
        for nbuf1 in ((1, 0) if one_tile else (1,)):
            with tuned(direct_conv=0, ring=0, conv_pipe=pipe, nbuf1_kt=nbuf1):
                assert tile(case) == want_tile
                generic_only(case)
                out = launch(case, d)
            check(out, o["want"], f"{case.name} tile {want_tile} pipe={pipe} nbuf1_kt={nbuf1}")
    print(f"{case.name}: generic implicit GEMM, tile {want_tile}, rows {rows(case)}, "
          f"{'one' if one_tile else 'several'} K tile(s)")


@pytest.mark.parametrize("case", ec.OPTION_CASES + ec.STEM_CASES, ids=lambda c: c.name)
def test_epilogue_prologue_options_and_stems(gpu, case):
    """Residual, accumulate onto a non-zero base, fp32 output, bias on columns < nbias, the
    BN+ReLU prologue under 3x3 padding (a padding tap must stay 0, not relu(shift)); and the
    stems, whose padded channels meet non-zero weights."""
    o = ec.operands(case)
    d = to_gpu(case, o, gpu)
    if case.pre:   # the padding must be told from relu(shift): some shift is positive
        assert float(o["sh"].max()) > 0
    for pipe in (0, 1):
        with tuned(direct_conv=0, ring=0, conv_pipe=pipe):
            generic_only(case)
            t = tile(case)
            out = launch(case, d)
        check(out, o["want"], f"{case.name} tile {t} pipe={pipe}")
    big = rows(case) >= 4096 and case.ncol % 128 == 0
    assert t == ((128, 128) if big else (64, min(64, max(16, case.ncol))))
    print(f"{case.name}: generic implicit GEMM, tile {t}")


# ---------------------------------------------------------------------------
# split-K
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.SPLITK_CASES, ids=lambda c: c.name)
def test_splitk_slices(gpu, case):
    """1, 2 and 4 slices of an under-filled FAST grid, launched twice (the last arriver
    resets the tile's ticket): the same bits as the oracle each time."""
    nat = fn.native()
    o = ec.operands(case)
    d = to_gpu(case, o, gpu)
    for slices in (1, 2, 4):
        with tuned(splitk=slices, ring=0):
            generic_only(case)
            nbytes = nat.conv_gemm_splitk_bytes(mode_id(case), case.geom())
            bm, bn = tile(case)
            tiles = -(-rows(case) // bm) * -(-case.ncol // bn)
            assert (nbytes > 0) == (slices > 1)
            assert nbytes % (tiles * bm * bn * 4) == 0
            for rep in range(2):
                out = launch(case, d)
                check(out, o["want"], f"{case.name} splitk={slices} launch {rep}")
        print(f"{case.name}: split-K max {slices}, {nbytes} slab bytes, {tiles} tiles {bm}x{bn}")


# ---------------------------------------------------------------------------
# stride-2 dgrad by parity class
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.PARITY_CASES, ids=lambda c: c.name)
def test_parity_class_dgrad(gpu, case):
    """k in {1, 3}; even H and odd H (the four classes then have different row counts);
    with and without accumulate; parity classes on and off."""
    o = ec.operands(case)
    d = to_gpu(case, o, gpu)
    for parity in (0, 1):
        with tuned(parity_dgrad=parity, ring=0):
            generic_only(case)
            out = launch(case, d)
        check(out, o["want"], f"{case.name} parity={parity}")
    print(f"{case.name}: stride-2 dgrad, parity classes and masked taps, tile {tile(case)}")


# ---------------------------------------------------------------------------
# LDS-DMA ring loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.RING_CASES, ids=lambda c: c.name)
def test_ring_loop(gpu, case):
    nat = fn.native()
    o = ec.operands(case)
    d = to_gpu(case, o, gpu)
    bn_want = 64 if case.name.endswith("n64") else 128
    for ring in (0, 1):
        with tuned(ring=ring):
            assert nat.conv_ring_covers(mode_id(case), case.geom()) == bool(ring)
            assert not nat.conv_direct_covers(mode_id(case), case.geom())
            assert tile(case) == (128, bn_want)
            nbytes = nat.conv_gemm_splitk_bytes(mode_id(case), case.geom())
            if ring:
                assert (nbytes > 0) == (case.name in ec.RING_SPLITK)
            for rep in range(2):
                out = launch(case, d)
                check(out, o["want"], f"{case.name} ring={ring} launch {rep}")
    print(f"{case.name}: ring loop and register loop, tile 128x{bn_want}, split-K bytes {nbytes}")


# ---------------------------------------------------------------------------
# direct 3x3 kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.DIRECT_CASES, ids=lambda c: c.name)
def test_direct_3x3(gpu, case):
    """Forward (plain; prologue + residual) and dgrad (plain; accumulate) of the direct
    kernel at 16@32, 32@16 and 64@8, one image and three, with the column split automatic,
    off and fully on."""
    nat = fn.native()
    o = ec.operands(case)
    d = to_gpu(case, o, gpu)
    for splitn in (-1, 0, 7):
        with tuned(direct_splitn=splitn):
            assert nat.conv_direct_covers(mode_id(case), case.geom())
            out = launch(case, d)
        check(out, o["want"], f"{case.name} direct_splitn={splitn}")
    print(f"{case.name}: direct 3x3 kernel, row tile {tile(case)[0]}")


@pytest.mark.parametrize("C,H,N", ec.ABWD_CASES)
@pytest.mark.parametrize("with_add", [False, True])
def test_direct_dgrad_fused_bn_backward_exact(gpu, C, H, N, with_add):
    """The direct dgrad's BN-backward prologue with precomputed coefficients (cnt = 0):
    a_out == a*g - b - c*xhat (+ add) and the dgrad of it, both exactly."""
    nat = fn.native()
    o = ec.abwd_operands(C, H, N, with_add)
    bf = {k: o[k].to(BF).to(gpu) for k in ("da", "x", "add")}
    f32 = {k: o[k].float().to(gpu) for k in ("mean", "rstd", "scale", "shift", "coef")}
    w = o["w"].to(BF).to(gpu)
    gamma = torch.ones(C, device=gpu)
    dg, db = torch.zeros(C, device=gpu), torch.zeros(C, device=gpu)
    for splitn in (-1, 0, 7):
        dh = torch.full((N, H, H, C), float("nan"), device=gpu, dtype=BF)
        dx = torch.full((N, H, H, C), float("nan"), device=gpu, dtype=BF)
        with tuned(direct_splitn=splitn):
            assert nat.conv_direct_covers(1, [N, H, H, C, H, H, C, 3, 3, 1, 1])
            fn.conv2d_dgrad(bf["da"], w, (N, H, H, C), 1, out=dx,
                            abwd=[bf["x"], bf["add"] if with_add else 0, f32["mean"], f32["rstd"],
                                  f32["scale"], f32["shift"], gamma, 0, 0, dh, dg, db,
                                  f32["coef"]])
        check(dh, o["dh"], f"abwd {C}@{H} n{N} a_out splitn={splitn}")
        check(dx, o["want"], f"abwd {C}@{H} n{N} dgrad splitn={splitn}")
    print(f"abwd {C}@{H} n{N} add={with_add}: direct dgrad with the fused BN backward")


# ---------------------------------------------------------------------------
# streaming 1x1 kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,C,K", ec.BNF_CASES)
@pytest.mark.parametrize("pre", [False, True], ids=["nopre", "pre"])
def test_streaming_1x1_forward(gpu, M, C, K, pre):
    nat = fn.native()
    assert nat.bnf1x1_covers(M, C, K)
    assert not nat.bnf1x1_covers(M + 8, C, K)      # whole row tiles only
    case, o = ec.bnf_operands(M, C, K, pre)
    d = to_gpu(case, o, gpu)
    out = torch.full((M, C), float("nan"), device=gpu, dtype=BF)
    sacc = torch.zeros(nat.bn_acc_rep() * 2 * C, device=gpu, dtype=torch.float64)
    nat.bnf1x1([d["a"].data_ptr(), d["w_ohwi"].data_ptr(), d["res"].data_ptr(), out.data_ptr(),
                d["sc"].data_ptr() if pre else 0, d["sh"].data_ptr() if pre else 0,
                sacc.data_ptr()], [], M, C, K, 0.997, BN_EPS, 1, fn._stream())
    check(out, o["want"], f"bnf1x1 {(M, C, K)} pre={pre}")
    print(f"bnf1x1 {(M, C, K)} {'pre' if pre else 'nopre'} + residual: streaming forward")


@pytest.mark.parametrize("M,C,K", ec.BND_CASES)
@pytest.mark.parametrize("with_add", [False, True])
def test_streaming_1x1_dgrad_apply(gpu, M, C, K, with_add):
    """bnd1x1 mode 1 with given coefficients.  The kernel rounds the dgrad to bf16 before the
    BN backward on purpose (exact_conv.bnd_operands): the operands keep that intermediate an
    integer of magnitude <= 256, which bf16 holds exactly, so one rounding acts."""
    nat = fn.native()
    assert nat.bnd1x1_covers(M, C, K)
    assert not nat.bnd1x1_covers(M + 8, C, K)
    o = ec.bnd_operands(M, C, K, with_add)
    bf = {k: o[k].to(BF).to(gpu).contiguous() for k in ("dz", "w", "x", "add")}
    f32 = {k: o[k].float().to(gpu) for k in ("mean", "rstd", "scale", "shift", "coef")}
    out = torch.full((M, C), float("nan"), device=gpu, dtype=BF)
    nat.bnd1x1(1, [bf["dz"].data_ptr(), bf["w"].data_ptr(), bf["x"].data_ptr(),
                   bf["add"].data_ptr() if with_add else 0, out.data_ptr(),
                   f32["mean"].data_ptr(), f32["rstd"].data_ptr(), f32["scale"].data_ptr(),
                   f32["shift"].data_ptr(), f32["coef"].data_ptr(), 0], M, C, K, fn._stream())
    check(out, o["want"], f"bnd1x1 mode 1 {(M, C, K)} add={with_add}")
    print(f"bnd1x1 {(M, C, K)} add={with_add}: streaming dgrad + BN backward apply")


# ---------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------
SENTINEL = -777.0


def _wgrad_slabs(wc, o, gpu, remainder=True):
    """Launch conv_wgrad under the current tuning; (slabs, splits)."""
    nat = fn.native()
    x, dy = o["x"].to(BF).to(gpu), o["dy"].to(BF).to(gpu)
    sc = o["sc"].float().to(gpu) if wc.pre else None
    sh = o["sh"].float().to(gpu) if wc.pre else None
    splits, pps = nat.wgrad_pick_splits(wc.geom())
    P = wc.N * wc.Ho * wc.Ho
    assert splits >= 2
    if remainder:
        assert P % pps != 0, "the last split must hold a remainder"
    part = torch.full((splits * wc.K * wc.k * wc.k * wc.C,), float("nan"), device=gpu)
    nat.conv_wgrad(dy.data_ptr(), x.data_ptr(), fn._ptr(sc), fn._ptr(sh), part.data_ptr(),
                   wc.geom(), splits, pps, fn._stream())
    torch.cuda.synchronize()
    return part, splits


def _reduce_variants(wc):
    return [(1.0, False, wc.K, wc.C), (0.25, True, wc.K - 6, wc.C - 5), (0.25, False, wc.K, wc.C - 8)]


@pytest.mark.parametrize("wc", ec.WGRAD_CASES, ids=lambda c: c.name)
def test_wgrad_paths_and_reduce(gpu, wc):
    """Generic split-K loop (pipelined and not), ring (on / off) and direct (on / off)
    weight gradients, then wgrad_reduce with scale, accumulate, K_valid < K and C_valid < C
    into a sentinel-filled oversized buffer: the HWIO gradient exactly, the rest untouched."""
    nat = fn.native()
    o = ec.wgrad_operands(wc)
    taps, NT = wc.k * wc.k, wc.k * wc.k * wc.C
    settings = {"generic": [dict(conv_pipe=1), dict(conv_pipe=0)],
                "ring": [dict(ring_wgrad=1), dict(ring_wgrad=0, conv_pipe=1),
                         dict(ring_wgrad=0, conv_pipe=0)],
                "direct": [dict(direct_wgrad=1), dict(direct_wgrad=0)]}[wc.path]
    for keys in settings:
        with tuned(**keys):
            direct = nat.wgrad_direct_bmp(wc.geom()) > 0
            assert direct == (wc.path == "direct" and keys["direct_wgrad"] == 1)
            # no binding tells whether the ring wgrad runs: its documented condition
            # (128x128 tiles: K > 64 and taps * C > 64)
            assert (wc.K > 64 and NT > 64) == (wc.path == "ring")
            part, splits = _wgrad_slabs(wc, o, gpu, remainder=wc.path != "direct")
        for scale, acc, kv, cv in _reduce_variants(wc):
            n = taps * cv * kv
            buf = torch.full((n + 64,), SENTINEL, device=gpu)
            want = ec.crop_hwio(o["want"], kv, cv) * scale
            if acc:
                base = ec.crop_hwio(o["base"], kv, cv)
                buf[:n] = base.float().reshape(-1).to(gpu)
                want = want + base
            nat.wgrad_reduce(part.data_ptr(), buf.data_ptr(), splits, wc.K, kv, taps, wc.C, cv,
                             scale, int(acc), fn._stream())
            what = f"{wc.name} {keys} splits={splits} scale={scale} acc={acc} Kv={kv} Cv={cv}"
            check(buf[:n].view(wc.k, wc.k, cv, kv), want, what)
            check(buf[n:], torch.full((64,), SENTINEL, dtype=torch.float64), what + " (tail)")
        print(f"{wc.name}: {wc.path} wgrad {keys}, {splits} splits")


def test_wgrad_reduce_grouped_exact(gpu):
    """wgrad_reduce_grouped over two convs in one group -- few splits (the transposed wide
    form) and many (the deep form) -- with scale 1/4, K_valid < K and C_valid < C."""
    from distributed_tensorflow_resnet_amd.train.layout import WGD_DTYPE

    nat = fn.native()
    cases = [next(c for c in ec.WGRAD_CASES if c.name == n) for n in ("wg-generic", "wg-direct-16")]
    arr = np.zeros(len(cases), dtype=WGD_DTYPE)
    keep, chunk = [], 0
    for i, wc in enumerate(cases):
        o = ec.wgrad_operands(wc)
        part, splits = _wgrad_slabs(wc, o, gpu, remainder=wc.path != "direct")
        kv, cv, taps = wc.K - 6, wc.C - 5, wc.k * wc.k
        n = taps * cv * kv
        buf = torch.full((n + 64,), SENTINEL, device=gpu)
        arr[i] = (part.data_ptr(), buf.data_ptr(), splits, wc.K, kv, taps, wc.C, cv, chunk)
        chunk += nat.wgrad_reduce_chunks(splits, wc.K, taps, wc.C)
        keep.append((wc, part, buf, n, kv, cv, splits, ec.crop_hwio(o["want"], kv, cv) * 0.25))
    assert min(k[6] for k in keep) <= 8 < max(k[6] for k in keep)   # both work-unit forms
    t = torch.from_numpy(arr.view(np.uint8).copy()).to(gpu)
    nat.wgrad_reduce_grouped(t.data_ptr(), len(cases), chunk, 0.25, fn._stream())
    for wc, part, buf, n, kv, cv, splits, want in keep:
        check(buf[:n].view(wc.k, wc.k, cv, kv), want, f"grouped {wc.name} splits={splits}")
        check(buf[n:], torch.full((64,), SENTINEL, dtype=torch.float64), f"grouped {wc.name} tail")
    print(f"wgrad_reduce_grouped: splits {[k[6] for k in keep]}")
