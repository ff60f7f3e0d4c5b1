"""Every BatchNorm kernel of csrc/bn.hip (and bnrelu_avgpool / avgpool_bwd of csrc/head.hip)
against the fp64 oracle tests/bn_oracle.py, per element or per channel, each kernel handed
the oracle's (or a checked kernel's) inputs so that a failure points at that kernel alone.
Every tolerance is a bound function of bn_oracle (derivations there); a failure names the
worst offender's index.  Both finalize variants are forced with set_fin_version on every
shape, and the automatic choice is pinned bitwise to the variant the documented rule names
(C <= 512 and tiles >= 1024 forward, >= 256 backward -> the per-channel kernel)."""
import contextlib

import pytest
import torch

import bn_oracle as bo
from bn_oracle import f64
from distributed_tensorflow_resnet_amd import native
from distributed_tensorflow_resnet_amd.ops import functional as fn

pytestmark = pytest.mark.gpu
F32 = torch.float32
FWD_VARIANTS = {"tree": 0, "chan": 2}     # bn_finalize_kernel / bn_finalize_chan_kernel
BWD_VARIANTS = {"tile": 0, "chan": 2}     # bn_bwd_finalize_kernel / bn_bwd_finalize_chan_kernel


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(name, got, ref, bound, alt=None, alt_ok=None):
    msg = bo.worst(got, ref, bound, alt, alt_ok)
    assert msg is None, f"{name}: {msg}"


@contextlib.contextmanager
def fin_version(v):
    nat = native(required=True)
    nat.set_fin_version(v)
    try:
        yield nat
    finally:
        nat.set_fin_version(1)


def _capped(amb):
    share = bo.ambiguous_share(amb)
    assert share <= bo.AMBIGUOUS_CAP, f"ambiguous-mask set holds {share:.2%} of the elements"


# ---------------------------------------------------------------------------
# forward finalize
# ---------------------------------------------------------------------------
def _run_fin(nat, gpu, part, tiles, tile_rows, M, C, vecs, update=1):
    gamma, beta, mm, mv = (v.to(gpu) for v in vecs)
    mm, mv = mm.clone(), mv.clone()
    outs = [torch.full((C,), float("nan"), device=gpu) for _ in range(4)]
    p = part.to(gpu)
    nat.bn_finalize(p.data_ptr(), tiles, tile_rows, M, C, gamma.data_ptr(), beta.data_ptr(),
                    mm.data_ptr(), mv.data_ptr(), bo.MOMENTUM, bo.EPS, update,
                    *[t.data_ptr() for t in outs], _st())
    torch.cuda.synchronize()
    return [t.cpu() for t in outs] + [mm.cpu(), mv.cpu()]


def _check_fin(name, out, fin, variant, tiles, vecs):
    gamma, beta, mm, mv = vecs
    mean, rstd, sc, sh, mm2, mv2 = out
    ulps = float(bo.ulp_distance32(f64(rstd), bo.round_f32(fin.rstd)).max())
    print(f"RSTD_ULP [{name}] {ulps:.2f}")
    _ok(name + " mean", mean, fin.mean, bo.fin_mean_bound(variant, tiles, fin))
    _ok(name + " rstd", rstd, fin.rstd, bo.rstd_bound(fin))
    _ok(name + " scale", sc, f64(gamma) * f64(rstd), bo.scale_bound(gamma, rstd))
    _ok(name + " shift", sh, f64(beta) - f64(mean) * f64(sc), bo.shift_bound(beta, mean, sc))
    _ok(name + " moving_mean", mm2, fin.mm, bo.fin_mm_bound(variant, tiles, fin, mm))
    _ok(name + " moving_var", mv2, fin.mv, bo.fin_mv_bound(variant, tiles, fin, mv))


def _fin_ids(variants):
    return [pytest.param(v, t, last, C, id=f"{v}-tiles{t}-last{last}-C{C}")
            for t in bo.FIN_TILES for last in bo.FIN_LAST for v in variants for C in bo.FIN_CS]


@pytest.mark.parametrize("variant,tiles,last,C", _fin_ids(FWD_VARIANTS))
def test_bn_finalize_fwd(gpu, variant, tiles, last, C):
    """Synthetic 4-row partials (M = 1 with tiles = last = 1; the last tile full or one row;
    4097 and 5003 tiles run the per-channel kernel's beyond-one-round loops), nonzero
    starting moving averages, the forced variant against the oracle, and the automatic
    choice bitwise equal to it where the rule names it."""
    M, _, p = bo.fin_source(tiles, last)
    part = bo.pack_partials(p.mean[:, :C], p.m2[:, :C])
    vecs = bo.make_vecs(C, tiles)
    fin = bo.finalize(part, tiles, bo.FIN_TILE_ROWS, M, *vecs)
    with fin_version(FWD_VARIANTS[variant]) as nat:
        out = _run_fin(nat, gpu, part, tiles, bo.FIN_TILE_ROWS, M, C, vecs)
    _check_fin(f"fwd-{variant} tiles={tiles} last={last} C={C}", out, fin, variant, tiles, vecs)
    rule = "chan" if (C <= 512 and tiles >= 1024) else "tree"
    if rule == variant:
        auto = _run_fin(native(required=True), gpu, part, tiles, bo.FIN_TILE_ROWS, M, C, vecs)
        for a, b in zip(auto, out):
            assert torch.equal(a, b), "auto dispatch is not the variant the rule names"


@pytest.mark.parametrize("variant", ["tree", "chan", "acc"])
def test_bn_finalize_fwd_keeps_moving_averages(gpu, variant):
    """update_moving = 0: mm and mv untouched bit for bit, the statistics unchanged."""
    tiles, last, C = 257, 1, 80
    M, x, p = bo.fin_source(tiles, last)
    vecs = bo.make_vecs(C, tiles)
    nat = native(required=True)
    if variant == "acc":
        part, t_arg, ver = bo.make_acc(x[:, :C], nat.bn_acc_rep()), -1, 1
    else:
        part, t_arg, ver = bo.pack_partials(p.mean[:, :C], p.m2[:, :C]), tiles, FWD_VARIANTS[variant]
    with fin_version(ver):
        on = _run_fin(nat, gpu, part, t_arg, bo.FIN_TILE_ROWS, M, C, vecs, update=1)
        off = _run_fin(nat, gpu, part, t_arg, bo.FIN_TILE_ROWS, M, C, vecs, update=0)
    assert torch.equal(off[4], vecs[2]) and torch.equal(off[5], vecs[3])
    assert not torch.equal(on[4], vecs[2]) and not torch.equal(on[5], vecs[3])
    for a, b in zip(on[:4], off[:4]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("C", bo.ACC_CS)
@pytest.mark.parametrize("M", [1, 1003])
def test_bn_finalize_fwd_acc(gpu, M, C):
    """bn_finalize_acc_kernel: replicas with unequal shares, C across the 256-thread block."""
    nat = native(required=True)
    x = f64(bo.make_x(M, C, bo.case_seed(M, C)))
    acc = bo.make_acc(x, nat.bn_acc_rep())
    vecs = bo.make_vecs(C, M)
    fin = bo.finalize_acc(acc, M, *vecs)
    out = _run_fin(nat, gpu, acc, -1, 0, M, C, vecs)
    _check_fin(f"fwd-acc M={M} C={C}", out, fin, "acc", 0, vecs)


# ---------------------------------------------------------------------------
# backward finalize
# ---------------------------------------------------------------------------
def _run_bwd_fin(nat, gpu, part, tiles, M, C, gamma, rstd):
    outs = [torch.full((n,), float("nan"), device=gpu) for n in (C, C, 3 * C)]   # dgamma dbeta coef
    p, g, r = part.to(gpu), gamma.to(gpu), rstd.to(gpu)
    nat.bn_bwd_finalize(p.data_ptr(), tiles, M, C, g.data_ptr(), r.data_ptr(),
                        *[t.data_ptr() for t in outs], _st())
    torch.cuda.synchronize()
    return [t.cpu() for t in outs]


def _check_bwd_fin(name, out, s1, s2, a1, a2, chain, M, gamma, rstd):
    dgamma, dbeta, coef = out
    bf = bo.bwd_finalize(s1, s2, M, gamma, rstd)
    d1, d2 = bo.sum_bound(chain, a1), bo.sum_bound(chain, a2)
    _ok(name + " dbeta", dbeta, bf.dbeta, d1)
    _ok(name + " dgamma", dgamma, bf.dgamma, d2)
    _ok(name + " coef", coef, bf.coef, bo.coef_bounds(bf, M, d1, d2))


@pytest.mark.parametrize("variant,tiles,last,C", _fin_ids(BWD_VARIANTS))
def test_bn_bwd_finalize(gpu, variant, tiles, last, C):
    """The backward finalize only sums its partials, so they are random fp32 numbers with a
    per-channel offset (no two tiles or channels alike); C = 80 is a partial 64-channel
    block of the tile kernel."""
    M = (tiles - 1) * bo.FIN_TILE_ROWS + last
    g = torch.Generator().manual_seed(bo.case_seed(tiles, last, C))
    part = (torch.randn(tiles, 2, C, generator=g) + torch.linspace(-1, 1, C)).contiguous()
    gamma, _, _, rstd = bo.make_vecs(C, tiles)
    s = bo.sum_partials(part, tiles)
    with fin_version(BWD_VARIANTS[variant]) as nat:
        out = _run_bwd_fin(nat, gpu, part, tiles, M, C, gamma, rstd)
    _check_bwd_fin(f"bwd-{variant}", out, *s, bo.bwd_fin_chain(variant, tiles), M, gamma, rstd)
    rule = "chan" if (C <= 512 and tiles >= 256) else "tile"
    if rule == variant:
        auto = _run_bwd_fin(native(required=True), gpu, part, tiles, M, C, gamma, rstd)
        for a, b in zip(auto, out):
            assert torch.equal(a, b), "auto dispatch is not the variant the rule names"


@pytest.mark.parametrize("C", bo.ACC_CS)
def test_bn_bwd_finalize_acc(gpu, C):
    nat = native(required=True)
    M = 1003
    g = torch.Generator().manual_seed(bo.case_seed(M, C))
    a = torch.randn(M, C, dtype=bo.F64, generator=g)
    b = torch.randn(M, C, dtype=bo.F64, generator=g) * 3 + 0.5
    acc = bo.make_acc(a, nat.bn_acc_rep(), second=b)
    gamma, _, _, rstd = bo.make_vecs(C, M)
    s1, s2 = bo.acc_sums(acc)
    out = _run_bwd_fin(nat, gpu, acc, -1, M, C, gamma, rstd)
    _check_bwd_fin("bwd-acc", out, s1, s2, s1.abs(), s2.abs(), bo.bwd_fin_chain("acc", 0), M,
                   gamma, rstd)


# ---------------------------------------------------------------------------
# bn_eval
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 257 * 8])
def test_bn_eval(gpu, C):
    nat = native(required=True)
    gamma, beta, mm, mv = bo.make_vecs(C, C)
    d = [v.to(gpu) for v in (gamma, beta, mm, mv)]
    scale, shift = (torch.full((C,), float("nan"), device=gpu) for _ in range(2))
    nat.bn_eval(*[t.data_ptr() for t in d], bo.EPS, C, scale.data_ptr(), shift.data_ptr(), _st())
    torch.cuda.synchronize()
    ref_scale, _ = bo.eval_reference(gamma, beta, mm, mv)
    _ok("bn_eval scale", scale, ref_scale, bo.eval_scale_bound(gamma, mv))
    sc = scale.cpu()
    _ok("bn_eval shift", shift, f64(beta) - f64(mm) * f64(sc), bo.shift_bound(beta, mm, sc))


# ---------------------------------------------------------------------------
# per-tile partials
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", bo.STATS_CASES)
def test_bn_stats_partials(gpu, M, C):
    """rows_per_iter 128, 32, 8, 1 x the 8-row batched loop, its remainder loop and a last
    tile with fewer rows than rows_per_iter: (mean, M2) per tile and channel."""
    inp = bo.inputs(M, C)
    part, tiles, rows = fn.bn_stats(inp.x.to(gpu))
    assert rows == bo.BN_TILE_ROWS
    p = bo.tile_partials(f64(inp.x), rows)
    got = part.view(tiles, 2, C).cpu()
    _ok("bn_stats mean", got[:, 0], p.mean, bo.stats_mean_bound(C, p))
    _ok("bn_stats M2", got[:, 1], p.m2, bo.stats_m2_bound(C, p))


def _stat_ptrs(inp, gpu):
    d = [v.to(gpu) for v in (inp.mean, inp.rstd, inp.scale, inp.shift)]
    return d, [t.data_ptr() for t in d]


@pytest.mark.parametrize("M,C", bo.STATS_CASES)
def test_bn_bwd_reduce_partials(gpu, M, C):
    nat = native(required=True)
    inp = bo.inputs(M, C)
    s = bo.bwd_sums(f64(inp.dy), f64(inp.x), *[f64(v) for v in (inp.mean, inp.rstd, inp.scale, inp.shift)])
    _capped(s.amb)
    tiles = nat.bn_bwd_tiles(M, C)
    assert tiles == s.sg.shape[0]
    part = torch.full((tiles, 2, C), float("nan"), device=gpu)
    dy, x = inp.dy.to(gpu), inp.x.to(gpu)
    keep, ptrs = _stat_ptrs(inp, gpu)
    nat.bn_bwd_reduce(dy.data_ptr(), x.data_ptr(), *ptrs, M, C, part.data_ptr(), _st())
    torch.cuda.synchronize()
    b1, b2 = bo.bwd_reduce_bounds(C, s)
    _ok("bn_bwd_reduce sum g", part[:, 0], s.sg, b1)
    _ok("bn_bwd_reduce sum g*xhat", part[:, 1], s.sgx, b2)


# ---------------------------------------------------------------------------
# backward apply
# ---------------------------------------------------------------------------
def _vec64(inp):
    return [f64(v) for v in (inp.mean, inp.rstd, inp.scale, inp.shift)]


@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("M,C", bo.BWD_APPLY_CASES)
def test_bn_bwd_apply(gpu, M, C, with_add):
    """U = 2 grid, 4096-block cap: nvec no multiple of 512, and (65539, 256) with a second
    grid-stride round and a ragged end.  The coefficients are the oracle's."""
    nat = native(required=True)
    inp = bo.inputs(M, C)
    dy64, x64, vec = f64(inp.dy), f64(inp.x), _vec64(inp)
    g, gx, _, _ = bo.bwd_terms(dy64, x64, *vec)
    coef = bo.bwd_finalize(g.sum(0), gx.sum(0), M, inp.gamma, inp.rstd).coef.to(F32)
    del g, gx
    add64 = f64(inp.add) if with_add else None
    ref, flip, S, amb = bo.bwd_apply(dy64, x64, *vec, f64(coef), add64)
    _capped(amb)
    dy, x, cf = inp.dy.to(gpu), inp.x.to(gpu), coef.to(gpu).contiguous()
    ad = inp.add.to(gpu) if with_add else None
    keep, ptrs = _stat_ptrs(inp, gpu)
    dx = torch.full_like(dy, float("nan"))
    nat.bn_bwd_apply(dy.data_ptr(), x.data_ptr(), *ptrs, cf.data_ptr(),
                     ad.data_ptr() if with_add else 0, dx.data_ptr(), M, C, _st())
    torch.cuda.synchronize()
    _ok("bn_bwd_apply dx", dx, ref, bo.bf16_out_bound(ref, S, bo.K_BWD_APPLY), flip, amb)


@pytest.mark.parametrize("M,C", bo.BWD_APPLY_ACC_CASES)
def test_bn_bwd_apply_acc(gpu, M, C):
    """The apply with the accumulator finalize fused in: the U = 2 grid (C <= 64) and the
    capped U = 4 grid past 256*256*4 vectors, from TRUE accumulator sums of g and g*xhat
    (unequal replica shares): dgamma, dbeta, coef per channel, dx per element."""
    nat = native(required=True)
    assert nat.bn_bwd_apply_acc_fits(M, C), "the grid rule no longer admits this shape"
    inp = bo.inputs(M, C)
    dy64, x64, vec = f64(inp.dy), f64(inp.x), _vec64(inp)
    g, gx, amb, _ = bo.bwd_terms(dy64, x64, *vec)
    _capped(amb)
    acc = bo.make_acc(g, nat.bn_acc_rep(), second=gx)
    s1, s2 = bo.acc_sums(acc)
    dy, x, ad, accd, gam_ = (t.to(gpu) for t in (inp.dy, inp.x, inp.add, acc, inp.gamma))
    keep, ptrs = _stat_ptrs(inp, gpu)
    dg, db, coef = (torch.full((n,), float("nan"), device=gpu) for n in (C, C, 3 * C))
    dx = torch.full_like(dy, float("nan"))
    nat.bn_bwd_apply_acc(dy.data_ptr(), x.data_ptr(), *ptrs,
                         [accd.data_ptr(), gam_.data_ptr(), dg.data_ptr(), db.data_ptr(),
                          coef.data_ptr()], ad.data_ptr(), dx.data_ptr(), M, C, _st())
    torch.cuda.synchronize()
    _check_bwd_fin("bwd_apply_acc", [dg.cpu(), db.cpu(), coef.cpu()], s1, s2, s1.abs(), s2.abs(),
                   bo.bwd_fin_chain("acc", 0), M, inp.gamma, inp.rstd)
    ref, flip, S, amb = bo.bwd_apply(dy64, x64, *vec, f64(coef).view(3, C), f64(inp.add))
    _ok("bn_bwd_apply_acc dx", dx, ref, bo.bf16_out_bound(ref, S, bo.K_BWD_APPLY), flip, amb)


# ---------------------------------------------------------------------------
# forward apply
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", bo.APPLY_CASES)
def test_bn_relu_apply(gpu, M, C):
    """(65539, 256): the 8192-block cap plus a tail."""
    inp = bo.inputs(M, C)
    ref, S, amb = bo.apply(f64(inp.x), f64(inp.scale), f64(inp.shift))
    _capped(amb)
    y = fn.bn_relu_apply(inp.x.to(gpu), inp.scale.to(gpu), inp.shift.to(gpu))
    _ok("bn_relu_apply y", y, ref, bo.bf16_out_bound(ref, S, bo.K_APPLY))


@pytest.mark.parametrize("M,C", bo.APPLY_ACC_CASES)
def test_bn_relu_apply_acc(gpu, M, C):
    """Finalize fused into the materializing pass: all four statistics and both moving
    averages per channel against finalize_acc, y per element from the kernel's own
    (checked) scale and shift."""
    nat = native(required=True)
    inp = bo.inputs(M, C)
    x64 = f64(inp.x)
    acc = bo.make_acc(x64, nat.bn_acc_rep())
    vecs = (inp.gamma, inp.beta, inp.mm, inp.mv)
    fin = bo.finalize_acc(acc, M, *vecs)
    x, accd = inp.x.to(gpu), acc.to(gpu)
    gamma, beta, mm, mv = (v.to(gpu).clone() for v in vecs)
    outs = [torch.full((C,), float("nan"), device=gpu) for _ in range(4)]
    y = torch.full_like(x, float("nan"))
    nat.bn_relu_apply_acc(x.data_ptr(), y.data_ptr(), M, C, accd.data_ptr(), gamma.data_ptr(),
                          beta.data_ptr(), mm.data_ptr(), mv.data_ptr(), bo.MOMENTUM, bo.EPS, 1,
                          *[t.data_ptr() for t in outs], _st())
    torch.cuda.synchronize()
    out = [t.cpu() for t in outs] + [mm.cpu(), mv.cpu()]
    _check_fin(f"apply_acc M={M} C={C}", out, fin, "acc", 0, vecs)
    ref, S, amb = bo.apply(x64, f64(out[2]), f64(out[3]))
    _capped(amb)
    _ok("bn_relu_apply_acc y", y, ref, bo.bf16_out_bound(ref, S, bo.K_APPLY))


# ---------------------------------------------------------------------------
# pooled head
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,HW,C", bo.POOL_CASES)
def test_bnrelu_avgpool_and_backward(gpu, N, HW, C):
    nat = native(required=True)
    inp = bo.inputs(N * HW, C)
    x = inp.x.view(N, HW, C)
    ref, S, widen, amb = bo.avgpool(f64(x), f64(inp.scale), f64(inp.shift))
    _capped(amb)
    xd, sc, sh = x.to(gpu), inp.scale.to(gpu), inp.shift.to(gpu)
    pooled = torch.full((N, C), float("nan"), device=gpu, dtype=bo.BF)
    nat.bnrelu_avgpool(xd.data_ptr(), sc.data_ptr(), sh.data_ptr(), pooled.data_ptr(), N, HW, C,
                       _st())
    torch.cuda.synchronize()
    _ok("bnrelu_avgpool", pooled, ref,
        bo.bf16_out_bound(ref, S, bo.pool_chain(HW, C) + 1) + widen)
    dp = inp.dy[:N].contiguous()
    r, Sb = bo.avgpool_bwd(f64(dp), HW)
    dpd = dp.to(gpu)
    dx = torch.full((N, HW, C), float("nan"), device=gpu, dtype=bo.BF)
    nat.avgpool_bwd(dpd.data_ptr(), dx.data_ptr(), N, HW, C, _st())
    torch.cuda.synchronize()
    _ok("avgpool_bwd", dx, r, bo.bf16_out_bound(r, Sb, bo.K_POOL_BWD))


# ---------------------------------------------------------------------------
# the chain, once
# ---------------------------------------------------------------------------
def test_bn_chain_on_hard_input(gpu):
    """bn_stats -> bn_finalize -> bn_relu_backward on (769, 64) with per-channel means over
    [-40, 40] and std 0.5 (a one-pass variance loses its digits there).  Each stage is
    held to its own bound given the previous stage's output, and the statistics of the
    ORIGINAL x to the bounds composed: the partials' errors carried through an exact Chan
    combine (stats_chain_propagation) on top of the finalize's own."""
    nat = native(required=True)
    M, C = bo.CHAIN_CASE
    inp = bo.inputs(M, C, hard=True)
    x64, dy64 = f64(inp.x), f64(inp.dy)
    x, dy = inp.x.to(gpu), inp.dy.to(gpu)
    vecs = (inp.gamma, inp.beta, inp.mm, inp.mv)
    part, tiles, rows = fn.bn_stats(x)
    p = bo.tile_partials(x64, rows)
    pk = part.view(tiles, 2, C).cpu()
    _ok("chain stats mean", pk[:, 0], p.mean, bo.stats_mean_bound(C, p))
    _ok("chain stats M2", pk[:, 1], p.m2, bo.stats_m2_bound(C, p))
    mm, mv = inp.mm.to(gpu).clone(), inp.mv.to(gpu).clone()
    gam_, bet = inp.gamma.to(gpu), inp.beta.to(gpu)
    mean, rstd, scale, shift = fn.bn_finalize(part, tiles, rows, M, gam_, bet, mm, mv,
                                              momentum=bo.MOMENTUM, eps=bo.EPS)
    torch.cuda.synchronize()
    out = [t.cpu() for t in (mean, rstd, scale, shift, mm, mv)]
    variant = "chan" if (C <= 512 and tiles >= 1024) else "tree"
    fin_k = bo.finalize(pk, tiles, rows, M, *vecs)          # of the kernel's partials
    _check_fin("chain finalize", out, fin_k, variant, tiles, vecs)
    # composed: against the statistics of x itself
    fin_x = inp.fin
    dmean, dm2 = bo.stats_chain_propagation(p, fin_x)
    k = 1.0 - bo.f32(bo.MOMENTUM)
    d_mean = bo.fin_mean_bound(variant, tiles, fin_k) + dmean
    _ok("chain mean of x", out[0], x64.mean(0), d_mean)
    # rstd, scale, shift of x: the partials' M2 error through d rstd / d var, the finalize's
    # own M2 error likewise, RSTD_ULPS for the rsqrt, then one / two roundings more
    var_x = x64.var(0, unbiased=False)
    d_var = (dm2 + bo.fin_m2_bound(variant, tiles, fin_k)) / M
    rstd_x = (var_x + bo.f32(bo.EPS)) ** -0.5
    d_rstd = bo.rstd_bound(fin_k) + bo.rstd_propagation(var_x, fin_k.var, d_var)
    _ok("chain rstd of x", out[1], rstd_x, d_rstd)
    g64, b64 = f64(inp.gamma), f64(inp.beta)
    scale_x = g64 * rstd_x
    d_scale = g64.abs() * d_rstd + bo.scale_bound(inp.gamma, out[1])
    _ok("chain scale of x", out[2], scale_x, d_scale)
    d_shift = (x64.mean(0).abs() * d_scale + (scale_x.abs() + d_scale) * d_mean
               + bo.shift_bound(inp.beta, out[0], out[2]))
    _ok("chain shift of x", out[3], b64 - x64.mean(0) * scale_x, d_shift)
    uvar = x64.var(0, unbiased=True)
    mv_x = f64(inp.mv) - k * (f64(inp.mv) - uvar)
    _ok("chain moving_var of x", out[5], mv_x,
        bo.fin_mv_bound(variant, tiles, fin_k, inp.mv) + k * dm2 / (M - 1))
    # backward from the kernel's statistics
    vec = [f64(t) for t in out[:4]]
    s = bo.bwd_sums(dy64, x64, *vec)
    _capped(s.amb)
    dx, dgamma, dbeta = fn.bn_relu_backward(dy, x, mean, rstd, scale, shift, gam_)
    torch.cuda.synchronize()
    b1, b2 = bo.bwd_reduce_bounds(C, s)
    ch = bo.bwd_fin_chain("chan" if (C <= 512 and tiles >= 256) else "tile", tiles)
    d1 = b1.sum(0) + bo.sum_bound(ch, s.abs_g.sum(0) + b1.sum(0))
    d2 = b2.sum(0) + bo.sum_bound(ch, s.abs_gx.sum(0) + b2.sum(0))
    _ok("chain dbeta", dbeta, s.sg.sum(0), d1)
    _ok("chain dgamma", dgamma, s.sgx.sum(0), d2)
    # dx from the coefficients those sums imply (fp32, as the apply reads them)
    a32 = inp.gamma * out[1]
    coef = torch.stack([a32, a32 * dbeta.cpu() / M, a32 * dgamma.cpu() / M])
    ref, flip, S, amb = bo.bwd_apply(dy64, x64, *vec, f64(coef))
    bfin = bo.BwdFinal(None, None, f64(coef))
    cb = bo.coef_bounds(bfin, M, torch.zeros(C, dtype=bo.F64), torch.zeros(C, dtype=bo.F64))
    xh = ((x64 - vec[0]) * vec[1]).abs()
    slack = cb[0] * dy64.abs() + cb[1] + cb[2] * xh       # the kernel's own coef roundings
    _ok("chain dx", dx, ref, bo.bf16_out_bound(ref, S, bo.K_BWD_APPLY) + slack, flip, amb)
