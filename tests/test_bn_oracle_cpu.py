"""tests/bn_oracle.py against independent truth, all on the CPU: the Chan combine against
torch's mean / var, the backward against autograd, every bound helper against a plain fp32
evaluation of the same expression (inside) and three planted kernel mistakes (outside), and
the ambiguity cap on every input set the GPU tests (test_bn_exact_gpu.py) use."""
import pytest
import torch

import bn_oracle as bo
from bn_oracle import F64, f64

F32 = torch.float32


def _rel(a, b):
    return float(((a - b).abs() / b.abs().clamp(min=1e-300)).max())


@pytest.mark.parametrize("M,tile_rows", [(1, 4), (4, 4), (8, 4), (9, 4), (11, 4), (512, 256),
                                         (513, 256), (767, 256), (1000, 7), (20009, 4)])
def test_chan_combine_equals_mean_and_var(M, tile_rows):
    x = f64(bo.make_x(M, 24, bo.case_seed(M, tile_rows)))
    p = bo.tile_partials(x, tile_rows)
    tiles = p.mean.shape[0]
    assert tiles == -(-M // tile_rows) and float(p.n.sum()) == M
    part = torch.stack([p.mean, p.m2], 1)          # fp64: no rounding of the partials here
    gamma, beta, mm, mv = bo.make_vecs(24, 1)
    fin = bo.finalize(part, tiles, tile_rows, M, gamma, beta, mm, mv)
    assert _rel(fin.mean, x.mean(0)) < 1e-12
    if M > 1:
        assert _rel(fin.var, x.var(0, unbiased=False)) < 1e-12
        assert _rel(fin.uvar, x.var(0, unbiased=True)) < 1e-12
    else:
        assert float(fin.var.abs().max()) == 0.0 and float(fin.uvar.abs().max()) == 0.0
    k = 1.0 - bo.f32(bo.MOMENTUM)
    assert _rel(fin.mm, f64(mm) - k * (f64(mm) - x.mean(0))) < 1e-12
    assert _rel(fin.rstd, (fin.var + bo.f32(bo.EPS)) ** -0.5) < 1e-12
    # accumulator form of the same statistics
    acc = bo.make_acc(x, 8)
    fa = bo.finalize_acc(acc, M, gamma, beta, mm, mv)
    assert _rel(fa.mean, fin.mean) < 1e-12
    assert float((fa.var - fin.var).abs().max()) <= 1e-12 * float((x * x).mean(0).max())


@pytest.mark.parametrize("M,C,with_add", [(37, 8, False), (300, 16, True), (769, 8, True)])
def test_backward_equals_autograd(M, C, with_add):
    inp = bo.inputs(M, C)
    x, dy = f64(inp.x), f64(inp.dy)
    add = f64(inp.add) if with_add else None
    gamma, beta = f64(inp.gamma), f64(inp.beta)
    # oracle, from exact (unrounded) statistics so that both sides see the same function
    p = bo.tile_partials(x, 256)
    fin = bo.finalize(torch.stack([p.mean, p.m2], 1), p.mean.shape[0], 256, M, inp.gamma,
                      inp.beta, inp.mm, inp.mv)
    s = bo.bwd_sums(dy, x, fin.mean, fin.rstd, fin.scale, fin.shift)
    bf = bo.bwd_finalize(s.sg.sum(0), s.sgx.sum(0), M, inp.gamma, fin.rstd)
    dx, _, S, amb = bo.bwd_apply(dy, x, fin.mean, fin.rstd, fin.scale, fin.shift, bf.coef, add)
    assert not bool(amb.any())
    # autograd of sum(relu(bn(x)) * dy) (+ the residual branch's sum(x * add))
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    xh = (xr - xr.mean(0)) / torch.sqrt(xr.var(0, unbiased=False) + bo.f32(bo.EPS))
    loss = (torch.relu(xh * gr + br) * dy).sum()
    if with_add:
        loss = loss + (xr * add).sum()
    loss.backward()
    assert float((dx - xr.grad).abs().max()) < 1e-10 * float(S.max())
    assert float((bf.dgamma - gr.grad).abs().max()) < 1e-10 * float(s.abs_gx.sum(0).max())
    assert float((bf.dbeta - br.grad).abs().max()) < 1e-10 * float(s.abs_g.sum(0).max())


# ---------------------------------------------------------------------------
# plain fp32 evaluations of the kernels' expressions (torch on the CPU: no fma contraction)
# ---------------------------------------------------------------------------
def _fp32_tree(n, m, q):
    """Pairwise Welford (wcombine) tree in fp32 over [T][C] partials."""
    n = n.to(F32)[:, None].expand_as(m).clone()
    m, q = m.clone(), q.clone()
    while n.shape[0] > 1:
        if n.shape[0] % 2:
            z = torch.zeros(1, n.shape[1], dtype=F32)
            n, m, q = torch.cat([n, z]), torch.cat([m, z]), torch.cat([q, z])
        h = n.shape[0] // 2
        (na, nb), (ma, mb), (qa, qb) = (n[:h], n[h:]), (m[:h], m[h:]), (q[:h], q[h:])
        nn = na + nb
        d = mb - ma
        fb = nb / nn.clamp(min=1)
        m = ma + d * fb
        q = qa + qb + d * d * na * fb
        n = nn
    return n[0], m[0], q[0]


def _fp32_finalize(part, n_rows, gamma, beta, mm, mv, variant, bessel=True):
    """fp32 finalize from partials [tiles][2][C] with the given per-tile row counts."""
    m, q = part[:, 0], part[:, 1]
    nf = n_rows.to(F32)
    if variant == "tree":
        N, mean, m2 = _fp32_tree(nf, m, q)
        N = float(N[0])
    else:
        N = float(nf.sum())
        mean = (nf[:, None] * m).sum(0) / N
        d = m - mean
        m2 = (q + nf[:, None] * d * d).sum(0)
    eps, k = torch.tensor(bo.EPS, dtype=F32), torch.tensor(1.0, dtype=F32) - torch.tensor(bo.MOMENTUM, dtype=F32)
    rstd = 1.0 / torch.sqrt(m2 / N + eps)
    sc = gamma * rstd
    sh = beta - mean * sc
    uvar = m2 / (N - 1) if (N > 1 and bessel) else (m2 / N if N > 1 else m2)
    return mean, rstd, sc, sh, mm - k * (mm - mean), mv - k * (mv - uvar)


def _fin_case(tiles, last, C=16):
    M, x, p = bo.fin_source(tiles, last)
    part = bo.pack_partials(p.mean[:, :C], p.m2[:, :C])
    gamma, beta, mm, mv = bo.make_vecs(C, tiles)
    fin = bo.finalize(part, tiles, bo.FIN_TILE_ROWS, M, gamma, beta, mm, mv)
    return M, part, p.n, (gamma, beta, mm, mv), fin


def _fin_failures(out, fin, variant, tiles, vecs):
    gamma, beta, mm, mv = vecs
    mean, rstd, sc, sh, mm2, mv2 = out
    checks = {
        "mean": bo.worst(mean, fin.mean, bo.fin_mean_bound(variant, tiles, fin)),
        "rstd": bo.worst(rstd, fin.rstd, bo.rstd_bound(fin)),
        "scale": bo.worst(sc, f64(gamma) * f64(rstd), bo.scale_bound(gamma, rstd)),
        "shift": bo.worst(sh, f64(beta) - f64(mean) * f64(sc), bo.shift_bound(beta, mean, sc)),
        "mm": bo.worst(mm2, fin.mm, bo.fin_mm_bound(variant, tiles, fin, mm)),
        "mv": bo.worst(mv2, fin.mv, bo.fin_mv_bound(variant, tiles, fin, mv)),
    }
    return {k: v for k, v in checks.items() if v}


@pytest.mark.parametrize("variant", ["chan", "tree"])
@pytest.mark.parametrize("tiles,last", [(1, 1), (1, 4), (257, 1), (4097, 1), (5003, 4)])
def test_fp32_finalize_inside_bounds(variant, tiles, last):
    M, part, n, vecs, fin = _fin_case(tiles, last)
    out = _fp32_finalize(part, n, *vecs, variant)
    assert not _fin_failures(out, fin, variant, tiles, vecs)


@pytest.mark.parametrize("variant", ["chan", "tree"])
def test_planted_last_tile_counted_full_is_caught(variant):
    """The mistake the beyond-one-round loop could make: 4097 tiles, 1 row in the last,
    counted as tile_rows rows."""
    tiles = 4097
    M, part, n, vecs, fin = _fin_case(tiles, 1)
    wrong = n.clone()
    wrong[-1] = bo.FIN_TILE_ROWS
    bad = _fin_failures(_fp32_finalize(part, wrong, *vecs, variant), fin, variant, tiles, vecs)
    assert "mean" in bad and "mm" in bad, bad


@pytest.mark.parametrize("variant", ["chan", "tree"])
@pytest.mark.parametrize("tiles,last", [(1, 4), (257, 1), (1024, 4)])
def test_planted_biased_moving_var_is_caught(variant, tiles, last):
    M, part, n, vecs, fin = _fin_case(tiles, last)
    out = _fp32_finalize(part, n, *vecs, variant, bessel=False)
    bad = _fin_failures(out, fin, variant, tiles, vecs)
    assert set(bad) == {"mv"}, bad


def _fp32_apply(x, scale, shift):
    return (x.to(F32) * scale + shift).clamp(min=0).to(bo.BF)


@pytest.mark.parametrize("M,C", [(257, 64), (129, 2048)])
def test_fp32_apply_inside_bound_and_shifted_group_is_caught(M, C):
    inp = bo.inputs(M, C)
    y, S, amb = bo.apply(f64(inp.x), f64(inp.scale), f64(inp.shift))
    bound = bo.bf16_out_bound(y, S, bo.K_APPLY)
    assert bo.worst(_fp32_apply(inp.x, inp.scale, inp.shift), y, bound) is None
    # planted: channel group 3 reads the coefficients of group 4
    sc, sh = inp.scale.clone(), inp.shift.clone()
    sc[24:32], sh[24:32] = inp.scale[32:40], inp.shift[32:40]
    msg = bo.worst(_fp32_apply(inp.x, sc, sh), y, bound)
    assert msg is not None and "worst at" in msg
    # planted: a small leak on the masked elements (y == 0 owes a bound of k u S, no bf16 ulp)
    good = _fp32_apply(inp.x, inp.scale, inp.shift)
    masked = y == 0
    assert 0.2 < float(masked.double().mean()) < 0.8
    assert float(bound[masked].max()) <= bo.K_APPLY * bo.U32 * float(S.max()) * 1.0001
    leak = torch.where(masked, torch.full_like(good, 1e-4), good)
    assert bo.worst(leak, y, bound) is not None
    # ... and a ReLU threshold slightly below zero
    pre32 = inp.x.to(F32) * inp.scale + inp.shift
    low = torch.where(pre32 > -1.5e-3, pre32, torch.zeros_like(pre32)).to(bo.BF)
    assert bool((f64(low) != f64(good)).any()) and bo.worst(low, y, bound) is not None


@pytest.mark.parametrize("M,C,with_add", [(257, 64, True), (129, 2048, False)])
def test_fp32_backward_inside_bounds(M, C, with_add):
    inp = bo.inputs(M, C)
    x, dy = f64(inp.x), f64(inp.dy)
    vec = [f64(v) for v in (inp.mean, inp.rstd, inp.scale, inp.shift)]
    s = bo.bwd_sums(dy, x, *vec)
    # fp32 reduce
    x32, dy32 = inp.x.to(F32), inp.dy.to(F32)
    g32 = torch.where(x32 * inp.scale + inp.shift > 0, dy32, torch.zeros_like(dy32))
    gx32 = g32 * (x32 - inp.mean) * inp.rstd
    tiles = s.sg.shape[0]
    rows = [slice(t * 256, min(M, (t + 1) * 256)) for t in range(tiles)]
    sg32 = torch.stack([g32[r].sum(0) for r in rows])
    sgx32 = torch.stack([gx32[r].sum(0) for r in rows])
    b1, b2 = bo.bwd_reduce_bounds(C, s)
    assert bo.worst(sg32, s.sg, b1) is None
    assert bo.worst(sgx32, s.sgx, b2) is None
    # fp32 finalize of those partials, both chains
    part = torch.stack([sg32, sgx32], 1)
    s1, s2, a1, a2 = bo.sum_partials(part, tiles)
    bf = bo.bwd_finalize(s1, s2, M, inp.gamma, inp.rstd)
    a32 = inp.gamma * inp.rstd
    c32 = torch.stack([a32, a32 * sg32.sum(0) / M, a32 * sgx32.sum(0) / M])
    for variant in ("tile", "chan"):
        n = bo.bwd_fin_chain(variant, tiles)
        d1, d2 = bo.sum_bound(n, a1), bo.sum_bound(n, a2)
        assert bo.worst(sg32.sum(0), bf.dbeta, d1) is None
        assert bo.worst(sgx32.sum(0), bf.dgamma, d2) is None
        assert bo.worst(c32, bf.coef, bo.coef_bounds(bf, M, d1, d2)) is None
    # fp32 apply from the fp32 coefficients
    add = inp.add if with_add else None
    dx, flip, S, amb = bo.bwd_apply(dy, x, *vec, f64(c32), f64(add) if with_add else None)
    assert bo.ambiguous_share(amb) <= bo.AMBIGUOUS_CAP
    r32 = c32[0] * g32 - c32[1] - c32[2] * ((x32 - inp.mean) * inp.rstd)
    if with_add:
        r32 = r32 + add.to(F32)
    bound = bo.bf16_out_bound(dx, S, bo.K_BWD_APPLY)
    assert bo.worst(r32.to(bo.BF), dx, bound, flip, amb) is None
    # planted: one channel group shifted by 8 in the apply's coefficients
    cs = c32.clone()
    cs[:, 8:16] = c32[:, 16:24]
    w32 = cs[0] * g32 - cs[1] - cs[2] * ((x32 - inp.mean) * inp.rstd)
    if with_add:
        w32 = w32 + add.to(F32)
    assert bo.worst(w32.to(bo.BF), dx, bound, flip, amb) is not None


@pytest.mark.parametrize("M,C", [(255, 16), (775, 64), (257, 2048)])
def test_fp32_stats_inside_bounds(M, C):
    x = bo.make_x(M, C, bo.case_seed(M, C))
    p = bo.tile_partials(f64(x), 256)
    x32 = x.to(F32)
    rows = [slice(t * 256, min(M, (t + 1) * 256)) for t in range(p.mean.shape[0])]
    mean32 = torch.stack([x32[r].sum(0) / (r.stop - r.start) for r in rows])
    m232 = torch.stack([((x32[r] - mean32[i]) ** 2).sum(0) for i, r in enumerate(rows)])
    assert bo.worst(mean32, p.mean, bo.stats_mean_bound(C, p)) is None
    assert bo.worst(m232, p.m2, bo.stats_m2_bound(C, p)) is None
    # a one-pass variance on the hard input (means up to 40, std 0.5) is outside
    xh = bo.make_x(M, C, bo.case_seed(M, C), hard=True)
    ph = bo.tile_partials(f64(xh), 256)
    xh32 = xh.to(F32)
    onepass = torch.stack([(xh32[r] ** 2).sum(0) - xh32[r].sum(0) ** 2 / (r.stop - r.start)
                           for r in rows])
    assert bo.worst(onepass, ph.m2, bo.stats_m2_bound(C, ph)) is not None


@pytest.mark.parametrize("N,HW,C", bo.POOL_CASES)
def test_fp32_pool_inside_bounds(N, HW, C):
    inp = bo.inputs(N * HW, C)
    x = inp.x.view(N, HW, C)
    pooled, S, widen, amb = bo.avgpool(f64(x), f64(inp.scale), f64(inp.shift))
    p32 = ((x.to(F32) * inp.scale + inp.shift).clamp(min=0).sum(1) / HW).to(bo.BF)
    bound = bo.bf16_out_bound(pooled, S, bo.pool_chain(HW, C) + 1) + widen
    assert bo.worst(p32, pooled, bound) is None
    dp = inp.dy[:N]
    r, Sb = bo.avgpool_bwd(f64(dp), HW)
    d32 = (dp.to(F32) * (torch.tensor(1.0, dtype=F32) / HW))[:, None, :].expand(N, HW, C).to(bo.BF)
    assert bo.worst(d32, r, bo.bf16_out_bound(r, Sb, bo.K_POOL_BWD)) is None


def test_ulp_helpers_at_zero_and_powers_of_two():
    v = torch.tensor([0.0, 1.0, 1.5, 2.0, -3.0, 2.0 ** -140], dtype=F64)
    assert bo.ulp32(v).tolist() == [2.0 ** -149, 2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -22,
                                    2.0 ** -149]
    assert bo.ulp_bf16(v).tolist() == [2.0 ** -133, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6,
                                       2.0 ** -133]
    one = torch.tensor([1.0], dtype=torch.float32)
    assert float(bo.ulp32(f64(one))) == float(torch.nextafter(one, one + 1) - one)


def test_worst_reports_the_offender():
    ref = torch.zeros(3, 5, dtype=F64)
    got = ref.clone()
    got[2, 1] = 1.0
    got[1, 4] = 0.25
    msg = bo.worst(got, ref, torch.full_like(ref, 0.1))
    assert msg.startswith("2 of 15") and "(2, 1)" in msg
    assert bo.worst(got, ref, torch.full_like(ref, 2.0)) is None
    got[0, 0] = float("nan")
    assert "(0, 0)" in bo.worst(got, ref, torch.full_like(ref, 2.0))


def _gpu_input_sets():
    sets = {(M, C, False) for M, C in bo.STATS_CASES + bo.BWD_APPLY_CASES + bo.BWD_APPLY_ACC_CASES
            + bo.APPLY_CASES + bo.APPLY_ACC_CASES}
    sets |= {(N * HW, C, False) for N, HW, C in bo.POOL_CASES}
    sets.add(bo.CHAIN_CASE + (True,))
    return sorted(sets)


@pytest.mark.parametrize("M,C,hard", _gpu_input_sets())
def test_ambiguity_cap_on_gpu_inputs(M, C, hard):
    """Every (x, scale, shift) the GPU tests feed a masked kernel: the oracle alone keeps
    the ambiguous-mask set under 0.1 % of the elements."""
    inp = bo.inputs(M, C, hard)
    _, _, amb = bo.ambiguous(f64(inp.x), f64(inp.scale), f64(inp.shift))
    assert bo.ambiguous_share(amb) <= bo.AMBIGUOUS_CAP
