"""Shampoo on the device (csrc/shampoo.hip) against the fp64 references of tests/shampoo_oracle.py.
The yardstick of every matrix result is d_ref, the distance of the oracle's own plain fp32 run
from fp64: the kernel must stay within 4 d_ref (the MFMA adds in another order).  The
element-wise parts are held bit for bit, and the engine's step to mom's until the first refresh."""
import numpy as np
import pytest
import torch

import optim_oracle as oo
import shampoo_oracle as so
from test_adam_gpu import _sa, _st, nat  # noqa: F401
from test_muon_gpu import SPECS, _engine, _hwio_only
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.ops import functional as F
from distributed_tensorflow_resnet_amd.train.layout import shampoo_block_table
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr

pytestmark = pytest.mark.gpu
EPS = 1e-4


def _spd(rng, n, lo=0.5, hi=2.0):
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    a = (q * rng.uniform(lo, hi, n)) @ q.T
    return ((a + a.T) / 2).astype(np.float32)


def _slot(a, fill=0.0):
    s = np.full((64, 64), fill, np.float32)
    s[:a.shape[0], :a.shape[1]] = a
    return s


# one tile; padding inside the tile; three tiles; all of the block
@pytest.mark.parametrize("kind", ("logspace", "gram"))
@pytest.mark.parametrize("n", (16, 27, 48, 64))
def test_roots_against_fp64(gpu, n, kind):
    rng = np.random.default_rng(100 * n + len(kind))
    if kind == "logspace":
        q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        A = (q * np.logspace(-3, 0, n)) @ q.T
    else:   # rank deficient, what the first refresh sees
        g = rng.standard_normal((n, max(4, n // 4)))
        A = g @ g.T
    A = ((A + A.T) / 2).astype(np.float32)
    stat = torch.full((3, 64, 64), 3.0)
    stat[1] = torch.from_numpy(_slot(A))
    root0 = torch.full((3, 64, 64), -7.0)
    root0[1] = torch.from_numpy(_slot(np.eye(n, dtype=np.float32)))
    sd, rd = stat.to(gpu), root0.to(gpu)
    fail = torch.zeros(1, dtype=torch.int32, device=gpu)
    F.shampoo_roots(sd[1:2], rd[1:2], [n], epsilon=EPS, step=3, every=2, fail=fail)
    assert torch.equal(rd.cpu(), root0)                       # t % every != 0: nothing moves
    F.shampoo_roots(sd[1:2], rd[1:2], [n], epsilon=EPS, step=4, every=2, fail=fail)
    got = rd.cpu()
    assert torch.equal(sd.cpu(), stat) and int(fail.item()) == 0
    assert torch.equal(got[0], root0[0]) and torch.equal(got[2], root0[2])   # the neighbours
    assert not bool(got[1, n:].any()) and not bool(got[1, :, n:].any())   # the padding stays zero
    exact = so.root_exact(A, EPS)
    x32, steps, _ = so.root_iter(A, EPS, np.float32)
    d_ref, err = so.rel(x32, exact), so.rel(got[1, :n, :n].numpy(), exact)
    print(f"shampoo roots {kind} n={n}: steps {steps} d_ref {d_ref:.3g} err {err:.3g} "
          f"ratio {err / d_ref:.3f}")
    assert err <= 4 * d_ref


def test_a_zero_statistic_keeps_its_root_and_counts_as_failed(gpu):
    stat = torch.zeros(1, 64, 64, device=gpu)
    root = torch.from_numpy(_slot(np.eye(16, dtype=np.float32)))[None].to(gpu)
    fail = torch.zeros(1, dtype=torch.int32, device=gpu)
    F.shampoo_roots(stat, root, [16], epsilon=EPS, fail=fail)
    assert int(fail.item()) == 1 and torch.equal(root.cpu()[0, :16, :16], torch.eye(16))


def _stats_dir_case(gpu, R, K, lo, b2, scale=0.5):
    """One tensor between sentinels through stats + precondition; everything on the host."""
    rng, n, hi = np.random.default_rng(1000 * R + K), R * K, 9
    G = rng.standard_normal((R, K)).astype(np.float32)
    g = torch.full((lo + n + hi,), 3.0)
    g[lo:lo + n] = torch.from_numpy(G).flatten()
    bl = so.blocks(R, K)
    st = {k: np.stack([_slot(_spd(rng, r if k in "L PL" else c)) for _, _, r, c in bl])
          for k in ("L", "R", "PL", "PR")}
    dev = {k: torch.from_numpy(v).to(gpu) for k, v in st.items()}
    gd, out = g.to(gpu), torch.full_like(g, -7.0).to(gpu)
    _, part, tab = F.shampoo_stats_precondition(gd, [(R, K)], [lo], dev["L"], dev["R"], dev["PL"],
                                                dev["PR"], beta2=b2, grad_scale=scale, out=out)
    assert torch.equal(gd.cpu(), g)                           # grad is only read
    assert [(int(b["r"]), int(b["k"])) for b in tab] == [(r, c) for _, _, r, c in bl]
    return G * np.float32(scale), bl, st, {k: v.cpu().numpy() for k, v in dev.items()}, \
        out.cpu(), part.cpu().numpy()


# scalar head and tail; three row blocks; one block; 2 x 2 ragged blocks; two column blocks
@pytest.mark.parametrize("b2", (1.0, 0.9))
@pytest.mark.parametrize("R,K,lo", [(27, 16, 7), (144, 16, 8), (16, 32, 8), (80, 72, 8),
                                    (64, 128, 8)])
def test_statistics_and_direction_against_fp64(gpu, R, K, lo, b2):
    Gs, bl, st, new, out, part = _stats_dir_case(gpu, R, K, lo, b2)
    n, U = R * K, out[lo:lo + R * K].view(R, K).numpy()
    assert bool((out[:lo] == -7.0).all()) and bool((out[lo + n:] == -7.0).all())
    assert np.array_equal(new["PL"], st["PL"]) and np.array_equal(new["PR"], st["PR"])
    ref = {k: ([], [], []) for k in ("L", "R", "U")}          # fp64, fp32, kernel
    for s, (i, j, r, c) in enumerate(bl):
        Gb = Gs[i:i + r, j:j + c]
        for k, v in (("L", new["L"][s]), ("R", new["R"][s])):
            m = r if k == "L" else c
            assert not v[m:].any() and not v[:, m:].any()     # the padding stays zero
        for dt, col in ((np.float64, 0), (np.float32, 1)):
            L, Rt = so.stats(st["L"][s, :r, :r], st["R"][s, :c, :c], Gb, b2, dt)
            u = so.direction(st["PL"][s, :r, :r], Gb, st["PR"][s, :c, :c], dt)
            for k, v in (("L", L), ("R", Rt), ("U", u)):
                ref[k][col].append(v.ravel())
        for k, v in (("L", new["L"][s, :r, :r]), ("R", new["R"][s, :c, :c]), ("U", U[i:i + r, j:j + c])):
            ref[k][2].append(v.ravel())
        want = (float((Gb.astype(np.float64) ** 2).sum()), float((ref["U"][0][-1] ** 2).sum()))
        assert np.allclose(part[s], want, rtol=1e-5, atol=0)
    for k, (x64, x32, got) in ref.items():
        x64, x32, got = (np.concatenate(x) for x in (x64, x32, got))
        d_ref, err = so.rel(x32, x64), so.rel(got, x64)
        print(f"shampoo {k} {R}x{K} b2={b2}: d_ref {d_ref:.3g} err {err:.3g} ratio {err / d_ref:.3f}")
        assert err <= 4 * d_ref
    again = _stats_dir_case(gpu, R, K, lo, b2)                # a second launch: the same bits
    assert torch.equal(again[4], out) and np.array_equal(again[5], part)
    assert all(np.array_equal(again[3][k], new[k]) for k in new)


MOM, WD, LR, SCALE = 0.8, 0.01, 0.05, 0.5


def test_graft_and_update_bit_exact(gpu, nat):
    seg, _, n, bf_total, _, _ = oo.build_seg_table(SPECS)
    segs_d = torch.from_numpy(seg.view(np.uint8).copy()).to(gpu)
    shapes, offs = [(144, 16), (16, 32)], [0, 2330]
    _, tens = shampoo_block_table([(0, 0, 144, 16), (2330, 3, 16, 32)])
    ttab = torch.from_numpy(tens.view(np.uint8).copy()).to(gpu)
    gen, rng = torch.Generator().manual_seed(3), np.random.default_rng(3)
    w0, g, m0 = (torch.randn(n, generator=gen) for _ in range(3))
    conv = torch.zeros(n, dtype=torch.bool)
    conv[:2304] = conv[2330:] = True
    roots = [np.stack([_slot(_spd(rng, r if side == 0 else c)) for _, _, r, c in
                       so.blocks(144, 16) + so.blocks(16, 32)]) for side in (0, 1)]
    pre = torch.tensor([1, 0, 0, 1], dtype=torch.int32, device=gpu)
    gstep = torch.tensor([3], dtype=torch.int64, device=gpu)

    def run():
        w, m, gd = w0.to(gpu), m0.to(gpu), g.to(gpu)
        L, Rt = (torch.zeros(4, 64, 64, device=gpu) for _ in range(2))
        PL, PR = (torch.from_numpy(r).to(gpu) for r in roots)
        wbf, lr_out = torch.zeros(bf_total, dtype=torch.bfloat16, device=gpu), torch.zeros(1, device=gpu)
        U, part, _ = F.shampoo_stats_precondition(gd, shapes, offs, L, Rt, PL, PR, grad_scale=SCALE)
        out = torch.ones(3, 4, device=gpu)
        nat.shampoo_graft(part.data_ptr(), ttab.data_ptr(), 2, 4, out.data_ptr(), _st())
        nat.shampoo_update_pack(w.data_ptr(), gd.data_ptr(), m.data_ptr(), U.data_ptr(), n,
                                *_sa(constant_lr(LR)), gstep.data_ptr(), MOM, WD, SCALE,
                                segs_d.data_ptr(), 4, pre.data_ptr(), out.data_ptr(),
                                wbf.data_ptr(), lr_out.data_ptr(), _st())
        torch.cuda.synchronize()
        return w.cpu(), m.cpu(), U.cpu(), out.cpu(), wbf.cpu()

    w1, m1, U, out, wbf = run()
    assert bool((U[~conv] == 0).all()) and out[0, 1] == 1 and out[0, 2] == 1
    vec = so.vector_path(seg["offset"], seg["numel"], n)
    for s, (a, b) in ((0, (0, 2304)), (3, (2330, n))):
        gn, un = (float(x[a:b].double().norm()) for x in (SCALE * g, U))
        assert abs(float(out[0, s]) / (gn / un) - 1) < 1e-6
        assert abs(float(out[1, s]) / gn - 1) < 1e-6 and abs(float(out[2, s]) / un - 1) < 1e-6
        d = (out[0, s] * U[a:b]).numpy()                      # c U, one rounding
        ww, mm = so.update32(w0[a:b].numpy(), m0[a:b].numpy(), d, LR, MOM, WD, vec[a:b])
        assert np.array_equal(w1[a:b].numpy(), ww) and np.array_equal(m1[a:b].numpy(), mm)
    # the other segments: sgd_update_pack itself on the same inputs
    ws, ms = w0.to(gpu), m0.to(gpu)
    nat.sgd_update_pack(ws.data_ptr(), g.to(gpu).data_ptr(), ms.data_ptr(), n, *_sa(constant_lr(LR)),
                        gstep.data_ptr(), MOM, WD, SCALE, 1, segs_d.data_ptr(), len(seg), 0, 0, 1,
                        _st())
    assert torch.equal(w1[~conv], ws.cpu()[~conv]) and torch.equal(m1[~conv], ms.cpu()[~conv])
    assert torch.equal(wbf.float(), _hwio_only(seg, w1, bf_total))
    for x, y in zip(run(), (w1, m1, U, out, wbf)):            # a second launch: the same bits
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------ engine
def _oracle_direction(grads, R, K, dtype):
    """c U of one tensor after the statistics of `grads` (b2 = 1) and a refresh, in `dtype`
    (fp64: exact roots; fp32: the iteration and the products in fp32)."""
    G, U = grads[-1], np.zeros((R, K))
    for i, j, r, c in so.blocks(R, K):
        L = sum(so.stats(0, 0, g[i:i + r, j:j + c], 1.0, dtype)[0] for g in grads)
        Rt = sum(so.stats(0, 0, g[i:i + r, j:j + c], 1.0, dtype)[1] for g in grads)
        root = (lambda a: so.root_exact(a, EPS)) if dtype is np.float64 else \
            (lambda a: so.root_iter(a, EPS, dtype)[0])
        U[i:i + r, j:j + c] = so.direction(root(L), G[i:i + r, j:j + c], root(Rt), dtype)
    return np.linalg.norm(G.astype(np.float64)) / np.linalg.norm(U) * U


@pytest.mark.parametrize("persist", (0, 1))
def test_engine_shampoo_step(gpu, monkeypatch, persist):
    monkeypatch.setenv("DTR_TUNE", f"persist={persist},opt_fused=0")
    ref = _engine(cifar_spec(8), gpu, optimizer="mom")
    monkeypatch.setenv("DTR_TUNE", f"persist={persist}")
    eng = _engine(cifar_spec(8), gpu, optimizer="shampoo", shampoo_precond_every=3,
                  shampoo_epsilon=EPS)
    assert eng.persist == bool(persist) and not eng.opt_fused and "shampoo" in eng.opt_fused_reason
    a, b = eng.seg["opt"]
    assert [n for n in eng.plan.names()[a:b] if "pack" in n or "shampoo" in n] == \
        ["shampoo_stats", "shampoo_roots", "shampoo_precondition", "shampoo_graft",
         "shampoo_update_pack", "ohwi_pack"]
    grads = []
    for step in (1, 2, 3):
        w2, m2 = eng.params.master.clone().cpu(), eng.mom.clone().cpu()
        eng.step()
        ref.step()
        torch.cuda.synchronize()
        assert not eng.persist_error() and torch.equal(eng.grad, ref.grad)
        grads.append(eng.grad.cpu())
        if step < 3:   # the roots are the identity: mom's step, bit for bit
            assert torch.equal(eng.params.master, ref.params.master) and torch.equal(eng.mom, ref.mom)
    st = eng.shampoo_state()
    assert st["t"] == 3 and st["failed"] == 0 and st["state_bytes"] == 4 * len(eng.shampoo_blocks) * 16384
    w3, m3, w_ref, checked = eng.params.master.cpu(), eng.mom.cpu(), ref.params.master.cpu(), 0
    for s in eng.params.train_slots:
        sl = slice(s.offset, s.offset + s.numel)
        assert torch.equal(w3[sl], w_ref[sl]) == (s.kind != "conv"), s.name
        if s.kind != "conv" or checked == 2:
            continue
        K = s.shape[-1]
        R = s.numel // K
        # acc' = 0.9 acc + c U + wd w: the direction taken, to a few fp32 roundings of acc'
        got = (m3[sl].double() - 0.9 * m2[sl].double() - 5e-4 * w2[sl].double()).view(R, K).numpy()
        gs = [g[sl].view(R, K).numpy() for g in grads]
        want = _oracle_direction(gs, R, K, np.float64)
        d_ref, err = so.rel(_oracle_direction(gs, R, K, np.float32), want), so.rel(got, want)
        gn, un, c = st["tensors"][s.name]
        print(f"{s.name} {R}x{K}: graft {c:.4f} d_ref {d_ref:.3g} err {err:.3g}")
        assert err <= 4 * d_ref + 1e-6 and abs(c / (gn / un) - 1) < 1e-6
        checked += 1
    assert checked == 2
    assert torch.equal(eng.wbf, oo.expected_wbf(eng.seg_arr, eng.params.master, eng.wbf.numel()))


def test_engine_shampoo_imagenet_blocks_and_the_clip_refusal(gpu):
    eng = _engine(imagenet_spec(18, image_hw=64), gpu, optimizer="shampoo", shampoo_precond_every=1)
    convs = [s for s in eng.params.train_slots if s.kind == "conv"]
    nblocks = sum(-(-(s.numel // s.shape[-1]) // 64) * -(-s.shape[-1] // 64) for s in convs)
    assert max(s.shape[-1] for s in convs) > 64 and nblocks == len(eng.shampoo_blocks) > 1000
    eng.step()
    st = eng.shampoo_state()
    assert st["state_bytes"] == 4 * nblocks * 64 * 64 * 4 and st["t"] == 1
    assert bool(torch.isfinite(eng.params.master).all()) and bool(torch.isfinite(st["PL"]).all())
    assert len(st["tensors"]) == len(convs) and all(c > 0 for _, _, c in st["tensors"].values())
    with pytest.raises(ValueError, match="clip_grad_norm"):
        _engine(cifar_spec(8), gpu, optimizer="shampoo", clip_grad_norm=1.0)
