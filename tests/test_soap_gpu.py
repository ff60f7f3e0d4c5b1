"""SOAP on the device (csrc/soap.hip) against tests/soap_oracle.py: within 4 d_ref, the distance of the
oracle's own fp32 run from fp64; element-wise parts and the steps before the first refresh bit for bit."""
import numpy as np
import pytest
import torch

import shampoo_oracle as so
import soap_oracle as sp
from test_shampoo_gpu import _slot
from test_soap_cpu import SHAPES, SIZES, rand_orth, refresh_case
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.ops import functional as F
from distributed_tensorflow_resnet_amd.train.backends import GPUBackend
from distributed_tensorflow_resnet_amd.train.engine import Engine
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr
from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver

pytestmark = pytest.mark.gpu
B1, B2, EPS, LR, WD = 0.9, 0.999, 1e-8, 1e-3, 5e-4
f64 = lambda x: np.asarray(x, np.float64)   # noqa: E731
_state = lambda eng: (eng.params.master, eng.mom, eng.adam_v, eng.shampoo_state_buf)   # noqa: E731


# the last case: a rank-deficient statistic, G G^T with G 64 x 16
@pytest.mark.parametrize("n,basis,rank", [(n, "random", None) for n in SIZES]
                         + [(64, "identity", None), (64, "random", 16)])
def test_refresh_against_fp64(gpu, n, basis, rank):
    S, Q0 = refresh_case(n, basis, rank)
    stat, q0 = torch.full((3, 64, 64), 3.0), torch.full((3, 64, 64), -7.0)   # slot 1 of 3
    stat[1], q0[1] = torch.from_numpy(_slot(S)), torch.from_numpy(_slot(Q0))
    sd, qd, fail = stat.to(gpu), q0.to(gpu), torch.zeros(1, dtype=torch.int32, device=gpu)
    F.soap_refresh(sd[1:2], qd[1:2], [n], step=5, every=3, fail=fail)
    assert torch.equal(qd.cpu(), q0)                          # t % every != 0: nothing moves
    F.soap_refresh(sd[1:2], qd[1:2], [n], step=6, every=3, fail=fail)
    got = qd.cpu()
    assert torch.equal(sd.cpu(), stat) and torch.equal(got[0], q0[0]) and torch.equal(got[2], q0[2])
    assert not bool(got[1, n:].any()) and not bool(got[1, :, n:].any())   # the padding stays zero
    Q, A = got[1, :n, :n].numpy(), f64(S) @ Q0
    Q64, Q32 = sp.refresh(S, Q0), sp.refresh(S, Q0, np.float32)
    o_ref, o = sp.orth_err(Q32), sp.orth_err(Q)
    if rank:   # Q is not unique: what its first `rank` columns leave of range(S Q0), relative
        d_ref, d = (float(np.linalg.norm(A - p @ (p.T @ A)) / np.linalg.norm(A))
                    for p in (f64(Q32)[:, :rank], f64(Q)[:, :rank]))
    else:
        d_ref, d = float(np.abs(Q32 - Q64).max()), float(np.abs(Q - Q64).max())
        assert (np.diag(f64(Q).T @ A) >= 0).all()
    print(f"soap refresh n={n} {basis} rank={rank}: orth ref {o_ref:.3g} got {o:.3g} ratio "
          f"{o / o_ref:.3f}; Q d_ref {d_ref:.3g} err {d:.3g} ratio {d / d_ref:.3f}")
    assert int(fail.item()) == 0 and np.isfinite(Q).all() and o <= 4 * o_ref and d <= 4 * d_ref


@pytest.mark.parametrize("basis", ("random", "identity"))
@pytest.mark.parametrize("t", (1, 7))   # zero moments; moments as after some steps
@pytest.mark.parametrize("r,k", SHAPES)
def test_rotate_adam_against_fp64(gpu, r, k, t, basis):
    # guards around the block; the ragged block at an odd offset (the scalar loads)
    rng, lo, scale = np.random.default_rng(100 * r + k + t), 7 if r % 4 else 8, 0.5
    (g, m, v), body = (np.full(lo + r * k + 9, 3.0, np.float32) for _ in range(3)), slice(lo, lo + r * k)
    g[body] = rng.standard_normal(r * k)
    m[body], v[body] = (0.3 * rng.standard_normal(r * k), rng.uniform(0.01, 1.0, r * k)) if t > 1 else (0, 0)
    QL, QR = ((np.eye(s) if basis == "identity" else rand_orth(rng, s)).astype(np.float32)
              for s in (r, k))
    gd, md, vd, out = (torch.from_numpy(x).to(gpu) for x in (g, m, v, np.full_like(g, -7.0)))
    F.soap_rotate_adam(gd, md, vd, [(r, k)], [lo], torch.from_numpy(_slot(QL))[None].to(gpu),
                       torch.from_numpy(_slot(QR))[None].to(gpu), beta1=B1, beta2=B2, epsilon=EPS,
                       grad_scale=scale, out=out)
    got = [x.cpu().numpy() for x in (md, vd, out)]
    assert np.array_equal(gd.cpu().numpy(), g)                # grad is only read
    for x, guard in zip(got, (3.0, 3.0, -7.0)):               # nothing outside the block moves
        assert (x[:lo] == guard).all() and (x[lo + r * k:] == guard).all()
    G, M, V = ((x[body] * np.float32(s)).reshape(r, k) for x, s in ((g, scale), (m, 1), (v, 1)))
    if basis == "identity":   # adam.hip's element expressions, bit for bit
        c1, o1, c2, o2, e = sp.coefs(B1, B2, EPS)
        m1, v1 = so.fma32(c1, M, o1 * G), so.fma32(c2, V, o2 * (G * G))
        for x, want in zip(got, (m1, v1, m1 / (np.sqrt(v1) + e))):
            assert np.array_equal(x[body].reshape(r, k), want)
        return
    ref = (sp.rotate_adam(G, M, V, QL, QR, B1, B2, EPS, dt) for dt in (np.float64, np.float32))
    for name, x, w64, w32 in zip(("M'", "V'", "N"), got, *ref):
        d_ref, err = so.rel(w32, w64), so.rel(x[body].reshape(r, k), w64)
        print(f"soap rotate {r}x{k} t={t} {name}: d_ref {d_ref:.3g} err {err:.3g} ratio {err / d_ref:.3f}")
        assert err <= 4 * d_ref


# ------------------------------------------------------------------------------------ engine
def _engine(gpu, optimizer="shampoo", seed=0, **kw):
    soap = {"shampoo_variant": "soap", "shampoo_precond_every": 3, "shampoo_beta2": 0.95}
    kw, spec = {**(soap if optimizer == "shampoo" else {}), **kw}, cifar_spec(8)
    eng = Engine(spec, 8, weight_decay=WD, lr_schedule=constant_lr(LR), optimizer=optimizer,
                 device=gpu, input_mode="nhwc", seed=seed, adam_beta1=B1, adam_beta2=B2,
                 adam_epsilon=EPS, **kw)
    gen = torch.Generator().manual_seed(5)
    imgs = torch.randn(8, spec.image_h, spec.image_w, 3, generator=gen).to(torch.bfloat16).float()
    eng.set_batch(imgs.to(gpu), torch.randint(0, spec.num_classes, (8,), generator=gen).to(gpu))
    return eng


def _tensor_state(eng, st, ten, s):   # soap_oracle's state of conv slot s, fp64
    K, b0, sl = s.shape[-1], int(ten["block0"]), slice(s.offset, s.offset + s.numel)
    side = {"L": 0, "QL": 0, "R": 1, "QR": 1}
    bl = [[f64(st[key][b0 + i, :rk[side[key]], :rk[side[key]]].cpu()) for key in ("L", "R", "QL", "QR")]
          for i, (_, _, *rk) in enumerate(so.blocks(s.numel // K, K))]
    return {"blocks": bl, "M": f64(eng.mom[sl].view(-1, K).cpu()), "V": f64(eng.adam_v[sl].view(-1, K).cpu())}


@pytest.mark.parametrize("persist", (0, 1))
def test_engine_soap_step(gpu, monkeypatch, persist):
    monkeypatch.setenv("DTR_TUNE", f"persist={persist}")
    ref, eng = _engine(gpu, "adamw"), _engine(gpu)
    assert eng.persist == bool(persist) and not eng.opt_fused and "soap" in eng.opt_fused_reason
    assert [n for n in eng.plan.names() if "shampoo" in n or "soap" in n] == \
        ["shampoo_stats", "soap_refresh", "soap_rotate_adam", "soap_update_pack"]
    for step in (1, 2):   # the bases are the identity: adamw's step, bit for bit
        eng.step()
        ref.step()
        torch.cuda.synchronize()
        assert not eng.persist_error() and torch.equal(eng.grad, ref.grad)
        assert all(torch.equal(x, y) for x, y in zip(_state(eng)[:3], _state(ref))), step
        assert eng.adam_state() == ref.adam_state()
    eng.step()
    st, moved, worst = eng.shampoo_state(), 0, 0.0
    assert (st["t"], st["failed"], st["variant"]) == (3, 0, "soap") and "PL" not in st
    for blk in eng.shampoo_blocks:   # every basis against the oracle's fp32 refresh from the identity
        for key, stat, n in (("QL", "L", int(blk["r"])), ("QR", "R", int(blk["k"]))):
            Q, S = (st[x][int(blk["slot"]), :n, :n].cpu().numpy() for x in (key, stat))
            o_ref, o = sp.orth_err(sp.refresh(S, np.eye(n), np.float32)), sp.orth_err(Q)
            worst, moved = max(worst, o / o_ref), moved + (not np.array_equal(Q, np.eye(n)))
            assert o <= 4 * o_ref, (key, int(blk["slot"]), o, o_ref)
    print(f"engine persist={persist}: worst orthonormality ratio {worst:.3f}, {moved} bases moved")
    assert moved > 0
    # step 4, teacher-forced: the oracle's step from the engine's state and gradient
    convs = [s for s in eng.params.train_slots if s.kind == "conv"]
    before = [(s, _tensor_state(eng, st, ten, s), eng.params.master[s.offset:s.offset + s.numel].cpu())
              for s, ten in zip(convs, eng.shampoo_tensors)]
    eng.step()
    torch.cuda.synchronize()
    assert eng.adam_state()[0] == 4 and not eng.persist_error()
    grad, w4, hp = eng.grad.cpu(), eng.params.master.cpu(), (B1, B2, EPS, 0.95, 3)
    for s, state, w in before:
        K, sl = s.shape[-1], slice(s.offset, s.offset + s.numel)
        G, w = grad[sl].view(-1, K).numpy(), w.view(-1, K).numpy()   # (fp32 inputs for both runs)
        s32 = {"blocks": [[x.astype(np.float32) for x in bl] for bl in state["blocks"]],
               "M": state["M"].astype(np.float32), "V": state["V"].astype(np.float32)}
        w64 = sp.tensor_step(state, w, G, 4, LR, WD, hp)[1]
        w32 = sp.tensor_step(s32, w, G, 4, LR, WD, hp, np.float32)[1]
        d_ref, err = so.rel(w32 - w, w64 - w), so.rel(w4[sl].view(-1, K).numpy() - w, w64 - w)
        print(f"{s.name}: step d_ref {d_ref:.3g} err {err:.3g} ratio {err / d_ref:.3f}")
        assert err <= 4 * d_ref, s.name


def test_the_default_variant_records_no_soap_op_and_soap_resumes_bitwise(gpu, tmp_path):
    eng = _engine(gpu, shampoo_variant="roots")
    assert eng.shampoo_state()["variant"] == "roots" and eng.adam_state() is None \
        and not [n for n in eng.plan.names() if n.startswith("soap_")]
    straight, first = _engine(gpu), GPUBackend(_engine(gpu))
    for i in range(6):
        (straight.step(), first.step()) if i < 4 else straight.step()
    torch.cuda.synchronize()
    tensors = first.state_tensors()
    assert int(tensors["shampoo_variant"]) == 1 and tensors["conv2d/kernel/soap_QL"].shape == (1, 64, 64)
    assert "conv2d/kernel/Adam_1" in tensors and "conv2d/kernel/shampoo_PL" not in tensors
    second = GPUBackend(_engine(gpu, seed=9))
    second.load_state(Saver.restore(Saver(str(tmp_path)).save(tensors, 4)))
    assert second.global_step == 4 and int(second.engine.shampoo_start.item()) == 0
    for _ in range(2):
        second.step()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(_state(straight), _state(second.engine)))
    assert second.adam_state() == straight.adam_state() and straight.adam_state()[0] == 6
