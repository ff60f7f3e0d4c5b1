"""The LAMB kernels (csrc/lamb.hip: lamb_moments_norms, lamb_trust, lamb_update_pack) launched
directly on synthetic parameter tables, and the engine's adamw optimizer with adam_trust on, on
both plans, against the fp64 reference and the derived bounds of tests/lamb_oracle.py.  The
data is O(1) and bounded away from zero with v0 = x^2, so every term of the update is far above
its bound: a dropped or doubled term, swapped betas, a missing bias correction, decay in the
wrong mode, a norm over the wrong elements or a trust ratio on a skipped tensor fails."""
import gc

import numpy as np
import pytest
import torch

import adam_oracle as ao
import lamb_oracle as lmo
import optim_oracle as oo
from test_adam_gpu import CLIP_SLOT, COEFFS, COSINE
from test_adam_gpu import Table as AdamTable
from test_adam_gpu import _check_lr, _check_wbf, _sa, _st
from test_lars_gpu import SEVEN, TABLE_A, V, _dev
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule
from distributed_tensorflow_resnet_amd.train.layout import (LARS_CHUNK, adam_decay_table,
                                                              lars_tables)

pytestmark = pytest.mark.gpu

STEPS = [1, 2, 1000, 2 ** 31 + 5]


@pytest.fixture(scope="module")
def nat(gpu):
    import distributed_tensorflow_resnet_amd as dtr

    return dtr.native(required=True)


class Table(AdamTable):
    """test_adam_gpu's table with LARS's chunk tables for a trust skip ('vectors': every
    rank-1 tensor is not adapted)."""

    def lars(self, skip):
        sk = [skip == "vectors" and len(s) == 1 for s in self.shapes]
        lseg, blk = lars_tables(self.seg, sk)
        assert len(blk) == len(lmo.chunk_bounds(self.seg, LARS_CHUNK))
        return sk, _dev(lseg, self.gpu), torch.tensor(blk, dtype=torch.int32, device=self.gpu)


def _launch(nat, T, sched, gstep_v, start_v, coeff, mode, wd_seg, skip, clip_on):
    """The three launches + ohwi_pack on fresh buffers."""
    b1, b2, eps, _, gs = coeff
    gpu = T.gpu
    w, m, v, wbf = T.fresh()
    g0 = T.g.clone()
    sk, lseg_d, blk_d = T.lars(skip)
    gstep = torch.tensor([gstep_v], dtype=torch.int64, device=gpu)
    start = torch.tensor([start_v], dtype=torch.int64, device=gpu)
    lr_out = torch.full((1,), 7.0, device=gpu)
    out = torch.full((3,), float("nan"), device=gpu)
    part = torch.full((2 * blk_d.numel(),), float("nan"), dtype=torch.float64, device=gpu)
    lout = torch.full((3, T.nseg), float("nan"), device=gpu)
    clip = torch.tensor(CLIP_SLOT, device=gpu) if clip_on else None
    wd_d = torch.from_numpy(wd_seg).to(gpu)
    extra = () if sched.decay == "piecewise" else (sched.decay_args(),)
    lo = lout.data_ptr()
    # (with a clip slot the host grad_scale must be ignored: a wrong one is handed in)
    nat.lamb_moments_norms(w.data_ptr(), T.g.data_ptr(), m.data_ptr(), v.data_ptr(),
                           gstep.data_ptr(), start.data_ptr(), b1, b2, eps,
                           55.0 if clip_on else gs, clip.data_ptr() if clip_on else 0, mode,
                           T.segs_d.data_ptr(), lseg_d.data_ptr(), blk_d.data_ptr(), blk_d.numel(),
                           wd_d.data_ptr(), part.data_ptr(), _st())
    nat.lamb_trust(part.data_ptr(), lseg_d.data_ptr(), T.nseg, lo, lo + 4 * T.nseg,
                   lo + 8 * T.nseg, _st())
    nat.lamb_update_pack(w.data_ptr(), m.data_ptr(), v.data_ptr(), T.n, *_sa(sched),
                         gstep.data_ptr(), start.data_ptr(), b1, b2, eps, mode,
                         T.segs_d.data_ptr(), T.nseg, wd_d.data_ptr(), lo, wbf.data_ptr(),
                         lr_out.data_ptr(), out.data_ptr(), *extra, _st())
    nat.ohwi_pack(w.data_ptr(), T.segs_d.data_ptr(), T.tile0_d.data_ptr(), T.nseg, T.tiles,
                  wbf.data_ptr(), gstep.data_ptr(), _st())
    torch.cuda.synchronize()
    assert int(gstep) == gstep_v + 1 and int(start) == start_v
    assert torch.equal(T.g, g0)            # the gradient buffer is only read
    if clip_on:
        assert tuple(clip.tolist()) == tuple(oo.f32(c) for c in CLIP_SLOT)
    return dict(w=w, m=m, v=v, wbf=wbf, lr=float(lr_out), out=out.cpu().tolist(),
                part=part.cpu().tolist(), lout=lout.cpu().tolist(), skip=sk)


def _check_state(R, got, skip, what):
    """(trust, wn, un) slots against the reference's per-tensor values and bounds."""
    trust, wn, un = got
    for i, sk in enumerate(skip):
        assert abs(wn[i] - R["wn"][i]) <= lmo.NORM_REL * R["wn"][i], (what, "wn", i)
        assert abs(un[i] - R["un"][i]) <= R["Bun"][i], (what, "un", i, un[i], R["un"][i])
        assert abs(trust[i] - R["trust"][i]) <= R["TR"][i] * R["trust"][i], \
            (what, "trust", i, trust[i], R["trust"][i])
        if sk or R["wn"][i] == 0 or R["un"][i] == 0:
            assert trust[i] == 1.0, (what, i, trust[i])


def _check(T, res, t, coeff, mode, wd_seg, scale, what):
    b1, b2, eps, _, _ = coeff
    R = lmo.lamb_reference(T.w0, T.g, T.m0, T.v0, T.seg, wd_seg, res["skip"], res["lr"], t, b1, b2,
                           eps, scale, mode)
    worst = []
    for name, B in (("w", "Bw"), ("m", "Bm"), ("v", "Bv")):
        x = res[name]
        err = (x.double() - R[name]).abs()
        worst.append(float((err / R[B].clamp_min(1e-300)).max()))
        bad = (err > R[B]).nonzero().flatten()
        assert bad.numel() == 0, (what, name, bad[:8].tolist(), float(err.max()))
        assert bool(torch.isfinite(x).all()), (what, name)
    # every chunk's two partial sums
    chunks = lmo.chunk_bounds(T.seg, LARS_CHUNK)
    cw, cu, Bcw, Bcu = lmo.sums_reference(T.w0, R["u"], R["Eu"], chunks)
    part = res["part"]
    assert len(part) == 2 * len(chunks)
    for c in range(len(chunks)):
        assert abs(part[2 * c] - cw[c]) <= Bcw[c], (what, "part w", c, part[2 * c], cw[c])
        assert abs(part[2 * c + 1] - cu[c]) <= Bcu[c], (what, "part u", c, part[2 * c + 1], cu[c])
    _check_state(R, res["lout"], res["skip"], what)
    print(f"{what} max err/bound: w {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
    return R


def _check_slot(out, lr, t, coeff, what):
    """adam_update_pack's {lr, alpha, t} slot, which adam_state() keeps reading."""
    b1, b2 = coeff[:2]
    assert out[0] == lr and out[2] == float(np.float32(t)), (what, out)
    ref = ao.alpha_reference(lr, t, b1, b2)
    assert abs(out[1] - ref) <= ao.ulp(ref), (what, t, out[1], ref)


def _full(nat, T, sched, gstep_v, t, coeff, mode, decay_skip, skip, clip_on, what):
    wd_seg = T.wd_table(coeff[3], decay_skip)
    res = _launch(nat, T, sched, gstep_v, gstep_v - t + 1, coeff, mode, wd_seg, skip, clip_on)
    _check_lr(sched, gstep_v, res["lr"])
    _check_slot(res["out"], res["lr"], t, coeff, what)
    _check(T, res, t, coeff, mode, wd_seg, CLIP_SLOT[1] if clip_on else coeff[4], what)
    _check_wbf(T.seg, res["w"], res["wbf"], what)
    return res


def _same(a, b):
    for k in ("w", "m", "v", "wbf"):
        assert torch.equal(a[k], b[k]), k
    assert a["part"] == b["part"] and a["lout"] == b["lout"] and a["out"] == b["out"]


# ---------------------------------------------------------------- (a) synthetic tables
@pytest.fixture(scope="module")
def table_a(gpu):
    T = Table([s for s, _ in TABLE_A], gpu, seed=31)
    offs = [int(r["offset"]) for r in T.seg]
    assert {o % 4 for o in offs} == {0, 1, 2, 3} and T.n % 4 != 0
    return T


@pytest.mark.parametrize("clip_on", [False, True])
@pytest.mark.parametrize("skip", ["vectors", "none"])
@pytest.mark.parametrize("mode", ["decoupled", "l2"])
@pytest.mark.parametrize("ci", [0, 1])
def test_lamb_kernels_against_fp64(gpu, nat, table_a, ci, mode, skip, clip_on):
    T = table_a
    sk = T.lars(skip)[0]
    assert any(sk) == (skip == "vectors") and not all(sk)
    for k, t in enumerate(STEPS):
        # the schedule sees global_step, the bias correction global_step - start + 1
        sched = (SEVEN, COSINE)[k % 2]
        a = _full(nat, T, sched, t + 2, t, COEFFS[ci], mode, "vectors" if ci else "none", skip,
                  clip_on, f"table A {sched.decay} t={t}")
        for i, s in enumerate(sk):          # skipped tensors: exactly 1
            assert not s or a["lout"][0][i] == 1.0
    b = _full(nat, T, COSINE, STEPS[-1] + 2, STEPS[-1], COEFFS[ci], mode,
              "vectors" if ci else "none", skip, clip_on, "again")
    _same(a, b)                             # a second identical run: bit-equal


# ---------------------------------------------------------------- (b) zero norms
@pytest.mark.parametrize("mode", ["decoupled", "l2"])
def test_lamb_zero_norms_give_trust_one(gpu, nat, mode):
    zero = {1, 4, 7, 13}   # a conv, a 5-vector, the kpad > K conv, the 10-class dense
    T = Table([s for s, _ in TABLE_A], gpu, seed=32, zero=zero)
    o, k = int(T.seg[9]["offset"]), int(T.seg[9]["numel"])   # an all-zero tensor (w too)
    for x in (T.w0, T.g, T.m0, T.v0):
        x[o:o + k] = 0.0
    coeff = (0.9, 0.999, 1e-8, 0.0, 1.0)
    wd_seg = T.wd_table(0.0, "none")
    res = _launch(nat, T, SEVEN, 12, 0, coeff, mode, wd_seg, "none", False)
    z = T.zero_mask.clone()
    z[o:o + k] = True
    assert torch.equal(res["w"][z], T.w0[z])                 # bit for bit
    assert int(res["m"][z].count_nonzero()) == 0 and int(res["v"][z].count_nonzero()) == 0
    assert not torch.equal(res["w"][~z], T.w0[~z])
    trust, wn, un = res["lout"]
    for i in zero:
        assert un[i] == 0.0 and wn[i] > 0.0 and trust[i] == 1.0
    assert (wn[9], un[9], trust[9]) == (0.0, 0.0, 1.0)
    assert sum(t != 1.0 for t in trust) == T.nseg - len(zero) - 1
    _check(T, res, 13, coeff, mode, wd_seg, 1.0, f"zero blocks {mode}")
    _check_wbf(T.seg, res["w"], res["wbf"])


# ---------------------------------------------------------------- (c) neighbour safety
def test_lamb_chunks_stay_inside_their_tensor(gpu, nat):
    """Poison m and v in the first and last elements of every skipped tensor: large moments
    (|u| ~ 1e6 there).  They must come out as that tensor's own update -- its own decay, trust
    1 -- and the neighbours' sums, norms and trust ratios must not see them."""
    T = Table([s for s, _ in TABLE_A], gpu, seed=35)
    sk = T.lars("vectors")[0]
    n_poison = 0
    for r, s in zip(T.seg, sk):
        if s:
            o, k = int(r["offset"]), int(r["numel"])
            for e in {o, o + 1, o + k - 2, o + k - 1} & set(range(o, o + k)):
                T.m0[e] = 3e4 * (1 if e % 2 else -1)
                T.v0[e] = 1e-4
                n_poison += 1
    assert n_poison >= 12
    for mode in ("l2", "decoupled"):
        # (decay skip 'vectors': a skipped tensor's decay differs from its neighbours')
        _full(nat, T, SEVEN, 12, 3, COEFFS[1], mode, "vectors", "vectors", False,
              f"poisoned {mode}")


# ---------------------------------------------------------------- (d) table and grid extremes
def test_lamb_long_tables(gpu, nat):
    """More than 640 segments: the update reads the segment table from global memory."""
    specs = []
    for i in range(700):
        k = i % 4
        specs.append(("conv", 1, 1, 4, 8, 4, 8, True, True) if k == 0 else
                     ("conv", 3, 3, 4, 4, 8, 4, True, True) if k == 2 else
                     V(1 + i % 9) if k == 1 else V(1 + i % 5))
    T = Table(specs, gpu, seed=33)
    assert T.nseg == 700
    _full(nat, T, SEVEN, 12, 5, COEFFS[0], "decoupled", "vectors", "vectors", False, "700 segments")
    _full(nat, T, COSINE, 12, 5, COEFFS[1], "l2", "vectors", "none", True, "700 segments l2")


def test_lamb_grid_stride(gpu, nat):
    """More float4s than 4096 x 256 threads: the update loop's second trip, tensors of many
    chunks, and segment ends off the multiples of 4."""
    n = 4 * 256 * 4096 + 4099
    specs, off = [], 0
    special = {0: ("conv", 1, 1, 333, 1001, 333, 1001, False, True),
               3: ("conv", 1, 1, 129, 515, 129, 520, False, True)}
    for i in range(8):
        s = special.get(i)
        if s is None:
            size = 500003 + 1000 * i
            while (off + size) % 4 == 0:
                size += 1
            s = V(size)
        specs.append(s)
        off += s[1] * s[2] * s[3] * s[4]
    specs.append(V(n - off))
    T = Table(specs, gpu, seed=34)
    assert T.n == n and (n + 3) // 4 > 4096 * 256
    _full(nat, T, cifar_lr_schedule(), 7, 3, COEFFS[1], "decoupled", "vectors", "none", False,
          "grid-stride")


# ---------------------------------------------------------------- (e) the bindings' checks
def test_lamb_bindings_reject_unaligned_buffers_and_bad_coefficients(gpu, nat, table_a):
    T = table_a
    w, m, v, wbf = T.fresh()
    g = T.g.clone()
    _, lseg_d, blk_d = T.lars("vectors")
    gstep = torch.zeros(1, dtype=torch.int64, device=gpu)
    start = torch.zeros(1, dtype=torch.int64, device=gpu)
    wd_d = torch.from_numpy(T.wd_table(0.1, "none")).to(gpu)
    part = torch.zeros(2 * blk_d.numel(), dtype=torch.float64, device=gpu)
    lout = torch.ones(3, T.nseg, device=gpu)

    def norms(ptrs, b1=0.9, b2=0.999, eps=1e-8, mode="decoupled"):
        nat.lamb_moments_norms(*ptrs, gstep.data_ptr(), start.data_ptr(), b1, b2, eps, 1.0, 0,
                               mode, T.segs_d.data_ptr(), lseg_d.data_ptr(), blk_d.data_ptr(),
                               blk_d.numel(), wd_d.data_ptr(), part.data_ptr(), _st())

    def update(ptrs, b1=0.9, b2=0.999, eps=1e-8, mode="decoupled"):
        nat.lamb_update_pack(*ptrs, T.n - 4, *_sa(SEVEN), gstep.data_ptr(), start.data_ptr(), b1,
                             b2, eps, mode, T.segs_d.data_ptr(), T.nseg, wd_d.data_ptr(),
                             lout.data_ptr(), wbf.data_ptr(), 0, 0, _st())

    for fn, base in ((norms, [w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()]),
                     (update, [w.data_ptr(), m.data_ptr(), v.data_ptr()])):
        for i in range(len(base)):
            ptrs = list(base)
            ptrs[i] += 4
            with pytest.raises(ValueError):
                fn(ptrs)
        for kw in (dict(b1=1.0), dict(b1=-0.1), dict(b2=1.5), dict(b2=-0.1), dict(eps=0.0),
                   dict(eps=-1e-8), dict(eps=float("nan")), dict(eps=float("inf")),
                   dict(mode="adamw")):
            with pytest.raises(ValueError):
                fn(base, **kw)
    torch.cuda.synchronize()
    assert torch.equal(w, T.w0) and torch.equal(m, T.m0) and torch.equal(v, T.v0)
    assert int(wbf.count_nonzero()) == 0 and int(part.count_nonzero()) == 0


# ---------------------------------------------------------------- (f) engine
WD = 5e-4
ADAM = dict(adam_beta1=0.9, adam_beta2=0.99, adam_epsilon=1e-6)
N = 8


def _engine(spec, gpu, optimizer="adamw", seed=0, trust="on", n=N, **kw):
    if optimizer == "adamw":
        kw = {**ADAM, "adam_trust": trust, **kw}
    eng = Engine(spec, n, weight_decay=WD, lr_schedule=cifar_lr_schedule(), optimizer=optimizer,
                 device=gpu, input_mode="nhwc", seed=seed, **kw)
    gen = torch.Generator().manual_seed(5)
    imgs = torch.randn(n, spec.image_h, spec.image_w, 3, generator=gen).to(torch.bfloat16).float()
    eng.set_batch(imgs.to(gpu), torch.randint(0, spec.num_classes, (n,), generator=gen).to(gpu))
    return eng


def _check_engine_step(eng, w0, m0, v0, step, t, what):
    """The engine's own gradient through lamb_reference against its master, moments,
    lamb_state() and adam_state(): the optimizer alone, without the convolutions' bf16 noise."""
    n = eng.params.n_train
    lr = oo.f32(oo.lr_reference(eng.sched, step))
    assert eng.metrics()["lr"] == lr
    scale = 1.0
    if eng.clip_grad_norm > 0:
        norm, scale = eng.clip_state()
        assert scale < 1.0, (norm, scale)
    wd_seg = adam_decay_table([s.shape for s in eng.params.train_slots], eng.wd,
                              eng.adam_decay_skip)
    skip = [eng.adam_trust_skip == "vectors" and len(s.shape) == 1 for s in eng.params.train_slots]
    assert skip == eng.lars_skipped
    R = lmo.lamb_reference(w0, eng.grad, m0, v0, eng.seg_arr, wd_seg, skip, lr, t, eng.adam_beta1,
                           eng.adam_beta2, eng.adam_epsilon, scale, eng.adam_decay)
    worst = []
    for x, name, B in ((eng.params.master[:n], "w", "Bw"), (eng.mom[:n], "m", "Bm"),
                       (eng.adam_v[:n], "v", "Bv")):
        err = (x.double() - R[name]).abs()
        worst.append(float((err / R[B].clamp_min(1e-300)).max()))
        assert bool((err <= R[B]).all()), (what, step, name, float(err.max()))
    print(f"{what} step {step}: max err/bound master {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
    st = eng.lamb_state()
    assert list(st) == eng.seg_names
    wn, un, trust = (list(x) for x in zip(*st.values()))
    _check_state(R, (trust, wn, un), skip, what)
    sm = eng.lamb_summary()
    adapted = sorted(tr for tr, sk in zip(trust, skip) if not sk)
    assert sm == {"lamb_trust_min": adapted[0], "lamb_trust_median": adapted[len(adapted) // 2],
                  "lamb_trust_max": adapted[-1]}
    t_k, alpha = eng.adam_state()
    ref = ao.alpha_reference(lr, t, eng.adam_beta1, eng.adam_beta2)
    assert t_k == t and abs(alpha - ref) <= ao.ulp(ref), (what, t_k, alpha, ref)
    assert torch.equal(eng.wbf, oo.expected_wbf(eng.seg_arr, eng.params.master, eng.wbf.numel()))


def _run_steps(eng, steps, what):
    assert eng.lamb_state() is None and eng.lamb_summary() is None   # before the first step
    for step in range(steps):
        w0, m0, v0 = eng.params.master.clone(), eng.mom.clone(), eng.adam_v.clone()
        assert int(eng.gstep.item()) == step
        eng.step()
        torch.cuda.synchronize()
        assert not eng.persist_error()
        _check_engine_step(eng, w0, m0, v0, step, step + 1, what)
    assert int(eng.gstep.item()) == steps


OPT_OPS = ("grad_sqnorm", "clip_scale", "adam_update_pack", "ohwi_pack", "sgd_update_pack",
           "sgd_clip_update_pack", "sgd_tiles", "lars_update_pack", "lars_norms", "lars_trust",
           "lamb_moments_norms", "lamb_trust", "lamb_update_pack", "ema_update")
LAMB_OPS = ["lamb_moments_norms", "lamb_trust", "lamb_update_pack", "ohwi_pack"]


@pytest.mark.parametrize("clip", [0.0, 0.05])
@pytest.mark.parametrize("persist", [0, 1])
def test_engine_lamb_step(gpu, monkeypatch, persist, clip):
    monkeypatch.setenv("DTR_TUNE", f"persist={persist}")
    eng = _engine(cifar_spec(8), gpu, clip_grad_norm=clip,
                  adam_decay="l2" if clip else "decoupled",
                  adam_decay_skip="vectors" if clip else "none",
                  adam_trust_skip="none" if clip else "vectors", ema_decay=0.99 if clip else 0.0)
    assert eng.persist == bool(persist) and eng.adam and eng.lamb
    assert not eng.opt_fused and "adam_trust" in eng.opt_fused_reason
    names = eng.plan.names()
    a, b = eng.seg["opt"]
    assert [n for n in names[a:b] if n in OPT_OPS] == \
        (["grad_sqnorm", "clip_scale"] if clip else []) + LAMB_OPS + (["ema_update"] if clip else [])
    _run_steps(eng, 2, f"cifar8 persist={persist} clip={clip}")   # step 1: non-zero moments


def test_engine_lamb_imagenet_s2d_stem(gpu, monkeypatch):
    monkeypatch.setenv("DTR_TUNE", "persist=0")
    eng = _engine(imagenet_spec(18, image_hw=64), gpu)
    assert eng.stem_s2d
    _run_steps(eng, 2, "imagenet18 s2d")


@pytest.mark.parametrize("dtype,persist", [("fp32", "0"), ("bf16", "1")])
def test_engine_lamb_takes_the_exchanged_gradient(gpu, monkeypatch, dtype, persist):
    """comm = the doubling loopback: the update is formed from the all-reduced gradient
    (2x the local one; bf16: rebuilt from the bf16 exchange)."""
    import distributed_tensorflow_resnet_amd as dtr

    monkeypatch.setenv("DTR_TUNE", f"persist={persist}")
    spec = cifar_spec(8)
    ref = _engine(spec, gpu, optimizer="mom")
    eng = _engine(spec, gpu, comm=dtr.native().Comm.loopback(2.0), bucket_mb=0.05,
                  allreduce_dtype=dtype)
    assert eng.persist == (persist == "1") and not eng.opt_fused
    names = eng.plan.names()
    a, b = eng.seg["opt"]
    assert [n for n in names[a:b] if n in OPT_OPS] == LAMB_OPS
    assert torch.equal(eng.params.master, ref.params.master)
    w0, m0, v0 = eng.params.master.clone(), eng.mom.clone(), eng.adam_v.clone()
    ref.step()
    eng.step()
    torch.cuda.synchronize()
    base = ref.grad if dtype == "fp32" else ref.grad.to(torch.bfloat16).float()
    assert torch.equal(eng.grad, 2 * base)
    _check_engine_step(eng, w0, m0, v0, 0, 1, f"loopback {dtype}")


def _state(eng):
    return [eng.params.master.clone(), eng.mom.clone(), eng.adam_v.clone(),
            eng.params.stats.clone(), eng.wbf.clone(), eng.gstep.clone(), eng.adam_start.clone()]


def test_engine_lamb_same_seed_engines_agree_bitwise(gpu):
    a, b = _engine(cifar_spec(8), gpu), _engine(cifar_spec(8), gpu)
    for _ in range(5):
        a.step()
        b.step()
    torch.cuda.synchronize()
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    assert a.lamb_state() == b.lamb_state() and a.adam_state() == b.adam_state()
    assert a.adam_state()[0] == 5
    plain = _engine(cifar_spec(8), gpu, trust="off")     # and trust changes the run
    plain.step()
    assert not torch.equal(plain.params.master, a.params.master)


def test_engine_lamb_resume_is_bitwise(gpu, tmp_path):
    from distributed_tensorflow_resnet_amd.train.backends import GPUBackend
    from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver

    straight = _engine(cifar_spec(8), gpu)
    for _ in range(4):
        straight.step()
    first = GPUBackend(_engine(cifar_spec(8), gpu))
    for _ in range(2):
        first.step()
    torch.cuda.synchronize()
    tensors = first.state_tensors()
    plain = GPUBackend(_engine(cifar_spec(8), gpu, trust="off"))
    assert set(tensors) == set(plain.state_tensors())     # the trust ratio has no state
    assert int(tensors["adam_start_step"]) == 0 and "conv2d/kernel/Adam_1" in tensors
    prefix = Saver(str(tmp_path)).save(tensors, 2)
    second = GPUBackend(_engine(cifar_spec(8), gpu, seed=9))
    second.load_state(Saver.restore(prefix))
    assert second.global_step == 2 and int(second.engine.adam_start.item()) == 0
    for _ in range(2):
        second.step()
    torch.cuda.synchronize()
    for x, y in zip(_state(straight), _state(second.engine)):
        assert torch.equal(x, y)
    assert second.lamb_state() == straight.lamb_state()
    assert second.adam_state() == straight.adam_state()


def test_engine_lamb_and_adamw_checkpoints_interchange(gpu):
    from distributed_tensorflow_resnet_amd.train.backends import GPUBackend

    plain = GPUBackend(_engine(cifar_spec(8), gpu, trust="off"))
    for _ in range(2):
        plain.step()
    torch.cuda.synchronize()
    be = GPUBackend(_engine(cifar_spec(8), gpu, seed=9))
    be.step()
    be.load_state(plain.state_tensors())                  # trust on <- a trust-off checkpoint
    eng = be.engine
    assert be.global_step == 2 and int(eng.adam_start.item()) == 0
    for x, y in zip(_state(eng)[:3], _state(plain.engine)[:3]):
        assert torch.equal(x, y)
    w0, m0, v0 = eng.params.master.clone(), eng.mom.clone(), eng.adam_v.clone()
    be.step()
    torch.cuda.synchronize()
    _check_engine_step(eng, w0, m0, v0, 2, 3, "after a trust-off checkpoint")
    back = GPUBackend(_engine(cifar_spec(8), gpu, seed=7, trust="off"))
    back.load_state(be.state_tensors())                   # and the reverse
    assert back.global_step == 3 and back.lamb_state() is None
    for x, y in zip(_state(back.engine)[:3], _state(eng)[:3]):
        assert torch.equal(x, y)
    back.step()
    torch.cuda.synchronize()
    assert back.adam_state()[0] == 4
    # a mom checkpoint: fresh moments and a bias correction that restarts, as for adamw
    mom = GPUBackend(_engine(cifar_spec(8), gpu, optimizer="mom"))
    for _ in range(3):
        mom.step()
    torch.cuda.synchronize()
    be.load_state(mom.state_tensors())
    assert int(eng.adam_start.item()) == 3 and int(eng.mom.count_nonzero()) == 0
    w0, m0, v0 = eng.params.master.clone(), eng.mom.clone(), eng.adam_v.clone()
    be.step()
    torch.cuda.synchronize()
    _check_engine_step(eng, w0, m0, v0, 3, 1, "after a mom checkpoint")


def test_engine_lamb_graph_replay_equals_eager(gpu):
    spec = cifar_spec(8)
    eager = _engine(spec, gpu, use_graph=True)   # the same recording,
    graph = _engine(spec, gpu, use_graph=True)   # stepped eagerly / replayed
    for _ in range(6):
        eager.step()
    done = graph.capture(warmup=2)
    assert graph.graph is not None
    for _ in range(6 - done):
        graph.step()
    torch.cuda.synchronize()
    assert int(graph.gstep.item()) == 6
    for x, y in zip(_state(eager), _state(graph)):
        assert torch.equal(x, y)
    assert graph.lamb_state() == eager.lamb_state()
    assert graph.adam_state() == eager.adam_state() and graph.adam_state()[0] == 6


# ---------------------------------------------------------------- (g) trust off changes nothing
class _PlanSpy:
    """A Plan that also keeps (method, arguments) of every call recorded into it."""

    def __init__(self, plan, calls):
        self.__dict__["_plan"], self.__dict__["_calls"] = plan, calls

    def __getattr__(self, name):
        fn = getattr(self._plan, name)
        if not callable(fn):
            return fn

        def call(*a, **k):
            self._calls.append((name, a, tuple(sorted(k.items()))))
            return fn(*a, **k)
        return call


def _recorded_calls(gpu, monkeypatch, **kw):
    """An engine built over a spying Plan: its recorded calls with every device address
    replaced by (the engine tensor it points into, offset)."""
    import distributed_tensorflow_resnet_amd as dtr

    nat, calls = dtr.native(required=True), []
    real = nat.Plan
    with monkeypatch.context() as mp:
        mp.setattr(nat, "Plan", lambda: _PlanSpy(real(), calls))
        gc.collect()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(gpu)
        eng = _engine(cifar_spec(8), gpu, **kw)
        torch.cuda.synchronize()
        grown = torch.cuda.memory_allocated(gpu) - before
    tensors = {k: v for k, v in vars(eng).items() if torch.is_tensor(v) and v.is_cuda}
    tensors.update({"master": eng.params.master, "stats": eng.params.stats})
    spans = sorted((v.data_ptr(), v.data_ptr() + max(v.numel() * v.element_size(), 1), k)
                   for k, v in tensors.items())

    def norm(x):
        if isinstance(x, int) and x >= 1 << 32:
            for a, b, k in spans:
                if a <= x < b:
                    return (k, x - a)
            return "device address"
        if isinstance(x, (list, tuple)):
            return tuple(norm(y) for y in x)
        return x if isinstance(x, (int, float, str, bool, type(None))) else type(x).__name__

    ops = [(n, norm(a), norm(k)) for n, a, k in calls
           if n not in ("run", "size", "names", "op_kinds", "op_streams", "op_events")]
    return eng, ops, grown


@pytest.mark.parametrize("persist", [0, 1])
def test_trust_off_records_adamw_plan(gpu, monkeypatch, persist):
    monkeypatch.setenv("DTR_TUNE", f"persist={persist}")
    base, ops0, grown0 = _recorded_calls(gpu, monkeypatch, trust="off")
    off, ops1, grown1 = _recorded_calls(gpu, monkeypatch, trust="off", adam_trust_skip="none")
    on, ops2, grown2 = _recorded_calls(gpu, monkeypatch, trust="on")
    assert len(ops0) > 10 and any(n == "adam_update_pack" for n, *_ in ops0)
    assert ops1 == ops0 and off.plan.names() == base.plan.names()
    assert grown1 == grown0 and grown2 > grown0           # no new allocation
    for eng in (base, off):
        assert not eng.lamb and eng.lamb_state() is None and eng.lamb_summary() is None
        assert not hasattr(eng, "lars_segs") and not hasattr(eng, "lars_part")
        assert "adam_trust" not in eng.opt_fused_reason and "adamw" in eng.opt_fused_reason
        assert not any(n.startswith("lamb_") for n in eng.plan.names())
    assert [n for n, *_ in ops2 if n.startswith(("lamb_", "adam_"))] == LAMB_OPS[:3]
    off.step()
    torch.cuda.synchronize()
    assert off.lamb_state() is None and off.adam_state()[0] == 1


def test_mom_engine_is_unchanged(gpu, monkeypatch):
    monkeypatch.setenv("DTR_TUNE", "persist=1")
    eng = _engine(cifar_spec(8), gpu, optimizer="mom")
    other = _engine(cifar_spec(8), gpu, optimizer="mom", adam_trust="off", adam_trust_skip="none")
    assert not eng.adam and not eng.lamb and eng.lamb_state() is None
    assert eng.adam_v is None and not hasattr(eng, "lars_segs")
    assert eng.opt_fused and eng.opt_fused_reason == "" and eng.persist
    assert eng.plan.names() == other.plan.names()
    assert not any(n.startswith("lamb_") for n in eng.plan.names())
    eng.step()
    torch.cuda.synchronize()
    assert eng.lamb_state() is None and eng.lamb_summary() is None
    for opt in ("mom", "sgd", "lars"):
        with pytest.raises(ValueError):
            _engine(cifar_spec(8), gpu, optimizer=opt, adam_trust="on")
    with pytest.raises(ValueError):
        _engine(cifar_spec(8), gpu, adam_trust_skip="biases")
