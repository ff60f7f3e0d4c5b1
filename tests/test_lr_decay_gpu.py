"""--lr_decay cosine | poly on the device.  Kernel level: each of the four ops that evaluate
the schedule (sgd_update_pack, sgd_tiles, lars_update_pack, sgd_clip_update_pack) recorded in
a Plan with the decay overload, global_step set to every step of tests/lr_decay_oracle.py's
cases: lr_out within one fp32 ulp of the mpmath oracle (exact in warm-up and from D on), the
updated weights and momentum within optim_oracle's bound B of the fp64 step at the oracle's
rate.  Engine level: the persistent step keeps its one-launch optimizer, metrics()["lr"]
follows the oracle, same-seed runs agree bit for bit; the per-layer plan and LARS likewise;
and with the flags' defaults nothing moves."""
import numpy as np
import pytest
import torch

import lr_decay_oracle as lo
import optim_oracle as oo
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.train.engine import Engine
from distributed_tensorflow_resnet_amd.train.schedule import (cifar_lr_schedule,
                                                                decay_lr_schedule,
                                                                schedule_from_flags)
from distributed_tensorflow_resnet_amd.utils.flags import build_parser

pytestmark = pytest.mark.gpu

CASES = lo.cases()
MOMENTUM, WD = 0.9, 2e-4
SCALE = 0.5                                    # the clip slot's scale / the host grad_scale
TRUST = (0.5, 2.0, 1.0)                        # powers of two: lr * trust is exact


def V(n):
    return ("vec", 1, 1, 1, n, 1, 1, False, False)


# ~1000 floats in 3 segments; the first ends at 333, inside a float4 (the straddling path)
FLAT = [V(333), ("conv", 1, 1, 16, 32, 16, 32, True, True), V(150)]
# the smallest tiled work table of the optimizer tests: one 3x3 16-to-16 weight and a vector
TILED = [("conv", 3, 3, 16, 16, 16, 16, True, True), V(16)]
OPS = ("sgd_update_pack", "sgd_tiles", "lars_update_pack", "sgd_clip_update_pack")


@pytest.fixture(scope="module")
def nat(gpu):
    import distributed_tensorflow_resnet_amd as dtr

    n = dtr.native(required=True)
    assert oo.SEG_DTYPE.itemsize == n.param_seg_bytes()
    assert oo.OPTW_DTYPE.itemsize == n.opt_work_bytes()
    return n


def _dev(arr, gpu):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).to(gpu)


class Table:
    """A synthetic parameter table and its (unchanging) random state."""

    def __init__(self, specs, gpu, seed):
        self.seg, self.names, self.n, self.bf_total, _, _ = oo.build_seg_table(specs)
        self.gpu, self.nseg = gpu, len(self.seg)
        self.segs_d = _dev(self.seg, gpu)
        gen = torch.Generator().manual_seed(seed)

        def rand():   # O(1) values bounded away from zero
            x = torch.randn(self.n, generator=gen)
            return (x + 0.25 * torch.sign(x)).to(gpu)

        self.w0, self.g, self.m0 = rand(), rand(), rand()
        work, blk = oo.build_opt_work(self.seg, self.names)
        self.work_d, self.nblk = _dev(work, gpu), len(blk)
        self.blk_d = torch.tensor(blk, dtype=torch.int32, device=gpu)
        # per-element trust of lars_update_pack (segment s: TRUST[s % 3])
        self.trust = torch.tensor([TRUST[i % 3] for i in range(self.nseg)], device=gpu)
        self.trust_el = torch.cat([torch.full((int(r["numel"]),), TRUST[i % 3])
                                   for i, r in enumerate(self.seg)]).to(gpu)
        self.clip = torch.tensor([1.0, SCALE], device=gpu)


@pytest.fixture(scope="module")
def flat(gpu):
    T = Table(FLAT, gpu, seed=21)
    assert T.n == 995 and int(T.seg[1]["offset"]) % 4 == 1
    return T


@pytest.fixture(scope="module")
def tiled(gpu):
    T = Table(TILED, gpu, seed=22)
    assert T.nblk == 4      # 144 rows = 64 + 64 + 16, and the vector's one chunk
    return T


def _run_steps(nat, op, T, sched, steps):
    """One Plan: for step i its own copies of (w, mom, wbf), global_step and lr_out slot,
    one launch of `op` each.  Returns (w [k][n], mom [k][n], lr_out [k], gstep [k])."""
    k, gpu = len(steps), T.gpu
    pad = lambda n: -(-n // 64) * 64   # noqa: E731  (every row 16-byte aligned, as the engine's)
    w = torch.zeros(k, pad(T.n), device=gpu)[:, :T.n]
    mom = torch.zeros(k, pad(T.n), device=gpu)[:, :T.n]
    w.copy_(T.w0[None].expand(k, -1))
    mom.copy_(T.m0[None].expand(k, -1))
    wbf = torch.zeros(k, pad(T.bf_total), dtype=torch.bfloat16, device=gpu)[:, :T.bf_total]
    gstep = torch.tensor(steps, dtype=torch.int64, device=gpu)
    lr_out = torch.full((k,), -1.0, device=gpu)
    g = T.g.clone()
    sa, da = sched.launch_args(), sched.decay_args()
    plan = nat.Plan()
    for i in range(k):
        a = (w[i].data_ptr(), g.data_ptr(), mom[i].data_ptr())
        gs, lr, bf = gstep.data_ptr() + 8 * i, lr_out.data_ptr() + 4 * i, wbf[i].data_ptr()
        if op == "sgd_update_pack":
            plan.sgd_update_pack(*a, T.n, *sa, gs, MOMENTUM, WD, SCALE, 1, T.segs_d.data_ptr(),
                                 T.nseg, bf, lr, 1, da)
        elif op == "sgd_tiles":   # (a null ticket: no global_step += 1)
            plan.sgd_tiles(*a, *sa, gs, MOMENTUM, WD, SCALE, 1, T.segs_d.data_ptr(),
                           T.work_d.data_ptr(), T.blk_d.data_ptr(), T.nblk, bf, lr, 0, 0, 0, 0, da)
        elif op == "lars_update_pack":
            plan.lars_update_pack(*a, T.n, *sa, gs, MOMENTUM, WD, SCALE, T.segs_d.data_ptr(),
                                  T.nseg, T.trust.data_ptr(), bf, lr, da)
        else:
            plan.sgd_clip_update_pack(*a, T.n, *sa, gs, MOMENTUM, WD, T.clip.data_ptr(), 1,
                                      T.segs_d.data_ptr(), T.nseg, bf, lr, da)
    assert plan.size() == k
    plan.run(0, k, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(g, T.g)
    return w, mom, lr_out.tolist(), gstep.tolist(), wbf


def _check(op, T, sched, steps, out, what):
    w, mom, lrs, gsteps, wbf = out
    assert gsteps == list(steps)               # the step is only read
    refs = []
    for s, got in zip(steps, lrs):
        ref = lo.check_rate(sched, s, got, what)
        print(f"{what} step {s}: device {got!r} oracle {ref!r} "
              f"({(got - ref) / lo.ulp(ref or 1.0):+.0f} ulp)")
        refs.append(ref)
    # the fp64 SGD step at the oracle's rate, all steps at once ([k][n])
    lr = torch.tensor(refs, dtype=torch.float64, device=T.gpu)[:, None]
    if op == "lars_update_pack":
        lr = lr * T.trust_el.double()[None, :]
    k = len(steps)
    w_ref, m_ref, B = oo.sgd_reference(T.w0.repeat(k, 1), T.g.repeat(k, 1), T.m0.repeat(k, 1), lr,
                                       oo.f32(MOMENTUM), oo.f32(WD), oo.f32(SCALE), True)
    ew, em = (w.double() - w_ref).abs(), (mom.double() - m_ref).abs()
    print(f"{what}: max err/B w {float((ew / B).max()):.3f} mom {float((em / B).max()):.3f}")
    assert bool((ew <= B).all()), (what, "w", float((ew / B).max()))
    assert bool((em <= B).all()), (what, "mom", float((em / B).max()))
    seg = T.seg
    if op != "sgd_tiles":   # the pack kernels write the HWIO copy; the OHWI one is ohwi_pack's
        seg = T.seg.copy()
        seg["bf_ohwi"] = -1
    for i in range(k):
        assert torch.equal(wbf[i], oo.expected_wbf(seg, w[i], T.bf_total)), (what, steps[i])


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_rate_and_update(gpu, nat, flat, tiled, op, name):
    sched, steps = CASES[name]
    T = tiled if op == "sgd_tiles" else flat
    _check(op, T, sched, steps, _run_steps(nat, op, T, sched, steps), f"{op} {name}")


@pytest.mark.parametrize("op", [o for o in OPS if o != "sgd_tiles"])
def test_kernel_long_segment_table(gpu, nat, op):
    """nseg > SEG_LDS_MAX (640): no LDS table, so the barrier that publishes the rate is
    the path's own."""
    T = Table([V(1 + i % 5) for i in range(641)], gpu, seed=23)
    assert T.nseg == 641 and T.n % 4 != 0
    sched, _ = CASES["cosine_2_7"]
    steps = [0, 2, 4, 6, 7, 8]
    _check(op, T, sched, steps, _run_steps(nat, op, T, sched, steps), f"{op} 641 segments")


def test_piecewise_kind_through_the_overload_is_the_old_launch(gpu, nat, flat):
    """("piecewise", ...) as the trailing argument: bit for bit the launch without it."""
    T, sched = flat, cifar_lr_schedule()
    outs = []
    for extra in ((), (sched.decay_args(),)):
        w, mom = T.w0.clone(), T.m0.clone()
        wbf = torch.zeros(T.bf_total, dtype=torch.bfloat16, device=gpu)
        gstep = torch.tensor([40002], dtype=torch.int64, device=gpu)
        lr_out = torch.zeros(1, device=gpu)
        nat.sgd_update_pack(w.data_ptr(), T.g.data_ptr(), mom.data_ptr(), T.n,
                            *sched.launch_args(), gstep.data_ptr(), MOMENTUM, WD, 1.0, 1,
                            T.segs_d.data_ptr(), T.nseg, wbf.data_ptr(), lr_out.data_ptr(), 1,
                            *extra, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append((w, mom, wbf, lr_out))
    assert float(outs[0][3]) == oo.f32(0.01)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("decay", [("cosine", 2, 0.0, 2.0), ("poly", 7, 0.0, 0.0),
                                   ("poly", 7, 0.0, float("nan")), ("cosine", 7, -1.0, 2.0),
                                   ("cosine", 7, float("inf"), 2.0), ("linear", 7, 0.0, 2.0)])
def test_overloads_check_the_constraints(gpu, nat, flat, decay):
    """make_sched: D > W >= 0, power > 0, rates finite and >= 0 -- nothing is launched."""
    T = flat
    w, mom = T.w0.clone(), T.m0.clone()
    wbf = torch.zeros(T.bf_total, dtype=torch.bfloat16, device=gpu)
    gstep = torch.zeros(1, dtype=torch.int64, device=gpu)
    sa = (0.01, 2, 0.01, 0.1, [], [0.1])
    a = (w.data_ptr(), T.g.data_ptr(), mom.data_ptr())
    plan = nat.Plan()
    with pytest.raises(ValueError):
        plan.sgd_update_pack(*a, T.n, *sa, gstep.data_ptr(), MOMENTUM, WD, 1.0, 1,
                             T.segs_d.data_ptr(), T.nseg, wbf.data_ptr(), 0, 1, decay)
    with pytest.raises(ValueError):
        plan.lars_update_pack(*a, T.n, *sa, gstep.data_ptr(), MOMENTUM, WD, 1.0,
                              T.segs_d.data_ptr(), T.nseg, T.trust.data_ptr(), wbf.data_ptr(), 0,
                              decay)
    with pytest.raises(ValueError):
        plan.sgd_clip_update_pack(*a, T.n, *sa, gstep.data_ptr(), MOMENTUM, WD, T.clip.data_ptr(),
                                  1, T.segs_d.data_ptr(), T.nseg, wbf.data_ptr(), 0, decay)
    with pytest.raises(ValueError):
        plan.sgd_tiles(*a, *sa, gstep.data_ptr(), MOMENTUM, WD, 1.0, 1, T.segs_d.data_ptr(),
                       T.work_d.data_ptr(), T.blk_d.data_ptr(), T.nblk, wbf.data_ptr(), 0, 0, 0, 0,
                       0, decay)
    assert plan.size() == 0


# ---------------------------------------------------------------- engine
ENG_SCHED = decay_lr_schedule("cosine", 0.1, 5, warm_steps=2)


def _engine(gpu, monkeypatch, sched, tune="", N=8, **kw):
    monkeypatch.setenv("DTR_TUNE", tune)
    spec = cifar_spec(8)
    eng = Engine(spec, N, weight_decay=5e-4, lr_schedule=sched, device=gpu, input_mode="nhwc",
                 seed=3, **kw)
    gen = torch.Generator().manual_seed(5)
    imgs = torch.randn(N, spec.image_h, spec.image_w, 3, generator=gen).to(torch.bfloat16).float()
    eng.set_batch(imgs.to(gpu), torch.randint(0, spec.num_classes, (N,), generator=gen).to(gpu))
    return eng


def _state(eng):
    return [eng.params.master.clone(), eng.mom.clone(), eng.params.stats.clone(),
            eng.wbf.clone(), eng.gstep.clone()]


def _run7(eng, sched, what):
    """7 steps (W = 2, D = 5: start, warm-up, decay, end); per step the logged rate against
    the oracle and the state after it."""
    states = []
    for s in range(7):
        eng.step()
        torch.cuda.synchronize()
        assert not eng.persist_error()
        m = eng.metrics()
        assert m["global_step"] == s + 1
        lo.check_rate(sched, s, m["lr"], f"{what} step {s}")
        print(f"{what} step {s}: lr {m['lr']!r} oracle {lo.lr_oracle(sched, s)!r}")
        states.append(_state(eng))
    return states


@pytest.mark.parametrize("tune,optimizer", [("persist=1", "mom"), ("persist=0", "mom"),
                                            ("persist=1", "lars"), ("persist=0", "lars")])
def test_engine_follows_the_curve(gpu, monkeypatch, tune, optimizer):
    persist = tune == "persist=1"
    a = _engine(gpu, monkeypatch, ENG_SCHED, tune, optimizer=optimizer)
    b = _engine(gpu, monkeypatch, ENG_SCHED, tune, optimizer=optimizer)
    assert a.persist == persist
    if persist and optimizer == "mom":   # the one-launch optimizer, not a fall-back
        assert a.opt_fused and not a.opt_fused_reason
    what = f"{'persistent' if persist else 'per-layer'} {optimizer}"
    sa, sb = _run7(a, ENG_SCHED, what), _run7(b, ENG_SCHED, what)
    for x, y in zip(sa, sb):               # two same-seed runs agree bit for bit
        for p, q in zip(x, y):
            assert torch.equal(p, q)
    # steps 0 and 1 run at rate 0 (warm_from): with zero momentum to start from, nothing
    # moves; at the end rate 0 only the position stops, the accumulator goes on
    w = [s[0][:a.params.n_train] for s in sa]
    assert torch.equal(w[0], w[1]) and not torch.equal(w[1], w[2])
    assert not torch.equal(w[4], w[5]) and torch.equal(w[5], w[6])
    assert not torch.equal(sa[5][1], sa[6][1])


def test_engine_lars_rate_uses_the_decayed_lr(gpu, monkeypatch):
    """One LARS step in the decay (global_step 4: t = 3, q = 2/3): the update is the fp64
    step at the rate oracle-lr * trust, trust as the device logged it."""
    eng = _engine(gpu, monkeypatch, ENG_SCHED, "persist=0", optimizer="lars")
    eng.gstep.fill_(4)
    n = eng.params.n_train
    w0, m0 = eng.params.master.clone(), eng.mom.clone()
    eng.step()
    torch.cuda.synchronize()
    lr = lo.check_rate(ENG_SCHED, 4, eng.metrics()["lr"], "lars")
    assert 0 < lr < lo.f32(0.1)
    trust = eng.lars_out[0].double()        # rows: trust, |w|, |g| per segment
    assert trust.numel() == eng.nseg == len(eng.seg_arr)
    per_el = torch.cat([trust[i].repeat(int(r["numel"])) for i, r in enumerate(eng.seg_arr)])[:n]
    w_ref, m_ref, B = oo.sgd_reference(w0[:n], eng.grad[:n], m0[:n], lr * per_el,
                                       oo.f32(eng.momentum), oo.f32(eng.wd), 1.0, True)
    assert bool(((eng.params.master[:n].double() - w_ref).abs() <= B).all())
    assert bool(((eng.mom[:n].double() - m_ref).abs() <= B).all())
    assert float((eng.params.master[:n] - w0[:n]).abs().max()) > 0


@pytest.mark.parametrize("tune", ["persist=1", "persist=0"])
def test_default_flags_move_nothing(gpu, monkeypatch, tune):
    """The schedule the flags' defaults build against cifar_lr_schedule() itself: the same
    recorded launches, and weights, momentum and BN statistics bit-identical after 3 steps."""
    flags = build_parser("cifar").parse_args([])
    a = _engine(gpu, monkeypatch, schedule_from_flags(flags), tune)
    b = _engine(gpu, monkeypatch, cifar_lr_schedule(), tune)
    assert a.plan.size() == b.plan.size()
    for _ in range(3):
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert a.metrics()["lr"] == b.metrics()["lr"] == oo.f32(0.1)
    for p, q in zip(_state(a), _state(b)):
        assert torch.equal(p, q)
