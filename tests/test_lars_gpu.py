"""The LARS kernels (csrc/lars.hip: lars_norms, lars_trust, lars_update_pack) launched
directly on synthetic parameter tables, and the engine's lars optimizer on both plans,
against the fp64 reference and the derived bounds of tests/lars_oracle.py.  Neighbouring
segments are scaled 1000x apart, so one element read from a neighbour breaks a norm."""
import numpy as np
import pytest
import torch

import lars_oracle as lo
import optim_oracle as oo
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.train.engine import (LARS_CHUNK, LARS_DTYPE, Engine,
                                                              LRSchedule, cifar_lr_schedule,
                                                              lars_tables)

pytestmark = pytest.mark.gpu

SEVEN = LRSchedule(0.3, [10, 20, 35, 50, 80, 81, 1000],
                   [0.3, 0.2, 0.1, 0.05, 0.02, 0.01, 0.005, 0.001],
                   warm_steps=5, warm_from=0.01, warm_to=0.3)
COEFFS = [(0.9, 2e-4, 1.0), (0.75, 0.05, 1 / 128)]   # momentum, wd, grad_scale
LARS = [(0.001, 0.0), (0.02, 1e-3)]                  # eeta, epsilon


def V(n):
    return ("vec", 1, 1, 1, n, 1, 1, False, False)


# (spec, skipped): vectors of 1, 3, 5, 7, 10 at unaligned offsets, a conv with kpad > K,
# one chunk / one chunk + 1 / two chunks + 5, skipped and adapted side by side
TABLE_A = [(V(3), False),
           (("conv", 3, 3, 3, 16, 8, 16, True, False), False),
           (V(1), False),
           (("conv", 1, 1, 64, 64, 64, 64, True, True), False),     # exactly one chunk
           (V(5), True),
           (V(LARS_CHUNK + 1), False),
           (V(7), False),
           (("conv", 1, 1, 16, 24, 16, 32, True, True), False),     # kpad > K
           (V(10), True),
           (V(2 * LARS_CHUNK + 5), False),
           (V(16), False),                                          # gradient all zero
           (("conv", 3, 3, 16, 16, 16, 16, True, True), False),     # weights all zero
           (V(6), True),
           (("dense", 1, 1, 64, 10, 64, 16, True, True), False),
           (V(3), False)]
ZERO_G, ZERO_W = 10, 11


@pytest.fixture(scope="module")
def nat(gpu):
    import distributed_tensorflow_resnet_amd as dtr

    n = dtr.native(required=True)
    assert LARS_DTYPE.itemsize == n.lars_seg_bytes() and LARS_CHUNK == n.LARS_CHUNK
    return n


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(arr, gpu):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).to(gpu)


def _sa(s):
    return (s.init, s.warm_steps, s.warm_from, s.warm_to, list(s.bounds), list(s.values))


class Table:
    """A synthetic table with its LARS work map and O(1) values bounded away from zero,
    every other segment scaled by 1000."""

    def __init__(self, specs, skip, gpu, seed, zero_g=(), zero_w=()):
        (self.seg, self.names, self.n, self.bf_total, tile0, self.tiles) = oo.build_seg_table(specs)
        self.skip = list(skip)
        self.gpu, self.nseg = gpu, len(self.seg)
        self.segs_d = _dev(self.seg, gpu)
        self.tile0_d = torch.from_numpy(tile0).to(gpu)
        self.lseg, blk = lars_tables(self.seg, self.skip)
        # the work map, checked by hand: chunks of a segment are consecutive workgroups
        want = [i for i, r in enumerate(self.seg) for _ in range(-(-int(r["numel"]) // LARS_CHUNK))]
        assert blk == want and [int(x) for x in self.lseg["skip"]] == [int(s) for s in self.skip]
        assert all(int(l["chunk0"]) == want.index(i) for i, l in enumerate(self.lseg))
        self.nblk = len(blk)
        self.lseg_d = _dev(self.lseg, gpu)
        self.blk_d = torch.tensor(blk, dtype=torch.int32, device=gpu)
        gen = torch.Generator().manual_seed(seed)

        def rand():
            x = torch.randn(self.n, generator=gen)
            return x + 0.25 * torch.sign(x)

        w, g, m = rand(), rand(), rand()
        for i, r in enumerate(self.seg):
            o, k = int(r["offset"]), int(r["numel"])
            if i % 2:
                for t in (w, g, m):
                    t[o:o + k] *= 1000.0
            if i in zero_g:
                g[o:o + k] = 0.0
            if i in zero_w:
                w[o:o + k] = 0.0
        self.w0, self.g, self.m0 = w.to(gpu), g.to(gpu), m.to(gpu)

    def fresh(self):
        return (self.w0.clone(), self.m0.clone(),
                torch.zeros(self.bf_total, dtype=torch.bfloat16, device=self.gpu))


def _norms_trust(nat, T, w, g, coeff, lars, poison=float("nan")):
    """lars_norms + lars_trust; returns (part, out[3][nseg] = trust, wn, gn)."""
    _, wd, gs = coeff
    eeta, eps = lars
    part = torch.full((2 * T.nblk,), poison, dtype=torch.float64, device=T.gpu)
    out = torch.full((3, T.nseg), poison, device=T.gpu)
    nat.lars_norms(w.data_ptr(), g.data_ptr(), T.segs_d.data_ptr(), T.lseg_d.data_ptr(),
                   T.blk_d.data_ptr(), T.nblk, part.data_ptr(), _st())
    o = out.data_ptr()
    nat.lars_trust(part.data_ptr(), T.lseg_d.data_ptr(), T.nseg, eeta, wd, eps, gs, o,
                   o + 4 * T.nseg, o + 8 * T.nseg, _st())
    return part, out


def _update(nat, T, w, g, mom, wbf, out, sched, gstep, coeff, lr_out):
    momentum, wd, gs = coeff
    nat.lars_update_pack(w.data_ptr(), g.data_ptr(), mom.data_ptr(), T.n, *_sa(sched),
                         gstep.data_ptr(), momentum, wd, gs, T.segs_d.data_ptr(), T.nseg,
                         out.data_ptr(), wbf.data_ptr(), lr_out.data_ptr(), _st())
    nat.ohwi_pack(w.data_ptr(), T.segs_d.data_ptr(), T.tile0_d.data_ptr(), T.nseg, T.tiles,
                  wbf.data_ptr(), gstep.data_ptr(), _st())


def _check_norms(T, part, out, coeff, lars, what=""):
    _, wd, gs = (oo.f32(c) for c in coeff)
    eeta, eps = (oo.f32(c) for c in lars)
    ssw, ssg, wn, gn = lo.lars_norms_reference(T.w0, T.g, T.seg, gs)
    trust = lo.trust_reference(wn, gn, T.skip, eeta, wd, eps)
    part = part.cpu().view(-1, 2)
    t_k, wn_k, gn_k = (x.tolist() for x in out.cpu().double())
    worst = 0.0
    for i, l in enumerate(T.lseg):
        c0, nc = int(l["chunk0"]), int(l["nchunks"])
        for got, ref in ((float(part[c0:c0 + nc, 0].sum()), ssw[i]),
                         (float(part[c0:c0 + nc, 1].sum()), ssg[i])):
            assert abs(got - ref) <= lo.SS_REL * ref, (what, "sumsq", i, got, ref)
        assert abs(wn_k[i] - wn[i]) <= lo.NORM_REL * wn[i], (what, "wn", i, wn_k[i], wn[i])
        assert abs(gn_k[i] - gn[i]) <= lo.NORM_REL * gn[i], (what, "gn", i, gn_k[i], gn[i])
        if T.skip[i] or wn[i] == 0 or gn[i] == 0:
            assert t_k[i] == 1.0, (what, "trust of a skipped / zero-norm tensor", i, t_k[i])
        else:
            assert trust[i] != 1.0
            err = abs(t_k[i] - trust[i])
            worst = max(worst, err / (lo.TRUST_REL * trust[i]))
            assert err <= lo.TRUST_REL * trust[i], (what, "trust", i, t_k[i], trust[i])
    print(f"{what} worst trust err / bound {worst:.3f}")


def _check_update(T, w, mom, lr, coeff, lars, what=""):
    momentum, wd, gs = (oo.f32(c) for c in coeff)
    eeta, eps = (oo.f32(c) for c in lars)
    w_ref, m_ref, Bw, Bm, _, _, _ = lo.lars_reference(T.w0, T.g, T.m0, T.seg, T.skip, lr, momentum,
                                                      wd, gs, eeta, eps)
    ew, em = (w.double() - w_ref).abs(), (mom.double() - m_ref).abs()
    print(f"{what} max err/bound: w {float((ew / Bw.clamp_min(1e-300)).max()):.3f} "
          f"mom {float((em / Bm.clamp_min(1e-300)).max()):.3f}")
    bad = (ew > Bw).nonzero().flatten()
    assert bad.numel() == 0, (what, "w", bad[:8].tolist(), float(ew.max()))
    bad = (em > Bm).nonzero().flatten()
    assert bad.numel() == 0, (what, "mom", bad[:8].tolist(), float(em.max()))


def _check_wbf(seg, w1, wbf, what=""):
    want = oo.expected_wbf(seg, w1, wbf.numel())
    if not torch.equal(wbf, want):
        bad = (wbf != want).nonzero().flatten()
        raise AssertionError((what, "wbf differs at", bad[:8].tolist(), bad.numel()))


def _full_step(nat, T, sched, step, coeff, lars, what):
    """norms -> trust -> update -> ohwi_pack on fresh buffers, everything checked; returns
    the buffers for bit comparisons."""
    gpu = T.gpu
    w, mom, wbf = T.fresh()
    gstep = torch.tensor([step], dtype=torch.int64, device=gpu)
    lr_out = torch.full((1,), 7.0, device=gpu)
    part, out = _norms_trust(nat, T, w, T.g, coeff, lars)
    _update(nat, T, w, T.g, mom, wbf, out, sched, gstep, coeff, lr_out)
    torch.cuda.synchronize()
    _check_norms(T, part, out, coeff, lars, what)
    ref = oo.lr_reference(oo.f32_schedule(sched), step)
    lr = float(lr_out)
    if oo.lr_in_warmup(sched, step):
        assert abs(lr - ref) <= oo.lr_bound(sched), (step, lr, ref)
    else:
        assert lr == oo.f32(ref), (step, lr, ref)
    assert int(gstep) == step + 1
    _check_update(T, w, mom, lr, coeff, lars, what)
    _check_wbf(T.seg, w, wbf, what)
    return w, mom, wbf, part, out


@pytest.fixture(scope="module")
def table_a(gpu):
    T = Table([s for s, _ in TABLE_A], [k for _, k in TABLE_A], gpu, seed=21,
              zero_g={ZERO_G}, zero_w={ZERO_W})
    offs = [int(r["offset"]) for r in T.seg]
    assert {o % 4 for o in offs} == {0, 1, 2, 3} and T.n % 4 != 0
    assert [int(l["nchunks"]) for l in T.lseg][3:10:2] == [1, 2, 1, 3]
    return T


@pytest.mark.parametrize("coeff,lars,sched,step", [(COEFFS[0], LARS[0], cifar_lr_schedule(), 100),
                                                   (COEFFS[1], LARS[1], SEVEN, 3)])
def test_lars_kernels_against_fp64(gpu, nat, table_a, coeff, lars, sched, step):
    T = table_a
    a = _full_step(nat, T, sched, step, coeff, lars, "table A")
    out = a[4].cpu()
    assert float(out[0, ZERO_G]) == 1.0 and float(out[2, ZERO_G]) == 0.0
    assert float(out[0, ZERO_W]) == 1.0 and float(out[1, ZERO_W]) == 0.0
    b = _full_step(nat, T, sched, step, coeff, lars, "table A again")
    for x, y in zip(a, b):   # a second identical launch: bit-equal, partials included
        assert torch.equal(x, y)


def test_lars_skipped_tensors_update_like_momentum(gpu, nat, table_a):
    """Every tensor skipped: trust == 1 everywhere and the update is sgd_update_pack's, bit
    for bit (weight decay included)."""
    T = table_a
    coeff, step = COEFFS[1], 36
    skip_all = Table([s for s, _ in TABLE_A], [True] * len(TABLE_A), gpu, seed=21,
                     zero_g={ZERO_G}, zero_w={ZERO_W})
    assert torch.equal(skip_all.w0, T.w0)
    w, mom, wbf, _, out = _full_step(nat, skip_all, SEVEN, step, coeff, LARS[1], "all skipped")
    assert bool((out[0] == 1.0).all())
    w2, mom2, wbf2 = T.fresh()
    gstep = torch.tensor([step], dtype=torch.int64, device=gpu)
    nat.sgd_update_pack(w2.data_ptr(), T.g.data_ptr(), mom2.data_ptr(), T.n, *_sa(SEVEN),
                        gstep.data_ptr(), *coeff, 1, T.segs_d.data_ptr(), T.nseg, wbf2.data_ptr(),
                        0, 1, _st())
    nat.ohwi_pack(w2.data_ptr(), T.segs_d.data_ptr(), T.tile0_d.data_ptr(), T.nseg, T.tiles,
                  wbf2.data_ptr(), 0, _st())
    torch.cuda.synchronize()
    assert torch.equal(w, w2) and torch.equal(mom, mom2) and torch.equal(wbf, wbf2)


def test_lars_norms_rejects_unaligned_buffers(gpu, nat, table_a):
    T = table_a
    part = torch.zeros(2 * T.nblk, dtype=torch.float64, device=gpu)
    with pytest.raises(ValueError):
        nat.lars_norms(T.w0.data_ptr() + 4, T.g.data_ptr(), T.segs_d.data_ptr(),
                       T.lseg_d.data_ptr(), T.blk_d.data_ptr(), T.nblk, part.data_ptr(), _st())
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(part)) == 0


def test_lars_long_tables(gpu, nat):
    """More than 640 segments: the update reads the segment table from global memory."""
    specs, skip = [], []
    for i in range(700):
        k = i % 4
        specs.append(("conv", 1, 1, 4, 8, 4, 8, True, True) if k == 0 else
                     ("conv", 3, 3, 4, 4, 8, 4, True, True) if k == 2 else
                     V(1 + i % 9) if k == 1 else V(1 + i % 5))
        skip.append(k == 3 and i % 8 == 3)
    T = Table(specs, skip, gpu, seed=22)
    assert T.nseg == 700 and T.nblk == 700
    _full_step(nat, T, SEVEN, 12, COEFFS[0], LARS[1], "700 segments")


def test_lars_grid_stride(gpu, nat):
    """More float4s than 4096 x 256 threads: the update loop's second trip, segment ends
    off the multiples of 4, and tensors of hundreds of chunks."""
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
    T = Table(specs, [i in (2, 5) for i in range(9)], gpu, seed=23)
    assert T.n == n and (n + 3) // 4 > 4096 * 256 and max(int(l["nchunks"]) for l in T.lseg) > 64
    _full_step(nat, T, cifar_lr_schedule(), 7, COEFFS[1], LARS[0], "grid-stride")


# ---------------------------------------------------------------- engine
WD = 5e-4
ENG_LARS = dict(lars_eeta=0.01, lars_epsilon=1e-6)


def _engine(spec, N, gpu, optimizer="lars", seed=0, **kw):
    eng = Engine(spec, N, weight_decay=WD, lr_schedule=cifar_lr_schedule(), optimizer=optimizer,
                 device=gpu, input_mode="nhwc", seed=seed,
                 **(ENG_LARS if optimizer == "lars" else {}), **kw)
    gen = torch.Generator().manual_seed(5)
    imgs = torch.randn(N, spec.image_h, spec.image_w, 3, generator=gen).to(torch.bfloat16).float()
    eng.set_batch(imgs.to(gpu), torch.randint(0, spec.num_classes, (N,), generator=gen).to(gpu))
    return eng


def _check_engine_step(eng, w0, m0, step, what):
    """The engine's own gradient through lars_reference against its master, momentum and
    lars_state(): the optimizer alone, without the convolutions' bf16 noise."""
    n = eng.params.n_train
    lr = oo.f32(oo.lr_reference(eng.sched, step))
    assert eng.metrics()["lr"] == lr
    skip = [len(s.shape) == 1 for s in eng.params.train_slots] if eng.lars_skip == "vectors" \
        else [False] * eng.nseg
    w_ref, m_ref, Bw, Bm, wn, gn, trust = lo.lars_reference(
        w0, eng.grad, m0, eng.seg_arr, skip, lr, oo.f32(eng.momentum), oo.f32(eng.wd), 1.0,
        oo.f32(eng.lars_eeta), oo.f32(eng.lars_epsilon))
    ew = (eng.params.master[:n].double() - w_ref).abs()
    em = (eng.mom[:n].double() - m_ref).abs()
    print(f"{what} step {step}: max err/bound master {float((ew / Bw.clamp_min(1e-300)).max()):.3f}"
          f" mom {float((em / Bm.clamp_min(1e-300)).max()):.3f}")
    assert bool((ew <= Bw).all()), (what, step, float(ew.max()))
    assert bool((em <= Bm).all()), (what, step, float(em.max()))
    state = eng.lars_state()
    assert list(state) == eng.seg_names
    adapted = 0
    for i, name in enumerate(eng.seg_names):
        wn_k, gn_k, t_k = state[name]
        assert abs(wn_k - wn[i]) <= lo.NORM_REL * wn[i], (what, name, wn_k, wn[i])
        assert abs(gn_k - gn[i]) <= lo.NORM_REL * gn[i], (what, name, gn_k, gn[i])
        if trust[i] == 1.0:
            assert t_k == 1.0, (what, name, t_k)
        else:
            adapted += 1
            assert abs(t_k - trust[i]) <= lo.TRUST_REL * trust[i], (what, name, t_k, trust[i])
    assert adapted >= len([s for s in eng.params.train_slots if len(s.shape) > 1])
    assert torch.equal(eng.wbf, oo.expected_wbf(eng.seg_arr, eng.params.master, eng.wbf.numel()))
    return state


def _run_steps(eng, steps, what):
    for step in range(steps):
        w0, m0 = eng.params.master.clone(), eng.mom.clone()
        assert int(eng.gstep.item()) == step
        eng.step()
        torch.cuda.synchronize()
        assert not eng.persist_error()
        _check_engine_step(eng, w0, m0, step, what)
    assert int(eng.gstep.item()) == steps


@pytest.mark.parametrize("persist", [0, 1])
def test_engine_lars_step(gpu, monkeypatch, persist):
    monkeypatch.setenv("DTR_TUNE", f"persist={persist}")
    eng = _engine(cifar_spec(8), 16, gpu)
    assert eng.persist == bool(persist) and eng.lars
    assert not eng.opt_fused and "lars" in eng.opt_fused_reason
    names = eng.plan.names()
    a, b = eng.seg["opt"]
    assert [n for n in names[a:b] if n in ("lars_norms", "lars_trust", "lars_update_pack",
                                           "ohwi_pack", "sgd_update_pack", "sgd_tiles")] == \
        ["lars_norms", "lars_trust", "lars_update_pack", "ohwi_pack"]
    _run_steps(eng, 2, f"cifar8 persist={persist}")   # step 1 starts from a non-zero accumulator


def test_engine_lars_imagenet_s2d_stem(gpu, monkeypatch):
    monkeypatch.setenv("DTR_TUNE", "persist=0")
    eng = _engine(imagenet_spec(18, image_hw=64), 8, gpu, lars_skip="none")
    assert eng.stem_s2d
    _run_steps(eng, 2, "imagenet18 s2d, no tensor skipped")


@pytest.mark.parametrize("dtype,persist", [("fp32", "0"), ("bf16", "1")])
def test_engine_lars_norms_of_the_exchanged_gradient(gpu, monkeypatch, dtype, persist):
    """comm = the doubling loopback: the gradient the norms are taken from is the
    all-reduced one (2x the local one; bf16: rebuilt from the bf16 exchange)."""
    import distributed_tensorflow_resnet_amd as dtr

    monkeypatch.setenv("DTR_TUNE", f"persist={persist}")
    spec = cifar_spec(8)
    ref = _engine(spec, 16, gpu, optimizer="mom")
    eng = _engine(spec, 16, gpu, comm=dtr.native().Comm.loopback(2.0), bucket_mb=0.05,
                  allreduce_dtype=dtype)
    assert eng.persist == (persist == "1") and not eng.opt_fused
    assert torch.equal(eng.params.master, ref.params.master)
    w0, m0 = eng.params.master.clone(), eng.mom.clone()
    ref.step()
    eng.step()
    torch.cuda.synchronize()
    base = ref.grad if dtype == "fp32" else ref.grad.to(torch.bfloat16).float()
    assert torch.equal(eng.grad, 2 * base)
    state = _check_engine_step(eng, w0, m0, 0, f"loopback {dtype}")
    _, _, _, gn = lo.lars_norms_reference(w0, 2 * base, eng.seg_arr, 1.0)
    for i, name in enumerate(eng.seg_names):
        assert abs(state[name][1] - gn[i]) <= lo.NORM_REL * gn[i], (name, state[name][1], gn[i])


def _state(eng):
    return [eng.params.master.clone(), eng.mom.clone(), eng.params.stats.clone(),
            eng.wbf.clone(), eng.gstep.clone()]


def test_engine_lars_same_seed_engines_agree_bitwise(gpu):
    a, b = _engine(cifar_spec(8), 16, gpu), _engine(cifar_spec(8), 16, gpu)
    for _ in range(5):
        a.step()
        b.step()
    torch.cuda.synchronize()
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    assert a.lars_state() == b.lars_state()


def test_engine_lars_resume_is_bitwise(gpu, tmp_path):
    from distributed_tensorflow_resnet_amd.train.backends import GPUBackend
    from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver

    straight = _engine(cifar_spec(8), 16, gpu)
    for _ in range(4):
        straight.step()
    first = GPUBackend(_engine(cifar_spec(8), 16, gpu))
    for _ in range(2):
        first.step()
    torch.cuda.synchronize()
    prefix = Saver(str(tmp_path)).save(first.state_tensors(), 2)
    second = GPUBackend(_engine(cifar_spec(8), 16, gpu, seed=9))
    second.load_state(Saver.restore(prefix))
    assert second.global_step == 2
    for _ in range(2):
        second.step()
    torch.cuda.synchronize()
    for x, y in zip(_state(straight), _state(second.engine)):
        assert torch.equal(x, y)


def test_mom_engine_has_no_lars_state(gpu, monkeypatch):
    monkeypatch.setenv("DTR_TUNE", "persist=1")
    eng = _engine(cifar_spec(8), 16, gpu, optimizer="mom")
    assert not eng.lars and eng.lars_state() is None and eng.lars_summary() is None
    assert eng.opt_fused and eng.opt_fused_reason == "" and eng.persist
    eng.step()
    torch.cuda.synchronize()
    assert eng.lars_state() is None and int(eng.gstep.item()) == 1
    with pytest.raises(ValueError):
        _engine(cifar_spec(8), 16, gpu, optimizer="adam")
