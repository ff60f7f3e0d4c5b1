"""The optimizer kernels (csrc/optim.hip: sgd_update_pack, ohwi_pack, sgd_tiles,
l2_half_sum, step_increment) launched directly on synthetic parameter tables and
compared with the fp64 reference of tests/optim_oracle.py: the update within the derived
bound B, the whole bf16 weight buffer exactly (built from the kernel's own master, so
padding and the space between copies must stay zero), the device learning rate at every
edge of the schedule.  Momentum, weights and coefficients are chosen so that every term
of the update is far above B: a dropped or doubled term fails."""
import math

import numpy as np
import pytest
import torch

import optim_oracle as oo
from distributed_tensorflow_resnet_amd.train.engine import (WGD_DTYPE, LRSchedule,
                                                              cifar_lr_schedule, constant_lr,
                                                              imagenet_lr_schedule,
                                                              lr_values_scaled, scaled)

pytestmark = pytest.mark.gpu

COEFFS = [(0.9, 2e-4, 1.0), (0.75, 0.05, 1 / 128)]   # momentum, wd, grad_scale
SEVEN = LRSchedule(0.3, [10, 20, 35, 50, 80, 81, 1000],
                   [0.3, 0.2, 0.1, 0.05, 0.02, 0.01, 0.005, 0.001],
                   warm_steps=5, warm_from=0.01, warm_to=0.3)
IMAGENET = imagenet_lr_schedule()


def V(n):
    return ("vec", 1, 1, 1, n, 1, 1, False, False)


STEM = ("conv", 3, 3, 3, 16, 8, 16, True, False)
TABLE_A = [STEM, V(16), V(16),
           ("conv", 3, 3, 16, 16, 16, 16, True, True),
           ("conv", 1, 1, 16, 32, 16, 32, True, True),
           V(10), V(7), V(1), V(5),
           ("dense", 1, 1, 64, 10, 64, 16, True, True),
           V(3)]


@pytest.fixture(scope="module")
def nat(gpu):
    import distributed_tensorflow_resnet_amd as dtr

    n = dtr.native(required=True)
    assert oo.SEG_DTYPE.itemsize == n.param_seg_bytes()
    assert oo.OPTW_DTYPE.itemsize == n.opt_work_bytes()
    assert WGD_DTYPE.itemsize == n.wg_desc_bytes()
    return n


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(arr, gpu):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).to(gpu)


def _sa(s):
    return (s.init, s.warm_steps, s.warm_from, s.warm_to, list(s.bounds), list(s.values))


def _rand(n, gen, gpu):
    """O(1) values bounded away from zero."""
    x = torch.randn(n, generator=gen)
    return (x + 0.25 * torch.sign(x)).to(gpu)


class Table:
    def __init__(self, specs, gpu, seed=0):
        (self.seg, self.names, self.n, self.bf_total, self.tile0,
         self.tiles) = oo.build_seg_table(specs)
        self.gpu = gpu
        self.nseg = len(self.seg)
        self.segs_d = _dev(self.seg, gpu)
        self.tile0_d = torch.from_numpy(self.tile0).to(gpu)
        gen = torch.Generator().manual_seed(seed)
        self.w0, self.g, self.m0 = (_rand(self.n, gen, gpu) for _ in range(3))

    def fresh(self):
        return (self.w0.clone(), self.m0.clone(),
                torch.zeros(self.bf_total, dtype=torch.bfloat16, device=self.gpu))


def _i64(v, gpu):
    return torch.tensor([v], dtype=torch.int64, device=gpu)


def _pack(nat, T, w, g, mom, wbf, sched, gstep, coeff, use_mom=1, update=1, lr_out=None,
          segs=None, nseg=None, n=None):
    momentum, wd, gs = coeff
    nat.sgd_update_pack(w.data_ptr(), g.data_ptr(), mom.data_ptr(), T.n if n is None else n,
                        *_sa(sched), gstep.data_ptr() if gstep is not None else 0, momentum, wd,
                        gs, use_mom, (T.segs_d if segs is None else segs).data_ptr(),
                        T.nseg if nseg is None else nseg, wbf.data_ptr(),
                        lr_out.data_ptr() if lr_out is not None else 0, update, _st())


def _ohwi(nat, T, w, wbf, gstep_inc=None, tiles=None):
    nat.ohwi_pack(w.data_ptr(), T.segs_d.data_ptr(), T.tile0_d.data_ptr(), T.nseg,
                  T.tiles if tiles is None else tiles, wbf.data_ptr(),
                  gstep_inc.data_ptr() if gstep_inc is not None else 0, _st())


def _check_lr(sched, step, lr_out):
    """The device's rate for `step` against the fp64 schedule; returns it (fp32 value)."""
    got = float(lr_out)
    ref = oo.lr_reference(oo.f32_schedule(sched), step)
    if oo.lr_in_warmup(sched, step):
        assert abs(got - ref) <= oo.lr_bound(sched), (step, got, ref)
    else:
        assert got == oo.f32(ref), (step, got, ref)
    return got


def _check_update(w0, g, m0, w1, m1, lr, coeff, use_mom=True, what=""):
    momentum, wd, gs = (oo.f32(c) for c in coeff)
    w_ref, m_ref, B = oo.sgd_reference(w0, g, m0, lr, momentum, wd, gs, use_mom)
    ew, em = (w1.double() - w_ref).abs(), (m1.double() - m_ref).abs()
    print(f"{what} max err/B: w {float((ew / B).max()):.3f} mom {float((em / B).max()):.3f}")
    bad = (ew > B).nonzero().flatten()
    assert bad.numel() == 0, (what, "w", bad[:8].tolist(), float(ew.max()))
    bad = (em > B).nonzero().flatten()
    assert bad.numel() == 0, (what, "mom", bad[:8].tolist(), float(em.max()))


def _check_wbf(seg, w1, wbf, what=""):
    want = oo.expected_wbf(seg, w1, wbf.numel())
    if not torch.equal(wbf, want):
        bad = (wbf != want).nonzero().flatten()
        raise AssertionError((what, "wbf differs at", bad[:8].tolist(), bad.numel()))


# ---------------------------------------------------------------- (a) sgd_pack + ohwi_pack
@pytest.fixture(scope="module")
def table_a(gpu):
    T = Table(TABLE_A, gpu, seed=11)
    assert T.n % 4 != 0 and T.tiles == 6
    assert list(T.tile0) == [0, 1, 1, 1, 4, 5, 5, 5, 5, 5, 6]   # zero-tile segments all round
    return T


@pytest.mark.parametrize("coeff,sched,step", [(COEFFS[0], IMAGENET, 100), (COEFFS[1], SEVEN, 36)])
def test_pack_update_with_momentum(gpu, nat, table_a, coeff, sched, step):
    T = table_a
    w, mom, wbf = T.fresh()
    gstep, lr_out = _i64(step, gpu), torch.full((1,), 7.0, device=gpu)
    _pack(nat, T, w, T.g, mom, wbf, sched, gstep, coeff, lr_out=lr_out)
    _ohwi(nat, T, w, wbf, gstep_inc=gstep)
    torch.cuda.synchronize()
    lr = _check_lr(sched, step, lr_out)
    assert int(gstep) == step + 1
    _check_update(T.w0, T.g, T.m0, w, mom, lr, coeff, what="pack")
    _check_wbf(T.seg, w, wbf)


def test_pack_without_momentum_leaves_accumulator(gpu, nat, table_a):
    T = table_a
    w, mom, wbf = T.fresh()
    gstep, lr_out = _i64(12, gpu), torch.zeros(1, device=gpu)
    _pack(nat, T, w, T.g, mom, wbf, SEVEN, gstep, COEFFS[1], use_mom=0, lr_out=lr_out)
    _ohwi(nat, T, w, wbf)
    torch.cuda.synchronize()
    lr = _check_lr(SEVEN, 12, lr_out)
    assert torch.equal(mom, T.m0)
    assert int(gstep) == 12   # no gstep_inc: the counter is ohwi_pack's only on request
    _check_update(T.w0, T.g, T.m0, w, mom, lr, COEFFS[1], use_mom=False, what="no momentum")
    _check_wbf(T.seg, w, wbf)


def test_pack_only_writes_copies(gpu, nat, table_a):
    """update = 0 (repack after loading a checkpoint): nothing but the bf16 copies moves."""
    T = table_a
    w, mom, wbf = T.fresh()
    gstep, lr_out = _i64(5, gpu), torch.full((1,), 7.0, device=gpu)
    _pack(nat, T, w, T.g, mom, wbf, SEVEN, gstep, COEFFS[0], update=0, lr_out=lr_out)
    torch.cuda.synchronize()
    assert torch.equal(w, T.w0) and torch.equal(mom, T.m0) and float(lr_out) == 7.0
    hwio_only = T.seg.copy()
    hwio_only["bf_ohwi"] = -1
    _check_wbf(hwio_only, w, wbf, "hwio")
    _ohwi(nat, T, w, wbf)
    torch.cuda.synchronize()
    _check_wbf(T.seg, w, wbf)
    assert int(gstep) == 5 and torch.equal(w, T.w0)


def test_pack_null_step_uses_initial_rate(gpu, nat, table_a):
    T = table_a
    w, mom, wbf = T.fresh()
    lr_out = torch.zeros(1, device=gpu)
    _pack(nat, T, w, T.g, mom, wbf, IMAGENET, None, COEFFS[0], lr_out=lr_out)
    torch.cuda.synchronize()
    assert float(lr_out) == oo.f32(IMAGENET.init) != oo.f32(IMAGENET.warm_from)
    _check_update(T.w0, T.g, T.m0, w, mom, float(lr_out), COEFFS[0], what="null gstep")


def test_ohwi_pack_without_tiles_still_counts(gpu, nat, table_a):
    T = table_a
    w, _, wbf = T.fresh()
    gstep = _i64(41, gpu)
    _ohwi(nat, T, w, wbf, gstep_inc=gstep, tiles=0)
    torch.cuda.synchronize()
    assert int(gstep) == 42 and int(torch.count_nonzero(wbf)) == 0
    _ohwi(nat, T, w, wbf, tiles=0)
    torch.cuda.synchronize()
    assert int(gstep) == 42


# ---------------------------------------------------------------- (b) grid-stride path
def _table_b():
    n = 4 * 256 * 4096 + 4099
    special = {0: ("conv", 1, 1, 333, 1001, 333, 1001, False, True),
               5: ("conv", 3, 3, 5, 77, 5, 77, False, True),
               11: ("conv", 1, 1, 129, 515, 129, 520, False, True),    # kpad > K
               20: ("conv", 1, 1, 7, 9, 7, 9, False, True)}
    numel = lambda s: s[1] * s[2] * s[3] * s[4]   # noqa: E731
    specs, off = [], 0
    for i in range(36):
        s = special.get(i)
        if s is None:
            after = numel(special[i + 1]) if i + 1 in special else 0
            size = 100003 + 1000 * i   # no end on a multiple of 4, the next weight's neither
            while (off + size) % 4 == 0 or (off + size + after) % 4 == 0:
                size += 1
            s = V(size)
        specs.append(s)
        off += numel(s)
        assert off % 4 != 0, i
    assert 0 < n - off
    specs.append(V(n - off))
    return specs, n


def test_pack_grid_stride(gpu, nat):
    """More float4s than 4096 x 256 threads: the loop's second trip, and the per-thread
    segment index advanced across many segment ends, none on a multiple of 4."""
    specs, n = _table_b()
    T = Table(specs, gpu, seed=12)
    assert T.n == n and T.nseg == 37 and (n + 3) // 4 > 4096 * 256
    w, mom, wbf = T.fresh()
    gstep, lr_out = _i64(7, gpu), torch.zeros(1, device=gpu)
    _pack(nat, T, w, T.g, mom, wbf, IMAGENET, gstep, COEFFS[1], lr_out=lr_out)
    torch.cuda.synchronize()
    lr = _check_lr(IMAGENET, 7, lr_out)
    _check_update(T.w0, T.g, T.m0, w, mom, lr, COEFFS[1], what="grid-stride")
    _check_wbf(T.seg, w, wbf)


# ---------------------------------------------------------------- (c) long segment tables
def _table_c():
    def spec(i):
        k = i % 4
        if k == 0:
            return ("conv", 1, 1, 4, 8, 4, 8, True, True)
        if k == 2:
            return ("conv", 3, 3, 4, 4, 8, 4, True, True)
        return V(1 + i % 9) if k == 1 else V(1 + i % 5)

    specs, off = [], 0
    for i in range(700):
        s = spec(i)
        if i == 349:   # the second half starts on a float4, like the first
            s = V(4 - off % 4)
        specs.append(s)
        off += s[1] * s[2] * s[3] * s[4]
        if i == 349:
            assert off % 4 == 0
    return specs


def test_pack_long_tables(gpu, nat):
    """700 segments: both kernels read the table from global memory (> 640 entries).  The
    reference must hold, and the same update done as two launches over 350-segment tables
    (the LDS branch; the second with offsets rebased to its first segment) is bit-equal."""
    T = Table(_table_c(), gpu, seed=13)
    assert T.nseg == 700
    coeff, step = COEFFS[0], 3
    w, mom, wbf = T.fresh()
    gstep, lr_out = _i64(step, gpu), torch.zeros(1, device=gpu)
    _pack(nat, T, w, T.g, mom, wbf, SEVEN, gstep, coeff, lr_out=lr_out)
    _ohwi(nat, T, w, wbf)
    # two halves on a second set of buffers
    w2, mom2, wbf2 = T.fresh()
    cut = int(T.seg[350]["offset"])
    assert cut % 4 == 0
    halves = []
    for lo, hi, base in ((0, 350, 0), (350, 700, cut)):
        seg = T.seg[lo:hi].copy()
        seg["offset"] -= base
        tile0, tiles = oo.ohwi_tile_table(seg)
        n = int(seg[-1]["offset"] + seg[-1]["numel"])
        halves.append((_dev(seg, gpu), torch.from_numpy(tile0).to(gpu), tiles, n, base))
    assert sum(h[3] for h in halves) == T.n
    for segs_d, tile0_d, tiles, n, base in halves:
        _pack(nat, T, w2[base:], T.g[base:], mom2[base:], wbf2, SEVEN, gstep, coeff,
              segs=segs_d, nseg=350, n=n)
        nat.ohwi_pack(w2[base:].data_ptr(), segs_d.data_ptr(), tile0_d.data_ptr(), 350, tiles,
                      wbf2.data_ptr(), 0, _st())
    torch.cuda.synchronize()
    lr = _check_lr(SEVEN, step, lr_out)
    _check_update(T.w0, T.g, T.m0, w, mom, lr, coeff, what="700 segments")
    _check_wbf(T.seg, w, wbf)
    assert torch.equal(w2, w) and torch.equal(mom2, mom) and torch.equal(wbf2, wbf)


# ---------------------------------------------------------------- sgd_tiles
def _tiles(nat, T, w, g, mom, wbf, sched, gstep, coeff, work, blk, use_mom=1, lr_out=None,
           ticket=None, gin=None, gout=None, pack=0):
    momentum, wd, gs = coeff
    gpu = T.gpu
    work_d = _dev(work, gpu)
    blk_d = torch.tensor(blk, dtype=torch.int32, device=gpu)
    nat.sgd_tiles(w.data_ptr(), g.data_ptr(), mom.data_ptr(), *_sa(sched), gstep.data_ptr(),
                  momentum, wd, gs, use_mom, T.segs_d.data_ptr(), work_d.data_ptr(),
                  blk_d.data_ptr(), len(blk), wbf.data_ptr(),
                  lr_out.data_ptr() if lr_out is not None else 0,
                  ticket.data_ptr() if ticket is not None else 0,
                  gin.data_ptr() if gin is not None else 0,
                  gout.data_ptr() if gout is not None else 0, pack, _st())
    torch.cuda.synchronize()   # work_d / blk_d stay alive until the launch is done


@pytest.fixture(scope="module")
def table_d(gpu):
    specs = list(TABLE_A)
    specs[1] = V(3000)   # three 1024-element chunks, the last partial
    return Table(specs, gpu, seed=14)


@pytest.mark.parametrize("coeff,sched,step", [(COEFFS[0], SEVEN, 21), (COEFFS[1], IMAGENET, 6241)])
def test_tiles_update_no_slabs(gpu, nat, table_d, coeff, sched, step):
    T = table_d
    work, blk = oo.build_opt_work(T.seg, T.names)
    assert int(work[1]["tiled"]) == 0 and blk.count(1) == 3 and blk.count(3) == 3
    w, mom, wbf = T.fresh()
    g = T.g.clone()
    gstep, lr_out = _i64(step, gpu), torch.zeros(1, device=gpu)
    ticket = torch.zeros(1, dtype=torch.int32, device=gpu)
    _tiles(nat, T, w, g, mom, wbf, sched, gstep, coeff, work, blk, lr_out=lr_out, ticket=ticket)
    lr = _check_lr(sched, step, lr_out)
    assert int(gstep) == step + 1 and int(ticket) == 0
    assert torch.equal(g, T.g)
    _check_update(T.w0, T.g, T.m0, w, mom, lr, coeff, what="tiles")
    _check_wbf(T.seg, w, wbf)
    # a second launch re-uses the re-armed ticket; a null ticket leaves the step alone
    _tiles(nat, T, w, g, mom, wbf, sched, gstep, coeff, work, blk, ticket=ticket)
    assert int(gstep) == step + 2 and int(ticket) == 0
    _tiles(nat, T, w, g, mom, wbf, sched, gstep, coeff, work, blk, use_mom=0)
    assert int(gstep) == step + 2
    _check_wbf(T.seg, w, wbf)


TABLE_E = [("conv", 3, 3, 16, 16, 16, 16, True, True),    # rows 144 = 64 + 64 + 16
           V(16),
           ("conv", 3, 3, 32, 32, 32, 32, True, True),
           ("conv", 1, 1, 16, 32, 16, 32, True, True),
           STEM,                                          # cslab 8, kslab 16
           V(7),
           ("conv", 1, 1, 16, 24, 16, 24, True, True)]    # kslab 32 > K
SLAB_PAD = {0: (16, 16), 2: (32, 32), 3: (32, 16), 4: (16, 8), 6: (32, 16)}   # kslab, cslab
SENTINEL = 1e30


class Slabs:
    """Random split-K slabs [split][kslab][taps*cslab] for TABLE_E's weights, the padding
    rows and channels holding a sentinel that any read of them would carry into a sum."""

    def __init__(self, T, splits, seed):
        gen = torch.Generator().manual_seed(seed)
        self.splits, self.parts, self.dims = splits, {}, {}
        for i, (kslab, cslab) in SLAB_PAD.items():
            r = T.seg[i]
            taps, C, K = int(r["kh"] * r["kw"]), int(r["C"]), int(r["K"])
            p = torch.randn(splits, kslab, taps, cslab, generator=gen)
            p[:, K:] = SENTINEL
            p[..., C:] = SENTINEL
            self.parts[i] = p.to(T.gpu).contiguous()
            self.dims[i] = (kslab, cslab, taps, C, K)
        self.T = T

    def work(self, grad, nosplit=(64, 64)):
        T = self.T
        slabs = {T.names[i]: (p.data_ptr(), self.splits) + SLAB_PAD[i]
                 for i, p in self.parts.items()}
        return oo.build_opt_work(T.seg, T.names, grad.data_ptr(), slabs, None, nosplit)

    def check_grad(self, g_in, g_out):
        """g_out: slab sums within splits * u * sum |part| of fp64; other segments as were."""
        T = self.T
        for i, r in enumerate(T.seg):
            o, m = int(r["offset"]), int(r["numel"])
            if i not in self.parts:
                assert torch.equal(g_out[o:o + m], g_in[o:o + m]), i
                continue
            kslab, cslab, taps, C, K = self.dims[i]
            s, a = oo.slab_sum_reference(self.parts[i], self.splits, kslab, cslab, taps, C, K)
            err = (g_out[o:o + m].double().view(taps * C, K) - s).abs()
            bound = self.splits * oo.U32 * a
            assert bool((err <= bound).all()), (i, self.splits, float(err.max()))

    def grouped_reduce(self, nat, g):
        """The same slabs through wgrad_reduce_grouped into g."""
        T = self.T
        arr = np.zeros(len(self.parts), dtype=WGD_DTYPE)
        chunk = 0
        for j, (i, p) in enumerate(self.parts.items()):
            kslab, cslab, taps, C, K = self.dims[i]
            arr[j] = (p.data_ptr(), g.data_ptr() + 4 * int(T.seg[i]["offset"]), self.splits,
                      kslab, K, taps, cslab, C, chunk)
            chunk += nat.wgrad_reduce_chunks(self.splits, kslab, taps, cslab)
        d = _dev(arr, T.gpu)
        nat.wgrad_reduce_grouped(d.data_ptr(), len(arr), chunk, 1.0, _st())
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def table_e(gpu):
    return Table(TABLE_E, gpu, seed=15)


@pytest.mark.parametrize("splits", [1, 3, 8, 9, 32])
def test_tiles_update_from_slabs(gpu, nat, table_e, splits):
    """The slab sums (sequential up to 8 splits, 4 interleaved groups past that) against
    fp64 and, bit for bit, against the grouped reduce; then the update from that gradient."""
    T = table_e
    S = Slabs(T, splits, seed=100 + splits)
    coeff = COEFFS[splits % 2]
    w, mom, wbf = T.fresh()
    g = T.g.clone()
    work, blk = S.work(g)
    assert all(int(work[i]["splits"]) == splits for i in SLAB_PAD)
    if splits == 32:
        assert (int(work[0]["tr"]), int(work[0]["tc"])) == (16, 16)
    step = 60
    gstep, lr_out = _i64(step, gpu), torch.zeros(1, device=gpu)
    ticket = torch.zeros(1, dtype=torch.int32, device=gpu)
    _tiles(nat, T, w, g, mom, wbf, SEVEN, gstep, coeff, work, blk, lr_out=lr_out, ticket=ticket)
    lr = _check_lr(SEVEN, step, lr_out)
    assert int(gstep) == step + 1 and int(ticket) == 0
    S.check_grad(T.g, g)
    g2 = T.g.clone()
    S.grouped_reduce(nat, g2)
    assert torch.equal(g, g2)   # the grouped reduce's summation order (optim.hip)
    _check_update(T.w0, g, T.m0, w, mom, lr, coeff, what=f"slabs x{splits}")
    _check_wbf(T.seg, w, wbf)


@pytest.mark.parametrize("splits", [0, 9])
@pytest.mark.parametrize("with_gout", [True, False])
def test_tiles_pack_mode(gpu, nat, table_e, splits, with_gout):
    """MODE 1: only the gradient leaves (bf16 into gout, slab sums into grad)."""
    T = table_e
    w, mom, wbf = T.fresh()
    g = T.g.clone()
    if splits:
        S = Slabs(T, splits, seed=7)
        work, blk = S.work(g)
    else:
        work, blk = oo.build_opt_work(T.seg, T.names)
    gout = torch.full((T.n,), 3.0, dtype=torch.bfloat16, device=gpu) if with_gout else None
    gstep = _i64(9, gpu)
    ticket = torch.zeros(1, dtype=torch.int32, device=gpu)
    _tiles(nat, T, w, g, mom, wbf, SEVEN, gstep, COEFFS[0], work, blk, ticket=ticket, gout=gout,
           pack=1)
    assert torch.equal(w, T.w0) and torch.equal(mom, T.m0)
    assert int(torch.count_nonzero(wbf)) == 0 and int(gstep) == 9 and int(ticket) == 0
    if splits:
        S.check_grad(T.g, g)
        g2 = T.g.clone()
        S.grouped_reduce(nat, g2)
        assert torch.equal(g, g2)
    else:
        assert torch.equal(g, T.g)
    if with_gout:
        assert torch.equal(gout, g.to(torch.bfloat16))


def test_tiles_update_from_bf16_gradient(gpu, nat, table_d):
    """MODE 2: the gradient is the all-reduced bf16 buffer, 32 x 64 tiles."""
    T = table_d
    work, blk = oo.build_opt_work(T.seg, T.names, nosplit=(32, 64))
    assert (int(work[3]["tr"]), int(work[3]["tc"])) == (32, 64) and blk.count(3) == 5
    coeff, step = COEFFS[1], 82
    w, mom, wbf = T.fresh()
    gin = T.g.to(torch.bfloat16)
    g = torch.full((T.n,), 5.0, device=gpu)
    gstep, lr_out = _i64(step, gpu), torch.zeros(1, device=gpu)
    ticket = torch.zeros(1, dtype=torch.int32, device=gpu)
    _tiles(nat, T, w, g, mom, wbf, SEVEN, gstep, coeff, work, blk, lr_out=lr_out, ticket=ticket,
           gin=gin)
    lr = _check_lr(SEVEN, step, lr_out)
    assert int(gstep) == step + 1 and int(ticket) == 0
    assert torch.equal(g, gin.float())
    _check_update(T.w0, g, T.m0, w, mom, lr, coeff, what="gin")
    _check_wbf(T.seg, w, wbf)


# ---------------------------------------------------------------- (g) device learning rate
SCHEDULES = {
    "cifar": cifar_lr_schedule(),
    "imagenet": IMAGENET,
    "imagenet_steps_x0.37": scaled(IMAGENET, 0.37),
    "imagenet_values_x0.25": lr_values_scaled(IMAGENET, 0.25),
    "seven": SEVEN,
    "constant": constant_lr(0.0625 * 1.1),
}


@pytest.mark.parametrize("kernel", ["sgd_pack", "sgd_tiles"])
@pytest.mark.parametrize("name", list(SCHEDULES))
def test_device_learning_rate(gpu, nat, name, kernel):
    sched = SCHEDULES[name]
    steps = oo.lr_steps(sched)
    T = Table([V(1)], gpu, seed=16)
    w, mom, wbf = T.fresh()
    g = torch.zeros(1, device=gpu)
    gsteps = torch.tensor(steps, dtype=torch.int64, device=gpu)
    lr_out = torch.full((len(steps),), -1.0, device=gpu)
    work, blk = oo.build_opt_work(T.seg, T.names)
    work_d, blk_d = _dev(work, gpu), torch.tensor(blk, dtype=torch.int32, device=gpu)
    assert blk == [0]
    for i in range(len(steps)):   # momentum = wd = 0, g = 0: the weight stays put
        if kernel == "sgd_pack":
            nat.sgd_update_pack(w.data_ptr(), g.data_ptr(), mom.data_ptr(), 1, *_sa(sched),
                                gsteps.data_ptr() + 8 * i, 0.0, 0.0, 1.0, 1, T.segs_d.data_ptr(),
                                1, wbf.data_ptr(), lr_out.data_ptr() + 4 * i, 1, _st())
        else:
            nat.sgd_tiles(w.data_ptr(), g.data_ptr(), mom.data_ptr(), *_sa(sched),
                          gsteps.data_ptr() + 8 * i, 0.0, 0.0, 1.0, 1, T.segs_d.data_ptr(),
                          work_d.data_ptr(), blk_d.data_ptr(), 1, wbf.data_ptr(),
                          lr_out.data_ptr() + 4 * i, 0, 0, 0, 0, _st())
    torch.cuda.synchronize()
    assert gsteps.tolist() == steps and torch.equal(w, T.w0)
    got = lr_out.tolist()
    warm = 0
    for s, v in zip(steps, got):
        _check_lr(sched, s, v)
        warm += oo.lr_in_warmup(sched, s)
    assert (warm >= 3) == (sched.warm_steps > 0)


@pytest.mark.parametrize("bounds,vals", [(list(range(1, 9)), [0.1] * 9), ([10, 20], [0.1, 0.2]),
                                         ([10], [0.1, 0.2, 0.3])])
def test_schedule_shape_is_checked(gpu, nat, bounds, vals):
    T = Table([V(1)], gpu, seed=17)
    w, mom, wbf = T.fresh()
    gstep = _i64(0, gpu)
    work, blk = oo.build_opt_work(T.seg, T.names)
    work_d, blk_d = _dev(work, gpu), torch.tensor(blk, dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError):
        nat.sgd_update_pack(w.data_ptr(), T.g.data_ptr(), mom.data_ptr(), 1, 0.1, 0, 0.0, 0.0,
                            bounds, vals, gstep.data_ptr(), 0.9, 0.0, 1.0, 1,
                            T.segs_d.data_ptr(), 1, wbf.data_ptr(), 0, 1, _st())
    with pytest.raises(ValueError):
        nat.sgd_tiles(w.data_ptr(), T.g.data_ptr(), mom.data_ptr(), 0.1, 0, 0.0, 0.0, bounds, vals,
                      gstep.data_ptr(), 0.9, 0.0, 1.0, 1, T.segs_d.data_ptr(), work_d.data_ptr(),
                      blk_d.data_ptr(), 1, wbf.data_ptr(), 0, 0, 0, 0, 0, _st())
    torch.cuda.synchronize()
    assert torch.equal(w, T.w0) and int(gstep) == 0


# ---------------------------------------------------------------- (h) cost and step counter
@pytest.mark.parametrize("n", [1, 255, 131072, 131073, 1_000_003])
def test_l2_half_sum(gpu, nat, n):
    gen = torch.Generator().manual_seed(n)
    v = _rand(n, gen, gpu)
    ws = torch.full((nat.l2_workspace_floats(),), float("nan"), device=gpu)
    out = torch.full((2,), float("nan"), device=gpu)
    for i in range(2):
        nat.l2_half_sum(v.data_ptr(), n, ws.data_ptr(), out.data_ptr() + 4 * i, _st())
    torch.cuda.synchronize()
    sumsq = float((v.double() ** 2).sum())
    err = abs(float(out[0]) - 0.5 * sumsq)
    print(f"n {n}: err / bound {err / oo.l2_bound(n, sumsq):.4f}")
    assert err <= oo.l2_bound(n, sumsq)
    assert out[0].item() == out[1].item() and math.isfinite(out[0].item())


@pytest.mark.parametrize("start", [0, 2 ** 40])
def test_step_increment(gpu, nat, start):
    gstep = torch.tensor([-7, start, -9], dtype=torch.int64, device=gpu)
    nat.step_increment(gstep.data_ptr() + 8, _st())
    torch.cuda.synchronize()
    assert gstep.tolist() == [-7, start + 1, -9]
