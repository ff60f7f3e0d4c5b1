"""Recording of the training step's native plan.

A StepRecorder lives for one recording: it reads the engine's buffers, layer tables and
tune-derived switches, emits every launch of a step into the plan, and owns all the state
that only means something while ops are being emitted.  It writes nothing back to the
engine; what the running engine needs of a recording comes back as one RecordedStep.
Three plans: record_layers() (a launch per layer) and record_persistent() (train/persist.py),
the latter with or without the bucket all-reduces overlapping the backward launch.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from .engine import _ACC_CNT, _DIAG_SKIP, BF16, BN_DECAY, BN_EPS
from .layout import OPTW_DTYPE, WGD_DTYPE, _ceil, sgd_tiles_work


@dataclass
class RecordedStep:
    """What a recording leaves behind for the engine that runs the plan."""
    seg: dict = field(default_factory=dict)           # segment name -> (first op, end op)
    ready_index: dict = field(default_factory=dict)   # slot name -> op its gradient is final at
    t_fwd0: int = -1                                  # timing points (Plan.elapsed_ms)
    t_bwd0: int = -1
    t_bwd_done: int = -1
    t_joined: int = -1
    t_opt_end: int = -1
    n_allreduce: int = 0
    allreduce_bytes: int = 0
    head_fused: bool = False
    n_bap: int = 0   # identity blocks whose first dgrad applies its BN backward (bap)
    # stream check: device-side waits {op: (producer op, buffers covered)}, {op: buffers touched}
    device_deps: dict = field(default_factory=dict)
    op_buffers: dict = field(default_factory=dict)
    keep: list = field(default_factory=list)          # tensors the plan's pointers refer to


class StepRecorder:
    def __init__(self, engine, plan):
        self.e, self.plan, self.out = engine, plan, RecordedStep()
        for bn in engine.bns.values():
            bn.pending = None     # forward statistics not yet finalized (_BN.pending)
        self._pending = {}        # slot name -> split-K slab descriptor awaiting its reduce
        self._produced = {"dense/bias", engine.dense_name}   # slots whose gradient is emitted
        self._flushed, self._reduced = set(), set()          # buckets / (bucket, group) done
        self._side_q, self._side_blocks = [], 0              # queued side-stream ops
        self._main_wgrad = False  # a main-stream wgrad not yet ordered before the side stream
        self._reduce_main = False                            # slab reduces on the main stream
        self._pending_bwd = None  # a BN backward whose finalize + apply are deferred
        self._bnb_src = None      # (sums ptr, count) the last dgrad epilogue left
        self._comm_forks = 0

    # ------------------------------------------------------------------ forward pieces
    def _take_prefin(self, pre) -> list:
        """The BN-finalize prologue of the conv consuming BN `pre` (BnPreFin: 12 pointers /
        counts), taking over the BN's pending statistics; [] when nothing is pending."""
        if pre is None or pre.pending is None:
            return []
        if pre.pending[0] == "acc":
            _, part, M0 = pre.pending
            cnt, rows = _ACC_CNT, 0
        else:
            part, cnt, rows, M0 = pre.pending
        pre.pending = None
        return [part, cnt, rows, M0, pre.gamma, pre.beta, *pre.stat_ptrs(), pre.mmean, pre.mvar]

    def _conv_fwd(self, c, x, out, N, pre=None, residual=None, stats_for=None):
        """One conv launch.  BatchNorm statistics of the output (``stats_for``) go
        into the BN's fp64 accumulators (bn_acc, default), which its first consumer
        reads; or, as per-tile partials, are finalized by the first consumer's prologue
        (few tiles) or else by a separate bn_finalize launch."""
        e = self.e
        geom = e._geom(c, N)
        if self._fwd_stream(c, N, pre, stats_for):
            self._conv_fwd_stream(c, x, out, N, pre, residual, stats_for)
            return
        stat_ptr, fin, pfin, b = 0, [], self._take_prefin(pre), stats_for
        if b is not None:
            M, nc = N * c.spec.ho * c.spec.wo, c.spec.cout
            bm = e.nat.conv_gemm_bm(M, nc)
            T = _ceil(M, bm)
            stat_ptr = b.part.data_ptr()
            b.pending = (stat_ptr, T, bm, M)
            # measured (CIFAR bs 128 / 32): the consumer prologue when the tiles are few,
            # else a separate finalize, beats producer-side last-arriver finalizes
            if e.bn_acc_on:
                fin = [b.acc.data_ptr()]
                b.pending = ("acc", b.acc.data_ptr(), M)
            elif T > e._consumer_cap(nc):
                b.pending = ("separate", stat_ptr, T, bm, M)
        self.plan.conv_gemm(0, x.data_ptr(), c.ohwi, out.data_ptr(), 0,
                            0 if residual is None else residual.data_ptr(),
                            0 if pre is None else pre.scale.data_ptr(),
                            0 if pre is None else pre.shift.data_ptr(), 0, 0, stat_ptr, 0, geom,
                            [], fin, [], pfin, [], BN_DECAY, BN_EPS, 1)

    def _fwd_stream(self, c, N, pre, stats_for) -> bool:
        """Whether a forward conv takes the streaming narrow-K 1x1 kernel (bn_fwd1x1.hip):
        1x1 stride 1, K = 64..256 input channels, >= 256-wide output, statistics (if any) in
        fp64 accumulators, its BN prologue (if any) finalized or pending in accumulators."""
        e, s = self.e, c.spec
        if not e.fwd1x1_stream or e.stem_s2d and s.name == e.spec.stem.name:
            return False
        if (s.kh != 1 or s.kw != 1 or s.stride != 1
                or not e.nat.bnf1x1_covers(N * s.ho * s.wo, s.cout, c.cin)):
            return False
        if stats_for is not None and not e.bn_acc_on:
            return False
        return pre is None or pre.pending is None or pre.pending[0] == "acc"

    def _conv_fwd_stream(self, c, x, out, N, pre, residual, stats_for):
        s = c.spec
        M = N * s.ho * s.wo
        pfin, ps, psh = self._take_prefin(pre), 0, 0
        if pre is not None and not pfin:
            ps, psh = pre.scale.data_ptr(), pre.shift.data_ptr()
        acc = 0
        if stats_for is not None:
            acc = stats_for.acc.data_ptr()
            stats_for.pending = ("acc", acc, M)
        self.plan.bnf1x1([x.data_ptr(), c.ohwi, 0 if residual is None else residual.data_ptr(),
                          out.data_ptr(), ps, psh, acc], pfin, M, s.cout, c.cin, BN_DECAY,
                         BN_EPS, 1)

    def _bn_input(self, bn, x, y):
        """Operand of the conv consuming BN(x): (y, None) after materializing
        y = ReLU(BN(x)) when the engine gave the BN a buffer `y` (_alloc_activations),
        else (x, bn) -- the conv applies BN+ReLU while staging (PRE)."""
        plan = self.plan
        if y is None:
            self._bn_finalize(bn)
            return x, bn
        C = bn.spec.channels
        if bn.pending is not None and bn.pending[0] == "acc":
            # the apply pass finalizes too (no bn_finalize launch in between)
            _, part, M = bn.pending
            bn.pending = None
            plan.bn_relu_apply_acc(x.data_ptr(), y.data_ptr(), M, C, part, bn.gamma, bn.beta,
                                   bn.mmean, bn.mvar, BN_DECAY, BN_EPS, 1, *bn.stat_ptrs())
            return y, None
        self._bn_finalize(bn, consumer_conv=False)
        plan.bn_relu_apply(x.data_ptr(), bn.scale.data_ptr(), bn.shift.data_ptr(), y.data_ptr(),
                           x.numel() // C, C)
        return y, None

    def _bn_finalize(self, bn, train=True, consumer_conv: bool = True):
        """Called where the BN's statistics are next needed.  Deferred to the first
        consumer conv when that conv can combine the partials itself (BnPreFin);
        otherwise (or for a non-conv consumer) one bn_finalize launch (case (d))."""
        if bn.pending is None:
            return
        if bn.pending[0] == "acc":
            if consumer_conv:
                return
            _, part, M = bn.pending
            tiles, rows = -1, 0
        elif bn.pending[0] == "separate":
            _, part, tiles, rows, M = bn.pending
        elif consumer_conv:
            return
        else:
            part, tiles, rows, M = bn.pending
        bn.pending = None
        self.plan.bn_finalize(part, tiles, rows, M, bn.spec.channels, bn.gamma,
                              bn.beta, bn.mmean, bn.mvar, BN_DECAY, BN_EPS, int(train),
                              *bn.stat_ptrs())

    def _mark(self, *names):
        idx = self.plan.size()
        for n in names:
            self.out.ready_index[n] = idx

    # ------------------------------------------------------------------ backward pieces
    def _bap_ok(self, c, N) -> bool:
        """Whether the first 1x1 dgrad of an identity bottleneck block emits its input
        BatchNorm's backward output itself (_conv_bwd ``bap``): accumulator-mode sums,
        a shape the streaming kernel covers, and the block's wide input channels within
        the ``bap_maxc`` bound (0 = off)."""
        e = self.e
        return e.bn_bacc_on and 0 < c.cin <= e.bap_maxc and self._dgrad1x1_covers(c, N)

    def _dgrad1x1_covers(self, c, N) -> bool:
        """A 1x1 stride-1 dgrad the streaming kernel (bn_dgrad1x1.hip) covers and the
        direct (CIFAR) kernel does not."""
        e, s = self.e, c.spec
        if s.kh != 1 or s.kw != 1 or s.stride != 1:
            return False
        return (e.nat.bnd1x1_covers(N * s.h * s.w, c.cin, s.cout)
                and not e.nat.conv_direct_covers(1, e._geom(c, N)))

    def _dgrad_stream_ok(self, c, N) -> bool:
        """1x1 stride-1 dgrads with BN-backward sums whose weights fit the streaming kernel
        (bn_dgrad1x1.hip mode 2): the expanding conv's dgrad at stages 1-2, the first
        conv's at stage 3 (tune dgrad1x1_stream)."""
        return self.e.dgrad1x1_stream and self._dgrad1x1_covers(c, N)

    def _conv_bwd(self, c, dy, x, N, pre, dx=None, accumulate=False,
                  bnb: tuple | None = None, side: bool = True, bap: tuple | None = None):
        """dgrad into dx (optional), then wgrad (+ reduce into the flat gradient).

        ``bnb=(bn, bn_input)``: the dgrad epilogue also emits that BN's backward
        partial sums (sum g, sum g*xhat of dx).  If ``dy`` is the output of a
        pending BN backward (_bn_bwd), the direct dgrad applies that BN backward
        while staging dy (BnBwdPre) and materializes dy for the wgrad.

        ``bap=(bn, add)`` (bn's input is ``x``, the 1x1 conv's own input): dx receives
        the BN+ReLU backward OUTPUT, BNbwd(dgrad) + add, with no separate apply pass.
        The dgrad runs twice on the streaming kernel (bn_dgrad1x1.hip): a first pass only
        sums (sum g, sum g*xhat into the fp64 accumulators, no store), a finalize turns
        the sums into the apply coefficients, and the second pass recomputes the same
        GEMM tile (bitwise the same fp32 values) and applies BN backward + add.
        For a bottleneck block's first conv the GEMM is narrow (K = 64..512 input
        rows), while the BN'd tensor is wide (256..2048 channels): recomputing it
        costs less than writing the wide gradient, re-reading it and x, and writing
        dx in a separate apply (reference: FusedBatchNormGrad after
        Conv2DBackpropInput, resnet_model_official.py:133-175)."""
        e, plan = self.e, self.plan
        geom = e._geom(c, N)
        s = c.spec
        abw = []
        a_src = dy
        pb = self._pending_bwd
        if pb is not None:
            fuse = pb["out"] is dy and dx is not None
            # the direct (CIFAR) dgrad applies the pending BN backward while staging dy;
            # the implicit-GEMM dgrads keep the separate apply (fusing it there repeated
            # the per-element work per column tile and tap: ImageNet 13.3 -> 17.8 ms)
            if fuse and e.nat.conv_direct_covers(1, geom):
                bn = pb["bn"]
                add = pb["add"]
                part, cnt = pb["part"], pb["cnt"]
                if cnt != -1 and cnt > e._consumer_cap(s.cout):
                    # too many partials for the prologue: finalize separately, the
                    # dgrad then reads the coefficients (cnt = 0)
                    plan.bn_bwd_finalize(part, cnt, pb["M"], bn.spec.channels, bn.gamma,
                                         bn.rstd.data_ptr(), bn.dgamma, bn.dbeta,
                                         e.coef.data_ptr())
                    part, cnt = 0, 0
                abw = [pb["x"].data_ptr(), 0 if add is None else add.data_ptr(),
                       *bn.stat_ptrs(), bn.gamma, part, _ACC_CNT if cnt == -1 else cnt,
                       dy.data_ptr(), bn.dgamma, bn.dbeta, e.coef.data_ptr()]
                self._produced.update(bn.names)
                self._pending_bwd = None
                a_src = pb["da"]        # the dgrad stages BNbwd(da) and writes dy itself
            else:
                self._emit_bn_bwd()
        if dx is not None and bap is not None:
            bn, add = bap
            self.out.n_bap += 1
            assert not abw, "bap: the dgrad's input is not a pending BN-backward output"
            M, C = N * s.h * s.w, c.cin
            # the streaming kernel (bn_dgrad1x1.hip) runs both passes (_bap_ok checked coverage)
            base = [a_src.data_ptr(), c.hwio, x.data_ptr()]
            bnp = bn.stat_ptrs()
            plan.bnd1x1(0, base + [0, 0] + bnp + [0, bn.bacc.data_ptr()], M, C, s.cout)
            plan.bn_bwd_finalize(bn.bacc.data_ptr(), -1, M, C, bn.gamma, bn.rstd.data_ptr(),
                                 bn.dgamma, bn.dbeta, e.coef.data_ptr())
            self._produced.update(bn.names)
            addp = 0 if add is None else add.data_ptr()
            plan.bnd1x1(1, base + [addp, dx.data_ptr()] + bnp + [e.coef.data_ptr(), 0], M, C,
                        s.cout)
        elif dx is not None:
            bl, bfl = [], []
            if bnb is not None:
                bn, bx = bnb
                Mx = N * s.h * s.w
                C = c.cin
                T = _ceil(Mx, e.nat.conv_gemm_bm(Mx, C))
                bl = [bx.data_ptr(), *bn.stat_ptrs(), bn.bpart.data_ptr()]
                self._bnb_src = (bn.bpart.data_ptr(), T)
                if e.bn_bacc_on:
                    bfl = [bn.bacc.data_ptr()]
                    self._bnb_src = (bn.bacc.data_ptr(), -1)
            stream_bnb = (bnb is not None and e.bn_bacc_on and not accumulate and not abw
                          and self._dgrad_stream_ok(c, N))
            if stream_bnb and "dgrad" not in _DIAG_SKIP:
                # 1x1 dgrad + BN-backward sums on the streaming kernel (bn_dgrad1x1.hip mode 2)
                plan.bnd1x1(2, [a_src.data_ptr(), c.hwio, bx.data_ptr(), 0, dx.data_ptr()] +
                            bl[1:5] + [0, bn.bacc.data_ptr()], Mx, C, s.cout)
            elif "dgrad" not in _DIAG_SKIP:
                plan.conv_gemm(1, a_src.data_ptr(), c.hwio, dx.data_ptr(), 0, 0, 0, 0, 0, 0,
                               0, int(accumulate), geom, bl, [], bfl, [], abw, BN_DECAY, BN_EPS,
                               1)
        # The weight gradient only feeds the bucket's grouped reduce, so it runs on
        # the side stream, overlapping the dgrad -> BN-backward chain.  Forks are
        # batched per residual block (_flush_side): a cross-stream event pair costs
        # ~6 us of device time on ROCm, about a third of a CIFAR wgrad.
        off, sp, pps = e.wg_off[s.name]
        part = e.wg_part.data_ptr() + 4 * off

        desc = (dy.data_ptr(), x.data_ptr(), 0 if pre is None else pre.scale.data_ptr(),
                0 if pre is None else pre.shift.data_ptr(), part, tuple(geom), sp, pps)
        if e.fork_wgrad and side:
            self._side_q.append(desc)
        else:
            self._emit_wgrads([desc])
            # a side-stream reduce of this slab must fork after it (_flush_side)
            self._main_wgrad = e.fork_wgrad
        if e.stem_s2d and s.name == e.spec.stem.name:   # 4x4x16 HWIO, mapped back by _emit_reduce
            self._pending[c.name] = (part, e.stem_g4.data_ptr(), sp, s.cout, s.cout, 16, 16, 16)
        else:
            self._pending[c.name] = (part, c.grad, sp, s.cout, s.cout, s.kh * s.kw, c.cin,
                                     c.cin_valid)
        self._produced.add(c.name)

    def _bn_bwd(self, bn, dy, x, dx, add=None, reduced: bool = False):
        """BN+ReLU backward dx = BNbwd(dy) (+ add).  ``reduced``: the producing dgrad
        already wrote the partial sums (conv epilogue BNB).  The finalize + apply are
        deferred: the next dgrad consuming dx applies them while staging its input
        (_conv_bwd), else _emit_bn_bwd launches them."""
        C = bn.spec.channels
        M = x.numel() // C
        if self._pending_bwd is not None:
            self._emit_bn_bwd()
        if reduced:
            part, cnt = self._bnb_src
        else:
            cnt = self.e.nat.bn_bwd_tiles(M, C)
            part = bn.bpart.data_ptr()
            self.plan.bn_bwd_reduce(dy.data_ptr(), x.data_ptr(), *bn.stat_ptrs(), M, C, part)
        self._pending_bwd = dict(bn=bn, da=dy, x=x, out=dx, add=add, part=part, cnt=cnt, M=M)

    def _emit_bn_bwd(self):
        """Launch the pending BN backward's finalize + apply (no fusing consumer)."""
        e, plan = self.e, self.plan
        pb = self._pending_bwd
        if pb is None:
            return
        self._pending_bwd = None
        bn, M, C = pb["bn"], pb["M"], pb["bn"].spec.channels
        add = pb["add"]
        self._produced.update(bn.names)
        if pb["cnt"] == -1 and e.nat.bn_bwd_apply_acc_fits(M, C):
            # accumulator sums, small C: the apply launch finalizes too (one launch less)
            plan.bn_bwd_apply_acc(pb["da"].data_ptr(), pb["x"].data_ptr(), *bn.stat_ptrs(),
                                  [pb["part"], bn.gamma, bn.dgamma, bn.dbeta, e.coef.data_ptr()],
                                  0 if add is None else add.data_ptr(), pb["out"].data_ptr(), M, C)
            return
        plan.bn_bwd_finalize(pb["part"], pb["cnt"], M, C, bn.gamma, bn.rstd.data_ptr(),
                             bn.dgamma, bn.dbeta, e.coef.data_ptr())
        plan.bn_bwd_apply(pb["da"].data_ptr(), pb["x"].data_ptr(), *bn.stat_ptrs(),
                          e.coef.data_ptr(), 0 if add is None else add.data_ptr(),
                          pb["out"].data_ptr(), M, C)

    def _flush_side(self, force: bool = False):
        """Fork: emit the queued weight gradients on the side stream behind ONE event
        (every `fork_every` residual blocks, or now if `force`)."""
        plan = self.plan
        if not self._side_q and not (force and self._main_wgrad):
            return
        self._side_blocks += 1
        if not force and self._side_blocks < self.e.fork_every:
            return
        self._main_wgrad = False   # the fork orders them before everything queued now
        ev = plan.new_event()
        plan.record(ev)
        plan.use_stream(1)
        plan.wait(ev)
        self._emit_wgrads(self._side_q)
        plan.use_stream(0)
        self._side_q, self._side_blocks = [], 0

    def _split_tail(self) -> list:
        """End of the dgrad chain (first block done): fork the first part of the queued
        weight gradients to the side stream now and return the last `tail_main`
        fraction, which the main stream runs after the stem instead of idling until the
        side stream drains them.  The bucket reduces are emitted afterwards (forced
        flush), so no reduce can read a slab before its main-stream wgrad."""
        q = self._side_q
        k = len(q) - int(round(self.e.tail_main * len(q)))
        while k < len(q) and callable(q[k]):   # queued non-wgrad side ops stay on the side
            k += 1
        self._side_q = q[:k]
        if self._side_q:
            self._flush_side(force=True)
        else:
            self._side_blocks = 0
        return q[k:]

    def _emit_wgrads(self, descs):
        """Weight-gradient launches on the current stream, in queue order (queued
        non-wgrad side ops -- the head's batch folds, the dense wgrad -- are callables)."""
        for d in descs:
            if callable(d):
                d()
            elif "wgrad" not in _DIAG_SKIP:   # (diagnostics only: scripts/diag_step.py)
                self.plan.conv_wgrad(d[0], d[1], d[2], d[3], d[4], list(d[5]), d[6], d[7])

    def _flush_buckets(self, force: bool = False):
        """Emit the grouped split-K reduce of every reduce group whose gradients are
        all produced (all remaining ones if `force`).  A bucket whose groups are all
        reduced is ready for its all-reduce (world > 1): with the native communicator
        the comm stream waits on the main stream (BN parameter gradients) AND on the
        side stream (the bucket's reduces), so the main stream's dgrad chain never
        waits for the side stream mid-backward; for host-issued c10d all-reduces the
        side stream is joined into the main stream (the host issues on main).  With
        one process the only join is the final one."""
        e = self.e
        for bi, (lo, hi, names) in enumerate(e.buckets):
            if bi in self._flushed:
                continue
            for gi, gnames in enumerate(e.reduce_groups[bi]):
                if (bi, gi) in self._reduced or not (
                        force or all(n in self._produced for n in gnames)):
                    continue
                self._flush_side(force=True)   # the group's wgrads precede its reduce
                self._emit_reduce(gnames)
                self._reduced.add((bi, gi))
            if not all((bi, gi) in self._reduced for gi in range(len(e.reduce_groups[bi]))):
                continue
            if e.comm is not None:
                self._mark(*names)
                self._flushed.add(bi)
                self._emit_allreduce(lo, hi, side_dep=e.fork_wgrad and not self._reduce_main)
                continue
            if e.reduce_buckets or force:
                if e.fork_wgrad and not self._reduce_main:
                    self._join(1)   # (and with the main stream the bucket's all-reduce)
                self._mark(*names)
                self._flushed.add(bi)

    def _emit_allreduce(self, lo: int, hi: int, side_dep: bool, on_main: bool = False,
                        packed: bool = False):
        """Fork the comm stream off the main stream (and, with ``side_dep``, off the
        side stream, where the bucket's split-K reduces ran) at the bucket's ready
        point and all-reduce grad[lo:hi) there (bf16 exchange: cast kernels on the
        comm stream around a bf16 all-reduce), while the compute streams continue.
        ``on_main``: on the main stream itself, no fork and no join (the persistent
        step: nothing is left to overlap, and each event costs ~5 us between launches).
        ``packed``: grad_bf16[lo:hi) already holds the bf16 input (_emit_pack) and the
        optimizer reads the result from it: no cast launches."""
        e, plan = self.e, self.plan
        if on_main:
            assert not side_dep
        else:
            evs = [plan.new_event()]
            plan.record(evs[0])
            if side_dep:
                evs.append(plan.new_event())
                plan.use_stream(1)
                plan.record(evs[1])
            plan.use_stream(2)
            for ev in evs:
                plan.wait(ev)
        n = hi - lo
        g = e.grad.data_ptr() + 4 * lo
        if e.grad_bf16 is not None:
            gb = e.grad_bf16.data_ptr() + 2 * lo
            if not packed:
                plan.cast_f32_bf16(g, gb, n)
            plan.all_reduce(e.comm, gb, n, e.nat.COMM_BF16)
            if not packed:
                plan.cast_bf16_f32(gb, g, n)
        else:
            plan.all_reduce(e.comm, g, n, e.nat.COMM_F32)
        self.out.n_allreduce += 1
        self._comm_forks += 0 if on_main else 1
        self.out.allreduce_bytes += n * (2 if e.grad_bf16 is not None else 4)
        plan.use_stream(0)

    def _join(self, stream: int):
        """The main stream waits for everything queued on `stream` (1 side, 2 comm)."""
        plan = self.plan
        ev = plan.new_event()
        plan.use_stream(stream)
        plan.record(ev)
        plan.use_stream(0)
        plan.wait(ev)

    def _join_comm(self):
        """The optimizer (main stream) waits for every bucket's all-reduce."""
        if self.e.comm is not None and self._comm_forks:
            self._join(2)

    def _emit_reduce(self, names, stream: int | None = None):
        e, plan = self.e, self.plan
        descs = [self._pending.pop(n) for n in names if n in self._pending]
        if not descs:
            return
        arr = np.zeros(len(descs), dtype=WGD_DTYPE)
        chunk = 0
        for i, (part, grad, sp, K, Kv, taps, C, Cv) in enumerate(descs):
            arr[i] = (part, grad, sp, K, Kv, taps, C, Cv, chunk)
            chunk += e.nat.wgrad_reduce_chunks(sp, K, taps, C)
        t = torch.from_numpy(arr.view(np.uint8).copy()).to(e.device)
        self.out.keep.append(t)
        if stream is None:
            stream = 1 if e.fork_wgrad and not self._reduce_main else 0
        plan.use_stream(stream)
        plan.wgrad_reduce_grouped(t.data_ptr(), len(descs), chunk, 1.0)
        st = e.spec.stem
        sc = e.convs[st.name]
        if e.stem_s2d and sc.name in names:   # names: slot names ("conv2d/kernel")
            plan.stem_s2d_grad(e.stem_g4.data_ptr(), sc.grad, st.cout)
        plan.use_stream(0)

    def _g(self, shape):
        """A fresh gradient buffer per backward tensor: with weight gradients on the side stream
        a rotating pool would need WAR fences; 288 GB of HBM makes this the simpler choice."""
        t = torch.empty(shape, dtype=BF16, device=self.e.device)
        self.out.keep.append(t)
        return t

    # ------------------------------------------------------------------ optimizer launches
    def _packed_gin(self) -> int:
        """The optimizer's gradient source after a packed all-reduce: grad_bf16 (bf16
        exchange) or grad itself (0: fp32 exchange, the pack summed the slabs into it)."""
        return self.e.grad_bf16.data_ptr() if self.e.grad_bf16 is not None else 0

    def _sgd_tiles_work(self, slabs, names=None, gin=0):
        """sgd_tiles_work for the engine's segments, as device tensors.  Reading the
        all-reduced bf16 (`gin`) there is nothing to sum: 32 x 64 tiles, twice the
        workgroups of 64 x 64 for a launch that is all load latency."""
        e = self.e
        work, blk = sgd_tiles_work(e.seg_arr, e.seg_names, slabs, e.grad.data_ptr(), names,
                                   (32, 64) if gin else (64, 64))
        assert OPTW_DTYPE.itemsize == e.nat.opt_work_bytes()
        wt = torch.from_numpy(work.view(np.uint8).copy()).to(e.device)
        bt = torch.tensor(blk, dtype=torch.int32, device=e.device)
        self.out.keep += [wt, bt]
        return wt, bt, len(blk)

    def _sgd_tiles(self, wt, bt, nblk, *, lr_slot=0, ticket=0, gin=0, gout=0, pack=0):
        """One sgd_tiles launch over the work map.  lr_slot: where it logs the LR; ticket: its
        last workgroup also does global_step += 1; gin: the bf16 buffer the gradient is read from
        (0: grad); pack, gout: no update, only the all-reduce input (into grad, or bf16 gout)."""
        e = self.e
        self.plan.sgd_tiles(e.params.master.data_ptr(), e.grad.data_ptr(), e.mom.data_ptr(),
                            *e.sched.launch_args(), e.gstep.data_ptr(), e.momentum, e.wd, 1.0,
                            int(e.use_momentum), e.segs.data_ptr(), wt.data_ptr(), bt.data_ptr(),
                            nblk, e.wbf.data_ptr(), lr_slot, ticket, gin, gout, pack,
                            *e.sched.extra_launch_args())

    def _emit_pack(self, names, stream: int = 0):
        """The all-reduce input of `names`' gradients in ONE launch (sgd_tiles pack mode,
        the optimizer's own slab summation): split-K slab sums and the other gradients as
        bf16 into grad_bf16 (fp32 exchange: the slab sums into grad).  Replaces a grouped
        reduce plus a cast launch; the optimizer then reads the all-reduced bf16 (gin)."""
        slabs = {n: self._pending.pop(n) for n in names if n in self._pending}
        work = self._sgd_tiles_work(slabs, names=set(names))
        self.plan.use_stream(stream)
        self._sgd_tiles(*work, gout=self._packed_gin(), pack=1)
        self.plan.use_stream(0)

    def _emit_update(self, names, gin=0, step=True, slabs=None):
        """ONE sgd_tiles launch updating the segments `names` (None: all) from grad or the
        all-reduced bf16 `gin`, summing the split-K `slabs` (a dict) of those still in
        slabs; step: it also does global_step += 1 (the step's last update launch)."""
        e = self.e
        work = self._sgd_tiles_work(slabs or {}, names=names, gin=gin)
        self._sgd_tiles(*work, lr_slot=e.scalars.data_ptr() + 8,
                        ticket=e.opt_ticket.data_ptr() if step else 0, gin=gin)

    def _emit_optimizer(self, fused_slabs=None, gin=0, names=None):
        """Optimizer segment (fused SGD-momentum + wd + bf16 re-pack, global_step += 1)
        and the `cost` segment (1/2 sum v^2 of the weights).  fused_slabs (a dict, the
        persistent step): ONE sgd_tiles launch that also sums those weights' slabs.
        gin: the gradient is read from that bf16 buffer (the all-reduced pack, _emit_pack).
        names: only those segments (the rest were updated ahead, _emit_update)."""
        e, plan, out = self.e, self.plan, self.out
        spec, sp, b2 = e.spec, e.scalars.data_ptr(), plan.size()
        master, grad, mom = e.params.master.data_ptr(), e.grad.data_ptr(), e.mom.data_ptr()
        if names is not None or fused_slabs is not None:
            assert not e.lars and not (names is not None and fused_slabs)
            self._emit_update(names, gin, slabs=fused_slabs)
        else:
            if e.lars:
                # grad is complete here (reduced, all-reduced and joined; the s2d stem's
                # mapped back): every rank forms the same norms from the same bits
                lo = e.lars_out.data_ptr()
                plan.lars_norms(master, grad, e.segs.data_ptr(), e.lars_segs.data_ptr(),
                                e.lars_blk.data_ptr(), e.lars_blk.numel(), e.lars_part.data_ptr())
                plan.lars_trust(e.lars_part.data_ptr(), e.lars_segs.data_ptr(), e.nseg,
                                e.lars_eeta, e.wd, e.lars_epsilon, 1.0, lo, lo + 4 * e.nseg,
                                lo + 8 * e.nseg)
                plan.lars_update_pack(master, grad, mom, e.params.n_train, *e.sched.launch_args(),
                                      e.gstep.data_ptr(), e.momentum, e.wd, 1.0,
                                      e.segs.data_ptr(), e.nseg, lo, e.wbf.data_ptr(), sp + 8,
                                      *e.sched.extra_launch_args())
            elif e.adam:
                # one launch (csrc/adam.hip); with clipping the norm launches go in front and
                # the update reads the scale from the device slot, as sgd_clip_update_pack does
                clip, co = e.clip_grad_norm > 0, 0
                i0 = plan.size()
                if clip:
                    co = e.clip_out.data_ptr()
                    plan.grad_sqnorm(grad, e.params.n_train, e.clip_part.data_ptr())
                    plan.clip_scale(e.clip_part.data_ptr(), e.clip_chunks,
                                    float(np.float32(e.clip_grad_norm)), co)
                lamb = ()
                if e.lamb:
                    # adam_trust on (csrc/lamb.hip): the moments and the chunk sums of w^2 and
                    # u^2, the per-tensor trust ratios, then the update at lr * trust -- grad is
                    # complete here, as for lars, and only the first launch reads it
                    lo = e.lars_out.data_ptr()
                    coef = (e.adam_beta1, e.adam_beta2, e.adam_epsilon)
                    j0 = plan.lamb_moments_norms(
                        master, grad, mom, e.adam_v.data_ptr(), e.gstep.data_ptr(),
                        e.adam_start.data_ptr(), *coef, 1.0, co, e.adam_decay,
                        e.segs.data_ptr(), e.lars_segs.data_ptr(), e.lars_blk.data_ptr(),
                        e.lars_blk.numel(), e.adam_wd.data_ptr(), e.lars_part.data_ptr())
                    j1 = plan.lamb_trust(e.lars_part.data_ptr(), e.lars_segs.data_ptr(), e.nseg,
                                         lo, lo + 4 * e.nseg, lo + 8 * e.nseg)
                    i1 = plan.lamb_update_pack(
                        master, mom, e.adam_v.data_ptr(), e.params.n_train,
                        *e.sched.launch_args(), e.gstep.data_ptr(), e.adam_start.data_ptr(),
                        *coef, e.adam_decay, e.segs.data_ptr(), e.nseg, e.adam_wd.data_ptr(), lo,
                        e.wbf.data_ptr(), sp + 8, e.adam_out.data_ptr(),
                        *e.sched.extra_launch_args())
                    lamb = (j0, j1)
                else:
                    i1 = plan.adam_update_pack(master, grad, mom, e.adam_v.data_ptr(),
                                               e.params.n_train, *e.sched.launch_args(),
                                               e.gstep.data_ptr(), e.adam_start.data_ptr(),
                                               e.adam_beta1, e.adam_beta2, e.adam_epsilon, 1.0, co,
                                               e.adam_decay, e.segs.data_ptr(), e.nseg,
                                               e.adam_wd.data_ptr(), e.wbf.data_ptr(), sp + 8,
                                               e.adam_out.data_ptr(), *e.sched.extra_launch_args())
                if out.op_buffers:   # the overlap plan declares what its ops touch
                    gb = {f"grad:{b}" for b in range(len(e.buckets))}
                    pb = {f"param:{b}" for b in range(len(e.buckets))}
                    if clip:
                        out.op_buffers[i0] = gb | {"clip"}
                        out.op_buffers[i0 + 1] = {"clip"}
                    if lamb:
                        out.op_buffers[lamb[0]] = (gb | pb | {"adam", "lamb", "gstep"}
                                                   | ({"clip"} if clip else set()))
                        out.op_buffers[lamb[1]] = {"lamb"}
                        out.op_buffers[i1] = pb | {"adam", "lamb", "lr", "gstep"}
                    else:
                        out.op_buffers[i1] = (gb | pb | {"adam", "lr", "gstep"}
                                              | ({"clip"} if clip else set()))
            elif e.lion:
                # one launch (csrc/lion.hip), as adamw's: with clipping the norm launches go in
                # front and the update reads the scale from the device slot
                clip, co = e.clip_grad_norm > 0, 0
                i0 = plan.size()
                if clip:
                    co = e.clip_out.data_ptr()
                    plan.grad_sqnorm(grad, e.params.n_train, e.clip_part.data_ptr())
                    plan.clip_scale(e.clip_part.data_ptr(), e.clip_chunks,
                                    float(np.float32(e.clip_grad_norm)), co)
                i1 = plan.lion_update_pack(master, grad, mom, e.params.n_train,
                                           *e.sched.launch_args(), e.gstep.data_ptr(),
                                           e.lion_beta1, e.lion_beta2, 1.0, co,
                                           e.segs.data_ptr(), e.nseg, e.lion_wd.data_ptr(),
                                           e.wbf.data_ptr(), sp + 8, *e.sched.extra_launch_args())
                if out.op_buffers:   # the overlap plan declares what its ops touch
                    gb = {f"grad:{b}" for b in range(len(e.buckets))}
                    pb = {f"param:{b}" for b in range(len(e.buckets))}
                    if clip:
                        out.op_buffers[i0] = gb | {"clip"}
                        out.op_buffers[i0 + 1] = {"clip"}
                    out.op_buffers[i1] = (gb | pb | {"lr", "gstep"}
                                          | ({"clip"} if clip else set()))
            elif e.rmsprop:
                # one launch (csrc/rmsprop.hip), as adamw's: with clipping the norm launches go
                # in front and the update reads the scale from the device slot
                clip, co = e.clip_grad_norm > 0, 0
                i0 = plan.size()
                if clip:
                    co = e.clip_out.data_ptr()
                    plan.grad_sqnorm(grad, e.params.n_train, e.clip_part.data_ptr())
                    plan.clip_scale(e.clip_part.data_ptr(), e.clip_chunks,
                                    float(np.float32(e.clip_grad_norm)), co)
                i1 = plan.rmsprop_update_pack(
                    master, grad, e.rms_ms.data_ptr(),
                    e.rms_mg.data_ptr() if e.rmsprop_centered else 0, mom, e.params.n_train,
                    *e.sched.launch_args(), e.gstep.data_ptr(), e.rmsprop_rho,
                    e.rmsprop_momentum, e.rmsprop_epsilon, 1.0, co, int(e.rmsprop_centered),
                    e.rmsprop_wd, e.segs.data_ptr(), e.nseg, e.rmsprop_wd_seg.data_ptr(),
                    e.wbf.data_ptr(), sp + 8, *e.sched.extra_launch_args())
                if out.op_buffers:   # the overlap plan declares what its ops touch
                    gb = {f"grad:{b}" for b in range(len(e.buckets))}
                    pb = {f"param:{b}" for b in range(len(e.buckets))}
                    if clip:
                        out.op_buffers[i0] = gb | {"clip"}
                        out.op_buffers[i0 + 1] = {"clip"}
                    out.op_buffers[i1] = (gb | pb | {"rmsprop", "lr", "gstep"}
                                          | ({"clip"} if clip else set()))
            elif e.clip_grad_norm > 0:
                # as for lars: grad is complete here and every other stream is joined, so
                # every rank forms the same norm from the same bits
                co = e.clip_out.data_ptr()
                i0 = plan.grad_sqnorm(grad, e.params.n_train, e.clip_part.data_ptr())
                plan.clip_scale(e.clip_part.data_ptr(), e.clip_chunks,
                                float(np.float32(e.clip_grad_norm)), co)
                plan.sgd_clip_update_pack(master, grad, mom, e.params.n_train,
                                          *e.sched.launch_args(), e.gstep.data_ptr(), e.momentum,
                                          e.wd, co, int(e.use_momentum), e.segs.data_ptr(),
                                          e.nseg, e.wbf.data_ptr(), sp + 8,
                                          *e.sched.extra_launch_args())
                if out.op_buffers:   # the overlap plan declares what its ops touch
                    gb = {f"grad:{b}" for b in range(len(e.buckets))}
                    out.op_buffers[i0] = gb | {"clip"}
                    out.op_buffers[i0 + 1] = {"clip"}
                    out.op_buffers[i0 + 2] = (gb | {f"param:{b}" for b in range(len(e.buckets))}
                                              | {"clip", "lr", "gstep"})
            else:
                plan.sgd_update_pack(master, grad, mom, e.params.n_train, *e.sched.launch_args(),
                                     e.gstep.data_ptr(), e.momentum, e.wd, 1.0, int(e.use_momentum),
                                     e.segs.data_ptr(), e.nseg, e.wbf.data_ptr(), sp + 8, 1,
                                     *e.sched.extra_launch_args())
            plan.ohwi_pack(master, e.segs.data_ptr(), e.ohwi_tile0.data_ptr(), e.nseg,
                           e.ohwi_tiles, e.wbf.data_ptr(), e.gstep.data_ptr())   # + global_step += 1
        if e.stem_s2d:
            plan.stem_s2d_pack(e.stem_master, e.stem_w4.data_ptr(), spec.stem.cout)
        if e.ema is not None:
            # the shadows follow the step's last update and its global_step += 1 (k = steps
            # completed); main stream, every other stream joined: ordinary in-order work
            i = plan.ema_update(master, e.ema.data_ptr(), e.params.n_train, e.gstep.data_ptr(),
                                float(np.float32(1.0 - e.ema_decay)), int(e.ema_warmup))
            if out.op_buffers:   # the overlap plan declares what its ops touch
                out.op_buffers[i] = ({f"param:{b}" for b in range(len(e.buckets))}
                                     | {"ema", "gstep"})
        out.t_opt_end = plan.timing_point("opt_end")
        out.seg["opt"] = (b2, plan.size())
        # 1/2 sum v^2 of the weights, which only feeds the logged `cost`
        # (resnet_model.py:85-86; the gradient's wd*v is fused into the optimizer):
        # its own segment, run before the forward of the steps whose metrics are read
        # (step(need_cost=True); ImageNet RN50: 25.5 M floats, ~0.1 ms per step saved
        # on every other step).
        b3 = plan.size()
        plan.l2_half_sum(master, e.params.n_train, e.l2_ws.data_ptr(), sp + 12)
        out.seg["cost"] = (b3, plan.size())
        missing = [s.name for s in e.params.train_slots if s.name not in out.ready_index]
        assert not missing, f"gradients never produced: {missing[:4]}"

    # ------------------------------------------------------------------ the plans
    def _record_input(self, zero):
        """The step's input launch, which also clears `zero` = (pointer, bytes): the BN accumulators
        (and the persistent step's pool sums and barrier region) start every step at zero.  Input
        modes without a launch of their own get a memset, when there is something to clear."""
        e, plan, spec = self.e, self.plan, self.e.spec
        H, W = spec.image_h, spec.image_w
        # mixup on: the ops' trailing arguments (lam table, [labels,] labels_b, mix_lam, log);
        # CutMix on: three more (box-size table, threshold, log)
        cut = () if e.cut_table is None else (e.cut_table.data_ptr(), e.cut_thresh,
                                              e.cut_log.data_ptr())
        mix = lambda *labels: (  # noqa: E731
            () if e.mix_table is None else
            (e.mix_table.data_ptr(), e.mix_table.numel(), *labels, e.labels_b.data_ptr(),
             e.mix_lam.data_ptr(), e.mix_log.data_ptr(), *cut))
        if e.input_mode == "cifar_u8":
            plan.cifar_augment(e.img_u8.data_ptr(), e.x_in.data_ptr(), e.N, H, W, e.cpad_in, 4,
                               e.data_seed, e.gstep.data_ptr(), 1, 0, *zero,
                               *mix(e.labels.data_ptr()))
        elif e.input_mode == "cifar_resident":
            # records and labels are picked on the device from global_step, so the step
            # (and its hipGraph) needs nothing from the host
            plan.cifar_augment_resident(
                e.records_u8.data_ptr(), e.labels_all.data_ptr(), e.x_in.data_ptr(),
                e.labels.data_ptr(), e.gstep.data_ptr(), e.N, H, W, e.cpad_in, e.records,
                e.rank, e.world, 1, e.shuffle_seed & (2 ** 64 - 1), 4, e.data_seed, 1, 0, 0,
                *zero, *mix())
        elif e.input_mode == "imagenet_u8":
            plan.imagenet_u8_pack(e.img_u8.data_ptr(), e.x_in.data_ptr(), e.N, H, W,
                                  e.data_seed, e.gstep.data_ptr(), 1, *zero, int(e.stem_s2d),
                                  *mix(e.labels.data_ptr()))
        elif zero[0]:
            plan.memset(*zero)
        self._erase_op = None
        if e.erase_tab is not None:
            # Random Erasing: a launch of its own on the main stream, directly behind the input
            # launch and before the forward, so every input kernel above stays as it is
            noise = e.erase_noise
            self._erase_op = plan.erase_boxes(
                e.x_in.data_ptr(), e.N, H, W, e.cpad_in, int(e.stem_s2d), e.data_seed,
                e.gstep.data_ptr(), e.erase_tab.data_ptr(), e.erase_tab.numel(), e.erase_thresh,
                noise.data_ptr() if noise is not None else 0,
                noise.numel() if noise is not None else 0, e.erase_log.data_ptr())

    def record_layers(self) -> RecordedStep:
        """The launch-per-layer step."""
        e, plan, out = self.e, self.plan, self.out
        b0 = plan.size()
        out.t_fwd0 = plan.timing_point("fwd_begin")
        # no accumulator mode on: nothing to clear
        self._record_input((e.bn_acc.data_ptr(), e.bn_acc.numel() * 8)
                           if (e.bn_acc_on or e.bn_bacc_on) else (0, 0))
        self._forward()
        dact = self._head()
        out.seg["fwd"] = (b0, plan.size())
        b1 = plan.size()
        out.t_bwd0 = plan.timing_point("bwd_begin")
        self._backward(dact)
        out.t_bwd_done = plan.timing_point("bwd_compute_done")
        self._join_comm()
        out.t_joined = plan.timing_point("allreduce_joined")
        out.seg["bwd"] = (b1, plan.size())
        self._emit_optimizer()
        return out

    def _forward(self):
        """Stem (+ max-pool) and the residual blocks, up to the last block's output."""
        e, plan, spec, N = self.e, self.plan, self.e.spec, self.e.N
        st, blocks = spec.stem, spec.blocks
        stem, first_bn = e.convs[st.name], e.bns[blocks[0].bns[0].name]
        if spec.maxpool:
            self._conv_fwd(stem, e.x_in, e.stem_out, N)
            geom = e._maxpool_geom(N)
            plan.maxpool_fwd(e.stem_out.data_ptr(), e.pool_out.data_ptr(),
                             e.pool_arg.data_ptr(), geom, 3)
            M = N * geom[4] * geom[5]
            plan.bn_stats(e.pool_out.data_ptr(), M, st.cout, first_bn.part.data_ptr())
            T = e.nat.bn_bwd_tiles(M, st.cout)
            rows = e.nat.bn_stats_tile_rows()
            first_bn.pending = (first_bn.part.data_ptr(), T, rows, M)
            if T > e._consumer_cap(st.cout):
                first_bn.pending = ("separate",) + first_bn.pending
        else:
            self._conv_fwd(stem, e.x_in, e.stem_out, N, stats_for=first_bn)
        for i, b in enumerate(blocks):
            X, Xn = e.X[i], e.X[i + 1]
            bns = [e.bns[s.name] for s in b.bns]
            convs = [e.convs[c.name] for c in b.convs]
            nxt = e.bns[blocks[i + 1].bns[0].name] if i + 1 < len(blocks) else \
                e.bns[spec.final_bn.name]
            self._bn_finalize(bns[0])
            residual = X
            if b.proj is not None:
                pc = e.convs[b.proj.name]
                sc = e.sc_buf[:N * b.ho * b.wo * b.cout].view(N, b.ho, b.wo, b.cout)
                self._conv_fwd(pc, X, sc, N, pre=bns[0])
                residual = sc
            self._conv_fwd(convs[0], X, e.H1[i], N, pre=bns[0], stats_for=bns[1])
            if b.kind == "building":
                self._bn_finalize(bns[1])
                self._conv_fwd(convs[1], e.H1[i], Xn, N, pre=bns[1], residual=residual,
                               stats_for=nxt)
            else:
                a1, p1 = self._bn_input(bns[1], e.H1[i], e.Y1[i])
                self._conv_fwd(convs[1], a1, e.H2[i], N, pre=p1, stats_for=bns[2])
                a2, p2 = self._bn_input(bns[2], e.H2[i], e.Y2[i])
                self._conv_fwd(convs[2], a2, Xn, N, pre=p2, residual=residual, stats_for=nxt)

    def _head(self):
        """Final BN-ReLU + average pool + dense + softmax cross-entropy.  Returns the
        gradient buffer of the last block's output's BN-ReLU (the fused head fills it)."""
        e, plan, spec, N = self.e, self.plan, self.e.spec, self.e.N
        fbn, XL, sp = e.bns[spec.final_bn.name], e.X[-1], e.scalars.data_ptr()
        HL, WL, F = XL.shape[1:]
        # Small (CIFAR) heads: ONE launch for final BN finalize + BN-ReLU-avgpool + dense +
        # softmax-xent rows + dense dgrad + avgpool backward + the final BN's backward
        # sums (head_fused, head.hip) instead of 8 dependent launches; the batch folds
        # (loss, precision, dbias) and the dense wgrad go to the side stream.
        self.out.head_fused = (e.bn_acc_on and e.bn_bacc_on and fbn.pending is not None
                               and fbn.pending[0] == "acc" and e.fused_head
                               and e.nat.head_fused_supported(N, HL * WL, F, spec.num_classes,
                                                              e.kpad))
        dact = self._g((N, HL, WL, F))
        if self.out.head_fused:
            fbn.pending = None
            plan.head_fused(XL.data_ptr(),
                            [fbn.acc.data_ptr(), fbn.gamma, fbn.beta, fbn.mmean, fbn.mvar,
                             *fbn.stat_ptrs()], BN_DECAY, BN_EPS, 1, e.dense_hwio,
                            e.dense_bias, e.labels.data_ptr(),
                            [N, HL * WL, F, spec.num_classes, e.kpad], 1.0 / e.global_batch,
                            [e.pooled.data_ptr(), e.dlogits.data_ptr(),
                             e.xent_ws.data_ptr(), dact.data_ptr(), fbn.bacc.data_ptr()],
                            e.label_smoothing, e.topk, *e.mix_head_ptrs())
        else:
            self._bn_finalize(fbn, consumer_conv=False)   # consumer: bnrelu_avgpool
            plan.bnrelu_avgpool(XL.data_ptr(), fbn.scale.data_ptr(), fbn.shift.data_ptr(),
                                e.pooled.data_ptr(), N, HL * WL, F)
            plan.conv_gemm(0, e.pooled.data_ptr(), e.dense_ohwi, 0, e.logits.data_ptr(),
                           0, 0, 0, e.dense_bias, spec.num_classes, 0, 0, e._dense_geom(N),
                           [], [], [], [], [], BN_DECAY, BN_EPS, 1)
            plan.softmax_xent(e.logits.data_ptr(), e.kpad, e.labels.data_ptr(), N,
                              spec.num_classes, sp, sp + 4, e.dlogits.data_ptr(),
                              e.dense_bias_grad, 1.0 / e.global_batch, 0, e.xent_ws.data_ptr(),
                              e.label_smoothing, e.topk, sp + 20, *e.mix_head_ptrs())
        return dact

    def _backward(self, dact):
        """The hand-scheduled reverse pass, from the head to the stem's weight gradient,
        with every bucket's reduce (and all-reduce) emitted."""
        e, plan, spec, N = self.e, self.plan, self.e.spec, self.e.N
        blocks, fbn, XL, sp = spec.blocks, e.bns[spec.final_bn.name], e.X[-1], e.scalars.data_ptr()
        HL, WL, F = XL.shape[1:]
        head_fused = self.out.head_fused
        # the dense wgrad below runs on the main stream (unless the head is fused)
        self._main_wgrad = e.fork_wgrad and not head_fused
        dg = e._dense_geom(N)
        off, spl, pps = e.wg_off["dense"]
        dpart = e.wg_part.data_ptr() + 4 * off
        dense_wgrad = lambda: plan.conv_wgrad(e.dlogits.data_ptr(),  # noqa: E731
                                              e.pooled.data_ptr(), 0, 0, dpart, dg, spl, pps)
        self._pending[e.dense_name] = (dpart, e.dense_grad, spl, e.kpad, spec.num_classes, 1,
                                       F, F)
        dout = self._g(tuple(XL.shape))
        if head_fused:
            # batch folds of the head's rows (loss, precision, dbias) and the dense
            # weight gradient: side stream; the final BN backward is pending on its
            # accumulator sums for the first dgrad's BN-backward prologue
            xr = lambda: plan.softmax_xent_reduce(  # noqa: E731
                e.xent_ws.data_ptr(), e.kpad, N, spec.num_classes, sp, sp + 4,
                e.dense_bias_grad, sp + 20)
            if e.fork_wgrad:
                self._side_q += [xr, dense_wgrad]
            else:
                xr()
                dense_wgrad()
            self._bnb_src = (fbn.bacc.data_ptr(), -1)
            self._bn_bwd(fbn, dact, XL, dout, reduced=True)
        else:
            dense_wgrad()
            plan.conv_gemm(1, e.dlogits.data_ptr(), e.dense_hwio, e.dpooled.data_ptr(), 0,
                           0, 0, 0, 0, 0, 0, 0, dg, [], [], [], [], [], BN_DECAY, BN_EPS, 1)
            plan.avgpool_bwd(e.dpooled.data_ptr(), dact.data_ptr(), N, HL * WL, F)
            self._bn_bwd(fbn, dact, XL, dout)
        main_tail = []
        for i in range(len(blocks) - 1, -1, -1):
            b = blocks[i]
            X = e.X[i]
            bns = [e.bns[s.name] for s in b.bns]
            convs = [e.convs[c.name] for c in b.convs]
            # the inner convs, last first (a bottleneck's 3x3 and expanding 1x1, a building
            # block's second 3x3); wgrad inputs: the materialized BN-ReLU output (Y), or
            # the BN input + PRE
            dcur = dout
            for j in range(len(convs) - 1, 0, -1):
                h, y = (e.H1[i], e.Y1[i]) if j == 1 else (e.H2[i], e.Y2[i])
                a, p = (y, None) if y is not None else (h, bns[j])
                da = self._g(tuple(h.shape))
                self._conv_bwd(convs[j], dcur, a, N, p, dx=da, bnb=(bns[j], h))
                dcur = self._g(tuple(h.shape))
                self._bn_bwd(bns[j], da, h, dcur, reduced=True)
            proj = b.proj is not None
            dx = self._g(tuple(X.shape))
            if not proj and b.kind != "building" and self._bap_ok(convs[0], N):
                # identity bottleneck: conv1's dgrad emits BNbwd(.) + dout itself
                self._conv_bwd(convs[0], dcur, X, N, bns[0], dx=dx, bap=(bns[0], dout))
            else:
                da1 = self._g(tuple(X.shape))
                self._conv_bwd(convs[0], dcur, X, N, bns[0], dx=da1,
                               bnb=None if proj else (bns[0], X))
                if proj:
                    self._conv_bwd(e.convs[b.proj.name], dout, X, N, bns[0], dx=da1,
                                   accumulate=True, bnb=(bns[0], X))
                self._bn_bwd(bns[0], da1, X, dx, add=None if proj else dout, reduced=True)
            dout = dx
            if i == 0 and e.split_tail:
                main_tail = self._split_tail()
                continue
            # the last block's weight gradients go out now so they overlap the stem's
            # backward (max-pool gather) instead of queueing behind it
            self._flush_side(force=i == 0)
            self._flush_buckets()
        # stem (no dgrad: the input needs no gradient)
        self._emit_bn_bwd()     # the stem's consumers (maxpool_bwd / wgrad) are not fusing
        if spec.maxpool:
            dstem = self._g(tuple(e.stem_out.shape))
            plan.maxpool_bwd(e.pool_arg.data_ptr(), dout.data_ptr(), dstem.data_ptr(),
                             e._maxpool_geom(N), 3)
            dout = dstem
        # The stem's weight gradient is the main stream's last op (nothing else is
        # left for it), running alongside the side stream's last weight gradients.
        self._conv_bwd(e.convs[spec.stem.name], dout, e.x_in, N, None, side=False)
        if main_tail:   # the main stream's share of the tail; the reduces fork after it
            self._emit_wgrads(main_tail)
            self._main_wgrad = True
        if e.split_tail and e.reduce_main_tail:
            # the remaining reduces run on the main stream after ONE join of the side
            # stream, instead of a fork to the side and a join back per bucket
            self._flush_side(force=False)   # (the queue is empty after the split)
            self._join(1)
            self._main_wgrad = False
            self._reduce_main = True
        self._flush_side(force=True)
        self._flush_buckets(force=True)

    def record_persistent(self) -> RecordedStep:
        """The persistent small-batch step (train/persist.py): input, ONE forward launch;
        ONE backward launch (dgrad chain + BN backward on the image row-slice workgroups,
        the weight gradients on the remaining CUs); the head's batch folds; on one GPU
        the optimizer launch (sum of the weight-gradient slabs included), else the
        grouped slab reduce, ONE all-reduce and the optimizer."""
        e, plan, out = self.e, self.plan, self.out
        b0 = plan.size()
        out.t_fwd0 = plan.timing_point("fwd_begin")
        # BN accumulators, the pool sums and the two barrier counters start every step at zero
        self._record_input((e.bn_acc.data_ptr(), e.bn_acc.numel() * 8))
        plan.prn(0, e.prn.args(e.prn_pool, e.prn_bar, BN_DECAY, BN_EPS, fwd=True))
        args = e.prn.args(e.prn_pool, e.prn_bar, BN_DECAY, BN_EPS)
        out.seg["fwd"] = (b0, plan.size())

        b1 = plan.size()
        out.t_bwd0 = plan.timing_point("bwd_begin")
        self._pending = dict(e.prn.pending())
        self._produced |= set(self._pending)
        self._reduce_main = True   # the slab reduces run on the main stream
        if e.prn.overlap:
            early = self._emit_persist_overlap(args)
            if self._erase_op is not None and out.op_buffers:
                out.op_buffers[self._erase_op] = {"input"}   # the overlap plan declares its ops
            out.seg["bwd"] = (b1, plan.size())
            if e.opt_fused:   # the rest: the last bucket's segments
                self._emit_optimizer(fused_slabs={}, gin=self._packed_gin(),
                                     names={n for n in e.seg_names if n not in early})
            else:
                self._emit_optimizer()
            return out
        plan.prn(1, args)
        # the head's batch folds (loss, precision, dense bias and weight gradients): one
        # workgroup on the main stream -- no side stream, no fork/join events
        plan.prn(2, args)
        # every slab is complete when the backward launch ends, and that launch holds
        # every CU (nothing can overlap it): ONE grouped reduce of all the slabs, then
        # (world > 1) ONE all-reduce of the whole gradient -- the per-bucket launches of
        # the per-layer plan only pay off when they overlap a backward (bs16: 6 reduce
        # launches 32 us vs 1).  With nothing to all-reduce and opt_fused, the slabs are
        # summed by the optimizer launch itself (sgd_tiles).
        all_names = [n for (_, _, names) in e.buckets for n in names]
        slabs = None
        packed = e.comm is not None and e.opt_fused
        if e.opt_fused and not e.reduce_buckets:
            slabs = {n: self._pending.pop(n) for n in all_names if n in self._pending}
        elif packed:   # the all-reduce input in one launch, read back by the optimizer
            self._emit_pack(all_names)
        else:
            self._emit_reduce(all_names)
        for bi, (lo, hi, names) in enumerate(e.buckets):
            self._mark(*names)
            self._flushed.add(bi)
        if e.comm is not None:
            self._emit_allreduce(min(b[0] for b in e.buckets), max(b[1] for b in e.buckets),
                                 side_dep=False, on_main=True, packed=packed)
        out.t_bwd_done = plan.timing_point("bwd_compute_done")
        self._join_comm()
        out.t_joined = plan.timing_point("allreduce_joined")
        out.seg["bwd"] = (b1, plan.size())
        self._emit_optimizer(fused_slabs=(slabs or {}) if e.opt_fused else None,
                             gin=self._packed_gin() if packed else 0)
        if slabs:
            # not part of the step: the slab sums alone, for callers that want this
            # step's gradient without the update (forward_backward)
            b4 = plan.size()
            self._pending.update(slabs)
            self._emit_reduce(list(slabs))
            out.seg["gsum"] = (b4, plan.size())
        return out

    def _emit_persist_overlap(self, args):
        """World > 1: the persistent backward launch on the main stream, and on the comm
        stream (forked before it): the head's batch folds, then per gradient bucket but the
        last, in the order the backward completes them (persist.bucket_ranges), a one-wave
        wait for the bucket's line in the launch's barrier region to reach its count, the
        bucket's pack (or grouped slab reduce), its all-reduce and (opt_fused) the update of
        its parameters -- all while the backward still runs on the CUs left out of its
        grid.  The main stream joins the comm stream right after the backward (its buckets
        are long done by then) and packs, all-reduces and updates the last bucket itself.
        The stream check takes each bucket wait as a PARTIAL dependency on the backward
        launch (device_deps with the buffers it covers: the bucket's gradients / slabs and
        parameters, which the launch publishes complete and no longer reads once the count
        is reached, plus the lr slot and global step the launch never touches), and holds
        every comm-stream op before the join to the buffers it declares (op_buffers, R5).
        Returns the segment names updated on the comm stream."""
        from .persist import bucket_ranges

        e, plan, out = self.e, self.plan, self.out
        fork = plan.new_event()
        plan.record(fork)
        plan.use_stream(2)
        plan.wait(fork)
        plan.prn(2, args)        # head folds (loss, precision, dense grads)
        plan.use_stream(0)
        bwd_op = plan.size()
        plan.prn(1, args)        # backward: dgrad chain + weight gradients
        err = e.prn.err.data_ptr()
        ranges = bucket_ranges(e)

        def declare(a0, bset):
            for i in range(a0, plan.size()):
                out.op_buffers[i] = set(bset)

        def bucket(b, lo, hi, names, stream):
            a0 = plan.size()
            if e.opt_fused:
                self._emit_pack(names, stream=stream)
            else:
                self._emit_reduce(names, stream=stream)
            plan.use_stream(stream)
            self._mark(*names)
            self._emit_allreduce(lo, hi, side_dep=False, on_main=True, packed=e.opt_fused)
            declare(a0, {f"grad:{b}"})

        early = set()
        for b, (lo, hi, names) in enumerate(ranges[:-1]):
            plan.use_stream(2)                 # (_emit_reduce/_emit_allreduce end on main)
            out.device_deps[plan.size()] = (bwd_op, {f"grad:{b}", f"param:{b}", "lr", "gstep"})
            plan.prn_bucket_wait(e.prn_bar, b, e.prn.bucket_target(b), err)
            bucket(b, lo, hi, names, 2)
            if e.opt_fused:
                # the bucket's parameters updated right behind its all-reduce, still beside
                # the backward: it has finished with them (their stage's dgrads and BN
                # backwards precede the count that released this bucket); global_step is
                # stepped by the last update launch
                plan.use_stream(2)
                a0 = plan.size()
                self._emit_update(set(names), self._packed_gin(), step=False)
                declare(a0, {f"grad:{b}", f"param:{b}", "lr", "gstep"})
                plan.use_stream(0)
                early |= set(names)
        self._join(2)
        out.t_bwd_done = plan.timing_point("bwd_compute_done")
        bucket(len(ranges) - 1, *ranges[-1], 0)   # the last bucket behind the backward, in order
        for bi in range(len(e.buckets)):
            self._flushed.add(bi)
        out.t_joined = plan.timing_point("allreduce_joined")
        return early
