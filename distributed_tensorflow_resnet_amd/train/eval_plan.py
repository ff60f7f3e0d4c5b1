"""Inference forward plans of the engine (Engine.build_eval_plan)."""
from __future__ import annotations

import torch

from ..data.cifar import upload_resident
from .engine import BF16, BN_DECAY, BN_EPS


class _EvalPlan:
    """Inference forward (resnet_cifar_main.py:361-421 evaluate()): batch-norm
    with moving statistics, no statistics update, softmax probabilities."""

    def __init__(self, eng, N: int, persist: bool = False):
        self.eng = eng
        self.N = N
        self.kind = "persistent" if persist else "per-layer"
        nat, spec, dev = eng.nat, eng.spec, eng.device
        H, W = spec.image_h, spec.image_w
        self.img_u8 = torch.zeros((N, 3, H, W), dtype=torch.uint8, device=dev)
        self.x_in = torch.zeros(eng._x_in_shape(N), dtype=BF16, device=dev)
        self.labels = torch.zeros(N, dtype=torch.int32, device=dev)
        self.probs = torch.zeros((N, eng.kpad), device=dev)
        self.xent_ws = torch.empty(eng.nat.softmax_xent_ws_floats(N, eng.kpad), device=dev)
        self.logits = torch.zeros((N, eng.kpad), device=dev)
        self.scalars = torch.zeros(4, device=dev)   # loss_sum, correct, in-top-5 count
        self.top5 = 0.0   # the last run's in-top-5 count (tf.nn.in_top_k, k = min(5, classes))
        p = nat.Plan()
        self.plan = p
        self.input_plan = nat.Plan()
        self.resident_plan = None   # attach(): the input plan of a device-resident split
        if not eng.stem_s2d:   # raw uint8 CIFAR records (run(raw_u8=True))
            self.input_plan.cifar_augment(self.img_u8.data_ptr(), self.x_in.data_ptr(), N, H, W,
                                          eng.cpad_in, 4, 0, 0, 0, 0, 0, 0)
        if persist:
            # ONE launch from the images to the fp32 logits (no per-BN scale / shift
            # buffer, no activation tensor: nothing the training plan owns is written)
            from .persist import PersistInfer
            self.prn = PersistInfer(eng)
            self.prn.record(p, self.x_in, self.logits, N, BN_EPS)
            self._bufs = []
        else:
            self._record_layers(p)
        sp = self.scalars.data_ptr()
        # evaluation is never smoothed: the loss stays comparable across training recipes
        p.softmax_xent(self.logits.data_ptr(), eng.kpad, self.labels.data_ptr(), N,
                       spec.num_classes, sp, sp + 4, 0, 0, 1.0, self.probs.data_ptr(),
                       self.xent_ws.data_ptr(), 0.0, min(5, spec.num_classes), sp + 8)

    def attach(self, images, labels):
        """Keep a whole eval split (uint8 [M,3,32,32] + labels) on the device:
        run_resident(i) then scores batch i with no per-batch image copy.  The resident
        input plan reads the batch index from `batch_pos`, an int64 counter this plan
        owns, unshuffled -- positions at or past the end of the split (the tail batch)
        read the batch's first record, the padding GPUInference.run gives a short batch."""
        eng, N = self.eng, self.N
        if eng.stem_s2d:
            raise ValueError("resident eval split: CIFAR records only")
        self.records_u8, self.labels_all = upload_resident((images, labels), eng.spec, eng.device)
        self.records = int(self.records_u8.shape[0])
        self.batch_pos = torch.zeros(1, dtype=torch.int64, device=eng.device)
        self.resident_plan = eng.nat.Plan()
        self.resident_plan.cifar_augment_resident(
            self.records_u8.data_ptr(), self.labels_all.data_ptr(), self.x_in.data_ptr(),
            self.labels.data_ptr(), self.batch_pos.data_ptr(), N, eng.spec.image_h,
            eng.spec.image_w, eng.cpad_in, self.records, 0, 1, 0, 0, 4, 0, 0, 0, 0, 0, 0)

    @property
    def resident_batches(self) -> int:
        """Batches of the attached split, the tail batch included."""
        return -(-self.records // self.N)

    def run_resident(self, batch_index: int):
        """run() on batch `batch_index` of the attached split (see attach)."""
        if not 0 <= batch_index < self.resident_batches:
            raise IndexError(f"batch {batch_index} of {self.resident_batches}")
        st = torch.cuda.current_stream().cuda_stream
        self.batch_pos.fill_(batch_index)   # a device fill: no synchronous copy
        self.resident_plan.run(0, self.resident_plan.size(), st, 0)
        return self.run()

    def _record_layers(self, p):
        """The launch-per-layer forward: bn_eval per BatchNorm, conv_gemm per conv, pool,
        dense -> self.logits."""
        eng, N = self.eng, self.N
        spec, dev = eng.spec, eng.device
        st = spec.stem
        stem = eng.convs[st.name]
        bufs = []

        def buf(shape):
            t = torch.empty(shape, dtype=BF16, device=dev)
            bufs.append(t)
            return t

        for bn in eng.bns.values():
            p.bn_eval(bn.gamma, bn.beta, bn.mmean, bn.mvar, BN_EPS, bn.spec.channels,
                      bn.scale.data_ptr(), bn.shift.data_ptr())
        y = buf((N, st.ho, st.wo, st.cout))
        p.conv_gemm(0, self.x_in.data_ptr(), stem.ohwi, y.data_ptr(), 0, 0, 0, 0, 0, 0, 0, 0,
                    eng._geom(stem, N), [], [], [], [], [], BN_DECAY, BN_EPS, 1)
        if spec.maxpool:
            geom = eng._maxpool_geom(N)
            z = buf((N, geom[4], geom[5], st.cout))
            p.maxpool_fwd(y.data_ptr(), z.data_ptr(), 0, geom, 3)
            y = z
        x = y
        for b in spec.blocks:
            bns = [eng.bns[s.name] for s in b.bns]
            convs = [eng.convs[c.name] for c in b.convs]
            res = x
            if b.proj is not None:
                pc = eng.convs[b.proj.name]
                res = buf((N, b.ho, b.wo, b.cout))
                self._conv(p, pc, x, res, bns[0])
            h = x
            for j, c in enumerate(convs):
                last = j == len(convs) - 1
                o = buf((N, c.spec.ho, c.spec.wo, c.spec.cout))
                self._conv(p, c, h, o, bns[j], residual=res if last else None)
                h = o
            x = h
        fbn = eng.bns[spec.final_bn.name]
        F = spec.dense_in
        self.pooled = torch.empty((N, F), dtype=BF16, device=dev)
        p.bnrelu_avgpool(x.data_ptr(), fbn.scale.data_ptr(), fbn.shift.data_ptr(),
                         self.pooled.data_ptr(), N, x.shape[1] * x.shape[2], F)
        p.conv_gemm(0, self.pooled.data_ptr(), eng.dense_ohwi, 0, self.logits.data_ptr(), 0, 0, 0,
                    eng.dense_bias, spec.num_classes, 0, 0, eng._dense_geom(N), [], [], [], [], [],
                    BN_DECAY, BN_EPS, 1)
        self._bufs = bufs

    def _conv(self, p, c, x, out, pre, residual=None):
        p.conv_gemm(0, x.data_ptr(), c.ohwi, out.data_ptr(), 0,
                    0 if residual is None else residual.data_ptr(), pre.scale.data_ptr(),
                    pre.shift.data_ptr(), 0, 0, 0, 0, self.eng._geom(c, self.N), [], [], [], [],
                    [], BN_DECAY, BN_EPS, 1)

    def run(self, images=None, labels=None, raw_u8: bool = True):
        """Returns (loss_sum, correct, probs[N, classes]) for one eval batch; the batch's
        in-top-5 count is left in ``self.top5``.

        NOTE: the per-layer plan shares the per-BN scale/shift buffers with the
        training plan, so it must not run concurrently with a training step (the
        evaluator runs in its own process, like the reference's side-car).  The
        persistent plan writes only this plan's own logits / probabilities."""
        st = torch.cuda.current_stream().cuda_stream
        if images is not None:
            if raw_u8:
                self.img_u8.copy_(images)
                self.input_plan.run(0, self.input_plan.size(), st, 0)
            else:
                x = images.to(self.eng.device)
                if tuple(x.shape) != tuple(self.x_in.shape):
                    x = self.eng._stem_input(x.float())
                self.x_in.copy_(x.to(BF16))
        if labels is not None:
            self.labels.copy_(labels.to(torch.int32))
        self.plan.run(0, self.plan.size(), st, 0)
        v = self.scalars.cpu().tolist()
        self.top5 = v[2]
        return v[0], v[1], self.probs[:, :self.eng.spec.num_classes]
