"""Execution backends behind TrainingSession.

GPUBackend  the MI355X engine (native plan + HIP kernels + RCCL all-reduce)
CPUBackend  fp32 PyTorch autograd with TF semantics (BASELINE config 1,
            `resnet_single.py`; also runs multi-process data parallel over
            gloo for CPU tests of the distributed logic)
Both expose the same small interface (set_batch / step / metrics /
state_tensors / load_state / broadcast_parameters) and the same TF-named
checkpoint layout, so a run can be resumed on either.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from ..data.cifar import (MIXUP_TABLE_LEN, augment_cpu, cutmix_draw, cutmix_table, cutmix_thresh,
                          erase_draw, erase_noise_index, erase_noise_table, erase_table,
                          erase_thresh, mixup_draw, mixup_table)
from ..models.params import ParamStore
from ..models.resnet_torch import TorchResNet
from ..models.spec import ModelSpec
from ..ops import reference as ref
from ..parallel.dist import local_device_index
from ..utils.checkpoint import (check_rmsprop_form, state_to_tf, tf_to_adam, tf_to_lion,
                                tf_to_rmsprop, tf_to_state)
from .layout import (check_adam_trust, check_lion, check_rmsprop, lamb_bias_corrections, lamb_trust_summary,  # noqa: E501
                     OPTIMIZERS, adam_alpha, adam_decay_table, check_adam, check_clip_grad_norm, check_cutmix_alpha, check_mix_switch_prob,
                     check_mixup_alpha, check_erase)


class GPUBackend:
    def __init__(self, engine, use_graph: bool = False):
        self.engine = engine
        self.use_graph = use_graph
        self._host_step = int(engine.gstep.item())
        self.profile_phases = False
        self.last_phase_ms = None
        self._captured = False
        self._eager_done = False

    @property
    def global_step(self) -> int:
        return self._host_step

    def set_batch(self, images, labels):
        self.engine.set_batch(images, labels)

    def step(self, need_cost: bool = False):
        eng = self.engine
        if self.profile_phases:
            self.last_phase_ms = eng.step_timed(need_cost)
        elif self.use_graph:
            # first step eager (initialises RCCL communicators), second step
            # captures the hipGraph (capture executes nothing) and replays it:
            # exactly one training step per call either way.
            if self._eager_done and not self._captured:
                eng.capture(warmup=0)
                self._captured = True
            eng.step(need_cost)
            self._eager_done = True
        else:
            eng.step(need_cost)
        self._host_step += 1

    def metrics(self, top5: bool = False):
        # rank-local (the session's hooks read metrics on their own schedules, chief-only
        # hooks on the chief only, so a collective here would be joined by nobody -- or,
        # with the c10d transport, by another rank's gradient all-reduce).  Like the
        # reference's per-worker LoggingTensorHook, each rank logs its own batch.
        return self.engine.metrics(reduce=False, top5=top5)

    def synchronize(self):
        torch.cuda.synchronize()

    def check_health(self):
        """Raise (engine.PersistentStepError) if a persistent launch failed: called before
        every checkpoint save, so a half-computed step never reaches a checkpoint."""
        self.engine.check_health()

    def state_tensors(self):
        self.check_health()
        eng = self.engine
        adam = None
        if eng.adam:
            adam = {"v": eng.adam_v, "start_step": int(eng.adam_start.item()),
                    "beta1": eng.adam_beta1, "beta2": eng.adam_beta2}
        rms = {"ms": eng.rms_ms, "mg": eng.rms_mg} if eng.rmsprop else None
        return state_to_tf(eng.params, eng.mom, self.global_step, ema=eng.ema, adam=adam,
                           lion=eng.lion, rmsprop=rms)

    def load_state(self, tensors):
        eng = self.engine
        # adamw: the momentum buffer is the first moment, loaded from the Adam slots
        # (lion: it is m, loaded from the Lion slots; rmsprop: from the RMSProp slots)
        own = eng.adam or eng.lion or eng.rmsprop
        if eng.rmsprop:   # first: a checkpoint of the other form is refused before anything moves
            check_rmsprop_form(tensors, eng.params, eng.rmsprop_centered)
        gs = tf_to_state(tensors, eng.params, None if own else eng.mom, strict=True, ema=eng.ema)
        if eng.rmsprop:   # (after the weights, as the adam and lion slots)
            tf_to_rmsprop(tensors, eng.params, eng.rms_ms, eng.rms_mg, eng.mom)
        if eng.adam:
            eng.set_adam_start(tf_to_adam(tensors, eng.params, eng.mom, eng.adam_v))
        if eng.lion:
            tf_to_lion(tensors, eng.params, eng.mom)
        eng.sync_from_params(ema_loaded=True)
        self._host_step = gs

    def adam_state(self):
        return self.engine.adam_state()

    def rmsprop_state(self):
        return self.engine.rmsprop_state()

    @property
    def ema_decay(self) -> float:
        return self.engine.ema_decay

    def ema_state(self):
        return self.engine.ema_state()

    def lars_summary(self):
        return self.engine.lars_summary()

    def lamb_state(self):
        return self.engine.lamb_state()

    def lamb_summary(self):
        return self.engine.lamb_summary()

    def clip_state(self):
        return self.engine.clip_state()

    def mixup_state(self):
        return self.engine.mixup_state()

    def mix_state(self):
        return self.engine.mix_state()

    def erase_state(self):
        return self.engine.erase_state()

    def broadcast_parameters(self, src: int = 0):
        self.engine.broadcast_parameters(src)
        self._host_step = int(self.engine.gstep.item())


class CPUBackend:
    """fp32 autograd trainer; DP over torch.distributed (gloo) when dist_ctx given."""

    def __init__(self, spec: ModelSpec, batch_size: int, *, weight_decay: float, lr_schedule,
                 optimizer: str = "mom", momentum: float = 0.9, seed: int = 0, dist_ctx=None,
                 global_batch: int | None = None, threads: int = 0,
                 allreduce_dtype: str = "fp32", lars_eeta: float = 0.001,
                 lars_epsilon: float = 0.0, lars_skip: str = "vectors",
                 label_smoothing: float = 0.0, ema_decay: float = 0.0, ema_warmup: bool = True,
                 clip_grad_norm: float = 0.0, mixup_alpha: float = 0.0, data_seed: int = 1234,
                 cutmix_alpha: float = 0.0, mix_switch_prob: float = 0.5,
                 adam_beta1: float = 0.9, adam_beta2: float = 0.999,
                 adam_epsilon: float = 1e-8, adam_decay: str = "decoupled",
                 adam_decay_skip: str = "none", adam_trust="off",
                 adam_trust_skip: str = "vectors", erase_prob: float = 0.0,
                 erase_area_min: float = 0.02, erase_area_max: float = 1.0 / 3.0,
                 erase_aspect_min: float = 0.3, erase_fill: str = "zero",
                 lion_beta1: float = 0.9, lion_beta2: float = 0.99,
                 lion_decay_skip: str = "none", rmsprop_rho: float = 0.9,
                 rmsprop_momentum: float = 0.9, rmsprop_epsilon: float = 1e-10,
                 rmsprop_centered: bool = False, rmsprop_wd: str = "l2",
                 rmsprop_decay_skip: str = "none"):
        # mixup, csrc/data.hip's blend in fp32 torch from the same table and draw (0 = off)
        self.mixup_alpha = check_mixup_alpha(mixup_alpha)
        self.data_seed = data_seed
        self.mix_table = mixup_table(self.mixup_alpha, data_seed) if self.mixup_alpha > 0 else None
        self._mixup_state = None
        # CutMix, the same launches' paste on the augmented fp32 batch (0 = off); with CutMix
        # alone every step pastes and the lam table (all 1, as the engine's) is never read
        self.cutmix_alpha = check_cutmix_alpha(cutmix_alpha)
        self.cut_thresh = cutmix_thresh(self.mixup_alpha, self.cutmix_alpha,
                                        check_mix_switch_prob(mix_switch_prob))
        self.cut_table = None
        if self.cutmix_alpha > 0:
            self.cut_table = cutmix_table(self.cutmix_alpha, data_seed, spec.image_h, spec.image_w)
            if self.mix_table is None:
                self.mix_table = np.ones(MIXUP_TABLE_LEN, dtype=np.float32)
        self._mix_state = None
        self._cut_area = None
        self.last_input = None     # the batch the last step fed the model (mixup / CutMix /
        #                            erasing on)
        # Random Erasing, csrc/erase.hip's boxes on the fp32 batch after its mix, from the same
        # tables and draw (0 = off); the noise values are the fp32 table's
        (self.erase_prob, self.erase_area_min, self.erase_area_max, self.erase_aspect_min,
         self.erase_fill) = check_erase(erase_prob, erase_area_min, erase_area_max,
                                        erase_aspect_min, erase_fill, spec.dataset)
        self.erase_tab = self.erase_noise = self._erase_state = None
        if self.erase_prob > 0:
            self.erase_tab = erase_table(data_seed, spec.image_h, spec.image_w,
                                         self.erase_area_min, self.erase_area_max,
                                         self.erase_aspect_min)
            self.erase_thresh = erase_thresh(self.erase_prob)
            if self.erase_fill == "noise":
                self.erase_noise = erase_noise_table(data_seed)
        # global gradient-norm clipping, csrc/clip.hip's expressions in fp32 torch (0 = off)
        self.clip_grad_norm = check_clip_grad_norm(clip_grad_norm, optimizer)
        self._clip_state = None
        # intra-op threads: DTR_CPU_THREADS, default 1 -- on small containers the
        # OpenMP pool's spin-waits oversubscribe the CPU quota (measured here: one
        # 8x32x32x16 conv fwd+bwd 1.2 ms on 1 thread, 612 ms on 8)
        threads = threads or int(os.environ.get("DTR_CPU_THREADS", "1"))
        if threads > 0:
            torch.set_num_threads(threads)
        self.spec = spec
        self.N = batch_size
        self.dist = dist_ctx
        self.world = dist_ctx.world_size if dist_ctx is not None else 1
        self.global_batch = global_batch or batch_size * self.world
        self.store = ParamStore(spec)
        self.store.initialize(seed)
        self.model = TorchResNet(spec, self.store)
        self.mom = torch.zeros(self.store.n_train)
        # EMA shadows of the trainables: csrc/ema.hip's expressions in fp32 torch
        if not 0.0 <= ema_decay < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay!r}")
        self.ema_decay, self.ema_warmup = float(ema_decay), bool(ema_warmup)
        self.ema = self.store.master.detach().clone() if self.ema_decay > 0 else None
        self.wd = weight_decay
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing!r}")
        self.label_smoothing = float(label_smoothing)
        self.last_logits = None    # the last step's logits (detached)
        self.last_eval_top5 = 0.0  # in-top-5 count of the last evaluate_batch
        self.momentum = momentum
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be mom, sgd, lars, adamw, lion or rmsprop, got {optimizer!r}")
        # adamw, csrc/adam.hip's expressions in fp32 torch: the first moment in `mom`, the
        # second in `adam_v`; t counts from adam_start
        self.adam = optimizer == "adamw"
        self.adam_beta1, self.adam_beta2, self.adam_epsilon = check_adam(
            adam_beta1, adam_beta2, adam_epsilon, adam_decay, adam_decay_skip)
        self.adam_decay = adam_decay
        self.adam_v, self.adam_start, self._adam_state = None, 0, None
        # adam_trust on: LAMB, csrc/lamb.hip's expressions in fp32 torch
        self.lamb = check_adam_trust(adam_trust, adam_trust_skip, optimizer)
        self.adam_trust_skip = adam_trust_skip
        self._lamb_state = None
        if self.adam:
            self.adam_v = torch.zeros(self.store.n_train)
            wd_seg = adam_decay_table([s.shape for s in self.store.train_slots], weight_decay,
                                      adam_decay_skip)
            self.adam_wd = torch.repeat_interleave(
                torch.from_numpy(wd_seg), torch.tensor([s.numel for s in self.store.train_slots]))
        # lion, csrc/lion.hip's expressions in fp32 torch: m in `mom`, nothing else kept
        self.lion = optimizer == "lion"
        self.lion_beta1, self.lion_beta2 = check_lion(lion_beta1, lion_beta2, lion_decay_skip)
        if self.lion:
            wd_seg = adam_decay_table([s.shape for s in self.store.train_slots], weight_decay,
                                      lion_decay_skip)
            self.lion_wd = torch.repeat_interleave(
                torch.from_numpy(wd_seg), torch.tensor([s.numel for s in self.store.train_slots]))
        # rmsprop, csrc/rmsprop.hip's expressions in fp32 torch: its momentum in `mom`, the
        # mean square (from ones) in `rms_ms`, centered the mean gradient in `rms_mg`
        self.rmsprop = optimizer == "rmsprop"
        (self.rmsprop_rho, self.rmsprop_momentum, self.rmsprop_epsilon,
         self.rmsprop_centered) = check_rmsprop(rmsprop_rho, rmsprop_momentum, rmsprop_epsilon,
                                                rmsprop_centered, rmsprop_wd, rmsprop_decay_skip)
        self.rmsprop_wd = rmsprop_wd   # the mode; the per-element decay is rmsprop_wd_seg
        self.rms_ms = self.rms_mg = None
        if self.rmsprop:
            self.rms_ms = torch.ones(self.store.n_train)
            if self.rmsprop_centered:
                self.rms_mg = torch.zeros(self.store.n_train)
            wd_seg = adam_decay_table([s.shape for s in self.store.train_slots], weight_decay,
                                      rmsprop_decay_skip)
            self.rmsprop_wd_seg = torch.repeat_interleave(
                torch.from_numpy(wd_seg), torch.tensor([s.numel for s in self.store.train_slots]))
        if lars_skip not in ("vectors", "none"):
            raise ValueError(f"lars_skip must be vectors or none, got {lars_skip!r}")
        self.lars = optimizer == "lars"
        self.lars_eeta, self.lars_epsilon = float(lars_eeta), float(lars_epsilon)
        self.lars_skip = lars_skip
        self._lars_state = None
        self.use_momentum = optimizer in ("mom", "lars")
        self.sched = lr_schedule
        self.step_count = 0
        self.gen = torch.Generator().manual_seed(seed + 97 * (dist_ctx.rank if dist_ctx else 0))
        self._x = None
        self._y = None
        self._last = {}
        self._last_top5 = 0.0      # in-top-5 fraction of the last step
        self.profile_phases = False
        self.last_phase_ms = None
        if allreduce_dtype not in ("fp32", "bf16"):
            raise ValueError(f"allreduce_dtype must be fp32 or bf16, got {allreduce_dtype!r}")
        self.allreduce_bf16 = allreduce_dtype == "bf16"

    @property
    def global_step(self) -> int:
        return self.step_count

    def set_batch(self, images, labels):
        if images.dtype == torch.uint8:
            images = augment_cpu(images, train=True, generator=self.gen)
        self._x = images.float()
        self._y = labels.long()

    def step(self, need_cost: bool = False):   # the CPU loss always includes the l2 term
        m = self.model
        master = self.store.master
        if master.grad is not None:
            master.grad = None
        x, y, mix = self._x, self._y, {}
        if self.mix_table is not None:
            # one draw per step for the whole batch; the partner of n is (n + shift) % N
            idx, shift = mixup_draw(self.data_seed, self.step_count, self.N, len(self.mix_table))
            d = {"cut": False}
            if self.cut_table is not None:
                d = cutmix_draw(self.data_seed, self.step_count, self.N, len(self.mix_table),
                                x.shape[1], x.shape[2], self.cut_table, self.cut_thresh)
            if d["cut"]:   # a select: the partner's pixels inside the box, its own outside
                lam = torch.tensor(d["lam"])
                box = torch.zeros((x.shape[1], x.shape[2], 1), dtype=torch.bool)   # x is NHWC
                box[d["y0"]:d["y1"], d["x0"]:d["x1"]] = True
                x = torch.where(box, torch.roll(x, -shift, 0), x)
            else:
                lam = torch.tensor(self.mix_table[idx])
                x = lam * x + (1.0 - lam) * torch.roll(x, -shift, 0)
            mix = {"labels_b": torch.roll(y, -shift, 0), "lam": lam}
            self._mixup_state = (float(lam), shift)
            self._mix_state = {"mode": "cutmix" if d["cut"] else "mixup", "lam": float(lam),
                               "shift": shift,
                               "box": (d["y0"], d["y1"], d["x0"], d["x1"]) if d["cut"] else None}
            self._cut_area = d["area"] if d["cut"] else None
            self.last_input = x
            if not float(lam) >= 0.5:   # precision is counted against the dominant label
                y = mix["labels_b"]
        if self.erase_tab is not None:
            x = self._erase(x)
            self.last_input = x
        logits = m(x, True)
        xent, _ = m.loss(logits, self._y, self.wd, self.label_smoothing, **mix)
        # mean over the GLOBAL batch: local mean * (local/global), then sum-allreduce
        (xent * (self.N / self.global_batch)).backward()
        g = master.grad
        if self.dist is not None and self.world > 1:
            if self.allreduce_bf16:   # compressed exchange, fp32 accumulate of the result
                gb = g.to(torch.bfloat16)
                self.dist.all_reduce_sum(gb)
                g = gb.float()
            else:
                self.dist.all_reduce_sum(g)
        lr = self.sched.at(self.step_count)
        with torch.no_grad():
            if self.adam or self.lion or self.rmsprop:
                gp = None   # (its decay is per tensor and per mode: _adam_update, _lion_update,
                #             _rmsprop_update)
            elif self.clip_grad_norm > 0:
                # after the all-reduce: every rank forms the same norm from the same bits
                gp = self._clip_scale(g) * g + self.wd * master
            else:
                gp = g + self.wd * master
            if self.lamb:
                self._lamb_update(master, g, lr)
            elif self.adam:
                self._adam_update(master, g, lr)
            elif self.lion:
                self._lion_update(master, g, lr)
            elif self.rmsprop:
                self._rmsprop_update(master, g, lr)
            elif self.lars:
                self.mom.mul_(self.momentum).add_(gp)
                master.sub_(lr * self._lars_trust(master, g) * self.mom)
            elif self.use_momentum:
                self.mom.mul_(self.momentum).add_(gp)
                master.sub_(lr * self.mom)
            else:
                master.sub_(lr * gp)
            l2 = 0.5 * float((master * master).sum())
            correct = float((logits.argmax(1) == y).float().sum())
            top5 = float(ref.in_top_k(logits, y, 5).float().sum())
            self.last_logits = logits.detach()
        loss_sum = float(xent.detach()) * self.N
        if self.dist is not None and self.world > 1:
            t = torch.tensor([loss_sum, correct, top5])
            self.dist.all_reduce_sum(t)
            loss_sum, correct, top5 = t.tolist()
        n = self.global_batch
        self.step_count += 1
        if self.ema is not None:
            self._ema_update()
        self._last = {"global_step": self.step_count, "cross_entropy": loss_sum / n,
                      "cost": loss_sum / n + self.wd * l2, "precision": correct / n, "lr": lr,
                      "l2": l2}
        self._last_top5 = top5 / n

    def _adam_update(self, master, g, lr):
        """csrc/adam.hip's update in fp32 torch; alpha in fp64 from the step, rounded once."""
        f = lambda x: torch.tensor(x, dtype=torch.float32)   # noqa: E731
        b1, b2, eps = f(self.adam_beta1), f(self.adam_beta2), f(self.adam_epsilon)
        omb1, omb2 = f(1.0 - float(b1)), f(1.0 - float(b2))
        lr32 = f(lr)
        t = max(1, self.step_count - self.adam_start + 1)
        alpha = f(adam_alpha(float(lr32), t, self.adam_beta1, self.adam_beta2))
        w, wd = master, self.adam_wd
        gp = g * self._clip_scale(g) if self.clip_grad_norm > 0 else g.clone()
        if self.adam_decay == "l2":
            gp = gp + wd * w
        dec = (lr32 * wd) * w   # decoupled: of the old w
        self.mom.mul_(b1).add_(omb1 * gp)
        self.adam_v.mul_(b2).add_(omb2 * (gp * gp))
        w.sub_(alpha * (self.mom / (torch.sqrt(self.adam_v) + eps)))
        if self.adam_decay == "decoupled":
            w.sub_(dec)
        self._adam_state = (t, float(alpha))

    def adam_state(self):
        """(t, alpha) of the last step (None: not adamw, or no step yet)."""
        return self._adam_state

    def _lion_update(self, master, g, lr):
        """csrc/lion.hip's update in fp32 torch: every product, sum and difference on its own."""
        f = lambda x: torch.tensor(x, dtype=torch.float32)   # noqa: E731
        b1, b2 = f(self.lion_beta1), f(self.lion_beta2)
        omb1, omb2 = f(1.0 - float(b1)), f(1.0 - float(b2))
        lr32 = f(lr)
        w, m = master, self.mom
        gp = g * self._clip_scale(g) if self.clip_grad_norm > 0 else g.clone()
        c = b1 * m + omb1 * gp
        one = torch.ones_like(c)
        u = torch.where(c > 0, one, torch.where(c < 0, -one, c))   # +-0 and NaN stay
        dec = (lr32 * self.lion_wd) * w   # decoupled: of the old w
        m.copy_(b2 * m + omb2 * gp)
        w.copy_((w - lr32 * u) - dec)

    def _rmsprop_update(self, master, g, lr):
        """csrc/rmsprop.hip's update in fp32 torch: every product, sum, difference, square root
        and quotient on its own."""
        f = lambda x: torch.tensor(x, dtype=torch.float32)   # noqa: E731
        rho, mo, eps = f(self.rmsprop_rho), f(self.rmsprop_momentum), f(self.rmsprop_epsilon)
        omr = f(1.0 - float(rho))
        lr32 = f(lr)
        w, ms, mom = master, self.rms_ms, self.mom
        gp = g * self._clip_scale(g) if self.clip_grad_norm > 0 else g.clone()
        decoupled = self.rmsprop_wd == "decoupled"
        if not decoupled:
            gp = gp + self.rmsprop_wd_seg * w
        ms.copy_(rho * ms + omr * (gp * gp))
        d = ms
        if self.rmsprop_centered:
            mg = self.rms_mg
            mg.copy_(rho * mg + omr * gp)
            d = ms - mg * mg
        d = d + eps
        # (the root through fp64 and rounded once more: correctly rounded in fp32, as the
        # kernel's, whichever vector sqrt the torch build uses)
        mom.copy_(mo * mom + (lr32 * gp) / d.double().sqrt().float())
        wn = w - mom
        if decoupled:
            wn = wn - (lr32 * self.rmsprop_wd_seg) * w   # of the old w
        w.copy_(wn)

    def rmsprop_state(self):
        """As Engine.rmsprop_state(): the coefficients and flat views of ms (and mg)."""
        if not self.rmsprop:
            return None
        st = {"rho": self.rmsprop_rho, "momentum": self.rmsprop_momentum,
              "epsilon": self.rmsprop_epsilon, "centered": self.rmsprop_centered,
              "ms": self.rms_ms.view(-1)}
        if self.rmsprop_centered:
            st["mg"] = self.rms_mg.view(-1)
        return st

    def _lamb_update(self, master, g, lr):
        """csrc/lamb.hip's three stages in fp32 torch (the norms in fp64, as the kernels'
        are from the wave on); k1, k2 in fp64 from the step, each rounded once."""
        f = lambda x: torch.tensor(x, dtype=torch.float32)   # noqa: E731
        b1, b2, eps = f(self.adam_beta1), f(self.adam_beta2), f(self.adam_epsilon)
        omb1, omb2 = f(1.0 - float(b1)), f(1.0 - float(b2))
        lr32 = f(lr)
        t = max(1, self.step_count - self.adam_start + 1)
        k1, k2 = (f(k) for k in lamb_bias_corrections(t, self.adam_beta1, self.adam_beta2))
        w, wd = master, self.adam_wd
        gp = g * self._clip_scale(g) if self.clip_grad_norm > 0 else g.clone()
        if self.adam_decay == "l2":
            gp = gp + wd * w
        self.mom.mul_(b1).add_(omb1 * gp)
        self.adam_v.mul_(b2).add_(omb2 * (gp * gp))
        u = (self.mom * k1) / (torch.sqrt(self.adam_v * k2) + eps)
        if self.adam_decay == "decoupled":
            u = u + wd * w
        rate = torch.empty_like(w)
        self._lamb_state = {}
        for s in self.store.train_slots:
            sl = slice(s.offset, s.offset + s.numel)
            wn = float(torch.sqrt((w[sl].double() ** 2).sum()))
            un = float(torch.sqrt((u[sl].double() ** 2).sum()))
            skipped = self.adam_trust_skip == "vectors" and len(s.shape) == 1
            tr = 1.0
            if not skipped and wn > 0 and un > 0:
                tr = wn / un
            tr = f(tr)
            rate[sl] = lr32 * tr
            self._lamb_state[s.name] = (float(f(wn)), float(f(un)), float(tr), skipped)
        w.sub_(rate * u)
        self._adam_state = (t, adam_alpha(float(lr32), t, self.adam_beta1, self.adam_beta2))

    def lamb_state(self):
        """{tensor name: (wn, un, trust)} of the last step (None: adam_trust off, or no step
        yet)."""
        if self._lamb_state is None:
            return None
        return {n: v[:3] for n, v in self._lamb_state.items()}

    def lamb_summary(self):
        if self._lamb_state is None:
            return None
        return lamb_trust_summary({n: v[:3] for n, v in self._lamb_state.items() if not v[3]})

    def _ema_update(self):
        """shadow -= om * (shadow - master), k = the steps completed (csrc/ema.hip)."""
        om = torch.tensor(1.0 - self.ema_decay, dtype=torch.float32)
        if self.ema_warmup:
            k = torch.tensor(float(10 + self.step_count), dtype=torch.float32)
            om = torch.maximum(om, torch.tensor(9.0, dtype=torch.float32) / k)
        with torch.no_grad():
            self.ema.sub_(om * (self.ema - self.store.master))

    def ema_state(self):
        """{tensor name: view of its shadow} (None: ema_decay 0)."""
        if self.ema is None:
            return None
        return {s.name: self.ema[s.offset:s.offset + s.numel].view(s.shape)
                for s in self.store.train_slots}

    def _clip_scale(self, g):
        """The scale of the clipped update (csrc/clip.hip): 1 if norm <= c, c / norm if
        norm > c, NaN if the sum of squares is not finite; the gradient is not rescaled."""
        ss = (g.double() * g.double()).sum()
        norm = torch.sqrt(ss)
        c = torch.tensor(self.clip_grad_norm, dtype=torch.float32).double()
        if not bool(torch.isfinite(ss)):
            scale = torch.tensor(float("nan"), dtype=torch.float64)
        elif bool(norm > c):
            scale = c / norm
        else:
            scale = torch.tensor(1.0, dtype=torch.float64)
        norm, scale = norm.float(), scale.float()
        self._clip_state = (float(norm), float(scale))
        return scale

    def clip_state(self):
        """(norm, scale) of the last step (None: clipping off, or no step yet)."""
        return self._clip_state

    def mixup_state(self):
        """(lam, shift) of the last step (None: mixup off, or no step yet)."""
        return self._mixup_state

    def mix_state(self):
        """As Engine.mix_state (None: mixup and CutMix off, or no step yet)."""
        return self._mix_state

    def _erase(self, x):
        """x [N, H, W, C] with each image's box of this step (erase_draw) set to the fill."""
        N, H, W, C = x.shape
        x = x.clone()
        state = np.zeros((N, 5), dtype=np.int64)
        for n in range(N):
            d = erase_draw(self.data_seed, self.step_count, n, len(self.erase_tab), H, W,
                           self.erase_tab, self.erase_thresh)
            if not d["on"]:
                continue
            y0, x0, eh, ew = d["y0"], d["x0"], d["eh"], d["ew"]
            state[n] = (1, y0, x0, eh, ew)
            if self.erase_noise is None:
                x[n, y0:y0 + eh, x0:x0 + ew] = 0.0
                continue
            idx = [[[erase_noise_index(d["h2"], y, xx, c, W, len(self.erase_noise))
                     for c in range(C)] for xx in range(x0, x0 + ew)]
                   for y in range(y0, y0 + eh)]
            x[n, y0:y0 + eh, x0:x0 + ew] = torch.from_numpy(self.erase_noise[np.array(idx)])
        self._erase_state = state
        return x

    def erase_state(self):
        """As Engine.erase_state (None: erasing off, or no step yet)."""
        return self._erase_state

    def _lars_trust(self, master, g):
        """The per-element trust ratio of the LARS update (csrc/lars.hip, in fp32 torch):
        per tensor eeta * |w| / (|g| + wd * |w| + epsilon) from the all-reduced gradient
        before decay; exactly 1 for a skipped tensor or a zero norm."""
        trust = torch.ones_like(master)
        self._lars_state = {}
        for s in self.store.train_slots:
            w, gs = master[s.offset:s.offset + s.numel], g[s.offset:s.offset + s.numel]
            wn, gn = float(torch.linalg.vector_norm(w)), float(torch.linalg.vector_norm(gs))
            t = 1.0
            skipped = self.lars_skip == "vectors" and len(s.shape) == 1
            if not skipped and wn > 0 and gn > 0:
                t = self.lars_eeta * wn / (gn + self.wd * wn + self.lars_epsilon)
            trust[s.offset:s.offset + s.numel] = t
            self._lars_state[s.name] = (wn, gn, t, skipped)
        return trust

    def lars_state(self):
        """{tensor name: (wn, gn, trust)} of the last step (None: not lars, or no step yet)."""
        if self._lars_state is None:
            return None
        return {n: v[:3] for n, v in self._lars_state.items()}

    def lars_summary(self):
        if self._lars_state is None:
            return None
        from .engine import lars_trust_summary

        return lars_trust_summary({n: v[:3] for n, v in self._lars_state.items() if not v[3]})

    def metrics(self, top5: bool = False):
        """The last step's scalars; ``top5`` adds `precision_top5` (as Engine.metrics)."""
        m = dict(self._last)
        if top5:
            m["precision_top5"] = self._last_top5
        if self._clip_state is not None:
            m["grad_norm"], m["clip_scale"] = self._clip_state
        if self._adam_state is not None:
            m["adam_alpha"] = self._adam_state[1]
        if self.lion:
            m["optimizer"] = "lion"
        if self.rmsprop:
            m["optimizer"] = "rmsprop"
        if self._mixup_state is not None:
            m["mixup_lam"] = self._mixup_state[0]
            m["mix_mode"] = int(self._cut_area is not None)
            if self._cut_area is not None:
                m["cutmix_area"] = self._cut_area
        if self._erase_state is not None:
            box = self._erase_state
            m["erase_count"] = int(box[:, 0].sum())
            m["erase_area"] = float((box[:, 3] * box[:, 4]).sum() /
                                    (self.N * self.spec.image_h * self.spec.image_w))
        return m

    def synchronize(self):
        pass

    def check_health(self):
        pass

    def state_tensors(self):
        adam = None
        if self.adam:
            adam = {"v": self.adam_v, "start_step": self.adam_start, "beta1": self.adam_beta1,
                    "beta2": self.adam_beta2}
        rms = {"ms": self.rms_ms, "mg": self.rms_mg} if self.rmsprop else None
        return state_to_tf(self.store, self.mom, self.step_count, ema=self.ema, adam=adam,
                           lion=self.lion, rmsprop=rms)

    def load_state(self, tensors):
        with torch.no_grad():
            if self.rmsprop:   # first: a checkpoint of the other form is refused untouched
                check_rmsprop_form(tensors, self.store, self.rmsprop_centered)
            own = self.adam or self.lion or self.rmsprop
            self.step_count = tf_to_state(tensors, self.store, None if own else self.mom,
                                          ema=self.ema)
            if self.adam:
                self.adam_start = tf_to_adam(tensors, self.store, self.mom, self.adam_v)
            if self.lion:
                tf_to_lion(tensors, self.store, self.mom)
            if self.rmsprop:   # (after the weights, as the adam and lion slots)
                tf_to_rmsprop(tensors, self.store, self.rms_ms, self.rms_mg, self.mom)

    def broadcast_parameters(self, src: int = 0):
        if self.dist is not None and self.world > 1:
            with torch.no_grad():
                for t in (self.store.master, self.store.stats, self.mom) + (
                        (self.ema,) if self.ema is not None else ()) + (
                        (self.adam_v,) if self.adam else ()):
                    self.dist.broadcast(t.data, src)
                s = torch.tensor([self.step_count, self.adam_start])
                self.dist.broadcast(s, src)
                self.step_count, self.adam_start = (int(x) for x in s.tolist())

    # -------------------------------------------------------------- eval
    def evaluate_batch(self, images, labels):
        """(loss_sum, correct, probs) in inference mode (moving BN statistics)."""
        if images.dtype == torch.uint8:
            images = augment_cpu(images, train=False)
        with torch.no_grad():
            logits = self.model(images.float(), False)
            probs = torch.softmax(logits, 1)
            loss = torch.nn.functional.cross_entropy(logits, labels.long(), reduction="sum")
            correct = (logits.argmax(1) == labels.long()).float().sum()
            self.last_eval_top5 = float(ref.in_top_k(logits, labels, 5).float().sum())
        return float(loss), float(correct), probs


def make_backend(spec: ModelSpec, batch_size: int, *, device: str, weight_decay: float,
                 lr_schedule, optimizer: str = "mom", seed: int = 0, dist_ctx=None,
                 bucket_mb: float | None = None, use_graph: bool = False, global_batch=None,
                 input_mode: str = "auto", data_seed: int = 1234,
                 allreduce_dtype: str = "fp32", resident=None, shuffle_seed: int = 0,
                 lars_eeta: float = 0.001, lars_epsilon: float = 0.0,
                 lars_skip: str = "vectors", label_smoothing: float = 0.0,
                 ema_decay: float = 0.0, ema_warmup: bool = True, clip_grad_norm: float = 0.0,
                 mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0,
                 mix_switch_prob: float = 0.5, adam_beta1: float = 0.9,
                 adam_beta2: float = 0.999, adam_epsilon: float = 1e-8,
                 adam_decay: str = "decoupled", adam_decay_skip: str = "none",
                 adam_trust="off", adam_trust_skip: str = "vectors", erase_prob: float = 0.0,
                 erase_area_min: float = 0.02, erase_area_max: float = 1.0 / 3.0,
                 erase_aspect_min: float = 0.3, erase_fill: str = "zero",
                 lion_beta1: float = 0.9, lion_beta2: float = 0.99,
                 lion_decay_skip: str = "none", rmsprop_rho: float = 0.9,
                 rmsprop_momentum: float = 0.9, rmsprop_epsilon: float = 1e-10,
                 rmsprop_centered: bool = False, rmsprop_wd: str = "l2",
                 rmsprop_decay_skip: str = "none"):
    """device: gpu | cpu | auto.  ``resident`` (GPU, input_mode='cifar_resident'): the
    (images, labels) of the split the engine keeps on the device."""
    if device == "auto":
        device = "gpu" if torch.cuda.is_available() else "cpu"
    adam = dict(adam_beta1=adam_beta1, adam_beta2=adam_beta2, adam_epsilon=adam_epsilon,
                adam_decay=adam_decay, adam_decay_skip=adam_decay_skip, adam_trust=adam_trust,
                adam_trust_skip=adam_trust_skip, lion_beta1=lion_beta1, lion_beta2=lion_beta2,
                lion_decay_skip=lion_decay_skip, rmsprop_rho=rmsprop_rho,
                rmsprop_momentum=rmsprop_momentum, rmsprop_epsilon=rmsprop_epsilon,
                rmsprop_centered=rmsprop_centered, rmsprop_wd=rmsprop_wd,
                rmsprop_decay_skip=rmsprop_decay_skip)
    erase = dict(erase_prob=erase_prob, erase_area_min=erase_area_min,
                 erase_area_max=erase_area_max, erase_aspect_min=erase_aspect_min,
                 erase_fill=erase_fill)
    if device == "gpu":
        from .engine import Engine

        local = local_device_index()
        torch.cuda.set_device(local)
        eng = Engine(spec, batch_size, weight_decay=weight_decay, lr_schedule=lr_schedule,
                     optimizer=optimizer, device=torch.device("cuda", local), dist_ctx=dist_ctx,
                     bucket_mb=bucket_mb, seed=seed, input_mode=input_mode,
                     global_batch=global_batch, use_graph=use_graph, data_seed=data_seed,
                     allreduce_dtype=allreduce_dtype, resident=resident,
                     shuffle_seed=shuffle_seed, lars_eeta=lars_eeta,
                     lars_epsilon=lars_epsilon, lars_skip=lars_skip,
                     label_smoothing=label_smoothing, ema_decay=ema_decay,
                     ema_warmup=ema_warmup, clip_grad_norm=clip_grad_norm,
                     mixup_alpha=mixup_alpha, cutmix_alpha=cutmix_alpha,
                     mix_switch_prob=mix_switch_prob, **adam, **erase)
        return GPUBackend(eng, use_graph=use_graph)
    if resident is not None:
        raise ValueError("a device-resident split needs the GPU backend")
    return CPUBackend(spec, batch_size, weight_decay=weight_decay, lr_schedule=lr_schedule,
                      optimizer=optimizer, seed=seed, dist_ctx=dist_ctx,
                      global_batch=global_batch, allreduce_dtype=allreduce_dtype,
                      lars_eeta=lars_eeta, lars_epsilon=lars_epsilon, lars_skip=lars_skip,
                      label_smoothing=label_smoothing, ema_decay=ema_decay,
                      ema_warmup=ema_warmup, clip_grad_norm=clip_grad_norm,
                      mixup_alpha=mixup_alpha, data_seed=data_seed, cutmix_alpha=cutmix_alpha,
                      mix_switch_prob=mix_switch_prob, **adam, **erase)
