"""GPU training engine: flat buffers + one static native plan per step.

This replaces the reference's TF graph + MonitoredTrainingSession hot loop
(`mon_sess.run(train_op)`, resnet_cifar_main.py:339-358).  The
ResNet v2 graph is static, so instead of an autograd tape the engine records
ONE native plan (csrc/bindings.cpp `Plan`) holding every launch of a training
step with all pointers bound:

  forward   input augmentation -> stem -> blocks -> BN-ReLU+avg-pool -> dense ->
            softmax-xent (+training precision, +dense-bias grad)
            * BN-ReLU is never materialised: each conv applies the previous BN's
              scale/shift + ReLU while staging its A operand (PRE), and emits the
              next BN's Welford partials from its epilogue (STATS);
            * the residual add is fused into the last conv of each block;
  backward  hand-scheduled reverse pass: per conv a dgrad (MFMA) and a split-K
            wgrad (MFMA, fused BN-ReLU recompute of its input) + deterministic
            reduce into the flat fp32 gradient; per BN one reduce / finalize /
            apply (ReLU mask and residual-gradient add fused);
  allreduce after the op that finalises each gradient bucket
            (parallel/buckets.py): a plan op on the comm stream -- the native
            RCCL communicator (csrc/comm.h) all-reduces the bucket while the
            compute streams continue the backward; the optimizer waits on it
            (c10d all-reduces between plan segments for gloo rehearsals);
  optimizer one fused SGD-momentum + weight-decay + bf16 re-pack launch, LR from
            the device-resident global_step, then global_step += 1.

The plan runs natively segment by segment (no Python per op); `use_graph`
captures the whole step into a hipGraph instead (measured slower than the eager
native plan on this runtime, profiles/launch_mode_ab.md).

Here: the device state and the step runtime.  The plan is recorded by train/recorder.py from
the host tables of train/layout.py; LR schedules: train/schedule.py; inference: eval_plan.py.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np
import torch

from .. import native
from ..data.cifar import (MIXUP_TABLE_LEN, cutmix_table, cutmix_thresh, erase_noise_table,
                          erase_table, erase_thresh, mixup_table,
                          resident_steps_per_epoch, upload_resident)
from ..models.params import ParamStore
from ..models.spec import BNSpec, ConvSpec, ModelSpec
from ..parallel.buckets import assign_buckets, schedule_buckets
from ..utils import tune
from ..utils.streamcheck import check_plan
from .layout import (LARS_CHUNK, LARS_DTYPE, LARS_SKIPS, OPT_TILE_LOADS,  # noqa: F401
                     OPTW_DTYPE, SEG_DTYPE, WGD_DTYPE, _ceil, _pow2ceil, lars_tables,
                     OPT_FUSED_CLIP_REASON, CLIP_CHUNK, MIXUP_INPUT_MODES, check_clip_grad_norm,
                     check_mixup_alpha, check_cutmix_alpha, check_mix_switch_prob, check_erase,
                     lars_trust_summary, opt_tile, param_segments, sgd_tiles_work,
                     OPTIMIZERS, OPT_FUSED_ADAM_REASON, adam_decay_table, check_adam,
                     OPT_FUSED_LAMB_REASON, check_adam_trust, lamb_trust_summary,
                     OPT_FUSED_LION_REASON, check_lion, OPT_FUSED_RMSPROP_REASON, check_rmsprop)
from .schedule import (LRSchedule, cifar_lr_schedule, constant_lr,  # noqa: F401
                       imagenet_lr_schedule, lr_values_scaled, scaled)

BF16 = torch.bfloat16
BN_DECAY = 0.997
# Diagnostics: DTR_DIAG_SKIP=wgrad,dgrad,... drops those launches (wrong math; timing only)
_DIAG_SKIP = set(filter(None, os.environ.get("DTR_DIAG_SKIP", "").split(",")))
from ..ops.reference import BN_EPS  # noqa: E402  (TF's effective 1.001e-5)


class PersistentStepError(RuntimeError):
    """A persistent CIFAR launch's grid barrier timed out (csrc/prn_device.h: every
    wait is bounded, a timed-out workgroup sets the error flag and exits).  The step's
    results are invalid; the driver exits with code 3 so parallel/launch.py restarts the
    job from the last good checkpoint, on the per-layer plan."""


# partial count meaning "the pointer is a fp64 accumulator" in the pointer-vector
# arguments of plan.conv_gemm (pfin / abwd; read back as int -1 by the bindings)
_ACC_CNT = 0xFFFFFFFF


@dataclass
class _BN:
    spec: BNSpec
    gamma: int          # pointers into master / grad / stats buffers
    beta: int
    dgamma: int
    dbeta: int
    mmean: int
    mvar: int
    mean: torch.Tensor = None
    rstd: torch.Tensor = None
    scale: torch.Tensor = None
    shift: torch.Tensor = None
    # while a plan is recorded (train/recorder.py): forward statistics not yet
    # finalized, (partials ptr, count, rows per partial, M)
    pending: tuple = None
    names: tuple = ()
    part: torch.Tensor = None     # this BN's forward tile partials [T][2][C]
    bpart: torch.Tensor = None    # backward partial sums [T][2][C]
    acc: torch.Tensor = None      # accumulator mode: fp64 [REP][2][C] sum y, sum y^2
    bacc: torch.Tensor = None     # ... and sum g, sum g*xhat (zeroed once per step)

    def stat_ptrs(self) -> list:
        """Device pointers of [mean, rstd, scale, shift], the order the kernels take."""
        return [t.data_ptr() for t in (self.mean, self.rstd, self.scale, self.shift)]


@dataclass
class _Conv:
    spec: ConvSpec
    cin: int            # effective (padded) input channels
    ohwi: int           # bf16 pointers
    hwio: int
    grad: int           # fp32 gradient pointer (TF HWIO)
    cin_valid: int
    name: str = ""


class Engine:
    """Owns all device state of one data-parallel rank."""

    def __init__(self, spec: ModelSpec, batch_size: int, *, weight_decay: float,
                 lr_schedule: LRSchedule, optimizer: str = "mom", momentum: float = 0.9,
                 device=None, dist_ctx=None, bucket_mb: float | None = None, reduce_mb: float | None = None,
                 seed: int = 0,
                 input_mode: str = "auto", global_batch: int | None = None,
                 use_graph: bool = False, data_seed: int = 1234, fork_wgrad: bool | None = None,
                 allreduce_dtype: str = "fp32", native_comm: bool | None = None, comm=None,
                 resident=None, shuffle_seed: int = 0, lars_eeta: float = 0.001,
                 lars_epsilon: float = 0.0, lars_skip: str = "vectors",
                 label_smoothing: float = 0.0, ema_decay: float = 0.0, ema_warmup: bool = True,
                 clip_grad_norm: float = 0.0, mixup_alpha: float = 0.0,
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
        # global gradient-norm clipping (csrc/clip.hip): 0 = off (nothing allocated, no op
        # recorded), inf = the norm is only measured
        self.clip_grad_norm = check_clip_grad_norm(clip_grad_norm, optimizer)
        self.nat = native(required=True)
        tune.validate(k for k, *_ in self.nat.tune_table())
        self.spec = spec
        self.N = batch_size
        self.device = torch.device(device or "cuda")
        self.dist = dist_ctx
        self.world = dist_ctx.world_size if dist_ctx is not None else 1
        self.global_batch = global_batch or batch_size * self.world
        self.wd = float(weight_decay)
        self.momentum = float(momentum)
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be mom, sgd, lars, adamw, lion or rmsprop, got {optimizer!r}")
        if lars_skip not in LARS_SKIPS:
            raise ValueError(f"lars_skip must be one of {LARS_SKIPS}, got {lars_skip!r}")
        # lars: SGD-momentum at a per-tensor rate lr * trust (csrc/lars.hip); the momentum
        # buffer means what it means for mom, so checkpoints move between the two
        self.lars = optimizer == "lars"
        self.lars_eeta, self.lars_epsilon = float(lars_eeta), float(lars_epsilon)
        self.lars_skip = lars_skip
        self.use_momentum = optimizer in ("mom", "lars")
        # adamw: Adam in tf.train.AdamOptimizer's form with decoupled (or l2) weight decay, one
        # launch on the generic optimizer path (csrc/adam.hip).  The first moment lives in the
        # momentum buffer; the second moment, the start-step slot and the {lr, alpha, t} slot
        # exist only for adamw
        self.adam = optimizer == "adamw"
        self.adam_beta1, self.adam_beta2, self.adam_epsilon = check_adam(
            adam_beta1, adam_beta2, adam_epsilon, adam_decay, adam_decay_skip)
        self.adam_decay, self.adam_decay_skip = adam_decay, adam_decay_skip
        # adam_trust on: LAMB, adamw's direction at a per-tensor rate lr * |w| / |u| in three
        # launches (csrc/lamb.hip) over LARS's chunk table; no state of its own, so checkpoints
        # move between trust on and off.  Off: nothing allocated, every plan as adamw's
        self.lamb = check_adam_trust(adam_trust, adam_trust_skip, optimizer)
        self.adam_trust_skip = adam_trust_skip
        # lion: the sign of an interpolated momentum with decoupled weight decay, one launch on
        # the generic optimizer path (csrc/lion.hip).  Its only state, an average of the
        # gradient, lives in the momentum buffer; nothing else is allocated but the decay table
        self.lion = optimizer == "lion"
        self.lion_beta1, self.lion_beta2 = check_lion(lion_beta1, lion_beta2, lion_decay_skip)
        self.lion_decay_skip = lion_decay_skip
        # rmsprop: TF 1.12's RMSPropOptimizer (momentum, epsilon inside the root, optionally
        # centered), one launch on the generic optimizer path (csrc/rmsprop.hip).  Its `mom`
        # lives in the momentum buffer; ms (from ones) and, centered only, mg exist only for it
        self.rmsprop = optimizer == "rmsprop"
        (self.rmsprop_rho, self.rmsprop_momentum, self.rmsprop_epsilon,
         self.rmsprop_centered) = check_rmsprop(rmsprop_rho, rmsprop_momentum, rmsprop_epsilon,
                                                rmsprop_centered, rmsprop_wd, rmsprop_decay_skip)
        # (rmsprop_wd is the mode, as adam_decay; the per-segment table is rmsprop_wd_seg)
        self.rmsprop_wd, self.rmsprop_decay_skip = rmsprop_wd, rmsprop_decay_skip
        # smoothed training targets (1 - eps) * onehot + eps / classes in whichever head the
        # plan records (csrc/xent_row.h); 0 is bit-for-bit the plain cross-entropy.  The
        # eval plans never smooth.
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing!r}")
        self.label_smoothing = float(label_smoothing)
        self.topk = min(5, spec.num_classes)   # k of the `precision_top5` count
        # mixup in the step's input launch (csrc/data.hip) and two-label targets in whichever
        # head the plan records: lam ~ Beta(alpha, alpha) from a host-made table, one draw per
        # step keyed by (data_seed, global_step) (data/cifar.py mixup_draw).  0 = off: nothing
        # allocated, every plan op for op the same.  The eval plans never mix; training
        # precision is counted against the dominant label.
        self.mixup_alpha = check_mixup_alpha(mixup_alpha)
        # CutMix in the same launch (data/cifar.py cutmix_draw): a step whose draw falls under
        # cut_thresh (of 2^24) pastes one box of the partner's image instead of blending, and
        # the heads see lam = 1 - area / (H * W).  With both on, mix_switch_prob is the share
        # of CutMix steps.  0 = off: every plan records what it records without it.
        self.cutmix_alpha = check_cutmix_alpha(cutmix_alpha)
        self.mix_switch_prob = check_mix_switch_prob(mix_switch_prob)
        self.cut_thresh = cutmix_thresh(self.mixup_alpha, self.cutmix_alpha, self.mix_switch_prob)
        # Random Erasing in a launch of its own behind the input launch (csrc/erase.hip;
        # data/cifar.py erase_draw): each image gets, with probability erase_prob, one box
        # overwritten by the fill -- after the mix, when one is on; labels and lam are untouched.
        # 0 = off: nothing allocated, no op recorded.  The eval plans never erase.
        (self.erase_prob, self.erase_area_min, self.erase_area_max, self.erase_aspect_min,
         self.erase_fill) = check_erase(erase_prob, erase_area_min, erase_area_max,
                                        erase_aspect_min, erase_fill, spec.dataset)
        # shadow (exponential moving average) copy of the trainables, advanced by one launch
        # at the end of the optimizer segment (csrc/ema.hip); 0 = off: no buffer, no launch
        if not 0.0 <= ema_decay < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay!r}")
        self.ema_decay, self.ema_warmup = float(ema_decay), bool(ema_warmup)
        self.sched = lr_schedule
        self.use_graph = use_graph
        self.data_seed = data_seed
        if allreduce_dtype not in ("fp32", "bf16"):
            raise ValueError(f"allreduce_dtype must be fp32 or bf16, got {allreduce_dtype!r}")
        # bf16 gradient exchange: each bucket is cast into a bf16 staging buffer, all-reduced
        # (half the xGMI bytes) and cast back into the fp32 flat gradient before the update
        self.allreduce_bf16 = allreduce_dtype == "bf16"
        if fork_wgrad is None:
            # measured: eager + forked wgrad stream beats hipGraph replay (which
            # handles the cross-stream event edges poorly); graphs stay single-stream
            fw = tune.get("fork_wgrad")
            fork_wgrad = (not use_graph) if fw < 0 else bool(fw)
        # residual blocks per side-stream fork (tune fork_every)
        fe = tune.get("fork_every")
        self.fork_every = max(1, fe if fe > 0 else (4 if spec.dataset.startswith("cifar") else 2))
        # Backward tail: the weight gradients still queued for the side stream when the
        # main stream's dgrad chain ends (the first stage's) are shared out -- this
        # fraction of them, the last-queued ones, runs on the otherwise idle main stream
        # after the stem (_split_tail).  0 = all on the side stream.  Measured (CIFAR RN50,
        # ms/step, 0 / 0.5 / 0.75 / 1): bs16 0.978 / 0.972 / 0.972 / 0.970, bs32 1.002 /
        # 0.994 / 1.017 / 1.011, bs64 1.128 / 1.131 / 1.131 / 1.130, bs128 1.326 / 1.316 /
        # 1.314 / 1.303 (scripts/ab_tail.sh).  ImageNet, after the streaming 1x1 kernels
        # shortened the main stream's chain: RN50 bs128 1 / 0.5 / 0.25 = 10.56 / 10.49 /
        # 10.49 ms, RN101 bs256 1 / 0.5 = 32.78 / 32.66 ms (scripts/gpurun/gpu_r3_final.sh).
        tm = tune.get("tail_main")
        if tm < 0:
            tm = 1.0 if spec.dataset.startswith("cifar") else 0.5
        self.tail_main = min(1.0, max(0.0, tm))
        # ...and the last reduces then run on the main stream behind one join
        # (reduce_main_tail=0: forked to the side stream like the earlier buckets)
        self.reduce_main_tail = bool(tune.get("reduce_main_tail"))
        self.markers = os.environ.get("DTR_ROCTX", "0") != "0"
        self.fork_wgrad = fork_wgrad
        self.split_tail = fork_wgrad and self.tail_main > 0
        # kernel choices of the recorder: the streaming 1x1 kernels, the channel bound of
        # the dgrad that applies its BN backward itself (bap, 0 = off), the one-launch head
        self.fwd1x1_stream = bool(tune.get("fwd1x1_stream"))
        self.dgrad1x1_stream = bool(tune.get("dgrad1x1_stream"))
        self.bap_maxc = tune.get("bap_maxc")
        self.fused_head = bool(tune.get("fused_head"))
        if input_mode == "auto":
            input_mode = "cifar_u8" if spec.dataset.startswith("cifar") else "nhwc"
        self.input_mode = input_mode
        if self.mixup_alpha > 0 and input_mode not in MIXUP_INPUT_MODES:
            raise ValueError(f"mixup_alpha > 0 needs an input launch to mix in (input_mode one of "
                             f"{MIXUP_INPUT_MODES}), got input_mode={input_mode!r}")
        if self.cutmix_alpha > 0 and input_mode not in MIXUP_INPUT_MODES:
            raise ValueError(f"cutmix_alpha > 0 needs an input launch to paste in (input_mode one "
                             f"of {MIXUP_INPUT_MODES}), got input_mode={input_mode!r}")
        if self.erase_prob > 0:
            # the input buffer must be rewritten by a launch every step, or boxes would pile up
            if input_mode not in MIXUP_INPUT_MODES:
                raise ValueError(f"erase_prob > 0 needs an input launch to erase behind "
                                 f"(input_mode one of {MIXUP_INPUT_MODES}), got "
                                 f"input_mode={input_mode!r}")
            if input_mode.startswith("cifar") and (spec.image_h, spec.image_w) != (32, 32):
                raise ValueError("erase_prob > 0: not with the generic-shape CIFAR augment "
                                 f"kernel ({spec.image_h}x{spec.image_w} images)")
        # input_mode "cifar_resident": the whole split (uint8 [M,3,32,32] + labels) lives on
        # the device and the step's input launch picks its own records through the keyed
        # permutation of global_step (data/cifar.py resident_index; csrc/data.hip).  Uploaded
        # once, here, because the plan holds fixed pointers.  ``shuffle_seed`` is the job's,
        # the same on every rank (disjoint rank shards); data_seed keeps seeding the crops.
        self.rank = dist_ctx.rank if dist_ctx is not None else 0
        self.shuffle_seed = int(shuffle_seed)
        self.records_u8 = self.labels_all = None
        if input_mode == "cifar_resident":
            if resident is None:
                raise ValueError("input_mode='cifar_resident' needs resident=(images, labels)")
            self.records_u8, self.labels_all = upload_resident(resident, spec, self.device)
            self.records = int(self.records_u8.shape[0])
            self.steps_per_epoch = resident_steps_per_epoch(self.records, batch_size, self.world)
        elif resident is not None:
            raise ValueError("resident= is only for input_mode='cifar_resident'")
        self.kpad = _ceil(spec.num_classes, 16) * 16
        self.cpad_in = 8
        # ImageNet stem as a space-to-depth 4x4/1 conv over [N, H/2, W/2, 16] (data.hip
        # stem_s2d_*: K 392 -> 256, stride-1 gathers, a 2-tile weight gradient instead of 4)
        st = spec.stem
        self.stem_s2d = (bool(tune.get("stem_s2d")) and st.kh == 7 and
                         st.kw == 7 and st.stride == 2 and st.cin <= 3 and
                         spec.image_h % 2 == 0 and spec.image_w % 2 == 0 and
                         2 * st.ho == spec.image_h and 2 * st.wo == spec.image_w)

        dev = self.device
        self.params = ParamStore(spec, device=dev)
        self.params.initialize(seed)
        self.grad = torch.zeros(self.params.n_train, device=dev)
        self.mom = torch.zeros(self.params.n_train, device=dev)
        self.ema = self.params.master.detach().clone() if self.ema_decay > 0 else None
        self.adam_v = self.adam_start = self.adam_out = self.adam_wd = None
        if self.adam:
            self.adam_v = torch.zeros(self.params.n_train, device=dev)
            # the step the moments started at (t = global_step - start + 1): kernels only read
            # it; the host writes it here and on restore
            self.adam_start = torch.zeros(1, dtype=torch.int64, device=dev)
            self.adam_out = torch.zeros(3, device=dev)   # {lr, alpha, t} of the last step
        self.rms_ms = self.rms_mg = None
        if self.rmsprop:
            self.rms_ms = torch.ones(self.params.n_train, device=dev)   # TF's `rms` slot: ones
            if self.rmsprop_centered:
                self.rms_mg = torch.zeros(self.params.n_train, device=dev)
        self.gstep = torch.zeros(1, dtype=torch.int64, device=dev)
        # loss_sum, correct, lr, l2, health word (persistent step), in-top-5 count
        self.scalars = torch.zeros(8, device=dev)
        # sgd_tiles' last-workgroup ticket (the launch that steps global_step; left at zero)
        self.opt_ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        # weight-gradient and all-reduce streams: one pair per process, created before
        # the process group's (parallel/dist.py engine_streams: hardware queue order)
        from ..parallel.dist import engine_streams
        self.side, self.comm_stream = engine_streams(dev)
        # Native communicator (csrc/comm.h: RCCL, or the shm rehearsal transport):
        # the bucket all-reduces are plan ops on the comm stream.  None: world 1
        # (nothing to reduce), the c10d transport, or a fallback after a failed
        # native init (c10d all-reduces issued by the host between plan segments,
        # _issue_bwd; the reason in comm_fallback_reason).  native_comm=True forces
        # a single-rank RCCL communicator, `comm=` takes a prebuilt one (tests:
        # _C.Comm.loopback(2), the doubling stand-in for an all-reduce).
        self.comm = comm
        self.comm_fallback_reason = None
        didx = dev.index if dev.index is not None else torch.cuda.current_device()
        if comm is not None:
            pass
        elif self.dist is not None and (self.world > 1 or native_comm):
            if native_comm is not False:
                self.comm = self.dist.native_comm(didx, force=bool(native_comm))
                self.comm_fallback_reason = self.dist.comm_fallback_reason
        elif native_comm:
            from ..parallel.dist import DistContext
            self.comm = DistContext().native_comm(didx, force=True)
        self.grad_bf16 = (torch.zeros(self.params.n_train, dtype=BF16, device=dev)
                          if self.allreduce_bf16 and (self.world > 1 or self.comm is not None)
                          else None)
        self._build_weight_layout()
        self._alloc_activations()
        # Persistent small-batch CIFAR step (train/persist.py, csrc/prn_*.hip): the
        # forward and the backward each as ONE launch (tune persist: -1 auto = per-rank
        # batch <= AUTO_MAX_BATCH on a supported CIFAR network, 0 off, 1 whenever supported)
        from . import persist as _persist
        from ..parallel.dist import gpu_shared_by_ranks
        pm = tune.get("persist")
        self.persist_slices = tune.get("persist_slices")
        self.persist_overlap_tune = bool(tune.get("persist_overlap"))
        self.opt_fused = bool(tune.get("opt_fused"))
        # why the one-launch optimizer is off although tuned on ("" = as tuned): a trust
        # ratio needs its tensor's whole all-reduced gradient before any of it is updated
        self.opt_fused_reason = ""
        if self.lars and self.opt_fused:
            self.opt_fused = False
            self.opt_fused_reason = ("optimizer lars: the norms are taken over the complete "
                                     "fp32 gradient, before the update")
        if self.adam and self.opt_fused:   # (before clipping: with both, adamw is the reason)
            self.opt_fused = False
            self.opt_fused_reason = OPT_FUSED_LAMB_REASON if self.lamb else OPT_FUSED_ADAM_REASON
        if self.lion and self.opt_fused:   # (before clipping, as adamw)
            self.opt_fused = False
            self.opt_fused_reason = OPT_FUSED_LION_REASON
        if self.rmsprop and self.opt_fused:   # (before clipping, as adamw)
            self.opt_fused = False
            self.opt_fused_reason = OPT_FUSED_RMSPROP_REASON
        if self.clip_grad_norm > 0 and self.opt_fused:
            self.opt_fused = False
            self.opt_fused_reason = OPT_FUSED_CLIP_REASON
        # why the persistent step is off ("" = on); never on a GPU shared by several ranks
        # (its grids need every CU to themselves), and the same choice on EVERY rank (the
        # two plans issue different collectives)
        if pm == 0:
            reason = "tune persist=0"
        elif pm != 1 and self.N > _persist.AUTO_MAX_BATCH:
            reason = f"per-rank batch {self.N} > {_persist.AUTO_MAX_BATCH} (auto)"
        elif gpu_shared_by_ranks(self.dist, didx):
            reason = "GPU shared by several ranks"
        else:
            reason = _persist.check(self)
        if self.dist is not None and self.dist.active and not self.dist._agree(reason == ""):
            reason = reason or "another rank cannot run the persistent step"
        self.persist_reason = reason
        self.persist = reason == ""
        # world > 1 (or a forced communicator): the gradient buckets' reduces and
        # all-reduces overlap the persistent backward launch (tune persist_overlap)
        self.persist_overlap = self.persist and _persist.overlap_planned(self)
        if self.persist and self.dist is not None and self.dist.active:
            # one plan shape on every rank (3 bucket all-reduces or 1)
            self.persist_overlap = self.dist._agree(self.persist_overlap)
        self.prn = _persist.PersistStep(self) if self.persist else None
        self.plan = self.nat.Plan()
        self.reduce_buckets = self.world > 1 or self.comm is not None
        if self.reduce_buckets:
            if not bucket_mb:
                # ~4 buckets, at most 25 MB each: ImageNet RN50's 97 MB of gradients in
                # 25 MB all-reduces overlapping the backward; CIFAR RN50's 2.9 MB in four,
                # so all but the last (stage 1's small kernels) overlap the backward
                # instead of one latency-bound all-reduce after it
                bucket_mb = min(25.0, 4.0 * self.params.n_train / 2 ** 20 / 4)
            self.buckets = assign_buckets(self.params.train_slots, int(bucket_mb * 2 ** 20))
        else:  # one bucket: nothing to all-reduce, only the split-K reduces
            self.buckets = [(0, self.params.n_train, [s.name for s in self.params.train_slots])]
        # Split-K reduce groups nest inside the buckets: each group's grouped reduce
        # runs on the side stream as soon as its weight gradients are queued, so
        # only the last group's reduce (stem + first stage) sits at the end of
        # backward.  (One reduce of all of ResNet-50's slabs at the end was ~0.45 ms
        # of tail; the group size trades that tail against launch count.)
        if reduce_mb is None:
            # ~6 groups, at most 4 MB each (measured: CIFAR RN50's 3 MB of gradients in
            # 0.5 MB groups -2.3 % step time vs one group, whose 78 us reduce of 290 MB
            # of split-K slabs sat alone at the end of backward)
            reduce_mb = min(4.0, 4.0 * self.params.n_train / 2 ** 20 / 6)
        if tune.get("reduce_mb") > 0:
            reduce_mb = tune.get("reduce_mb")
        slot_of = {s.name: s for s in self.params.train_slots}
        self.reduce_groups = []
        for lo, hi, names in self.buckets:
            sub = assign_buckets([slot_of[n] for n in names], int(reduce_mb * 2 ** 20))
            self.reduce_groups.append([g[2] for g in sub])
        self._build_train_plan()
        if self.reduce_buckets and self.comm is None:
            # gloo rehearsal: the host issues each bucket's c10d all-reduce at its
            # ready index, between Plan.run calls (_issue_bwd)
            self.bucket_sched = schedule_buckets(self.buckets, self.ready_index)
        else:
            self.bucket_sched = []
        errs = check_plan(self.plan, self.seg, barriers=[i for i, _, _ in self.bucket_sched],
                          device_deps=self.recorded.device_deps,
                          op_buffers=self.recorded.op_buffers)
        if errs:   # fork/join structure of the three streams (race check)
            raise RuntimeError("plan stream-ordering violations:\n  " + "\n  ".join(errs[:8]))
        self.graph = None
        self._captured = False
        self._steps_run, self._cost_at = 0, -1
        self.eval_plans = {}
        self.repack()

    # ------------------------------------------------------------------ layout
    def _build_weight_layout(self):
        """Device side of train/layout.py's segment table: the table itself, the bf16
        weight buffer it indexes, and the per-layer pointers derived from it."""
        spec, ps, dev = self.spec, self.params, self.device
        mptr = ps.master.data_ptr()
        gptr = self.grad.data_ptr()
        seg_arr, bf_total = param_segments(spec, ps.train_slots, cpad_in=self.cpad_in,
                                           kpad=self.kpad, stem_s2d=self.stem_s2d)
        assert SEG_DTYPE.itemsize == self.nat.param_seg_bytes()
        self.seg_arr, self.seg_names = seg_arr, [s.name for s in ps.train_slots]
        self.segs = torch.from_numpy(seg_arr.view(np.uint8).copy()).to(dev)
        self.nseg = len(seg_arr)
        # OHWI transpose tiles (ohwi_pack): ceil(taps*C/64) x ceil(K/64) per weight
        tiles = [(_ceil(int(r["kh"] * r["kw"] * r["C"]), 64) * _ceil(int(r["K"]), 64)
                  if r["bf_ohwi"] >= 0 else 0) for r in seg_arr]
        self.ohwi_tiles = int(sum(tiles))
        self.ohwi_tile0 = torch.tensor(np.concatenate([[0], np.cumsum(tiles)[:-1]]).astype(np.int64),
                                       device=dev)
        self.wbf = torch.zeros(max(bf_total, 1), dtype=BF16, device=dev)
        if self.lars or self.lamb:
            # chunk / skip table, chunk partials and (trust, wn, gn): fixed pointers (lamb:
            # the same tables under adam_trust_skip, gn holding the norm of the direction u)
            by = self.lars_skip if self.lars else self.adam_trust_skip
            skip = [by == "vectors" and len(s.shape) == 1 for s in ps.train_slots]
            tab, blk = lars_tables(seg_arr, skip)
            assert LARS_DTYPE.itemsize == self.nat.lars_seg_bytes()
            assert LARS_CHUNK == self.nat.LARS_CHUNK
            self.lars_skipped = skip
            self.lars_segs = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
            self.lars_blk = torch.tensor(blk, dtype=torch.int32, device=dev)
            self.lars_part = torch.zeros(2 * len(blk), dtype=torch.float64, device=dev)
            self.lars_out = torch.ones(3, self.nseg, device=dev)
        if self.adam:
            # the per-segment decay the kernel reads, as the LARS kernel reads trust[]
            self.adam_wd = torch.from_numpy(adam_decay_table(
                [s.shape for s in ps.train_slots], self.wd, self.adam_decay_skip)).to(dev)
        self.lion_wd = None
        if self.lion:   # the same table under lion_decay_skip
            self.lion_wd = torch.from_numpy(adam_decay_table(
                [s.shape for s in ps.train_slots], self.wd, self.lion_decay_skip)).to(dev)
        self.rmsprop_wd_seg = None
        if self.rmsprop:   # the same table under rmsprop_decay_skip
            self.rmsprop_wd_seg = torch.from_numpy(adam_decay_table(
                [s.shape for s in ps.train_slots], self.wd, self.rmsprop_decay_skip)).to(dev)
        self.clip_part = self.clip_out = None
        if self.clip_grad_norm > 0:
            # chunk partials and the {norm, scale} slot: fixed pointers
            assert CLIP_CHUNK == self.nat.CLIP_CHUNK
            self.clip_chunks = self.nat.clip_chunks(ps.n_train)
            self.clip_part = torch.zeros(self.clip_chunks, dtype=torch.float64, device=dev)
            self.clip_out = torch.tensor([0.0, 1.0], device=dev)
        bptr = self.wbf.data_ptr()
        self.convs: dict[str, _Conv] = {}
        conv_specs = {c.name: c for c in spec.all_convs()}
        for rec, s in zip(seg_arr, ps.train_slots):
            ohwi = bptr + 2 * int(rec["bf_ohwi"])
            hwio = bptr + 2 * int(rec["bf_hwio"]) if rec["bf_hwio"] >= 0 else 0
            if s.kind == "conv":
                c = conv_specs[s.name.split("/")[0]]
                cin = int(rec["cpad"])
                if self.stem_s2d and c.name == spec.stem.name:
                    cin = 16
                    self.stem_w4 = torch.zeros(c.cout * 256, dtype=BF16, device=dev)
                    self.stem_g4 = torch.zeros(c.cout * 256, device=dev)
                    self.stem_master = mptr + 4 * s.offset
                    ohwi = self.stem_w4.data_ptr()
                self.convs[c.name] = _Conv(c, cin, ohwi, hwio, gptr + 4 * s.offset, c.cin, s.name)
            elif s.kind == "dense_kernel":
                self.dense_ohwi, self.dense_hwio = ohwi, hwio
                self.dense_grad = gptr + 4 * s.offset
                self.dense_name = s.name
        bslot = ps.slot("dense/bias")
        self.dense_bias = mptr + 4 * bslot.offset
        self.dense_bias_grad = gptr + 4 * bslot.offset

        # BatchNorm bookkeeping
        self.bns: dict[str, _BN] = {}
        sptr = ps.stats.data_ptr()
        bn_specs = [b for blk in spec.blocks for b in blk.bns] + [spec.final_bn]
        total_c = sum(b.channels for b in bn_specs)
        self.bnbuf = torch.zeros(4 * total_c, device=dev)
        off = 0
        for b in bn_specs:
            g = ps.slot(f"{b.name}/gamma")
            be = ps.slot(f"{b.name}/beta")
            mm = ps.slot(f"{b.name}/moving_mean")
            mv = ps.slot(f"{b.name}/moving_variance")
            C = b.channels
            e = _BN(b, mptr + 4 * g.offset, mptr + 4 * be.offset, gptr + 4 * g.offset,
                    gptr + 4 * be.offset, sptr + 4 * mm.offset, sptr + 4 * mv.offset,
                    names=(g.name, be.name))
            e.mean = self.bnbuf[off:off + C]
            e.rstd = self.bnbuf[total_c + off:total_c + off + C]
            e.scale = self.bnbuf[2 * total_c + off:2 * total_c + off + C]
            e.shift = self.bnbuf[3 * total_c + off:3 * total_c + off + C]
            off += C
            self.bns[b.name] = e

    def _alloc_activations(self):
        spec, N, dev = self.spec, self.N, self.device
        H, W = spec.image_h, spec.image_w
        if self.input_mode == "cifar_u8":
            self.img_u8 = torch.zeros((N, 3, H, W), dtype=torch.uint8, device=dev)
        elif self.input_mode == "imagenet_u8":   # VGG crops, HWC (imagenet_u8_pack)
            self.img_u8 = torch.zeros((N, H, W, 3), dtype=torch.uint8, device=dev)
        self.x_in = torch.zeros(self._x_in_shape(N), dtype=BF16, device=dev)
        self.labels = torch.zeros(N, dtype=torch.int32, device=dev)
        self.mix_table = self.labels_b = self.mix_lam = self.mix_log = None
        self.cut_table = self.cut_log = None
        if self.mixup_alpha > 0 or self.cutmix_alpha > 0:
            # the lam table (uploaded once), the input launch's side outputs the heads read
            # (partner labels, lam per row) and its {index, shift} log: fixed pointers.  With
            # CutMix alone every step pastes and the lam table (all 1) is never read.
            self.mix_table = (
                torch.from_numpy(mixup_table(self.mixup_alpha, self.data_seed)).to(dev)
                if self.mixup_alpha > 0 else torch.ones(MIXUP_TABLE_LEN, device=dev))
            self.labels_b = torch.zeros(N, dtype=torch.int32, device=dev)
            self.mix_lam = torch.ones(N, device=dev)
            self.mix_log = torch.zeros(2, dtype=torch.int32, device=dev)
        if self.cutmix_alpha > 0:
            # the box sizes (uploaded once) and the launch's {cut, y0, y1, x0, x1, area, cy, cx}
            self.cut_table = torch.from_numpy(
                cutmix_table(self.cutmix_alpha, self.data_seed, H, W)).to(dev)
            self.cut_log = torch.zeros(8, dtype=torch.int32, device=dev)
        self.erase_tab = self.erase_noise = self.erase_log = None
        self.erase_thresh = 0
        if self.erase_prob > 0:
            # the box sizes and (noise fill) the noise values, uploaded once, and the launch's
            # per-image {on, y0, x0, eh, ew}: fixed pointers
            self.erase_tab = torch.from_numpy(erase_table(
                self.data_seed, H, W, self.erase_area_min, self.erase_area_max,
                self.erase_aspect_min)).to(dev)
            self.erase_thresh = erase_thresh(self.erase_prob)
            if self.erase_fill == "noise":
                self.erase_noise = torch.from_numpy(erase_noise_table(self.data_seed)).to(dev)
            self.erase_log = torch.zeros((N, 5), dtype=torch.int32, device=dev)
        st = spec.stem
        self.stem_out = torch.empty((N, st.ho, st.wo, st.cout), dtype=BF16, device=dev)
        if spec.maxpool:
            mh = _ceil(st.ho, 2)
            self.pool_out = torch.empty((N, mh, mh, st.cout), dtype=BF16, device=dev)
            self.pool_arg = torch.empty((N, mh, mh, st.cout), dtype=torch.uint8, device=dev)
        self.X = []     # block inputs (X[i] = input of block i, X[-1] = last output)
        self.H1, self.H2 = [], []
        x0 = self.pool_out if spec.maxpool else self.stem_out
        self.X.append(x0)
        sc_max = 0
        self.Y1, self.Y2 = [], []   # materialized inner BN-ReLU outputs (_materialize_bn)
        for b in spec.blocks:
            f = b.convs[0].cout
            if b.kind == "building":
                self.H1.append(torch.empty((N, b.ho, b.wo, f), dtype=BF16, device=dev))
                self.H2.append(None)
                self.Y1.append(None)
                self.Y2.append(None)
            else:
                self.H1.append(torch.empty((N, b.h, b.w, f), dtype=BF16, device=dev))
                self.H2.append(torch.empty((N, b.ho, b.wo, f), dtype=BF16, device=dev))
                for h, ys in ((self.H1[-1], self.Y1), (self.H2[-1], self.Y2)):
                    ys.append(torch.empty_like(h) if self._materialize_bn(h.numel() // f, f)
                              else None)
            self.X.append(torch.empty((N, b.ho, b.wo, b.cout), dtype=BF16, device=dev))
            if b.proj is not None:
                sc_max = max(sc_max, N * b.ho * b.wo * b.cout)
        self.sc_buf = torch.empty(max(sc_max, 1), dtype=BF16, device=dev)
        F = spec.dense_in
        self.pooled = torch.empty((N, F), dtype=BF16, device=dev)
        self.dpooled = torch.empty((N, F), dtype=BF16, device=dev)
        self.logits = torch.empty((N, self.kpad), device=dev)
        self.dlogits = torch.empty((N, self.kpad), dtype=BF16, device=dev)
        # scratch: per-BN forward / backward partials (the BN's first consumer may combine
        # them -- BnPreFin / BnBwdPre -- while the same kernel produces the next BN's
        # partials, so no sharing), wgrad split-K slabs
        for b in self.bns.values():
            C = b.spec.channels
            M = N * b.spec.h * b.spec.w
            bm = min(self.nat.conv_gemm_bm(M, C), self.nat.bn_stats_tile_rows())
            b.part = torch.empty(_ceil(M, bm) * 2 * C, device=dev)
            tb = max(self.nat.bn_bwd_tiles(M, C), _ceil(M, self.nat.conv_gemm_bm(M, C)))
            b.bpart = torch.empty(tb * 2 * C, device=dev)
        # Accumulator mode (tune bn_acc, default on): the producing conv's workgroups add
        # their tile sums into BN_ACC_REP fp64 replicas per BatchNorm with memory-side
        # atomics, and the consumer reads 2 x REP values per channel instead of
        # combining every tile partial in its prologue or a finalize launch (measured on
        # the CIFAR direct convs: ~4 us per consumer prologue at 512 tiles).  All the
        # replicas live in one buffer zeroed by one memset at the start of the step.
        self.bn_acc_on = self.bn_bacc_on = bool(tune.get("bn_acc"))
        # (each BN's block holds the larger of the per-layer and the persistent kernels'
        # replica counts; a kernel uses the first replicas of the block)
        rep = max(self.nat.bn_acc_rep(), self.nat.prn_acc_rep())
        tot = sum(4 * rep * b.spec.channels for b in self.bns.values())
        # (+ N x 64 doubles and the barrier region: the persistent step's average-pool sums
        # and its sharded barrier counters / readiness line / item queue (128-B aligned lines),
        # zeroed with the accumulators at the start of every step -- train/persist.py)
        base = max(_ceil(tot, 2) * 2, 2)
        bar_d = _ceil(self.nat.prn_bar_words(), 2) + 16   # + up to 128 B of alignment
        self.bn_acc = torch.zeros(base + 64 * N + bar_d, dtype=torch.float64, device=dev)
        self.prn_pool = self.bn_acc.data_ptr() + 8 * base
        self.prn_bar = _ceil(self.bn_acc.data_ptr() + 8 * (base + 64 * N), 128) * 128
        off = 0
        for b in self.bns.values():
            n = 2 * rep * b.spec.channels
            b.acc = self.bn_acc[off:off + n]
            b.bacc = self.bn_acc[off + n:off + 2 * n]
            off += 2 * n
        max_c = max(b.spec.channels for b in self.bns.values())
        self.coef = torch.empty(3 * max_c, device=dev)
        # per-conv split-K partial slabs (persist until the bucket's grouped reduce)
        self.wg_off = {}
        tot = 0
        for name, c in self.convs.items():
            g = self._geom(c, N)
            sp, pps = self.nat.wgrad_pick_splits(g)
            self.wg_off[name] = (tot, sp, pps)
            tot += sp * c.spec.cout * g[7] * g[8] * g[3]
        sp, pps = self.nat.wgrad_pick_splits(self._dense_geom(N))
        self.wg_off["dense"] = (tot, sp, pps)
        tot += sp * self.kpad * F
        self.wg_part = torch.empty(max(tot, 1), device=dev)
        self.l2_ws = torch.empty(self.nat.l2_workspace_floats(), device=dev)
        self.xent_ws = torch.empty(self.nat.softmax_xent_ws_floats(N, self.kpad), device=dev)

    # ------------------------------------------------------------------ helpers
    def _x_in_shape(self, N):
        H, W = self.spec.image_h, self.spec.image_w
        return (N, H // 2, W // 2, 16) if self.stem_s2d else (N, H, W, self.cpad_in)

    def _stem_input(self, x):
        """[N, H, W, C <= cpad] image batch -> the stem's operand layout (x_in)."""
        x = x.to(self.device)
        N, H, W, C = x.shape
        if self.stem_s2d:   # channel (rh * 2 + rw) * 4 + c of pixel (2q + rh, 2p + rw)
            if C > 4:       # an NHWC-8 (zero-padded) batch: its 3 image channels
                x, C = x[..., :3], 3
            xp = torch.zeros((N, H, W, 4), dtype=BF16, device=self.device)
            xp[..., :C] = x.to(BF16)
            return xp.view(N, H // 2, 2, W // 2, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(
                N, H // 2, W // 2, 16)
        if C != self.cpad_in:
            xp = torch.zeros((N, H, W, self.cpad_in), dtype=BF16, device=self.device)
            xp[..., :C] = x.to(BF16)
            return xp
        return x.to(BF16)

    def _geom(self, c: _Conv, N):
        s = c.spec
        if self.stem_s2d and s.name == self.spec.stem.name:
            return [N, s.h // 2, s.w // 2, 16, s.ho, s.wo, s.cout, 4, 4, 1, 2]
        return [N, s.h, s.w, c.cin, s.ho, s.wo, s.cout, s.kh, s.kw, s.stride, (s.kh - 1) // 2]

    def _dense_geom(self, N):
        return [N, 1, 1, self.spec.dense_in, 1, 1, self.kpad, 1, 1, 1, 0]

    def _maxpool_geom(self, N):
        """The 3x3/2 SAME max-pool behind the stem as conv geometry (output h, w at [4], [5])."""
        st = self.spec.stem
        ph = _ceil(st.ho, 2)
        pad = max((ph - 1) * 2 + 3 - st.ho, 0) // 2
        return [N, st.ho, st.wo, st.cout, ph, ph, st.cout, 3, 3, 2, pad]

    def _consumer_cap(self, C: int) -> int:
        """Max partials a consumer prologue combines (bn_prefin_table / _sums)."""
        return self.nat.pfin_cap(C)

    def _materialize_bn(self, M: int, C: int) -> bool:
        """Inner bottleneck BN: materialize ReLU(BN(x)) once instead of applying it in
        the consumer conv's A staging (PRE), whose VALU work is repeated by every
        output-column tile and, beside the MFMAs of the small 64x64 tiles of the 7x7
        layers, cost more than the MFMAs (3x3 512->512: 66 -> 103 us).  Materializing
        is one streaming pass: a win where the tensor is small and the consumers'
        column tiles many (tune mat_bn_elems: M*C threshold, 0 = never; mat_bn_minc: min
        channels).  Measured (RN50 bs128): stages 3-4 (14x14 / 7x7) +1.3 %; adding stage 2
        no gain."""
        return C >= tune.get("mat_bn_minc") and M * C <= tune.get("mat_bn_elems")

    # ------------------------------------------------------------------ plan
    def _build_train_plan(self):
        """Record the step into self.plan and keep what the runtime needs of the recording:
        `recorded` (a RecordedStep) and, as attributes for their readers, some of its fields."""
        from .recorder import StepRecorder
        rec = StepRecorder(self, self.plan)
        r = self.recorded = rec.record_persistent() if self.persist else rec.record_layers()
        self.seg, self.ready_index, self._keep = r.seg, r.ready_index, r.keep
        self.n_bap, self._head_fused = r.n_bap, r.head_fused

    def forward_backward(self, st=None):
        """Forward + backward of the current batch with `grad` complete and no update
        (the persistent step on one GPU otherwise leaves its weight-gradient slabs to
        the optimizer launch)."""
        if self.persist_overlap:
            # the overlap plan updates the early buckets' parameters on the comm stream
            # inside the backward segment: no update-free backward exists
            raise RuntimeError("forward_backward: the persistent overlap plan (world > 1, "
                               "tune persist_overlap=1) updates parameters during the backward")
        st = torch.cuda.current_stream().cuda_stream if st is None else st
        self._run("fwd", st)
        self._run_bwd(st)
        if "gsum" in self.seg:
            self._run("gsum", st)

    def lars_state(self):
        """{tensor name: (wn, gn, trust)} of the last step's LARS update: the norms of the
        fp32 master and of the all-reduced gradient it was formed from (synchronises).
        None unless the optimizer is lars."""
        if not self.lars:
            return None
        torch.cuda.synchronize(self.device)
        t, wn, gn = self.lars_out.cpu().tolist()
        return {n: (wn[i], gn[i], t[i]) for i, n in enumerate(self.seg_names)}

    def lars_summary(self):
        """min / median / max trust ratio over the adapted tensors (None: not lars)."""
        st = self.lars_state()
        if st is None:
            return None
        return lars_trust_summary({n: v for (n, v), skip in zip(st.items(), self.lars_skipped)
                                   if not skip})

    def lamb_state(self):
        """{tensor name: (wn, un, trust)} of the last step's LAMB update: the norms of the fp32
        master and of the direction u it was moved along, and their ratio (1 for a skipped
        tensor or a zero norm; synchronises).  None before the first step, and unless the
        optimizer is adamw with adam_trust on."""
        if not self.lamb or self._steps_run == 0:
            return None
        torch.cuda.synchronize(self.device)
        t, wn, un = self.lars_out.cpu().tolist()
        return {n: (wn[i], un[i], t[i]) for i, n in enumerate(self.seg_names)}

    def lamb_summary(self):
        """min / median / max trust ratio over the adapted tensors (None: as lamb_state)."""
        st = self.lamb_state()
        if st is None:
            return None
        return lamb_trust_summary({n: v for (n, v), skip in zip(st.items(), self.lars_skipped)
                                   if not skip})

    def clip_state(self):
        """(norm, scale) of the last step's clipping: the global norm of the complete
        gradient and the factor its update applied (synchronises).  None: clipping off."""
        if self.clip_out is None:
            return None
        torch.cuda.synchronize(self.device)
        norm, scale = self.clip_out.cpu().tolist()
        return norm, scale

    def adam_state(self):
        """(t, alpha) of the last step's adamw update: the step count of the bias correction
        (global_step - adam_start_step + 1 when the step began; read back from an fp32 slot,
        so exact below 2^24) and the bias-corrected rate lr * sqrt(1 - b2^t) / (1 - b1^t)
        (synchronises).  None unless the optimizer is adamw."""
        if not self.adam:
            return None
        torch.cuda.synchronize(self.device)
        _, alpha, t = self.adam_out.cpu().tolist()
        return int(t), alpha

    def rmsprop_state(self):
        """{"rho", "momentum", "epsilon", "centered"} of the rmsprop optimizer plus "ms" (and,
        centered, "mg"): flat views of the state buffers, in the master's layout (`mom` is the
        momentum buffer).  None unless the optimizer is rmsprop."""
        if not self.rmsprop:
            return None
        st = {"rho": self.rmsprop_rho, "momentum": self.rmsprop_momentum,
              "epsilon": self.rmsprop_epsilon, "centered": self.rmsprop_centered,
              "ms": self.rms_ms.view(-1)}
        if self.rmsprop_centered:
            st["mg"] = self.rms_mg.view(-1)
        return st

    def set_adam_start(self, step: int):
        """The step the moments count from (a restore's: the checkpoint's adam_start_step, or
        global_step when the moments restart from zero)."""
        if self.adam:
            self.adam_start.fill_(int(step))

    def mixup_state(self):
        """(lam, shift) of the last step's mixup: batch position n was blended with position
        (n + shift) % batch at weight lam (synchronises).  None: mixup off."""
        if self.mix_log is None:
            return None
        torch.cuda.synchronize(self.device)
        return float(self.mix_lam[0].item()), int(self.mix_log[1].item())

    def mix_state(self):
        """The last step's input mixing (synchronises): {"mode": "mixup" | "cutmix", "lam" (the
        applied one), "shift", "box": (y0, y1, x0, x1) of a CutMix step, else None}.  None:
        mixup and CutMix off."""
        if self.mix_log is None:
            return None
        lam, shift = self.mixup_state()
        cut = self.cut_log.cpu().tolist() if self.cut_log is not None else [0] * 8
        return {"mode": "cutmix" if cut[0] else "mixup", "lam": lam, "shift": shift,
                "box": tuple(cut[1:5]) if cut[0] else None}

    def erase_state(self):
        """The last step's erased boxes (synchronises): int array [N, 5] of {on, y0, x0, eh, ew}
        per batch position, data/cifar.py erase_draw's (0s: not erased).  None: erasing off, or
        no step yet."""
        if self.erase_log is None or self._steps_run == 0:
            return None
        torch.cuda.synchronize(self.device)
        return self.erase_log.cpu().numpy()

    def mix_head_ptrs(self) -> tuple:
        """The loss heads' trailing mixup arguments (labels_b, mix_lam); () with mixup off."""
        return () if self.labels_b is None else (self.labels_b.data_ptr(), self.mix_lam.data_ptr())

    def ema_state(self):
        """{tensor name: view of its shadow in the flat EMA buffer} (None: --ema_decay 0)."""
        if self.ema is None:
            return None
        return {s.name: self.ema[s.offset:s.offset + s.numel].view(s.shape)
                for s in self.params.train_slots}

    def reset_ema(self):
        """Shadows := the current weights (a fresh start, or a checkpoint without shadows)."""
        if self.ema is not None:
            self.ema.copy_(self.params.master.detach())

    def persist_error(self) -> bool:
        """Whether a persistent launch's barrier wait ever timed out (synchronises)."""
        return self.prn is not None and bool(self.prn.err.item())

    def check_health(self, err_word: float | None = None):
        """Raise PersistentStepError when a persistent launch's grid barrier timed out:
        its workgroups exited early, so that step's gradient, weights and BN statistics
        are garbage and must neither reach a checkpoint nor keep training.  `err_word`:
        the flag slot (scalars[4]) if the caller has read the scalars already."""
        if self.prn is None:
            return
        if err_word is None:
            bad = bool(self.prn.err.item())
        else:
            bad = err_word != 0.0
        if bad:
            raise PersistentStepError(
                "a persistent-step grid barrier timed out (workgroups not co-resident or lost); "
                f"the step's results are invalid (err={int(self.prn.err.item())})")

    def clear_persist_error(self):
        if self.prn is not None:
            self.prn.err.zero_()

    # ------------------------------------------------------------------ running
    def repack(self):
        """Refresh the bf16 weight copies from the fp32 master (no update)."""
        st = torch.cuda.current_stream().cuda_stream
        # (a zero-momentum, zero-decay update at a constant rate: only its re-pack acts)
        self.nat.sgd_update_pack(self.params.master.data_ptr(), self.grad.data_ptr(),
                                 self.mom.data_ptr(), self.params.n_train,
                                 *constant_lr(self.sched.init).launch_args(), 0, 0.0, 0.0, 1.0,
                                 0, self.segs.data_ptr(), self.nseg, self.wbf.data_ptr(), 0, 0, st)
        self.nat.ohwi_pack(self.params.master.data_ptr(), self.segs.data_ptr(),
                           self.ohwi_tile0.data_ptr(), self.nseg, self.ohwi_tiles,
                           self.wbf.data_ptr(), 0, st)
        if self.stem_s2d:
            self.nat.stem_s2d_pack(self.stem_master, self.stem_w4.data_ptr(),
                                   self.spec.stem.cout, st)

    def _run(self, name, stream):
        a, b = self.seg[name]
        self.plan.run(a, b, stream, self.side.cuda_stream, self.comm_stream.cuda_stream)

    def _step_eager(self, need_cost: bool = False):
        st = torch.cuda.current_stream().cuda_stream
        if need_cost:
            self._run("cost", st)
        if self.markers:
            return self._step_marked(st)
        self._run("fwd", st)
        self._run_bwd(st)
        self._run("opt", st)

    def _step_marked(self, st):
        """The eager step inside roctx ranges (DTR_ROCTX=1 / bench --roctx): the
        phases show up as markers in `rocprofv3 --marker-trace` timelines."""
        nvtx = torch.cuda.nvtx   # roctx on ROCm builds of PyTorch
        nvtx.range_push("dtr.step")
        for name, fn in (("fwd", lambda: self._run("fwd", st)), ("bwd+allreduce",
                         lambda: self._run_bwd(st)), ("opt", lambda: self._run("opt", st))):
            nvtx.range_push(f"dtr.{name}")
            fn()
            nvtx.range_pop()
        nvtx.range_pop()

    def _host_allreduce(self, lo, hi):
        """gloo rehearsal: a c10d all-reduce of grad[lo:hi) issued by the host."""
        if self.grad_bf16 is not None:
            buf = self.grad_bf16[lo:hi]
            buf.copy_(self.grad[lo:hi])
            return self.dist.all_reduce_async(buf), lo, hi
        return self.dist.all_reduce_async(self.grad[lo:hi]), lo, hi

    def _host_allreduce_wait(self, works):
        for w, lo, hi in works:
            w.wait()
            if self.grad_bf16 is not None:
                self.grad[lo:hi].copy_(self.grad_bf16[lo:hi])

    def _issue_bwd(self, st) -> list:
        """Issue the backward segment; with host-issued all-reduces (bucket_sched) each
        bucket's goes out at its ready index, between Plan.run calls.  Returns their work
        handles for _host_allreduce_wait."""
        a, b = self.seg["bwd"]
        side, comm = self.side.cuda_stream, self.comm_stream.cuda_stream
        works, prev = [], a
        for idx, lo, hi in self.bucket_sched:
            if idx > prev:
                self.plan.run(prev, idx, st, side, comm)
                prev = idx
            works.append(self._host_allreduce(lo, hi))
        if b > prev:
            self.plan.run(prev, b, st, side, comm)
        return works

    def _run_bwd(self, st):
        self._host_allreduce_wait(self._issue_bwd(st))

    def step_timed(self, need_cost: bool = False) -> dict:
        """One eager step with HIP-event timing per phase (ProfilerHook, bench.py):
        forward, backward compute, the exposed all-reduce tail (from the end of
        the backward's compute to the optimizer's join of the last bucket's
        all-reduce; for gloo rehearsals, the host's c10d waits) and the optimizer."""
        st = torch.cuda.current_stream().cuda_stream
        p, r = self.plan, self.recorded
        self._steps_run += 1
        if need_cost:
            self._run("cost", st)
            self._cost_at = self._steps_run
        if self.bucket_sched:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            ev[0].record()
            self._run("fwd", st)
            ev[1].record()
            works = self._issue_bwd(st)
            ev[2].record()
            self._host_allreduce_wait(works)
            ev[3].record()
            self._run("opt", st)
            ev[4].record()
            torch.cuda.synchronize()
            return {"forward": ev[0].elapsed_time(ev[1]), "backward": ev[1].elapsed_time(ev[2]),
                    "allreduce_exposed": ev[2].elapsed_time(ev[3]),
                    "backward+allreduce": ev[1].elapsed_time(ev[3]),
                    "optimizer": ev[3].elapsed_time(ev[4])}
        p.set_timing(True)
        try:
            self._run("fwd", st)
            self._run_bwd(st)
            self._run("opt", st)
            torch.cuda.synchronize()
        finally:
            p.set_timing(False)
        bwd = p.elapsed_ms(r.t_bwd0, r.t_bwd_done)
        exposed = p.elapsed_ms(r.t_bwd_done, r.t_joined)
        return {"forward": p.elapsed_ms(r.t_fwd0, r.t_bwd0), "backward": bwd,
                "allreduce_exposed": exposed, "backward+allreduce": bwd + exposed,
                "optimizer": p.elapsed_ms(r.t_joined, r.t_opt_end)}

    def comm_info(self) -> dict:
        """How the gradients are exchanged (bench.py JSON)."""
        nat = self.comm is not None
        per = 2 if self.grad_bf16 is not None else 4
        transport = self.comm.transport if nat else ("c10d" if self.bucket_sched else None)
        return {"native_rccl": nat and transport == "rccl",
                "native": nat,
                "transport": transport,
                "fallback_reason": self.comm_fallback_reason,
                "buckets": len(self.buckets) if self.reduce_buckets else 0,
                "allreduce_ops": self.recorded.n_allreduce if nat else len(self.bucket_sched),
                "allreduce_bytes": (self.recorded.allreduce_bytes if nat else
                                    sum((hi - lo) * per for _, lo, hi in self.bucket_sched)),
                "rccl_library": self.comm.library_path if nat else None,
                "rccl_version": (self.nat.Comm.rccl_version()
                                 if nat and transport == "rccl" else None),
                # the persistent overlap plan's CU budget: CUs left out of the backward
                # grid for the comm stream, and RCCL's channel cap / reported channels
                "overlap_reserve_cus": (self.prn.cus - self.N * self.prn.P - self.prn.wgrad_wgs
                                        if self.persist_overlap else 0),
                **(self.dist.rccl_channel_info() if self.dist is not None else
                   {"rccl_max_nchannels": os.environ.get("NCCL_MAX_NCHANNELS"),
                    "rccl_channels": None}),
                # the communication environment of this run (RCCL / HSA knobs)
                "env": {k: v for k, v in sorted(os.environ.items())
                        if k.startswith(("NCCL_", "RCCL_", "HSA_"))}}

    def capture(self, warmup: int = 2):
        """Run `warmup` real steps on a side stream, then capture one step."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self._step_eager()
                self._steps_run += 1
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step_eager()
        self.graph = g
        self._captured = True
        return warmup

    def step(self, need_cost: bool = False):
        """One training step (global_step += 1 on the device).  ``need_cost``: also
        compute 1/2 sum v^2 of this step's (pre-update) weights for the logged cost."""
        if self.graph is not None:
            if need_cost:
                self._run("cost", torch.cuda.current_stream().cuda_stream)
            self.graph.replay()
        else:
            self._step_eager(need_cost)
        self._steps_run += 1
        if need_cost:
            self._cost_at = self._steps_run

    # ------------------------------------------------------------------ io
    def set_batch(self, images, labels):
        """Copy a host/device batch into the static input buffers."""
        self._no_host_input("set_batch")
        if self.input_mode in ("cifar_u8", "imagenet_u8"):
            self.img_u8.copy_(images, non_blocking=True)
        else:
            x = images
            if x.dim() == 4 and tuple(x.shape) != tuple(self.x_in.shape):
                x = self._stem_input(x)
            self.x_in.copy_(x, non_blocking=True)
        self.labels.copy_(labels.to(torch.int32), non_blocking=True)

    def _no_host_input(self, what: str):
        if self.input_mode == "cifar_resident":
            raise RuntimeError(
                f"{what}: input_mode='cifar_resident' takes no batches from the host -- the "
                "plan reads its records and labels from the device-resident split")

    def fill_synthetic(self, seed: int = 0):
        self._no_host_input("fill_synthetic")
        g = torch.Generator(device="cpu").manual_seed(seed)
        if self.input_mode in ("cifar_u8", "imagenet_u8"):
            self.img_u8.copy_(torch.randint(0, 256, tuple(self.img_u8.shape), generator=g,
                                            dtype=torch.uint8))
        else:
            npix = self.N * self.spec.image_h * self.spec.image_w
            # s2d: every 16-channel row holds 4 pixels of 3 (+1 zero) channels
            self.nat.synthetic_images(self.x_in.data_ptr(), npix, 3,
                                      4 if self.stem_s2d else self.cpad_in, seed,
                                      torch.cuda.current_stream().cuda_stream)
        self.labels.copy_(torch.randint(0, self.spec.num_classes, (self.N,), generator=g,
                                        dtype=torch.int32))

    def metrics(self, reduce: bool = True, top5: bool = False) -> dict:
        """Host read of the last step's scalars (synchronises).  The `cost` term
        wd * 1/2 sum v^2 is exact (pre-update weights) when the step ran with
        need_cost=True; otherwise it is computed now from the updated weights.
        ``reduce``: loss and precision over the whole global batch -- a collective
        that EVERY rank must call at the same point; False: this rank's batch.
        ``top5`` adds `precision_top5` (in-top-k, k = min(5, classes)); without it the
        keys are the ones callers that store every scalar have always got.  With clipping
        on, `grad_norm` and `clip_scale` of the last step are added (clip_state()); with mixup
        on, `mixup_lam` (mixup_state()); with mixup or CutMix on, also `mix_mode` (0 mixup,
        1 CutMix) and, for a CutMix step, `cutmix_area` (mix_state())."""
        if self._cost_at != self._steps_run:
            self._run("cost", torch.cuda.current_stream().cuda_stream)
            self._cost_at = self._steps_run
        v = self.scalars.detach().cpu().tolist()
        self.check_health(v[4])
        loss_sum, correct, lr, l2, top5_sum = v[0], v[1], v[2], v[3], v[5]
        if reduce and self.dist is not None and self.world > 1:
            t = torch.tensor([loss_sum, correct, top5_sum], device=self.device)
            self.dist.all_reduce_sum(t)
            loss_sum, correct, top5_sum = t.tolist()
            n = self.N * self.world
        else:
            n = self.N
        xent = loss_sum / n
        m = {"global_step": int(self.gstep.item()), "cross_entropy": xent,
             "cost": xent + self.wd * l2, "precision": correct / n, "lr": lr, "l2": l2}
        if top5:
            m["precision_top5"] = top5_sum / n
        if self.clip_out is not None:
            m["grad_norm"], m["clip_scale"] = self.clip_out.cpu().tolist()
        if self.adam:
            m["adam_alpha"] = float(self.adam_out[1].item())
        if self.lion:
            m["optimizer"] = "lion"
        if self.rmsprop:
            m["optimizer"] = "rmsprop"
        if self.mix_lam is not None:
            m["mixup_lam"] = float(self.mix_lam[0].item())
            cut = self.cut_log.cpu().tolist() if self.cut_log is not None else [0] * 8
            m["mix_mode"] = int(cut[0])
            if cut[0]:
                m["cutmix_area"] = int(cut[5])
        if self.erase_log is not None:
            box = self.erase_log.cpu().numpy().astype(np.int64)
            m["erase_count"] = int(box[:, 0].sum())
            m["erase_area"] = float((box[:, 3] * box[:, 4]).sum() /
                                    (self.N * self.spec.image_h * self.spec.image_w))
        return m

    def sync_from_params(self, ema_loaded: bool = False):
        """After loading master/stats from a checkpoint: reset step and repack.  The shadows
        start from the loaded weights unless the caller has loaded them too (ema_loaded)."""
        self.gstep.fill_(self.params.global_step)
        if not ema_loaded:
            self.reset_ema()
        self.repack()

    def _replicated(self):
        """The state every rank holds a copy of (the shadows too when EMA is on)."""
        ts = (self.params.master, self.params.stats, self.mom, self.gstep)
        if self.adam:
            ts += (self.adam_v, self.adam_start)
        if self.rmsprop:
            ts += (self.rms_ms,) + ((self.rms_mg,) if self.rmsprop_centered else ())
        return ts + (self.ema,) if self.ema is not None else ts

    def broadcast_parameters(self, src: int = 0):
        """hvd.BroadcastGlobalVariablesHook(0) equivalent: weights, momentum,
        BN moving statistics, global_step (and the EMA shadows) from `src` to every rank."""
        if self.dist is None or self.world == 1:
            return
        if self.comm is not None:
            st = torch.cuda.current_stream().cuda_stream
            for t in self._replicated():
                code = self.nat.COMM_I64 if t.dtype == torch.int64 else self.nat.COMM_F32
                self.comm.broadcast(t.data_ptr(), t.numel(), code, src, st)
        else:
            for t in self._replicated():
                self.dist.broadcast(t, src)
        self.repack()

    # ------------------------------------------------------------------ eval
    def build_eval_plan(self, batch: int, persist: bool | None = None):
        """Forward-only plan in inference mode (BN from moving statistics).  ``persist``:
        True the one-launch persistent forward (train/persist.py PersistInfer; ValueError
        with the reason where the network is not covered), False the launch-per-layer
        plan, None by tune ``persist_eval`` (1: persistent wherever supported, else
        quietly per-layer; -1 auto: the same -- it is the faster plan at every measured
        batch, profiles/cifar_persist_infer.md -- except that tune persist=0 keeps meaning
        "the launch-per-layer engine"; 0: per-layer)."""
        from . import persist as _persist
        from .eval_plan import _EvalPlan
        if persist is None:
            pe = tune.get("persist_eval")
            if pe == 0 or (pe < 0 and tune.get("persist") == 0):
                persist = False
            else:
                persist = _persist.infer_check(self) == ""
        elif persist:
            reason = _persist.infer_check(self)
            if reason:
                raise ValueError(f"persistent eval plan unsupported: {reason}")
        key = (batch, "persistent" if persist else "per-layer")
        if key not in self.eval_plans:
            self.eval_plans[key] = _EvalPlan(self, batch, persist=bool(persist))
        return self.eval_plans[key]
