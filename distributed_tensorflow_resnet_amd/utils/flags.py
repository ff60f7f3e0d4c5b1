"""Command-line flags with the reference's names and defaults.

The reference defines ~25 `tf.app.flags` per entrypoint (resnet_cifar_main.py:
34-97, resnet_imagenet_main.py:33-104, resnet_model.py:30, the *_eval.py
scripts).  One argparse builder reproduces them all -- same spelling, same
defaults per entrypoint -- and accepts absl's boolean spellings (`--flag`,
`--noflag`, `--flag=true|false`).  New flags for this framework:

  --resnet_size      (reference hard-codes 50, resnet_model.py:72,74 -- defect #8)
  --dtype            bf16 (GPU compute) | fp32 (CPU path)
  --synthetic        synthetic data of the dataset's shape
  --resident_data    CIFAR split resident on the GPU, shuffled on the device
  --ema_decay        device-side EMA of the weights, checkpointed; --eval_ema scores it
  --clip_grad_norm   clip the gradient by its global norm on the device (inf: only log it)
  --optimizer adamw  Adam with decoupled (or l2) weight decay in one device launch:
                     --adam_beta1/_beta2/_epsilon, --adam_decay, --adam_decay_skip;
                     --adam_trust on makes it LAMB (per-tensor trust ratios), --adam_trust_skip
  --optimizer lion   Lion (sign of an interpolated momentum, one state buffer) in one device
                     launch: --lion_beta1/_beta2, --lion_decay_skip
  --optimizer rmsprop  tf.train.RMSPropOptimizer's form (momentum, epsilon inside the root) in
                     one device launch: --rmsprop_rho/_momentum/_epsilon, --rmsprop_centered,
                     --rmsprop_wd, --rmsprop_decay_skip
  --lr_decay         piecewise | cosine | poly, with --lr_peak, --lr_warmup_steps/_from,
                     --lr_decay_steps, --lr_end, --lr_poly_power (evaluated on the device)
  --bucket_mb        gradient all-reduce bucket size
  --device           auto | gpu | cpu
  --use_graph        capture the training step in a hipGraph
  --seed, --log_every, --save_checkpoint_steps/_secs, --profile_steps, ...
"""
from __future__ import annotations

import argparse
import sys

VARIABLE_UPDATES = ("parameter_server", "replicated", "distributed_replicated", "independent",
                    "distributed_all_reduce", "collective_all_reduce", "horovod")

_DEFAULTS = {
    # name: (cifar, imagenet)
    "dataset": ("cifar10", "imagenet"),
    "train_data_path": ("/home/hdd0/dataset/cifar10_data", ""),
    "train_steps": (2000, 200),
    "batch_size": (32, 128),
    "resnet_size": (50, 50),
    "log_every": (20, 40),            # LoggingTensorHook every_n_iter
    "weight_decay": (2e-4, 1e-4),     # _WEIGHT_DECAY (resnet_cifar_main.py:112) / :472
}


def str2bool(v) -> bool:
    if isinstance(v, bool):
        return v
    s = str(v).strip().lower()
    if s in ("1", "true", "t", "yes", "y"):
        return True
    if s in ("0", "false", "f", "no", "n"):
        return False
    raise argparse.ArgumentTypeError(f"not a boolean: {v!r}")


def _smoothing(v) -> float:
    try:
        f = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {v!r}") from None
    if not 0.0 <= f < 1.0:
        raise argparse.ArgumentTypeError(f"label smoothing must be in [0, 1), got {v!r}")
    return f


def _ema_decay(v) -> float:
    try:
        f = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {v!r}") from None
    if not 0.0 <= f < 1.0:
        raise argparse.ArgumentTypeError(f"EMA decay must be in [0, 1), got {v!r}")
    return f


def _adam_beta(v) -> float:
    try:
        f = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {v!r}") from None
    if not 0.0 <= f < 1.0:   # NaN included
        raise argparse.ArgumentTypeError(f"an Adam beta must be in [0, 1), got {v!r}")
    return f


def _lion_beta(v) -> float:
    try:
        f = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {v!r}") from None
    if not 0.0 <= f < 1.0:   # NaN included
        raise argparse.ArgumentTypeError(f"a Lion beta must be in [0, 1), got {v!r}")
    return f


def _rmsprop_coef(v) -> float:
    try:
        f = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {v!r}") from None
    if not 0.0 <= f < 1.0:   # NaN included
        raise argparse.ArgumentTypeError(f"rmsprop's rho and momentum must be in [0, 1), got {v!r}")
    return f


def _rmsprop_epsilon(v) -> float:
    try:
        f = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {v!r}") from None
    if not 0.0 < f < float("inf"):   # zero, negative, inf or NaN
        raise argparse.ArgumentTypeError(f"rmsprop's epsilon must be positive and finite, got {v!r}")
    return f


def _adam_epsilon(v) -> float:
    try:
        f = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {v!r}") from None
    if not 0.0 < f < float("inf"):   # zero, negative, inf or NaN
        raise argparse.ArgumentTypeError(f"the Adam epsilon must be positive and finite, got {v!r}")
    return f


def _clip_norm(v) -> float:
    try:
        f = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {v!r}") from None
    if not f >= 0.0:   # negative or NaN
        raise argparse.ArgumentTypeError(f"clip norm must be 0 (off), positive or inf, got {v!r}")
    return f


def _mixup_alpha(v) -> float:
    try:
        f = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {v!r}") from None
    if not 0.0 <= f < float("inf"):   # negative, inf or NaN
        raise argparse.ArgumentTypeError(f"mixup alpha must be finite and >= 0, got {v!r}")
    return f


def _cutmix_alpha(v) -> float:
    try:
        f = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {v!r}") from None
    if not 0.0 <= f < float("inf"):   # negative, inf or NaN
        raise argparse.ArgumentTypeError(f"cutmix alpha must be finite and >= 0, got {v!r}")
    return f


def _unit_float(what: str):
    """argparse type: a float in [0, 1] (NaN refused), named `what` in the error."""
    def parse(v) -> float:
        try:
            f = float(v)
        except ValueError:
            raise argparse.ArgumentTypeError(f"not a number: {v!r}") from None
        if not 0.0 <= f <= 1.0:   # NaN included
            raise argparse.ArgumentTypeError(f"{what} must be in [0, 1], got {v!r}")
        return f
    return parse


_switch_prob = _unit_float("a switch probability")
_erase_prob = _unit_float("an erase probability")


def _lr_rate(v) -> float:
    try:
        f = float(v)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {v!r}") from None
    if not 0.0 <= f < float("inf"):   # negative, inf or NaN
        raise argparse.ArgumentTypeError(f"a learning rate must be finite and >= 0, got {v!r}")
    return f


def _absl_bools(argv, bool_names):
    """Translate absl `--noflag` / bare `--flag` spellings for boolean flags."""
    out = []
    for a in argv:
        if a.startswith("--no") and a[4:] in bool_names:
            out.append(f"--{a[4:]}=false")
        elif a.startswith("--") and "=" not in a and a[2:] in bool_names:
            out.append(f"--{a[2:]}=true")
        else:
            out.append(a)
    return out


class FlagParser(argparse.ArgumentParser):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self._bools = set()

    def add_bool(self, name, default, help_):
        self._bools.add(name)
        self.add_argument(f"--{name}", type=str2bool, default=default, nargs="?", const=True,
                          help=help_)

    def parse_args(self, args=None, namespace=None):
        argv = sys.argv[1:] if args is None else list(args)
        ns = super().parse_args(_absl_bools(argv, self._bools), namespace)
        if getattr(ns, "clip_grad_norm", 0.0) > 0 and getattr(ns, "optimizer", "") == "lars":
            self.error("--clip_grad_norm cannot be combined with --optimizer lars: the trust "
                       "ratio already normalises by the gradient norm")
        if hasattr(ns, "adam_beta1"):
            from ..train.layout import check_adam

            try:   # (the fp32 values the kernel gets: a beta that rounds to 1, an epsilon to 0)
                check_adam(ns.adam_beta1, ns.adam_beta2, ns.adam_epsilon, ns.adam_decay,
                           ns.adam_decay_skip)
            except ValueError as e:
                self.error(str(e))
        if hasattr(ns, "lion_beta1"):
            from ..train.layout import check_lion

            try:   # (the fp32 values the kernel gets: a beta that rounds to 1)
                check_lion(ns.lion_beta1, ns.lion_beta2, ns.lion_decay_skip)
            except ValueError as e:
                self.error(str(e))
        if hasattr(ns, "rmsprop_rho"):
            from ..train.layout import check_rmsprop

            try:   # (the fp32 values the kernel gets: a rho that rounds to 1, an epsilon to 0)
                check_rmsprop(ns.rmsprop_rho, ns.rmsprop_momentum, ns.rmsprop_epsilon,
                              ns.rmsprop_centered, ns.rmsprop_wd, ns.rmsprop_decay_skip)
            except ValueError as e:
                self.error(str(e))
        if hasattr(ns, "adam_trust"):
            from ..train.layout import check_adam_trust

            try:   # on: layer-wise adaptation of adamw, of no other optimizer
                check_adam_trust(ns.adam_trust, ns.adam_trust_skip,
                                 getattr(ns, "optimizer", "adamw"))
            except ValueError as e:
                self.error("--adam_trust: " + str(e))
        if getattr(ns, "mixup_alpha", 0.0) > 0 and getattr(ns, "synthetic", False):
            self.error("--mixup_alpha cannot be combined with --synthetic: the synthetic "
                       "input has no input launch to mix in")
        if getattr(ns, "cutmix_alpha", 0.0) > 0 and getattr(ns, "synthetic", False):
            self.error("--cutmix_alpha cannot be combined with --synthetic: the synthetic "
                       "input has no input launch to paste in")
        if hasattr(ns, "mix_switch_prob"):
            if ns.mix_switch_prob is None:   # not given
                ns.mix_switch_prob = 0.5
            elif not (getattr(ns, "mixup_alpha", 0.0) > 0 and getattr(ns, "cutmix_alpha", 0.0) > 0):
                self.error("--mix_switch_prob chooses between mixup and CutMix per step: it needs "
                           "--mixup_alpha > 0 and --cutmix_alpha > 0")
        if hasattr(ns, "erase_prob"):
            from ..train.layout import check_erase

            try:   # the sub-flags are checked, and otherwise unused, at --erase_prob 0
                check_erase(ns.erase_prob, ns.erase_area_min, ns.erase_area_max,
                            ns.erase_aspect_min, ns.erase_fill, getattr(ns, "dataset", ""))
            except ValueError as e:
                self.error("--erase_prob: " + str(e))
            if ns.erase_prob > 0 and getattr(ns, "synthetic", False):
                self.error("--erase_prob cannot be combined with --synthetic: the synthetic "
                           "input has no input launch to erase behind")
        if hasattr(ns, "lr_decay"):
            from ..train.schedule import schedule_from_flags

            try:   # the run's schedule must exist: decay_steps > warm-up, power > 0, ...
                schedule_from_flags(ns)
            except ValueError as e:
                self.error(str(e))
        return ns

    def parse_known_args(self, args=None, namespace=None):
        argv = sys.argv[1:] if args is None else list(args)
        return super().parse_known_args(_absl_bools(argv, self._bools), namespace)


def build_parser(kind: str = "cifar", description: str | None = None) -> FlagParser:
    """kind: cifar | imagenet (train entrypoints), cifar_eval | imagenet_eval, single."""
    from ..train.layout import ERASE_FILLS

    im = 1 if kind.startswith("imagenet") else 0
    p = FlagParser(description=description, allow_abbrev=False)
    d = {k: v[im] for k, v in _DEFAULTS.items()}
    is_eval = kind.endswith("_eval")
    # ---- reference flags (resnet_cifar_main.py:34-97 / resnet_imagenet_main.py:33-104)
    p.add_argument("--dataset", default=d["dataset"], help="cifar10, cifar100 or imagenet")
    p.add_argument("--mode", default="eval" if is_eval else "train",
                   help="train | eval | train_and_eval")
    p.add_argument("--train_data_path", default=d["train_data_path"],
                   help="Filepattern/dir for training data.")
    p.add_argument("--eval_data_path", default="", help="Filepattern/dir for eval data")
    p.add_argument("--image_size", type=int, default=32, help="Image side length (declared, unused).")
    p.add_argument("--train_dir", default="", help="Directory to keep training outputs (checkpoints).")
    p.add_argument("--eval_dir", default="", help="Directory to keep eval outputs.")
    p.add_argument("--eval_batch_count", type=int, default=50, help="Number of batches to eval.")
    p.add_bool("eval_once", False, "Whether evaluate the model only once.")
    p.add_argument("--log_dir", default="", help="Directory for training summaries.")
    p.add_argument("--log_root", default="", help="Legacy root dir (resnet_single/eval scripts).")
    p.add_argument("--num_gpus", type=int, default=0,
                   help="GPUs per worker (reference: gpu = task_index %% num_gpus).")
    p.add_argument("--task_index", type=int, default=None, help="Worker index (PS mode).")
    p.add_argument("--replicas_to_aggregate", type=int, default=None,
                   help="Gradients to aggregate per step (PS sync mode).")
    p.add_argument("--train_steps", type=int, default=d["train_steps"],
                   help="Number of (global) training steps to perform.")
    p.add_argument("--num_epochs", type=int, default=90 if im else 1000, help="Dataset repeats.")
    p.add_argument("--batch_size", type=int, default=d["batch_size"], help="Per-process batch size.")
    p.add_argument("--learning_rate", type=float, default=0.01,
                   help="Declared, unused by ResNet (the LR schedule hook sets it).")
    p.add_argument("--_FILE_SHUFFLE_BUFFER", type=float, default=1024)
    p.add_argument("--_SHUFFLE_BUFFER", type=float, default=1024)
    p.add_bool("sync_replicas", True, "Synchronous replicas (always true here: sync DP).")
    p.add_bool("existing_servers", False, "Use existing servers (PS mode; ignored).")
    p.add_argument("--ps_hosts", default="localhost:2222", help="PS hosts (ignored: no PS).")
    p.add_argument("--worker_hosts", default="localhost:2223,localhost:2224",
                   help="Worker hosts; for multi-node runs use MASTER_ADDR/torchrun instead.")
    p.add_argument("--job_name", default=None, help="worker | ps")
    p.add_argument("--data_format", default="channels_first",
                   help="Accepted for compatibility; kernels are always NHWC.")
    p.add_argument("--num_intra_threads", type=int, default=0)
    p.add_argument("--num_inter_threads", type=int, default=0)
    p.add_argument("--variable_update", default="parameter_server", choices=VARIABLE_UPDATES,
                   help="All synchronous modes map to RCCL all-reduce data parallelism; "
                        "'independent' trains ranks without gradient exchange.")
    p.add_bool("use_horovod", False, "Accepted for compatibility (all-reduce is always on).")
    p.add_argument("--num_parallel_calls", type=int, default=5, help="Input pipeline workers.")
    # ---- new flags
    p.add_argument("--resnet_size", type=int, default=d["resnet_size"])
    p.add_argument("--num_classes", type=int, default=None)
    p.add_argument("--device", default="auto", choices=("auto", "gpu", "cpu"))
    p.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"))
    p.add_bool("synthetic", False, "Synthetic data of the dataset's shape.")
    p.add_bool("resident_data", False,
               "CIFAR on the GPU, real data: keep the whole split on the device and let the "
               "step's input launch pick its records through a keyed permutation of "
               "global_step (no per-step host work; the order is a function of --seed and "
               "the step, so a resumed run continues its epoch).  Ignored otherwise.")
    p.add_argument("--weight_decay", type=float, default=d["weight_decay"])
    p.add_argument("--optimizer", default="mom", choices=("mom", "sgd", "lars", "adamw", "lion", "rmsprop"),
                   help="mom / sgd: the reference's optimizers.  lars: SGD-momentum at a "
                        "per-tensor rate lr * trust, trust = eeta * |w| / (|g| + wd * |w| + "
                        "epsilon) (layer-wise adaptive rate scaling, for large global batches).  "
                        "adamw: Adam (tf.train.AdamOptimizer's form) with decoupled weight "
                        "decay; the presets' learning rates are SGD rates, so set --lr_peak "
                        "(e.g. 1e-3) or --lr_value_scale with it.  lion: the sign of an "
                        "interpolated momentum (Chen et al. 2023) with decoupled weight decay "
                        "and one state buffer; every element moves by lr, so set a rate well "
                        "below adamw's (the paper: 3-10x) and a correspondingly larger decay.  "
                        "rmsprop: tf.train.RMSPropOptimizer's form (timm's rmsproptf): momentum, "
                        "epsilon inside the square root, ms from ones, no bias correction; the "
                        "presets' learning rates (0.1 / 0.4) are SGD rates, so set --lr_peak "
                        "(e.g. 1e-3) with it; the recipe-scale epsilon (TF-slim uses 1.0) is "
                        "--rmsprop_epsilon's to set.")
    p.add_argument("--adam_beta1", type=_adam_beta, default=0.9,
                   help="adamw: decay of the first moment, in [0, 1).")
    p.add_argument("--adam_beta2", type=_adam_beta, default=0.999,
                   help="adamw: decay of the second moment, in [0, 1).")
    p.add_argument("--adam_epsilon", type=_adam_epsilon, default=1e-8,
                   help="adamw: added to sqrt(v), outside the bias correction (TF's epsilon "
                        "hat); > 0.")
    p.add_argument("--adam_decay", default="decoupled", choices=("decoupled", "l2"),
                   help="adamw: 'decoupled' = w -= lr * wd * w beside the Adam step (Loshchilov "
                        "& Hutter), 'l2' = wd * w added to the gradient (plain Adam on the "
                        "reference's cost).")
    p.add_argument("--adam_decay_skip", default="none", choices=("none", "vectors"),
                   help="adamw: tensors without weight decay: 'none' = every trainable is "
                        "decayed (this project's rule), 'vectors' = every rank-1 tensor (BN "
                        "gamma / beta, the dense bias) is not.")
    p.add_argument("--adam_trust", default="off", choices=("off", "on"),
                   help="adamw: 'on' = LAMB (You et al. 2020), the Adam direction u at a "
                        "per-tensor rate lr * trust, trust = |w| / |u| (layer-wise adaptation, "
                        "for large global batches); an error with any other --optimizer.")
    p.add_argument("--adam_trust_skip", default="vectors", choices=("vectors", "none"),
                   help="--adam_trust on: tensors that are not adapted (trust = 1): 'vectors' = "
                        "every rank-1 tensor (BN gamma / beta, the dense bias), 'none' = adapt "
                        "them too.  Unused with --adam_trust off.")
    p.add_argument("--lion_beta1", type=_lion_beta, default=0.9,
                   help="lion: weight of the momentum in the interpolation whose sign is the "
                        "update, in [0, 1).")
    p.add_argument("--lion_beta2", type=_lion_beta, default=0.99,
                   help="lion: decay of the momentum, in [0, 1).")
    p.add_argument("--lion_decay_skip", default="none", choices=("none", "vectors"),
                   help="lion: tensors without weight decay, as --adam_decay_skip.")
    p.add_argument("--rmsprop_rho", type=_rmsprop_coef, default=0.9,
                   help="rmsprop: decay of the mean square (TF's `decay`), in [0, 1).")
    p.add_argument("--rmsprop_momentum", type=_rmsprop_coef, default=0.9,
                   help="rmsprop: momentum, in [0, 1).  0.9 is TF-slim's value; TF's own default "
                        "of 0 is a valid setting.")
    p.add_argument("--rmsprop_epsilon", type=_rmsprop_epsilon, default=1e-10,
                   help="rmsprop: epsilon, inside the square root; must be > 0.  1e-10 is TF's "
                        "default; TF-slim's recipes use 1.0.")
    p.add_bool("rmsprop_centered", False,
               "rmsprop: the centered form (the denominator is the estimated variance: a third "
               "state buffer mg).")
    p.add_argument("--rmsprop_wd", default="l2", choices=("l2", "decoupled"),
                   help="rmsprop: l2 = the decay term is part of the gradient (plain TF RMSProp "
                        "on the reference's cost); decoupled = taken off the old weight at the "
                        "scheduled lr, as adamw's.")
    p.add_argument("--rmsprop_decay_skip", default="none", choices=("none", "vectors"),
                   help="rmsprop: tensors without weight decay, as --adam_decay_skip.")
    p.add_argument("--lars_eeta", type=float, default=0.001,
                   help="LARS trust coefficient.")
    p.add_argument("--lars_epsilon", type=float, default=0.0,
                   help="Added to the denominator of the LARS trust ratio.")
    p.add_argument("--lars_skip", default="vectors", choices=("vectors", "none"),
                   help="Tensors LARS does not adapt (trust = 1; they keep their weight decay): "
                        "'vectors' = every rank-1 tensor (BN gamma / beta, the dense bias), "
                        "'none' = adapt them too.")
    p.add_argument("--label_smoothing", type=_smoothing, default=0.0,
                   help="Training-loss label smoothing eps in [0, 1): targets (1 - eps) * onehot "
                        "+ eps / classes (tf.losses.softmax_cross_entropy's label_smoothing).  "
                        "Evaluation is never smoothed.")
    p.add_argument("--ema_decay", type=_ema_decay, default=0.0,
                   help="Keep an exponential moving average of the trainable weights on the "
                        "device: shadow -= (1 - decay) * (shadow - weight) after every step "
                        "(tf.train.ExponentialMovingAverage; 0.9999 is TF's usual value), saved "
                        "as <name>/ExponentialMovingAverage.  In [0, 1); 0 = off.")
    p.add_argument("--clip_grad_norm", type=_clip_norm, default=0.0,
                   help="Clip the gradient by its global norm (tf.clip_by_global_norm): the "
                        "update uses g * min(1, c / |g|), |g| over all trainables of the "
                        "all-reduced mean gradient, before weight decay (the decay term is not "
                        "clipped).  The norm and the scale are logged (grad_norm, clip_scale); a "
                        "non-finite norm gives a NaN scale.  0 = off, inf = only measure.  Not "
                        "with --optimizer lars.  On the persistent step it replaces the "
                        "one-launch optimizer by the generic one.")
    p.add_argument("--mixup_alpha", type=_mixup_alpha, default=0.0,
                   help="Mixup (Zhang et al. 2018) on the device: every step trains on lam * x + "
                        "(1 - lam) * x' with the targets mixed the same way, x' the batch rotated "
                        "by a per-step shift, lam ~ Beta(alpha, alpha) (one draw per step and "
                        "rank, a function of the seed and global_step, so a resumed run continues "
                        "the sequence).  Training precision is counted against the dominant "
                        "label; evaluation never mixes.  0 = off.  Needs real data (not "
                        "--synthetic); on the GPU, CIFAR or the uint8 ImageNet feed.")
    p.add_argument("--cutmix_alpha", type=_cutmix_alpha, default=0.0,
                   help="CutMix (Yun et al. 2019) on the device: a step pastes one box of x' (the "
                        "batch rotated by the per-step shift) into x and trains against both "
                        "labels at lam = 1 - box area / image area.  The box's area share is "
                        "1 - Beta(alpha, alpha), its centre uniform, clipped at the borders; one "
                        "box per step and rank, a function of the seed and global_step.  0 = off. "
                        " With --mixup_alpha > 0 too, each step is one or the other "
                        "(--mix_switch_prob).  Same input requirements as --mixup_alpha.")
    p.add_argument("--mix_switch_prob", type=_switch_prob, default=None,
                   help="Probability in [0, 1] that a step is a CutMix step when --mixup_alpha "
                        "and --cutmix_alpha are both > 0 (default 0.5).  An error otherwise.")
    p.add_argument("--erase_prob", type=_erase_prob, default=0.0,
                   help="Random Erasing (Zhong et al. 2020; with the zero fill, Cutout) on the "
                        "device: each training image gets, with this probability, one random "
                        "rectangle overwritten by the fill, in a launch of its own behind the "
                        "input launch (after mixup / CutMix).  The draw is per image, a function "
                        "of the seed, global_step and the batch position.  0 = off.  Evaluation "
                        "never erases.  Same input requirements as --mixup_alpha.")
    p.add_argument("--erase_area_min", type=float, default=0.02,
                   help="--erase_prob: smallest erased share of the image (0 < min <= max <= 1).")
    p.add_argument("--erase_area_max", type=float, default=1.0 / 3.0,
                   help="--erase_prob: largest erased share of the image.")
    p.add_argument("--erase_aspect_min", type=float, default=0.3,
                   help="--erase_prob: the box's aspect ratio is log-uniform in [a, 1 / a]; a in "
                        "(0, 1].")
    p.add_argument("--erase_fill", default="zero", choices=ERASE_FILLS,
                   help="--erase_prob: 'zero' = the mean pixel of the standardised input, "
                        "'noise' = unit normal values from a host-made table (CIFAR only: an "
                        "error with ImageNet, whose inputs are not scaled).")
    p.add_bool("ema_warmup", True,
               "EMA decay min(decay, (1 + step) / (10 + step)), as TF's num_updates=global_step: "
               "the average forgets the initial weights quickly.")
    p.add_bool("eval_ema", False,
               "Evaluate the checkpoint's EMA shadows instead of its raw weights (BN moving "
               "statistics stay the raw ones); an error if the checkpoint has none.")
    p.add_argument("--bucket_mb", type=float, default=0.0,
                   help="All-reduce bucket size (MiB); 0 = auto (~4 buckets, <= 25 MiB).")
    p.add_bool("use_graph", False, "Capture the training step in a hipGraph (single stream; "
               "default eager native plan with a second weight-gradient stream).")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--log_every", type=int, default=d["log_every"])
    p.add_argument("--summary_every", type=int, default=100)
    p.add_argument("--save_checkpoint_steps", type=int, default=1000)
    p.add_argument("--save_checkpoint_secs", type=float, default=0.0,
                   help="If > 0, checkpoint every N seconds (Horovod path used 60).")
    p.add_argument("--max_to_keep", type=int, default=5)
    p.add_argument("--eval_interval_secs", type=float, default=60.0)
    p.add_argument("--eval_batch_size", type=int, default=100)
    p.add_argument("--profile_steps", default="", help="e.g. '50:60' -> per-phase timing report")
    p.add_bool("check_numerics", False, "Abort on NaN/Inf loss (tf.check_numerics analogue).")
    p.add_argument("--fault_kill_step", type=int, default=-1,
                   help="Fault injection: rank --fault_kill_rank exits at this step.")
    p.add_argument("--fault_kill_rank", type=int, default=0)
    p.add_bool("reset_persist_fault", False,
               "Delete the persist_fault marker in --train_dir (left by an attempt whose "
               "persistent CIFAR step failed a grid barrier) so this attempt selects the "
               "persistent step again.")
    p.add_argument("--step_watchdog_secs", type=float, default=0.0,
                   help="If > 0, abort (exit 3, for the launcher to restart from the latest "
                        "checkpoint) when no step completes for this many seconds.  Multi-rank "
                        "jobs always run the watchdog (limit --comm_timeout_secs when this is 0), "
                        "which also polls the native communicator's async error.")
    p.add_argument("--comm_timeout_secs", type=float, default=600.0,
                   help="Collective timeout: the process group's, the native communicator's "
                        "init / shm waits, and the multi-rank step watchdog's default limit "
                        "(on expiry: ncclCommAbort, exit 3).")
    p.add_argument("--lr_schedule_scale", type=float, default=1.0,
                   help="Multiply the LR schedule's step boundaries (and warm-up) by this "
                        "factor: compressed schedules for short runs (convergence tests).")
    p.add_argument("--lr_value_scale", type=float, default=1.0,
                   help="Multiply every LR value of the schedule (and its warm-up) by this "
                        "factor: the linear scaling rule when the global batch differs from "
                        "the reference's (ImageNet: 0.4 for 8 x 128 images).")
    p.add_argument("--lr_decay", default="piecewise", choices=("piecewise", "cosine", "poly"),
                   help="Shape of the LR schedule after its warm-up: the reference's piecewise "
                        "steps, or a decay from --lr_peak to --lr_end over --lr_decay_steps, "
                        "evaluated on the device like the steps: cosine, end + (peak - end) * "
                        "0.5 (1 + cos(pi p)), or poly, end + (peak - end) * (1 - p)^power, with "
                        "p = (t - warmup) / (decay_steps - warmup) and t = step - 1 (the "
                        "reference's hook feeds step s the rate of s - 1).  LARS recipes use "
                        "warm-up + poly (power 2).")
    p.add_argument("--lr_peak", type=_lr_rate, default=None,
                   help="Rate after the warm-up (piecewise: its first value, the drops keep "
                        "their ratios).  Default: the dataset's (CIFAR 0.1, ImageNet 0.4), "
                        "before --lr_value_scale.")
    p.add_argument("--lr_warmup_steps", type=int, default=-1,
                   help="Linear warm-up length; -1 = the dataset's (CIFAR 0, ImageNet 6240).  "
                        "A value >= 0 also applies to --lr_decay piecewise.")
    p.add_argument("--lr_warmup_from", type=_lr_rate, default=None,
                   help="Rate the warm-up starts from.  Default: the dataset's (ImageNet 0.1), "
                        "0 where it has none.")
    p.add_argument("--lr_decay_steps", type=int, default=0,
                   help="cosine / poly: the step at which the rate reaches --lr_end and stays "
                        "there; 0 = --train_steps.  Must exceed the warm-up.")
    p.add_argument("--lr_end", type=_lr_rate, default=0.0, help="cosine / poly: the final rate.")
    p.add_argument("--lr_poly_power", type=float, default=2.0,
                   help="poly: the exponent (> 0).")
    p.add_argument("--allreduce_dtype", default="fp32", choices=("fp32", "bf16"),
                   help="Gradient all-reduce precision: bf16 halves the bytes on xGMI (fp32 "
                        "master weights and optimizer are unchanged).")
    return p


def warn_unsupported(flags, log) -> None:
    """Flags the MI355X framework accepts but does not act on (PS/gRPC topology)."""
    if flags.variable_update == "parameter_server" and flags.job_name:
        log(f"[flags] --variable_update=parameter_server --job_name={flags.job_name}: parameter "
            "servers are not rebuilt; running synchronous RCCL data parallelism instead.")
        if flags.job_name == "ps":
            log("[flags] this process was started as a PS task and has nothing to do; exiting.")
    if not flags.sync_replicas:
        log("[flags] --sync_replicas=False (async PS) is not supported; training synchronously.")
