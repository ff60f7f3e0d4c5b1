"""Step time with --cutmix_alpha off and on, on one GPU (profiles/cutmix.md): engines of the
same network in one process, timed interleaved, rounds x variants, best / median / max
ms/step as JSON lines:
    default   mixup and CutMix off (the plan of a tree without the flags, op for op)
    mixup     mixup_alpha=0.2 (the mixup-only launch, as before CutMix)
    cutmix    cutmix_alpha=1.0 (every step pastes)
    switch    mixup_alpha=0.2, cutmix_alpha=1.0, mix_switch_prob=0.5
then the input launch alone -- unmixed, mixup, and the CutMix kernel in a pasting and in a
blending step -- timed with events around back-to-back launches over different output
buffers.  `default` and `mixup` are scripts/mixup_step_time.py's variants of the same name,
so a tree without CutMix is measured with that script.

    python scripts/cutmix_step_time.py [cifar_resnet50:128,...] [steps] [rounds] [variants]
"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import distributed_tensorflow_resnet_amd as dtr  # noqa: E402
import distributed_tensorflow_resnet_amd.train.engine as E  # noqa: E402
from distributed_tensorflow_resnet_amd.models.spec import build_spec  # noqa: E402

VARIANTS = {"default": {}, "mixup": {"mixup_alpha": 0.2}, "cutmix": {"cutmix_alpha": 1.0},
            "switch": {"mixup_alpha": 0.2, "cutmix_alpha": 1.0, "mix_switch_prob": 0.5}}


def build(model, N, variant):
    dataset, size = model.split("_resnet")
    cifar = dataset.startswith("cifar")
    eng = E.Engine(build_spec(dataset, int(size)), N, weight_decay=2e-4 if cifar else 1e-4,
                   lr_schedule=E.cifar_lr_schedule() if cifar else E.imagenet_lr_schedule(),
                   device=torch.device("cuda", 0),
                   input_mode="cifar_u8" if cifar else "imagenet_u8", **VARIANTS[variant])
    eng.fill_synthetic(0)
    for _ in range(20):
        eng.step()
    torch.cuda.synchronize()
    return eng


def timed(eng, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        eng.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def input_alone(N, reps=50):
    """us per cifar_augment launch of N images: `reps` launches into `reps` different output
    buffers, the best and the median of 5 batches, per kind of launch."""
    nat = dtr.native(required=True)
    dev = torch.device("cuda", 0)
    img = torch.randint(0, 256, (N, 3, 32, 32), dtype=torch.uint8, device=dev)
    labels = torch.zeros(N, dtype=torch.int32, device=dev)
    outs = [torch.empty((N, 32, 32, 8), dtype=torch.bfloat16, device=dev) for _ in range(reps)]
    gstep = torch.zeros(1, dtype=torch.int64, device=dev)
    table = torch.full((4096,), 0.3, device=dev)
    cuts = torch.full((4096,), 16 << 16 | 16, dtype=torch.int32, device=dev)   # a 16 x 16 box
    labels_b, lam = torch.zeros_like(labels), torch.zeros(N, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    mix = (table.data_ptr(), 4096, labels.data_ptr(), labels_b.data_ptr(), lam.data_ptr(), 0)

    def batch(extra):
        res = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for o in outs:
                nat.cifar_augment(img.data_ptr(), o.data_ptr(), N, 32, 32, 8, 4, 1234,
                                  gstep.data_ptr(), 1, 0, 0, 0, *extra, st)
            b.record()
            torch.cuda.synchronize()
            res.append(a.elapsed_time(b) * 1e3 / reps)
        return [round(min(res), 3), round(statistics.median(res), 3)]

    # the CutMix kernel at threshold 2^24 pastes in every step, at 1 (of 2^24) it blends
    return {"unmixed_us": batch(()), "mixup_us": batch(mix),
            "cutmix_paste_us": batch((*mix, cuts.data_ptr(), 1 << 24, 0)),
            "cutmix_blend_us": batch((*mix, cuts.data_ptr(), 1, 0))}


def main():
    cases = (sys.argv[1] if len(sys.argv) > 1 else
             "cifar_resnet50:128,cifar_resnet50:16").split(",")
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    variants = (sys.argv[4] if len(sys.argv) > 4 else "default,mixup,cutmix,switch").split(",")
    for case in cases:
        model, N = case.split(":")
        N = int(N)
        engs = {v: build(model, N, v) for v in variants}
        res = {name: [] for name in engs}
        for _ in range(rounds):
            for name, eng in engs.items():
                res[name].append(timed(eng, steps))
        for name, eng in engs.items():
            assert not eng.persist_error(), name
            print(json.dumps({"model": model, "batch": N, "variant": name, "steps": steps,
                              "rounds": rounds, "best_ms": round(min(res[name]), 4),
                              "median_ms": round(statistics.median(res[name]), 4),
                              "max_ms": round(max(res[name]), 4),
                              "plan": "persistent" if eng.persist else "per-layer",
                              "plan_ops": eng.plan.size()}), flush=True)
        del engs
        torch.cuda.empty_cache()
        if model.startswith("cifar") and "cutmix" in variants:
            print(json.dumps({"model": model, "batch": N, "input_launch": input_alone(N)}),
                  flush=True)


if __name__ == "__main__":
    main()
