"""Step time with --erase_prob off and on, on one GPU (profiles/random_erasing.md): engines of
the same network in one process, timed interleaved, rounds x variants, best / median / max
ms/step as JSON lines:
    default   erasing off (the plan of a tree without the flag, op for op)
    erase     erase_prob=0.25, zero fill (one more launch behind the input launch)
    erase1    erase_prob=1.0: every image is erased
    noise     erase_prob=1.0, noise fill (CIFAR only)
then the erase launch alone, timed with events around back-to-back launches over different
buffers.  `default` passes no new argument, so a tree without the flag is measured with this
same script and `default` alone.

    python scripts/erase_step_time.py [cifar_resnet50:128,...] [steps] [rounds] [variants]
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

VARIANTS = {"default": {}, "erase": {"erase_prob": 0.25}, "erase1": {"erase_prob": 1.0},
            "noise": {"erase_prob": 1.0, "erase_fill": "noise"}}


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


def erase_alone(N, H, W, s2d, reps=50):
    """us per erase_boxes launch over N images: `reps` launches over `reps` different buffers,
    the best and the median of 5 batches, per threshold and fill."""
    from distributed_tensorflow_resnet_amd.data import cifar

    nat = dtr.native(required=True)
    dev = torch.device("cuda", 0)
    shape = (N, H // 2, W // 2, 16) if s2d else (N, H, W, 8)
    bufs = [torch.zeros(shape, dtype=torch.bfloat16, device=dev) for _ in range(reps)]
    gstep = torch.zeros(1, dtype=torch.int64, device=dev)
    table = torch.from_numpy(cifar.erase_table(1234, H, W)).to(dev)
    noise = torch.from_numpy(cifar.erase_noise_table(1234)).to(dev)
    st = torch.cuda.current_stream().cuda_stream

    def batch(thresh, nz):
        res = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for x in bufs:
                nat.erase_boxes(x.data_ptr(), N, H, W, 8, int(s2d), 1234, gstep.data_ptr(),
                                table.data_ptr(), table.numel(), thresh,
                                nz.data_ptr() if nz is not None else 0,
                                nz.numel() if nz is not None else 0, 0, st)
            b.record()
            torch.cuda.synchronize()
            res.append(a.elapsed_time(b) * 1e3 / reps)
        return [round(min(res), 3), round(statistics.median(res), 3)]

    out = {"off_us": batch(0, None), "p25_zero_us": batch(1 << 22, None),
           "p100_zero_us": batch(1 << 24, None)}
    if H == 32:
        out["p100_noise_us"] = batch(1 << 24, noise)
    return out


def main():
    cases = (sys.argv[1] if len(sys.argv) > 1 else
             "cifar_resnet50:128,imagenet_resnet50:128").split(",")
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    variants = (sys.argv[4] if len(sys.argv) > 4 else "default,erase,erase1").split(",")
    for case in cases:
        model, N = case.split(":")
        N = int(N)
        engs = {v: build(model, N, v) for v in variants
                if not (v == "noise" and model.startswith("imagenet"))}
        res = {name: [] for name in engs}
        for _ in range(rounds):
            for name, eng in engs.items():
                res[name].append(timed(eng, steps))
        s2d = False
        for name, eng in engs.items():
            assert not eng.persist_error(), name
            s2d = bool(eng.stem_s2d)
            print(json.dumps({"model": model, "batch": N, "variant": name, "steps": steps,
                              "rounds": rounds, "best_ms": round(min(res[name]), 4),
                              "median_ms": round(statistics.median(res[name]), 4),
                              "max_ms": round(max(res[name]), 4),
                              "plan": "persistent" if eng.persist else "per-layer",
                              "plan_ops": eng.plan.size()}), flush=True)
        del engs
        torch.cuda.empty_cache()
        if any(v != "default" for v in variants):
            hw = 32 if model.startswith("cifar") else 224
            print(json.dumps({"model": model, "batch": N, "s2d": s2d,
                              "erase_launch": erase_alone(N, hw, hw, s2d)}), flush=True)


if __name__ == "__main__":
    main()
