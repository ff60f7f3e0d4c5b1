"""Step time with --ema_decay off and on, on one GPU (profiles/ema.md): two engines of the
same network in one process, timed interleaved, rounds x variants, best and median ms/step
as JSON lines; then the ema_update kernel alone over the network's parameter count, timed
with events around `reps` back-to-back launches, and its bytes/s against the 12 n bytes
every update has to move (8 read, 4 written per element).

    python scripts/ema_step_time.py [cifar_resnet50:128,cifar_resnet50:16,imagenet_resnet50:128] [steps] [rounds]
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


def build(model, N, ema_decay):
    dataset, size = model.split("_resnet")
    cifar = dataset.startswith("cifar")
    eng = E.Engine(build_spec(dataset, int(size)), N, weight_decay=2e-4 if cifar else 1e-4,
                   lr_schedule=E.cifar_lr_schedule() if cifar else E.imagenet_lr_schedule(),
                   device=torch.device("cuda", 0), ema_decay=ema_decay,
                   input_mode="cifar_u8" if cifar else "imagenet_u8")
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


def kernel_alone(n, reps=50):
    """us per ema_update launch over n elements, buffers as cold as a step leaves them:
    `reps` launches over `reps` different buffer pairs (no pair is touched twice)."""
    nat = dtr.native(required=True)
    dev = torch.device("cuda", 0)
    pairs = min(reps, max(2, (6 << 30) // (8 * n)))
    bufs = [(torch.randn(n, device=dev), torch.randn(n, device=dev)) for _ in range(pairs)]
    gstep = torch.full((1,), 1000, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    best = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for m, s in bufs:
            nat.ema_update(m.data_ptr(), s.data_ptr(), n, gstep.data_ptr(), 1e-4, 1, st)
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b) * 1e3 / pairs)
    return min(best), statistics.median(best), pairs


def main():
    cases = (sys.argv[1] if len(sys.argv) > 1 else
             "cifar_resnet50:128,cifar_resnet50:16,imagenet_resnet50:128").split(",")
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    for case in cases:
        model, N = case.split(":")
        N = int(N)
        engs = {"off": build(model, N, 0.0), "on": build(model, N, 0.9999)}
        res = {name: [] for name in engs}
        for _ in range(rounds):
            for name, eng in engs.items():
                res[name].append(timed(eng, steps))
        n = engs["on"].params.n_train
        for name, eng in engs.items():
            assert not eng.persist_error(), name
            print(json.dumps({"model": model, "batch": N, "ema": name, "steps": steps,
                              "rounds": rounds, "best_ms": round(min(res[name]), 4),
                              "median_ms": round(statistics.median(res[name]), 4),
                              "plan": "persistent" if eng.persist else "per-layer",
                              "plan_ops": eng.plan.size(), "parameters": n}), flush=True)
        del engs
        torch.cuda.empty_cache()
        best, med, pairs = kernel_alone(n)
        print(json.dumps({"model": model, "kernel": "ema_update", "n": n, "buffer_pairs": pairs,
                          "best_us": round(best, 3), "median_us": round(med, 3),
                          "floor_bytes": 12 * n,
                          "best_TBps": round(12 * n / best / 1e6, 3)}), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
