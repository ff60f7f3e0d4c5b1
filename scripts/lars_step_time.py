"""Step time of --optimizer lars against mom on one GPU (profiles/lars.md): three engines
of the same network in one process -- mom as tuned (the one-launch optimizer where the
plan has it), mom with DTR_TUNE=opt_fused=0 (the launches lars replaces one of) and lars --
timed interleaved, rounds x variants, best and median ms/step as JSON lines.

    python scripts/lars_step_time.py [cifar_resnet50|imagenet_resnet50,...] [batch] [steps] [rounds]

With --trace it instead runs `steps` lars steps of the first model and nothing else: the
run to put under `rocprofv3 --kernel-trace --stats` for the three kernels' times.
"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import distributed_tensorflow_resnet_amd.train.engine as E  # noqa: E402
from distributed_tensorflow_resnet_amd.models.spec import build_spec  # noqa: E402

VARIANTS = [("mom", "mom", ""), ("mom opt_fused=0", "mom", "opt_fused=0"), ("lars", "lars", "")]


def build(model, N, optimizer, tune_extra):
    dataset, size = model.split("_resnet")
    cifar = dataset.startswith("cifar")
    base = os.environ.get("DTR_TUNE")
    os.environ["DTR_TUNE"] = ",".join(filter(None, [base or "", tune_extra]))
    try:
        eng = E.Engine(build_spec(dataset, int(size)), N, weight_decay=2e-4 if cifar else 1e-4,
                       lr_schedule=E.cifar_lr_schedule() if cifar else E.imagenet_lr_schedule(),
                       optimizer=optimizer, device=torch.device("cuda", 0),
                       input_mode="cifar_u8" if cifar else "imagenet_u8")
    finally:
        if base is None:
            del os.environ["DTR_TUNE"]
        else:
            os.environ["DTR_TUNE"] = base
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


def main():
    argv = [a for a in sys.argv[1:] if a != "--trace"]
    models = (argv[0] if argv else "cifar_resnet50,imagenet_resnet50").split(",")
    N = int(argv[1]) if len(argv) > 1 else 128
    steps = int(argv[2]) if len(argv) > 2 else 200
    rounds = int(argv[3]) if len(argv) > 3 else 5
    if "--trace" in sys.argv:
        eng = build(models[0], N, "lars", "")
        timed(eng, steps)
        return
    for model in models:
        engs = {name: build(model, N, opt, tune) for name, opt, tune in VARIANTS}
        res = {name: [] for name in engs}
        for _ in range(rounds):
            for name, eng in engs.items():
                res[name].append(timed(eng, steps))
        for name, eng in engs.items():
            assert not eng.persist_error(), name
            a, b = eng.seg["opt"]
            print(json.dumps({"model": model, "batch": N, "variant": name, "steps": steps,
                              "rounds": rounds, "best_ms": round(min(res[name]), 4),
                              "median_ms": round(statistics.median(res[name]), 4),
                              "plan": "persistent" if eng.persist else "per-layer",
                              "opt_fused": eng.opt_fused,
                              "opt_launches": [n for n in eng.plan.names()[a:b]
                                               if n not in ("record", "wait", "timing_point")],
                              "parameters": eng.params.n_train,
                              "lars_trust": eng.lars_summary()}), flush=True)
        del engs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
