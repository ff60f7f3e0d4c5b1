"""Step time with --clip_grad_norm off and on, on one GPU (profiles/clip_grad_norm.md):
engines of the same network in one process, timed interleaved, rounds x variants, best and
median ms/step as JSON lines:
    default   clipping off, the optimizer as tuned (the one-launch sgd_tiles where it applies)
    unfused   clipping off, DTR_TUNE=opt_fused=0 (the generic optimizer launches)
    clip      clip_grad_norm=1.0 (grad_sqnorm + clip_scale in front of the generic update)
then grad_sqnorm + clip_scale alone over the network's parameter count, timed with events
around back-to-back launches over different buffers, and grad_sqnorm's bytes/s against the
4 n bytes it has to read.  `default,unfused` also run on a tree without the flag.

    python scripts/clip_step_time.py [cifar_resnet50:128,...] [steps] [rounds] [variants]
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

VARIANTS = {"default": ("", 0.0), "unfused": ("opt_fused=0", 0.0), "clip": ("", 1.0)}


def build(model, N, variant):
    tune, clip = VARIANTS[variant]
    dataset, size = model.split("_resnet")
    cifar = dataset.startswith("cifar")
    kw = {"clip_grad_norm": clip} if clip else {}
    old = os.environ.get("DTR_TUNE")
    os.environ["DTR_TUNE"] = ",".join(filter(None, [old, tune]))
    try:
        eng = E.Engine(build_spec(dataset, int(size)), N, weight_decay=2e-4 if cifar else 1e-4,
                       lr_schedule=E.cifar_lr_schedule() if cifar else E.imagenet_lr_schedule(),
                       device=torch.device("cuda", 0),
                       input_mode="cifar_u8" if cifar else "imagenet_u8", **kw)
    finally:
        if old is None:
            del os.environ["DTR_TUNE"]
        else:
            os.environ["DTR_TUNE"] = old
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


def kernels_alone(n, reps=50):
    """us per launch of grad_sqnorm and of clip_scale over n elements, buffers as cold as a
    step leaves them: `reps` launches over `reps` different gradients (none touched twice)."""
    nat = dtr.native(required=True)
    dev = torch.device("cuda", 0)
    nbuf = min(reps, max(2, (6 << 30) // (4 * n)))
    nch = nat.clip_chunks(n)
    bufs = [torch.randn(n, device=dev) for _ in range(nbuf)]
    parts = [torch.zeros(nch, dtype=torch.float64, device=dev) for _ in range(nbuf)]
    out = torch.zeros(2, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def batch(fn):
        best = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for g, p in zip(bufs, parts):
                fn(g, p)
            b.record()
            torch.cuda.synchronize()
            best.append(a.elapsed_time(b) * 1e3 / nbuf)
        return min(best), statistics.median(best)

    sq = batch(lambda g, p: nat.grad_sqnorm(g.data_ptr(), n, p.data_ptr(), st))
    sc = batch(lambda g, p: nat.clip_scale(p.data_ptr(), nch, 1.0, out.data_ptr(), st))
    return sq, sc, nbuf, nch


def main():
    cases = (sys.argv[1] if len(sys.argv) > 1 else
             "cifar_resnet50:128,cifar_resnet50:16,imagenet_resnet50:128").split(",")
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    variants = (sys.argv[4] if len(sys.argv) > 4 else "default,unfused,clip").split(",")
    for case in cases:
        model, N = case.split(":")
        N = int(N)
        engs = {v: build(model, N, v) for v in variants}
        res = {name: [] for name in engs}
        for _ in range(rounds):
            for name, eng in engs.items():
                res[name].append(timed(eng, steps))
        n = next(iter(engs.values())).params.n_train
        for name, eng in engs.items():
            assert not eng.persist_error(), name
            print(json.dumps({"model": model, "batch": N, "variant": name, "steps": steps,
                              "rounds": rounds, "best_ms": round(min(res[name]), 4),
                              "median_ms": round(statistics.median(res[name]), 4),
                              "max_ms": round(max(res[name]), 4),
                              "plan": "persistent" if eng.persist else "per-layer",
                              "opt_fused": bool(eng.opt_fused),
                              "plan_ops": eng.plan.size(), "parameters": n}), flush=True)
        del engs
        torch.cuda.empty_cache()
        if "clip" in variants:
            sq, sc, nbuf, nch = kernels_alone(n)
            print(json.dumps({"model": model, "n": n, "buffers": nbuf, "chunks": nch,
                              "grad_sqnorm_best_us": round(sq[0], 3),
                              "grad_sqnorm_median_us": round(sq[1], 3),
                              "clip_scale_best_us": round(sc[0], 3),
                              "clip_scale_median_us": round(sc[1], 3), "floor_bytes": 4 * n,
                              "grad_sqnorm_best_TBps": round(4 * n / sq[0] / 1e6, 3)}),
                  flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
