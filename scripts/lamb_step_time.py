"""What --optimizer adamw --adam_trust on (LAMB) costs on one GPU (profiles/lamb.md).

1. The optimizer segment alone: the update launches of adamw (adam_update_pack), lars
   (lars_norms, lars_trust, lars_update_pack) and LAMB (lamb_moments_norms, lamb_trust,
   lamb_update_pack) on the same synthetic buffers over a network's real segment and chunk
   tables, timed with events around `reps` back-to-back segments, best and median of 5
   batches, as us per segment and as bytes/s.  ohwi_pack, which follows all three, is left
   out.  Bytes per element: adamw 28 (+2 per element with a bf16 copy), lars 28 = 8 + 20,
   LAMB 40 = 24 (w, g, m, v read; m, v written) + 16 (w, m, v read; w written).
2. The whole step: engines of the same network in one process, timed interleaved, rounds x
   variants, best / median / max ms/step, for adamw, lars and lamb.
Everything is printed as JSON lines; run it in several fresh processes for the
process-to-process spread.

    python scripts/lamb_step_time.py [cifar_resnet50:128,...] [steps] [rounds] [variants]
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import distributed_tensorflow_resnet_amd as dtr  # noqa: E402
import distributed_tensorflow_resnet_amd.train.engine as E  # noqa: E402
from distributed_tensorflow_resnet_amd.models.params import ParamStore  # noqa: E402
from distributed_tensorflow_resnet_amd.models.spec import build_spec  # noqa: E402
from distributed_tensorflow_resnet_amd.train.layout import lars_tables, param_segments  # noqa: E402

VARIANTS = {"adamw": {"optimizer": "adamw"}, "lars": {"optimizer": "lars"},
            "lamb": {"optimizer": "adamw", "adam_trust": "on"}}


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


def segments_alone(model, reps=20):
    """us per optimizer segment and TB/s of the three optimizers over `model`'s tables."""
    nat = dtr.native(required=True)
    dev = torch.device("cuda", 0)
    dataset, size = model.split("_resnet")
    spec = build_spec(dataset, int(size))
    slots = ParamStore(spec).train_slots
    seg, bf_total = param_segments(spec, slots, cpad_in=8, kpad=-(-spec.num_classes // 16) * 16,
                                   stem_s2d=False)
    n, nseg = int(seg[-1]["offset"] + seg[-1]["numel"]), len(seg)
    segs = torch.from_numpy(seg.view(np.uint8).copy()).to(dev)
    tab, blk = lars_tables(seg, [len(s.shape) == 1 for s in slots])
    lsegs = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    blk_d = torch.tensor(blk, dtype=torch.int32, device=dev)
    part = torch.zeros(2 * len(blk), dtype=torch.float64, device=dev)
    lout = torch.ones(3, nseg, device=dev)
    lo = lout.data_ptr()
    gen = torch.Generator(device=dev).manual_seed(1)
    w, g, m = (torch.randn(n, generator=gen, device=dev) for _ in range(3))
    v = torch.rand(n, generator=gen, device=dev)
    wbf = torch.zeros(max(bf_total, 1), dtype=torch.bfloat16, device=dev)
    wd = torch.full((nseg,), 1e-4, device=dev)
    gstep = torch.full((1,), 100, dtype=torch.int64, device=dev)
    start = torch.zeros(1, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    sched = (1e-3, 0, 0.0, 0.0, [], [1e-3])

    def adam():
        nat.adam_update_pack(w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, *sched,
                             gstep.data_ptr(), start.data_ptr(), 0.9, 0.999, 1e-8, 1.0, 0,
                             "decoupled", segs.data_ptr(), nseg, wd.data_ptr(), wbf.data_ptr(),
                             0, 0, st)

    def lars():
        nat.lars_norms(w.data_ptr(), g.data_ptr(), segs.data_ptr(), lsegs.data_ptr(),
                       blk_d.data_ptr(), len(blk), part.data_ptr(), st)
        nat.lars_trust(part.data_ptr(), lsegs.data_ptr(), nseg, 0.001, 1e-4, 0.0, 1.0, lo,
                       lo + 4 * nseg, lo + 8 * nseg, st)
        nat.lars_update_pack(w.data_ptr(), g.data_ptr(), m.data_ptr(), n, *sched,
                             gstep.data_ptr(), 0.9, 1e-4, 1.0, segs.data_ptr(), nseg, lo,
                             wbf.data_ptr(), 0, st)

    def lamb_norms():
        nat.lamb_moments_norms(w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                               gstep.data_ptr(), start.data_ptr(), 0.9, 0.999, 1e-8, 1.0, 0,
                               "decoupled", segs.data_ptr(), lsegs.data_ptr(), blk_d.data_ptr(),
                               len(blk), wd.data_ptr(), part.data_ptr(), st)

    def lamb_update():
        nat.lamb_update_pack(w.data_ptr(), m.data_ptr(), v.data_ptr(), n, *sched,
                             gstep.data_ptr(), start.data_ptr(), 0.9, 0.999, 1e-8, "decoupled",
                             segs.data_ptr(), nseg, wd.data_ptr(), lo, wbf.data_ptr(), 0, 0, st)

    def lamb():
        lamb_norms()
        nat.lamb_trust(part.data_ptr(), lsegs.data_ptr(), nseg, lo, lo + 4 * nseg, lo + 8 * nseg,
                       st)
        lamb_update()

    def batch(fn):
        res = []
        for _ in range(3):
            fn()
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            res.append(a.elapsed_time(b) * 1e3 / reps)
        return min(res), statistics.median(res)

    # the bf16 HWIO copy is written for the segments that have one
    hwio = sum(int(r["numel"]) for r in seg if r["bf_hwio"] >= 0)
    out = {"model": model, "elements": n, "segments": nseg, "chunks": len(blk)}
    for name, fn, per, copy in (("adamw", adam, 28, 1), ("lars", lars, 28, 1), ("lamb", lamb, 40, 1),
                                ("lamb_moments_norms", lamb_norms, 24, 0),
                                ("lamb_update_pack", lamb_update, 16, 1), ("adamw_again", adam, 28, 1)):
        best, med = batch(fn)
        nbytes = per * n + 2 * hwio * copy
        out[name] = {"best_us": round(best, 2), "median_us": round(med, 2),
                     "bytes": nbytes, "best_TBps": round(nbytes / best / 1e6, 3),
                     "median_TBps": round(nbytes / med / 1e6, 3)}
    assert bool(torch.isfinite(w).all())
    return out


def main():
    cases = (sys.argv[1] if len(sys.argv) > 1 else
             "cifar_resnet50:128,imagenet_resnet50:128").split(",")
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    variants = (sys.argv[4] if len(sys.argv) > 4 else "adamw,lars,lamb").split(",")
    for model in dict.fromkeys(c.split(":")[0] for c in cases):
        print(json.dumps({"segments_alone": segments_alone(model)}), flush=True)
    for case in cases:
        if steps <= 0:
            break
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
                              "opt_fused": bool(eng.opt_fused),
                              "plan_ops": eng.plan.size()}), flush=True)
        del engs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
