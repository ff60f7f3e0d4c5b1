"""What --optimizer rmsprop costs on one GPU (profiles/rmsprop.md).

1. The kernels alone: rmsprop_update_pack, plain and centered, beside adam_update_pack (the
   yardstick: an existing kernel with plain rmsprop's byte count) on the same synthetic buffers
   over a network's real segment table, in one process, timed with events around `reps`
   back-to-back launches, best and median of 5 batches, twice around (adam, rmsprop,
   rmsprop_centered, adam, rmsprop, rmsprop_centered), as us per launch and as bytes/s.  The
   two adam timings of one process are the run-to-run spread the ratio is read against.  Per
   element the Adam and the plain RMSProp kernel move 28 bytes (w, g and two state buffers
   read; w and the two written), the centered one 36 (mg read and written too); all add 2 bytes
   of bf16 HWIO copy where there is one.
2. The whole step: engines of the same network in one process, timed interleaved, rounds x
   variants, best / median / max ms/step:
       adamw             adam_update_pack + ohwi_pack
       rmsprop           rmsprop_update_pack + ohwi_pack
       rmsprop_centered  the same with --rmsprop_centered
   (mom and mom_generic, scripts/adam_step_time.py's, can be named too.)
Everything is printed as JSON lines.  The A/B of non-temporal against plain accesses to the
state buffers is this script run on a second build of the extension with -DDTR_RMSPROP_NT=0
for csrc/rmsprop.hip.

    python scripts/rmsprop_step_time.py [cifar_resnet50:128,...] [steps] [rounds] [variants]
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import distributed_tensorflow_resnet_amd as dtr  # noqa: E402
from distributed_tensorflow_resnet_amd.models.params import ParamStore  # noqa: E402
from distributed_tensorflow_resnet_amd.models.spec import build_spec  # noqa: E402
from distributed_tensorflow_resnet_amd.train.layout import param_segments  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_step_time as ast  # noqa: E402

# (epsilon 1.0, TF-slim's: the presets' SGD rates then stay SGD-sized steps on synthetic data)
ast.VARIANTS["rmsprop"] = ({"optimizer": "rmsprop", "rmsprop_epsilon": 1.0}, "")
ast.VARIANTS["rmsprop_centered"] = ({"optimizer": "rmsprop", "rmsprop_epsilon": 1.0,
                                     "rmsprop_centered": True}, "")


def kernels_alone(model, reps=20):
    """us per launch and TB/s of the update kernels over `model`'s segment table."""
    nat = dtr.native(required=True)
    dev = torch.device("cuda", 0)
    dataset, size = model.split("_resnet")
    spec = build_spec(dataset, int(size))
    slots = ParamStore(spec).train_slots
    seg, bf_total = param_segments(spec, slots, cpad_in=8, kpad=-(-spec.num_classes // 16) * 16,
                                   stem_s2d=False)
    n, nseg = int(seg[-1]["offset"] + seg[-1]["numel"]), len(seg)
    segs = torch.from_numpy(seg.view(np.uint8).copy()).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    w, g, m = (torch.randn(n, generator=gen, device=dev) for _ in range(3))
    v = torch.rand(n, generator=gen, device=dev)
    # rmsprop's own state, one set per variant (the plain launches must not run ms down under
    # the centered ones' mg): mom from zero, ms in [1, 2), mg ~ 0.1 randn, so ms >= 4 mg^2 at
    # the start.  batch() puts it back before every timed batch, and epsilon is the recipe-scale
    # 1.0 (TF-slim's), so the centered denominator ms' - mg'^2 + eps stays positive however
    # many launches follow one another with the same gradient: ms' - mg'^2 >= 0 up to rounding
    # once ms >= mg^2 holds (convexity), and eps = 1 is far above that rounding.
    ms0 = 1.0 + torch.rand(n, generator=gen, device=dev)
    mg0 = 0.1 * torch.randn(n, generator=gen, device=dev)
    w0 = w.clone()
    state = {c: (ms0.clone(), mg0.clone() if c else None, torch.zeros(n, device=dev))
             for c in (False, True)}

    def reset():
        w.copy_(w0)
        for ms, mg, mom in state.values():
            ms.copy_(ms0)
            mom.zero_()
            if mg is not None:
                mg.copy_(mg0)
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

    def rms(centered):
        ms, mg, mom = state[centered]
        nat.rmsprop_update_pack(w.data_ptr(), g.data_ptr(), ms.data_ptr(),
                                mg.data_ptr() if centered else 0, mom.data_ptr(), n, *sched,
                                gstep.data_ptr(), 0.9, 0.9, 1.0, 1.0, 0, int(centered), "l2",
                                segs.data_ptr(), nseg, wd.data_ptr(), wbf.data_ptr(), 0, st)

    def batch(fn):
        res = []
        for _ in range(3):
            fn()
        for _ in range(5):
            reset()
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
    out = {"model": model, "elements": n, "segments": nseg}
    plain, centered = (lambda: rms(False)), (lambda: rms(True))
    for name, fn, per in (("adam", adam, 28), ("rmsprop", plain, 28),
                          ("rmsprop_centered", centered, 36), ("adam_again", adam, 28),
                          ("rmsprop_again", plain, 28), ("rmsprop_centered_again", centered, 36)):
        best, med = batch(fn)
        nbytes = per * n + 2 * hwio
        out[name] = {"best_us": round(best, 2), "median_us": round(med, 2),
                     "bytes": nbytes, "best_TBps": round(nbytes / best / 1e6, 3),
                     "median_TBps": round(nbytes / med / 1e6, 3)}
    assert bool(torch.isfinite(w).all())
    for ms, mg, mom in state.values():
        assert bool(torch.isfinite(ms).all()) and bool(torch.isfinite(mom).all())
    return out


def main():
    cases = (sys.argv[1] if len(sys.argv) > 1 else
             "cifar_resnet50:128,imagenet_resnet50:128").split(",")
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    variants = (sys.argv[4] if len(sys.argv) > 4 else
                "adamw,rmsprop,rmsprop_centered").split(",")
    for model in dict.fromkeys(c.split(":")[0] for c in cases):
        print(json.dumps({"kernels_alone": kernels_alone(model)}), flush=True)
    for case in cases:
        if steps <= 0:
            break
        model, N = case.split(":")
        N = int(N)
        engs = {v: ast.build(model, N, v) for v in variants}
        res = {name: [] for name in engs}
        for _ in range(rounds):
            for name, eng in engs.items():
                res[name].append(ast.timed(eng, steps))
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
