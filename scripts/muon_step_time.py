"""What --optimizer muon costs on one GPU (profiles/muon.md).

1. The kernels alone, over a CIFAR network's real segment table on synthetic buffers, in one
   process: muon_orthogonalize (one workgroup per conv kernel; the launch lasts as long as its
   largest matrix), muon_update_pack and, for scale, sgd_update_pack; then muon_orthogonalize
   on ONE matrix of each shape of the network, which is the time of that shape's workgroup.
   Events around `reps` back-to-back launches, best and median of 5 batches, us per launch.
2. The whole step: engines of the same network in one process, timed interleaved, rounds x
   variants, best / median / max ms/step: mom (as tuned), mom_generic (DTR_TUNE=opt_fused=0:
   sgd_update_pack + ohwi_pack, the generic path muon takes) and muon.
3. An ImageNet network (imagenet_resnet18:128, imagenet_resnet50:128) takes --muon_tiled: part 1
   becomes each of csrc/muon_tiled.hip's five launches alone and the whole 3 + 3 * steps
   sequence over the network's tiled conv kernels; part 2's muon variant is muon_tiled.
Everything is printed as JSON lines.

    python scripts/muon_step_time.py [cifar_resnet50:128,cifar_resnet20:128] [steps] [rounds]
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
from distributed_tensorflow_resnet_amd.ops import functional as F  # noqa: E402
from distributed_tensorflow_resnet_amd.train.layout import muon_tables, param_segments  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_step_time as ast  # noqa: E402

ast.VARIANTS["muon"] = ({"optimizer": "muon"}, "")
ast.VARIANTS["muon_tiled"] = ({"optimizer": "muon", "muon_tiled": True}, "")


def _batch(fn, reps):
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
    return {"best_us": round(min(res), 2), "median_us": round(statistics.median(res), 2)}


def kernels_alone(model, reps=20):
    nat = dtr.native(required=True)
    dev = torch.device("cuda", 0)
    dataset, size = model.split("_resnet")
    spec = build_spec(dataset, int(size))
    slots = ParamStore(spec).train_slots
    seg, bf_total = param_segments(spec, slots, cpad_in=8, kpad=-(-spec.num_classes // 16) * 16,
                                   stem_s2d=False)
    tab, mseg, q = muon_tables(slots)
    n, nseg = int(seg[-1]["offset"] + seg[-1]["numel"]), len(seg)
    segs = torch.from_numpy(seg.view(np.uint8).copy()).to(dev)
    dtab = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    mseg_d, q_d = torch.from_numpy(mseg).to(dev), torch.from_numpy(q).to(dev)
    rows, cols = [int(r) for r in tab["R"]], [int(k) for k in tab["K"]]
    gen = torch.Generator(device=dev).manual_seed(1)
    w, g, m = (torch.randn(n, generator=gen, device=dev) for _ in range(3))
    d = torch.zeros(n, device=dev)
    wbf = torch.zeros(max(bf_total, 1), dtype=torch.bfloat16, device=dev)
    gstep = torch.full((1,), 100, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    sched = (1e-3, 0, 0.0, 0.0, [], [1e-3])

    def ortho():
        nat.muon_orthogonalize(g.data_ptr(), m.data_ptr(), d.data_ptr(), dtab.data_ptr(), rows,
                               cols, 0.5, 1, 5, 1.0, st)

    def update():
        nat.muon_update_pack(w.data_ptr(), g.data_ptr(), m.data_ptr(), d.data_ptr(), n, *sched,
                             gstep.data_ptr(), 0.9, 1e-4, 1.0, 1.0, segs.data_ptr(), nseg,
                             mseg_d.data_ptr(), q_d.data_ptr(), wbf.data_ptr(), 0, st)

    def sgd():
        nat.sgd_update_pack(w.data_ptr(), g.data_ptr(), m.data_ptr(), n, *sched,
                            gstep.data_ptr(), 0.9, 1e-4, 1.0, 1, segs.data_ptr(), nseg,
                            wbf.data_ptr(), 0, 1, st)

    out = {"model": model, "elements": n, "segments": nseg, "conv_kernels": len(tab)}
    for name, fn in (("muon_orthogonalize", ortho), ("muon_update_pack", update),
                     ("sgd_update_pack", sgd), ("muon_orthogonalize_again", ortho),
                     ("muon_update_pack_again", update), ("sgd_update_pack_again", sgd)):
        out[name] = _batch(fn, reps)
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(w).all())
    for R, K in sorted(set(zip(rows, cols))):   # one workgroup of each shape
        gg = torch.randn(R * K, generator=gen, device=dev)
        mm, oo = torch.zeros_like(gg), torch.zeros_like(gg)
        out[f"one_{R}x{K}"] = _batch(
            lambda: F.muon_orthogonalize(gg, mm, [(R, K)], momentum=0.5, out=oo), reps)
    return out


def tiled_alone(model, reps=10):
    """us per launch of the five tiled launches and of the whole sequence (5 steps)."""
    nat = dtr.native(required=True)
    dev = torch.device("cuda", 0)
    dataset, size = model.split("_resnet")
    slots = ParamStore(build_spec(dataset, int(size))).train_slots
    tt = muon_tables(slots, tiled=True)[3]
    buf = F.muon_tiled_buffers(tt, dev)
    n = int(slots[-1].offset + slots[-1].numel)
    gen = torch.Generator(device=dev).manual_seed(1)
    g, m = (torch.randn(n, generator=gen, device=dev) for _ in range(2))
    d = torch.zeros(n, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    class One:   # the sequence with every launch but `name` (and `epi`) left out
        def __init__(self, name, epi=None):
            self.name, self.epi = name, epi

        def __getattr__(self, op):
            def call(*a):
                if op == self.name and (self.epi is None or a[4] == self.epi):
                    getattr(nat, op)(*a)
            return call

    def seq(api, steps):
        return lambda: F.muon_tiled_sequence(api, buf, g.data_ptr(), m.data_ptr(), d.data_ptr(),
                                             0.5, True, steps, 1.0, tail=(st,))

    seq(nat, 5)()   # (the scratch holds a real iterate before any launch is timed alone)
    flop = sum(4.0 * int(r["SP"]) * int(r["SP"]) * int(r["LP"]) + 2.0 * int(r["SP"]) ** 3
               for r in tt["tab"])
    out = {"model": model, "tiled_kernels": len(tt["tab"]), "scratch_mb": tt["scratch"] * 2 / 2 ** 20,
           "workgroups": {k: len(tt[k]) for k in ("blk", "stage", "syrk_a", "apply")},
           "gflop_per_ns_step": round(flop / 1e9, 2)}
    for name, api in (("moments", One("muon_tiled_moments")), ("stage", One("muon_tiled_stage")),
                      ("syrk_a", One("muon_tiled_syrk", 0)), ("syrk_b", One("muon_tiled_syrk", 1)),
                      ("apply", One("muon_tiled_apply")), ("unstage", One("muon_tiled_unstage"))):
        out[name] = _batch(seq(api, 1), reps)
    out["sequence_5_steps"] = _batch(seq(nat, 5), reps)
    assert bool(torch.isfinite(d).all())
    return out


def main():
    cases = (sys.argv[1] if len(sys.argv) > 1 else
             "cifar_resnet50:128,cifar_resnet20:128").split(",")
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    for model in dict.fromkeys(c.split(":")[0] for c in cases):
        alone = tiled_alone if model.startswith("imagenet") else kernels_alone
        print(json.dumps({"kernels_alone": alone(model)}), flush=True)
    for case in cases:
        if steps <= 0:
            break
        model, N = case.split(":")
        variants = ("mom", "mom_generic", "muon_tiled" if model.startswith("imagenet") else "muon")
        engs = {v: ast.build(model, int(N), v) for v in variants}
        res = {name: [] for name in engs}
        for _ in range(rounds):
            for name, eng in engs.items():
                res[name].append(ast.timed(eng, steps))
        for name, eng in engs.items():
            assert not eng.persist_error(), name
            print(json.dumps({"model": model, "batch": int(N), "variant": name, "steps": steps,
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
