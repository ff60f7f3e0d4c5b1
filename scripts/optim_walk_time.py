#!/usr/bin/env python3
"""us per launch of every optimizer kernel that uses optim_device.h's shared walks, alone, over
a network's real segment and chunk tables (profiles/optim_walk.md): sgd_update_pack,
sgd_clip_update_pack, lars_update_pack, adam_update_pack, lamb_update_pack (the flat walk),
lars_norms, lamb_moments_norms, grad_sqnorm (the chunk reduction).  The method is
lamb_step_time.py's segments_alone: synthetic buffers, events around `reps` back-to-back
launches, best and median of 5 batches.  One JSON line per model; run it in several fresh
processes for the process-to-process spread.  --ext loads another build of the extension
(an A/B against an older tree's _C).

    python scripts/optim_walk_time.py [--ext FILE] [cifar_resnet50,imagenet_resnet50] [reps]
"""
import importlib.util
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import distributed_tensorflow_resnet_amd as dtr  # noqa: E402

if len(sys.argv) > 2 and sys.argv[1] == "--ext":
    _name = "distributed_tensorflow_resnet_amd._C"
    _spec = importlib.util.spec_from_file_location(_name, sys.argv[2])
    sys.modules[_name] = dtr._C = importlib.util.module_from_spec(_spec)
    _spec.loader.exec_module(dtr._C)
    del sys.argv[1:3]

from distributed_tensorflow_resnet_amd.models.params import ParamStore  # noqa: E402
from distributed_tensorflow_resnet_amd.models.spec import build_spec  # noqa: E402
from distributed_tensorflow_resnet_amd.train.layout import lars_tables, param_segments  # noqa: E402


def kernels_alone(model, reps):
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
    cpart = torch.zeros(nat.clip_chunks(n), dtype=torch.float64, device=dev)
    trust = torch.ones(nseg, device=dev)
    clip = torch.tensor([1.0, 0.5], device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    w, g, m = (torch.randn(n, generator=gen, device=dev) for _ in range(3))
    v = torch.rand(n, generator=gen, device=dev)
    wbf = torch.zeros(max(bf_total, 1), dtype=torch.bfloat16, device=dev)
    wd = torch.full((nseg,), 1e-4, device=dev)
    gstep = torch.full((1,), 100, dtype=torch.int64, device=dev)
    start = torch.zeros(1, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    sched = (1e-3, 0, 0.0, 0.0, [], [1e-3])
    W, G, M, V = w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
    S, L, B, BF = segs.data_ptr(), lsegs.data_ptr(), blk_d.data_ptr(), wbf.data_ptr()
    GS, ST = gstep.data_ptr(), start.data_ptr()
    adam = (0.9, 0.999, 1e-8)
    launches = {
        "sgd_update_pack": lambda: nat.sgd_update_pack(W, G, M, n, *sched, GS, 0.9, 1e-4, 1.0, 1, S,
                                                       nseg, BF, 0, 1, st),
        "sgd_clip_update_pack": lambda: nat.sgd_clip_update_pack(W, G, M, n, *sched, GS, 0.9, 1e-4,
                                                                 clip.data_ptr(), 1, S, nseg, BF, 0,
                                                                 st),
        "lars_update_pack": lambda: nat.lars_update_pack(W, G, M, n, *sched, GS, 0.9, 1e-4, 1.0, S,
                                                         nseg, trust.data_ptr(), BF, 0, st),
        "adam_update_pack": lambda: nat.adam_update_pack(W, G, M, V, n, *sched, GS, ST, *adam, 1.0, 0,
                                                         "decoupled", S, nseg, wd.data_ptr(), BF, 0,
                                                         0, st),
        "lamb_update_pack": lambda: nat.lamb_update_pack(W, M, V, n, *sched, GS, ST, *adam,
                                                         "decoupled", S, nseg, wd.data_ptr(),
                                                         trust.data_ptr(), BF, 0, 0, st),
        "lars_norms": lambda: nat.lars_norms(W, G, S, L, B, len(blk), part.data_ptr(), st),
        "lamb_moments_norms": lambda: nat.lamb_moments_norms(W, G, M, V, GS, ST, *adam, 1.0, 0,
                                                             "decoupled", S, L, B, len(blk),
                                                             wd.data_ptr(), part.data_ptr(), st),
        "grad_sqnorm": lambda: nat.grad_sqnorm(G, n, cpart.data_ptr(), st),
    }
    out = {"model": model, "elements": n, "segments": nseg, "chunks": len(blk), "reps": reps}
    for name, fn in launches.items():
        for _ in range(3):
            fn()
        res = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            res.append(a.elapsed_time(b) * 1e3 / reps)
        out[name] = {"best_us": round(min(res), 2), "median_us": round(statistics.median(res), 2)}
    assert bool(torch.isfinite(w).all())
    return out


def main():
    models = (sys.argv[1] if len(sys.argv) > 1 else "cifar_resnet50,imagenet_resnet50").split(",")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    for model in models:
        print(json.dumps(kernels_alone(model, reps)), flush=True)


if __name__ == "__main__":
    main()
