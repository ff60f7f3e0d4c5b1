"""Plan and state signatures of the engine over a grid of configurations: one line per
configuration with two sha256 values.  Two trees whose lines are identical record the same
plans op for op and compute the same bits (the step is bit-deterministic), so this is the
before / after check of a host-side refactor: run it from each tree against the same built
extension and diff the outputs.

  plan   plan.names(), op_streams(), op_kinds(), op_events(), eng.seg, eng.ready_index
  state  master, mom, stats, gstep, scalars[:4] after fill_synthetic(3) + 3 x step(need_cost=True)

Uses only the public Engine API.  A configuration the engine rejects at construction prints
its error message instead.  `python scripts/plan_signature.py [first [last]]` runs the
configurations first..last-1 (default: all).
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_tensorflow_resnet_amd import native  # noqa: E402
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec  # noqa: E402
from distributed_tensorflow_resnet_amd.train.engine import (Engine, cifar_lr_schedule,  # noqa: E402
                                                             imagenet_lr_schedule)
from distributed_tensorflow_resnet_amd.utils import tune  # noqa: E402

C8, C20 = ("cifar", 8), ("cifar", 20)
I18, I50 = ("imagenet", 18), ("imagenet", 50)
LOOP = dict(comm="loopback", bucket_mb=0.05)
# (label, spec, batch, DTR_TUNE, constructor options)
CONFIGS = [
    ("1a", C8, 16, "persist=0", {}),
    ("1b", C8, 16, "persist=1", {}),
    ("1c", C8, 16, "persist=1,opt_fused=0", {}),
    ("1d", C8, 16, "persist=0,bn_acc=0", {}),
    ("1e", C8, 16, "persist=0,fused_head=0", {}),
    ("1f", C8, 16, "persist=0", dict(use_graph=True)),
    ("2a", C20, 32, "persist=0,fork_every=1", {}),
    ("2b", C20, 32, "persist=1", {}),
    *[(f"3{k}-{dt}", C8, 16, t, dict(LOOP, allreduce_dtype=dt))
      for k, t in (("a", "persist=0"), ("b", "persist=1"), ("c", "persist=1,persist_overlap=0"))
      for dt in ("fp32", "bf16")],
    ("4a", C8, 16, "persist=0", dict(optimizer="lars")),
    ("4b", C8, 16, "persist=1", dict(optimizer="lars")),
    ("5a", I18, 8, "stem_s2d=1", {}),
    ("5b", I18, 8, "stem_s2d=0", {}),
    ("6a", I50, 8, "", {}),
    ("6b", I50, 8, "bap_maxc=0", {}),
    ("7a", C8, 16, "persist=0", dict(input_mode="cifar_resident")),
    ("7b", C8, 16, "persist=1", dict(input_mode="cifar_resident")),
]


def sha(*parts) -> str:
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else repr(p).encode())
    return h.hexdigest()[:16]


def build(spec_id, batch, tune_str, opts):
    os.environ["DTR_TUNE"] = tune_str   # (engine-side keys only: read at construction)
    assert set(tune.overrides()) <= set(tune.ENGINE), tune_str
    kind, size = spec_id
    spec = cifar_spec(size) if kind == "cifar" else imagenet_spec(size, image_hw=64)
    sched = cifar_lr_schedule() if kind == "cifar" else imagenet_lr_schedule()
    opts = dict(opts)
    if opts.get("comm") == "loopback":
        opts["comm"] = native().Comm.loopback(2.0)
    if opts.get("input_mode") == "cifar_resident":
        g = np.random.default_rng(5)
        opts["resident"] = (g.integers(0, 256, (256, 3, 32, 32), dtype=np.uint8),
                            g.integers(0, 10, 256))
    return Engine(spec, batch, weight_decay=2e-4, lr_schedule=sched, seed=7, data_seed=99,
                  device=torch.device("cuda", 0), **opts)


def signature(eng):
    p = eng.plan
    plan = sha(p.names(), p.op_streams(), p.op_kinds(), p.op_events(), sorted(eng.seg.items()),
               sorted(eng.ready_index.items()))
    if eng.input_mode != "cifar_resident":
        eng.fill_synthetic(3)
    if eng.use_graph:
        eng.capture()
    for _ in range(3):
        eng.step(need_cost=True)
    torch.cuda.synchronize()
    state = sha(*(t.cpu().numpy().tobytes() for t in (eng.params.master, eng.mom, eng.params.stats,
                                                     eng.gstep, eng.scalars[:4])))
    return plan, state


def eval_signature(eng, persist):
    ev = eng.build_eval_plan(16, persist=persist)
    g = torch.Generator().manual_seed(11)
    images = torch.randint(0, 256, (16, 3, 32, 32), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (16,), generator=g)
    _, _, probs = ev.run(images.cuda(), labels.cuda())
    torch.cuda.synchronize()
    return sha(ev.plan.names()), sha(probs.cpu().numpy().tobytes())


def main():
    lo = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    hi = int(sys.argv[2]) if len(sys.argv) > 2 else len(CONFIGS)
    for label, spec_id, batch, tune_str, opts in CONFIGS[lo:hi]:
        desc = f"{label} {spec_id[0]}{spec_id[1]} bs{batch} [{tune_str}] {sorted(opts.items())}"
        try:
            eng = build(spec_id, batch, tune_str, opts)
        except (ValueError, RuntimeError, AssertionError) as err:
            print(f"{desc}: rejected: {type(err).__name__}: {str(err)[:120]}", flush=True)
            continue
        plan, state = signature(eng)
        print(f"{desc}: persist={int(eng.persist)} overlap={int(eng.persist_overlap)} "
              f"ops={eng.plan.size()} plan={plan} state={state}", flush=True)
        if label == "1a":
            for persist in (False, True):
                names, probs = eval_signature(eng, persist)
                print(f"1a eval persist={int(persist)}: names={names} probs={probs}", flush=True)
        del eng


if __name__ == "__main__":
    main()
