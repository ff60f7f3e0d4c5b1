"""Eval-batch time of the two inference plans (Engine.build_eval_plan: the launch-per-layer
plan and the one-launch persistent forward), same process, same engine, back to back.

Per (network, batch): after warm-up, `runs` timed runs of each plan, alternating, each
between two HIP events with a host synchronisation after it (the evaluator reads the
loss / correct scalars after every batch); the input upload is outside the events.
Median, best and the 10th-90th percentile band are printed.  Then one full
evaluate_checkpoint (restore + 50 batches of 100 raw uint8 images, end to end on the
host clock) through GPUInference on each path.

    python scripts/eval_step_time.py [runs] [out.json]
"""
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import distributed_tensorflow_resnet_amd.train.engine as E  # noqa: E402
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec  # noqa: E402
from distributed_tensorflow_resnet_amd.train import evaluator  # noqa: E402
from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver, state_to_tf  # noqa: E402

CASES = [(50, 1), (50, 16), (50, 100), (50, 128), (50, 512), (20, 100)]
WARMUP = 20


def timed(ev, st):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ev.plan.run(0, ev.plan.size(), st, 0)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3   # us


def stats(v):
    v = sorted(v)
    return {"median_us": statistics.median(v), "best_us": v[0],
            "p10_us": v[len(v) // 10], "p90_us": v[(9 * len(v)) // 10]}


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(dev)
    res = {"device": props.name, "cus": props.multi_processor_count, "runs": runs, "cases": [],
           "host": os.uname().nodename}
    print(f"{props.name}, {props.multi_processor_count} CUs, host {res['host']}", flush=True)
    engines = {}
    for depth, batch in CASES:
        if depth not in engines:
            engines[depth] = E.Engine(cifar_spec(depth), 16, weight_decay=2e-4,
                                      lr_schedule=E.cifar_lr_schedule(), device=dev, use_graph=False)
        eng = engines[depth]
        st = torch.cuda.current_stream().cuda_stream
        g = torch.Generator().manual_seed(batch)
        imgs = torch.randint(0, 256, (batch, 3, 32, 32), generator=g, dtype=torch.uint8).to(dev)
        labels = torch.randint(0, 10, (batch,), generator=g).to(dev)
        plans = {k: eng.build_eval_plan(batch, persist=(k == "persistent"))
                 for k in ("per-layer", "persistent")}
        probs = {}
        for k, ev in plans.items():   # upload + input plan once, outside the timing
            _, _, p = ev.run(imgs, labels, raw_u8=True)
            probs[k] = p.float().clone()
            for _ in range(WARMUP):
                timed(ev, st)
        t = {k: [] for k in plans}
        for _ in range(runs):
            for k, ev in plans.items():
                t[k].append(timed(ev, st))
        diff = ((probs["persistent"] - probs["per-layer"]).norm() / probs["per-layer"].norm()).item()
        row = {"resnet": depth, "batch": batch, "launches": {k: ev.plan.size() for k, ev in plans.items()},
               "probs_rel_diff": diff, **{k: stats(v) for k, v in t.items()}}
        res["cases"].append(row)
        print(f"resnet{depth} bs{batch}: per-layer {row['per-layer']['median_us']:.1f} us "
              f"(best {row['per-layer']['best_us']:.1f}, {plans['per-layer'].plan.size()} launches), "
              f"persistent {row['persistent']['median_us']:.1f} us (best "
              f"{row['persistent']['best_us']:.1f}), probs rel diff {diff:.2e}", flush=True)
        eng.eval_plans.clear()
        del plans
        torch.cuda.empty_cache()

    # one full evaluate_checkpoint: 50 batches of 100, restore included, host clock
    spec = cifar_spec(50)
    with tempfile.TemporaryDirectory() as td:
        eng = engines[50]
        prefix = Saver(td).save(state_to_tf(eng.params, eng.mom, 0), 0)
        g = torch.Generator().manual_seed(0)
        data = [(torch.randint(0, 256, (100, 3, 32, 32), generator=g, dtype=torch.uint8),
                 torch.randint(0, 10, (100,), generator=g)) for _ in range(50)]
        res["evaluate_checkpoint"] = {}
        old = os.environ.get("DTR_TUNE")
        for k, setting in (("per-layer", "persist_eval=0"), ("persistent", "persist_eval=1")):
            os.environ["DTR_TUNE"] = setting
            model = evaluator.GPUInference(spec, 100, device=dev)
            assert model.eval_path == k, (model.eval_path, k)
            times = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                prec, loss, _ = evaluator.evaluate_checkpoint(model, prefix, lambda: iter(data), 50)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            res["evaluate_checkpoint"][k] = {"ms": times, "precision": prec, "loss": loss}
            print(f"evaluate_checkpoint 50 x 100 [{k}]: {', '.join(f'{x:.1f}' for x in times)} ms "
                  f"(precision {prec:.3f}, loss {loss:.3f})", flush=True)
        if old is None:
            del os.environ["DTR_TUNE"]
        else:
            os.environ["DTR_TUNE"] = old
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
