"""What the CIFAR input costs a training step, host-fed against device-resident
(profiles/cifar_resident_input.md).  One process, the variants interleaved round by
round on the same GPU; best and median per variant, and the spread of the repeated
baseline runs next to every difference.

    python scripts/input_step_time.py plan [batch,...] [steps] [rounds]
        plan-only step time: cifar_u8 (one static batch in img_u8, no feeding) against
        cifar_resident (50,000 resident records, shuffled on the device)
    python scripts/input_step_time.py fed [batch,...] [steps] [rounds]
        fed step rate: a TrainingSession with the CLI's default hooks on a written
        50,000-record split, CifarData + Prefetcher against the resident split
    python scripts/input_step_time.py eval [rounds]
        evaluate_checkpoint of 50 x 100 images, host-fed against the attached split
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/input_step_time.py kernel [batch] [launches]
        the two input launches alone, for their kernel times

Every line of the result is JSON on stdout.
"""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_tensorflow_resnet_amd import native  # noqa: E402
from distributed_tensorflow_resnet_amd.data import cifar  # noqa: E402
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec  # noqa: E402
from distributed_tensorflow_resnet_amd.train import hooks as H  # noqa: E402
from distributed_tensorflow_resnet_amd.train.backends import GPUBackend  # noqa: E402
from distributed_tensorflow_resnet_amd.train.driver import Prefetcher  # noqa: E402
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule  # noqa: E402
from distributed_tensorflow_resnet_amd.train.evaluator import (GPUInference,  # noqa: E402
                                                               evaluate_checkpoint)
from distributed_tensorflow_resnet_amd.train.session import TrainingSession  # noqa: E402
from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver  # noqa: E402

RECORDS, SIZE = 50000, 50
DEV = torch.device("cuda", 0)


def split(records=RECORDS, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (records, 3, 32, 32), dtype=np.uint8),
            rng.integers(0, 10, records).astype(np.int64))


def engine(batch, resident=None):
    kw = dict(weight_decay=2e-4, lr_schedule=cifar_lr_schedule(), device=DEV, use_graph=False)
    if resident is None:
        eng = Engine(cifar_spec(SIZE), batch, input_mode="cifar_u8", **kw)
        eng.fill_synthetic(0)
    else:
        eng = Engine(cifar_spec(SIZE), batch, input_mode="cifar_resident", resident=resident,
                     shuffle_seed=0, **kw)
    return eng


def timed(eng, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        eng.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def summary(v):
    return {"best": round(min(v), 4), "median": round(statistics.median(v), 4),
            "spread": round(max(v) - min(v), 4), "runs": [round(x, 4) for x in v]}


def plan_mode(batches, steps, rounds):
    data = split()
    for N in batches:
        # two engines per variant: the difference between two instances of the same plan
        # (their buffers sit at other addresses) is the floor under any A/B difference
        engs = {"cifar_u8": engine(N), "cifar_resident": engine(N, data),
                "cifar_u8#2": engine(N), "cifar_resident#2": engine(N, data)}
        for e in engs.values():
            timed(e, 50)
        res = {k: [] for k in engs}
        for _ in range(rounds):
            for name, e in engs.items():
                res[name].append(timed(e, steps))
        for name, e in engs.items():
            assert not e.persist_error(), name
        out = {"mode": "plan", "batch": N, "steps": steps, "unit": "ms/step",
               "step": "persistent" if engs["cifar_u8"].persist else "per-layer"}
        out.update({k: summary(v) for k, v in res.items()})
        print(json.dumps(out), flush=True)
        del engs
        torch.cuda.empty_cache()


def kernel_mode(N, launches):
    """The two input launches alone, alternating, for a kernel trace (run under
    `rocprofv3 --kernel-trace --stats`): cifar_augment on one static batch against
    cifar_augment_resident on the 50,000-record split, a fresh step every launch, both
    clearing the same 128 KB buffer as the step's input launch does."""
    from distributed_tensorflow_resnet_amd.ops import functional as F

    imgs, labels = split()
    rec = torch.from_numpy(imgs).to(DEV)
    lab = torch.from_numpy(labels).to(device=DEV, dtype=torch.int32)
    batch = rec[:N].contiguous()
    zero = torch.zeros(32768, device=DEV)
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    nat = native(required=True)
    out = torch.empty((N, 32, 32, 8), device=DEV, dtype=torch.bfloat16)
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(launches):
        pos.add_(1)
        nat.cifar_augment(batch.data_ptr(), out.data_ptr(), N, 32, 32, 8, 4, 1234,
                          pos.data_ptr(), 1, 0, zero.data_ptr(), zero.numel() * 4, st)
        F.cifar_augment_resident(rec, lab, pos, N, seed=1234, key_seed=0, zero=zero)
    torch.cuda.synchronize()
    print(json.dumps({"mode": "kernel", "batch": N, "launches": launches}), flush=True)


class _Clock(H.Hook):
    """Wall time between two steps, a device synchronise at each end."""

    def __init__(self, first, last):
        self.first, self.last, self.t0, self.t1 = first, last, None, None

    def after_run(self, session, step):
        if step == self.first or step == self.last:
            session.synchronize()
            if step == self.first:
                self.t0 = time.perf_counter()
            else:
                self.t1 = time.perf_counter()


def session_rate(eng, feeder, steps, warm):
    """steps/s of a TrainingSession with the CLI's default hooks (train/driver.py)."""
    first = int(eng.gstep.item()) + warm
    clock = _Clock(first, first + steps)
    sched = cifar_lr_schedule()
    hooks = [H.LearningRateSetterHook(sched), H.LoggingTensorHook(20, "precision"),
             H.StepCounterHook(100, eng.N, None), H.StopAtStepHook(first + steps), clock]
    sess = TrainingSession(GPUBackend(eng), hooks, [], checkpoint_dir=None, feeder=feeder)
    with sess:
        while not sess.should_stop():
            sess.run()
    return steps / (clock.t1 - clock.t0)


def fed_mode(batches, steps, rounds):
    imgs, labels = split()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "train.bin")
        cifar.write_records(path, imgs, labels)
        data = cifar.CifarData(path, "cifar10", train=True)
        for N in batches:
            fed, res = engine(N), engine(N, (data.images, data.labels))
            rates = {"host_fed": [], "resident": []}
            for _ in range(rounds):
                feeder = Prefetcher(data.batches(N, seed=0))
                rates["host_fed"].append(session_rate(fed, feeder, steps, 100))
                rates["resident"].append(session_rate(res, None, steps, 100))
            plan = {"cifar_u8": 1e3 / timed(fed, 500), "cifar_resident": 1e3 / timed(res, 500)}
            out = {"mode": "fed", "batch": N, "steps": steps, "unit": "steps/s",
                   "plan_only": {k: round(v, 1) for k, v in plan.items()}}
            for k, v in rates.items():
                out[k] = {"best": round(max(v), 1), "median": round(statistics.median(v), 1),
                          "runs": [round(x, 1) for x in v]}
            print(json.dumps(out), flush=True)
            del fed, res
            torch.cuda.empty_cache()


def eval_mode(rounds):
    bs, count = 100, 50
    imgs, labels = split(bs * count, seed=1)
    ti, tl = torch.from_numpy(imgs), torch.from_numpy(labels)
    with tempfile.TemporaryDirectory() as tmp:
        eng = Engine(cifar_spec(SIZE), 16, weight_decay=2e-4, lr_schedule=cifar_lr_schedule(),
                     device=DEV, use_graph=False)
        prefix = Saver(tmp).save(GPUBackend(eng).state_tensors(), 0)
        host = GPUInference(cifar_spec(SIZE), bs, device=DEV)
        res = GPUInference(cifar_spec(SIZE), bs, device=DEV)
        res.attach(imgs, labels)

        def batches():
            for s in range(0, bs * count, bs):
                yield ti[s:s + bs], tl[s:s + bs]

        def once(model):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = evaluate_checkpoint(model, prefix, batches, count)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3, r

        ms = {"host_fed": [], "resident": []}
        scores = {}
        for name, m in (("host_fed", host), ("resident", res)):
            once(m)
        for _ in range(rounds):
            for name, m in (("host_fed", host), ("resident", res)):
                t, scores[name] = once(m)
                ms[name].append(t)
        out = {"mode": "eval", "images": bs * count, "batch": bs, "path": host.eval_path,
               "unit": "ms per evaluate_checkpoint (checkpoint read included)",
               "same_score": scores["host_fed"][0] == scores["resident"][0]}
        out.update({k: summary(v) for k, v in ms.items()})
        print(json.dumps(out), flush=True)


def main():
    if not torch.cuda.is_available():
        sys.exit("input_step_time.py needs a GPU")
    mode = sys.argv[1] if len(sys.argv) > 1 else "plan"
    if mode == "eval":
        return eval_mode(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    if mode == "kernel":
        return kernel_mode(int(sys.argv[2]) if len(sys.argv) > 2 else 128,
                           int(sys.argv[3]) if len(sys.argv) > 3 else 500)
    batches = [int(b) for b in (sys.argv[2] if len(sys.argv) > 2 else "128,16").split(",")]
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else (2000 if mode == "fed" else 1000)
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else (3 if mode == "fed" else 5)
    (fed_mode if mode == "fed" else plan_mode)(batches, steps, rounds)


if __name__ == "__main__":
    main()
