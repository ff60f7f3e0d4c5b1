"""What --optimizer shampoo costs on one GPU (profiles/shampoo.md).

1. Each of csrc/shampoo.hip's five launches alone, over a network's real block table on an
   engine's own buffers (after two real steps, so the statistics are real): us per launch, events
   around `reps` back-to-back launches, best and median of 5 batches.  shampoo_roots is timed
   twice: with every = 1 (each launch refreshes) and with an interval no step count meets (the
   workgroups leave at once, which is what nine steps of ten pay).
2. The whole step: engines of the same network in one process, timed interleaved, rounds x
   variants, best / median / max ms/step: mom (as tuned), mom_generic (DTR_TUNE=opt_fused=0, the
   generic path shampoo takes), shampoo (every 10) and shampoo_every1 (a refresh in every step).
With --variant soap (profiles/soap.md) the launches are csrc/soap.hip's (shampoo_stats,
soap_refresh with every = 1 and idle, soap_rotate_adam, soap_update_pack) and the step variants
are adamw, shampoo (roots, every 10), soap (every 10) and soap_every1.
Everything is printed as JSON lines.

    python scripts/shampoo_step_time.py [cifar_resnet50:128,imagenet_resnet50:128] [steps] [rounds]
                                        [--variant roots|soap]
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_step_time as ast  # noqa: E402
from muon_step_time import _batch  # noqa: E402

ast.VARIANTS["shampoo"] = ({"optimizer": "shampoo"}, "")
ast.VARIANTS["shampoo_every1"] = ({"optimizer": "shampoo", "shampoo_precond_every": 1}, "")
SOAP = {"optimizer": "shampoo", "shampoo_variant": "soap", "shampoo_beta2": 0.95}
ast.VARIANTS["soap"] = (SOAP, "")
ast.VARIANTS["soap_every1"] = ({**SOAP, "shampoo_precond_every": 1}, "")
STEP_VARIANTS = {"roots": ("mom", "mom_generic", "shampoo", "shampoo_every1"),
                 "soap": ("adamw", "shampoo", "soap", "soap_every1")}


def kernels_alone(model, N, reps=20):
    eng = ast.build(model, N, "shampoo")
    for _ in range(2):
        eng.step()
    nat, st = eng.nat, torch.cuda.current_stream().cuda_stream
    sb, tab, nb = eng.shampoo_state_buf, eng.shampoo_tab.data_ptr(), len(eng.shampoo_blocks)
    L, Rt, PL, PR = (sb[i].data_ptr() for i in range(4))
    grad, gs, s0 = eng.grad.data_ptr(), eng.gstep.data_ptr(), eng.shampoo_start.data_ptr()
    fail, part = eng.shampoo_fail.data_ptr(), eng.shampoo_part.data_ptr()
    d, out = eng.shampoo_dir.data_ptr(), eng.shampoo_out.data_ptr()
    w, m = eng.params.master.clone(), eng.mom.clone()   # the update moves copies
    launches = {
        "shampoo_stats": lambda: nat.shampoo_stats(grad, tab, nb, L, Rt, 1.0, 1.0, gs, s0, 1 << 30,
                                                   fail, st),
        "shampoo_roots_refresh": lambda: nat.shampoo_roots(tab, nb, 2, L, Rt, PL, PR, gs, s0, 1,
                                                           eng.shampoo_epsilon, fail, st),
        "shampoo_roots_idle": lambda: nat.shampoo_roots(tab, nb, 2, L, Rt, PL, PR, gs, s0, 1 << 30,
                                                        eng.shampoo_epsilon, fail, st),
        "shampoo_precondition": lambda: nat.shampoo_precondition(grad, tab, nb, PL, PR, d, part,
                                                                 1.0, st),
        "shampoo_graft": lambda: nat.shampoo_graft(part, eng.shampoo_ttab.data_ptr(),
                                                   len(eng.shampoo_tensors), eng.nseg, out, st),
        "shampoo_update_pack": lambda: nat.shampoo_update_pack(
            w.data_ptr(), grad, m.data_ptr(), d, eng.params.n_train, *eng.sched.launch_args(), gs,
            eng.momentum, eng.wd, 1.0, eng.segs.data_ptr(), eng.nseg, eng.shampoo_seg.data_ptr(),
            out, eng.wbf.data_ptr(), 0, *eng.sched.extra_launch_args(), st),
    }
    res = {"model": model, "blocks": nb, "conv_kernels": len(eng.shampoo_tensors),
           "state_mb": round(sb.numel() * 4 / 2 ** 20, 1)}
    for name, fn in launches.items():
        res[name] = _batch(fn, reps)
    res["failed_blocks"] = eng.shampoo_state()["failed"]
    assert bool(torch.isfinite(sb).all())
    return res


def soap_kernels_alone(model, N, reps=20):
    eng = ast.build(model, N, "soap")
    for _ in range(2):
        eng.step()
    nat, st = eng.nat, torch.cuda.current_stream().cuda_stream
    sb, tab, nb = eng.shampoo_state_buf, eng.shampoo_tab.data_ptr(), len(eng.shampoo_blocks)
    L, Rt, QL, QR = (sb[i].data_ptr() for i in range(4))
    grad, gs, s0 = eng.grad.data_ptr(), eng.gstep.data_ptr(), eng.shampoo_start.data_ptr()
    fail, d = eng.shampoo_fail.data_ptr(), eng.shampoo_dir.data_ptr()
    coef = (eng.adam_beta1, eng.adam_beta2, eng.adam_epsilon)
    w, m, v = eng.params.master.clone(), eng.mom.clone(), eng.adam_v.clone()   # copies move
    launches = {
        "shampoo_stats": lambda: nat.shampoo_stats(grad, tab, nb, L, Rt, eng.shampoo_beta2, 1.0, gs,
                                                   s0, 1 << 30, fail, st),
        "soap_refresh_refresh": lambda: nat.soap_refresh(tab, nb, 2, L, Rt, QL, QR, gs, s0, 1, fail,
                                                         st),
        "soap_refresh_idle": lambda: nat.soap_refresh(tab, nb, 2, L, Rt, QL, QR, gs, s0, 1 << 30,
                                                      fail, st),
        "soap_rotate_adam": lambda: nat.soap_rotate_adam(grad, tab, nb, QL, QR, m.data_ptr(),
                                                         v.data_ptr(), d, *coef, 1.0, st),
        "soap_update_pack": lambda: nat.soap_update_pack(
            w.data_ptr(), grad, m.data_ptr(), v.data_ptr(), d, eng.params.n_train,
            *eng.sched.launch_args(), gs, s0, *coef, 1.0, eng.segs.data_ptr(), eng.nseg,
            eng.adam_wd.data_ptr(), eng.shampoo_seg.data_ptr(), eng.wbf.data_ptr(), 0, 0,
            *eng.sched.extra_launch_args(), st),
    }
    res = {"model": model, "blocks": nb, "conv_kernels": len(eng.shampoo_tensors),
           "state_mb": round((sb.numel() + 2 * eng.adam_v.numel()) * 4 / 2 ** 20, 1)}
    for name, fn in launches.items():
        res[name] = _batch(fn, reps)
    res["failed_blocks"] = eng.shampoo_state()["failed"]
    assert bool(torch.isfinite(sb).all())
    return res


def main():
    argv, variant = list(sys.argv[1:]), "roots"
    if "--variant" in argv:
        i = argv.index("--variant")
        variant = argv[i + 1]
        del argv[i:i + 2]
    cases = (argv[0] if len(argv) > 0 else "cifar_resnet50:128,imagenet_resnet50:128").split(",")
    steps = int(argv[1]) if len(argv) > 1 else 100
    rounds = int(argv[2]) if len(argv) > 2 else 5
    alone = soap_kernels_alone if variant == "soap" else kernels_alone
    for case in cases:
        model, N = case.split(":")
        print(json.dumps({"kernels_alone": alone(model, int(N))}), flush=True)
        torch.cuda.empty_cache()
        engs = {v: ast.build(model, int(N), v) for v in STEP_VARIANTS[variant]}
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
                              "plan_ops": eng.plan.size(),
                              "failed_blocks": eng.shampoo_state()["failed"] if eng.shampoo else None}),
                  flush=True)
        del engs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
