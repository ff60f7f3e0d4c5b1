"""--lr_decay cosine | poly without a GPU: the host mirror LRSchedule.at against the mpmath
oracle of tests/lr_decay_oracle.py at every step at which the formula can go wrong, the
scaling helpers, the flags (defaults = today's presets, errors), the recorder's extra launch
argument, the CLI on the CPU backend (rates in metrics.jsonl, a resumed run on the same curve)
and the compiler's resource remarks of the four optimizer kernels."""
import argparse
import dataclasses
import json
import os
import subprocess
import sys

import pytest

import kernel_resources as kr
import lr_decay_oracle as lo
from distributed_tensorflow_resnet_amd.train.schedule import (LRSchedule, cifar_lr_schedule,
                                                                decay_lr_schedule,
                                                                imagenet_lr_schedule,
                                                                lr_values_scaled, scaled,
                                                                schedule_from_flags)
from distributed_tensorflow_resnet_amd.utils.flags import build_parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = lo.cases()


# ---------------------------------------------------------------- the mirror
@pytest.mark.parametrize("name", list(CASES))
def test_mirror_matches_oracle(name):
    sched, steps = CASES[name]
    kinds = set()
    for s in steps:
        got = sched.at(s)
        assert got == lo.f32(got), (name, s, got)     # an fp32 value
        ref = lo.check_rate(sched, s, got, name)
        kinds.add("warm" if lo.in_warmup(sched, s) else "end" if s - 1 >= sched.decay_steps
                  else "start" if s < 1 else "decay")
        print(f"{name} step {s}: at {got!r} oracle {ref!r} "
              f"({(got - ref) / lo.ulp(ref or 1):+.0f} ulp)")
    assert {"decay", "end"} <= kinds
    if 1 in steps:
        assert ("warm" in kinds) == (sched.warm_steps > 0)


def test_oracle_is_the_textbook_curve():
    """The oracle itself, where the curve is known in closed form."""
    s = decay_lr_schedule("cosine", 0.5, 8, warm_steps=0, end=0.25)   # fp32 numbers
    assert lo.lr_oracle(s, 0) == 0.5 and lo.lr_oracle(s, 1) == 0.5
    assert lo.lr_oracle(s, 5) == 0.375                                # p = 1/2
    assert lo.lr_oracle(s, 9) == 0.25 and lo.lr_oracle(s, 2 ** 40) == 0.25
    p = decay_lr_schedule("poly", 0.5, 8, warm_steps=4, warm_from=0.25, end=0.0, power=2.0)
    assert [lo.lr_oracle(p, k) for k in (0, 1, 3, 5, 7, 9)] == [0.25, 0.25, 0.375, 0.5,
                                                                 0.5 * 0.25, 0.0]
    lin = dataclasses.replace(p, power=1.0)
    assert lo.lr_oracle(lin, 7) == 0.25
    # the cancellation the kernel's form avoids: at p = 1 - 1e-6 the rate is ~peak * 2.5e-12
    c, steps = CASES["cosine_cancel"]
    r = lo.lr_oracle(c, c.decay_steps)
    assert 0 < r < 1e-12 and steps[1] == c.decay_steps - 1


def test_decay_is_monotone_and_ends_exactly():
    for decay in ("cosine", "poly"):
        s = decay_lr_schedule(decay, 0.1, 50, warm_steps=5, warm_from=0.01, end=0.001)
        r = [s.at(k) for k in range(0, 60)]
        assert r[0] == r[1] == lo.f32(0.01) and r[6] == lo.f32(0.1) == max(r)
        assert all(a < b for a, b in zip(r[1:6], r[2:7]))
        assert all(a > b for a, b in zip(r[6:51], r[7:52]))
        assert r[51:] == [lo.f32(0.001)] * 9


def test_scaling_helpers_carry_the_new_fields():
    s = decay_lr_schedule("poly", 0.4, 1000, warm_steps=100, warm_from=0.1, end=0.004, power=3.0)
    t = scaled(s, 0.25)
    assert (t.warm_steps, t.decay_steps) == (25, 250)
    assert (t.decay, t.power, t.end, t.warm_to, t.warm_from, t.init) == ("poly", 3.0, 0.004, 0.4,
                                                                         0.1, 0.1)
    assert scaled(s, 1.0) is s and scaled(s, 1e-6).decay_steps == 1   # D > W survives
    v = lr_values_scaled(s, 0.5)
    assert (v.warm_to, v.end, v.warm_from, v.init) == (0.2, 0.002, 0.05, 0.05)
    assert (v.warm_steps, v.decay_steps, v.decay, v.power) == (100, 1000, "poly", 3.0)
    assert v.at(101) == lo.f32(0.2) and v.at(2000) == lo.f32(0.002)
    assert lr_values_scaled(s, 1.0) is s
    # the piecewise helpers give what they always gave
    im = imagenet_lr_schedule()
    assert scaled(im, 0.5) == LRSchedule(0.4, [18720, 37440, 49920], [0.4, 0.04, 0.004, 0.0004],
                                         3120, 0.1, 0.4)
    assert lr_values_scaled(im, 0.5).values == [0.2, 0.02, 0.002, 0.0002]


def test_launch_arguments():
    """launch_args() stays the piecewise 6-tuple; the decay parameters travel apart, and
    only for a decay schedule (a default run records the launches it always did)."""
    s = decay_lr_schedule("cosine", 0.1, 7, warm_steps=2, warm_from=0.01, end=0.001)
    assert s.launch_args() == (0.01, 2, 0.01, 0.1, [], [0.1])
    assert s.decay_args() == ("cosine", 7, 0.001, 2.0)
    assert s.extra_launch_args() == (s.decay_args(),)
    for p in (cifar_lr_schedule(), imagenet_lr_schedule()):
        assert p.extra_launch_args() == () and p.decay_args()[0] == "piecewise"
        assert len(p.launch_args()) == 6


@pytest.mark.parametrize("kw", [dict(decay_steps=2, warm_steps=2), dict(decay_steps=0),
                                dict(power=0.0), dict(power=-1.0), dict(power=float("nan")),
                                dict(end=-0.1), dict(end=float("inf")), dict(warm_from=-1.0),
                                dict(peak=float("nan"))])
def test_schedule_constraints(kw):
    a = dict(decay="poly", peak=0.1, decay_steps=10, warm_steps=1)
    a.update(kw)
    with pytest.raises(ValueError):
        decay_lr_schedule(a.pop("decay"), a.pop("peak"), a.pop("decay_steps"), **a)
    with pytest.raises(ValueError):
        decay_lr_schedule("piecewise", 0.1, 10)
    with pytest.raises(ValueError):
        LRSchedule(0.1, [], [0.1], decay="linear")


# ---------------------------------------------------------------- flags
@pytest.mark.parametrize("kind,preset", [("cifar", cifar_lr_schedule()),
                                         ("imagenet", imagenet_lr_schedule())])
def test_flag_defaults_build_the_preset(kind, preset):
    ns = build_parser(kind).parse_args([])
    assert (ns.lr_decay, ns.lr_peak, ns.lr_warmup_steps, ns.lr_warmup_from, ns.lr_decay_steps,
            ns.lr_end, ns.lr_poly_power) == ("piecewise", None, -1, None, 0, 0.0, 2.0)
    assert schedule_from_flags(ns) == preset
    assert schedule_from_flags(ns).extra_launch_args() == ()
    for flag in ("--lr_decay", "--lr_peak", "--lr_warmup_steps", "--lr_warmup_from",
                 "--lr_decay_steps", "--lr_end", "--lr_poly_power"):
        assert flag in build_parser(kind).format_help()


def test_flags_build_decay_schedules():
    ns = build_parser("cifar").parse_args(["--lr_decay", "cosine", "--train_steps", "300"])
    assert schedule_from_flags(ns) == decay_lr_schedule("cosine", 0.1, 300)
    ns = build_parser("imagenet").parse_args(["--lr_decay", "poly", "--train_steps", "112590"])
    assert schedule_from_flags(ns) == decay_lr_schedule("poly", 0.4, 112590, warm_steps=6240,
                                                        warm_from=0.1, power=2.0)
    ns = build_parser("imagenet").parse_args(
        ["--lr_decay", "poly", "--lr_peak", "3.2", "--lr_warmup_steps", "500", "--lr_warmup_from",
         "0", "--lr_decay_steps", "9000", "--lr_end", "0.0001", "--lr_poly_power", "1.5"])
    assert schedule_from_flags(ns) == decay_lr_schedule("poly", 3.2, 9000, warm_steps=500,
                                                        warm_from=0.0, end=0.0001, power=1.5)
    # piecewise takes the peak (its drops keep their ratios) and a warm-up
    ns = build_parser("cifar").parse_args(["--lr_peak", "0.2", "--lr_warmup_steps", "10"])
    s = schedule_from_flags(ns)
    assert (s.decay, s.bounds, s.warm_steps, s.warm_from, s.warm_to) == (
        "piecewise", [40000, 60000, 80000], 10, 0.0, 0.2)
    assert s.values[0] == 0.2 and s.values[1] == pytest.approx(0.02) and s.init == 0.2
    ns = build_parser("imagenet").parse_args(["--lr_warmup_steps", "0"])
    assert schedule_from_flags(ns).at(1) == 0.4


@pytest.mark.parametrize("args", [
    ["--lr_decay", "cosine", "--lr_warmup_steps", "10", "--lr_decay_steps", "10"],
    ["--lr_decay", "poly", "--lr_warmup_steps", "300", "--train_steps", "200"],
    ["--lr_decay", "cosine", "--dataset", "imagenet", "--train_steps", "6240"],   # preset warm-up
    ["--lr_decay", "cosine", "--lr_peak=-0.1"], ["--lr_decay", "cosine", "--lr_peak", "inf"],
    ["--lr_decay", "cosine", "--lr_end", "nan"], ["--lr_decay", "cosine", "--lr_end=-1"],
    ["--lr_warmup_from=-0.5"], ["--lr_peak", "x"],
    ["--lr_decay", "poly", "--lr_poly_power", "0"], ["--lr_decay", "poly", "--lr_poly_power=-2"],
    ["--lr_decay", "poly", "--lr_poly_power", "nan"],
    ["--lr_decay_steps", "100"], ["--lr_end", "0.01"], ["--lr_poly_power", "3"],
    ["--lr_decay", "piecewise", "--lr_end", "0.01"], ["--lr_decay", "linear"]])
def test_flag_errors(args, capsys):
    with pytest.raises(SystemExit) as ei:
        build_parser("cifar").parse_args(args)
    assert ei.value.code == 2 and "--lr_" in capsys.readouterr().err


def test_flag_error_messages(capsys):
    for args, text in ((["--lr_decay", "cosine", "--lr_warmup_steps", "9", "--lr_decay_steps", "9"],
                        "must exceed the warm-up"),
                       (["--lr_end", "0.01"], "cannot be combined with --lr_decay piecewise"),
                       (["--lr_decay", "poly", "--lr_poly_power", "0"], "positive")):
        with pytest.raises(SystemExit):
            build_parser("cifar").parse_args(args)
        assert text in capsys.readouterr().err


def test_flags_namespace_is_all_the_builder_needs():
    ns = argparse.Namespace(dataset="cifar10", train_steps=10, lr_decay="cosine", lr_peak=None,
                            lr_warmup_steps=2, lr_warmup_from=None, lr_decay_steps=5, lr_end=0.0,
                            lr_poly_power=2.0)
    assert schedule_from_flags(ns) == decay_lr_schedule("cosine", 0.1, 5, warm_steps=2)


# ---------------------------------------------------------------- the CLI on the CPU backend
CLI_SCHED = decay_lr_schedule("cosine", 0.1, 5, warm_steps=2)


def _cli(args):
    e = dict(os.environ)
    e.update({"CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": "", "OMP_NUM_THREADS": "2"})
    return subprocess.run([sys.executable, "resnet_cifar_main.py", "--device", "cpu", "--synthetic",
                           "--resnet_size", "8", "--batch_size", "4", "--log_every", "1",
                           "--summary_every", "1", "--lr_decay", "cosine", "--lr_warmup_steps", "2",
                           "--lr_decay_steps", "5"] + args,
                          cwd=ROOT, capture_output=True, text=True, timeout=600, env=e)


def _rates(log_dir):
    rows = [json.loads(line) for line in open(os.path.join(log_dir, "metrics.jsonl"))]
    return [(r["global_step"], r["lr"]) for r in rows]


@pytest.fixture(scope="module")
def cli_straight(tmp_path_factory):
    d = tmp_path_factory.mktemp("straight")
    r = _cli(["--train_steps", "6", "--train_dir", str(d / "train"), "--log_dir", str(d / "log")])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return _rates(str(d / "log")), r.stdout + r.stderr


def test_cli_writes_the_oracle_rates(cli_straight):
    rates, out = cli_straight
    assert [g for g, _ in rates] == [1, 2, 3, 4, 5, 6]
    for g, lr in rates:   # the row of global_step g is training step g - 1
        lo.check_rate(CLI_SCHED, g - 1, lr, "cli")
    want = [lo.lr_oracle(CLI_SCHED, s) for s in range(6)]
    assert want[0] == want[1] == 0.0 and want[3] == lo.f32(0.1) and want[2] == lo.f32(0.1) / 2
    assert want[3] > want[4] > want[5] > 0
    assert f"lr = {want[4]:.6g}" in out       # LearningRate / logging hooks show the decayed rate


def test_cli_resumed_run_continues_on_the_curve(cli_straight, tmp_path):
    td, ld = str(tmp_path / "train"), str(tmp_path / "log")
    for steps in ("3", "6"):   # two processes: the second restores step 3's checkpoint
        r = _cli(["--train_steps", steps, "--train_dir", td, "--log_dir", ld])
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert _rates(ld) == cli_straight[0]


# ---------------------------------------------------------------- compiler remarks
OPT_KERNELS = {"optim.hip": ("sgd_pack_kernel", "sgd_tiles_kernel"),
               "lars.hip": ("lars_sgd_pack_kernel",), "clip.hip": ("sgd_clip_pack_kernel",)}


@pytest.mark.skipif(not kr.have_compiler(), reason="no ROCm compiler")
@pytest.mark.parametrize("src", list(OPT_KERNELS))
def test_optimizer_kernels_have_no_spills(src):
    """The fp64 decay (sinpi, exp, log) is inlined into every kernel that evaluates the
    schedule: none may spill VGPRs or use scratch for it (profiles/lr_schedules.md has the
    counts before and after)."""
    rows = kr._resources(os.path.join(kr.CSRC, src))
    kernels = {n: r for n, r in rows.items() if any(k in n for k in OPT_KERNELS[src])}
    assert len(kernels) == (4 if src == "optim.hip" else 1), sorted(rows)   # sgd_tiles: 3 modes
    for name, r in kernels.items():
        assert int(r["VGPRs Spill"]) == 0, (name, r)
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)


# kernel: (instantiations, waves per SIMD before the walks were shared in optim_device.h)
WALK_KERNELS = {"sgd_pack_kernel": (1, 4), "lars_sgd_pack_kernel": (1, 4),
                "sgd_clip_pack_kernel": (1, 4), "adam_pack_kernel": (2, 4),
                "lamb_pack_kernel": (1, 4), "lars_norms_kernel": (1, 7),
                "lamb_moments_norms_kernel": (2, 3), "lars_trust_kernel": (1, 8),
                "lamb_trust_kernel": (1, 8), "grad_sqnorm_kernel": (1, 8),
                "clip_scale_kernel": (1, 8)}


@pytest.mark.skipif(not kr.have_compiler(), reason="no ROCm compiler")
def test_shared_walks_keep_the_optimizer_kernels_occupancy():
    """The flat walk, the chunk reduction and the partial sums are force-inlined templates of
    optim_device.h: no kernel that uses them may spill, use scratch or hold fewer waves than
    its own copy did (profiles/optim_walk.md; VGPR and SGPR counts are printed, not pinned)."""
    rows = [(n, r) for n, r in kr.optimizer_resources() if n in WALK_KERNELS]
    assert {n: sum(m == n for m, _ in rows) for n in WALK_KERNELS} == \
        {n: k for n, (k, _) in WALK_KERNELS.items()}
    for name, r in rows:
        print(f"{name}: VGPRs {r['VGPRs']} SGPRs {r['TotalSGPRs']} "
              f"waves/SIMD {r['Occupancy [waves/SIMD]']}")
        assert int(r["VGPRs Spill"]) == 0, (name, r)
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= WALK_KERNELS[name][1], (name, r)
