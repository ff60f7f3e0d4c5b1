"""Random Erasing off the GPU: the specification (data/cifar.py erase_table / erase_thresh /
erase_draw / erase_noise_table) against its own stated properties and the plain-integer
re-derivation of tests/erase_oracle.py, the flags, and the CPU trainer's erase."""
import json
import math
import types

import numpy as np
import pytest
import torch
import erase_oracle as eo

from distributed_tensorflow_resnet_amd.data import cifar
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.train import hooks as H
from distributed_tensorflow_resnet_amd.train import layout
from distributed_tensorflow_resnet_amd.train.backends import CPUBackend
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr
from distributed_tensorflow_resnet_amd.utils import flags as flags_mod
from distributed_tensorflow_resnet_amd.utils.flags import build_parser

SEED = 4321
ONE = 2 ** 24
DEFAULTS = (0.02, 1.0 / 3.0, 0.3)


# ---------------------------------------------------------------- 1. table
@pytest.mark.parametrize("H,W", [(32, 32), (224, 224), (12, 20)])
@pytest.mark.parametrize("params", [DEFAULTS, (0.1, 0.1, 1.0), (0.5, 1.0, 0.1)])
def test_table_entries(H, W, params):
    amin, amax, aspect = params
    t = cifar.erase_table(SEED, H, W, amin, amax, aspect)
    assert t.dtype == np.int32 and t.shape == (4096,) and (t >= 0).all()
    nz = t[t != 0].astype(np.int64)
    eh, ew = nz >> 16, nz & 0xFFFF
    assert ((1 <= eh) & (eh < H) & (1 <= ew) & (ew < W)).all()
    # the rounding bound: eh = round(a), ew = round(b) with a * b = area, so |eh - a| <= 1/2,
    # |ew - b| <= 1/2 and |eh * ew - area| <= (a + b) / 2 + 1/4 <= (eh + ew + 1) / 2 + 1/4
    slack = (eh + ew + 1) / 2 + 0.25
    area = eh * ew
    assert (area >= amin * H * W - slack).all() and (area <= amax * H * W + slack).all()
    # the aspect ratio, within the same rounding: a / b in [aspect, 1 / aspect]
    assert ((eh + 0.5) / (ew - 0.5 + 1e-9) >= aspect).all()
    assert ((eh - 0.5) / (ew + 0.5) <= 1 / aspect).all()
    # reproducible by seed, and a function of it
    assert np.array_equal(t, cifar.erase_table(SEED, H, W, amin, amax, aspect))
    if amin < amax:   # (a fixed area at aspect 1 is one box, whatever the seed)
        assert not np.array_equal(t, cifar.erase_table(SEED + 1, H, W, amin, amax, aspect))
    assert cifar.erase_table(SEED, H, W, amin, amax, aspect, 16).shape == (16,)


@pytest.mark.parametrize("H", [32, 224])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_default_table_has_few_empty_entries(H, seed):
    t = cifar.erase_table(seed, H, H, *DEFAULTS).astype(np.int64)
    assert (t == 0).mean() <= 0.01   # the condition; the simulation found none
    eh, ew = t[t != 0] >> 16, t[t != 0] & 0xFFFF
    print(f"{H}x{H} seed {seed}: zero {(t == 0).sum()}, sizes {min(eh.min(), ew.min())}.."
          f"{max(eh.max(), ew.max())}, odd eh {(eh & 1).mean():.3f}, "
          f"mean area {(eh * ew).mean() / (H * H):.4f}")
    assert (eh & 1).any() and (ew & 1).any() and not (eh & 1).all() and not (ew & 1).all()


def test_table_refuses_bad_arguments():
    for bad in ((0.0, 0.3, 0.3), (0.4, 0.3, 0.3), (0.02, 1.1, 0.3), (0.02, 0.3, 0.0),
                (0.02, 0.3, 1.5), (float("nan"), 0.3, 0.3), (0.02, 0.3, float("nan"))):
        with pytest.raises(ValueError):
            cifar.erase_table(SEED, 32, 32, *bad)
    for H, W in ((1, 32), (32, 1 << 15)):
        with pytest.raises(ValueError):
            cifar.erase_table(SEED, H, W, *DEFAULTS)
    # a box that can never fit (the whole image at H, W: eh < H fails) gives the 0 entry
    assert (cifar.erase_table(SEED, 4, 4, 1.0, 1.0, 1.0, 8) == 0).all()


def test_thresh():
    assert cifar.erase_thresh(0.0) == 0 and cifar.erase_thresh(1.0) == ONE
    assert cifar.erase_thresh(0.5) == 2 ** 23 and cifar.erase_thresh(0.3) == round(0.3 * ONE)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            cifar.erase_thresh(bad)


def test_noise_table():
    t = cifar.erase_noise_table(SEED)
    assert t.dtype == np.float32 and t.shape == (4096,) and np.isfinite(t).all()
    assert np.array_equal(t, cifar.erase_noise_table(SEED))
    assert not np.array_equal(t, cifar.erase_noise_table(SEED + 1))
    assert abs(float(t.mean())) < 5 / math.sqrt(4096) and 0.9 < float(t.std()) < 1.1
    assert cifar.erase_noise_table(SEED, 8).shape == (8,)


# ---------------------------------------------------------------- 2. draw
@pytest.mark.parametrize("H,W", [(32, 32), (224, 224), (12, 20)])
def test_draw_fits_and_equals_the_oracle(H, W):
    t = cifar.erase_table(SEED, H, W, *DEFAULTS)
    for step in (0, 1, 7, 2 ** 32 + 3, 2 ** 40 + 1):
        for n in range(64):
            d = cifar.erase_draw(SEED, step, n, len(t), H, W, t, ONE)
            want = eo.draw(SEED, step, n, t, H, W, ONE)
            assert d == want, (step, n)
            assert d["on"] is (int(t[d["index"]]) != 0)   # always on at 2^24, but for entry 0
            assert cifar.erase_draw(SEED, step, n, len(t), H, W, t, 0)["on"] is False
            if d["on"]:
                assert t[d["index"]] == (d["eh"] << 16 | d["ew"])
                assert 0 <= d["y0"] and d["y0"] + d["eh"] <= H
                assert 0 <= d["x0"] and d["x0"] + d["ew"] <= W
    off = cifar.erase_draw(SEED, 0, 0, len(t), H, W, t, 0)
    assert (off["y0"], off["x0"], off["eh"], off["ew"]) == (0, 0, 0, 0)


def test_draw_zero_entry_is_off_and_bad_arguments():
    assert cifar.erase_draw(SEED, 3, 1, 1, 32, 32, [0], ONE)["on"] is False
    d = cifar.erase_draw(SEED, 3, 1, 1, 32, 32, [31 << 16 | 31], ONE)
    assert d["on"] and d["y0"] in (0, 1) and d["x0"] in (0, 1)
    with pytest.raises(ValueError):   # an entry that does not fit the image
        cifar.erase_draw(SEED, 3, 1, 1, 32, 32, [33 << 16 | 4], ONE)
    for bad in (-1, ONE + 1):
        with pytest.raises(ValueError):
            cifar.erase_draw(SEED, 0, 0, 1, 32, 32, [0], bad)
    with pytest.raises(ValueError):
        cifar.erase_draw(SEED, -1, 0, 1, 32, 32, [0], ONE)


def test_draw_rate_is_binomial():
    t = [5 << 16 | 7]   # never the 0 entry: `on` is the threshold's decision alone
    p, thresh = 0.25, cifar.erase_thresh(0.25)
    n_on = sum(cifar.erase_draw(SEED, step, n, 1, 32, 32, t, thresh)["on"]
               for step in range(1000) for n in range(100))
    total = 100000
    sd = math.sqrt(total * p * (1 - p))
    print(f"on {n_on} of {total}: {(n_on - total * p) / sd:+.2f} sd")
    assert abs(n_on - total * p) <= 5 * sd


def test_draw_hash_is_no_crop_and_no_mix_hash():
    for step in (0, 1, 5, 2 ** 32 + 3):
        for n in range(16):
            h = cifar.erase_hash(SEED, step, n)
            assert h == eo.draw_hash(SEED, step, n)
            assert h != eo.crop_hash(SEED, step, n)
            assert h != cifar.splitmix((SEED & eo.M64) ^
                                       cifar.splitmix((step * 0x100000001B3 + n) & eo.M64))
            assert h != cifar._mix_hash(SEED, step)
    # per image: the positions of one step draw differently
    assert len({cifar.erase_hash(SEED, 0, n) for n in range(128)}) == 128


def test_draw_is_exact_past_32_bits():
    t = cifar.erase_table(SEED, 32, 32, *DEFAULTS)
    step, n = 2 ** 32 + 3, 2
    # the unbounded-integer formula, written out
    P, M = 0x100000001B3, (1 << 64) - 1
    h = eo.splitmix(eo.splitmix((SEED ^ cifar.ERASE_SALT) & M) ^ eo.splitmix((step * P + n) % 2 ** 64))
    h2 = eo.splitmix(h ^ cifar.ERASE_SALT)
    d = cifar.erase_draw(SEED, step, n, len(t), 32, 32, t, ONE)
    e = int(t[(h & 0xFFFFFFFF) % len(t)])
    eh, ew = e >> 16, e & 0xFFFF
    assert (d["index"], d["eh"], d["ew"]) == ((h & 0xFFFFFFFF) % len(t), eh, ew)
    assert (d["y0"], d["x0"]) == ((h2 & 0xFFFFFFFF) % (32 - eh + 1), (h2 >> 32) % (32 - ew + 1))
    key = lambda s: tuple(cifar.erase_draw(SEED, s, n, len(t), 32, 32, t, ONE).values())  # noqa: E731
    assert len({key(3), key(step), key(step + 1)}) == 3   # not the step modulo 2^32


# ---------------------------------------------------------------- 3. flags
@pytest.mark.parametrize("kind", ["cifar", "imagenet"])
def test_flags(kind):
    p = lambda *a: build_parser(kind).parse_args(list(a))   # noqa: E731
    ns = p()
    assert (ns.erase_prob, ns.erase_area_min, ns.erase_area_max, ns.erase_aspect_min,
            ns.erase_fill) == (0.0, 0.02, 1.0 / 3.0, 0.3, "zero")
    ns = p("--erase_prob", "0.25", "--erase_area_min=0.1", "--erase_area_max=0.2",
           "--erase_aspect_min=0.5")
    assert (ns.erase_prob, ns.erase_area_min, ns.erase_area_max, ns.erase_aspect_min) == \
        (0.25, 0.1, 0.2, 0.5)
    for edge in ("0", "1"):
        assert p(f"--erase_prob={edge}").erase_prob == float(edge)
    for bad in ("-0.1", "1.5", "nan", "x"):
        with pytest.raises(SystemExit):
            p(f"--erase_prob={bad}")
    for bad in (("--erase_area_min=0",), ("--erase_area_min=0.5", "--erase_area_max=0.4"),
                ("--erase_area_max=1.5",), ("--erase_area_min=nan",),
                ("--erase_aspect_min=0",), ("--erase_aspect_min=1.5",),
                ("--erase_aspect_min=nan",), ("--erase_fill=mean",)):
        for prob in ("0", "0.5"):   # a violation is an error with the flag off too
            with pytest.raises(SystemExit):
                p(f"--erase_prob={prob}", *bad)
    assert p("--erase_area_min=0.25", "--erase_area_max=0.25", "--erase_aspect_min=1").erase_prob == 0
    with pytest.raises(SystemExit):
        p("--erase_prob", "0.5", "--synthetic")
    assert p("--erase_prob", "0", "--synthetic").synthetic
    if kind == "imagenet":   # mean-subtracted, unscaled inputs: unit noise is a constant
        with pytest.raises(SystemExit):
            p("--erase_prob", "0.5", "--erase_fill", "noise")
        assert p("--erase_prob", "0.5", "--erase_fill", "zero").erase_fill == "zero"
    else:
        assert p("--erase_prob", "0.5", "--erase_fill", "noise").erase_fill == "noise"


def test_defaults_are_todays_namespace_plus_the_new_fields(monkeypatch):
    new = {"erase_prob", "erase_area_min", "erase_area_max", "erase_aspect_min", "erase_fill"}
    add = flags_mod.FlagParser.add_argument

    def without_erase(self, *names, **kw):   # the parser as it is without the five flags
        if not names[0].startswith("--erase_"):
            return add(self, *names, **kw)

    for kind in ("cifar", "imagenet", "cifar_eval", "imagenet_eval", "single"):
        ns = vars(build_parser(kind).parse_args([]))
        with monkeypatch.context() as mp:
            mp.setattr(flags_mod.FlagParser, "add_argument", without_erase)
            today = vars(build_parser(kind).parse_args([]))
        assert not new & set(today) and set(ns) == set(today) | new
        assert {k: ns[k] for k in today} == today   # every other field, value for value
        assert len(today) > 60 and ns["cutmix_alpha"] == 0.0 and ns["mix_switch_prob"] == 0.5
        assert ns["batch_size"] == (128 if kind.startswith("imagenet") else 32)
        assert {k: ns[k] for k in sorted(new)} == {
            "erase_area_max": 1.0 / 3.0, "erase_area_min": 0.02, "erase_aspect_min": 0.3,
            "erase_fill": "zero", "erase_prob": 0.0}
        on = vars(build_parser(kind).parse_args(["--erase_prob=0.5"]))
        assert {k for k in ns if ns[k] != on[k]} == {"erase_prob"}


@pytest.mark.parametrize("on", [False, True])
def test_hooks_carry_the_erase_values_only_with_the_flag(tmp_path, capsys, on):
    m = {"global_step": 1, "cross_entropy": 2.0, "cost": 2.5, "precision": 0.25, "lr": 0.1,
         "l2": 3.0}
    if on:
        m.update(erase_count=3, erase_area=0.171875)
    s = types.SimpleNamespace(metrics=lambda: m, is_chief=True,
                              backend=types.SimpleNamespace(), global_step=1)
    path = str(tmp_path / "metrics.jsonl")
    H.JsonlMetricsHook(path, every=1).after_run(s, 1)
    row = json.loads(open(path).read())
    assert ("erase_count" in row, "erase_area" in row) == (on, on)
    if on:
        assert (row["erase_count"], row["erase_area"]) == (3, 0.171875)
    capsys.readouterr()
    H.LoggingTensorHook(every_n_iter=1).after_run(s, 1)
    line = capsys.readouterr().out
    assert (", erased = 3 (area 0.1719)" in line) == on and "lr = 0.1" in line
    assert ("erased" in line) == on


def test_layout_check():
    assert layout.check_erase(0) == (0.0, 0.02, 1.0 / 3.0, 0.3, "zero")
    assert layout.check_erase("0.5", 0.1, 0.2, 1, "noise", "cifar10")[4] == "noise"
    for bad in ((-0.1,), (1.1,), (float("nan"),), ("x",), (None,), (0.5, 0.0), (0.5, 0.3, 0.2),
                (0.5, 0.02, 1.5), (0.5, 0.02, 0.3, 0.0), (0.5, 0.02, 0.3, 2.0),
                (0.5, 0.02, 0.3, 0.3, "mean"), (0.5, 0.02, 0.3, 0.3, "noise", "imagenet")):
        with pytest.raises(ValueError):
            layout.check_erase(*bad)


# ---------------------------------------------------------------- 4. CPU backend
def _trainer(**kw):
    return CPUBackend(cifar_spec(8), 4, weight_decay=2e-4, lr_schedule=constant_lr(0.1), **kw)


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(4, 32, 32, 3, generator=g), torch.randint(0, 10, (4,), generator=g)


@pytest.mark.parametrize("fill", ["zero", "noise"])
@pytest.mark.parametrize("mixup", [0.0, 0.4])
def test_cpu_trainer_erases_after_its_mix(fill, mixup):
    x, y = _batch(5)
    be = _trainer(erase_prob=1.0, erase_fill=fill, data_seed=SEED, mixup_alpha=mixup)
    off = _trainer(erase_prob=0.0, erase_fill=fill, data_seed=SEED, mixup_alpha=mixup)
    assert be.erase_state() is None and off.erase_state() is None
    table, noise = cifar.erase_table(SEED, 32, 32, *DEFAULTS), cifar.erase_noise_table(SEED)
    for step in range(2):
        for b in (be, off):
            b.set_batch(x, y)
            b.step()
        # the p = 0 run's input: the (mixed) batch itself
        base = off.last_input.numpy() if mixup else x.numpy()
        st = be.erase_state()
        assert np.array_equal(st, eo.state(SEED, step, 4, table, 32, 32, ONE))
        assert st[:, 0].all()   # p = 1 and no empty entry among these draws
        mask = eo.box_mask(st, 32, 32)
        got = be.last_input.numpy()
        assert np.array_equal(got[~mask], base[~mask])   # every other pixel, bit for bit
        for n in range(4):
            d = eo.draw(SEED, step, n, table, 32, 32, ONE)
            box = got[n, d["y0"]:d["y0"] + d["eh"], d["x0"]:d["x0"] + d["ew"]]
            if fill == "zero":
                assert (box == 0).all() and not np.signbit(box).any()
            else:
                want = np.array([[[noise[eo.splitmix(d["h2"] ^ ((yy * 32 + xx) * 4 + c)) % 4096]
                                   for c in range(3)]
                                  for xx in range(d["x0"], d["x0"] + d["ew"])]
                                 for yy in range(d["y0"], d["y0"] + d["eh"])])
                assert np.array_equal(box, want)
        m = be.metrics()
        assert m["erase_count"] == 4
        assert m["erase_area"] == float((st[:, 3] * st[:, 4]).sum() / (4 * 1024))
        assert "erase_count" not in off.metrics()
        if mixup:   # labels and lam are untouched
            assert be.mix_state() == off.mix_state()


def test_cpu_trainer_zero_prob_is_the_default():
    plain = _trainer(data_seed=SEED)
    zero = _trainer(data_seed=SEED, erase_prob=0.0, erase_area_min=0.1, erase_area_max=0.2,
                    erase_aspect_min=0.5, erase_fill="noise")
    for step in range(3):
        x, y = _batch(10 + step)
        for be in (plain, zero):
            be.set_batch(x, y)
            be.step()
            assert torch.equal(be._x, x)   # the batch fed to the model
        assert plain.metrics(top5=True) == zero.metrics(top5=True)
    assert torch.equal(plain.store.master, zero.store.master)
    assert torch.equal(plain.mom, zero.mom)
    assert torch.equal(plain.store.stats, zero.store.stats)
    assert zero.erase_state() is None and zero.erase_tab is None
    # and erasing is visible in the weights
    on = _trainer(data_seed=SEED, erase_prob=1.0)
    for step in range(3):
        on.set_batch(*_batch(10 + step))
        on.step()
    assert not torch.equal(plain.store.master, on.store.master)
    for bad in ({"erase_prob": 1.5}, {"erase_prob": 0.5, "erase_area_min": 0.0},
                {"erase_prob": 0.5, "erase_fill": "mean"}):
        with pytest.raises(ValueError):
            _trainer(**bad)
