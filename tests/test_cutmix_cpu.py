"""CutMix off the GPU: the specification (data/cifar.py cutmix_table / cutmix_thresh /
cutmix_draw) against the plain-integer re-derivation of tests/cutmix_oracle.py, the flags, and
one pasted step of the CPU trainer against the host paste and the two-label fp64 loss."""
import numpy as np
import pytest
import torch
import cutmix_oracle as co
import mixup_oracle as mo

from distributed_tensorflow_resnet_amd.data import cifar
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.train import layout
from distributed_tensorflow_resnet_amd.train.backends import CPUBackend
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr
from distributed_tensorflow_resnet_amd.utils.flags import build_parser

SEED = 4321
ONE = 2 ** 24
STEPS = [0, 1, 7, 2 ** 32 + 3] + list(range(100, 400))


@pytest.mark.parametrize("H,W,batch", [(32, 32, 5), (12, 20, 3), (224, 224, 128), (32, 32, 1)])
def test_draw_equals_the_oracle(H, W, batch):
    entries = cifar.cutmix_table(1.0, SEED, H, W)
    n_clipped = n_interior = 0
    for step in STEPS:
        d = cifar.cutmix_draw(SEED, step, batch, len(entries), H, W, entries, ONE)
        want = co.draw(SEED, step, batch, len(entries), H, W, entries, ONE)
        assert (d["index"], d["shift"]) == cifar.mixup_draw(SEED, step, batch, len(entries))
        assert d["cut"] is True
        for k, v in want.items():
            assert d[k] == v, (step, k)
        assert 0 <= d["y0"] <= d["y1"] <= H and 0 <= d["x0"] <= d["x1"] <= W
        assert d["area"] == (d["y1"] - d["y0"]) * (d["x1"] - d["x0"])
        lam = np.float32(H * W - d["area"]) / np.float32(H * W)
        assert d["lam"].dtype == np.float32 and d["lam"] == lam and 0.0 <= lam <= 1.0
        e = int(entries[d["index"]])
        full = (2 * ((e >> 16) // 2)) * (2 * ((e & 0xFFFF) // 2))
        n_clipped += d["area"] < full
        n_interior += d["area"] == full > 0
    assert n_clipped > 10 and n_interior > 10   # both kinds of box are drawn


def test_draw_is_exact_past_32_bits():
    entries = cifar.cutmix_table(1.0, SEED, 32, 32)
    lo, hi = 3, 2 ** 32 + 3
    key = lambda d: (d["index"], d["shift"], d["cy"], d["cx"])   # noqa: E731
    draws = {key(cifar.cutmix_draw(SEED, s, 128, 4096, 32, 32, entries, ONE))
             for s in (lo, hi, hi + 1)}
    assert len(draws) == 3


def test_thresh_decides_the_mode():
    entries = cifar.cutmix_table(1.0, SEED, 32, 32)
    cut = lambda s, t: cifar.cutmix_draw(SEED, s, 5, 4096, 32, 32, entries, t)  # noqa: E731
    for s in STEPS:
        d = cut(s, 0)
        assert d["cut"] is False and d["lam"] is None
        assert (d["y0"], d["y1"], d["x0"], d["x1"], d["area"], d["cy"], d["cx"]) == (0,) * 7
        assert (d["index"], d["shift"]) == cifar.mixup_draw(SEED, s, 5, 4096)
        assert cut(s, ONE)["cut"] is True
    n = sum(cut(s, 2 ** 23)["cut"] for s in range(4096))
    assert 0.45 <= n / 4096 <= 0.55
    for s in range(64):   # the oracle agrees on the mode at a threshold in between
        assert cut(s, 2 ** 23)["cut"] == co.draw(SEED, s, 5, 4096, 32, 32, entries, 2 ** 23)["cut"]
    for bad in (-1, ONE + 1):
        with pytest.raises(ValueError):
            cut(0, bad)


def test_cutmix_thresh():
    assert cifar.cutmix_thresh(0.2, 0.0, 0.5) == 0
    assert cifar.cutmix_thresh(0.0, 0.0, 0.5) == 0
    assert cifar.cutmix_thresh(0.0, 1.0, 0.5) == ONE
    assert cifar.cutmix_thresh(0.2, 1.0, 0.5) == 2 ** 23
    assert cifar.cutmix_thresh(0.2, 1.0, 0.0) == 0
    assert cifar.cutmix_thresh(0.2, 1.0, 1.0) == ONE
    assert cifar.cutmix_thresh(0.2, 1.0, 0.3) == round(0.3 * ONE)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            cifar.cutmix_thresh(0.2, 1.0, bad)


@pytest.mark.parametrize("H,W", [(32, 32), (224, 224), (12, 20)])
def test_table_is_the_fp64_formula(H, W):
    t = cifar.cutmix_table(1.0, 7, H, W)
    lam = cifar.mixup_table(1.0, 7 ^ 0x4355544D4958)
    assert t.dtype == np.int32 and t.shape == (4096,)
    assert np.array_equal(t.astype(np.int64), co.table(lam, H, W))
    assert ((t >> 16) <= H).all() and ((t & 0xFFFF) <= W).all() and (t >= 0).all()
    assert cifar.cutmix_table(0.5, 7, H, W, 16).shape == (16,)
    assert not np.array_equal(t, cifar.cutmix_table(1.0, 8, H, W))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            cifar.cutmix_table(bad, 7, H, W)


def test_table_entry_of_lam_one_is_empty(monkeypatch):
    monkeypatch.setattr(cifar, "mixup_table",
                        lambda a, s, n: np.array([1.0, 0.0, 0.75], dtype=np.float32))
    t = cifar.cutmix_table(1.0, 7, 32, 20, 3)
    assert t.tolist() == [0, 32 << 16 | 20, 16 << 16 | 10]
    d = cifar.cutmix_draw(SEED, 0, 5, 1, 32, 20, t[:1], ONE)
    assert d["cut"] and d["area"] == 0 and d["lam"] == np.float32(1.0)


@pytest.mark.parametrize("kind", ["cifar", "imagenet"])
def test_flags(kind):
    p = lambda *a: build_parser(kind).parse_args(list(a))   # noqa: E731
    ns = p()
    assert ns.cutmix_alpha == 0.0 and ns.mix_switch_prob == 0.5
    ns = p("--cutmix_alpha", "1.0")
    assert ns.cutmix_alpha == 1.0 and ns.mix_switch_prob == 0.5 and ns.mixup_alpha == 0.0
    ns = p("--cutmix_alpha", "1.0", "--mixup_alpha", "0.2", "--mix_switch_prob", "0.25")
    assert (ns.cutmix_alpha, ns.mixup_alpha, ns.mix_switch_prob) == (1.0, 0.2, 0.25)
    for edge in ("0", "1"):
        assert p("--cutmix_alpha=1", "--mixup_alpha=0.2",
                 f"--mix_switch_prob={edge}").mix_switch_prob == float(edge)
    for bad in ("-0.1", "nan", "inf", "x"):
        with pytest.raises(SystemExit):
            p(f"--cutmix_alpha={bad}")
    for bad in ("-0.1", "1.5", "nan", "x"):
        with pytest.raises(SystemExit):
            p("--cutmix_alpha=1", "--mixup_alpha=0.2", f"--mix_switch_prob={bad}")
    with pytest.raises(SystemExit):
        p("--cutmix_alpha", "1.0", "--synthetic")
    assert p("--cutmix_alpha", "0", "--synthetic").synthetic
    # the switch probability needs both augmentations
    for alphas in ((), ("--cutmix_alpha=1",), ("--mixup_alpha=0.2",),
                   ("--cutmix_alpha=0", "--mixup_alpha=0.2")):
        with pytest.raises(SystemExit):
            p(*alphas, "--mix_switch_prob", "0.5")


def test_layout_checks():
    assert layout.check_cutmix_alpha(0) == 0.0 and layout.check_cutmix_alpha("1.5") == 1.5
    for bad in (-0.1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError):
            layout.check_cutmix_alpha(bad)
    assert layout.check_mix_switch_prob(0) == 0.0 and layout.check_mix_switch_prob(1) == 1.0
    for bad in (-0.1, 1.01, float("nan"), "x", None):
        with pytest.raises(ValueError):
            layout.check_mix_switch_prob(bad)


def _trainer(**kw):
    return CPUBackend(cifar_spec(8), 4, weight_decay=2e-4, lr_schedule=constant_lr(0.1), **kw)


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(4, 32, 32, 3, generator=g), torch.randint(0, 10, (4,), generator=g)


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_cpu_trainer_pasted_step(eps):
    x, y = _batch(5)
    be = _trainer(cutmix_alpha=1.0, data_seed=SEED, label_smoothing=eps)
    assert be.mix_state() is None
    be.set_batch(x, y)
    be.step()
    entries = cifar.cutmix_table(1.0, SEED, 32, 32)
    d = co.draw(SEED, 0, 4, len(entries), 32, 32, entries, ONE)
    assert d["cut"] and 0 < d["area"] < 1024   # this seed's first box is a real one
    box = (d["y0"], d["y1"], d["x0"], d["x1"])
    st = be.mix_state()
    assert st == {"mode": "cutmix", "lam": float(d["lam"]), "shift": d["shift"], "box": box}
    assert be.mixup_state() == (float(d["lam"]), d["shift"])
    m = be.metrics(top5=True)
    assert (m["mixup_lam"], m["mix_mode"], m["cutmix_area"]) == (float(d["lam"]), 1, d["area"])
    # the batch fed to the model is the host paste of the unmixed batch, bit for bit
    want = co.paste(x.numpy(), d["shift"], box)
    assert np.array_equal(be.last_input.numpy(), want)
    assert not np.array_equal(want, x.numpy())
    # the loss is the two-label loss at the area-adjusted lam
    yb = y.numpy()[(np.arange(4) + d["shift"]) % 4]
    logits = be.last_logits.numpy()
    rows, _, grad = mo.mixed_xent(logits, y.numpy(), yb, float(d["lam"]), eps)
    np.testing.assert_allclose(m["cross_entropy"], rows.mean(), rtol=1e-4, atol=1e-6)
    s = be.store.slot("dense/bias")
    db = be.store.master.grad[s.offset:s.offset + s.numel].numpy()
    np.testing.assert_allclose(db, (grad / 4).sum(axis=0), rtol=1e-4, atol=1e-6)
    yd = mo.dominant(y.numpy(), yb, float(d["lam"]))
    assert m["precision"] == float((logits.argmax(axis=1) == yd).mean())
    # the logits are those of the pasted input: a second trainer fed the paste, unmixed
    plain = _trainer(label_smoothing=eps)
    plain.set_batch(torch.from_numpy(want), y)
    plain.step()
    assert torch.equal(plain.last_logits, be.last_logits)


def test_cpu_trainer_switches_between_the_modes():
    be = _trainer(cutmix_alpha=1.0, mixup_alpha=0.4, mix_switch_prob=0.5, data_seed=SEED)
    assert be.cut_thresh == 2 ** 23
    entries, lams = cifar.cutmix_table(1.0, SEED, 32, 32), cifar.mixup_table(0.4, SEED)
    modes = set()
    for step in range(6):
        x, y = _batch(10 + step)
        be.set_batch(x, y)
        be.step()
        d = co.draw(SEED, step, 4, 4096, 32, 32, entries, 2 ** 23)
        st, m = be.mix_state(), be.metrics()
        modes.add(st["mode"])
        if d["cut"]:
            assert st == {"mode": "cutmix", "lam": float(d["lam"]), "shift": d["shift"],
                          "box": (d["y0"], d["y1"], d["x0"], d["x1"])}
            assert m["mix_mode"] == 1 and m["cutmix_area"] == d["area"]
            assert np.array_equal(be.last_input.numpy(),
                                  co.paste(x.numpy(), d["shift"], st["box"]))
        else:
            lam = float(lams[d["index"]])
            assert st == {"mode": "mixup", "lam": lam, "shift": d["shift"], "box": None}
            assert m["mix_mode"] == 0 and "cutmix_area" not in m and m["mixup_lam"] == lam
    assert modes == {"mixup", "cutmix"}   # asserted: these six steps of this seed have both


def test_cpu_trainer_zero_alpha_is_the_default():
    x, y = _batch(6)
    for kw in ({}, {"mixup_alpha": 0.4, "data_seed": SEED}):
        a, b = _trainer(**kw), _trainer(cutmix_alpha=0.0, mix_switch_prob=0.5, **kw)
        for be in (a, b):
            be.set_batch(x, y)
            be.step()
        assert torch.equal(a.store.master, b.store.master)
        assert torch.equal(a.mom, b.mom)
        assert a.metrics(top5=True) == b.metrics(top5=True)
        assert a.mix_state() == b.mix_state()
    assert "mix_mode" not in _trainer().metrics()
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _trainer(cutmix_alpha=bad)
    with pytest.raises(ValueError):
        _trainer(cutmix_alpha=1.0, mixup_alpha=0.2, mix_switch_prob=1.5)
