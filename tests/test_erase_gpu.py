"""Random Erasing on the device: the eager launch (_C.erase_boxes, csrc/erase.hip) against the
numpy oracle of tests/erase_oracle.py on whole buffers, in both device layouts, and the engine's
plans (per-layer, persistent): the erased input, the composition with mixup, graph replay, the
flag-off plan, determinism and the schedule-perturbation race check.

The cases are chosen by evaluating the oracle on the host, and the choice is asserted."""
import functools

import numpy as np
import pytest
import torch
import erase_oracle as eo

import distributed_tensorflow_resnet_amd as dtr
from distributed_tensorflow_resnet_amd.data import cifar
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule
from distributed_tensorflow_resnet_amd.utils.racecheck import perturbation_check

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SEED = 4321
ONE, HALF = 2 ** 24, 2 ** 23
BIG_STEP = 2 ** 32 + 3
DEFAULTS = (0.02, 1.0 / 3.0, 0.3)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _prefill(N, H, W, s2d):
    """Random bf16 values in the 3 image channels, zero padding channels (host, shared)."""
    g = torch.Generator().manual_seed(11 + H + s2d)
    if s2d:
        x = torch.randn((N, H // 2, W // 2, 4, 4), generator=g)
        x[..., 3] = 0
        return x.reshape(N, H // 2, W // 2, 16).to(BF)
    x = torch.randn((N, H, W, 8), generator=g)
    x[..., 3:] = 0
    return x.to(BF)


@functools.lru_cache(maxsize=None)
def _noise():
    return cifar.erase_noise_table(SEED)


def _launch(gpu, x0, H, W, s2d, step, table, thresh, noise=None, log=True):
    """One eager erase_boxes launch on a copy of x0 -> (buffer bits, log [N, 5] or None)."""
    nat, N = dtr.native(required=True), x0.shape[0]
    x = x0.to(gpu).clone()
    tab = torch.tensor(list(table), dtype=torch.int32, device=gpu)
    nz = torch.from_numpy(noise).to(gpu) if noise is not None else None
    lg = torch.full((N, 5), -7, dtype=torch.int32, device=gpu) if log else None
    gstep = torch.tensor([step], dtype=torch.int64, device=gpu)
    nat.erase_boxes(x.data_ptr(), N, H, W, 8, int(s2d), SEED, gstep.data_ptr(), tab.data_ptr(),
                    tab.numel(), thresh, nz.data_ptr() if nz is not None else 0,
                    nz.numel() if nz is not None else 0, lg.data_ptr() if log else 0, _st())
    torch.cuda.synchronize()
    return _bits(x), (lg.cpu().numpy() if log else None)


# ---------------------------------------------------------------- 5. CIFAR layout
@pytest.mark.parametrize("fill", ["zero", "noise"])
def test_cifar_layout_equals_the_oracle(gpu, fill):
    N, H, W = 5, 32, 32
    x0 = _prefill(N, H, W, 0)
    table = cifar.erase_table(SEED, H, W, *DEFAULTS)
    noise = _noise() if fill == "noise" else None
    seen = set()
    for thresh in (HALF, ONE):
        for step in (0, 1, BIG_STEP):
            got, log = _launch(gpu, x0, H, W, 0, step, table, thresh, noise)
            want = eo.erase(_bits(x0), SEED, step, table, H, W, thresh, noise)
            st = eo.state(SEED, step, N, table, H, W, thresh)
            assert np.array_equal(log, st), (thresh, step)
            assert np.array_equal(got, want), (thresh, step)
            assert not got.reshape(N, H, W, 8)[..., 3:].any()   # padding channels stay 0
            seen |= {(thresh, bool(on)) for on in st[:, 0]}
            if thresh == ONE:
                assert st[:, 0].all() and not np.array_equal(got, _bits(x0))
    assert (HALF, True) in seen and (HALF, False) in seen   # the threshold decides per image
    # without a log pointer the launch writes the same buffer
    got, _ = _launch(gpu, x0, H, W, 0, 1, table, ONE, noise, log=False)
    assert np.array_equal(got, eo.erase(_bits(x0), SEED, 1, table, H, W, ONE, noise))


@pytest.mark.parametrize("fill", ["zero", "noise"])
def test_cifar_box_touching_the_borders(gpu, fill):
    """A hand-made table whose only entry is (H-1, W-1): y0, x0 in {0, 1}, so the box touches
    the first or the last row and column; and entry 0, which erases nothing."""
    N, H, W = 5, 32, 32
    x0 = _prefill(N, H, W, 0)
    table = [eo.entry(H - 1, W - 1)]
    noise = _noise() if fill == "noise" else None
    corners = set()
    for step in (0, 1, BIG_STEP):
        got, log = _launch(gpu, x0, H, W, 0, step, table, ONE, noise)
        st = eo.state(SEED, step, N, table, H, W, ONE)
        assert np.array_equal(log, st)
        assert np.array_equal(got, eo.erase(_bits(x0), SEED, step, table, H, W, ONE, noise))
        corners |= {(int(r[1]), int(r[2])) for r in st}
    assert {y for y, _ in corners} == {0, 1} and {x for _, x in corners} == {0, 1}
    got, log = _launch(gpu, x0, H, W, 0, 0, [0], ONE, noise)
    assert np.array_equal(got, _bits(x0)) and not log.any()
    got, log = _launch(gpu, x0, H, W, 0, 0, table, 0, noise)    # threshold 0: never
    assert np.array_equal(got, _bits(x0)) and not log.any()
    # an entry that does not fit the image counts as off: nothing is written
    got, log = _launch(gpu, x0, H, W, 0, 0, [eo.entry(H + 1, 4)], ONE, noise)
    assert np.array_equal(got, _bits(x0)) and not log.any()


def test_refusals(gpu):
    nat = dtr.native(required=True)
    x = torch.zeros((2, 32, 32, 8), dtype=BF, device=gpu)
    tab = torch.tensor([eo.entry(3, 3)], dtype=torch.int32, device=gpu)
    ok = [x.data_ptr(), 2, 32, 32, 8, 0, SEED, 0, tab.data_ptr(), 1, ONE, 0, 0, 0]
    nat.erase_boxes(*ok, _st())
    for i, bad in ((0, 0), (0, x.data_ptr() + 8), (1, 0), (2, 1), (3, 1 << 15), (4, 4), (8, 0),
                   (9, 0), (10, -1), (10, ONE + 1)):
        args = list(ok)
        args[i] = bad
        with pytest.raises(ValueError):
            nat.erase_boxes(*args, _st())
    with pytest.raises(ValueError):   # s2d needs even H, W
        nat.erase_boxes(x.data_ptr(), 2, 31, 32, 8, 1, SEED, 0, tab.data_ptr(), 1, ONE, 0, 0, 0,
                        _st())
    with pytest.raises(ValueError):   # a noise table without values
        nat.erase_boxes(*ok[:11], tab.data_ptr(), 0, 0, _st())
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. ImageNet layouts
@functools.lru_cache(maxsize=None)
def _imagenet_steps():
    """Steps whose boxes (N = 3, 224 x 224, default table) have, between them, an odd y0, an
    odd x0, an odd eh and an odd ew, and an even one of each: found on the host."""
    N, H, W = 3, 224, 224
    table = cifar.erase_table(SEED, H, W, *DEFAULTS)
    need = {(k, p) for k in (1, 2, 3, 4) for p in (0, 1)}   # (column of the state, parity)
    steps = []
    for step in list(range(16)) + [BIG_STEP]:
        st = eo.state(SEED, step, N, table, H, W, ONE)
        new = {(k, int(r[k]) & 1) for r in st if r[0] for k in (1, 2, 3, 4)} & need
        if new:
            steps.append(step)
            need -= new
        if not need:
            break
    return tuple(steps), tuple(sorted(need))


@pytest.mark.parametrize("s2d", [0, 1])
def test_imagenet_layouts_equal_the_oracle(gpu, s2d):
    N, H, W = 3, 224, 224
    steps, missing = _imagenet_steps()
    assert not missing and len(steps) <= 6   # the condition: every phase of y0, x0, eh, ew
    x0 = _prefill(N, H, W, s2d)
    table = cifar.erase_table(SEED, H, W, *DEFAULTS)
    parities = set()
    for step in steps:
        got, log = _launch(gpu, x0, H, W, s2d, step, table, ONE)
        st = eo.state(SEED, step, N, table, H, W, ONE)
        assert np.array_equal(log, st), step
        want = eo.erase(_bits(x0), SEED, step, table, H, W, ONE, None, bool(s2d))
        assert np.array_equal(got, want), step
        parities |= {(k, int(r[k]) & 1) for r in st if r[0] for k in (1, 2, 3, 4)}
        # from the box alone: outside it every element is the prefill's, padding included,
        # inside it the pixel's 4 (or 8) channels are 0 -- so the other three pixels of a
        # touched 16-channel row are unchanged
        before = _bits(x0)
        if s2d:
            view = lambda b: b.reshape(N, H // 2, W // 2, 2, 2, 4).transpose(0, 1, 3, 2, 4, 5) \
                .reshape(N, H, W, 4)   # noqa: E731
            got, before = view(got), view(before)
        mask = eo.box_mask(st, H, W)
        assert np.array_equal(got[~mask], before[~mask]), step
        assert not got[mask].any() and before[mask][:, :3].any(), step
        assert not got[..., 3:].any(), step
    assert {(k, 1) for k in (1, 2, 3, 4)} <= parities   # odd y0, x0, eh and ew among the cases


# ---------------------------------------------------------------- engine
N_ENG = 4
PLANS = {"per_layer": "persist=0", "persistent": "persist=1"}


@functools.lru_cache(maxsize=None)
def _records(n, seed=7):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (n, 3, 32, 32), generator=g, dtype=torch.uint8),
            torch.randint(0, 10, (n,), generator=g, dtype=torch.int32))


def _engine(monkeypatch, gpu, tune, **kw):
    monkeypatch.setenv("DTR_TUNE", tune)
    kw.setdefault("use_graph", False)
    eng = Engine(cifar_spec(8), N_ENG, weight_decay=2e-4, lr_schedule=cifar_lr_schedule(),
                 device=gpu, input_mode="cifar_u8", data_seed=SEED, seed=3, **kw)
    eng.set_batch(*_records(N_ENG))
    if tune:
        assert eng.persist == (tune == "persist=1")
    return eng


def _state(eng):
    torch.cuda.synchronize()
    assert not eng.persist_error()
    return {"master": eng.params.master.clone(), "mom": eng.mom.clone(),
            "stats": eng.params.stats.clone(), "gstep": eng.gstep.clone()}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def _table():
    return cifar.erase_table(SEED, 32, 32, *DEFAULTS)


def _spec_state(step):
    t = _table()
    rows = []
    for n in range(N_ENG):
        d = cifar.erase_draw(SEED, step, n, len(t), 32, 32, t, ONE)
        rows.append([int(d["on"]), d["y0"], d["x0"], d["eh"], d["ew"]])
    return np.array(rows)


# ---------------------------------------------------------------- 7. engine step
@pytest.mark.parametrize("mixup", [0.0, 0.4])
@pytest.mark.parametrize("fill", ["zero", "noise"])
@pytest.mark.parametrize("plan", list(PLANS))
def test_engine_step_erases_the_input(gpu, monkeypatch, plan, fill, mixup):
    eng = _engine(monkeypatch, gpu, PLANS[plan], erase_prob=1.0, erase_fill=fill,
                  mixup_alpha=mixup)
    off = _engine(monkeypatch, gpu, PLANS[plan], mixup_alpha=mixup)
    assert eng.erase_state() is None and off.erase_state() is None
    assert off.erase_tab is None and off.erase_log is None and off.erase_noise is None
    noise = _noise() if fill == "noise" else None
    assert (eng.erase_noise is None) == (noise is None) and eng.erase_thresh == ONE
    for step in range(2):
        eng.step()
        off.step()
        torch.cuda.synchronize()
        assert not eng.persist_error() and not off.persist_error()
        want = eo.erase(_bits(off.x_in), SEED, step, _table(), 32, 32, ONE, noise)
        assert np.array_equal(_bits(eng.x_in), want), step
        assert not np.array_equal(want, _bits(off.x_in))
        st = eng.erase_state()
        assert np.array_equal(st, _spec_state(step)) and st[:, 0].all()
        assert np.array_equal(st, eo.state(SEED, step, N_ENG, _table(), 32, 32, ONE))
        m = eng.metrics(reduce=False)
        assert m["erase_count"] == N_ENG
        assert m["erase_area"] == float((st[:, 3] * st[:, 4]).sum() / (N_ENG * 1024))
        assert "erase_count" not in off.metrics(reduce=False)
        if mixup:   # labels and lam are untouched
            assert eng.mix_state() == off.mix_state()
            assert torch.equal(eng.labels_b, off.labels_b)
    assert "erase_boxes" in eng.plan.names() and "erase_boxes" not in off.plan.names()
    assert not _same(_state(eng), _state(off))   # erasing is visible in the weights


def test_engine_step_on_the_persistent_overlap_plan(gpu, monkeypatch):
    """comm = the doubling loopback: the plan that declares op buffers.  The erase launch sits
    on the main stream behind the input launch, declares the input buffer, and the stream check
    passes at build."""
    monkeypatch.setenv("DTR_TUNE", "persist=1")

    def mk(**kw):
        eng = Engine(cifar_spec(8), 16, weight_decay=2e-4, lr_schedule=cifar_lr_schedule(),
                     device=gpu, input_mode="cifar_u8", data_seed=SEED, seed=3, use_graph=False,
                     bucket_mb=0.05, comm=dtr.native().Comm.loopback(2.0), **kw)
        eng.set_batch(*_records(16))
        return eng
    eng, off = mk(erase_prob=1.0), mk()
    assert eng.persist and eng.persist_overlap and off.persist_overlap
    names = eng.plan.names()
    i = names.index("erase_boxes")
    assert names.count("erase_boxes") == 1 and names[i - 1] == "cifar_augment"
    assert eng.plan.op_streams()[i] == 0 and eng.recorded.op_buffers[i] == {"input"}
    assert [n for n in names if n != "erase_boxes"] == off.plan.names()
    for step in range(2):
        eng.step()
        off.step()
        torch.cuda.synchronize()
        assert not eng.persist_error()
        want = eo.erase(_bits(off.x_in), SEED, step, _table(), 32, 32, ONE)
        assert np.array_equal(_bits(eng.x_in), want), step
        assert np.array_equal(eng.erase_state(), eo.state(SEED, step, 16, _table(), 32, 32, ONE))


# ---------------------------------------------------------------- 8. graph replay
@pytest.mark.parametrize("plan", list(PLANS))
def test_graph_replay_draws_fresh_boxes(gpu, monkeypatch, plan):
    eng = _engine(monkeypatch, gpu, PLANS[plan], erase_prob=1.0, use_graph=True)
    off = _engine(monkeypatch, gpu, PLANS[plan])
    done = eng.capture(warmup=2)
    for _ in range(done):
        off.step()
    states = []
    for step in range(done, done + 3):
        eng.step()
        off.step()
        torch.cuda.synchronize()
        st = eng.erase_state()
        assert np.array_equal(st, _spec_state(step)), step
        want = eo.erase(_bits(off.x_in), SEED, step, _table(), 32, 32, ONE)
        # (off's weights differ by now, its input buffer does not depend on them)
        assert np.array_equal(_bits(eng.x_in), want), step
        states.append(st.tolist())
    assert eng.graph is not None
    assert states[0] != states[1] != states[2] != states[0]   # the boxes differ between steps
    eager = _engine(monkeypatch, gpu, PLANS[plan], erase_prob=1.0)
    for _ in range(done + 3):
        eager.step()
    assert _same(_state(eng), _state(eager))


# ---------------------------------------------------------------- 9. flag off
@pytest.mark.parametrize("plan", list(PLANS))
def test_zero_prob_is_bitwise_the_default(gpu, monkeypatch, plan):
    plain = _engine(monkeypatch, gpu, PLANS[plan])
    zero = _engine(monkeypatch, gpu, PLANS[plan], erase_prob=0.0, erase_area_min=0.1,
                   erase_area_max=0.2, erase_aspect_min=0.5, erase_fill="noise")
    assert zero.erase_tab is None and zero.erase_noise is None and zero.erase_log is None
    assert zero.erase_thresh == 0
    assert zero.plan.size() == plain.plan.size() and zero.plan.names() == plain.plan.names()
    assert "erase_boxes" not in zero.plan.names()
    on = _engine(monkeypatch, gpu, PLANS[plan], erase_prob=0.5)
    assert on.plan.size() == plain.plan.size() + 1
    assert [n for n in on.plan.names() if n != "erase_boxes"] == plain.plan.names()
    i = on.plan.names().index("erase_boxes")   # directly behind the input launch
    assert on.plan.names()[i - 1] == "cifar_augment" and on.plan.op_streams()[i] == 0
    for _ in range(3):
        plain.step()
        zero.step()
    assert _same(_state(plain), _state(zero))
    assert zero.erase_state() is None and "erase_count" not in zero.metrics(reduce=False)


def test_input_modes_without_an_input_launch_refuse_erasing(gpu, monkeypatch):
    monkeypatch.setenv("DTR_TUNE", "")
    kw = dict(weight_decay=2e-4, lr_schedule=cifar_lr_schedule(), device=gpu, data_seed=SEED)
    with pytest.raises(ValueError, match="input launch"):
        Engine(cifar_spec(8), N_ENG, input_mode="nhwc", erase_prob=0.5, **kw)
    Engine(cifar_spec(8), N_ENG, input_mode="nhwc", erase_prob=0.0, **kw)
    for bad in ({"erase_prob": 1.5}, {"erase_prob": 0.5, "erase_area_min": 0.0},
                {"erase_prob": 0.5, "erase_area_min": 0.5, "erase_area_max": 0.4},
                {"erase_prob": 0.5, "erase_aspect_min": 0.0}, {"erase_prob": 0.5, "erase_fill": "x"}):
        with pytest.raises(ValueError):
            Engine(cifar_spec(8), N_ENG, input_mode="cifar_u8", **bad, **kw)
    # the eval plans never erase: built on an erasing engine, they score a batch as one without
    eng = _engine(monkeypatch, gpu, "", erase_prob=1.0)
    plain = _engine(monkeypatch, gpu, "")
    x, y = _records(N_ENG)
    a = eng.build_eval_plan(N_ENG).run(x, y)
    b = plain.build_eval_plan(N_ENG).run(x, y)
    assert a[0] == b[0] and a[1] == b[1]


# ---------------------------------------------------------------- 10. determinism, races
@pytest.mark.parametrize("plan", list(PLANS))
def test_two_engines_are_bitwise_equal(gpu, monkeypatch, plan):
    a = _engine(monkeypatch, gpu, PLANS[plan], erase_prob=0.5, erase_fill="noise")
    b = _engine(monkeypatch, gpu, PLANS[plan], erase_prob=0.5, erase_fill="noise")
    for _ in range(3):
        a.step()
        b.step()
    assert _same(_state(a), _state(b))
    assert torch.equal(a.x_in.view(torch.int16), b.x_in.view(torch.int16))
    assert np.array_equal(a.erase_state(), b.erase_state())


def test_erasing_step_is_schedule_independent(gpu, monkeypatch):
    monkeypatch.setenv("DTR_TUNE", "")

    def make():
        eng = Engine(cifar_spec(8), N_ENG, weight_decay=2e-4, lr_schedule=cifar_lr_schedule(),
                     device=gpu, input_mode="cifar_u8", data_seed=SEED, seed=3, use_graph=False,
                     erase_prob=1.0, erase_fill="noise")
        eng.set_batch(*_records(N_ENG))
        assert "erase_boxes" in eng.plan.names()
        return eng
    res = perturbation_check(make, steps=3, trials=1, prob=0.5, max_us=20.0)
    print(res)
    assert res["ok"], res["mismatches"]
