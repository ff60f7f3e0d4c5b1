"""The parameter-segment table (train/layout.py param_segments) and LRSchedule.launch_args:
pure host arithmetic, checked without a GPU or the native module."""
import pytest

from distributed_tensorflow_resnet_amd.models.params import ParamStore
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.train.layout import param_segments
from distributed_tensorflow_resnet_amd.train.schedule import LRSchedule, imagenet_lr_schedule

CPAD_IN = 8
CASES = {
    "cifar8": (lambda: cifar_spec(8), False),
    "imagenet18": (lambda: imagenet_spec(18, image_hw=64), False),
    "imagenet18-s2d": (lambda: imagenet_spec(18, image_hw=64), True),
}


@pytest.fixture(scope="module", params=list(CASES))
def table(request):
    make, s2d = CASES[request.param]
    spec = make()
    slots = ParamStore(spec, device="cpu").train_slots
    kpad = -(-spec.num_classes // 16) * 16
    seg, bf_total = param_segments(spec, slots, cpad_in=CPAD_IN, kpad=kpad, stem_s2d=s2d)
    assert len(seg) == len(slots)
    return spec, slots, seg, int(bf_total), kpad, s2d


def test_offsets_follow_the_slots(table):
    _, slots, seg, *_ = table
    assert [int(r["offset"]) for r in seg] == [s.offset for s in slots]
    assert [int(r["numel"]) for r in seg] == [s.numel for s in slots]


def test_bf16_copies_tile_the_buffer(table):
    _, _, seg, bf_total, _, _ = table
    ranges = []
    for r in seg:
        taps = int(r["kh"] * r["kw"])
        if r["bf_ohwi"] >= 0:
            ranges.append((int(r["bf_ohwi"]), int(r["bf_ohwi"]) + int(r["kpad"]) * taps * int(r["cpad"])))
        if r["bf_hwio"] >= 0:
            ranges.append((int(r["bf_hwio"]), int(r["bf_hwio"]) + taps * int(r["C"]) * int(r["kpad"])))
    ranges.sort()
    assert ranges and ranges[0][0] == 0 and ranges[-1][1] == bf_total
    # sorted, each range starts where the one before ends: disjoint and without a gap
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    assert all(lo < hi for lo, hi in ranges)


def test_convs(table):
    spec, slots, seg, _, _, s2d = table
    convs = {c.name: c for c in spec.all_convs()}
    seen = 0
    for r, s in zip(seg, slots):
        if s.kind != "conv":
            continue
        seen += 1
        c = convs[s.name.split("/")[0]]
        assert (r["kh"], r["kw"], r["C"], r["K"], r["kpad"]) == (c.kh, c.kw, c.cin, c.cout, c.cout)
        if c.cin < 8:
            assert r["bf_hwio"] == -1 and r["cpad"] == CPAD_IN
        else:
            assert r["bf_hwio"] >= 0 and r["cpad"] == c.cin
        is_stem = c.name == spec.stem.name
        assert (r["bf_ohwi"] == -1) == (is_stem and s2d)
    assert seen == len(convs) and spec.stem.cin < 8


def test_dense_kernel(table):
    spec, slots, seg, _, kpad, _ = table
    (r,) = [r for r, s in zip(seg, slots) if s.kind == "dense_kernel"]
    assert kpad % 16 == 0 and 0 <= kpad - spec.num_classes < 16
    assert (r["kh"], r["kw"], r["C"], r["K"]) == (1, 1, spec.dense_in, spec.num_classes)
    assert r["kpad"] == kpad and r["cpad"] == spec.dense_in
    assert r["bf_ohwi"] >= 0 and r["bf_hwio"] >= 0


def test_other_slots_have_no_copy(table):
    _, slots, seg, *_ = table
    others = [r for r, s in zip(seg, slots) if s.kind not in ("conv", "dense_kernel")]
    assert others
    for r in others:
        assert (r["kh"], r["kw"], r["C"], r["K"]) == (1, 1, 1, 1)
        assert r["bf_ohwi"] == -1 and r["bf_hwio"] == -1


def test_launch_args_round_trip():
    s = imagenet_lr_schedule()
    init, warm_steps, warm_from, warm_to, bounds, values = s.launch_args()
    assert LRSchedule(init, bounds, values, warm_steps, warm_from, warm_to) == s
    assert bounds is not s.bounds and values is not s.values   # copies: the plan keeps its own
