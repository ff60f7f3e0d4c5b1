"""Tiled Muon's host side: the flag, the split of the tables, the work tables, the CPU backend."""
import numpy as np
import torch

from distributed_tensorflow_resnet_amd.models.spec import imagenet_spec
from distributed_tensorflow_resnet_amd.train.backends import CPUBackend
from distributed_tensorflow_resnet_amd.train.layout import (muon_apply_bn, muon_covers,
                                                              muon_tables, muon_tiled_covers)
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr
from distributed_tensorflow_resnet_amd.utils.flags import build_parser


def test_muon_tiled_flag_and_cover():
    assert build_parser("imagenet").parse_args([]).muon_tiled is False
    assert build_parser("imagenet").parse_args(["--optimizer", "muon", "--muon_tiled"]).muon_tiled
    assert build_parser("cifar").parse_args(["--muon_tiled=true"]).muon_tiled   # unused with mom
    assert muon_tiled_covers(4608, 512) and muon_tiled_covers(1024, 2048)
    assert not muon_tiled_covers(1025, 1025) and not muon_tiled_covers(64, 8193)


def _backend():
    return CPUBackend(imagenet_spec(18, image_hw=64), 2, weight_decay=1e-3,
                      lr_schedule=constant_lr(1e-2), optimizer="muon", muon_tiled=True)


def test_muon_tiled_tables_of_resnet18():
    slots = _backend().store.train_slots
    small, seg, q, tt = muon_tables(slots, tiled=True)
    tab = tt["tab"]
    convs = [s for s in slots if s.kind == "conv"]
    shape = lambda s: (s.numel // s.shape[-1], s.shape[-1])   # noqa: E731
    assert [slots[i].name for i in small["seg"]] == [s.name for s in convs if muon_covers(*shape(s))]
    assert [slots[i].name for i in tab["seg"]] == [s.name for s in convs if not muon_covers(*shape(s))]
    assert (1152, 128) in {(int(r["R"]), int(r["K"])) for r in tab} and int(seg.sum()) == len(convs)
    end = 0
    for t, r in enumerate(tab):
        R, K, SP, LP = (int(r[k]) for k in ("R", "K", "SP", "LP"))
        assert q[int(r["seg"])] == np.sqrt(np.float32(max(1.0, K / R)))
        assert (SP, LP) == (-(-min(R, K) // 64) * 64, -(-max(R, K) // 64) * 64)
        assert (int(r["x_off"]), int(r["a_off"]), int(r["b_off"])) == \
            (end, end + SP * LP, end + SP * LP + SP * SP)          # disjoint, back to back
        end += SP * LP + 2 * SP * SP
        tri = sorted((i, j) for i in range(SP // 64) for j in range(i, SP // 64))
        for name, red in (("syrk_a", LP), ("syrk_b", SP)):
            mine = [w for w in tt[name] if w["t"] == t]
            assert sorted((int(w["i"]), int(w["j"])) for w in mine) == tri
            assert all(int(w["len"]) == red for w in mine)
        bn = muon_apply_bn(SP)
        assert sorted((int(w["i"]), int(w["j"])) for w in tt["apply"] if w["t"] == t) == \
            [(i, bn) for i in range(LP // bn)]
        assert sorted((int(w["i"]), int(w["j"])) for w in tt["stage"] if w["t"] == t) == \
            [(i, j) for i in range(SP // 64) for j in range(LP // 64)]
        assert list(tt["blk"]).count(t) == int(r["nchunks"]) == -(-R * K // 4096)
        assert int(tt["blk"][int(r["chunk0"])]) == t
    assert end == tt["scratch"] and tt["max_sp"] == int(tab["SP"].max())
    for name in ("syrk_a", "syrk_b", "apply"):   # the longest reduction first
        assert list(tt[name]["len"]) == sorted(tt[name]["len"], reverse=True)


def test_cpu_backend_takes_a_tiled_muon_step():
    be = _backend()
    w0 = be.store.master.clone()
    gen = torch.Generator().manual_seed(3)
    be.set_batch(torch.randn(2, 64, 64, 3, generator=gen), torch.randint(0, 1000, (2,), generator=gen))
    be.step()
    assert bool(torch.isfinite(be.store.master).all()) and not torch.equal(be.store.master, w0)
