"""Muon's host side: flags, tables, the CPU backend's update and its checkpoint entries."""
import numpy as np
import pytest
import torch

from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.train.backends import CPUBackend
from distributed_tensorflow_resnet_amd.train.layout import (OPT_FUSED_MUON_REASON, OPTIMIZERS,
                                                              muon_tables)
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr
from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver
from distributed_tensorflow_resnet_amd.utils.flags import build_parser


def test_muon_flags():
    f = build_parser("cifar").parse_args(["--optimizer", "muon"])
    assert (f.muon_momentum, f.muon_nesterov, f.muon_ns_steps, f.muon_aux_lr_scale) == \
        (0.95, True, 5, 1.0)
    f = build_parser("cifar").parse_args(["--optimizer", "muon", "--muon_nesterov=false",
                                          "--muon_ns_steps", "8", "--muon_momentum", "0"])
    assert (f.muon_nesterov, f.muon_ns_steps, f.muon_momentum) == (False, 8, 0.0)
    for bad in (["--muon_ns_steps", "0"], ["--muon_ns_steps", "9"], ["--muon_momentum", "1"],
                ["--muon_aux_lr_scale", "0"], ["--optimizer", "muon", "--clip_grad_norm", "1"]):
        with pytest.raises(SystemExit):
            build_parser("cifar").parse_args(bad)
    assert "muon" in OPTIMIZERS and "muon" in OPT_FUSED_MUON_REASON


def _backend(optimizer, seed=0, **kw):
    return CPUBackend(cifar_spec(8), 4, weight_decay=1e-3, lr_schedule=constant_lr(1e-2),
                      optimizer=optimizer, seed=seed, **kw)


def test_muon_tables_of_cifar8_and_the_imagenet_refusal():
    be = _backend("muon")
    tab, seg, q = muon_tables(be.store.train_slots)
    slots = be.store.train_slots
    assert [bool(x) for x in seg] == [s.kind == "conv" for s in slots] and len(tab) == int(seg.sum())
    by_shape = {(int(r["R"]), int(r["K"])): r for r in tab}
    assert (27, 16) in by_shape and (16, 32) in by_shape
    for (R, K), r in by_shape.items():
        s = slots[int(r["seg"])]
        assert int(r["offset"]) == s.offset and R * K == s.numel and K == s.shape[-1]
        assert int(r["transpose"]) == int(K <= R)
    assert q[int(by_shape[(27, 16)]["seg"])] == 1.0
    assert q[int(by_shape[(16, 32)]["seg"])] == np.sqrt(np.float32(2.0))
    with pytest.raises(ValueError, match="576"):
        CPUBackend(imagenet_spec(18, image_hw=64), 2, weight_decay=1e-3,
                   lr_schedule=constant_lr(1e-2), optimizer="muon")
    with pytest.raises(ValueError, match="clip_grad_norm"):
        _backend("muon", clip_grad_norm=1.0)


def _steps(be, n):
    gen = torch.Generator().manual_seed(3)
    x, y = torch.randn(4, 32, 32, 3, generator=gen), torch.randint(0, 10, (4,), generator=gen)
    for _ in range(n):
        be.set_batch(x, y)
        be.step()


def test_cpu_backend_muon_steps_and_checkpoint_round_trip(tmp_path):
    be, mom = _backend("muon"), _backend("mom")
    _steps(be, 3)
    _steps(mom, 3)
    assert bool(torch.isfinite(be.store.master).all()) and bool(torch.isfinite(be.mom).all())
    assert not torch.equal(be.store.master, mom.store.master)
    assert be.metrics()["optimizer"] == "muon"
    t = be.state_tensors()
    s = be.store.train_slots[0]
    assert np.array_equal(t[s.name + "/Momentum"].reshape(-1),
                          be.mom[s.offset:s.offset + s.numel].numpy())
    second = _backend("muon", seed=9)
    second.load_state(Saver.restore(Saver(str(tmp_path)).save(t, 3)))
    assert second.global_step == 3 and torch.equal(second.mom, be.mom)
    assert torch.equal(second.store.master, be.store.master)
