"""Shampoo's host side: flags, the block table, the oracle's iteration, the CPU backend's update
and its checkpoint entries."""
import numpy as np
import pytest
import torch

import shampoo_oracle as so
from test_muon_cpu import _backend, _steps
from distributed_tensorflow_resnet_amd.train.layout import (OPT_FUSED_SHAMPOO_REASON, OPTIMIZERS,
                                                              shampoo_tables)
from distributed_tensorflow_resnet_amd.utils.checkpoint import Saver
from distributed_tensorflow_resnet_amd.utils.flags import build_parser


def test_shampoo_flags():
    f = build_parser("cifar").parse_args(["--optimizer", "shampoo"])
    assert (f.shampoo_beta2, f.shampoo_epsilon, f.shampoo_precond_every) == (1.0, 1e-6, 10)
    f = build_parser("cifar").parse_args(["--shampoo_beta2", "0.9"])   # unused with mom: accepted
    assert f.optimizer == "mom" and f.shampoo_beta2 == 0.9
    for bad in (["--shampoo_beta2", "0"], ["--shampoo_beta2", "1.5"], ["--shampoo_epsilon", "0"],
                ["--shampoo_epsilon", "inf"], ["--shampoo_precond_every", "0"],
                ["--optimizer", "shampoo", "--clip_grad_norm", "1"],
                ["--optimizer", "shampoo", "--adam_trust", "on"]):
        with pytest.raises(SystemExit):
            build_parser("cifar").parse_args(bad)
    assert OPTIMIZERS[5:] == ("muon", "shampoo", "rmsprop") and "shampoo" in OPT_FUSED_SHAMPOO_REASON


def test_block_table_of_cifar8():
    slots = _backend("mom").store.train_slots
    blocks, tens, seg, names = shampoo_tables(slots)
    assert [bool(x) for x in seg] == [s.kind == "conv" for s in slots]
    assert names == [s.name for s in slots if s.kind == "conv"] and len(tens) == len(names)
    assert [int(s) for s in blocks["slot"]] == list(range(len(blocks)))
    for t in tens:
        s = slots[int(t["seg"])]
        K = s.shape[-1]
        R = s.numel // K
        mine = blocks[int(t["block0"]):int(t["block0"]) + int(t["nblocks"])]
        assert len(mine) == -(-R // 64) * -(-K // 64) and set(mine["seg"]) == {int(t["seg"])}
        want = [(s.offset + i * K + j, K, r, k) for i, j, r, k in so.blocks(R, K)]
        assert [tuple(int(b[f]) for f in ("offset", "K", "r", "k")) for b in mine] == want
        assert sum(int(b["r"]) * int(b["k"]) for b in mine) == s.numel
    stem = blocks[0]   # the 3 x 3 x 3 x 16 stem: one ragged block
    assert (int(stem["r"]), int(stem["k"]), int(tens[0]["nblocks"])) == (27, 16, 1)
    assert {(int(b["r"]), int(b["k"])) for b in blocks} >= {(64, 16), (16, 16), (64, 64)}


@pytest.mark.parametrize("n", (16, 27, 64))
def test_oracle_iteration_against_eigh(n):
    rng = np.random.default_rng(n)
    g = rng.standard_normal((n, max(4, n // 4)))
    A = g @ g.T                                   # rank deficient: the first refresh's input
    X, steps, res = so.root_iter(A, 1e-4)
    # X = D^(-1/4) Mk^(1/4) throughout, so X is off by about |Mk - I|_2 / 4 <= n max|Mk - I| / 4
    assert res < 1e-5 and steps <= 16
    assert so.rel(X, so.root_exact(A, 1e-4)) <= n * res / 4 + 1e-12
    X32, _, res32 = so.root_iter(A.astype(np.float32), 1e-4, np.float32)
    assert res32 < 1e-2 and so.rel(X32, so.root_exact(A.astype(np.float32), 1e-4)) < 1e-3


def test_cpu_backend_is_mom_until_the_first_refresh_then_round_trips(tmp_path):
    be, mom = _backend("shampoo", shampoo_precond_every=3), _backend("mom")
    _steps(be, 2)
    _steps(mom, 2)
    assert torch.equal(be.store.master, mom.store.master) and torch.equal(be.mom, mom.mom)
    _steps(be, 1)
    _steps(mom, 1)
    st = be.shampoo_state()
    assert st["t"] == 3 and st["failed"] == 0 and st["state_bytes"] == 4 * st["L"].numel() * 4
    assert bool(torch.isfinite(be.store.master).all()) and float(st["L"].abs().max()) > 0
    for s in be.store.train_slots:   # conv kernels moved differently, every other tensor as mom's
        sl = slice(s.offset, s.offset + s.numel)
        assert torch.equal(be.store.master[sl], mom.store.master[sl]) == (s.kind != "conv"), s.name
    m = be.metrics()
    assert m["optimizer"] == "shampoo" and 0 < m["shampoo_graft_min"] <= m["shampoo_graft_max"]
    t = be.state_tensors()
    name, nb = be.shampoo_names[-1], int(be.shampoo_tensors[-1]["nblocks"])
    assert nb > 1 and t[name + "/shampoo_PL"].shape == (nb, 64, 64)
    assert t["shampoo_start_step"].dtype == np.int64 and int(t["shampoo_start_step"]) == 0
    assert name + "/Momentum" in t
    second = _backend("shampoo", seed=9, shampoo_precond_every=3)
    second.load_state(Saver.restore(Saver(str(tmp_path)).save(t, 3)))
    for k in ("L", "R", "PL", "PR"):
        assert torch.equal(second.shampoo_state()[k], st[k]), k
    assert second.global_step == 3 and torch.equal(second.mom, be.mom)
    _steps(be, 1)
    _steps(second, 1)
    assert torch.equal(second.store.master, be.store.master)   # resume is bitwise
    assert "shampoo_start_step" not in mom.state_tensors()


def test_a_checkpoint_without_the_slots_restarts_the_state(tmp_path, capsys):
    mom = _backend("mom")
    _steps(mom, 2)
    be = _backend("shampoo", shampoo_precond_every=2)
    _steps(be, 2)
    be.load_state(Saver.restore(Saver(str(tmp_path)).save(mom.state_tensors(), 2)))
    assert capsys.readouterr().out.count("no shampoo slots") == 1
    st = be.shampoo_state()
    assert be.shampoo_start == 2 and float(st["L"].abs().max()) == 0
    assert torch.equal(st["PL"][0, :27, :27], torch.eye(27)) and float(st["PL"][0].sum()) == 27
    assert torch.equal(be.mom, mom.mom)
