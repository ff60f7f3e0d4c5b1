"""SOAP's host side: flags, the oracle's fp32 run, the CPU backend against the oracle, the plan makers."""
import numpy as np
import pytest
import torch

import shampoo_oracle as so
import soap_oracle as sp
from test_bindings_cpu import ODD, P, PIECEWISE, SCHED
from test_muon_cpu import _backend, _steps
from distributed_tensorflow_resnet_amd.utils.flags import build_parser

SHAPES = [(64, 64), (27, 16), (64, 16), (48, 64)]   # full tiles; ragged; r > k; r < k
SIZES = (64, 27, 16, 48)                            # the sides of those blocks
SOAP = ["--optimizer", "shampoo", "--shampoo_variant", "soap"]
rand_orth = lambda rng, n: sp.qr_q(rng.standard_normal((n, n)))   # noqa: E731


def refresh_case(n, basis="random", rank=None):
    """(S, Q0): S SPD with the geometric spectrum 1 .. 1e-3, or G G^T of rank `rank`."""
    rng = np.random.default_rng(7 * n + (rank or 0))
    u = rng.standard_normal((n, rank)) if rank else rand_orth(rng, n) * np.logspace(0, -1.5, n)
    S, Q0 = u @ u.T, np.eye(n) if basis == "identity" else rand_orth(rng, n)
    return ((S + S.T) / 2).astype(np.float32), Q0.astype(np.float32)


@pytest.mark.parametrize("args,ok", [
    (SOAP, True), (["--shampoo_variant", "soap", "--adam_decay", "l2"], True),   # unused with mom
    (["--optimizer", "soap"], False), (SOAP + ["--adam_decay", "l2"], False),
    (SOAP + ["--clip_grad_norm", "1"], False)])
def test_soap_flags(args, ok):
    assert build_parser("cifar").parse_args([]).shampoo_variant == "roots"
    if ok:
        assert build_parser("cifar").parse_args(args).shampoo_variant == "soap"
    else:
        with pytest.raises(SystemExit):
            build_parser("cifar").parse_args(args)


# what the GPU tests feed soap_refresh: the fp32 run that sets their bound is itself orthonormal
@pytest.mark.parametrize("n,basis,rank", [(n, "random", None) for n in SIZES]
                         + [(64, "identity", None), (64, "random", 16)])
def test_oracle_fp32_refresh_is_orthonormal_and_signed(n, basis, rank):
    S, Q0 = refresh_case(n, basis, rank)
    Q64, Q32, A = sp.refresh(S, Q0), sp.refresh(S, Q0, np.float32), S.astype(np.float64) @ Q0
    assert Q32.dtype == np.float32 and sp.orth_err(Q64) < 1e-13 and sp.orth_err(Q32) < 2e-5
    R = Q64.T @ A
    assert (np.diag(R)[:rank or n] > 0).all() and np.abs(np.tril(R, -1)).max() < 1e-12
    if not rank:   # full rank: the factor is unique, numpy's QR with the same signs gives it
        q, r = np.linalg.qr(A)
        assert np.abs(q * np.sign(np.diag(r)) - Q64).max() < 1e-10


def test_cpu_backend_is_adamw_until_the_first_refresh_then_the_oracle():
    hp, kw = (0.9, 0.999, 1e-8, 0.95, 2), dict(shampoo_variant="soap", shampoo_beta2=0.95, shampoo_precond_every=2)
    be, adam = _backend("shampoo", **kw), _backend("adamw")
    _steps(be, 1), _steps(adam, 1)
    assert all(torch.equal(x, y) for x, y in zip((be.store.master, be.mom, be.adam_v),
                                                  (adam.store.master, adam.mom, adam.adam_v)))
    assert be.adam_state() == adam.adam_state()
    # two steps across a refresh, teacher-forced on a gradient of its own, from a fresh state
    be, gen = _backend("shampoo", **kw), torch.Generator().manual_seed(11)
    view = lambda x, s: x.detach()[s.offset:s.offset + s.numel].view(-1, s.shape[-1]).numpy()  # noqa: E731
    w0, convs = be.store.master.detach().clone(), [s for s in be.store.train_slots if s.kind == "conv"][:3]
    ref = {s.name: [(sp.fresh(s.numel // s.shape[-1], s.shape[-1], dt), view(w0, s).astype(dt))
                    for dt in (np.float64, np.float32)] for s in convs}
    for t in (1, 2):
        g = 0.1 * torch.randn(be.store.n_train, generator=gen)
        be.step_count = t - 1
        with torch.no_grad():
            be._soap_update(be.store.master, g, 1e-2)
        for s in convs:
            ref[s.name] = [sp.tensor_step(st, w, view(g, s), t, 1e-2, 1e-3, hp, dt)
                           for (st, w), dt in zip(ref[s.name], (np.float64, np.float32))]
    st = be.shampoo_state()
    assert st["variant"] == "soap" and st["failed"] == 0 and "PL" not in st and be.adam_state()[0] == 2
    for s in convs:
        (s64, w64), (_, w32) = ref[s.name]
        d0 = view(w0, s)   # the error of the two steps taken
        d_ref, err = so.rel(w32 - d0, w64 - d0), so.rel(view(be.store.master, s) - d0, w64 - d0)
        print(f"{s.name}: d_ref {d_ref:.3g} err {err:.3g}")
        assert err <= 4 * d_ref and sp.orth_err(s64["blocks"][0][2]) < 1e-13


COEF = [("beta1", 0.9), ("beta2", 0.999), ("epsilon", 1e-8), ("grad_scale", 1.0)]
ARGS = {
    "soap_refresh": [("tab", P), ("nblocks", 2), ("sides", 2)] + [
        (k, P) for k in ("L", "Rt", "QL", "QR", "gstep", "start")] + [("every", 3), ("fail", P)],
    "soap_rotate_adam": [("grad", P), ("tab", P), ("nblocks", 2)] + [(k, P) for k in ("QL", "QR", "mom", "v", "dir")] + COEF,
    "soap_update_pack": [(k, P) for k in ("master", "grad", "m", "v", "dir")] + [("n", 64)] + SCHED + [
        ("gstep", P), ("start", P)] + COEF + [("segs", P), ("nseg", 1)] + [
        (k, P) for k in ("wd_seg", "pre_seg", "bf", "lr_out", "adam_out")] + [("decay", PIECEWISE)]}


@pytest.mark.parametrize("op,ptr,coef", [("soap_refresh", "QL", {"every": 0}),
                                         ("soap_rotate_adam", "v", {"beta1": 1.0}),
                                         ("soap_update_pack", "dir", {"beta2": 1.0})])
def test_makers_record_one_op_and_check_their_arguments(op, ptr, coef):
    from distributed_tensorflow_resnet_amd import _C as nat

    def rec(**bad):   # on a fresh Plan with dummy pointers; `bad` overrides arguments by name
        plan = nat.Plan()
        getattr(plan, op)(*[bad.get(k, v) for k, v in ARGS[op]])
        return plan.size()

    assert rec() == 1
    for bad in ({ptr: ODD}, {ptr: 0}, coef):   # misaligned, null, a coefficient out of range
        with pytest.raises(ValueError, match=op):
            rec(**bad)
