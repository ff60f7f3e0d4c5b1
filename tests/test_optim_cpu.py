"""The optimizer tests' reference (tests/optim_oracle.py) pinned to implementations
nobody here wrote (torch.optim.SGD), to the engine's host mirror of the schedule, and
to index loops written out by hand.  No GPU."""
import pytest
import torch

import optim_oracle as oo
from distributed_tensorflow_resnet_amd.train.schedule import (LRSchedule, cifar_lr_schedule,
                                                                imagenet_lr_schedule)

SEVEN = LRSchedule(0.3, [10, 20, 35, 50, 80, 81, 1000],
                   [0.3, 0.2, 0.1, 0.05, 0.02, 0.01, 0.005, 0.001],
                   warm_steps=5, warm_from=0.01, warm_to=0.3)


@pytest.mark.parametrize("momentum,wd,grad_scale", [(0.9, 2e-4, 1.0), (0.75, 0.05, 1 / 128),
                                                    (0.9, 0.05, 1 / 128)])
def test_sgd_reference_matches_torch_sgd(momentum, wd, grad_scale):
    g0 = torch.Generator().manual_seed(1)
    n, lr = 257, 0.37
    w0 = torch.randn(n, generator=g0, dtype=torch.float64)
    p = torch.nn.Parameter(w0.clone())
    opt = torch.optim.SGD([p], lr=lr, momentum=momentum, weight_decay=wd, dampening=0,
                          nesterov=False)
    w, mom = w0.clone(), torch.zeros(n, dtype=torch.float64)
    for _ in range(4):
        g = torch.randn(n, generator=g0, dtype=torch.float64) * 3
        p.grad = g * grad_scale
        opt.step()
        w, mom, B = oo.sgd_reference(w, g, mom, lr, momentum, wd, grad_scale, True)
        assert (B > 0).all()
        torch.testing.assert_close(w, p.detach(), rtol=1e-12, atol=0)
        torch.testing.assert_close(mom, opt.state[p]["momentum_buffer"], rtol=1e-12, atol=0)


def test_sgd_reference_without_momentum_matches_torch_sgd():
    g0 = torch.Generator().manual_seed(2)
    n, lr, wd, gs = 65, 0.1, 0.05, 1 / 128
    w = torch.randn(n, generator=g0, dtype=torch.float64)
    p = torch.nn.Parameter(w.clone())
    opt = torch.optim.SGD([p], lr=lr, momentum=0, weight_decay=wd)
    mom = torch.randn(n, generator=g0, dtype=torch.float64)
    for _ in range(4):
        g = torch.randn(n, generator=g0, dtype=torch.float64)
        p.grad = g * gs
        opt.step()
        w, m2, _ = oo.sgd_reference(w, g, mom, lr, 0.9, wd, gs, False)
        assert torch.equal(m2, mom)
        torch.testing.assert_close(w, p.detach(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("sched", [cifar_lr_schedule(), imagenet_lr_schedule(), SEVEN],
                         ids=["cifar", "imagenet", "seven"])
def test_lr_reference_matches_host_mirror(sched):
    steps = oo.lr_steps(sched)
    assert {0, 1, 2, 2 ** 31 + 5} <= set(steps)
    for b in sched.bounds:
        assert {b - 1, b, b + 1, b + 2} <= set(steps)
    for s in steps:
        assert abs(oo.lr_reference(sched, s) - sched.at(s)) <= 1e-12, s
    # the shape of the schedule itself: step 0 is begin(), step s sees f(s - 1)
    assert oo.lr_reference(sched, 0) == sched.init
    b0 = sched.bounds[0]
    assert oo.lr_reference(sched, b0) == sched.values[0]
    assert oo.lr_reference(sched, b0 + 1) == sched.values[1]
    assert oo.lr_reference(sched, sched.bounds[-1] + 1000) == sched.values[-1]


def test_expected_wbf_hand_example():
    """One 3x3 kernel C=3 K=4 (cpad 8, OHWI only) and one dense 4x3 kernel (kpad 8, both
    copies) against index loops."""
    specs = [("conv", 3, 3, 3, 4, 8, 4, True, False),
             ("dense", 1, 1, 4, 3, 4, 8, True, True)]
    seg, names, n, total, tile0, tiles = oo.build_seg_table(specs, gap=8)
    assert n == 108 + 12 and tiles == 2 and list(tile0) == [0, 1]
    assert [int(r["offset"]) for r in seg] == [0, 108]
    master = torch.arange(1, n + 1, dtype=torch.float32)   # distinct, exact in bf16
    got = oo.expected_wbf(seg, master, total).float()
    want = torch.zeros(total)
    o0 = int(seg[0]["bf_ohwi"])
    for co in range(4):
        for tap in range(9):
            for ci in range(3):
                want[o0 + (co * 9 + tap) * 8 + ci] = master[(tap * 3 + ci) * 4 + co]
    o1, h1 = int(seg[1]["bf_ohwi"]), int(seg[1]["bf_hwio"])
    for co in range(3):
        for ci in range(4):
            want[o1 + co * 4 + ci] = master[108 + ci * 3 + co]
            want[h1 + ci * 8 + co] = master[108 + ci * 3 + co]
    assert torch.equal(got, want)
    # the three copies do not overlap, start on multiples of 8 and leave the gaps zero
    assert seg[0]["bf_hwio"] == -1
    assert o0 % 8 == 0 and o1 % 8 == 0 and h1 % 8 == 0
    assert o0 >= 8 and o1 >= o0 + 4 * 9 * 8 + 8 and h1 >= o1 + 8 * 4 + 8 and total >= h1 + 32 + 8
    assert int((got != 0).sum()) == 108 + 12 + 12


def test_opt_work_builder_uses_engine_tiles():
    specs = [("conv", 3, 3, 16, 16, 16, 16, True, True), ("vec", 1, 1, 1, 3000, 1, 1, False, False),
             ("conv", 3, 3, 3, 16, 8, 16, True, False)]
    seg, names, n, total, _, _ = oo.build_seg_table(specs)
    work, blk = oo.build_opt_work(seg, names)
    assert [int(w["tiled"]) for w in work] == [1, 0, 1]
    assert blk == [0] * 3 + [1] * 3 + [2]
    assert [int(w["tile0"]) for w in work] == [0, 3, 6]
    work, blk = oo.build_opt_work(seg, names, grad_ptr=1 << 20,
                                  slabs={names[0]: (4096, 32, 16, 16), names[2]: (8192, 9, 16, 8)})
    assert (int(work[0]["tr"]), int(work[0]["tc"])) == (16, 16)
    assert int(work[2]["tr"]) == 27 and int(work[2]["cslab"]) == 8
    assert len(blk) == 9 + 3 + 16 // int(work[2]["tc"])
