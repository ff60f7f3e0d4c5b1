"""Tiled Muon on the device (csrc/muon_tiled.hip): the grouped Newton-Schulz launches against
the fp64 references of tests/muon_oracle.py, next to the one-workgroup kernel, and in the engine."""
import numpy as np
import pytest
import torch

import muon_oracle as mo
import optim_oracle as oo
from test_adam_gpu import nat  # noqa: F401
from distributed_tensorflow_resnet_amd.models.spec import imagenet_spec
from distributed_tensorflow_resnet_amd.ops import functional as F
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule
from distributed_tensorflow_resnet_amd.train.layout import muon_covers

pytestmark = pytest.mark.gpu

TILED = ["muon_tiled_moments", "muon_tiled_stage"] + \
    ["muon_tiled_syrk", "muon_tiled_syrk", "muon_tiled_apply"] * 5 + ["muon_tiled_unstage"]


def _buffers(gpu, shapes, offsets, total):
    g, m = torch.full((total,), 3.0), torch.full((total,), 5.0)
    us = []
    for (R, K), lo in zip(shapes, offsets):
        u = torch.randn(R, K, generator=torch.Generator().manual_seed(1000 * R + K))
        g[lo:lo + R * K], m[lo:lo + R * K] = u.flatten(), 0.0
        us.append(u)
    return g, m, us, (g.to(gpu), m.to(gpu), torch.full_like(g, -7.0).to(gpu))


def _within_bound(got, u, steps, what):
    exact, rnd = mo.ns_exact(u, steps), mo.ns_bf16(u, steps)
    d_ref = float((rnd - exact).norm() / exact.norm())
    err = float((got.double() - rnd).norm() / exact.norm())
    print(f"muon tiled {what} steps={steps}: d_ref {d_ref:.5f} err {err:.5f} ratio {err / d_ref:.3f}")
    assert err <= d_ref


# just past the small kernel, padded, transposed | as it lies, k-tiles, a mirrored tile | padded
# short side over a tile edge | a 5 x 5 triangle, both padded | ResNet-18's | the cover limit
@pytest.mark.parametrize("R,K,steps", [(80, 72, 1), (80, 72, 5), (128, 640, 1), (128, 640, 5),
                                       (600, 130, 5), (272, 300, 5), (1152, 128, 5),
                                       (1024, 1040, 1)])
def test_newton_schulz_against_the_rounding_faithful_reference(gpu, R, K, steps):
    """test_muon_gpu.py's construction and criterion: err <= d_ref, sentinels untouched, grad only
    read, m' = u at momentum 0; a second launch gives the same bits."""
    n, lo = R * K, 7
    g, m, (u,), (gd, md, od) = _buffers(gpu, [(R, K)], [lo], lo + n + 9)
    F.muon_orthogonalize_tiled(gd, md, [(R, K)], [lo], momentum=0.0, nesterov=False, steps=steps,
                               out=od)
    got, m1 = od.cpu(), md.cpu()
    assert torch.equal(gd.cpu(), g) and torch.equal(m1[lo:lo + n], u.flatten())
    for t, fill in ((got, -7.0), (m1, 5.0)):
        assert bool((t[:lo] == fill).all()) and bool((t[lo + n:] == fill).all())
    _within_bound(got[lo:lo + n].view(R, K), u, steps, f"{R}x{K}")
    if (R, K) == (272, 300):
        md2, od2 = m.to(gpu), torch.full_like(od, -7.0)
        F.muon_orthogonalize_tiled(gd, md2, [(R, K)], [lo], momentum=0.0, nesterov=False,
                                   steps=steps, out=od2)
        assert torch.equal(od2.cpu(), got) and torch.equal(md2.cpu(), m1)


def test_mixed_table_keeps_the_small_kernel_bit_for_bit(gpu):
    shapes, offs = [(144, 16), (128, 640)], [0, 2305]
    n = 2305 + 128 * 640 + 3
    g, m, us, (gd, md, od) = _buffers(gpu, shapes, offs, n)
    F.muon_orthogonalize_tiled(gd, md, shapes, offs, momentum=0.9, nesterov=True, steps=5, out=od)
    m2, o2 = m.to(gpu), torch.full_like(od, -7.0)
    F.muon_orthogonalize(gd, m2, shapes[:1], offs[:1], momentum=0.9, nesterov=True, steps=5, out=o2)
    assert torch.equal(od[:2304], o2[:2304]) and torch.equal(md[:2304], m2[:2304])
    assert float(od[2304]) == -7.0 and bool((od[-3:] == -7.0).all())
    _, u = mo.moment(us[1], torch.zeros_like(us[1]), 0.9, 1.0, True)
    _within_bound(od[2305:-3].cpu().view(128, 640), u, 5, "128x640 beside 144x16")


def test_cover_predicate(gpu, nat):
    assert nat.muon_tiled_covers(4608, 512) and nat.muon_tiled_covers(1024, 2048)
    assert not nat.muon_tiled_covers(1025, 1025) and not nat.muon_tiled_covers(64, 8193)
    x = torch.zeros(1025 * 1025, device=gpu)
    with pytest.raises(ValueError):
        F.muon_orthogonalize_tiled(x, x.clone(), [(1025, 1025)])


def _engine(gpu, optimizer, **kw):
    spec = imagenet_spec(18, image_hw=64)
    eng = Engine(spec, 8, weight_decay=5e-4, lr_schedule=cifar_lr_schedule(), optimizer=optimizer,
                 device=gpu, input_mode="nhwc", seed=0, **kw)
    gen = torch.Generator().manual_seed(5)
    imgs = torch.randn(8, 64, 64, 3, generator=gen).to(torch.bfloat16).float()
    eng.set_batch(imgs.to(gpu), torch.randint(0, spec.num_classes, (8,), generator=gen).to(gpu))
    return eng


def test_engine_muon_tiled_step(gpu, monkeypatch):
    """The plan, the gradients, every non-conv slot against a mom engine bit for bit (the dense
    kernel's 512,000 elements take both paths of the flat walk), the tiled directions' singular
    values and the bf16 copies."""
    monkeypatch.setenv("DTR_TUNE", "persist=0,opt_fused=0")
    ref = _engine(gpu, "mom")
    monkeypatch.setenv("DTR_TUNE", "persist=0")
    eng = _engine(gpu, "muon", muon_tiled=True)
    a, b = eng.seg["opt"]
    assert [n for n in eng.plan.names()[a:b] if n == "ohwi_pack" or "muon" in n] == \
        ["muon_orthogonalize"] + TILED + ["muon_update_pack", "ohwi_pack"]
    w0 = eng.params.master.clone().cpu()
    eng.step()
    ref.step()
    torch.cuda.synchronize()
    assert int(eng.gstep.item()) == 1 and torch.equal(eng.grad, ref.grad)
    w1, w_ref, g = eng.params.master.cpu(), ref.params.master.cpu(), eng.grad.cpu()
    lr, ntiled = float(np.float32(0.1)), 0
    for i, s in enumerate(eng.params.train_slots):
        sl = slice(s.offset, s.offset + s.numel)
        if s.kind != "conv":      # mom's update, bit for bit
            assert torch.equal(w1[sl], w_ref[sl]), (s.name, int((w1[sl] != w_ref[sl]).sum()))
            continue
        K = s.shape[-1]
        R = s.numel // K
        if muon_covers(R, K) or ntiled == 2:
            continue
        qv = float(eng.muon_q[i].item())
        o = (((w0[sl] - (lr * 5e-4) * w0[sl]) - w1[sl]).double() / (lr * qv)).view(R, K)
        u = (1.95 * g[sl]).view(R, K)          # m = 0: m' = g, u = g + 0.95 g
        exact, want = mo.ns_exact(u, 5), mo.ns_bf16(u, 5)
        sv, sw = torch.linalg.svdvals(o), torch.linalg.svdvals(want)
        # Weyl: a singular value moves by at most ||dO||_F <= d_ref ||O||_F, this tensor's own
        slack = float((want - exact).norm() / exact.norm()) * float(want.norm())
        print(f"{s.name} {R}x{K}: sv [{float(sv.min()):.3f}, {float(sv.max()):.3f}] reference "
              f"[{float(sw.min()):.3f}, {float(sw.max()):.3f}] slack {slack:.3f}")
        assert float(sw.min()) - slack <= float(sv.min()) and float(sv.max()) <= float(sw.max()) + slack
        ntiled += 1
    assert ntiled == 2
    assert torch.equal(eng.wbf, oo.expected_wbf(eng.seg_arr, eng.params.master, eng.wbf.numel()))
