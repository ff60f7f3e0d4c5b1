"""Muon on the device (csrc/muon.hip): the Newton-Schulz workgroup against the fp64 references of
tests/muon_oracle.py, the element-wise parts bit for bit, and the engine's step."""
import numpy as np
import pytest
import torch

import muon_oracle as mo
import optim_oracle as oo
from test_adam_gpu import _sa, _st, nat  # noqa: F401
from distributed_tensorflow_resnet_amd.models.spec import cifar_spec, imagenet_spec
from distributed_tensorflow_resnet_amd.ops import functional as F
from distributed_tensorflow_resnet_amd.train.engine import Engine, cifar_lr_schedule
from distributed_tensorflow_resnet_amd.train.schedule import constant_lr

pytestmark = pytest.mark.gpu


# one tile; padding on both sides; the other orientation; more k-steps; 64 wide; all of LDS
@pytest.mark.parametrize("steps", (1, 5))
@pytest.mark.parametrize("R,K", [(16, 16), (27, 16), (16, 32), (144, 16), (32, 64), (576, 64)])
def test_newton_schulz_against_the_rounding_faithful_reference(gpu, R, K, steps):
    """||kernel - ns_bf16|| / ||ns_exact|| <= d_ref = ||ns_bf16 - ns_exact|| / ||ns_exact||, the
    rounding noise of the algorithm itself; sentinels around the tensor stay as they were."""
    n, lo, hi = R * K, 7, 9
    u = torch.randn(R, K, generator=torch.Generator().manual_seed(1000 * R + K))
    g = torch.full((lo + n + hi,), 3.0)
    g[lo:lo + n] = u.flatten()
    m = torch.full_like(g, 5.0)
    m[lo:lo + n] = 0.0
    gd, md, od = g.to(gpu), m.to(gpu), torch.full_like(g, -7.0).to(gpu)
    F.muon_orthogonalize(gd, md, [(R, K)], [lo], momentum=0.0, nesterov=False, steps=steps, out=od)
    got, m1 = od.cpu(), md.cpu()
    assert torch.equal(gd.cpu(), g)                          # grad is only read
    assert torch.equal(m1[lo:lo + n], u.flatten())           # m' = 0 m + g
    for t, fill in ((got, -7.0), (m1, 5.0)):
        assert bool((t[:lo] == fill).all()) and bool((t[lo + n:] == fill).all())
    exact, rnd = mo.ns_exact(u, steps), mo.ns_bf16(u, steps)
    d_ref = float((rnd - exact).norm() / exact.norm())
    err = float((got[lo:lo + n].view(R, K).double() - rnd).norm() / exact.norm())
    print(f"muon ns {R}x{K} steps={steps}: d_ref {d_ref:.5f} err {err:.5f} ratio {err / d_ref:.3f}")
    assert err <= d_ref


def test_launcher_refuses_what_one_workgroup_cannot_hold(gpu, nat):
    assert nat.muon_covers(576, 64) and nat.muon_covers(64, 576)
    assert not nat.muon_covers(577, 64) and not nat.muon_covers(65, 65)
    x = torch.zeros(65 * 65, device=gpu)
    with pytest.raises(ValueError):
        F.muon_orthogonalize(x, x.clone(), [(65, 65)])


# conv 144 x 16 (transposed) | gamma 16 | bias 10 | conv 16 x 32 (as it lies, from element 2330)
SPECS = [("conv", 3, 3, 16, 16, 16, 16, True, True), ("vec", 1, 1, 1, 16, 1, 1, False, False),
         ("vec", 1, 1, 1, 10, 1, 1, False, False), ("conv", 1, 1, 16, 32, 16, 32, True, True)]
MU, SCALE, MOM, WD, AUX, LR = 0.9, 0.5, 0.8, 0.01, 0.5, 0.05


@pytest.mark.parametrize("nesterov", (True, False))
def test_elementwise_parts_bit_exact(gpu, nat, nesterov):
    seg, _, n, bf_total, _, _ = oo.build_seg_table(SPECS)
    assert [int(r["offset"]) for r in seg] == [0, 2304, 2320, 2330] and n == 2842
    segs_d = torch.from_numpy(seg.view(np.uint8).copy()).to(gpu)
    gen = torch.Generator().manual_seed(3)
    w0, g, m0 = (torch.randn(n, generator=gen) for _ in range(3))
    conv = torch.zeros(n, dtype=torch.bool)
    conv[:2304] = conv[2330:] = True
    mseg = torch.tensor([1, 0, 0, 1], dtype=torch.int32, device=gpu)
    q = torch.tensor([1.0, 0.0, 0.0, 2.0 ** 0.5], device=gpu)
    gstep = torch.tensor([3], dtype=torch.int64, device=gpu)

    def run():
        w, m, gd = w0.to(gpu), m0.to(gpu), g.to(gpu)
        wbf, lr_out = torch.zeros(bf_total, dtype=torch.bfloat16, device=gpu), torch.zeros(1, device=gpu)
        d = F.muon_orthogonalize(gd, m, [(144, 16), (16, 32)], [0, 2330], momentum=MU,
                                 nesterov=nesterov, steps=5, grad_scale=SCALE)
        m_mid = m.cpu()
        nat.muon_update_pack(w.data_ptr(), gd.data_ptr(), m.data_ptr(), d.data_ptr(), n,
                             *_sa(constant_lr(LR)), gstep.data_ptr(), MOM, WD, AUX, SCALE,
                             segs_d.data_ptr(), len(seg), mseg.data_ptr(), q.data_ptr(),
                             wbf.data_ptr(), lr_out.data_ptr(), _st())
        torch.cuda.synchronize()
        return w.cpu(), m.cpu(), d.cpu(), wbf.cpu(), m_mid, float(lr_out.item())

    w1, m1, d, wbf, m_mid, lr = run()
    assert lr == float(np.float32(LR))
    want_m, _ = mo.moment(g, m0, MU, SCALE, nesterov)
    assert torch.equal(m_mid[conv], want_m[conv]) and torch.equal(m_mid[~conv], m0[~conv])
    assert bool((d[~conv] == 0).all()) and float(d[conv].abs().max()) > 0.01
    f = lambda x: torch.tensor(x, dtype=torch.float32)   # noqa: E731
    for a, b, qv in ((0, 2304, 1.0), (2330, n, 2.0 ** 0.5)):
        assert torch.equal(w1[a:b], mo.weight(w0[a:b], d[a:b], f(LR), f(WD), f(qv)))
    # the other segments: sgd_update_pack itself at lr * aux_scale on the same inputs
    ws, ms = w0.to(gpu), m0.to(gpu)
    nat.sgd_update_pack(ws.data_ptr(), g.to(gpu).data_ptr(), ms.data_ptr(), n,
                        *_sa(constant_lr(float(np.float32(LR) * np.float32(AUX)))),
                        gstep.data_ptr(), MOM, WD, SCALE, 1, segs_d.data_ptr(), len(seg), 0, 0, 1,
                        _st())
    assert torch.equal(w1[~conv], ws.cpu()[~conv]) and torch.equal(m1[~conv], ms.cpu()[~conv])
    assert torch.equal(wbf.float(), _hwio_only(seg, w1, bf_total))
    for x, y in zip(run(), (w1, m1, d, wbf, m_mid, lr)):   # a second launch: the same bits
        assert x == y if isinstance(x, float) else torch.equal(x, y)


def _hwio_only(seg, w, total):
    """After the walk alone: the HWIO copies of bf16(w'), zero elsewhere (OHWI is ohwi_pack's)."""
    out = torch.zeros(total)
    for r in seg:
        if r["bf_hwio"] >= 0:
            o, a = int(r["bf_hwio"]), int(r["offset"])
            out[o:o + int(r["numel"])] = w[a:a + int(r["numel"])].to(torch.bfloat16).float()
    return out


# ------------------------------------------------------------------------------------ engine
def _engine(spec, gpu, optimizer="muon", **kw):
    eng = Engine(spec, 8, weight_decay=5e-4, lr_schedule=cifar_lr_schedule(), optimizer=optimizer,
                 device=gpu, input_mode="nhwc", seed=0, **kw)
    gen = torch.Generator().manual_seed(5)
    imgs = torch.randn(8, spec.image_h, spec.image_w, 3, generator=gen).to(torch.bfloat16).float()
    eng.set_batch(imgs.to(gpu), torch.randint(0, spec.num_classes, (8,), generator=gen).to(gpu))
    return eng


@pytest.mark.parametrize("persist", (0, 1))
def test_engine_muon_step(gpu, monkeypatch, persist):
    monkeypatch.setenv("DTR_TUNE", f"persist={persist},opt_fused=0")
    ref = _engine(cifar_spec(8), gpu, optimizer="mom")
    monkeypatch.setenv("DTR_TUNE", f"persist={persist}")
    eng = _engine(cifar_spec(8), gpu)
    assert eng.persist == bool(persist) and not eng.opt_fused and "muon" in eng.opt_fused_reason
    a, b = eng.seg["opt"]
    assert [n for n in eng.plan.names()[a:b] if "pack" in n or "muon" in n] == \
        ["muon_orthogonalize", "muon_update_pack", "ohwi_pack"]
    w0 = eng.params.master.clone().cpu()
    eng.step()
    ref.step()
    torch.cuda.synchronize()
    assert not eng.persist_error() and int(eng.gstep.item()) == 1
    assert torch.equal(eng.grad, ref.grad)
    w1, w_ref, g = eng.params.master.cpu(), ref.params.master.cpu(), eng.grad.cpu()
    lr, nconv = float(np.float32(0.1)), 0
    for i, s in enumerate(eng.params.train_slots):
        sl = slice(s.offset, s.offset + s.numel)
        if s.kind != "conv":      # mom's update, bit for bit
            assert torch.equal(w1[sl], w_ref[sl]), s.name
            continue
        K = s.shape[-1]
        R = s.numel // K
        qv = float(eng.muon_q[i].item())
        assert qv == float(np.sqrt(np.float32(max(1.0, K / R))))
        o = ((w0[sl] - (lr * 5e-4) * w0[sl]) - w1[sl]).double() / (lr * qv)   # the direction taken
        assert abs(float((w1[sl] - w0[sl]).norm()) / (lr * qv * float(o.norm())) - 1) < 1e-2
        if nconv < 2:             # the singular values are those ns_bf16 gives for the same u
            u = (1.95 * g[sl]).view(R, K)          # m = 0: m' = g, u = g + 0.95 g
            sv = torch.linalg.svdvals(o.view(R, K))
            want = torch.linalg.svdvals(mo.ns_bf16(u, 5))
            print(f"{s.name} {R}x{K}: sv [{float(sv.min()):.3f}, {float(sv.max()):.3f}] reference "
                  f"[{float(want.min()):.3f}, {float(want.max()):.3f}]")
            # Weyl: a singular value moves by at most ||dO||_2 <= ||dO||_F, and the kernel is
            # within d_ref <= 0.022 (5 steps) of ns_bf16 relative to ||O||_F
            slack = 0.022 * float(want.norm())
            assert float(want.min()) - slack <= float(sv.min())
            assert float(sv.max()) <= float(want.max()) + slack
            nconv += 1
    assert nconv == 2
    assert torch.equal(eng.wbf, oo.expected_wbf(eng.seg_arr, eng.params.master, eng.wbf.numel()))


def test_engine_muon_refusals(gpu):
    with pytest.raises(ValueError, match="576"):
        _engine(imagenet_spec(18, image_hw=64), gpu)
    with pytest.raises(ValueError, match="clip_grad_norm"):
        _engine(cifar_spec(8), gpu, clip_grad_norm=1.0)
