"""The exact-conv oracle (tests/exact_conv.py) against a naive loop and ops/reference.py,
and the two conditions every GPU case of test_exact_conv_gpu.py rests on: the 2**24
exactness guard, and outputs on which the ONE bf16 rounding can be told from none and
from round-half-away."""
import numpy as np
import pytest
import torch

import exact_conv as ec
from distributed_tensorflow_resnet_amd.ops import reference as ref


def _naive_conv(x, w, s):
    """Six loops over (n, ho, wo, r, c, ci) on Python / numpy integers; the output
    channels ride along as an int64 vector."""
    N, H, W, C = x.shape
    kh, kw, _, K = w.shape
    (bh, _), (bw, _) = ec.pads(kh), ec.pads(kw)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    y = np.zeros((N, Ho, Wo, K), dtype=np.int64)
    for n in range(N):
        for ho in range(Ho):
            for wo in range(Wo):
                for r in range(kh):
                    for c in range(kw):
                        h, v = ho * s + r - bh, wo * s + c - bw
                        if not (0 <= h < H and 0 <= v < W):
                            continue
                        for ci in range(C):
                            y[n, ho, wo] += x[n, h, v, ci] * w[r, c, ci]
    return y


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("s", [1, 2])
def test_oracle_matches_naive_loop_and_reference(k, s):
    N, H, C, K = 2, 5, 8, 16
    g = ec.gen(k * 10 + s)
    x, w = ec.ints(g, (N, H, H, C), -3, 3), ec.ints(g, (k, k, C, K), -2, 2)
    dy = ec.ints(g, (N, ec.out_size(H, k, s), ec.out_size(H, k, s), K), -3, 3)
    y = ec.conv_fwd(x, w, s)
    assert y.shape == (N, (H - 1) // s + 1, (H - 1) // s + 1, K)
    assert np.array_equal(y.numpy(), _naive_conv(x.numpy(), w.numpy(), s).astype(np.float64))
    # ops/reference.py (F.pad + F.conv2d), written independently: exact agreement, and of
    # the two gradients with its autograd
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    yr = ref.conv2d(xr, wr, s)
    assert torch.equal(yr.detach(), y)
    yr.backward(dy.double())
    assert torch.equal(ec.conv_dgrad(dy, w, tuple(x.shape), s), xr.grad)
    assert torch.equal(ec.conv_wgrad(dy, x, k, s), wr.grad)
    # the gradients against the naive loop too: <dy, conv(e_i)> for a few unit inputs
    dx = ec.conv_dgrad(dy, w, tuple(x.shape), s)
    for idx in [(0, 0, 0, 0), (1, H - 1, H - 1, C - 1), (0, 2, 3, 5), (1, H - 1, 0, 2)]:
        e = np.zeros((N, H, H, C), dtype=np.int64)
        e[idx] = 1
        assert float(dx[idx]) == float((_naive_conv(e, w.numpy(), s) * dy.numpy()).sum())


def test_oracle_epilogue_terms():
    """Prologue, bias on columns < nbias only, residual and accumulate base, as operands()
    combines them."""
    c = ec.Case("t", "fwd", 2, 5, 8, 16, 3, 2, res=True, acc=True, nbias=10, pre=True, seed=5)
    o = ec.operands(c)
    a = torch.relu(o["a"] * o["sc"] + o["sh"])
    want = ec.conv_fwd(a, o["w"], 2) + o["res"] + o["base"]
    want[..., :10] += o["bias"]
    assert torch.equal(o["want"], want)
    assert float((a * 2).frac().abs().max()) == 0 and float(a.max()) <= 8   # half-integers
    dw = ec.conv_wgrad(o["res"], o["a"], 3, 2)
    assert ec.crop_hwio(dw, 10, 3).shape == (3, 3, 3, 10)
    assert torch.equal(ec.crop_hwio(dw, 10, 3), dw[:, :, :3, :10])


def test_rounding_census_counts():
    t = torch.tensor([256.0, 257.0, 259.0, 258.0, -257.0, 1.5, 128.5, 129.5, 513.0, 514.0],
                     dtype=torch.float64)
    # rounded at all: 257, 259, -257, 128.5, 129.5, 513, 514; ties where RNE truncates and
    # half-away increments: 257, -257, 128.5, 514
    assert ec.rounding_census(t) == (7, 4)
    assert t.to(torch.bfloat16).tolist()[:5] == [256.0, 256.0, 260.0, 258.0, -256.0]


@pytest.mark.parametrize("case", ec.conv_cases(), ids=lambda c: c.name)
def test_case_is_exact_and_rounds(case):
    """The guard holds; and unless the case's whole range is below 256 (1x1 convs of <= 32
    channels, 6 * 32 + 8, and the CIFAR stem's 27 real terms, 6 * 27: no value bf16 could
    round, asserted) or its output is fp32, the expected output holds values that bf16 rounds
    and RNE-vs-half-away ties."""
    o = ec.operands(case)
    assert o["bound"] < ec.EXACT_LIMIT
    if case.f32:
        return
    rounded, ties = ec.rounding_census(o["want"])
    if o["bound"] < 256:
        assert case.kdim <= 32 and rounded == 0
        return
    print(f"{case.name}: bound {o['bound']:.0f}, rounded {rounded}, ties {ties}")
    assert rounded > 0, "no output is rounded: change the seed"
    assert ties > 0, "no RNE tie: change the seed"


@pytest.mark.parametrize("C,H,N", ec.ABWD_CASES)
@pytest.mark.parametrize("with_add", [False, True])
def test_abwd_case_is_exact_and_rounds(C, H, N, with_add):
    o = ec.abwd_operands(C, H, N, with_add)
    assert o["bound"] < ec.EXACT_LIMIT
    rounded, ties = ec.rounding_census(o["want"])
    print(f"abwd {C}@{H} n{N}: bound {o['bound']:.0f}, rounded {rounded}, ties {ties}")
    assert rounded > 0 and ties > 0
    # the ReLU mask sits on its edge somewhere with a non-zero gradient: > and >= differ
    edge = ((o["x"] * o["scale"] + o["shift"]) == 0) & (o["da"] != 0)
    assert int(edge.sum()) > 0


@pytest.mark.parametrize("M,C,K", ec.BNF_CASES)
@pytest.mark.parametrize("pre", [False, True])
def test_streaming_fwd_case_is_exact_and_rounds(M, C, K, pre):
    case, o = ec.bnf_operands(M, C, K, pre)
    assert o["bound"] < ec.EXACT_LIMIT
    rounded, ties = ec.rounding_census(o["want"])
    print(f"{case.name}: bound {o['bound']:.0f}, rounded {rounded}, ties {ties}")
    assert rounded > 0 and ties > 0


@pytest.mark.parametrize("M,C,K", ec.BND_CASES)
@pytest.mark.parametrize("with_add", [False, True])
def test_streaming_dgrad_case_is_exact_and_rounds(M, C, K, with_add):
    o = ec.bnd_operands(M, C, K, with_add)     # asserts the intermediate is bf16-exact
    assert o["bound"] < ec.EXACT_LIMIT
    rounded, ties = ec.rounding_census(o["want"])
    print(f"bnd {M} {C} {K}: rounded {rounded}, ties {ties}")
    assert rounded > 0 and ties > 0


@pytest.mark.parametrize("wc", ec.WGRAD_CASES, ids=lambda c: c.name)
def test_wgrad_case_is_exact(wc):
    """fp32 outputs owe the exact number: only the guard applies; scaled by 1/4 and added
    to an integer base the result is still far inside fp32's 24 bits."""
    o = ec.wgrad_operands(wc)
    assert o["bound"] < ec.EXACT_LIMIT
    assert 4 * o["bound"] < ec.EXACT_LIMIT
    assert float(o["want"].abs().max()) > 0
