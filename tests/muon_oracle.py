"""Reference for csrc/muon.hip: the momentum and weight formulas in the dtype they are given
(fp64 for a reference, fp32 tensors for the bit-exact checks: every torch op rounds once) and
the quintic Newton-Schulz iteration in fp64, without rounding (ns_exact) and with the one bf16
rounding of X0, A, B and X that the kernel's specification has (ns_bf16)."""
import torch

A, B, C = 3.4445, -4.7750, 2.0315


def moment(g, m, mu, scale, nesterov):
    """(m', u) of the specification: g' = s g, m' = mu m + g', u = g' + mu m' or m'."""
    gp = scale * g
    m1 = mu * m + gp
    return m1, (gp + mu * m1 if nesterov else m1)


def weight(w, o, lr, wd, q):
    """w' = (w - (lr wd) w) - (lr q) O; lr, wd and q as 0-d tensors of w's dtype."""
    return (w - (lr * wd) * w) - (lr * q) * o


def _ns(u, steps, rnd):
    R, K = u.shape
    x = rnd(u / (u.norm() + 1e-7))
    x = x.T if K <= R else x          # short x long
    for _ in range(steps):
        a = rnd(x @ x.T)
        b = rnd(B * a + C * (a @ a))
        x = rnd(A * x + b @ x)
    return x.T if K <= R else x       # back to the R x K orientation


def ns_exact(u, steps):
    return _ns(u.double(), steps, lambda x: x)


def ns_bf16(u, steps):
    return _ns(u.double(), steps, lambda x: x.to(torch.bfloat16).to(torch.float64))
