"""An independent fp64 reference for the distillation loss head, per row, and the bounds the
distillation tests hold the kernels to.  Plain numpy; nothing here calls the kernels.

  q = softmax(t / tau)     p = softmax(z)     p_tau = softmax(z / tau)
  loss = (1 - alpha) * L_h + alpha * tau^2 * sum_c q_c * (log q_c - log p_tau_c)
  g_c  = (1 - alpha) * (p_c - t_c) + alpha * tau * (p_tau_c - q_c)      (before any batch scale)

with L_h and t_c the hard loss and target: label smoothing eps and a mixup partner (yb, lam)
included, as tests/xent_oracle.py and csrc/xent_row.h define them.

Bounds.  The label-smoothing tests (tests/test_label_smoothing_gpu.py) hold one `__expf` /
`__logf` softmax of these kernels to rtol 1e-4 + atol 1e-6 per probability (P_RTOL, P_ATOL)
and its loss to 1e-4 (LOSS_TOL).  The hard term keeps those, weighted (1 - alpha).  The soft
term is two more softmaxes of the same kind (p_tau and q), entering the gradient with weight
alpha * tau and the loss with weight alpha * tau^2, so each adds that weight times the
per-softmax bound.  bf16 dlogits add half a bf16 ulp (8 significant bits: 2^(e - 8) for a
value in [2^e, 2^(e + 1))) of the reference value, batch scale included.
Everything carries a factor 2 (MARGIN) for the order of the wave folds.
"""
import numpy as np

P_RTOL, P_ATOL, LOSS_TOL, MARGIN = 1e-4, 1e-6, 1e-4, 2.0


def _log_softmax(z):
    m = z.max(axis=1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))


def distill_rows(z, t, y, tau, alpha, eps=0.0, yb=None, lam=1.0):
    """fp64 rows: dict(loss [N], grad [N, K], p, p_tau, q [N, K])."""
    z, t = np.asarray(z, dtype=np.float64), np.asarray(t, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    N, K = z.shape
    rows = np.arange(N)
    tgt = np.zeros((N, K))
    tgt[rows, y] += lam
    if yb is not None:
        tgt[rows, np.asarray(yb, dtype=np.int64)] += 1.0 - lam
    tgt = (1.0 - eps) * tgt + eps / K
    lp, ls, lq = _log_softmax(z), _log_softmax(z / tau), _log_softmax(t / tau)
    p, p_tau, q = np.exp(lp), np.exp(ls), np.exp(lq)
    hard = -(tgt * lp).sum(axis=1)
    kl = np.where(q > 0, q * (lq - ls), 0.0).sum(axis=1)
    return {"loss": (1.0 - alpha) * hard + alpha * tau * tau * kl,
            "grad": (1.0 - alpha) * (p - tgt) + alpha * tau * (p_tau - q),
            "p": p, "p_tau": p_tau, "q": q}


def _p_bound(p):
    return P_RTOL * p + P_ATOL


def grad_bound(r, tau, alpha, scale=1.0, bf16=False):
    """Per-element bound [N, K] on a gradient row times the batch scale `scale`."""
    b = (1.0 - alpha) * _p_bound(r["p"]) + alpha * tau * (_p_bound(r["p_tau"]) + _p_bound(r["q"]))
    b = MARGIN * b * scale
    if bf16:
        g = np.abs(r["grad"]) * scale
        b = b + np.where(g > 0, 2.0 ** (np.floor(np.log2(np.maximum(g, 1e-300))) - 8), 0.0)
    return b


def loss_bound(tau, alpha):
    """Bound on one row's loss."""
    return MARGIN * ((1.0 - alpha) * LOSS_TOL + alpha * tau * tau * 2.0 * LOSS_TOL)
