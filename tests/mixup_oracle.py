"""An independent fp64 reference for mixup (Zhang et al. 2018): the blended input and the
two-label softmax cross-entropy, with tf.losses.softmax_cross_entropy's label smoothing.

Plain numpy; nothing here calls the kernels, ops/reference.py or the engine.

  input     x   = lam * x_a + (1 - lam) * x_b
  target    t_c = eps / K + (1 - eps) * (lam * [c == ya] + (1 - lam) * [c == yb])
  row loss      = lse(z) - (1 - eps) * (lam * z[ya] + (1 - lam) * z[yb]) - (eps / K) * sum_c z[c]
  gradient  g_c = softmax(z)_c - t_c                    (per row, before any batch scale)
  precision     : top-1 / in-top-k against the dominant label, ya if lam >= 0.5 else yb
"""
import numpy as np


def blend(xa, xb, lam):
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    return lam * xa + (1.0 - lam) * xb


def mixed_xent(logits, ya, yb, lam, eps=0.0):
    """(row losses [N], softmax [N, K], row gradients softmax - target [N, K]), fp64.
    `lam`: a number or one value per row."""
    z = np.asarray(logits, dtype=np.float64)
    ya, yb = np.asarray(ya, dtype=np.int64), np.asarray(yb, dtype=np.int64)
    N, K = z.shape
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (N,))
    m = z.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(axis=1))
    p = np.exp(z - lse[:, None])
    r = np.arange(N)
    t = np.full((N, K), eps / K)
    np.add.at(t, (r, ya), (1.0 - eps) * lam)
    np.add.at(t, (r, yb), (1.0 - eps) * (1.0 - lam))
    loss = lse - (1.0 - eps) * (lam * z[r, ya] + (1.0 - lam) * z[r, yb]) - (eps / K) * z.sum(axis=1)
    return loss, p, p - t


def dominant(ya, yb, lam):
    """The label the training precision is counted against."""
    ya, yb = np.asarray(ya, dtype=np.int64), np.asarray(yb, dtype=np.int64)
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), ya.shape)
    return np.where(lam >= 0.5, ya, yb)
