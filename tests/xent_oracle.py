"""An independent fp64 reference for the loss head: smoothed softmax cross-entropy
(tf.losses.softmax_cross_entropy(label_smoothing=eps)) and tf.nn.in_top_k.

Plain numpy; nothing here calls the kernels, ops/reference.py or the engine.

  target    t_c = (1 - eps) * [c == y] + eps / K
  row loss      = lse(z) - (1 - eps) * z[y] - (eps / K) * sum_c z[c]
  gradient  g_c = softmax(z)_c - t_c                    (per row, before any batch scale)
  in_top_k      = 0 <= y < K  and  z[y] finite  and  #{c : z[c] > z[y]} < k
"""
import numpy as np


def smoothed_xent(logits, labels, eps=0.0):
    """(row losses [N], softmax [N, K], row gradients softmax - target [N, K]), fp64."""
    z = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    N, K = z.shape
    m = z.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(axis=1))
    p = np.exp(z - lse[:, None])
    t = np.full((N, K), eps / K)
    t[np.arange(N), y] += 1.0 - eps
    loss = lse - (1.0 - eps) * z[np.arange(N), y] - (eps / K) * z.sum(axis=1)
    return loss, p, p - t


def in_top_k(logits, labels, k):
    """bool [N]: ties that straddle the k-th place count as in."""
    z = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    N, K = z.shape
    out = np.zeros(N, dtype=bool)
    for i in range(N):
        if not 0 <= y[i] < K or not np.isfinite(z[i, y[i]]):
            continue
        out[i] = int((z[i] > z[i, y[i]]).sum()) < k
    return out
