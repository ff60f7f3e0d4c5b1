"""AugMix's Jensen-Shannon head in fp64 numpy: rows n, n + B, n + 2B of [3B, C] logits are
one image's clean view and two AugMix views (csrc/xent_row.h; train/jsd.py)."""
import numpy as np


def jsd_head(logits, labels, B, weight, eps=0.0, k=5):
    """-> dict(loss, top1, topk [3B] per-row outputs, grad, p [3B, C], mean: the scalar loss)."""
    z = np.asarray(logits, dtype=np.float64)
    N, C = z.shape
    assert N == 3 * B
    y = np.asarray(labels)[:B].astype(np.int64)
    l = z - z.max(1, keepdims=True)
    l = (l - np.log(np.exp(l).sum(1, keepdims=True))).reshape(3, B, C)
    p = np.exp(l)
    mx = l.max(0)
    log_m = mx + np.log(np.exp(l - mx).sum(0)) - np.log(3.0)
    with np.errstate(invalid="ignore"):
        kl = np.where(p > 0, p * (l - log_m), 0.0).sum(2)                      # [3, B]
        soft = np.where(p > 0, p * (l - log_m - kl[..., None]), 0.0)
    t = np.full((B, C), eps / C)
    t[np.arange(B), y] += 1.0 - eps
    hard = -(t * l[0]).sum(1)                                                  # L_h, [B]
    loss = np.zeros(N)
    loss[:B] = 3.0 * (hard + weight * kl.mean(0))
    g = weight * soft
    g[0] += 3.0 * (p[0] - t)
    y3 = np.tile(y, 3)
    zy = z[np.arange(N), y3]
    return {"loss": loss, "mean": loss.sum() / N, "grad": g.reshape(N, C) / N, "p": p.reshape(N, C),
            "top1": (z.argmax(1) == y3).astype(np.float64),
            "topk": ((z > zy[:, None]).sum(1) < min(k, C)).astype(np.float64)}
