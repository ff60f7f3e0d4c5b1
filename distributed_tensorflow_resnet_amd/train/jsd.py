"""AugMix's Jensen-Shannon consistency loss (Hendrycks et al. 2020) in fp32 torch: the CPU
backend's loss and the statement of what csrc/xent_row.h's jsd_rows computes.

The network runs on N = 3B rows; rows n, n + B, n + 2B are image n's clean view and two
AugMix views.  With l_i = log_softmax(z_i), p_i = exp(l_i), weight w:

    log M_c = logsumexp_i(l_ic) - log 3
    KL_i    = sum_c p_ic * (l_ic - log M_c)           (p_ic == 0 adds exactly 0)
    JSD_n   = (KL_0 + KL_1 + KL_2) / 3
    loss    = mean_{n<B} [ L_h(z_0, y_n) + w * JSD_n ]
    g_ic    = ([i == 0] * 3 * (p_0c - t_c) + w * p_ic * (l_ic - log M_c - KL_i)) / N

log M_c takes the place of the paper's clamp of M to [1e-7, 1]: no log of a probability is
ever taken.  Precision is counted over all three views against the image's label.
"""
from __future__ import annotations

import math

import torch

from ..ops import reference as ref


def jsd_terms(logits: torch.Tensor, B: int):
    """(l [3, B, C] log-probabilities, log M [B, C], KL [3, B]) of [3B, C] logits."""
    l = torch.log_softmax(logits, 1).reshape(3, B, -1)
    log_m = torch.logsumexp(l, 0) - math.log(3.0)
    p = torch.exp(l)
    kl = torch.where(p > 0, p * (l - log_m), torch.zeros_like(p)).sum(2)
    return l, log_m, kl


def jsd_loss(logits: torch.Tensor, labels: torch.Tensor, B: int, weight: float,
             label_smoothing: float = 0.0) -> torch.Tensor:
    """The scalar loss above; `labels` [B] or [3B] (the first B are read)."""
    _, _, kl = jsd_terms(logits, B)
    hard = ref.softmax_cross_entropy(logits[:B], labels[:B], label_smoothing)   # the mean
    return hard + weight * kl.mean(0).mean()


def jsd_grad(logits: torch.Tensor, labels: torch.Tensor, B: int, weight: float,
             label_smoothing: float = 0.0) -> torch.Tensor:
    """The closed form g_ic of d loss / d logits, [3B, C] (what the kernels write)."""
    l, log_m, kl = jsd_terms(logits, B)
    p = torch.exp(l)
    C = logits.shape[1]
    t = torch.full((B, C), label_smoothing / C, dtype=logits.dtype)
    t[torch.arange(B), labels[:B].long()] += 1.0 - label_smoothing
    g = weight * torch.where(p > 0, p * (l - log_m - kl[..., None]), torch.zeros_like(p))
    g[0] += 3.0 * (p[0] - t)
    return g.reshape(3 * B, C) / (3 * B)
