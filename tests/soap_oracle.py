"""SOAP (csrc/soap.hip has the formulas) restated in numpy: every function takes the dtype it
computes in, so one text gives the fp64 reference and the plain fp32 run whose distance from it
(d_ref) is the yardstick the kernels are held to, as in shampoo_oracle."""
import numpy as np

from shampoo_oracle import blocks, stats


def qr_q(A, dtype=np.float64):
    """The orthonormal factor of A's Householder QR, diag(R) >= 0; a zero column is skipped."""
    A = np.array(A, dtype)
    n = len(A)
    W, sign = np.eye(n, dtype=dtype), np.ones(n, dtype)   # W becomes Q^T = H_{n-1} .. H_0
    for j in range(n):
        v = A[j:, j].copy()
        nrm = np.sqrt((v * v).sum(dtype=dtype))
        if not nrm > 0:
            continue
        beta = -nrm if v[0] >= 0 else nrm   # R[j][j]
        v[0] -= beta
        den = -beta * v[0]
        A[j:, j + 1:] -= np.outer(v, (v @ A[j:, j + 1:]) / den)
        W[j:] -= np.outer(v, (v @ W[j:]) / den)
        sign[j] = -1 if beta < 0 else 1
    return W.T * sign


def refresh(S, Q, dtype=np.float64):
    return qr_q(np.asarray(S, dtype) @ np.asarray(Q, dtype), dtype)


def orth_err(Q):
    return float(np.abs(np.asarray(Q, np.float64).T @ np.asarray(Q, np.float64) - np.eye(Q.shape[1])).max())


def coefs(b1, b2, eps):
    """(b1, 1 - b1, b2, 1 - b2, eps) in fp32, the differences rounded once from fp64."""
    b1, b2 = np.float32(b1), np.float32(b2)
    return b1, np.float32(1.0 - float(b1)), b2, np.float32(1.0 - float(b2)), np.float32(eps)


def rotate_adam(G, M, V, QL, QR, b1, b2, eps, dtype=np.float64):
    """(M', V', N) of one block; G is the scaled gradient."""
    c1, o1, c2, o2, e = (dtype(x) for x in coefs(b1, b2, eps))
    G, M, V, QL, QR = (np.asarray(x, dtype) for x in (G, M, V, QL, QR))
    M1 = c1 * M + o1 * G
    Gt, Mt = QL.T @ G @ QR, QL.T @ M1 @ QR
    V1 = c2 * V + o2 * (Gt * Gt)
    return M1, V1, QL @ (Mt / (np.sqrt(V1) + e)) @ QR.T


def tensor_step(st, w, G, t, lr, wd, hp, dtype=np.float64):
    """One step of an R x K conv kernel: st = {"blocks": [L, R, QL, QR] per block at the live
    sizes, "M", "V": R x K}, hp = (b1, b2, eps, shampoo_beta2, every).  Returns (st', w')."""
    b1, b2, eps, sb2, every = hp
    w, G = np.asarray(w, dtype), np.asarray(G, dtype)
    M, V, N, new = np.zeros_like(G), np.zeros_like(G), np.zeros_like(G), []
    for (i, j, r, k), (L, R, QL, QR) in zip(blocks(*G.shape), st["blocks"]):
        sl = (slice(i, i + r), slice(j, j + k))
        L, R = stats(L, R, G[sl], sb2, dtype)
        if t % every == 0:
            QL, QR = refresh(L, QL, dtype), refresh(R, QR, dtype)
        M[sl], V[sl], N[sl] = rotate_adam(G[sl], st["M"][sl], st["V"][sl], QL, QR, b1, b2, eps, dtype)
        new.append([L, R, QL, QR])
    f1, f2 = float(np.float32(b1)), float(np.float32(b2))
    alpha = dtype(float(lr) * np.sqrt(1.0 - f2 ** t) / (1.0 - f1 ** t))
    w1 = (w - alpha * N) - (dtype(np.float32(lr)) * dtype(np.float32(wd))) * w
    return {"blocks": new, "M": M, "V": V}, w1


def fresh(R, K, dtype=np.float64):
    """The state of a new R x K tensor: zero statistics and moments, identity bases."""
    z, eye = (lambda *s: np.zeros(s, dtype)), (lambda n: np.eye(n, dtype=dtype))
    return {"blocks": [[z(r, r), z(k, k), eye(r), eye(k)] for _, _, r, k in blocks(R, K)],
            "M": z(R, K), "V": z(R, K)}
