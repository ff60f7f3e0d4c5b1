"""Blocked Shampoo with SGD grafting (csrc/shampoo.hip) restated in numpy: every function takes
the dtype it computes in, so one text gives the fp64 reference and the plain fp32 run whose
distance from it (d_ref) is the yardstick the kernels are held to.

Per 64 x 64 block G of the scaled gradient of a conv kernel (the row-major R x K matrix):
L' = b2 L + c G G^T, R' = b2 R + c G^T G (c = 1 for b2 = 1, else 1 - b2 rounded to fp32 once);
on a refresh step the roots (A + eps ||A||_F I)^(-1/4) by the coupled Newton iteration below;
U = PL G PR; per tensor c = ||g'|| / ||U||; then mom's update with c U for the gradient."""
import numpy as np

BLOCK = 64


def blocks(R, K):
    """(i0, j0, r, k) of every block of an R x K matrix, row blocks first (the table's order)."""
    return [(i, j, min(BLOCK, R - i), min(BLOCK, K - j))
            for i in range(0, R, BLOCK) for j in range(0, K, BLOCK)]


def root_exact(A, eps):
    """(A + eps ||A||_F I)^(-1/4) by eigh in fp64."""
    A = np.asarray(A, np.float64)
    w, V = np.linalg.eigh(A + eps * np.linalg.norm(A) * np.eye(len(A)))
    return (V * w ** -0.25) @ V.T


def root_iter(A, eps, dtype=np.float64, max_iters=32, tol=1e-5):
    """The coupled Newton iteration for the same root in `dtype`: (X, steps taken, last
    max|Mk - I|)."""
    A = np.asarray(A, dtype)
    n, eye = len(A), np.eye(len(A), dtype=dtype)
    D = A + dtype(eps) * np.linalg.norm(A).astype(dtype) * eye
    z = dtype(5.0) / (dtype(2.0) * np.linalg.norm(D).astype(dtype))
    X, Mk, it = z ** dtype(0.25) * eye, z * D, 0
    res = float(np.abs(Mk - eye).max())
    while it < max_iters and not res < tol:
        T = (dtype(5.0) * eye - Mk) / dtype(4.0)
        T2 = T @ T
        Mk, X, it = (T2 @ T2) @ Mk, X @ T, it + 1
        res = float(np.abs(Mk - eye).max())
    return X, it, res


def stat_coef(b2):
    b2 = np.float32(b2)
    return b2, np.float32(1.0) if b2 == 1 else np.float32(1.0 - float(b2))


def stats(L, R, G, b2, dtype=np.float64):
    """(L', R') of one block."""
    b, c = (dtype(x) for x in stat_coef(b2))
    G = np.asarray(G, dtype)
    return b * np.asarray(L, dtype) + c * (G @ G.T), b * np.asarray(R, dtype) + c * (G.T @ G)


def direction(PL, G, PR, dtype=np.float64):
    return (np.asarray(PL, dtype) @ np.asarray(G, dtype)) @ np.asarray(PR, dtype)


def rel(x, ref):
    return float(np.linalg.norm(np.asarray(x, np.float64) - ref) / np.linalg.norm(ref))


def fma32(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64)
            + np.asarray(c, np.float64)).astype(np.float32)


def update32(w, m, d, lr, momentum, wd, vec):
    """The update's fp32 expressions for direction d (c U, one rounding, or s g): gv =
    fma(wd, w, d) on the 16-byte path (vec), wd w + d with both rounded on the scalar path;
    m' = fma(momentum, m, gv), w' = fma(-lr, m', w).  Returns (w', m')."""
    f = np.float32
    gv = np.where(vec, fma32(f(wd), w, d), f(wd) * w + d)
    m1 = fma32(f(momentum), m, gv)
    return fma32(-f(lr), m1, w), m1


def vector_path(seg_offsets, seg_numels, n):
    """Per element of the flat buffer: whether FlatWalk updates it in a whole 16-byte group (its
    aligned group of four lies inside one segment and inside n)."""
    seg = np.full(n + 4, -1)
    for i, (o, k) in enumerate(zip(seg_offsets, seg_numels)):
        seg[o:o + k] = i
    g4 = seg[:(n + 3) // 4 * 4].reshape(-1, 4)
    whole = (g4 == g4[:, :1]).all(1) & (g4[:, 0] >= 0)
    return np.repeat(whole, 4)[:n]
