"""Soft inequality rows: the seeded problems of tests/golden/make_golden_soft.py, tests/test_emu_soft.py and
tests/test_gpu_soft.py, and the AUGMENTED dense QP a caller had to write before QPFunction took `rho`:

    min 1/2 z'Qz + p'z + 1/2 sum_i rho_i t_i^2   s.t.  Gz <= h + t,  Az = b
    variables (z, t_soft):  Q' = blkdiag(Q, diag rho_soft),  p' = (p, 0),  G' = [G, -E],  A' = [A, 0]

E (nineq x nsoft) picks the soft rows.  numpy only.
"""
import numpy as np

import problems

# label -> (B, n, m, q): the smallest sizes that reach each pre-factorisation form (tests/test_emu_soft.py)
SHAPES = {
    "a": (3, 10, 20, 3),        # sweep + Rm; the diagonal crosses a 16-tile edge
    "b0": (3, 36, 20, 0),       # matrix-core pre-factorisation without ...
    "b1": (3, 40, 24, 4),       # ... and with equalities
    "c2": (2, 2, 120, 0),       # float32: Rg + Rw images of 8 / 15 blocks
    "d": (2, 100, 100, 10),     # large-QP family (sum 210 > 208); m = 100 crosses a 64-block edge
}
SEED = 41
FIXTURES = ("a", "b0", "b1", "d")


def soft_problem(label, dtype=np.float64):
    """(Q, p, G, h, A, b, rho): random_dense_qp with every fourth row hard (rho = inf) and the others soft, rho in [0.5, 5.5];
    the soft rows' h is lowered by up to 1 so that some of them are violated at the solution (the hard rows stay feasible
    at z0)."""
    B, n, m, q = SHAPES[label]
    Q, p, G, h, A, b = problems.random_dense_qp(B, n, m, q, seed=SEED)
    r = np.random.RandomState(SEED + 1)
    rho = 0.5 + 5.0 * r.rand(B, m)
    rho[:, ::4] = np.inf
    h = h - np.where(np.isfinite(rho), r.rand(B, m), 0.0)
    return tuple(np.ascontiguousarray(np.asarray(x).astype(dtype)) for x in (Q, p, G, h, A, b, rho))


def augment(Q, p, G, h, A, b, rho):
    """the augmented dense QP of ONE problem (no batch dimension: the soft set may differ per QP); returns
    (Q', p', G', h, A', b) and the indices of the soft rows"""
    n, m = Q.shape[0], G.shape[0]
    q = A.shape[0] if np.size(A) else 0
    soft = np.flatnonzero(np.isfinite(rho))
    ns = len(soft)
    Qa = np.zeros((n + ns, n + ns), Q.dtype)
    Qa[:n, :n] = Q
    Qa[n:, n:] = np.diag(rho[soft])
    pa = np.concatenate([p, np.zeros(ns, Q.dtype)])
    Ga = np.zeros((m, n + ns), Q.dtype)
    Ga[:, :n] = G
    Ga[soft, n + np.arange(ns)] = -1.0
    if q:
        Aa = np.zeros((q, n + ns), Q.dtype)
        Aa[:, :n] = A
    else:
        Aa = np.zeros(0, Q.dtype)
    return (Qa, pa, Ga, h.copy(), Aa, np.asarray(b).copy()), soft


def loss_vector(label):
    """c (B, n) of the loss <c, zhat> whose gradients the fixtures store"""
    B, n, m, q = SHAPES[label]
    return np.random.RandomState(SEED + 2).randn(B, n)
