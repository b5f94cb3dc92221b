"""Elastic inequality rows: the seeded problems of tests/golden/make_golden_elastic.py, tests/test_emu_elastic.py
and tests/test_gpu_elastic.py, the AUGMENTED dense QP a caller had to write before QPFunction took `l1`,

    min 1/2 z'Qz + p'z + sum_F ( gamma_i t_i + 1/2 rho_i t_i^2 )   s.t.  Gz <= h + E t,  t >= 0,  Az = b
    ->   x = (z, t_F),  Q' = blkdiag(Q, diag rho_F),  p' = (p, gamma_F),  G' = [[G, -E], [0, -I]],  h' = (h, 0),  A' = [A, 0]

(F: the rows with finite gamma and rho; E (m, k) picks them), and the way its gradients fold back onto the eight inputs.
numpy only.
"""
import numpy as np

# label -> (B, n, m, q): the smallest sizes that reach each form of the loop's elastic role (those of the range role)
SHAPES = {
    "t1a": (2, 6, 4, 2),          # one tile row
    "t1b": (2, 12, 9, 3),         # one tile row
    "t2": (2, 20, 24, 3),         # two tile rows
    "t4": (2, 20, 40, 4),         # four tile rows, one wave
    "t7s": (2, 10, 70, 0),        # m crosses a 64-lane slot
    "c4": (2, 100, 50, 10),       # four-row chain form
    "c7": (2, 100, 100, 0),       # seven-row chain form: the headline shape
    "g10": (2, 40, 130, 0),       # thread grid, 10 blocks
    "g13": (2, 20, 170, 2),       # thread grid, 13 blocks
}
KINDS = ("all", "half")           # every row elastic / every second row hard (gamma = +inf)
SEED = 71
# label -> its own seed where the plain one leaves a row near a kink of the solution map or misses a row kind (the generator
# of the fixtures asserts both; tests/golden/make_golden_elastic.py)
SEEDS = {"t1a": 72, "t1b": 72, "t7s": 73, "c4": 72, "c7": 76, "g10": 72, "g13": 73}
COUNTED = ("t1a", "t1b", "t2", "t4")      # <= 40 rows: iteration counts are gated against oracle/qp_oracle on the augmented QP


def fixture_name(label, kind):
    return "elastic_%s_%s_b%d_n%d_m%d_q%d" % ((label, kind) + SHAPES[label])


def elastic_problem(label, kind="all", dtype=np.float64):
    """(Q, p, G, h, A, b, rho, gamma): the recipe of problems.random_dense_qp (Q = L L^T / n + I) with gamma in [0.2, 3.2],
    rho in [0.5, 4.5] and h = G z0 + 0.5 U, pulled 1.5 U BELOW G z0 on every third row -- so that rows end violated (t > 0),
    rows end held at h with a multiplier below gamma, and rows end inactive (the generator of the fixtures asserts all three).
    On a hard row of kind = "half" (every second row, gamma = +inf) the pull is left out: the QP stays feasible."""
    B, n, m, q = SHAPES[label]
    r = np.random.RandomState(SEEDS.get(label, SEED))
    L = r.randn(B, n, n)
    Q = np.matmul(L, L.transpose((0, 2, 1))) / n + np.eye(n)
    G = r.randn(B, m, n)
    z0 = r.randn(B, n)
    p = r.randn(B, n)
    gamma = 0.2 + 3.0 * r.rand(B, m)
    rho = 0.5 + 4.0 * r.rand(B, m)
    pull = 1.5 * r.rand(B, m) * (np.arange(m) % 3 == 0)
    h = np.einsum("bmn,bn->bm", G, z0) + 0.5 * r.rand(B, m)
    A = r.randn(B, q, n)
    b = np.einsum("bqn,bn->bq", A, z0)
    if kind == "half":
        gamma[:, 1::2] = np.inf
        pull[:, 1::2] = 0.0
    h = h - pull
    if q == 0:
        A, b = np.zeros(0), np.zeros(0)
    return tuple(np.ascontiguousarray(np.asarray(x).astype(dtype)) for x in (Q, p, G, h, A, b, rho, gamma))


def loss_vector(label):
    """c (B, n) of the loss <c, zhat> whose gradients the fixtures store"""
    B, n, m, q = SHAPES[label]
    return np.random.RandomState(SEED + 2).randn(B, n)


def elastic_rows(gamma, rho):
    return np.flatnonzero(np.isfinite(gamma) & np.isfinite(rho))


def augment(Q, p, G, h, A, gamma, rho):
    """the augmented QP of ONE problem (no batch dimension: F may differ per QP): (Q', p', G', h', A', F); A' is empty where A is"""
    n, m = Q.shape[0], G.shape[0]
    F = elastic_rows(gamma, rho)
    k = F.size
    E = np.zeros((m, k))
    E[F, np.arange(k)] = 1.0
    Q2 = np.zeros((n + k, n + k))
    Q2[:n, :n] = Q
    Q2[n:, n:] = np.diag(rho[F])
    p2 = np.concatenate([p, gamma[F]])
    G2 = np.block([[G, -E], [np.zeros((k, n)), -np.eye(k)]])
    h2 = np.concatenate([h, np.zeros(k)])
    A2 = np.concatenate([A, np.zeros((A.shape[0], k))], axis=1) if np.size(A) else np.zeros(0)
    return Q2, p2, G2, h2, A2, F


def split(x2, F, m, fill):
    """a vector over the augmented rows -> (the rows' part (m), t's part (m)); `fill` on the hard rows of t's part"""
    tt = np.full(m, fill, x2.dtype)
    tt[F] = x2[m:]
    return x2[:m], tt


def fold(dQ2, dp2, dG2, dh2, dA2, F, n, m):
    """gradients of the augmented QP -> (dQ, dp, dG, dh, dA, drho, dgamma) of the elastic rows: dgamma is the t-part of dp',
    drho the diagonal of the t-block of dQ' (0 on a hard row)"""
    dgamma, drho = np.zeros(m, dp2.dtype), np.zeros(m, dp2.dtype)
    dgamma[F] = dp2[n:]
    drho[F] = np.diag(dQ2[n:, n:])
    dA = dA2[:, :n] if np.size(dA2) else dA2
    return dQ2[:n, :n], dp2[:n], dG2[:m, :n], dh2[:m], dA, drho, dgamma
