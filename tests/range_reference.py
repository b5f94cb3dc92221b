"""Two-sided inequality rows: the seeded problems of tests/golden/make_golden_range.py, tests/test_emu_range.py
and tests/test_gpu_range.py, the DOUBLED QP a caller had to write before QPFunction took `lower`,

    lower <= Gz <= h   ->   G' = [G; -G_F],  h' = [h; -lower_F]        (F: the rows with a finite lower bound)

the way its gradients fold back onto the nineq rows, and the closed form of the box with Q = G = I.  numpy only.
"""
import numpy as np

# label -> (B, n, m, q): the smallest sizes that reach each form of the loop's range role
SHAPES = {
    "t1a": (2, 6, 4, 2),          # one tile row
    "t1b": (2, 12, 9, 3),         # one tile row
    "t2": (2, 20, 24, 3),         # two tile rows
    "t4": (2, 20, 40, 4),         # four tile rows, one wave
    "t7s": (2, 10, 70, 0),        # m crosses a 64-lane slot
    "c4": (2, 100, 50, 10),       # four-row chain form
    "box": (2, 100, 100, 0),      # G = I, the box on all variables: seven-row chain form
    "g10": (2, 40, 130, 0),       # thread grid, 10 blocks
    "g13": (2, 20, 170, 2),       # thread grid, 13 blocks
}
SIDES = ("all", "half")           # every row two-sided / about half of them one-sided (lower = -inf)
SEED = 53
# label -> its own seed: with the plain one the fixture has a row within 2e-6 of its bound with a zero multiplier, a kink of the
# solution map at which no two solvers agree on a gradient (the generator of the fixtures asserts there is none)
SEEDS = {"box": 54}
COUNTED = ("t1a", "t1b", "t2", "t4")      # <= 40 rows: iteration counts are gated against oracle/qp_oracle on the doubled QP


def fixture_name(label, sides):
    return "range_%s_%s_b%d_n%d_m%d_q%d" % ((label, sides) + SHAPES[label])


def range_problem(label, sides="all", dtype=np.float64):
    """(Q, p, G, h, A, b, lower): the recipe of problems.random_dense_qp (Q = L L^T / n + I; G = I for the box) with the band
    lower = G z0 - sl0 <= G z <= G z0 + s0 = h  around a feasible point z0, s0 and sl0 in [0.05, 0.55]: narrow enough that
    rows end at h, rows end at lower and rows stay inside (the generator of the fixtures asserts all three);
    sides = "half": every second row one-sided."""
    B, n, m, q = SHAPES[label]
    r = np.random.RandomState(SEEDS.get(label, SEED))
    L = r.randn(B, n, n)
    Q = np.matmul(L, L.transpose((0, 2, 1))) / n + np.eye(n)
    G = np.broadcast_to(np.eye(n), (B, n, n)).copy() if label == "box" else r.randn(B, m, n)
    z0 = r.randn(B, n)
    p = (3.0 if label == "box" else 1.0) * r.randn(B, n)              # (the box: a good part of the variables at a bound)
    gz = np.einsum("bmn,bn->bm", G, z0)
    h = gz + 0.05 + 0.5 * r.rand(B, m)
    lower = gz - 0.05 - 0.5 * r.rand(B, m)
    A = r.randn(B, q, n)
    b = np.einsum("bqn,bn->bq", A, z0)
    if sides == "half":
        lower[:, 1::2] = -np.inf
    if q == 0:
        A, b = np.zeros(0), np.zeros(0)
    return tuple(np.ascontiguousarray(np.asarray(x).astype(dtype)) for x in (Q, p, G, h, A, b, lower))


def loss_vector(label):
    """c (B, n) of the loss <c, zhat> whose gradients the fixtures store"""
    B, n, m, q = SHAPES[label]
    return np.random.RandomState(SEED + 2).randn(B, n)


def double(G, h, lower):
    """the doubled rows of ONE problem (no batch dimension: F may differ per QP): (G', h', F)"""
    F = np.flatnonzero(np.isfinite(lower))
    return np.concatenate([G, -G[F]]), np.concatenate([h, -lower[F]]), F


def split(x2, F, m, fill):
    """a vector over the doubled rows -> (upper (m), lower (m)); `fill` on the one-sided rows of the lower part"""
    lo = np.full(m, fill, x2.dtype)
    lo[F] = x2[m:]
    return x2[:m], lo


def fold(dG2, dh2, F, m):
    """gradients of the doubled QP -> (dG, dh, dlower) of the two-sided rows: G enters as +G on top and -G_F below, lower as -h'"""
    dG = dG2[:m].copy()
    dG[F] -= dG2[m:]
    dlower = np.zeros(m, dh2.dtype)
    dlower[F] = -dh2[m:]
    return dG, dh2[:m], dlower


def box_closed_form(p, lo, up):
    """Q = I, G = I, no equalities:  zhat = clip(-p, lo, up),  lam_u = max(0, -p - up),  lam_l = max(0, lo + p)"""
    return np.clip(-p, lo, up), np.maximum(0.0, -p - up), np.maximum(0.0, lo + p)
