"""Soft two-sided inequality rows: the seeded problems of tests/golden/make_golden_soft_range.py,
tests/test_emu_soft_range.py and tests/test_gpu_soft_range.py, the AUGMENTED dense QP a caller had to write before QPFunction
took `soft_range`,

    min 1/2 z'Qz + p'z + sum ( gu tu + 1/2 ru tu^2 + gl tl + 1/2 rl tl^2 )   s.t.  l - tl <= Gz <= h + tu,  tu, tl >= 0,  Az = b
    ->   x = (z, tu_Fu, tl_Fl),  Q' = blkdiag(Q, diag ru_Fu, diag rl_Fl),  p' = (p, gu_Fu, gl_Fl),  A' = [A, 0, 0],
         rows  G z - Eu tu <= h,   -G_L z - El tl <= -l_L,   -tu <= 0,   -tl <= 0

(L: the rows with a finite lower bound; Fu: the rows whose upper side has finite gamma and rho; Fl: the rows of L whose lower
side has), and the way its gradients fold back onto the eleven inputs.  numpy only.
"""
import numpy as np

# label -> (B, n, m, q): the smallest sizes that reach each form of the loop's soft-range role (those of the elastic role)
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
# all: every row soft on both sides; mixed: by i % 4 soft on both sides, hard upper / soft lower, soft upper / hard lower,
# one-sided elastic
KINDS = ("all", "mixed")
SEED = 81
# label -> its own seed where the plain one leaves a pair near a kink of the solution map or misses a row kind (the generator of
# the fixtures asserts both; tests/golden/make_golden_soft_range.py)
SEEDS = {"t1a": 132, "t1b": 90, "c4": 82}
COUNTED = ("t1a", "t1b", "t2", "t4")      # the four smallest: iteration counts are gated against oracle/qp_oracle on the augmented QP
FIELDS = ("lower", "gamma_u", "rho_u", "gamma_l", "rho_l")
INF = np.inf


def fixture_name(label, kind):
    return "softrange_%s_%s_b%d_n%d_m%d_q%d" % ((label, kind) + SHAPES[label])


def soft_range_problem(label, kind="all", dtype=np.float64):
    """(Q, p, G, h, A, b, lower, gamma_u, rho_u, gamma_l, rho_l): the recipe of the elastic rows (Q = L L^T / n + I, gamma in
    [0.2, 3.2], rho in [0.5, 4.5], h = G z0 + 0.5 U) with the band lower = h - (0.3 + U); on the rows i % 6 == 0 the band is
    pulled 1.5 U BELOW G z0 (rows end violated upwards, tu > 0), on the rows i % 6 == 3 it is pushed so that lower lies 1.5 U
    ABOVE G z0 (rows end violated downwards, tl > 0).  kind = "mixed": the row kinds by i % 4; the pulled rows are even and
    keep a soft upper side, the pushed rows are odd and keep a soft lower side or none, so z0 satisfies every hard side."""
    B, n, m, q = SHAPES[label]
    r = np.random.RandomState(SEEDS.get((label, kind), SEEDS.get(label, SEED)))
    L = r.randn(B, n, n)
    Q = np.matmul(L, L.transpose((0, 2, 1))) / n + np.eye(n)
    G = r.randn(B, m, n)
    z0 = r.randn(B, n)
    p = r.randn(B, n)
    gamma_u = 0.2 + 3.0 * r.rand(B, m)
    rho_u = 0.5 + 4.0 * r.rand(B, m)
    gamma_l = 0.2 + 3.0 * r.rand(B, m)
    rho_l = 0.5 + 4.0 * r.rand(B, m)
    i = np.arange(m)
    width = 0.3 + r.rand(B, m)
    pull = 1.5 * r.rand(B, m)
    gz = np.einsum("bmn,bn->bm", G, z0)
    h = gz + 0.5 * r.rand(B, m)
    h = np.where(i % 6 == 0, h - pull, h)
    h = np.where(i % 6 == 3, gz + pull + width, h)
    lower = h - width
    A = r.randn(B, q, n)
    b = np.einsum("bqn,bn->bq", A, z0)
    if kind == "mixed":
        gamma_u[:, i % 4 == 1] = INF
        gamma_l[:, i % 4 == 2] = INF
        lower[:, i % 4 == 3] = -INF
    if q == 0:
        A, b = np.zeros(0), np.zeros(0)
    return tuple(np.ascontiguousarray(np.asarray(x).astype(dtype)) for x in (Q, p, G, h, A, b, lower, gamma_u, rho_u, gamma_l, rho_l))


def loss_vector(label):
    """c (B, n) of the loss <c, zhat> whose gradients the fixtures store"""
    B, n, m, q = SHAPES[label]
    return np.random.RandomState(SEED + 2).randn(B, n)


def row_sets(lower, gamma_u, rho_u, gamma_l, rho_l):
    """(L, Fu, Fl) of ONE problem: the two-sided rows, the rows with a soft upper side, the two-sided rows with a soft lower side"""
    two = np.isfinite(lower)
    return (np.flatnonzero(two), np.flatnonzero(np.isfinite(gamma_u) & np.isfinite(rho_u)),
            np.flatnonzero(two & np.isfinite(gamma_l) & np.isfinite(rho_l)))


def augment(Q, p, G, h, A, lower, gamma_u, rho_u, gamma_l, rho_l):
    """the augmented QP of ONE problem (no batch dimension: the row sets may differ per QP): (Q', p', G', h', A', sets); A' is
    empty where A is"""
    n, m = Q.shape[0], G.shape[0]
    sets = row_sets(lower, gamma_u, rho_u, gamma_l, rho_l)
    L, Fu, Fl = sets
    ku, kl, nl = Fu.size, Fl.size, L.size
    Eu = np.zeros((m, ku))
    Eu[Fu, np.arange(ku)] = 1.0
    El = np.zeros((m, kl))
    El[Fl, np.arange(kl)] = 1.0
    Q2 = np.zeros((n + ku + kl, n + ku + kl))
    Q2[:n, :n] = Q
    Q2[n:n + ku, n:n + ku] = np.diag(rho_u[Fu])
    Q2[n + ku:, n + ku:] = np.diag(rho_l[Fl])
    p2 = np.concatenate([p, gamma_u[Fu], gamma_l[Fl]])
    G2 = np.block([[G, -Eu, np.zeros((m, kl))],
                   [-G[L], np.zeros((nl, ku)), -El[L]],
                   [np.zeros((ku, n)), -np.eye(ku), np.zeros((ku, kl))],
                   [np.zeros((kl, n)), np.zeros((kl, ku)), -np.eye(kl)]])
    h2 = np.concatenate([h, -lower[L], np.zeros(ku + kl)])
    A2 = np.concatenate([A, np.zeros((A.shape[0], ku + kl))], axis=1) if np.size(A) else np.zeros(0)
    return Q2, p2, G2, h2, A2, sets


def split(x2, sets, m, fill):
    """a vector over the augmented rows -> (upper rows, lower rows, tu's rows, tl's rows), each (m); `fill` where a side is absent"""
    L, Fu, Fl = sets
    lo, tu, tl = np.full(m, fill, x2.dtype), np.full(m, fill, x2.dtype), np.full(m, fill, x2.dtype)
    lo[L] = x2[m:m + L.size]
    tu[Fu] = x2[m + L.size:m + L.size + Fu.size]
    tl[Fl] = x2[m + L.size + Fu.size:]
    return x2[:m], lo, tu, tl


def split_t(x2, sets, n, m):
    """the variables of the augmented QP -> (z (n), tu (m), tl (m)); 0 where a side is hard or absent"""
    L, Fu, Fl = sets
    tu, tl = np.zeros(m, x2.dtype), np.zeros(m, x2.dtype)
    tu[Fu] = x2[n:n + Fu.size]
    tl[Fl] = x2[n + Fu.size:]
    return x2[:n], tu, tl


def fold(dQ2, dp2, dG2, dh2, dA2, sets, n, m):
    """gradients of the augmented QP -> (dQ, dp, dG, dh, dA, dlower, dgamma_u, drho_u, dgamma_l, drho_l): G enters as +G on top
    and -G_L below, lower as -h'; dgamma is the t-part of dp', drho the diagonal of the t-block of dQ' (0 on a hard or absent
    side)"""
    L, Fu, Fl = sets
    ku = Fu.size
    dG = dG2[:m, :n].copy()
    dG[L] -= dG2[m:m + L.size, :n]
    dlower = np.zeros(m, dh2.dtype)
    dlower[L] = -dh2[m:m + L.size]
    dgu, dru, dgl, drl = (np.zeros(m, dp2.dtype) for _ in range(4))
    dgu[Fu] = dp2[n:n + ku]
    dgl[Fl] = dp2[n + ku:]
    dq = np.diag(dQ2)
    dru[Fu] = dq[n:n + ku]
    drl[Fl] = dq[n + ku:]
    dA = dA2[:, :n] if np.size(dA2) else dA2
    return dQ2[:n, :n], dp2[:n], dG, dh2[:m], dA, dlower, dgu, dru, dgl, drl
