"""Float64 reference of QPFunction(duals=True)'s backward, shared by tests/test_emu_duals.py and tests/test_gpu_duals.py
(numpy, on the host): the six per-QP gradients of a loss l(zhat, lam, nu) from a dense solve of the 3-block system the
forward-mode tests use (tests/test_emu_jvp.py: full_kkt_tangent),

    K3 = [[Q, G^T, A^T], [D G, -I, 0], [A, 0, 0]],   (z', lam', nu') = -K3^-1 (rx, D rz, ry),   D = diag(d),

whose adjoint is  w = -K3^-T (g_z, g_lam, g_nu),  dx = w_x,  dz = d * w_lam,  dy = w_nu  -- then the formulas of qp.py:157-173.
Beside it the tolerance of that comparison, taken from the fixtures of tests/golden/make_golden_duals.py."""
import numpy as np

from conftest import load_golden

NAMES = ("dQ", "dp", "dG", "dh", "dA", "db")
FIXTURES = {(100, 100, 0): "duals_b4_n100_m100", (100, 50, 10): "duals_b4_n100_m50_q10", (12, 9, 3): "duals_b2_n12_m9_q3"}


def dense_tol(n, m, q):
    """max(1e-8, 10 x the reference's own LU-vs-dense gap at the nearest fixture shape): 1e-8 is what the forward-mode tests
    ask of the same solve; the reference's factor_kkt + solve_kkt, a condensed factorisation like the kernels', shows
    how much of the d-conditioning noise (d = lam / s spans 1e-10 .. 1e8) such a factorisation carries at that shape."""
    key = min(FIXTURES, key=lambda k: (k[0] - n) ** 2 + (k[1] - m) ** 2 + (k[2] - q) ** 2)
    return max(1e-8, 10.0 * float(load_golden(FIXTURES[key])["lu_vs_dense_gap"]))


def _bat(x, B, nd):
    x = np.asarray(x, np.float64)
    if x.ndim == nd - 1 or x.shape[0] == 1:
        return np.broadcast_to(x.reshape(x.shape[-(nd - 1):]), (B,) + x.shape[-(nd - 1):])
    return x


def dense_grads(arrs, sol, cots, chunk=256):
    """{name: (B, ...)} per-QP gradients for cotangents cots = (g_z, g_lam, g_nu), each an array or None (zero), at the
    solution sol = (zhat, lam, slacks, nu); dA, db only with equality constraints"""
    zh, lam, sl, nu = [np.asarray(x, np.float64) for x in sol]
    B, n = zh.shape
    m, q = lam.shape[1], nu.shape[1]
    Q, G = _bat(arrs[0], B, 3), _bat(arrs[2], B, 3)
    A = _bat(arrs[4], B, 3) if q else np.zeros((B, 0, n))
    gz, gl, gn = [np.zeros((B, k)) if g is None else np.asarray(g, np.float64) for g, k in zip(cots, (n, m, q))]
    d = np.maximum(lam, 1e-8) / np.maximum(sl, 1e-8)
    N = n + m + q
    dx, dz, dy = np.empty((B, n)), np.empty((B, m)), np.empty((B, q))
    for lo in range(0, B, chunk):
        s = slice(lo, min(B, lo + chunk))
        K = np.zeros((s.stop - lo, N, N))
        K[:, :n, :n], K[:, :n, n:n + m], K[:, :n, n + m:] = Q[s], G[s].transpose(0, 2, 1), A[s].transpose(0, 2, 1)
        K[:, n:n + m, :n] = d[s][:, :, None] * G[s]
        K[:, n:n + m, n:n + m] = -np.eye(m)
        K[:, n + m:, :n] = A[s]
        w = -np.linalg.solve(K.transpose(0, 2, 1), np.concatenate([gz[s], gl[s], gn[s]], 1)[:, :, None])[:, :, 0]
        dx[s], dz[s], dy[s] = w[:, :n], d[s] * w[:, n:n + m], w[:, n + m:]
    o = lambda u, v: u[:, :, None] * v[:, None, :]      # noqa: E731
    out = {"dQ": 0.5 * (o(dx, zh) + o(zh, dx)), "dp": dx, "dG": o(dz, zh) + o(lam, dx), "dh": -dz}
    if q:
        out["dA"], out["db"] = o(dy, zh) + o(nu, dx), -dy
    return out


def checksum(*arrs):
    """of regenerated inputs, as tests/golden/make_golden.py stores it"""
    return np.array([float(np.sum(np.asarray(a, np.float64) * np.cos(np.arange(np.asarray(a).size).reshape(np.shape(a)) % 97)))
                     for a in arrs if np.asarray(a).size])


def rel(a, b):
    """per-QP relative L2 distance of a from b (rows = QPs)"""
    a = np.asarray(a, np.float64).reshape(len(a), -1)
    b = np.asarray(b, np.float64).reshape(len(b), -1)
    return np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-300)
