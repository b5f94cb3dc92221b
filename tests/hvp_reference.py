"""Float64 reference of the SECOND-ORDER pass of QPFunction, shared by tests/test_hvp_reference.py,
tests/test_emu_backward2.py and tests/test_gpu_backward2.py (numpy, on the host, dense solves per QP).

At a solution (zhat, lam, s, nu), with the kernels' clamps d = clamp(lam, 1e-8) / clamp(s, 1e-8) and

    M = [[Q, G^T, A^T], [G, -diag(1/d), 0], [A, 0, 0]],

the first backward solves M (dx, dz, dy) = -(r_z, r_lam, r_nu) and returns
    dQ = 1/2 (dx zhat' + zhat dx'), dp = dx, dG = dz zhat' + lam dx', dh = -dz, dA = dy zhat' + nu dx', db = -dy.
For cotangents W = (W_Q, W_p, W_G, W_h, W_A, W_b) on those six, psi = sum_i <W_i, grad_i>; `second_order` returns the gradient
of psi with respect to (r_z, r_lam, r_nu) -- (zdot, lamdot, nudot) -- and to the six parameters (HQ .. Hb):

    S = 1/2 (W_Q + W_Q'),  t_x = S zhat + W_p + W_G' lam + W_A' nu,  t_z = W_G zhat - W_h,  t_y = W_A zhat - W_b
    M (zdot, lamdot, nudot) = -(t_x, t_z, t_y)
    a = dz / clamp(lam, 1e-8)
    g_z = S dx + W_G' dz + W_A' dy + G' (a lamdot),  g_lam = W_G dx + a (G zdot + t_z),  g_nu = W_A dx
    M (ex, ez, ey) = -(g_z, g_lam, g_nu)
    HQ = 1/2 (dx zdot' + zdot dx') + 1/2 (ex zhat' + zhat ex'),   Hp = ex
    HG = lamdot dx' + dz zdot' + (a lamdot) zhat' + ez zhat' + lam ex',   Hh = -(a lamdot) - ez
    HA = nudot dx' + dy zdot' + ey zhat' + nu ex',   Hb = -ey

The dense solves use the row-scaled system of tests/duals_reference.py ([d G, -I, 0] in the second block row): the same
solution, without entries of size 1/d ~ 1e8 in the matrix."""
import numpy as np

NAMES = ("HQ", "Hp", "HG", "Hh", "HA", "Hb")


def _bat(x, B, nd):
    x = np.asarray(x, np.float64)
    if x.ndim == nd - 1 or x.shape[0] == 1:
        return np.broadcast_to(x.reshape(x.shape[-(nd - 1):]), (B,) + x.shape[-(nd - 1):])
    return x


def clamp_d(lam, sl):
    return np.maximum(lam, 1e-8) / np.maximum(sl, 1e-8)


def kkt_solve(Q, G, A, d, rx, rz, ry):
    """(x, z, y) with M (x, z, y) = -(rx, rz, ry), one QP"""
    n, m, q = Q.shape[0], G.shape[0], A.shape[0]
    K = np.zeros((n + m + q, n + m + q))
    K[:n, :n], K[:n, n:n + m], K[:n, n + m:] = Q, G.T, A.T
    K[n:n + m, :n] = d[:, None] * G
    K[n:n + m, n:n + m] = -np.eye(m)
    K[n + m:, :n] = A
    w = np.linalg.solve(K, -np.concatenate([rx, d * rz, ry]))
    return w[:n], w[n:n + m], w[n + m:]


def first_backward(arrs, sol, cots, solve=None):
    """(dx, dz, dy), each (B, .), of the first backward for cotangents cots = (r_z, r_lam, r_nu) (None = zero).
    solve(i, rx, rz, ry) -> (x, z, y): QP i's solve by another route than kkt_solve (tests/kkt_checks.py: the refined one)"""
    zh, lam, sl, nu = [np.asarray(x, np.float64) for x in sol]
    B, n = zh.shape
    m, q = lam.shape[1], nu.shape[1]
    Q, G = _bat(arrs[0], B, 3), _bat(arrs[2], B, 3)
    A = _bat(arrs[4], B, 3) if q else np.zeros((B, 0, n))
    r = [np.zeros((B, k)) if g is None else np.asarray(g, np.float64) for g, k in zip(cots, (n, m, q))]
    d = clamp_d(lam, sl)
    if solve is None:
        solve = lambda i, rx, rz, ry: kkt_solve(Q[i], G[i], A[i], d[i], rx, rz, ry)      # noqa: E731
    out = [solve(i, r[0][i], r[1][i], r[2][i]) for i in range(B)]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def first_grads(sol, bsol):
    """the six per-QP gradients the first backward returns, from its KKT solution"""
    zh, lam, sl, nu = [np.asarray(x, np.float64) for x in sol]
    dx, dz, dy = bsol
    o = lambda u, v: u[:, :, None] * v[:, None, :]      # noqa: E731
    return (0.5 * (o(dx, zh) + o(zh, dx)), dx, o(dz, zh) + o(lam, dx), -dz, o(dy, zh) + o(nu, dx), -dy)


def second_order(arrs, sol, bsol, W, solve=None):
    """{zdot, lamdot, nudot, HQ .. Hb}, each (B, ...), at the solution sol = (zhat, lam, slacks, nu) and the first backward's
    bsol = (dx, dz, dy), for per-QP cotangents W = (W_Q, W_p, W_G, W_h, W_A, W_b), each (B, ...) or None (zero); solve: as
    first_backward's"""
    zh, lam, sl, nu = [np.asarray(x, np.float64) for x in sol]
    dx, dz, dy = [np.asarray(x, np.float64) for x in bsol]
    B, n = zh.shape
    m, q = lam.shape[1], nu.shape[1]
    Q, G = _bat(arrs[0], B, 3), _bat(arrs[2], B, 3)
    A = _bat(arrs[4], B, 3) if q else np.zeros((B, 0, n))
    shapes = ((n, n), (n,), (m, n), (m,), (q, n), (q,))
    WQ, Wp, WG, Wh, WA, Wb = [np.zeros((B,) + s) if w is None else _bat(w, B, len(s) + 1) for w, s in zip(W, shapes)]
    d = clamp_d(lam, sl)
    if solve is None:
        solve = lambda i, rx, rz, ry: kkt_solve(Q[i], G[i], A[i], d[i], rx, rz, ry)      # noqa: E731
    out = {k: [] for k in ("zdot", "lamdot", "nudot") + NAMES}
    for i in range(B):
        S = 0.5 * (WQ[i] + WQ[i].T)
        tx = S @ zh[i] + Wp[i] + WG[i].T @ lam[i] + WA[i].T @ nu[i]
        tz = WG[i] @ zh[i] - Wh[i]
        ty = WA[i] @ zh[i] - Wb[i]
        zd, ld, nd = solve(i, tx, tz, ty)
        a = dz[i] / np.maximum(lam[i], 1e-8)
        u = a * ld
        gz = S @ dx[i] + WG[i].T @ dz[i] + WA[i].T @ dy[i] + G[i].T @ u
        gl = WG[i] @ dx[i] + a * (G[i] @ zd + tz)
        gn = WA[i] @ dx[i]
        ex, ez, ey = solve(i, gz, gl, gn)
        o = np.outer
        vals = (zd, ld, nd,
                0.5 * (o(dx[i], zd) + o(zd, dx[i])) + 0.5 * (o(ex, zh[i]) + o(zh[i], ex)), ex,
                o(ld, dx[i]) + o(dz[i], zd) + o(u, zh[i]) + o(ez, zh[i]) + o(lam[i], ex), -u - ez,
                o(nd, dx[i]) + o(dy[i], zd) + o(ey, zh[i]) + o(nu[i], ex), -ey)
        for k, v in zip(out, vals):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


def random_W(B, n, m, q, seed):
    r = np.random.RandomState(seed)
    return [r.randn(B, n, n), r.randn(B, n), r.randn(B, m, n), r.randn(B, m), r.randn(B, q, n), r.randn(B, q)]


def psi(grads, W):
    """per QP: sum_i <W_i, grad_i>"""
    return sum(np.einsum("bi,bi->b", np.asarray(w).reshape(len(g), -1), np.asarray(g).reshape(len(g), -1))
               for g, w in zip(grads, W) if g is not None and w is not None and np.size(g))
