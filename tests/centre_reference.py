"""Float64 reference of the barrier-smoothed QP, shared by tests/test_centre_reference.py, tests/test_emu_centre.py
and tests/test_gpu_centre.py (numpy, on the host, dense solves per QP).

The point of the central path at kappa > 0 (per row):

    Q z + p + G' lam + A' nu = 0,   G z + s = h,   A z = b,   s_i lam_i = kappa_i   (s, lam > 0)

`centre` finds it by a damped Newton method on the full (z, s, lam, nu) system with dense KKT solves -- started from a few
predictor-corrector interior-point iterations so that the iterate is near the path -- and runs until `residual` <= 1e-13 or
until it stops falling (the floor of float64 on the data).  `residual` is the stop test of qpx_centre:

    res = max(|rx|_inf, |rz|_inf, |ry|_inf, max_i |s_i lam_i - kappa_i| / kappa_i)

Derivatives at a centred point are those of tests/hvp_reference.py (first_backward / first_grads / second_order: d = lam / s
holds as it stands), plus d loss / d kappa_i = dz_i / lam_i with dz the inequality block of the backward's KKT solution."""
import numpy as np

from hvp_reference import first_backward, first_grads


def _kkt(Q, G, A, d, rx, rs, rz, ry):
    """(dx, ds, dz, dy) of  Q dx + G'dz + A'dy = -rx,  d ds + dz = -rs,  G dx + ds = -rz,  A dx = -ry,  d = lam / s"""
    n, m, q = Q.shape[0], G.shape[0], A.shape[0]
    K = np.zeros((n + 2 * m + q,) * 2)
    K[:n, :n], K[:n, n + m:n + 2 * m], K[:n, n + 2 * m:] = Q, G.T, A.T
    K[n:n + m, n:n + m], K[n:n + m, n + m:n + 2 * m] = np.diag(d), np.eye(m)
    K[n + m:n + 2 * m, :n], K[n + m:n + 2 * m, n:n + m] = G, np.eye(m)
    K[n + 2 * m:, :n] = A
    w = np.linalg.solve(K, -np.concatenate([rx, rs, rz, ry]))
    return w[:n], w[n:n + m], w[n + m:n + 2 * m], w[n + 2 * m:]


def _to_boundary(v, dv):
    neg = dv < 0
    return min(1.0, float((-v[neg] / dv[neg]).min())) if neg.any() else 1.0


def _start(Q, p, G, h, A, b, eps, max_iter=40):
    """predictor-corrector interior-point iterations until ||rx|| + ||rz|| + ||ry|| + m mu < eps: an iterate near the path"""
    n, m, q = Q.shape[0], G.shape[0], A.shape[0]
    x, s, z, y = _kkt(Q, G, A, np.ones(m), p, np.zeros(m), -h, -b)
    if z.min() < 0:
        z = z + 1 - z.min()
    if s.min() < 0:
        s = s + 1 - s.min()
    for _ in range(max_iter):
        rx, rz, ry = A.T @ y + G.T @ z + Q @ x + p, G @ x + s - h, A @ x - b
        mu = abs(s @ z) / m
        if np.linalg.norm(rx) + np.linalg.norm(rz) + np.linalg.norm(ry) + m * mu < eps:
            break
        d = z / s
        dxa, dsa, dza, dya = _kkt(Q, G, A, d, rx, z, rz, ry)
        al = min(_to_boundary(z, dza), _to_boundary(s, dsa))
        sig = ((s + al * dsa) @ (z + al * dza) / (s @ z)) ** 3
        dxc, dsc, dzc, dyc = _kkt(Q, G, A, d, np.zeros(n), (-mu * sig + dsa * dza) / s, np.zeros(m), np.zeros(q))
        dx, ds, dz, dy = dxa + dxc, dsa + dsc, dza + dzc, dya + dyc
        al = min(0.999 * min(_to_boundary(z, dz), _to_boundary(s, ds)), 1.0)
        x, s, z, y = x + al * dx, s + al * ds, z + al * dz, y + al * dy
    return x, s, z, y


def _res1(Q, p, G, h, A, b, x, s, z, y, kappa):
    rx, rz, ry = A.T @ y + G.T @ z + Q @ x + p, G @ x + s - h, A @ x - b
    rc = s * z - kappa
    res = max(np.abs(rx).max(), np.abs(rz).max(), np.abs(ry).max() if ry.size else 0.0, np.abs(rc / kappa).max())
    return rx, rz, ry, rc, float(res) if np.isfinite(res) else np.inf


def _centre1(Q, p, G, h, A, b, kappa, start, tol, max_steps):
    x, s, z, y = start if start is not None else _start(Q, p, G, h, A, b, G.shape[0] * kappa.min())
    best, stall, k = np.inf, 0, 0
    while True:
        rx, rz, ry, rc, res = _res1(Q, p, G, h, A, b, x, s, z, y, kappa)
        stall = 0 if (res < 0.5 * best or res > 1e-9) else stall + 1       # (only near the floor: far out, damped steps are slow)
        best = min(best, res)
        if res <= tol or k == max_steps or stall >= 3:
            return x, s, z, y, k, res
        dx, ds, dz, dy = _kkt(Q, G, A, z / s, rx, rc / s, rz, ry)
        al = min(_to_boundary(z, dz), _to_boundary(s, ds))
        al = 1.0 if al >= 1.0 else 0.99 * al
        x, s, z, y = x + al * dx, s + al * ds, z + al * dz, y + al * dy
        k += 1


def _batched(arrs, B):
    Q, p, G, h, A, b = [np.asarray(a, np.float64) for a in arrs]
    n = G.shape[-1]
    out = []
    for X, nd in ((Q, 3), (p, 2), (G, 3), (h, 2)):
        out.append(np.broadcast_to(X, (B,) + X.shape[-(nd - 1):]) if X.ndim == nd - 1 or X.shape[0] == 1 else X)
    if A.size:
        out.append(np.broadcast_to(A, (B,) + A.shape[-2:]) if A.ndim == 2 or A.shape[0] == 1 else A)
        out.append(np.broadcast_to(b, (B,) + b.shape[-1:]) if b.ndim == 1 or b.shape[0] == 1 else b)
    else:
        out += [np.zeros((B, 0, n)), np.zeros((B, 0))]
    return [out[i] for i in (0, 1, 2, 3, 4, 5)]


def kappa_rows(kappa, B, m):
    """kappa as (B, m) from (B, m), (m,), () or a float"""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(kappa, np.float64), (B, m)))


def centre(arrs, kappa, B=None, start=None, tol=1e-13, max_steps=100):
    """The central-path point of every QP: (zhat, lam, s, nu), each (B, .), the Newton steps taken (B,) and the final
    residuals (B,).  arrs = (Q, p, G, h, A, b), batched or not (A, b empty: no equalities); kappa (B, m), (m,) or a float;
    start: (zhat, lam, s, nu), each (B, .), to start Newton's method from instead of the interior-point iterations."""
    if B is None:
        B = max([np.asarray(a).shape[0] for a, nd in zip(arrs, (3, 2, 3, 2, 3, 2)) if np.asarray(a).ndim == nd and np.size(a)] + [1])
    Q, p, G, h, A, b = _batched(arrs, B)
    kap = kappa_rows(kappa, B, G.shape[1])
    out = []
    for i in range(B):
        st = None if start is None else (start[0][i], start[2][i], start[1][i], start[3][i])
        out.append(_centre1(Q[i], p[i], G[i], h[i], A[i], b[i], kap[i], st, tol, max_steps))
    x, s, z, y = [np.stack([o[k] for o in out]) for k in range(4)]
    return (x, z, s, y), np.array([o[4] for o in out]), np.array([o[5] for o in out])


def residual(arrs, sol, kappa):
    """(B,): the stop test's residual of sol = (zhat, lam, s, nu) at kappa"""
    x, z, s, y = [np.asarray(v, np.float64) for v in sol]
    B = x.shape[0]
    Q, p, G, h, A, b = _batched(arrs, B)
    kap = kappa_rows(kappa, B, G.shape[1])
    yy = y if y.size else np.zeros((B, 0))
    return np.array([_res1(Q[i], p[i], G[i], h[i], A[i], b[i], x[i], s[i], z[i], yy[i], kap[i])[4] for i in range(B)])


def grads(arrs, sol, cots):
    """The first-order derivatives at a centred point sol = (zhat, lam, s, nu) for cotangents cots = (r_z, r_lam, r_nu), None =
    zero: (six per-QP gradients dQ .. db, dkappa (B, m), the backward's KKT solution (dx, dz, dy))"""
    B = np.asarray(sol[0]).shape[0]
    full = _batched(arrs, B)
    sol = [np.asarray(v, np.float64) for v in sol]
    if not sol[3].size:
        sol[3] = np.zeros((B, 0))
    bsol = first_backward(full, sol, cots)
    return first_grads(sol, bsol), bsol[1] / sol[1], bsol
