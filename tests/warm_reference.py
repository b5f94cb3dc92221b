"""Float64 numpy reference of the warm-started PDIPM loop (KKTFactors.ipm(warm=...), qpx_ipm_warm), shared by
tests/test_emu_warm.py and tests/test_gpu_warm.py: the reference's loop (batch.py:92-207) restated one QP at a time with a
dense solve of the full KKT system per step, entered either at the reference's own start point (batch.py:61-87) or at a
given (lam0, s0).

The warm entry: z = max(lam0, f), s = max(s0, f) and (x, y) from  [[Q, A^T], [A, 0]] (x, y) = (-p - G^T z, b)  -- the
dual-feasible, equality-feasible point the condensed formulation implies for that z: rx = ry = 0 there, and
stay 0, so the only residual left is rz = G x + s - h.

The stop is per QP, by the library's `stall_policy` (include/qpx.h): 0 never on stall, 1 the reference's not-improved
counter as it behaves for a batch of one, 2 the round-off floor rule.  `iters` counts the passes that evaluated the
residuals, the stopping one included, as the kernels and the oracle do.
"""
import numpy as np

# the inputs of the warm-start tests: generator seed, the seed of the perturbation, the floor
SEED, PERTURB_SEED, FLOOR = 11, 7, 1e-2
# (B, nz, nineq, neq) of the table in DESIGN 4.7
TABLE_SHAPES = ((2, 12, 9, 3), (1, 40, 52, 0), (2, 20, 70, 3), (2, 40, 52, 0), (2, 64, 64, 0), (4, 100, 100, 0), (4, 100, 50, 10))


def perturb(arrs, delta, seed=PERTURB_SEED):
    """p' = p + delta randn, h' = h + delta rand (h only loosens: the generator's z0 stays feasible); p first, then h"""
    Q, p, G, h, A, b = arrs
    r = np.random.RandomState(seed)
    p2 = p + delta * r.randn(*p.shape)
    h2 = h + delta * r.rand(*h.shape)
    return Q, p2.astype(p.dtype), G, h2.astype(h.dtype), A, b


def _solve_kkt(Q, G, A, d, rx, rs, rz, ry):
    """solve_kkt (batch.py:349-372) as one dense solve:
        Q dx + G^T dz + A^T dy = -rx,   D ds + dz = -rs,   G dx + ds = -rz,   A dx = -ry;   unknowns (dx, ds, dz, dy)"""
    m, n = G.shape
    q = A.shape[0]
    N = n + 2 * m + q
    K = np.zeros((N, N))
    K[:n, :n] = Q
    K[:n, n + m:n + 2 * m] = G.T
    K[n:n + m, n:n + m] = np.diag(d)
    K[n:n + m, n + m:n + 2 * m] = np.eye(m)
    K[n + m:n + 2 * m, :n] = G
    K[n + m:n + 2 * m, n:n + m] = np.eye(m)
    if q:
        K[:n, n + 2 * m:] = A.T
        K[n + 2 * m:, :n] = A
    v = np.linalg.solve(K, -np.concatenate([rx, rs, rz, ry]))
    return v[:n], v[n:n + m], v[n + m:n + 2 * m], v[n + 2 * m:]


def _get_step(v, dv):
    """get_step (batch.py:210-213) for a batch of one"""
    with np.errstate(divide="ignore", invalid="ignore"):
        a = -v / dv
    a = np.where(dv > 0, max(1.0, a.max()), a)
    return a.min()


def implied_xy(Q, p, G, A, b, z):
    """(x, y) of  [[Q, A^T], [A, 0]] (x, y) = (-p - G^T z, b)"""
    n, q = Q.shape[0], A.shape[0]
    K = np.zeros((n + q, n + q))
    K[:n, :n] = Q
    if q:
        K[:n, n:] = A.T
        K[n:, :n] = A
    v = np.linalg.solve(K, np.concatenate([-p - G.T @ z, b]))
    return v[:n], v[n:]


def _one(Q, p, G, h, A, b, lam0, s0, floor, eps, maxIter, notImprovedLim, stall_policy):
    m, n = G.shape
    q = A.shape[0]
    if lam0 is None:
        # batch.py:61-87
        x, s, z, y = _solve_kkt(Q, G, A, np.ones(m), p, np.zeros(m), -h, -b)
        if s.min() < 0:
            s = s - (s.min() - 1)
        if z.min() < 0:
            z = z - (z.min() - 1)
    else:
        z, s = np.maximum(lam0, floor), np.maximum(s0, floor)
        x, y = implied_xy(Q, p, G, A, b, z)
    best = None
    bres = np.inf
    nnot = floor_hit = 0
    feas_prev = alpha_prev = 0.0
    trace, iters = [], 0
    for it in range(maxIter):
        rx = (A.T @ y if q else 0.0) + G.T @ z + Q @ x + p
        rs = z
        rz = G @ x + s - h
        ry = A @ x - b if q else np.zeros(0)
        mu = abs((s * z).sum() / m)
        pri = np.linalg.norm(rz) + (np.linalg.norm(ry) if q else 0.0)
        dual = np.linalg.norm(rx)
        feas = pri + dual
        resid = feas + m * mu
        trace.append((pri, dual, mu))
        iters = it + 1
        better = it == 0 or resid < bres
        if better:
            bres, nnot = resid, 0
            best = (x.copy(), y.copy(), z.copy(), s.copy())
        elif stall_policy == 1 or (stall_policy == 2 and m * mu < feas):
            nnot += 1
        else:
            nnot = 0
        if stall_policy == 2 and it >= 1 and feas > 2.0 * (1.0 - alpha_prev) * feas_prev:
            floor_hit = 1
        feas_prev = feas
        if (stall_policy != 0 and nnot >= notImprovedLim) or bres < eps or mu > 1e32:
            break
        if stall_policy == 2 and floor_hit and m * mu < 1e-2 * feas:
            break
        if not np.isfinite(resid):
            break
        d = z / s
        dxa, dsa, dza, dya = _solve_kkt(Q, G, A, d, rx, rs, rz, ry)
        alpha = min(_get_step(z, dza), _get_step(s, dsa), 1.0)
        sig = (((s + alpha * dsa) * (z + alpha * dza)).sum() / (s * z).sum()) ** 3
        rs2 = (-mu * sig + dsa * dza) / s
        dxc, dsc, dzc, dyc = _solve_kkt(Q, G, A, d, np.zeros(n), rs2, np.zeros(m), np.zeros(q))
        dx, ds, dz, dy = dxa + dxc, dsa + dsc, dza + dzc, dya + dyc
        alpha = min(0.999 * min(_get_step(z, dz), _get_step(s, ds)), 1.0)
        alpha_prev = alpha
        x, s, z, y = x + alpha * dx, s + alpha * ds, z + alpha * dz, y + alpha * dy
    return best, iters, bres, trace


def solve(Q, p, G, h, A, b, lam0=None, s0=None, floor=FLOOR, eps=1e-12, maxIter=20, notImprovedLim=3, stall_policy=1):
    """The batch, one QP at a time.  lam0, s0 (B, nineq) or None (the reference's cold start).  Returns a dict:
    zhat (B,n), nu (B,q), lam, slacks (B,m): the best iterate;  iters (B,);  best_resid (B,);
    trace: per QP the list of (pri_resid, dual_resid, mu), one triple per pass."""
    Q, p, G, h = (np.asarray(X, np.float64) for X in (Q, p, G, h))
    B, m, n = G.shape
    q = A.shape[1] if np.size(A) else 0
    A = np.asarray(A, np.float64).reshape(B, q, n) if q else np.zeros((B, 0, n))
    b = np.asarray(b, np.float64).reshape(B, q) if q else np.zeros((B, 0))
    out = dict(zhat=np.zeros((B, n)), nu=np.zeros((B, q)), lam=np.zeros((B, m)), slacks=np.zeros((B, m)),
               iters=np.zeros(B, np.int32), best_resid=np.zeros(B), trace=[])
    for i in range(B):
        l0 = None if lam0 is None else np.asarray(lam0[i], np.float64)
        s0i = None if lam0 is None else np.asarray(s0[i], np.float64)
        best, iters, bres, trace = _one(Q[i], p[i], G[i], h[i], A[i], b[i], l0, s0i, floor, eps, maxIter, notImprovedLim, stall_policy)
        out["zhat"][i], out["nu"][i], out["lam"][i], out["slacks"][i] = best
        out["iters"][i], out["best_resid"][i] = iters, bres
        out["trace"].append(trace)
    return out
