"""The reference of tests/kkt_checks.py against arithmetic it cannot share an error with: kkt_checks.Dense.solve (float64 LU,
residuals in np.longdouble, five rounds of refinement) against a 50-digit mpmath LU solve of the same row-scaled KKT system,
with d drawn log-uniformly from 1e-8 to 1e8 (the sixteen decades of the backward's d).  The difference is scaled by
max(1, max |ref|) per block, as every gate of kkt_checks is; it must stay REF_TOL = 1e-11, 1e3 below the tightest of them.
Measured: (12, 9, 3) 2.5e-19, (20, 40, 4) 3.5e-19 (the unrefined float64 solve: 3e-15 at (12, 9, 3)).  mpmath's LU costs
seconds from a hundred unknowns on (23 s at (100, 100, 0), measured 2e-18 there once): these two shapes only."""
import mpmath
import numpy as np
import pytest

import kkt_checks as C
import problems


@pytest.mark.parametrize("shape", [(12, 9, 3), (20, 40, 4)], ids=lambda s: C.tag(s))
def test_refined_dense_solve_against_mpmath(shape):
    n, m, q = shape
    Q, _, G, _, A, _ = problems.prof_qp(1, n, m, q, seed=C.SEED)
    A = A if q else np.zeros((1, 0, n))
    r = np.random.RandomState(5)
    d = 10.0 ** r.uniform(-8, 8, (1, m))
    rhs = [r.randn(1, 1, k) for k in (n, m, m, q)]
    D = C.Dense(Q, G, A, d)
    ref = D.solve(*rhs)
    raw = D.solve(*rhs, rounds=0)
    with mpmath.workdps(50):
        N = n + m + q
        K = mpmath.zeros(N, N)
        for i in range(n):
            for j in range(n):
                K[i, j] = mpmath.mpf(Q[0, i, j])
            for j in range(m):
                K[i, n + j] = mpmath.mpf(G[0, j, i])
                K[n + j, i] = mpmath.mpf(d[0, j]) * mpmath.mpf(G[0, j, i])
            for j in range(q):
                K[i, n + m + j] = K[n + m + j, i] = mpmath.mpf(A[0, j, i])
        for j in range(m):
            K[n + j, n + j] = mpmath.mpf(-1)
        b = [-mpmath.mpf(v) for v in rhs[0][0, 0]]
        b += [-(mpmath.mpf(d[0, j]) * mpmath.mpf(rhs[2][0, 0, j]) - mpmath.mpf(rhs[1][0, 0, j])) for j in range(m)]
        b += [-mpmath.mpf(v) for v in rhs[3][0, 0]]
        x = mpmath.lu_solve(K, mpmath.matrix(b))
        dx = [x[i] for i in range(n)]
        ds = [-mpmath.mpf(rhs[2][0, 0, j]) - mpmath.fsum(mpmath.mpf(G[0, j, i]) * dx[i] for i in range(n)) for j in range(m)]
        exact = [dx, ds, [x[n + j] for j in range(m)], [x[n + m + j] for j in range(q)]]

        def gap(mine):
            worst = 0.0
            for a, e in zip(mine, exact):
                if e:
                    scale = max(mpmath.mpf(1), max(abs(v) for v in e))
                    worst = max(worst, float(max(abs(mpmath.mpf(float(v)) + mpmath.mpf(float(v - C.LD(float(v)))) - t)
                                                 for v, t in zip(a[0, 0], e)) / scale))
            return worst

        refined, unrefined = gap(ref), gap(raw)
    print("refined reference against mpmath %.2e, the float64 LU solve alone %.2e" % (refined, unrefined))
    assert refined <= C.REF_TOL, refined
