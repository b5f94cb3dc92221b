"""TEST INFRASTRUCTURE: the finishing stage (qpx_polish, include/qpx.h) step by step in numpy, NOT built from the library.

One step is one iteration of the reference's loop (qpth/solvers/pdipm/batch.py:92-198) in the original variables
(x, s, z, y) -- the sequence tests/polish_reference.py spells out in torch on the library's own solve:

  1. rx = Q x + p + G'z + A'y, rz = G x + s - h, ry = A x - b from the caller's data; mu = |s'z| / nineq;
     total = ||rx|| + ||rz|| + ||ry|| + nineq mu                                       (batch.py:93-107)
  2. d = z / s
  3. the affine solve with rs = z                                                      (batch.py:145-151)
  4. alpha_aff = min(1, min step); sigma = ((s + alpha_aff ds_a)'(z + alpha_aff dz_a) / s'z)^3;
     rs_cor = (-mu sigma + ds_a dz_a) / s                                              (batch.py:160-172)
  5. the corrector solve on zero residuals
  6. alpha = min(1, 0.999 min step)                                                    (batch.py:189-198)
  7. (x, s, z, y) += alpha (dx, ds, dz, dy)
  8. best iterate by the total, strict <, the start iterate competes, NaN never wins   (batch.py:118-139)

Both KKT solves go through kkt_checks.Dense: the dense row-scaled system, a float64 LU refined with np.longdouble residuals
(tests/test_kkt_reference.py holds it against mpmath).  Residuals, directions and the iterate are kept in np.longdouble.
`solver` selects what the two solves are, for the reference-side figures behind a gate that rests on a rule: "refined" (the
reference), "lu64" (the float64 LU alone), "f32" (a float32 dense solve of the same system).  tests/test_polish_reference.py
ties a step of this module to oracle/qp_oracle's iterates."""
import numpy as np
import torch

from kkt_checks import Dense

LD = np.longdouble


def residuals(arrs, it):
    """(rx, rz, ry, mu, total) of the iterate it = (x, s, z, y), all np.longdouble; mu and total (B,)"""
    Q, p, G, h, A, b = [np.asarray(a, LD) for a in arrs]
    x, s, z, y = it
    e = np.einsum
    rx = e("bij,bj->bi", Q, x) + p + e("bmn,bm->bn", G, z) + e("bqn,bq->bn", A, y)
    rz = e("bmn,bn->bm", G, x) + s - h
    ry = e("bqn,bn->bq", A, x) - b
    m = G.shape[1]
    mu = np.abs((s * z).sum(1)) / m
    nrm = lambda v: np.sqrt((v * v).sum(1))      # noqa: E731
    return rx, rz, ry, mu, nrm(rx) + nrm(rz) + nrm(ry) + m * mu


def step_length(v, dv):
    """min over dv < 0 of -v / dv per QP, inf where no entry shrinks"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(dv < 0, -v / np.where(dv < 0, dv, -1), np.inf)
    return r.min(1)


def _solve(D, rx, rs, rz, ry, solver):
    rhs = [v[:, None] for v in (rx, rs, rz, ry)]
    if solver == "f32":
        n, m = D.n, D.m
        r32, rzl = D.rhs(*rhs)
        sol = torch.linalg.solve(D.K64.float(), torch.from_numpy(r32.astype(np.float32)).transpose(1, 2)).transpose(1, 2).numpy().astype(LD)
        dx = sol[..., :n]
        out = dx, -rzl - np.einsum("bmn,bkn->bkm", D.G, dx), sol[..., n:n + m], sol[..., n + m:]
    else:
        out = D.solve(*rhs, rounds=0 if solver == "lu64" else 5)
    return [np.asarray(v[:, 0], LD) for v in out]


def one_step(arrs, it, solver="refined"):
    """the iterate after one step from it = (x, s, z, y)"""
    x, s, z, y = [np.asarray(v, LD) for v in it]
    rx, rz, ry, mu, _ = residuals(arrs, (x, s, z, y))
    D = Dense(np.asarray(arrs[0], np.float64), np.asarray(arrs[2], np.float64), np.asarray(arrs[4], np.float64), z / s)
    dxa, dsa, dza, dya = _solve(D, rx, z, rz, ry, solver)
    al = np.minimum(np.minimum(step_length(z, dza), step_length(s, dsa)), 1.0)[:, None]
    sig = (((s + al * dsa) * (z + al * dza)).sum(1) / (s * z).sum(1)) ** 3
    rsc = (-(mu * sig)[:, None] + dsa * dza) / s
    zero = lambda v: np.zeros(v.shape, LD)       # noqa: E731
    dxc, dsc, dzc, dyc = _solve(D, zero(rx), rsc, zero(rz), zero(ry), solver)
    dx, ds, dz, dy = dxa + dxc, dsa + dsc, dza + dzc, dya + dyc
    alpha = np.minimum(0.999 * np.minimum(step_length(z, dz), step_length(s, ds)), 1.0)[:, None]
    return x + alpha * dx, s + alpha * ds, z + alpha * dz, y + alpha * dy


def run(arrs, start, steps, solver="refined"):
    """arrs: (Q, p, G, h, A, b) batched float64 arrays, A (B, 0, n) and b (B, 0) without equalities; start: (x, s, z, y), each
    (B, .).  Returns {"iterates": [(x, s, z, y) after step 0 .. steps], "totals": (steps + 1, B), "best": (B,) the index of the
    iterate qpx_polish(steps) returns, "best_resid": (B,) its total (inf where no total is finite)}, np.longdouble."""
    it = tuple(np.asarray(v, LD) for v in start)
    iterates, totals = [it], [residuals(arrs, it)[4]]
    for _ in range(steps):
        it = one_step(arrs, it, solver)
        iterates.append(it)
        totals.append(residuals(arrs, it)[4])
    totals = np.stack(totals)
    B = totals.shape[1]
    best, best_resid = np.zeros(B, int), np.full(B, np.inf, LD)
    for k in range(steps + 1):
        better = totals[k] < best_resid          # False for NaN
        best = np.where(better, k, best)
        best_resid = np.where(better, totals[k], best_resid)
    return {"iterates": iterates, "totals": totals, "best": best, "best_resid": best_resid}
