#!/usr/bin/env python3
"""Generate tests/golden/duals_*.npz from the REFERENCE ITSELF (locuslab/qpth at /root/reference): gradients of a loss that
depends on the multipliers, l(zhat, lam, nu).

Run in the build container only (the GPU box has no /root/reference):

    python tests/golden/make_golden_duals.py

The reference's QPFunction.backward only takes dl/dzhat (qp.py:151-155: solve_kkt(dl_dzhat, 0, 0, 0)).  Its solver entry
points, imported unmodified as in make_golden.py (cvxpy stubbed), do the general solve: after the reference forward this
script calls factor_kkt + solve_kkt(g_z, 0, g_lam, g_nu) with seeded cotangents and applies the formulas of qp.py:157-173
(bger) to the resulting (dx, dlam, dnu).  Each fixture stores, numbers only,

  zhat, nu, lam, slacks ....... the reference forward (batch.py:47-207)
  g_z, g_lam, g_nu ............ the cotangents
  dQ, dp, dG, dh, dA, db ...... the gradients, per QP
  lu_vs_dense_gap ............. the reference's own noise: max over QPs and gradients of the relative distance between
                                these gradients and the ones formed from a dense float64 numpy solve of the same 4-block KKT
                                system (lu_vs_dense_gap_per_grad: the same per gradient) -- the tests derive the tolerance
                                of their dense-solve comparison from it (tests/test_emu_duals.py)

and duals_fd_*.npz: central finite differences (eps = 1e-6) of the reference forward's (zhat, lam, nu) along seeded tangents
tQ (symmetric), tp, tG, th, tA, tb of all six parameters, stored with the tangents -- fd_z, fd_lam, fd_nu.
"""
import os
import sys
import types

import numpy as np

sys.modules.setdefault("cvxpy", types.ModuleType("cvxpy"))
sys.path.insert(0, "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402
import qpth  # noqa: E402,F401
import qpth.solvers.pdipm.batch as pdipm_b  # noqa: E402
from qpth.util import bger  # noqa: E402

import problems  # noqa: E402
from make_golden import checksum, save  # noqa: E402

NAMES = ("dQ", "dp", "dG", "dh", "dA", "db")


def formulas(zh, lam, nu, dx, dz, dy):
    """qp.py:157-173 on torch tensors (dy / nu None without equality constraints)"""
    g = {"dQ": 0.5 * (bger(dx, zh) + bger(zh, dx)), "dp": dx, "dG": bger(dz, zh) + bger(lam, dx), "dh": -dz}
    if dy is not None:
        g["dA"] = bger(dy, zh) + bger(nu, dx)
        g["db"] = -dy
    return g


def dense_solution(Q, G, A, d, gz, gl, gn):
    """(dx, dz, dy) of K sol = -(g_z, 0, g_lam, g_nu) by numpy.linalg.solve on the 4-block matrix of batch.py:313-346,
    unknowns ordered (x, s, z, y)"""
    B, m, n = G.shape
    q = A.shape[1] if A is not None else 0
    dx, dz, dy = np.empty((B, n)), np.empty((B, m)), np.empty((B, q))
    for i in range(B):
        N = n + 2 * m + q
        K = np.zeros((N, N))
        K[:n, :n] = Q[i]
        K[:n, n + m:n + 2 * m] = G[i].T
        K[n:n + m, n:n + m] = np.diag(d[i])
        K[n:n + m, n + m:n + 2 * m] = np.eye(m)
        K[n + m:n + 2 * m, :n] = G[i]
        K[n + m:n + 2 * m, n:n + m] = np.eye(m)
        if q:
            K[:n, n + 2 * m:] = A[i].T
            K[n + 2 * m:, :n] = A[i]
        r = np.concatenate([gz[i], np.zeros(m), gl[i], gn[i] if q else np.zeros(0)])
        x = np.linalg.solve(K, -r)
        dx[i], dz[i], dy[i] = x[:n], x[n + m:n + 2 * m], x[n + 2 * m:]
    return dx, dz, dy


def case(name, arrs, seed, store_inputs):
    Q, p, G, h, A, b = [torch.tensor(np.asarray(x)) for x in arrs]
    B, m, n = G.shape
    q = A.shape[1] if A.nelement() else 0
    if q == 0:
        A = b = torch.Tensor().double()
    with torch.no_grad():
        Q_LU, S_LU, R = pdipm_b.pre_factor_kkt(Q, G, A)
        zh, nu, lam, sl = pdipm_b.forward(Q, p, G, h, A, b, Q_LU, S_LU, R, 1e-12, -1, 3, 20)
        r = np.random.RandomState(seed)
        gz, gl, gn = r.randn(B, n), r.randn(B, m), r.randn(B, q)
        d = torch.clamp(lam, min=1e-8) / torch.clamp(sl, min=1e-8)                      # qp.py:148
        pdipm_b.factor_kkt(S_LU, R, d)
        dx, _, dz, dy = pdipm_b.solve_kkt(Q_LU, d, G, A, S_LU, torch.tensor(gz), torch.zeros(B, m).double(), torch.tensor(gl),
                                          torch.tensor(gn) if q else torch.Tensor().double())
        grads = {k: v.numpy().copy() for k, v in formulas(zh, lam, nu if q else None, dx, dz, dy if q else None).items()}
        # the reference's own noise: the same formulas on a dense solve of the same system
        ddx, ddz, ddy = dense_solution(Q.numpy(), G.numpy(), A.numpy() if q else None, d.numpy(), gz, gl, gn)
        dense = formulas(zh, lam, nu if q else None, torch.tensor(ddx), torch.tensor(ddz), torch.tensor(ddy) if q else None)
    gaps = []
    for k in NAMES:
        if k in grads:
            a, c = grads[k].reshape(B, -1), dense[k].numpy().reshape(B, -1)
            gaps.append((np.linalg.norm(a - c, axis=1) / np.linalg.norm(c, axis=1)).max())
    extra = dict(zip(("Q", "p", "G", "h", "A", "b"), arrs)) if store_inputs else {}
    save(name, input_checksum=checksum(*arrs), zhat=zh.numpy(), lam=lam.numpy(), slacks=sl.numpy(),
         nu=nu.numpy() if q else np.zeros((B, 0)), g_z=gz, g_lam=gl, g_nu=gn,
         lu_vs_dense_gap=np.array(max(gaps)), lu_vs_dense_gap_per_grad=np.array(gaps), **extra, **grads)
    print("    LU vs dense: %.2e  (%s)" % (max(gaps), " ".join("%.1e" % g for g in gaps)))


def reference_forward(arrs):
    Q, p, G, h, A, b = [torch.tensor(np.asarray(x)) for x in arrs]
    if A.nelement() == 0:
        A = b = torch.Tensor().double()
    with torch.no_grad():
        Q_LU, S_LU, R = pdipm_b.pre_factor_kkt(Q, G, A)
        zh, nu, lam, _ = pdipm_b.forward(Q, p, G, h, A, b, Q_LU, S_LU, R, 1e-12, -1, 3, 20)
    return zh.numpy(), lam.numpy(), (nu.numpy() if A.nelement() else np.zeros((zh.shape[0], 0)))


def fd_case(name, arrs, seed, eps=1e-6):
    r = np.random.RandomState(seed)
    tans = []
    for k, x in zip("QpGhAb", arrs):
        t = r.randn(*np.shape(x)) if np.size(x) else np.zeros(0)
        tans.append(0.5 * (t + np.swapaxes(t, -1, -2)) if k == "Q" else t)
    plus = reference_forward([np.asarray(x) + eps * t for x, t in zip(arrs, tans)])
    minus = reference_forward([np.asarray(x) - eps * t for x, t in zip(arrs, tans)])
    fd = [(a - c) / (2 * eps) for a, c in zip(plus, minus)]
    save(name, eps=np.array(eps), input_checksum=checksum(*arrs), fd_z=fd[0], fd_lam=fd[1], fd_nu=fd[2],
         **{"t" + k: t for k, t in zip("QpGhAb", tans)})


def main():
    # (one thread: torch.linalg.lu_factor with more hangs in the build container's MKL from order 160 up, see make_golden.py)
    torch.set_num_threads(1)
    case("duals_b4_n100_m100", problems.prof_qp(4, 100, 100, 0, 0), 31, False)
    case("duals_b4_n100_m50_q10", problems.prof_qp(4, 100, 50, 10, 0), 32, False)
    case("duals_b2_n12_m9_q3", problems.random_dense_qp(2, 12, 9, 3, seed=24), 33, True)
    fd_case("duals_fd_b2_n10_m8", problems.random_dense_qp(2, 10, 8, 0, seed=24), 25)
    fd_case("duals_fd_b2_n12_m9_q3", problems.random_dense_qp(2, 12, 9, 3, seed=24), 25)


if __name__ == "__main__":
    main()
