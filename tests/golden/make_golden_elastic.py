#!/usr/bin/env python3
"""Generate tests/golden/elastic_*.npz from the REFERENCE ITSELF (locuslab/qpth at /root/reference): QPs with elastic rows
G z <= h + t, t >= 0 and the penalty gamma't + 1/2 t'diag(rho)t, solved by the unmodified reference as the AUGMENTED dense QP in
(z, t_F) (tests/elastic_reference.py: augment), float64.

Run in the build container only (the GPU box has no /root/reference):

    python tests/golden/make_golden_elastic.py

Each QP is solved alone (batch of one: the reference's stopping test is batch-global, the kernels' per QP).  Each fixture
stores, numbers only: the inputs p, h, b, rho and gamma (+inf = a hard row; the matrices are regenerated from the seed,
elastic_reference.elastic_problem, and the stored vectors pin the generator); zhat, nu, lam, slacks of the rows and lam_t,
slacks_t, t of t >= 0 (0, +inf and 0 on a hard row); c and, for the loss <c, zhat>, the gradients dQ, dp, dG, dh, dA, db, drho,
dgamma folded back (elastic_reference.fold).  The fixtures of DUALS also store seeded cotangents g_z, g_lam, g_nu of a loss on
(zhat, lam, nu) and its gradients du_*: the reference's factor_kkt + solve_kkt(g_z', 0, g_lam', g_nu) at its own solution of
the augmented QP (g' zero-padded on t and on t's rows) with the formulas of qp.py:157-173, as make_golden_duals.py does.

A fixture must have, among its elastic rows, violated rows (t > 0, lam = gamma + rho t), rows held at h with 0 < lam < gamma
(t = 0) and inactive rows -- asserted here: one without all three shows nothing -- and strict complementarity on both pairs
(max(lam, s) >= 1e-4, max(lam_t, s_t) >= 1e-4): the fixtures carry gradients.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import run_ref, save  # noqa: E402  (stubs cvxpy, imports the reference)

import torch  # noqa: E402
import qpth.solvers.pdipm.batch as pdipm_b  # noqa: E402
from qpth.util import bger  # noqa: E402

import elastic_reference as R  # noqa: E402

ACTIVE = 1e-6
DUALS = ("t1b",)
GRADS = ("dQ", "dp", "dG", "dh", "dA", "db", "drho", "dgamma")


def duals_ref(Q2, p2, G2, h2, A2, b, gz2, gl2, gn):
    """the reference's general KKT solve at its own solution: gradients of a loss on (x, lam', nu) with cotangents gz2, gl2, gn"""
    t = lambda x: torch.tensor(np.asarray(x))[None] if np.size(x) else torch.Tensor().double()  # noqa: E731
    Q, p, G, h, A, bb = t(Q2), t(p2), t(G2), t(h2), t(A2), t(b)
    q = A.shape[1] if A.nelement() else 0
    with torch.no_grad():
        Q_LU, S_LU, Rm = pdipm_b.pre_factor_kkt(Q, G, A)
        zh, nu, lam, sl = pdipm_b.forward(Q, p, G, h, A, bb, Q_LU, S_LU, Rm, 1e-12, -1, 3, 20)
        d = torch.clamp(lam, min=1e-8) / torch.clamp(sl, min=1e-8)
        pdipm_b.factor_kkt(S_LU, Rm, d)
        dx, _, dz, dy = pdipm_b.solve_kkt(Q_LU, d, G, A, S_LU, t(gz2), torch.zeros_like(lam), t(gl2), t(gn) if q else torch.Tensor().double())
        g = {"dQ": 0.5 * (bger(dx, zh) + bger(zh, dx)), "dp": dx, "dG": bger(dz, zh) + bger(lam, dx), "dh": -dz}
        if q:
            g["dA"] = bger(dy, zh) + bger(nu, dx)
            g["db"] = -dy
    return {k: v[0].numpy() for k, v in g.items()}


def case(label, kind):
    Q, p, G, h, A, b, rho, gamma = R.elastic_problem(label, kind)
    B, n, m, q = R.SHAPES[label]
    c = R.loss_vector(label)
    keys = ("zhat", "nu", "lam", "slacks", "lam_t", "slacks_t", "t") + GRADS
    out = {k: [] for k in keys}
    du = {"du_" + k: [] for k in GRADS}
    rc = np.random.RandomState(R.SEED + 5)
    g_z, g_lam, g_nu = rc.randn(B, n), rc.randn(B, m), rc.randn(B, q)
    for i in range(B):
        Q2, p2, G2, h2, A2, F = R.augment(Q[i], p[i], G[i], h[i], A[i] if q else A, gamma[i], rho[i])
        k = F.size
        o = run_ref(Q2[None], p2[None], G2[None], h2[None], A2[None] if q else A2, b[i][None] if q else b,
                    dl=np.concatenate([c[i], np.zeros(k)])[None])
        lam, lam_t = R.split(o["lam"][0], F, m, 0.0)
        sl, sl_t = R.split(o["slacks"][0], F, m, np.inf)
        tt = np.zeros(m)
        tt[F] = o["zhat"][0][n:]
        dA2 = o["dA"][0] if q else np.zeros((0, n))
        folded = R.fold(o["dQ"][0], o["dp"][0], o["dG"][0], o["dh"][0], dA2, F, n, m)
        vals = (o["zhat"][0][:n], o["nu"][0], lam, sl, lam_t, sl_t, tt) + folded[:5] + (o["db"][0] if q else np.zeros(0),) + folded[5:]
        for kk, v in zip(keys, vals):
            out[kk].append(v)
        if label in DUALS:
            g = duals_ref(Q2, p2, G2, h2, A2, b[i] if q else b, np.concatenate([g_z[i], np.zeros(k)]),
                          np.concatenate([g_lam[i], np.zeros(k)]), g_nu[i])
            f = R.fold(g["dQ"], g["dp"], g["dG"], g["dh"], g["dA"] if q else np.zeros((0, n)), F, n, m)
            for kk, v in zip(GRADS, f[:5] + (g["db"] if q else np.zeros(0),) + f[5:]):
                du["du_" + kk].append(v)
    out = {k: np.stack(v) for k, v in out.items()}
    el = np.isfinite(gamma) & np.isfinite(rho)
    viol = el & (out["t"] > ACTIVE)
    held = el & (out["t"] < ACTIVE) & (out["lam"] > ACTIVE) & (out["lam"] < gamma - ACTIVE)
    inact = el & (out["lam"] < ACTIVE)
    print("%-4s %-4s elastic rows violated %3d, held at h %3d, inactive %3d" % (label, kind, viol.sum(), held.sum(), inact.sum()))
    assert viol.any() and held.any() and inact.any(), (label, kind)
    assert np.abs(out["lam"] - gamma - rho * out["t"])[viol].max() < 1e-8
    weak = (np.maximum(out["lam"], out["slacks"]) < 1e-4) | (np.maximum(out["lam_t"], out["slacks_t"]) < 1e-4)
    assert not weak.any(), (label, kind, np.argwhere(weak))
    extra = {}
    if label in DUALS:
        extra = dict(g_z=g_z, g_lam=g_lam, g_nu=g_nu, **{k: np.stack(v) for k, v in du.items()})
    save(R.fixture_name(label, kind), p=p, h=h, b=b, rho=rho, gamma=gamma, c=c, **out, **extra)


def main():
    # (one thread: torch.linalg.lu_factor with more hangs in the build container's MKL from order 160 up, see make_golden.py)
    torch.set_num_threads(1)
    only = sys.argv[1:]
    for label in R.SHAPES:
        if only and label not in only:
            continue
        for kind in R.KINDS:
            case(label, kind)


if __name__ == "__main__":
    main()
