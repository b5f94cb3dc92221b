#!/usr/bin/env python3
"""Generate tests/golden/softrange_*.npz from the REFERENCE ITSELF (locuslab/qpth at /root/reference): QPs with soft two-sided
rows l - tl <= G z <= h + tu, tu, tl >= 0 and the penalty gamma t + 1/2 rho t^2 on each side, solved by the unmodified reference
as the AUGMENTED dense QP in (z, tu, tl) (tests/soft_range_reference.py: augment), float64.

Run in the build container only (the GPU box has no /root/reference):

    python tests/golden/make_golden_soft_range.py [label ...]

Each QP is solved alone (batch of one: the reference's stopping test is batch-global, the kernels' per QP).  Each fixture
stores, numbers only: the inputs p, h, b, lower, gamma_u, rho_u, gamma_l, rho_l (the matrices are regenerated from the seed,
soft_range_reference.soft_range_problem, and the stored vectors pin the generator); zhat, nu, the four multiplier / slack pairs
lam, slacks (upper rows), lam_lo, slacks_lo (lower rows), lam_t, slacks_t (tu >= 0), lam_tl, slacks_tl (tl >= 0), t and t_lo
(0, +inf and 0 where a side is absent); c and, for the loss <c, zhat>, the gradients dQ, dp, dG, dh, dA, db, dlower, dgamma_u,
drho_u, dgamma_l, drho_l folded back (soft_range_reference.fold).

A fixture must have, over its batch, a row violated upwards (tu > 0), one violated downwards (tl > 0), a row held at h and one
held at lower (t = 0 with a multiplier), a row strictly inside -- asserted here: one without all five shows nothing -- and
strict complementarity on all four pairs of every row (max(lam, s) >= 1e-4): the fixtures carry gradients.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import run_ref, save  # noqa: E402  (stubs cvxpy, imports the reference)

import torch  # noqa: E402

import soft_range_reference as R  # noqa: E402

ACTIVE = 1e-6
PAIRS = (("lam", "slacks"), ("lam_lo", "slacks_lo"), ("lam_t", "slacks_t"), ("lam_tl", "slacks_tl"))
GRADS = ("dQ", "dp", "dG", "dh", "dA", "db", "dlower", "dgamma_u", "drho_u", "dgamma_l", "drho_l")


def case(label, kind):
    arrs = R.soft_range_problem(label, kind)
    Q, p, G, h, A, b = arrs[:6]
    B, n, m, q = R.SHAPES[label]
    c = R.loss_vector(label)
    keys = ("zhat", "nu") + tuple(k for pair in PAIRS for k in pair) + ("t", "t_lo") + GRADS
    out = {k: [] for k in keys}
    for i in range(B):
        Q2, p2, G2, h2, A2, sets = R.augment(Q[i], p[i], G[i], h[i], A[i] if q else A, *[x[i] for x in arrs[6:]])
        k = Q2.shape[0] - n
        o = run_ref(Q2[None], p2[None], G2[None], h2[None], A2[None] if q else A2, b[i][None] if q else b,
                    dl=np.concatenate([c[i], np.zeros(k)])[None])
        lam = R.split(o["lam"][0], sets, m, 0.0)
        sl = R.split(o["slacks"][0], sets, m, np.inf)
        z, tu, tl = R.split_t(o["zhat"][0], sets, n, m)
        dA2 = o["dA"][0] if q else np.zeros((0, n))
        f = R.fold(o["dQ"][0], o["dp"][0], o["dG"][0], o["dh"][0], dA2, sets, n, m)
        vals = (z, o["nu"][0], lam[0], sl[0], lam[1], sl[1], lam[2], sl[2], lam[3], sl[3], tu, tl) \
            + f[:5] + (o["db"][0] if q else np.zeros(0),) + f[5:]
        for kk, v in zip(keys, vals):
            out[kk].append(v)
    out = {k: np.stack(v) for k, v in out.items()}
    two = np.isfinite(arrs[6])
    up, dn = out["t"] > ACTIVE, out["t_lo"] > ACTIVE
    at_h = (out["t"] < ACTIVE) & (out["lam"] > ACTIVE)
    at_l = two & (out["t_lo"] < ACTIVE) & (out["lam_lo"] > ACTIVE)
    inside = two & (out["lam"] < ACTIVE) & (out["lam_lo"] < ACTIVE)
    print("%-4s %-5s violated up %3d, down %3d, held at h %3d, at lower %3d, inside %3d"
          % (label, kind, up.sum(), dn.sum(), at_h.sum(), at_l.sum(), inside.sum()))
    assert up.any() and dn.any() and at_h.any() and at_l.any() and inside.any(), (label, kind)
    weak = np.zeros((B, m), bool)
    for lk, sk in PAIRS:
        weak |= np.maximum(out[lk], out[sk]) < 1e-4
    assert not weak.any(), (label, kind, np.argwhere(weak))
    save(R.fixture_name(label, kind), p=p, h=h, b=b, c=c, **dict(zip(R.FIELDS, arrs[6:])), **out)


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
