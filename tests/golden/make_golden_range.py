#!/usr/bin/env python3
"""Generate tests/golden/range_*.npz from the REFERENCE ITSELF (locuslab/qpth at /root/reference): QPs with two-sided rows
lower <= Gz <= h, solved by the unmodified reference as the DOUBLED QP [G; -G_F] z <= [h; -lower_F] (tests/range_reference.py:
double), float64.

Run in the build container only (the GPU box has no /root/reference):

    python tests/golden/make_golden_range.py

Each QP is solved alone (batch of one, as make_golden.py's b1_* entries: the reference's stopping test is batch-global, the
kernels' per QP).  Each fixture stores, numbers only: the inputs p, h, b and lower (-inf = a one-sided row; the matrices are
regenerated from the seed, range_reference.range_problem, and the stored vectors pin the generator); zhat, nu,
lam, slacks of the rows G z <= h and lam_lo, slacks_lo of the rows lower <= G z (0 and +inf on a one-sided row); c and, for the
loss <c, zhat>, the gradients dQ, dp, dG, dh, dA, db, dlower folded back onto the nineq rows (range_reference.fold).

A fixture must have rows active at h, rows active at lower and inactive rows -- asserted here: one without all three shows
nothing -- and strict complementarity on every row (max(lam, slack) >= 1e-4): the fixtures carry gradients.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import run_ref, save  # noqa: E402  (stubs cvxpy, imports the reference)

import torch  # noqa: E402

import range_reference as R  # noqa: E402

ACTIVE = 1e-6        # a row is active where its multiplier exceeds this, inactive where both sides' stay below


def case(label, sides):
    Q, p, G, h, A, b, lower = R.range_problem(label, sides)
    B, n, m, q = R.SHAPES[label]
    c = R.loss_vector(label)
    keys = ("zhat", "nu", "lam", "slacks", "lam_lo", "slacks_lo", "dQ", "dp", "dG", "dh", "dA", "db", "dlower")
    out = {k: [] for k in keys}
    for i in range(B):
        G2, h2, F = R.double(G[i], h[i], lower[i])
        o = run_ref(Q[i][None], p[i][None], G2[None], h2[None], A[i][None] if q else A, b[i][None] if q else b, dl=c[i][None])
        lam, lam_lo = R.split(o["lam"][0], F, m, 0.0)
        sl, sl_lo = R.split(o["slacks"][0], F, m, np.inf)
        dG, dh, dlower = R.fold(o["dG"][0], o["dh"][0], F, m)
        for k, v in zip(keys, (o["zhat"][0], o["nu"][0], lam, sl, lam_lo, sl_lo, o["dQ"][0], o["dp"][0], dG, dh,
                               o["dA"][0] if q else np.zeros((0, n)), o["db"][0] if q else np.zeros(0), dlower)):
            out[k].append(v)
    out = {k: np.stack(v) for k, v in out.items()}
    at_h, at_lower = out["lam"] > ACTIVE, out["lam_lo"] > ACTIVE
    inactive = (out["lam"] < ACTIVE) & (out["lam_lo"] < ACTIVE)
    print("%-4s %-4s rows active at h %3d, at lower %3d, inactive %3d" % (label, sides, at_h.sum(), at_lower.sum(), inactive.sum()))
    assert at_h.any() and at_lower.any() and inactive.any(), (label, sides)
    assert not (at_h & at_lower).any()
    # ... and no row near a kink of the solution map (a bound reached with a zero multiplier): gradients are compared, and the
    # backward's d = clamp(lam, 1e-8) / clamp(s, 1e-8) is the same number for two solvers only while the vanishing one of
    # (lam, s) ends below the clamp: lam s ~ 1e-13 at the stop, so the other has to stay above 1e-5 -- 1e-4 with a margin
    weak = (np.maximum(out["lam"], out["slacks"]) < 1e-4) | (np.maximum(out["lam_lo"], out["slacks_lo"]) < 1e-4)
    assert not weak.any(), (label, sides, np.argwhere(weak))
    save(R.fixture_name(label, sides), p=p, h=h, b=b, lower=lower, c=c, **out)


def main():
    # (one thread: torch.linalg.lu_factor with more hangs in the build container's MKL from order 160 up, see make_golden.py)
    torch.set_num_threads(1)
    for label in R.SHAPES:
        for sides in R.SIDES:
            case(label, sides)


if __name__ == "__main__":
    main()
