#!/usr/bin/env python3
"""Generate tests/golden/soft_*.npz from the REFERENCE ITSELF (locuslab/qpth at /root/reference): QPs with soft inequality
rows, solved by the unmodified reference as the AUGMENTED dense QP in (z, t) (tests/soft_reference.py: augment), float64.

Run in the build container only (the GPU box has no /root/reference):

    python tests/golden/make_golden_soft.py

Each QP is solved alone (batch of one, as make_golden.py's b1_* entries: the reference's stopping test is batch-global, the
kernels' per QP).  Each fixture stores, numbers only: the inputs Q, p, G, h, A, b and rho (inf = a hard row); zhat, t
(violations, 0 on the hard rows), lam, nu, slacks of the augmented solve; c and, for the loss <c, zhat>, the gradients
dQ, dp, dG, dh, dA, db (the leading blocks of the augmented gradients) and drho (the diagonal of the (t, t) block of dQ',
0 on the hard rows).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import run_ref, save  # noqa: E402  (stubs cvxpy, imports the reference)

import torch  # noqa: E402

import soft_reference as S  # noqa: E402


def case(label):
    Q, p, G, h, A, b, rho = S.soft_problem(label)
    B, n, m, q = S.SHAPES[label]
    c = S.loss_vector(label)
    out = {k: [] for k in ("zhat", "t", "lam", "nu", "slacks", "dQ", "dp", "dG", "dh", "dA", "db", "drho")}
    for i in range(B):
        aug, soft = S.augment(Q[i], p[i], G[i], h[i], A[i] if q else A, b[i] if q else b, rho[i])
        ns = len(soft)
        dl = np.concatenate([c[i], np.zeros(ns)])[None]
        o = run_ref(*[np.asarray(x)[None] if np.size(x) else x for x in aug], dl=dl)
        t = np.zeros(m)
        t[soft] = o["zhat"][0, n:]
        drho = np.zeros(m)
        drho[soft] = np.diagonal(o["dQ"][0])[n:]
        out["zhat"].append(o["zhat"][0, :n])
        out["t"].append(t)
        out["lam"].append(o["lam"][0])
        out["nu"].append(o["nu"][0])
        out["slacks"].append(o["slacks"][0])
        out["dQ"].append(o["dQ"][0, :n, :n])
        out["dp"].append(o["dp"][0, :n])
        out["dG"].append(o["dG"][0, :, :n])
        out["dh"].append(o["dh"][0])
        out["dA"].append(o["dA"][0, :, :n] if q else np.zeros((0, n)))
        out["db"].append(o["db"][0] if q else np.zeros(0))
        out["drho"].append(drho)
    save("soft_%s_b%d_n%d_m%d_q%d" % (label, B, n, m, q), Q=Q, p=p, G=G, h=h, A=A, b=b, rho=rho, c=c,
         **{k: np.stack(v) for k, v in out.items()})


def main():
    # (one thread: torch.linalg.lu_factor with more hangs in the build container's MKL from order 160 up, see make_golden.py)
    torch.set_num_threads(1)
    for label in S.FIXTURES:
        case(label)


if __name__ == "__main__":
    main()
