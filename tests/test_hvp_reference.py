"""The closed form of the second-order pass (tests/hvp_reference.py) against central differences of the
project's CPU oracle: psi(theta) = sum_i <W_i, grad_i(theta)> with grad_i the six per-QP gradients of the oracle's backward for
a fixed cotangent v on zhat; d psi / d theta along one random direction per parameter block (and along one direction of v)
must equal <H_block, direction> (<zdot, direction>).  Second derivatives of a QP solution exist only under strict
complementarity, so the test first asserts that no row is near-degenerate: min_i max(lam_i, s_i) >= 1e-3.

Step 1e-5, gate 1e-5 relative -- |fd - <H, D>| over the sum of the magnitudes of the inner product's terms, see `gap` --, no row
masked.  Measured (worst block per case): 1.3e-7, 2.0e-7, 1.9e-6, 2.5e-6; min_i max(lam_i, s_i) = 2.0e-1, 4.7e-2, 2.7e-2, 2.8e-3."""
import numpy as np
import pytest

import problems
from hvp_reference import NAMES, first_backward, psi, random_W, second_order
from oracle import qp_oracle as orc

CASES = [((2, 12, 9, 3), 1), ((2, 10, 8, 0), 1), ((2, 100, 50, 10), 0), ((2, 100, 100, 0), 3)]
STEP, GATE = 1e-5, 1e-5


def oracle_grads(arrs, v):
    q = arrs[4].shape[-2] if np.size(arrs[4]) else 0
    x, y, z, s, grads, _ = orc.qp_forward_backward(*arrs, dl_dz=v, per_qp=True, stall_policy=2)
    B = x.shape[0]
    return (x, z, s, y if q else np.zeros((B, 0))), grads


def gap(fd, H, D):
    """|fd - <H, D>| over the sum of the inner product's terms' magnitudes, worst QP: the normalisation of the project's other
    finite-difference and adjoint checks (tests/test_emu_jvp.py: adjoint_terms) -- an inner product with a random direction
    cancels, so its own magnitude says nothing about the size of what was differenced"""
    B = len(fd)
    terms = H.reshape(B, -1) * D.reshape(B, -1)
    return float((np.abs(fd - terms.sum(1)) / (np.abs(terms).sum(1) + np.abs(fd))).max())


@pytest.mark.parametrize("shape,seed", CASES, ids=["%dx%dx%dx%d" % c[0] for c in CASES])
def test_closed_form_against_central_differences_of_the_oracle(shape, seed):
    B, n, m, q = shape
    arrs = [np.asarray(a, np.float64) for a in problems.prof_qp(B, n, m, q, seed=seed)]
    r = np.random.RandomState(100 + seed)
    v = r.randn(B, n)
    W = random_W(B, n, m, q, 200 + seed)
    if not q:
        W[4] = W[5] = None
    sol, _ = oracle_grads(arrs, v)
    margin = np.maximum(sol[1], sol[2]).min()
    print("min_i max(lam_i, s_i) = %.1e" % margin)
    assert margin >= 1e-3                                    # strict complementarity: the second derivative exists
    ref = second_order(arrs, sol, first_backward(arrs, sol, (v, None, None)), W)

    def psi_at(arrs_, v_):
        return psi(oracle_grads(arrs_, v_)[1], W)

    worst = {}
    for k, name in enumerate(NAMES):
        if not q and k >= 4:
            continue
        D = r.randn(*arrs[k].shape)
        if k == 0:
            D = 0.5 * (D + D.transpose(0, 2, 1))            # Q stays symmetric
        hi, lo = [list(arrs) for _ in range(2)]
        hi[k], lo[k] = arrs[k] + STEP * D, arrs[k] - STEP * D
        fd = (psi_at(hi, v) - psi_at(lo, v)) / (2 * STEP)
        worst[name] = gap(fd, ref[name], D)
    D = r.randn(B, n)
    fd = (psi_at(arrs, v + STEP * D) - psi_at(arrs, v - STEP * D)) / (2 * STEP)
    worst["zdot"] = gap(fd, ref["zdot"], D)
    print("finite-difference gaps", {k: "%.1e" % e for k, e in worst.items()})
    assert max(worst.values()) <= GATE, worst
