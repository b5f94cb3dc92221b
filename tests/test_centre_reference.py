"""tests/centre_reference.py validated against central finite differences (step 1e-6) of its own damped-Newton solver: the
claim of DESIGN 4.10 that the derivative formulas of the hard QP (tests/hvp_reference.py) hold unchanged at a point of the
central path, and that d loss / d kappa_i = dz_i / lam_i.

GATE 1e-5 relative to each gradient's largest entry: the float64 prototype of the issue measured absolute errors <= 2.3e-7
(<= 5e-7 for dkappa) on gradients of size ~1; one to two decades are added for the noise of finite differences."""
import numpy as np
import pytest

import centre_reference as cr
import problems
from hvp_reference import psi, random_W, second_order

GATE = 1e-5
STEP = 1e-6
CASES = [((6, 4, 2), 1e-1), ((6, 4, 2), 1e-3), ((12, 9, 3), 1e-1), ((12, 9, 3), 1e-3)]
IDS = ["6x4x2_1e-1", "6x4x2_1e-3", "12x9x3_1e-1", "12x9x3_1e-3"]


class Case:
    """one QP, a per-row kappa spread over a decade around `kappa`, cotangents on (zhat, lam, nu), the centred point"""

    def __init__(self, shape, kappa, seed=3):
        n, m, q = shape
        self.arrs = [np.asarray(a, np.float64) for a in problems.random_dense_qp(1, n, m, q, seed)]
        r = np.random.RandomState(seed + 1)
        self.kappa = kappa * 10 ** r.uniform(-0.5, 0.5, (1, m))
        self.cots = (r.randn(1, n), r.randn(1, m), r.randn(1, q))
        self.W = random_W(1, n, m, q, seed + 2)
        self.sol, _, res = cr.centre(self.arrs, self.kappa)
        assert res.max() <= 1e-12

    def point(self, arrs, kappa):
        sol, _, res = cr.centre(arrs, kappa, start=self.sol)
        assert res.max() <= 1e-12
        return sol

    def loss(self, arrs, kappa):
        z, lam, _, nu = self.point(arrs, kappa)
        return float((self.cots[0] * z).sum() + (self.cots[1] * lam).sum() + (self.cots[2] * nu).sum())

    def psi(self, arrs):
        sol = self.point(arrs, self.kappa)
        return float(psi(cr.grads(arrs, sol, self.cots)[0], self.W)[0])

    def fd(self, f, idx):
        """central differences of f(arrs, kappa) in arrs[idx] (idx 6: kappa)"""
        base = self.kappa if idx == 6 else self.arrs[idx]
        out = np.zeros(base.shape)
        for i in np.ndindex(*base.shape):
            vals = []
            for sgn in (1.0, -1.0):
                x = base.copy()
                x[i] += sgn * STEP * (base[i] if idx == 6 else 1.0)          # (kappa: a relative step, it spans decades)
                arrs = [x if k == idx else a for k, a in enumerate(self.arrs)]
                vals.append(f(arrs, x if idx == 6 else self.kappa))
            out[i] = (vals[0] - vals[1]) / (2 * STEP * (base[i] if idx == 6 else 1.0))
        return out


_CASES = {}


def case(shape, kappa):
    if (shape, kappa) not in _CASES:
        _CASES[shape, kappa] = Case(shape, kappa)
    return _CASES[shape, kappa]


def gap(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("shape,kappa", CASES, ids=IDS)
def test_the_reference_solver_lands_on_the_central_path(shape, kappa):
    c = case(shape, kappa)
    z, lam, s, nu = c.sol
    assert (lam > 0).all() and (s > 0).all()
    assert np.abs(lam * s / c.kappa - 1).max() <= 1e-12
    assert cr.residual(c.arrs, c.sol, c.kappa).max() <= 1e-12
    # the minimiser of the barrier problem: its gradient vanishes on the null space of A
    Q, p, G, h, A, b = [a[0] for a in c.arrs]
    g = Q @ z[0] + p + G.T @ (c.kappa[0] / (h - G @ z[0]))
    assert np.abs(g + A.T @ nu[0]).max() <= 1e-10


@pytest.mark.parametrize("shape,kappa", CASES, ids=IDS)
def test_first_order_gradients_and_dkappa_against_finite_differences(shape, kappa):
    c = case(shape, kappa)
    six, dkappa, _ = cr.grads(c.arrs, c.sol, c.cots)
    for idx, name in enumerate(("dQ", "dp", "dG", "dh", "dA", "db")):
        f = c.fd(c.loss, idx)
        if name == "dQ":
            f = 0.5 * (f + f.transpose(0, 2, 1))
        print(name, "%.1e" % gap(six[idx], f))
        assert gap(six[idx], f) <= GATE, name
    f = c.fd(c.loss, 6)
    print("dkappa", "%.1e" % gap(dkappa, f))
    assert gap(dkappa, f) <= GATE


@pytest.mark.parametrize("shape,kappa", CASES, ids=IDS)
def test_second_order_closed_form_against_finite_differences(shape, kappa):
    c = case(shape, kappa)
    _, _, bsol = cr.grads(c.arrs, c.sol, c.cots)
    so = second_order(c.arrs, c.sol, bsol, c.W)
    for idx, name in ((1, "Hp"), (3, "Hh"), (5, "Hb")):
        f = c.fd(lambda arrs, _k: c.psi(arrs), idx)
        print(name, "%.1e" % gap(so[name], f))
        assert gap(so[name], f) <= GATE, name


def test_kappa_to_zero_recovers_the_hard_qp():
    from oracle import qp_oracle as orc
    arrs = [np.asarray(a, np.float64) for a in problems.random_dense_qp(2, 12, 9, 3, 5)]
    x = orc.qp_forward_backward(*arrs, dl_dz=np.ones((2, 12)), per_qp=True)[0]
    gaps = [np.abs(cr.centre(arrs, k)[0][0] - x).max() for k in (1e-2, 1e-5, 1e-8)]
    print(gaps)
    assert gaps[0] > gaps[1] > gaps[2] and gaps[2] <= 1e-6
