"""tests/polish_step_reference.py against oracle/qp_oracle (pinned to the reference by tests/test_oracle_golden.py): from the
oracle's iterate after k iterations, ONE step of the numpy reference reproduces the oracle's iterate after k + 1 -- both are
float64-or-better restatements of batch.py:92-198, so the gate is 1e-9 of max(1, max |ref|).  maxIter = k makes the oracle
return the best of its first k iterates, the start point included (k = 1 returns the start point: loop_checks); the test
asserts first that the residual fell at every one of them, so that the best is the last.  The steps are k = 2 .. 5: the
finishing stage's regular start is k = 3 (tests/polish_checks.py).  Measured: 1.7e-12 at (12, 9, 3), 6.5e-11 at (20, 40, 4).

Not covered by the tie, and said here because it is where the two restatements part: the oracle and batch.py take a vector of
which NO entry shrinks as a step of max(1, largest ratio of the batch), the finishing stage (tests/polish_reference.py, the
kernels, this reference) as +inf.  The two agree wherever both s and z have a shrinking entry, which a QP with more than a
handful of rows always has; at (1, 1, 0) they differ (1.4e-5 after one step from k = 2), so that shape is not one of the two."""
import numpy as np
import pytest

import loop_checks as L
import polish_checks as C
import polish_step_reference as R

GATE = 1e-9
B = 3


def oracle_iterate(shape, k):
    rows = [L.oracle(shape, B, i, 1e-12, k) for i in range(B)]
    x, y, z, s = [np.stack([np.asarray(r[j][0], np.float64) if r[j] is not None else np.zeros(0) for r in rows]) for j in range(4)]
    return (x, s, z, y), np.array([float(r[4]["best_resid"][0]) for r in rows]), np.array([int(r[4]["iters"][0]) for r in rows])


@pytest.mark.parametrize("shape", [(12, 9, 3), (20, 40, 4)], ids=lambda s: L.tag(s))
def test_one_step_reproduces_the_oracles_next_iterate(shape):
    arrs = C.arrs_of(shape, B, "f64")
    worst = 0.0
    for k in (2, 3, 4, 5):
        it, best, iters = oracle_iterate(shape, k)
        nxt, best_next, iters_next = oracle_iterate(shape, k + 1)
        assert (iters == k).all() and (iters_next == k + 1).all() and (best_next < best).all()       # the best iterate is the last one
        total = R.residuals(arrs, [np.asarray(v, R.LD) for v in it])[4]
        assert np.abs(np.asarray(total, np.float64) / best - 1).max() <= GATE                        # ... and its total the oracle's
        mine = R.one_step(arrs, it)
        for a, r in zip(mine, nxt):
            for i in range(B):
                worst = max(worst, L.fig(a[i], r[i]))
    print("one reference step against the oracle's next iterate %s: %.3e" % (L.tag(shape), worst))
    assert worst <= GATE


def test_best_iterate_bookkeeping_of_the_reference():
    """strict <, the start competes, a non-finite total never wins"""
    t = np.array([[3.0, 2.0, np.nan, 5.0], [2.0, 2.0, 1.0, 5.0], [1.0, 1.5, np.nan, 4.0], [1.0, 1.0, 0.5, np.nan]], R.LD).T       # (steps, QPs)
    best, val, _ = C.returned(t, 3)
    assert best.tolist() == [1, 2, 0, 2] and np.asarray(val, float).tolist() == [2.0, 1.0, 1.0, 0.5]
    best, val, _ = C.returned(np.full((3, 1), np.nan, R.LD), 2)
    assert best.tolist() == [0] and np.isinf(val[0])
