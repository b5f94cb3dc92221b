"""The barrier-smoothed QP on the MI355X (QPFunction(...)(Q, p, G, h, A, b, kappa=...), qpx_centre): the checks of
tests/centre_checks.py against tests/centre_reference.py, one shape per form family of the centring role:

    (10,5,0) one tile row | (12,9,3) one tile row, equalities | (20,24,3) two tile rows | (20,40,4) four tile rows
    (100,50,10) four tile rows, equalities | (100,100,0) seven tile rows | (60,112,0) the tile limit
    (40,130,0) thread-grid only (nineq > 112), ten blocks | (20,170,2) thirteen blocks (nineq > 160; not in the issue's list)

each at kappa in {1e-1, 1e-3, 1e-6}, a per-row kappa spread over two decades and a per-QP kappa.  Four and seven tile rows run
the chain-wave form; the finishing stage's rule (which the centring role follows) switches four tile rows to one wave per QP
beyond 8192 QPs only: test_one_wave_form_beyond_8192_qps.  Every case fails on the parent:
`kappa=` is a TypeError there and qpx_centre is missing from the library.

The step-time gate (the issue's one measurement): B = 512, nz = nineq = 100, kappa = 1e-3 -- the time of a qpx_centre launch per
Newton step against the time of qpx_polish(steps=k, refine=0) per step, on the same factors and start iterate, with 5 % for the
noise of the box: the centring step is one factorisation and one solve, the finishing step one factorisation and two solves.
(The finishing-stage kernels are the parent's, instruction for instruction; scripts/bench_centre.py --parent times the parent's
library itself and wrote profiles/centre.json.)"""
import contextlib
import statistics

import numpy as np
import pytest
import torch

import centre_checks as C
import problems

pytestmark = pytest.mark.gpu

ONE_WAVE = 2048           # the A/B knob: one wave per QP in the tile kernels
KINDS = (1e-1, 1e-3, 1e-6, "rows", "qps")
SHAPES = [((4, 10, 5, 0), 0), ((4, 12, 9, 3), 0), ((2, 20, 24, 3), 0), ((2, 20, 40, 4), 0), ((2, 100, 50, 10), 0), ((2, 100, 100, 0), 0), ((2, 60, 112, 0), 0),
          ((2, 40, 130, 0), 0), ((1, 20, 170, 2), 0)]
FORWARD = [(s, v, k) for s, v in SHAPES for k in KINDS]


class Env:
    def __init__(self, dev):
        self.dev = dev

    @contextlib.contextmanager
    def run(self, variant=0):
        from qpth_amd import _lib
        dll = _lib.hip().dll
        old = dll.qpx_set_ipm_variant(variant)
        try:
            yield
        finally:
            dll.qpx_set_ipm_variant(old)


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return Env(torch.device("cuda:0"))


# ---------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("shape,variant,kind", FORWARD, ids=["%dx%dx%dx%d-%d-%s" % (s + (v, k)) for s, v, k in FORWARD])
def test_forward_against_the_reference(env, shape, variant, kind):
    C.forward(env, shape, 1, kind, variant)


def test_one_wave_form_beyond_8192_qps(env):
    """(20,40,4) at B = 8200: the batch of the chain-form case, repeated -- every QP centred by the numpy residual, and the same
    answer as the chain form gave its QP"""
    import centre_reference as cr
    from qpth_amd.qp import QPFunction
    B0, n, m, q = shape = (2, 20, 40, 4)
    arrs, kappa, ref = C.problem(shape, 1, 1e-3)
    rep = 4100
    big = [np.tile(a, (rep,) + (1,) * (a.ndim - 1)) for a in arrs]
    f = QPFunction(verbose=-1, duals=True, kappa_tol=C.KAPPA_TOL, kappa_steps=C.KAPPA_STEPS)
    with env.run():
        small = [C.host(x) for x in f(*C.on(arrs, env.dev), kappa=kappa)]
        out = [C.host(x) for x in f(*C.on(big, env.dev), kappa=kappa)]
    z, nu, lam, s = out
    worst = cr.residual(big, (z, lam, s, nu), kappa).max()
    C.note("one-wave form, B = 8200: numpy residual", worst)
    assert worst <= 10 * C.KAPPA_TOL
    for a, c, e in zip(out, small, (ref[0], ref[3], ref[1], ref[2])):
        assert C.rel_err(a[:B0], e).max() <= C.TOL_REF
        assert C.rel_err(a, np.tile(c, (rep, 1))).max() <= 1e-9         # (two forms, two orders of summation)


def test_which_family_serves_which_shape(env):
    from qpth_amd import _lib
    dll = _lib.hip().dll
    fam = lambda n, m, q: dll.qpx_kernel_family(_lib.QPX_F64, n, m, q)      # noqa: E731
    assert fam(60, 112, 0) == _lib.FAMILY_TILE and fam(40, 130, 0) == _lib.FAMILY_GRID and fam(150, 150, 0) == _lib.FAMILY_BIG
    assert dll.qpx_centre_supported(_lib.QPX_F64, 40, 130, 0) == 1 and dll.qpx_centre_supported(_lib.QPX_F64, 150, 150, 0) == 0
    assert dll.qpx_centre_supported(_lib.QPX_F32, 12, 9, 3) == 0 and dll.qpx_centre_supported(_lib.QPX_F32_WIDE, 12, 9, 3) == 0


# ---------------------------------------------------------------- 2. first order
@pytest.mark.parametrize("kind", [1e-3, "rows", "qps"], ids=str)
@pytest.mark.parametrize("duals", [False, True], ids=["zhat", "duals"])
@pytest.mark.parametrize("shape", [(2, 12, 9, 3), (2, 100, 100, 0)], ids=["12x9x3", "100x100x0"])
def test_first_order_gradients_and_dkappa(env, shape, kind, duals):
    C.first_order(env, shape, 1, kind, duals)


def test_first_order_thread_grid(env):
    C.first_order(env, (2, 40, 130, 0), 1, "rows", True)


def test_unbatched_parameters_get_the_mean(env):
    C.first_order(env, (3, 12, 9, 3), 1, "rows", True, unbatched=(0, 3))


@pytest.mark.parametrize("shape", [(2, 12, 9, 3), (2, 100, 50, 10)], ids=["12x9x3", "100x50x10"])
def test_adjoint_identity(env, shape):
    C.adjoint_identity(env, shape, 1)


# ---------------------------------------------------------------- 3. second order
@pytest.mark.parametrize("shape,seed", [((2, 12, 9, 3), 1), ((2, 100, 100, 0), 3)], ids=["12x9x3", "100x100x0"])
def test_second_order(env, shape, seed):
    C.second_order_check(env, shape, seed)


def test_kink(env):
    C.kink(env)


# ---------------------------------------------------------------- 4. limit, 5. composition, 6. refusals
def test_limit(env):
    C.limit(env)


def test_warm_start(env):
    C.warm_start(env)


def test_sensitivity_jacobian(env):
    C.sensitivity_jacobian(env)


def test_refusals(env):
    C.refusals(env)


def test_kappa_none_is_the_call_as_before(env):
    from qpth_amd.qp import QPFunction
    tq = C.on(problems.prof_qp(2, 12, 9, 3, seed=1), env.dev, grad=True)
    a = QPFunction(verbose=-1)(*tq)
    b = QPFunction(verbose=-1)(*tq, kappa=None)
    assert torch.equal(a, b) and type(a.grad_fn).__name__ == type(b.grad_fn).__name__ == "QPFunctionFnBackward"


# ---------------------------------------------------------------- the step-time gate
def step_times(dev, B=512, n=100, m=100, kappa=1e-3, k=8, reps=5, rounds=5, polish_lib=None):
    """(ms per centring step, ms per finishing step, every round): k steps each -- a tolerance nothing meets makes every QP
    take all k centring steps --, alternating rounds, medians.  polish_lib: a QpxLib whose qpx_polish is timed instead of this
    build's (scripts/bench_centre.py --parent)."""
    from qpth_amd.kkt import KKTFactors
    Q, p, G, h, A, b = C.on(problems.prof_qp(B, n, m, 0, seed=0), dev)
    fac = KKTFactors.build(Q, G, A, nBatch=B)
    r0 = fac.ipm(p, h, b, m * kappa)
    start = [x.clone() for x in (r0.zhat, r0.lam, r0.slacks)]
    kap = torch.full((m,), kappa, dtype=torch.float64, device=dev)
    lib = fac.lib

    def reset():
        for x, s in zip((r0.zhat, r0.lam, r0.slacks), start):
            x.copy_(s)

    def centre():
        fac.centre(p, h, b, r0, kap, tol=1e-300, max_steps=k)

    def polish():
        fac.lib = polish_lib or lib
        try:
            fac.polish(p, h, b, r0, steps=k, refine=0)
        finally:
            fac.lib = lib

    def timed(fn):
        total = 0.0
        for _ in range(reps):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            total += e0.elapsed_time(e1)
        return total / reps / k

    timed(centre), timed(polish)                             # warm-up: code objects, the LDS opt-in
    assert (r0.centre_steps == k).all()
    t = {"centre": [], "polish": []}
    for _ in range(rounds):
        t["centre"].append(timed(centre))
        t["polish"].append(timed(polish))
    return statistics.median(t["centre"]), statistics.median(t["polish"]), t


def test_step_time_against_the_finishing_stage(env):
    c, p, t = step_times(env.dev)
    print("ms per step at B = 512, nz = nineq = 100: centring %.4f, finishing stage %.4f (ratio %.3f); rounds %s" % (c, p, c / p, t))
    assert c <= 1.05 * p
