"""-m gpu: the warm start of the PDIPM loop (KKTFactors.ipm(warm=...), QPFunction(warm_start=...); qpx_ipm_warm)
on a real MI355X, through libqpx_hip.so.  Inputs as in tests/test_emu_warm.py: prof_qp(seed=11), solved cold by the oracle;
the perturbed problem p + delta randn, h + delta rand (RandomState(7)) at delta = 1e-3; the warm start is the base problem's
(lam, slacks).  The library's defaults everywhere (eps = 1e-12, the round-off-floor stall rule): what a caller gets.  A few
seconds in all."""
import functools

import numpy as np
import pytest
import torch

import problems
import warm_reference as W
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-6
TILE, GRID16, ONE_WAVE = 1024, 256, 2048            # include/qpx.h: qpx_set_ipm_variant
ORACLE_THREADS = 8                                  # one per QP: the oracle's default, a thread per CPU the box reports, costs seconds per call where the process may use a few of them


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from qpth_amd import _lib
    _lib.hip()                              # the HIP extension must be the thing that runs
    assert _lib._TEST_BACKEND is None
    return torch.device("cuda:0")


def on(arrs, dev, dtype=torch.float64):
    return [torch.tensor(np.asarray(x), dtype=dtype, device=dev) if np.asarray(x).size else torch.empty(0, dtype=dtype, device=dev)
            for x in arrs]


@functools.lru_cache(maxsize=None)
def problem(shape, dtype=np.float64):
    """base and perturbed problem (rounded to dtype), the oracle's float64 cold solutions of both"""
    from oracle import qp_oracle as orc
    base = problems.prof_qp(*shape, seed=W.SEED)
    pert = W.perturb(base, 1e-3)
    base, pert = [[np.asarray(x, dtype) for x in arrs] for arrs in (base, pert)]
    sols = []
    for arrs in (base, pert):
        x, y, lam, s, _, info = orc.qp_forward_backward(*[np.asarray(a, np.float64) for a in arrs], per_qp=True, stall_policy=2, nthreads=ORACLE_THREADS)
        sols.append(dict(zhat=x, nu=y, lam=lam, slacks=s))
    return base, pert, sols[0], sols[1]


class knob:
    def __init__(self, variant):
        self.variant = variant

    def __enter__(self):
        from qpth_amd import _lib
        self.old = _lib.hip().dll.qpx_set_ipm_variant(self.variant)

    def __exit__(self, *exc):
        from qpth_amd import _lib
        _lib.hip().dll.qpx_set_ipm_variant(self.old)


def cold_and_warm(shape, variant, dev, lam0, s0):
    from qpth_amd.kkt import KKTFactors
    _, pert, _, _ = problem(shape)
    Q, p, G, h, A, b = on(pert, dev)
    with knob(variant):
        fac = KKTFactors.build(Q, G, A, shape[0])
        cold = fac.ipm(p, h, b)
        hot = fac.ipm(p, h, b, warm=(lam0, s0))
    torch.cuda.synchronize()
    return fac, cold, hot


def close_to(res, sol, q):
    worst = {k: rel_err(getattr(res, k).cpu().numpy(), sol[k]).max() for k in ("zhat", "lam", "slacks") + (("nu",) if q else ())}
    assert max(worst.values()) < TOL, worst


@pytest.mark.parametrize("shape,variant", [((8, 100, 100, 0), 0),                      # the seven-row chain-wave form
                                           ((8, 100, 50, 10), 0),                      # the four-row chain-wave form
                                           ((16, 64, 64, 0), TILE + ONE_WAVE),         # the one-wave tile form
                                           ((8, 12, 9, 3), GRID16)])                   # a thread grid
def test_warm_start_saves_passes(dev, shape, variant):
    _, _, sb, sp = problem(shape)
    lam0, s0 = on((sb["lam"], sb["slacks"]), dev)
    _, cold, hot = cold_and_warm(shape, variant, dev, lam0, s0)
    ci, wi = cold.iters.cpu().numpy(), hot.iters.cpu().numpy()
    print("iters cold", ci, "warm", wi, "ratio %.3f" % (wi.sum() / ci.sum()))
    close_to(hot, sp, shape[3])
    assert (hot.warm_used == 1).all() and (cold.warm_used == 0).all()
    assert (wi < ci).all()
    assert wi.sum() <= 0.7 * ci.sum()


def test_non_finite_entries_start_cold(dev):
    shape = (8, 100, 100, 0)
    _, _, sb, sp = problem(shape)
    lam0, s0 = on((sb["lam"], sb["slacks"]), dev)
    lam0[1, 99] = float("nan")
    s0[2, 0] = float("inf")
    _, cold, hot = cold_and_warm(shape, 0, dev, lam0, s0)
    assert hot.warm_used.tolist() == [1, 0, 0, 1, 1, 1, 1, 1]
    for k in ("zhat", "lam", "slacks", "iters", "best_resid"):
        assert torch.equal(getattr(hot, k)[1:3], getattr(cold, k)[1:3]), k
    close_to(hot, sp, 0)


def test_large_qp_family_starts_cold(dev):
    from qpth_amd import _lib
    from qpth_amd.kkt import KKTFactors
    B, n, m, q = 4, 150, 150, 0
    assert _lib.hip().dll.qpx_warm_supported(_lib.QPX_F64, n, m, q) == 0
    Q, p, G, h, A, b = on(problems.prof_qp(B, n, m, q, seed=W.SEED), dev)
    fac = KKTFactors.build(Q, G, A, B)
    cold = fac.ipm(p, h, b)
    hot = fac.ipm(p, h, b, warm=(cold.lam, cold.slacks))
    torch.cuda.synchronize()
    assert (hot.warm_used == 0).all()
    for k in ("zhat", "lam", "slacks", "iters", "best_resid"):
        assert torch.equal(getattr(hot, k), getattr(cold, k)), k


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_qpfunction_two_calls(dev, dtype):
    """the same holder on two successive calls, the second on the perturbed problem: warm everywhere, and the gradients of
    the warm call are the oracle's (float32: tensors in float64 arithmetic, the oracle on the float32-rounded data)"""
    from oracle import qp_oracle as orc
    from qpth_amd import WarmStart
    from qpth_amd.qp import QPFunction
    shape = (8, 100, 100, 0)
    B, n, m, q = shape
    base, pert, _, sp = problem(shape, np.float32 if dtype == torch.float32 else np.float64)
    dl = np.random.RandomState(5).randn(B, n)
    _, _, _, _, grads_ref, _ = orc.qp_forward_backward(*[np.asarray(a, np.float64) for a in pert], dl, per_qp=True, stall_policy=2, nthreads=ORACLE_THREADS)
    ws = WarmStart()
    QPFunction(verbose=-1, warm_start=ws)(*on(base, dev, dtype))
    assert (ws.used == 0).all() and ws.lam.dtype == dtype
    tq = on(pert, dev, dtype)
    for x in tq[:4]:
        x.requires_grad_(True)
    z = QPFunction(verbose=-1, warm_start=ws)(*tq)
    z.backward(torch.tensor(dl, dtype=dtype, device=dev))
    torch.cuda.synchronize()
    assert (ws.used == 1).all()
    assert z.dtype == dtype and rel_err(z.detach().cpu().numpy(), sp["zhat"]).max() < TOL
    for x, ref in zip(tq[:4], grads_ref[:4]):
        assert np.abs(x.grad.cpu().numpy() - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
