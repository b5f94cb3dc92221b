"""qpx_centre (the centring role of the finishing-stage forms) on the host-thread emulator: through the C ABI --
parity with tests/centre_reference.py, the status bits, the QPX_ERR_* cases, qpx_centre_supported -- and through QPFunction(...,
kappa=...), the checks of tests/centre_checks.py that tests/test_gpu_centre.py runs on the MI355X at the larger shapes too."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import centre_checks as C
import centre_reference as cr
import problems
from emu.harness import emu_lib, emulated
from qpth_amd import _lib
from qpth_amd.kkt import KKTFactors

GRID16 = 256              # the A/B knob: thread-grid kernels where the tile kernels would serve the size


class Env:
    dev = torch.device("cpu")

    @staticmethod
    @contextlib.contextmanager
    def run(variant=0):
        with emulated(256, variant):
            yield


ENV = Env()


# ---------------------------------------------------------------- 1. the kernel role against the reference
KINDS = (1e-1, 1e-3, 1e-6, "rows", "qps")
FORWARD = ([((2, 10, 5, 0), 0, k) for k in KINDS] + [((2, 12, 9, 3), 0, k) for k in KINDS] + [((2, 12, 9, 3), GRID16, k) for k in KINDS]
           + [((2, 20, 40, 4), 0, k) for k in KINDS]
           # the chain-wave form at two kappas here, at every kappa on the MI355X (tests/test_gpu_centre.py)
           + [((2, 100, 50, 10), 0, k) for k in (1e-3, "rows")]
           + [((1, 20, 170, 2), 0, 1e-3)])                                 # the thread grid's largest form: thirteen blocks


@pytest.mark.parametrize("shape,variant,kind", FORWARD, ids=["%dx%dx%dx%d-%d-%s" % (s + (v, k)) for s, v, k in FORWARD])
def test_forward_against_the_reference(shape, variant, kind):
    C.forward(ENV, shape, 1, kind, variant)


def _state(shape=(2, 12, 9, 3), seed=1, eps=1e-2):
    arrs = problems.prof_qp(*shape, seed=seed)
    tq = C.on(arrs, ENV.dev)
    with emulated(256):
        fac = KKTFactors.build(tq[0], tq[2], tq[4], nBatch=shape[0])
        r = fac.ipm(tq[1], tq[3], tq[5], eps)
    return arrs, tq, fac, r


def test_status_bits():
    """a kappa entry that is not finite and > 0: QPX_ST_NONFINITE for that QP alone, its arrays untouched; one step from a
    loose start: QPX_ST_NOT_CENTRED and the last iterate"""
    B, n, m, q = shape = (2, 12, 9, 3)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        arrs, tq, fac, r = _state(shape)
        start = [x.clone() for x in (r.zhat, r.lam, r.slacks, r.nu)]
        kap = torch.full((B, m), 1e-3, dtype=torch.float64)
        kap[1, 2] = bad
        with emulated(256):
            r = fac.centre(tq[1], tq[3], tq[5], r, kap)
        st = fac.status.numpy()
        assert st[1] & _lib.ST_NONFINITE and not st[0] & (_lib.ST_NONFINITE | _lib.ST_NOT_CENTRED)
        assert r.centre_steps[1] == 0 and np.isinf(r.centre_resid[1].item()) and r.centre_resid[0] <= 1e-9
        for a, s0 in zip((r.zhat, r.lam, r.slacks, r.nu), start):
            assert torch.equal(a[1], s0[1]) and not torch.equal(a[0], s0[0])
    arrs, tq, fac, r = _state(shape)
    with emulated(256):
        r = fac.centre(tq[1], tq[3], tq[5], r, torch.full((m,), 1e-3, dtype=torch.float64), max_steps=1)
    assert (fac.status.numpy() & _lib.ST_NOT_CENTRED).all() and (r.centre_steps == 1).all() and (r.centre_resid > 1e-9).all()
    sol = [x.numpy() for x in (r.zhat, r.lam, r.slacks, r.nu)]
    assert np.allclose(cr.residual(arrs, sol, 1e-3), r.centre_resid.numpy(), rtol=1e-6, atol=1e-14)       # resid is the LAST iterate's


def test_a_shared_kappa_is_the_expanded_one():
    B, n, m, q = shape = (2, 12, 9, 3)
    kap = torch.tensor(C.kappa_of("rows", B, m))
    out = []
    for k in (kap, kap.unsqueeze(0).expand(B, m).contiguous()):
        arrs, tq, fac, r = _state(shape)
        with emulated(256):
            r = fac.centre(tq[1], tq[3], tq[5], r, k)
        out.append((r.zhat, r.lam, r.slacks, r.nu))
    for a, e in zip(*out):
        assert torch.equal(a, e)


def test_error_codes_and_supported():
    lib = emu_lib()
    dll = lib.dll
    assert dll.qpx_centre_supported(_lib.QPX_F64, 12, 9, 3) == 1
    assert dll.qpx_centre_supported(_lib.QPX_F64, 40, 130, 0) == 1           # thread-grid only: nineq > 112
    assert dll.qpx_centre_supported(_lib.QPX_F64, 60, 112, 0) == 1           # the tile limit
    assert dll.qpx_centre_supported(_lib.QPX_F32, 12, 9, 3) == 0
    assert dll.qpx_centre_supported(_lib.QPX_F32_WIDE, 12, 9, 3) == 0
    assert dll.qpx_centre_supported(_lib.QPX_F64, 150, 150, 0) == 0
    B, n, m, q = shape = (2, 12, 9, 3)
    arrs, tq, fac, r = _state(shape)
    Q, p, G, h, A, b = tq
    kap = torch.full((B, m), 1e-3, dtype=torch.float64)
    resid, steps = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.int32)

    def call(dtype=_lib.QPX_F64, kappa=kap, tol=1e-9, max_steps=20, dims=(B, n, m, q)):
        P = _lib._ptr
        return dll.qpx_centre(dtype, *dims, P(Q), n * n, P(p), n, P(G), m * n, P(h), m, P(A), q * n, P(b), q, P(fac.blob), fac.sfac,
                              P(kappa), m, ctypes.c_double(tol), max_steps, P(r.zhat), P(r.nu), P(r.lam), P(r.slacks), P(resid), P(steps),
                              P(fac.status), None)

    with emulated(256):
        assert call(kappa=None) == -1                        # QPX_ERR_ARG
        assert call(tol=0.0) == -1 and call(tol=-1.0) == -1 and call(tol=float("nan")) == -1
        assert call(max_steps=0) == -1
        assert call(dtype=_lib.QPX_F32) == -2 and call(dtype=_lib.QPX_F32_WIDE) == -2       # QPX_ERR_UNSUPPORTED, nothing launched
        assert call(dims=(B, 150, 150, 0)) == -2
        assert call() == 0 and (resid <= 1e-9).all() and (steps >= 1).all()
    # soft factors are refused on the host side, as polish does
    with emulated(256):
        soft = KKTFactors.build(Q, G, A, nBatch=B, w=torch.full((m,), 0.1, dtype=torch.float64))
        rs = soft.ipm(p, h, b)
        with pytest.raises(ValueError, match="soft rows"):
            soft.centre(p, h, b, rs, kap)


# ---------------------------------------------------------------- 2. QPFunction(..., kappa=...)
@pytest.mark.parametrize("kind", [1e-3, "rows", "qps"], ids=str)
@pytest.mark.parametrize("duals", [False, True], ids=["zhat", "duals"])
def test_first_order_gradients_and_dkappa(kind, duals):
    C.first_order(ENV, (2, 12, 9, 3), 1, kind, duals)


def test_unbatched_parameters_get_the_mean():
    C.first_order(ENV, (3, 12, 9, 3), 1, "rows", True, unbatched=(0, 3))


def test_adjoint_identity():
    C.adjoint_identity(ENV, (2, 12, 9, 3), 1)


def test_second_order():
    C.second_order_check(ENV, (2, 12, 9, 3), 1)


def test_kink():
    C.kink(ENV)


def test_limit():
    C.limit(ENV)


def test_warm_start():
    C.warm_start(ENV)


def test_sensitivity_jacobian():
    C.sensitivity_jacobian(ENV)


def test_refusals():
    C.refusals(ENV, big=(1, 150, 150, 0))


def test_kappa_none_is_the_call_as_before():
    """the same node and the same answer, bit for bit, with and without the keyword"""
    tq = C.on(problems.prof_qp(2, 12, 9, 3, seed=1), ENV.dev, grad=True)
    from qpth_amd.qp import QPFunction
    with emulated(256):
        a = QPFunction(verbose=-1)(*tq)
        b = QPFunction(verbose=-1)(*tq, kappa=None)
    assert torch.equal(a, b) and type(a.grad_fn).__name__ == type(b.grad_fn).__name__ == "QPFunctionFnBackward"
