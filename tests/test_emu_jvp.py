"""Forward-mode AD through QPFunction (QPFunctionFn.jvp -> qpx_jvp) on the host-thread emulator: the kernel bodies of every
family form the tangent right-hand side and solve the KKT system of the backward with it.  Checked against a float64 solve
of the full KKT system at the forward's own solution, against the shipped backward by the adjoint identity, with shared
parameters, tangents on a subset of the inputs, float32 data in float64 arithmetic, the external-solver path, central finite
differences of the oracle's solutions, and the argument checks of the C ABI."""
import ctypes

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import problems
from emu.harness import emu_lib, emulated
from oracle import qp_oracle as orc
from qpth_amd import _lib
from qpth_amd.kkt import KKTFactors
from qpth_amd.qp import QPFunction, QPSolvers

NAMES = ("Q", "p", "G", "h", "A", "b")
# every form of the kernels the dispatcher can pick (include/qpx.h, qpx_set_ipm_variant; as tests/test_emu_parity.py)
FORMS = [3, 256, 512, 1024 + 2048, 1024 + 4096, 1024 + 8192]


def _t(x, dtype=torch.float64):
    x = np.asarray(x)
    return torch.tensor(x, dtype=dtype) if x.size else torch.empty(0, dtype=dtype)


def tangents_for(arrs, seed, which=NAMES, sym_q=False):
    r = np.random.RandomState(seed)
    out = []
    for name, x in zip(NAMES, arrs):
        x = np.asarray(x)
        if name not in which or x.size == 0:
            out.append(None)
            continue
        t = r.randn(*x.shape)
        if sym_q and name == "Q":
            t = 0.5 * (t + np.swapaxes(t, -1, -2))
        out.append(t)
    return out


def jvp_of(arrs, tans, dtype=torch.float64, threads=128, variant=0, **kw):
    """zhat and its tangent: QPFunction on dual inputs (a tangent of None: that input is not dual)"""
    prim = [_t(x, dtype) for x in arrs]
    with emulated(threads, variant):
        with fwAD.dual_level():
            ins = [fwAD.make_dual(x, _t(t, dtype)) if t is not None else x for x, t in zip(prim, tans)]
            z = QPFunction(verbose=-1, **kw)(*ins)
            zp, zt = fwAD.unpack_dual(z)
    assert zt is not None and zt.shape == zp.shape and zt.dtype == zp.dtype
    return zp.numpy(), zt.numpy()


def solution_of(arrs, threads=128, variant=0):
    """(zhat, lam, slacks, nu) as the float64 forward of QPFunction computes them (pre-factorisation + loop)"""
    Q, p, G, h, A, b = [_t(x) for x in arrs]
    with emulated(threads, variant):
        fac = KKTFactors.build(Q, G, A if A.nelement() else None, Q.size(0) if Q.dim() == 3 else None)
        r = fac.ipm(p, h, b)
    nu = r.nu.numpy() if r.nu.nelement() else np.zeros((r.zhat.shape[0], 0))
    return r.zhat.numpy(), r.lam.numpy(), r.slacks.numpy(), nu


def _bat(x, B, nd):
    x = np.asarray(x, np.float64)
    if x.ndim == nd - 1 or x.shape[0] == 1:
        return np.broadcast_to(x.reshape(x.shape[-(nd - 1):]), (B,) + x.shape[-(nd - 1):])
    return x


def full_kkt_tangent(arrs, tans, sol, duals=False):
    """z' from a float64 solve of the full KKT system at (zhat, lam, s, nu) with the backward's d (qp.py:148):
         [Q   G^T  A^T] [z' ]     [rx  ]   rx = 1/2 (tQ + tQ^T) zhat + tp + tG^T lam + tA^T nu
         [DG  -I    0 ] [l' ] = - [D rz]   rz = tG zhat - th,   ry = tA zhat - tb,   D = diag(d)
         [A    0    0 ] [nu']     [ry  ]   (the second block row: G z' + s' = -rz with s' = -l'/d, times d)"""
    zh, lam, sl, nu = sol
    B, n = zh.shape
    m, q = lam.shape[1], nu.shape[1]
    Q, G = _bat(arrs[0], B, 3), _bat(arrs[2], B, 3)
    A = _bat(arrs[4], B, 3) if q else np.zeros((B, 0, n))
    zero = (np.zeros((B, n, n)), np.zeros((B, n)), np.zeros((B, m, n)), np.zeros((B, m)), np.zeros((B, q, n)), np.zeros((B, q)))
    tQ, tp, tG, th, tA, tb = [_bat(t, B, z.ndim) if t is not None else z for t, z in zip(tans, zero)]
    d = np.maximum(lam, 1e-8) / np.maximum(sl, 1e-8)
    out, lt, nt = np.empty((B, n)), np.empty((B, m)), np.empty((B, q))
    for i in range(B):
        rx = 0.5 * (tQ[i] + tQ[i].T) @ zh[i] + tp[i] + tG[i].T @ lam[i] + tA[i].T @ nu[i]
        rz = tG[i] @ zh[i] - th[i]
        ry = tA[i] @ zh[i] - tb[i]
        K = np.zeros((n + m + q, n + m + q))
        K[:n, :n], K[:n, n:n + m], K[:n, n + m:] = Q[i], G[i].T, A[i].T
        K[n:n + m, :n], K[n:n + m, n:n + m] = d[i][:, None] * G[i], -np.eye(m)
        K[n + m:, :n] = A[i]
        x = np.linalg.solve(K, -np.concatenate([rx, d[i] * rz, ry]))
        out[i], lt[i], nt[i] = x[:n], x[n:n + m], x[n + m:]
    return (out, lt, nt) if duals else out


def rel(a, b):
    a = np.asarray(a, np.float64).reshape(len(a), -1)
    b = np.asarray(b, np.float64).reshape(len(b), -1)
    return np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-300)


def check_against_full_solve(arrs, tans, tol=1e-9, **kw):
    z, zt = jvp_of(arrs, tans, **kw)
    sol = solution_of(arrs, kw.get("threads", 128), kw.get("variant", 0))
    assert np.array_equal(z, sol[0])                       # the same forward
    err = rel(zt, full_kkt_tangent(arrs, tans, sol)).max()
    assert err <= tol, err


# ---------------------------------------------------------------- every kernel form
@pytest.mark.parametrize("variant", FORMS)
@pytest.mark.parametrize("shape", [(2, 12, 9, 3), (1, 40, 52, 0)])
def test_every_kernel_form_against_the_full_kkt_solve(variant, shape):
    B, n, m, q = shape
    arrs = problems.random_dense_qp(B, n, m, q, seed=11)
    check_against_full_solve(arrs, tangents_for(arrs, 5), variant=variant)


def test_chain_wave_form_against_the_full_kkt_solve():
    arrs = problems.random_dense_qp(2, 20, 70, 3, seed=11)
    check_against_full_solve(arrs, tangents_for(arrs, 6), threads=256)


def test_large_qp_family_two_blocks_against_the_full_kkt_solve():
    arrs = problems.random_dense_qp(2, 70, 80, 5, seed=18)
    check_against_full_solve(arrs, tangents_for(arrs, 19), threads=256, variant=3)


# ---------------------------------------------------------------- the adjoint of the backward
def grads_of(arrs, gbar, dtype=torch.float64, threads=128, variant=0, **kw):
    tq = [_t(x, dtype) for x in arrs]
    for x in tq:
        if x.nelement():
            x.requires_grad_(True)
    with emulated(threads, variant):
        z = QPFunction(verbose=-1, **kw)(*tq)
        z.backward(_t(gbar, dtype))
    return [x.grad.numpy() if x.grad is not None else None for x in tq]


def adjoint_terms(zt, gbar, grads, tans, B):
    """per QP: <gbar, z'> and the <grad, tangent> terms.  A shared parameter's gradient is the batch MEAN (qp.py:159-177):
    its term, B <grad, tangent> summed over the batch, is spread evenly over the QPs."""
    lhs = np.einsum("bi,bi->b", gbar, zt)
    terms = []
    for g, t in zip(grads, tans):
        if t is None or g is None:
            continue
        t = np.asarray(t)
        if g.shape == t.shape and g.ndim in (2, 3) and g.shape[0] == B and B > 1:
            terms.append(np.einsum("bi,bi->b", g.reshape(B, -1), t.reshape(B, -1)))
        else:
            terms.append(np.full(B, np.sum(g * t)))
    return lhs, np.stack(terms)


@pytest.mark.parametrize("shape,variant,threads", [((2, 12, 9, 3), 0, 128), ((2, 20, 70, 3), 0, 256),
                                                   ((2, 40, 52, 0), 256, 128), ((2, 66, 70, 5), 3, 256)])
def test_adjoint_identity_against_the_backward(shape, variant, threads):
    B, n, m, q = shape
    arrs = problems.prof_qp(B, n, m, q, seed=2)
    tans = tangents_for(arrs, 8)                            # tQ not symmetric: the JVP symmetrises it, as dQ is symmetric
    gbar = np.random.RandomState(9).randn(B, n)
    _, zt = jvp_of(arrs, tans, threads=threads, variant=variant)
    grads = grads_of(arrs, gbar, threads=threads, variant=variant)
    lhs, terms = adjoint_terms(zt, gbar, grads, tans, B)
    scale = np.abs(terms).sum(0) + np.abs(lhs)
    assert (np.abs(lhs - terms.sum(0)) <= 1e-10 * scale).all(), (lhs, terms.sum(0))


# ---------------------------------------------------------------- shared parameters, subsets
def test_shared_parameters_equal_the_expanded_batch():
    """un-batched Q and h with tangents of their own shape (batch stride 0 in the kernel): z' equals the run on the explicitly
    expanded batch, and the adjoint identity holds with the backward's batch mean times B"""
    B, n, m, q = 3, 14, 10, 2
    arrs = list(problems.random_dense_qp(B, n, m, q, seed=4))
    arrs[0], arrs[3] = arrs[0][0], arrs[3][0]
    tans = tangents_for(arrs, 10)
    _, zt = jvp_of(arrs, tans)
    expand = lambda xs: [np.broadcast_to(x, (B,) + x.shape).copy() if i in (0, 3) else x for i, x in enumerate(xs)]  # noqa: E731
    _, zt_e = jvp_of(expand(arrs), expand(tans))
    assert rel(zt, zt_e).max() <= 1e-12
    gbar = np.random.RandomState(3).randn(B, n)
    grads = grads_of(arrs, gbar)
    assert grads[0].shape == (n, n) and grads[3].shape == (m,)
    lhs, terms = adjoint_terms(zt, gbar, grads, tans, B)
    assert abs(lhs.sum() - terms.sum()) <= 1e-10 * (np.abs(terms).sum() + np.abs(lhs).sum())


@pytest.mark.parametrize("which", [("p",), ("h",), ("b",), ("Q",), ("G", "h"), ("A", "p")])
def test_tangents_on_a_subset_of_the_inputs(which):
    arrs = problems.random_dense_qp(2, 12, 9, 3, seed=12)
    check_against_full_solve(arrs, tangents_for(arrs, 13, which=which))


def test_batch_of_one_and_expanded_tangents_through_kkt_factors():
    """KKTFactors.jvp: a (1, m, n) or expand()ed tangent of a (B, m, n) parameter goes in with batch stride 0; lam' and nu'
    on request"""
    B, n, m, q = 2, 12, 9, 3
    arrs = problems.random_dense_qp(B, n, m, q, seed=14)
    tans = tangents_for(arrs, 15, which=("G", "b"))
    tans[2] = np.broadcast_to(tans[2][:1], tans[2].shape).copy()
    sol = solution_of(arrs)
    ref, lref, nref = full_kkt_tangent(arrs, tans, sol, duals=True)
    Q, p, G, h, A, b = [_t(x) for x in arrs]
    tG1 = _t(tans[2][:1])
    with emulated():
        fac = KKTFactors.build(Q, G, A)
        r = fac.ipm(p, h, b)
        for tG in (tG1, tG1.expand(B, m, n)):
            zt, lt, nt = fac.jvp(r.zhat, r.lam, r.slacks, r.nu, (None, None, tG, None, None, _t(tans[5])), want_duals=True)
            assert rel(zt.numpy(), ref).max() <= 1e-9
            assert rel(lt.numpy(), lref).max() <= 1e-8 and rel(nt.numpy(), nref).max() <= 1e-8
        with pytest.raises(RuntimeError, match="tangent of G has shape"):
            fac.jvp(r.zhat, r.lam, r.slacks, r.nu, (None, None, tG1[:, :-1], None, None, None))


# ---------------------------------------------------------------- float32
@pytest.mark.parametrize("shape,variant", [((2, 20, 30, 3), 0), ((2, 66, 70, 5), 3)])
def test_float32_data_in_float64_arithmetic(shape, variant):
    """QPX_F32_WIDE: float32 tangents widened on load, z' narrowed on store; against the float64 run on the same data"""
    B, n, m, q = shape
    arrs32 = problems.random_dense_qp(B, n, m, q, seed=16, dtype=np.float32)
    tans = [None if t is None else t.astype(np.float32) for t in tangents_for(arrs32, 17)]
    _, zt32 = jvp_of(arrs32, tans, dtype=torch.float32, threads=256, variant=variant)
    _, zt64 = jvp_of([np.asarray(a, np.float64) for a in arrs32], [None if t is None else t.astype(np.float64) for t in tans],
                     threads=256, variant=variant)
    assert zt32.dtype == np.float32
    assert rel(zt32, zt64).max() <= 1e-5


def test_float32_kernels_with_refinement():
    """refine=2 on float32 tensors: the float32 thread-grid kernels, the tangent solve refined once as the backward's is"""
    arrs32 = problems.random_dense_qp(2, 20, 12, 2, seed=20, dtype=np.float32)
    tans = [None if t is None else t.astype(np.float32) for t in tangents_for(arrs32, 21)]
    _, zt32 = jvp_of(arrs32, tans, dtype=torch.float32, refine=2)
    _, zt64 = jvp_of([np.asarray(a, np.float64) for a in arrs32], [None if t is None else t.astype(np.float64) for t in tans])
    assert zt32.dtype == np.float32
    assert rel(zt32, zt64).max() <= 1e-3


# ---------------------------------------------------------------- the external-solver path
def test_external_solver_path():
    """QPSolvers.CVXPY: the forward by an external solver (a stand-in that replays the kernels' own solution), the tangent
    by qpx_jvp on factors rebuilt as the backward rebuilds them"""
    from qpth_amd.solvers import external
    arrs = problems.random_dense_qp(3, 12, 9, 3, seed=22)
    tans = tangents_for(arrs, 23)
    sol = solution_of(arrs)
    calls = []

    def replay(Q, p, G, h, A, b):
        i = len(calls)
        calls.append(i)
        return sol[0][i], sol[3][i], sol[1][i], sol[2][i]

    external.set_solver(replay)
    try:
        z, zt = jvp_of(arrs, tans, solver=QPSolvers.CVXPY)
    finally:
        external.set_solver(None)
    assert len(calls) == 3 and np.array_equal(z, sol[0])
    assert rel(zt, full_kkt_tangent(arrs, tans, sol)).max() <= 1e-9


# ---------------------------------------------------------------- finite differences of the oracle
@pytest.mark.parametrize("shape", [(2, 10, 8, 0), (2, 12, 9, 3)])
def test_central_finite_differences_of_the_oracle(shape):
    B, n, m, q = shape
    arrs = problems.random_dense_qp(B, n, m, q, seed=24)
    tans = tangents_for(arrs, 25, sym_q=True)
    _, zt = jvp_of(arrs, tans)
    eps = 1e-6

    def solve(sign):
        pert = [np.asarray(x) + sign * eps * t if t is not None else x for x, t in zip(arrs, tans)]
        return orc.qp_forward_backward(*pert, per_qp=True)[0]

    fd = (solve(1.0) - solve(-1.0)) / (2 * eps)
    assert rel(zt, fd).max() <= 1e-4


# ---------------------------------------------------------------- the C ABI
def test_argument_errors():
    lib = emu_lib()
    B, n, m = 1, 4, 3
    fac = np.zeros(lib.factor_elems(_lib.QPX_F64, n, m, 2))
    zh, dz, lam, sl = [np.zeros(64) for _ in range(4)]
    st = np.zeros(B, np.int32)

    def p(a):
        return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None

    def call(dtype=_lib.QPX_F64, zhat=zh, dzhat=dz, q=0):
        return lib.dll.qpx_jvp(dtype, B, n, m, q, p(fac), 0, p(zhat), p(lam), p(sl), None,
                               None, 0, None, 0, None, 0, None, 0, None, 0, None, 0,
                               p(dzhat), None, None, None, 0, None, 0, None, 0, None, 0, p(st), None)

    assert call(zhat=None) == -1            # QPX_ERR_ARG
    assert call(dzhat=None) == -1
    assert call(dtype=7) == -1
    assert call(q=2) == -1                  # equality constraints need nu
