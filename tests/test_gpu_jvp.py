"""-m gpu: forward-mode AD through QPFunction (QPFunctionFn.jvp -> qpx_jvp) on a real MI355X, at the benchmark's sizes.

At every shape: z' against torch.linalg.solve of the full KKT system in float64 on the device at the forward's own
(zhat, lam, s, nu) with the backward's d, and the adjoint identity against QPFunction's backward.  Beside: central finite
differences on a few C2 QPs, and the external-solver path.  Whole file ~ tens of seconds."""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import problems

pytestmark = pytest.mark.gpu


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


def tangents(prim, seed):
    g = torch.Generator(device=prim[0].device).manual_seed(seed)
    return [torch.randn(x.shape, generator=g, dtype=x.dtype, device=x.device) if x.nelement() else None for x in prim]


def jvp(prim, tans, **kw):
    from qpth_amd.qp import QPFunction
    with fwAD.dual_level():
        ins = [fwAD.make_dual(x, t) if t is not None else x for x, t in zip(prim, tans)]
        z = QPFunction(verbose=-1, **kw)(*ins)
        zp, zt = fwAD.unpack_dual(z)
    assert zt is not None and zt.shape == zp.shape and zt.dtype == zp.dtype
    return zp, zt


def solution(prim):
    """(zhat, lam, slacks, nu) as the float64 forward of QPFunction computes them"""
    from qpth_amd.kkt import KKTFactors
    Q, p, G, h, A, b = prim
    fac = KKTFactors.build(Q, G, A if A.nelement() else None)
    r = fac.ipm(p, h, b)
    return r.zhat, r.lam, r.slacks, (r.nu if A.nelement() else torch.zeros(Q.size(0), 0, dtype=Q.dtype, device=Q.device))


def full_kkt_tangent(prim, tans, sol):
    """z' by torch.linalg.solve in float64 of  [[Q, G^T, A^T], [D G, -I, 0], [A, 0, 0]] x = -[rx; D rz; ry]  (see
    tests/test_emu_jvp.py: full_kkt_tangent)"""
    zh, lam, sl, nu = [x.double() for x in sol]
    Q, p, G, h, A, b = [x.double() for x in prim]
    B, n = zh.shape
    m, q = lam.shape[1], nu.shape[1]
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=zh.device)   # noqa: E731
    tQ, tp, tG, th, tA, tb = [t.double() if t is not None else z(B, *shp) for t, shp in
                              zip(tans, ((n, n), (n,), (m, n), (m,), (q, n), (q,)))]
    if q == 0:
        A = z(B, 0, n)
    d = lam.clamp(min=1e-8) / sl.clamp(min=1e-8)
    mv = lambda M, v: torch.einsum("bij,bj->bi", M, v)   # noqa: E731
    mtv = lambda M, v: torch.einsum("bij,bi->bj", M, v)  # noqa: E731
    rx = 0.5 * (mv(tQ, zh) + mtv(tQ, zh)) + tp + mtv(tG, lam) + mtv(tA, nu)
    rz = mv(tG, zh) - th
    ry = mv(tA, zh) - tb
    N = n + m + q
    K = z(B, N, N)
    K[:, :n, :n], K[:, :n, n:n + m], K[:, :n, n + m:] = Q, G.transpose(1, 2), A.transpose(1, 2)
    K[:, n:n + m, :n] = d[:, :, None] * G
    K[:, n:n + m, n:n + m] = -torch.eye(m, dtype=torch.float64, device=zh.device)
    K[:, n + m:, :n] = A
    rhs = -torch.cat([rx, d * rz, ry], 1)
    # (eight systems per call: the batched LU behind torch.linalg.solve fails to allocate its workspace for 512 systems of
    # order 160 or 200 -- HIPBLAS_STATUS_ALLOC_FAILED -- while 4 096 of order 128 and 8 of order 620 go through)
    x = torch.cat([torch.linalg.solve(K[i:i + 8], rhs[i:i + 8]) for i in range(0, B, 8)])
    return x[:, :n]


def rel(a, b):
    a, b = a.double().reshape(len(a), -1), b.double().reshape(len(b), -1)
    return ((a - b).norm(dim=1) / b.norm(dim=1).clamp(min=1e-300)).max().item()


def adjoint_gap(prim, tans, zt, seed=3):
    """max over QPs of |<gbar, z'> - sum <grad, tangent>| / (sum of the terms' magnitudes), grads from QPFunction's backward"""
    from qpth_amd.qp import QPFunction
    leaves = [x.detach().clone().requires_grad_(True) if x.nelement() else x for x in prim]
    gbar = torch.randn(zt.shape, generator=torch.Generator(device=zt.device).manual_seed(seed), dtype=zt.dtype, device=zt.device)
    QPFunction(verbose=-1)(*leaves).backward(gbar)
    lhs = (gbar.double() * zt.double()).sum(1)
    terms = [(x.grad.double() * t.double()).flatten(1).sum(1) for x, t in zip(leaves, tans) if t is not None and x.grad is not None]
    terms = torch.stack(terms)
    return ((lhs - terms.sum(0)).abs() / (terms.abs().sum(0) + lhs.abs())).max().item()


@pytest.mark.parametrize("shape", [(512, 100, 100, 0), (512, 100, 50, 10), (4096, 64, 64, 0), (8, 300, 300, 20)],
                         ids=["C2", "C3", "B4096_64_64", "large_300_300_20"])
def test_tangent_against_the_full_kkt_solve_and_the_backward(dev, shape):
    prim = on(problems.prof_qp(*shape, seed=1), dev)
    tans = tangents(prim, 2)
    z, zt = jvp(prim, tans)
    sol = solution(prim)
    assert torch.equal(z, sol[0])
    ref = full_kkt_tangent(prim, tans, sol)
    assert rel(zt, ref) <= 1e-8
    assert adjoint_gap(prim, tans, zt) <= 1e-10
    torch.cuda.synchronize()


def test_float32_data_in_float64_arithmetic_at_c2(dev):
    arrs32 = problems.prof_qp(512, 100, 100, 0, seed=4, dtype=np.float32)
    prim32 = on(arrs32, dev, torch.float32)
    tans32 = tangents(prim32, 5)
    z32, zt32 = jvp(prim32, tans32)
    assert zt32.dtype == torch.float32
    prim64 = [x.double() for x in prim32]
    ref = full_kkt_tangent(prim64, [t.double() if t is not None else None for t in tans32], solution(prim64))
    assert rel(zt32, ref) <= 1e-6              # float32 rounding of the narrowed output


def test_central_finite_differences_on_c2_qps(dev):
    from qpth_amd.qp import QPFunction
    prim = on(problems.prof_qp(512, 100, 100, 0, seed=6), dev)
    prim = [x[:4] if x.nelement() else x for x in prim]          # four QPs of C2
    tans = tangents(prim, 7)
    tans[0] = 0.5 * (tans[0] + tans[0].transpose(1, 2))
    _, zt = jvp(prim, tans)
    eps = 1e-6
    plus = QPFunction(verbose=-1)(*[x + eps * t if t is not None else x for x, t in zip(prim, tans)])
    minus = QPFunction(verbose=-1)(*[x - eps * t if t is not None else x for x, t in zip(prim, tans)])
    assert rel(zt, (plus - minus) / (2 * eps)) <= 1e-4


def test_external_solver_path(dev):
    from qpth_amd.qp import QPSolvers
    from qpth_amd.solvers import external
    prim = on(problems.prof_qp(8, 100, 50, 10, seed=8), dev)
    tans = tangents(prim, 9)
    sol = [x.cpu().numpy() for x in solution(prim)]
    calls = []

    def replay(Q, p, G, h, A, b):
        i = len(calls)
        calls.append(i)
        return sol[0][i], sol[3][i], sol[1][i], sol[2][i]

    external.set_solver(replay)
    try:
        z, zt = jvp(prim, tans, solver=QPSolvers.CVXPY)
    finally:
        external.set_solver(None)
    assert len(calls) == prim[0].size(0)
    ref = full_kkt_tangent(prim, tans, [torch.tensor(x, device=dev) for x in sol])
    assert rel(zt, ref) <= 1e-8
