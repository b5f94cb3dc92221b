"""-m gpu: the KKT solve for K right-hand sides per QP in one launch (qpx_factor_solve_kkt_multi) and the Jacobians of
qpth_amd/sensitivity.py on a real MI355X, through libqpx_hip.so.  The two parity checks of tests/test_emu_multi.py at the
benchmark's shapes: every (QP, k) against KKTFactors.solve_kkt and against a float64 dense solve of the full KKT matrix on
the device (tests/multi_reference.py), 1e-8 relative per output (ds with a random rs: multi_reference.ds_tol).  Measured maxima
in float64: 3.0e-11 against solve_kkt, 7.4e-12 against the dense solve, ds 3.6e-12 (rs None) and 1.0e-7 (random rs).  About a
second per test."""
import numpy as np
import pytest
import torch

import problems
from multi_reference import dense_solve_many, ds_tol, kkt_matrix, rel_many
from qpth_amd.kkt import MULTI_RHS_BLOCK as RB        # kKktMultiRB of the kernels: tests/test_emu_multi.py holds the two equal

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


def no_breakdown(fac):
    from qpth_amd import _lib
    torch.cuda.synchronize()
    assert int(fac.status.max()) & _lib.ST_KKT_BREAKDOWN == 0


def random_rhs(B, K, n, m, q, dev, seed, dtype=torch.float64):
    g = torch.Generator(device=dev).manual_seed(seed)
    return [torch.randn(B, K, k, generator=g, dtype=torch.float64, device=dev).to(dtype) if k else None for k in (n, m, m, q)]


def check_many(fac, Q, G, A, d, rhs, tol=1e-8, refine=0, tol_single=None):
    tol_single = tol if tol_single is None else tol_single
    out = fac.solve_kkt_many(d, *rhs, refine=refine)
    worst_single = 0.0
    for k in range(out[0].shape[1]):
        ref = fac.solve_kkt(d, *[None if X is None else X[:, k] for X in rhs], refine=refine)
        for o, r_ in zip(out, ref):
            if o is not None:
                worst_single = max(worst_single, float(rel_many(o[:, k:k + 1], r_.unsqueeze(1)).max()))
    ref = dense_solve_many(Q, G, A, d, *rhs)
    worst_dense = max(float(rel_many(o, r_).max()) for o, r_ in zip(out[::2] + out[3:], ref[::2] + ref[3:]) if o is not None)
    ds_dense = float(rel_many(out[1], ref[1]).max())          # its bound: multi_reference.ds_tol
    print("solve_kkt_many K=%d: max rel err vs solve_kkt %.2e, (dx, dz, dy) vs dense float64 %.2e, ds vs -rz - G dx %.2e (rs %s)"
          % (out[0].shape[1], worst_single, worst_dense, ds_dense, "None" if rhs[1] is None else "random"))
    assert worst_single <= tol_single, worst_single
    assert worst_dense <= tol, worst_dense
    assert ds_dense <= ds_tol(tol, rhs[1]), ds_dense
    return out


def solved(shape, dev, B=8, dtype=torch.float64, wide=False):
    from qpth_amd.kkt import KKTFactors
    n, m, q = shape
    Q, p, G, h, A, b = on(problems.prof_qp(B, n, m, q, seed=3), dev, dtype)
    fac = KKTFactors.build(Q, G, A if q else None, wide=wide)
    r = fac.ipm(p, h, b)
    d = torch.clamp(r.lam, min=1e-8) / torch.clamp(r.slacks, min=1e-8)              # the backward's d (qp.py:148): 16 decades
    return fac, Q, G, (A if q else None), d


@pytest.mark.parametrize("shape", [(100, 100, 0), (100, 50, 10), (64, 64, 0), (20, 10, 4)])
def test_parity_float64(dev, shape):
    n, m, q = shape
    fac, Q, G, A, d = solved(shape, dev)
    for K in (1, RB + 1, n):
        out = check_many(fac, Q, G, A, d, random_rhs(8, K, n, m, q, dev, seed=K))
        assert out[0].shape == (8, K, n)
    rhs = random_rhs(8, RB + 1, n, m, q, dev, seed=30)
    rhs[1] = None                                   # the backward's right-hand side: ds too to 1e-8 against the dense solve
    check_many(fac, Q, G, A, d, rhs)
    no_breakdown(fac)


def test_parity_float32_data_in_float64_arithmetic(dev):
    n, m, q = 100, 100, 0
    fac, Q, G, A, d = solved((n, m, q), dev, dtype=torch.float32, wide=True)
    out = check_many(fac, Q, G, A, d, random_rhs(8, RB + 1, n, m, q, dev, seed=21, dtype=torch.float32), tol=1e-6)
    assert out[0].dtype == torch.float32
    no_breakdown(fac)


def test_parity_float32_thread_grid_kernels(dev):
    """QPX_F32: a well-conditioned system (d = 1) against the float64 dense solve to 1e-3, as tests/test_emu_multi.py"""
    from qpth_amd.kkt import KKTFactors
    B, n, m, q = 8, 20, 12, 2
    Q, _, G, _, A, _ = on(problems.random_dense_qp(B, n, m, q, seed=20, dtype=np.float32), dev, torch.float32)
    fac = KKTFactors.build(Q, G, A)
    d = torch.ones(B, m, dtype=torch.float32, device=dev)
    check_many(fac, Q, G, A, d, random_rhs(B, 2 * RB + 3, n, m, q, dev, seed=22, dtype=torch.float32), tol=1e-3, tol_single=1e-5)
    assert not fac.wide
    no_breakdown(fac)


def test_jacobian_against_the_dense_inverse_and_the_backward(dev):
    from qpth_amd import sensitivity
    from qpth_amd.qp import QPFunction
    B, n, m, q = 8, 100, 100, 0
    arrs = problems.prof_qp(B, n, m, q, seed=7)
    Q, p, G, h, A, b = on(arrs, dev)
    sol = sensitivity.solve(Q, p, G, h, A, b)
    J = sol.jacobian()
    assert J["z", "p"].shape == (B, n, n) and J["z", "h"].shape == (B, n, m) and J["z", "b"].shape == (B, n, 0)
    d = torch.clamp(sol.lam, min=1e-8) / torch.clamp(sol.slacks, min=1e-8)
    Kinv = torch.linalg.inv(kkt_matrix(Q, G, None, d))
    ref = -Kinv[:, :n, :n].transpose(1, 2)
    scale = ref.norm(dim=(1, 2))
    err = float(((J["z", "p"] - ref).norm(dim=(1, 2)) / scale).max())
    sym = float(((J["z", "p"] - J["z", "p"].transpose(1, 2)).norm(dim=(1, 2)) / scale).max())
    errh = float(((J["z", "h"] - Kinv[:, n:, :n].transpose(1, 2)).norm(dim=(1, 2)) / Kinv[:, n:, :n].norm(dim=(1, 2))).max())
    print("J[z,p] vs the dense inverse %.2e, asymmetry %.2e; J[z,h] %.2e" % (err, sym, errh))
    assert err <= 1e-8 and sym <= 1e-8 and errh <= 1e-8
    tq = on(arrs, dev)
    for x in tq[:4]:
        x.requires_grad_(True)
    z = QPFunction(verbose=-1)(*tq)
    for i in (0, 1, 57, n - 1):
        gp, gh = torch.autograd.grad(z[:, i].sum(), [tq[1], tq[3]], retain_graph=True)
        for got, g in ((J["z", "p"][:, i], gp), (J["z", "h"][:, i], gh)):
            e = float(((got - g).norm(dim=1) / g.norm(dim=1)).max())
            assert e <= 1e-8, (i, e)
    no_breakdown(sol.fac)


def test_large_family_fallback(dev):
    from qpth_amd import _lib
    B, n, m, q, K = 2, 300, 300, 20, 2
    fac, Q, G, A, d = solved((n, m, q), dev, B=B)
    assert _lib.hip().dll.qpx_multi_supported(_lib.QPX_F64, n, m, q) == 0
    out = check_many(fac, Q, G, A, d, random_rhs(B, K, n, m, q, dev, seed=25))
    assert out[3].shape == (B, K, q)
    no_breakdown(fac)
