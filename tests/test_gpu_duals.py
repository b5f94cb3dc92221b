"""-m gpu: QPFunction(duals=True) on a real MI355X at the benchmark's sizes -- a loss of (zhat, lam, nu) back-propagated by
qpx_backward_duals.

At every shape: the six gradients against a float64 dense solve at the forward's own solution (tests/duals_reference.py;
tolerance from the reference's own LU-vs-dense gap at the nearest fixture shape), and the adjoint identity against forward
mode through the public QPFunction.  Beside: the reference's gradients (tests/golden/duals_*.npz), a zhat-only loss bit for
bit against duals=False, cotangents on lam / nu alone, shared parameters, float32 in float64 arithmetic, float32 with
refine=2, the external-solver path.  Whole file: 5.2 s on an MI355X, the slowest case 0.93 s."""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import problems
from conftest import load_golden
from duals_reference import NAMES, dense_grads, dense_tol, rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from qpth_amd import _lib
    _lib.hip()                              # the HIP extension must be the thing that runs
    assert _lib._TEST_BACKEND is None
    return torch.device("cuda:0")


def on(arrs, dev, dtype=torch.float64, grad=False):
    out = [torch.tensor(np.asarray(x), dtype=dtype, device=dev) if np.asarray(x).size else torch.empty(0, dtype=dtype, device=dev)
           for x in arrs]
    if grad:
        for x in out:
            if x.nelement():
                x.requires_grad_(True)
    return out


def cotangents(prim, seed, which=("z", "lam", "nu")):
    B, m, n = prim[2].shape
    q = prim[4].shape[1] if prim[4].nelement() else 0
    g = torch.Generator(device=prim[0].device).manual_seed(seed)
    gz, gl, gn = [torch.randn(B, k, generator=g, dtype=prim[0].dtype, device=prim[0].device) for k in (n, m, q)]
    return (gz if "z" in which else None, gl if "lam" in which else None, gn if ("nu" in which and q) else None)


def grads_of(prim, cots, **kw):
    """(zhat, lam, slacks, nu) of QPFunction(duals=True) and the gradients of <g_z, zhat> + <g_lam, lam> + <g_nu, nu>"""
    from qpth_amd.qp import QPFunction
    tq = [x.detach().clone().requires_grad_(True) if x.nelement() else x for x in prim]
    z, nu, lam, sl = QPFunction(verbose=-1, duals=True, **kw)(*tq)
    sum((o * g).sum() for o, g in zip((z, lam, nu), cots) if g is not None).backward()
    return (z.detach(), lam.detach(), sl, nu.detach()), {k: x.grad for k, x in zip(NAMES, tq)}


def host(xs):
    return [None if x is None else x.detach().cpu().numpy() for x in xs]


def dense_gaps(prim, sol, cots, grads):
    ref = dense_grads(host(prim), host(sol), host(cots))
    return {k: rel(grads[k].cpu().numpy(), ref[k]).max() for k in ref}


def adjoint_gap(prim, cots, grads, seed=3):
    """max over QPs of |<g_z, z'> + <g_lam, lam'> + <g_nu, nu'> - sum <grad, tangent>| / (sum of the terms' magnitudes),
    tangents from QPFunction(duals=True) in forward mode (normalised as tests/test_gpu_jvp.py: adjoint_gap)"""
    from qpth_amd.qp import QPFunction
    g = torch.Generator(device=prim[0].device).manual_seed(seed)
    tans = [torch.randn(x.shape, generator=g, dtype=x.dtype, device=x.device) if x.nelement() else None for x in prim]
    with fwAD.dual_level():
        ins = [fwAD.make_dual(x, t) if t is not None else x for x, t in zip(prim, tans)]
        z, nu, lam, sl = [fwAD.unpack_dual(o) for o in QPFunction(verbose=-1, duals=True)(*ins)]
        assert sl.tangent is None
        tangs = (z.tangent, lam.tangent, nu.tangent)
    lhs = torch.stack([(c.double() * t.double()).sum(1) for c, t in zip(cots, tangs) if c is not None])
    terms = torch.stack([(grads[k].double() * t.double()).flatten(1).sum(1) for k, t in zip(NAMES, tans) if t is not None])
    return ((lhs.sum(0) - terms.sum(0)).abs() / (terms.abs().sum(0) + lhs.abs().sum(0))).max().item()


@pytest.mark.parametrize("shape", [(512, 100, 100, 0), (512, 100, 50, 10), (4096, 64, 64, 0), (8, 300, 300, 20)],
                         ids=["C2", "C3", "B4096_64_64", "large_300_300_20"])
def test_gradients_against_the_dense_solve_and_forward_mode(dev, shape):
    B, n, m, q = shape
    prim = on(problems.prof_qp(*shape, seed=1), dev)
    cots = cotangents(prim, 2)
    sol, grads = grads_of(prim, cots)
    gaps = dense_gaps(prim, sol, cots, grads)
    tol = dense_tol(n, m, q)
    adj = adjoint_gap(prim, cots, grads)
    print("dense-solve gaps", {k: "%.2e" % v for k, v in gaps.items()}, "tol %.1e" % tol, "adjoint gap %.2e" % adj)
    assert max(gaps.values()) <= tol, gaps
    assert adj <= 1e-9
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,shape", [("duals_b4_n100_m100", (4, 100, 100, 0)), ("duals_b4_n100_m50_q10", (4, 100, 50, 10))])
def test_gradients_of_the_reference(dev, name, shape):
    """end to end against the unmodified reference's forward + factor_kkt + solve_kkt(g_z, 0, g_lam, g_nu) + qp.py:157-173
    (tests/golden/make_golden_duals.py): the project's parity gate, 1e-6 relative per QP and gradient"""
    g = load_golden(name)
    prim = on(problems.prof_qp(*shape, seed=0), dev)
    q = shape[3]
    cots = [torch.tensor(g[k], device=dev) if (k != "g_nu" or q) else None for k in ("g_z", "g_lam", "g_nu")]
    _, grads = grads_of(prim, cots)
    worst = {k: rel(grads[k].cpu().numpy(), g[k]).max() for k in NAMES if k in g}
    print("reference gaps", {k: "%.2e" % v for k, v in worst.items()})
    assert max(worst.values()) <= 1e-6, worst


@pytest.mark.parametrize("shape", [(64, 100, 50, 10), (8, 300, 300, 20)], ids=["C3_tile", "large"])
def test_subsets_of_the_outputs(dev, shape):
    """lam only, nu only: dl/dzhat reaches the kernel as NULL; zhat only under duals=True: the launch of duals=False, bit for
    bit"""
    from qpth_amd.qp import QPFunction
    B, n, m, q = shape
    prim = on(problems.prof_qp(*shape, seed=3), dev)
    for which in (("lam",), ("nu",)):
        cots = cotangents(prim, 4, which)
        sol, grads = grads_of(prim, cots)
        assert max(dense_gaps(prim, sol, cots, grads).values()) <= dense_tol(n, m, q), which
    gz = cotangents(prim, 5, ("z",))
    _, grads = grads_of(prim, gz)
    tq = [x.detach().clone().requires_grad_(True) for x in prim]
    QPFunction(verbose=-1)(*tq).backward(gz[0])
    for k, x in zip(NAMES, tq):
        assert torch.equal(grads[k], x.grad), k


def test_shared_parameters_equal_the_expanded_batch(dev):
    """Q and p un-batched (the matrix and the vector reduction of KKTFactors.backward): the batch mean of the expanded run"""
    B, n, m, q = 64, 100, 50, 10
    arrs = list(problems.prof_qp(B, n, m, q, seed=6))
    arrs[0], arrs[1] = np.ascontiguousarray(arrs[0][0]), np.ascontiguousarray(arrs[1][0])
    prim = on(arrs, dev)
    full_prim = [x.expand(B, *x.shape).contiguous() if i < 2 else x for i, x in enumerate(prim)]
    cots = cotangents(full_prim, 7)
    _, shared = grads_of(prim, cots)
    _, full = grads_of(full_prim, cots)
    assert shared["dQ"].shape == (n, n) and shared["dp"].shape == (n,)
    for k in NAMES:
        want = full[k].mean(0) if shared[k].dim() < full[k].dim() else full[k]
        assert (shared[k] - want).abs().max().item() <= 1e-11 * max(1.0, want.abs().max().item()), k


def test_float32_data_in_float64_arithmetic_at_c2(dev):
    """QPX_F32_WIDE: float32 cotangents through In<T>, gradients narrowed on store: <= 1e-6 of the float64 run"""
    prim32 = on(problems.prof_qp(512, 100, 100, 0, seed=4, dtype=np.float32), dev, torch.float32)
    cots32 = cotangents(prim32, 5)
    _, g32 = grads_of(prim32, cots32)
    _, g64 = grads_of([x.double() for x in prim32], [c.double() if c is not None else None for c in cots32])
    worst = {k: rel(g32[k].cpu().numpy(), g64[k].cpu().numpy()).max() for k in NAMES[:4]}
    print("float32-wide gaps", {k: "%.2e" % v for k, v in worst.items()})
    assert g32["dQ"].dtype == torch.float32
    assert max(worst.values()) <= 1e-6, worst


def test_float32_kernels_with_refinement(dev):
    """refine=2 on float32 tensors: the float32 thread-grid kernels, one refinement step in the backward solve, whose
    residuals re-read the dual cotangents.  Gate as tests/test_emu_duals.py."""
    prim32 = on(problems.random_dense_qp(64, 20, 12, 2, seed=20, dtype=np.float32), dev, torch.float32)
    cots32 = cotangents(prim32, 21)
    _, g32 = grads_of(prim32, cots32, refine=2)
    _, g64 = grads_of([x.double() for x in prim32], [c.double() for c in cots32])
    assert max(rel(g32[k].cpu().numpy(), g64[k].cpu().numpy()).max() for k in NAMES) <= 1e-3


def test_external_solver_path(dev):
    from qpth_amd.kkt import KKTFactors
    from qpth_amd.qp import QPSolvers
    from qpth_amd.solvers import external
    B, n, m, q = 8, 100, 50, 10
    prim = on(problems.prof_qp(B, n, m, q, seed=8), dev)
    cots = cotangents(prim, 9)
    fac = KKTFactors.build(prim[0], prim[2], prim[4])
    r = fac.ipm(prim[1], prim[3], prim[5])
    sol = host((r.zhat, r.lam, r.slacks, r.nu))
    calls = []

    def replay(Q, p, G, h, A, b):
        i = len(calls)
        calls.append(i)
        return sol[0][i], sol[3][i], sol[1][i], sol[2][i]

    external.set_solver(replay)
    try:
        outs, grads = grads_of(prim, cots, solver=QPSolvers.CVXPY)
    finally:
        external.set_solver(None)
    assert len(calls) == B
    assert max(dense_gaps(prim, outs, cots, grads).values()) <= dense_tol(n, m, q)


def test_slacks_are_not_differentiable(dev):
    from qpth_amd.qp import QPFunction
    prim = on(problems.prof_qp(8, 10, 5, 0, seed=0), dev, grad=True)
    z, nu, lam, sl = QPFunction(verbose=-1, duals=True)(*prim)
    assert not sl.requires_grad and nu.shape == (8, 0) and not nu.requires_grad and lam.requires_grad
    with pytest.raises(RuntimeError, match="does not require grad"):
        sl.sum().backward()
