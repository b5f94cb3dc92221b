"""Second derivatives through QPFunction on the MI355X: torch.autograd.grad(..., create_graph=True), then the grad
of <W, grads> -- the second-order pass, qpx_backward2 where the library serves the size, composed from qpx_jvp and
qpx_backward_duals elsewhere -- against the dense float64 closed form of tests/hvp_reference.py at the GPU's own solution.

GATE: the rule of tests/test_emu_backward2.py -- 100 x the worst relative error (conftest.rel_err, per QP and output) of the
Hessian-vector products below against the dense reference, measured on the MI355X, but no looser than 1e-8.  Measured:
(2,12,9,3) 2.9e-14, (2,100,100,0) 1.5e-12, (2,100,50,10) 2.5e-12, (16,64,64,0) one wave 8.4e-13: GATE = 100 x 2.5e-12."""
import numpy as np
import pytest
import torch

import problems
from conftest import rel_err
from hvp_reference import NAMES, first_backward, random_W, second_order

pytestmark = pytest.mark.gpu

GATE = 2.5e-10
ONE_WAVE = 2048


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return torch.device("cuda:0")


class knob:
    def __init__(self, variant):
        self.variant = variant

    def __enter__(self):
        from qpth_amd import _lib
        self.dll = _lib.hip().dll
        self.old = self.dll.qpx_set_ipm_variant(self.variant)

    def __exit__(self, *exc):
        self.dll.qpx_set_ipm_variant(self.old)


def leaves(arrs, dev, unbatched=()):
    tq = []
    for i, a in enumerate(arrs):
        a = np.asarray(a, np.float64)
        x = torch.tensor(a[0] if i in unbatched else a, device=dev) if a.size else torch.empty(0, dtype=torch.float64, device=dev)
        tq.append(x.requires_grad_(True) if x.nelement() else x)
    return tq


def second_grads(arrs, dev, cots, W, unbatched=(), **kw):
    """(solution, second-order gradients w.r.t. the parameters that exist): grads of <cots, (zhat, lam, nu)> with
    create_graph=True, then the grad of <W, grads>"""
    from qpth_amd.qp import QPFunction
    tq = leaves(arrs, dev, unbatched)
    params = [x for x in tq if x.nelement()]
    z, nu, lam, sl = QPFunction(verbose=-1, duals=True, **kw)(*tq)
    loss = sum((o * torch.tensor(c, device=dev)).sum() for o, c in zip((z, lam, nu), cots) if c is not None)
    g1 = torch.autograd.grad(loss, params, create_graph=True)
    Wt = [torch.tensor(w[0] if i in unbatched else w, device=dev) for i, w in enumerate(W) if np.size(w)]
    g2 = torch.autograd.grad(sum((g * w).sum() for g, w in zip(g1, Wt)), params)
    return [x.detach().cpu().numpy() for x in (z, lam, sl, nu)], [g.cpu().numpy() for g in g2]


def reference(arrs, sol, cots, W, unbatched=()):
    B = sol[0].shape[0]
    full = [np.asarray(a, np.float64) for a in arrs]
    if unbatched:          # every QP of the batch sees row 0 of an un-batched parameter; its per-QP cotangent is W / B
        full = [np.broadcast_to(a[0], a.shape).copy() if i in unbatched else a for i, a in enumerate(full)]
        W = [np.broadcast_to(w[0] / B, w.shape) if i in unbatched else w for i, w in enumerate(W)]
    ref = second_order(full, sol, first_backward(full, sol, cots), [w if np.size(w) else None for w in W])
    return [ref[k].sum(0) if i in unbatched else ref[k] for i, k in enumerate(NAMES) if np.size(ref[k])]


def worst(got, ref, whole=()):
    """worst relative error per QP and gradient (`whole`: gradients of un-batched parameters, one array for the batch)"""
    gaps = [float(rel_err(g[None] if i in whole else g, r[None] if i in whole else r).max()) for i, (g, r) in enumerate(zip(got, ref))]
    print("gaps against the dense reference", ["%.1e" % e for e in gaps])
    return max(gaps)


@pytest.mark.parametrize("shape,seed,variant", [((2, 12, 9, 3), 1, 0), ((2, 100, 100, 0), 3, 0), ((2, 100, 50, 10), 0, 0),
                                                ((16, 64, 64, 0), 0, ONE_WAVE)],
                         ids=["2x12x9x3", "2x100x100x0", "2x100x50x10", "16x64x64x0_one_wave"])
def test_hessian_vector_product(dev, shape, seed, variant):
    """fails on the parent: its gradients carry no graph, the second grad raises"""
    from qpth_amd import _lib
    B, n, m, q = shape
    arrs = problems.prof_qp(B, n, m, q, seed=seed)
    v = np.random.RandomState(seed + 50).randn(B, n)
    W = random_W(B, n, m, q, seed + 70)
    with knob(variant):
        assert _lib.hip().dll.qpx_backward2_supported(_lib.QPX_F64, n, m, q) == 1
        sol, got = second_grads(arrs, dev, (v, None, None), W)
    assert worst(got, reference(arrs, sol, (v, None, None), W)) <= GATE


def test_duals_and_a_loss_of_the_multipliers(dev):
    B, n, m, q = 2, 12, 9, 3
    arrs = problems.prof_qp(B, n, m, q, seed=1)
    r = np.random.RandomState(7)
    cots = (r.randn(B, n), r.randn(B, m), r.randn(B, q))
    W = random_W(B, n, m, q, 79)
    sol, got = second_grads(arrs, dev, cots, W)
    assert worst(got, reference(arrs, sol, cots, W)) <= GATE


def test_hessian_of_half_the_squared_norm_is_symmetric(dev):
    """d^2 (1/2 ||zhat||^2) / dp^2 at (2,10,8,0), column by column: the cotangent on zhat is zhat itself, so the second grad
    also flows through zdot back into the first-order backward"""
    from qpth_amd.qp import QPFunction
    B, n, m, q = 2, 10, 8, 0
    tq = leaves(problems.prof_qp(B, n, m, q, seed=1), dev)
    z = QPFunction(verbose=-1)(*tq)
    (g,) = torch.autograd.grad(0.5 * (z * z).sum(), tq[1], create_graph=True)
    H = torch.stack([torch.autograd.grad(g[:, j].sum(), tq[1], retain_graph=True)[0] for j in range(n)], 1).cpu().numpy()
    gap = rel_err(H, H.transpose(0, 2, 1)).max()
    print("asymmetry %.1e" % gap)
    assert np.abs(H).max() > 1e-3 and gap <= GATE


def test_shared_parameters(dev):
    """Q and h un-batched: per-QP cotangent W / B, second-order gradient the sum over the batch"""
    B, n, m, q = 4, 12, 9, 3
    arrs = [np.asarray(a, np.float64) for a in problems.prof_qp(B, n, m, q, seed=1)]
    v = np.random.RandomState(6).randn(B, n)
    W = random_W(B, n, m, q, 78)
    sol, got = second_grads(arrs, dev, (v, None, None), W, unbatched=(0, 3))
    assert got[0].shape == (n, n) and got[3].shape == (m,)
    assert worst(got, reference(arrs, sol, (v, None, None), W, unbatched=(0, 3)), whole=(0, 3)) <= GATE


def test_large_qp_family_takes_the_composed_path(dev):
    """(2,150,150,0): qpx_backward2 declines, KKTFactors.backward2 composes the pass from the family's jvp and backward; the gate
    of the family's first-order gradients in tests/test_gpu_parity.py, 1e-5 of the gradient's scale"""
    from qpth_amd import _lib
    B, n, m, q = 2, 150, 150, 0
    assert _lib.hip().dll.qpx_backward2_supported(_lib.QPX_F64, n, m, q) == 0
    arrs = problems.prof_qp(B, n, m, q, seed=3)
    v = np.random.RandomState(53).randn(B, n)
    W = random_W(B, n, m, q, 73)
    sol, got = second_grads(arrs, dev, (v, None, None), W)
    for k, a_, r_ in zip(NAMES, got, reference(arrs, sol, (v, None, None), W)):
        assert np.abs(a_ - r_).max() <= 1e-5 * max(1.0, np.abs(r_).max()), k


def test_first_order_path_is_unchanged(dev):
    """without create_graph: the gradients of QPFunction are bit-equal to a direct KKTFactors.backward made as before"""
    from qpth_amd.kkt import KKTFactors
    from qpth_amd.qp import QPFunction
    B, n, m, q = 8, 100, 100, 0
    arrs = problems.prof_qp(B, n, m, q, seed=0)
    tq = leaves(arrs, dev)
    v = torch.tensor(np.random.RandomState(5).randn(B, n), device=dev)
    z = QPFunction(verbose=-1)(*tq)
    g = torch.autograd.grad((z * v).sum(), tq[:4])
    assert not any(x.requires_grad for x in g)
    Q, p, G, h, A, b = [x.detach() for x in tq]
    fac = KKTFactors.build(Q, G, A, B)
    r = fac.ipm(p, h, b, 1e-12, 20, 3)
    direct = fac.backward(r.zhat, r.lam, r.slacks, r.nu, v, want=(True, True, True, True, False, False), shared=(False,) * 6,
                          refine=0, dl_dlam=None, dl_dnu=None, want_dz=False)
    assert torch.equal(z.detach(), r.zhat)
    for a, d in zip(g, direct[:4]):
        assert torch.equal(a, d)


def test_fused_equals_composed(dev):
    from qpth_amd.kkt import KKTFactors
    B, n, m, q = 8, 100, 100, 0
    arrs = problems.prof_qp(B, n, m, q, seed=0)
    Q, p, G, h, A, b = leaves(arrs, dev)
    with torch.no_grad():
        fac = KKTFactors.build(Q, G, A, B)
        r = fac.ipm(p, h, b)
        v = torch.tensor(np.random.RandomState(5).randn(B, n), device=dev)
        sol = fac.backward(r.zhat, r.lam, r.slacks, r.nu, v, want_sol=True)[-1]
        W = [torch.tensor(w, device=dev) if w.size else None for w in random_W(B, n, m, q, 75)]
        f = fac.backward2(r.zhat, r.lam, r.slacks, r.nu, sol, W, fused=True)
        c = fac.backward2(r.zhat, r.lam, r.slacks, r.nu, sol, W, fused=False)
    gaps = [float(rel_err(a.cpu().numpy(), e.cpu().numpy()).max()) for a, e in zip(f[0] + f[1], c[0] + c[1]) if a is not None]
    print("fused against composed", ["%.1e" % e for e in gaps])
    assert max(gaps) <= GATE


def test_what_is_not_served_raises_on_the_second_grad(dev):
    from qpth_amd.qp import QPFunction, QPSolvers
    from qpth_amd.solvers import external
    B, n, m, q = 2, 12, 9, 3
    arrs = problems.prof_qp(B, n, m, q, seed=1)

    def second_grad(f, *extra):
        tq = leaves(arrs, dev)
        z = f(*tq, *extra)
        (g,) = torch.autograd.grad(z.sum(), tq[1], create_graph=True)          # the first grad is served
        return torch.autograd.grad(g.sum(), tq[1])

    with pytest.raises(RuntimeError, match="second derivatives.*soft rows"):
        second_grad(QPFunction(verbose=-1), torch.full((m,), 10.0, dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError, match="second derivatives.*refine"):
        second_grad(QPFunction(verbose=-1, refine=1))
    tq = leaves(arrs, dev)
    with torch.no_grad():
        zs, nus, lams, sls = [x.cpu().numpy() for x in QPFunction(verbose=-1, duals=True)(*tq)]
    calls = []

    def replay(Q, p, G, h, A, b):
        i = len(calls)
        calls.append(i)
        return zs[i], nus[i], lams[i], sls[i]

    external.set_solver(replay)
    try:
        with pytest.raises(RuntimeError, match="second derivatives.*external"):
            second_grad(QPFunction(verbose=-1, solver=QPSolvers.CVXPY))
    finally:
        external.set_solver(None)
