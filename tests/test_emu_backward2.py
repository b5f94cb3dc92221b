"""qpx_backward2 (the second-order pass of the backward) on the host-thread emulator, through the C ABI and through
KKTFactors.backward2: against tests/hvp_reference.py evaluated at the SAME (zhat, lam, s, nu, dx, dz, dy) the kernel was given
-- the kernel's arithmetic alone --, one case per kernel structure, QPX_F32_WIDE, NULL handling bit for bit, shared strides,
shared factors (sfac = 0), the fused entry against the composed path, and the autograd surface (create_graph=True).

Gates.  float64: 100 x the worst relative error (conftest.rel_err, per QP and output) of the fused entry against the dense
reference measured on the emulator at the shapes of CASES, but no looser than 1e-8.  Measured: 16x16 grid (2,12,9,3) 1.8e-14,
q = 0 (2,10,8,0) 6.2e-14, seven tile rows (2,100,100,0) 1.3e-12, four tile rows with equalities (2,100,50,10) 2.6e-12, one-wave
form (2,64,64,0) 2.1e-13: GATE = 100 x 2.6e-12 = 2.6e-10.  QPX_F32_WIDE at (2,12,9,3) against the float64 reference at the
float32 inputs widened: measured 3.8e-8 (the rounding of the float32 outputs, 2^-24 = 6e-8 per element):
GATE_WIDE = 100 x 3.8e-8 = 3.8e-6."""
import numpy as np
import pytest
import torch

import problems
from conftest import rel_err
from emu.harness import emu_lib, emulated
from hvp_reference import NAMES, first_backward, first_grads, psi, random_W, second_order
from qpth_amd import _lib
from qpth_amd.kkt import KKTFactors
from qpth_amd.qp import QPFunction, QPSolvers

GATE = 2.6e-10
GATE_WIDE = 3.8e-6
OUTS = ("zdot", "lamdot", "nudot") + NAMES
ONE_WAVE = 2048


def _t(x, dtype=torch.float64):
    x = np.asarray(x)
    return torch.tensor(x, dtype=dtype) if x.size else torch.empty(0, dtype=dtype)


_STATE = {}


def state(shape, seed, variant=0, dtype=torch.float64, shared_factors=False):
    """factors, solution and first backward of a case, made once: (fac, sol, bsol, arrs) with sol, bsol tuples of tensors"""
    key = (shape, seed, variant, dtype, shared_factors)
    if key not in _STATE:
        B, n, m, q = shape
        arrs = [np.asarray(a, np.float64) for a in problems.prof_qp(B, n, m, q, seed=seed)]
        if shared_factors:
            for i in (0, 2, 4):
                arrs[i] = arrs[i][0]
        Q, p, G, h, A, b = [_t(x, dtype) for x in arrs]
        v = _t(np.random.RandomState(seed + 50).randn(B, n), dtype)
        with emulated(256, variant):
            fac = KKTFactors.build(Q, G, A, nBatch=B, wide=dtype == torch.float32)
            r = fac.ipm(p, h, b)
            out = fac.backward(r.zhat, r.lam, r.slacks, r.nu, v, want_sol=True)
        sol = (r.zhat, r.lam, r.slacks, r.nu)
        bsol = tuple(x if x is not None else torch.zeros(B, 0, dtype=dtype) for x in out[-1])
        _STATE[key] = (fac, sol, bsol, arrs)
    return _STATE[key]


def run(fac, sol, bsol, W, variant=0, **kw):
    with emulated(256, variant):
        (zd, ld, nd), H = fac.backward2(*sol, bsol, W, **kw)
    return dict(zip(OUTS, (zd, ld, nd) + tuple(H)))


def reference(arrs, sol, bsol, W):
    return second_order(arrs, [x.double().numpy() for x in sol], [x.double().numpy() for x in bsol],
                        [None if w is None else np.asarray(w, np.float64) for w in W])


def worst_gap(got, ref, q):
    gaps = {k: float(rel_err(got[k].numpy(), ref[k]).max()) for k in OUTS if got[k] is not None and (q or k not in ("nudot", "HA", "Hb"))}
    print("gaps against the dense reference", {k: "%.1e" % e for k, e in gaps.items()})
    return max(gaps.values())


def cotangents(shape, seed, dtype=torch.float64):
    B, n, m, q = shape
    W = random_W(B, n, m, q, seed)
    return [_t(w, dtype) if w.size else None for w in W]


# ---------------------------------------------------------------- 1. one case per kernel structure, against the dense reference
CASES = [((2, 12, 9, 3), 1, 256), ((2, 10, 8, 0), 1, 0), ((2, 100, 100, 0), 3, 0), ((2, 100, 50, 10), 0, 0), ((2, 64, 64, 0), 0, ONE_WAVE)]


@pytest.mark.parametrize("shape,seed,variant", CASES, ids=["grid16", "q0", "seven_tile_rows", "four_tile_rows_eq", "one_wave"])
def test_fused_entry_against_the_dense_reference(shape, seed, variant):
    fac, sol, bsol, arrs = state(shape, seed, variant)
    assert fac.backward2_fused()
    W = cotangents(shape, seed + 70)
    got = run(fac, sol, bsol, W, variant, fused=True)
    assert int(fac.status.max()) & _lib.ST_KKT_BREAKDOWN == 0
    assert worst_gap(got, reference(arrs, sol, bsol, W), shape[3]) <= GATE


def test_float32_data_in_float64_arithmetic():
    shape = (2, 12, 9, 3)
    fac, sol, bsol, arrs = state(shape, 1, dtype=torch.float32)
    assert fac.wide and fac.backward2_fused()
    W = cotangents(shape, 71, torch.float32)
    got = run(fac, sol, bsol, W, fused=True)
    assert all(got[k].dtype == torch.float32 for k in OUTS)
    arrs32 = [np.asarray(a, np.float32).astype(np.float64) for a in arrs]
    assert worst_gap(got, reference(arrs32, sol, bsol, [w.numpy() for w in W]), 3) <= GATE_WIDE


# ---------------------------------------------------------------- 2. the C ABI's conventions
def test_a_null_cotangent_is_zero_and_a_null_output_costs_nothing():
    """each W_i NULL in turn = that W_i zero; each output NULL in turn: every requested output equals its value from the
    all-present call bit for bit"""
    shape = (2, 12, 9, 3)
    fac, sol, bsol, arrs = state(shape, 1)
    W = cotangents(shape, 72)
    full = run(fac, sol, bsol, W, fused=True)
    for i in range(6):
        cut = list(W)
        cut[i] = None
        zero = list(W)
        zero[i] = torch.zeros_like(W[i])
        a, z = run(fac, sol, bsol, cut, fused=True), run(fac, sol, bsol, zero, fused=True)
        for k in OUTS:
            assert torch.equal(a[k], z[k]), (i, k)
    for i in range(6):
        want = [j != i for j in range(6)]
        part = run(fac, sol, bsol, W, fused=True, want=want)
        assert part[NAMES[i]] is None
        for k in OUTS:
            if k != NAMES[i]:
                assert torch.equal(part[k], full[k]), (i, k)
    # lamdot, nudot NULL: straight through the C ABI
    lib = emu_lib()
    B, n, m, q = shape
    zd = torch.empty(B, n, dtype=torch.float64)
    Hp = torch.empty(B, n, dtype=torch.float64)
    with emulated(256):
        lib.backward2(B, n, m, q, fac.blob, fac.sfac, *sol, *bsol, *W, zd, None, None, None, Hp, None, None, None, None, fac.status)
    assert torch.equal(zd, full["zdot"]) and torch.equal(Hp, full["Hp"])


def test_shared_strides():
    """W_Q and W_h one copy for the batch (stride 0) = the same values expanded"""
    shape = (2, 12, 9, 3)
    fac, sol, bsol, arrs = state(shape, 1)
    W = cotangents(shape, 73)
    shared = list(W)
    shared[0], shared[3] = W[0][0], W[3][0]
    expanded = list(W)
    expanded[0], expanded[3] = W[0][:1].expand_as(W[0]).contiguous(), W[3][:1].expand_as(W[3]).contiguous()
    a, e = run(fac, sol, bsol, shared, fused=True), run(fac, sol, bsol, expanded, fused=True)
    for k in OUTS:
        assert torch.equal(a[k], e[k]), k


def test_shared_factors():
    """Q, G, A shared by the batch: one blob, sfac = 0"""
    shape = (2, 12, 9, 3)
    fac, sol, bsol, arrs = state(shape, 1, shared_factors=True)
    assert fac.sfac == 0
    W = cotangents(shape, 74)
    got = run(fac, sol, bsol, W, fused=True)
    assert worst_gap(got, reference(arrs, sol, bsol, W), 3) <= GATE


@pytest.mark.parametrize("shape,seed,variant", [CASES[0], CASES[3]], ids=["grid16", "four_tile_rows_eq"])
def test_fused_against_composed(shape, seed, variant):
    fac, sol, bsol, arrs = state(shape, seed, variant)
    W = cotangents(shape, seed + 75)
    f, c = run(fac, sol, bsol, W, variant, fused=True), run(fac, sol, bsol, W, variant, fused=False)
    gaps = {k: float(rel_err(f[k].numpy(), c[k].numpy()).max()) for k in OUTS if f[k] is not None and f[k].numel()}
    print("fused against composed", {k: "%.1e" % e for k, e in gaps.items()})
    assert max(gaps.values()) <= GATE


def test_composed_path_serves_what_the_fused_entry_declines():
    """the large-QP family (knob 3) and the two-wave tile form of the A/B knob: qpx_backward2_supported is 0, fused=True raises,
    the default takes the composed path and meets the reference"""
    for shape, variant in (((2, 12, 9, 3), 3), ((2, 64, 64, 0), 1024 + 4096)):
        fac, sol, bsol, arrs = state(shape, 1, variant)
        assert not fac.backward2_fused()
        W = cotangents(shape, 76)
        with pytest.raises(RuntimeError, match="qpx_backward2 does not serve"):
            run(fac, sol, bsol, W, variant, fused=True)
        got = run(fac, sol, bsol, W, variant)
        assert worst_gap(got, reference(arrs, sol, bsol, W), shape[3]) <= GATE
    lib = emu_lib()
    assert lib.dll.qpx_backward2_supported(_lib.QPX_F32, 12, 9, 3) == 0
    assert lib.dll.qpx_backward2_supported(_lib.QPX_F64, 150, 150, 0) == 0
    assert lib.dll.qpx_backward2_supported(_lib.QPX_F64, 100, 100, 0) == 1
    assert lib.dll.qpx_backward2_supported(_lib.QPX_F32_WIDE, 100, 50, 10) == 1


# ---------------------------------------------------------------- 3. autograd: create_graph=True
def leaves(arrs, dtype=torch.float64):
    tq = [_t(x, dtype) for x in arrs]
    for x in tq:
        if x.nelement():
            x.requires_grad_(True)
    return tq


def hvp_through_autograd(arrs, v, W, **kw):
    """grads of <v, zhat> with create_graph=True, then grad of <W, grads> w.r.t. the parameters and v"""
    tq = leaves(arrs)
    vt = _t(v).requires_grad_(True)
    params = [x for x in tq if x.nelement()]
    with emulated(256):
        z = QPFunction(verbose=-1, **kw)(*tq)
        g1 = torch.autograd.grad((z * vt).sum(), params, create_graph=True)
        assert all(g.requires_grad for g in g1)
        g2 = torch.autograd.grad(sum((g * _t(w)).sum() for g, w in zip(g1, W)), params + [vt])
    return z.detach(), [g.detach().numpy() for g in g1], [g.numpy() for g in g2]


def test_second_grad_through_qpfunction():
    B, n, m, q = shape = (2, 12, 9, 3)
    arrs = [np.asarray(a, np.float64) for a in problems.prof_qp(B, n, m, q, seed=1)]
    v = np.random.RandomState(5).randn(B, n)
    W = random_W(B, n, m, q, 77)
    z, g1, g2 = hvp_through_autograd(arrs, v, W)
    fac, sol, _, _ = state(shape, 1)
    assert torch.equal(z, sol[0])
    sol_np = [x.numpy() for x in sol]
    bsol = first_backward(arrs, sol_np, (v, None, None))
    ref = second_order(arrs, sol_np, bsol, W)
    for got, want in zip(g2, [ref[k] for k in NAMES] + [ref["zdot"]]):
        assert rel_err(got, want).max() <= GATE
    for got, want in zip(g1, first_grads(sol_np, bsol)):
        assert rel_err(got, want).max() <= 1e-8


def test_shared_parameters_take_w_over_b_and_the_sum():
    """Q and h un-batched: the first backward returns their gradient as the batch MEAN, so the per-QP cotangent is W / B and
    the second-order gradient the SUM over the batch of the per-QP results"""
    B, n, m, q = 4, 12, 9, 3
    arrs = [np.asarray(a, np.float64) for a in problems.prof_qp(B, n, m, q, seed=1)]
    arrs[0], arrs[3] = arrs[0][0], arrs[3][0]
    v = np.random.RandomState(6).randn(B, n)
    W = random_W(B, n, m, q, 78)
    W[0], W[3] = W[0][0], W[3][0]
    z, g1, g2 = hvp_through_autograd(arrs, v, W)
    full = [np.broadcast_to(a, (B,) + a.shape).copy() if i in (0, 3) else a for i, a in enumerate(arrs)]
    Q, p, G, h, A, b = [_t(x) for x in full]
    with emulated(256):
        fac = KKTFactors.build(Q, G, A)
        r = fac.ipm(p, h, b)
    sol_np = [x.numpy() for x in (r.zhat, r.lam, r.slacks, r.nu)]
    bsol = first_backward(full, sol_np, (v, None, None))
    Wq = [np.broadcast_to(w / B, (B,) + w.shape) if i in (0, 3) else w for i, w in enumerate(W)]
    ref = second_order(full, sol_np, bsol, Wq)
    want = [ref[k].sum(0, keepdims=True) if i in (0, 3) else ref[k] for i, k in enumerate(NAMES)] + [ref["zdot"]]
    for got, w in zip(g2, want):
        assert rel_err(got.reshape(w.shape), w).max() <= GATE


def test_duals_and_a_loss_of_the_multipliers():
    B, n, m, q = 2, 12, 9, 3
    arrs = [np.asarray(a, np.float64) for a in problems.prof_qp(B, n, m, q, seed=1)]
    r = np.random.RandomState(7)
    cz, cl, cn = r.randn(B, n), r.randn(B, m), r.randn(B, q)
    W = random_W(B, n, m, q, 79)
    tq = leaves(arrs)
    with emulated(256):
        z, nu, lam, sl = QPFunction(verbose=-1, duals=True)(*tq)
        loss = (z * _t(cz)).sum() + (lam * _t(cl)).sum() + (nu * _t(cn)).sum()
        g1 = torch.autograd.grad(loss, tq, create_graph=True)
        g2 = torch.autograd.grad(sum((g * _t(w)).sum() for g, w in zip(g1, W)), tq)
    sol_np = [x.detach().numpy() for x in (z, lam, sl, nu)]
    ref = second_order(arrs, sol_np, first_backward(arrs, sol_np, (cz, cl, cn)), W)
    for got, k in zip(g2, NAMES):
        assert rel_err(got.numpy(), ref[k]).max() <= GATE, k


def test_without_create_graph_nothing_changes():
    """the first-order path: the same launch as before, its gradients bit for bit those of a direct fac.backward"""
    B, n, m, q = 2, 12, 9, 3
    arrs = [np.asarray(a, np.float64) for a in problems.prof_qp(B, n, m, q, seed=1)]
    v = _t(np.random.RandomState(5).randn(B, n))
    tq = leaves(arrs)
    with emulated(256):
        z = QPFunction(verbose=-1)(*tq)
        g = torch.autograd.grad((z * v).sum(), tq)
        assert not any(x.requires_grad for x in g)
        fac = KKTFactors.build(*[tq[i].detach() for i in (0, 2, 4)])
        r = fac.ipm(*[tq[i].detach() for i in (1, 3, 5)])
        direct = fac.backward(r.zhat, r.lam, r.slacks, r.nu, v)
    for a, d in zip(g, direct):
        assert torch.equal(a, d)


def test_what_is_not_served_raises():
    """soft rows, refine > 0 and the external-solver path: a RuntimeError naming the limitation on the second grad; third
    derivatives: the second-order pass is once differentiable"""
    from qpth_amd.solvers import external
    B, n, m, q = 2, 12, 9, 3
    arrs = [np.asarray(a, np.float64) for a in problems.prof_qp(B, n, m, q, seed=1)]

    def second_grad(f, *extra):
        tq = leaves(arrs)
        z = f(*tq, *extra)
        (g,) = torch.autograd.grad(z.sum(), tq[1], create_graph=True)
        return torch.autograd.grad(g.sum(), tq[1], create_graph=True)[0], tq[1]

    sol = state((B, n, m, q), 1)[1]
    with emulated(256):
        with pytest.raises(RuntimeError, match="second derivatives.*soft rows"):
            second_grad(QPFunction(verbose=-1), torch.full((m,), 10.0, dtype=torch.float64))
        with pytest.raises(RuntimeError, match="second derivatives.*refine"):
            second_grad(QPFunction(verbose=-1, refine=1))
        calls = []

        def replay(Q, p, G, h, A, b):
            i = len(calls)
            calls.append(i)
            return sol[0][i].numpy(), sol[3][i].numpy(), sol[1][i].numpy(), sol[2][i].numpy()

        external.set_solver(replay)
        try:
            with pytest.raises(RuntimeError, match="second derivatives.*external"):
                second_grad(QPFunction(verbose=-1, solver=QPSolvers.CVXPY))
        finally:
            external.set_solver(None)
        h2, leaf = second_grad(QPFunction(verbose=-1))
        with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):
            torch.autograd.grad(h2.sum(), leaf)
