"""QPFunction(duals=True) on the host-thread emulator: (zhat, nu, lam, slacks) as outputs, lam and nu differentiable.  The
backward of a loss l(zhat, lam, nu) is the backward's kernel with the right-hand side (dl/dzhat, 0, dl/dlam, dl/dnu)
(qpx_backward_duals).  Checked in every kernel family against a float64 dense solve at the forward's own
solution, against gradients produced by the unmodified reference (tests/golden/make_golden_duals.py), against forward mode
by the adjoint identity, against central finite differences of the reference's (zhat, lam, nu), and case by case: cotangents
on a subset of the outputs, shared parameters, no equality constraints, float32, the external-solver path, the slacks,
and the argument checks of the C ABI."""
import ctypes

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import problems
import test_emu_jvp as J
from conftest import load_golden
from duals_reference import NAMES, checksum, dense_grads, dense_tol, rel
from emu.harness import emu_lib, emulated
from qpth_amd import _lib
from qpth_amd.kkt import KKTFactors
from qpth_amd.qp import QPFunction, QPSolvers

_t = J._t


def cotangents(B, n, m, q, seed, which=("z", "lam", "nu")):
    r = np.random.RandomState(seed)
    gz, gl, gn = r.randn(B, n), r.randn(B, m), r.randn(B, q)
    return (gz if "z" in which else None, gl if "lam" in which else None, gn if ("nu" in which and q) else None)


def leaves(arrs, dtype=torch.float64):
    tq = [_t(x, dtype) for x in arrs]
    for x in tq:
        if x.nelement():
            x.requires_grad_(True)
    return tq


def grads_of(arrs, cots, dtype=torch.float64, threads=128, variant=0, **kw):
    """outputs of QPFunction(duals=True) and the gradients of  <g_z, zhat> + <g_lam, lam> + <g_nu, nu>  (a cotangent of
    None: that output does not enter the loss)"""
    tq = leaves(arrs, dtype)
    with emulated(threads, variant):
        z, nu, lam, sl = QPFunction(verbose=-1, duals=True, **kw)(*tq)
        loss = sum((o * _t(g, dtype)).sum() for o, g in zip((z, lam, nu), cots) if g is not None)
        loss.backward()
    outs = [o.detach().numpy() for o in (z, lam, sl, nu)]
    return outs, {k: (x.grad.numpy() if x.grad is not None else None) for k, x in zip(NAMES, tq)}


def check_against_dense(arrs, cots, tol, threads=128, variant=0):
    sol, grads = grads_of(arrs, cots, threads=threads, variant=variant)
    mine = J.solution_of(arrs, threads, variant)
    for a, c in zip(sol, mine):
        assert np.array_equal(a, c)                         # the outputs ARE the forward's solution
    ref = dense_grads(arrs, sol, cots)
    worst = {k: rel(grads[k], ref[k]).max() for k in ref}
    print("dense-solve gaps", {k: "%.2e" % v for k, v in worst.items()}, "tol %.1e" % tol)
    assert max(worst.values()) <= tol, worst


# ---------------------------------------------------------------- 1. every kernel form against the dense solve
@pytest.mark.parametrize("variant", J.FORMS)
@pytest.mark.parametrize("shape", [(2, 12, 9, 3), (1, 40, 52, 0)])
def test_every_kernel_form_against_the_dense_solve(variant, shape):
    B, n, m, q = shape
    arrs = problems.random_dense_qp(B, n, m, q, seed=11)
    check_against_dense(arrs, cotangents(B, n, m, q, 5), dense_tol(n, m, q), variant=variant)


def test_chain_wave_form_against_the_dense_solve():
    arrs = problems.random_dense_qp(2, 20, 70, 3, seed=11)
    check_against_dense(arrs, cotangents(2, 20, 70, 3, 6), dense_tol(20, 70, 3), threads=256)


def test_large_qp_family_two_blocks_against_the_dense_solve():
    arrs = problems.random_dense_qp(2, 70, 80, 5, seed=18)
    check_against_dense(arrs, cotangents(2, 70, 80, 5, 19), dense_tol(70, 80, 5), threads=256, variant=3)


# ---------------------------------------------------------------- 2. gradients of the unmodified reference
@pytest.mark.parametrize("name,gen,threads", [
    ("duals_b4_n100_m100", lambda: problems.prof_qp(4, 100, 100, 0, 0), 256),
    ("duals_b4_n100_m50_q10", lambda: problems.prof_qp(4, 100, 50, 10, 0), 256),
    ("duals_b2_n12_m9_q3", lambda: problems.random_dense_qp(2, 12, 9, 3, seed=24), 128)])
def test_gradients_of_the_reference(name, gen, threads):
    """end to end (our forward, our backward) against the reference's forward + factor_kkt + solve_kkt(g_z, 0, g_lam, g_nu)
    + qp.py:157-173; the project's parity gate, 1e-6 relative, per QP and gradient"""
    g = load_golden(name)
    arrs = gen()
    assert np.allclose(checksum(*arrs), g["input_checksum"], rtol=1e-12)
    q = g["nu"].shape[1]
    sol, grads = grads_of(arrs, (g["g_z"], g["g_lam"], g["g_nu"] if q else None), threads=threads)
    for a, k in zip(sol, ("zhat", "lam", "slacks") + (("nu",) if q else ())):
        assert np.abs(a - g[k]).max() <= 1e-6 * max(1.0, np.abs(g[k]).max()), k
    worst = {k: rel(grads[k], g[k]).max() for k in NAMES if k in g}
    print("reference gaps", {k: "%.2e" % v for k, v in worst.items()}, "reference's own LU-vs-dense %.2e" % g["lu_vs_dense_gap"])
    assert float(g["lu_vs_dense_gap"]) < 1e-6              # the gate is not vacuous for the reference itself
    assert max(worst.values()) <= 1e-6, worst


# ---------------------------------------------------------------- 4. the adjoint of forward mode
def tangents_of_outputs(arrs, tans, threads=128, variant=0, **kw):
    prim = [_t(x) for x in arrs]
    with emulated(threads, variant):
        with fwAD.dual_level():
            ins = [fwAD.make_dual(x, _t(t)) if t is not None else x for x, t in zip(prim, tans)]
            outs = QPFunction(verbose=-1, duals=True, **kw)(*ins)
            z, nu, lam, sl = [fwAD.unpack_dual(o) for o in outs]
    assert sl.tangent is None                               # the slacks are not differentiable
    return z.tangent.numpy(), lam.tangent.numpy(), (nu.tangent.numpy() if nu.tangent is not None else None)


def adjoint_gap(tangs, cots, grads, tans, B):
    """|<g_z, z'> + <g_lam, lam'> + <g_nu, nu'> - sum <grad, tangent>| over the sum of the terms' magnitudes, per QP
    (normalised as tests/test_gpu_jvp.py: adjoint_gap)"""
    lhs_terms = np.stack([np.einsum("bi,bi->b", g, t) for g, t in zip(cots, tangs) if g is not None and t is not None])
    _, terms = J.adjoint_terms(np.zeros_like(tangs[0]), np.zeros_like(tangs[0]), [grads[k] for k in NAMES], tans, B)
    return np.abs(lhs_terms.sum(0) - terms.sum(0)) / (np.abs(terms).sum(0) + np.abs(lhs_terms).sum(0))


@pytest.mark.parametrize("shape,variant,threads", [((2, 12, 9, 3), 0, 128), ((2, 20, 70, 3), 0, 256),
                                                   ((2, 40, 52, 0), 256, 128), ((2, 66, 70, 5), 3, 256)])
def test_adjoint_identity_with_forward_mode(shape, variant, threads):
    B, n, m, q = shape
    arrs = problems.prof_qp(B, n, m, q, seed=2)
    tans = J.tangents_for(arrs, 8)
    cots = cotangents(B, n, m, q, 9)
    tangs = tangents_of_outputs(arrs, tans, threads, variant)
    assert (tangs[2] is None) == (q == 0)
    _, grads = grads_of(arrs, cots, threads=threads, variant=variant)
    gap = adjoint_gap(tangs, cots, grads, tans, B)
    print("adjoint gap %.2e" % gap.max())
    assert gap.max() <= 1e-9, gap


# ---------------------------------------------------------------- 5. finite differences of the reference
@pytest.mark.parametrize("name,shape", [("duals_fd_b2_n10_m8", (2, 10, 8, 0)), ("duals_fd_b2_n12_m9_q3", (2, 12, 9, 3))])
def test_central_finite_differences_of_the_reference(name, shape):
    """d/dt of (zhat, lam, nu) along seeded tangents of all six parameters, central differences (eps = 1e-6) of the unmodified
    reference's forward, stored with the tangents by tests/golden/make_golden_duals.py: forward mode's (z', lam', nu') output
    by output, reverse mode through <cotangent, difference> = sum <grad, tangent>; the forward-mode test's gate, 1e-4"""
    B, n, m, q = shape
    g = load_golden(name)
    arrs = problems.random_dense_qp(B, n, m, q, seed=24)
    assert np.allclose(checksum(*arrs), g["input_checksum"], rtol=1e-12)
    tans = [g["t" + k] if g["t" + k].size else None for k in "QpGhAb"]
    fd = [g["fd_z"], g["fd_lam"], g["fd_nu"] if q else None]
    cots = cotangents(B, n, m, q, 26)
    tangs = tangents_of_outputs(arrs, tans)
    for t, f in zip(tangs, fd):
        if f is not None:
            assert rel(t, f).max() <= 1e-4
    _, grads = grads_of(arrs, cots)
    lhs = sum(np.einsum("bi,bi->b", c, f) for c, f in zip(cots, fd) if c is not None)
    _, terms = J.adjoint_terms(fd[0], fd[0], [grads[k] for k in NAMES], tans, B)
    assert (np.abs(lhs - terms.sum(0)) <= 1e-4 * (np.abs(terms).sum(0) + np.abs(lhs))).all(), (lhs, terms.sum(0))


# ---------------------------------------------------------------- 6. case by case
@pytest.mark.parametrize("which", [("lam",), ("nu",), ("lam", "nu")])
def test_cotangents_on_a_subset_of_the_outputs(which):
    """a loss of lam only, of nu only: dl/dzhat reaches the kernel as NULL"""
    arrs = problems.random_dense_qp(2, 12, 9, 3, seed=12)
    check_against_dense(arrs, cotangents(2, 12, 9, 3, 13, which=which), dense_tol(12, 9, 3))


@pytest.mark.parametrize("shape,variant,threads", [((2, 12, 9, 3), 0, 128), ((2, 20, 70, 3), 0, 256), ((2, 66, 70, 5), 3, 256)])
def test_a_loss_of_zhat_alone_is_the_old_backward_bit_for_bit(shape, variant, threads):
    B, n, m, q = shape
    arrs = problems.random_dense_qp(B, n, m, q, seed=14)
    gz = cotangents(B, n, m, q, 15)[0]
    _, with_duals = grads_of(arrs, (gz, None, None), threads=threads, variant=variant)
    plain = J.grads_of(arrs, gz, threads=threads, variant=variant)
    for k, g in zip(NAMES, plain):
        assert np.array_equal(with_duals[k], g), k


def test_no_cotangent_is_none_not_zeros():
    """ctx.set_materialize_grads(False): an output the loss does not use hands the backward None, so the launch is the one
    of qpx_backward; and with dl_dz = None the C call takes the duals entry point"""
    arrs = problems.random_dense_qp(2, 12, 9, 3, seed=14)
    seen = []
    lib = emu_lib()
    real = lib.backward

    def spy(*a, **kw):
        seen.append((a[10] is None, kw.get("dl_dlam") is None, kw.get("dl_dnu") is None, "dl_dlam" in kw))
        return real(*a, **kw)

    lib.backward = spy
    try:
        grads_of(arrs, cotangents(2, 12, 9, 3, 15, which=("z",)))
        grads_of(arrs, cotangents(2, 12, 9, 3, 15, which=("lam",)))
    finally:
        del lib.backward
    assert seen == [(False, True, True, False), (True, False, True, True)]


def test_shared_parameters_equal_the_expanded_batch():
    B, n, m, q = 3, 14, 10, 2
    arrs = list(problems.random_dense_qp(B, n, m, q, seed=4))
    for i in (0, 3, 4):
        arrs[i] = arrs[i][0]                                # Q, h, A un-batched
    cots = cotangents(B, n, m, q, 10)
    _, shared = grads_of(arrs, cots)
    expanded = [np.broadcast_to(x, (B,) + x.shape).copy() if i in (0, 3, 4) else x for i, x in enumerate(arrs)]
    sol, full = grads_of(expanded, cots)
    assert shared["dQ"].shape == (n, n) and shared["dh"].shape == (m,) and shared["dA"].shape == (q, n)
    for k in NAMES:
        want = full[k].mean(0) if shared[k].ndim < full[k].ndim else full[k]         # qp.py:159-177
        assert np.abs(shared[k] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), k
    ref = dense_grads(expanded, sol, cots)
    assert max(rel(full[k], ref[k]).max() for k in NAMES) <= dense_tol(n, m, q)


def test_without_equality_constraints():
    B, n, m = 2, 10, 8
    arrs = problems.random_dense_qp(B, n, m, 0, seed=16)
    tq = leaves(arrs)
    with emulated():
        z, nu, lam, sl = QPFunction(verbose=-1, duals=True)(*tq)
    assert nu.shape == (B, 0) and not nu.requires_grad and z.requires_grad and lam.requires_grad
    with emulated():
        (lam * lam).sum().backward()
    assert tq[4].grad is None and tq[5].grad is None
    ref = dense_grads(arrs, [x.detach().numpy() for x in (z, lam, sl, nu)], (None, 2 * lam.detach().numpy(), None))
    for k, x in zip(NAMES[:4], tq):
        assert rel(x.grad.numpy(), ref[k]).max() <= dense_tol(n, m, 0), k


def test_slacks_are_returned_but_not_differentiable():
    arrs = problems.random_dense_qp(2, 12, 9, 3, seed=17)
    tq = leaves(arrs)
    with emulated():
        z, nu, lam, sl = QPFunction(verbose=-1, duals=True)(*tq)
        assert not sl.requires_grad and sl.grad_fn is None
        h, G = tq[3], tq[2]
        assert np.abs((h - torch.einsum("bmn,bn->bm", G, z)).detach().numpy() - sl.numpy()).max() <= 1e-8
        with pytest.raises(RuntimeError, match="does not require grad"):
            sl.sum().backward()
        # a loss that mixes the slacks in: they contribute nothing, the rest flows
        (sl.sum() + z.sum()).backward()
    assert tq[1].grad is not None


def test_outputs_hold_no_cycle_through_ctx():
    """ctx keeps detached aliases of lam, nu, slacks: dropping the outputs frees the graph at once (no garbage collector)"""
    import gc
    import weakref
    arrs = problems.random_dense_qp(2, 12, 9, 3, seed=17)
    gc.disable()
    try:
        with emulated():
            outs = QPFunction(verbose=-1, duals=True)(*leaves(arrs))
        node = weakref.ref(outs[2].grad_fn)
        assert node() is not None
        del outs
        assert node() is None
    finally:
        gc.enable()


@pytest.mark.parametrize("shape,variant", [((2, 20, 30, 3), 0), ((2, 66, 70, 5), 3)])
def test_float32_data_in_float64_arithmetic(shape, variant):
    """QPX_F32_WIDE: float32 cotangents widened on load through In<T>, gradients narrowed on store; against the float64 run
    on the same data -- 1e-6 relative: the rounding of the narrowed outputs (2^-24 = 6e-8 per element) and of the float32
    lam, nu, zhat the backward reads back"""
    B, n, m, q = shape
    arrs32 = problems.random_dense_qp(B, n, m, q, seed=16, dtype=np.float32)
    cots = [c.astype(np.float32) for c in cotangents(B, n, m, q, 17)]
    _, g32 = grads_of(arrs32, cots, dtype=torch.float32, threads=256, variant=variant)
    _, g64 = grads_of([np.asarray(a, np.float64) for a in arrs32], [c.astype(np.float64) for c in cots], threads=256, variant=variant)
    worst = {k: rel(g32[k], g64[k]).max() for k in NAMES}
    print("float32-wide gaps", {k: "%.2e" % v for k, v in worst.items()})
    assert all(g32[k].dtype == np.float32 for k in NAMES)
    assert max(worst.values()) <= 1e-6, worst


def test_float32_kernels_with_refinement():
    """refine=2 on float32 tensors: the float32 thread-grid kernels, the backward solve refined once; its residuals re-read
    the dual cotangents (the loop that re-forms the right-hand side).  Gate as the forward-mode test of the same solve."""
    arrs32 = problems.random_dense_qp(2, 20, 12, 2, seed=20, dtype=np.float32)
    cots = [c.astype(np.float32) for c in cotangents(2, 20, 12, 2, 21)]
    _, g32 = grads_of(arrs32, cots, dtype=torch.float32, refine=2)
    _, g64 = grads_of([np.asarray(a, np.float64) for a in arrs32], [c.astype(np.float64) for c in cots])
    assert max(rel(g32[k], g64[k]).max() for k in NAMES) <= 1e-3


@pytest.mark.parametrize("shape,threads", [((2, 12, 9, 3), 128), ((2, 20, 70, 3), 256)], ids=["one_wave", "chain_wave"])
def test_refinement_re_reads_the_dual_cotangents(shape, threads):
    """float64, KKTFactors.backward(refine=1) with cotangents on lam and nu, in the one-wave and in the chain-wave tile form: a
    refinement step on a converged solve changes nothing beyond rounding -- it would, by O(1), if the right-hand side kept for
    the residuals (vLM, vNU) dropped dl_dlam or dl_dnu -- and the refined gradients meet the dense solve"""
    B, n, m, q = shape
    arrs = problems.random_dense_qp(B, n, m, q, seed=12)
    Q, p, G, h, A, b = [_t(x) for x in arrs]
    cots = cotangents(B, n, m, q, 13)
    gz, gl, gn = [_t(c) for c in cots]
    with emulated(threads):
        fac = KKTFactors.build(Q, G, A)
        r = fac.ipm(p, h, b)
        g0 = fac.backward(r.zhat, r.lam, r.slacks, r.nu, gz, dl_dlam=gl, dl_dnu=gn)
        g1 = fac.backward(r.zhat, r.lam, r.slacks, r.nu, gz, dl_dlam=gl, dl_dnu=gn, refine=1)
        with pytest.raises(RuntimeError, match="at least one of"):
            fac.backward(r.zhat, r.lam, r.slacks, r.nu, None)
    ref = dense_grads(arrs, [x.numpy() for x in (r.zhat, r.lam, r.slacks, r.nu)], cots)
    for k, a, c in zip(NAMES, g0, g1):
        assert rel(c.numpy(), a.numpy()).max() <= 1e-9, k
        assert rel(c.numpy(), ref[k]).max() <= dense_tol(n, m, q), k


def test_large_qp_family_in_two_parts():
    """knob bits 16..19 = 2: the batch is split into two parts on two streams, each with its own offsets into dl_dlam and
    dl_dnu (advio); three QPs, so the parts differ in length"""
    B, n, m, q = 3, 20, 24, 3
    arrs = problems.random_dense_qp(B, n, m, q, seed=27)
    check_against_dense(arrs, cotangents(B, n, m, q, 28), dense_tol(n, m, q), threads=256, variant=3 | (2 << 16))


def test_external_solver_path():
    """QPSolvers.CVXPY (ctx.fac is None): the forward by an external solver (a stand-in that replays the kernels' own
    solution), the backward on factors rebuilt from Q, G, A"""
    from qpth_amd.solvers import external
    B, n, m, q = 3, 12, 9, 3
    arrs = problems.random_dense_qp(B, n, m, q, seed=22)
    cots = cotangents(B, n, m, q, 23)
    sol = J.solution_of(arrs)
    calls = []

    def replay(Q, p, G, h, A, b):
        i = len(calls)
        calls.append(i)
        return sol[0][i], sol[3][i], sol[1][i], sol[2][i]

    external.set_solver(replay)
    try:
        outs, grads = grads_of(arrs, cots, solver=QPSolvers.CVXPY)
    finally:
        external.set_solver(None)
    assert len(calls) == B
    for a, c in zip(outs, sol):
        assert np.array_equal(a, c)
    ref = dense_grads(arrs, sol, cots)
    assert max(rel(grads[k], ref[k]).max() for k in NAMES) <= dense_tol(n, m, q)


def test_duals_false_is_unchanged():
    arrs = problems.random_dense_qp(2, 12, 9, 3, seed=12)
    with emulated():
        z = QPFunction(verbose=-1)(*leaves(arrs))
        z2 = QPFunction(verbose=-1, duals=False)(*leaves(arrs))
    assert isinstance(z, torch.Tensor) and torch.equal(z, z2)


# ---------------------------------------------------------------- the C ABI
def test_argument_errors():
    lib = emu_lib()
    B, n, m = 1, 4, 3
    fac = np.zeros(lib.factor_elems(_lib.QPX_F64, n, m, 2))
    zh, gz, gl, gn, lam, sl, nu = [np.zeros(64) for _ in range(7)]
    st = np.zeros(B, np.int32)

    def p(a):
        return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None

    def call(dtype=_lib.QPX_F64, zhat=zh, dl_dz=None, dl_dlam=None, dl_dnu=None, q=0, nu_=None, refine=0):
        return lib.dll.qpx_backward_duals(dtype, B, n, m, q, p(fac), 0, p(zhat), p(lam), p(sl), p(nu_), p(dl_dz), p(dl_dlam), p(dl_dnu),
                                          None, None, None, None, None, None, None, None, None, refine,
                                          None, 0, None, 0, None, 0, p(st), None)

    assert call() == -1                                      # all three cotangents NULL: QPX_ERR_ARG
    assert call(dl_dnu=gn) == -1                             # ... dl_dnu does not count without equality constraints
    assert call(q=2, nu_=nu) == -1
    assert call(dl_dlam=gl, zhat=None) == -1
    assert call(dl_dlam=gl, dtype=7) == -1
    assert call(dl_dlam=gl, q=2) == -1                       # equality constraints need nu
    assert call(dl_dz=gz, refine=-1) == -1
    # qpx_backward keeps requiring dl_dz
    assert lib.dll.qpx_backward(_lib.QPX_F64, B, n, m, 0, p(fac), 0, p(zh), p(lam), p(sl), None, None,
                                None, None, None, None, None, None, None, None, None, 0,
                                None, 0, None, 0, None, 0, p(st), None) == -1
