"""Warm start of the PDIPM loop (KKTFactors.ipm(warm=...), QPFunction(warm_start=...), qpx_ipm_warm) on the
host-thread emulator: the loop entered at a previous solution's (lam, slacks) instead of the reference's start point.

Inputs everywhere: problems.prof_qp(B, n, m, q, seed=11) as the base problem, solved cold by the oracle; the perturbed
problem p' = p + delta randn, h' = h + delta rand from RandomState(7) (tests/warm_reference.py: perturb); the warm start is
the base problem's (lam, slacks).  The reference of the warm loop is tests/warm_reference.py (numpy float64, dense KKT
solves), the reference of the solution the oracle's cold solve of the perturbed problem.

Iteration counts of the kernels (against warm_reference's, and warm against cold) are compared at eps = EPS_COUNT = 1e-9, in
the kernel and in the reference alike, not at the default 1e-12.  The kernels evaluate the primal residual in the condensed
variables, rz = s - c - R z, whose round-off floor is about cond(Q) 2^-52 |c|: 1e-12 .. 1e-11 on this generator where
nz < nineq (R = G Q^-1 G^T is rank deficient there), which is ABOVE the default eps.  There the count at eps = 1e-12 under
stall policy 1 is "the pass that reached the floor + however long the residual wanders at the floor until three passes in
a row do not improve it", cold and warm alike: it counts round-off, not convergence, while the dense reference goes below
1e-12 and stops.  (Measured, (2,30,100,0) on the 16x16 grid, cold / warm / reference: [20 15] / [17 16] / [7 7]; the 8x8
grid at (2,20,70,3): [13 12] / [14 6] / [6 6]; the iterates agree with the reference's to four digits in every pass down
to the floor.  The tile forms: [20 18] / [13 13].  test_every_form prints the counts at 1e-12 too.)  1e-9 lies above that
floor and below the residual of every pass that has not converged (the residual falls by ~1e-3 per pass at the end), so
the count there is the number of passes to convergence, which is what the checks are about.  The solution itself is
checked at the default eps.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import problems
import test_emu_duals as D
import test_emu_jvp as J
import warm_reference as W
from conftest import rel_err
from emu.harness import emu_lib, emulated
from oracle import qp_oracle as orc
from qpth_amd import WarmStart, _lib, sensitivity
from qpth_amd.kkt import KKTFactors
from qpth_amd.qp import QPFunction
from test_emu_parity import LOOP_FORMS

TOL = 1e-6
EPS_COUNT = 1e-9
FORMS = [v for v in LOOP_FORMS if v != 3]                 # every form of the thread-grid / tile kernels
FORM_SHAPES = [(2, 12, 9, 3), (1, 40, 52, 0), (2, 20, 70, 3), (2, 30, 100, 0)]     # the last two: chain-wave sizes
QPX_ERR_ARG, QPX_ERR_UNSUPPORTED = -1, -2                 # include/qpx.h

_t = J._t


@functools.lru_cache(maxsize=None)
def problem(shape, delta):
    """base problem, perturbed problem, the oracle's cold solutions of both (stall policy 1, per QP)"""
    base = problems.prof_qp(*shape, seed=W.SEED)
    pert = W.perturb(base, delta)
    sols = []
    for arrs in (base, pert):
        x, y, lam, s, _, info = orc.qp_forward_backward(*arrs, per_qp=True, stall_policy=1)
        sols.append(dict(zhat=x, nu=y, lam=lam, slacks=s, iters=info["iters"]))
    return base, pert, sols[0], sols[1]


@functools.lru_cache(maxsize=None)
def reference(shape, delta, eps=1e-12):
    base, pert, sb, _ = problem(shape, delta)
    return W.solve(*pert, lam0=sb["lam"], s0=sb["slacks"], eps=eps)


def as_np(res):
    out = {k: getattr(res, k).numpy().copy() for k in ("zhat", "lam", "slacks", "iters", "best_resid", "warm_used")}
    out["nu"] = res.nu.numpy().copy()
    out["trace"] = res.trace.numpy().copy() if res.trace is not None else None
    return out


def factors(arrs, B, dtype=torch.float64, wide=False):
    Q, p, G, h, A, b = [_t(x, dtype) for x in arrs]
    return KKTFactors.build(Q, G, A, B, wide=wide), p, h, b


@functools.lru_cache(maxsize=None)
def run_form(variant, shape, delta, eps=1e-12):
    """cold and warm run of one form on the perturbed problem, same factors, stall policy 1"""
    base, pert, sb, _ = problem(shape, delta)
    warm = (_t(sb["lam"]), _t(sb["slacks"]))
    with emulated(256, variant):
        fac, p, h, b = factors(pert, shape[0])
        cold = as_np(fac.ipm(p, h, b, eps=eps, stall_policy=1))
        hot = as_np(fac.ipm(p, h, b, eps=eps, stall_policy=1, warm=warm))
    return cold, hot


def close_to(res, sol, q, tol=TOL):
    worst = {k: rel_err(res[k], sol[k]).max() for k in ("zhat", "lam", "slacks") + (("nu",) if q else ())}
    assert max(worst.values()) < tol, worst


# ---------------------------------------------------------------- 1. the reference alone
def test_reference_alone():
    """pins the inputs: from the base solution at delta = 1e-3 the dense float64 loop reaches the oracle's cold solution of
    the perturbed QP in at most cold - 1 passes per QP and at most 0.7 of the cold passes in all"""
    cold_sum = warm_sum = 0
    for shape in W.TABLE_SHAPES:
        _, _, _, sp = problem(shape, 1e-3)
        r = reference(shape, 1e-3)
        print(shape, "cold", sp["iters"], "warm", r["iters"])
        close_to(r, sp, shape[3])
        assert (r["iters"] <= sp["iters"] - 1).all(), (shape, r["iters"], sp["iters"])
        cold_sum += int(sp["iters"].sum())
        warm_sum += int(r["iters"].sum())
    print("sum: cold %d warm %d ratio %.3f" % (cold_sum, warm_sum, warm_sum / cold_sum))
    assert warm_sum <= 0.7 * cold_sum


# ---------------------------------------------------------------- 2. every form of the thread-grid / tile kernels
@pytest.mark.parametrize("delta", [1e-3, 0.1])
@pytest.mark.parametrize("shape", FORM_SHAPES)
@pytest.mark.parametrize("variant", FORMS)
def test_every_form(variant, shape, delta):
    _, _, _, sp = problem(shape, delta)
    cold, hot = run_form(variant, shape, delta)
    print("iters cold", cold["iters"], "warm", hot["iters"], "reference at 1e-12", reference(shape, delta)["iters"])
    close_to(hot, sp, shape[3])
    assert (hot["warm_used"] == 1).all() and (cold["warm_used"] == 0).all()
    # the counts, at an eps above the condensed residual's round-off floor (see the top of the file)
    ref = reference(shape, delta, EPS_COUNT)
    cold9, hot9 = run_form(variant, shape, delta, EPS_COUNT)
    print("iters at eps = 1e-9: cold", cold9["iters"], "warm", hot9["iters"], "reference", ref["iters"])
    close_to(hot9, sp, shape[3])
    assert (np.abs(hot9["iters"] - ref["iters"]) <= 1).all(), (hot9["iters"], ref["iters"])
    if delta == 1e-3:
        assert (hot9["iters"] < cold9["iters"]).all(), (hot9["iters"], cold9["iters"])


@pytest.mark.parametrize("variant", FORMS)
def test_every_form_saves_passes_in_all(variant):
    """summed over the shapes of test_every_form at delta = 1e-3: warm passes <= 0.7 x the same form's cold passes"""
    cold_sum = warm_sum = 0
    for shape in FORM_SHAPES:
        cold, hot = run_form(variant, shape, 1e-3, EPS_COUNT)
        cold_sum += int(cold["iters"].sum())
        warm_sum += int(hot["iters"].sum())
    print("cold %d warm %d ratio %.3f" % (cold_sum, warm_sum, warm_sum / cold_sum))
    assert warm_sum <= 0.7 * cold_sum


# ---------------------------------------------------------------- 3. the entry state
@pytest.mark.parametrize("variant,shape", [(0, (2, 12, 9, 3)), (256, (2, 12, 9, 3)), (1024 + 2048, (1, 40, 52, 0)), (0, (2, 20, 70, 3))])
def test_entry_state(variant, shape):
    """entries below the floor and negative ones are floored; pass 0 sees mu and the primal residual of the reference's
    entry point, and a dual residual of exactly zero (sigma_z = 0: the start is dual-feasible by construction)"""
    B, n, m, q = shape
    _, pert, sb, _ = problem(shape, 1e-3)
    lam0, s0 = sb["lam"].copy(), sb["slacks"].copy()
    lam0[:, 0], lam0[:, 1], s0[:, 2], s0[:, 3] = -0.5, 1e-5, -2.0, 3e-3
    assert (lam0 < W.FLOOR).any() and (s0 < W.FLOOR).any()
    ref = W.solve(*pert, lam0=lam0, s0=s0)
    with emulated(256, variant):
        fac, p, h, b = factors(pert, B)
        res = as_np(fac.ipm(p, h, b, stall_policy=1, warm=(_t(lam0), _t(s0)), want_trace=True))
    assert (res["warm_used"] == 1).all()
    for i in range(B):
        pri, dual, mu = res["trace"][0, i]
        rpri, _, rmu = ref["trace"][i][0]
        print("QP %d: pri %.12e (ref %.12e) mu %.12e (ref %.12e) dual %g" % (i, pri, rpri, mu, rmu, dual))
        assert abs(mu - rmu) <= 1e-9 * rmu and abs(pri - rpri) <= 1e-9 * rpri
        assert dual == 0.0


# ---------------------------------------------------------------- 4. a NaN or an Inf: that QP starts cold
@pytest.mark.parametrize("variant,shape", [(256, (4, 12, 9, 3)), (1024 + 2048, (4, 12, 9, 3)), (0, (4, 20, 70, 3))])
def test_non_finite_entries_start_cold(variant, shape):
    B, n, m, q = shape
    _, pert, sb, _ = problem(shape, 1e-3)
    lam0, s0 = sb["lam"].copy(), sb["slacks"].copy()
    lam0[1, m - 1] = np.nan
    s0[2, 0] = np.inf
    with emulated(256, variant):
        fac, p, h, b = factors(pert, B)
        cold = as_np(fac.ipm(p, h, b, stall_policy=1))
        hot = as_np(fac.ipm(p, h, b, stall_policy=1, warm=(_t(lam0), _t(s0))))
    assert hot["warm_used"].tolist() == [1, 0, 0, 1]
    for k in ("zhat", "lam", "slacks", "nu", "iters", "best_resid"):
        assert np.array_equal(hot[k][1:3], cold[k][1:3]), k


# ---------------------------------------------------------------- 5. no warm start: qpx_ipm as it was
def raw_ipm_warm(lib, fac, p, h, b, lam0, s0, floor, used, stall_policy=1):
    """qpx_ipm_warm called directly; returns (code, outputs)"""
    B, n, m, q = fac.B, fac.n, fac.m, fac.q
    dt = p.dtype
    out = dict(zhat=torch.empty(B, n, dtype=dt), nu=torch.empty(B, q, dtype=dt), lam=torch.empty(B, m, dtype=dt),
               slacks=torch.empty(B, m, dtype=dt), iters=torch.empty(B, dtype=torch.int32), best_resid=torch.empty(B, dtype=dt))
    ptr = _lib._ptr
    code = lib.dll.qpx_ipm_warm(
        _lib.QPX_F64, B, n, m, q, ptr(p), n, ptr(h), m, ptr(b) if q else None, q, ptr(fac.blob), int(fac.sfac), 1e-12, 20, 3,
        stall_policy, ptr(out["zhat"]), ptr(out["nu"]) if q else None, ptr(out["lam"]), ptr(out["slacks"]), ptr(out["iters"]),
        ptr(fac.status), ptr(out["best_resid"]), None, ptr(lam0), ptr(s0), ctypes.c_double(floor), ptr(used), None)
    return code, out


@pytest.mark.parametrize("variant,shape", [(256, (2, 12, 9, 3)), (1024 + 2048, (1, 40, 52, 0)), (0, (2, 20, 70, 3))])
def test_without_a_warm_start_the_call_is_qpx_ipm(variant, shape):
    _, pert, _, _ = problem(shape, 1e-3)
    with emulated(256, variant):
        fac, p, h, b = factors(pert, shape[0])
        mine = as_np(fac.ipm(p, h, b, stall_policy=1, warm=None))
        code, raw = raw_ipm_warm(emu_lib(), fac, p, h, b, None, None, 1e-2, None)
    assert code == 0
    assert (mine["warm_used"] == 0).all()
    for k in ("zhat", "lam", "slacks", "iters", "best_resid") + (("nu",) if shape[3] else ()):
        assert np.array_equal(mine[k], raw[k].numpy()), k


# ---------------------------------------------------------------- 6. the large-QP family and the argument errors
@pytest.mark.parametrize("shape", [(2, 12, 9, 3), (2, 70, 80, 5)])
def test_large_qp_family_starts_cold(shape):
    B, n, m, q = shape
    _, pert, sb, _ = problem(shape, 1e-3)
    lam0, s0 = _t(sb["lam"]), _t(sb["slacks"])
    lib = emu_lib()
    with emulated(256, 3):
        assert lib.dll.qpx_warm_supported(_lib.QPX_F64, n, m, q) == 0
        fac, p, h, b = factors(pert, B)
        cold = as_np(fac.ipm(p, h, b, stall_policy=1))
        hot = as_np(fac.ipm(p, h, b, stall_policy=1, warm=(lam0, s0)))
        used = torch.zeros(B, dtype=torch.int32)
        code, _ = raw_ipm_warm(lib, fac, p, h, b, lam0, s0, 1e-2, used)
    assert code == QPX_ERR_UNSUPPORTED
    assert (hot["warm_used"] == 0).all()
    for k in ("zhat", "lam", "slacks", "nu", "iters", "best_resid"):
        assert np.array_equal(hot[k], cold[k]), k


def test_argument_errors():
    shape = (2, 12, 9, 3)
    _, pert, sb, _ = problem(shape, 1e-3)
    lam0, s0 = _t(sb["lam"]), _t(sb["slacks"])
    lib = emu_lib()
    with emulated(128, 0):
        assert lib.dll.qpx_warm_supported(_lib.QPX_F64, 12, 9, 3) == 1
        assert lib.dll.qpx_warm_supported(_lib.QPX_F32, 12, 9, 3) == 1
        assert lib.dll.qpx_warm_supported(_lib.QPX_F32_WIDE, 12, 9, 3) == 1
        assert lib.dll.qpx_warm_supported(_lib.QPX_F64, 150, 150, 0) == 0
        assert lib.dll.qpx_warm_supported(7, 12, 9, 3) == 0
        fac, p, h, b = factors(pert, shape[0])
        assert raw_ipm_warm(lib, fac, p, h, b, lam0, None, 1e-2, None)[0] == QPX_ERR_ARG
        assert raw_ipm_warm(lib, fac, p, h, b, None, s0, 1e-2, None)[0] == QPX_ERR_ARG
        for bad in (0.0, -1e-2, float("nan"), float("inf")):
            assert raw_ipm_warm(lib, fac, p, h, b, lam0, s0, bad, None)[0] == QPX_ERR_ARG, bad
        code, out = raw_ipm_warm(lib, fac, p, h, b, lam0, s0, 1e-2, None)          # warm_used may be NULL
        assert code == 0 and torch.isfinite(out["zhat"]).all()
        with pytest.raises(ValueError, match="warm_floor"):
            fac.ipm(p, h, b, warm=(lam0, s0), warm_floor=0.0)
        with pytest.raises(RuntimeError, match="lam0"):
            fac.ipm(p, h, b, warm=(lam0[:, :5], s0))
    with pytest.raises(ValueError, match="floor"):
        WarmStart(floor=-1.0)


# ---------------------------------------------------------------- 7. starts far from the solution
@pytest.mark.parametrize("kind", ["ones", "noise"])
@pytest.mark.parametrize("variant,shape", [(256, (2, 12, 9, 3)), (1024 + 2048, (1, 40, 52, 0)), (0, (2, 20, 70, 3)), (0, (2, 30, 100, 0))])
def test_far_starts(variant, shape, kind):
    B, n, m, q = shape
    _, pert, _, sp = problem(shape, 1e-3)
    if kind == "ones":
        lam0, s0 = np.ones((B, m)), np.ones((B, m))
    else:
        rs = [np.random.RandomState(100 + k) for k in range(B)]
        lam0 = np.stack([r.rand(m) * 3 for r in rs])
        s0 = np.stack([r.rand(m) * 3 for r in rs])
    ref = W.solve(*pert, lam0=lam0, s0=s0, maxIter=30)
    close_to(ref, sp, q)                                     # the input is one the reference itself solves
    with emulated(256, variant):
        fac, p, h, b = factors(pert, B)
        res = as_np(fac.ipm(p, h, b, maxIter=30, stall_policy=1, warm=(_t(lam0), _t(s0))))
    print("iters", res["iters"], "reference", ref["iters"])
    assert (res["warm_used"] == 1).all()
    close_to(res, sp, q)


# ---------------------------------------------------------------- 8. data types and shared factors
@pytest.mark.parametrize("shape", [(1, 40, 52, 0), (2, 20, 70, 3)])
def test_float32_tensors_in_float64_arithmetic(shape):
    """QPX_F32_WIDE: lam0, s0 are float32 arrays too; against the float64 warm run on the same float32-rounded data"""
    B, n, m, q = shape
    _, pert, sb, _ = problem(shape, 1e-3)
    a32 = [np.asarray(x, np.float32) for x in pert]
    a64 = [np.asarray(x, np.float64) for x in a32]
    w32 = (np.asarray(sb["lam"], np.float32), np.asarray(sb["slacks"], np.float32))
    with emulated(256, 0):
        f32, p, h, b = factors(a32, B, torch.float32, wide=True)
        r32 = f32.ipm(p, h, b, warm=(_t(w32[0], torch.float32), _t(w32[1], torch.float32)))
        f64, p, h, b = factors(a64, B)
        r64 = f64.ipm(p, h, b, warm=(_t(w32[0]), _t(w32[1])))
    assert r32.zhat.dtype == torch.float32 and f32.blob.dtype == torch.float64
    assert (r32.warm_used == 1).all() and (r64.warm_used == 1).all()
    assert torch.equal(r32.iters, r64.iters)
    for k in ("zhat", "lam", "slacks") + (("nu",) if q else ()):
        assert rel_err(getattr(r32, k).numpy(), getattr(r64, k).numpy()).max() < 1e-6, k


def test_pure_float32_on_a_thread_grid():
    """the float32 kernels alone (refine = 0): warm against the same kernels' cold result, at the gate of test_float32"""
    shape = (2, 12, 9, 3)
    _, pert, sb, _ = problem(shape, 1e-3)
    a32 = [np.asarray(x, np.float32) for x in pert]
    with emulated(256, 256):
        fac, p, h, b = factors(a32, shape[0], torch.float32)
        cold = fac.ipm(p, h, b)
        hot = fac.ipm(p, h, b, warm=(_t(sb["lam"], torch.float32), _t(sb["slacks"], torch.float32)))
    assert (hot.warm_used == 1).all()
    err = rel_err(hot.zhat.numpy(), cold.zhat.numpy())
    print("float32 warm against cold", err)
    assert err.max() < 5e-3


@pytest.mark.parametrize("delta", [1e-3, 0.1])
@pytest.mark.parametrize("variant,shape", [(256, (2, 12, 9, 3)), (0, (2, 20, 70, 3))])
def test_shared_factors(variant, shape, delta):
    """un-batched Q, G, A (one factor blob, sfac = 0) with batched p, h: QP 0's matrices for the whole batch, p and h of
    QP 0 moved apart per QP (h only loosens: feasible), then the perturbation; the checks of test_every_form"""
    B, n, m, q = shape
    Q, p, G, h, A, b = problems.prof_qp(B, n, m, q, seed=W.SEED)
    r = np.random.RandomState(3)
    Q0, G0 = Q[0], G[0]
    A0, b0 = (A[0], b[0]) if q else (A, b)
    base = (Q0, p[:1] + 0.1 * r.randn(B, n), G0, h[:1] + 0.1 * r.rand(B, m), A0, b0)
    pert = W.perturb(base, delta)
    exp = lambda arrs: (np.broadcast_to(Q0, (B, n, n)), arrs[1], np.broadcast_to(G0, (B, m, n)), arrs[3],      # noqa: E731
                        np.broadcast_to(A0, (B, q, n)) if q else A0, np.broadcast_to(b0, (B, q)) if q else b0)
    xb, yb, lb, sb, _, _ = orc.qp_forward_backward(*exp(base), per_qp=True, stall_policy=1)
    xp, yp, lp, sp, _, _ = orc.qp_forward_backward(*exp(pert), per_qp=True, stall_policy=1)
    sol = dict(zhat=xp, nu=yp, lam=lp, slacks=sp)
    with emulated(256, variant):
        fac, pt, ht, bt = factors(pert, B)
        assert fac.shared and fac.sfac == 0
        cold = as_np(fac.ipm(pt, ht, bt, stall_policy=1))
        hot = as_np(fac.ipm(pt, ht, bt, stall_policy=1, warm=(_t(lb), _t(sb))))
        cold9 = as_np(fac.ipm(pt, ht, bt, eps=EPS_COUNT, stall_policy=1))
        hot9 = as_np(fac.ipm(pt, ht, bt, eps=EPS_COUNT, stall_policy=1, warm=(_t(lb), _t(sb))))
    ref = W.solve(*exp(pert), lam0=lb, s0=sb, eps=EPS_COUNT)
    print("iters cold", cold["iters"], "warm", hot["iters"], "at 1e-9", hot9["iters"], "reference", ref["iters"])
    close_to(hot, sol, q)
    assert (hot["warm_used"] == 1).all()
    assert (np.abs(hot9["iters"] - ref["iters"]) <= 1).all()
    if delta == 1e-3:
        assert (hot9["iters"] < cold9["iters"]).all()


# ---------------------------------------------------------------- 9. the public surface
def leaves(arrs):
    return D.leaves(arrs)


def test_qpfunction_two_calls():
    shape = (2, 20, 70, 3)
    B, n, m, q = shape
    base, pert, _, _ = problem(shape, 1e-3)
    dl = np.random.RandomState(5).randn(B, n)
    _, _, _, _, grads_ref, _ = orc.qp_forward_backward(*pert, dl, per_qp=True, stall_policy=2)
    ws = WarmStart()
    assert ws.lam is None and ws.used is None
    with emulated(256, 0):
        z1 = QPFunction(verbose=-1, warm_start=ws)(*leaves(base))
        assert ws.lam.shape == (B, m) and not ws.lam.requires_grad and (ws.used == 0).all()        # the first call is cold
        first = ws.lam
        tq = leaves(pert)
        z2 = QPFunction(verbose=-1, warm_start=ws)(*tq)
        z2.backward(_t(dl))
    assert (ws.used == 1).all() and ws.lam is not first
    _, _, _, sp = problem(shape, 1e-3)
    assert rel_err(z2.detach().numpy(), sp["zhat"]).max() < TOL
    for x, ref in zip(tq, grads_ref):
        if ref is not None and x.grad is not None:
            assert np.abs(x.grad.numpy() - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    ws.clear()
    assert ws.lam is None and ws.slacks is None and ws.used is None


def test_duals_adjoint_identity_at_the_warm_solution():
    shape = (2, 12, 9, 3)
    B, n, m, q = shape
    base, pert, _, _ = problem(shape, 1e-3)
    tans = J.tangents_for(pert, 8)
    cots = D.cotangents(B, n, m, q, 9)
    ws = WarmStart()
    with emulated(128, 0):
        QPFunction(verbose=-1, warm_start=ws)(*[_t(x) for x in base])
        with fwAD.dual_level():
            ins = [fwAD.make_dual(_t(x), _t(t)) if t is not None else _t(x) for x, t in zip(pert, tans)]
            outs = QPFunction(verbose=-1, duals=True, warm_start=ws)(*ins)
            z, nu, lam, sl = [fwAD.unpack_dual(o) for o in outs]
            tangs = (z.tangent.numpy(), lam.tangent.numpy(), nu.tangent.numpy())
        assert (ws.used == 1).all()
        tq = leaves(pert)
        z, nu, lam, sl = QPFunction(verbose=-1, duals=True, warm_start=ws)(*tq)
        sum((o * _t(g)).sum() for o, g in zip((z, lam, nu), cots)).backward()
        assert (ws.used == 1).all()
    grads = {k: x.grad.numpy() for k, x in zip(D.NAMES, tq)}
    gap = D.adjoint_gap(tangs, cots, grads, tans, B)
    print("adjoint gap %.2e" % gap.max())
    assert gap.max() <= 1e-9, gap


def test_a_holder_of_another_shape_is_ignored_and_overwritten():
    base, _, _, _ = problem((2, 12, 9, 3), 1e-3)
    other = problems.prof_qp(1, 40, 52, 0, seed=W.SEED)
    ws = WarmStart()
    with emulated(128, 0):
        QPFunction(verbose=-1, warm_start=ws)(*[_t(x) for x in base])
        assert ws.lam.shape == (2, 9)
        cold = QPFunction(verbose=-1)(*[_t(x) for x in other])
        z = QPFunction(verbose=-1, warm_start=ws)(*[_t(x) for x in other])
        assert ws.lam.shape == (1, 52) and (ws.used == 0).all()
        assert torch.equal(z, cold)
        # ... another dtype likewise
        z32 = QPFunction(verbose=-1, warm_start=ws)(*[_t(x, torch.float32) for x in other])
        assert ws.lam.dtype == torch.float32 and (ws.used == 0).all() and z32.dtype == torch.float32
        z32b = QPFunction(verbose=-1, warm_start=ws)(*[_t(x, torch.float32) for x in other])
        assert (ws.used == 1).all() and rel_err(z32b.numpy(), z32.numpy()).max() < 1e-6


def test_sensitivity_solve():
    shape = (2, 12, 9, 3)
    base, pert, _, _ = problem(shape, 1e-3)
    ws = WarmStart()
    with emulated(128, 0):
        sensitivity.solve(*[_t(x) for x in base], warm_start=ws)
        cold = sensitivity.solve(*[_t(x) for x in pert])
        hot = sensitivity.solve(*[_t(x) for x in pert], warm_start=ws)
        assert (ws.used == 1).all()
        Jc, Jh = cold.jacobian(of=("z", "lam"), wrt=("p", "h", "b")), hot.jacobian(of=("z", "lam"), wrt=("p", "h", "b"))
    for k in Jc:
        assert np.abs(Jh[k].numpy() - Jc[k].numpy()).max() <= 1e-8 * max(1.0, np.abs(Jc[k].numpy()).max()), k
