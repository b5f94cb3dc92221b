"""Warm start and K-right-hand-side sensitivities of two-sided rows (KKTFactors.ipm_range(warm=...), qpx_ipm_range_warm,
QPFunction(warm_start=RangeWarmStart())(..., lower=l), sensitivity.solve(..., lower=l)): the checks that
tests/test_emu_range_warm.py runs on the host-thread emulator and tests/test_gpu_range_warm.py on a real MI355X.  Every check
takes an `env` as those of tests/range_checks.py: env.dev and env.run(variant=0).

Problems: tests/range_reference.py (nine shapes x {all, half}, B = 2) as the base problem; the perturbed problem at delta = 1e-3
from RandomState(warm_reference.PERTURB_SEED): p += delta randn, then h += delta rand, then lower -= delta rand, drawn in that
order (both bounds only loosen: the generator's z0 stays feasible; -inf stays -inf).  The warm start is the base problem's
solution by tests/warm_reference.py on the DOUBLED QP [G; -G_F] z <= [h; -lower_F], each QP alone, split into the two sides
(0 and +inf on the lower side of a one-sided row: what a range solve writes there).

References: warm_reference.solve on the doubled QP of the perturbed problem -- cold at eps = 1e-12 for the solution, warm at
eps = 1e-9 for the counts (tests/test_emu_warm.py says why counts are compared at 1e-9: it lies above the round-off floor of the
condensed residual and below the residual of every pass that has not converged); the library's own ipm(warm=...) on the
doubled QP at the shapes whose doubled QP the one-sided kernels serve (range_reference.COUNTED); sensitivity.solve on the
doubled QP, folded, for the K-right-hand-side solve.

Gates: 1e-6 against a reference (the project's range gate; close_to says on which vectors); 1e-12 for the one-sided equivalence (the cold equivalence's gate:
the same operations on a one-sided row); 1e-9 relative for mu and the primal residual of pass 0 (two evaluations of one
formula in float64).
"""
import ctypes
import functools

import numpy as np
import torch

import range_checks as C
import range_reference as R
import warm_reference as W
from conftest import rel_err

TOL = 1e-6
EPS_COUNT = 1e-9
DELTA = 1e-3
QPX_ERR_ARG, QPX_ERR_UNSUPPORTED = -1, -2                 # include/qpx.h
on, host, close = C.on, C.host, C.close
SIDE_KEYS = ("lam", "slacks", "lam_lo", "slacks_lo")


def perturbed(label, sides, delta=DELTA):
    Q, p, G, h, A, b, lower = R.range_problem(label, sides)
    r = np.random.RandomState(W.PERTURB_SEED)
    p2 = p + delta * r.randn(*p.shape)
    h2 = h + delta * r.rand(*h.shape)
    lower2 = lower - delta * r.rand(*lower.shape)
    return Q, p2, G, h2, A, b, lower2


def solve_doubled(arrs, warm=None, eps=1e-12, maxIter=20):
    """warm_reference.solve on the doubled QP, each QP alone (F may differ per QP), folded back onto the nineq rows.
    warm: (lam, slacks, lam_lo, slacks_lo), each (B, m); the lower side's entries of the rows in F go below the upper side's"""
    Q, p, G, h, A, b, lower = arrs
    B, m, n = G.shape
    q = A.shape[1] if np.size(A) else 0
    out = dict(zhat=np.zeros((B, n)), nu=np.zeros((B, q)), lam=np.zeros((B, m)), slacks=np.zeros((B, m)), lam_lo=np.zeros((B, m)),
               slacks_lo=np.zeros((B, m)), iters=np.zeros(B, np.int32), trace=[])
    for i in range(B):
        G2, h2, F = R.double(G[i], h[i], lower[i])
        kw = {}
        if warm is not None:
            kw = dict(lam0=np.concatenate([warm[0][i], warm[2][i][F]])[None], s0=np.concatenate([warm[1][i], warm[3][i][F]])[None])
        r = W.solve(Q[i][None], p[i][None], G2[None], h2[None], A[i][None] if q else np.zeros(0), b[i][None] if q else np.zeros(0),
                    eps=eps, maxIter=maxIter, **kw)
        out["zhat"][i], out["nu"][i], out["iters"][i] = r["zhat"][0], r["nu"][0], r["iters"][0]
        out["lam"][i], out["lam_lo"][i] = R.split(r["lam"][0], F, m, 0.0)
        out["slacks"][i], out["slacks_lo"][i] = R.split(r["slacks"][0], F, m, np.inf)
        out["trace"].append(r["trace"][0])
    return out


# the references of one (label, sides), each computed once per process and left unchanged
@functools.lru_cache(maxsize=None)
def base_solution(label, sides):
    return solve_doubled(R.range_problem(label, sides))


@functools.lru_cache(maxsize=None)
def reference_cold(label, sides, eps=1e-12):
    return solve_doubled(perturbed(label, sides), eps=eps)


@functools.lru_cache(maxsize=None)
def reference_warm(label, sides, eps=EPS_COUNT):
    sb = base_solution(label, sides)
    return solve_doubled(perturbed(label, sides), warm=[sb[k] for k in SIDE_KEYS], eps=eps)


def as_np(res):
    out = {k: host(getattr(res, k)).copy() for k in ("zhat", "nu", "iters", "best_resid", "warm_used") + SIDE_KEYS}
    out["trace"] = host(res.trace).copy() if res.trace is not None else None
    return out


def close_to(res, sol, q):
    """zhat, nu, the multipliers and the slacks against `sol`, per-QP relative L2 error.  The multipliers and the slacks are those
    of the doubled QP, (lam, lam_lo) and (slacks, slacks_lo on the two-sided rows) as ONE vector each: a side on which no row
    is active (t1a has such QPs) is zero at the solution, what a run leaves there is round-off of ITS path (1e-14 here, warm
    and cold differ in it), and an error relative to that is no figure.  Each side alone is held to the same 1e-6 by the
    project's gate on slacks and gradients, max |a - ref| <= 1e-6 max(1, max |ref|).  The one-sided rows must be 0 / +inf."""
    fin = np.isfinite(sol["slacks_lo"])
    assert np.array_equal(np.isfinite(res["slacks_lo"]), fin)
    assert np.all(res["lam_lo"][~fin] == 0.0)
    s_lo, ref_s_lo = np.where(fin, res["slacks_lo"], 0.0), np.where(fin, sol["slacks_lo"], 0.0)
    worst = {k: rel_err(res[k], sol[k]).max() for k in ("zhat",) + (("nu",) if q else ())}
    worst["lam'"] = rel_err(np.concatenate([res["lam"], res["lam_lo"]], axis=1), np.concatenate([sol["lam"], sol["lam_lo"]], axis=1)).max()
    worst["slacks'"] = rel_err(np.concatenate([res["slacks"], s_lo], axis=1), np.concatenate([sol["slacks"], ref_s_lo], axis=1)).max()
    for k in ("lam", "lam_lo", "slacks"):
        worst[k] = close(res[k], sol[k])
    worst["slacks_lo"] = close(s_lo, ref_s_lo)
    assert max(worst.values()) <= TOL, worst
    return max(worst.values())


# ---------------------------------------------------------------- 1. the reference alone (no library call)
def check_reference_alone():
    """pins the inputs: from the base solution at delta = 1e-3 the dense float64 loop on the doubled QP needs at most cold - 1
    passes per QP at eps = 1e-9 and at most 0.7 of the cold passes in all (measured: cold - 2 at most, 178 against 360)"""
    cold_sum = warm_sum = 0
    for label in R.SHAPES:
        for sides in R.SIDES:
            cold, warm = reference_cold(label, sides, EPS_COUNT), reference_warm(label, sides)
            print(label, sides, "cold", cold["iters"], "warm", warm["iters"])
            assert (warm["iters"] <= cold["iters"] - 1).all(), (label, sides, warm["iters"], cold["iters"])
            cold_sum += int(cold["iters"].sum())
            warm_sum += int(warm["iters"].sum())
    print("sum: cold %d warm %d ratio %.3f" % (cold_sum, warm_sum, warm_sum / cold_sum))
    assert warm_sum <= 0.7 * cold_sum


# ---------------------------------------------------------------- 2. every form of the range role
def run_form(env, label, sides, variant, eps, warm=None, **kw):
    """cold and warm run on the perturbed problem, same factors, the reference's stall counter"""
    from qpth_amd.kkt import KKTFactors
    tq = on(perturbed(label, sides), env.dev)
    if warm is None:
        sb = base_solution(label, sides)
        warm = [sb[k] for k in SIDE_KEYS]
    wt = [torch.tensor(x, dtype=torch.float64, device=env.dev) for x in warm]
    with env.run(variant):
        fac = KKTFactors.build(tq[0], tq[2], tq[4], R.SHAPES[label][0])
        cold = as_np(fac.ipm_range(tq[1], tq[3], tq[6], tq[5], eps=eps, stall_policy=1, **kw))
        hot = as_np(fac.ipm_range(tq[1], tq[3], tq[6], tq[5], eps=eps, stall_policy=1, warm=wt, **kw))
    return cold, hot


def library_doubled_warm(env, label, sides, eps):
    """the library's own ipm(warm=...) on the doubled QP, each QP alone, under the default dispatch: its iteration counts"""
    from qpth_amd.kkt import KKTFactors
    Q, p, G, h, A, b, lower = perturbed(label, sides)
    B, n, m, q = R.SHAPES[label]
    sb = base_solution(label, sides)
    iters = np.zeros(B, np.int32)
    for i in range(B):
        G2, h2, F = R.double(G[i], h[i], lower[i])
        t = on((Q[i][None], p[i][None], G2[None], h2[None], A[i][None] if q else np.zeros(0), b[i][None] if q else np.zeros(0),
                np.concatenate([sb["lam"][i], sb["lam_lo"][i][F]])[None], np.concatenate([sb["slacks"][i], sb["slacks_lo"][i][F]])[None]),
               env.dev)
        with env.run():
            fac = KKTFactors.build(t[0], t[2], t[4], 1)
            res = fac.ipm(t[1], t[3], t[5], eps=eps, stall_policy=1, warm=(t[6], t[7]))
        assert host(res.warm_used)[0] == 1
        iters[i] = host(res.iters)[0]
    return iters


def check_every_form(env, label, sides, variant=0):
    q = R.SHAPES[label][3]
    sol = reference_cold(label, sides)
    cold, hot = run_form(env, label, sides, variant, 1e-12)
    print("iters at eps = 1e-12: cold", cold["iters"], "warm", hot["iters"])
    C.note("warm/%s%s/%s" % (label, "-1w" if variant else "", sides), close_to(hot, sol, q))
    assert (hot["warm_used"] == 1).all() and (cold["warm_used"] == 0).all()
    ref = reference_warm(label, sides)
    cold9, hot9 = run_form(env, label, sides, variant, EPS_COUNT)
    print("iters at eps = 1e-9: cold", cold9["iters"], "warm", hot9["iters"], "reference", ref["iters"])
    # (the solution is gated at the default eps above: a run that stops at a residual of 1e-9 owes nobody six digits)
    assert (hot9["warm_used"] == 1).all() and (cold9["warm_used"] == 0).all()
    assert (np.abs(hot9["iters"] - ref["iters"]) <= 1).all(), (hot9["iters"], ref["iters"])
    assert (hot9["iters"] < cold9["iters"]).all(), (hot9["iters"], cold9["iters"])
    if label in R.COUNTED:
        mine = library_doubled_warm(env, label, sides, EPS_COUNT)
        print("ipm(warm=) on the doubled QP", mine)
        assert np.array_equal(hot9["iters"], mine), (hot9["iters"], mine)


# ---------------------------------------------------------------- 3. lower = -inf everywhere: ipm(warm=(lam0, s0))
def check_one_sided_equivalence(env, label, variant=0):
    """the warm start is the library's own cold solution of the base problem without lower bounds; the lower side's arrays
    carry what a range solve wrote on one-sided rows (0, +inf) and are never read"""
    from qpth_amd.kkt import KKTFactors
    B, n, m, q = R.SHAPES[label]
    tb = on(R.range_problem(label, "all"), env.dev)
    tq = on(perturbed(label, "all"), env.dev)
    none = torch.full_like(tq[6], -float("inf"))
    with env.run(variant):
        fac = KKTFactors.build(tb[0], tb[2], tb[4], B)
        first = fac.ipm(tb[1], tb[3], tb[5], stall_policy=1)
        warm = (first.lam, first.slacks, torch.zeros_like(first.lam), torch.full_like(first.lam, float("inf")))
        one = fac.ipm(tq[1], tq[3], tq[5], stall_policy=1, warm=warm[:2])
        two = fac.ipm_range(tq[1], tq[3], none, tq[5], stall_policy=1, warm=warm)
    assert (host(one.warm_used) == 1).all() and (host(two.warm_used) == 1).all()
    assert np.all(host(two.lam_lo) == 0.0) and np.all(np.isposinf(host(two.slacks_lo)))
    print("iters ipm", host(one.iters), "ipm_range", host(two.iters))
    assert np.array_equal(host(one.iters), host(two.iters))
    worst = max(close(host(getattr(two, k)), host(getattr(one, k))) for k in ("zhat", "lam", "slacks") + (("nu",) if q else ()))
    C.note("warm_one_sided/" + label + ("-1w" if variant else ""), worst)
    assert worst <= 1e-12


# ---------------------------------------------------------------- 4. the entry state
def check_entry_state(env, label, sides, variant=0):
    """entries below the floor and negative ones on both sides are floored; pass 0 sees mu and the primal residual of the
    reference's entry point on the doubled QP, and a dual residual of exactly zero (x = x0 - M^T (zu - zl) is dual-feasible)"""
    B, n, m, q = R.SHAPES[label]
    sb = base_solution(label, sides)
    warm = [sb[k].copy() for k in SIDE_KEYS]
    two = np.flatnonzero(np.isfinite(sb["slacks_lo"][0]))                  # (the same rows in every QP of these problems)
    assert len(two) >= 4
    warm[0][:, 0], warm[0][:, 1], warm[1][:, 2], warm[1][:, 3] = -0.5, 1e-5, -2.0, 3e-3
    warm[2][:, two[0]], warm[2][:, two[1]], warm[3][:, two[2]], warm[3][:, two[3]] = -0.25, 2e-5, -1.0, 5e-3
    for x in warm:
        assert (x < W.FLOOR).any()
    ref = solve_doubled(perturbed(label, sides), warm=warm)
    _, hot = run_form(env, label, sides, variant, 1e-12, warm=warm, want_trace=True)
    assert (hot["warm_used"] == 1).all()
    for i in range(B):
        pri, dual, mu = hot["trace"][0, i]
        rpri, _, rmu = ref["trace"][i][0]
        print("QP %d: pri %.12e (ref %.12e) mu %.12e (ref %.12e) dual %g" % (i, pri, rpri, mu, rmu, dual))
        assert abs(mu - rmu) <= 1e-9 * rmu and abs(pri - rpri) <= 1e-9 * rpri
        assert dual == 0.0


# ---------------------------------------------------------------- 5. per-QP fallback in one batch
def check_per_qp_fallback(env, label, variant=0):
    """four QPs (the two of the `half` problem, twice) in one launch, the rule of the finiteness check row by row:
    QP 0: a NaN in lam0_lo on a two-sided row                      -> cold, outputs bit-equal to the cold call's
    QP 1: (0, +inf) lower entries on rows one-sided in this call   -> warm (every QP of `half` has them)
    QP 2: the same (0, +inf) on a row two-sided in this call       -> cold
    QP 3: a NaN in lam0_lo and an Inf in s0_lo on ONE-SIDED rows   -> warm: those entries are never read"""
    from qpth_amd.kkt import KKTFactors
    B, n, m, q = R.SHAPES[label]
    arrs = perturbed(label, "half")
    sb = base_solution(label, "half")
    four = [np.concatenate([x, x]) if np.size(x) else x for x in arrs]
    warm = [np.concatenate([sb[k], sb[k]]) for k in SIDE_KEYS]
    fin = np.isfinite(four[6])
    two, one = np.flatnonzero(fin[0]), np.flatnonzero(~fin[0])
    assert np.all(warm[2][~fin] == 0.0) and np.all(np.isposinf(warm[3][~fin]))          # what the previous solve wrote
    warm[2][0, two[1]] = np.nan
    warm[2][2, two[0]], warm[3][2, two[0]] = 0.0, np.inf
    warm[2][3, one[0]], warm[3][3, one[-1]] = np.nan, -np.inf
    tq = on(four, env.dev)
    wt = [torch.tensor(x, dtype=torch.float64, device=env.dev) for x in warm]
    with env.run(variant):
        fac = KKTFactors.build(tq[0], tq[2], tq[4], 4)
        cold = as_np(fac.ipm_range(tq[1], tq[3], tq[6], tq[5], stall_policy=1))
        hot = as_np(fac.ipm_range(tq[1], tq[3], tq[6], tq[5], stall_policy=1, warm=wt))
    assert hot["warm_used"].tolist() == [0, 1, 0, 1], hot["warm_used"]
    assert cold["warm_used"].tolist() == [0, 0, 0, 0]
    for k in ("zhat", "nu", "iters", "best_resid") + SIDE_KEYS:
        assert np.array_equal(hot[k][[0, 2]], cold[k][[0, 2]]), k
    sol = reference_cold(label, "half")
    close_to({k: hot[k][[1, 3]] for k in hot if k != "trace"}, {k: sol[k][[1, 1]] for k in ("zhat", "nu") + SIDE_KEYS}, q)
    assert (hot["iters"][[1, 3]] <= cold["iters"][[1, 3]]).all()


# ---------------------------------------------------------------- 6. the C ABI
def raw_range(dll, fac, tq, warm, floor, used, name="qpx_ipm_range_warm", dtype=None):
    """qpx_ipm_range_warm (or qpx_ipm_range) called directly; warm: four tensors or None each; returns (code, outputs)"""
    from qpth_amd import _lib
    B, n, m, q = fac.B, fac.n, fac.m, fac.q
    dev = tq[1].device
    new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)      # noqa: E731
    out = dict(zhat=new(B, n), nu=new(B, q), lam=new(B, m), slacks=new(B, m), lam_lo=new(B, m), slacks_lo=new(B, m),
               iters=torch.empty(B, dtype=torch.int32, device=dev), best_resid=new(B), status=fac.status.clone())
    gt1 = fac.gt1_of(tq[6], tq[3])
    ptr = _lib._ptr
    args = [_lib.QPX_F64 if dtype is None else dtype, B, n, m, q, ptr(tq[1]), n, ptr(tq[3]), m, ptr(tq[5]) if q else None, q,
            ptr(fac.blob), int(fac.sfac), 1e-12, 20, 3, 1, ptr(out["zhat"]), ptr(out["nu"]) if q else None, ptr(out["lam"]),
            ptr(out["slacks"]), ptr(out["iters"]), ptr(out["status"]), ptr(out["best_resid"]), None, ptr(tq[6]), m,
            ptr(gt1), ptr(out["lam_lo"]), ptr(out["slacks_lo"])]
    if name == "qpx_ipm_range_warm":
        args += [ptr(w) for w in warm] + [ctypes.c_double(floor), ptr(used)]
    code = getattr(dll, name)(*args, _lib._stream(tq[1]))
    return code, out


def check_abi(env, label="t1b", sides="half"):
    from qpth_amd import _lib
    from qpth_amd.kkt import KKTFactors
    B, n, m, q = R.SHAPES[label]
    tq = on(perturbed(label, sides), env.dev)
    sb = base_solution(label, sides)
    w = [torch.tensor(sb[k], dtype=torch.float64, device=env.dev) for k in SIDE_KEYS]
    none = [None] * 4
    with env.run():
        dll = _lib.backend_for(tq[0]).dll
        # qpx_range_warm_supported beside qpx_range_supported: served sizes, unserved ones, the dtypes, a bad dtype
        sizes = [R.SHAPES[k][1:] for k in R.SHAPES] + [(100, 100, 10), (100, 200, 0), (0, 4, 0)]
        for (n_, m_, q_) in sizes:
            for dt in (_lib.QPX_F64, _lib.QPX_F32, _lib.QPX_F32_WIDE, 7):
                assert dll.qpx_range_warm_supported(dt, n_, m_, q_) == dll.qpx_range_supported(dt, n_, m_, q_)
        assert dll.qpx_range_warm_supported(_lib.QPX_F64, n, m, q) == 1
        assert dll.qpx_range_warm_supported(_lib.QPX_F64, 100, 100, 10) == 0
        assert dll.qpx_range_warm_supported(7, n, m, q) == 0
        fac = KKTFactors.build(tq[0], tq[2], tq[4], B)
        # NULL arrays: qpx_ipm_range, bit for bit (warm_used is not written then)
        used = torch.full((B,), 7, dtype=torch.int32, device=env.dev)
        code0, old = raw_range(dll, fac, tq, None, 0, None, name="qpx_ipm_range")
        code1, new = raw_range(dll, fac, tq, none, 1e-2, used)
        assert code0 == 0 and code1 == 0
        for k in old:
            assert np.array_equal(host(old[k]), host(new[k])), k
        assert host(used).tolist() == [7] * B
        # all four given
        code, hot = raw_range(dll, fac, tq, w, 1e-2, used)
        assert code == 0 and host(used).tolist() == [1] * B
        assert rel_err(host(hot["zhat"]), host(old["zhat"])).max() <= TOL
        code, _ = raw_range(dll, fac, tq, w, 1e-2, None)                       # warm_used may be NULL
        assert code == 0
        # some but not all of the four
        for k in range(4):
            assert raw_range(dll, fac, tq, [x if j != k else None for j, x in enumerate(w)], 1e-2, None)[0] == QPX_ERR_ARG, k
            assert raw_range(dll, fac, tq, [x if j == k else None for j, x in enumerate(w)], 1e-2, None)[0] == QPX_ERR_ARG, k
        for bad in (0.0, -1e-2, float("nan"), float("inf")):
            assert raw_range(dll, fac, tq, w, bad, None)[0] == QPX_ERR_ARG, bad
        # dtype, size and form
        assert raw_range(dll, fac, tq, w, 1e-2, None, dtype=_lib.QPX_F32)[0] == QPX_ERR_UNSUPPORTED
        assert raw_range(dll, fac, tq, w, 1e-2, None, dtype=_lib.QPX_F32_WIDE)[0] == QPX_ERR_UNSUPPORTED
        assert raw_range(dll, fac, tq, w, 1e-2, None, dtype=7)[0] == QPX_ERR_ARG
        P = ctypes.c_void_p(tq[0].data_ptr())
        i32 = ctypes.c_void_p(used.data_ptr())
        assert dll.qpx_ipm_range_warm(_lib.QPX_F64, 1, 100, 100, 10, P, 0, P, 0, P, 0, P, 0, 1e-8, 20, 3, 1, P, P, P, P, i32, i32, P,
                                      None, P, 0, None, P, P, P, P, P, P, 1e-2, None, None) == QPX_ERR_UNSUPPORTED
        old_knob = dll.qpx_set_ipm_variant(256)                                # the 16x16 thread grid at every size: no range role
        try:
            assert dll.qpx_range_warm_supported(_lib.QPX_F64, n, m, q) == 0
            assert raw_range(dll, fac, tq, w, 1e-2, None)[0] == QPX_ERR_UNSUPPORTED
        finally:
            dll.qpx_set_ipm_variant(old_knob)
        # the host entry
        import pytest
        with pytest.raises(ValueError, match="warm_floor"):
            fac.ipm_range(tq[1], tq[3], tq[6], tq[5], warm=w, warm_floor=0.0)
        with pytest.raises(ValueError, match="lam0, s0, lam0_lo, s0_lo"):
            fac.ipm_range(tq[1], tq[3], tq[6], tq[5], warm=w[:2])
        with pytest.raises(RuntimeError, match="lam0_lo"):
            fac.ipm_range(tq[1], tq[3], tq[6], tq[5], warm=(w[0], w[1], w[2][:, :5], w[3]))


# ---------------------------------------------------------------- 7. QPFunction(warm_start=RangeWarmStart())
def check_qpfunction_loop(env, label="c4", sides="half"):
    """three steps with ONE holder, p moving by delta per step: step 1 cold, steps 2 and 3 warm with fewer passes than the
    cold call of the same step (eps = 1e-9, see the top of tests/test_emu_warm.py); the gradients of step 3 are the cold call's"""
    from qpth_amd import RangeWarmStart
    from qpth_amd.kkt import KKTFactors
    from qpth_amd.qp import QPFunction
    B, n, m, q = R.SHAPES[label]
    arrs = R.range_problem(label, sides)
    r = np.random.RandomState(W.PERTURB_SEED)
    steps = [arrs[1] + k * DELTA * r.randn(B, n) for k in range(3)]
    c = torch.tensor(R.loss_vector(label), device=env.dev)
    seen = []
    plain = KKTFactors.ipm_range

    def recording(self, *a, **kw):
        res = plain(self, *a, **kw)
        seen.append(host(res.iters).copy())
        return res

    def leaves(p):
        tq = on(arrs[:1] + (p,) + arrs[2:], env.dev)
        for t in tq:
            if t.nelement():
                t.requires_grad_(True)
        return tq

    ws = RangeWarmStart()
    assert ws.lam is None and ws.lam_lo is None and ws.used is None
    KKTFactors.ipm_range = recording
    try:
        with env.run():
            used, grads = [], []
            for p in steps:
                for holder in (ws, None):
                    tq = leaves(p)
                    z = QPFunction(verbose=-1, eps=EPS_COUNT, warm_start=holder)(*tq[:6], lower=tq[6])
                    (z * c).sum().backward()
                    grads.append([host(z)] + [host(t.grad) for t in tq if t.nelement()])
                used.append(host(ws.used).copy())
                assert ws.lam.shape == (B, m) and ws.lam_lo.shape == (B, m) and not ws.lam.requires_grad
    finally:
        KKTFactors.ipm_range = plain
    warm_it, cold_it = seen[0::2], seen[1::2]
    print("used", used, "iters warm", warm_it, "cold", cold_it)
    assert (used[0] == 0).all() and (used[1] == 1).all() and (used[2] == 1).all()
    assert np.array_equal(warm_it[0], cold_it[0])
    assert (warm_it[1] < cold_it[1]).all() and (warm_it[2] < cold_it[2]).all()
    worst = max(close(a, ref) for a, ref in zip(grads[4], grads[5]))
    C.note("qpfunction_loop/grads", worst)
    assert worst <= TOL
    ws.clear()
    assert ws.lam is None and ws.slacks is None and ws.lam_lo is None and ws.slacks_lo is None and ws.used is None


def check_holder_of_another_batch(env):
    """a holder of another (B, nineq) is ignored -- that call is cold -- and overwritten"""
    from qpth_amd import RangeWarmStart
    from qpth_amd.qp import QPFunction
    a, b = on(R.range_problem("t1a", "half"), env.dev), on(R.range_problem("t1b", "half"), env.dev)
    ws = RangeWarmStart()
    with env.run():
        QPFunction(verbose=-1, warm_start=ws)(*a[:6], lower=a[6])
        assert ws.lam.shape == (2, 4)
        cold = QPFunction(verbose=-1)(*b[:6], lower=b[6])
        z = QPFunction(verbose=-1, warm_start=ws)(*b[:6], lower=b[6])
        assert ws.lam.shape == (2, 9) and (host(ws.used) == 0).all()
        assert torch.equal(z, cold)
        z = QPFunction(verbose=-1, warm_start=ws)(*b[:6], lower=b[6])
        assert (host(ws.used) == 1).all() and rel_err(host(z), host(cold)).max() <= TOL


def check_refusals(env, pytest):
    from qpth_amd import RangeWarmStart, SoftRange, WarmStart, sensitivity
    from qpth_amd.qp import QPFunction
    tq = on(R.range_problem("t1b", "half"), env.dev)
    six, lower = tq[:6], tq[6]
    with env.run():
        f = QPFunction(verbose=-1, warm_start=RangeWarmStart())
        with pytest.raises(ValueError, match="without lower"):
            f(*six)
        with pytest.raises(ValueError, match="with rho"):
            f(*six, 2.5, lower=lower)
        with pytest.raises(ValueError, match="with rho"):
            f(*six, 2.5)
        with pytest.raises(ValueError, match="with kappa"):
            f(*six, kappa=1e-3, lower=lower)
        with pytest.raises(ValueError, match="l1"):
            f(*six, 2.5, l1=1.0)
        with pytest.raises(ValueError, match="soft_range"):
            f(*six, soft_range=SoftRange(lower, 1.0, 1.0))
        with pytest.raises(ValueError, match="RangeWarmStart"):            # (the refusal as before, with the pointer)
            QPFunction(verbose=-1, warm_start=WarmStart())(*six, lower=lower)
        with pytest.raises(ValueError, match="floor"):
            RangeWarmStart(floor=0.0)
        # sensitivity.solve
        with pytest.raises(ValueError, match="RangeWarmStart"):
            sensitivity.solve(*six, lower=lower, warm_start=WarmStart())
        with pytest.raises(ValueError, match="lower"):
            sensitivity.solve(*six, warm_start=RangeWarmStart())
        with pytest.raises(ValueError, match="rho"):
            sensitivity.solve(*six, lower=lower, rho=2.5)
        with pytest.raises(ValueError, match="kappa"):
            sensitivity.solve(*six, lower=lower, kappa=1e-3)
        with pytest.raises(ValueError, match=r"\[G; -G\] z <= \[h; -lower\]"):
            sensitivity.solve(*[t.float() for t in six], lower=lower.float())
        big = on(R.range_problem("box", "all"), env.dev)
        A = torch.zeros(2, 10, 100, dtype=torch.float64, device=env.dev)
        with pytest.raises(ValueError, match=r"\[G; -G\] z <= \[h; -lower\]"):      # nz + neq + nineq = 210
            sensitivity.solve(big[0], big[1], big[2], big[3], A, A[:, :, 0], lower=big[6])
        sol = sensitivity.solve(*six)
        with pytest.raises(ValueError, match="lower"):
            sol.vjp_many(dl_dz=torch.ones(2, 1, 12, dtype=torch.float64, device=env.dev), want=("lower",))
        with pytest.raises(ValueError, match="dl_dlam_lo"):
            sol.vjp_many(dl_dlam_lo=torch.ones(2, 1, 9, dtype=torch.float64, device=env.dev))
        with pytest.raises(ValueError, match="lam_lo"):
            sol.jacobian(of=("lam_lo",))


# ---------------------------------------------------------------- 8. sensitivity.solve(..., lower=): the K-right-hand-side solve
def check_sensitivity(env, label, sides):
    """vjp_many with random cotangents on zhat, lam, lam_lo, nu and the Jacobians of all four outputs with respect to p, h,
    lower, b against sensitivity.solve on the DOUBLED QP, each QP alone, folded back (range_reference.split / fold)"""
    from qpth_amd import RangeWarmStart, sensitivity
    B, n, m, q = R.SHAPES[label]
    arrs = R.range_problem(label, sides)
    tq = on(arrs, env.dev)
    K = 3
    r = np.random.RandomState(17)
    cz, cl, cll, cn = r.randn(B, K, n), r.randn(B, K, m), r.randn(B, K, m), r.randn(B, K, q)
    t = lambda x: torch.tensor(x, dtype=torch.float64, device=env.dev)      # noqa: E731
    wrt, of = ("p", "h", "lower", "b") if q else ("p", "h", "lower"), ("z", "lam", "lam_lo", "nu") if q else ("z", "lam", "lam_lo")
    ws = RangeWarmStart()
    with env.run():
        sol = sensitivity.solve(*tq[:6], lower=tq[6], warm_start=ws)
        assert (host(ws.used) == 0).all()
        again = sensitivity.solve(*tq[:6], lower=tq[6], warm_start=ws)
        assert (host(ws.used) == 1).all() and rel_err(host(again.zhat), host(sol.zhat)).max() <= TOL
        assert sol.lam_lo.shape == (B, m) and sol.slacks_lo.shape == (B, m) and sol.lower.shape == (B, m)
        g = sol.vjp_many(t(cz), t(cl), t(cn) if q else None, want=wrt + ("G",), dl_dlam_lo=t(cll))
        J = sol.jacobian(of=of, wrt=wrt)
    fin = np.isfinite(arrs[6])
    worst = 0.0
    for i in range(B):
        G2, h2, F = R.double(arrs[2][i], arrs[3][i], arrs[6][i])
        t2 = on((arrs[0][i][None], arrs[1][i][None], G2[None], h2[None], arrs[4][i][None] if q else np.zeros(0),
                 arrs[5][i][None] if q else np.zeros(0)), env.dev)
        with env.run():
            sol2 = sensitivity.solve(*t2)
            g2 = sol2.vjp_many(t(cz[i:i + 1]), t(np.concatenate([cl[i], cll[i][:, F]], axis=1)[None]), t(cn[i:i + 1]) if q else None,
                               want=("p", "h", "b", "G") if q else ("p", "h", "G"))
            J2 = sol2.jacobian(of=("z", "lam", "nu") if q else ("z", "lam"), wrt=("p", "h", "b") if q else ("p", "h"))
        # the K gradients
        for k in range(K):
            dG, dh, dlo = R.fold(host(g2["G"])[0, k], host(g2["h"])[0, k], F, m)
            fig = [close(host(g["p"])[i, k], host(g2["p"])[0, k]), close(host(g["h"])[i, k], dh), close(host(g["lower"])[i, k], dlo),
                   close(host(g["G"])[i, k], dG)]
            if q:
                fig.append(close(host(g["b"])[i, k], host(g2["b"])[0, k]))
            worst = max([worst] + fig)
        # the Jacobians: rows of lam' -> (lam, lam_lo), columns of h' -> (h, -lower)
        for o in of:
            for w in wrt:
                mine = host(J[o, w])[i]
                o2, w2 = ("lam" if o == "lam_lo" else o), ("h" if w == "lower" else w)
                ref = host(J2[o2, w2])[0]
                if o == "lam":
                    ref = ref[:m]
                elif o == "lam_lo":
                    full = np.zeros((m,) + ref.shape[1:])
                    full[F] = ref[m:]
                    ref = full
                if w == "h":
                    ref = ref[:, :m]
                elif w == "lower":
                    full = np.zeros(ref.shape[:1] + (m,))
                    full[:, F] = -ref[:, m:]
                    ref = full
                worst = max(worst, close(mine, ref))
    C.note("sensitivity/%s/%s" % (label, sides), worst)
    assert worst <= TOL, worst
    # the lower columns of one-sided rows, and the lam_lo rows of one-sided rows: exactly 0
    for o in of:
        Jl = host(J[o, "lower"])
        assert np.all(np.swapaxes(Jl, 1, 2)[~fin] == 0.0), o
    assert np.all(host(g["lower"]).transpose(0, 2, 1)[~fin] == 0.0)
    for w in wrt:
        assert np.all(host(J["lam_lo", w])[~fin] == 0.0), w


def check_jacobian_against_backward_calls(env, label="t1b", sides="half"):
    """J["z", "lower"] row by row from backward calls of QPFunction(lower=): one per component of zhat"""
    from qpth_amd import sensitivity
    from qpth_amd.qp import QPFunction
    B, n, m, q = R.SHAPES[label]
    tq = on(R.range_problem(label, sides), env.dev)
    with env.run():
        J = host(sensitivity.solve(*tq[:6], lower=tq[6]).jacobian(of=("z",), wrt=("lower", "h"))["z", "lower"])
        lo = tq[6].clone().requires_grad_(True)
        z = QPFunction(verbose=-1)(*tq[:6], lower=lo)
        rows = []
        for i in range(n):
            e = torch.zeros(B, n, dtype=torch.float64, device=env.dev)
            e[:, i] = 1.0
            (gl,) = torch.autograd.grad(z, lo, e, retain_graph=True)
            rows.append(host(gl))
    ref = np.stack(rows, axis=1)
    assert J.shape == (B, n, m) and np.abs(ref).max() > 1e-3
    worst = close(J, ref)
    C.note("jacobian_z_lower/" + label, worst)
    assert worst <= TOL
    assert np.all(np.swapaxes(J, 1, 2)[~np.isfinite(host(tq[6]))] == 0.0)
