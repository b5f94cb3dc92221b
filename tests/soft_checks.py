"""Soft inequality rows (QPFunction(...)(Q, p, G, h, A, b, rho), qpx_pre_factor_soft): the checks that
tests/test_emu_soft.py runs on the host-thread emulator and tests/test_gpu_soft.py on a real MI355X.  Every check takes an
`env`: env.dev (the torch device) and env.run(variant=0), a context manager around the library calls.

Problems: tests/soft_reference.py (random_dense_qp, seed 41, every fourth row hard, rho in [0.5, 5.5] on the others, the soft
rows' h lowered so that some are violated).  References: the unmodified reference on the augmented dense QP
(tests/golden/soft_*.npz, made by tests/golden/make_golden_soft.py) and, where no reference is needed, the library's own
hard path -- on the augmented problem, or with d / (1 + w d) in place of d.

Gates: against the reference 1e-6 (float64; the project's gate, README) and 1e-5 (float32 tensors in float64 arithmetic);
the KKT solves 1e-8 (float64, as test_kkt_solver_entry_points against its golden) and 1e-5 (float32 tensors in float64
arithmetic: both sides round their outputs, and one of them d / (1 + w d), to float32, 6e-8 each, times the condition of
T = R + diag(1/d + w), <= 1e2 here).  The float32 kernels (c1, c2) have no KKT-solve gate in the existing tests; theirs is
worked out: the two sides differ in where 1/d + w is rounded (R_ii + w in the blob, then + 1/d, against 1/d' formed on the
host), a relative perturbation of <= 2 x 6e-8 of the diagonal of T, and both factor T in float32, 6e-8 per operation over
m <= 120 pivots; the solution answers with the condition of T, d in [1e-2, 1e2] against ||R|| ~ 1e1: <= 1e3.  2 x 6e-8 x 1e3
+ slack for the factorisations = 2e-4.
"""

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

import soft_reference as S
from conftest import load_golden, rel_err

TOL_REF, TOL_WIDE = 1e-6, 1e-5
NAMES = ("dQ", "dp", "dG", "dh", "dA", "db")
# label -> (problem, dtype, QPFunction's refine): (a)-(e) of the issue
CASES = {
    "a": ("a", torch.float64, None), "b0": ("b0", torch.float64, None), "b1": ("b1", torch.float64, None),
    "c1": ("a", torch.float32, 0), "c2": ("c2", torch.float32, 0), "d": ("d", torch.float64, None),
    "e": ("a", torch.float32, None),
}
measured = {}        # check name -> worst figure seen (scripts/bench_soft.py writes them to profiles/soft.json)


def note(key, value):
    measured[key] = max(float(value), measured.get(key, 0.0))
    print("%-40s %.3e" % (key, value))


def fixture_name(label):
    return "soft_%s_b%d_n%d_m%d_q%d" % ((label,) + S.SHAPES[label])


def on(arrs, dev, dtype):
    return [torch.tensor(np.asarray(x), dtype=dtype, device=dev) if np.asarray(x).size else torch.empty(0, dtype=dtype, device=dev)
            for x in arrs]


def host(t):
    return t.detach().cpu().numpy()


def close(a, ref, tol):
    """the project's gate on gradients: max |a - ref| <= tol max(1, max |ref|); returns the figure that must be <= tol"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(1.0, np.abs(ref).max()) if ref.size else 0.0


def factors(env, label, soft, zero_w=False, shared_w=False):
    """(KKTFactors, the problem's tensors, w) of a case: the hard factors, or the soft ones"""
    from qpth_amd.kkt import KKTFactors
    prob, dtype, refine = CASES[label]
    arrs = S.soft_problem(prob, np.float32 if dtype == torch.float32 else np.float64)
    Q, p, G, h, A, b, rho = on(arrs, env.dev, dtype)
    w = rho.reciprocal()
    if zero_w:
        w = torch.zeros_like(w)
    if shared_w:
        w = w[0].clone()
    wide = dtype == torch.float32 and refine is None
    fac = KKTFactors.build(Q, G, A, S.SHAPES[prob][0], wide=wide, w=w if soft else None)
    return fac, (Q, p, G, h, A, b, rho), w


def bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ---------------------------------------------------------------- 1. the blob contract
def check_zero_w_blob(env, label):
    """an all-zero w -- per QP and shared -- leaves the blob of qpx_pre_factor, bit for bit"""
    with env.run():
        hard, _, _ = factors(env, label, False)
        soft, _, _ = factors(env, label, True, zero_w=True)
        assert soft.soft and not soft.refine_ok and not soft.polish_ok
        assert hard.blob.shape == soft.blob.shape
        assert torch.equal(bits(hard.blob), bits(soft.blob))
        assert torch.equal(hard.status, soft.status)
        sh, _, _ = factors(env, label, True, zero_w=True, shared_w=True)
        assert torch.equal(bits(hard.blob), bits(sh.blob))


def check_rho_none_is_the_six_input_call(env):
    from qpth_amd.qp import QPFunction
    arrs = S.soft_problem("a")[:6]
    outs = []
    for extra in ((), (None,)):
        tq = on(arrs, env.dev, torch.float64)
        for t in tq:
            t.requires_grad_(True)
        with env.run():
            z = QPFunction(verbose=-1)(*tq, *extra)
            z.backward(torch.ones_like(z))
        outs.append([host(z)] + [host(t.grad) for t in tq])
    for a, c in zip(*outs):
        assert np.array_equal(a, c)


def check_per_qp_w_on_shared_matrices(env):
    """Q, G, A shared by the batch: a shared w keeps the one blob, a w per QP means one blob per QP, each the blob the
    batched call writes for that QP"""
    from qpth_amd.kkt import KKTFactors
    Q, p, G, h, A, b, rho = on(S.soft_problem("a"), env.dev, torch.float64)
    B, m = rho.shape
    w = rho.reciprocal()
    with env.run():
        one = KKTFactors.build(Q[0], G[0], A[0], B, w=w[0])
        many = KKTFactors.build(Q[0], G[0], A[0], B, w=w)
        ref = KKTFactors.build(Q[:1].expand(B, -1, -1).contiguous(), G[:1].expand(B, -1, -1).contiguous(),
                               A[:1].expand(B, -1, -1).contiguous(), B, w=w)
    assert one.shared and one.blob.numel() == one.elems and one.sfac == 0
    assert not many.shared and many.blob.numel() == B * many.elems
    assert torch.equal(bits(many.blob), bits(ref.blob))
    assert torch.equal(bits(many.blob[:one.elems]), bits(one.blob))


# ---------------------------------------------------------------- 2. KKT equivalence
def check_kkt_equivalence(env, label):
    """solve_kkt(soft factors, d) = solve_kkt(hard factors, d / (1 + w d)) for rs = 0: T = R + diag(w) + diag(1/d)"""
    prob, dtype, refine = CASES[label]
    B, n, m, q = S.SHAPES[prob]
    r = np.random.RandomState(5)
    d = 10.0 ** r.uniform(-2, 2, (B, m))
    rx, rz, ry = r.randn(B, n), r.randn(B, m), r.randn(B, q)
    d, rx, rz, ry = on((d, rx, rz, ry), env.dev, dtype)
    with env.run():
        hard, _, w = factors(env, label, False)
        soft, _, _ = factors(env, label, True)
        mine = soft.solve_kkt(d, rx, None, rz, ry if q else None)
        ref = hard.solve_kkt(d / (1 + w * d), rx, None, rz, ry if q else None)
        soft.raise_on_failure()
    tol = 1e-8 if dtype == torch.float64 else (TOL_WIDE if refine is None else 2e-4)
    worst = max(close(host(mine[i]), host(ref[i]), tol) for i in ((0, 2, 3) if q else (0, 2)))
    note("kkt_equivalence/" + label, worst)
    assert worst <= tol


# ---------------------------------------------------------------- 3. parity with the reference on the augmented QP
def solve_with_grads(env, label, **kw):
    from qpth_amd.qp import QPFunction
    prob, dtype, refine = CASES[label]
    g = load_golden(fixture_name(prob))
    arrs = S.soft_problem(prob, np.float32 if dtype == torch.float32 else np.float64)
    assert np.array_equal(np.asarray(arrs[6], np.float64), g["rho"].astype(arrs[6].dtype).astype(np.float64))
    tq = on(arrs, env.dev, dtype)
    for t in tq:
        if t.nelement():
            t.requires_grad_(True)
    with env.run():
        z, nu, lam, sl = QPFunction(verbose=-1, duals=True, refine=refine, **kw)(*tq)
        (z * torch.tensor(g["c"], dtype=dtype, device=env.dev)).sum().backward()
    return g, tq, (z, nu, lam, sl)


def check_reference_parity(env, label):
    prob, dtype, refine = CASES[label]
    g, tq, (z, nu, lam, sl) = solve_with_grads(env, label)
    tol = TOL_REF if dtype == torch.float64 else TOL_WIDE
    q = S.SHAPES[prob][3]
    rho = g["rho"]
    fig = {"zhat": rel_err(host(z), g["zhat"]).max(), "lam": rel_err(host(lam), g["lam"]).max(),
           "slacks": close(host(sl), g["slacks"], tol), "t": close(host(lam) / rho, g["t"], tol)}
    if q:
        fig["nu"] = rel_err(host(nu), g["nu"]).max()
    for k, t in zip(NAMES, tq[:6]):
        if t.nelement():
            fig[k] = close(host(t.grad), g[k], tol)
    fig["drho"] = close(host(tq[6].grad), g["drho"], tol)
    assert np.all(host(tq[6].grad)[~np.isfinite(rho)] == 0.0)          # hard rows: exactly zero
    for k, v in fig.items():
        note("parity/%s/%s" % (label, k), v)
    assert max(fig.values()) <= tol, fig


# ---------------------------------------------------------------- 4. the stop rule: || G'^T 1 ||
def check_stop_rule(env, label):
    """iterations and the verbose=1 trace (pri_resid, dual_resid, mu per pass) equal those of the library's own run on the
    augmented dense QP, which stays in the same kernel family at these sizes"""
    from qpth_amd.kkt import KKTFactors
    prob, dtype, _ = CASES[label]
    arrs = S.soft_problem(prob)
    B, n, m, q = S.SHAPES[prob]
    aug = [S.augment(*[x[i] if np.size(x) else x for x in arrs[:6]], arrs[6][i])[0] for i in range(B)]
    aug = [np.stack([a[k] for a in aug]) if np.size(aug[0][k]) else aug[0][k] for k in range(6)]
    Q, p, G, h, A, b, rho = on(arrs, env.dev, dtype)
    Qa, pa, Ga, ha, Aa, ba = on(aug, env.dev, dtype)
    with env.run():
        soft = KKTFactors.build(Q, G, A, B, w=rho.reciprocal())
        rs = soft.ipm(p, h, b, want_trace=True)
        hard = KKTFactors.build(Qa, Ga, Aa, B)
        assert soft.lib.dll.qpx_kernel_family(1, n, m, q) == hard.lib.dll.qpx_kernel_family(1, Qa.size(-1), m, q)
        ra = hard.ipm(pa, ha, ba, want_trace=True)
    it_s, it_a = host(rs.iters), host(ra.iters)
    print("iters soft", it_s, "augmented", it_a)
    assert np.array_equal(it_s, it_a)
    ts, ta = host(rs.trace), host(ra.trace)
    worst = 0.0
    for i in range(B):
        rows_s, rows_a = ts[:it_s[i], i], ta[:it_a[i], i]
        worst = max(worst, (np.abs(rows_s - rows_a) / np.maximum(1.0, np.abs(rows_a))).max())
    note("stop_rule/" + label, worst)
    assert worst <= TOL_REF
    assert rel_err(host(rs.zhat), host(ra.zhat)[:, :n]).max() <= TOL_REF


# ---------------------------------------------------------------- 5. adjointness, gradcheck, reductions
def check_adjoint_identity(env):
    """per QP: <v, z'> + <u, lam'> + <y, nu'> = sum over the seven inputs of <grad, tangent>"""
    from qpth_amd.qp import QPFunction
    arrs = S.soft_problem("a")
    B, n, m, q = S.SHAPES["a"]
    r = np.random.RandomState(9)
    tans = [r.randn(*np.shape(x)) for x in arrs]
    tans[0] = 0.5 * (tans[0] + np.swapaxes(tans[0], -1, -2))
    tans[6] = np.where(np.isfinite(arrs[6]), tans[6], 0.0)
    cots = [r.randn(B, n), r.randn(B, q), r.randn(B, m)]                # on zhat, nu, lam
    prim, tang = on(arrs, env.dev, torch.float64), on(tans, env.dev, torch.float64)
    with env.run(), fwAD.dual_level():
        duals = [fwAD.make_dual(x, t) for x, t in zip(prim, tang)]
        outs = QPFunction(verbose=-1, duals=True)(*duals)
        jv = [host(fwAD.unpack_dual(o).tangent) for o in outs[:3]]
    tq = on(arrs, env.dev, torch.float64)
    for t in tq:
        t.requires_grad_(True)
    with env.run():
        z, nu, lam, _ = QPFunction(verbose=-1, duals=True)(*tq)
        sum((o * c).sum() for o, c in zip((z, nu, lam), on(cots, env.dev, torch.float64))).backward()
    lhs = np.stack([np.einsum("bi,bi->b", c, j) for c, j in zip(cots, jv)])
    rhs = np.stack([(np.nan_to_num(host(t.grad)) * tn).reshape(B, -1).sum(1) for t, tn in zip(tq, tans)])
    gap = np.abs(lhs.sum(0) - rhs.sum(0)) / (np.abs(lhs).sum(0) + np.abs(rhs).sum(0))
    note("adjoint_gap", gap.max())
    assert np.abs(rhs[6]).min() > 0                                     # the rho term takes part
    assert gap.max() <= 1e-9, gap


def small_problem(dev):
    B, n, m, q = 2, 6, 5, 2
    r = np.random.RandomState(3)
    L = r.randn(B, n, n) / np.sqrt(n)
    G, z0, A = r.randn(B, m, n), r.randn(B, n), r.randn(B, q, n)
    h = np.einsum("bmn,bn->bm", G, z0) + r.rand(B, m) - 0.5
    rho = 0.5 + 5.0 * r.rand(B, m)
    return on((L, r.randn(B, n), G, h, A, np.einsum("bqn,bn->bq", A, z0), rho), dev, torch.float64)


def check_gradcheck(env):
    """torch.autograd.gradcheck over all seven inputs (Q = L L' + I through L: the kernels read one triangle of Q, and the
    gradient is the symmetrised one of the reference).  eps = 1e-6; atol 1e-5 covers the central difference's noise, the
    solution's ~1e-11 over 2 eps, rtol 1e-3 its truncation error."""
    from qpth_amd.qp import QPFunction
    ins = small_problem(env.dev)
    for t in ins:
        t.requires_grad_(True)
    eye = torch.eye(6, dtype=torch.float64, device=env.dev)

    def f(L, p, G, h, A, b, rho):
        return QPFunction(verbose=-1)(L @ L.transpose(-1, -2) + eye, p, G, h, A, b, rho)

    with env.run():
        assert torch.autograd.gradcheck(f, ins, eps=1e-6, atol=1e-5, rtol=1e-3)


def check_rho_reductions(env):
    """a rho the batch shares: the `.mean(0)` of the per-QP gradient; a scalar: summed over the rows as well"""
    from qpth_amd.qp import QPFunction
    L, p, G, h, A, b, rho = small_problem(env.dev)
    Q = L @ L.transpose(-1, -2) + torch.eye(6, dtype=torch.float64, device=env.dev)
    c = torch.tensor(np.random.RandomState(4).randn(2, 6), device=env.dev)

    def grad_of(r):
        r = r.clone().requires_grad_(True) if torch.is_tensor(r) else r
        with env.run():
            z = QPFunction(verbose=-1)(Q, p, G, h, A, b, r)
            if not torch.is_tensor(r):
                return host(z), None
            (z * c).sum().backward()
        return host(z), host(r.grad)

    vec = rho[0]
    z1, g_pq = grad_of(vec.expand(2, -1).contiguous())
    z2, g_sh = grad_of(vec)
    assert np.array_equal(z1, z2) and g_sh.shape == (5,)
    assert close(g_sh, g_pq.mean(0), 1e-12) <= 1e-12
    z3, g_pq = grad_of(torch.full_like(rho, 2.5))
    z4, g_sc = grad_of(torch.tensor(2.5, dtype=torch.float64, device=env.dev))
    z5, _ = grad_of(2.5)
    assert np.array_equal(z3, z4) and np.array_equal(z3, z5) and g_sc.shape == ()
    assert close(g_sc, g_pq.mean(0).sum(), 1e-12) <= 1e-12


# ---------------------------------------------------------------- 6. the infeasible box
def check_infeasible_box(env):
    """z <= -1 and -z <= -1 with Q = I, p = 0, rho = 10: zhat = 0, lam = 10, t = 1, slacks = 0"""
    from qpth_amd.qp import QPFunction
    n = 4
    eye = np.eye(n)
    arrs = (eye, np.zeros(n), np.concatenate([eye, -eye]), -np.ones(2 * n), np.zeros(0), np.zeros(0))
    tq = on(arrs, env.dev, torch.float64)
    with env.run():
        z, nu, lam, sl = QPFunction(verbose=-1, duals=True)(*tq, 10.0)
    fig = {"zhat": np.abs(host(z)).max(), "lam": np.abs(host(lam) - 10.0).max() / 10.0, "slacks": np.abs(host(sl)).max()}
    for k, v in fig.items():
        note("box/" + k, v)
    assert max(fig.values()) <= TOL_REF, fig


# ---------------------------------------------------------------- 7. the other paths
def check_warm_start(env):
    from qpth_amd import WarmStart
    from qpth_amd.qp import QPFunction
    tq = on(S.soft_problem("a"), env.dev, torch.float64)
    ws = WarmStart()
    with env.run():
        f = QPFunction(verbose=-1, duals=True, warm_start=ws)
        cold = [host(o) for o in f(*tq)]
        assert not host(ws.used).any()
        warm = [host(o) for o in f(*tq)]
        assert host(ws.used).all()
    for a, c in zip(warm, cold):
        assert close(a, c, TOL_REF) <= TOL_REF


def check_sensitivity(env):
    from qpth_amd import sensitivity
    from qpth_amd.qp import QPFunction
    arrs = S.soft_problem("a")
    B, n, m, q = S.SHAPES["a"]
    tq = on(arrs, env.dev, torch.float64)
    K = 3
    V = torch.tensor(np.random.RandomState(6).randn(B, K, n), device=env.dev)
    with env.run():
        sol = sensitivity.solve(*tq[:6], rho=tq[6])
        many = host(sol.vjp_many(dl_dz=V, want=("rho",))["rho"])
        J = sol.jacobian(wrt=("h", "rho"))
        singles = []
        for k in range(K):
            ins = [t.clone().requires_grad_(True) for t in tq]
            z = QPFunction(verbose=-1)(*ins)
            z.backward(V[:, k].contiguous())
            singles.append(host(ins[6].grad))
    assert many.shape == (B, K, m)
    fig = close(many, np.stack(singles, 1), 1e-9)
    note("vjp_many_vs_single", fig)
    assert fig <= 1e-9                         # one factorisation for K right-hand sides against K of them: round-off
    lam, rho = host(sol.lam), arrs[6]
    # h_eff = h + w lam, w = 1 / rho: J[z,rho] = J[z,h] diag(lam) (-1 / rho^2), row-wise (gradcheck pins the sign)
    want = host(J["z", "h"]) * (-lam / rho ** 2)[:, None, :]
    assert host(J["z", "rho"]).shape == (B, n, m)
    assert close(host(J["z", "rho"]), want, 1e-12) <= 1e-12


# ---------------------------------------------------------------- 8. errors
def check_refinement_is_refused_on_soft_factors(env, pytest):
    """refinement and the finishing stage evaluate residuals of the caller's Q, G, A -- the hard QP: every way to them on soft
    factors raises, none runs"""
    from qpth_amd.kkt import KKTFactors
    from qpth_amd.solvers.pdipm import batch as pdipm_b
    Q, p, G, h, A, b, rho = on(S.soft_problem("a"), env.dev, torch.float64)
    B, n, m, q = S.SHAPES["a"]
    d, rx, rz, ry = torch.ones_like(h), torch.ones_like(p), torch.ones_like(h), torch.ones_like(b)
    with env.run():
        fac = KKTFactors.build(Q, G, A, B, w=rho.reciprocal())
        fac.solve_kkt(d, rx, None, rz, ry)                                  # refine = 0: served
        with pytest.raises(ValueError, match="refine=0"):
            fac.solve_kkt(d, rx, None, rz, ry, refine=1)
        with pytest.raises(ValueError, match="refine=0"):
            fac.solve_kkt_many(d, rx.unsqueeze(1), None, None, None, refine=1)
        res = fac.ipm(p, h, b)
        with pytest.raises(ValueError, match="refine=0"):
            fac.backward(res.zhat, res.lam, res.slacks, res.nu, rx, refine=1)
        with pytest.raises(ValueError, match="refine=0"):
            fac.jvp(res.zhat, res.lam, res.slacks, res.nu, (None, rx, None, None, None, None), refine=1)
        with pytest.raises(ValueError, match="soft rows"):
            fac.polish(p, h, b, res)
        Q_LU, S_LU, R = pdipm_b.pre_factor_kkt(Q, G, A, rho)
        with pytest.raises(ValueError, match="refine=0"):
            pdipm_b.solve_kkt_ir(Q_LU, d, G, A, S_LU, rx, None, rz, ry, niter=1)
        with pytest.raises(ValueError, match="soft rows"):
            pdipm_b.forward(Q, p, G, h, A, b, Q_LU, S_LU, R, verbose=-1, solver=pdipm_b.KKTSolvers.IR_UNOPT)
        z = pdipm_b.forward(Q, p, G, h, A, b, *pdipm_b.pre_factor_kkt(Q, G, A, 2.5), verbose=-1)[0]       # a number as rho
        z2 = pdipm_b.forward(Q, p, G, h, A, b, *pdipm_b.pre_factor_kkt(Q, G, A, torch.full_like(rho, 2.5)), verbose=-1)[0]
    assert np.array_equal(host(z), host(z2))


def check_errors(env, pytest):
    from qpth_amd.qp import QPFunction, QPSolvers
    tq = on(S.soft_problem("a"), env.dev, torch.float64)
    six, rho = tq[:6], tq[6]
    with env.run():
        with pytest.raises(ValueError, match="PDIPM_BATCHED"):
            QPFunction(verbose=-1, solver=QPSolvers.CVXPY)(*six, rho)
        with pytest.raises(ValueError, match="refine=0"):
            QPFunction(verbose=-1, refine=1)(*six, rho)
        big32 = on(S.soft_problem("c2", np.float32), env.dev, torch.float32)       # nineq = 120: the float32 kernels + finishing steps
        with pytest.raises(ValueError, match="refine=0"):
            QPFunction(verbose=-1)(*big32)
        for bad in (0.0, -1.0, float("nan")):
            r = rho.clone()
            r[1, 3] = bad
            with pytest.raises(ValueError, match="rho must be positive"):
                QPFunction(verbose=-1)(*six, r)
        with pytest.raises(ValueError, match="rho must be positive"):
            QPFunction(verbose=-1)(*six, 0.0)
        with pytest.raises(ValueError, match="shape"):
            QPFunction(verbose=-1)(*six, rho[:, :-1])
        with pytest.raises(ValueError, match="shape"):
            QPFunction(verbose=-1)(*six, rho[:2])
        with pytest.raises(ValueError, match="float32"):
            QPFunction(verbose=-1)(*six, rho.float())
