"""Elastic inequality rows (QPFunction(...)(Q, p, G, h, A, b, rho, l1=gamma), qpx_ipm_elastic): the checks that
tests/test_emu_elastic.py runs on the host-thread emulator and tests/test_gpu_elastic.py on a real MI355X.  Every check takes
an `env`: env.dev (the torch device) and env.run(variant=0), a context manager around the library calls.

Problems: tests/elastic_reference.py (each shape with every row elastic and with every second row hard).
References: the unmodified reference on the AUGMENTED QP in (z, t) (tests/golden/elastic_*.npz, made by
tests/golden/make_golden_elastic.py), oracle/qp_oracle on the augmented QP for the iteration counts, and the library's own
six- and seven-input calls where no reference is needed.

Gates: against the reference 1e-6 (float64; the project's gate, README); the hard-row equivalence 1e-12 (the two calls run the
same operations on a hard row up to the order in which the step length's minimum is taken); the adjoint identity 1e-9
relative (as tests/soft_checks.py: two solves of one KKT matrix, round-off times its condition).
"""
import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

import elastic_reference as R
import problems
from conftest import load_golden, rel_err

TOL_REF = 1e-6
NAMES = ("dQ", "dp", "dG", "dh", "dA", "db", "drho", "dgamma")
INF = float("inf")
measured = {}        # check name -> worst figure seen (scripts/bench_elastic.py writes them to profiles/elastic.json)


def note(key, value):
    measured[key] = max(float(value), measured.get(key, 0.0))
    print("%-44s %.3e" % (key, value))


def on(arrs, dev):
    return [torch.tensor(np.asarray(x), dtype=torch.float64, device=dev) if np.asarray(x).size
            else torch.empty(0, dtype=torch.float64, device=dev) for x in arrs]


def host(t):
    return t.detach().cpu().numpy()


def close(a, ref):
    """the project's gate on gradients: max |a - ref| <= tol max(1, max |ref|); returns the figure that must be <= tol"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(1.0, np.abs(ref).max()) if ref.size else 0.0


def with_grad(tq):
    for t in tq:
        if t.nelement():
            t.requires_grad_(True)
    return tq


def problem(label, kind):
    """the seeded problem and its fixture; the stored vectors pin the generator"""
    arrs = R.elastic_problem(label, kind)
    g = load_golden(R.fixture_name(label, kind))
    for k, x in zip(("p", "h", "b", "rho", "gamma"), (arrs[1], arrs[3], arrs[5], arrs[6], arrs[7])):
        assert np.array_equal(x, g[k]), k
    return arrs, g


# ---------------------------------------------------------------- 1. parity with the reference on the augmented QP
ONE_WAVE = 2048      # the A/B knob: one wave per QP in the tile kernels -- what the default dispatch picks at four tile rows beyond 512 QPs


def check_reference_parity(env, label, kind, variant=0):
    from qpth_amd.kkt import KKTFactors
    from qpth_amd.qp import QPFunction
    arrs, g = problem(label, kind)
    B, n, m, q = R.SHAPES[label]
    tq = with_grad(on(arrs, env.dev))
    with env.run(variant):
        z = QPFunction(verbose=-1)(*tq[:7], l1=tq[7])
        (z * torch.tensor(g["c"], device=env.dev)).sum().backward()
        # t and the multipliers of t >= 0 are no outputs of the node: the same launch once more, from the factors
        with torch.no_grad():
            fac = KKTFactors.build(tq[0], tq[2], tq[4], B)
            res = fac.ipm_elastic(tq[1], tq[3], tq[7], tq[6], tq[5])
    assert np.array_equal(host(res.zhat), host(z))
    fin = np.isfinite(g["slacks_t"])
    assert np.array_equal(np.isfinite(host(res.slacks_t)), fin) and np.all(host(res.lam_t)[~fin] == 0.0) and np.all(host(res.t)[~fin] == 0.0)
    fig = {"zhat": rel_err(host(z), g["zhat"]).max(), "lam": rel_err(host(res.lam), g["lam"]).max(),
           "lam_t": rel_err(host(res.lam_t), g["lam_t"]).max(), "slacks": close(host(res.slacks), g["slacks"]),
           "slacks_t": close(np.where(fin, host(res.slacks_t), 0.0), np.where(fin, g["slacks_t"], 0.0)),
           "t": close(host(res.t), g["t"])}
    if q:
        fig["nu"] = rel_err(host(res.nu), g["nu"]).max()
    for k, t in zip(NAMES, tq):
        if t.nelement():
            fig[k] = close(host(t.grad), g[k])
    assert np.all(host(tq[6].grad)[~fin] == 0.0) and np.all(host(tq[7].grad)[~fin] == 0.0)        # hard rows: exactly zero
    for k, v in fig.items():
        note("parity/%s%s/%s/%s" % (label, "-1w" if variant else "", kind, k), v)
    assert max(fig.values()) <= TOL_REF, fig


# ---------------------------------------------------------------- 2. iteration counts; the trace of the augmented QP
def augmented(arrs, i):
    Q, p, G, h, A, b, rho, gamma = arrs
    q = np.shape(A)[1] if np.size(A) else 0
    return R.augment(Q[i], p[i], G[i], h[i], A[i] if q else np.zeros(0), gamma[i], rho[i]) + (b[i] if q else np.zeros(0),)


def oracle_iters(arrs, i, eps):
    from oracle import qp_oracle as orc
    Q2, p2, G2, h2, A2, F, b = augmented(arrs, i)
    q = b.size
    # (one thread: a QP of this size is microseconds of work, and the default pool is sized by the machine's CPU count)
    o = orc.OracleQP(Q2[None], p2[None], G2[None], h2[None], A2[None] if q else None, b[None] if q else None, nthreads=1)
    return o.forward(eps, 20, 3, True, 1)[4]["iters"][0]


def check_iteration_counts(env, label, kind, variant=0, gated=True):
    """eps = 1e-8, the reference's stall counter: the counts of oracle/qp_oracle on the augmented QP, each QP alone (gated at
    the shapes of R.COUNTED, printed elsewhere)"""
    from qpth_amd.kkt import KKTFactors
    arrs = R.elastic_problem(label, kind)
    B = R.SHAPES[label][0]
    tq = on(arrs, env.dev)
    with env.run(variant):
        fac = KKTFactors.build(tq[0], tq[2], tq[4], B)
        res = fac.ipm_elastic(tq[1], tq[3], tq[7], tq[6], tq[5], eps=1e-8, stall_policy=1)
    mine = host(res.iters)
    ref = np.array([oracle_iters(arrs, i, 1e-8) for i in range(B)])
    print("iters %s/%s elastic" % (label, kind), mine, "augmented", ref)
    note("iters_gap/%s%s/%s" % (label, "-1w" if variant else "", kind), np.abs(mine - ref).max())
    if gated:
        assert np.array_equal(mine, ref)


TRACED = (("t1a", "all"), ("t1b", "half"), ("t2", "all"), ("t4", "all"))      # nz' + neq + m' <= 208: 20, 34, 95, 144


def check_trace(env, label, kind):
    """the trace (pri_resid, dual_resid, mu per iteration) is that of the library's own six-input loop on the augmented QP, each QP
    alone: this pins || G'^T 1 || (the dual residual's norm) and m' (mu's divisor)"""
    from qpth_amd.kkt import KKTFactors
    arrs = R.elastic_problem(label, kind)
    B = R.SHAPES[label][0]
    tq = on(arrs, env.dev)
    with env.run():
        fac = KKTFactors.build(tq[0], tq[2], tq[4], B)
        res = fac.ipm_elastic(tq[1], tq[3], tq[7], tq[6], tq[5], eps=1e-8, stall_policy=1, want_trace=True)
    tr, it = host(res.trace), host(res.iters)
    worst, top = 0.0, 0.0
    for i in range(B):
        Q2, p2, G2, h2, A2, F, b = augmented(arrs, i)
        t2 = on((Q2[None], p2[None], G2[None], h2[None], A2[None] if b.size else A2, b[None] if b.size else b), env.dev)
        with env.run():
            f2 = KKTFactors.build(t2[0], t2[2], t2[4] if b.size else None, 1)
            r2 = f2.ipm(t2[1], t2[3], t2[5] if b.size else None, eps=1e-8, stall_policy=1, want_trace=True)
        it2 = host(r2.iters)[0]
        assert it[i] == it2, (it[i], it2)
        mine, ref = tr[:it2, i], host(r2.trace)[:it2, 0]
        worst = max(worst, (np.abs(mine - ref) / np.maximum(1.0, np.abs(ref))).max())
        top = max(top, ref[:, 1].max())
    note("trace/%s/%s" % (label, kind), worst)
    assert top > 1e-3, top                       # the shift of the start point is there: || G'^T 1 || takes part
    assert worst <= TOL_REF


# ---------------------------------------------------------------- 3. exactness; 4. hard rows; 5. gamma = 0
def feasible(label, dev):
    B, n, m, q = R.SHAPES[label]
    return on(problems.random_dense_qp(B, n, m, q, seed=R.SEED), dev), B


def check_exactness(env, label="t1b"):
    """a feasible hard QP and gamma = 10 max lam* of the six-input call: the hard QP's solution, t = 0"""
    from qpth_amd.kkt import KKTFactors
    six, B = feasible(label, env.dev)
    with env.run():
        fac = KKTFactors.build(six[0], six[2], six[4], B)
        hard = fac.ipm(six[1], six[3], six[5])
        gam = torch.full_like(six[3], 10.0 * float(hard.lam.max()))
        res = fac.ipm_elastic(six[1], six[3], gam, torch.full_like(six[3], 2.0), six[5])
    assert float(hard.lam.max()) > 1e-2
    fig = {"zhat": close(host(res.zhat), host(hard.zhat)), "t": float(host(res.t).max())}
    for k, v in fig.items():
        note("exact/%s/%s" % (label, k), v)
    assert fig["zhat"] <= TOL_REF and fig["t"] <= 1e-8 and host(res.t).min() >= -1e-8


def check_hard_rows(env, label, variant=0):
    """gamma = +inf everywhere is the six-input call: its iteration counts, its values to 1e-12, dgamma = drho = 0 exactly"""
    from qpth_amd.kkt import KKTFactors
    from qpth_amd.qp import QPFunction
    B, n, m, q = R.SHAPES[label]
    arrs = problems.random_dense_qp(B, n, m, q, seed=R.SEED)            # (feasible as a hard QP: the elastic fixtures' h is not)
    c = torch.tensor(R.loss_vector(label), device=env.dev)
    outs = []
    for elastic in (False, True):
        tq = with_grad(on(arrs, env.dev))
        rho = torch.full((B, m), 3.0, dtype=torch.float64, device=env.dev, requires_grad=True)
        gam = torch.full((B, m), INF, dtype=torch.float64, device=env.dev, requires_grad=True)
        with env.run(variant):
            z = QPFunction(verbose=-1)(*tq, rho, l1=gam) if elastic else QPFunction(verbose=-1)(*tq)
            (z * c).sum().backward()
            with torch.no_grad():
                fac = KKTFactors.build(tq[0], tq[2], tq[4], B)
                res = fac.ipm_elastic(tq[1], tq[3], gam.detach(), rho.detach(), tq[5]) if elastic else fac.ipm(tq[1], tq[3], tq[5])
        outs.append((host(res.iters), [host(z)] + [host(t.grad) for t in tq if t.nelement()] + [host(res.lam), host(res.slacks)]))
        if elastic:
            assert np.all(host(rho.grad) == 0.0) and np.all(host(gam.grad) == 0.0)
            assert np.all(host(res.lam_t) == 0.0) and np.all(np.isposinf(host(res.slacks_t))) and np.all(host(res.t) == 0.0)
    assert np.array_equal(outs[0][0], outs[1][0]), (outs[0][0], outs[1][0])
    worst = max(close(a, r) for a, r in zip(outs[1][1], outs[0][1]))
    note("hard_rows/" + label + ("-1w" if variant else ""), worst)
    assert worst <= 1e-12


def check_gamma_zero(env, label="t1b"):
    """gamma = 0 is the quadratic penalty alone: zhat of the positional-rho call"""
    from qpth_amd.qp import QPFunction
    arrs = R.elastic_problem(label, "all")
    tq = on(arrs, env.dev)
    with env.run():
        z = QPFunction(verbose=-1)(*tq[:7], l1=0.0)
        zs = QPFunction(verbose=-1)(*tq[:7])
    fig = close(host(z), host(zs))
    note("gamma_zero/" + label, fig)
    assert fig <= TOL_REF


# ---------------------------------------------------------------- 6. the closed form
def check_closed_form(env):
    """z <= -1, -z <= -1 with Q = I, p = 0, gamma = 2, rho = 10: zhat = 0, t = 1, lam = 12, s = 0 on both rows"""
    from qpth_amd.kkt import KKTFactors
    Q, p, G, h = on((np.eye(1)[None], np.zeros((1, 1)), np.array([[[1.0], [-1.0]]]), np.array([[-1.0, -1.0]])), env.dev)
    with env.run():
        fac = KKTFactors.build(Q, G, None, 1)
        res = fac.ipm_elastic(p, h, torch.full_like(h, 2.0), torch.full_like(h, 10.0), None)
    fig = {"zhat": np.abs(host(res.zhat)).max(), "t": np.abs(host(res.t) - 1.0).max(), "lam": np.abs(host(res.lam) - 12.0).max() / 12.0,
           "s": np.abs(host(res.slacks)).max()}
    for k, v in fig.items():
        note("closed_form/" + k, v)
    assert max(fig.values()) <= TOL_REF, fig


# ---------------------------------------------------------------- 7. gradcheck, 8. adjointness, 9. duals, reductions
def small_problem(dev):
    """(6, 4, 2) with a violated row, away from kinks (asserted by the callers): (L, p, G, h, A, b, rho, gamma), Q = L L' + I"""
    B, n, m, q = 2, 6, 4, 2
    r = np.random.RandomState(13)
    L = r.randn(B, n, n) / np.sqrt(n)
    G, z0, A = r.randn(B, m, n), r.randn(B, n), r.randn(B, q, n)
    h = np.einsum("bmn,bn->bm", G, z0) + 0.4 * r.rand(B, m) - 1.2 * r.rand(B, m) * (np.arange(m) % 2 == 0)
    return on((L, 2.0 * r.randn(B, n), G, h, A, np.einsum("bqn,bn->bq", A, z0), 0.5 + 2.0 * r.rand(B, m), 0.3 + r.rand(B, m)), dev)


def small_solution(env, ins):
    from qpth_amd.kkt import KKTFactors
    eye = torch.eye(6, dtype=torch.float64, device=env.dev)
    with env.run():
        fac = KKTFactors.build(ins[0] @ ins[0].transpose(-1, -2) + eye, ins[2], ins[4], 2)
        res = fac.ipm_elastic(ins[1], ins[3], ins[7], ins[6], ins[5])
    lu, lt, su, st, t = [host(x) for x in (res.lam, res.lam_t, res.slacks, res.slacks_t, res.t)]
    assert np.all(np.maximum(lu, su) > 1e-2) and np.all(np.maximum(lt, st) > 1e-2), (lu, su, lt, st)          # no kink nearby
    assert (t > 1e-2).any() and (lt > 1e-2).any()
    return eye


def check_gradcheck(env):
    """torch.autograd.gradcheck over all eight inputs in reverse mode (Q = L L' + I through L, as tests/soft_checks.py).
    eps = 1e-6; atol 1e-5 covers the central difference's noise, the solution's ~1e-11 over 2 eps, rtol 1e-3 its truncation."""
    from qpth_amd.qp import QPFunction
    ins = small_problem(env.dev)
    eye = small_solution(env, ins)
    for t in ins:
        t.requires_grad_(True)

    def f(L, p, G, h, A, b, rho, gam):
        return QPFunction(verbose=-1)(L @ L.transpose(-1, -2) + eye, p, G, h, A, b, rho, l1=gam)

    with env.run():
        assert torch.autograd.gradcheck(f, ins, eps=1e-6, atol=1e-5, rtol=1e-3, check_forward_ad=False)


def check_adjoint_identity(env, label="t1b", kind="half"):
    """per QP: <v, z'> = sum over the eight inputs of <grad, tangent>, z' from forward mode through the public call, the
    tangents of gamma and rho included; under duals=True the same with cotangents on lam and nu"""
    from qpth_amd.qp import QPFunction
    arrs = R.elastic_problem(label, kind)
    B, n, m, q = R.SHAPES[label]
    r = np.random.RandomState(9)
    tans = [r.randn(*np.shape(x)) for x in arrs]
    tans[0] = 0.5 * (tans[0] + np.swapaxes(tans[0], -1, -2))
    tans[7] = np.where(np.isfinite(arrs[7]), tans[7], 0.0)
    v, vl, vn = r.randn(B, n), r.randn(B, m), r.randn(B, q)
    for duals in (False, True):
        tq = with_grad(on(arrs, env.dev))
        with env.run():
            out = QPFunction(verbose=-1, duals=duals)(*tq[:7], l1=tq[7])
            if duals:
                loss = (out[0] * torch.tensor(v, device=env.dev)).sum() + (out[2] * torch.tensor(vl, device=env.dev)).sum() \
                    + (out[1] * torch.tensor(vn, device=env.dev)).sum()
            else:
                loss = (out * torch.tensor(v, device=env.dev)).sum()
            loss.backward()
        rhs = np.stack([(host(t.grad) * tn).reshape(B, -1).sum(1) for t, tn in zip(tq, tans)])
        prim, tang = on(arrs, env.dev), on(tans, env.dev)
        with env.run(), fwAD.dual_level():
            out = QPFunction(verbose=-1, duals=duals)(*[fwAD.make_dual(x, t) for x, t in zip(prim[:7], tang[:7])],
                                                      l1=fwAD.make_dual(prim[7], tang[7]))
            if duals:
                zt, nt, lt = [host(fwAD.unpack_dual(o).tangent) for o in out[:3]]
                lhs = (zt * v).sum(1) + (lt * vl).sum(1) + (nt * vn).sum(1)
            else:
                lhs = (host(fwAD.unpack_dual(out).tangent) * v).sum(1)
        gap = np.abs(lhs - rhs.sum(0)) / (np.abs(lhs) + np.abs(rhs).sum(0))
        note("adjoint_gap" + ("/duals" if duals else ""), gap.max())
        assert np.abs(rhs[6]).min() > 0 and np.abs(rhs[7]).min() > 0              # the rho and gamma terms take part
        assert gap.max() <= 1e-9, gap


def check_duals(env, label="t1b"):
    """duals=True: (zhat, nu, lam, slacks) and the gradients of a loss on (zhat, lam, nu) against the reference's general KKT
    solve at its own solution of the augmented QP (the fixtures' du_*)"""
    from qpth_amd.qp import QPFunction
    for kind in R.KINDS:
        arrs, g = problem(label, kind)
        tq = with_grad(on(arrs, env.dev))
        with env.run():
            z, nu, lam, sl = QPFunction(verbose=-1, duals=True)(*tq[:7], l1=tq[7])
            assert not sl.requires_grad
            ((z * torch.tensor(g["g_z"], device=env.dev)).sum() + (lam * torch.tensor(g["g_lam"], device=env.dev)).sum()
             + (nu * torch.tensor(g["g_nu"], device=env.dev)).sum()).backward()
        fig = {"zhat": rel_err(host(z), g["zhat"]).max(), "nu": rel_err(host(nu), g["nu"]).max(),
               "lam": rel_err(host(lam), g["lam"]).max(), "slacks": close(host(sl), g["slacks"])}
        for k, t in zip(NAMES, tq):
            fig["du_" + k] = close(host(t.grad), g["du_" + k])
        for k, v in fig.items():
            note("duals/%s/%s/%s" % (label, kind, k), v)
        assert max(fig.values()) <= TOL_REF, fig
        # an output the loss does not use costs nothing, and no cotangent at all gives no gradient
        tq = with_grad(on(arrs, env.dev))
        with env.run():
            z, nu, lam, sl = QPFunction(verbose=-1, duals=True)(*tq[:7], l1=tq[7])
            lam.sum().backward()
        assert all(t.grad is not None for t in tq)


def check_reductions(env):
    """gamma and rho the batch shares: the `.mean(0)` of the per-QP gradient; a scalar: summed over the rows as well"""
    from qpth_amd.qp import QPFunction
    L, p, G, h, A, b, rho, gam = small_problem(env.dev)
    Q = L @ L.transpose(-1, -2) + torch.eye(6, dtype=torch.float64, device=env.dev)
    c = torch.tensor(np.random.RandomState(4).randn(2, 6), device=env.dev)

    def grads_of(r_, g_):
        r_ = (r_.clone() if torch.is_tensor(r_) else torch.tensor(r_, dtype=torch.float64, device=env.dev)).requires_grad_(True)
        g_ = (g_.clone() if torch.is_tensor(g_) else torch.tensor(g_, dtype=torch.float64, device=env.dev)).requires_grad_(True)
        with env.run():
            z = QPFunction(verbose=-1)(Q, p, G, h, A, b, r_, l1=g_)
            (z * c).sum().backward()
        return host(z), host(r_.grad), host(g_.grad)

    z1, r1, g1 = grads_of(rho[0].expand(2, -1).contiguous(), gam[0].expand(2, -1).contiguous())
    z2, r2, g2 = grads_of(rho[0], gam[0])
    assert np.array_equal(z1, z2) and r2.shape == (4,) and g2.shape == (4,)
    assert close(r2, r1.mean(0)) <= 1e-12 and close(g2, g1.mean(0)) <= 1e-12
    assert np.abs(r1).max() > 0 and np.abs(g1).max() > 0
    z3, r3, g3 = grads_of(torch.full((2, 4), 1.5, dtype=torch.float64, device=env.dev), torch.full((2, 4), 0.7, dtype=torch.float64, device=env.dev))
    z4, r4, g4 = grads_of(1.5, 0.7)
    assert np.array_equal(z3, z4) and r4.shape == () and g4.shape == ()
    assert close(r4, r3.mean(0).sum()) <= 1e-12 and close(g4, g3.mean(0).sum()) <= 1e-12
    with env.run():                                                   # Python floats
        z5 = QPFunction(verbose=-1)(Q, p, G, h, A, b, 1.5, l1=0.7)
    assert np.array_equal(host(z5), z4)


# ---------------------------------------------------------------- 10. status, refusals, the old call
def check_abi_codes(env):
    """QPX_ERR_* of the entry point and qpx_elastic_supported, no launch"""
    from qpth_amd import _lib
    with env.run():
        dll = _lib.backend_for(torch.empty(0, device=env.dev)).dll
        for (n, m, q) in [R.SHAPES[k][1:] for k in R.SHAPES]:
            assert dll.qpx_elastic_supported(_lib.QPX_F64, n, m, q) == 1
            assert dll.qpx_elastic_supported(_lib.QPX_F32, n, m, q) == 0
            assert dll.qpx_elastic_supported(_lib.QPX_F32_WIDE, n, m, q) == 0
        assert dll.qpx_elastic_supported(_lib.QPX_F64, 100, 100, 10) == 0          # the large-QP family
        assert dll.qpx_elastic_supported(_lib.QPX_F64, 200, 200, 0) == 0           # the augmented QP itself
        assert dll.qpx_elastic_supported(_lib.QPX_F64, 0, 4, 0) == 0
        one = torch.ones(512, dtype=torch.float64, device=env.dev)
        i32 = torch.zeros(8, dtype=torch.int32, device=env.dev)
        P = one.data_ptr()

        def ipm(dtype, n, m, q, gamma=P, rho=P, gt1=P, lam_t=P, t=P, sg=0):
            return dll.qpx_ipm_elastic(dtype, 1, n, m, q, P, 0, P, 0, P, 0, P, 0, 1e-8, 20, 3, 1, P, P, P, P, i32.data_ptr(),
                                       i32.data_ptr(), P, None, gamma, sg, rho, 0, gt1, lam_t, P, t, None)

        assert ipm(_lib.QPX_F32, 6, 4, 2) == -2 and ipm(_lib.QPX_F32_WIDE, 6, 4, 2) == -2                    # QPX_ERR_UNSUPPORTED
        assert ipm(_lib.QPX_F64, 100, 100, 10) == -2
        for kw in ({"gamma": None}, {"rho": None}, {"gt1": None}, {"lam_t": None}, {"t": None}, {"sg": -1}):      # QPX_ERR_ARG
            assert ipm(_lib.QPX_F64, 6, 4, 2, **kw) == -1, kw
        assert ipm(7, 6, 4, 2) == -1 and ipm(_lib.QPX_F64, 6, 0, 2) == -1
        # the A/B knob: a form without the role declines
        old = dll.qpx_set_ipm_variant(256)                                       # the 16x16 thread grid at every size
        try:
            assert dll.qpx_elastic_supported(_lib.QPX_F64, 6, 4, 2) == 0 and ipm(_lib.QPX_F64, 6, 4, 2) == -2
        finally:
            dll.qpx_set_ipm_variant(old)


def check_bad_entries(env, pytest):
    from qpth_amd import _lib
    from qpth_amd.kkt import KKTFactors
    from qpth_amd.qp import QPFunction
    arrs = R.elastic_problem("t1b", "half")
    tq = on(arrs, env.dev)
    six, rho, gam = tq[:6], tq[6], tq[7]
    with env.run():
        for bad in (float("nan"), -0.5, -INF):
            g = gam.clone()
            g[1, 4] = bad
            with pytest.raises(ValueError, match="l1 must be non-negative"):
                QPFunction(verbose=-1)(*six, rho, l1=g)
        for bad in (float("nan"), 0.0, -1.0):
            r_ = rho.clone()
            r_[1, 4] = bad
            with pytest.raises(ValueError, match="rho must be positive"):
                QPFunction(verbose=-1)(*six, r_, l1=gam)
        with pytest.raises(ValueError, match="l1 must be non-negative"):
            QPFunction(verbose=-1)(*six, rho, l1=-1.0)
        # the QP is left as the `Q not SPD` path leaves one; its neighbour is solved
        g = gam.clone()
        g[1, 4] = float("nan")
        fac = KKTFactors.build(tq[0], tq[2], tq[4], 2)
        res = fac.ipm_elastic(tq[1], tq[3], g, rho, tq[5])
        good = fac.ipm_elastic(tq[1], tq[3], gam, rho, tq[5])
    st = host(res.status)
    assert st[1] & _lib.ST_NONFINITE and not st[0] & _lib.ST_NONFINITE
    assert host(res.iters)[1] == 0 and np.isposinf(host(res.best_resid)[1])
    for x in (res.zhat, res.nu, res.lam, res.slacks, res.lam_t, res.slacks_t, res.t):
        assert np.isnan(host(x)[1]).all()
    assert np.array_equal(host(res.zhat)[0], host(good.zhat)[0])
    # the bit stays with the launch that met it; the factors' own status words never saw it
    with env.run():
        fac.raise_on_failure()
        fac.ipm_elastic(tq[1], tq[3], g, rho, tq[5])
        with pytest.raises(ValueError, match="l1 must be non-negative"):
            fac.raise_on_failure()
    assert not (host(fac.status) & _lib.ST_NONFINITE).any()


def check_refusals(env, pytest):
    from qpth_amd import WarmStart
    from qpth_amd.qp import QPFunction, QPSolvers
    arrs = R.elastic_problem("t1b", "half")
    tq = on(arrs, env.dev)
    six, rho, gam = tq[:6], tq[6], tq[7]
    way_out = r"augmented dense QP"
    with env.run():
        with pytest.raises(ValueError, match="curvature.*pure l1 penalty"):
            QPFunction(verbose=-1)(*six, l1=gam)
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1)(*[t.float() for t in six], rho.float(), l1=gam.float())
        big = on(R.elastic_problem("c7", "all"), env.dev)
        A = torch.zeros(2, 10, 100, dtype=torch.float64, device=env.dev)
        with pytest.raises(ValueError, match=way_out):                     # nz + neq + nineq = 210: the large-QP family
            QPFunction(verbose=-1)(big[0], big[1], big[2], big[3], A, A[:, :, 0], big[6], l1=big[7])
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1)(*six, rho, kappa=1e-3, l1=gam)
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1)(*six, rho, lower=tq[3] - 1.0, l1=gam)
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1, refine=1)(*six, rho, l1=gam)
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1, warm_start=WarmStart())(*six, rho, l1=gam)
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1, solver=QPSolvers.CVXPY)(*six, rho, l1=gam)
        with pytest.raises(ValueError, match="shape"):
            QPFunction(verbose=-1)(*six, rho, l1=gam[:, :-1])
        with pytest.raises(ValueError, match="shape"):
            QPFunction(verbose=-1)(*six, rho, l1=gam[:1].expand(3, -1))
        # a second grad
        ins = [t.clone().requires_grad_(True) for t in tq]
        z = QPFunction(verbose=-1)(*ins[:7], l1=ins[7])
        (gp,) = torch.autograd.grad(z.sum(), ins[1], create_graph=True)
        with pytest.raises(RuntimeError):
            torch.autograd.grad(gp.sum(), ins[3])


def check_l1_none_is_the_old_call(env):
    from qpth_amd.qp import QPFunction
    arrs = R.elastic_problem("t1b", "all")[:7]
    for k, node in ((6, "QPFunctionFn"), (7, "QPSoftFunctionFn")):
        outs = []
        for extra in ({}, {"l1": None}):
            tq = with_grad(on(arrs[:k], env.dev))
            with env.run():
                z = QPFunction(verbose=-1)(*tq, **extra)
                assert type(z.grad_fn).__name__.startswith(node)
                z.backward(torch.ones_like(z))
            outs.append([host(z)] + [host(t.grad) for t in tq])
        for a, c in zip(*outs):
            assert np.array_equal(a, c)


# ---------------------------------------------------------------- 11. the library's own call on the augmented QP (shapes without a fixture)
SLOT_SHAPES = {          # the slot counts no fixture reaches: nz > 64 or > 128 beside few rows -- (n, m, q) -> the loop form
    "s12": (130, 9, 0),      # one tile row, four slots
    "s22": (100, 20, 30),    # two tile rows, two slots
    "s44": (130, 60, 10),    # four-row chain form, four slots
    "s74": (130, 70, 5),     # seven-row chain form, four slots
    "s11b": (70, 12, 0),     # one tile row, two slots
    "s24": (130, 20, 0),     # two tile rows, four slots
}


def check_augmented_call(env, key, kind="half", variant=0):
    """elastic call against the library's six-input call on the augmented QP, each QP alone: zhat and the eight gradients folded
    back, at the project's gate (two paths of the library, whichever family serves the augmented QP)"""
    from qpth_amd.qp import QPFunction
    n, m, q = SLOT_SHAPES[key]
    B = 2
    r = np.random.RandomState(61)
    L = r.randn(B, n, n)
    Q = np.matmul(L, L.transpose((0, 2, 1))) / n + np.eye(n)
    G, z0, p, A = r.randn(B, m, n), r.randn(B, n), r.randn(B, n), r.randn(B, q, n)
    gamma, rho = 0.2 + 3.0 * r.rand(B, m), 0.5 + 4.0 * r.rand(B, m)
    pull = 1.5 * r.rand(B, m) * (np.arange(m) % 3 == 0)
    h = np.einsum("bmn,bn->bm", G, z0) + 0.5 * r.rand(B, m)
    b = np.einsum("bqn,bn->bq", A, z0)
    if kind == "half":
        gamma[:, 1::2] = np.inf
        pull[:, 1::2] = 0.0
    h = h - pull
    c = r.randn(B, n)
    arrs = (Q, p, G, h, A if q else np.zeros(0), b if q else np.zeros(0), rho, gamma)
    tq = with_grad(on(arrs, env.dev))
    with env.run(variant):
        z = QPFunction(verbose=-1)(*tq[:7], l1=tq[7])
        (z * torch.tensor(c, device=env.dev)).sum().backward()
    worst = 0.0
    for i in range(B):
        Q2, p2, G2, h2, A2, F, bi = augmented(arrs, i)
        t2 = with_grad(on((Q2, p2, G2, h2, A2, bi), env.dev))
        with env.run():
            z2 = QPFunction(verbose=-1)(*t2)
            (z2[:, :n] * torch.tensor(c[i:i + 1], device=env.dev)).sum().backward()
        dA2 = host(t2[4].grad) if q else np.zeros((0, n))
        f = R.fold(host(t2[0].grad), host(t2[1].grad), host(t2[2].grad), host(t2[3].grad), dA2, F, n, m)
        ref = [host(z2)[0, :n]] + list(f[:4]) + list(f[5:]) + ([f[4], host(t2[5].grad)] if q else [])
        mine = [host(z)[i]] + [host(tq[k].grad)[i] for k in (0, 1, 2, 3, 6, 7)] + ([host(tq[4].grad)[i], host(tq[5].grad)[i]] if q else [])
        worst = max([worst] + [close(a, x) for a, x in zip(mine, ref)])
    note("augmented_call/%s/%s" % (key, kind), worst)
    assert worst <= TOL_REF
