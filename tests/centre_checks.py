"""The barrier-smoothed QP (QPFunction(...)(Q, p, G, h, A, b, kappa=...), qpx_centre): the checks that
tests/test_emu_centre.py runs on the host-thread emulator and tests/test_gpu_centre.py on a real MI355X.  Every check takes an
`env`: env.dev (the torch device) and env.run(variant=0), a context manager around the library calls.

Problems: problems.prof_qp (the benchmark generator).  Reference: tests/centre_reference.py, computed once per (shape, kappa)
and shared.  Gates: the project's 1e-6 against the reference (conftest.rel_err per QP for zhat, lam, s, nu; max |a - ref| <=
1e-6 max(1, max |ref|) for gradients, as tests/soft_checks.py); the second-order pass tests/test_gpu_backward2.py's 2.5e-10
against the closed form at the kernel's own centred point; the adjoint identity 1e-9; the stop test kappa_tol = 1e-9 in
kappa_steps = 20 steps."""
import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

import centre_reference as cr
import problems
from conftest import rel_err
from hvp_reference import NAMES as HNAMES, first_backward, random_W, second_order

TOL_REF = 1e-6
TOL_B2 = 2.5e-10          # tests/test_gpu_backward2.py: GATE
KAPPA_TOL, KAPPA_STEPS = 1e-9, 20
measured = {}             # name -> worst figure seen (scripts/bench_centre.py writes the step counts to profiles/centre.json)


def note(key, value):
    measured[key] = max(float(value), measured.get(key, 0.0))
    print("%-44s %.3e" % (key, value))


def on(arrs, dev, grad=False):
    out = []
    for x in arrs:
        x = np.asarray(x, np.float64)
        t = torch.tensor(x, device=dev) if x.size else torch.empty(0, dtype=torch.float64, device=dev)
        out.append(t.requires_grad_(True) if (grad and x.size) else t)
    return out


def host(t):
    return t.detach().cpu().numpy()


def close(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(1.0, np.abs(ref).max()) if ref.size else 0.0


def kappa_of(kind, B, m):
    """a float, or a numpy array: "rows" -- (m,), spread over two decades; "qps" -- (B, m), one value per QP over two decades"""
    if kind == "rows":
        return 1e-3 * 10 ** np.random.RandomState(11).uniform(-1, 1, m)
    if kind == "qps":
        return np.repeat((1e-3 * 10 ** np.linspace(-1, 1, B))[:, None], m, 1)
    return float(kind)


_REF = {}


def problem(shape, seed, kind):
    """(arrs, kappa, reference (zhat, lam, s, nu)) -- made once, never written to"""
    key = (shape, seed, str(kind))
    if key not in _REF:
        B, n, m, q = shape
        arrs = [np.asarray(a, np.float64) for a in problems.prof_qp(B, n, m, q, seed=seed)]
        kappa = kappa_of(kind, B, m)
        sol, _, res = cr.centre(arrs, kappa, B=B)
        assert res.max() <= 1e-11, res                      # the floor of float64 on the data at nz = 100: ~3e-13
        _REF[key] = (arrs, kappa, sol)
    return _REF[key]


def kappa_input(kappa, dev, grad=False):
    if isinstance(kappa, float):
        return kappa
    t = torch.tensor(kappa, device=dev)
    return t.requires_grad_(True) if grad else t


# ------------------------------------------------------------------------------------------------ 1. forward
def forward(env, shape, seed, kind, variant=0):
    """the launches of QPFunction's forward one by one -- the kernel's own figures -- and QPFunction itself"""
    from qpth_amd import _lib
    from qpth_amd.kkt import KKTFactors
    from qpth_amd.qp import QPFunction
    B, n, m, q = shape
    arrs, kappa, ref = problem(shape, seed, kind)
    Q, p, G, h, A, b = on(arrs, env.dev)
    kap = torch.tensor(cr.kappa_rows(kappa, B, m), device=env.dev)
    eps = max(1e-12, m * kappa) if isinstance(kappa, float) else 1e-12
    with env.run(variant):
        assert _lib.backend_for(Q).dll.qpx_centre_supported(_lib.QPX_F64, n, m, q) == 1
        fac = KKTFactors.build(Q, G, A, nBatch=B)
        r = fac.ipm(p, h, b, eps)
        loop_iters = host(r.iters).copy()
        r = fac.centre(p, h, b, r, kap, tol=KAPPA_TOL, max_steps=KAPPA_STEPS)
        out = QPFunction(verbose=-1, duals=True, kappa_tol=KAPPA_TOL, kappa_steps=KAPPA_STEPS)(Q, p, G, h, A, b, kappa=kappa_input(kappa, env.dev))
    sol = [host(x) for x in (r.zhat, r.lam, r.slacks, r.nu)]
    steps, resid, status = host(r.centre_steps), host(r.centre_resid), host(fac.status)
    tag = "%dx%dx%dx%d/%s/%d" % (shape + (kind, variant))
    print(tag, "loop iterations", loop_iters.tolist(), "centring steps", steps.tolist())
    note("centre_steps " + tag, steps.max())
    note("centre_steps worst", steps.max())
    note("centre_resid " + tag, resid.max())
    assert (resid <= KAPPA_TOL).all() and not (status & _lib.ST_NOT_CENTRED).any() and not (status & _lib.ST_KKT_BREAKDOWN).any()
    assert (steps <= KAPPA_STEPS).all()
    mine = cr.residual(arrs, sol, kappa).max()
    note("numpy residual " + tag, mine)
    assert mine <= 10 * KAPPA_TOL
    assert (sol[1] > 0).all() and (sol[2] > 0).all()
    for name, a, c in zip(("zhat", "lam", "s", "nu"), sol, ref):
        if c.size:
            gap = rel_err(a, c).max()
            note("%s vs reference %s" % (name, tag), gap)
            assert gap <= TOL_REF, name
    # QPFunction makes the same launches: (zhat, nu, lam, slacks)
    for a, c in zip(out, (r.zhat, r.nu, r.lam, r.slacks)):
        assert torch.equal(a.detach(), c) or not c.numel()


# ------------------------------------------------------------------------------------------------ 2. first order
def reduce_dkappa(dk, kappa):
    """the per-QP (B, m) gradient as the call returns it for this kappa: `.mean(0)` for a shared one, a scalar also summed"""
    if isinstance(kappa, float) or np.ndim(kappa) == 0:
        return dk.mean(0).sum()
    return dk.mean(0) if np.ndim(kappa) == 1 else dk


def first_order(env, shape, seed, kind, duals, unbatched=(), variant=0):
    """all six gradients and dkappa of a loss of zhat (duals: of zhat, lam, nu) against the reference at ITS centred point"""
    from qpth_amd.qp import QPFunction
    B, n, m, q = shape
    arrs, kappa, ref = problem(shape, seed, kind)
    if unbatched:          # every QP sees row 0 of an un-batched parameter
        arrs = [np.broadcast_to(a[0], a.shape).copy() if i in unbatched else a for i, a in enumerate(arrs)]
        ref = cr.centre(arrs, kappa, B=B)[0]
    r = np.random.RandomState(seed + 50)
    cots = (r.randn(B, n), r.randn(B, m) if duals else None, r.randn(B, q) if (duals and q) else None)
    tq = on([a[0] if i in unbatched else a for i, a in enumerate(arrs)], env.dev, grad=True)
    kt = kappa_input(kappa, env.dev, grad=True)
    if isinstance(kt, float):
        kt = torch.tensor(kt, dtype=torch.float64, device=env.dev, requires_grad=True)         # a 0-dim tensor: the scalar kappa
    with env.run(variant):
        out = QPFunction(verbose=-1, duals=duals, eps=1e-12 if not isinstance(kappa, float) else max(1e-12, m * kappa),
                         kappa_tol=KAPPA_TOL, kappa_steps=KAPPA_STEPS)(*tq, kappa=kt)
        z, nu, lam = (out[0], out[1], out[2]) if duals else (out, None, None)
        loss = sum((o * torch.tensor(c, device=env.dev)).sum() for o, c in zip((z, lam, nu), cots) if c is not None)
        params = [x for x in tq if x.nelement()]
        g = torch.autograd.grad(loss, params + [kt])
    six, dk, _ = cr.grads(arrs, ref, cots)
    want = [x.mean(0) if i in unbatched else x for i, x in enumerate(six) if x.size]
    names = [nm for nm, x in zip(("dQ", "dp", "dG", "dh", "dA", "db"), six) if x.size]
    tag = "%dx%dx%dx%d/%s%s" % (shape + (kind, "/duals" if duals else ""))
    for nm, a, w in zip(names, g[:-1], want):
        gap = close(host(a), w)
        note("%s %s" % (nm, tag), gap)
        assert gap <= TOL_REF, nm
    wk = reduce_dkappa(dk, kappa)
    assert tuple(g[-1].shape) == tuple(np.shape(wk))
    gap = close(host(g[-1]), wk)
    note("dkappa %s" % tag, gap)
    assert gap <= TOL_REF
    assert np.abs(wk).max() > 1e-6                       # (the gate is not met by zeros)


def adjoint_identity(env, shape, seed, variant=0):
    """forward mode against reverse mode: <dl, (z', lam', nu')> = sum <grad_i, t_i> + <dkappa, tkappa>, per-QP kappa"""
    from qpth_amd.qp import QPFunction
    B, n, m, q = shape
    arrs, kappa, _ = problem(shape, seed, "qps")
    r = np.random.RandomState(seed + 60)
    prim = on(arrs, env.dev, grad=True) + [torch.tensor(kappa, device=env.dev, requires_grad=True)]
    tans = [torch.tensor(r.randn(*x.shape), device=env.dev) if x.nelement() else None for x in prim]
    tans[0] = 0.5 * (tans[0] + tans[0].transpose(1, 2))                      # (Q stays symmetric)
    tans[6] = tans[6] * prim[6].detach()                                     # (a relative tangent: kappa spans decades)
    cots = [torch.tensor(r.randn(B, k), device=env.dev) for k in (n, m, q)]
    f = QPFunction(verbose=-1, duals=True, kappa_tol=KAPPA_TOL, kappa_steps=KAPPA_STEPS)
    with env.run(variant):
        z, nu, lam, _ = f(*prim[:6], kappa=prim[6])
        loss = (z * cots[0]).sum() + (lam * cots[1]).sum() + ((nu * cots[2]).sum() if q else 0.0)
        g = torch.autograd.grad(loss, [x for x in prim if x.nelement()])
        with fwAD.dual_level():
            ins = [fwAD.make_dual(x.detach(), t) if t is not None else x.detach() for x, t in zip(prim, tans)]
            zd, nud, lamd, _ = f(*ins[:6], kappa=ins[6])
            zt, lt = fwAD.unpack_dual(zd).tangent, fwAD.unpack_dual(lamd).tangent
            nt = fwAD.unpack_dual(nud).tangent if q else None
    lhs = float((zt * cots[0]).sum() + (lt * cots[1]).sum() + ((nt * cots[2]).sum() if q else 0.0))
    rhs = float(sum((a * t).sum() for a, t in zip(g, [t for t in tans if t is not None])))
    gap = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    note("adjoint identity %dx%dx%dx%d" % shape, gap)
    assert abs(lhs) > 1e-3 and gap <= 1e-9


# ------------------------------------------------------------------------------------------------ 3. second order
def second_order_check(env, shape, seed, kappa=1e-3, variant=0):
    """grad(..., create_graph=True), then the grad of <W, grads>, against the closed form at the kernel's own centred point"""
    from qpth_amd.qp import QPFunction
    B, n, m, q = shape
    arrs = [np.asarray(a, np.float64) for a in problems.prof_qp(B, n, m, q, seed=seed)]
    v = np.random.RandomState(seed + 50).randn(B, n)
    W = random_W(B, n, m, q, seed + 70)
    tq = on(arrs, env.dev, grad=True)
    params = [x for x in tq if x.nelement()]
    kt = torch.tensor(kappa, dtype=torch.float64, device=env.dev, requires_grad=True)
    with env.run(variant):
        z, nu, lam, sl = QPFunction(verbose=-1, duals=True, kappa_tol=KAPPA_TOL, kappa_steps=KAPPA_STEPS)(*tq, kappa=kt)
        g1 = torch.autograd.grad((z * torch.tensor(v, device=env.dev)).sum(), params + [kt], create_graph=True)
        assert all(x.requires_grad for x in g1[:-1]) and not g1[-1].requires_grad       # dkappa carries no graph
        Wt = [torch.tensor(w, device=env.dev) for w in W if np.size(w)]
        g2 = torch.autograd.grad(sum((a * w).sum() for a, w in zip(g1[:-1], Wt)), params + [kt], allow_unused=True)
    assert g2[-1] is None                                # the second-order gradient with respect to kappa is not offered
    sol = [host(x) for x in (z, lam, sl, nu)]
    ref = second_order(arrs, sol, first_backward(arrs, sol, (v, None, None)), [w if np.size(w) else None for w in W])
    for k, a in zip([k for k in HNAMES if np.size(ref[k])], g2[:-1]):
        gap = rel_err(host(a), ref[k]).max()
        note("%s %dx%dx%dx%d" % ((k,) + shape), gap)
        assert gap <= TOL_B2, k


def kink(env, variant=0):
    """The projection min 1/2 ||z - y||^2 s.t. z <= h with y = h exactly: every row is weakly active, the hard layer's second
    derivative is one-sided there.  At kappa = 1e-2 the Hessian-vector product of <v, zhat> in p equals central differences
    (step 1e-6) of the first gradient taken through the reference, to 1e-5."""
    from qpth_amd.qp import QPFunction
    B, n = 2, 6
    r = np.random.RandomState(4)
    hh = r.randn(B, n)
    arrs = [np.broadcast_to(np.eye(n), (B, n, n)).copy(), -hh, np.broadcast_to(np.eye(n), (B, n, n)).copy(), hh,
            np.zeros(0), np.zeros(0)]
    v, w = r.randn(B, n), r.randn(B, n)
    kappa = 1e-2
    tq = on(arrs, env.dev, grad=True)
    with env.run(variant):
        z = QPFunction(verbose=-1, kappa_tol=KAPPA_TOL, kappa_steps=KAPPA_STEPS)(*tq, kappa=kappa)
        (g,) = torch.autograd.grad((z * torch.tensor(v, device=env.dev)).sum(), tq[1], create_graph=True)
        (hv,) = torch.autograd.grad((g * torch.tensor(w, device=env.dev)).sum(), tq[1])

    def grad_p(p):
        a = [arrs[0], p, arrs[2], arrs[3], arrs[4], arrs[5]]
        return cr.grads(a, cr.centre(a, kappa, B=B)[0], (v, None, None))[0][1]

    step = 1e-6
    fd = (grad_p(arrs[1] + step * w) - grad_p(arrs[1] - step * w)) / (2 * step)
    gap = np.abs(host(hv) - fd).max() / np.abs(fd).max()
    note("kink: HVP vs finite differences", gap)
    assert np.abs(fd).max() > 1e-3 and gap <= 1e-5


# ------------------------------------------------------------------------------------------------ 4. limit, 5. composition
def limit(env, variant=0):
    from qpth_amd.qp import QPFunction
    shape = (2, 12, 9, 3)
    tq = on(problems.prof_qp(*shape, seed=1), env.dev)
    with env.run(variant):
        hard = QPFunction(verbose=-1)(*tq)
        smooth = QPFunction(verbose=-1)(*tq, kappa=1e-8)
    gap = np.abs(host(hard) - host(smooth)).max()
    note("kappa = 1e-8 against the hard QP", gap)
    assert 0 < gap <= 1e-5


def warm_start(env, variant=0):
    import qpth_amd
    from qpth_amd.qp import QPFunction
    shape = (4, 12, 9, 3)
    tq = on(problems.prof_qp(*shape, seed=1), env.dev)
    ws = qpth_amd.WarmStart()
    with env.run(variant):
        cold = QPFunction(verbose=-1)(*tq, kappa=1e-3)
        first = QPFunction(verbose=-1, warm_start=ws)(*tq, kappa=1e-3)
        assert torch.equal(first, cold)                      # the holder was empty
        second = QPFunction(verbose=-1, warm_start=ws)(*tq, kappa=1e-3)
    assert (host(ws.used) == 1).all()
    assert np.abs(host(ws.lam) * host(ws.slacks) / 1e-3 - 1).max() <= 1e-8       # the holder took the CENTRED pair: s lam = kappa
    gap = rel_err(host(second), host(cold)).max()
    note("warm against cold", gap)
    assert gap <= 1e-8


def sensitivity_jacobian(env, variant=0):
    from qpth_amd import sensitivity
    shape = (2, 12, 9, 3)
    B, n, m, q = shape
    arrs, kappa, ref = problem(shape, 1, "rows")
    tq = on(arrs, env.dev)
    with env.run(variant):
        J = sensitivity.solve(*tq, kappa=torch.tensor(kappa, device=env.dev)).jacobian(of=("z",), wrt=("p", "h"))
    Jp, Jh = np.zeros((B, n, n)), np.zeros((B, n, m))
    for i in range(n):
        e = np.zeros((B, n))
        e[:, i] = 1.0
        six = cr.grads(arrs, ref, (e, None, None))[0]
        Jp[:, i], Jh[:, i] = six[1], six[3]
    for nm, a, w in (("J[z,p]", J["z", "p"], Jp), ("J[z,h]", J["z", "h"], Jh)):
        gap = close(host(a), w)
        note(nm, gap)
        assert gap <= TOL_REF


# ------------------------------------------------------------------------------------------------ 6. refusals
def refusals(env, big=(2, 150, 150, 0)):
    import pytest
    from qpth_amd.qp import QPFunction, QPSolvers
    shape = (2, 12, 9, 3)
    B, n, m, q = shape
    arrs = problems.prof_qp(*shape, seed=1)
    tq = on(arrs, env.dev)
    with env.run():
        with pytest.raises(ValueError, match="kappa.*rho"):
            QPFunction(verbose=-1)(*tq, rho=10.0, kappa=1e-3)
        with pytest.raises(ValueError, match="kappa.*float64"):
            QPFunction(verbose=-1)(*[x.float() for x in tq], kappa=1e-3)
        with pytest.raises(ValueError, match="kappa.*refine"):
            QPFunction(verbose=-1, refine=1)(*tq, kappa=1e-3)
        with pytest.raises(ValueError, match="kappa.*PDIPM_BATCHED"):
            QPFunction(verbose=-1, solver=QPSolvers.CVXPY)(*tq, kappa=1e-3)
        with pytest.raises(ValueError, match="kappa.*208"):
            QPFunction(verbose=-1)(*on(problems.prof_qp(*big, seed=0), env.dev), kappa=1e-3)
        with pytest.raises(ValueError, match="kappa has shape"):
            QPFunction(verbose=-1)(*tq, kappa=torch.ones(m + 1, dtype=torch.float64, device=env.dev))
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            kap = torch.full((B, m), 1e-3, dtype=torch.float64, device=env.dev)
            kap[1, 2] = bad                                  # one entry of one QP of the batch
            with pytest.raises(ValueError, match="kappa must be positive"):
                QPFunction(verbose=-1)(*tq, kappa=kap)
        with pytest.raises(ValueError, match="kappa must be positive"):
            QPFunction(verbose=-1)(*tq, kappa=-1e-3)
