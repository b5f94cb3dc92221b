"""Two-sided inequality rows (QPFunction(...)(Q, p, G, h, A, b, lower=l), qpx_ipm_range, qpx_backward_range): the
checks that tests/test_emu_range.py runs on the host-thread emulator and tests/test_gpu_range.py on a real MI355X.  Every
check takes an `env`: env.dev (the torch device) and env.run(variant=0), a context manager around the library calls.

Problems: tests/range_reference.py (seed 53; each shape with every row two-sided and with every second row one-sided).
References: the unmodified reference on the DOUBLED QP [G; -G_F] z <= [h; -lower_F] (tests/golden/range_*.npz, made by
tests/golden/make_golden_range.py), oracle/qp_oracle on the doubled QP for the iteration counts, and the library's own
six-input call where no reference is needed.

Gates: against the reference 1e-6 (float64; the project's gate, README); the one-sided equivalence 1e-12 (the two calls run
the same operations on a one-sided row up to the order in which the step length's minimum is taken); the adjoint identity
1e-9 relative (as tests/soft_checks.py: two solves of one KKT matrix, round-off times its condition).
"""
import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

import range_reference as R
from conftest import load_golden, rel_err

TOL_REF = 1e-6
NAMES = ("dQ", "dp", "dG", "dh", "dA", "db", "dlower")
measured = {}        # check name -> worst figure seen (scripts/bench_range.py writes them to profiles/range.json)


def note(key, value):
    measured[key] = max(float(value), measured.get(key, 0.0))
    print("%-44s %.3e" % (key, value))


def on(arrs, dev):
    return [torch.tensor(np.asarray(x), dtype=torch.float64, device=dev) if np.asarray(x).size
            else torch.empty(0, dtype=torch.float64, device=dev) for x in arrs]


def host(t):
    return t.detach().cpu().numpy()


def close(a, ref, tol=None):
    """the project's gate on gradients: max |a - ref| <= tol max(1, max |ref|); returns the figure that must be <= tol"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(1.0, np.abs(ref).max()) if ref.size else 0.0


def problem(label, sides):
    """the seeded problem and its fixture; the stored vectors pin the generator"""
    arrs = R.range_problem(label, sides)
    g = load_golden(R.fixture_name(label, sides))
    for k, x in zip(("p", "h", "b", "lower"), (arrs[1], arrs[3], arrs[5], arrs[6])):
        assert np.array_equal(x, g[k]), k
    return arrs, g


# ---------------------------------------------------------------- 1. parity with the reference on the doubled QP
ONE_WAVE = 2048      # the A/B knob: one wave per QP in the tile kernels -- what the default dispatch picks at four tile rows beyond 512 QPs


def check_reference_parity(env, label, sides, variant=0):
    from qpth_amd.kkt import KKTFactors
    from qpth_amd.qp import QPFunction
    arrs, g = problem(label, sides)
    B, n, m, q = R.SHAPES[label]
    tq = on(arrs, env.dev)
    for t in tq:
        if t.nelement():
            t.requires_grad_(True)
    with env.run(variant):
        z = QPFunction(verbose=-1)(*tq[:6], lower=tq[6])
        (z * torch.tensor(g["c"], device=env.dev)).sum().backward()
        # the multipliers are no outputs of the node: the same launch once more, from the factors
        with torch.no_grad():
            fac = KKTFactors.build(tq[0], tq[2], tq[4], B)
            res = fac.ipm_range(tq[1], tq[3], tq[6], tq[5])
    assert np.array_equal(host(res.zhat), host(z))
    fin = np.isfinite(g["slacks_lo"])
    assert np.array_equal(np.isfinite(host(res.slacks_lo)), fin) and np.all(host(res.lam_lo)[~fin] == 0.0)
    fig = {"zhat": rel_err(host(z), g["zhat"]).max(), "lam": rel_err(host(res.lam), g["lam"]).max(),
           "lam_lo": rel_err(host(res.lam_lo), g["lam_lo"]).max(), "slacks": close(host(res.slacks), g["slacks"]),
           "slacks_lo": close(np.where(fin, host(res.slacks_lo), 0.0), np.where(fin, g["slacks_lo"], 0.0))}
    if q:
        fig["nu"] = rel_err(host(res.nu), g["nu"]).max()
    for k, t in zip(NAMES, tq):
        if t.nelement():
            fig[k] = close(host(t.grad), g[k])
    assert np.all(host(tq[6].grad)[~fin] == 0.0)                      # one-sided rows: exactly zero
    for k, v in fig.items():
        note("parity/%s%s/%s/%s" % (label, "-1w" if variant else "", sides, k), v)
    assert max(fig.values()) <= TOL_REF, fig


# ---------------------------------------------------------------- 2. iteration counts; the stop rule's || G^T e ||
def oracle_doubled(arrs, i, eps, want_trace=False, maxIter=20):
    from oracle import qp_oracle as orc
    Q, p, G, h, A, b, lower = arrs
    q = np.shape(A)[1] if np.size(A) else 0
    G2, h2, F = R.double(G[i], h[i], lower[i])
    # (one thread: a QP of this size is microseconds of work, and the default pool is sized by the machine's CPU count)
    o = orc.OracleQP(Q[i:i + 1], p[i:i + 1], G2[None], h2[None], A[i:i + 1] if q else None, b[i:i + 1] if q else None, nthreads=1)
    return o.forward(eps, maxIter, 3, True, 1, want_trace=want_trace)


def check_iteration_counts(env, label, sides, variant=0):
    """eps = 1e-8, the reference's stall counter: the counts of oracle/qp_oracle on the doubled QP, each QP alone"""
    from qpth_amd.kkt import KKTFactors
    arrs = R.range_problem(label, sides)
    B = R.SHAPES[label][0]
    tq = on(arrs, env.dev)
    with env.run(variant):
        fac = KKTFactors.build(tq[0], tq[2], tq[4], B)
        res = fac.ipm_range(tq[1], tq[3], tq[6], tq[5], eps=1e-8, stall_policy=1)
    mine = host(res.iters)
    ref = np.array([oracle_doubled(arrs, i, 1e-8)[4]["iters"][0] for i in range(B)])
    print("iters range", mine, "doubled", ref)
    assert np.array_equal(mine, ref)


def check_trace_dual_resid(env, label="t1b"):
    """a mixed fixture: the trace's dual_resid = tau sigma_z || G^T e || is the doubled QP's tau sigma_z || G'^T 1 ||, and not 0"""
    from qpth_amd.kkt import KKTFactors
    arrs = R.range_problem(label, "half")
    B = R.SHAPES[label][0]
    tq = on(arrs, env.dev)
    with env.run():
        fac = KKTFactors.build(tq[0], tq[2], tq[4], B)
        res = fac.ipm_range(tq[1], tq[3], tq[6], tq[5], eps=1e-8, stall_policy=1, want_trace=True)
    tr, it = host(res.trace), host(res.iters)
    worst, top = 0.0, 0.0
    for i in range(B):
        info = oracle_doubled(arrs, i, 1e-8, want_trace=True)[4]
        assert it[i] == info["iters"][0]
        mine, ref = tr[:it[i], i], info["trace"][:it[i]]
        worst = max(worst, (np.abs(mine - ref) / np.maximum(1.0, np.abs(ref))).max())
        top = max(top, ref[:, 1].max())
    note("trace/" + label, worst)
    assert top > 1e-3, top                       # the shift of the start point is there: || G^T e || takes part
    assert worst <= TOL_REF


def check_iterates_after_k(env, label, sides="half", ks=(2, 5)):
    """the range role's PATH: capped at k iterations (eps = 1e-12, the reference's stall counter) its best iterate is the one
    oracle/qp_oracle reaches on the doubled QP under the same cap, each QP alone -- zhat, both rows' multipliers and slacks,
    nu as max |a - ref| / max(1, max |ref|), and the same `iters`.  A loop with another direction, centring or step length
    than the reference's reaches the same optimum by another path: tests/loop_checks.py, check 1, for this role."""
    from qpth_amd.kkt import KKTFactors
    arrs = R.range_problem(label, sides)
    B, n, m, q = R.SHAPES[label]
    tq = on(arrs, env.dev)
    worst = 0.0
    with env.run():
        fac = KKTFactors.build(tq[0], tq[2], tq[4], B)
        for k in ks:
            res = fac.ipm_range(tq[1], tq[3], tq[6], tq[5], eps=1e-12, maxIter=k, stall_policy=1)
            it = host(res.iters)
            for i in range(B):
                x, y, z2, s2, info = oracle_doubled(arrs, i, 1e-12, maxIter=k)
                assert it[i] == info["iters"][0], (k, i, it, info["iters"])
                F = np.flatnonzero(np.isfinite(arrs[6][i]))
                lam, lam_lo = R.split(z2[0], F, m, 0.0)
                s, s_lo = R.split(s2[0], F, m, np.inf)
                fin = np.isfinite(s_lo)
                mine_lo = host(res.slacks_lo)[i]
                assert np.array_equal(np.isfinite(mine_lo), fin)
                fig = [close(host(res.zhat)[i], x[0]), close(host(res.lam)[i], lam), close(host(res.lam_lo)[i], lam_lo),
                       close(host(res.slacks)[i], s), close(np.where(fin, mine_lo, 0.0), np.where(fin, s_lo, 0.0))]
                if q:
                    fig.append(close(host(res.nu)[i], y[0]))
                worst = max([worst] + fig)
    note("iterates/%s/%s" % (label, sides), worst)
    assert worst <= TOL_REF, worst


# ---------------------------------------------------------------- 3. lower = -inf everywhere is the six-input call
def check_one_sided_equivalence(env, label, variant=0):
    from qpth_amd.kkt import KKTFactors
    from qpth_amd.qp import QPFunction
    arrs = R.range_problem(label, "all")
    B, n, m, q = R.SHAPES[label]
    c = torch.tensor(R.loss_vector(label), device=env.dev)
    outs = []
    for ranged in (False, True):
        tq = on(arrs, env.dev)
        tq[6] = torch.full_like(tq[6], -float("inf"))
        for t in tq:
            if t.nelement():
                t.requires_grad_(True)
        with env.run(variant):
            z = QPFunction(verbose=-1)(*tq[:6], **({"lower": tq[6]} if ranged else {}))
            (z * c).sum().backward()
            with torch.no_grad():
                fac = KKTFactors.build(tq[0], tq[2], tq[4], B)
                res = fac.ipm_range(tq[1], tq[3], tq[6], tq[5]) if ranged else fac.ipm(tq[1], tq[3], tq[5])
        outs.append((host(res.iters), [host(z)] + [host(t.grad) for t in tq[:6] if t.nelement()] + [host(res.lam), host(res.slacks)]))
        if ranged:
            assert np.all(host(tq[6].grad) == 0.0)
            assert np.all(host(res.lam_lo) == 0.0) and np.all(np.isposinf(host(res.slacks_lo)))
    assert np.array_equal(outs[0][0], outs[1][0]), (outs[0][0], outs[1][0])
    worst = max(close(a, r) for a, r in zip(outs[1][1], outs[0][1]))
    note("one_sided/" + label + ("-1w" if variant else ""), worst)
    assert worst <= 1e-12


# ---------------------------------------------------------------- 3b. the library's own doubled call (shapes without a fixture)
SLOT_SHAPES = {          # the slot counts no fixture reaches: nz > 64 or > 128 beside few rows -- (n, m, q) -> the loop form
    "s12": (130, 9, 0),      # one tile row, four slots
    "s22": (100, 20, 30),    # two tile rows, two slots
    "s44": (130, 60, 10),    # four-row chain form, four slots
    "s74": (130, 70, 5),     # seven-row chain form, four slots
    "s11b": (70, 12, 0),     # one tile row, two slots
    "s24": (130, 20, 0),     # two tile rows, four slots
}


def check_doubled_call(env, key, sides="half", variant=0):
    """range call against the library's six-input call on the doubled QP, each QP alone: zhat and the seven gradients folded
    back, at the project's gate (two paths of the library, whichever family serves the doubled QP)"""
    from qpth_amd.qp import QPFunction
    n, m, q = SLOT_SHAPES[key]
    B = 2
    r = np.random.RandomState(61)
    L = r.randn(B, n, n)
    Q = np.matmul(L, L.transpose((0, 2, 1))) / n + np.eye(n)
    G, z0, p, A = r.randn(B, m, n), r.randn(B, n), r.randn(B, n), r.randn(B, q, n)
    gz = np.einsum("bmn,bn->bm", G, z0)
    h, lower = gz + 0.05 + 0.5 * r.rand(B, m), gz - 0.05 - 0.5 * r.rand(B, m)
    b = np.einsum("bqn,bn->bq", A, z0)
    if sides == "half":
        lower[:, 1::2] = -np.inf
    c = r.randn(B, n)
    tq = on((Q, p, G, h, A if q else np.zeros(0), b if q else np.zeros(0), lower), env.dev)
    for t in tq:
        if t.nelement():
            t.requires_grad_(True)
    with env.run(variant):
        z = QPFunction(verbose=-1)(*tq[:6], lower=tq[6])
        (z * torch.tensor(c, device=env.dev)).sum().backward()
    worst = 0.0
    for i in range(B):
        G2, h2, F = R.double(G[i], h[i], lower[i])
        t2 = on((Q[i], p[i], G2, h2, A[i] if q else np.zeros(0), b[i] if q else np.zeros(0)), env.dev)
        for t in t2:
            if t.nelement():
                t.requires_grad_(True)
        with env.run():
            z2 = QPFunction(verbose=-1)(*t2)
            (z2 * torch.tensor(c[i:i + 1], device=env.dev)).sum().backward()
        dG, dh, dlo = R.fold(host(t2[2].grad), host(t2[3].grad), F, m)
        ref = [host(z2)[0], host(t2[0].grad), host(t2[1].grad), dG, dh, dlo] + ([host(t2[4].grad), host(t2[5].grad)] if q else [])
        mine = [host(z)[i]] + [host(tq[k].grad)[i] for k in (0, 1, 2, 3, 6)] + ([host(tq[4].grad)[i], host(tq[5].grad)[i]] if q else [])
        worst = max([worst] + [close(a, x) for a, x in zip(mine, ref)])
    note("doubled_call/%s/%s" % (key, sides), worst)
    assert worst <= TOL_REF


# ---------------------------------------------------------------- 4. the closed form of the box
def check_closed_form(env):
    """Q = I, G = I, no equalities: zhat = clip(-p, l, u), lam_u = max(0, -p - u), lam_l = max(0, l + p)"""
    from qpth_amd.kkt import KKTFactors
    B, n = 3, 12
    r = np.random.RandomState(7)
    p = 2.0 * r.randn(B, n)
    lo = -0.2 - r.rand(B, n)
    up = 0.2 + r.rand(B, n)
    eye = np.eye(n)
    Q, pt, G, h, lower = on((eye, p, eye, up, lo), env.dev)
    with env.run():
        fac = KKTFactors.build(Q, G, None, B)
        res = fac.ipm_range(pt, h, lower, None)
    z, lu, ll = R.box_closed_form(p, lo, up)
    assert (lu > 0.1).any() and (ll > 0.1).any() and ((lu == 0) & (ll == 0)).any()
    fig = {"zhat": close(host(res.zhat), z), "lam": close(host(res.lam), lu), "lam_lo": close(host(res.lam_lo), ll)}
    for k, v in fig.items():
        note("closed_form/" + k, v)
    assert max(fig.values()) <= TOL_REF, fig


# ---------------------------------------------------------------- 5. gradcheck, adjointness, reductions
def small_problem(dev):
    """(6, 4, 2), away from kinks: strictly active or strictly inactive rows (asserted)"""
    B, n, m, q = 2, 6, 4, 2
    r = np.random.RandomState(11)
    L = r.randn(B, n, n) / np.sqrt(n)
    G, z0, A = r.randn(B, m, n), r.randn(B, n), r.randn(B, q, n)
    gz = np.einsum("bmn,bn->bm", G, z0)
    h = gz + 0.1 + 0.4 * r.rand(B, m)
    lower = gz - 0.1 - 0.4 * r.rand(B, m)
    return on((L, 2.0 * r.randn(B, n), G, h, A, np.einsum("bqn,bn->bq", A, z0), lower), dev)


def check_gradcheck(env):
    """torch.autograd.gradcheck over all seven inputs in reverse mode (Q = L L' + I through L, as tests/soft_checks.py).
    eps = 1e-6; atol 1e-5 covers the central difference's noise, the solution's ~1e-11 over 2 eps, rtol 1e-3 its truncation."""
    from qpth_amd.kkt import KKTFactors
    from qpth_amd.qp import QPFunction
    ins = small_problem(env.dev)
    eye = torch.eye(6, dtype=torch.float64, device=env.dev)
    with env.run():
        fac = KKTFactors.build(ins[0] @ ins[0].transpose(-1, -2) + eye, ins[2], ins[4], 2)
        res = fac.ipm_range(ins[1], ins[3], ins[6], ins[5])
    lu, ll, su, sl = host(res.lam), host(res.lam_lo), host(res.slacks), host(res.slacks_lo)
    assert np.all(np.maximum(lu, su) > 1e-2) and np.all(np.maximum(ll, sl) > 1e-2)          # no kink nearby
    assert (lu > 1e-2).any() and (ll > 1e-2).any()
    for t in ins:
        t.requires_grad_(True)

    def f(L, p, G, h, A, b, lower):
        return QPFunction(verbose=-1)(L @ L.transpose(-1, -2) + eye, p, G, h, A, b, lower=lower)

    with env.run():
        assert torch.autograd.gradcheck(f, ins, eps=1e-6, atol=1e-5, rtol=1e-3, check_forward_ad=False)


def check_adjoint_identity(env, label="t1b", sides="half"):
    """per QP: <v, z'> = sum over the seven inputs of <grad, tangent>, z' from the library's FORWARD mode on the doubled QP
    along the doubled tangents (tG' = [tG; -tG_F], th' = [th; -tlower_F]) -- the range role itself has no forward mode"""
    from qpth_amd.qp import QPFunction
    arrs = R.range_problem(label, sides)
    B, n, m, q = R.SHAPES[label]
    r = np.random.RandomState(9)
    tans = [r.randn(*np.shape(x)) for x in arrs]
    tans[0] = 0.5 * (tans[0] + np.swapaxes(tans[0], -1, -2))
    tans[6] = np.where(np.isfinite(arrs[6]), tans[6], 0.0)
    v = r.randn(B, n)
    tq = on(arrs, env.dev)
    for t in tq:
        t.requires_grad_(True)
    with env.run():
        z = QPFunction(verbose=-1)(*tq[:6], lower=tq[6])
        (z * torch.tensor(v, device=env.dev)).sum().backward()
    rhs = np.stack([(host(t.grad) * tn).reshape(B, -1).sum(1) for t, tn in zip(tq, tans)])
    lhs = np.zeros(B)
    for i in range(B):
        G2, h2, F = R.double(arrs[2][i], arrs[3][i], arrs[6][i])
        tG2 = np.concatenate([tans[2][i], -tans[2][i][F]])
        th2 = np.concatenate([tans[3][i], -tans[6][i][F]])
        prim = on((arrs[0][i], arrs[1][i], G2, h2, arrs[4][i], arrs[5][i]), env.dev)
        tang = on((tans[0][i], tans[1][i], tG2, th2, tans[4][i], tans[5][i]), env.dev)
        with env.run(), fwAD.dual_level():
            out = QPFunction(verbose=-1)(*[fwAD.make_dual(x, t) for x, t in zip(prim, tang)])
            lhs[i] = float((fwAD.unpack_dual(out).tangent.cpu().numpy().reshape(-1) * v[i]).sum())
    gap = np.abs(lhs - rhs.sum(0)) / (np.abs(lhs) + np.abs(rhs).sum(0))
    note("adjoint_gap", gap.max())
    assert np.abs(rhs[6]).min() > 0                                     # the lower term takes part
    assert gap.max() <= 1e-9, gap


def check_lower_reductions(env):
    """a lower the batch shares: the `.mean(0)` of the per-QP gradient, and the same solution"""
    from qpth_amd.qp import QPFunction
    L, p, G, h, A, b, lower = small_problem(env.dev)
    Q = L @ L.transpose(-1, -2) + torch.eye(6, dtype=torch.float64, device=env.dev)
    c = torch.tensor(np.random.RandomState(4).randn(2, 6), device=env.dev)
    vec = torch.minimum(lower[0], lower[1])                              # below both QPs' h

    def grad_of(lo, Gm=G):
        lo = lo.clone().requires_grad_(True)
        with env.run():
            z = QPFunction(verbose=-1)(Q, p, Gm, h, A, b, lower=lo)
            (z * c).sum().backward()
        return host(z), host(lo.grad)

    z1, g_pq = grad_of(vec.expand(2, -1).contiguous())
    z2, g_sh = grad_of(vec)
    assert np.array_equal(z1, z2) and g_sh.shape == (4,)
    assert close(g_sh, g_pq.mean(0)) <= 1e-12
    # G shared as well: || G^T e || is formed once for the batch
    half = vec.clone()
    half[1::2] = -float("inf")
    z3, g3 = grad_of(half.expand(2, -1).contiguous(), G[0].expand(2, -1, -1).contiguous())
    z4, g4 = grad_of(half, G[0])
    assert close(z4, z3) <= 1e-12 and close(g4, g3.mean(0)) <= 1e-12
    assert np.all(g4[1::2] == 0.0)


# ---------------------------------------------------------------- 6. status and refusals
def check_abi_codes(env):
    """QPX_ERR_* of the two entry points and qpx_range_supported, no launch"""
    from qpth_amd import _lib
    with env.run():
        dll = _lib.backend_for(torch.empty(0, device=env.dev)).dll
        for (n, m, q) in [R.SHAPES[k][1:] for k in R.SHAPES]:
            assert dll.qpx_range_supported(_lib.QPX_F64, n, m, q) == 1
            assert dll.qpx_range_supported(_lib.QPX_F32, n, m, q) == 0
            assert dll.qpx_range_supported(_lib.QPX_F32_WIDE, n, m, q) == 0
        assert dll.qpx_range_supported(_lib.QPX_F64, 100, 100, 10) == 0          # the large-QP family
        assert dll.qpx_range_supported(_lib.QPX_F64, 100, 200, 0) == 0           # the doubled box itself
        assert dll.qpx_range_supported(_lib.QPX_F64, 0, 4, 0) == 0
        one = torch.zeros(512, dtype=torch.float64, device=env.dev)
        i32 = torch.zeros(8, dtype=torch.int32, device=env.dev)
        P = one.data_ptr()

        def ipm(dtype, n, m, q, lower=P, lam_lo=P):
            return dll.qpx_ipm_range(dtype, 1, n, m, q, P, 0, P, 0, P, 0, P, 0, 1e-8, 20, 3, 1, P, P, P, P, i32.data_ptr(),
                                     i32.data_ptr(), P, None, lower, 0, None, lam_lo, P, None)

        def bwd(dtype, n, m, q, refine=0, lam_lo=P):
            return dll.qpx_backward_range(dtype, 1, n, m, q, P, 0, P, P, P, P, P, None, P, None, None, None, None, None, None,
                                          None, refine, None, 0, None, 0, None, 0, i32.data_ptr(), lam_lo, P, None)

        assert ipm(_lib.QPX_F32, 6, 4, 2) == -2 and bwd(_lib.QPX_F32, 6, 4, 2) == -2                    # QPX_ERR_UNSUPPORTED
        assert ipm(_lib.QPX_F32_WIDE, 6, 4, 2) == -2 and bwd(_lib.QPX_F32_WIDE, 6, 4, 2) == -2
        assert ipm(_lib.QPX_F64, 100, 100, 10) == -2 and bwd(_lib.QPX_F64, 100, 100, 10) == -2
        assert bwd(_lib.QPX_F64, 6, 4, 2, refine=1) == -2
        assert ipm(_lib.QPX_F64, 6, 4, 2, lower=None) == -1 and ipm(_lib.QPX_F64, 6, 4, 2, lam_lo=None) == -1   # QPX_ERR_ARG
        assert bwd(_lib.QPX_F64, 6, 4, 2, lam_lo=None) == -1 and bwd(_lib.QPX_F64, 6, 4, 2, refine=-1) == -1
        assert ipm(7, 6, 4, 2) == -1 and ipm(_lib.QPX_F64, 6, 0, 2) == -1
        # the A/B knob: a form without the role declines
        old = dll.qpx_set_ipm_variant(256)                                       # the 16x16 thread grid at every size
        try:
            assert dll.qpx_range_supported(_lib.QPX_F64, 6, 4, 2) == 0 and ipm(_lib.QPX_F64, 6, 4, 2) == -2
        finally:
            dll.qpx_set_ipm_variant(old)


def check_bad_lower(env, pytest):
    from qpth_amd.kkt import KKTFactors
    from qpth_amd.qp import QPFunction
    arrs = R.range_problem("t1b", "half")
    tq = on(arrs, env.dev)
    six, lower, h = tq[:6], tq[6], tq[3]
    with env.run():
        for bad in (float("nan"), float("inf"), float(h[1, 4]), float(h[1, 4]) + 1.0):
            lo = lower.clone()
            lo[1, 4] = bad
            with pytest.raises(ValueError, match="lower must be below h"):
                QPFunction(verbose=-1)(*six, lower=lo)
        # the QP is left as the `Q not SPD` path leaves one; its neighbour is solved
        lo = lower.clone()
        lo[1, 4] = float("nan")
        fac = KKTFactors.build(tq[0], tq[2], tq[4], 2)
        res = fac.ipm_range(tq[1], h, lo, tq[5])
        good = fac.ipm_range(tq[1], h, lower, tq[5])
    from qpth_amd import _lib
    st = host(res.status)
    assert st[1] & _lib.ST_NONFINITE and not st[0] & _lib.ST_NONFINITE
    assert host(res.iters)[1] == 0 and np.isposinf(host(res.best_resid)[1])
    for x in (res.zhat, res.nu, res.lam, res.slacks, res.lam_lo, res.slacks_lo):
        assert np.isnan(host(x)[1]).all()
    assert np.array_equal(host(res.zhat)[0], host(good.zhat)[0])
    # the bit stays with the launch that met it: a good launch on the same factors raises nothing, nor does one that is
    # asked for 0 iterations, and the factors' own status words never saw it
    with env.run():
        fac.raise_on_failure()
        fac.ipm_range(tq[1], h, lower, tq[5], maxIter=0)
        fac.raise_on_failure()
        fac.ipm_range(tq[1], h, lo, tq[5])
        with pytest.raises(ValueError, match="lower must be below h"):
            fac.raise_on_failure()
    assert not (host(fac.status) & _lib.ST_NONFINITE).any()


def check_refusals(env, pytest):
    from qpth_amd import WarmStart
    from qpth_amd.qp import QPFunction, QPSolvers
    arrs = R.range_problem("t1b", "half")
    tq = on(arrs, env.dev)
    six, lower = tq[:6], tq[6]
    way_out = r"\[G; -G\] z <= \[h; -lower\]"
    with env.run():
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1)(*[t.float() for t in six], lower=lower.float())
        big = on(R.range_problem("box", "all"), env.dev)
        A = torch.zeros(2, 10, 100, dtype=torch.float64, device=env.dev)
        with pytest.raises(ValueError, match=way_out):                     # nz + neq + nineq = 210: the large-QP family
            QPFunction(verbose=-1)(big[0], big[1], big[2], big[3], A, A[:, :, 0], lower=big[6])
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1)(*six, 2.5, lower=lower)
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1)(*six, kappa=1e-3, lower=lower)
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1, refine=1)(*six, lower=lower)
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1, duals=True)(*six, lower=lower)
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1, warm_start=WarmStart())(*six, lower=lower)
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1, solver=QPSolvers.CVXPY)(*six, lower=lower)
        with pytest.raises(ValueError, match="shape"):
            QPFunction(verbose=-1)(*six, lower=lower[:, :-1])
        with pytest.raises(ValueError, match="shape"):
            QPFunction(verbose=-1)(*six, lower=lower[:1].expand(3, -1))
        # forward mode and a second grad
        with pytest.raises(RuntimeError), fwAD.dual_level():
            QPFunction(verbose=-1)(*six[:1], fwAD.make_dual(six[1], torch.ones_like(six[1])), *six[2:], lower=lower)
        ins = [t.clone().requires_grad_(True) for t in tq]
        z = QPFunction(verbose=-1)(*ins[:6], lower=ins[6])
        (gp,) = torch.autograd.grad(z.sum(), ins[1], create_graph=True)
        with pytest.raises(RuntimeError):
            torch.autograd.grad(gp.sum(), ins[3])


def check_lower_none_is_the_six_input_call(env):
    from qpth_amd.qp import QPFunction
    arrs = R.range_problem("t1b", "all")[:6]
    outs = []
    for extra in ({}, {"lower": None}):
        tq = on(arrs, env.dev)
        for t in tq:
            t.requires_grad_(True)
        with env.run():
            z = QPFunction(verbose=-1)(*tq, **extra)
            assert type(z.grad_fn).__name__.startswith("QPFunctionFn")
            z.backward(torch.ones_like(z))
        outs.append([host(z)] + [host(t.grad) for t in tq])
    for a, c in zip(*outs):
        assert np.array_equal(a, c)
