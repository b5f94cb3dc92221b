"""Soft two-sided inequality rows (QPFunction(...)(Q, p, G, h, A, b, soft_range=SoftRange(...)), qpx_ipm_soft_range):
the checks that tests/test_emu_soft_range.py runs on the host-thread emulator and tests/test_gpu_soft_range.py on a real MI355X.
Every check takes an `env`: env.dev (the torch device) and env.run(variant=0), a context manager around the library calls.

Problems: tests/soft_range_reference.py (each shape with every row soft on both sides and with the four row kinds mixed).
References: the unmodified reference on the AUGMENTED QP in (z, tu, tl) (tests/golden/softrange_*.npz, made by
tests/golden/make_golden_soft_range.py), oracle/qp_oracle on the augmented QP for the iteration counts and the trace, and the
library's own `lower=`, `rho, l1=`, six-input and augmented dense calls where no reference is needed.

Gates: against the reference 1e-6 (float64; the project's gate, README); the reductions to the existing roles 1e-12 (a row
whose kind is an existing role's runs that role's operations, up to the order in which a step length's maximum and a sum
over the rows are taken); the exact penalty 1e-8 on t (tests/elastic_checks.py: check_exactness).
"""
import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

import elastic_reference as ER
import problems
import range_reference as RR
import soft_range_reference as R
from conftest import load_golden, rel_err

TOL_REF = 1e-6
NAMES = ("dQ", "dp", "dG", "dh", "dA", "db", "dlower", "dgamma_u", "drho_u", "dgamma_l", "drho_l")
PAIRS = (("lam", "slacks"), ("lam_lo", "slacks_lo"), ("lam_t", "slacks_t"), ("lam_tl", "slacks_tl"))
INF = float("inf")
measured = {}        # check name -> worst figure seen (scripts/bench_soft_range.py writes them to profiles/soft_range.json)


def note(key, value):
    measured[key] = max(float(value), measured.get(key, 0.0))
    print("%-48s %.3e" % (key, value))


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


def holder(fields):
    from qpth_amd import SoftRange
    return SoftRange(*fields)


def problem(label, kind):
    """the seeded problem and its fixture; the stored vectors pin the generator"""
    arrs = R.soft_range_problem(label, kind)
    g = load_golden(R.fixture_name(label, kind))
    for k, x in zip(("p", "h", "b") + R.FIELDS, (arrs[1], arrs[3], arrs[5]) + arrs[6:]):
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
        z = QPFunction(verbose=-1)(*tq[:6], soft_range=holder(tq[6:]))
        (z * torch.tensor(g["c"], device=env.dev)).sum().backward()
        # the multipliers, slacks and violations are no outputs of the node: the same launch once more, from the factors
        with torch.no_grad():
            fac = KKTFactors.build(tq[0], tq[2], tq[4], B)
            res = fac.ipm_soft_range(tq[1], tq[3], *tq[6:], tq[5])
    assert np.array_equal(host(res.zhat), host(z))
    fig = {"zhat": rel_err(host(z), g["zhat"]).max(), "t": close(host(res.t), g["t"]), "t_lo": close(host(res.t_lo), g["t_lo"])}
    if q:
        fig["nu"] = rel_err(host(res.nu), g["nu"]).max()
    live = {}
    for lk, sk in PAIRS:
        fin = live[lk] = np.isfinite(g[sk])
        mine_l, mine_s = host(getattr(res, lk)), host(getattr(res, "slacks" + lk[3:]))
        # an absent side reads 0 / +inf (and t = 0 below)
        assert np.array_equal(np.isfinite(mine_s), fin) and np.all(mine_l[~fin] == 0.0), lk
        fig[lk] = rel_err(mine_l, g[lk]).max()
        fig[sk] = close(np.where(fin, mine_s, 0.0), np.where(fin, g[sk], 0.0))
    assert np.all(host(res.t)[~live["lam_t"]] == 0.0) and np.all(host(res.t_lo)[~live["lam_tl"]] == 0.0)
    for k, t in zip(NAMES, tq):
        if t.nelement():
            fig[k] = close(host(t.grad), g[k])
    # the gradients are exactly 0 on an absent or hard side
    assert np.all(host(tq[6].grad)[~live["lam_lo"]] == 0.0)
    assert np.all(host(tq[7].grad)[~live["lam_t"]] == 0.0) and np.all(host(tq[8].grad)[~live["lam_t"]] == 0.0)
    assert np.all(host(tq[9].grad)[~live["lam_tl"]] == 0.0) and np.all(host(tq[10].grad)[~live["lam_tl"]] == 0.0)
    for k, v in fig.items():
        note("parity/%s%s/%s/%s" % (label, "-1w" if variant else "", kind, k), v)
    assert max(fig.values()) <= TOL_REF, fig


# ---------------------------------------------------------------- 2. iteration counts and the trace of the augmented QP
def augmented(arrs, i):
    q = np.shape(arrs[4])[1] if np.size(arrs[4]) else 0
    out = R.augment(arrs[0][i], arrs[1][i], arrs[2][i], arrs[3][i], arrs[4][i] if q else np.zeros(0), *[x[i] for x in arrs[6:]])
    return out + (arrs[5][i] if q else np.zeros(0),)


def oracle_augmented(arrs, i, eps, want_trace=False):
    from oracle import qp_oracle as orc
    Q2, p2, G2, h2, A2, sets, b = augmented(arrs, i)
    q = b.size
    # (one thread: a QP of this size is little work, and the default pool is sized by the machine's CPU count)
    o = orc.OracleQP(Q2[None], p2[None], G2[None], h2[None], A2[None] if q else None, b[None] if q else None, nthreads=1)
    return o.forward(eps, 20, 3, True, 1, want_trace=want_trace)[4]


def check_iteration_counts(env, label, kind, variant=0, gated=True):
    """eps = 1e-8, the reference's stall counter: the counts of oracle/qp_oracle on the augmented QP, each QP alone (gated at
    the shapes of R.COUNTED, printed elsewhere)"""
    from qpth_amd.kkt import KKTFactors
    arrs = R.soft_range_problem(label, kind)
    B = R.SHAPES[label][0]
    tq = on(arrs, env.dev)
    with env.run(variant):
        fac = KKTFactors.build(tq[0], tq[2], tq[4], B)
        res = fac.ipm_soft_range(tq[1], tq[3], *tq[6:], tq[5], eps=1e-8, stall_policy=1)
    mine = host(res.iters)
    ref = np.array([oracle_augmented(arrs, i, 1e-8)["iters"][0] for i in range(B)])
    print("iters %s/%s soft range" % (label, kind), mine, "augmented", ref)
    note("iters_gap/%s%s/%s" % (label, "-1w" if variant else "", kind), np.abs(mine - ref).max())
    if gated:
        assert np.array_equal(mine, ref)


# nz' + neq + m' <= 208 of the augmented QP: 32, 60, 167, 194 -- the largest of each shape that qualifies, on both devices
TRACED = (("t1a", "all"), ("t1b", "mixed"), ("t2", "all"), ("t4", "mixed"))
# the other kind of the three shapes where both kinds qualify (t4/all is 264; check_trace asserts the order): on the emulator
TRACED_OTHER_KIND = (("t1a", "mixed"), ("t1b", "all"), ("t2", "mixed"))


def check_trace(env, label, kind):
    """the trace (pri_resid, dual_resid, mu per iteration) is the oracle's on the augmented QP, each QP alone: this pins
    || G'^T 1 || (the dual residual's norm) and the number of live pairs (mu's divisor)"""
    from qpth_amd.kkt import KKTFactors
    arrs = R.soft_range_problem(label, kind)
    B = R.SHAPES[label][0]
    tq = on(arrs, env.dev)
    with env.run():
        fac = KKTFactors.build(tq[0], tq[2], tq[4], B)
        res = fac.ipm_soft_range(tq[1], tq[3], *tq[6:], tq[5], eps=1e-8, stall_policy=1, want_trace=True)
    tr, it = host(res.trace), host(res.iters)
    worst, top = 0.0, 0.0
    for i in range(B):
        aug = augmented(arrs, i)
        assert aug[0].shape[0] + aug[2].shape[0] + aug[6].size <= 208
        info = oracle_augmented(arrs, i, 1e-8, want_trace=True)
        assert it[i] == info["iters"][0], (it[i], info["iters"])
        mine, ref = tr[:it[i], i], info["trace"][:it[i]]
        worst = max(worst, (np.abs(mine - ref) / np.maximum(1.0, np.abs(ref))).max())
        top = max(top, ref[:, 1].max())
    note("trace/%s/%s" % (label, kind), worst)
    assert top > 1e-3, top                       # the shift of the start point is there: || G'^T 1 || takes part
    assert worst <= TOL_REF


# ---------------------------------------------------------------- 3. reductions to the existing roles
TOL_ROLE = 1e-12
RANGE_LABEL = {"t1b": "t1b", "c4": "c4", "c7": "box"}        # the range role's fixture problems of the same shapes


def _run(env, call, tq, c, variant=0):
    with env.run(variant):
        z = call(tq)
        (z * c).sum().backward()
    return host(z)


HARD_BY_L1 = (INF, 2.0, INF, 2.0)            # (l1, rho, l1_lower, rho_lower): a side is hard by either of its penalties
HARD_BY_RHO = (0.7, INF, 0.4, INF)           # a finite l1 beside rho = +inf: the kernel, the stop rule's || G'^T 1 || and the
                                             # backward's rho each decide it from both fields


def check_hard_sides_are_the_range_call(env, label, variant=0, penalties=HARD_BY_L1):
    """l1 = +inf (or rho = +inf beside a finite l1) on both sides: the `lower=` call (about half of the rows one-sided) --
    zhat and its seven gradients"""
    from qpth_amd.qp import QPFunction
    arrs = RR.range_problem(RANGE_LABEL[label], "half")
    B, n, m, q = R.SHAPES[label]
    c = torch.tensor(R.loss_vector(label), device=env.dev)
    a = with_grad(on(arrs, env.dev))
    za = _run(env, lambda t: QPFunction(verbose=-1)(*t[:6], lower=t[6]), a, c, variant)
    s = with_grad(on(arrs, env.dev))
    pen = [torch.full((B, m), v, dtype=torch.float64, device=env.dev, requires_grad=True) for v in penalties]
    zs = _run(env, lambda t: QPFunction(verbose=-1)(*t[:6], soft_range=holder([t[6]] + pen)), s, c, variant)
    assert all(np.all(host(x.grad) == 0.0) for x in pen)
    worst = max([close(zs, za)] + [close(host(x.grad), host(y.grad)) for x, y in zip(s, a) if x.nelement()])
    note("reduces_to_range%s/%s%s" % ("" if penalties is HARD_BY_L1 else "_by_rho", label, "-1w" if variant else ""), worst)
    assert worst <= TOL_ROLE


def check_no_lower_is_the_elastic_call(env, label, variant=0):
    """lower = -inf everywhere: the `rho, l1=` call (every second row hard) -- zhat and its eight gradients"""
    from qpth_amd.qp import QPFunction
    arrs = ER.elastic_problem(label, "half")
    B, n, m, q = R.SHAPES[label]
    c = torch.tensor(R.loss_vector(label), device=env.dev)
    a = with_grad(on(arrs, env.dev))
    za = _run(env, lambda t: QPFunction(verbose=-1)(*t[:7], l1=t[7]), a, c, variant)
    s = with_grad(on(arrs, env.dev))
    lower = torch.full((B, m), -INF, dtype=torch.float64, device=env.dev, requires_grad=True)
    low = [torch.full((B, m), v, dtype=torch.float64, device=env.dev, requires_grad=True) for v in (0.5, 2.0)]
    zs = _run(env, lambda t: QPFunction(verbose=-1)(*t[:6], soft_range=holder([lower, t[7], t[6]] + low)), s, c, variant)
    assert all(np.all(host(x.grad) == 0.0) for x in [lower] + low)
    worst = max([close(zs, za)] + [close(host(x.grad), host(y.grad)) for x, y in zip(s, a) if x.nelement()])
    note("reduces_to_elastic/" + label + ("-1w" if variant else ""), worst)
    assert worst <= TOL_ROLE


def check_hard_one_sided_is_the_six_input_call(env, label, variant=0):
    """both together: the six-input call"""
    from qpth_amd.qp import QPFunction
    B, n, m, q = R.SHAPES[label]
    arrs = problems.random_dense_qp(B, n, m, q, seed=R.SEED)
    c = torch.tensor(R.loss_vector(label), device=env.dev)
    a = with_grad(on(arrs, env.dev))
    za = _run(env, lambda t: QPFunction(verbose=-1)(*t), a, c, variant)
    s = with_grad(on(arrs, env.dev))
    f = [torch.full((B, m), v, dtype=torch.float64, device=env.dev, requires_grad=True) for v in (-INF, INF, INF, INF, INF)]
    zs = _run(env, lambda t: QPFunction(verbose=-1)(*t, soft_range=holder(f)), s, c, variant)
    assert all(np.all(host(x.grad) == 0.0) for x in f)
    worst = max([close(zs, za)] + [close(host(x.grad), host(y.grad)) for x, y in zip(s, a) if x.nelement()])
    note("reduces_to_six_inputs/" + label + ("-1w" if variant else ""), worst)
    assert worst <= TOL_ROLE


# ---------------------------------------------------------------- 4. the exact penalty
def check_exactness(env, label="t1b"):
    """a feasible hard range QP and gamma = 10 max multiplier of the `lower=` call on both sides: its solution, t = t_lo = 0"""
    from qpth_amd.kkt import KKTFactors
    arrs = RR.range_problem(RANGE_LABEL[label], "all")
    B = R.SHAPES[label][0]
    tq = on(arrs, env.dev)
    with env.run():
        fac = KKTFactors.build(tq[0], tq[2], tq[4], B)
        hard = fac.ipm_range(tq[1], tq[3], tq[6], tq[5])
        top = max(float(hard.lam.max()), float(hard.lam_lo.max()))
        gam, rho = torch.full_like(tq[3], 10.0 * top), torch.full_like(tq[3], 2.0)
        res = fac.ipm_soft_range(tq[1], tq[3], tq[6], gam, rho, gam, rho, tq[5])
    assert float(hard.lam.max()) > 1e-2 and float(hard.lam_lo.max()) > 1e-2
    fig = {"zhat": close(host(res.zhat), host(hard.zhat)), "t": float(np.abs(host(res.t)).max()),
           "t_lo": float(np.abs(host(res.t_lo)).max())}
    for k, v in fig.items():
        note("exact/%s/%s" % (label, k), v)
    assert fig["zhat"] <= 1e-8 and fig["t"] <= 1e-8 and fig["t_lo"] <= 1e-8


# ---------------------------------------------------------------- 5. gradcheck
SMALL_SEED = 17


def small_problem(dev):
    """(1, 6, 4, 2), the four row kinds of `mixed`, away from kinks (asserted by check_gradcheck):
    (L, p, G, h, A, b, lower, gamma_u, rho_u, gamma_l, rho_l), Q = L L' + I"""
    B, n, m, q = 1, 6, 4, 2
    r = np.random.RandomState(SMALL_SEED)
    L = r.randn(B, n, n) / np.sqrt(n)
    G, z0, A = r.randn(B, m, n), r.randn(B, n), r.randn(B, q, n)
    gz = np.einsum("bmn,bn->bm", G, z0)
    h = gz + 0.4 * r.rand(B, m) - np.array([1.2, 0.0, 0.0, 0.8]) * r.rand(B, m)
    lower = h - 0.3 - r.rand(B, m)
    lower[:, 1] = gz[:, 1] + 0.6 * r.rand(B)              # (the row with the soft lower side: pushed above G z0)
    h[:, 1] = lower[:, 1] + 0.5
    gu, ru, gl, rl = 0.3 + r.rand(B, m), 0.5 + 2.0 * r.rand(B, m), 0.3 + r.rand(B, m), 0.5 + 2.0 * r.rand(B, m)
    gu[:, 1] = INF
    gl[:, 2] = INF
    lower[:, 3] = -INF
    return on((L, 2.0 * r.randn(B, n), G, h, A, np.einsum("bqn,bn->bq", A, z0), lower, gu, ru, gl, rl), dev)


def check_gradcheck(env):
    """torch.autograd.gradcheck over all eleven inputs in reverse mode (Q = L L' + I through L, as tests/elastic_checks.py).
    eps = 1e-6; atol 1e-5 covers the central difference's noise, the solution's ~1e-11 over 2 eps, rtol 1e-3 its truncation."""
    from qpth_amd.kkt import KKTFactors
    from qpth_amd.qp import QPFunction
    ins = small_problem(env.dev)
    eye = torch.eye(6, dtype=torch.float64, device=env.dev)
    with env.run():
        fac = KKTFactors.build(ins[0] @ ins[0].transpose(-1, -2) + eye, ins[2], ins[4], 1)
        res = fac.ipm_soft_range(ins[1], ins[3], *ins[6:], ins[5])
    for lk, sk in PAIRS:                                   # no kink nearby, on any live pair
        lam, s = host(getattr(res, lk)), host(getattr(res, "slacks" + lk[3:]))
        assert np.all(np.maximum(lam, s) > 1e-2), (lk, lam, s)
    assert (host(res.t) > 1e-2).any() and (host(res.t_lo) > 1e-2).any()
    for t in ins:
        t.requires_grad_(True)

    def f(L, p, G, h, A, b, lower, gu, ru, gl, rl):
        return QPFunction(verbose=-1)(L @ L.transpose(-1, -2) + eye, p, G, h, A, b, soft_range=holder((lower, gu, ru, gl, rl)))

    with env.run():
        assert torch.autograd.gradcheck(f, ins, eps=1e-6, atol=1e-5, rtol=1e-3, check_forward_ad=False)


# ---------------------------------------------------------------- 6. the library's own call on the augmented QP (shapes without a fixture)
SLOT_SHAPES = {          # slot counts no fixture reaches: nz > 64 and nz > 128 beside few rows -- (n, m, q) -> the loop form
    "s11b": (70, 12, 0),     # one tile row, two slots
    "s12": (130, 9, 0),      # one tile row, four slots
}


def check_augmented_call(env, key, variant=0):
    """the soft_range call against the library's six-input call on the augmented QP, each QP alone: zhat and the eleven
    gradients folded back, at the project's gate (two paths of the library, whichever family serves the augmented QP)"""
    from qpth_amd.qp import QPFunction
    n, m, q = SLOT_SHAPES[key]
    B = 2
    r = np.random.RandomState(61)
    L = r.randn(B, n, n)
    Q = np.matmul(L, L.transpose((0, 2, 1))) / n + np.eye(n)
    G, z0, p, A = r.randn(B, m, n), r.randn(B, n), r.randn(B, n), r.randn(B, q, n)
    gu, ru, gl, rl = 0.2 + 3.0 * r.rand(B, m), 0.5 + 4.0 * r.rand(B, m), 0.2 + 3.0 * r.rand(B, m), 0.5 + 4.0 * r.rand(B, m)
    i = np.arange(m)
    gz = np.einsum("bmn,bn->bm", G, z0)
    width, pull = 0.3 + r.rand(B, m), 1.5 * r.rand(B, m)
    h = gz + 0.5 * r.rand(B, m)
    h = np.where(i % 6 == 0, h - pull, h)
    h = np.where(i % 6 == 3, gz + pull + width, h)
    lower = h - width
    gu[:, i % 4 == 1] = INF
    gl[:, i % 4 == 2] = INF
    lower[:, i % 4 == 3] = -INF
    b = np.einsum("bqn,bn->bq", A, z0)
    c = r.randn(B, n)
    arrs = (Q, p, G, h, A if q else np.zeros(0), b if q else np.zeros(0), lower, gu, ru, gl, rl)
    tq = with_grad(on(arrs, env.dev))
    with env.run(variant):
        z = QPFunction(verbose=-1)(*tq[:6], soft_range=holder(tq[6:]))
        (z * torch.tensor(c, device=env.dev)).sum().backward()
    worst = 0.0
    for k in range(B):
        Q2, p2, G2, h2, A2, sets, bk = augmented(arrs, k)
        t2 = with_grad(on((Q2, p2, G2, h2, A2, bk), env.dev))
        with env.run():
            z2 = QPFunction(verbose=-1)(*t2)
            (z2[:, :n] * torch.tensor(c[k:k + 1], device=env.dev)).sum().backward()
        dA2 = host(t2[4].grad) if q else np.zeros((0, n))
        f = R.fold(host(t2[0].grad), host(t2[1].grad), host(t2[2].grad), host(t2[3].grad), dA2, sets, n, m)
        ref = [host(z2)[0, :n]] + list(f[:4]) + list(f[5:]) + ([f[4], host(t2[5].grad)] if q else [])
        mine = [host(z)[k]] + [host(tq[j].grad)[k] for j in (0, 1, 2, 3, 6, 7, 8, 9, 10)] \
            + ([host(tq[4].grad)[k], host(tq[5].grad)[k]] if q else [])
        worst = max([worst] + [close(a, x) for a, x in zip(mine, ref)])
    note("augmented_call/%s" % key, worst)
    assert worst <= TOL_REF


# ---------------------------------------------------------------- 7. status, refusals, reductions, the old call
def check_abi_codes(env):
    """QPX_ERR_* of the entry point and qpx_soft_range_supported, no launch"""
    from qpth_amd import _lib
    with env.run():
        dll = _lib.backend_for(torch.empty(0, device=env.dev)).dll
        for (n, m, q) in [R.SHAPES[k][1:] for k in R.SHAPES]:
            assert dll.qpx_soft_range_supported(_lib.QPX_F64, n, m, q) == 1
            assert dll.qpx_soft_range_supported(_lib.QPX_F32, n, m, q) == 0
            assert dll.qpx_soft_range_supported(_lib.QPX_F32_WIDE, n, m, q) == 0
        for (n, m, q) in SLOT_SHAPES.values():
            assert dll.qpx_soft_range_supported(_lib.QPX_F64, n, m, q) == 1
        assert dll.qpx_soft_range_supported(_lib.QPX_F64, 100, 100, 10) == 0          # the large-QP family
        assert dll.qpx_soft_range_supported(_lib.QPX_F64, 300, 400, 0) == 0           # the augmented QP itself
        assert dll.qpx_soft_range_supported(_lib.QPX_F64, 0, 4, 0) == 0
        one = torch.ones(512, dtype=torch.float64, device=env.dev)
        i32 = torch.zeros(8, dtype=torch.int32, device=env.dev)
        P = one.data_ptr()
        names = ("lower", "gamma_u", "rho_u", "gamma_l", "rho_l", "gt1", "lam_lo", "slack_lo", "lam_t", "slack_t", "lam_tl",
                 "slack_tl", "t", "t_lo")

        def ipm(dtype, n, m, q, stride=None, **null):
            a = {k: (None if k in null else P) for k in names}
            s = {k: (-1 if k == stride else 0) for k in names[:5]}
            return dll.qpx_ipm_soft_range(dtype, 1, n, m, q, P, 0, P, 0, P, 0, P, 0, 1e-8, 20, 3, 1, P, P, P, P, i32.data_ptr(),
                                          i32.data_ptr(), P, None, a["lower"], s["lower"], a["gamma_u"], s["gamma_u"], a["rho_u"],
                                          s["rho_u"], a["gamma_l"], s["gamma_l"], a["rho_l"], s["rho_l"], a["gt1"], a["lam_lo"],
                                          a["slack_lo"], a["lam_t"], a["slack_t"], a["lam_tl"], a["slack_tl"], a["t"], a["t_lo"], None)

        assert ipm(_lib.QPX_F32, 6, 4, 2) == -2 and ipm(_lib.QPX_F32_WIDE, 6, 4, 2) == -2                    # QPX_ERR_UNSUPPORTED
        assert ipm(_lib.QPX_F64, 100, 100, 10) == -2
        for k in names:                                                                                  # QPX_ERR_ARG
            assert ipm(_lib.QPX_F64, 6, 4, 2, **{k: True}) == -1, k
        for k in names[:5]:
            assert ipm(_lib.QPX_F64, 6, 4, 2, stride=k) == -1, k
        assert ipm(7, 6, 4, 2) == -1 and ipm(_lib.QPX_F64, 6, 0, 2) == -1
        # the A/B knob: a form without the role declines
        old = dll.qpx_set_ipm_variant(256)                                       # the 16x16 thread grid at every size
        try:
            assert dll.qpx_soft_range_supported(_lib.QPX_F64, 6, 4, 2) == 0 and ipm(_lib.QPX_F64, 6, 4, 2) == -2
        finally:
            dll.qpx_set_ipm_variant(old)


def check_bad_entries(env, pytest):
    from qpth_amd import _lib
    from qpth_amd.kkt import KKTFactors
    from qpth_amd.qp import QPFunction
    arrs = R.soft_range_problem("t1b", "mixed")
    tq = on(arrs, env.dev)
    six, fields, h = tq[:6], tq[6:], tq[3]
    nan = float("nan")
    bad = {0: ((nan, INF, float(h[1, 4]), float(h[1, 4]) + 1.0), "lower must be below h"),
           1: ((nan, -0.5, -INF), "l1 must be non-negative"), 2: ((nan, 0.0, -1.0), "rho must be positive"),
           3: ((nan, -0.5), "l1_lower must be non-negative"), 4: ((nan, 0.0, -1.0), "rho_lower must be positive")}
    with env.run():
        for k, (values, msg) in bad.items():
            for v in values:
                f = [x.clone() for x in fields]
                f[k][1, 4] = v
                with pytest.raises(ValueError, match=msg):
                    QPFunction(verbose=-1)(*six, soft_range=holder(f))
        # (the lower side's penalty of a ONE-SIDED row is checked too: a NaN anywhere)
        f = [x.clone() for x in fields]
        f[3][1, 3] = nan
        with pytest.raises(ValueError, match="l1_lower must be non-negative"):
            QPFunction(verbose=-1)(*six, soft_range=holder(f))
        with pytest.raises(ValueError, match="rho must be positive"):              # the pure l1 side
            QPFunction(verbose=-1)(*six, soft_range=holder([fields[0], fields[1], 0.0]))
        # the QP is left as the `Q not SPD` path leaves one; its neighbour is bit-equal to the clean launch
        f = [x.clone() for x in fields]
        f[2][1, 4] = nan
        fac = KKTFactors.build(tq[0], tq[2], tq[4], 2)
        res = fac.ipm_soft_range(tq[1], h, *f, tq[5])
        good = fac.ipm_soft_range(tq[1], h, *fields, tq[5])
    st = host(res.status)
    assert st[1] & _lib.ST_NONFINITE and not st[0] & _lib.ST_NONFINITE
    assert host(res.iters)[1] == 0 and np.isposinf(host(res.best_resid)[1])
    outs = ("zhat", "nu", "lam", "slacks", "lam_lo", "slacks_lo", "lam_t", "slacks_t", "lam_tl", "slacks_tl", "t", "t_lo")
    for k in outs:
        assert np.isnan(host(getattr(res, k))[1]).all(), k
        assert np.array_equal(host(getattr(res, k))[0], host(getattr(good, k))[0]), k
    # the bit stays with the launch that met it; the factors' own status words never saw it
    with env.run():
        fac.raise_on_failure()
        fac.ipm_soft_range(tq[1], h, *f, tq[5])
        with pytest.raises(ValueError, match="rho must be positive"):
            fac.raise_on_failure()
    assert not (host(fac.status) & _lib.ST_NONFINITE).any()


def check_refusals(env, pytest):
    from qpth_amd import WarmStart
    from qpth_amd.qp import QPFunction, QPSolvers
    arrs = R.soft_range_problem("t1b", "mixed")
    tq = on(arrs, env.dev)
    six, fields = tq[:6], tq[6:]
    sr = holder(fields)
    way_out = r"augmented dense QP"
    with env.run():
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1)(*[t.float() for t in six], soft_range=holder([t.float() for t in fields]))
        big = on(R.soft_range_problem("c7", "all"), env.dev)
        A = torch.zeros(2, 10, 100, dtype=torch.float64, device=env.dev)
        with pytest.raises(ValueError, match=way_out):                     # nz + neq + nineq = 210: the large-QP family
            QPFunction(verbose=-1)(big[0], big[1], big[2], big[3], A, A[:, :, 0], soft_range=holder(big[6:]))
        for extra in ({"rho": 2.5}, {"kappa": 1e-3}, {"lower": fields[0]}, {"l1": 1.0}):
            with pytest.raises(ValueError, match=way_out):
                QPFunction(verbose=-1)(*six, soft_range=sr, **extra)
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1, refine=1)(*six, soft_range=sr)
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1, duals=True)(*six, soft_range=sr)
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1, warm_start=WarmStart())(*six, soft_range=sr)
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1, solver=QPSolvers.CVXPY)(*six, soft_range=sr)
        with pytest.raises(ValueError, match="SoftRange"):
            QPFunction(verbose=-1)(*six, soft_range=tuple(fields))
        with pytest.raises(ValueError, match="shape"):
            QPFunction(verbose=-1)(*six, soft_range=holder([fields[0][:, :-1]] + fields[1:]))
        with pytest.raises(ValueError, match="shape"):
            QPFunction(verbose=-1)(*six, soft_range=holder([fields[0], fields[1][:1].expand(3, -1), fields[2]]))
        with pytest.raises(AttributeError):
            sr.lower = fields[0]
        # the refusal of the two keywords together stays as it was
        with pytest.raises(ValueError, match=way_out):
            QPFunction(verbose=-1)(*six, fields[2], lower=fields[0], l1=fields[1])
        # forward mode and a second grad
        with pytest.raises(RuntimeError), fwAD.dual_level():
            QPFunction(verbose=-1)(*six[:1], fwAD.make_dual(six[1], torch.ones_like(six[1])), *six[2:], soft_range=sr)
        ins = [t.clone().requires_grad_(True) for t in tq]
        z = QPFunction(verbose=-1)(*ins[:6], soft_range=holder(ins[6:]))
        (gp,) = torch.autograd.grad(z.sum(), ins[1], create_graph=True)
        with pytest.raises(RuntimeError):
            torch.autograd.grad(gp.sum(), ins[3])


def check_reductions(env):
    """fields the batch shares: the `.mean(0)` of the per-QP gradient; scalars and floats: summed over the rows as well;
    l1_lower, rho_lower default to the upper side's"""
    from qpth_amd.qp import QPFunction
    arrs = R.soft_range_problem("t1a", "all")
    tq = on(arrs, env.dev)
    six = tq[:3] + [tq[3][0]] + tq[4:6]              # (h of the first QP for both: a shared lower has to lie below every h)
    c = torch.tensor(R.loss_vector("t1a"), device=env.dev)

    def grads_of(fields):
        f = [(x.clone() if torch.is_tensor(x) else torch.tensor(x, dtype=torch.float64, device=env.dev)).requires_grad_(True) for x in fields]
        with env.run():
            z = QPFunction(verbose=-1)(*six, soft_range=holder(f))
            (z * c).sum().backward()
        return host(z), [host(x.grad) for x in f]

    shared = [x[0] for x in tq[6:]]
    z1, g1 = grads_of([x.expand(2, -1).contiguous() for x in shared])
    z2, g2 = grads_of(shared)
    assert np.array_equal(z1, z2) and all(g.shape == (4,) for g in g2)
    assert max(close(b, a.mean(0)) for a, b in zip(g1, g2)) <= 1e-12 and min(np.abs(a).max() for a in g1) > 0
    lo = float(host(tq[6]).min()) - 0.5
    vals = (lo, 0.7, 1.5, 0.4, 2.5)
    z3, g3 = grads_of([torch.full((2, 4), v, dtype=torch.float64, device=env.dev) for v in vals])
    z4, g4 = grads_of(vals)
    assert np.array_equal(z3, z4) and all(g.shape == () for g in g4)
    assert max(close(b, a.mean(0).sum()) for a, b in zip(g3, g4)) <= 1e-12
    with env.run():                                                   # Python floats; the lower side's default
        z5 = QPFunction(verbose=-1)(*six, soft_range=holder(vals))
        z6 = QPFunction(verbose=-1)(*six, soft_range=holder(vals[:3]))
        z7 = QPFunction(verbose=-1)(*six, soft_range=holder(vals[:3] + vals[1:3]))
    assert np.array_equal(host(z5), z4) and np.array_equal(host(z6), host(z7)) and not np.array_equal(host(z6), z4)


def check_none_is_the_old_call(env):
    """soft_range=None: the same node, bit for bit the old call -- six inputs, with rho, with lower"""
    from qpth_amd.qp import QPFunction
    arrs = ER.elastic_problem("t1b", "all")
    lower = arrs[3] - 5.0
    cases = (((), {}, "QPFunctionFn"), ((arrs[6],), {}, "QPSoftFunctionFn"), ((), {"lower": lower}, "QPRangeFunctionFn"),
             ((arrs[6],), {"l1": arrs[7]}, "QPElasticFunctionFn"))
    for pos, kw, node in cases:
        outs = []
        for extra in ({}, {"soft_range": None}):
            tq = with_grad(on(arrs[:6] + pos, env.dev))
            kws = {k: torch.tensor(v, device=env.dev) for k, v in kw.items()}
            with env.run():
                z = QPFunction(verbose=-1)(*tq, **kws, **extra)
                assert type(z.grad_fn).__name__.startswith(node)
                z.backward(torch.ones_like(z))
            outs.append([host(z)] + [host(t.grad) for t in tq])
        for a, c in zip(*outs):
            assert np.array_equal(a, c)
