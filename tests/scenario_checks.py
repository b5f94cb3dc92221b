"""Scenario batches (scenarios=K): B groups of K consecutive QPs, one factor blob per group.  The checks that
tests/test_emu_scenarios.py runs on the host-thread emulator and tests/test_gpu_scenarios.py on the GPU; `env` is the
module's Env (dev, run(variant)).  The reference everywhere is the library's own existing call on the EXPANDED batch of B K
QPs -- batched Q, G, A as X.repeat_interleave(K, 0), p, h, b flattened --; at (6,4,2) and (12,9,3) oracle/qp_oracle too, at
the project's 1e-6 gate.

Gates.  The forward, and dp, dh, db of the backward: bitwise (the same kernel form on the same per-QP data; only the blob's
address differs).  A contracted matrix gradient out[g] = scale sum_k (u_k^T v_k + w_k^T x_k) against another order of the
same additions: elementwise within 4 K 2^-53 S, S = scale sum_k (|u_k|^T |v_k| + |w_k|^T |x_k|), the sum of the magnitudes of
the 2 K products that are added -- 2 K 2^-53 S bounds the rounding of one order of a sum of 2 K terms (Higham, Accuracy and
Stability, (4.4), gamma_{2K-1} with exactly rounded products inside the fused multiply-adds), and both sides of a comparison
carry it.  (The magnitudes are those of the PRODUCTS: u_k^T v_k + w_k^T x_k may cancel, and a bound in terms of its value
would not hold even for K = 1.)  float32: the same with 2^-24."""
import numpy as np
import pytest
import torch

import problems
from oracle import qp_oracle as orc
from qpth_amd import _lib
from qpth_amd.kkt import KKTFactors
from qpth_amd.qp import QPFunction, QPSolvers

# one shape per loop form of the default dispatch (thread grid 16x16 at 1, 2, 3 blocks; tiles at 4 and 7 rows with and without
# equality constraints; thread grid beyond the tiles' 112 rows at two sizes)
FORM_SHAPES = [(12, 9, 3), (20, 24, 3), (20, 40, 4), (100, 50, 10), (100, 100, 0), (40, 130, 0), (20, 170, 2)]
ONE_WAVE = 2048                               # knob: the tile kernels with one wave per QP
ONE_WAVE_SHAPES = [(20, 40, 4), (100, 50, 10)]
OUTER_SHAPES = [(12, 9), (100, 100), (10, 100)]
OUTER_KS = [1, 3, 16, 17, 257]                # 17 crosses a wave's 16-QP trip, 257 a workgroup's 256-QP trip
GRADCHECK_SEED = 1                            # a (6,4,2) instance away from kinks (asserted by check_gradcheck)
U64 = 2.0 ** -53
FWD = ("zhat", "nu", "lam", "slacks", "iters", "status", "best_resid")


def tag(shape):
    return "n%d_m%d_q%d" % tuple(shape)


def _t(x, dev, dtype=torch.float64):
    x = np.asarray(x)
    return torch.tensor(x, dtype=dtype, device=dev) if x.size else torch.empty(0, dtype=dtype, device=dev)


_DATA = {}


def data(shape, B, K, seed=5):
    """numpy: Q, G, A of B groups (problems.prof_qp) and p, h, b of B K QPs, feasible by construction (h = G z0 + s0, b = A z0
    with the group's G, A); made once per case"""
    key = (tuple(shape), B, K, seed)
    if key not in _DATA:
        n, m, q = shape
        Q, _, G, _, A, _ = problems.prof_qp(B, n, m, q, seed=seed)
        r = np.random.RandomState(seed + 1000)
        z0, s0, p = r.randn(B, K, n), r.rand(B, K, m), r.randn(B, K, n)
        h = np.einsum("gmn,gkn->gkm", G, z0) + s0
        b = np.einsum("gqn,gkn->gkq", A, z0) if q else np.zeros(0)
        _DATA[key] = (Q, p, G, h, A, b)
    return _DATA[key]


def lib_of(env):
    """the library the calls inside env.run() go to"""
    with env.run(0):
        return _lib.backend_for(torch.zeros(1, device=env.dev))


def tensors(env, shape, B, K, dtype=torch.float64, seed=5):
    """-> (Q, G, A) of the groups, (p, h, b) flattened to (B K, .), (Q, G, A) of the expanded batch"""
    Q, p, G, h, A, b = [_t(x, env.dev, dtype) for x in data(shape, B, K, seed)]
    n, m, q = shape
    vec = [p.reshape(B * K, n), h.reshape(B * K, m), b.reshape(B * K, q) if q else b]
    exp = [X.repeat_interleave(K, 0) if X.nelement() else X for X in (Q, G, A)]
    return (Q, G, A), vec, exp


def solve_both(env, shape, B=2, K=3, knob=0, dtype=torch.float64, wide=False):
    """the grouped factors and loop result, and the expanded batch's, under `knob`"""
    (Q, G, A), (p, h, b), (Qe, Ge, Ae) = tensors(env, shape, B, K, dtype)
    with env.run(knob):
        fg = KKTFactors.build(Q, G, A, nBatch=B, wide=wide, scenarios=K)
        rg = fg.ipm(p, h, b)
        fe = KKTFactors.build(Qe, Ge, Ae, wide=wide)
        re = fe.ipm(p, h, b)
    return fg, rg, fe, re


def check_forward_bitwise(env, shape, B=2, K=3, knob=0, dtype=torch.float64, wide=False):
    n, m, q = shape
    fg, rg, fe, re = solve_both(env, shape, B, K, knob, dtype, wide)
    assert fg.blob.numel() == B * fg.elems and fe.blob.numel() == B * K * fe.elems and fg.elems == fe.elems
    assert fg.status.numel() == B * K
    for name in FWD:
        g, e = getattr(rg, name), getattr(re, name)
        assert g.shape == e.shape and g.shape[0] == B * K, name
        assert torch.equal(g, e), (name, shape, B, K, knob)
    assert int(rg.status.max()) & 7 == 0 and bool(torch.isfinite(rg.zhat).all())
    assert int(rg.iters.min()) > 0


def _terms(u, v, w, x, K, scale):
    """numpy: per group the sum of the products in float64, and S, the sum of their magnitudes (module docstring)"""
    u, v, w, x = [a.detach().cpu().double().numpy() for a in (u, v, w, x)]
    B = u.shape[0] // K
    u, v, w, x = [a.reshape(B, K, -1) for a in (u, v, w, x)]
    val = scale * (np.einsum("gkr,gkc->grc", u, v) + np.einsum("gkr,gkc->grc", w, x))
    mag = scale * (np.einsum("gkr,gkc->grc", np.abs(u), np.abs(v)) + np.einsum("gkr,gkc->grc", np.abs(w), np.abs(x)))
    return val, mag


def _within(got, ref, mag, K, what, unit=U64):
    got, ref = got.detach().cpu().double().numpy(), np.asarray(ref)
    bound = 4 * K * unit * mag
    worst = float(np.max(np.abs(got - ref) / np.maximum(bound, 1e-300)))
    print("%s: max |difference| / (4 K u S) = %.3f (K = %d)" % (what, worst, K))
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    assert worst <= 1.0, (what, worst)


def check_backward(env, shape, duals, B=2, K=3, knob=0):
    """dp, dh, db bitwise; dQ, dG, dA per group against the sum over k of the expanded call's per-QP gradients"""
    n, m, q = shape
    fg, rg, fe, re = solve_both(env, shape, B, K, knob)
    g = torch.Generator().manual_seed(7)
    cot = [torch.randn(B * K, k, generator=g, dtype=torch.float64).to(env.dev) for k in (n, m, max(q, 1))]
    kw = dict(dl_dlam=cot[1], dl_dnu=cot[2][:, :q] if q else None) if duals else {}
    with env.run(knob):
        got = fg.backward(rg.zhat, rg.lam, rg.slacks, rg.nu, cot[0], **kw)
        out = fe.backward(re.zhat, re.lam, re.slacks, re.nu, cot[0], want_sol=True, **kw)
    exp, (dx, dz, dy) = out[:6], out[6]
    for i, name in ((1, "dp"), (3, "dh"), (5, "db")):
        if exp[i] is None:
            assert got[i] is None and q == 0
            continue
        assert got[i].shape[0] == B * K and torch.equal(got[i], exp[i]), (name, shape)
    zh, lm, nv = re.zhat, re.lam, re.nu
    mats = [(0, "dQ", dx, zh, zh, dx, 0.5, n), (2, "dG", dz, zh, lm, dx, 1.0, m)] + ([(4, "dA", dy, zh, nv, dx, 1.0, q)] if q else [])
    for i, name, u, v, w, x, scale, rows in mats:
        _, mag = _terms(u, v, w, x, K, scale)
        ref = exp[i].reshape(B, K, rows, n).sum(1).cpu().numpy()
        assert got[i].shape == (B, rows, n), name
        _within(got[i], ref, mag, K, "%s %s duals=%s" % (name, tag(shape), duals))
    if not q:
        assert got[4] is None and got[5] is None
    assert int(fg.status.max()) & _lib.ST_KKT_BREAKDOWN == 0


def check_outer(env, rc, K, B=3, dtype=torch.float64):
    """qpx_group_outer alone against numpy; a neighbouring group's rows filled with NaN stay out of a group's sum"""
    r, c = rc
    g = torch.Generator().manual_seed(100 * r + c + K)
    u, w = [torch.randn(B * K, r, generator=g, dtype=torch.float64).to(dtype).to(env.dev) for _ in range(2)]
    v, x = [torch.randn(B * K, c, generator=g, dtype=torch.float64).to(dtype).to(env.dev) for _ in range(2)]
    lib = lib_of(env)
    unit = U64 if dtype == torch.float64 else 2.0 ** -24
    val, mag = _terms(u, v, w, x, K, 0.5)
    out = torch.empty(B, r, c, dtype=dtype, device=env.dev)
    with env.run(0):
        lib.group_outer(K, u, v, w, x, 0.5, out)
        _within(out, val, mag, K, "group_outer %dx%d" % rc, unit)
        # one product only (w, x NULL)
        one = torch.empty(B, r, c, dtype=dtype, device=env.dev)
        lib.group_outer(K, u, v, None, None, 1.0, one)
        val1, mag1 = _terms(u, v, torch.zeros_like(u), torch.zeros_like(v), K, 1.0)
        _within(one, val1, mag1, K, "group_outer %dx%d, one product" % rc, unit)
        # deterministic: the same bits again
        again = torch.empty(B, r, c, dtype=dtype, device=env.dev)
        lib.group_outer(K, u, v, w, x, 0.5, again)
        assert torch.equal(again, out)
        # group 1 poisoned: groups 0 and 2 keep their bits, group 1 is NaN
        for a in (u, v, w, x):
            a[K:2 * K] = float("nan")
        nan = torch.empty(B, r, c, dtype=dtype, device=env.dev)
        lib.group_outer(K, u, v, w, x, 0.5, nan)
    assert torch.equal(nan[0], out[0]) and torch.equal(nan[2], out[2])
    assert bool(torch.isnan(nan[1]).all())


def check_one_factorisation_per_group(env, shape=(12, 9, 3), B=2, K=3):
    """the pre-factorisation entry is called once, with B blobs"""
    (Q, G, A), (p, h, b), _ = tensors(env, shape, B, K)
    lib = lib_of(env)
    calls, real = [], lib.pre_factor
    lib.pre_factor = lambda nblob, *a, **k: calls.append(nblob) or real(nblob, *a, **k)
    try:
        with env.run(0):
            z = QPFunction(verbose=-1, scenarios=K)(Q, p.reshape(B, K, -1), G, h.reshape(B, K, -1), A, b.reshape(B, K, -1))
    finally:
        del lib.pre_factor
    assert calls == [B], calls
    assert z.shape == (B, K, shape[0])
    code = _lib.QPX_F64
    assert lib.factor_elems(code, *shape) > 0


def qp_inputs(env, shape, B, K, mixed=True, seed=5, grad=True):
    """the six inputs of a scenarios= call and of the expanded call; mixed: p (B,K,.), h (B,.), b (.) -- else all (B,K,.)"""
    n, m, q = shape
    Q, p, G, h, A, b = [_t(x, env.dev) for x in data(shape, B, K, seed)]
    if mixed:
        # h shared by a group's scenarios, b by all QPs: feasible for every scenario (z = 0 strictly inside)
        h = h.abs().amax(1) + 1.0
        b = torch.zeros(q, dtype=torch.float64, device=env.dev) if q else b
        G = G.clone()
    six = [Q, p, G, h, A, b]
    exp = [Q.repeat_interleave(K, 0), p.reshape(B * K, n), G.repeat_interleave(K, 0),
           h.repeat_interleave(K, 0) if mixed else h.reshape(B * K, m),
           A.repeat_interleave(K, 0) if q else A, b if (mixed or not q) else b.reshape(B * K, q)]
    if grad:
        six = [x.clone().requires_grad_(True) if x.nelement() else x for x in six]
    return six, exp


def check_qpfunction_equals_expanded(env, shape, B=2, K=3, duals=False, mixed=False, knob=0):
    """QPFunction(scenarios=K) against QPFunction on the expanded batch written out with torch operations (autograd adds
    a group's gradients up): outputs bitwise, per-QP vector gradients bitwise, the rest within the contraction's bound"""
    n, m, q = shape
    six, _ = qp_inputs(env, shape, B, K, mixed=mixed)
    ref = [x.detach().clone().requires_grad_(True) if x.nelement() else x for x in six]
    Q, p, G, h, A, b = ref
    exp = [Q.repeat_interleave(K, 0), p.reshape(B * K, n), G.repeat_interleave(K, 0),
           (h.unsqueeze(1).expand(B, K, m) if mixed else h).reshape(B * K, m),
           A.repeat_interleave(K, 0) if q else A, b if (mixed or not q) else b.reshape(B * K, q)]
    g = torch.Generator().manual_seed(11)
    cz, cl, cn = [torch.randn(B, K, k, generator=g, dtype=torch.float64).to(env.dev) for k in (n, m, max(q, 1))]
    with env.run(knob):
        og = QPFunction(verbose=-1, duals=duals, scenarios=K)(*six)
        oe = QPFunction(verbose=-1, duals=duals)(*exp)
        if duals:
            for a, e in zip(og, oe):
                assert a.shape[:2] == (B, K) and torch.equal(a.reshape(e.shape), e)
            lg = (og[0] * cz).sum() + (og[2] * cl).sum() + ((og[1] * cn[..., :q]).sum() if q else 0)
            le = (oe[0] * cz.reshape(B * K, n)).sum() + (oe[2] * cl.reshape(B * K, m)).sum() + ((oe[1] * cn[..., :q].reshape(B * K, q)).sum() if q else 0)
        else:
            assert og.shape == (B, K, n) and torch.equal(og.reshape(B * K, n), oe)
            lg, le = (og * cz).sum(), (oe * cz.reshape(B * K, n)).sum()
        lg.backward()
        le.backward()
    for a, e, name in zip(six, ref, "QpGhAb"):
        if not a.nelement():
            continue
        ga, ge = a.grad, e.grad
        assert ga is not None and ga.shape == a.shape, name
        if name == "p" or (not mixed and name in "hb"):
            assert torch.equal(ga, ge), name            # per QP: the kernel's own rows
        else:
            # sums over a group (or means over the batch) in another order: K (or B K) terms of the reference's magnitude
            scale = float(ge.abs().max()) + 1e-300
            err = float((ga - ge).abs().max()) / scale
            print("QPFunction(scenarios=%d) %s: d%s max err / max |ref| %.2e" % (K, tag(shape), name, err))
            assert err <= 1e-9, (name, err)
    return og


def check_oracle(env, shape, B=2, K=3):
    """the grouped call against oracle/qp_oracle on the expanded batch: zhat and every gradient at the 1e-6 gate"""
    n, m, q = shape
    six, exp = qp_inputs(env, shape, B, K, mixed=False)
    with env.run(0):
        z = QPFunction(verbose=-1, scenarios=K)(*six)
        z.backward(torch.ones_like(z))
    Qe, pe, Ge, he, Ae, be = [x.detach().cpu().numpy() for x in exp]
    x, y, lam, s, grads, info = orc.qp_forward_backward(Qe, pe, Ge, he, Ae, be, dl_dz=np.ones((B * K, n)), per_qp=True, nthreads=2)
    err = np.linalg.norm(z.detach().cpu().numpy().reshape(B * K, n) - x, axis=1) / np.linalg.norm(x, axis=1)
    assert err.max() < 1e-6, err.max()
    for i, (a, name) in enumerate(zip(six, "QpGhAb")):
        if not a.nelement():
            continue
        ref = np.asarray(grads[i])
        if a.dim() == 3 and name in "QGA":
            ref = ref.reshape((B, K) + ref.shape[1:]).sum(1)          # a group's gradient: the sum over its scenarios
        else:
            ref = ref.reshape(a.shape)
        gerr = np.abs(a.grad.cpu().numpy() - ref).max() / max(1.0, np.abs(ref).max())
        print("scenarios vs oracle %s: d%s %.2e" % (tag(shape), name, gerr))
        assert gerr < 1e-6, (name, gerr)


def check_gradcheck(env, shape=(6, 4, 2), B=2, K=3):
    """torch.autograd.gradcheck over the six inputs, p (B,K,.), h (B,.), b (.)"""
    six, _ = qp_inputs(env, shape, B, K, mixed=True, seed=GRADCHECK_SEED)
    assert six[1].dim() == 3 and six[3].dim() == 2 and six[5].dim() == 1
    with env.run(0):
        _, nu, lam, s = QPFunction(verbose=-1, duals=True, scenarios=K)(*[x.detach() for x in six])
    assert float(torch.maximum(lam, s).min()) > 1e-2, torch.maximum(lam, s).min()          # no kink nearby
    assert float(lam.max()) > 1e-2                                                         # ... and an active row

    def f(Lq, p, G, h, A, b):
        # Q = L L' stays SPD along every perturbation.  An un-batched parameter gets the `.mean(0)` of the expanded call's B K
        # per-QP gradients (qp.py:159-177), not their sum: the hook turns that convention back into the derivative gradcheck measures
        b = b * 1.0
        b.register_hook(lambda g: g * (B * K))
        return QPFunction(verbose=-1, scenarios=K)(Lq @ Lq.transpose(1, 2), p, G, h, A, b)

    Lq = torch.linalg.cholesky(six[0].detach()).requires_grad_(True)
    with env.run(0):
        # eps = 1e-6; atol 1e-5 covers the central difference's noise, the solution's ~1e-11 over 2 eps, rtol 1e-3 its truncation
        assert torch.autograd.gradcheck(f, [Lq] + six[1:], eps=1e-6, atol=1e-5, rtol=1e-3, check_forward_ad=False)


def check_status(env, shape=(12, 9, 3), B=2, K=3):
    """a non-SPD Q in group 1 of 2: QPFunction raises as the expanded call does; at the KKTFactors level group 0's QPs are
    solved bit-identically, group 1's are NaN with the status bit set"""
    n, m, q = shape
    (Q, G, A), (p, h, b), _ = tensors(env, shape, B, K)
    good = solve_both(env, shape, B, K)[1]
    Q = Q.clone()
    Q[1] = -Q[1]
    msgs = []
    for scen in (K, None):
        args = (Q, p.reshape(B, K, n), G, h.reshape(B, K, m), A, b.reshape(B, K, q) if q else b) if scen else \
               (Q.repeat_interleave(K, 0), p, G.repeat_interleave(K, 0), h, A.repeat_interleave(K, 0) if q else A, b)
        with env.run(0), pytest.raises(RuntimeError) as e:
            QPFunction(verbose=-1, scenarios=scen)(*args)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1] and "Q is not SPD" in msgs[0]
    with env.run(0):
        fac = KKTFactors.build(Q, G, A, nBatch=B, scenarios=K)
        r = fac.ipm(p, h, b)
        with pytest.raises(RuntimeError, match="not SPD"):
            fac.raise_on_failure(check_Q_spd=True)
    for name in ("zhat", "nu", "lam", "slacks", "iters", "best_resid"):
        assert torch.equal(getattr(r, name)[:K], getattr(good, name)[:K]), name
    assert torch.equal(r.status[:K], good.status[:K])
    assert bool(torch.isnan(r.zhat[K:]).all())
    assert bool(((r.status[K:] & _lib.ST_Q_NOT_SPD) != 0).all()) and r.status.numel() == B * K


def check_abi(env):
    """error codes without a launch, and qpx_group_supported"""
    dev = env.dev
    lib = lib_of(env)
    dll, F64 = lib.dll, _lib.QPX_F64
    with env.run(0):
        for shape in FORM_SHAPES + [(6, 4, 2)]:
            assert dll.qpx_group_supported(F64, *shape) == 1 == dll.qpx_can_share_factors(F64, *shape), shape
        assert dll.qpx_group_supported(_lib.QPX_F32, 12, 9, 3) == 1 and dll.qpx_group_supported(_lib.QPX_F32_WIDE, 12, 9, 3) == 1
        assert dll.qpx_group_supported(F64, 120, 100, 10) == 0             # the large-QP family
        assert dll.qpx_group_supported(F64, 2000, 10, 0) == 0 and dll.qpx_group_supported(7, 12, 9, 3) == 0
    with env.run(3):
        assert dll.qpx_group_supported(F64, 20, 10, 4) == 0                # ... forced by the knob
    with env.run(ONE_WAVE):
        assert all(dll.qpx_group_supported(F64, *s) == 1 for s in ONE_WAVE_SHAPES)
    n, m, q, B, K = 12, 9, 3, 2, 3
    t = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)      # noqa: E731
    fac, st, it = t(B * lib.factor_elems(F64, n, m, q)), torch.zeros(B * K, dtype=torch.int32, device=dev), torch.zeros(B * K, dtype=torch.int32, device=dev)
    P = _lib._ptr
    sf = lib.factor_elems(F64, n, m, q)

    def ipm(K=K, n=n, m=m, q=q, p=t(B * K, n), zhat=t(B * K, n), nu=t(B * K, q), b=t(B * K, q)):
        return dll.qpx_ipm_group(F64, B, K, n, m, q, P(p), n, P(t(B * 3, m)), m, P(b), q, P(fac), sf, 1e-12, 20, 3, 2, P(zhat), P(nu),
                                 P(t(B * 3, m)), P(t(B * 3, m)), P(it), P(st), P(t(B * 3)), None, None)

    def bwd(K=K, n=n, m=m, q=q, dQ=None, dG=None, dA=None, refine=0, zhat=t(B * K, n), dl_dz=t(B * K, n)):
        return dll.qpx_backward_group(F64, B, K, n, m, q, P(fac), sf, P(zhat), P(t(B * 3, m)), P(t(B * 3, m)), P(t(B * 3, q)), P(dl_dz), None,
                                      None, P(dQ), P(t(B * 3, n)), P(dG), None, P(dA), None, None, None, None, refine, None, 0, None, 0,
                                      None, 0, P(st), None)

    with env.run(0):
        assert ipm(K=0) == -1 and ipm(K=-2) == -1 and ipm(p=None) == -1 and ipm(zhat=None) == -1 and ipm(nu=None) == -1 and ipm(b=None) == -1
        assert ipm(n=120, m=100, q=10) == -2                                # unsupported size, before any launch
        assert bwd(K=0) == -1 and bwd(zhat=None) == -1 and bwd(dl_dz=None) == -1
        assert bwd(dQ=t(1)) == -1 and bwd(dG=t(1)) == -1 and bwd(dA=t(1)) == -1
        assert bwd(refine=1) == -2 and bwd(refine=-1) == -1 and bwd(n=120, m=100, q=10) == -2
        u = t(6, 4)
        go = lambda **k: dll.qpx_group_outer(k.get("dt", F64), k.get("B", 2), k.get("K", 3), 4, k.get("c", 4), P(k.get("u", u)), P(k.get("v", u)),      # noqa: E731
                                             P(k.get("w")), P(k.get("x")), 1.0, P(k.get("out", t(2, 4, 4))), P(k.get("ws")), k.get("n", 0), None)
        assert go(K=0) == -1 and go(B=0) == -1 and go(u=None) == -1 and go(out=None) == -1 and go(w=u) == -1 and go(dt=_lib.QPX_F32_WIDE) == -1
        assert go(v=None) == -1                                             # a column of ones needs c = 1
        assert go() == -1                                                   # B > 1 without the workspace
        assert dll.qpx_group_outer_workspace_elems(F64, 2, 3, 4, 4) == 2 * 256 and dll.qpx_group_outer_workspace_elems(F64, 1, 3, 4, 4) == 0
        assert dll.qpx_group_outer_workspace_elems(F64, 3, 5, 100, 100) == 3 * 49 * 256
    with env.run(3):
        assert ipm() == -2 and bwd() == -2
    assert int(st.max()) == 0 and int(it.max()) == 0                        # nothing ran


def check_refusals(env, shape=(12, 9, 3), B=2, K=3):
    from qpth_amd import SoftRange, WarmStart
    six, _ = qp_inputs(env, shape, B, K, mixed=False, grad=False)
    m = shape[1]
    one = torch.ones(m, dtype=torch.float64, device=env.dev)
    way_out = "expanded batch"
    with env.run(0):
        for kw in (dict(rho=one), dict(kappa=1e-3), dict(lower=-one * 1e3), dict(rho=one, l1=one),
                   dict(soft_range=SoftRange(-one * 1e3, one, one))):
            with pytest.raises(ValueError, match=way_out):
                QPFunction(verbose=-1, scenarios=K)(*six, **kw)
        for opt in (dict(warm_start=WarmStart()), dict(refine=1), dict(solver=QPSolvers.CVXPY)):
            with pytest.raises(ValueError, match=way_out):
                QPFunction(verbose=-1, scenarios=K, **opt)(*six)
        for bad in (0, -1, 2.5):
            with pytest.raises(ValueError, match="positive integer"):
                QPFunction(verbose=-1, scenarios=bad)(*six)
        with pytest.raises(ValueError, match="has shape"):
            QPFunction(verbose=-1, scenarios=K + 1)(*six)
        # forward mode and second derivatives
        import torch.autograd.forward_ad as fwAD
        with fwAD.dual_level():
            p = fwAD.make_dual(six[1], torch.ones_like(six[1]))
            with pytest.raises(RuntimeError, match="forward mode"):
                QPFunction(verbose=-1, scenarios=K)(six[0], p, *six[2:])
        p = six[1].clone().requires_grad_(True)
        z = QPFunction(verbose=-1, scenarios=K)(six[0], p, *six[2:])
        (g,) = torch.autograd.grad(z.sum(), p, create_graph=True)
        with pytest.raises(RuntimeError):
            g.sum().backward()
        # the launches beside the loop and the backward are not served on grouped factors
        fac = KKTFactors.build(six[0], six[2], six[4], nBatch=B, scenarios=K)
        with pytest.raises(RuntimeError, match="scenarios"):
            fac.jvp(z.detach().reshape(B * K, -1), None, None, None, (None,) * 6)


def check_shared_matrices_take_the_one_blob_path(env, shape=(12, 9, 3), B=2, K=3):
    """Q, G, A all un-batched: the existing call on B K QPs, one blob"""
    n, m, q = shape
    Q, p, G, h, A, b = [_t(x, env.dev) for x in data(shape, B, K)]
    Q, G, A = Q[0], G[0], (A[0] if q else A)
    h = h.abs().amax((0, 1)) + 1.0
    b = torch.zeros(q, dtype=torch.float64, device=env.dev) if q else b
    with env.run(0):
        got = QPFunction(verbose=-1, scenarios=K)(Q, p, G, h, A, b)
        ref = QPFunction(verbose=-1)(Q, p.reshape(B * K, n), G, h, A, b)
        fac = KKTFactors.build(Q, G, A, nBatch=B, scenarios=K)
    assert got.shape == (B, K, n) and torch.equal(got.reshape(B * K, n), ref)
    assert fac.K is None and fac.shared and fac.B == B * K and fac.blob.numel() == fac.elems


def check_fallback_equals_expanded(env, shape=(120, 100, 10), B=1, K=2):
    """where qpx_group_supported is 0 the call runs the expanded batch itself"""
    n, m, q = shape
    six, exp = qp_inputs(env, shape, B, K, mixed=False)
    ref = [x.detach().clone().requires_grad_(True) if x.nelement() else x for x in exp]
    with env.run(0):
        assert not _lib.backend_for(six[0]).group_supported(_lib.QPX_F64, n, m, q)
        got = QPFunction(verbose=-1, scenarios=K)(*six)
        want = QPFunction(verbose=-1)(*ref)
        got.sum().backward()
        want.sum().backward()
    assert got.shape == (B, K, n) and torch.equal(got.reshape(B * K, n), want)
    assert torch.equal(six[1].grad.reshape(B * K, n), ref[1].grad)
    assert torch.allclose(six[0].grad, ref[0].grad.reshape(B, K, n, n).sum(1), rtol=1e-12, atol=0)
