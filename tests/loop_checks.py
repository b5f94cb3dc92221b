"""The PATH of the hard-QP interior-point loop (KKTFactors.ipm, qpx_ipm), not only its end: the checks that
tests/test_emu_loop.py runs on the host-thread emulator and tests/test_gpu_loop.py on a real MI355X.  Every check takes an
`env`: env.dev (the torch device) and env.run(variant=0), a context manager around the library calls (the A/B knob of
include/qpx.h, qpx_set_ipm_variant: which form of the loop kernel runs).

A primal-dual interior-point loop corrects itself: with a wrong Newton direction, centring parameter, step length or start
point it still reaches the optimum, by another path and in another number of passes.  The tests of the converged answer
cannot see that; these compare the ITERATES, the iteration counts and the per-iteration residuals with oracle/qp_oracle
(pinned to the reference by tests/test_oracle_golden.py), QP by QP.

Problems: problems.prof_qp(B, n, m, q, SEED) at SHAPES; batches of three (two where a form gives every QP a launch
sequence of its own: the large-QP family).  Oracle: each QP ALONE (batch of one, one thread), per_qp=True, stall_policy=1.

Checks, gates and the worst figure measured over all of CASES (the host-thread emulator | one MI355X):

  1. iterates after k = 1, 2, 3, 5, 8 iterations (maxIter = k, eps = 1e-12): zhat, nu, lam, slacks as
     max |a - ref| / max(1, max |ref|) per QP, `iters` equal.  k = 1 returns the start point (batch.py:61-90).
     Gate TOL = 1e-6, the project's gate (README).                      measured: 3.3e-9 | 3.3e-9, both at (20, 170, 2) knob 3
     best_resid of the same launches is a sum of the numbers of check 2's trace and is compared as they are:
     |a - ref| / max(1, |ref|) <= 1e-6, and the plain relative difference <= 1e-6 where |ref| >= 1e-3 (measured on
     the emulator's case list 9.6e-10 and 1.6e-8 | on the MI355X over all of CASES 2.9e-9 and 2.8e-8 at (33, 112, 7) knob 3).
     Below 1e-3 the plain relative difference is recorded, not gated: it is <= 2.5e-7 down to best_resid = 1.7e-6, and
     1.1e-6 .. 0.85 at the 50 of 535 (case, k) whose capped run has come to best_resid <= 6.2e-8 (k = 8 at eight shapes, k = 5
     too at (1, 1, 0)) -- there the two sides differ by 1e-15 .. 1e-13 absolute, the round-off of an iterate that agrees to
     1e-12, which no two correct codes share (the library's dual residual is an exact zero by construction there, the
     oracle's the round-off of Q z + p + G' lam + A' nu).
  2. eps = 1e-8: `iters` equal to the oracle's for every QP; trace[:iters] (pri_resid, dual_resid, mu) as
     |a - ref| / max(1, |ref|) <= 1e-6 (measured 1.7e-8 | 1.7e-8 at (100, 50, 10)); the plain relative difference over the
     entries with |ref| >= 1e-3 <= TRACE_REL = 100 x the emulator's worst, 1.979e-7 at (120, 100, 10) (the rule: 1e-6 had the
     emulator's worst been below 1e-8; it is not, and the MI355X measures the same 1.979e-7; next: 1.2e-7 at (100, 50, 10),
     every form); the rows of the NaN-filled trace buffer from `iters` on are still NaN.
  3. best-iterate bookkeeping (no reference): best_resid = min over the recorded iterations of pri + dual + nineq mu
     (batch.py:118-140; oracle/qp_oracle.c forms `resid` the same way, qpo_forward) to 1e-12 relative (measured 0 | 2.2e-16),
     and the launch capped at that iteration returns the same zhat, lam, slacks bit for bit.
  4. stall_policy = 0 with the stop rule out of reach runs maxIter passes exactly, sets QPX_ST_MAXITER on every QP and
     returns finite numbers (check_no_stall_counter: why out of reach is eps = 0 and what is asserted at eps = 1e-30).
     Counts at the default eps = 1e-12 are round-off in the end game and differ between forms and from the oracle: they
     are recorded (`counts`), not asserted -- on the MI355X e.g. (100, 100, 0) 16 / 20 / 16 passes against the oracle's
     12 / 13 / 13, (130, 70, 5) 13 / 11 / 11 against 17 / 17 / 15; equal at (1, 1, 0), (12, 9, 3), (16, 16, 0), (20, 24, 3), (20, 40, 4).
  5. float32 tensors in float64 arithmetic (QPX_F32_WIDE) at k = 2, 5 against the oracle on the float32-rounded data: 1e-5,
     the gate of that path in tests/test_gpu_parity.py (the outputs are rounded to float32: 6e-8 of their scale).
                                                                        measured: 5.1e-8 | 5.1e-8 at (100, 100, 0)
The range role's counterpart of check 1 is range_checks.check_iterates_after_k (measured 1.2e-13 | 1.2e-13).

What the gates see (scratch builds of the emulator, never committed): Mehrotra's exponent 3 -> 2 in qpx_grid.h's hard loop
makes check 1 fail at every case that runs it with 6e-2 .. 1.1 (gate 1e-6) and check 2 at every one by its counts or its
trace -- except (1, 1, 0), where one row's affine step ends on the boundary and sigma is 0 under either exponent; the step
damping 0.999 -> 0.99 there: every case, (1, 1, 0) included, 1e-2 .. 0.25.  The same two changes in qpx_big.h: every knob-3
case and (120, 100, 10), 5e-2 .. 0.18 and 1.6e-2 .. 0.16.  The start point (k = 1) stays at <= 4e-10 under all four.

scripts/check_loop.py runs all of it on the GPU and writes `measured` and `counts` to profiles/loop_trajectory.json.
"""
import functools

import numpy as np
import torch

import problems

TOL = 1e-6
TOL_WIDE = 1e-5
TRACE_REL = 100 * 1.979e-7          # 100 x the emulator's worst (at (120, 100, 10)): it is above 1e-8, see the docstring
SEED = 11
KS = (1, 2, 3, 5, 8)
# include/qpx.h, qpx_set_ipm_variant; the list of tests/test_gpu_parity.py and tests/test_emu_parity.py (both runners assert
# that it still is): 3 = the large-QP family forced at a small size, +256 / +512 = the 16x16 / 8x8 thread grid, +1024 =
# matrix-core tiles with 1 / 2 / 4 waves per QP (+2048 / +4096 / +8192); 0 = what the dispatcher picks.  A form that does not
# serve a shape falls through to another one: nothing here asserts which kernel ran.
LOOP_FORMS = [3, 256, 512, 1024 + 2048, 1024 + 4096, 1024 + 8192]
FORMS = [0] + LOOP_FORMS
SHAPES = [                # (n, m, q)
    (1, 1, 0),            # smallest
    (12, 9, 3),           # one tile row, one slot
    (16, 16, 0),          # exact tile edge
    (65, 17, 0),          # two tile rows, two slots, both edges + 1
    (20, 24, 3),          # two tile rows
    (20, 40, 4),          # four tile rows
    (64, 64, 0),          # the C5 shape, exact edges
    (100, 50, 10),        # C3
    (100, 100, 0),        # C2
    (33, 112, 7),         # seven rows, full; n + q at the matrix-core pre-factorisation's lower edge
    (130, 70, 5),         # seven rows, four slots
    (130, 9, 0),          # four slots beside one tile row
    (70, 12, 0),          # two slots beside one tile row
    (40, 130, 0),         # thread grid, 10 blocks
    (20, 170, 2),         # thread grid, 13 blocks
]
BIG = (120, 100, 10)      # the large-QP family at its natural size: n + q + m = 230 > 208; knob 0 only
CASES = [(s, f) for s in SHAPES for f in FORMS] + [(BIG, 0)]
# the emulator runs a GPU thread as a fibre: all of CASES is five minutes there, so every form at six shapes (one, two, four
# and seven tile rows, one to four slots, exact edges) and the default form at the others; the GPU runs all of CASES
EMU_ALL_FORMS = [(12, 9, 3), (65, 17, 0), (20, 40, 4), (64, 64, 0), (100, 100, 0), (130, 70, 5)]
EMU_CASES = [(s, f) for s, f in CASES if f == 0 or s in EMU_ALL_FORMS]
WIDE_SHAPES = [(100, 100, 0), (12, 9, 3)]
WIDE_KS = (2, 5)
ONE_WAVE_SHAPE, ONE_WAVE_B, ONE_WAVE_STEP = (20, 40, 4), 520, 40      # beyond 512 QPs the default dispatch goes to one wave per QP

measured = {}        # check name -> worst figure seen (scripts/check_loop.py writes them to profiles/loop_trajectory.json)
counts = {}          # shape -> iteration counts at eps = 1e-12 of the library's default form and of the oracle (check 4)


def note(key, value):
    measured[key] = max(float(value), measured.get(key, 0.0))
    print("%-44s %.3e" % (key, value))


def tag(shape, form=0):
    return "%dx%dx%d/%d" % (tuple(shape) + (form,))


def batch_of(shape, form, B=None):
    """three QPs wherever QPs may share a workgroup or a launch's grid; the large-QP family works on each QP by itself.
    B: the caller's own batch size (tests/big_checks.py)"""
    if B is not None:
        return B
    return 2 if (form == 3 or tuple(shape) == BIG) else 3


def host(t):
    return t.detach().cpu().numpy()


def fig(a, ref):
    """max |a - ref| / max(1, max |ref|) of one QP's vector"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / max(1.0, np.abs(ref).max())) if ref.size else 0.0


@functools.lru_cache(maxsize=None)
def problem(shape, B, dtype="f64", prob="prof"):
    """prof_qp in float64 (prob = "dense": problems.random_dense_qp); "f32": the same data rounded to float32 (returned as
    float64 arrays: what the oracle is given)"""
    arrs = (problems.random_dense_qp if prob == "dense" else problems.prof_qp)(B, *shape, seed=SEED)
    if dtype == "f32":
        arrs = tuple(np.asarray(np.asarray(x, np.float32), np.float64) for x in arrs)
    for x in arrs:
        x.setflags(write=False)
    return arrs


@functools.lru_cache(maxsize=None)
def oracle(shape, B, i, eps, maxIter, want_trace=False, dtype="f64", prob="prof"):
    """QP i of the batch ALONE (one thread: microseconds of work each), the loop of batch.py:47-207 with the per-QP stop rule
    and the reference's stall counter: (x, y, z, s, info).  Computed once per (problem, setting), shared by every form."""
    from oracle import qp_oracle as orc
    Q, p, G, h, A, b = problem(shape, B, dtype, prob)
    q = shape[2]
    o = orc.OracleQP(Q[i:i + 1], p[i:i + 1], G[i:i + 1], h[i:i + 1], A[i:i + 1] if q else None, b[i:i + 1] if q else None,
                     nthreads=1)
    return o.forward(eps, maxIter, 3, True, 1, want_trace=want_trace)


def factors(env, shape, B, dtype="f64", prob="prof"):
    """(fac, p, h, b) on env.dev; call inside env.run(form)"""
    from qpth_amd.kkt import KKTFactors
    td = torch.float64 if dtype == "f64" else torch.float32
    Q, p, G, h, A, b = [torch.tensor(np.asarray(x), dtype=td, device=env.dev) if np.size(x) else
                        torch.empty(0, dtype=td, device=env.dev) for x in problem(shape, B, dtype, prob)]
    return KKTFactors.build(Q, G, A, B, wide=(dtype == "f32")), p, h, b


# ---------------------------------------------------------------- 1. the iterates after k iterations
def compare_iterates(res, shape, B, k, dtype="f64", qps=None, prob="prof"):
    """the launch's best iterate against the oracle capped at the same k, over the chosen QPs: the worst figure of the
    iterates, and best_resid's as the trace's numbers are compared in check 2 (it is their sum): |a - ref| / max(1, |ref|), and
    the plain relative difference where |ref| >= 1e-3; below that the plain relative difference is only kept for the record"""
    q = shape[2]
    z, lam, s, it, best = host(res.zhat), host(res.lam), host(res.slacks), host(res.iters), host(res.best_resid)
    nu = host(res.nu) if q else None
    out = {"iterates": 0.0, "best": 0.0, "best_rel": 0.0, "best_rel_small": 0.0}
    for i in (range(B) if qps is None else qps):
        x, y, zr, sr, info = oracle(shape, B, i, 1e-12, k, False, dtype, prob)
        assert it[i] == info["iters"][0], (i, k, it, info["iters"])
        f = [fig(z[i], x[0]), fig(lam[i], zr[0]), fig(s[i], sr[0])]
        if q:
            f.append(fig(nu[i], y[0]))
        out["iterates"] = max(out["iterates"], max(f))
        ref = float(info["best_resid"][0])
        assert np.isfinite(best[i]) and ref > 0
        out["best"] = max(out["best"], abs(best[i] - ref) / max(1.0, ref))
        key = "best_rel" if ref >= 1e-3 else "best_rel_small"
        out[key] = max(out[key], abs(best[i] - ref) / ref)
    return out


_runs = {}           # (device type, shape, form) -> the capped launches' figures


def iterates_run(env, shape, form, ks=KS, B=None, prob="prof"):
    key = (env.dev.type, tuple(shape), form) + (() if (ks, B, prob) == (KS, None, "prof") else (tuple(ks), B, prob))
    if key not in _runs:
        B = batch_of(shape, form, B)
        out = {}
        with env.run(form):
            fac, p, h, b = factors(env, shape, B, prob=prob)
            for k in ks:
                out[k] = compare_iterates(fac.ipm(p, h, b, eps=1e-12, maxIter=k, stall_policy=1), shape, B, k, prob=prob)
        _runs[key] = out
    return _runs[key]


def gate_iterates(name, out, tol=TOL):
    """note and assert the figures of compare_iterates over the k of one case"""
    worst = {f: max(v[f] for v in out.values()) for f in ("iterates", "best", "best_rel", "best_rel_small")}
    note("iterates/" + name, worst["iterates"])
    note("best_resid_k/" + name, worst["best"])
    note("best_resid_k_rel/" + name, worst["best_rel"])
    note("best_resid_k_rel_below_1e-3/" + name, worst["best_rel_small"])          # (the record only: round-off near the optimum)
    assert max(worst["iterates"], worst["best"], worst["best_rel"]) <= tol, out


def check_iterates_after_k(env, shape, form=0, ks=KS, B=None, prob="prof"):
    gate_iterates(tag(shape, form), iterates_run(env, shape, form, ks, B, prob))


def one_wave_run(env):
    """B = 520 at four tile rows: the capped launches' figures on every 40th QP and the launch at eps = 1e-8"""
    key = (env.dev.type, ONE_WAVE_SHAPE, "B%d" % ONE_WAVE_B)
    if key not in _runs:
        shape, B = ONE_WAVE_SHAPE, ONE_WAVE_B
        out = {}
        with env.run(0):
            fac, p, h, b = factors(env, shape, B)
            for k in KS:
                out[k] = compare_iterates(fac.ipm(p, h, b, eps=1e-12, maxIter=k, stall_policy=1), shape, B, k,
                                          qps=range(0, B, ONE_WAVE_STEP))
            _runs[key] = (out, fac.ipm(p, h, b, eps=1e-8, stall_policy=1, want_trace=True))
    return _runs[key]


def check_one_wave_beyond_512(env):
    """B = 520 at four tile rows: the default dispatch's one-wave form; every 40th QP against the oracle"""
    shape, B = ONE_WAVE_SHAPE, ONE_WAVE_B
    out, res = one_wave_run(env)
    gate_iterates("%s/B%d" % (tag(shape), B), out)
    tr = compare_trace(res, shape, B, 20, qps=range(0, B, ONE_WAVE_STEP))
    note("trace/%s/B%d" % (tag(shape), B), tr[0])
    note("trace_rel/%s/B%d" % (tag(shape), B), tr[1])
    assert tr[0] <= TOL and tr[1] <= TRACE_REL, tr


# ---------------------------------------------------------------- 2. iteration counts and the trace at eps = 1e-8
def compare_trace(res, shape, B, maxIter, qps=None, prob="prof"):
    """`iters` equal; trace[:iters] against the oracle's: (worst |a - ref| / max(1, |ref|), worst relative difference over
    |ref| >= 1e-3); the buffer's rows from `iters` on untouched"""
    it, tr = host(res.iters), host(res.trace)
    assert tr.shape == (maxIter, B, 3)
    worst, rel = 0.0, 0.0
    for i in (range(B) if qps is None else qps):
        info = oracle(shape, B, i, 1e-8, maxIter, True, "f64", prob)[4]
        assert it[i] == info["iters"][0], (i, it, info["iters"])
        mine, ref = tr[:it[i], i], info["trace"][:it[i]]
        assert np.isfinite(mine).all() and np.isfinite(ref).all()
        assert np.isnan(tr[it[i]:, i]).all(), (i, it[i], tr[it[i]:, i])          # nothing written past the stop
        worst = max(worst, float((np.abs(mine - ref) / np.maximum(1.0, np.abs(ref))).max()))
        big = np.abs(ref) >= 1e-3
        if big.any():
            rel = max(rel, float((np.abs(mine - ref)[big] / np.abs(ref)[big]).max()))
    return worst, rel


def run_to_1e8(env, shape, form, B=None, prob="prof"):
    """the run of checks 2 and 3: (fac, p, h, b, B, result); call inside env.run(form)"""
    B = batch_of(shape, form, B)
    fac, p, h, b = factors(env, shape, B, prob=prob)
    return fac, p, h, b, B, fac.ipm(p, h, b, eps=1e-8, maxIter=20, stall_policy=1, want_trace=True)


def check_counts_and_trace(env, shape, form=0, B=None, prob="prof"):
    with env.run(form):
        fac, p, h, b, B, res = run_to_1e8(env, shape, form, B, prob)
    worst, rel = compare_trace(res, shape, B, 20, prob=prob)
    note("trace/" + tag(shape, form), worst)
    note("trace_rel/" + tag(shape, form), rel)
    assert worst <= TOL, worst
    assert rel <= TRACE_REL, rel


# ---------------------------------------------------------------- 3. the best iterate's bookkeeping
def check_best_iterate(env, shape, form=0, B=None, prob="prof"):
    m = shape[1]
    with env.run(form):
        fac, p, h, b, B, res = run_to_1e8(env, shape, form, B, prob)
        it, tr, best = host(res.iters), host(res.trace), host(res.best_resid)
        outs = [host(x) for x in (res.zhat, res.lam, res.slacks)]
        worst = 0.0
        for i in range(B):
            resid = tr[:it[i], i, 0] + tr[:it[i], i, 1] + m * tr[:it[i], i, 2]
            worst = max(worst, abs(best[i] - resid.min()) / resid.min())
            # the launch that stops right behind that iteration returns it (every QP of the batch runs; QP i is looked at)
            again = fac.ipm(p, h, b, eps=1e-8, maxIter=int(resid.argmin()) + 1, stall_policy=1)
            for a, x in zip(outs, (again.zhat, again.lam, again.slacks)):
                assert np.array_equal(a[i], host(x)[i]), (i, int(resid.argmin()), it[i])
    note("best_resid/" + tag(shape, form), worst)
    assert worst <= 1e-12, worst


# ---------------------------------------------------------------- 4. stall_policy = 0; the counts at eps = 1e-12
def check_no_stall_counter(env, shape, form=0, maxIter=20, B=None, prob="prof"):
    """Without the stall counter and with the stop rule's best_resid < eps out of reach the loop runs maxIter passes exactly,
    says QPX_ST_MAXITER for every QP and returns finite numbers.  Out of reach is eps = 0: at eps = 1e-30 it is not -- on small
    QPs both residual norms come out as exact zeros and nineq mu falls by 1e3 per pass, so best_resid does get below 1e-30
    (at (1, 1, 0) after 11 or 12 passes, in oracle/qp_oracle too).  At eps = 1e-30 therefore: a QP that stopped early, or at
    maxIter without the bit, is one whose best_resid is below 1e-30 -- nothing else may end the loop."""
    from qpth_amd import _lib
    B = batch_of(shape, form, B)
    with env.run(form):
        fac, p, h, b = factors(env, shape, B, prob=prob)
        res = fac.ipm(p, h, b, eps=0.0, maxIter=maxIter, stall_policy=0)
        # (status words accumulate on the factors: fresh ones for the second launch)
        fac30, p, h, b = factors(env, shape, B, prob=prob)
        r30 = fac30.ipm(p, h, b, eps=1e-30, maxIter=maxIter, stall_policy=0)
    assert np.array_equal(host(res.iters), np.full(B, maxIter)), host(res.iters)
    assert (host(res.status) & _lib.ST_MAXITER).all(), host(res.status)
    ran_out = (host(r30.iters) == maxIter) & ((host(r30.status) & _lib.ST_MAXITER) != 0)
    assert (ran_out | (host(r30.best_resid) < 1e-30)).all(), (host(r30.iters), host(r30.status), host(r30.best_resid))
    assert (host(r30.status) & (_lib.ST_KKT_BREAKDOWN | _lib.ST_NONFINITE) == 0).all(), host(r30.status)
    for r in (res, r30):
        for x in (r.zhat, r.lam, r.slacks, r.best_resid) + ((r.nu,) if shape[2] else ()):
            assert np.isfinite(host(x)).all()


def record_counts(env, shape):
    """eps = 1e-12, the reference's stall counter, the default form: an observation for the record, not a gate"""
    B = batch_of(shape, 0)
    with env.run(0):
        fac, p, h, b = factors(env, shape, B)
        mine = host(fac.ipm(p, h, b, eps=1e-12, maxIter=20, stall_policy=1).iters)
    ref = [int(oracle(shape, B, i, 1e-12, 20)[4]["iters"][0]) for i in range(B)]
    counts["%dx%dx%d" % tuple(shape)] = {"library": [int(v) for v in mine], "oracle": ref}
    print("iters at eps=1e-12 %-12s library %s oracle %s" % ("%dx%dx%d" % tuple(shape), [int(v) for v in mine], ref))
    assert (mine >= 1).all() and (mine <= 20).all()


# ---------------------------------------------------------------- 5. float32 tensors in float64 arithmetic
def check_wide_iterates(env, shape, B=None):
    B = batch_of(shape, 0, B)
    worst = {}
    with env.run(0):
        fac, p, h, b = factors(env, shape, B, "f32")
        assert fac.blob.dtype == torch.float64
        for k in WIDE_KS:
            res = fac.ipm(p, h, b, eps=1e-12, maxIter=k, stall_policy=1)
            assert res.zhat.dtype == torch.float32
            worst[k] = compare_iterates(res, shape, B, k, "f32")
    note("wide/" + tag(shape), max(max(v["iterates"], v["best"], v["best_rel"]) for v in worst.values()))
    assert max(max(v["iterates"], v["best"], v["best_rel"]) for v in worst.values()) <= TOL_WIDE, worst
