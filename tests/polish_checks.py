"""The FINISHING role of the finishing-stage kernels (qpx_polish; polish_mat_role of qpth_amd/csrc/qpx_grid.h, big_polish_body of
qpx_big_polish.h) STEP BY STEP in every form: the checks that tests/test_emu_polish.py runs on the host-thread
emulator and tests/test_gpu_polish.py on a real MI355X.  Every check takes an `env`: env.dev (the torch device) and
env.run(variant=0), a context manager around the library calls (the A/B knob of include/qpx.h, qpx_set_ipm_variant).  Every
launch goes through the ctypes layer's `polish` directly (KKTFactors.polish passes no best_resid).

A finishing step corrects itself as the loop does: with a wrong sigma exponent, damping, step-length rule, `rs` of the affine
solve or best-iterate comparison it still lands near the optimum, and the end-to-end float32 gates (1e-5 and looser) cannot see
it.  These compare the iterate after k steps with tests/polish_step_reference.py: one iteration of the reference's loop
(batch.py:92-198) in numpy, np.longdouble residuals and iterate, both KKT solves through kkt_checks.Dense (a dense float64 LU
refined in np.longdouble, held against mpmath by tests/test_kkt_reference.py) -- nothing of it is built from the library.
tests/test_polish_reference.py ties a step of it to oracle/qp_oracle's iterates (1e-9).

Start iterates.  Regular: per QP, oracle/qp_oracle's iterate after three iterations (loop_checks.oracle, maxIter = 3); QPX_F32:
its float32 rounding, on the float32-rounded data.  Ill-centred (ILL): ONE QP of the batch -- the others keep their regular
start -- gets, from the reference's own iterate (x*, s*, lam*, nu*) after eight further steps, "swap" s = max(lam*, 1e-3),
lam = max(s*, 1e-3); "sq" s = 1e-4 s* + 1e-10, lam = lam* + 1; "flat" s = 1e-6, lam = 1.  Before the library is called every
case asserts on the reference alone that each comparison of totals that decides which iterate comes back differs by
>= MARGIN = 1e-3 relative (`decisive`): no case sits near a tie.

Cases (CASES; batches of three QPs, two in the large-QP family, loop_checks.batch_of) and the form of api_polish's rule each
reaches (form_of restates the rule; nothing asserts which kernel ran beyond the *_supported queries):

  float64, knob 0    tile (1,1)        (1,1,0) (12,9,3) (16,16,0)     tile (2,1)        (20,24,3) (65,17,0)
                     tile (4,4,chain)  (20,40,4) (64,64,0) (100,50,10) tile (7,4,chain)  (100,100,0) (33,112,7)
                     tile (4,1)        (20,40,4) at B = 8200, GPU only (polish_tile_chain: one wave beyond 8192 QPs)
                     grid 10           (40,130,0) (16,113,0)          grid 13           (20,170,2)
                     large-QP family   (120,100,10) (130,100,0) (280,70,6)
  float64, knob 256  grid 1, 2, 4, 7   (12,9,3) (20,24,3) (20,40,4) (100,100,0)
  float64, knob 3    large-QP family   (12,9,3) (130,70,5)
  QPX_F32, knob 0    grid 1 .. 13      kkt_checks.F32_SHAPES on problems.random_dense_qp
  QPX_F32, knob 3    large-QP family   (70,66,3) on problems.random_dense_qp

Checks, gates and the worst figure measured (the host-thread emulator | one MI355X); the error measure is loop_checks.fig,
max |a - ref| / max(1, max |ref|) per output array and per QP:

  1. iterates after k = 1, 2, 3 steps at refine = 0, and k = 2 at refine = 1, 2 (not the large-QP family: it refuses
     refine > 0): zhat, lam, slacks, nu against the reference, gate loop_checks.TOL = 1e-6, the project's gate.
     best_resid as loop_checks check 1: |a - ref| / max(1, |ref|) <= 1e-6, plain relative <= 1e-6 where ref >= 1e-3.
     The reference-side figure (the same numpy steps with the float64 LU alone against the refined ones) is recorded for
     every case in `reference_side`; NO float64 case of check 1 needed the conditioning rule (COND_RULE is empty).
  2. QPX_F32 against the reference on the float32-rounded data: gate max(1e-3, 100 x the figure of the numpy steps with both
     solves done by a float32 dense solve, against the refined reference) -- kkt_checks' float32 rule.
  3. the best-iterate rule on ILL (the gates and the 100-gate distance concern the QP with the ill-centred start).  "never": all four outputs the inputs bit for bit at steps = 1, 2, 3, best_resid the start's
     total.  "then": the returned iterate is the reference's best one (steps = 2 and 3 return different ones at "sq"), gate
     max(1e-6, 100 x the float64-LU figure) (d spans many decades: recorded in rule_decided whether the rule decided),
     best_resid its total; asserted on the reference first: every other iterate is >= 100 x the gate away from the best.
  4. steps = 0: outputs bitwise the inputs, best_resid the start's total to check 1's gate.
  5. p, h, b un-batched (stride 0), and Q, G, A shared with one blob (sfac = 0), each separately at (12,9,3) and (100,50,10):
     bitwise the expanded batch, and held to the reference.  The large-QP family answers QPX_ERR_ARG to shared factors at B > 1.
  6. a NaN in lam of QP 1 of three (one tile form, one grid form, the large-QP family): QPs 0 and 2 bitwise what they are
     without it, their status words unchanged; QP 1's outputs its inputs bit for bit, its best_resid +inf.
  7. outputs allocated with one spare row on each side (NaN-filled): unchanged after the call, at (1,1,0), (16,16,0),
     (65,17,0), (33,112,7).
  8. qpx_polish_supported and the error codes: QPX_F32_WIDE and max dimension 513 unsupported; refine > 0 on the large-QP
     family QPX_ERR_UNSUPPORTED.

Worst figures measured (the host-thread emulator | one MI355X; every figure: profiles/polish_steps.json):

  check 1, float64, all of CASES: iterates 1.9e-11 | 1.9e-11, best_resid 4.0e-10 | 4.0e-10 (plain relative the same), all three at
  (33, 112, 7) k = 3, tile (7,4,chain); the thread grid's worst 7.5e-12 at (20, 170, 2), the large-QP family's 1.6e-13 (best_resid 8.6e-12).  The
  reference-side figure (float64 LU alone) is <= 2.4e-13 over these cases: nothing is near 1e-6, no gate rests on the rule.
  tile (4,1) at B = 8200 (MI355X only): iterates 1.9e-13, best_resid 2.0e-12; against the chain form's answer 1.1e-14 (gate 1e-9).
  check 2, QPX_F32: iterates 1.1e-5 | 1.1e-5 at (20, 170, 2) (gate there 1.4e-3 | 1.3e-3: the float32 dense solve has 1.4e-5 on
  the emulator's host; the rule also decides at (60, 112, 0), and at (40, 130, 0) on the MI355X's host), best_resid 3.3e-5; its plain
  relative figure 5.8e-4 | 5.8e-4 at (20, 24, 3) k = 3 against 1e-3 -- the total there is 2e-3 and an iterate that agrees to
  2e-7 moves a residual by 1e-6 absolute.  The large-QP family in float32: 1.7e-6, 1.2e-5, 1.2e-4.
  check 3: "never" bit for bit at all four cases; "then" 9.1e-12 | 9.3e-12 at (100, 50, 10) "flat" (gate there 1.3e-6 on the
  emulator's host: the float64 LU alone has 1.3e-8 with d over twelve decades -- the one float64 gate a rule decided here; on the MI355X's
  host it also decides at (130, 70, 5) "flat").  The reference's other iterates are >= 0.18 from the returned one.
  checks 4-7: best_resid at steps = 0 5.9e-15; stride-0 p, h, b and shared factors bitwise the expanded batch on both, 1.4e-12 and
  5.6e-13 from the reference; the NaN and spare-row checks hold bit for bit in every family, so include/qpx.h needed no word.
  Counts and wall time: tests/test_emu_polish.py 84 tests in 38 s (the longest, (280, 70, 6), 6 s);
  tests/test_gpu_polish.py 85 tests in 3.1 s on one MI355X, the references included (the longest test 0.2 s).

What the gates see (scratch builds of the emulator, never committed; all of scripts/check_polish.py --emu on each):
  - polish_mat_role, sigma exponent 3 -> 2: checks 1 and 2 at 22 of the 23 thread-grid / tile cases (not (1, 1, 0): the affine
    step ends on the boundary, sigma is 0 under either exponent), iterates 1.9e-5 .. 0.17 (gate 1e-6), QPX_F32 1.2e-3 .. 0.12;
    check 3 at six cases 5.2e-4 .. 0.11; the stride, shared-factor and spare-row cases with them.
  - the damping 0.999 -> 0.99: the same 22 cases, 2.3e-4 .. 1.2, QPX_F32 1.5e-3 .. 2.7e-2; check 3 3.5e-3 .. 1.0.
  - the affine solve's rs = z replaced by s: all 23 cases, 2.5e-5 .. 3.2 (best_resid up to 2.6e2), QPX_F32 0.10 .. 2.2; check 3
    at all eight thread-grid / tile cases ("never" included: a step now helps where none should).
  - `tot < best` always true: check 3 at all eight thread-grid / tile cases, 0.43 .. 1.2e5 (best_resid 2e-3 .. 4.1e6), and check 6
    at both (the NaN iterate is handed back as "best"); of checks 1 and 2 one case.  `tot <= best` changes no output bit: it
    differs from `<` only where two totals are EQUAL, which is a step of length 0 -- the same iterate either way.
  - the write-back of lam without row m - 1: checks 1, 2, 3, 5, 7 at every thread-grid / tile case, 1.5e-6 (at (1, 1, 0)) .. 0.99;
    the arrays are updated in place, so the unwritten entry is the START's value of that row, not a NaN.  On a "never" QP itself
    the omission is invisible (its output is its input): those cases fail through the other QPs of their batch.
  - qpx_big_polish.h, sigma exponent 3 -> 2: all six large-family cases of checks 1 and 2, 1.7e-4 .. 0.11 (QPX_F32 7.3e-3 ..
    4.1e-2), check 3 at both "then" cases, the stride case; the damping 0.999 -> 0.99: the same, 1.3e-4 .. 0.22 and 5.5e-3 .. 1.2.

scripts/check_polish.py runs all of it on the GPU (--emu: on the emulator) and writes every figure, its gate and the
reference-side figures to profiles/polish_steps.json.
"""
import numpy as np
import pytest
import torch

import kkt_checks as K
import loop_checks as L
import polish_step_reference as R

LD = np.longdouble
TOL = L.TOL                # 1e-6, the project's gate
TOL_F32 = K.TOL_F32        # 1e-3, the floor of kkt_checks' float32 rule
MARGIN = 1e-3              # every deciding pair of reference totals differs by this much, relative
KS = (1, 2, 3)
REFINES = (1, 2)           # at k = 2
GRID16 = 256               # the A/B knob: the 16x16 thread grid where the tile kernels would serve the size
BIGK = 3                   # ... the large-QP family at every size
fig, tag, batch_of, host = L.fig, L.tag, L.batch_of, L.host

TILE_SHAPES = [(1, 1, 0), (12, 9, 3), (16, 16, 0), (20, 24, 3), (65, 17, 0), (20, 40, 4), (64, 64, 0), (100, 50, 10), (100, 100, 0), (33, 112, 7)]
GRID_SHAPES = [(40, 130, 0), (16, 113, 0), (20, 170, 2)]
KNOB256_SHAPES = [(12, 9, 3), (20, 24, 3), (20, 40, 4), (100, 100, 0)]
BIG_KNOB3_SHAPES = [(12, 9, 3), (130, 70, 5)]
BIG_SHAPES = [(120, 100, 10), (130, 100, 0), (280, 70, 6)]
F32_SHAPES = list(K.F32_SHAPES)
F32_BIG = (70, 66, 3)
# (shape, knob, dtype)
CASES = ([(s, 0, "f64") for s in TILE_SHAPES + GRID_SHAPES] + [(s, GRID16, "f64") for s in KNOB256_SHAPES]
         + [(s, BIGK, "f64") for s in BIG_KNOB3_SHAPES] + [(s, 0, "f64") for s in BIG_SHAPES])
F32_CASES = [(s, 0, "f32") for s in F32_SHAPES] + [(F32_BIG, BIGK, "f32")]
# the emulator runs all of it too (40 s in all; the longest case, (280, 70, 6), 6 s) -- but for B = 8200
EMU_CASES = list(CASES)
ONE_WAVE_SHAPE, ONE_WAVE_REP = (20, 40, 4), 4100        # B = 8200: beyond 8192 QPs four tile rows run one wave per QP
COND_RULE = set()          # float64 cases of check 1 held to the conditioning rule instead of TOL: none needed it
SHARED_SHAPES = [(12, 9, 3), (100, 50, 10)]
NAN_CASES = [((12, 9, 3), 0), ((12, 9, 3), GRID16), ((12, 9, 3), BIGK)]
SPARE_SHAPES = [(1, 1, 0), (16, 16, 0), (65, 17, 0), (33, 112, 7)]
# (kind, shape, knob, the QP that gets the ill-centred start, what the reference must say: "never" = the start stays the
# best through three steps; {steps: index of the returned iterate})
ILL = [
    ("swap", (1, 1, 0), 0, 1, "never"),                    # tile (1,1)
    ("swap", (1, 1, 0), GRID16, 1, "never"),               # grid 1
    ("swap", (1, 1, 0), BIGK, 0, "never"),                 # the large-QP family (a batch of two: other data)
    ("swap", (20, 170, 2), 0, 0, "never"),                 # grid 13
    ("sq", (12, 9, 3), 0, 1, {2: 1, 3: 3}),                # tile (1,1)
    ("sq", (12, 9, 3), GRID16, 1, {2: 1, 3: 3}),           # grid 1
    ("sq", (12, 9, 3), BIGK, 1, {2: 1, 3: 3}),             # the large-QP family
    ("flat", (100, 50, 10), 0, 1, {3: 2}),                 # tile (4,4,chain)
    ("flat", (100, 50, 10), GRID16, 1, {3: 2}),            # grid 4
    ("flat", (130, 70, 5), 0, 0, {3: 2}),                  # tile (7,4,chain)
    ("flat", (130, 70, 5), BIGK, 0, {3: 2}),               # the large-QP family
]

measured = {}        # "check/case" -> worst figure seen (scripts/check_polish.py writes them to profiles/polish_steps.json)
gates = {}           # the same keys -> the gate the figure was held to
reference_side = {}  # the figures behind the rules: the numpy steps with the float64 LU alone / a float32 dense solve
rule_decided = {}    # case -> did 100 x the reference-side figure exceed the constant (only the cases that ask for a rule)
forms = {}           # case -> the form api_polish's rule picks (form_of)


class Gate(K.Gate):
    def hold(self, key, value, gate):
        measured[key] = max(float(value), measured.get(key, 0.0))
        gates[key] = gate
        print("%-56s %.3e  (gate %.1e)" % (key, value, gate))
        if not value <= gate:
            self.bad.append((key, value, gate))


def name(shape, knob, dtype="f64", extra=""):
    return tag(shape, knob) + ("" if dtype == "f64" else "/" + dtype) + extra


# ---------------------------------------------------------------- which form serves a case (api_polish's rule, restated)
def form_of(shape, knob, dtype, B):
    n, m, q = shape
    if knob == BIGK or n + m + q > 208:
        return "big"
    if dtype == "f64" and m <= 112 and knob != GRID16:
        rows = K.tile_rows(m)
        chain = rows == 7 or (rows == 4 and B <= 8192)          # polish_tile_chain; ignores the knob's waves
        return "tile(%d,%d%s)" % (rows, 4 if chain else 1, ",chain" if chain else "")
    blocks = -(-m // 16)
    return "grid %d%s" % (next(b for b in (1, 2, 4, 7, 10, 13) if b >= blocks), "" if dtype == "f64" else " f32")


ALL_FORMS = (["tile(1,1)", "tile(2,1)", "tile(4,1)", "tile(4,4,chain)", "tile(7,4,chain)", "big"]
             + ["grid %d%s" % (b, s) for b in (1, 2, 4, 7, 10, 13) for s in ("", " f32")])


# ---------------------------------------------------------------- data, starts, the reference (made once, never written to)
def prob_of(dtype):
    return "prof" if dtype == "f64" else "dense"


def arrs_of(shape, B, dtype, prob=None):
    return K.problem(shape, B, dtype, prob or prob_of(dtype))


def frozen(vs):
    out = tuple(np.ascontiguousarray(v) for v in vs)
    for v in out:
        v.setflags(write=False)
    return out


def regular_start(shape, B, dtype):
    """(x, s, z, y) float64 (B, .): the oracle's iterate after three iterations, QP by QP; QPX_F32: rounded to float32"""
    def make():
        q = shape[2]
        rows = [L.oracle(tuple(shape), B, i, 1e-12, 3, False, dtype, prob_of(dtype)) for i in range(B)]
        x, y, z, s = [np.stack([np.asarray(r[j][0], np.float64) if r[j] is not None else np.zeros(0) for r in rows]) for j in range(4)]
        return frozen(K.rounded(v, dtype) for v in (x, s, z, y if q else np.zeros((B, 0))))
    return K.cached(("polish_start", tuple(shape), B, dtype), make)


def ill_start(kind, shape, B, qp):
    """the regular starts with QP `qp`'s (s, lam) replaced, from the reference's iterate after eight further steps"""
    def make():
        reg = regular_start(shape, B, "f64")
        xs, ss, zs, ys = [np.asarray(v, np.float64) for v in reference(shape, B, "f64", "regular", 8)["iterates"][8]]
        s_new, z_new = {"swap": (np.maximum(zs, 1e-3), np.maximum(ss, 1e-3)), "sq": (1e-4 * ss + 1e-10, zs + 1.0),
                        "flat": (np.full(ss.shape, 1e-6), np.ones(zs.shape))}[kind]
        x, s, z, y = [v.copy() for v in reg]
        x[qp], s[qp], z[qp], y[qp] = xs[qp], s_new[qp], z_new[qp], ys[qp]
        return frozen((x, s, z, y))
    return K.cached(("polish_ill", kind, tuple(shape), B, qp), make)


def start_of(shape, B, dtype, which):
    return regular_start(shape, B, dtype) if which == "regular" else ill_start(which[0], shape, B, which[1])


def reference(shape, B, dtype, which="regular", steps=3, solver="refined", prob=None, unbatched=False):
    """polish_step_reference.run on the case's data from the named start: made once, shared by every form"""
    def make():
        arrs = data_of(shape, B, dtype, prob, unbatched)
        return R.run(arrs, start_of(shape, B, dtype, which), steps, solver)
    return K.cached(("polish_ref", tuple(shape), B, dtype, which, steps, solver, prob, unbatched), make)


def data_of(shape, B, dtype, prob=None, unbatched=False):
    """the six arrays, batched; unbatched: p, h, b of QP 0 for every QP"""
    arrs = list(arrs_of(shape, B, dtype, prob))
    if unbatched:
        for i in (1, 3, 5):
            arrs[i] = np.broadcast_to(arrs[i][:1], arrs[i].shape).copy()
    return arrs


def returned(totals, steps):
    """(index of the iterate qpx_polish(steps) returns, its total, the smallest relative distance of a deciding comparison) per
    QP, from the totals of iterates 0 .. : strict <, the start competes, a non-finite total never wins"""
    nB = totals.shape[1]
    best, val, margin = np.zeros(nB, int), np.full(nB, np.inf, LD), np.full(nB, np.inf)
    for k in range(steps + 1):
        t = totals[k]
        if k:
            with np.errstate(invalid="ignore"):
                margin = np.minimum(margin, np.asarray(np.abs(t - val) / val, np.float64))
        better = t < val
        best, val = np.where(better, k, best), np.where(better, t, val)
    return best, val, margin


def decisive(ref, steps, label):
    """the condition on the reference alone: no deciding pair of totals is near a tie"""
    best, val, margin = returned(ref["totals"], steps)
    assert np.isfinite(np.asarray(ref["totals"][:steps + 1], np.float64)).all(), label
    assert (margin >= MARGIN).all(), ("a best-iterate decision of the reference is near a tie", label, steps, margin,
                                      np.asarray(ref["totals"], np.float64).T)
    return best, val


def side_figure(shape, B, dtype, which, solver, steps=3, prob=None, unbatched=False):
    """the numpy steps with the plain solver against the refined reference, worst over the iterates 1 .. steps"""
    a, b = reference(shape, B, dtype, which, steps, solver, prob, unbatched), reference(shape, B, dtype, which, steps, "refined", prob, unbatched)
    worst = 0.0
    for k in range(1, steps + 1):
        for u, v in zip(a["iterates"][k], b["iterates"][k]):
            worst = max(worst, max(fig(u[i], v[i]) for i in range(B)))
    return worst


def gate_of(shape, knob, dtype, B, which="regular", rule=False, prob=None, unbatched=False):
    """TOL; with `rule` (or a case of COND_RULE) kkt_checks' conditioning rule max(TOL, 100 x the float64 LU's figure); QPX_F32:
    max(1e-3, 100 x the float32 dense solve's figure).  The reference-side figure is recorded either way."""
    key = name(shape, knob if knob == BIGK else 0, dtype, "/B%d/%s" % (B, which if which == "regular" else "%s%d" % which)) + ("/" + prob if prob else "") + ("/unbatched" if unbatched else "")
    side = side_figure(shape, B, dtype, which, "lu64" if dtype == "f64" else "f32", prob=prob, unbatched=unbatched)
    reference_side[("dense64/" if dtype == "f64" else "dense32/") + key] = side
    if dtype == "f32":
        rule_decided[key] = bool(100.0 * side > TOL_F32)
        return max(TOL_F32, 100.0 * side)
    if rule or (tuple(shape), knob) in COND_RULE:
        rule_decided[key] = bool(100.0 * side > TOL)
        return max(TOL, 100.0 * side)
    return TOL


# ---------------------------------------------------------------- one launch
def tdtype(dtype):
    return torch.float64 if dtype == "f64" else torch.float32


def factors(env, shape, B, dtype, knob, prob=None, shared=False):
    """the case's factors under `knob`, built once; call inside env.run(knob)"""
    key = ("polish_fac", env.dev.type, tuple(shape), B, dtype, knob, prob, shared)
    return K.cached(key, lambda: K.build(env, arrs_of(shape, B, dtype, prob), B, dtype, shared))


def launch(env, shape, knob, dtype, B, start, steps, refine=0, prob=None, shared=False, unbatched=False, spare=0, want_best=True):
    """qpx_polish on copies of `start` (x, s, z, y): {"out": (zhat, slacks, lam, nu) host arrays, "best", "status" before and
    after, "spare": the rows allocated around every output}"""
    n, m, q = shape
    td = tdtype(dtype)
    with env.run(knob):
        fac = factors(env, shape, B, dtype, knob, prob, shared)
        arrs = data_of(shape, B, dtype, prob, unbatched)
        p, h, b = [torch.tensor(np.asarray(arrs[i][0] if unbatched else arrs[i]), dtype=td, device=env.dev) for i in (1, 3, 5)]
        bufs = []
        for v, w in zip(tuple(start) + (np.zeros((B,)),), (n, m, m, q, None)):
            full = torch.full((B + 2 * spare,) + (() if w is None else (w,)), float("nan"), dtype=td, device=env.dev)
            if w is None or w:
                full[spare:spare + B] = torch.tensor(np.asarray(v, np.float64), dtype=td, device=env.dev)
            bufs.append(full)
        x, s, z, y, best = [f[spare:spare + B] for f in bufs]
        assert all(v.is_contiguous() for v in (x, s, z, y, best))
        before = host(fac.status).copy()
        with fac._knob():
            fac.lib.polish(B, n, m, q, fac.Q, p, fac.G, h, fac.A if q else None, b if q else None, fac.blob, fac.sfac, steps, refine,
                           x, y if q else None, z, s, best if want_best else None, fac.status)
        after = host(fac.status).copy()
    return {"out": tuple(host(v).copy() for v in (x, s, z, y)), "best": host(best).copy(), "before": before, "after": after,
            "spare": [host(f).copy() for f in bufs] if spare else None}


def as_inputs(start, dtype):
    """the start as the tensors of the case's dtype hold it"""
    return tuple(np.asarray(np.asarray(v, np.float64).astype(np.float32 if dtype == "f32" else np.float64)) for v in start)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def hold_iterate(g, key, res, ref, k, val, gate, qps=None):
    """the four outputs against the reference's iterate k[i] of every QP i, and best_resid against its total"""
    B = len(k)
    worst = b_abs = b_rel = 0.0
    for i in (range(B) if qps is None else qps):
        for a, r in zip(res["out"], ref["iterates"][k[i]]):
            worst = max(worst, fig(a[i], r[i]) if np.isfinite(a[i]).all() else float("inf"))
        t, mine = float(val[i]), float(res["best"][i])
        if not np.isfinite(mine):
            b_abs = float("inf")
            continue
        b_abs = max(b_abs, abs(mine - t) / max(1.0, t))
        if t >= 1e-3:
            b_rel = max(b_rel, abs(mine - t) / t)
    g.hold("iterates/" + key, worst, gate)
    g.hold("best_resid/" + key, b_abs, gate)
    g.hold("best_resid_rel/" + key, b_rel, gate)


def no_new_bits(res, qps=None):
    sel = slice(None) if qps is None else list(qps)
    assert np.array_equal(res["before"][sel], res["after"][sel]), ("status words changed", res["before"], res["after"])


# ---------------------------------------------------------------- 1. / 2. the iterates after k steps
def check_steps(env, shape, knob=0, dtype="f64"):
    B = batch_of(shape, knob)
    n, m, q = shape
    key = name(shape, knob, dtype)
    forms[key] = form_of(shape, knob, dtype, B)
    code = 1 if dtype == "f64" else 0                        # QPX_F64 / QPX_F32
    start = regular_start(shape, B, dtype)
    ref = reference(shape, B, dtype)
    picks = {k: decisive(ref, k, key) for k in KS}
    gate = gate_of(shape, knob, dtype, B)
    g = Gate()
    with env.run(knob):
        fac = factors(env, shape, B, dtype, knob)
        assert fac.lib.dll.qpx_polish_supported(code, n, m, q) == 1, key
        refines = bool(fac.lib.dll.qpx_refine_supported(code, n, m, q))
    assert dtype == "f32" or refines == (forms[key] != "big"), (key, "qpx_refine_supported")
    for k in KS:
        res = launch(env, shape, knob, dtype, B, start, k)
        hold_iterate(g, "%s/k%d" % (key, k), res, ref, picks[k][0], picks[k][1], gate)
        no_new_bits(res)
    if refines and dtype == "f64":
        for r in REFINES:
            res = launch(env, shape, knob, dtype, B, start, 2, refine=r)
            hold_iterate(g, "%s/k2/refine%d" % (key, r), res, ref, picks[2][0], picks[2][1], gate)
            no_new_bits(res)
    g.done()


def check_one_wave_beyond_8192(env):
    """(20,40,4), the two-QP batch repeated 4100 times: tile (4,1).  The first two QPs against the reference; every QP against
    the chain form's answer for the same QP, 1e-9 (two forms, two orders of summation: tests/test_gpu_centre.py's comparison)"""
    shape, B0 = ONE_WAVE_SHAPE, 2
    n, m, q = shape
    B = B0 * ONE_WAVE_REP
    key = name(shape, 0, "f64", "/B%d" % B)
    forms[key] = form_of(shape, 0, "f64", B)
    assert forms[key] == "tile(4,1)" and form_of(shape, 0, "f64", B0) == "tile(4,4,chain)"
    from qpth_amd.kkt import KKTFactors
    arrs, start, ref = arrs_of(shape, B0, "f64"), regular_start(shape, B0, "f64"), reference(shape, B0, "f64")
    g = Gate()
    tile = lambda a: np.tile(a, (ONE_WAVE_REP,) + (1,) * (np.ndim(a) - 1))      # noqa: E731
    with env.run(0):
        Q, p, G, h, A, b = [torch.tensor(tile(a), device=env.dev) for a in arrs]
        fac = KKTFactors.build(Q, G, A, B)
        for k in KS:
            pick = decisive(ref, k, key)
            small = launch(env, shape, 0, "f64", B0, start, k)
            x, s, z, y = [torch.tensor(tile(v), device=env.dev) for v in start]
            best = torch.full((B,), float("nan"), dtype=torch.float64, device=env.dev)
            with fac._knob():
                fac.lib.polish(B, n, m, q, fac.Q, p, fac.G, h, fac.A, b, fac.blob, fac.sfac, k, 0, x, y, z, s, best, fac.status)
            res = {"out": tuple(host(v) for v in (x, s, z, y)), "best": host(best)}
            hold_iterate(g, "%s/k%d" % (key, k), res, ref, pick[0], pick[1], TOL, qps=range(B0))
            twin = max(float(np.abs(a - tile(c)).max() / max(1.0, np.abs(c).max())) for a, c in zip(res["out"], small["out"]))
            g.hold("one_wave_vs_chain/%s/k%d" % (key, k), twin, 1e-9)
            g.hold("one_wave_vs_chain_best_resid/%s/k%d" % (key, k), float(np.abs(res["best"] / tile(small["best"]) - 1).max()), 1e-9)
            assert np.isfinite(res["best"]).all()
    g.done()


# ---------------------------------------------------------------- 3. the best-iterate rule
def check_best_iterate_rule(env, kind, shape, knob, qp, expect):
    B = batch_of(shape, knob)
    which = (kind, qp)
    key = name(shape, knob, "f64", "/%s%d" % which)
    forms[key] = form_of(shape, knob, "f64", B)
    start, ref = ill_start(kind, shape, B, qp), reference(shape, B, "f64", which)
    gate = gate_of(shape, knob, "f64", B, which, rule=True)
    g = Gate()
    for steps in ((1, 2, 3) if expect == "never" else sorted(expect)):
        best, val = decisive(ref, steps, key)
        assert best[qp] == (0 if expect == "never" else expect[steps]), ("the reference does not give this case's pattern", key, steps, best,
                                                                          np.asarray(ref["totals"], np.float64).T)
        # the comparison identifies WHICH iterate came back: every other one is 100 gates away from it
        for j in range(steps + 1):
            if j != best[qp]:
                far = max(fig(u[qp], v[qp]) for u, v in zip(ref["iterates"][j], ref["iterates"][best[qp]]))
                assert far >= 100 * gate, (key, steps, j, far)
        res = launch(env, shape, knob, "f64", B, start, steps)
        hold_iterate(g, "rule/%s/steps%d" % (key, steps), res, ref, best, val, gate)
        if best[qp] == 0:
            for a, s0 in zip(res["out"], start):
                assert same_bits(a[qp], s0[qp]), ("a step that did not help was kept", key, steps)
        no_new_bits(res)
    g.done()


# ---------------------------------------------------------------- 4. steps = 0
def check_zero_steps(env, shape, knob=0, dtype="f64"):
    B = batch_of(shape, knob)
    key = name(shape, knob, dtype)
    start, ref = regular_start(shape, B, dtype), reference(shape, B, dtype)
    res = launch(env, shape, knob, dtype, B, start, 0)
    for a, s0 in zip(res["out"], as_inputs(start, dtype)):
        assert same_bits(a, s0), key
    g = Gate()
    hold_iterate(g, key + "/k0", res, ref, np.zeros(B, int), ref["totals"][0], gate_of(shape, knob, dtype, B))
    no_new_bits(res)
    g.done()


# ---------------------------------------------------------------- 5. strides and shared factors
def check_unbatched_phb(env, shape, knob=0):
    B = batch_of(shape, knob)
    key = name(shape, knob, "f64", "/unbatched")
    start, ref = regular_start(shape, B, "f64"), reference(shape, B, "f64", unbatched=True)
    g = Gate()
    for k in (1, 3):
        best, val = decisive(ref, k, key)
        one = launch(env, shape, knob, "f64", B, start, k, unbatched=True)
        each = launch_expanded_phb(env, shape, knob, B, start, k)
        for a, e in zip(one["out"] + (one["best"],), each["out"] + (each["best"],)):
            assert same_bits(a, e), ("stride-0 p, h, b against the expanded batch", key, k)
        hold_iterate(g, "%s/k%d" % (key, k), one, ref, best, val, gate_of(shape, knob, "f64", B, unbatched=True))
    g.done()


def launch_expanded_phb(env, shape, knob, B, start, k):
    """the launch of check_unbatched_phb with p, h, b expanded to dense (B, .) arrays of equal rows"""
    n, m, q = shape
    with env.run(knob):
        fac = factors(env, shape, B, "f64", knob)
        arrs = data_of(shape, B, "f64", None, True)
        p, h, b = [torch.tensor(np.asarray(arrs[i]), device=env.dev) for i in (1, 3, 5)]
        assert p.stride(0) == n
        x, s, z, y = [torch.tensor(np.asarray(v), device=env.dev) for v in start]
        best = torch.full((B,), float("nan"), dtype=torch.float64, device=env.dev)
        with fac._knob():
            fac.lib.polish(B, n, m, q, fac.Q, p, fac.G, h, fac.A if q else None, b if q else None, fac.blob, fac.sfac, k, 0,
                           x, y if q else None, z, s, best, fac.status)
    return {"out": tuple(host(v).copy() for v in (x, s, z, y)), "best": host(best).copy()}


def check_shared_factors(env, shape):
    """Q, G, A shared and ONE blob (sfac = 0): bitwise the expanded batch's, and held to the reference"""
    B = batch_of(shape, 0)
    key = name(shape, 0, "f64", "/shared")
    start, ref = regular_start(shape, B, "f64"), reference(shape, B, "f64", prob="shared")
    g = Gate()
    with env.run(0):
        one, each = factors(env, shape, B, "f64", 0, "shared", True), factors(env, shape, B, "f64", 0, "shared", False)
        assert one.shared and one.sfac == 0 and one.blob.numel() == one.elems and each.sfac == each.elems
    for k in (1, 3):
        best, val = decisive(ref, k, key)
        a = launch(env, shape, 0, "f64", B, start, k, prob="shared", shared=True)
        e = launch(env, shape, 0, "f64", B, start, k, prob="shared", shared=False)
        for u, v in zip(a["out"] + (a["best"],), e["out"] + (e["best"],)):
            assert same_bits(u, v), ("shared factors against the expanded batch", key, k)
        hold_iterate(g, "%s/k%d" % (key, k), a, ref, best, val, gate_of(shape, 0, "f64", B, prob="shared"))
    g.done()


def check_big_refuses_shared_factors(env, shape=(12, 9, 3)):
    """api_polish: the large-QP family works in its blob -- one blob for B > 1 QPs is QPX_ERR_ARG"""
    from qpth_amd import _lib
    n, m, q = shape
    B = 2
    with env.run(BIGK):
        fac = factors(env, shape, B, "f64", BIGK)
        arrs, start = arrs_of(shape, B, "f64"), regular_start(shape, B, "f64")
        Q, p, G, h, A, b = [torch.tensor(np.asarray(a), device=env.dev) for a in arrs]
        x, s, z, y = [torch.tensor(np.asarray(v), device=env.dev) for v in start]
        keep = [v.clone() for v in (x, s, z, y)]
        P = _lib._ptr
        stream = _lib._stream(fac.blob)
        call = lambda sfac, nb: fac.lib.dll.qpx_polish(_lib.QPX_F64, nb, n, m, q, P(Q), n * n, P(p), n, P(G), m * n, P(h), m, P(A), q * n, P(b), q,       # noqa: E731
                                                       P(fac.blob), sfac, 1, 0, P(x), P(y), P(z), P(s), None, P(fac.status), stream)
        assert call(0, B) == -1                              # QPX_ERR_ARG, nothing launched
        for v, w in zip((x, s, z, y), keep):
            assert torch.equal(v, w)
        assert call(0, 1) == 0 and not torch.equal(x[0], keep[0][0]) and torch.equal(x[1], keep[0][1])      # B = 1: one blob is all there is


# ---------------------------------------------------------------- 6. a non-finite QP beside healthy ones
def check_nan_beside_healthy(env, shape, knob):
    from qpth_amd import _lib
    B, qp = 3, 1
    key = name(shape, knob, "f64", "/nan")
    start = regular_start(shape, B, "f64")
    bad = [v.copy() for v in start]
    bad[2][qp, shape[1] // 2] = float("nan")                 # one entry of lam of QP 1
    for steps in (1, 3):
        clean = launch(env, shape, knob, "f64", B, start, steps)
        res = launch(env, shape, knob, "f64", B, bad, steps)
        for a, c, s0 in zip(res["out"], clean["out"], bad):
            assert same_bits(a[[0, 2]], c[[0, 2]]), ("a healthy QP's answer depends on its neighbour", key, steps)
            assert same_bits(a[qp], s0[qp]), ("the non-finite QP's arrays were changed", key, steps)
        assert same_bits(res["best"][[0, 2]], clean["best"][[0, 2]])
        assert res["best"][qp] == np.inf, (key, res["best"])
        no_new_bits(res, (0, 2))
        no_new_bits(clean)
        assert res["after"][qp] & ~(res["before"][qp] | _lib.ST_KKT_BREAKDOWN | _lib.ST_NONFINITE) == 0, (key, res["after"])


# ---------------------------------------------------------------- 7. untouched memory
def check_spare_rows(env, shape, knob=0):
    B = batch_of(shape, knob)
    start = regular_start(shape, B, "f64")
    res = launch(env, shape, knob, "f64", B, start, 2, spare=1)
    ref = reference(shape, B, "f64")
    best, val = decisive(ref, 2, name(shape, knob))
    for full in res["spare"]:
        assert np.isnan(full[0]).all() and np.isnan(full[-1]).all() and (full.shape[-1] == 0 or np.isfinite(full[1:-1]).all()), name(shape, knob)
    g = Gate()
    hold_iterate(g, name(shape, knob, "f64", "/spare/k2"), res, ref, best, val, TOL)
    g.done()


# ---------------------------------------------------------------- 8. qpx_polish_supported and the error codes
def check_supported_and_error_codes(env):
    from qpth_amd import _lib
    with env.run(0):
        dll = _lib.backend_for(torch.zeros(1, device=env.dev)).dll
        for shape in TILE_SHAPES + GRID_SHAPES + BIG_SHAPES:
            assert dll.qpx_polish_supported(_lib.QPX_F64, *shape) == 1 and dll.qpx_polish_supported(_lib.QPX_F32, *shape) == 1, shape
            assert dll.qpx_polish_supported(_lib.QPX_F32_WIDE, *shape) == 0, shape
        assert dll.qpx_polish_supported(_lib.QPX_F64, 512, 70, 6) == 1 and dll.qpx_polish_supported(_lib.QPX_F64, 70, 512, 6) == 1
        for dims in ((513, 70, 6), (70, 513, 6), (600, 70, 513)):
            assert dll.qpx_polish_supported(_lib.QPX_F64, *dims) == 0 and dll.qpx_polish_supported(_lib.QPX_F32, *dims) == 0, dims
        # the entry point answers the same and launches nothing (every pointer is one buffer larger than any array named)
        buf = torch.zeros(600 * 600, dtype=torch.float64, device=env.dev)
        st = torch.zeros(2, dtype=torch.int32, device=env.dev)
        P = _lib._ptr(buf)
        call = lambda code, n, m, q: dll.qpx_polish(code, 2, n, m, q, P, 0, P, 0, P, 0, P, 0, P, 0, P, 0,      # noqa: E731
                                                    P, 0, 1, 0, P, P, P, P, P, _lib._ptr(st), _lib._stream(buf))
        assert call(_lib.QPX_F32_WIDE, 12, 9, 3) == -2 and call(_lib.QPX_F64, 513, 70, 6) == -2          # QPX_ERR_UNSUPPORTED
    # refine > 0 on the large-QP family: QPX_ERR_UNSUPPORTED, the arrays untouched
    shape = (12, 9, 3)
    B = batch_of(shape, BIGK)
    start = regular_start(shape, B, "f64")
    with env.run(BIGK):
        assert dll.qpx_polish_supported(_lib.QPX_F64, *shape) == 1 and dll.qpx_refine_supported(_lib.QPX_F64, *shape) == 0
    with pytest.raises(RuntimeError, match=r"code -2"):
        launch(env, shape, BIGK, "f64", B, start, 1, refine=1)
