"""The KKT-solve kernels (api_kkt of qpth_amd/csrc/qpx_api.inc) in every ROLE -- the plain solve, the
backward with its duals cotangents, forward mode, K right-hand sides, the second-order pass -- and every FORM the A/B knob
reaches, against a dense solve: the checks that tests/test_emu_kkt.py runs on the host-thread emulator and
tests/test_gpu_kkt.py on a real MI355X.  Every check takes an `env`: env.dev (the torch device) and env.run(variant=0), a
context manager around the library calls (the knob of include/qpx.h, qpx_set_ipm_variant).  Everything goes through
qpth_amd.kkt.KKTFactors (forward mode's dslack, which KKTFactors.jvp does not return, through the same call of its ctypes
layer with the fourth output added).

The reference is not built from the code under test.  Per QP the dense row-scaled system of tests/multi_reference.py,

    [[Q, G', A'], [D G, -I, 0], [A, 0, 0]] (dx, dz, dy) = -(rx, d rz - rs, ry),     ds = -rz - G dx,

is factored by a float64 LU and REFINED: residuals of the system held in np.longdouble (64-bit mantissa), corrections from the
float64 factors, ROUNDS = 5 rounds, the solution kept in np.longdouble.  tests/test_kkt_reference.py holds that against a
50-digit mpmath LU with d log-uniform in 1e-8 .. 1e8 (measured there: 1.5e-18 at (12, 9, 3), 4.9e-19 at (20, 40, 4), where the
float64 LU alone has 6.4e-15 and 4.6e-15; its gate REF_TOL = 1e-11 is 1e3 below the 1e-8 of the float64 checks.  The one tighter
number here, K1_TOL = 1e-13, compares two launches with each other, not with the reference).  The gradients, the forward-mode right-hand side
and the second-order outputs follow from that solution by the formulas of include/qpx.h, on the host in float64
(tests/hvp_reference.py's first_backward and second_order with this refined solve handed in).

Problems: problems.prof_qp(3, n, m, q, SEED) at SHAPES (loop_checks.SHAPES and three shapes for this family); each at every
knob value of multi_reference.KNOB_FORMS and at 0, and BIG at 0.  Two values of d per case: "bwd", the backward's own
clamp(lam, 1e-8) / clamp(s, 1e-8) at the solution KKTFactors.ipm returns under the default knob (sixteen decades), and "mid",
rand + 0.1 (as lam with s = 1, beside a random zhat and nu, for the roles that form d themselves).  The error measure is
max |a - ref| / max(1, max |ref|) per output array and per QP (per (QP, k) for K right-hand sides): one wrong padded entry shows.

Checks (per case), gates, and the worst figure measured over all cases (the host-thread emulator | one MI355X):

  1. solve: rx, rs, rz, ry all random; each of rs, rz, ry None in turn (NULL = zeros); rx alone.  (dx, dz, dy), and ds without
     an rs: TOL = 1e-8, the project's gate of this family (tests/test_gpu_multi.py).     measured: 3.9e-11 | 1.2e-10
     ds with an rs: multi_reference.ds_tol = 1e-6.                                              measured: 2.0e-7 | 4.6e-7
  2. backward: dl_dz alone, then with dl_dlam and dl_dnu: the six gradients and (dx, dz, dy), TOL.  Once more with `want` false
     for dQ and dG: None comes back for the two (the Python layer takes no buffer in), every other output BITWISE that of the
     full call (it is, on both).                                                               measured: 1.3e-11 | 4.5e-11
  3. forward mode: tangents on all six parameters, want_duals: dzhat, dlam, dnu and dslack, TOL; with tG and tb alone; with an
     un-batched tQ (stride 0).                                                                  measured: 1.2e-11 | 2.4e-11
     The adjoint identity against check 2's gradients per QP, in the kernels' own numbers:
     |lhs - rhs| <= ADJOINT = 1e-10 (|lhs| + sum |terms|), the gate of tests/test_emu_jvp.py.    measured: 1.8e-12 | 2.0e-12
  4. K right-hand sides, K = 1, MULTI_RHS_BLOCK + 1, 2 MULTI_RHS_BLOCK + 3: every (QP, k), TOL.  measured: 4.2e-11 | 6.2e-11
     ds (every right-hand side has an rs): ds_tol = 1e-6.                                       measured: 1.5e-7 | 2.8e-7
     K = 1 against check 1's single solve, a test of its own (check_multi_k1): BITWISE, in all three dtypes, on both.  It was
     not before this module: the multi role took K = 1 through its block of MULTI_RHS_BLOCK accumulators, another order of the
     same additions, and came out up to 3.8e-12 | 3.8e-12 from the single solve (at (16, 113, 0), knob 0, d "bwd"; above 1e-13 at
     20 of the emulator's 50 cases and 47 of the MI355X's 111; QPX_F32 3.0e-6) -- each of the two 1e-12 .. 1e-10 from the refined
     reference, as a float64 LAPACK LU of the dense system is (reference_side: up to 4.8e-11), so neither was wrong, but
     include/qpx.h says K = 1 computes what qpx_factor_solve_kkt computes.  The dispatcher (qpx_api.inc,
     api_factor_solve_kkt_multi) now hands K = 1 to the single solve's kernel; the figure is still recorded beside K1_TOL = 1e-13
     (QPX_F32: 1e-5), the bound it would have to keep were it not bitwise.
  5. second order (the "bwd" d only, where backward2_fused() holds): zdot, lamdot, nudot and the six H for random W, at the
     REFERENCE's (dx, dz, dy) of check 2 handed to the kernel, TOL.  min(lam + s) > 1e-6 per row is asserted first (strict
     complementarity: a degenerate draw fails loudly).                                          measured: 2.8e-11 | 3.2e-11
  A form that declines a role is skipped for that role -- after the check has asserted that the *_supported query says so where
  this module knows the answer (multi_expected, b2_expected: the large-QP family for K right-hand sides and the second-order
  pass, the two-wave tile forms for the second-order pass); no error code is caught.

  Beside CASES, at the default knob: (20, 40, 4) at B = 520 (beyond 512 QPs the dispatcher takes the one-wave form at four tile
  rows; GPU only), checks 1-4; Q, G, A shared with one factor blob (sfac = 0) at (12, 9, 3) and (100, 50, 10), checks 1-4 against
  the reference and BITWISE against the expanded batch; QPX_F32 on the six thread-grid forms (F32_SHAPES, problems.random_dense_qp,
  the "mid" d), checks 1-4, gate max(1e-3, 100 x the error of a float32 torch.linalg.solve of the same system against the refined
  reference), K = 1 against the single solve 1e-5; wide=True (float32 tensors, float64 arithmetic) at WIDE_SHAPES, checks 1-4
  against the float64 reference rounded to float32, 1e-6 (tests/test_gpu_multi.py's gate of that path; there the adjoint
  identity is held to 1e-6 too: its inputs are rounded to float32).
  Measured there (emulator | MI355X): B = 520 (MI355X only) 6.2e-11 against TOL and 4.6e-7 against ds_tol; shared factors bitwise
  the expanded batch on both; QPX_F32 2.8e-5 | 2.8e-5 at (20, 170, 2) (gate there 1.1e-3: the float32 dense solve has 1.1e-5; 1e-3
  at the five other shapes, where it has <= 3.0e-6); wide=True 5.7e-9 | 5.7e-9, ds with an rs 2.0e-7 | 2.0e-7, adjoint 4.6e-8 | 4.6e-8.
  No float64 case came near 1e-8, so no gate rests on the conditioning rule (100 x the unrefined dense solve's error).

What the gates see (scratch builds of the emulator, never committed, made while K = 1 still ran the multi role):
  - qpx_grid.h, the solve's write-back of dz without row m - 1: check 1 at all 48 thread-grid / tile cases of the emulator's 55 and check 3 at all 48 (dlam),
    the QPX_F32, wide and shared-factors cases, K = 1 against the single solve -- the unwritten entry is the NaN that
    conftest.py fills torch.empty with: figure inf.
  - the same loop, the sign of rs flipped in ds: check 1's ds with an rs at the same 48 cases, 2.2 .. 9.4e8 (gate 1e-6).
  - kkt_multi_body, the second block of right-hand sides reads the first block's rz: check 4 at all 48 cases that run it,
    1.5e-2 .. 15 (ds 1.6e-2 .. 4.6); K = 1 and check 1 stay clean.
  - dG = dz zhat' + lam dx' formed with slack for lam: check 2 at every thread-grid / tile case (48), 1.2e-7 .. 1.9e2 (dl_dz alone; 3.5e-2 .. 1.9e2 with
    the duals cotangents), and check 3's adjoint identity at the same cases, 1.9e-2 .. 0.93 (gate 1e-10).
  - qpx_big.h, ry dropped from the right-hand side: checks 1, 2 and 3 at the four large-family cases with q > 0 ((12, 9, 3),
    (20, 40, 4), (130, 70, 5) at knob 3 and (120, 100, 10)): solve 0.15 .. 1.2, backward 0.26 .. 2.1, adjoint 4.7e-2 .. 0.91.

scripts/check_kkt.py runs all of it on the GPU and writes the figures, their gates and the reference-side figures to
profiles/kkt_roles.json.
"""
import numpy as np
import torch

import hvp_reference
import loop_checks
import problems
from multi_reference import KNOB_FORMS, ds_tol

LD = np.longdouble
TOL = 1e-8                 # float64 arithmetic: the project's gate of this family (tests/test_gpu_multi.py)
TOL_WIDE = 1e-6            # float32 tensors, float64 arithmetic (test_parity_float32_data_in_float64_arithmetic)
TOL_F32 = 1e-3             # QPX_F32: the floor of max(1e-3, 100 x the float32 dense solve's own error)
TOL_F32_SINGLE = 1e-5      # QPX_F32: K = 1 of the multi solve against the single solve
REF_TOL = TOL / 1e3        # the reference against mpmath (tests/test_kkt_reference.py)
ADJOINT = 1e-10            # tests/test_emu_jvp.py's gate of the adjoint identity
K1_TOL = 1e-13            # float64 arithmetic: K = 1 of the multi solve against the single solve, where it is not bitwise
ROUNDS = 5
SEED = loop_checks.SEED
B3 = 3
tag = loop_checks.tag
FORMS = (0,) + tuple(KNOB_FORMS)
SHAPES = list(loop_checks.SHAPES) + [
    (17, 33, 2),          # every dimension one past a tile edge
    (129, 17, 1),         # the third slot of n beside two tile rows, q = 1
    (16, 113, 0),         # the first m on the ten-block thread grid
]
BIG = loop_checks.BIG
CASES = [(s, f) for s in SHAPES for f in FORMS] + [(BIG, 0)]
# the emulator runs a GPU thread as a fibre: the split of loop_checks.EMU_CASES -- every form at six shapes, the default
# form at the others; the GPU runs all of CASES
EMU_CASES = [(s, f) for s, f in CASES if f == 0 or s in loop_checks.EMU_ALL_FORMS]
DKINDS = ("bwd", "mid")
ONE_WAVE_SHAPE, ONE_WAVE_B = loop_checks.ONE_WAVE_SHAPE, loop_checks.ONE_WAVE_B
SHARED_SHAPES = [(12, 9, 3), (100, 50, 10)]
F32_SHAPES = [(12, 9, 3), (20, 24, 3), (20, 40, 4), (60, 112, 0), (40, 130, 0), (20, 170, 2)]      # one per thread-grid form
WIDE_SHAPES = [(100, 100, 0), (12, 9, 3)]
NAMES = ("dQ", "dp", "dG", "dh", "dA", "db")
B2_OUTS = ("zdot", "lamdot", "nudot") + hvp_reference.NAMES

measured = {}        # "check/case/d" -> worst figure seen (scripts/check_kkt.py writes them to profiles/kkt_roles.json)
gates = {}           # the same keys -> the gate the figure was held to
reference_side = {}  # what the gates rest on: the unrefined float64 / the float32 dense solve against the refined reference
k1_bitwise = {}      # case -> did K = 1 of the multi solve equal the single solve bit for bit
rule_decided = {}    # case/d -> did 100 x the unrefined dense solve's error exceed TOL (only the cases that ask for the rule)


# ---------------------------------------------------------------- the reference
class Dense:
    """A batch's dense row-scaled KKT systems: float64 LU factors and the matrices in np.longdouble for the residuals"""

    def __init__(self, Q, G, A, d):
        B, m, n = G.shape
        q = A.shape[1]
        self.B, self.n, self.m, self.q = B, n, m, q
        K = np.zeros((B, n + m + q, n + m + q), LD)
        K[:, :n, :n] = Q
        K[:, :n, n:n + m] = G.transpose(0, 2, 1)
        K[:, n:n + m, :n] = d.astype(LD)[:, :, None] * G.astype(LD)
        K[:, n:n + m, n:n + m] = -np.eye(m)
        K[:, :n, n + m:] = A.transpose(0, 2, 1)
        K[:, n + m:, :n] = A
        self.K, self.G, self.d = K, G.astype(LD), d.astype(LD)
        self.K64 = torch.from_numpy(K.astype(np.float64))
        self.lu, self.piv = torch.linalg.lu_factor(self.K64)

    def rhs(self, rx, rs, rz, ry, sel=slice(None)):
        """-(rx, d rz - rs, ry) in np.longdouble, (B, k, N), and rz; each of the four (B, k, .) or None (zeros)"""
        B, k = next(X.shape[:2] for X in (rx, rs, rz, ry) if X is not None)
        rx, rs, rz, ry = [np.zeros((B, k, w), LD) if X is None else np.asarray(X, LD)
                          for X, w in ((rx, self.n), (rs, self.m), (rz, self.m), (ry, self.q))]
        return -np.concatenate([rx, self.d[sel][:, None, :] * rz - rs, ry], axis=2), rz

    def solve(self, rx, rs, rz, ry, rounds=ROUNDS, sel=slice(None)):
        """(dx, ds, dz, dy), each (B, k, .) np.longdouble, of the QPs `sel`.  rounds = 0: the float64 LU solve alone"""
        n, m = self.n, self.m
        rhs, rz = self.rhs(rx, rs, rz, ry, sel)
        K, lu, piv = self.K[sel], self.lu[sel], self.piv[sel]
        x = np.zeros(rhs.shape, LD)
        for r in range(rounds + 1):
            res = rhs - np.einsum("bij,bkj->bki", K, x) if r else rhs
            cor = torch.linalg.lu_solve(lu, piv, torch.from_numpy(res.astype(np.float64)).transpose(1, 2)).transpose(1, 2)
            x = x + cor.numpy().astype(LD)
        dx = x[..., :n]
        return dx, -rz - np.einsum("bmn,bkn->bkm", self.G[sel], dx), x[..., n:n + m], x[..., n + m:]

    def solve_one(self, i, rx, rz, ry):
        """QP i alone, (x, z, y) float64 with M (x, z, y) = -(rx, rz, ry): the `solve` hook of tests/hvp_reference.py"""
        dx, _, dz, dy = self.solve(np.asarray(rx)[None, None], None, np.asarray(rz)[None, None], np.asarray(ry)[None, None],
                                   sel=slice(i, i + 1))
        return [np.asarray(v[0, 0], np.float64) for v in (dx, dz, dy)]


def figs(a, ref, lead=1):
    """worst over the rows of max |a - ref| / max(1, max |ref|), a row = one QP's (one (QP, k)'s) output array"""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    rows = int(np.prod(ref.shape[:lead]))
    a, ref = a.reshape(rows, -1), ref.reshape(rows, -1)
    f = np.abs(a - ref).max(1) / np.maximum(1.0, np.abs(ref).max(1))
    return float(f.max()) if np.isfinite(f).all() else float("inf")


class Gate:
    """collects the figures of one check: every one is printed and recorded, then all are asserted"""

    def __init__(self):
        self.bad = []

    def hold(self, key, value, gate):
        measured[key] = max(float(value), measured.get(key, 0.0))
        gates[key] = gate
        print("%-52s %.3e  (gate %.1e)" % (key, value, gate))
        if not value <= gate:
            self.bad.append((key, value, gate))

    def done(self):
        assert not self.bad, self.bad


def rng(shape, salt):
    return np.random.RandomState([shape[0], shape[1], shape[2], salt])


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def rounded(x, dtype):
    """float64 arrays holding what the tensors of `dtype` hold"""
    return np.asarray(x, np.float64) if dtype == "f64" else np.asarray(np.asarray(x, np.float32), np.float64)


def problem(shape, B, dtype, prob):
    """(Q, p, G, h, A, b) as float64 arrays, batched (A (B, 0, n) without equalities).  prob: "prof" = problems.prof_qp,
    "shared" = the same with QP 0's Q, G, A for every QP, "dense" = problems.random_dense_qp"""
    def make():
        n, m, q = shape
        arrs = problems.random_dense_qp(B, n, m, q, seed=SEED) if prob == "dense" else problems.prof_qp(B, n, m, q, seed=SEED)
        arrs = [rounded(x, dtype) for x in arrs]
        if q == 0:
            arrs[4], arrs[5] = np.zeros((B, 0, n)), np.zeros((B, 0))
        if prob == "shared":
            for i in (0, 2, 4):
                arrs[i] = np.broadcast_to(arrs[i][:1], arrs[i].shape).copy()
        for x in arrs:
            x.setflags(write=False)
        return tuple(arrs)
    return cached(("problem", tuple(shape), B, dtype, prob), make)


def torch_dtype(dtype):
    return torch.float64 if dtype == "f64" else torch.float32


def on(x, dev, dtype):
    """a host array as a tensor of the case's dtype on its device; None and empty arrays: None"""
    if x is None or np.size(x) == 0:
        return None
    return torch.tensor(np.asarray(x, np.float64), dtype=torch_dtype(dtype), device=dev)


def build(env, arrs, B, dtype, shared=False):
    """KKTFactors of the batch; call inside env.run(form).  shared: Q, G, A un-batched -> one blob, sfac = 0"""
    from qpth_amd.kkt import KKTFactors
    Q, G, A = [on(arrs[i][0] if shared else arrs[i], env.dev, dtype) for i in (0, 2, 4)]
    return KKTFactors.build(Q, G, A, B, wide=(dtype == "wide"))


def solution(env, shape, B, dtype, prob):
    """(zhat, lam, slacks, nu) of KKTFactors.ipm under the default knob, as host arrays: where the "bwd" d is taken"""
    def make():
        arrs = problem(shape, B, dtype, prob)
        with env.run(0):
            fac = build(env, arrs, B, dtype)
            p, h, b = [on(arrs[i], env.dev, dtype) for i in (1, 3, 5)]
            r = fac.ipm(p, h, b)
            out = [x.detach().cpu().numpy().astype(np.float64) for x in (r.zhat, r.lam, r.slacks)]
            out.append(r.nu.detach().cpu().numpy().astype(np.float64) if shape[2] else np.zeros((B, 0)))
        assert all(np.isfinite(x).all() for x in out)
        return tuple(out)
    return cached(("solution", env.dev.type, tuple(shape), B, dtype, prob), make)


class Case:
    """One batch and one d: the data, the random inputs of every check and, made once and shared by every form, their
    references"""

    def __init__(self, env, shape, B, kind, dtype, prob, cond_rule=False):
        n, m, q = shape
        self.shape, self.B, self.kind, self.dtype, self.prob, self.dev = tuple(shape), B, kind, dtype, prob, env.dev
        self.cond_rule = cond_rule
        self.arrs = problem(shape, B, dtype, prob)
        Q, p, G, h, A, b = self.arrs
        r = rng(shape, 1 if kind == "bwd" else 2)
        rn = lambda *s: rounded(r.randn(*s), dtype)      # noqa: E731
        if kind == "bwd":
            zh, lam, sl, nu = solution(env, shape, B, dtype, prob)
        else:
            zh, nu, lam, sl = rn(B, n), rn(B, q), rounded(r.rand(B, m) + 0.1, dtype), np.ones((B, m))
        self.sol = (zh, lam, sl, nu)
        # d as the kernels form it from (lam, s) -- in float64, also from float32 tensors under wide=True -- and as a tensor of
        # the case's dtype, which is what solve_kkt and solve_kkt_many are handed
        self.d_sol = np.maximum(lam, 1e-8) / np.maximum(sl, 1e-8)
        if dtype == "f64":
            self.d_arg = self.d_sol
        else:
            self.d_arg = (np.maximum(lam.astype(np.float32), np.float32(1e-8))
                          / np.maximum(sl.astype(np.float32), np.float32(1e-8))).astype(np.float64)
            if dtype == "f32":
                self.d_sol = self.d_arg
        self.rhs = (rn(B, n), rn(B, m), rn(B, m), rn(B, q))
        self.cots = (rn(B, n), rn(B, m), rn(B, q))
        self.tans = (rn(B, n, n), rn(B, n), rn(B, m, n), rn(B, m), rn(B, q, n), rn(B, q))
        self.many = {K: (rn(B, K, n), rn(B, K, m), rn(B, K, m), rn(B, K, q)) for K in multi_ks()}
        self.W = (rn(B, n, n), rn(B, n), rn(B, m, n), rn(B, m), rn(B, q, n), rn(B, q))
        self._refs = {}

    def t(self, x):
        return on(x, self.dev, self.dtype)

    def name(self, form=0, extra=""):
        return "%s%s/%s" % (tag(self.shape, form), extra, self.kind)

    def dense(self, which):
        """which: "arg" (the d handed to solve_kkt) or "sol" (the d the kernels form from lam and s)"""
        d = self.d_arg if which == "arg" else self.d_sol
        if which == "sol" and np.array_equal(self.d_sol, self.d_arg):
            return self.dense("arg")
        return self.ref(("dense", which), lambda: Dense(self.arrs[0], self.arrs[2], self.arrs[4], d))

    def ref(self, key, make):
        if key not in self._refs:
            self._refs[key] = make()
        return self._refs[key]

    def out(self, x):
        """a reference array as the case's output dtype holds it"""
        return rounded(np.asarray(x, np.float64), "f64" if self.dtype == "f64" else "f32")

    # -- check 1
    def ref_solve(self, mask):
        def make():
            rhs = [X[:, None] if keep else None for X, keep in zip(self.rhs, mask)]
            return tuple(self.out(v[:, 0]) for v in self.dense("arg").solve(*rhs))
        return self.ref(("solve", mask), make)

    def reference_side(self):
        """the float64 LU solve alone (and, for float32 tensors, a float32 torch.linalg.solve) against the refined reference, all
        four right-hand sides of check 1: what this case's conditioning costs a dense solve"""
        def make():
            D = self.dense("arg")
            rhs = [X[:, None] for X in self.rhs]
            ref = D.solve(*rhs)
            raw = D.solve(*rhs, rounds=0)
            out = {"dense64": max(figs(np.asarray(a, np.float64), np.asarray(b, np.float64)) for a, b in zip(raw[::2] + raw[3:], ref[::2] + ref[3:]))}
            if self.dtype != "f64":
                r32, _ = D.rhs(*rhs)
                x = torch.linalg.solve(D.K64.float(), torch.from_numpy(r32.astype(np.float32)).transpose(1, 2)).transpose(1, 2).numpy()
                n, m = D.n, D.m
                out["dense32"] = max(figs(x[..., lo:hi], np.asarray(b, np.float64))
                                     for (lo, hi), b in zip(((0, n), (n, n + m), (n + m, n + m + D.q)), (ref[0], ref[2], ref[3])))
            return out
        return self.ref("reference_side", make)

    # -- check 2
    def ref_backward(self, duals):
        def make():
            gz, gl, gn = self.cots
            dx, _, dz, dy = [np.asarray(v[:, 0], np.float64) for v in
                             self.dense("sol").solve(gz[:, None], None, gl[:, None] if duals else None, gn[:, None] if duals else None)]
            out = dict(zip(NAMES, hvp_reference.first_grads(self.sol, (dx, dz, dy))))
            out.update(dx=dx, dz=dz, dy=dy)
            return {k: self.out(v) for k, v in out.items()}
        return self.ref(("backward", duals), make)

    # -- check 3
    def tangents(self, variant):
        """"all": the six; "Gb": tG and tb alone (tG alone without equalities); "Q0": the six, tQ un-batched"""
        t = list(self.tans)
        if variant == "Gb":
            t = [None, None, t[2], None, None, t[5] if self.shape[2] else None]
        elif variant == "Q0":
            t[0] = t[0][0]
        return t

    def ref_jvp(self, variant):
        def make():
            zh, lam, _, nu = self.sol
            B, (n, m, q) = self.B, self.shape
            zero = (np.zeros((B, n, n)), np.zeros((B, n)), np.zeros((B, m, n)), np.zeros((B, m)), np.zeros((B, q, n)), np.zeros((B, q)))
            tQ, tp, tG, th, tA, tb = [z if t is None else np.broadcast_to(t, z.shape) for t, z in zip(self.tangents(variant), zero)]
            e = np.einsum
            rx = 0.5 * (e("bij,bj->bi", tQ, zh) + e("bji,bj->bi", tQ, zh)) + tp + e("bmn,bm->bn", tG, lam) + e("bqn,bq->bn", tA, nu)
            rz = e("bmn,bn->bm", tG, zh) - th
            ry = e("bqn,bn->bq", tA, zh) - tb
            dx, ds, dz, dy = self.dense("sol").solve(rx[:, None], None, rz[:, None], ry[:, None])
            return {k: self.out(v[:, 0]) for k, v in (("dzhat", dx), ("dlam", dz), ("dnu", dy), ("dslack", ds))}
        return self.ref(("jvp", variant), make)

    # -- check 4
    def ref_multi(self, K):
        return self.ref(("multi", K), lambda: tuple(self.out(v) for v in self.dense("arg").solve(*self.many[K])))

    # -- check 5
    def ref_b2(self):
        def make():
            D = self.dense("sol")
            gz, gl, gn = self.cots
            bsol = hvp_reference.first_backward(self.arrs, self.sol, (gz, gl, gn), solve=D.solve_one)
            first = self.ref_backward(True)
            for a, k in zip(bsol, ("dx", "dz", "dy")):           # (the same refined solve, by another route)
                assert figs(a, first[k]) <= 1e-15, k
            bsol = tuple(self.out(v) for v in bsol)
            return bsol, {k: self.out(v) for k, v in hvp_reference.second_order(self.arrs, self.sol, bsol, self.W, solve=D.solve_one).items()}
        return self.ref("b2", make)


def multi_ks():
    from qpth_amd.kkt import MULTI_RHS_BLOCK as RB
    return (1, RB + 1, 2 * RB + 3)          # one, two and three blocks, the last ones ragged


def case(env, shape, kind, B=B3, dtype="f64", prob="prof", cond_rule=False):
    key = ("case", env.dev.type, tuple(shape), B, kind, dtype, prob, cond_rule)
    return cached(key, lambda: Case(env, shape, B, kind, dtype, prob, cond_rule))


def factors(env, c, form, shared=False):
    """the case's factors under knob `form`, built once (d is no part of them: both d share them); call inside env.run(form)"""
    key = ("factors", env.dev.type, c.shape, c.B, c.dtype, c.prob, form, shared)
    return cached(key, lambda: build(env, c.arrs, c.B, c.dtype, shared))


def no_breakdown(fac):
    from qpth_amd import _lib
    assert int(fac.status.max()) & _lib.ST_KKT_BREAKDOWN == 0


def code_of(fac):
    from qpth_amd import _lib
    return _lib.QPX_F32_WIDE if fac.wide else (_lib.QPX_F64 if fac.dtype == torch.float64 else _lib.QPX_F32)


def tol_of(c):
    """the gate of the case's dtype: TOL, TOL_WIDE, or for QPX_F32 max(1e-3, 100 x the float32 dense solve's error).  A float64
    case made with cond_rule=True (tests/big_checks.py: orders up to 1 088) takes the conditioning rule, max(TOL, 100 x the
    unrefined float64 dense solve against the refined reference), and records in rule_decided whether the second term decided"""
    if c.dtype == "f64":
        if c.cond_rule:
            side = 100.0 * c.reference_side()["dense64"]
            rule_decided["%s/B%d/%s/%s" % (tag(c.shape), c.B, c.prob, c.kind)] = bool(side > TOL)
            return max(TOL, side)
        return TOL
    if c.dtype == "wide":
        return TOL_WIDE
    return max(TOL_F32, 100.0 * c.reference_side()["dense32"])


def record_reference_side(c):
    for k, v in c.reference_side().items():
        reference_side["%s/%s%s/%s" % (k, tag(c.shape), "" if c.B == B3 else "/B%d" % c.B, c.kind) + ("" if c.dtype == "f64" else "/" + c.dtype)] = v


# ---------------------------------------------------------------- what each role returns (tensors, by name)
SOLVE_MASKS = {"all": (1, 1, 1, 1), "no_rs": (1, 0, 1, 1), "no_rz": (1, 1, 0, 1), "no_ry": (1, 1, 1, 0), "rx": (1, 0, 0, 0)}


def solve_masks(q):
    return {k: v for k, v in SOLVE_MASKS.items() if q or k != "no_ry"}


def run_solve(fac, c):
    d = c.t(c.d_arg)
    out = {}
    for name, mask in solve_masks(c.shape[2]).items():
        rhs = [c.t(X) if keep else None for X, keep in zip(c.rhs, mask)]
        out[name] = dict(zip(("dx", "ds", "dz", "dy"), fac.solve_kkt(d, *rhs)))
    return out


def run_backward(fac, c):
    sol = [c.t(x) for x in c.sol]
    gz, gl, gn = [c.t(x) for x in c.cots]
    out = {}
    for name, kw in (("z", {}), ("duals", dict(dl_dlam=gl, dl_dnu=gn)), ("part", dict(dl_dlam=gl, dl_dnu=gn, want=(False, True, False, True, True, True)))):
        r = fac.backward(*sol, gz, want_sol=True, **kw)
        out[name] = dict(zip(NAMES + ("dx", "dz", "dy"), tuple(r[:6]) + tuple(r[6])))
    return out


def run_jvp(fac, c):
    sol = [c.t(x) for x in c.sol]
    n, m, q = c.shape
    out = {}
    for variant in ("all", "Gb", "Q0"):
        ts = [c.t(t) for t in c.tangents(variant)]
        zt, lt, nt = fac.jvp(*sol, ts, want_duals=True)
        out[variant] = {"dzhat": zt, "dlam": lt, "dnu": nt}
    # dslack: KKTFactors.jvp does not return it -- its own call of the ctypes layer with the fourth output added
    ts = [c.t(t) for t in c.tangents("all")]
    zt, lt, sl = [torch.empty(c.B, k, dtype=fac.dtype, device=fac.device) for k in (n, m, m)]
    nt = torch.empty(c.B, q, dtype=fac.dtype, device=fac.device) if q else None
    with fac._knob():
        fac.lib.jvp(c.B, n, m, q, fac.blob, fac.sfac, *sol, *ts, zt, fac.status, dlam=lt, dnu=nt, dslack=sl, wide=fac.wide)
    assert torch.equal(zt, out["all"]["dzhat"]) and torch.equal(lt, out["all"]["dlam"])
    out["all"]["dslack"] = sl
    return out


def multi_supported(fac):
    with fac._knob():
        return bool(fac.lib.dll.qpx_multi_supported(code_of(fac), fac.n, fac.m, fac.q))


def run_multi(fac, c):
    d = c.t(c.d_arg)
    out = {K: dict(zip(("dx", "ds", "dz", "dy"), fac.solve_kkt_many(d, *[c.t(X) for X in c.many[K]]))) for K in multi_ks()}
    out["single"] = dict(zip(("dx", "ds", "dz", "dy"), fac.solve_kkt(d, *[c.t(X[:, 0]) for X in c.many[1]])))
    return out


def tile_rows(m):
    return 1 if m <= 16 else 2 if m <= 32 else 4 if m <= 64 else 7 if m <= 112 else 0


def multi_expected(shape, form):
    """qpx_multi_supported: every thread-grid / tile form, not the large-QP family"""
    return not (form == 3 or sum(shape) > 208)


def b2_expected(shape, form, dtype="f64"):
    """qpx_backward2_supported: not QPX_F32, not the large-QP family, not the two-wave tile forms -- +4096 at four and seven tile
    rows, and +2048 at seven, where no one-wave form is built and two waves stand in (qpx_api.inc: tile_waves)"""
    if dtype == "f32" or form == 3 or sum(shape) > 208:
        return False
    rows = tile_rows(shape[1])
    if form & 1024 and ((form & 4096 and rows in (4, 7)) or (form & 2048 and rows == 7)):
        return False
    return True


# ---------------------------------------------------------------- the gates of each role
def gate_solve(g, c, out, name):
    tol = tol_of(c)
    worst, worst_ds = 0.0, 0.0
    for variant, mask in solve_masks(c.shape[2]).items():
        ref = dict(zip(("dx", "ds", "dz", "dy"), c.ref_solve(mask)))
        got = out[variant]
        assert got["dx"].dtype == torch_dtype(c.dtype)
        for k in ("dx", "dz", "dy") + (() if mask[1] else ("ds",)):
            if got[k] is not None:
                worst = max(worst, figs(got[k], ref[k]))
        if mask[1]:
            worst_ds = max(worst_ds, figs(got["ds"], ref["ds"]))
    g.hold("solve/" + name, worst, tol)
    g.hold("solve_ds_with_rs/" + name, worst_ds, ds_tol(tol, True))


def gate_backward(g, c, out, name):
    tol = tol_of(c)
    q = c.shape[2]
    keys = [k for k in NAMES + ("dx", "dz", "dy") if q or k not in ("dA", "db", "dy")]
    for variant, duals in (("z", False), ("duals", True)):
        ref = c.ref_backward(duals)
        g.hold("backward_%s/%s" % (variant, name), max(figs(out[variant][k], ref[k]) for k in keys), tol)
    # `want` false for dQ and dG: nothing for the two, every other output bit for bit that of the full call
    full, part = out["duals"], out["part"]
    assert part["dQ"] is None and part["dG"] is None
    for k in keys:
        if k not in ("dQ", "dG"):
            assert torch.equal(part[k], full[k]), ("a wanted output depends on which others are wanted", name, k,
                                                   float((part[k] - full[k]).abs().max()))


def gate_jvp(g, c, out, name, grads):
    tol = tol_of(c)
    q = c.shape[2]
    for variant in ("all", "Gb", "Q0"):
        ref = c.ref_jvp(variant)
        keys = [k for k in out[variant] if q or k != "dnu"]
        assert variant != "all" or "dslack" in keys
        g.hold("jvp_%s/%s" % (variant, name), max(figs(out[variant][k], ref[k]) for k in keys), tol)
    # the adjoint identity against the backward's gradients, per QP, in the kernels' own numbers
    h = lambda x: x.detach().cpu().numpy().astype(np.float64).reshape(c.B, -1)      # noqa: E731
    gz, gl, gn = c.cots
    lhs = (gz * h(out["all"]["dzhat"])).sum(1) + (gl * h(out["all"]["dlam"])).sum(1)
    if q:
        lhs = lhs + (gn * h(out["all"]["dnu"])).sum(1)
    terms = np.stack([(h(grads[k]) * np.asarray(t).reshape(c.B, -1)).sum(1) for k, t in zip(NAMES, c.tans) if grads[k] is not None])
    gap = np.abs(lhs - terms.sum(0)) / (np.abs(lhs) + np.abs(terms).sum(0))
    g.hold("adjoint/" + name, float(gap.max()), ADJOINT if c.dtype == "f64" else tol)


def gate_multi(g, c, out, name):
    tol = tol_of(c)
    worst, worst_ds = 0.0, 0.0
    for K in multi_ks():
        ref = dict(zip(("dx", "ds", "dz", "dy"), c.ref_multi(K)))
        assert out[K]["dx"].shape == (c.B, K, c.shape[0])
        for k in ("dx", "dz", "dy"):
            if out[K][k] is not None:
                worst = max(worst, figs(out[K][k], ref[k], lead=2))
        worst_ds = max(worst_ds, figs(out[K]["ds"], ref["ds"], lead=2))
    g.hold("multi/" + name, worst, tol)
    g.hold("multi_ds_with_rs/" + name, worst_ds, ds_tol(tol, True))


def gate_multi_k1(g, c, out, name):
    """K = 1 of the multi solve against the single solve of the same right-hand side: bitwise (the dispatcher hands K = 1 to the
    single solve's kernel), in every dtype; the figure is recorded beside the bound it would have had to keep otherwise"""
    pairs = [(out[1][k][:, 0], out["single"][k]) for k in ("dx", "ds", "dz", "dy") if out[1][k] is not None]
    k1_bitwise[name] = all(torch.equal(a, b) for a, b in pairs)
    g.hold("multi_k1_vs_single/" + name, max(figs(a, b.cpu().numpy()) for a, b in pairs), K1_TOL if c.dtype != "f32" else TOL_F32_SINGLE)
    assert k1_bitwise[name], ("K = 1 of the multi solve is not the single solve bit for bit", name)


# ---------------------------------------------------------------- the checks
def checks_1_to_4(env, c, form, fac, name):
    """every role but the second-order pass on one set of factors: (the outputs by role, the Gate)"""
    g = Gate()
    out = {"solve": run_solve(fac, c), "backward": run_backward(fac, c), "jvp": run_jvp(fac, c)}
    gate_solve(g, c, out["solve"], name)
    gate_backward(g, c, out["backward"], name)
    gate_jvp(g, c, out["jvp"], name, out["backward"]["duals"])
    assert multi_supported(fac) == multi_expected(c.shape, form), (name, "qpx_multi_supported")
    if multi_supported(fac):
        out["multi"] = run_multi(fac, c)
        gate_multi(g, c, out["multi"], name)
        if c.dtype != "f64":          # (float64: check_multi_k1, a test of its own)
            gate_multi_k1(g, c, out["multi"], name)
    no_breakdown(fac)
    record_reference_side(c)
    return out, g


def check_solve(env, shape, form=0, B=B3, prob="prof", kinds=DKINDS, cond_rule=False):
    g = Gate()
    for kind in kinds:
        c = case(env, shape, kind, B, "f64", prob, cond_rule)
        with env.run(form):
            fac = factors(env, c, form)
            gate_solve(g, c, run_solve(fac, c), c.name(form))
            no_breakdown(fac)
        record_reference_side(c)
    g.done()


def check_backward(env, shape, form=0, B=B3, prob="prof", kinds=DKINDS, cond_rule=False):
    g = Gate()
    for kind in kinds:
        c = case(env, shape, kind, B, "f64", prob, cond_rule)
        with env.run(form):
            fac = factors(env, c, form)
            gate_backward(g, c, run_backward(fac, c), c.name(form))
            no_breakdown(fac)
    g.done()


def check_jvp(env, shape, form=0, B=B3, prob="prof", kinds=DKINDS, cond_rule=False):
    g = Gate()
    for kind in kinds:
        c = case(env, shape, kind, B, "f64", prob, cond_rule)
        with env.run(form):
            fac = factors(env, c, form)
            gate_jvp(g, c, run_jvp(fac, c), c.name(form), run_backward(fac, c)["duals"])
            no_breakdown(fac)
    g.done()


def check_multi(env, shape, form=0, B=B3, prob="prof", kinds=DKINDS, cond_rule=False):
    """returns False where the form declines the role (and the query was asserted to say so)"""
    g = Gate()
    for kind in kinds:
        c = case(env, shape, kind, B, "f64", prob, cond_rule)
        with env.run(form):
            fac = factors(env, c, form)
            assert multi_supported(fac) == multi_expected(shape, form), (shape, form, "qpx_multi_supported")
            if not multi_supported(fac):
                return False
            gate_multi(g, c, run_multi(fac, c), c.name(form))
            no_breakdown(fac)
    g.done()
    return True


def check_multi_k1(env, shape, form=0, B=B3, prob="prof"):
    """K = 1 of the multi solve against check 1's single solve, float64; returns False where the form declines the role"""
    g = Gate()
    extra = ("" if B == B3 else "/B%d" % B) + ("" if prob == "prof" else "/" + prob)
    for kind in DKINDS:
        c = case(env, shape, kind, B=B, prob=prob)
        with env.run(form):
            fac = factors(env, c, form, shared=(prob == "shared"))
            if not multi_supported(fac):
                assert not multi_expected(shape, form)
                return False
            gate_multi_k1(g, c, run_multi(fac, c), c.name(form, extra))
    g.done()
    return True


def check_backward2(env, shape, form=0, B=B3, prob="prof", kind="bwd"):
    """returns False where the form declines the role (and the query was asserted to say so)"""
    c = case(env, shape, kind, B, "f64", prob)
    g = Gate()
    with env.run(form):
        fac = factors(env, c, form)
        assert fac.backward2_fused() == b2_expected(shape, form), (shape, form, "qpx_backward2_supported")
        if not fac.backward2_fused():
            return False
        zh, lam, sl, nu = c.sol
        assert (lam + sl).min() > 1e-6, ("a degenerate draw: strict complementarity fails", shape, float((lam + sl).min()))
        bsol, ref = c.ref_b2()
        (zd, ld, nd), H = fac.backward2(*[c.t(x) for x in c.sol], [c.t(x) for x in bsol], [c.t(w) for w in c.W], fused=True)
        got = dict(zip(B2_OUTS, (zd, ld, nd) + tuple(H)))
        keys = [k for k in B2_OUTS if shape[2] or k not in ("nudot", "HA", "Hb")]
        g.hold("backward2/" + c.name(form), max(figs(got[k], ref[k]) for k in keys), TOL)
        no_breakdown(fac)
    g.done()
    return True


def check_one_wave_beyond_512(env):
    """B = 520 at four tile rows: the default dispatch's one-wave form, checks 1-4, every QP against the reference"""
    g = Gate()
    for kind in DKINDS:
        c = case(env, ONE_WAVE_SHAPE, kind, B=ONE_WAVE_B)
        with env.run(0):
            g.bad += checks_1_to_4(env, c, 0, factors(env, c, 0), c.name(0, "/B%d" % ONE_WAVE_B))[1].bad
    g.done()


def same_bits(a, b, path=""):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            same_bits(a[k], b[k], "%s/%s" % (path, k))
    elif a is None:
        assert b is None, path
    else:
        assert torch.equal(a, b), ("shared factors against the expanded batch", path, float((a - b).abs().max()))


def check_shared_factors(env, shape):
    """Q, G, A shared and ONE factor blob (sfac = 0): checks 1-4 against the reference, and bit for bit the expanded batch's"""
    g = Gate()
    for kind in DKINDS:
        c = case(env, shape, kind, prob="shared")
        with env.run(0):
            one, each = factors(env, c, 0, shared=True), factors(env, c, 0)
            assert one.shared and one.sfac == 0 and one.blob.numel() == one.elems and each.sfac == each.elems
            out, gg = checks_1_to_4(env, c, 0, one, c.name(0, "/shared"))
            g.bad += gg.bad
            same_bits(out, checks_1_to_4(env, c, 0, each, c.name(0, "/expanded"))[0])
    g.done()


def check_f32_grid(env, shape, B=B3):
    """QPX_F32 tensors on the thread-grid kernels (B=: tests/big_checks.py, the large-QP family's), the "mid" d"""
    c = case(env, shape, "mid", B=B, dtype="f32", prob="dense")
    with env.run(0):
        fac = factors(env, c, 0)
        assert not fac.wide and fac.blob.dtype == torch.float32
        checks_1_to_4(env, c, 0, fac, c.name(0, "/f32"))[1].done()


def check_wide(env, shape):
    """float32 tensors in float64 arithmetic (QPX_F32_WIDE)"""
    g = Gate()
    for kind in DKINDS:
        c = case(env, shape, kind, dtype="wide")
        with env.run(0):
            fac = factors(env, c, 0)
            assert fac.wide and fac.blob.dtype == torch.float64
            g.bad += checks_1_to_4(env, c, 0, fac, c.name(0, "/wide"))[1].bad
    g.done()
