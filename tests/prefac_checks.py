"""The pre-factorisation's factor blob (qpx_pre_factor / qpx_pre_factor_soft) in every FORM -- the symmetric
sweep at its seven block counts with the rank-1 and the four-pivot steps, the matrix-core form, the large-QP family, the soft
forms -- against a dense reference, array by array and WORD BY WORD: the checks that tests/test_emu_prefac.py runs on the
host-thread emulator and tests/test_gpu_prefac.py on a real MI355X.  Every check takes an `env` as tests/kkt_checks.py's do.
Blobs are built through qpth_amd.kkt.KKTFactors.build(Q, G, A, B, wide=, w=) under env.run(knob) and read back whole.

The reference (tests/prefac_reference.py, the only place that restates the layouts) is not built from the code under test:
np.linalg.inv of [[Q, A'], [A, 0]], four Newton corrections in np.longdouble, the blob's arrays from its blocks by longdouble
products; for the large family a longdouble Cholesky and substitutions written there, whose R must equal the other route's.
tests/test_prefac_reference.py holds it against a 50-digit mpmath inverse (6.2e-17 .. 2.2e-14, gate 1e-12).  The error measure
is kkt_checks.figs: max |a - ref| / max(1, max |ref|) per array and per QP.  A symmetric Q is assumed throughout: the forms
read different triangles of Q (the sweep and the matrix-core form the upper one, the large family all of it), so an
unsymmetric Q is out of scope and not tested.

Gate of float64 arithmetic, per array: max(TOL = 1e-9, 100 x lapack), lapack = the figure of the same array formed the plain
float64 way (np.linalg.inv and float64 products; np.linalg.cholesky and np.linalg.solve for the large family's factors)
against the refined reference -- recorded in `reference_side` beside every measured figure.  1e-9 is the gate the project
already holds blob against blob.  Before a reference is used its residual max |I - H X| must be <= 1e-3 x the case's LARGEST
gate (the residual bounds the error relative to the largest block of H^-1, the one with that gate: see Ref).  QPX_F32:
max(1e-3, 100 x the same arrays by float32 torch operations), the rule of kkt_checks.
figs divides by max(1, max |ref|), and NTn and S11i (at some shapes Kneg and W) lie wholly below 1 -- S11i below 1e-2 at
(20, 170, 2) --, so that two decades of a relative error in them would pass.  Where an array of family (a) has max |ref| < 1
it is therefore ALSO held, under the key "<array>:rel", to max |a - ref| / max |ref| with the gate formed by the same rule
from the plain route's figure in that measure.

Every word of a blob is in exactly one of three parts, and the parts are asserted to tile [0, elems) (prefac_reference.
expected_a, uncompared_big):
  compared      family (a): Kneg, MT, NTn, W, S11i, scal[0] = || G' 1 ||, every entry of R in every image the blob holds
                large family: the strictly-lower block triangle of Lq and of L11 (and L11' above the block diagonal: big_potrf
                with mirror = 1), W_kk in Wq, W_kk and W_kk' in Wy, the projected Zt, Yt, Vh, the lower block triangle of R with
                its diagonal blocks (big_gemm_r: lower = 1), scal[bsGt1]; pads included (zeros; the identity where a factor's
                diagonal is padded)
  pads          of the R images of family (a): EXACT zeros.  The sweep zero-fills each image it writes before the scatter
                (qpx_grid.h, sweep_body: "F[lay.Rg + e] = T(0)" and the two lines below), so Rg and Rw are zero-padded like Rm;
                the matrix-core form writes whole tiles of Rm.  Held on both.
  unspecified   family (a): scal[1..3] and the 8 profiling words (qpx_layout.h: "scal 4 [0] = ...; [4..11] phase timers of the
                profiling build"; QPX_PROF_DUMP is empty otherwise), and the words align4() leaves between two arrays
                (fac_layout: "o += align4(...)"; no consumer forms an address there).  They hold the NaN of conftest.py.
                large family, none of it read before it is written by its user:
                  T, Wt       the loop's work matrix and its block inverses (big_ipm: big_potrf(c, L.T, ..., from_r = true))
                  Us          "the scratch of the pre-factorisation (Vh L11^-1)" (comment above BigLayout)
                  vec         the loop's vectors (big_pre_factor only sets bvONE, bvPQ, bvY), ctrl (int words), pol (the
                              finishing stage), scal but [bsGt1] (written by the loop's phases)
                  the diagonal blocks of Lq and S11: "Nothing downstream reads the diagonal block of the factor itself"
                              (qpx_big.h, above BigPanelArgs) -- they keep the Schur complement the elimination started from
                  the upper block triangle of Lq (the copy of Q that big_pack_body left; big_potrf with mirror = 0), of R
                              ("lower block triangle (round 5: nothing reads the upper one any more)", big_gemm_r), and
                              W_kk' in Wq (kDiagNoWt: "nothing reads the transposed copy of this factor's blocks")

Checks, and the worst figure measured relative to its gate (the host-thread emulator | one MI355X):

  1. every word (check_blob): CASES -- B = 3 from problems.prof_qp(3, n, m, q, SEED), B = 2 for the large family -- under knob
     0, 1 << 14 (the sweep where the matrix-core form would run), 256 (Rg + Rw in float64) and 3 (the large family); the family
     the library reports (qpx_kernel_family) is asserted.  Knob 512 writes bitwise the blob of knob 256.
       measured: 8.2e-12 | 8.2e-12 at (101, 90, 0), knob 1 << 14, MT (lapack there 6.6e-12); ":rel" 2.1e-12 | 2.1e-12 (NTn at (64, 64, 40));
       360 figures over 57 cases, gate 1e-9 at every one
  2. conditioning (check_conditioning): Q = U diag(logspace(0, -c, n)) U', c = 2, 4, 6, 8, same gate rule (the 100 x lapack
     term decides from c = 6).
       measured, c = 8: 1.9e-9 | 1.9e-9 at (130, 70, 5), knob 3, Yt (lapack 6.7e-10, gate 6.7e-8); the sweep and the matrix-core form
       1.7e-10 .. 1.1e-9 in K, M, W and R, where the plain route has 6.0e-10 .. 4.3e-9.  No form's figure is above 4 x the plain route's at any c:
       none grows faster, and the factor 100 is never called on.  (q > 0 included: the sweep of the indefinite matrix at
       (100, 50, 10) stays BELOW the plain route at every c.)  Per c: profiles/prefac_blob.json, conditioning_ladder
  3. the other element types: wide=True (float32 tensors, float64 blob) against the reference of the float32-rounded data,
     float64 gate; QPX_F32 on kkt_checks.F32_SHAPES with problems.random_dense_qp (float32 blob, Rg + Rw).
       measured: wide 2.4e-12 | 2.4e-12 (gate 1e-9); QPX_F32 6.8e-7 | 6.8e-7 at (60, 112, 0), Kneg:rel (float32 torch: 3.6e-7; gate 1e-3
       at every shape: 100 x the float32 route never reaches it)
  4. soft rows (check_soft): w with zeros, 1e-8, 1e8 and values between, per QP and shared: only the diagonal of every R image
     and || G' 1 || differ from the hard blob; every other specified word is BITWISE the hard blob's; the diagonal and
     sqrt(|| G' 1 ||^2 + #{w_i > 0}) against the reference entry by entry (|a - ref| / max(1, |ref|): one 1e8 must not hide
     its neighbours).
       measured: diagonal 3.6e-12 | 3.6e-12 at (64, 64, 0), knob 3; gt1 <= 2.2e-16 on both; the bitwise part holds on both
  5. sharing and strides (check_strides, check_shared): Q un-batched with G batched and the reverse against the reference; Q, G,
     A all shared: ONE blob, sfac = 0, bitwise QP 0's of the expanded batch, once per family; the large family refuses
     (qpx_can_share_factors = 0) and writes B blobs.
       measured: 2.3e-12 | 2.3e-12; the bitwise part holds on both
  6. a failed QP leaves its neighbours alone (check_failure): batch of 3, QP 1 broken by Q[1, r, r] = -1 (r in the first, a
     middle, the last pivot block) or by a zero row of A[1]: status[1] is exactly QPX_ST_Q_NOT_SPD / QPX_ST_A_RANK, status[0]
     = status[2] = 0, the blobs of QPs 0 and 2 are bitwise the healthy batch's, and QP 1's blob is what include/qpx.h now
     documents: ALL ZEROS from the sweep and from the matrix-core form (both zero lay.total words); from the large family
     unspecified but for the failure bit in ctrl[bcFail] (a diagonal block that breaks down returns before it writes W_kk, and
     the launches behind it run on what is there).

Findings: none that needed a fix.  Both writers of family (a) zero-pad every R image they write, every compared word is written
in every form (no NaN met), the failed QP's blob is zeros in both, and no form loses more than the plain float64 route on the
conditioning ladder.  What was undocumented -- the failed QP's blob, the neighbours' bit identity -- is now in include/qpx.h.
The whole of tests/test_gpu_prefac.py (129 tests) is 7 s on the MI355X, tests/test_emu_prefac.py (130) 17 s.

What the gates see (scratch builds of the emulator with one deliberate error each, never committed):
  (a) qpx_grid.h, Rw written with a and b exchanged in the off-diagonal blocks: check 1 at the four knob-256 cases that hold an
      Rw (Rw 1.0 .. 1.1 at m = 24, 104; at m = 9, 60 the exchanged entries land in pads: "a pad of an R image is not an exact
      zero"), check 3 at the three QPX_F32 shapes with nbw <= 8 (0.63 .. 0.68 at (20, 24, 3) and (20, 40, 4), pads at (12, 9, 3)), check 4 at
      the two knob-256 cases with an Rw.  Nothing else: no other form writes an Rw.
  (b) the column sums of || G' 1 || without G's last row: gt1 at all 41 cases of check 1 that the sweep serves (4.6e-3 .. 1.0; gate
      1e-9), 8 of check 2, 7 of check 3, 10 of check 4 (20 figures, 1.6e-2 .. 0.24), 2 of check 5.  The matrix-core and large-family
      cases stay clean: they have their own sums.
  (c) the trailing (n + q) mod 4 pivots of the four-pivot groups skipped at NBL = 13: check 1 at the five cases with NBL = 13 and
      (n + q) mod 4 != 0 -- (101, 90, 0) under 1 << 14, (40, 130, 3) and (20, 170, 2) under both knobs -- every array, 0.69 ..
      2.8e3; QPX_F32 at (20, 170, 2), 0.32 .. 13.  (100, 100, 0), (n + q) mod 4 = 0, stays clean, as it must.
  (d) one pad entry of Rm (the last word of the image) left at 1e-300 by the sweep: the exact-zero assertion at 24 cases of check
      1 (every sweep-written Rm whose last tile is not full), 4 of check 2, the wide case of check 3 at (12, 9, 3), 3 cases of check 4, 1 of check 5; no figure moves.
  (e) qpx_big_host.inc, Ztp left unprojected: check 1 at the three large-family cases with q > 0 (Zt 3.7 .. 11, R 5.9 .. 62),
      all four of check 2's (0.17 .. 0.90), check 4 (diagonal 45 .. 1.8e2), check 5 at (120, 100, 10).  (65, 17, 0), q = 0, stays clean.

scripts/check_prefac.py runs all of it on the GPU and writes the figures, their gates, the reference-side figures and the
conditioning ladder to profiles/prefac_blob.json.
"""
import numpy as np
import torch

import kkt_checks
import loop_checks
import prefac_reference as R
import problems

figs = kkt_checks.figs
Gate = kkt_checks.Gate
tag = loop_checks.tag
SEED = loop_checks.SEED
TOL = 1e-9                 # float64 arithmetic: the gate the project holds blob against blob (test_matrix_core_prefactorisation_*)
TOL_F32 = 1e-3             # QPX_F32: the floor of max(1e-3, 100 x the float32 route's own error), the rule of kkt_checks
LAPACK_FACTOR = 100.0
B3 = 3
SWEEP, GRID16, GRID8, BIGK = 1 << 14, 256, 512, 3
FAMILY_GRID, FAMILY_TILE, FAMILY_BIG = 1, 2, 3
ST_Q_NOT_SPD, ST_A_RANK = 1, 2

# (n, m, q): the smallest shapes that reach each form and edge (the table of the issue this module answers)
SWEEP_SMALL = [(1, 1, 0), (6, 4, 2), (12, 9, 3), (16, 16, 0), (20, 24, 3), (17, 33, 2)]              # sweep NBL 1, 2, 4
SWEEP_MID = [(65, 17, 0), (33, 60, 7), (64, 64, 0)]                                                   # NBL 7, 8
SWEEP_GROUPS = [(100, 100, 0), (101, 90, 0), (100, 50, 10), (40, 130, 3), (16, 113, 0), (20, 170, 2)]   # NBL 10, 13: four-pivot groups, (n + q) mod 4 = 0, 1, 2, 3
MATRIX_CORE = [(30, 20, 3), (36, 40, 0), (64, 64, 0), (64, 64, 40), (100, 50, 10), (97, 111, 0)]      # 4 and 7 tile rows of n + q
MC_EDGES = [(29, 20, 3), (112, 3, 0), (113, 3, 0), (49, 1, 0)]                                        # n + q = 32 falls to the sweep; 112 | 113
RW_SHAPES = [(12, 9, 0), (12, 24, 0), (12, 60, 0), (12, 104, 0), (12, 130, 0)]                        # knob 256: nbw 2, 4, 8, 13, none
RG_SHAPES = [(40, 130, 0), (20, 170, 2)]                                                              # default knob, m > 112: nbg 10, 13
BIG_FORCED = [(12, 9, 3), (65, 17, 0), (130, 70, 5)]                                                  # knob 3: 1, 2, 3 blocks of 64
BIG = loop_checks.BIG                                                                                 # knob 0, n + q + m > 208


def _unique(seq):
    out = []
    for x in seq:
        if x not in out:
            out.append(x)
    return out


SHAPES01 = _unique(SWEEP_SMALL + SWEEP_MID + SWEEP_GROUPS + MATRIX_CORE + MC_EDGES + RG_SHAPES)
CASES = ([(s, k) for s in SHAPES01 for k in (0, SWEEP)] + [(s, GRID16) for s in RW_SHAPES]
         + [(s, BIGK) for s in BIG_FORCED] + [(BIG, 0)])
# (one launch per case: the whole list is seconds on the host-thread emulator too, so both runners take all of it)
COND_CS = (2, 4, 6, 8)
COND_CASES = [((64, 64, 0), 0), ((64, 64, 0), SWEEP), ((100, 50, 10), 0), ((100, 50, 10), SWEEP), ((130, 70, 5), BIGK)]
WIDE_SHAPES = [(100, 100, 0), (12, 9, 3), (100, 50, 10)]
F32_SHAPES = kkt_checks.F32_SHAPES
SOFT_KNOBS = (0, SWEEP, GRID16, BIGK)
SOFT_CASES = [(s, k) for s in [(12, 9, 3), (64, 64, 0), (100, 50, 10), (40, 130, 0)] for k in SOFT_KNOBS] + [((65, 17, 0), BIGK)]
STRIDE_CASES = [((12, 9, 3), 0), ((100, 50, 10), 0), ((40, 130, 0), 0), ((65, 17, 0), BIGK)]
SHARED_CASES = [((12, 9, 3), 0), ((100, 50, 10), 0), ((40, 130, 0), 0)]      # sweep -> tile image, matrix-core form, thread-grid family
# (shape, knob, how): how = ("Q", r): Q[1, r, r] = -1;  ("A", row): A[1, row] = 0
FAILURE_CASES = ([((12, 9, 3), 0, ("Q", r)) for r in (0, 6, 11)] + [((12, 9, 3), 0, ("A", 1))]               # the rank-1 sweep
                 + [((100, 50, 10), SWEEP, ("Q", r)) for r in (0, 50, 99)] + [((100, 50, 10), SWEEP, ("A", 5))]      # a pivot inside a group of four
                 + [((100, 50, 10), 0, ("Q", r)) for r in (3, 50, 98)] + [((100, 50, 10), 0, ("A", 5))]      # matrix-core; 98: the block with both kinds of pivot
                 + [((65, 17, 0), BIGK, ("Q", r)) for r in (0, 30, 64)] + [(BIG, 0, ("A", 5))])                # the large family

measured = {}        # "check/case/array" -> worst figure seen (scripts/check_prefac.py writes them to profiles/prefac_blob.json)
gates = {}           # the same keys -> the gate the figure was held to
reference_side = {}  # the same keys -> the float64 LAPACK (float32 torch) route's figure the gate rests on


class PGate(Gate):
    """kkt_checks.Gate filling this module's records"""

    def hold(self, key, value, gate, side=None):
        measured[key] = max(float(value), measured.get(key, 0.0))
        gates[key] = gate
        if side is not None:
            reference_side[key] = side
        print("%-64s %.3e  (gate %.1e%s)" % (key, value, gate, "" if side is None else ", lapack %.1e" % side))
        if not value <= gate:
            self.bad.append((key, value, gate))


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def batch_of(shape, knob, B=None):
    """B: the caller's own batch size (tests/big_checks.py)"""
    if B is not None:
        return B
    return 2 if (knob == BIGK or tuple(shape) == tuple(BIG)) else B3


def expected_family(shape, knob, dtype="f64"):
    """(qpx_kernel_family, image mask of the blob) as qpx_api.inc's blob_images decides them"""
    n, m, q = shape
    if (knob & 255) == 3 or R.grid_nb(n + q + m) == 0:
        return FAMILY_BIG, 8
    forced_grid = bool(knob & (GRID16 | GRID8))
    if dtype != "f32" and R.tile_nb(m) > 0 and not forced_grid:
        return FAMILY_TILE, 4
    return FAMILY_GRID, 3


def ladder_q(n, c, i):
    r = np.random.RandomState([SEED, n, c, i])
    U, _ = np.linalg.qr(r.randn(n, n))
    Q = (U * np.logspace(0, -c, n)) @ U.T
    return 0.5 * (Q + Q.T)


def problem(shape, B, dtype="f64", prob="prof"):
    """(Q, G, A) float64 arrays (B, n, n), (B, m, n), (B, q, n) holding what the tensors of `dtype` hold.  prob: "prof" =
    problems.prof_qp, "dense" = problems.random_dense_qp, "cond<c>" = prof_qp with Q from the conditioning ladder, "Q0" / "G0"
    / "shared" = prof_qp with QP 0's Q / G / Q, G and A for every QP"""
    def make():
        n, m, q = shape
        gen = problems.random_dense_qp if prob == "dense" else problems.prof_qp
        Q, _, G, _, A, _ = gen(B, n, m, q, seed=SEED)
        A = A if q else np.zeros((B, 0, n))
        if prob.startswith("cond"):
            Q = np.stack([ladder_q(n, int(prob[4:]), i) for i in range(B)])
        if prob in ("Q0", "shared"):
            Q = np.broadcast_to(Q[:1], Q.shape).copy()
        if prob in ("G0", "shared"):
            G = np.broadcast_to(G[:1], G.shape).copy()
        if prob == "shared":
            A = np.broadcast_to(A[:1], A.shape).copy()
        out = tuple(kkt_checks.rounded(x, "f64" if dtype == "f64" else "f32") for x in (Q, G, A))
        for x in out:
            x.setflags(write=False)
        return out
    return cached(("problem", tuple(shape), B, dtype, prob), make)


def _side_f32(Q, G, A):
    """the arrays of family (a) by float32 torch operations"""
    n = Q.shape[0]
    Qt, Gt, At = [torch.tensor(x, dtype=torch.float32) for x in (Q, G, A)]
    H = torch.zeros(n + At.shape[0], n + At.shape[0])
    H[:n, :n], H[:n, n:], H[n:, :n] = Qt, At.T, At
    X = torch.linalg.inv(H)
    K, N = X[:n, :n], X[:n, n:]
    GK = Gt @ K
    out = {"Kneg": -K, "MT": GK.T, "NTn": -N.T, "W": Gt @ N, "S11i": -X[n:, n:], "R": GK @ Gt.T, "gt1": Gt.sum(0).norm().reshape(1)}
    return {k: v.numpy().astype(np.float64) for k, v in out.items()}


def rel(a, ref):
    """max |a - ref| / max |ref|: figs without its floor of 1 under the norm, for the arrays whose entries are all below 1"""
    a, ref = np.asarray(a, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    if ref.size == 0 or not np.abs(ref).max() > 0:
        return 0.0
    f = np.abs(a - ref).max() / np.abs(ref).max()
    return float(f) if np.isfinite(f) else float("inf")


class Ref:
    """One batch's references (made once, shared by every knob and by both runners): per QP the arrays of the family, the
    plain float64 (float32) route's figure per array, the residual of the refined inverse"""

    def __init__(self, shape, B, dtype, prob, big, qps=None):
        self.shape, self.B, self.big = tuple(shape), B, big
        Q, G, A = problem(shape, B, dtype, prob)
        self.per_qp, self.side, self.side_rel = {}, {}, {}          # (per_qp: QP -> its arrays; qps: the QPs that get one)
        floor = TOL_F32 if dtype == "f32" else TOL
        for i in (range(B) if qps is None else qps):
            if big:
                # (the gate of R is not known before its lapack figure is: the two routes to R are first held to 1e-3 x the
                # floor, and to 1e-3 x the gate of R below)
                ref = R.big_reference(Q[i], G[i], A[i], tol=np.inf)
                lay = R.LayoutBig(*shape)
                want, lap = R.expected_big(ref, lay), R.expected_big(R.lapack_side_big(Q[i], G[i], A[i]), lay)
                side = {k: figs(lap[k][1][None], want[k][1][None]) for k in want}
                assert ref["r_gap"] <= 1e-3 * max(floor, LAPACK_FACTOR * side["R"]), ("the two routes to R disagree", shape, ref["r_gap"])
            else:
                ref = R.reference(Q[i], G[i], A[i])
                lap = _side_f32(Q[i], G[i], A[i]) if dtype == "f32" else R.lapack_side(Q[i], G[i], A[i])
                side = {k: figs(np.asarray(lap[k], np.float64).reshape(1, -1), np.asarray(ref[k], np.float64).reshape(1, -1)) for k in R.NAMES_A}
            self.per_qp[i] = ref
            for k, v in side.items():
                self.side[k] = max(v, self.side.get(k, 0.0))
            if not big:
                for k in R.NAMES_A:
                    self.side_rel[k] = max(rel(lap[k], ref[k]), self.side_rel.get(k, 0.0))
        self.gate = {k: max(floor, LAPACK_FACTOR * v) for k, v in self.side.items()}
        self.gate_rel = {k: max(floor, LAPACK_FACTOR * v) for k, v in self.side_rel.items()}
        self.resid = max(r["resid"] for r in self.per_qp.values())
        # || dX || <= || X || || I - H X ||: the residual bounds the reference's error relative to the LARGEST block of H^-1, the
        # one that carries the conditioning and has the case's largest gate (K; Lq^-1 in the large family) -- that gate it is
        # held to.  (What np.longdouble leaves of it is its own rounding, 2^-64 |H| |X|: 8.9e-12 at cond(Q) = 1e8, where the
        # largest gate is 4e-7; tests/test_prefac_reference.py measures 2.2e-14 against mpmath at such a Q.)
        assert self.resid <= 1e-3 * max(self.gate.values()), ("the reference's own residual", shape, prob, self.resid)

    def gate_of(self, name):
        return self.gate["R" if name in R.IMAGE_INDEX else name]        # an image of R: R's gate

    def side_of(self, name):
        return self.side["R" if name in R.IMAGE_INDEX else name]


def reference(shape, B, dtype="f64", prob="prof", big=False, qps=None):
    key = ("ref", tuple(shape), B, dtype, prob, big) + (() if qps is None else (tuple(qps),))
    return cached(key, lambda: Ref(shape, B, dtype, prob, big, qps))


class Built:
    """the blobs (nblob, elems) and status words of one KKTFactors.build, on the host, with what the library said about it"""

    def __init__(self, env, shape, arrs, knob, dtype="f64", w=None, B=None, raise_on_failure=True):
        from qpth_amd.kkt import KKTFactors
        n, m, q = shape
        td = torch.float64 if dtype == "f64" else torch.float32
        dev = lambda x: None if (x is None or np.size(x) == 0) else torch.tensor(np.asarray(x, np.float64), dtype=td, device=env.dev)     # noqa: E731
        with env.run(knob):
            fac = KKTFactors.build(dev(arrs[0]), dev(arrs[1]), dev(arrs[2]), B, wide=(dtype == "wide"), w=dev(w))
            if raise_on_failure:
                fac.raise_on_failure()
            self.family = int(fac.lib.dll.qpx_kernel_family(fac.code, n, m, q))
            self.can_share = int(fac.lib.dll.qpx_can_share_factors(fac.code, n, m, q))
        self.fac = fac
        self.blob = fac.blob.detach().reshape(-1, fac.elems).cpu().numpy().copy()
        self.status = fac.status.detach().cpu().numpy().copy()
        assert self.blob.dtype == (np.float32 if dtype == "f32" else np.float64)

    def bits(self):
        return self.blob.view(np.int32 if self.blob.dtype == np.float32 else np.int64)


def layout_of(shape, knob, dtype, built):
    """the layout this module expects, after asserting that the library reports the family it knows and sizes the blob alike"""
    fam, images = expected_family(shape, knob, dtype)
    assert built.family == fam, ("qpx_kernel_family", shape, knob, dtype, built.family, fam)
    lay = R.LayoutBig(*shape) if fam == FAMILY_BIG else R.LayoutA(*shape, images)
    assert built.blob.shape[1] == lay.total, ("qpx_factor_elems", shape, knob, built.blob.shape, lay.total)
    return fam, lay


def uncompared_big(lay, compared):
    """every word of the large family's blob that the docstring lists as not compared; asserts that these and `compared` (the
    index arrays of expected_big) tile [0, total)"""
    claimed = np.zeros(lay.total, np.int32)
    for idx in compared:
        np.add.at(claimed, idx, 1)
    for name in ("T", "Wt", "Us", "vec", "ctrl", "pol"):
        claimed[lay.off[name]:lay.off[name] + lay.size[name]] += 1
    scal = lay.off["scal"] + np.arange(16)
    claimed[scal[scal != lay.off["scal"] + R.BS_GT1]] += 1
    i, j = np.meshgrid(np.arange(lay.NP), np.arange(lay.NP), indexing="ij")
    keep = (i // 64) <= (j // 64)                                 # Lq: its diagonal blocks and everything above them
    claimed[lay.off["Lq"] + R.big_at(lay.NP, i[keep], j[keep])] += 1
    i, j = np.meshgrid(np.arange(lay.MP), np.arange(lay.MP), indexing="ij")
    keep = (i // 64) < (j // 64)                                  # R: the upper block triangle
    claimed[lay.off["R"] + R.big_at(lay.MP, i[keep], j[keep])] += 1
    for k in range(lay.NP // 64):                                 # Wq: the transposed halves
        claimed[lay.off["Wq"] + k * 8192 + 4096:lay.off["Wq"] + (k + 1) * 8192] += 1
    for k in range(lay.QP // 64):                                 # S11: its diagonal blocks
        claimed[lay.off["S11"] + R.big_blk(lay.QP, k, k):lay.off["S11"] + R.big_blk(lay.QP, k, k) + 4096] += 1
    if lay.q == 0:
        for name in ("Yt", "S11", "Wy", "Vh"):
            assert lay.size[name] == 0
    assert (claimed == 1).all(), ("the parts do not tile the blob", int((claimed == 0).sum()), int((claimed > 1).sum()))
    return claimed


def expected(ref, i, fam, lay, w=None):
    """QP i's blob as the reference has it: name -> (word indices, values), the pads' indices, and the specified words (bool)"""
    arrs = dict(ref.per_qp[i])
    if w is not None:
        R.soften(arrs, w)
    if fam == FAMILY_BIG:
        exp = R.expected_big(arrs, lay)
        spec = np.zeros(lay.total, bool)
        for idx, _ in exp.values():
            spec[idx] = True
        cached(("tiles_big", lay.n, lay.m, lay.q), lambda: uncompared_big(lay, [idx for idx, _ in exp.values()]))
        return exp, np.zeros(0, np.int64), spec
    vals, kind, regions = R.expected_a(arrs, lay)            # (asserts that the three parts tile the blob)
    exp = {name: (np.arange(o, o + size), vals[o:o + size]) for name, (o, size) in regions.items()}
    return exp, np.flatnonzero(kind == 2), kind != 1


def compare(g, key, built, ref, fam, lay, ws=None, only=None, qps=None):
    """every compared array of every QP of `built` (of the QPs `qps`) against the reference (worst over the QPs per array), the
    pads exact zeros"""
    worst, worst_rel = {}, {}
    for i in (range(built.blob.shape[0]) if qps is None else qps):
        exp, pads, _ = expected(ref, i, fam, lay, None if ws is None else ws[i])
        for name, (idx, vals) in exp.items():
            if only is None or name in only:
                worst[name] = max(worst.get(name, 0.0), figs(built.blob[i, idx][None], vals[None]))
                if name in ref.gate_rel and 0 < np.abs(vals).max() < 1:          # (family (a): NTn, S11i, at some shapes Kneg)
                    worst_rel[name] = max(worst_rel.get(name, 0.0), rel(built.blob[i, idx], vals))
        assert (built.blob[i, pads] == 0).all(), ("a pad of an R image is not an exact zero", key, i, int((built.blob[i, pads] != 0).sum()))
    for name, v in worst.items():
        g.hold("%s/%s" % (key, name), v, ref.gate_of(name), ref.side_of(name))
    for name, v in worst_rel.items():
        g.hold("%s/%s:rel" % (key, name), v, ref.gate_rel[name], ref.side_rel[name])


# ---------------------------------------------------------------- 1, 2, 3: every word
def check_blob(env, shape, knob, dtype="f64", prob="prof", check="blob", B=None):
    key = ("built", env.dev.type, tuple(shape), knob, dtype, prob) + (() if B is None else (B,))
    B = batch_of(shape, knob, B)
    fam = expected_family(shape, knob, dtype)[0]
    built = cached(key, lambda: Built(env, shape, problem(shape, B, dtype, prob), knob, dtype))
    assert (built.status == 0).all() and built.blob.shape[0] == B
    fam, lay = layout_of(shape, knob, dtype, built)
    ref = reference(shape, B, dtype, prob, fam == FAMILY_BIG)
    g = PGate()
    extra = ("" if dtype == "f64" else "/" + dtype) + ("" if prob in ("prof", "dense") else "/" + prob)
    compare(g, "%s/%s%s" % (check, tag(shape, knob), extra), built, ref, fam, lay)
    g.done()
    return built


def check_knob_512_writes_the_blob_of_knob_256(env, shape=(12, 24, 0)):
    arrs = problem(shape, B3)
    a, b = Built(env, shape, arrs, GRID16), Built(env, shape, arrs, GRID8)
    assert a.blob.shape == b.blob.shape and np.array_equal(a.bits(), b.bits())


def check_conditioning(env, shape, knob, c):
    check_blob(env, shape, knob, prob="cond%d" % c, check="cond")


def check_wide(env, shape):
    built = check_blob(env, shape, 0, dtype="wide", check="wide")
    assert built.fac.wide and built.blob.dtype == np.float64


def check_f32(env, shape):
    built = check_blob(env, shape, 0, dtype="f32", prob="dense", check="f32")
    assert not built.fac.wide and built.blob.dtype == np.float32 and built.family == FAMILY_GRID


# ---------------------------------------------------------------- 4: soft rows
W_VALUES = np.array([0.0, 1e-8, 1e8, 0.5, 0.0, 3.0, 1e-3, 1e3])


def soft_w(m, B):
    """(B, m): zeros, a 1e-8, a 1e8 and values between, another rotation per QP"""
    return np.stack([np.resize(np.roll(W_VALUES, i), m) for i in range(B)])


def each(a, ref):
    """max over the entries of |a - ref| / max(1, |ref|)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    f = np.abs(a - ref) / np.maximum(1.0, np.abs(ref))
    return float(f.max()) if np.isfinite(f).all() else float("inf")


def check_soft(env, shape, knob):
    B = batch_of(shape, knob)
    n, m, q = shape
    arrs = problem(shape, B)
    hard = cached(("built", env.dev.type, tuple(shape), knob, "f64", "prof"), lambda: Built(env, shape, arrs, knob))
    fam, lay = layout_of(shape, knob, "f64", hard)
    ref = reference(shape, B, big=(fam == FAMILY_BIG))
    g = PGate()
    for mode in ("per_qp", "shared"):
        ws = soft_w(m, B) if mode == "per_qp" else np.broadcast_to(soft_w(m, 1), (B, m))
        soft = Built(env, shape, arrs, knob, w=(ws if mode == "per_qp" else ws[0]))
        assert (soft.status == 0).all() and soft.blob.shape == hard.blob.shape and soft.fac.soft
        key = "soft/%s/%s" % (tag(shape, knob), mode)
        worst_d, worst_g = 0.0, 0.0
        for i in range(B):
            exp, pads, spec = expected(ref, i, fam, lay, ws[i])
            if fam == FAMILY_BIG:
                diag = {"R": R.big_r_diagonal(lay)}
                gt1 = lay.off["scal"] + R.BS_GT1
            else:
                diag = {name: lay.off[name] + R.image_diagonal(name, m) for name in lay.image_names()}
                gt1 = lay.off["gt1"]
            same = spec.copy()
            same[gt1] = False
            for idx in diag.values():
                same[idx] = False
            differ = np.flatnonzero(same & (soft.bits()[i] != hard.bits()[i]))
            assert differ.size == 0, ("a word beside the diagonal of R and || G' 1 || differs from the hard blob", key, i, differ[:8])
            assert (soft.blob[i, pads] == 0).all()
            want = np.asarray(np.diag(ref.per_qp[i]["R"]), np.float64) + ws[i]
            for name, idx in diag.items():
                worst_d = max(worst_d, each(soft.blob[i, idx], want))
                hard_rows = ws[i] == 0                      # a hard row's diagonal entry is the hard blob's, bit for bit
                assert np.array_equal(soft.bits()[i, idx[hard_rows]], hard.bits()[i, idx[hard_rows]]), (key, name)
            worst_g = max(worst_g, each(soft.blob[i, gt1], exp["gt1"][1][0]))
        g.hold(key + "/diag", worst_d, ref.gate_of("R"), ref.side_of("R"))
        g.hold(key + "/gt1", worst_g, ref.gate_of("gt1"), ref.side_of("gt1"))
    g.done()


# ---------------------------------------------------------------- 5: sharing and strides
def check_strides(env, shape, knob):
    """Q un-batched (2-D) beside a batched G, and the reverse: every QP's blob against the reference of the expanded batch"""
    B = batch_of(shape, knob)
    g = PGate()
    for prob, which in (("Q0", 0), ("G0", 1)):
        arrs = list(problem(shape, B, prob=prob))
        arrs[which] = arrs[which][0]
        built = Built(env, shape, arrs, knob, B=B)
        assert (built.status == 0).all() and built.blob.shape[0] == B and not built.fac.shared
        fam, lay = layout_of(shape, knob, "f64", built)
        compare(g, "strides/%s/%s" % (tag(shape, knob), prob), built, reference(shape, B, prob=prob, big=(fam == FAMILY_BIG)), fam, lay)
    g.done()


def check_shared(env, shape, knob=0):
    """Q, G, A all un-batched: one blob, sfac = 0, bitwise QP 0's blob of the expanded batch"""
    arrs = problem(shape, B3, prob="shared")
    one = Built(env, shape, [x[0] for x in arrs], knob, B=B3)
    per = Built(env, shape, arrs, knob)
    assert one.can_share == 1 and one.fac.shared and one.fac.sfac == 0 and one.blob.shape[0] == 1 and per.blob.shape[0] == B3
    assert (one.status == 0).all() and one.status.shape == (B3,)
    fam, lay = layout_of(shape, knob, "f64", one)
    _, _, spec = expected(reference(shape, B3, prob="shared"), 0, fam, lay)
    for i in range(B3):
        assert np.array_equal(one.bits()[0, spec], per.bits()[i, spec]), ("the shared blob against the expanded batch's", shape, i)


def check_large_family_refuses_sharing(env, shape, knob):
    arrs = problem(shape, 2, prob="shared")
    built = Built(env, shape, [x[0] for x in arrs], knob, B=2)
    fam, lay = layout_of(shape, knob, "f64", built)
    assert fam == FAMILY_BIG and built.can_share == 0 and not built.fac.shared and built.fac.sfac == lay.total and built.blob.shape[0] == 2
    g = PGate()
    compare(g, "strides/%s/shared" % tag(shape, knob), built, reference(shape, 2, prob="shared", big=True), fam, lay)
    g.done()


# ---------------------------------------------------------------- 6: a failed QP leaves its neighbours alone
def check_failure(env, shape, knob, how):
    n, m, q = shape
    arrs = problem(shape, B3)
    healthy = cached(("built3", env.dev.type, tuple(shape), knob), lambda: Built(env, shape, arrs, knob))
    assert (healthy.status == 0).all()
    fam, lay = layout_of(shape, knob, "f64", healthy)
    Q, G, A = [x.copy() for x in arrs]
    if how[0] == "Q":
        Q[1, how[1], how[1]] = -1.0
        want = ST_Q_NOT_SPD
    else:
        A[1, how[1]] = 0.0              # (b plays no part in the pre-factorisation: nothing to zero beside it here)
        want = ST_A_RANK
    broken = Built(env, shape, (Q, G, A), knob, raise_on_failure=False)
    assert broken.status.tolist() == [0, want, 0], ("status", shape, knob, how, broken.status.tolist())
    import pytest
    with pytest.raises(RuntimeError, match="LU factorization on Q" if want == ST_Q_NOT_SPD else "full row rank"):
        broken.fac.raise_on_failure()
    if fam == FAMILY_BIG:
        exp, _, spec = expected(reference(shape, B3, big=True), 0, fam, lay)
    else:
        spec = expected(reference(shape, B3), 0, fam, lay)[2]
    for i in (0, 2):
        assert np.array_equal(broken.bits()[i, spec], healthy.bits()[i, spec]), ("a neighbour of the failed QP", shape, knob, how, i)
    if fam == FAMILY_BIG:
        # unspecified but for the failure bit among the control words (int32 words at the place of ctrl)
        ctrl = broken.blob[1, lay.off["ctrl"]:lay.off["ctrl"] + 16].view(np.int32)
        assert ctrl[R.BC_FAIL] == want
    else:
        assert (broken.bits()[1] == 0).all(), ("the failed QP's blob is not all zeros", shape, knob, how)
