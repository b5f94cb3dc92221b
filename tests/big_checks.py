"""The large-QP family (qpx_big.h, qpx_big_host.inc) at ITS OWN sizes -- 4 to 16 blocks of 64 per dimension, the
batch worked on in parts, the knob's variant bits 26..29 -- held by the checks that already hold it at one to three blocks:
tests/loop_checks.py (the path of the interior-point loop against oracle/qp_oracle), tests/kkt_checks.py (the KKT-solve kernels
in every role against a dense solve refined in extended precision) and tests/prefac_checks.py (the factor blob word by word
against a longdouble reference).  This module holds the shape table, the knob variants and the few checks that are new (the
host forms, bit for bit); every reference, gate and error measure is the three modules'.  tests/test_emu_big.py runs it on the
host-thread emulator, tests/test_gpu_big.py on a real MI355X; every check takes an `env` as theirs do.

Why: the three modules reach this family at 1, 2 and 3 blocks (knob 3 at (12, 9, 3), (65, 17, 0), (130, 70, 5)) and at knob 0 at
(120, 100, 10) alone, always in a batch of two.  The family has code that depends on the block count and on the batch, none of
which runs there: the streamed blocks of big_trsv_body (the first at 4 blocks, all five slots at 8), its kLong instantiation
(nb > 8; rounds of MS = 5: two from 9 blocks, two full ones at 13, a third from 14, 16 the limit), big_ns_form (NS = 4 full at 4
blocks, NS = 8 at 5 to 8, NS = 16 from 9), big_gemv_body's LDS (8 blocks up to 512, 16 beyond), big_symv_body's slot per (I, J)
block pair, L11 = chol(A Q^-1 A') with its mirrored upper blocks, Wy and Vh in more than one block (neq > 64), big_split (2 to 4
parts on side streams, boundaries rounded to 8 once B >= 16 parts, pointer offsets per part), launch_big_gemm's XCD-ordered grid
(B % 8 == 0), and the variant bits 26 to 29.  Above three blocks the family was held end to end only (converged zhat at 1e-6),
and an interior-point loop corrects itself: a wrong Newton direction arrives by another path (tests/loop_checks.py).

Shapes: SHAPES, (n, m, q) at knob 0 with B = 2, each the smallest that reaches its path (the comment beside it), one dimension
long.  problems.prof_qp with loop_checks.SEED; (520, 40, 0) takes problems.random_dense_qp (prob_of).  At (70, 250, 0) the two QPs
stop after 14 and 13 passes at eps = 1e-8 (asserted: check_one_qp_stops_beside_a_running_one), so one QP's early return (bcStop)
beside a running one is exercised.

Checks per shape, every one on the gate of its module, and the worst figure (the host-thread emulator | one MI355X; the
emulator's list is shorter, see below):
  1. loop_checks: iterates after k in KS (k in (1, 3) above 512 in any dimension), counts and trace at eps = 1e-8, the best
     iterate's bookkeeping, stall_policy = 0; float32 tensors in float64 arithmetic at (40, 520, 0) (GPU).
       iterates 3.8e-8 | 3.8e-8 and best_resid after k 1.6e-7 | 1.6e-7 (gate TOL = 1e-6), trace 3.8e-7 | 3.8e-7 (1e-6), trace_rel
       2.9e-6 | 2.9e-6 (TRACE_REL = 1.979e-5), all at (150, 70, 130); best-iterate bookkeeping 0 | 0 (1e-12); wide - | 4.8e-8 (1e-5)
  2. kkt_checks: solve, backward with and without the duals cotangents, forward mode with the adjoint identity, both d ("bwd",
     "mid"), on its Gate rule max(1e-8, 100 x the unrefined float64 dense solve against the refined reference) (tol_of with
     cond_rule=True).  The rule decided NO case (kkt_checks.rule_decided, recorded per case): the unrefined solve is at most
     3.1e-12 | 6.5e-12 from the refined one (at (150, 70, 130), "bwd"; 6.0e-14 at (64, 1024, 0), order 1 088), so every gate
     is 1e-8.
       solve 2.2e-10 | 3.0e-10, ds with an rs 1.5e-7 | 2.2e-7 (1e-6), backward 4.4e-10 | 4.4e-10, forward mode 3.0e-10 | 3.0e-10,
       adjoint 3.0e-12 | 6.2e-12 (1e-10)
     K right-hand sides and the second-order pass are declined by this family: the *_supported queries are asserted to say
     so, as the module does, and nothing runs (check_declined_roles).
     QPX_F32 (the family's float32 kernels) once, (70, 250, 0), random_dense_qp, the "mid" d, kkt_checks' float32 gate
     max(1e-3, 100 x a float32 torch solve) = 1e-3: 2.1e-5 | 2.1e-5 (ds with an rs; forward mode 1.5e-5)
  3. prefac_checks.check_blob, every word and the parts tiling the blob, at BLOB_SHAPES.
       worst relative to its gate: Vh at (250, 70, 20), 3.1e-11 | 3.0e-11 against 2.1e-9 (the plain float64 route: 2.1e-11); the
       100 x lapack term decides the gates of Wq, Yt, Vh at (250, 70, 20) (2.1e-9 .. 3.5e-9) and nowhere else among SHAPES
     (520, 40, 0) is in NO blob check: prefac_reference.big_reference is 6.4 s per QP there (its refined longdouble inverse of
     order 520, four Newton corrections of two longdouble products each), against 0.1 .. 1.6 s at BLOB_SHAPES, and it was not
     made faster here.  The shape keeps its loop and KKT checks.

The host forms (HOST): on (130, 70, 5) under knob 3 and (70, 250, 0) under knob 0 the batch in 2 and 3 parts of B = 5 (2 + 3,
1 + 2 + 2), 4 parts of B = 5, 2 parts of B = 33 (16 + 17: the boundary rounded to 16), 3 parts of B = 48 (16 + 16 + 16), bit 26
(no helper stream) at B = 2 and bit 29 (the plain GEMM grid) at B = 8, where the default takes the XCD-ordered one: every
specified word of every QP's blob, the loop's result at eps = 1e-8 with its trace, the finishing stage's result, the KKT solve
and the backward (which do not split: big_split's `allow`) equal the one-part default launch of the same batch BIT FOR BIT
(check_host_form) -- all 14 hold on the MI355X, the 9 of EMU_HOST on the emulator.  These knobs move launches between streams
and tiles between workgroups; no addition is reordered.  On the emulator, which runs streams one after the other, the
comparison only guards the pointer offsets (adv, advio) and the part boundaries; the forks, joins and events are the MI355X's
part.  The default launch itself is held against the references at QPs 0, B - 1 and the last QP of every part
(check_default_launch: trace_rel <= 2.3e-7 | 2.3e-7 at (130, 70, 5), B = 5; the blob on its gates).  Bits 27 and 28, the two
other eliminations of a diagonal block, are other arithmetic: checks 1 to 3 at (70, 250, 0) on their gates (GPU: iterates 9.7e-11 and 8.8e-11, every figure
within those above).

What the gates see (scratch builds of the emulator with one deliberate error each, never committed; for these the nine-block
shapes, (40, 500, 0) and the B = 33 forms ran on the emulator once):
  (a) big_trsv_body<kLong>, the second round's blocks skipped (j0 += 2 MS): (40, 520, 0) iterates 5.3e2 .. 7.5e2, counts 9 / 8
      against 13, solve 2.7e3 (ds 1.5); (520, 40, 0) iterates 7.8e-2, solve 0.14.  (40, 500, 0) and everything below: clean.
  (b) big_ns_form, 9 blocks sent to the NS = 8 form: (40, 520, 0) iterates 2.1e3 (the start point already), counts 4 / 4 against
      13.  The KKT solve and the blob there stay clean (their launches hold no vector in NS slots), as does every other shape.
  (c) big_split, the second part starting 8 QPs late at B = 33: the 2-part form at B = 33 alone (QPs 16 .. 23 keep the words
      they had: their status is not the default launch's zeros).  Every other form and batch: clean.
  (d) big_symv_body, slot (I, J) read as (J, I) in the second launch: the loop from two block rows up -- all three shapes up to
      four blocks, (130, 70, 5), (40, 500, 0), (40, 520, 0): the unwritten slot is the NaN of conftest.py, best_resid is not
      finite and the counts are 1 against 9 .. 14.  The KKT solve and the blob (no R z' in them): clean.
  (e) L11's mirrored upper blocks left unwritten (big_potrf's panel launch with mirror = 0): (150, 70, 130) in every check --
      blob L11T 1.0e2, Zt 4.0e7, R 8.6e15, the breakdown bit in the KKT roles, counts 0.  (250, 70, 20) and (130, 70, 5), neq in
      one block: clean.

The two runners.  tests/test_gpu_big.py: everything above, 107 tests in 17 s on the MI355X, most of it the CPU references
(ref_seconds; the longest: the oracle at (64, 1024, 0) 2.4 s, the blob references 0.6 .. 4.9 s per case).  tests/test_emu_big.py:
the three shapes up to four blocks in full, the host forms at B <= 5 on both shapes and B = 8 at (130, 70, 5), and at nine
blocks the iterates ((40, 520, 0) 8 s, (520, 40, 0) 3 s), counts and trace (18 s), the KKT solve with the "mid" d (5 s) and the
blob (1 s).  Left to the GPU runner, with the emulator's seconds that decided it: B = 8 at (70, 250, 0) (38 s a launch), B = 33
(84 s a launch at (130, 70, 5)) and B = 48; (40, 500, 0) and the shapes from 13 blocks (they add no path to the emulator's nine
blocks but rounds, and the best-iterate and stall checks re-run the loop three times: 15 s each at four blocks already); the
"bwd" d at nine blocks; bits 27 and 28.  Per test on the emulator: <= 23 s; the module, 50 tests, 380 s.

scripts/check_big.py runs the GPU list (--emu: the emulator's) and writes every figure, its gate, the reference-side figure
and the references' CPU seconds per case to profiles/big_blocks.json.
"""
import time
import types

import numpy as np
import torch

import kkt_checks as K
import loop_checks as L
import prefac_checks as P

tag = L.tag
B2 = 2
# (n, m, q) at knob 0, B = 2: each the smallest shape that reaches its path, one dimension long (the CPU references stay cheap)
SHAPES = [
    (70, 250, 0),         # 2 / 4 / 0 blocks: NS = 4 full; the first streamed block (substitutions on T); 4 block rows of the symv
    (250, 70, 20),        # 4 / 2 / 1: the same on Lq; Zt and M wider than tall; neq in one block beside it
    (150, 70, 130),       # 3 / 2 / 3: L11, Wy, Vh in three blocks; every dimension one block count apart
    (40, 500, 0),         # 1 / 8 / 0: NS = 8 full; all five streamed slots; the last size of the short substitution and the 8-block gemv LDS
    (40, 520, 0),         # 1 / 9 / 0: NS = 16; kLong, two rounds; the 16-block mat-vec LDS
    (520, 40, 0),         # 9 / 1 / 0: kLong on Lq (the recovery of zhat and dx); a 9-block Cholesky and solve in the pre-factorisation
    (40, 800, 0),         # 1 / 13 / 0: two full rounds exactly
    (40, 840, 0),         # 1 / 14 / 0: the third round
    (64, 1024, 0),        # 1 / 16 / 0: the limit, no padding anywhere
]
BLOCKS = [(2, 4, 0), (4, 2, 1), (3, 2, 3), (1, 8, 0), (1, 9, 0), (9, 1, 0), (1, 13, 0), (1, 14, 0), (1, 16, 0)]
UP_TO_FOUR_BLOCKS = SHAPES[:3]                    # what the emulator runs in full
NINE_BLOCKS = (40, 520, 0)                        # the emulator: the loop's path, the KKT solve with the "mid" d, the blob
NINE_BLOCKS_LQ = (520, 40, 0)                     # the emulator: the iterates after k = 1, 3
WIDE_SHAPE = (40, 520, 0)
F32_SHAPE = (70, 250, 0)
# the blob word by word; (520, 40, 0) is not in it: prefac_reference.big_reference is 6.4 s per QP there (see the docstring)
BLOB_SHAPES = [(70, 250, 0), (250, 70, 20), (150, 70, 130), (40, 520, 0), (64, 1024, 0)]
# the host forms, forced at a small size: (shape, the knob the one-part default launch runs under)
HOST_BASES = [((130, 70, 5), 3), ((70, 250, 0), 0)]
PARTS = [(2, 5), (3, 5), (4, 5), (2, 33), (3, 48)]           # (bits 16..19, B): 2 + 3, 1 + 2 + 2, 1 + 1 + 1 + 2, 16 + 17, 16 + 16 + 16
BIT26, BIT27, BIT28, BIT29 = 1 << 26, 1 << 27, 1 << 28, 1 << 29
HOST_FORMS = [(parts << 16, B) for parts, B in PARTS] + [(BIT26, 2), (BIT29, 8)]      # scheduling alone: bit for bit
HOST = [(s, base, v, B) for s, base in HOST_BASES for v, B in HOST_FORMS]
# the emulator: the batches up to 8, and B = 8 at the three-block shape alone (at (70, 250, 0) that launch is 38 s of fibres)
EMU_HOST = [c for c in HOST if c[3] <= 5 or (c[3] == 8 and c[0] == (130, 70, 5))]
DIAG_FORMS = [BIT27, BIT28]                                  # other arithmetic in the diagonal blocks: checks 1 to 3 on their gates

ref_seconds = {}     # case -> CPU seconds the references of its checks took (scripts/check_big.py writes them out)
bitwise = {}         # host form -> did every comparison hold bit for bit


def prob_of(shape):
    """(520, 40, 0): problems.random_dense_qp (Q = L L'/n + I) -- prof_qp has cond(Q) near 1e8 at n = 520, and the figures
    would measure that, which is prefac_checks' check 2; every other shape: problems.prof_qp with loop_checks.SEED"""
    return "dense" if tuple(shape) == (520, 40, 0) else "prof"


def ks_of(shape):
    """above 512 in any dimension the oracle is seconds per capped run: k in (1, 3) -- the start point and two full passes"""
    return (1, 3) if max(shape) > 512 else L.KS


def bound(B, parts, i):
    """big_split's part boundaries (qpx_big_host.inc), restated: multiples of 8 once B >= 16 parts"""
    if i >= parts:
        return B
    x = B * i // parts
    return (x + 4) // 8 * 8 if B >= 16 * parts else x


def part_lengths(B, parts):
    return [bound(B, parts, i + 1) - bound(B, parts, i) for i in range(parts)]


def referenced_qps(B):
    """the QPs of a host-form batch that are held against the references: 0, B - 1 and the last QP of every part of every
    split of that batch (it sits behind the part's pointer offsets)"""
    qps = {0, B - 1}
    for parts, b in PARTS:
        if b == B:
            qps |= {bound(B, parts, i + 1) - 1 for i in range(parts)}
    return sorted(qps)


def timed(key, fn):
    t0 = time.process_time()
    out = fn()
    ref_seconds[key] = ref_seconds.get(key, 0.0) + time.process_time() - t0
    return out


# ---------------------------------------------------------------- 1. loop_checks
def warm_oracle(shape, B=B2, qps=None):
    """the oracle's runs of checks 1 and 2 made (and timed) before the launches: loop_checks.oracle keeps them"""
    prob = prob_of(shape)

    def make():
        for i in (range(B) if qps is None else qps):
            L.oracle(shape, B, i, 1e-8, 20, True, "f64", prob)
            if qps is None:
                for k in ks_of(shape):
                    L.oracle(shape, B, i, 1e-12, k, False, "f64", prob)
    timed("loop/" + tag(shape) + ("" if B == B2 else "/B%d" % B), make)


def check_iterates_after_k(env, shape, form=0):
    warm_oracle(shape)
    L.check_iterates_after_k(env, shape, form, ks_of(shape), B2, prob_of(shape))


def check_counts_and_trace(env, shape, form=0):
    warm_oracle(shape)
    L.check_counts_and_trace(env, shape, form, B2, prob_of(shape))


def check_best_iterate(env, shape, form=0):
    L.check_best_iterate(env, shape, form, B2, prob_of(shape))


def check_no_stall_counter(env, shape, form=0):
    L.check_no_stall_counter(env, shape, form, 20, B2, prob_of(shape))


def check_wide_iterates(env, shape=WIDE_SHAPE):
    L.check_wide_iterates(env, shape, B2)


def check_one_qp_stops_beside_a_running_one(shape=(70, 250, 0)):
    """the oracle's two QPs stop at different passes at eps = 1e-8 (14 and 13): the early return of one QP (bcStop) beside a
    running one is what check_counts_and_trace exercises at this shape"""
    its = [int(L.oracle(shape, B2, i, 1e-8, 20, True, "f64", prob_of(shape))[4]["iters"][0]) for i in range(B2)]
    assert its[0] != its[1], its
    return its


# ---------------------------------------------------------------- 2. kkt_checks
def kkt_args(shape, kinds):
    return dict(B=B2, prob=prob_of(shape), kinds=kinds, cond_rule=True)


def warm_dense(env, shape, kinds):
    def make():
        for kind in kinds:
            K.case(env, shape, kind, B2, "f64", prob_of(shape), True).reference_side()
    if not all(("case", env.dev.type, tuple(shape), B2, kind, "f64", prob_of(shape), True) in K._cache for kind in kinds):
        timed("kkt/" + tag(shape), make)


def check_solve(env, shape, form=0, kinds=K.DKINDS):
    warm_dense(env, shape, kinds)
    K.check_solve(env, shape, form, **kkt_args(shape, kinds))


def check_backward(env, shape, form=0, kinds=K.DKINDS):
    warm_dense(env, shape, kinds)
    K.check_backward(env, shape, form, **kkt_args(shape, kinds))


def check_jvp(env, shape, form=0, kinds=K.DKINDS):
    warm_dense(env, shape, kinds)
    K.check_jvp(env, shape, form, **kkt_args(shape, kinds))


def check_declined_roles(env, shape, form=0, kind="mid"):
    """K right-hand sides and the second-order pass: this family declines both, the *_supported queries are asserted to say so
    (kkt_checks.check_multi, check_backward2) and nothing runs"""
    assert K.check_multi(env, shape, form, B=B2, prob=prob_of(shape), kinds=(kind,), cond_rule=True) is False
    assert K.check_backward2(env, shape, form, B=B2, prob=prob_of(shape), kind=kind) is False


def check_f32(env, shape=F32_SHAPE):
    """QPX_F32, the family's float32 kernels: solve, backward, forward mode on kkt_checks' float32 gate"""
    K.check_f32_grid(env, shape, B=B2)


# ---------------------------------------------------------------- 3. prefac_checks
def check_blob(env, shape, knob=0):
    prob = prob_of(shape)
    if ("ref", tuple(shape), B2, "f64", prob, True) not in P._cache:
        timed("blob/" + tag(shape), lambda: P.reference(shape, B2, "f64", prob, True))
    built = P.check_blob(env, shape, knob, prob=prob, B=B2)
    assert built.family == P.FAMILY_BIG
    return built


# ---------------------------------------------------------------- the host forms, bit for bit
def specified_words(lay):
    """the words of the large family's blob that the pre-factorisation specifies (prefac_checks' `compared` part), from the
    layout alone: prefac_reference.expected_big on arrays of the right shapes"""
    n, m, q = lay.n, lay.m, lay.q
    arrs = {"Lq": np.eye(n), "Zt": np.zeros((m, n)), "R": np.zeros((m, m)), "gt1": np.zeros(1)}
    if q:
        arrs.update(Yt=np.zeros((q, n)), L11=np.eye(q), Vh=np.zeros((m, q)))
    spec = np.zeros(lay.total, bool)
    for idx, _ in P.R.expected_big(arrs, lay).values():
        spec[idx] = True
    return spec


def bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return x.view({4: np.int32, 8: np.int64}[x.dtype.itemsize]).copy()


def host_launch(env, shape, knob, B):
    """One batch under one knob, every entry point once: the blob behind the pre-factorisation, the loop at eps = 1e-8 with its
    trace, the finishing stage on its result (both entry points split the batch), the KKT solve and the backward (which do
    not: big_split's `allow`).  Returns the loop's result object and every output as its bit pattern."""
    def make():
        c = K.case(env, shape, "mid", B)
        out = {}
        with env.run(knob):
            fac = K.build(env, c.arrs, B, "f64")
            out["blob"] = bits(fac.blob.reshape(B, fac.elems))
            out["prefac/status"] = bits(fac.status)
            p, h, b = [c.t(c.arrs[i]) for i in (1, 3, 5)]
            res = fac.ipm(p, h, b, eps=1e-8, maxIter=20, stall_policy=1, want_trace=True)
            for k in ("zhat", "lam", "slacks", "iters", "best_resid", "trace") + (("nu",) if shape[2] else ()):
                out["ipm/" + k] = bits(getattr(res, k))
            keep = types.SimpleNamespace(iters=res.iters.clone(), trace=res.trace.clone())
            if fac.polish_ok:
                fac.polish(p, h, b, res, steps=2)
                for k in ("zhat", "lam", "slacks") + (("nu",) if shape[2] else ()):
                    out["polish/" + k] = bits(getattr(res, k))
            for name, vals in K.run_solve(fac, c)["all"].items():
                if vals is not None:
                    out["solve/" + name] = bits(vals)
            for name, vals in K.run_backward(fac, c)["duals"].items():
                if vals is not None:
                    out["backward/" + name] = bits(vals)
        return keep, out
    return K.cached(("host_launch", env.dev.type, tuple(shape), knob, B), make)


def check_default_launch(env, shape, base, B):
    """the one-part default launch of a host-form batch against the references, at referenced_qps(B): the blob (check_blob's
    comparison and gates) and the loop's counts and trace (check_counts_and_trace's)"""
    assert base >> 16 == 0 and B < 96          # (one part: big_auto_parts)
    qps = referenced_qps(B)
    keep, out = host_launch(env, shape, base, B)
    assert (out["prefac/status"] == 0).all(), out["prefac/status"]
    warm_oracle(shape, B, qps)
    worst, rel = L.compare_trace(keep, shape, B, 20, qps=qps)
    L.note("trace/%s/B%d" % (tag(shape, base), B), worst)
    L.note("trace_rel/%s/B%d" % (tag(shape, base), B), rel)
    assert worst <= L.TOL and rel <= L.TRACE_REL, (worst, rel)
    lay = P.R.LayoutBig(*shape)
    assert out["blob"].shape == (B, lay.total)
    ref = timed("blob/%s/B%d" % (tag(shape), B), lambda: P.reference(shape, B, "f64", "prof", True, qps))
    g = P.PGate()
    P.compare(g, "blob/%s/B%d" % (tag(shape, base), B), types.SimpleNamespace(blob=out["blob"].view(np.float64)), ref,
              P.FAMILY_BIG, lay, qps=qps)
    g.done()


def check_host_form(env, shape, base, variant, B):
    """the batch under base | variant against the one-part default launch of the same batch: every specified word of every
    QP's blob, the loop's result and trace, the finishing stage's result, the KKT solve and the backward, BIT FOR BIT.  The
    variants change where and when launches are enqueued (parts on side streams with their own pointer offsets, the helper
    stream, the order of a fused launch's tiles), never an addition.  On the emulator, which runs streams one after the
    other, this only guards the offsets (adv, advio) and the part boundaries; on the MI355X also the forks, joins and events."""
    parts = (variant >> 16) & 15
    if parts:
        assert part_lengths(B, parts) == {(2, 5): [2, 3], (3, 5): [1, 2, 2], (4, 5): [1, 1, 1, 2], (2, 33): [16, 17],
                                          (3, 48): [16, 16, 16]}[(parts, B)]
    _, ref = host_launch(env, shape, base, B)
    _, got = host_launch(env, shape, base | variant, B)
    assert ref.keys() == got.keys()
    spec = K.cached(("spec", tuple(shape)), lambda: specified_words(P.R.LayoutBig(*shape)))
    bad = []
    for k in ref:
        a, b = (ref[k][:, spec], got[k][:, spec]) if k == "blob" else (ref[k], got[k])
        if not np.array_equal(a, b):
            diff = np.flatnonzero((a != b).reshape(B, -1).any(1)) if a.shape[0] == B else np.flatnonzero((a != b).reshape(a.shape[0], B, -1).any((0, 2)))
            bad.append((k, "QPs", diff[:8].tolist()))
    name = "%s/B%d/%#x" % (tag(shape, base), B, variant)
    bitwise[name] = not bad
    print("%-40s %s" % (name, "bit for bit" if not bad else bad))
    assert not bad, (name, bad)
