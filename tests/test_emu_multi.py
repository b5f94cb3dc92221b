"""The KKT solve for K right-hand sides per QP in one launch (qpx_factor_solve_kkt_multi -> KKTFactors.solve_kkt_many) and the
Jacobians built on it (qpth_amd/sensitivity.py), on the host-thread emulator: the kernel bodies of every thread-grid / tile
form factor T once and walk the right-hand sides in blocks of RB.  Every (QP, k) against KKTFactors.solve_kkt on that
right-hand side and against a float64 dense solve of the full KKT matrix (tests/multi_reference.py), both to 1e-8 relative per
output -- the bound a single solve is held to -- with d taken from a real solution, so that it spans many decades.
ds = (-rs - dz) / d against ds = -rz - G dx of the dense solution: 1e-8 where rs is None (measured 3e-14); with a random rs
the bound is 1e-6 (multi_reference.ds_tol: where d ~ 1e-8, -rs - dz cancels -- DESIGN 4.5 --, in solve_kkt's ds exactly as
here; measured 4.7e-8), and ds is also held to the block row that defines it, D ds + dz = -rs, to rounding.  Measured maxima on the emulator (each test prints its own): against solve_kkt 3.7e-13, (dx, dz, dy)
against the dense solve 3.9e-11."""
import ctypes

import numpy as np
import pytest
import torch

import problems
from emu.harness import emu_lib, emulated
from multi_reference import KNOB_FORMS as FORMS, dense_solve_many, ds_tol, kkt_matrix, rel_many
from qpth_amd import _lib, sensitivity
from qpth_amd.kkt import MULTI_RHS_BLOCK as RB, KKTFactors
from qpth_amd.qp import QPFunction

SHAPES = [(10, 5, 0), (20, 10, 4), (40, 30, 6), (64, 64, 0), (100, 100, 0), (100, 50, 10)]
KS = [1, RB - 1, RB, RB + 1, 2 * RB + 3]
OUT = ("dx", "ds", "dz", "dy")
# each knob form of tests/test_emu_jvp.py at a size it serves (3 is the large-QP family: test_large_family_* below):
# 16x16 grid; 8x8 grid in the loop (the KKT kernels: 16x16); tiles with one wave, two waves (four and seven tile rows), four
FORM_SHAPES = [(256, (20, 10, 4)), (512, (40, 30, 6)), (1024 + 2048, (64, 64, 0)), (1024 + 4096, (100, 50, 10)),
               (1024 + 4096, (100, 100, 0)), (1024 + 8192, (100, 50, 10))]
assert {v for v, _ in FORM_SHAPES} | {3} == set(FORMS)


def _t(x, dtype=torch.float64):
    x = np.asarray(x)
    return torch.tensor(x, dtype=dtype) if x.size else torch.empty(0, dtype=dtype)


_SOLVED = {}


def backward_d(r):
    return torch.clamp(r.lam, min=1e-8) / torch.clamp(r.slacks, min=1e-8)


def solved(n, m, q, variant=0, B=2, dtype=torch.float64, wide=False):
    """factors + the d of a real solution of problems.prof_qp -- the backward's, clamp(lam, 1e-8) / clamp(slacks, 1e-8)
    (qp.py:148), as full_kkt_tangent of tests/test_emu_jvp.py takes it --, computed once per (shape, form)"""
    key = (n, m, q, variant, B, dtype, wide)
    if key not in _SOLVED:
        Q, p, G, h, A, b = [_t(x, dtype) for x in problems.prof_qp(B, n, m, q, seed=3)]
        with emulated(variant=variant):
            fac = KKTFactors.build(Q, G, A if q else None, wide=wide)
            r = fac.ipm(p, h, b)
        d = backward_d(r)
        assert float(d.max() / d.min()) > 1e6          # many decades
        _SOLVED[key] = (fac, Q, G, (A if q else None), d)
    return _SOLVED[key]


def random_rhs(B, K, n, m, q, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, K, k, generator=g, dtype=torch.float64).to(dtype) if k else None for k in (n, m, m, q)]


def check_many(fac, Q, G, A, d, rhs, variant=0, tol=1e-8, single=True, refine=0, tol_single=None):
    """solve_kkt_many on `rhs` against solve_kkt per right-hand side (tol_single, default tol) and against the dense float64
    solve (tol); -> the outputs"""
    tol_single = tol if tol_single is None else tol_single
    with emulated(variant=variant):
        out = fac.solve_kkt_many(d, *rhs, refine=refine)
        worst_single = 0.0
        if single:
            K = out[0].shape[1]
            for k in range(K):
                ref = fac.solve_kkt(d, *[None if X is None else X[:, k] for X in rhs], refine=refine)
                for o, r_ in zip(out, ref):
                    if o is not None:
                        worst_single = max(worst_single, float(rel_many(o[:, k:k + 1], r_.unsqueeze(1)).max()))
    ref = dense_solve_many(Q, G, A, d, *rhs)
    worst_dense = max(float(rel_many(o, r_).max()) for o, r_ in zip(out[::2] + out[3:], ref[::2] + ref[3:]) if o is not None)
    dx, ds, dz, dy = [None if o is None else o.double() for o in out]
    rs = torch.zeros_like(dz) if rhs[1] is None else rhs[1].double()
    row2 = float(((d.double().unsqueeze(1) * ds + dz + rs).norm(dim=2) / (dz.norm(dim=2) + rs.norm(dim=2))).max())
    ds_dense = float(rel_many(ds, ref[1]).max())
    print("solve_kkt_many: max rel err vs solve_kkt %.2e, (dx, dz, dy) vs dense float64 %.2e; D ds + dz + rs %.2e, ds vs -rz - G dx %.2e"
          % (worst_single, worst_dense, row2, ds_dense))
    assert worst_single <= tol_single, worst_single
    assert worst_dense <= tol, worst_dense
    assert ds_dense <= ds_tol(tol, rhs[1]), ds_dense
    # one rounding of the difference and one of the quotient in float64 (2^-52 each, measured 2e-16); float32 outputs: ds and
    # dz each narrowed once more (2^-24 each), so 4 * 2^-24 bounds it
    assert row2 <= (1e-14 if out[0].dtype == torch.float64 else 4 * 2.0 ** -24), row2
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_every_block_count_against_single_solves_and_the_dense_solve(shape):
    """K = 1, RB - 1, RB, RB + 1, 2 RB + 3: one block, a partial one, full ones, full + partial"""
    n, m, q = shape
    fac, Q, G, A, d = solved(n, m, q)
    for K in KS:
        out = check_many(fac, Q, G, A, d, random_rhs(2, K, n, m, q, seed=K))
        assert out[0].shape == (2, K, n) and out[1].shape == out[2].shape == (2, K, m)
        assert (out[3] is None) if q == 0 else (out[3].shape == (2, K, q))
    assert int(fac.status.max()) & _lib.ST_KKT_BREAKDOWN == 0


@pytest.mark.parametrize("variant,shape", FORM_SHAPES)
def test_every_kernel_form(variant, shape):
    n, m, q = shape
    fac, Q, G, A, d = solved(n, m, q, variant)
    for K in (1, RB + 1, 2 * RB + 3):
        check_many(fac, Q, G, A, d, random_rhs(2, K, n, m, q, seed=10 + K), variant=variant)


@pytest.mark.parametrize("missing", range(4))
def test_each_right_hand_side_null_in_turn(missing):
    n, m, q = 20, 10, 4
    fac, Q, G, A, d = solved(n, m, q)
    rhs = random_rhs(2, RB + 1, n, m, q, seed=20)
    rhs[missing] = None
    check_many(fac, Q, G, A, d, rhs)


def test_float32_data_in_float64_arithmetic():
    """QPX_F32_WIDE: float32 right-hand sides widened on load, outputs narrowed on store: 1e-6, the bound for narrowed outputs"""
    n, m, q = 40, 30, 6
    fac, Q, G, A, d = solved(n, m, q, dtype=torch.float32, wide=True)
    out = check_many(fac, Q, G, A, d, random_rhs(2, RB + 1, n, m, q, seed=21, dtype=torch.float32), tol=1e-6)
    assert out[0].dtype == torch.float32


def test_float32_kernels():
    """QPX_F32, the float32 thread-grid kernels: a well-conditioned system (d = 1, Q from random_dense_qp) against the float64
    dense solve to 1e-3, the bound tests/test_emu_jvp.py holds the float32 kernels to against float64"""
    B, n, m, q = 2, 20, 12, 2
    Q, _, G, _, A, _ = [_t(x, torch.float32) for x in problems.random_dense_qp(B, n, m, q, seed=20, dtype=np.float32)]
    with emulated():
        fac = KKTFactors.build(Q, G, A)
    d = torch.ones(B, m, dtype=torch.float32)
    # (against solve_kkt: the same float32 arithmetic per right-hand side, sums in another order -- 1e-5, a hundred roundings)
    out = check_many(fac, Q, G, A, d, random_rhs(B, 2 * RB + 3, n, m, q, seed=22, dtype=torch.float32), tol=1e-3, tol_single=1e-5)
    assert out[0].dtype == torch.float32 and not fac.wide


def test_shared_factors():
    """un-batched Q, G, A: one blob for the batch (sfac = 0), a d and right-hand sides per QP"""
    B, n, m, q = 3, 20, 10, 4
    Q, p, G, h, A, b = [_t(x) for x in problems.prof_qp(B, n, m, q, seed=5)]
    with emulated():
        fac = KKTFactors.build(Q[0], G[0], A[0], nBatch=B)
        assert fac.shared and fac.sfac == 0
        r = fac.ipm(p, h, b)
    d = backward_d(r)
    ex = lambda X: X[:1].expand(B, *X.shape[1:])  # noqa: E731
    check_many(fac, ex(Q), ex(G), ex(A), d, random_rhs(B, RB + 1, n, m, q, seed=23))


def test_refine_falls_back_to_single_solves():
    n, m, q = 20, 10, 4
    fac, Q, G, A, d = solved(n, m, q)
    calls = []
    real = fac.lib.factor_solve_kkt_multi
    fac.lib.factor_solve_kkt_multi = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        check_many(fac, Q, G, A, d, random_rhs(2, 3, n, m, q, seed=24), refine=1)
        assert not calls
        check_many(fac, Q, G, A, d, random_rhs(2, 3, n, m, q, seed=24), single=False)
        assert calls == [1]
    finally:
        del fac.lib.factor_solve_kkt_multi


def test_large_family_unsupported_and_fallback():
    """nz + nineq > 208: qpx_multi_supported says 0, the entry returns QPX_ERR_UNSUPPORTED, solve_kkt_many runs K single solves"""
    B, n, m, q, K = 2, 100, 110, 0, 3
    lib = emu_lib()
    assert lib.dll.qpx_multi_supported(_lib.QPX_F64, n, m, q) == 0
    assert lib.dll.qpx_multi_supported(_lib.QPX_F64, 100, 100, 0) == 1
    fac, Q, G, A, d = solved(n, m, q)
    rhs = random_rhs(B, K, n, m, q, seed=25)
    out = check_many(fac, Q, G, A, d, rhs)
    ptr = lambda X: ctypes.c_void_p(X.data_ptr())  # noqa: E731
    code = lib.dll.qpx_factor_solve_kkt_multi(_lib.QPX_F64, B, n, m, q, K, ptr(fac.blob), fac.sfac, ptr(d), ptr(rhs[0]), None, None,
                                              None, ptr(out[0]), None, None, None, ptr(fac.status), None)
    assert code == -2                       # QPX_ERR_UNSUPPORTED
    with emulated(variant=3):               # ... and under the knob that sends every size to that family
        assert lib.dll.qpx_multi_supported(_lib.QPX_F64, 20, 10, 4) == 0


def test_block_size_and_knob_forms_are_the_sources_own():
    """MULTI_RHS_BLOCK is kKktMultiRB of the kernels (the K sets above probe ITS block boundaries), KNOB_FORMS the list of
    tests/test_emu_jvp.py"""
    import os
    import re
    import test_emu_jvp
    src = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "qpx_forms.h")).read()
    assert int(re.search(r"constexpr int kKktMultiRB = (\d+);", src).group(1)) == RB
    assert list(FORMS) == list(test_emu_jvp.FORMS)


def test_argument_errors():
    lib = emu_lib()
    B, n, m, K = 1, 4, 3, 2
    fac = np.zeros(lib.factor_elems(_lib.QPX_F64, n, m, 0))
    d, rx, dx = np.ones(m), np.zeros(K * n), np.zeros(K * n)
    st = np.zeros(B, np.int32)

    def p(a):
        return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None

    def call(K=K, d=d, rx=rx, dx=dx, dtype=_lib.QPX_F64, q=0, ry=None):
        return lib.dll.qpx_factor_solve_kkt_multi(dtype, B, n, m, q, K, p(fac), 0, p(d), p(rx), None, None, p(ry), p(dx), None, None,
                                                  None, p(st), None)

    assert call() == 0
    assert call(K=0) == -1                  # QPX_ERR_ARG
    assert call(dx=None) == -1
    assert call(d=None) == -1
    assert call(rx=None) == -1              # all four right-hand sides NULL
    assert call(rx=None, ry=rx) == -1       # ... ry does not count without equality constraints
    assert call(dtype=7) == -1


def test_argument_checks_of_the_host_mirror():
    n, m, q = 20, 10, 4
    fac, Q, G, A, d = solved(n, m, q)
    rx = torch.zeros(2, 3, n, dtype=torch.float64)
    with emulated():
        with pytest.raises(RuntimeError, match="at least one"):
            fac.solve_kkt_many(d, None, None, None, None)
        with pytest.raises(RuntimeError, match="rz has shape"):
            fac.solve_kkt_many(d, rx, None, torch.zeros(2, 4, m, dtype=torch.float64), None)
        with pytest.raises(RuntimeError, match="rx is torch.float32"):
            fac.solve_kkt_many(d, rx.float(), None, None, None)
        with pytest.raises(RuntimeError, match=r"\(B, K, \.\)"):
            fac.solve_kkt_many(d, rx[:, 0], None, None, None)


# ---------------------------------------------------------------- Jacobians
def _backward_rows(arrs, which, count, duals=False):
    """row i of d out / d (p, h, b), out = zhat | lam | nu, as QPFunction's backward gives it: (out[:, i].sum()).backward()"""
    tq = [_t(x) for x in arrs]
    for x in tq:
        if x.nelement():
            x.requires_grad_(True)
    outs = QPFunction(verbose=-1, duals=duals)(*tq)
    out = {"z": outs[0], "nu": outs[1], "lam": outs[2]}[which] if duals else outs
    rows = []
    for i in range(count):
        g = torch.autograd.grad(out[:, i].sum(), [tq[1], tq[3], tq[5]], retain_graph=True, allow_unused=True)
        rows.append([x.detach() if x is not None else None for x in g])
    return rows


def _rows_agree(J, o, rows, tol=1e-8):
    worst = 0.0
    for i, (gp, gh, gb) in enumerate(rows):
        for w, g in (("p", gp), ("h", gh), ("b", gb)):
            if g is None or g.nelement() == 0:
                continue
            got = J[o, w][..., i, :]
            worst = max(worst, float(((got - g).norm(dim=-1) / g.norm(dim=-1).clamp_min(1e-300)).max()))
    print("jacobian rows of %s vs QPFunction's backward: max rel err %.2e" % (o, worst))
    assert worst <= tol, worst


def test_jacobian_against_the_dense_inverse_and_the_backward():
    B, n, m, q = 2, 12, 9, 3
    arrs = problems.prof_qp(B, n, m, q, seed=7)
    Q, p, G, h, A, b = [_t(x) for x in arrs]
    with emulated():
        sol = sensitivity.solve(Q, p, G, h, A, b)
        J = sol.jacobian(of=("z", "lam", "nu"))
        Jz = sol.jacobian()
        rows = {o: _backward_rows(arrs, o, k, duals=(o != "z")) for o, k in (("z", n), ("lam", m), ("nu", q))}
    assert J["z", "p"].shape == (B, n, n) and J["z", "h"].shape == (B, n, m) and J["z", "b"].shape == (B, n, q)
    assert J["lam", "h"].shape == (B, m, m) and J["nu", "b"].shape == (B, q, q)
    assert set(Jz) == {("z", "p"), ("z", "h"), ("z", "b")}
    # J[z, p][i, :] = dx of K (dx, dz, dy) = -(e_i, 0, 0): minus row i of the x-block of the inverse (transposed: column i)
    d = torch.clamp(sol.lam, min=1e-8) / torch.clamp(sol.slacks, min=1e-8)
    Kinv = torch.linalg.inv(kkt_matrix(Q, G, A, d))
    ref = -Kinv[:, :n, :n].transpose(1, 2)
    scale = ref.norm(dim=(1, 2), keepdim=True)
    for Jzp in (J["z", "p"], Jz["z", "p"]):
        err = float(((Jzp - ref).norm(dim=(1, 2), keepdim=True) / scale).max())
        sym = float(((Jzp - Jzp.transpose(1, 2)).norm(dim=(1, 2), keepdim=True) / scale).max())
        print("J[z,p] vs the dense inverse %.2e, asymmetry %.2e" % (err, sym))
        assert err <= 1e-8 and sym <= 1e-8
    # dh = -dz: J[z, h][i, j] = +(K^-1)[n + j, i];  db = -dy likewise
    assert float(((J["z", "h"] - Kinv[:, n:n + m, :n].transpose(1, 2)).norm(dim=(1, 2)) / Kinv[:, n:n + m, :n].norm(dim=(1, 2))).max()) <= 1e-8
    assert float(((J["z", "b"] - Kinv[:, n + m:, :n].transpose(1, 2)).norm(dim=(1, 2)) / Kinv[:, n + m:, :n].norm(dim=(1, 2))).max()) <= 1e-8
    for o in ("z", "lam", "nu"):
        _rows_agree(J, o, rows[o])


def test_unbatched_parameters_through_solve():
    """Q, G, h, A un-batched, p and b batched: the forward broadcasts them as QPFunction does, the factors are shared, and the
    Jacobian with respect to the shared h is the batch mean -- row by row what QPFunction's backward returns"""
    B, n, m, q = 3, 12, 9, 3
    arrs = list(problems.prof_qp(B, n, m, q, seed=8))
    for i in (0, 2, 3, 4):
        arrs[i] = arrs[i][0]
    arrs[5] = np.broadcast_to(arrs[4] @ np.ones(n), (B, q)).copy() + 0.01 * np.arange(B)[:, None]     # b for the shared A
    Q, p, G, h, A, b = [_t(x) for x in arrs]
    with emulated():
        sol = sensitivity.solve(Q, p, G, h, A, b)
        assert sol.fac.shared and sol.shared["h"] and not sol.shared["p"]
        zref = QPFunction(verbose=-1)(Q, p, G, h, A, b)
        assert torch.equal(sol.zhat, zref)
        J = sol.jacobian()
        rows = _backward_rows(arrs, "z", n)
    assert J["z", "p"].shape == (B, n, n) and J["z", "h"].shape == (n, m) and J["z", "b"].shape == (B, n, q)
    _rows_agree(J, "z", rows)


def test_vjp_many_matrix_gradients_and_checks():
    """ "Q", "G", "A" from (dx, dz, dy) by the formulas of qpx_backward_duals: against QPFunction's backward on the same cotangents"""
    B, n, m, q, K = 2, 12, 9, 3, RB + 1
    arrs = problems.prof_qp(B, n, m, q, seed=9)
    g = torch.Generator().manual_seed(26)
    V = torch.randn(B, K, n, generator=g, dtype=torch.float64)
    with emulated():
        sol = sensitivity.solve(*[_t(x) for x in arrs])
        got = sol.vjp_many(dl_dz=V, want=("Q", "p", "G", "h", "A", "b"))
        for k in (0, K - 1):
            tq = [_t(x).requires_grad_(True) for x in arrs]
            QPFunction(verbose=-1)(*tq).backward(V[:, k])
            for name, x in zip(("Q", "p", "G", "h", "A", "b"), tq):
                ref = x.grad
                err = float((got[name][:, k] - ref).flatten(1).norm(dim=1).div(ref.flatten(1).norm(dim=1)).max())
                assert err <= 1e-8, (name, k, err)
        with pytest.raises(RuntimeError, match="at least one"):
            sol.vjp_many()
        with pytest.raises(ValueError, match="unknown parameter"):
            sol.vjp_many(dl_dz=V, want=("z",))
        with pytest.raises(ValueError, match="only the vector parameters"):
            sol.jacobian(wrt=("Q",))
    assert got["Q"].shape == (B, K, n, n) and got["G"].shape == (B, K, m, n) and got["A"].shape == (B, K, q, n)
    assert not any(t.requires_grad for t in got.values())
