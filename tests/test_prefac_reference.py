"""tests/prefac_reference.py by itself (CPU, no emulator): the refined inverse and the arrays made from it against a 50-digit
mpmath inverse, the large family's Cholesky route against the same, and every index map against a hand-written two-block
example.

Measured (max |a - ref| / max(1, max |ref|) over the arrays of family (a), then of the large family; gate REF_TOL = 1e-12, 1e3
below the 1e-9 floor of the float64 checks of tests/prefac_checks.py):
    (12, 9, 3)   prof_qp         6.2e-17   7.9e-17     the float64 LAPACK route alone: 1.8e-14
    (20, 40, 4)  prof_qp         1.0e-16   1.0e-16                                     1.8e-14
    (20, 40, 4)  cond(Q) = 1e8   2.2e-14   1.7e-14                                     4.7e-11
(the first two rows sit at the rounding of the 50-digit values to float64, in which they are compared)
"""
import mpmath
import numpy as np
import pytest

import prefac_reference as R
import problems

REF_TOL = 1e-12
SEED = 11


def ladder_q(n, c, seed=SEED):
    r = np.random.RandomState([seed, n, c])
    U, _ = np.linalg.qr(r.randn(n, n))
    Q = (U * np.logspace(0, -c, n)) @ U.T
    return 0.5 * (Q + Q.T)


def qp(n, m, q, c=None):
    Q, _, G, _, A, _ = problems.prof_qp(1, n, m, q, seed=SEED)
    A = A[0] if q else np.zeros((0, n))
    return (Q[0] if c is None else ladder_q(n, c)), G[0], A


def fig(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(1.0, np.abs(ref).max())) if ref.size else 0.0


def mp_arrays(Q, G, A):
    mp = mpmath.mp
    n, q = Q.shape[0], A.shape[0]
    X = mp.matrix(R.kkt_matrix(Q, A).tolist()) ** -1
    Gm = mp.matrix(G.tolist())
    K, N = X[:n, :n], X[:n, n:]
    GK = Gm * K
    cols = [mp.fsum(Gm[i, j] for i in range(G.shape[0])) for j in range(n)]
    num = lambda M, r, c: np.array([[float(M[i, j]) for j in range(c)] for i in range(r)], np.float64).reshape(r, c)     # noqa: E731
    m = G.shape[0]
    return {"Kneg": -num(K, n, n), "MT": num(GK, m, n).T, "NTn": -num(N, n, q).T, "W": num(Gm * N, m, q) if q else np.zeros((m, 0)),
            "S11i": -num(X[n:, n:], q, q), "R": num(GK * Gm.T, m, m), "gt1": np.array([float(mp.sqrt(mp.fsum(c * c for c in cols)))])}


@pytest.mark.parametrize("n,m,q,c", [(12, 9, 3, None), (20, 40, 4, None), (20, 40, 4, 8)])
def test_reference_against_a_50_digit_inverse(n, m, q, c):
    Q, G, A = qp(n, m, q, c)
    with mpmath.workdps(50):
        want = mp_arrays(Q, G, A)
    ref = R.reference(Q, G, A)
    # max |I - H X| as np.longdouble evaluates it: its own rounding, 2^-64 |H| |X|, is what is left (|X| ~ 1e8 on the ladder)
    assert ref["resid"] <= (1e-15 if c is None else 1e-11)
    worst = max(fig(ref[k], want[k]) for k in R.NAMES_A)
    lap = R.lapack_side(Q, G, A)
    side = max(fig(lap[k], want[k]) for k in R.NAMES_A)
    # the large family's route: R = Ztp Ztp' from the np.longdouble Cholesky and substitutions
    big = R.big_reference(Q, G, A, tol=REF_TOL)
    worst_big = max(fig(big["R"], want["R"]), fig(big["gt1"], want["gt1"]))
    assert fig(big["Lq"] @ big["Lq"].T, Q) <= 1e-17
    if q:
        # K = Lq^-T (I - Yt' S11^-1 Yt) Lq^-1: M = G K = Ztp Lq^-1 and W = G N = Vh L11^-1 (the comment above BigLayout)
        MT = R.solve_lower_ld(big["Lq"].T[::-1, ::-1], big["Zt"].T[::-1])[::-1]
        worst_big = max(worst_big, fig(MT, want["MT"]))
        Wm = R.solve_lower_ld(big["L11"].T[::-1, ::-1], big["Vh"].T[::-1])[::-1].T
        worst_big = max(worst_big, fig(Wm, want["W"]))
    print("(%d, %d, %d) c=%s: reference %.1e, large-family route %.1e, float64 LAPACK route %.1e" % (n, m, q, c, worst, worst_big, side))
    assert worst <= REF_TOL and worst_big <= REF_TOL


def test_soft_rows():
    Q, G, A = qp(12, 9, 3)
    w = np.array([0, 1e-8, 1e8, 0.5, 0, 3.0, 0, 0, 2.0])
    hard, soft = R.reference(Q, G, A), R.reference(Q, G, A, w=w)
    assert np.array_equal(np.asarray(soft["R"] - hard["R"], np.float64), np.diag(np.asarray(np.diag(soft["R"]) - np.diag(hard["R"]), np.float64)))
    assert fig(np.diag(soft["R"]), np.asarray(np.diag(hard["R"]), np.float64) + w) <= 1e-16
    assert abs(float(soft["gt1"][0]) ** 2 - float(hard["gt1"][0]) ** 2 - 5) <= 1e-12


# ---------------------------------------------------------------- the index maps, each against numbers worked out by hand
def test_layout_of_family_a_by_hand():
    # n = 5, m = 20, q = 2, the tile image only: Kneg 25 -> 28, MT 100, NTn 10 -> 12, W 40, S11i 4, scal 4, prof 8, Rm two tile rows
    lay = R.LayoutA(5, 20, 2, 4)
    assert (lay.off["Kneg"], lay.off["MT"], lay.off["NTn"], lay.off["W"], lay.off["S11i"]) == (0, 28, 128, 140, 180)
    assert (lay.scal, lay.prof, lay.off["Rm"], lay.total) == (184, 188, 196, 196 + 3 * 256)
    # images 3 (Rg + Rw): m = 20 is two blocks of 16 and three of 8 -> the four-block 8x8 grid
    lay = R.LayoutA(5, 20, 2, 3)
    assert (lay.nbg, lay.nbw, lay.off["Rg"], lay.off["Rw"], lay.total) == (2, 4, 196, 196 + 768, 196 + 768 + 640)
    assert "Rm" not in lay.off
    # m = 130: no 8x8 grid (17 blocks of 8 > 13), ten blocks of 16
    lay = R.LayoutA(12, 130, 0, 3)
    assert (lay.nbg, lay.nbw, lay.nbt) == (10, 0, 0) and lay.image_names() == ["Rg"]
    assert [R.sweep_nb(o) for o in (16, 17, 64, 65, 113, 128, 129, 160, 161, 208, 209)] == [1, 2, 4, 7, 8, 8, 10, 10, 13, 13, 0]


def test_rg_index_by_hand():
    # two blocks of 16: R[17][3] is block (1, 0), a = 1, b = 3 -> 1 * 256 + 1 + 48; R[17][18]: block (1, 1) = third block
    assert R.rg_index(17, 3) == 256 + 49
    assert R.rg_index(17, 18) == 512 + 1 + 32
    assert R.rg_index(3, 2) == 3 + 32 and R.rg_index(2, 3) == 2 + 48        # a diagonal block holds both triangles
    img, pad = R.r_image(np.arange(400.0).reshape(20, 20), "Rg", 768)
    assert img[256 + 49] == 17 * 20 + 3 and img[2 + 48] == 2 * 20 + 3
    assert pad[256 + 4 + 16 * 0] and not pad[256 + 3]                        # R[20][0] does not exist, R[19][0] does
    assert pad.sum() == 768 - (256 + 4 * 16 + 16)                             # 16 x 16, 4 x 16 and 4 x 4 entries land


def test_rw_index_by_hand():
    # blocks of 8: R[9][3] is block (1, 0), a = 1, b = 3 -> 64 + 1 + 24; R[10][12]: block (1, 1) -> 128 + 2 + 32
    assert R.rw_index(9, 3) == 64 + 25
    assert R.rw_index(10, 12) == 128 + 34
    img, pad = R.r_image(np.arange(100.0).reshape(10, 10), "Rw", 3 * 64)
    assert img[64 + 25] == 93 and pad.sum() == 192 - (64 + 16 + 4)


def test_rm_index_by_hand():
    # tile (1, 0), row 17 -> r = 1: group 0, (r % 4) * 16 + c = 16 + 3;  row 22 -> r = 6: group 1 -> 64, (6 % 4) * 16 = 32
    assert R.rm_index(17, 3) == 256 + 19
    assert R.rm_index(22, 5) == 256 + 64 + 32 + 5
    assert R.rm_index(2, 3) == 2 * 16 + 3 and R.rm_index(3, 2) == 3 * 16 + 2
    img, pad = R.r_image(np.arange(576.0).reshape(24, 24), "Rm", 768)
    assert img[256 + 64 + 32 + 5] == 22 * 24 + 5 and not pad[256 + 19]
    assert pad[256 + 128:512].all() and not pad[256:256 + 128].any()         # rows 24 .. 31 of tile (1, 0) do not exist


def test_big_layout_by_hand():
    # n = 70, m = 10, q = 3: NP = 128, MP = 64, QP = 64, VP = 128
    lay = R.LayoutBig(70, 10, 3)
    assert (lay.NP, lay.MP, lay.QP, lay.VP) == (128, 64, 64, 128)
    o = lay.off
    assert (o["Lq"], o["Wq"], o["Zt"], o["Yt"], o["R"]) == (0, 16384, 16384 + 16384, 32768 + 8192, 40960 + 8192)
    assert (o["T"], o["Wt"], o["S11"], o["Wy"], o["Vh"], o["Us"]) == (53248, 57344, 65536, 69632, 77824, 81920)
    assert (o["vec"], o["scal"], o["ctrl"], o["pol"], lay.total) == (86016, 89344, 89360, 89376, 89376 + 4096)
    # two blocks per row (ld = 128): entry (65, 3) is block (1, 0) = the third block of 4096, row 1, column 3
    assert R.big_at(128, 65, 3) == 2 * 4096 + 64 + 3
    assert R.big_at(128, 3, 65) == 4096 + 3 * 64 + 1
    assert R.big_at(128, 70, 127) == 3 * 4096 + 6 * 64 + 63


def test_big_diagonal_block_inverses_by_hand():
    # L = [[2, 0], [1, 4]] padded to one block: W = [[1/2, 0], [-1/8, 1/4]] and the identity beyond; its transpose behind it
    L = np.array([[2.0, 0], [1, 4]], R.LD)
    arrs = {"Lq": L, "Zt": np.zeros((1, 2), R.LD), "R": np.zeros((1, 1), R.LD), "gt1": np.zeros(1, R.LD),
            "Yt": np.zeros((1, 2), R.LD), "L11": L[:1, :1], "Vh": np.zeros((1, 1), R.LD)}
    lay = R.LayoutBig(2, 1, 1)
    exp = R.expected_big(arrs, lay)
    idx, val = exp["Wq"]
    got = dict(zip(idx.tolist(), val.tolist()))
    base = lay.off["Wq"]
    assert (got[base], got[base + 1], got[base + 64], got[base + 65], got[base + 2 * 64 + 2]) == (0.5, 0.0, -0.125, 0.25, 1.0)
    assert len(idx) == 4096                                      # W_kk alone: no transposed copy beside Lq's blocks
    idx, val = exp["Wy"]
    got = dict(zip(idx.tolist(), val.tolist()))
    base = lay.off["Wy"]
    assert len(idx) == 8192 and got[base] == 0.5 and got[base + 4096] == 0.5 and got[base + 4096 + 65] == 1.0
    assert "Lq" not in exp                                       # one block: nothing strictly below the block diagonal
