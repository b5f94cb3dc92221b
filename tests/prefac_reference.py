"""A dense reference of the pre-factorisation's factor blob (qpx_pre_factor / qpx_pre_factor_soft), with nothing taken from the
library, and the ONLY place in the tests that restates the blob's layouts (qpth_amd/csrc/qpx_layout.h for the thread-grid /
matrix-core family, qpth_amd/csrc/qpx_big.h: BigLayout for the large-QP family).  tests/prefac_checks.py compares blobs with
it word by word; tests/test_prefac_reference.py holds it against a 50-digit mpmath inverse and each index map against a
hand-written two-block example.

Per QP, from float64 Q (symmetric: the forms read different triangles of Q, so an unsymmetric one is out of scope), G, A:

    H = [[Q, A'], [A, 0]],  X0 = np.linalg.inv(H),  X <- X + X (I - H X) in np.longdouble, ROUNDS = 4 rounds,
    H^-1 = [[K, N], [N', -S11^-1]]   =>   Kneg = -K, MT = (G K)', NTn = -N', W = G N, S11i = S11^-1, R = G K G',
    gt1 = || G' 1 ||_2, every product in np.longdouble; `resid` = max |I - H X| of the last iterate.
    Soft rows w: R + diag(w), sqrt(|| G' 1 ||^2 + #{w_i > 0})  (include/qpx.h, qpx_pre_factor_soft).

The large-QP family keeps triangular factors: they come from a np.longdouble Cholesky and substitutions written here
(big_reference), by the identities above BigLayout and in big_pre_factor (qpx_big_host.inc); the R they give is asserted to be
the G K G' of the refined inverse.

lapack_side() forms the same arrays the plain float64 way (np.linalg.inv, np.linalg.cholesky, float64 products): what the
conditioning of a case costs a correct float64 code, the figure the gates of prefac_checks rest on.
"""
import numpy as np

LD = np.longdouble
ROUNDS = 4
NAMES_A = ("Kneg", "MT", "NTn", "W", "S11i", "gt1", "R")


# ---------------------------------------------------------------- the arrays
def kkt_matrix(Q, A):
    n, q = Q.shape[0], A.shape[0]
    H = np.zeros((n + q, n + q), Q.dtype)
    H[:n, :n] = Q
    H[:n, n:] = A.T
    H[n:, :n] = A
    return H


def refined_inverse(H, rounds=ROUNDS):
    """(X, max |I - H X|): the float64 LAPACK inverse of H after `rounds` Newton corrections in np.longdouble"""
    Hl = np.asarray(H, LD)
    X = np.linalg.inv(np.asarray(H, np.float64)).astype(LD)
    I = np.eye(H.shape[0], dtype=LD)
    for _ in range(rounds):
        X = X + X @ (I - Hl @ X)
    return X, float(np.abs(I - Hl @ X).max())


def arrays_from_inverse(X, G, n, q):
    """the arrays of family (a) from H^-1 = [[K, N], [N', -S11^-1]] and G, in X's and G's type"""
    K, N = X[:n, :n], X[:n, n:]
    GK = G @ K
    c = G.sum(0)
    return {"Kneg": -K, "MT": GK.T, "NTn": -N.T, "W": G @ N, "S11i": -X[n:, n:], "R": GK @ G.T,
            "gt1": np.sqrt((c * c).sum()).reshape(1)}


def reference(Q, G, A, w=None):
    """one QP: {name: np.longdouble array} of NAMES_A, "resid" (max |I - H X|), and "K" itself.  w: soft rows"""
    Q, G, A = np.asarray(Q, np.float64), np.asarray(G, np.float64), np.asarray(A, np.float64).reshape(-1, Q.shape[0])
    n, q = Q.shape[0], A.shape[0]
    X, resid = refined_inverse(kkt_matrix(Q, A))
    out = arrays_from_inverse(X, G.astype(LD), n, q)
    out["K"], out["resid"] = X[:n, :n], resid
    if w is not None:
        soften(out, w)
    return out


def soften(arrs, w):
    """R + diag(w) and sqrt(|| G' 1 ||^2 + #{w_i > 0}), in place, in the arrays' own type"""
    w = np.asarray(w, np.float64)
    t = arrs["R"].dtype
    arrs["R"] = arrs["R"] + np.diag(w.astype(t))
    arrs["gt1"] = np.sqrt(arrs["gt1"] * arrs["gt1"] + t.type(int((w > 0).sum())))
    return arrs


def lapack_side(Q, G, A, dtype=np.float64):
    """the same arrays by np.linalg.inv and products in `dtype` (float64; float32: what QPX_F32's gates rest on)"""
    Q, G, A = [np.asarray(x, dtype) for x in (Q, G, np.asarray(A).reshape(-1, np.shape(Q)[0]))]
    n, q = Q.shape[0], A.shape[0]
    if dtype == np.float32:
        import torch
        X = torch.linalg.inv(torch.from_numpy(kkt_matrix(Q, A))).numpy()
    else:
        X = np.linalg.inv(kkt_matrix(Q, A))
    return arrays_from_inverse(X, G, n, q)


# ---------------------------------------------------------------- family (a): qpx_layout.h, fac_layout
def tri(i):
    return i * (i + 1) // 2


def align4(x):
    return (x + 3) & ~3


def _first(need, sizes):
    for s in sizes:
        if need <= s:
            return s
    return 0


def grid_nb(order):
    return _first((order + 15) // 16, (1, 2, 4, 7, 10, 13))


def wave_nb(m):
    return _first((m + 7) // 8, (2, 4, 8, 13))


def tile_nb(m):
    return _first((m + 15) // 16, (1, 2, 4, 7))


def sweep_nb(order):
    return 8 if (order + 15) // 16 == 8 else grid_nb(order)


class LayoutA:
    """offsets (in elements) of one QP's blob of family (a) for the image mask `images` (1 Rg, 2 Rw, 4 Rm)"""

    def __init__(self, n, m, q, images):
        self.n, self.m, self.q, self.images = n, m, q, images
        self.nbg, self.nbw, self.nbt = grid_nb(m), wave_nb(m), tile_nb(m)
        self.off, self.size = {}, {}
        o = 0
        for name, size in (("Kneg", n * n), ("MT", n * m), ("NTn", q * n), ("W", m * q), ("S11i", q * q)):
            self.off[name], self.size[name] = o, size
            o += align4(size)
        self.scal = o
        self.off["gt1"], self.size["gt1"] = o, 1
        o += 4
        self.prof = o
        o += 8
        for name, bit, size in (("Rg", 1, tri(self.nbg) * 256), ("Rw", 2, tri(self.nbw) * 64), ("Rm", 4, tri(self.nbt) * 256)):
            if images & bit and size:
                self.off[name], self.size[name] = o, size
                o += size
        self.total = o

    def image_names(self):
        return [k for k in ("Rg", "Rw", "Rm") if k in self.off]


def rg_index(i, j):
    """R[i][j] in the 16x16 thread grid's image; block row >= block column (diagonal blocks are held in full)"""
    li, a, lj, b = i // 16, i % 16, j // 16, j % 16
    return (tri(li) + lj) * 256 + a + 16 * b


def rw_index(i, j):
    """... in the 8x8 thread grid's image"""
    li, a, lj, b = i // 8, i % 8, j // 8, j % 8
    return (tri(li) + lj) * 64 + a + 8 * b


def rm_index(i, j):
    """... in the matrix-core tile image: tile (I, J), then the accumulator layout of the f64 16x16x4 instruction"""
    I, J, r, c = i // 16, j // 16, i % 16, j % 16
    return ((tri(I) + J) * 4 + r // 4) * 64 + (r % 4) * 16 + c


IMAGE_INDEX = {"Rg": (rg_index, 16), "Rw": (rw_index, 8), "Rm": (rm_index, 16)}


def r_image(R, name, size):
    """(image, pad): R of order m zero-padded into the image `name` of `size` words; pad: True where no entry of R lands"""
    index, bs = IMAGE_INDEX[name]
    m = R.shape[0]
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    keep = (i // bs) >= (j // bs)
    idx = index(i[keep], j[keep])
    img = np.zeros(size, R.dtype)
    pad = np.ones(size, bool)
    assert idx.max() < size and len(np.unique(idx)) == len(idx)
    img[idx] = R[keep]
    pad[idx] = False
    return img, pad


def image_diagonal(name, m):
    """where R[i][i] lies in the image, i < m"""
    i = np.arange(m)
    return IMAGE_INDEX[name][0](i, i)


def expected_a(arrs, lay):
    """One QP's blob of family (a) as the reference has it:  (values, kind, regions)
    values: float64[total]; kind: int8[total] -- 0 a compared word, 1 declared unspecified (scal[1..3], the profiling words,
    the words that align4 leaves between two arrays), 2 a pad of an R image (exact zero), -1 nothing (there must be none);
    regions: name -> (offset, size) of every compared array, the images whole"""
    vals = np.zeros(lay.total, np.float64)
    kind = np.full(lay.total, -1, np.int8)
    claimed = np.zeros(lay.total, np.int32)
    regions = {}
    for name in ("Kneg", "MT", "NTn", "W", "S11i", "gt1"):
        o, size = lay.off[name], lay.size[name]
        a = np.asarray(arrs[name], np.float64).reshape(-1)
        assert a.size == size, (name, a.size, size)
        vals[o:o + size] = a
        kind[o:o + size] = 0
        claimed[o:o + size] += 1
        if size:
            regions[name] = (o, size)
        if name != "gt1":
            kind[o + size:o + align4(size)] = 1
            claimed[o + size:o + align4(size)] += 1
    kind[lay.scal + 1:lay.scal + 4] = 1
    claimed[lay.scal + 1:lay.scal + 4] += 1
    kind[lay.prof:lay.prof + 8] = 1
    claimed[lay.prof:lay.prof + 8] += 1
    R = np.asarray(arrs["R"], np.float64)
    for name in lay.image_names():
        o, size = lay.off[name], lay.size[name]
        img, pad = r_image(R, name, size)
        vals[o:o + size] = img
        kind[o:o + size] = np.where(pad, 2, 0)
        claimed[o:o + size] += 1
        regions[name] = (o, size)
    assert (claimed == 1).all() and (kind >= 0).all(), "the three parts do not tile the blob"
    return vals, kind, regions


# ---------------------------------------------------------------- the large-QP family: qpx_big.h, BigLayout
KBB = 64
BIG_VECS = 26            # bvCount
BV_ONE, BV_PQ, BV_Y = 20, 25, 19
BS_GT1 = 15
BC_FAIL = 5
BIG_POL_VECS = 32


def big_pad(x):
    return (x + KBB - 1) // KBB * KBB


def big_blk(ld, rb, cb):
    return (rb * (ld // KBB) + cb) * KBB * KBB


def big_at(ld, i, j):
    """entry (i, j) of a matrix stored block by block, `ld` elements per row"""
    return big_blk(ld, i // KBB, j // KBB) + (i % KBB) * KBB + (j % KBB)


class LayoutBig:
    REGIONS = ("Lq", "Wq", "Zt", "Yt", "R", "T", "Wt", "S11", "Wy", "Vh", "Us", "vec", "scal", "ctrl", "pol")

    def __init__(self, n, m, q):
        self.n, self.m, self.q = n, m, q
        NP, MP, QP = big_pad(n), big_pad(m), (big_pad(q) if q else 0)
        self.NP, self.MP, self.QP, self.VP = NP, MP, QP, max(NP, MP)
        sizes = (NP * NP, NP // KBB * 2 * KBB * KBB, MP * NP, QP * NP, MP * MP, MP * MP, MP // KBB * 2 * KBB * KBB, QP * QP,
                 QP // KBB * 2 * KBB * KBB, MP * QP, MP * QP, BIG_VECS * self.VP, 16, 16, BIG_POL_VECS * self.VP)
        self.off, self.size = {}, {}
        o = 0
        for name, size in zip(self.REGIONS, sizes):
            self.off[name], self.size[name] = o, size
            o += size
        self.total = o


def cholesky_ld(A):
    """lower Cholesky factor in np.longdouble, column by column"""
    A = np.asarray(A, LD)
    n = A.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        assert d > 0, "not positive definite"
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower_ld(L, B):
    """L^-1 B by forward substitution, np.longdouble"""
    B = np.array(B, LD)
    X = np.zeros_like(B)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def padded(M, rows, cols, unit_diagonal=False):
    out = np.zeros((rows, cols), M.dtype)
    out[:M.shape[0], :M.shape[1]] = M
    if unit_diagonal:
        for i in range(M.shape[0], rows):
            out[i, i] = 1
    return out


def big_factors(Q, G, A, chol, lower_solve):
    """the large family's matrices, unpadded, with the Cholesky and the substitution handed in (np.longdouble here, float64 in
    lapack_side_big):  Lq = chol(Q), Yt = A Lq^-T, L11 = chol(Yt Yt'), Vh = (G Lq^-T) Yt' L11^-T, Ztp = G Lq^-T - Vh L11^-1 Yt,
    R = Ztp Ztp'"""
    q = A.shape[0]
    Lq = chol(Q)
    Zt = lower_solve(Lq, G.T).T
    out = {"Lq": Lq}
    if q:
        Yt = lower_solve(Lq, A.T).T
        L11 = chol(Yt @ Yt.T)
        Vh = lower_solve(L11, Yt @ Zt.T).T
        Zt = Zt - Vh @ lower_solve(L11, Yt)
        out.update(Yt=Yt, L11=L11, Vh=Vh)
    out["Zt"] = Zt
    out["R"] = Zt @ Zt.T
    c = G.sum(0)
    out["gt1"] = np.sqrt((c * c).sum()).reshape(1)
    return out


def big_reference(Q, G, A, w=None, tol=1e-12):
    """one QP: the matrices of big_factors in np.longdouble; R is asserted to be the G K G' of the refined inverse within `tol`
    (the figure is kept as "r_gap")"""
    Q, G, A = np.asarray(Q, np.float64), np.asarray(G, np.float64), np.asarray(A, np.float64).reshape(-1, np.shape(Q)[0])
    out = big_factors(Q.astype(LD), G.astype(LD), A.astype(LD), cholesky_ld, solve_lower_ld)
    ref = reference(Q, G, A)
    out["resid"] = ref["resid"]
    gap = float(np.abs(out["R"] - ref["R"]).max() / max(1.0, float(np.abs(ref["R"]).max())))
    out["r_gap"] = gap
    assert gap <= tol, ("the two routes to R disagree", gap, tol)
    if w is not None:
        soften(out, w)
    return out


def lapack_side_big(Q, G, A):
    Q, G, A = np.asarray(Q, np.float64), np.asarray(G, np.float64), np.asarray(A, np.float64).reshape(-1, np.shape(Q)[0])
    return big_factors(Q, G, A, np.linalg.cholesky, lambda L, B: np.linalg.solve(L, B))


def _block_inverses(L, P):
    """W_kk = L_kk^-1 of the 64 x 64 diagonal blocks of L padded to order P (identity on the padded diagonal): (P / 64, 64, 64)"""
    Lp = padded(L, P, P, unit_diagonal=True)
    I = np.eye(KBB, dtype=L.dtype)
    solve = solve_lower_ld if L.dtype == LD else (lambda a, b: np.linalg.solve(a, b))
    return np.stack([solve(Lp[k:k + KBB, k:k + KBB], I) for k in range(0, P, KBB)])


def _blocks(ld_rows, ld_cols, which):
    """(i, j) of every entry in the chosen 64 x 64 blocks of a (ld_rows x ld_cols) matrix: "lower" strictly below the block
    diagonal, "upper" strictly above, "lower+diag", "all" """
    i, j = np.meshgrid(np.arange(ld_rows), np.arange(ld_cols), indexing="ij")
    rb, cb = i // KBB, j // KBB
    keep = {"lower": rb > cb, "upper": rb < cb, "lower+diag": rb >= cb, "all": rb >= 0}[which]
    return i[keep], j[keep]


def expected_big(arrs, lay):
    """One QP's blob of the large family as the reference has it: name -> (word indices, float64 values) of every compared
    piece, pads included (zeros; the identity where a factor's diagonal is padded)"""
    n, m, q = lay.n, lay.m, lay.q
    NP, MP, QP = lay.NP, lay.MP, lay.QP
    out = {}

    def put(name, region, M, ld, which):
        i, j = _blocks(M.shape[0], M.shape[1], which)
        if len(i):
            out[name] = (lay.off[region] + big_at(ld, i, j), np.asarray(M[i, j], np.float64))

    def put_w(name, region, L, P, transposed_too):
        W = _block_inverses(L, P)
        idx, val = [], []
        e = np.arange(KBB * KBB)
        for k in range(P // KBB):
            base = lay.off[region] + k * 2 * KBB * KBB
            idx.append(base + e)
            val.append(W[k].reshape(-1))
            if transposed_too:
                idx.append(base + KBB * KBB + e)
                val.append(W[k].T.reshape(-1))
        out[name] = (np.concatenate(idx), np.asarray(np.concatenate(val), np.float64))

    put("Lq", "Lq", padded(arrs["Lq"], NP, NP, True), NP, "lower")
    put_w("Wq", "Wq", arrs["Lq"], NP, False)            # big_potrf of Lq runs with kDiagNoWt: W_kk alone
    put("Zt", "Zt", padded(arrs["Zt"], MP, NP), NP, "all")
    put("R", "R", padded(arrs["R"], MP, MP), MP, "lower+diag")
    if q:
        put("Yt", "Yt", padded(arrs["Yt"], QP, NP), NP, "all")
        L11 = padded(arrs["L11"], QP, QP, True)
        put("L11", "S11", L11, QP, "lower")
        put("L11T", "S11", L11.T.copy(), QP, "upper")     # (mirror = 1: L^T above the block diagonal)
        put_w("Wy", "Wy", arrs["L11"], QP, True)
        put("Vh", "Vh", padded(arrs["Vh"], MP, QP), QP, "all")
    out["gt1"] = (np.array([lay.off["scal"] + BS_GT1]), np.asarray(arrs["gt1"], np.float64).reshape(1))
    return out


def big_r_diagonal(lay):
    i = np.arange(lay.m)
    return lay.off["R"] + big_at(lay.MP, i, i)
