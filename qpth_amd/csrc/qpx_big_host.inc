// qpx_big_host.inc -- the large-QP family's host side (kernels: qpx_big.h, qpx_big_polish.h): the per-thread knobs, the
// split of a batch into parts on side streams, and the launch sequences of its pre-factorisation, loop, KKT solve /
// backward / forward mode and finishing stage.  Included by qpx_api.inc, inside namespace qpx, after the decision
// functions (use_big and the knobs of qpx_set_ipm_variant) and before the api_* dispatchers that call big_split / big_*.

// Large-QP family: the batch is worked on in `parts` parts on as many streams (the caller's + side streams forked
// from it), because one pass of that family alternates between phases that are latency-bound on one workgroup
// per QP (diagonal blocks, substitutions) and phases that fill the chip (trailing updates, mat-vecs): parts that
// are out of phase with each other overlap the two.  variant bits 16..19: parts (0 = auto), bits 20..27: initial
// stagger of the side streams in units of 16 us.
static thread_local int g_big_parts = 0, g_big_delay = 0;
static thread_local int g_big_no_swizzle = 0;  // variant bit 29: plain (qp, tile) grid for the GEMM launches
static thread_local int g_big_grid_diag = 0;   // variant bit 28: diagonal blocks on the thread grid instead of the matrix cores (f64)
static thread_local int g_big_no_overlap = 0;  // variant bit 26: R z' in the caller's stream in front of the factorisation (the round-3 order) instead of beside it
static thread_local int g_big_diag_one_wave = 0;   // variant bit 27: diagonal blocks on the matrix cores by ONE wave (the round-3 form) instead of the chain-wave form
// 0 = thread grid, 1 = matrix cores by one wave, 2 = by four waves in the chain-wave form
inline int big_diag_form() { return g_big_grid_diag ? 0 : (g_big_diag_one_wave ? 1 : 2); }
template <class P> inline P* adv(P* p, size_t off) { return p ? p + off : p; }
// the same for an array of the C boundary, which is float32 behind a double* when io32 is set (QPX_F32_WIDE)
template <class P> inline P* advio(P* p, size_t off, int io32)
{
    if (!p) return p;
    return (sizeof(P) == 8 && io32) ? (P*)((const float*)p + off) : p + off;
}
// Parts of a batch by default (knob bits 16..19 = 0).  Measured on MI355X, same box, f64 step / loop in ms, the parts
// WITHOUT helper streams against one part with its helper (profiles/r05d_ab_parts_by_shape.txt):
//   B=128 n=m=500 (C4): 1 part 12.35 / 9.92   2 parts 12.16 / 9.52   3 parts 12.13 / 9.37   4 parts 21.2 / 16.7
//   B=512 n=m=150:      1 part  5.18 / 4.31   2 parts  4.91 / 3.92   3 parts  4.98 / 3.93   4 parts  7.8 /  6.0
//   B=256 n=m=200: equal;  B=64 n=m=300: 4.76 / 5.00 / 5.24;  B=32 n=m=500: 7.80 / 8.18 / 8.50;  B=16 n=m=300 q=20: equal
// (round 2's kernels had measured no difference at C4: the faster the bandwidth-bound launches became, the larger the share
// of a pass that is latency chains one part cannot fill).  Four parts = four streams of the library beside the caller's
// other streams run into the device's four hardware queues and serialise: never picked; three leave no queue for a
// collective that runs beside the backward at N > 1 -- so two, from 96 QPs up, in the entry points whose launch sequence is
// long enough for it (pre-factorisation, loop, finishing stage; NOT qpx_factor_solve_kkt / qpx_backward: r06q).
inline int big_auto_parts(int B) { return B >= 96 ? 2 : 1; }
template <class F> int big_split(int B, void* stream, bool allow, F&& run)       // run(first QP, count, stream, part index, parts)
{
    int parts = g_big_parts ? g_big_parts : big_auto_parts(B);
    if (parts > kMaxSide + 1) parts = kMaxSide + 1;
    if (!allow || parts > B) parts = 1;
    if (parts == 1) return run(0, B, stream, 0, 1);
    void* side[kMaxSide];
    int e = stream_fork(stream, parts - 1, side, g_big_delay * 16);
    if (e) return e;
    // part boundaries on multiples of 8 where the batch allows it: the GEMM launches order their tiles XCD by XCD when the
    // part's batch is a multiple of the 8 XCDs (launch_big_gemm)
    auto bound = [&](int i) {
        if (i >= parts) return B;
        const int x = (int)((long long)B * i / parts);
        return B >= 16 * parts ? (x + 4) / 8 * 8 : x;
    };
    for (int i = 0; i < parts && !e; ++i) {
        const int q0 = bound(i), q1 = bound(i + 1);
        e = run(q0, q1 - q0, i == 0 ? stream : side[i - 1], i, parts);
    }
    const int j = stream_join(stream, parts - 1, side);      // always: the caller's stream must own all the work
    return e ? e : j;
}

template <class T> struct BigCtx {
    int B, n, m;
    T* fac; size_t fs;
    BigLayout L;
    void* stream;
    int q = 0;
    int* ctrl() const { return reinterpret_cast<int*>(fac + L.ctrl); }
    size_t sctrl() const { return fs * sizeof(T) / sizeof(int); }
};

// blocked Cholesky of the nb x nb-block matrix at blob offset `mat` (ld = 64 nb); src / dg: T = R + diag at the first step
template <class T>
int big_potrf(const BigCtx<T>& c, size_t mat, int nb, bool from_r, size_t wout, int fail_bit, int check_stop,
              const BigPhaseArgs<T>* pre = nullptr, int pre_phase = -1, int mirror = 0)
{
    // mirror: also store L^T above the diagonal.  Only the factor of S11 = A Q^-1 A^T asks for it (the pre-factorisation
    // forms Vh L11^-1 from the transposed tiles); the substitutions read the lower triangle in both directions since
    // round 5 (big_trsv_body), so the per-pass factor of T = R + diag(d) no longer writes the 115 MB of mirrored panels.
    const int ld = nb * kBB;
    // one launch each: the diagonal block of panel k (-> W_kk), the panel under it (X W_kk^T, mirrored above the
    // diagonal), a rank-(64 nk) update of the tiles [r0, nb) x [c0, c1) from the panels kb0 .. kb0 + nk - 1
    auto diag = [&](int k, bool first) {
        BigPanelArgs<T> p{};
        p.B = c.B; p.k = k;
        p.M = c.fac + (first ? c.L.R : mat); p.sM = c.fs; p.ld = ld;
        if (first) { p.dg = c.fac + c.L.v(bvD); p.sdg = c.fs; }
        p.W = c.fac + wout; p.sW = c.fs;
        p.ctrl = c.ctrl(); p.sctrl = c.sctrl(); p.fail_bit = fail_bit; p.check_stop = check_stop; p.tile = big_diag_form() | (mirror ? 0 : kDiagNoWt);
        if (k == 0 && pre) {                       // the wave-0 phase that produces diag(d) rides in the same launch
            BigDiagArgs<T> d{};
            d.p = p; d.ph = *pre; d.pre_phase = pre_phase;
            return launch_big_diag<T>(d, c.stream);
        }
        return launch_big_panel<T>(p, c.stream);
    };
    auto apply = [&](int k, bool first) {
        BigGemmArgs<T> g{}; g.no_swizzle = g_big_no_swizzle;
        g.B = c.B; g.nti = nb - k - 1; g.ntj = 1; g.crb0 = k + 1; g.ccb0 = k; g.arb0 = k + 1; g.brb0 = 0;
        g.akb0 = k; g.bkb0 = 0; g.nk = 1; g.lower = 0; g.mirror = mirror; g.zero_init = 1;
        g.C = c.fac + mat; g.sC = c.fs; g.ldc = ld;
        g.A = c.fac + (first ? c.L.R : mat); g.sA = c.fs; g.lda = ld;
        g.Bm = c.fac + wout + (size_t)k * 2 * kBB * kBB; g.sB = c.fs; g.ldb = kBB;
        g.alpha = T(1);
        g.ctrl = c.ctrl(); g.sctrl = c.sctrl(); g.check_stop = check_stop;
        return launch_big_gemm<T>(g, c.stream);
    };
    auto update = [&](int r0, int c0, int ncb, int kb0, int nk, bool first) {
        BigGemmArgs<T> g{}; g.no_swizzle = g_big_no_swizzle;
        g.B = c.B; g.nti = nb - r0; g.ntj = ncb; g.crb0 = g.arb0 = r0; g.ccb0 = g.brb0 = c0; g.akb0 = g.bkb0 = kb0; g.nk = nk;
        g.lower = 1; g.mirror = 0; g.zero_init = 0;
        // tile (0, 0) of every update is the diagonal block of the next panel: its workgroup eliminates it right away
        g.fuse = 1; g.fuse_k = r0; g.fail_bit = fail_bit; g.tile = big_diag_form() | (mirror ? 0 : kDiagNoWt); g.W = c.fac + wout; g.sW = c.fs;
        g.C = c.fac + mat; g.sC = c.fs; g.ldc = ld;
        if (first) { g.Cs = c.fac + c.L.R; g.sCs = c.fs; g.ldcs = ld; g.dg = c.fac + c.L.v(bvD); g.sdg = c.fs; }
        g.A = c.fac + mat; g.sA = c.fs; g.lda = ld;
        g.Bm = c.fac + mat; g.sB = c.fs; g.ldb = ld;
        g.alpha = T(-1);
        g.ctrl = c.ctrl(); g.sctrl = c.sctrl(); g.check_stop = check_stop;
        return launch_big_gemm<T>(g, c.stream);
    };
    // (Round 4 tried finishing the panel under a diagonal block INSIDE the update launch that eliminates the block -- its
    // tiles waiting on a flag for W_kk from their launch-mate: parity-green on the GPU, nine launches per factorisation
    // instead of fifteen, and 5 % SLOWER at C4, 13 % at n = m = 150: a waiting workgroup holds one of the two slots of
    // its CU while the other tiles of the launch queue behind it.  Deleted; profiles/archive/r04d, r04e.)
    // Panels are taken in PAIRS: after panel k only the next block column is brought up to date (it is all panel k+1
    // needs); the rest of the trailing matrix then gets both panels in one pass of rank 128 -- every trailing tile is
    // read and written once per pair instead of once per panel (the updates are HBM-bound: 2 MB per QP and pass).
    // The diagonal block of a panel is eliminated by the workgroup that finishes its last update (fused into the
    // update launches); only the very first one needs a launch of its own.
    // (Round 4 also tried a LOOK-AHEAD across launches: the rank-128 update of a pair split into the next block column on
    // the caller's stream and the rest of the trailing matrix on a helper stream, so that the chain column -> diagonal block
    // -> panel of the next pair runs beside the bulk.  Parity-green, 3.8 % SLOWER at C4 (13.56 -> 14.07 ms), equal at
    // n = m = 150: two bandwidth-bound streams share one HBM, and fork / join add bubbles.  Deleted; profiles/archive/r04l.)
    int e;
    if ((e = diag(0, from_r))) return e;
    for (int k = 0; k + 1 < nb; k += 2) {
        const bool first = from_r && k == 0;
        if ((e = apply(k, first))) return e;
        if ((e = update(k + 1, k + 1, 1, k, 1, first))) return e;          // ... and eliminates block k+1
        if (k + 2 == nb) break;
        if ((e = apply(k + 1, false))) return e;
        if ((e = update(k + 2, k + 2, nb - k - 2, k, 2, first))) return e;  // ... and eliminates block k+2
    }
    return QPX_OK;
}

// x <- +-(L L^T)^-1 xin for the factor at `mat` (dirs: 0 forward only, 1 backward only, 2 both)
template <class T>
int big_solve(const BigCtx<T>& c, size_t mat, size_t w, int nb, int dirs, size_t xin, size_t x, int negate, int check_stop)
{
    for (int d = 0; d < 2; ++d) {
        if ((dirs == 0 && d == 1) || (dirs == 1 && d == 0)) continue;
        BigTrsvArgs<T> t{};
        t.B = c.B; t.nb = nb; t.dir = d; t.post = (negate && (d == 1 || dirs == 0)) ? 1 : 0;
        t.M = c.fac + mat; t.sM = c.fs; t.ld = nb * kBB;
        t.W = c.fac + w; t.sW = c.fs;
        t.xin = c.fac + ((dirs == 2 && d == 1) ? x : xin); t.sxin = c.fs;
        t.x = c.fac + x; t.sx = c.fs;
        t.ctrl = c.ctrl(); t.sctrl = c.sctrl(); t.check_stop = check_stop;
        const int e = launch_big_trsv<T>(t, c.stream);
        if (e) return e;
    }
    return QPX_OK;
}

// x <- -(L L^T)^-1 xin in ONE launch, followed (post_phase >= 0) by the wave-0 phase that consumes x
template <class T>
int big_solve_fused(const BigCtx<T>& c, size_t mat, size_t w, int nb, size_t xin, size_t x, const BigPhaseArgs<T>& ph,
                    int post_phase, int check_stop, int pre_phase = 0)
{
    BigSolveArgs<T> s{};
    s.pre_phase = pre_phase;
    s.t.B = c.B; s.t.nb = nb;
    s.t.M = c.fac + mat; s.t.sM = c.fs; s.t.ld = nb * kBB;
    s.t.W = c.fac + w; s.t.sW = c.fs;
    s.t.xin = c.fac + xin; s.t.sxin = c.fs;
    s.t.x = c.fac + x; s.t.sx = c.fs;
    s.t.ctrl = c.ctrl(); s.t.sctrl = c.sctrl(); s.t.check_stop = check_stop;
    s.ph = ph; s.negate = 1; s.post_phase = post_phase;
    return launch_big_solve<T>(s, c.stream);
}

// y = beta y0 + alpha M x (trans: M^T x) on blob vectors; M at blob offset mat, rows x cols logical extent
template <class T>
int big_mv(const BigCtx<T>& c, size_t mat, int ld, int rows, int cols, int trans, size_t x, size_t y0, bool has_y0, size_t y,
           T alpha, T beta, int check_stop)
{
    BigGemvArgs<T> g{};
    g.B = c.B; g.rows = rows; g.cols = cols; g.trans = trans;
    g.M = c.fac + mat; g.sM = c.fs; g.ld = ld;
    g.x = c.fac + x; g.sx = c.fs;
    g.y0 = has_y0 ? c.fac + y0 : nullptr; g.sy0 = c.fs;
    g.y = c.fac + y; g.sy = c.fs;
    g.alpha = alpha; g.beta = beta;
    g.ctrl = c.ctrl(); g.sctrl = c.sctrl(); g.check_stop = check_stop;
    return launch_big_gemv<T>(g, c.stream);
}

// y = R x from the lower block triangle of the symmetric R (big_symv_body): block rows -> the workspace, then the sum.  The
// workspace is the finishing stage's region of the blob, which is dead while the loop runs.
template <class T>
int big_symv(const BigCtx<T>& c, size_t x, size_t y, int check_stop)
{
    BigSymvArgs<T> g{};
    g.B = c.B; g.rows = c.m;
    g.M = c.fac + c.L.R; g.sM = c.fs; g.ld = c.L.MP;
    g.x = c.fac + x; g.sx = c.fs;
    g.y = c.fac + y; g.sy = c.fs;
    g.ws = c.fac + c.L.pol; g.sws = c.fs;
    g.ctrl = c.ctrl(); g.sctrl = c.sctrl(); g.check_stop = check_stop;
    g.stage = 0;
    int e = launch_big_symv<T>(g, c.stream);
    if (e) return e;
    g.stage = 1;
    return launch_big_symv<T>(g, c.stream);
}

// R = Zt Zt^T, lower block triangle (round 5: nothing reads the upper one any more): the largest GEMM of the family
template <class T> int big_gemm_r(int B, int n, int m, T* fac, void* stream, int q = 0)
{
    const BigLayout L = big_layout(n, m, q);
    BigGemmArgs<T> g{}; g.no_swizzle = g_big_no_swizzle;
    g.B = B; g.nti = g.ntj = L.MP / kBB; g.nk = L.NP / kBB; g.lower = 1; g.mirror = 0; g.zero_init = 1;
    g.C = fac + L.R; g.sC = L.total; g.ldc = L.MP;
    g.A = fac + L.Zt; g.sA = L.total; g.lda = L.NP;
    g.Bm = fac + L.Zt; g.sB = L.total; g.ldb = L.NP;
    g.alpha = T(1);
    return launch_big_gemm<T>(g, stream);
}

// one GEMM launch on blob matrices: C[rows crb0.., cols ccb0..] (nti x ntj tiles) = (zero | C | Cs) (+ dg on the diagonal)
// + alpha sum_{kb < nk} A[arb0 + ti][akb0 + kb] B[brb0 + tj][bkb0 + kb]^T   (transb: B given as [k][column])
template <class T> struct BigMat { size_t off; int ld; };
template <class T>
int big_mm(const BigCtx<T>& c, BigMat<T> C, int crb0, int ccb0, int nti, int ntj, BigMat<T> A, int arb0, int akb0,
           BigMat<T> Bm, int brb0, int bkb0, int nk, T alpha, bool zero_init, int lower = 0, int mirror = 0, int transb = 0,
           const BigMat<T>* Cs = nullptr, long long dgvec = -1)
{
    BigGemmArgs<T> g{}; g.no_swizzle = g_big_no_swizzle;
    g.B = c.B; g.nti = nti; g.ntj = ntj; g.crb0 = crb0; g.ccb0 = ccb0; g.arb0 = arb0; g.brb0 = brb0; g.akb0 = akb0; g.bkb0 = bkb0;
    g.nk = nk; g.lower = lower; g.mirror = mirror; g.zero_init = zero_init ? 1 : 0; g.transb = transb;
    g.C = c.fac + C.off; g.sC = c.fs; g.ldc = C.ld;
    if (Cs) { g.Cs = c.fac + Cs->off; g.sCs = c.fs; g.ldcs = Cs->ld; }
    if (dgvec >= 0) { g.dg = c.fac + (size_t)dgvec; g.sdg = c.fs; }
    g.A = c.fac + A.off; g.sA = c.fs; g.lda = A.ld;
    g.Bm = c.fac + Bm.off; g.sB = c.fs; g.ldb = Bm.ld;
    g.alpha = alpha;
    return launch_big_gemm<T>(g, c.stream);
}

// X <- X L^-T for the nb x nb-block factor at `mat` (diagonal-block inverses at `w`): X has nrb row blocks and lives at
// blob offset `x` with row length nb * 64 -- block column by block column: X_k <- X_k W_kk^T, then the later block
// columns get X_j -= X_k L_jk^T
template <class T>
int big_trsm_right_lt(const BigCtx<T>& c, size_t x, int nrb, size_t mat, size_t w, int nb)
{
    const int ld = nb * kBB;
    const BigMat<T> X{x, ld}, Lm{mat, ld};
    for (int k = 0; k < nb; ++k) {
        const BigMat<T> Wk{w + (size_t)k * 2 * kBB * kBB, kBB};
        int e = big_mm<T>(c, X, 0, k, nrb, 1, X, 0, k, Wk, 0, 0, 1, T(1), true);
        if (e) return e;
        if (k + 1 < nb && (e = big_mm<T>(c, X, 0, k + 1, nrb, nb - k - 1, X, 0, k, Lm, k + 1, k, 1, T(-1), false))) return e;
    }
    return QPX_OK;
}

template <class T>
int big_pre_factor(int B, int n, int m, int q, const T* Q, int64_t sQ, const T* G, int64_t sG, const T* A, int64_t sA, T* fac,
                   int32_t* status, void* stream, int io32, const T* w = nullptr, int64_t sw = 0)
{
    BigCtx<T> c{B, n, m, fac, big_layout(n, m, q).total, big_layout(n, m, q), stream, q};
    const BigLayout& L = c.L;
    const int nbq = L.NP / kBB, nbm = L.MP / kBB, nbe = L.QP / kBB;
    int e;
    BigVecArgs<T> v{};
    v.B = B; v.op = 2; v.n = n; v.m = m; v.q = q; v.fac = fac; v.fac_stride = c.fs;
    if ((e = launch_big_vec<T>(v, stream))) return e;
    BigPackArgs<T> pk{};
    pk.io32 = io32;
    pk.B = B; pk.rows = n; pk.cols = n; pk.P = L.NP; pk.ldp = L.NP; pk.sym = 1;
    pk.src = Q; pk.ssrc = sQ; pk.dst = fac + L.Lq; pk.sdst = c.fs;
    if ((e = launch_big_pack<T>(pk, L.NP / 16, stream))) return e;
    if ((e = big_potrf<T>(c, L.Lq, nbq, false, L.Wq, QPX_ST_Q_NOT_SPD, 0))) return e;
    pk.rows = m; pk.cols = n; pk.P = L.MP; pk.ldp = L.NP; pk.sym = 0;
    pk.src = G; pk.ssrc = sG; pk.dst = fac + L.Zt;
    if ((e = launch_big_pack<T>(pk, L.MP / 16, stream))) return e;
    if (q > 0) {
        pk.rows = q; pk.P = L.QP; pk.src = A; pk.ssrc = sA; pk.dst = fac + L.Yt;
        if ((e = launch_big_pack<T>(pk, L.QP / 16, stream))) return e;
    }
    // || G^T 1 ||  (before G is overwritten by Zt)
    if ((e = big_mv<T>(c, L.Zt, L.NP, m, n, 1, L.v(bvONE), 0, false, L.v(bvY), T(1), T(0), 0))) return e;
    v = BigVecArgs<T>{};
    v.B = B; v.op = 1; v.len = n; v.x = fac + L.v(bvY); v.sx = c.fs; v.y = fac + L.scal + bsGt1; v.sy = c.fs;
    v.m = m; v.w = w; v.sw = sw; v.w32 = io32;                 // soft rows: + their number under the root
    if ((e = launch_big_vec<T>(v, stream))) return e;
    // [Zt; Yt] = [G; A] Lq^-T: one pass over the stacked rows (Yt lies right behind Zt with the same row length)
    if ((e = big_trsm_right_lt<T>(c, L.Zt, nbm + nbe, L.Lq, L.Wq, nbq))) return e;
    if (q > 0) {
        // equality constraints (batch.py:403-424), see the comment at BigLayout:
        const BigMat<T> Zt{L.Zt, L.NP}, Yt{L.Yt, L.NP}, S11{L.S11, L.QP}, Vh{L.Vh, L.QP}, Us{L.Us, L.QP};
        // S11 = Yt Yt^T (+ 1 on the padded diagonal), lower block triangle, then its Cholesky factor
        if ((e = big_mm<T>(c, S11, 0, 0, nbe, nbe, Yt, 0, 0, Yt, 0, 0, nbq, T(1), true, 1, 1, 0, nullptr, (long long)L.v(bvPQ)))) return e;
        if ((e = big_potrf<T>(c, L.S11, nbe, false, L.Wy, QPX_ST_A_RANK, 0, nullptr, -1, 1))) return e;
        // Vh = (Zt Yt^T) L11^-T
        if ((e = big_mm<T>(c, Vh, 0, 0, nbm, nbe, Zt, 0, 0, Yt, 0, 0, nbq, T(1), true))) return e;
        if ((e = big_trsm_right_lt<T>(c, L.Vh, nbm, L.S11, L.Wy, nbe))) return e;
        // Us = Vh L11^-1, block column by block column from the last: Us_k = (Vh_k - sum_{j > k} Us_j L_jk) W_kk
        // (L_jk as the transposed tile (k, j) of the copy of L^T the factor keeps above its diagonal)
        for (int k = nbe - 1; k >= 0; --k) {
            const BigMat<T> Wkt{L.Wy + (size_t)k * 2 * kBB * kBB + (size_t)kBB * kBB, kBB};
            if (k + 1 < nbe) {
                if ((e = big_mm<T>(c, Us, 0, k, nbm, 1, Us, 0, k + 1, S11, k, k + 1, nbe - k - 1, T(-1), false, 0, 0, 0, &Vh))) return e;
                if ((e = big_mm<T>(c, Us, 0, k, nbm, 1, Us, 0, k, Wkt, 0, 0, 1, T(1), true))) return e;
            } else {
                if ((e = big_mm<T>(c, Us, 0, k, nbm, 1, Vh, 0, k, Wkt, 0, 0, 1, T(1), true))) return e;
            }
        }
        // Ztp = Zt - Us Yt   (in place; Yt as [k][column])
        if ((e = big_mm<T>(c, Zt, 0, 0, nbm, nbq, Us, 0, 0, Yt, 0, 0, nbe, T(-1), false, 0, 0, 1))) return e;
    }
    if ((e = big_gemm_r<T>(B, n, m, fac, stream, q))) return e;
    if (w) {                                                   // soft rows: R + diag(w)
        v = BigVecArgs<T>{};
        v.B = B; v.op = 3; v.n = n; v.m = m; v.q = q; v.fac = fac; v.fac_stride = c.fs; v.w = w; v.sw = sw; v.w32 = io32;
        if ((e = launch_big_vec<T>(v, stream))) return e;
    }
    // status words: the pre-factorisation's failure bits
    BigPhaseArgs<T> ph{};
    ph.B = B; ph.n = n; ph.m = m; ph.q = q; ph.phase = 6; ph.fac = fac; ph.fac_stride = c.fs; ph.status = status;
    return launch_big_phase<T>(ph, stream);
}

template <class T>
int big_ipm(const IpmArgs<T>& a, void* stream, int part = 0, int nparts = 1)
{
    BigCtx<T> c{a.B, a.n, a.m, a.fac, a.fac_stride, big_layout(a.n, a.m, a.q), stream, a.q};
    const BigLayout& L = c.L;
    const int nbq = L.NP / kBB, nbm = L.MP / kBB, nbe = L.QP / kBB, q = a.q;
    int e;
    BigPhaseArgs<T> ph{};
    ph.B = a.B; ph.n = a.n; ph.m = a.m; ph.maxIter = a.maxIter; ph.notImprovedLim = a.notImprovedLim; ph.stall_policy = a.stall_policy;
    ph.fac = a.fac; ph.fac_stride = a.fac_stride; ph.p = a.p; ph.h = a.h; ph.sp = a.sp; ph.sh = a.sh; ph.eps = a.eps;
    ph.lam = a.lam; ph.slack = a.slack; ph.best_resid = a.best_resid; ph.trace = a.trace; ph.iters = a.iters; ph.status = a.status;
    ph.q = q; ph.bq = a.b; ph.sb = a.sb; ph.io32 = a.io32;
    ph.phase = 0;
    if ((e = launch_big_phase<T>(ph, stream))) return e;
    // u = Lq^-1 p;  c = h + Ztp u - Vh L11^-1 b;  R 1
    if ((e = big_solve<T>(c, L.Lq, L.Wq, nbq, 0, L.v(bvP), L.v(bvU), 0, 0))) return e;
    if ((e = big_mv<T>(c, L.Zt, L.NP, a.m, a.n, 0, L.v(bvU), L.v(bvC), true, L.v(bvC), T(1), T(1), 0))) return e;
    if (q > 0) {
        if ((e = big_solve<T>(c, L.S11, L.Wy, nbe, 0, L.v(bvBQ), L.v(bvTB), 0, 0))) return e;                              // L11^-1 b
        if ((e = big_mv<T>(c, L.Vh, L.QP, a.m, q, 0, L.v(bvTB), L.v(bvC), true, L.v(bvC), T(-1), T(1), 0))) return e;
        // t = S11^-1 (b + Yt u):  x0 = Lq^-T (-u + Yt^T t),  nu = -(t + L11^-T Vh^T z');  u <- u - Yt^T t for the recovery of zhat
        if ((e = big_mv<T>(c, L.Yt, L.NP, q, a.n, 0, L.v(bvU), L.v(bvBQ), true, L.v(bvT1), T(1), T(1), 0))) return e;
        if ((e = big_solve<T>(c, L.S11, L.Wy, nbe, 2, L.v(bvT1), L.v(bvT1), 0, 0))) return e;
        if ((e = big_mv<T>(c, L.Yt, L.NP, q, a.n, 1, L.v(bvT1), L.v(bvU), true, L.v(bvU), T(-1), T(1), 0))) return e;
    }
    if ((e = big_symv<T>(c, L.v(bvONE), L.v(bvR1), 0))) return e;
    // start point: T = R + I, z_i = -T^-1 c
    if ((e = big_potrf<T>(c, L.T, nbm, true, L.Wt, QPX_ST_KKT_BREAKDOWN, 1))) return e;
    if ((e = big_solve_fused<T>(c, L.T, L.Wt, nbm, L.v(bvC), L.v(bvX), ph, 1, 1))) return e;          // + start point
    // one pass = 18 launches: R z' | residuals, stop decision, d (wave 0) + first diagonal block | 14 panel / update
    // launches | affine solve + its wave-0 phase | corrector solve + update of the iterate
    // (round 4) R z' runs on a side stream BESIDE the factorisation, which needs d = s/z only (phase 7); the residuals,
    // the best-iterate bookkeeping and the stop decision (phase 2) then ride in front of the affine solve.  A QP that
    // stops in pass k has been factored once more than before -- its work matrix is dead by then.
    // R z' beside the factorisation on a helper stream: only when the batch is ONE part.  With parts, their phases already
    // overlap each other, and a helper stream per part measured far slower (C4, same box: 3 parts 11.9 ms without helpers,
    // 18.3 ms with -- six streams share the device's four hardware queues --, 2 parts 12.1 vs 12.5: profiles/r05b, r05c)
    const bool overlap = !g_big_no_overlap && nparts <= 1;
    const int helper = kMaxSide + part;          // this part's helper stream (pool slot)
    for (int it = 0; it < a.maxIter; ++it) {
        ph.it = it;
        if (overlap) {
            void* side[1];
            if ((e = stream_fork(stream, 1, side, 0, helper))) return e;
            BigCtx<T> cs = c; cs.stream = side[0];
            if ((e = big_symv<T>(cs, L.v(bvA), L.v(bvB), 1))) return e;
            ph.split = 1;
            if ((e = big_potrf<T>(c, L.T, nbm, true, L.Wt, QPX_ST_KKT_BREAKDOWN, 1, &ph, 7))) return e;
            if ((e = stream_join(stream, 1, side, helper))) return e;
            if ((e = big_solve_fused<T>(c, L.T, L.Wt, nbm, L.v(bvRH), L.v(bvX), ph, 3, 1, 2))) return e;
        } else {
            if ((e = big_symv<T>(c, L.v(bvA), L.v(bvB), 1))) return e;
            ph.split = 0;
            if ((e = big_potrf<T>(c, L.T, nbm, true, L.Wt, QPX_ST_KKT_BREAKDOWN, 1, &ph, 2))) return e;
            if ((e = big_solve_fused<T>(c, L.T, L.Wt, nbm, L.v(bvRH), L.v(bvX), ph, 3, 1))) return e;
        }
        if ((e = big_solve_fused<T>(c, L.T, L.Wt, nbm, L.v(bvRH), L.v(bvX), ph, 4, 1))) return e;
    }
    ph.phase = 5;
    if ((e = launch_big_phase<T>(ph, stream))) return e;
    // zhat = -Lq^-T (u + Ztp^T z'_best)
    if ((e = big_mv<T>(c, L.Zt, L.NP, a.m, a.n, 1, L.v(bvA), L.v(bvU), true, L.v(bvW), T(1), T(1), 0))) return e;
    if ((e = big_solve<T>(c, L.Lq, L.Wq, nbq, 1, L.v(bvW), L.v(bvW), 1, 0))) return e;
    BigVecArgs<T> v{};
    v.B = a.B; v.op = 0; v.len = a.n; v.x = a.fac + L.v(bvW); v.sx = a.fac_stride; v.y = a.zhat; v.sy = (size_t)a.n; v.alpha = T(1);
    v.out32 = a.io32;
    if ((e = launch_big_vec<T>(v, stream))) return e;
    if (q > 0) {
        // nu = -(t + L11^-T (Vh^T z'_best))
        if ((e = big_mv<T>(c, L.Vh, L.QP, a.m, q, 1, L.v(bvA), 0, false, L.v(bvNU), T(1), T(0), 0))) return e;
        if ((e = big_solve<T>(c, L.S11, L.Wy, nbe, 1, L.v(bvNU), L.v(bvNU), 0, 0))) return e;
        v.len = q; v.x = a.fac + L.v(bvNU); v.y0 = a.fac + L.v(bvT1); v.sy0 = a.fac_stride; v.y = a.nu; v.sy = (size_t)q; v.alpha = T(-1); v.beta = T(-1);
        if ((e = launch_big_vec<T>(v, stream))) return e;
    }
    return QPX_OK;
}

// The condensed KKT solve of the family on the blob's solve vectors (set up by big_kkt_body stage 0 or by the finishing
// stage): vD = 1/d, vRH = rs/d - rz, vU = rx, vBQ = ry  ->  dz = vX, dx = vW, dy = vNU.
//   u = Lq^-1 rx;  rhs += Ztp u + Vh L11^-1 ry;  T = R + 1/d;  dz = -T^-1 rhs;
//   t = S11^-1 (ry - Yt u);  dx = -Lq^-T (u + Ztp^T dz + Yt^T t);  dy = t - L11^-T Vh^T dz
// backward (= "ry is zero": a backward without a cotangent on nu): no L11^-1 ry term; factor = false: T's factor of the
// previous call is still in the blob (a second right-hand side with the same d: the finishing stage's corrector)
template <class T>
int big_kkt_core(const BigCtx<T>& c, bool backward, bool factor)
{
    const BigLayout& L = c.L;
    const int n = c.n, m = c.m, q = c.q;
    const int nbq = L.NP / kBB, nbm = L.MP / kBB, nbe = L.QP / kBB;
    int e;
    if ((e = big_solve<T>(c, L.Lq, L.Wq, nbq, 0, L.v(bvU), L.v(bvU), 0, 0))) return e;
    if ((e = big_mv<T>(c, L.Zt, L.NP, m, n, 0, L.v(bvU), L.v(bvRH), true, L.v(bvRH), T(1), T(1), 0))) return e;
    if (q > 0) {
        if (!backward) {
            if ((e = big_solve<T>(c, L.S11, L.Wy, nbe, 0, L.v(bvBQ), L.v(bvTB), 0, 0))) return e;
            if ((e = big_mv<T>(c, L.Vh, L.QP, m, q, 0, L.v(bvTB), L.v(bvRH), true, L.v(bvRH), T(1), T(1), 0))) return e;
        }
        if ((e = big_mv<T>(c, L.Yt, L.NP, q, n, 0, L.v(bvU), L.v(bvBQ), true, L.v(bvT1), T(-1), T(1), 0))) return e;
        if ((e = big_solve<T>(c, L.S11, L.Wy, nbe, 2, L.v(bvT1), L.v(bvT1), 0, 0))) return e;
        if ((e = big_mv<T>(c, L.Yt, L.NP, q, n, 1, L.v(bvT1), L.v(bvU), true, L.v(bvU), T(1), T(1), 0))) return e;          // u + Yt^T t
    }
    if (factor && (e = big_potrf<T>(c, L.T, nbm, true, L.Wt, QPX_ST_KKT_BREAKDOWN, 0))) return e;
    if ((e = big_solve<T>(c, L.T, L.Wt, nbm, 2, L.v(bvRH), L.v(bvX), 1, 0))) return e;
    if ((e = big_mv<T>(c, L.Zt, L.NP, m, n, 1, L.v(bvX), L.v(bvU), true, L.v(bvW), T(1), T(1), 0))) return e;
    if ((e = big_solve<T>(c, L.Lq, L.Wq, nbq, 1, L.v(bvW), L.v(bvW), 1, 0))) return e;
    if (q > 0) {
        if ((e = big_mv<T>(c, L.Vh, L.QP, m, q, 1, L.v(bvX), 0, false, L.v(bvNU), T(1), T(0), 0))) return e;
        if ((e = big_solve<T>(c, L.S11, L.Wy, nbe, 1, L.v(bvNU), L.v(bvNU), 0, 0))) return e;
        BigVecArgs<T> v{};
        v.B = c.B; v.op = 0; v.len = q; v.x = c.fac + L.v(bvNU); v.sx = c.fs; v.y0 = c.fac + L.v(bvT1); v.sy0 = c.fs;
        v.y = c.fac + L.v(bvNU); v.sy = c.fs; v.alpha = T(-1); v.beta = T(1);
        if ((e = launch_big_vec<T>(v, c.stream))) return e;
    }
    return QPX_OK;
}

// forward mode (qpx_jvp): the tangents' products on top of what stage 0 of big_kkt_body wrote (vU = tp, vRH = th, vBQ = -tb;
// zhat, lam, nu at bvZ, bvS, bvY), by mat-vecs on the caller's row-major tangents:
//   vU += 1/2 tQ zhat + 1/2 tQ^T zhat + tG^T lam + tA^T nu,   vRH -= tG zhat,   vBQ += tA zhat
template <class T>
int big_jvp_products(const BigCtx<T>& c, const KktArgs<T>& a)
{
    const BigLayout& L = c.L;
    auto mv = [&](const T* M, long long sM, int rows, int trans, int x, int y, T alpha) {
        BigGemvArgs<T> g{};
        g.B = c.B; g.rows = rows; g.cols = c.n; g.trans = trans;
        g.M = M; g.sM = (size_t)sM; g.ld = c.n; g.dense = 1; g.m32 = a.io32;
        g.x = c.fac + L.v(x); g.sx = c.fs;
        g.y0 = c.fac + L.v(y); g.sy0 = c.fs;
        g.y = c.fac + L.v(y); g.sy = c.fs;
        g.alpha = alpha; g.beta = T(1);
        return launch_big_gemv<T>(g, c.stream);
    };
    int e;
    if (a.tQ && ((e = mv(a.tQ, a.stQ, c.n, 0, bvZ, bvU, T(0.5))) || (e = mv(a.tQ, a.stQ, c.n, 1, bvZ, bvU, T(0.5))))) return e;
    if (a.tG && ((e = mv(a.tG, a.stG, c.m, 1, bvS, bvU, T(1))) || (e = mv(a.tG, a.stG, c.m, 0, bvZ, bvRH, T(-1))))) return e;
    if (c.q > 0 && a.tA && ((e = mv(a.tA, a.stA, c.q, 1, bvY, bvU, T(1))) || (e = mv(a.tA, a.stA, c.q, 0, bvZ, bvBQ, T(1))))) return e;
    return QPX_OK;
}

template <class T, bool kBw>
int big_kkt(const KktArgs<T>& a, void* stream)
{
    BigCtx<T> c{a.B, a.n, a.m, a.fac, a.fac_stride, big_layout(a.n, a.m, a.q), stream, a.q};
    const int q = a.q;
    int e;
    BigKktArgs<T> k{};
    k.B = a.B; k.n = a.n; k.m = a.m; k.q = q; k.backward = kBw ? 1 : 0; k.fac = a.fac; k.fac_stride = a.fac_stride; k.io32 = a.io32;
    k.d = a.d; k.rx = a.rx; k.rs = a.rs; k.rz = a.rz; k.ry = a.ry; k.zhat = a.zhat; k.lam = a.lam; k.slack = a.slack; k.nu = a.nu; k.dl_dz = a.dl_dz;
    k.dl_dlam = a.dl_dlam; k.dl_dnu = a.dl_dnu;
    k.dx = a.dx; k.ds = a.ds; k.dz = a.dz; k.dy = a.dy; k.dQ = a.dQ; k.dp = a.dp; k.dG = a.dG; k.dh = a.dh; k.dA = a.dA; k.db = a.db; k.status = a.status;
    if constexpr (!kBw) {
        k.jvp = a.jvp; k.tp = a.tp; k.th = a.th; k.tb = a.tb; k.stp = a.stp; k.sth = a.sth; k.stb = a.stb;
    }
    k.stage = 0;
    if ((e = launch_big_kkt<T>(k, 1, stream))) return e;
    if constexpr (!kBw) {
        if (a.jvp && (e = big_jvp_products<T>(c, a))) return e;
    }
    // (a backward without a cotangent on nu has ry = 0: big_kkt_core leaves the L11^-1 ry term out, as it always did there)
    if ((e = big_kkt_core<T>(c, kBw && !(q > 0 && a.dl_dnu), true))) return e;
    k.stage = 1;
    int rows = a.n > a.m ? a.n : a.m;
    return launch_big_kkt<T>(k, kBw ? 1 + (rows + 15) / 16 : 1, stream);
}

// The finishing stage of the family (qpx_big_polish.h): `steps` iterations of the reference's loop in the original variables,
// residuals from the caller's data, every launch stream-ordered on the caller's stream
template <class T>
int big_polish(const PolishArgs<T>& a, void* stream)
{
    BigCtx<T> c{a.B, a.n, a.m, a.fac, a.fac_stride, big_layout(a.n, a.m, a.q), stream, a.q};
    BigPolishArgs<T> p{};
    p.B = a.B; p.n = a.n; p.m = a.m; p.q = a.q; p.fac = a.fac; p.fac_stride = a.fac_stride;
    p.Q = a.Q; p.G = a.G; p.A = a.A; p.sQ = a.sQ; p.sG = a.sG; p.sA = a.sA;
    p.p = a.p; p.h = a.h; p.b = a.b; p.sp = a.sp; p.sh = a.sh; p.sb = a.sb;
    p.zhat = a.zhat; p.nu = a.nu; p.lam = a.lam; p.slack = a.slack; p.best_resid = a.best_resid; p.status = a.status;
    int e;
    for (int st = 0; st <= a.steps; ++st) {
        p.stage = 1; p.first = st == 0; p.last = st == a.steps;
        if ((e = launch_big_polish<T>(p, stream))) return e;
        if (p.last) break;
        if ((e = big_kkt_core<T>(c, false, true))) return e;          // affine direction (factors T = R + diag(s/z))
        p.stage = 2;
        if ((e = launch_big_polish<T>(p, stream))) return e;
        if ((e = big_kkt_core<T>(c, false, false))) return e;         // centring-corrector direction, same factor
        p.stage = 3;
        if ((e = launch_big_polish<T>(p, stream))) return e;
    }
    return QPX_OK;
}
