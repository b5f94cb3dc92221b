// qpx_api.inc -- the C ABI of include/qpx.h: argument checks and the (dtype, NS, LDS-or-HBM)
// dispatch.  Included once by qpx_hip.hip after it has defined the three launchers
//
//   launch_sweep / launch_prefac_tile / launch_ipm_grid / launch_ipm_tile / launch_kkt_* / launch_polish_* / launch_big_* ...
//   (declared in qpx_launch.h), and  size_t lds_budget_bytes();   // LDS a workgroup may use (160 KiB on gfx950)
//
// (the host-thread emulator of the test tree includes it the same way with its own launchers).

namespace qpx {

constexpr int kMaxDim = 1024;                 // NS <= 16 slots of 64 lanes (r6; 512 / 8 until then)
constexpr int kMaxDimPolish = 512;            // the large-QP family's finishing stage keeps (7 + 16) vectors per QP in LDS: 94 KB at 512

// The A/B knob of qpx_set_ipm_variant is per host thread: two threads may measure different forms at once,
// and every call of the library is re-entrant (nothing else is mutable).
static thread_local int g_grid_size = 0;      // 0 auto; 16 / 8 / 1 = force the 16x16 / 8x8 thread grid / the matrix-core tiles in the loop kernel (variant + 256 / 512 / 1024)
static thread_local int g_ipm_variant = 0;    // qpx_set_ipm_variant: 0 auto, 3 the large-QP family at every size

// The thread-grid kernels (sweep pre-factorisation, ldl_inv IPM loop and backward; format-3 blob)
// run whenever the augmented order n+q+m fits 13 blocks of 16.  All entry points of one solve
// must see the same decision: it depends only on (n, m, q) and the variant knob.
inline bool use_grid(int n, int m, int q)
{
    return g_ipm_variant == 0 && grid_nb(n + q + m) > 0;
}

static thread_local int g_prefac_sweep = 0;   // variant bit 14: pre_factor_kkt by the thread-grid sweep also where the matrix-core form (qpx_prefac.h) serves the size
static thread_local int g_tile_nw = 0;        // 0 auto; 1 / 2 / 4 waves per QP in the tile kernel (variant + 2048 / 4096 / 8192)
// chain-wave form of the four-wave tile kernels (qpx_tile.h): one wave eliminates the pivot blocks a panel ahead
inline bool tile_chain(int nbt, int nw) { return (nbt == 7 || nbt == 4) && nw == 4; }
// Waves per QP of the matrix-core tile kernels.  The per-panel bookkeeping is replicated in every
// wave of a QP, so fewer waves cost fewer instructions in total; more waves shorten one QP's critical
// path while the chip has idle SIMDs.  MI355X, f64: B=512, nineq=100: loop 0.975 ms with 4 waves per
// QP, 1.06 with 2, 1.09 with 1 (the last two with MFMA accumulators forced into VGPRs by a compiler flag
// that has since been dropped: at 7 tile rows only the 4-wave form fits 256 registers without spilling);
// B=8192, nineq=64: 2.1 ms with 1 wave per QP, 3.3 with 2.
inline int tile_waves(int nbt, int B)
{
    int nw = g_tile_nw;
    // four waves per QP = the chain-wave form, from 33 rows up.  (Round 2 measured FOUR TILE-OWNING waves against one at
    // <= 64 rows and one wave won at every batch size; the chain-wave form -- three tile waves + the wave that
    // eliminates the pivot blocks a panel ahead -- turns that around: same box, loop kernel, one wave -> chain form:
    // B=512 n=100 m=50 q=10 (C3) 0.307 -> 0.237 ms, B=512 n=m=64 0.325 -> 0.254, B=128 n=m=50 0.267 -> 0.188,
    // B=2048 n=m=64 0.661 -> 0.656, B=8192 n=m=64 2.32 -> 2.32: profiles/archive/r03ve.)
    // Beyond ~8 K QPs the chip is full either way and one wave per QP issues less in total: B=16384 4.48 vs 4.53 ms,
    // B=65536 (C5 on one GPU) 17.39 vs 17.72 ms (profiles/archive/r03vf).
    // (r6) One wave per QP now keeps six workgroups on a CU instead of four at four tile rows (26 KB of LDS each:
    // TileMat::kInPlace) and wins from the first batch that does not fit the chip as two chain-form QPs per CU: same box,
    // loop kernel one wave / chain form, n = m = 64: B=512 0.342 / 0.245 ms, B=1024 0.338 / 0.420, B=2048 0.639 / 0.638,
    // B=4096 1.00 / 1.20, B=8192 1.81 / 2.26; n=100 m=50 q=10: B=512 0.331 / 0.228, B=1024 0.347 / 0.416, B=4096 1.31 / 1.51
    // (profiles/r06l_ab_one_wave_vs_chain_form.txt).
    if (nw == 0) nw = nbt == 7 ? 4 : (nbt == 4 && B <= 2 * 256 ? 4 : 1);
    if (nbt == 7 && nw == 1) nw = 2;         // the one-wave form is not built at this size (register budget)
    if (nbt <= 2) nw = 1;
    if (nbt == 4 && nw > 2) nw = 4;          // (four waves at four tile rows: the chain-wave form only)
    return nw;
}

// Blob family of a solve (qpx_layout.h: fac_layout): 0 = workgroup kernels (Cholesky factors), else the
// register images of R the thread-grid / tile consumers load: f64 with the tile kernels -> the tile image
// only (loop and backward both use it); otherwise the 16x16 grid image and the 8x8 one the loop switches
// to on a full chip.  Depends on (dtype, n, m, q) and the per-thread knob only, never on B: a shared blob
// is built with B = 1 and consumed with the batch's B.
// The large-QP family (qpx_big.h: batched multi-kernel Cholesky / GEMM path): every size beyond the thread-grid / tile
// kernels (round 4; measured on MI355X against the round-1 workgroup kernels it replaced there, f64 step times,
// profiles/archive/r04b: B=512 n=m=150 5.6 vs 20.2 ms, B=512 n=m=120 neq=30 3.3 vs 8.8, B=128 n=m=190 3.1 vs 18.7), or forced by knob 3.
inline bool use_big(int n, int m, int q, size_t elem_bytes)
{
    (void)elem_bytes;
    return g_ipm_variant == 3 || !use_grid(n, m, q);
}

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

template <class T> inline int blob_images(int n, int m, int q)
{
    if (use_big(n, m, q, sizeof(T))) return 8;
    return (std::is_same<T, double>::value && tile_nb(m) > 0 && (g_grid_size == 0 || g_grid_size == 1)) ? 4 : 3;
}

inline int slots_for(int n, int m, int q)
{
    int d = n > m ? n : m;
    d = d > q ? d : q;
    if (d <= 64) return 1;
    if (d <= 128) return 2;
    if (d <= 256) return 4;
    if (d <= 512) return 8;
    if (d <= kMaxDim) return 16;
    return 0;
}

inline int check_dims(int dtype, int B, int n, int m, int q)
{
    if (dtype != QPX_F32 && dtype != QPX_F64 && dtype != QPX_F32_WIDE) return QPX_ERR_ARG;
    if (B < 1 || n < 1 || m < 1 || q < 0) return QPX_ERR_ARG;   // nineq >= 1 (qp.py:87-89)
    if (q > n) return QPX_ERR_ARG;
    if (!slots_for(n, m, q)) return QPX_ERR_UNSUPPORTED;
    return QPX_OK;
}

template <class T> inline size_t blob_elems(int n, int m, int q)
{
    const int images = blob_images<T>(n, m, q);
    return images == 8 ? big_layout(n, m, q).total : fac_layout(n, m, q, images).total;
}

// ---------------------------------------------------------------------------------- large-QP family: orchestration
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
                   int32_t* status, void* stream, int io32)
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
// backward: ry = 0 (no L11^-1 ry term); factor = false: T's factor of the previous call is still in the blob (a second
// right-hand side with the same d: the finishing stage's corrector)
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
    k.dx = a.dx; k.ds = a.ds; k.dz = a.dz; k.dy = a.dy; k.dQ = a.dQ; k.dp = a.dp; k.dG = a.dG; k.dh = a.dh; k.dA = a.dA; k.db = a.db; k.status = a.status;
    if constexpr (!kBw) {
        k.jvp = a.jvp; k.tp = a.tp; k.th = a.th; k.tb = a.tb; k.stp = a.stp; k.sth = a.sth; k.stb = a.stb;
    }
    k.stage = 0;
    if ((e = launch_big_kkt<T>(k, 1, stream))) return e;
    if constexpr (!kBw) {
        if (a.jvp && (e = big_jvp_products<T>(c, a))) return e;
    }
    if ((e = big_kkt_core<T>(c, kBw, true))) return e;
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

template <class T>
int api_pre_factor(int B, int n, int m, int q, const void* Q, int64_t sQ, const void* G, int64_t sG,
                   const void* A, int64_t sA, void* factors, int32_t* status, void* stream, int io32 = 0)
{
    if (!Q || !G || !factors || !status || (q > 0 && !A)) return QPX_ERR_ARG;
    PrefactorArgs<T> a;
    a.io32 = io32;
    a.B = B; a.n = n; a.m = m; a.q = q;
    a.Q = (const T*)Q; a.G = (const T*)G; a.A = (const T*)A;
    a.sQ = sQ; a.sG = sG; a.sA = sA;
    a.images = blob_images<T>(n, m, q);
    if (a.images == 8) {
        const size_t fs = big_layout(n, m, q).total;
        return big_split(B, stream, true, [&](int q0, int cnt, void* st, int part, int nparts) {
            return big_pre_factor<T>(cnt, n, m, q, advio(a.Q, (size_t)q0 * sQ, io32), sQ, advio(a.G, (size_t)q0 * sG, io32), sG,
                                     advio(a.A, (size_t)q0 * sA, io32), sA, (T*)factors + (size_t)q0 * fs, status + q0, st, io32);
        });
    }
    a.fac = (T*)factors; a.fac_stride = fac_layout(n, m, q, a.images).total; a.status = status;
    if constexpr (std::is_same<T, double>::value) {
        // f64 (and float32 arrays in f64 arithmetic), 33 <= nz + neq <= 112 (four or seven tile rows), the tile image only: factorisation of Q (of
        // [[Q, A^T], [A, 0]]) + tile products on the matrix cores (qpx_prefac.h) instead of the sweep
        if (use_grid(n, m, q) && !g_prefac_sweep && prefac_tile_serves(n, m, q, a.images)) {
            const int nbn = tile_nb(n + q);
            const size_t pb = lds_elems_prefac_tile(nbn, (m + 15) / 16) * sizeof(double);
            prefac_deal(nbn, n + q, m, a.pf_k, a.pf_r);
                    if (q > 0) return nbn == 7 ? launch_prefac_tile<7, true>(a, pb, stream) : launch_prefac_tile<4, true>(a, pb, stream);
            return nbn == 7 ? launch_prefac_tile<7, false>(a, pb, stream) : launch_prefac_tile<4, false>(a, pb, stream);
        }
    }
    if (use_grid(n, m, q)) {
        const int nba = sweep_nb(n + q + m);
        const size_t gb = lds_elems_sweep(nba) * sizeof(T);
        switch (nba) {
        case 8: return launch_sweep<T, 8>(a, gb, stream);
        case 1: return launch_sweep<T, 1>(a, gb, stream);
        case 2: return launch_sweep<T, 2>(a, gb, stream);
        case 4: return launch_sweep<T, 4>(a, gb, stream);
        case 7: return launch_sweep<T, 7>(a, gb, stream);
        case 10: return launch_sweep<T, 10>(a, gb, stream);
        case 13: return launch_sweep<T, 13>(a, gb, stream);
        }
    }
    return QPX_ERR_UNSUPPORTED;
}

template <class T>
int api_ipm(int B, int n, int m, int q, const void* p, int64_t sp, const void* h, int64_t sh,
            const void* bb, int64_t sb, void* factors, int64_t sfac, double eps, int maxIter, int notImprovedLim,
            int stall_policy, void* zhat, void* nu, void* lam, void* slack, int32_t* iters,
            int32_t* status, void* best_resid, void* trace, void* stream, int io32 = 0)
{
    if (!p || !h || !factors || !zhat || !lam || !slack || !iters || !status || !best_resid ||
        (q > 0 && (!nu || !bb)))
        return QPX_ERR_ARG;
    if (maxIter < 0 || stall_policy < 0 || stall_policy > 2) return QPX_ERR_ARG;
    IpmArgs<T> a;
    a.io32 = io32;
    a.B = B; a.n = n; a.m = m; a.q = q;
    a.p = (const T*)p; a.h = (const T*)h; a.b = (const T*)bb;
    a.sp = sp; a.sh = sh; a.sb = sb;
    a.fac = (T*)factors; a.fac_stride = (size_t)sfac;
    a.eps = (T)eps; a.maxIter = maxIter; a.notImprovedLim = notImprovedLim; a.stall_policy = stall_policy;
    a.zhat = (T*)zhat; a.nu = (T*)nu; a.lam = (T*)lam; a.slack = (T*)slack;
    a.iters = iters; a.status = status; a.best_resid = (T*)best_resid; a.trace = (T*)trace;
    a.images = blob_images<T>(n, m, q);
    if (a.images == 8) {
        if (sfac == 0 && B > 1) return QPX_ERR_ARG;       // per-QP work matrices live in the blob
        return big_split(B, stream, a.trace == nullptr, [&](int q0, int cnt, void* st, int part, int nparts) {     // trace is indexed [it][B][3]
            IpmArgs<T> s = a;
            const size_t o = (size_t)q0;
            s.B = cnt;
            s.p = advio(a.p, o * a.sp, io32); s.h = advio(a.h, o * a.sh, io32); s.b = advio(a.b, o * a.sb, io32);
            s.fac += o * a.fac_stride;
            s.zhat = advio(a.zhat, o * n, io32); s.lam = advio(a.lam, o * m, io32); s.slack = advio(a.slack, o * m, io32);
            s.nu = advio(a.nu, o * q, io32);
            s.iters += q0; s.status += q0; s.best_resid = advio(a.best_resid, o, io32);
            return big_ipm<T>(s, st, part, nparts);
        });
    }
    if (use_grid(n, m, q)) {
        // one wave per QP (8x8 grid) when it is instantiated: fewer instructions per column on the
        // critical path than four waves sharing the update, and no workgroup barrier
        const int nb8 = wave_nb(m);
        const int ns8 = nb8 > 0 ? slots_for(n, 8 * nb8, q) : 0;
        // Measured on MI355X (f64): at B=512, n=m=100 four waves per QP finish the loop in 1.52 ms, one
        // wave per QP in 2.06 ms (the chip is not full, latency per QP decides); at B=8192, n=m=64 it is
        // 7.1 ms against 5.1 ms (the chip is full, instructions per QP decide).
        const bool chip_full = a.B > 1024;
        if (((g_grid_size == 0 && chip_full && !(std::is_same<T, double>::value && tile_nb(m) > 0)) || g_grid_size == 8) && nb8 > 0 && (ns8 == 1 || ns8 == 2) &&
            !(ns8 == 1 && nb8 > 8)) {
            const size_t wb = lds_elems_ipm_grid(8, nb8, n, q) * sizeof(T);
            switch (nb8 * 10 + ns8) {
            case 21: return launch_ipm_grid8<T, 2, 1>(a, wb, stream);
            case 22: return launch_ipm_grid8<T, 2, 2>(a, wb, stream);
            case 41: return launch_ipm_grid8<T, 4, 1>(a, wb, stream);
            case 42: return launch_ipm_grid8<T, 4, 2>(a, wb, stream);
            case 81: return launch_ipm_grid8<T, 8, 1>(a, wb, stream);
            case 82: return launch_ipm_grid8<T, 8, 2>(a, wb, stream);
            case 132: return launch_ipm_grid8<T, 13, 2>(a, wb, stream);
            }
        }
        if constexpr (std::is_same<T, double>::value) {
            // matrix-core tiles (qpx_tile.h): rank-4 blocked factorisation, one MFMA per tile and panel
            const int nbt = tile_nb(m);
            const int nst = nbt > 0 ? slots_for(n, 16 * nbt, q) : 0;
            if ((g_grid_size == 0 || g_grid_size == 1) && nbt > 0 && nst >= 1 && nst <= 4 && !(nbt == 7 && nst == 1)) {
                // waves per QP: the per-panel bookkeeping is replicated in every wave of a QP, so fewer
                // waves cost fewer instructions in total; more waves shorten one QP's critical path
                // while the chip has idle SIMDs (B < ~2 per CU x 256 CUs)
                const int nw = tile_waves(nbt, a.B);
                const bool ch = tile_chain(nbt, nw);
                // (measurement hook, scripts/occupancy_probe.py: QPX_LDS_PAD_BYTES in the environment adds unused LDS to the
                // tile loop kernel's launches, i.e. lowers the workgroups a CU holds -- how a kernel's time answers to
                // occupancy is read off without rebuilding it)
                static const size_t lds_pad = [] { const char* e = std::getenv("QPX_LDS_PAD_BYTES"); return e ? (size_t)std::atol(e) : (size_t)0; }();
                const size_t tb = lds_elems_ipm_tile(nbt, nw, n, q, ch) * sizeof(T) + lds_pad;
                if (ch && nbt == 7) {
                    if (nst == 2) return launch_ipm_tile<7, 4, 2, true>(a, tb, stream);
                    if (nst == 4) return launch_ipm_tile<7, 4, 4, true>(a, tb, stream);
                }
                if (ch && nbt == 4) {
                    if (nst == 1) return launch_ipm_tile<4, 4, 1, true>(a, tb, stream);
                    if (nst == 2) return launch_ipm_tile<4, 4, 2, true>(a, tb, stream);
                    if (nst == 4) return launch_ipm_tile<4, 4, 4, true>(a, tb, stream);
                }
                switch ((nbt * 10 + nw) * 10 + nst) {
                case 111: return launch_ipm_tile<1, 1, 1>(a, tb, stream);
                case 112: return launch_ipm_tile<1, 1, 2>(a, tb, stream);
                case 114: return launch_ipm_tile<1, 1, 4>(a, tb, stream);
                case 211: return launch_ipm_tile<2, 1, 1>(a, tb, stream);
                case 212: return launch_ipm_tile<2, 1, 2>(a, tb, stream);
                case 214: return launch_ipm_tile<2, 1, 4>(a, tb, stream);
                case 411: return launch_ipm_tile<4, 1, 1>(a, tb, stream);
                case 412: return launch_ipm_tile<4, 1, 2>(a, tb, stream);
                case 414: return launch_ipm_tile<4, 1, 4>(a, tb, stream);
                case 421: return launch_ipm_tile<4, 2, 1>(a, tb, stream);
                case 422: return launch_ipm_tile<4, 2, 2>(a, tb, stream);
                case 424: return launch_ipm_tile<4, 2, 4>(a, tb, stream);
                case 722: return launch_ipm_tile<7, 2, 2>(a, tb, stream);
                case 724: return launch_ipm_tile<7, 2, 4>(a, tb, stream);
                }
            }
        }
        const int nbg = grid_nb(m);
        const int nsg = slots_for(n, 16 * nbg, q);
        const size_t gb = lds_elems_ipm_grid(16, nbg, n, q) * sizeof(T);
        switch (nbg * 10 + nsg) {
        case 11: return launch_ipm_grid<T, 1, 1>(a, gb, stream);
        case 12: return launch_ipm_grid<T, 1, 2>(a, gb, stream);
        case 14: return launch_ipm_grid<T, 1, 4>(a, gb, stream);
        case 21: return launch_ipm_grid<T, 2, 1>(a, gb, stream);
        case 22: return launch_ipm_grid<T, 2, 2>(a, gb, stream);
        case 24: return launch_ipm_grid<T, 2, 4>(a, gb, stream);
        case 41: return launch_ipm_grid<T, 4, 1>(a, gb, stream);
        case 42: return launch_ipm_grid<T, 4, 2>(a, gb, stream);
        case 44: return launch_ipm_grid<T, 4, 4>(a, gb, stream);
        case 72: return launch_ipm_grid<T, 7, 2>(a, gb, stream);
        case 74: return launch_ipm_grid<T, 7, 4>(a, gb, stream);
        case 104: return launch_ipm_grid<T, 10, 4>(a, gb, stream);
        case 134: return launch_ipm_grid<T, 13, 4>(a, gb, stream);
        }
        return QPX_ERR_UNSUPPORTED;
    }
    return QPX_ERR_UNSUPPORTED;
}

template <class T, bool kBw>
int api_kkt(KktArgs<T>& a, void* stream)
{
    const int n = a.n, m = a.m, q = a.q;
    a.images = blob_images<T>(n, m, q);
    if (a.images == 8) {
        if (a.fac_stride == 0 && a.B > 1) return QPX_ERR_ARG;
        // (parts only when the knob asks for them: one factorisation + one solve is too short a sequence for two parts to
        // fill each other's gaps -- same box, backward by events, one part / two: C4 0.643 / 0.645 ms, B=128 n=300 m=200 q=50
        // 0.273 / 0.297, B=512 n=m=150 0.303 / 0.319, and twice the host's enqueue time: profiles/r06q_backward_parts.txt)
        return big_split(a.B, stream, g_big_parts != 0, [&](int q0, int cnt, void* st, int part, int nparts) {
            KktArgs<T> s = a;
            const size_t o = (size_t)q0;
            const int w = a.io32;
            s.B = cnt;
            s.fac += o * a.fac_stride;
            s.d = advio(a.d, o * m, w); s.rx = advio(a.rx, o * n, w); s.rs = advio(a.rs, o * m, w); s.rz = advio(a.rz, o * m, w); s.ry = advio(a.ry, o * q, w);
            s.dx = advio(a.dx, o * n, w); s.ds = advio(a.ds, o * m, w); s.dz = advio(a.dz, o * m, w); s.dy = advio(a.dy, o * q, w);
            s.zhat = advio(a.zhat, o * n, w); s.lam = advio(a.lam, o * m, w); s.slack = advio(a.slack, o * m, w); s.nu = advio(a.nu, o * q, w);
            s.dl_dz = advio(a.dl_dz, o * n, w);
            s.dQ = advio(a.dQ, o * n * n, w); s.dp = advio(a.dp, o * n, w); s.dG = advio(a.dG, o * m * n, w); s.dh = advio(a.dh, o * m, w);
            s.dA = advio(a.dA, o * q * n, w); s.db = advio(a.db, o * q, w);
            s.tQ = advio(a.tQ, o * a.stQ, w); s.tp = advio(a.tp, o * a.stp, w); s.tG = advio(a.tG, o * a.stG, w);
            s.th = advio(a.th, o * a.sth, w); s.tA = advio(a.tA, o * a.stA, w); s.tb = advio(a.tb, o * a.stb, w);
            s.status = adv(a.status, o);
            return big_kkt<T, kBw>(s, st);
        });
    }
    if (use_grid(n, m, q)) {
        if constexpr (std::is_same<T, double>::value) {
            const int nbt = tile_nb(m);
            if ((g_grid_size == 0 || g_grid_size == 1) && nbt > 0) {
                const int nw = tile_waves(nbt, a.B);
                const bool ch = tile_chain(nbt, nw);
                const size_t tb = lds_elems_kkt_tile(nbt, nw, n, q, ch) * sizeof(T);
                if (ch && nbt == 7) return launch_kkt_tile<7, 4, kBw, true>(a, tb, stream);
                if (ch && nbt == 4) return launch_kkt_tile<4, 4, kBw, true>(a, tb, stream);
                switch (nbt * 10 + nw) {
                case 11: return launch_kkt_tile<1, 1, kBw>(a, tb, stream);
                case 21: return launch_kkt_tile<2, 1, kBw>(a, tb, stream);
                case 41: return launch_kkt_tile<4, 1, kBw>(a, tb, stream);
                case 42: return launch_kkt_tile<4, 2, kBw>(a, tb, stream);
                case 72: return launch_kkt_tile<7, 2, kBw>(a, tb, stream);
                }
            }
        }
        const int nbg = grid_nb(m);
        const size_t gb = lds_elems_kkt_grid(16, nbg, n, q) * sizeof(T);
        switch (nbg) {
        case 1: return launch_kkt_grid<T, 1, kBw>(a, gb, stream);
        case 2: return launch_kkt_grid<T, 2, kBw>(a, gb, stream);
        case 4: return launch_kkt_grid<T, 4, kBw>(a, gb, stream);
        case 7: return launch_kkt_grid<T, 7, kBw>(a, gb, stream);
        case 10: return launch_kkt_grid<T, 10, kBw>(a, gb, stream);
        case 13: return launch_kkt_grid<T, 13, kBw>(a, gb, stream);
        }
        return QPX_ERR_UNSUPPORTED;
    }
    return QPX_ERR_UNSUPPORTED;
}

// forward mode: the KKT solve of the backward (same d, same kernels: api_kkt<T, false>) with the right-hand side formed from
// the tangents inside them (KktArgs::jvp)
template <class T>
int api_jvp(int io32, int B, int n, int m, int q, void* factors, int64_t sfac, const void* zhat, const void* lam,
            const void* slack, const void* nu, const void* tQ, int64_t stQ, const void* tp, int64_t stp, const void* tG,
            int64_t stG, const void* th, int64_t sth, const void* tA, int64_t stA, const void* tb, int64_t stb, void* dzhat,
            void* dlam, void* dnu, void* dslack, int refine, const void* Q, int64_t sQ, const void* G, int64_t sG,
            const void* A, int64_t sA, int32_t* status, void* stream)
{
    // (kkt_jvp_rhs holds n <= 256 columns per lane in four slots: the thread-grid / tile sizes have n < 208)
    if (!use_big(n, m, q, sizeof(T)) && n > 4 * kWave) return QPX_ERR_UNSUPPORTED;
    KktArgs<T> a{};
    a.io32 = io32;
    a.B = B; a.n = n; a.m = m; a.q = q; a.fac = (T*)factors; a.fac_stride = (size_t)sfac;
    a.zhat = (const T*)zhat; a.lam = (const T*)lam; a.slack = (const T*)slack; a.nu = (const T*)nu;
    a.jvp = 1;
    a.tQ = (const T*)tQ; a.tp = (const T*)tp; a.tG = (const T*)tG; a.th = (const T*)th; a.tA = (const T*)tA; a.tb = (const T*)tb;
    a.stQ = stQ; a.stp = stp; a.stG = stG; a.sth = sth; a.stA = stA; a.stb = stb;
    a.dx = (T*)dzhat; a.dz = (T*)dlam; a.dy = (T*)dnu; a.ds = (T*)dslack;
    a.status = status;
    a.refine = refine; a.Q = (const T*)Q; a.G = (const T*)G; a.A = (const T*)A; a.sQ = sQ; a.sG = sG; a.sA = sA;
    return api_kkt<T, false>(a, stream);
}

// the finishing stage: every family has it (thread-grid / tile kernels: one kernel, the blob's register image of R decides the
// form; large-QP family: qpx_big_polish.h)
inline bool polish_served(int dtype, int n, int m, int q)
{
    const int d = n > m ? (n > q ? n : q) : (m > q ? m : q);
    return dtype != QPX_F32_WIDE && d <= kMaxDimPolish && (use_grid(n, m, q) || use_big(n, m, q, dtype != QPX_F32 ? 8 : 4));
}
template <class T>
int api_polish(PolishArgs<T>& a, void* stream)
{
    const int n = a.n, m = a.m, q = a.q;
    a.images = blob_images<T>(n, m, q);
    if (a.images == 8) {
        // the large-QP family: its KKT solve has no in-kernel refinement (qpx_refine_supported) -- asked for, it is refused
        if (a.refine > 0) return QPX_ERR_UNSUPPORTED;
        if (a.fac_stride == 0 && a.B > 1) return QPX_ERR_ARG;
        return big_split(a.B, stream, true, [&](int q0, int cnt, void* st, int part, int nparts) {
            PolishArgs<T> s2 = a;
            const size_t o = (size_t)q0;
            s2.B = cnt;
            s2.fac += o * a.fac_stride;
            s2.Q = adv(a.Q, o * a.sQ); s2.G = adv(a.G, o * a.sG); s2.A = adv(a.A, o * a.sA);
            s2.p = adv(a.p, o * a.sp); s2.h = adv(a.h, o * a.sh); s2.b = adv(a.b, o * a.sb);
            s2.zhat = adv(a.zhat, o * n); s2.lam = adv(a.lam, o * m); s2.slack = adv(a.slack, o * m); s2.nu = adv(a.nu, o * q);
            s2.best_resid = adv(a.best_resid, o); s2.status = adv(a.status, o);
            return big_polish<T>(s2, st);
        });
    }
    if (a.images != 3 && a.images != 4) return QPX_ERR_UNSUPPORTED;
    if constexpr (std::is_same<T, double>::value) {
        if (a.images == 4) {
            // the default forms of the tile kernels by (tile rows, batch): tile_waves() without its A/B knob
            const int nbt = tile_nb(m);
            const bool ch = nbt == 7 || (nbt == 4 && a.B <= 8192);
            const size_t tb = lds_elems_polish_mat(16 * (size_t)nbt, tile_scratch_elems(nbt, ch ? 3 : 1, ch), n, q, sizeof(T)) * sizeof(T);
            switch (nbt) {
            case 1: return launch_polish_tile<1, 1, false>(a, tb, stream);
            case 2: return launch_polish_tile<2, 1, false>(a, tb, stream);
            case 4: return ch ? launch_polish_tile<4, 4, true>(a, tb, stream) : launch_polish_tile<4, 1, false>(a, tb, stream);
            case 7: return launch_polish_tile<7, 4, true>(a, tb, stream);
            }
            return QPX_ERR_UNSUPPORTED;
        }
    }
    const int nbg = grid_nb(m);
    const size_t gb = lds_elems_polish_grid(16, nbg, n, q, sizeof(T)) * sizeof(T);
    switch (nbg) {
    case 1: return launch_polish_grid<T, 1>(a, gb, stream);
    case 2: return launch_polish_grid<T, 2>(a, gb, stream);
    case 4: return launch_polish_grid<T, 4>(a, gb, stream);
    case 7: return launch_polish_grid<T, 7>(a, gb, stream);
    case 10: return launch_polish_grid<T, 10>(a, gb, stream);
    case 13: return launch_polish_grid<T, 13>(a, gb, stream);
    }
    return QPX_ERR_UNSUPPORTED;
}

template <class T>
int api_batch_outer(int B, int r, int c, const void* u, const void* v, const void* w, const void* x, double scale,
                    void* out, void* ws, size_t ws_elems, void* stream)
{
    OuterArgs<T> a;
    a.B = B; a.r = r; a.c = c;
    a.u = (const T*)u; a.v = (const T*)v; a.w = (const T*)w; a.x = (const T*)x;
    a.scale = (T)(scale / (double)B); a.out = (T*)out;
    const int tiles = ((r + 15) / 16) * ((c + 15) / 16);
    // two stages (partial tiles per batch chunk -> sum in chunk order) when the caller brought the workspace for them
    a.chunks = outer_chunks(B, tiles);
    if (a.chunks > 1 && (!ws || ws_elems < (size_t)a.chunks * tiles * 256)) a.chunks = 1;
    a.chunk_len = outer_chunk_len(B, a.chunks);
    a.ws = a.chunks > 1 ? (T*)ws : nullptr;
    return launch_batch_outer<T>(a, tiles, stream);
}

}  // namespace qpx

extern "C" {

int qpx_abi_version(void) { return QPX_ABI_VERSION; }

const char* qpx_strerror(int code)
{
    switch (code) {
    case QPX_OK: return "ok";
    case QPX_ERR_ARG: return "invalid argument (dtype, sizes or null pointer)";
    case QPX_ERR_UNSUPPORTED: return "not supported by this build for this size / dtype (max(n,m,q) > 1024, or an option -- in-kernel refinement, QPX_F32_WIDE -- that the kernel family serving this size does not implement: qpx_supported, qpx_refine_supported)";
    case QPX_ERR_LAUNCH: return "HIP kernel launch failed";
    case QPX_ERR_NO_DEVICE: return "no HIP device";
    }
    return "unknown error";
}

size_t qpx_factor_elems(int dtype, int n, int m, int q)
{
    return dtype != QPX_F32 ? qpx::blob_elems<double>(n, m, q) : qpx::blob_elems<float>(n, m, q);   // QPX_F32_WIDE: doubles
}

int qpx_max_dim(void) { return qpx::kMaxDim; }

int qpx_supported(int dtype, int n, int m, int q) { return qpx::check_dims(dtype, 1, n, m, q); }

int qpx_kernel_family(int dtype, int n, int m, int q)
{
    if (const int e = qpx::check_dims(dtype, 1, n, m, q)) return e;
    if (qpx::use_big(n, m, q, dtype != QPX_F32 ? 8 : 4)) return QPX_FAMILY_BIG;
    return (dtype != QPX_F32 && qpx::tile_nb(m) > 0 && (qpx::g_grid_size == 0 || qpx::g_grid_size == 1)) ? QPX_FAMILY_TILE : QPX_FAMILY_GRID;
}

int qpx_refine_supported(int dtype, int n, int m, int q)
{
    // in-kernel iterative refinement lives in the thread-grid / tile KKT kernels (qpx_grid.h: kkt_mat_role), and it
    // reads Q, G, A in the kernels' own type
    if (qpx::check_dims(dtype, 1, n, m, q) != QPX_OK) return 0;
    return dtype != QPX_F32_WIDE && qpx::use_grid(n, m, q) ? 1 : 0;
}

int qpx_set_ipm_variant(int variant)
{
    const int old = qpx_get_ipm_variant();
    qpx::g_ipm_variant = (variant & 255) == 3 ? 3 : 0;        // (1 selected the round-1 workgroup kernels until v7)
    qpx::g_grid_size = (variant & 256) ? 16 : ((variant & 512) ? 8 : ((variant & 1024) ? 1 : 0));
    qpx::g_tile_nw = (variant & 2048) ? 1 : ((variant & 4096) ? 2 : ((variant & 8192) ? 4 : 0));
    qpx::g_prefac_sweep = (variant >> 14) & 1;
    qpx::g_big_parts = (variant >> 16) & 15;
    qpx::g_big_delay = (variant >> 20) & 31;
    qpx::g_big_no_overlap = (variant >> 26) & 1;
    qpx::g_big_diag_one_wave = (variant >> 27) & 1;
    qpx::g_big_grid_diag = (variant >> 28) & 1;
    qpx::g_big_no_swizzle = (variant >> 29) & 1;
    return old;
}

int qpx_get_ipm_variant(void)
{
    return qpx::g_ipm_variant | (qpx::g_grid_size == 16 ? 256 : 0) | (qpx::g_grid_size == 8 ? 512 : 0) |
           (qpx::g_grid_size == 1 ? 1024 : 0) | (qpx::g_tile_nw == 1 ? 2048 : 0) |
           (qpx::g_tile_nw == 2 ? 4096 : 0) | (qpx::g_tile_nw == 4 ? 8192 : 0) | (qpx::g_prefac_sweep << 14) | (qpx::g_big_parts << 16) |
           (qpx::g_big_delay << 20) | (qpx::g_big_no_overlap << 26) | (qpx::g_big_diag_one_wave << 27) | (qpx::g_big_grid_diag << 28) | (qpx::g_big_no_swizzle << 29);
}

int qpx_big_gemm_r(int dtype, int B, int n, int m, int q, void* factors, void* stream)
{
    if (const int e = qpx::check_dims(dtype, B, n, m, q)) return e;
    if (!factors) return QPX_ERR_ARG;
    if (!qpx::use_big(n, m, q, dtype != QPX_F32 ? 8 : 4)) return QPX_ERR_UNSUPPORTED;
    return dtype != QPX_F32 ? qpx::big_gemm_r<double>(B, n, m, (double*)factors, stream, q)
                            : qpx::big_gemm_r<float>(B, n, m, (float*)factors, stream, q);
}

int qpx_can_share_factors(int dtype, int n, int m, int q)
{
    // the thread-grid / tile kernels only read the blob; the large-QP family keeps per-QP work matrices in it
    if (qpx::check_dims(dtype, 1, n, m, q) != QPX_OK) return 0;
    return qpx::use_big(n, m, q, dtype != QPX_F32 ? 8 : 4) ? 0 : 1;
}

int qpx_pre_factor(int dtype, int B, int n, int m, int q, const void* Q, int64_t sQ, const void* G,
                   int64_t sG, const void* A, int64_t sA, void* factors, int32_t* status,
                   qpx_stream_t stream)
{
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    return dtype != QPX_F32
               ? qpx::api_pre_factor<double>(B, n, m, q, Q, sQ, G, sG, A, sA, factors, status, stream, dtype == QPX_F32_WIDE)
               : qpx::api_pre_factor<float>(B, n, m, q, Q, sQ, G, sG, A, sA, factors, status, stream);
}

int qpx_ipm(int dtype, int B, int n, int m, int q, const void* p, int64_t sp, const void* h,
            int64_t sh, const void* b, int64_t sb, void* factors, int64_t sfac, double eps, int maxIter,
            int notImprovedLim, int stall_policy, void* zhat, void* nu, void* lam, void* slack,
            int32_t* iters, int32_t* status, void* best_resid, void* trace, qpx_stream_t stream)
{
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    return dtype != QPX_F32
               ? qpx::api_ipm<double>(B, n, m, q, p, sp, h, sh, b, sb, factors, sfac, eps, maxIter, notImprovedLim, stall_policy, zhat, nu, lam, slack, iters, status, best_resid, trace, stream, dtype == QPX_F32_WIDE)
               : qpx::api_ipm<float>(B, n, m, q, p, sp, h, sh, b, sb, factors, sfac, eps, maxIter, notImprovedLim, stall_policy, zhat, nu, lam, slack, iters, status, best_resid, trace, stream);
}

int qpx_forward(int dtype, int B, int n, int m, int q, const void* Q, int64_t sQ, const void* p,
                int64_t sp, const void* G, int64_t sG, const void* h, int64_t sh, const void* A,
                int64_t sA, const void* b, int64_t sb, void* factors, double eps, int maxIter,
                int notImprovedLim, int stall_policy, void* zhat, void* nu, void* lam, void* slack,
                int32_t* iters, int32_t* status, void* best_resid, void* trace, qpx_stream_t stream)
{
    // (Round 5 built this entry point as ONE launch for C2's and C5's shapes -- the matrix-core pre-factorisation and the
    // chain-wave loop kernel back to back in one workgroup -- and measured it against the two launches on the same box:
    // 0.612 vs 0.568 ms at C2, 3.98 vs 2.86 ms at B = 8192 n = m = 64.  The launch boundary costs less than the union of the
    // two kernels' register and LDS budgets; starting the second workgroup of a CU late, so that the two QPs run out of
    // phase, lost exactly the delay.  Deleted; profiles/r05a_ab_forward_one_launch_*.txt.)
    int e = qpx_pre_factor(dtype, B, n, m, q, Q, sQ, G, sG, A, sA, factors, status, stream);
    if (e) return e;
    return qpx_ipm(dtype, B, n, m, q, p, sp, h, sh, b, sb, factors, (int64_t)qpx_factor_elems(dtype, n, m, q), eps, maxIter, notImprovedLim,
                   stall_policy, zhat, nu, lam, slack, iters, status, best_resid, trace, stream);
}

int qpx_factor_solve_kkt(int dtype, int B, int n, int m, int q, void* factors, int64_t sfac, const void* d,
                         const void* rx, const void* rs, const void* rz, const void* ry, void* dx,
                         void* ds, void* dz, void* dy, int refine, const void* Q, int64_t sQ, const void* G,
                         int64_t sG, const void* A, int64_t sA, int32_t* status, qpx_stream_t stream)
{
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    if (!factors || !d || !dx || !ds || !dz || (q > 0 && !dy)) return QPX_ERR_ARG;
    if (refine < 0) return QPX_ERR_ARG;
    if (refine > 0 && !qpx_refine_supported(dtype, n, m, q)) return QPX_ERR_UNSUPPORTED;   // loud: never silently ignored
    if (dtype != QPX_F32) {
        qpx::KktArgs<double> a{};
        a.io32 = dtype == QPX_F32_WIDE;
        a.B = B; a.n = n; a.m = m; a.q = q; a.fac = (double*)factors; a.fac_stride = (size_t)sfac;
        a.d = (const double*)d; a.rx = (const double*)rx; a.rs = (const double*)rs;
        a.rz = (const double*)rz; a.ry = (const double*)ry;
        a.dx = (double*)dx; a.ds = (double*)ds; a.dz = (double*)dz; a.dy = (double*)dy;
        a.status = status;
        a.refine = refine; a.Q = (const double*)Q; a.G = (const double*)G; a.A = (const double*)A; a.sQ = sQ; a.sG = sG; a.sA = sA;
        return qpx::api_kkt<double, false>(a, stream);
    }
    qpx::KktArgs<float> a{};
    a.B = B; a.n = n; a.m = m; a.q = q; a.fac = (float*)factors; a.fac_stride = (size_t)sfac;
    a.d = (const float*)d; a.rx = (const float*)rx; a.rs = (const float*)rs;
    a.rz = (const float*)rz; a.ry = (const float*)ry;
    a.dx = (float*)dx; a.ds = (float*)ds; a.dz = (float*)dz; a.dy = (float*)dy;
    a.status = status;
    a.refine = refine; a.Q = (const float*)Q; a.G = (const float*)G; a.A = (const float*)A; a.sQ = sQ; a.sG = sG; a.sA = sA;
    return qpx::api_kkt<float, false>(a, stream);
}

int qpx_backward(int dtype, int B, int n, int m, int q, void* factors, int64_t sfac, const void* zhat,
                 const void* lam, const void* slack, const void* nu, const void* dl_dz, void* dQ,
                 void* dp, void* dG, void* dh, void* dA, void* db, void* dx, void* dz, void* dy,
                 int refine, const void* Q, int64_t sQ, const void* G, int64_t sG, const void* A, int64_t sA,
                 int32_t* status, qpx_stream_t stream)
{
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    if (!factors || !zhat || !lam || !slack || !dl_dz || (q > 0 && !nu)) return QPX_ERR_ARG;
    if (refine < 0) return QPX_ERR_ARG;
    if (refine > 0 && !qpx_refine_supported(dtype, n, m, q)) return QPX_ERR_UNSUPPORTED;
    if (dtype != QPX_F32) {
        qpx::KktArgs<double> a{};
        a.io32 = dtype == QPX_F32_WIDE;
        a.B = B; a.n = n; a.m = m; a.q = q; a.fac = (double*)factors; a.fac_stride = (size_t)sfac;
        a.zhat = (const double*)zhat; a.lam = (const double*)lam; a.slack = (const double*)slack;
        a.nu = (const double*)nu; a.dl_dz = (const double*)dl_dz;
        a.dQ = (double*)dQ; a.dp = (double*)dp; a.dG = (double*)dG; a.dh = (double*)dh;
        a.dA = (double*)dA; a.db = (double*)db; a.status = status;
        a.dx = (double*)dx; a.dz = (double*)dz; a.dy = (double*)dy;
        a.refine = refine; a.Q = (const double*)Q; a.G = (const double*)G; a.A = (const double*)A; a.sQ = sQ; a.sG = sG; a.sA = sA;
        return qpx::api_kkt<double, true>(a, stream);
    }
    qpx::KktArgs<float> a{};
    a.B = B; a.n = n; a.m = m; a.q = q; a.fac = (float*)factors; a.fac_stride = (size_t)sfac;
    a.zhat = (const float*)zhat; a.lam = (const float*)lam; a.slack = (const float*)slack;
    a.nu = (const float*)nu; a.dl_dz = (const float*)dl_dz;
    a.dQ = (float*)dQ; a.dp = (float*)dp; a.dG = (float*)dG; a.dh = (float*)dh;
    a.dA = (float*)dA; a.db = (float*)db; a.status = status;
    a.dx = (float*)dx; a.dz = (float*)dz; a.dy = (float*)dy;
    a.refine = refine; a.Q = (const float*)Q; a.G = (const float*)G; a.A = (const float*)A; a.sQ = sQ; a.sG = sG; a.sA = sA;
    return qpx::api_kkt<float, true>(a, stream);
}

int qpx_jvp(int dtype, int B, int n, int m, int q, void* factors, int64_t sfac, const void* zhat, const void* lam,
            const void* slack, const void* nu, const void* tQ, int64_t stQ, const void* tp, int64_t stp, const void* tG,
            int64_t stG, const void* th, int64_t sth, const void* tA, int64_t stA, const void* tb, int64_t stb, void* dzhat,
            void* dlam, void* dnu, void* dslack, int refine, const void* Q, int64_t sQ, const void* G, int64_t sG,
            const void* A, int64_t sA, int32_t* status, qpx_stream_t stream)
{
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    if (!factors || !zhat || !lam || !slack || !dzhat || (q > 0 && !nu)) return QPX_ERR_ARG;
    if (refine < 0) return QPX_ERR_ARG;
    if (refine > 0 && !qpx_refine_supported(dtype, n, m, q)) return QPX_ERR_UNSUPPORTED;
    if (dtype != QPX_F32)
        return qpx::api_jvp<double>(dtype == QPX_F32_WIDE, B, n, m, q, factors, sfac, zhat, lam, slack, nu, tQ, stQ, tp, stp, tG, stG,
                                    th, sth, tA, stA, tb, stb, dzhat, dlam, dnu, dslack, refine, Q, sQ, G, sG, A, sA, status, stream);
    return qpx::api_jvp<float>(0, B, n, m, q, factors, sfac, zhat, lam, slack, nu, tQ, stQ, tp, stp, tG, stG, th, sth, tA, stA,
                               tb, stb, dzhat, dlam, dnu, dslack, refine, Q, sQ, G, sG, A, sA, status, stream);
}

int qpx_polish_supported(int dtype, int n, int m, int q)
{
    if (qpx::check_dims(dtype, 1, n, m, q) != QPX_OK) return 0;
    return qpx::polish_served(dtype, n, m, q) ? 1 : 0;
}

int qpx_polish(int dtype, int B, int n, int m, int q, const void* Q, int64_t sQ, const void* p, int64_t sp, const void* G,
               int64_t sG, const void* h, int64_t sh, const void* A, int64_t sA, const void* b, int64_t sb, void* factors,
               int64_t sfac, int steps, int refine, void* zhat, void* nu, void* lam, void* slack, void* best_resid,
               int32_t* status, qpx_stream_t stream)
{
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    if (!Q || !p || !G || !h || !factors || !zhat || !lam || !slack || (q > 0 && (!A || !b || !nu))) return QPX_ERR_ARG;
    if (steps < 0 || refine < 0) return QPX_ERR_ARG;
    if (!qpx::polish_served(dtype, n, m, q)) return QPX_ERR_UNSUPPORTED;
    if (dtype == QPX_F64) {
        qpx::PolishArgs<double> a{};
        a.B = B; a.n = n; a.m = m; a.q = q; a.fac = (double*)factors; a.fac_stride = (size_t)sfac;
        a.Q = (const double*)Q; a.G = (const double*)G; a.A = (const double*)A; a.sQ = sQ; a.sG = sG; a.sA = sA;
        a.p = (const double*)p; a.h = (const double*)h; a.b = (const double*)b; a.sp = sp; a.sh = sh; a.sb = sb;
        a.zhat = (double*)zhat; a.nu = (double*)nu; a.lam = (double*)lam; a.slack = (double*)slack;
        a.steps = steps; a.refine = refine; a.best_resid = (double*)best_resid; a.status = status;
        return qpx::api_polish<double>(a, stream);
    }
    qpx::PolishArgs<float> a{};
    a.B = B; a.n = n; a.m = m; a.q = q; a.fac = (float*)factors; a.fac_stride = (size_t)sfac;
    a.Q = (const float*)Q; a.G = (const float*)G; a.A = (const float*)A; a.sQ = sQ; a.sG = sG; a.sA = sA;
    a.p = (const float*)p; a.h = (const float*)h; a.b = (const float*)b; a.sp = sp; a.sh = sh; a.sb = sb;
    a.zhat = (float*)zhat; a.nu = (float*)nu; a.lam = (float*)lam; a.slack = (float*)slack;
    a.steps = steps; a.refine = refine; a.best_resid = (float*)best_resid; a.status = status;
    return qpx::api_polish<float>(a, stream);
}

int qpx_dense_solve(int dtype, int B, int k, void* M, void* rhs, int32_t* status, qpx_stream_t stream)
{
    if (dtype != QPX_F32 && dtype != QPX_F64) return QPX_ERR_ARG;
    if (B < 1 || k < 1 || !M || !rhs) return QPX_ERR_ARG;
    if (k > qpx::kMaxDim) return QPX_ERR_UNSUPPORTED;
    if (dtype == QPX_F64) {
        qpx::DenseSolveArgs<double> a{B, k, (double*)M, (double*)rhs, status};
        return qpx::launch_dense_solve<double>(a, stream);
    }
    qpx::DenseSolveArgs<float> a{B, k, (float*)M, (float*)rhs, status};
    return qpx::launch_dense_solve<float>(a, stream);
}

size_t qpx_batch_outer_workspace_elems(int dtype, int B, int r, int c)
{
    if ((dtype != QPX_F32 && dtype != QPX_F64) || B < 1 || r < 1 || c < 1) return 0;
    const int tiles = ((r + 15) / 16) * ((c + 15) / 16), chunks = qpx::outer_chunks(B, tiles);
    return chunks > 1 ? (size_t)chunks * tiles * 256 : 0;
}

int qpx_batch_outer(int dtype, int B, int r, int c, const void* u, const void* v, const void* w, const void* x,
                    double scale, void* out, void* ws, size_t ws_elems, qpx_stream_t stream)
{
    if (dtype != QPX_F32 && dtype != QPX_F64) return QPX_ERR_ARG;
    if (B < 1 || r < 1 || c < 1 || !u || !out) return QPX_ERR_ARG;
    if ((!v && c != 1) || (!w) != (!x)) return QPX_ERR_ARG;       // v8: v == NULL = a column of ones; w, x both or neither
    return dtype == QPX_F64 ? qpx::api_batch_outer<double>(B, r, c, u, v, w, x, scale, out, ws, ws_elems, stream)
                            : qpx::api_batch_outer<float>(B, r, c, u, v, w, x, scale, out, ws, ws_elems, stream);
}

}  // extern "C"
