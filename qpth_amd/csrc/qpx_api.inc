// qpx_api.inc -- the C ABI of include/qpx.h: argument checks, the decision functions (which kernel family, which
// form of it, how much LDS) and the dispatch to the launchers.  Included once by qpx_hip_api.hip, which sees
//
//   launch_sweep / launch_prefac_tile / launch_ipm_grid / launch_ipm_tile / launch_kkt_* / launch_polish_* / launch_big_* ...
//   (declared in qpx_launch.h, defined in qpx_hip_kernels.hip), and  size_t lds_budget_bytes();   // LDS a workgroup may use (160 KiB on gfx950)
//
// (the host-thread emulator of the test tree includes it the same way with its own launchers).  The forms of a family
// that exist are listed once, in qpx_forms.h: every dispatch below is one expansion of such a list, `if the chosen
// values are this form's, launch it`, and says in place what happens when no form matches.  The large-QP family's
// launch sequences live in qpx_big_host.inc.
#include "qpx_forms.h"

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
    // (r6) One wave per QP now keeps eight workgroups on a CU instead of four at four tile rows (20.4 KB of LDS each:
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
// The finishing stage on tiles (api_polish) has two forms per size at most, the one-wave form and the chain-wave form, and
// its own rule between them: NOT tile_chain(nbt, tile_waves(nbt, B)).  It ignores the A/B knob, and at four tile rows it
// still switches to one wave beyond 8192 QPs, where tile_waves moved to 512 in round 6 (the finishing stage was not
// measured again then).
inline bool polish_tile_chain(int nbt, int B) { return nbt == 7 || (nbt == 4 && B <= 8192); }

// The large-QP family (qpx_big.h: batched multi-kernel Cholesky / GEMM path): every size beyond the thread-grid / tile
// kernels (round 4; measured on MI355X against the round-1 workgroup kernels it replaced there, f64 step times,
// profiles/archive/r04b: B=512 n=m=150 5.6 vs 20.2 ms, B=512 n=m=120 neq=30 3.3 vs 8.8, B=128 n=m=190 3.1 vs 18.7), or forced by knob 3.
inline bool use_big(int n, int m, int q, size_t elem_bytes)
{
    (void)elem_bytes;
    return g_ipm_variant == 3 || !use_grid(n, m, q);
}

// Blob family of a solve (qpx_layout.h: fac_layout): 0 = workgroup kernels (Cholesky factors), else the
// register images of R the thread-grid / tile consumers load: f64 with the tile kernels -> the tile image
// only (loop and backward both use it); otherwise the 16x16 grid image and the 8x8 one the loop switches
// to on a full chip.  Depends on (dtype, n, m, q) and the per-thread knob only, never on B: a shared blob
// is built with B = 1 and consumed with the batch's B.
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

#include "qpx_big_host.inc"

template <class T>
int api_pre_factor(int B, int n, int m, int q, const void* Q, int64_t sQ, const void* G, int64_t sG,
                   const void* A, int64_t sA, void* factors, int32_t* status, void* stream, int io32 = 0,
                   const void* w = nullptr, int64_t sw = 0)
{
    if (!Q || !G || !factors || !status || (q > 0 && !A)) return QPX_ERR_ARG;
    PrefactorArgs<T> a;
    a.io32 = io32;
    a.w = (const T*)w; a.sw = sw;                // soft rows (qpx_pre_factor_soft); NULL: none
    a.B = B; a.n = n; a.m = m; a.q = q;
    a.Q = (const T*)Q; a.G = (const T*)G; a.A = (const T*)A;
    a.sQ = sQ; a.sG = sG; a.sA = sA;
    a.images = blob_images<T>(n, m, q);
    if (a.images == 8) {
        const size_t fs = big_layout(n, m, q).total;
        return big_split(B, stream, true, [&](int q0, int cnt, void* st, int part, int nparts) {
            return big_pre_factor<T>(cnt, n, m, q, advio(a.Q, (size_t)q0 * sQ, io32), sQ, advio(a.G, (size_t)q0 * sG, io32), sG,
                                     advio(a.A, (size_t)q0 * sA, io32), sA, (T*)factors + (size_t)q0 * fs, status + q0, st, io32,
                                     advio(a.w, (size_t)q0 * sw, io32), sw);
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
#define QPX_PICK(NBN, EQ) if (nbn == NBN && (q > 0) == EQ) return a.w ? launch_prefac_tile<NBN + kPrefacSoft, EQ>(a, pb, stream) : launch_prefac_tile<NBN, EQ>(a, pb, stream);
            QPX_FORMS_PREFAC_TILE(QPX_PICK)         // (prefac_tile_serves: one of them matches)
#undef QPX_PICK
        }
    }
    if (use_grid(n, m, q)) {
        const int nba = sweep_nb(n + q + m);
        const size_t gb = lds_elems_sweep(nba) * sizeof(T);
#define QPX_PICK(NBL) if (nba == NBL) return a.w ? launch_sweep<T, NBL + kPrefacSoft>(a, gb, stream) : launch_sweep<T, NBL>(a, gb, stream);
        QPX_FORMS_SWEEP(QPX_PICK)
#undef QPX_PICK
    }
    return QPX_ERR_UNSUPPORTED;
}

// the fields every loop entry point fills in the same way (api_ipm, qpx_ipm_range, qpx_ipm_elastic)
template <class T>
void ipm_common_args(IpmArgs<T>& a, int B, int n, int m, int q, const void* p, int64_t sp, const void* h, int64_t sh, const void* bb,
                     int64_t sb, void* factors, int64_t sfac, double eps, int maxIter, int notImprovedLim, int stall_policy,
                     void* zhat, void* nu, void* lam, void* slack, int32_t* iters, int32_t* status, void* best_resid, void* trace)
{
    a.B = B; a.n = n; a.m = m; a.q = q;
    a.p = (const T*)p; a.h = (const T*)h; a.b = (const T*)bb;
    a.sp = sp; a.sh = sh; a.sb = sb;
    a.fac = (T*)factors; a.fac_stride = (size_t)sfac;
    a.eps = (T)eps; a.maxIter = maxIter; a.notImprovedLim = notImprovedLim; a.stall_policy = stall_policy;
    a.zhat = (T*)zhat; a.nu = (T*)nu; a.lam = (T*)lam; a.slack = (T*)slack;
    a.iters = iters; a.status = status; a.best_resid = (T*)best_resid; a.trace = (T*)trace;
}

template <class T>
int api_ipm(int B, int n, int m, int q, const void* p, int64_t sp, const void* h, int64_t sh,
            const void* bb, int64_t sb, void* factors, int64_t sfac, double eps, int maxIter, int notImprovedLim,
            int stall_policy, void* zhat, void* nu, void* lam, void* slack, int32_t* iters,
            int32_t* status, void* best_resid, void* trace, void* stream, int io32 = 0,
            const void* lam0 = nullptr, const void* s0 = nullptr, double warm_floor = 0, int32_t* warm_used = nullptr,
            int fac_group = 0, bool launch = true)
{
    // (launch = false: the decision only -- QPX_OK where a form serves B QPs of this size under the calling thread's knob;
    // fac_group: IpmArgs::fac_group, scenario batches -- qpx_ipm_group)
    if (launch && (!p || !h || !factors || !zhat || !lam || !slack || !iters || !status || !best_resid ||
        (q > 0 && (!nu || !bb))))
        return QPX_ERR_ARG;
    if (maxIter < 0 || stall_policy < 0 || stall_policy > 2) return QPX_ERR_ARG;
    if ((lam0 == nullptr) != (s0 == nullptr)) return QPX_ERR_ARG;
    IpmArgs<T> a;
    a.io32 = io32;
    ipm_common_args(a, B, n, m, q, p, sp, h, sh, bb, sb, factors, sfac, eps, maxIter, notImprovedLim, stall_policy, zhat, nu, lam, slack, iters, status,
                    best_resid, trace);
    a.lam0 = (const T*)lam0; a.s0 = (const T*)s0; a.warm_floor = (T)warm_floor; a.warm_used = lam0 ? warm_used : nullptr;
    a.fac_group = fac_group;
    a.images = blob_images<T>(n, m, q);
    if (a.images == 8) {
        if (fac_group > 1 || !launch) return QPX_ERR_UNSUPPORTED;      // per-QP work matrices live in the blob: no groups (qpx_group_supported)
        if (lam0) return QPX_ERR_UNSUPPORTED;             // the large-QP family's start point is a launch sequence of its own: no warm entry (qpx_warm_supported)
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
#define QPX_PICK(NBL, NS) if (nb8 == NBL && ns8 == NS) return launch ? launch_ipm_grid8<T, NBL, NS>(a, wb, stream) : QPX_OK;
            QPX_FORMS_IPM_GRID8(QPX_PICK)           // no such form: on to the tiles / the 16x16 grid
#undef QPX_PICK
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
#define QPX_PICK(NBL, NW, NS, CH) if (nbt == NBL && nw == NW && nst == NS && ch == CH) return launch ? launch_ipm_tile<NBL, NW, NS, CH>(a, tb, stream) : QPX_OK;
                QPX_FORMS_IPM_TILE(QPX_PICK)        // no such form: on to the 16x16 grid
#undef QPX_PICK
            }
        }
        const int nbg = grid_nb(m);
        const int nsg = slots_for(n, 16 * nbg, q);
        const size_t gb = lds_elems_ipm_grid(16, nbg, n, q) * sizeof(T);
#define QPX_PICK(NBL, NS) if (nbg == NBL && nsg == NS) return launch ? launch_ipm_grid<T, NBL, NS>(a, gb, stream) : QPX_OK;
        QPX_FORMS_IPM_GRID(QPX_PICK)
#undef QPX_PICK
        return QPX_ERR_UNSUPPORTED;
    }
    return QPX_ERR_UNSUPPORTED;
}

// kRole: 0 the KKT solve, 1 the backward, 2 the solve for a.K right-hand sides per QP (qpx_forms.h: kKktMultiRole) -- the
// third role of the form the first two run in, so all three follow one rule for which form serves a size
// (launch = false: the decision only -- QPX_OK where a form serves a.B QPs of this size under the calling thread's knob)
template <class T, int kRole>
int api_kkt(KktArgs<T>& a, void* stream, bool launch = true)
{
    constexpr bool kBw = kRole == 1;
    constexpr int kForm = kRole == 2 ? kKktMultiRole : 0;
    const int n = a.n, m = a.m, q = a.q;
    a.images = blob_images<T>(n, m, q);
    if constexpr (kRole == 2) {
        if (a.images == 8) return QPX_ERR_UNSUPPORTED;       // the large-QP family has no such kernels: K calls of the single solve
    } else if (a.images == 8) {
        if (a.fac_group > 1 || !launch) return QPX_ERR_UNSUPPORTED;      // (as api_ipm: no groups in the large-QP family)
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
            s.dl_dz = advio(a.dl_dz, o * n, w); s.dl_dlam = advio(a.dl_dlam, o * m, w); s.dl_dnu = advio(a.dl_dnu, o * q, w);
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
                const size_t tb = (kRole == 2 ? lds_elems_kkt_multi_tile(nbt, nw, n, q, ch) : lds_elems_kkt_tile(nbt, nw, n, q, ch)) * sizeof(T);
#define QPX_PICK(NBL, NW, CH) if (nbt == NBL && nw == NW && ch == CH) return launch ? launch_kkt_tile<kForm + NBL, NW, kBw, CH>(a, tb, stream) : QPX_OK;
                QPX_FORMS_KKT_TILE(QPX_PICK)        // no such form: on to the 16x16 grid
#undef QPX_PICK
            }
        }
        const int nbg = grid_nb(m);
        const size_t gb = (kRole == 2 ? lds_elems_kkt_multi_grid(16, nbg, n, q) : lds_elems_kkt_grid(16, nbg, n, q)) * sizeof(T);
#define QPX_PICK(NBL) if (nbg == NBL) return launch ? launch_kkt_grid<T, kForm + NBL, kBw>(a, gb, stream) : QPX_OK;
        QPX_FORMS_KKT_GRID(QPX_PICK)
#undef QPX_PICK
        return QPX_ERR_UNSUPPORTED;
    }
    return QPX_ERR_UNSUPPORTED;
}

template <class T>
int api_factor_solve_kkt(int io32, int B, int n, int m, int q, void* factors, int64_t sfac, const void* d, const void* rx,
                         const void* rs, const void* rz, const void* ry, void* dx, void* ds, void* dz, void* dy, int refine,
                         const void* Q, int64_t sQ, const void* G, int64_t sG, const void* A, int64_t sA, int32_t* status, void* stream)
{
    KktArgs<T> a{};
    a.io32 = io32;
    a.B = B; a.n = n; a.m = m; a.q = q; a.fac = (T*)factors; a.fac_stride = (size_t)sfac;
    a.d = (const T*)d; a.rx = (const T*)rx; a.rs = (const T*)rs; a.rz = (const T*)rz; a.ry = (const T*)ry;
    a.dx = (T*)dx; a.ds = (T*)ds; a.dz = (T*)dz; a.dy = (T*)dy;
    a.status = status;
    a.refine = refine; a.Q = (const T*)Q; a.G = (const T*)G; a.A = (const T*)A; a.sQ = sQ; a.sG = sG; a.sA = sA;
    return api_kkt<T, 0>(a, stream);
}

template <class T>
int api_factor_solve_kkt_multi(int io32, int B, int n, int m, int q, int K, void* factors, int64_t sfac, const void* d, const void* rx,
                               const void* rs, const void* rz, const void* ry, void* dx, void* ds, void* dz, void* dy,
                               int32_t* status, void* stream)
{
    // K = 1 IS the single solve (include/qpx.h says it computes what qpx_factor_solve_kkt computes): the same kernel, so the same
    // bits -- the multi role's block of kKktMultiRB accumulators adds in another order (up to 4e-12 of the solution apart,
    // tests/kkt_checks.py) and would carry three zero vectors.  The role-0 body skips a NULL ds, dz, dy as the multi role does.
    if (K == 1)
        return api_factor_solve_kkt<T>(io32, B, n, m, q, factors, sfac, d, rx, rs, rz, q > 0 ? ry : nullptr, dx, ds, dz, dy, 0,
                                       nullptr, 0, nullptr, 0, nullptr, 0, status, stream);
    KktArgs<T> a{};
    a.io32 = io32;
    a.B = B; a.n = n; a.m = m; a.q = q; a.K = K; a.fac = (T*)factors; a.fac_stride = (size_t)sfac;
    a.d = (const T*)d; a.rx = (const T*)rx; a.rs = (const T*)rs; a.rz = (const T*)rz; a.ry = q > 0 ? (const T*)ry : nullptr;
    a.dx = (T*)dx; a.ds = (T*)ds; a.dz = (T*)dz; a.dy = (T*)dy;
    a.status = status;
    return api_kkt<T, 2>(a, stream);
}

template <class T>
int api_backward(int io32, int B, int n, int m, int q, void* factors, int64_t sfac, const void* zhat, const void* lam,
                 const void* slack, const void* nu, const void* dl_dz, const void* dl_dlam, const void* dl_dnu, void* dQ, void* dp,
                 void* dG, void* dh, void* dA, void* db, void* dx, void* dz, void* dy, int refine, const void* Q, int64_t sQ, const void* G, int64_t sG, const void* A,
                 int64_t sA, int32_t* status, void* stream, int fac_group = 0)
{
    KktArgs<T> a{};
    a.io32 = io32;
    a.B = B; a.n = n; a.m = m; a.q = q; a.fac = (T*)factors; a.fac_stride = (size_t)sfac;
    a.fac_group = fac_group;              // scenario batches (qpx_backward_group); else 0
    a.zhat = (const T*)zhat; a.lam = (const T*)lam; a.slack = (const T*)slack; a.nu = (const T*)nu; a.dl_dz = (const T*)dl_dz;
    a.dl_dlam = (const T*)dl_dlam; a.dl_dnu = q > 0 ? (const T*)dl_dnu : nullptr;
    a.dQ = (T*)dQ; a.dp = (T*)dp; a.dG = (T*)dG; a.dh = (T*)dh; a.dA = (T*)dA; a.db = (T*)db; a.status = status;
    a.dx = (T*)dx; a.dz = (T*)dz; a.dy = (T*)dy;
    a.refine = refine; a.Q = (const T*)Q; a.G = (const T*)G; a.A = (const T*)A; a.sQ = sQ; a.sG = sG; a.sA = sA;
    return api_kkt<T, 1>(a, stream);
}

// forward mode: the KKT solve of the backward (same d, same kernels: api_kkt<T, 0>) with the right-hand side formed from
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
    return api_kkt<T, 0>(a, stream);
}

// The second-order pass of the backward (qpx_backward2): the fourth role of the KKT forms (qpx_forms.h: kKktB2Role), in float64
// arithmetic.  Which form serves a size follows api_kkt's rule; a form without the role -- the two-wave tile forms, reachable
// through the A/B knob alone -- declines, it never falls through to a kernel that reads another image of the blob.
inline bool b2_tile_form(int nbt, int nw, bool ch)
{
#define QPX_PICK(NBL, NW, CH) if (nbt == NBL && nw == NW && ch == CH) return true;
    QPX_FORMS_KKT_B2_TILE(QPX_PICK)
#undef QPX_PICK
    return false;
}
// (B: the batch the tile forms' waves per QP depend on; every default choice has the role, so only the knob matters)
inline bool b2_served(int dtype, int n, int m, int q, int B)
{
    if (dtype == QPX_F32 || !use_grid(n, m, q) || n > 4 * kWave) return false;
    const int nbt = tile_nb(m);
    if ((g_grid_size == 0 || g_grid_size == 1) && nbt > 0) {
        const int nw = tile_waves(nbt, B);
        return b2_tile_form(nbt, nw, tile_chain(nbt, nw));
    }
    return grid_nb(m) > 0;
}
inline int api_backward2(KktArgs<double>& a, void* stream)
{
    const int n = a.n, m = a.m, q = a.q;
    a.images = blob_images<double>(n, m, q);
    const int nbt = tile_nb(m);
    if ((g_grid_size == 0 || g_grid_size == 1) && nbt > 0) {
        const int nw = tile_waves(nbt, a.B);
        const bool ch = tile_chain(nbt, nw);
        const size_t tb = lds_elems_kkt_b2_tile(nbt, nw, n, q, ch) * sizeof(double);
        if (tb > lds_budget_bytes()) return QPX_ERR_UNSUPPORTED;
#define QPX_PICK(NBL, NW, CH) if (nbt == NBL && nw == NW && ch == CH) return launch_kkt_tile<kKktB2Role + NBL, NW, false, CH>(a, tb, stream);
        QPX_FORMS_KKT_B2_TILE(QPX_PICK)
#undef QPX_PICK
        return QPX_ERR_UNSUPPORTED;
    }
    const int nbg = grid_nb(m);
    const size_t gb = lds_elems_kkt_b2_grid(16, nbg, n, q) * sizeof(double);
    if (gb > lds_budget_bytes()) return QPX_ERR_UNSUPPORTED;
#define QPX_PICK(NBL) if (nbg == NBL) return launch_kkt_grid<double, kKktB2Role + NBL, false>(a, gb, stream);
    QPX_FORMS_KKT_GRID(QPX_PICK)
#undef QPX_PICK
    return QPX_ERR_UNSUPPORTED;
}

// Two-sided rows (qpx_ipm_range, qpx_backward_range; DESIGN 4.11): the range role of the loop forms (qpx_forms.h: kIpmRangeRole)
// and of the backward (kKktRangeRole), float64 arithmetic.  Which form serves a size follows api_ipm's / api_kkt's rule for
// float64; a form without the role -- the two-wave tile forms and the small thread-grid forms, reachable through the A/B knob
// alone -- declines, it never falls through to a kernel that reads another image of the blob.  launch = false: the decision only.
// (kRoleBase: kIpmRangeRole, kIpmElasticRole or kIpmSoftRangeRole; kRole: the role's index in the LDS sizes, 1, 2 or 3 -- as
// ipm_loop_role's)
template <int kRoleBase, int kRole>
int api_ipm_role(IpmArgs<double>& a, void* stream, bool launch)
{
    const int n = a.n, m = a.m, q = a.q;
    if (!use_grid(n, m, q)) return QPX_ERR_UNSUPPORTED;            // the large-QP family has no such role
    a.images = blob_images<double>(n, m, q);
    if (a.images == 4) {
        const int nbt = tile_nb(m);
        const int nst = slots_for(n, 16 * nbt, q);
        const int nw = tile_waves(nbt, a.B);
        const bool ch = tile_chain(nbt, nw);
        const size_t tb = lds_elems_ipm_tile(nbt, nw, n, q, ch, kRole) * sizeof(double);
        if (tb > lds_budget_bytes()) return QPX_ERR_UNSUPPORTED;
#define QPX_PICK(NBL, NW, NS, CH) \
        if (nbt == NBL && nw == NW && nst == NS && ch == CH) return launch ? launch_ipm_tile<NBL + kRoleBase, NW, NS, CH>(a, tb, stream) : QPX_OK;
        QPX_FORMS_IPM_RANGE_TILE(QPX_PICK)
#undef QPX_PICK
        return QPX_ERR_UNSUPPORTED;
    }
    const int nbg = grid_nb(m);
    const int nsg = slots_for(n, 16 * nbg, q);
    const size_t gb = lds_elems_ipm_grid(16, nbg, n, q, kRole) * sizeof(double);
    if (gb > lds_budget_bytes()) return QPX_ERR_UNSUPPORTED;
#define QPX_PICK(NBL, NS) if (nbg == NBL && nsg == NS) return launch ? launch_ipm_grid<double, NBL + kRoleBase, NS>(a, gb, stream) : QPX_OK;
    QPX_FORMS_IPM_RANGE_GRID(QPX_PICK)
#undef QPX_PICK
    return QPX_ERR_UNSUPPORTED;
}
inline int api_ipm_range(IpmArgs<double>& a, void* stream, bool launch) { return api_ipm_role<kIpmRangeRole, 1>(a, stream, launch); }
inline int api_backward_range(KktArgs<double>& a, void* stream, bool launch)
{
    const int n = a.n, m = a.m, q = a.q;
    if (!use_grid(n, m, q)) return QPX_ERR_UNSUPPORTED;
    a.images = blob_images<double>(n, m, q);
    if (a.images == 4) {
        const int nbt = tile_nb(m);
        const int nw = tile_waves(nbt, a.B);
        const bool ch = tile_chain(nbt, nw);
        const size_t tb = lds_elems_kkt_tile(nbt, nw, n, q, ch) * sizeof(double);
#define QPX_PICK(NBL, NW, CH) if (nbt == NBL && nw == NW && ch == CH) return launch ? launch_kkt_tile<kKktRangeRole + NBL, NW, true, CH>(a, tb, stream) : QPX_OK;
        QPX_FORMS_KKT_RANGE_TILE(QPX_PICK)
#undef QPX_PICK
        return QPX_ERR_UNSUPPORTED;
    }
    const int nbg = grid_nb(m);
    const size_t gb = lds_elems_kkt_grid(16, nbg, n, q) * sizeof(double);
#define QPX_PICK(NBL) if (nbg == NBL) return launch ? launch_kkt_grid<double, kKktRangeRole + NBL, true>(a, gb, stream) : QPX_OK;
    QPX_FORMS_KKT_GRID(QPX_PICK)
#undef QPX_PICK
    return QPX_ERR_UNSUPPORTED;
}
// (B: the batch the tile forms' waves per QP depend on)
inline bool range_served(int dtype, int n, int m, int q, int B)
{
    if (dtype != QPX_F64) return false;
    IpmArgs<double> ia{};
    ia.B = B; ia.n = n; ia.m = m; ia.q = q;
    KktArgs<double> ka{};
    ka.B = B; ka.n = n; ka.m = m; ka.q = q;
    return api_ipm_range(ia, nullptr, false) == QPX_OK && api_backward_range(ka, nullptr, false) == QPX_OK;
}

// Elastic rows (qpx_ipm_elastic; DESIGN 4.12): the elastic role of the same loop forms (qpx_forms.h: kIpmElasticRole), picked by
// api_ipm_range's rule; the backward runs on the hard factors as it stands.  A form without the role declines.
inline int api_ipm_elastic(IpmArgs<double>& a, void* stream, bool launch) { return api_ipm_role<kIpmElasticRole, 2>(a, stream, launch); }
// (B: the batch the tile forms' waves per QP depend on)
inline bool elastic_served(int dtype, int n, int m, int q, int B)
{
    if (dtype != QPX_F64) return false;
    IpmArgs<double> ia{};
    ia.B = B; ia.n = n; ia.m = m; ia.q = q;
    return api_ipm_elastic(ia, nullptr, false) == QPX_OK;
}

// Soft two-sided rows (qpx_ipm_soft_range; DESIGN 4.13): the soft-range role of the same loop forms (kIpmSoftRangeRole), picked
// by api_ipm_range's rule; the backward is the range role's (api_backward_range) with effective slacks.  A form without the role
// declines, and so does one whose 49 vectors do not fit the LDS budget.
inline int api_ipm_soft_range(IpmArgs<double>& a, void* stream, bool launch) { return api_ipm_role<kIpmSoftRangeRole, 3>(a, stream, launch); }
// (B: the batch the tile forms' waves per QP depend on)
inline bool soft_range_served(int dtype, int n, int m, int q, int B)
{
    if (dtype != QPX_F64) return false;
    IpmArgs<double> ia{};
    ia.B = B; ia.n = n; ia.m = m; ia.q = q;
    KktArgs<double> ka{};
    ka.B = B; ka.n = n; ka.m = m; ka.q = q;
    return api_ipm_soft_range(ia, nullptr, false) == QPX_OK && api_backward_range(ka, nullptr, false) == QPX_OK;
}

// the finishing stage: every family has it (thread-grid / tile kernels: one kernel, the blob's register image of R decides the
// form; large-QP family: qpx_big_polish.h)
inline bool polish_served(int dtype, int n, int m, int q)
{
    const int d = n > m ? (n > q ? n : q) : (m > q ? m : q);
    return dtype != QPX_F32_WIDE && d <= kMaxDimPolish && (use_grid(n, m, q) || use_big(n, m, q, dtype != QPX_F32 ? 8 : 4));
}
template <class T>
int api_polish(int B, int n, int m, int q, const void* Q, int64_t sQ, const void* p, int64_t sp, const void* G, int64_t sG,
               const void* h, int64_t sh, const void* A, int64_t sA, const void* b, int64_t sb, void* factors, int64_t sfac,
               int steps, int refine, void* zhat, void* nu, void* lam, void* slack, void* best_resid, int32_t* status, void* stream)
{
    PolishArgs<T> a{};
    a.B = B; a.n = n; a.m = m; a.q = q; a.fac = (T*)factors; a.fac_stride = (size_t)sfac;
    a.Q = (const T*)Q; a.G = (const T*)G; a.A = (const T*)A; a.sQ = sQ; a.sG = sG; a.sA = sA;
    a.p = (const T*)p; a.h = (const T*)h; a.b = (const T*)b; a.sp = sp; a.sh = sh; a.sb = sb;
    a.zhat = (T*)zhat; a.nu = (T*)nu; a.lam = (T*)lam; a.slack = (T*)slack;
    a.steps = steps; a.refine = refine; a.best_resid = (T*)best_resid; a.status = status;
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
            const int nbt = tile_nb(m);
            const bool ch = polish_tile_chain(nbt, a.B);
            const size_t tb = lds_elems_polish_mat(16 * (size_t)nbt, tile_scratch_elems(nbt, ch ? 3 : 1, ch), n, q, sizeof(T)) * sizeof(T);
#define QPX_PICK(NBL, NW, CH) if (nbt == NBL && ch == CH) return launch_polish_tile<NBL, NW, CH>(a, tb, stream);
            QPX_FORMS_POLISH_TILE(QPX_PICK)         // (the waves follow from the form: one, or the chain-wave form's four)
#undef QPX_PICK
            return QPX_ERR_UNSUPPORTED;              // (the tile image has no thread-grid form)
        }
    }
    const int nbg = grid_nb(m);
    const size_t gb = lds_elems_polish_grid(16, nbg, n, q, sizeof(T)) * sizeof(T);
#define QPX_PICK(NBL) if (nbg == NBL) return launch_polish_grid<T, NBL>(a, gb, stream);
    QPX_FORMS_POLISH_GRID(QPX_PICK)
#undef QPX_PICK
    return QPX_ERR_UNSUPPORTED;
}

// Centring (qpx_centre): the centring role of the one-kernel finishing stage's forms (qpx_forms.h: kPolishCentreRole), float64
// arithmetic.  Which form serves a size is api_polish's rule; the large-QP family and the float32 kernels have no such role.
inline bool centre_served(int dtype, int n, int m, int q)
{
    if (dtype != QPX_F64 || !use_grid(n, m, q)) return false;
    const int images = blob_images<double>(n, m, q);
    if (images == 4) {                       // (a small and a large batch cover both choices of polish_tile_chain)
        const int nbt = tile_nb(m);
        return lds_elems_centre_tile(nbt, n, q, polish_tile_chain(nbt, 1)) * sizeof(double) <= lds_budget_bytes() &&
               lds_elems_centre_tile(nbt, n, q, polish_tile_chain(nbt, 1 << 20)) * sizeof(double) <= lds_budget_bytes();
    }
    return images == 3 && grid_nb(m) > 0 && lds_elems_centre_grid(16, grid_nb(m), n, q) * sizeof(double) <= lds_budget_bytes();
}
inline int api_centre(PolishArgs<double>& a, void* stream)
{
    const int n = a.n, m = a.m, q = a.q;
    a.images = blob_images<double>(n, m, q);
    if (a.images == 4) {
        const int nbt = tile_nb(m);
        const bool ch = polish_tile_chain(nbt, a.B);
        const size_t tb = lds_elems_centre_tile(nbt, n, q, ch) * sizeof(double);
        if (tb > lds_budget_bytes()) return QPX_ERR_UNSUPPORTED;
#define QPX_PICK(NBL, NW, CH) if (nbt == NBL && ch == CH) return launch_polish_tile<NBL + kPolishCentreRole, NW, CH>(a, tb, stream);
        QPX_FORMS_POLISH_TILE(QPX_PICK)
#undef QPX_PICK
        return QPX_ERR_UNSUPPORTED;
    }
    if (a.images != 3) return QPX_ERR_UNSUPPORTED;
    const int nbg = grid_nb(m);
    const size_t gb = lds_elems_centre_grid(16, nbg, n, q) * sizeof(double);
    if (gb > lds_budget_bytes()) return QPX_ERR_UNSUPPORTED;
#define QPX_PICK(NBL) if (nbg == NBL) return launch_polish_grid<double, NBL + kPolishCentreRole>(a, gb, stream);
    QPX_FORMS_POLISH_GRID(QPX_PICK)
#undef QPX_PICK
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

// Scenario batches (DESIGN 4.15): K consecutive QPs per factorisation.  Served where the blob is only read -- the thread-grid /
// tile families, qpx_can_share_factors -- and a loop form and a backward form exist for the size under the calling thread's
// knob (every default choice does; a small and a large batch cover both choices of the rules that depend on B).
template <class T> inline bool group_served_t(int n, int m, int q, int io32)
{
    for (const int B : {1, 1 << 20}) {
        if (api_ipm<T>(B, n, m, q, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, 0.0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr, nullptr, io32, nullptr, nullptr, 0, nullptr, 0, false) != QPX_OK)
            return false;
        KktArgs<T> ka{};
        ka.B = B; ka.n = n; ka.m = m; ka.q = q; ka.io32 = io32;
        if (api_kkt<T, 1>(ka, nullptr, false) != QPX_OK) return false;
    }
    return true;
}
inline bool group_served(int dtype, int n, int m, int q)
{
    if (check_dims(dtype, 1, n, m, q) != QPX_OK || use_big(n, m, q, dtype != QPX_F32 ? 8 : 4)) return false;
    return dtype != QPX_F32 ? group_served_t<double>(n, m, q, dtype == QPX_F32_WIDE) : group_served_t<float>(n, m, q, 0);
}

// out (B, r, c), out[g] = scale ( U_g^T V_g + W_g^T X_g ) over group g's K consecutive rows: the grouped mode of the batch
// contraction (qpx_reduce.h), a slab of groups per pair of launches
template <class T>
int api_group_outer(int B, int K, int r, int c, const void* u, const void* v, const void* w, const void* x, double scale,
                    void* out, void* ws, size_t ws_elems, void* stream)
{
    const int tiles = ((r + 15) / 16) * ((c + 15) / 16), slab = group_slab(B, tiles);
    if (slab > 1 && (!ws || ws_elems < (size_t)slab * tiles * 256)) return QPX_ERR_ARG;
    for (int g0 = 0; g0 < B; g0 += slab) {
        const int cnt = B - g0 < slab ? B - g0 : slab;
        const size_t row0 = (size_t)g0 * K;
        OuterArgs<T> a;
        a.B = cnt * K; a.r = r; a.c = c;
        a.u = (const T*)u + row0 * r; a.v = v ? (const T*)v + row0 * c : nullptr;
        a.w = w ? (const T*)w + row0 * r : nullptr; a.x = w ? (const T*)x + row0 * c : nullptr;
        a.scale = (T)scale; a.out = (T*)out + (size_t)g0 * r * c;
        a.grouped = 1; a.chunks = cnt; a.chunk_len = K;
        a.ws = cnt > 1 ? (T*)ws : nullptr;
        if (const int e = launch_batch_outer<T>(a, tiles, stream)) return e;
    }
    return QPX_OK;
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

int qpx_pre_factor_soft(int dtype, int B, int n, int m, int q, const void* Q, int64_t sQ, const void* G,
                        int64_t sG, const void* A, int64_t sA, const void* w, int64_t sw, void* factors,
                        int32_t* status, qpx_stream_t stream)
{
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    if (sw < 0) return QPX_ERR_ARG;
    return dtype != QPX_F32
               ? qpx::api_pre_factor<double>(B, n, m, q, Q, sQ, G, sG, A, sA, factors, status, stream, dtype == QPX_F32_WIDE, w, sw)
               : qpx::api_pre_factor<float>(B, n, m, q, Q, sQ, G, sG, A, sA, factors, status, stream, 0, w, sw);
}

int qpx_pre_factor(int dtype, int B, int n, int m, int q, const void* Q, int64_t sQ, const void* G,
                   int64_t sG, const void* A, int64_t sA, void* factors, int32_t* status,
                   qpx_stream_t stream)
{
    return qpx_pre_factor_soft(dtype, B, n, m, q, Q, sQ, G, sG, A, sA, nullptr, 0, factors, status, stream);
}

int qpx_warm_supported(int dtype, int n, int m, int q)
{
    // the thread-grid / tile loop kernels take a warm start (IpmArgs::lam0, s0), in all three dtypes
    if (qpx::check_dims(dtype, 1, n, m, q) != QPX_OK) return 0;
    return qpx::use_grid(n, m, q) ? 1 : 0;
}

int qpx_ipm_warm(int dtype, int B, int n, int m, int q, const void* p, int64_t sp, const void* h,
                 int64_t sh, const void* b, int64_t sb, void* factors, int64_t sfac, double eps, int maxIter,
                 int notImprovedLim, int stall_policy, void* zhat, void* nu, void* lam, void* slack,
                 int32_t* iters, int32_t* status, void* best_resid, void* trace,
                 const void* lam0, const void* s0, double warm_floor, int32_t* warm_used, qpx_stream_t stream)
{
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    if (!(warm_floor > 0) || !(warm_floor < __builtin_huge_val())) return QPX_ERR_ARG;      // NaN, Inf, <= 0
    return dtype != QPX_F32
               ? qpx::api_ipm<double>(B, n, m, q, p, sp, h, sh, b, sb, factors, sfac, eps, maxIter, notImprovedLim, stall_policy, zhat, nu, lam, slack, iters, status, best_resid, trace, stream, dtype == QPX_F32_WIDE,
                                      lam0, s0, warm_floor, warm_used)
               : qpx::api_ipm<float>(B, n, m, q, p, sp, h, sh, b, sb, factors, sfac, eps, maxIter, notImprovedLim, stall_policy, zhat, nu, lam, slack, iters, status, best_resid, trace, stream, 0,
                                     lam0, s0, warm_floor, warm_used);
}

int qpx_ipm(int dtype, int B, int n, int m, int q, const void* p, int64_t sp, const void* h,
            int64_t sh, const void* b, int64_t sb, void* factors, int64_t sfac, double eps, int maxIter,
            int notImprovedLim, int stall_policy, void* zhat, void* nu, void* lam, void* slack,
            int32_t* iters, int32_t* status, void* best_resid, void* trace, qpx_stream_t stream)
{
    return qpx_ipm_warm(dtype, B, n, m, q, p, sp, h, sh, b, sb, factors, sfac, eps, maxIter, notImprovedLim, stall_policy, zhat, nu, lam, slack,
                        iters, status, best_resid, trace, nullptr, nullptr, 1e-2, nullptr, stream);
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
    if (dtype != QPX_F32)
        return qpx::api_factor_solve_kkt<double>(dtype == QPX_F32_WIDE, B, n, m, q, factors, sfac, d, rx, rs, rz, ry, dx, ds, dz, dy, refine,
                                                 Q, sQ, G, sG, A, sA, status, stream);
    return qpx::api_factor_solve_kkt<float>(0, B, n, m, q, factors, sfac, d, rx, rs, rz, ry, dx, ds, dz, dy, refine, Q, sQ, G, sG, A, sA, status, stream);
}

int qpx_multi_supported(int dtype, int n, int m, int q)
{
    // the thread-grid / tile KKT kernels have the multi-right-hand-side role (qpx_grid.h: kkt_multi_role), in all three dtypes
    if (qpx::check_dims(dtype, 1, n, m, q) != QPX_OK) return 0;
    return qpx::use_grid(n, m, q) ? 1 : 0;
}

int qpx_factor_solve_kkt_multi(int dtype, int B, int n, int m, int q, int K, void* factors, int64_t sfac, const void* d,
                               const void* rx, const void* rs, const void* rz, const void* ry, void* dx, void* ds, void* dz,
                               void* dy, int32_t* status, qpx_stream_t stream)
{
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    if (K < 1 || !factors || !d || !dx) return QPX_ERR_ARG;
    if (!rx && !rs && !rz && !(q > 0 && ry)) return QPX_ERR_ARG;          // no right-hand side at all
    if (!qpx_multi_supported(dtype, n, m, q)) return QPX_ERR_UNSUPPORTED;
    if (dtype != QPX_F32)
        return qpx::api_factor_solve_kkt_multi<double>(dtype == QPX_F32_WIDE, B, n, m, q, K, factors, sfac, d, rx, rs, rz, ry, dx, ds, dz,
                                                       dy, status, stream);
    return qpx::api_factor_solve_kkt_multi<float>(0, B, n, m, q, K, factors, sfac, d, rx, rs, rz, ry, dx, ds, dz, dy, status, stream);
}

int qpx_backward(int dtype, int B, int n, int m, int q, void* factors, int64_t sfac, const void* zhat,
                 const void* lam, const void* slack, const void* nu, const void* dl_dz, void* dQ,
                 void* dp, void* dG, void* dh, void* dA, void* db, void* dx, void* dz, void* dy,
                 int refine, const void* Q, int64_t sQ, const void* G, int64_t sG, const void* A, int64_t sA,
                 int32_t* status, qpx_stream_t stream)
{
    // (dl_dz is required here; checked behind the sizes, as it always was)
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    if (!dl_dz) return QPX_ERR_ARG;
    return qpx_backward_duals(dtype, B, n, m, q, factors, sfac, zhat, lam, slack, nu, dl_dz, nullptr, nullptr, dQ, dp, dG, dh, dA, db,
                              dx, dz, dy, refine, Q, sQ, G, sG, A, sA, status, stream);
}

int qpx_backward_duals(int dtype, int B, int n, int m, int q, void* factors, int64_t sfac, const void* zhat,
                       const void* lam, const void* slack, const void* nu, const void* dl_dz, const void* dl_dlam,
                       const void* dl_dnu, void* dQ, void* dp, void* dG, void* dh, void* dA, void* db, void* dx, void* dz,
                       void* dy, int refine, const void* Q, int64_t sQ, const void* G, int64_t sG, const void* A, int64_t sA,
                       int32_t* status, qpx_stream_t stream)
{
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    if (!factors || !zhat || !lam || !slack || (q > 0 && !nu)) return QPX_ERR_ARG;
    if (!dl_dz && !dl_dlam && !(q > 0 && dl_dnu)) return QPX_ERR_ARG;       // no cotangent at all
    if (refine < 0) return QPX_ERR_ARG;
    if (refine > 0 && !qpx_refine_supported(dtype, n, m, q)) return QPX_ERR_UNSUPPORTED;
    if (dtype != QPX_F32)
        return qpx::api_backward<double>(dtype == QPX_F32_WIDE, B, n, m, q, factors, sfac, zhat, lam, slack, nu, dl_dz, dl_dlam, dl_dnu,
                                         dQ, dp, dG, dh, dA, db, dx, dz, dy, refine, Q, sQ, G, sG, A, sA, status, stream);
    return qpx::api_backward<float>(0, B, n, m, q, factors, sfac, zhat, lam, slack, nu, dl_dz, dl_dlam, dl_dnu, dQ, dp, dG, dh, dA, db,
                                    dx, dz, dy, refine, Q, sQ, G, sG, A, sA, status, stream);
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

int qpx_backward2_supported(int dtype, int n, int m, int q)
{
    if (qpx::check_dims(dtype, 1, n, m, q) != QPX_OK) return 0;
    // (the forms the default dispatch picks have the role at every batch size: a small and a large batch cover both of its choices)
    return qpx::b2_served(dtype, n, m, q, 1) && qpx::b2_served(dtype, n, m, q, 1 << 20) ? 1 : 0;
}

int qpx_backward2(int dtype, int B, int n, int m, int q, void* factors, int64_t sfac, const void* zhat, const void* lam,
                  const void* slack, const void* nu, const void* dx, const void* dz, const void* dy,
                  const void* W_Q, int64_t sWQ, const void* W_p, int64_t sWp, const void* W_G, int64_t sWG,
                  const void* W_h, int64_t sWh, const void* W_A, int64_t sWA, const void* W_b, int64_t sWb,
                  void* zdot, void* lamdot, void* nudot, void* HQ, void* Hp, void* HG, void* Hh, void* HA, void* Hb,
                  int32_t* status, qpx_stream_t stream)
{
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    if (!factors || !zhat || !lam || !slack || !dx || !dz || !zdot || (q > 0 && (!nu || !dy))) return QPX_ERR_ARG;
    if (sWQ < 0 || sWp < 0 || sWG < 0 || sWh < 0 || sWA < 0 || sWb < 0) return QPX_ERR_ARG;
    if (!qpx::b2_served(dtype, n, m, q, B)) return QPX_ERR_UNSUPPORTED;
    qpx::KktArgs<double> a{};
    a.io32 = dtype == QPX_F32_WIDE;
    a.B = B; a.n = n; a.m = m; a.q = q; a.fac = (double*)factors; a.fac_stride = (size_t)sfac;
    a.zhat = (const double*)zhat; a.lam = (const double*)lam; a.slack = (const double*)slack; a.nu = (const double*)nu;
    a.rx = (const double*)dx; a.rz = (const double*)dz; a.ry = q > 0 ? (const double*)dy : nullptr;      // the first backward's KKT solution
    a.jvp = 1;
    a.tQ = (const double*)W_Q; a.tp = (const double*)W_p; a.tG = (const double*)W_G; a.th = (const double*)W_h;
    a.tA = q > 0 ? (const double*)W_A : nullptr; a.tb = q > 0 ? (const double*)W_b : nullptr;
    a.stQ = sWQ; a.stp = sWp; a.stG = sWG; a.sth = sWh; a.stA = sWA; a.stb = sWb;
    a.dx = (double*)zdot; a.dz = (double*)lamdot; a.dy = q > 0 ? (double*)nudot : nullptr;
    a.dQ = (double*)HQ; a.dp = (double*)Hp; a.dG = (double*)HG; a.dh = (double*)Hh;
    a.dA = q > 0 ? (double*)HA : nullptr; a.db = q > 0 ? (double*)Hb : nullptr;
    a.status = status;
    return qpx::api_backward2(a, stream);
}

int qpx_range_supported(int dtype, int n, int m, int q)
{
    if (qpx::check_dims(dtype, 1, n, m, q) != QPX_OK) return 0;
    // (a small and a large batch cover both choices of the tile forms' waves per QP)
    return qpx::range_served(dtype, n, m, q, 1) && qpx::range_served(dtype, n, m, q, 1 << 20) ? 1 : 0;
}

int qpx_range_warm_supported(int dtype, int n, int m, int q)
{
    // every form with the range role has the role's warm entry (IpmArgs::lam0, s0, lam0_lo, s0_lo)
    return qpx_range_supported(dtype, n, m, q);
}

int qpx_ipm_range_warm(int dtype, int B, int n, int m, int q, const void* p, int64_t sp, const void* h, int64_t sh,
                       const void* b, int64_t sb, void* factors, int64_t sfac, double eps, int maxIter, int notImprovedLim,
                       int stall_policy, void* zhat, void* nu, void* lam, void* slack, int32_t* iters, int32_t* status,
                       void* best_resid, void* trace, const void* lower, int64_t slo, const void* gt1, void* lam_lo,
                       void* slack_lo, const void* lam0, const void* s0, const void* lam0_lo, const void* s0_lo,
                       double warm_floor, int32_t* warm_used, qpx_stream_t stream)
{
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    if (!p || !h || !lower || !factors || !zhat || !lam || !slack || !lam_lo || !slack_lo || !iters || !status || !best_resid ||
        (q > 0 && (!nu || !b)))
        return QPX_ERR_ARG;
    if (maxIter < 0 || stall_policy < 0 || stall_policy > 2 || slo < 0) return QPX_ERR_ARG;
    const int given = (lam0 != nullptr) + (s0 != nullptr) + (lam0_lo != nullptr) + (s0_lo != nullptr);
    if (given != 0 && given != 4) return QPX_ERR_ARG;
    if (!(warm_floor > 0) || !(warm_floor < __builtin_huge_val())) return QPX_ERR_ARG;      // NaN, Inf, <= 0 (as qpx_ipm_warm)
    if (!qpx::range_served(dtype, n, m, q, B)) return QPX_ERR_UNSUPPORTED;
    qpx::IpmArgs<double> a{};
    qpx::ipm_common_args(a, B, n, m, q, p, sp, h, sh, b, sb, factors, sfac, eps, maxIter, notImprovedLim, stall_policy, zhat, nu, lam, slack, iters,
                         status, best_resid, trace);
    a.lower = (const double*)lower; a.slo = slo; a.gt1 = (const double*)gt1;
    a.lam_lo = (double*)lam_lo; a.slack_lo = (double*)slack_lo;
    if (given) {
        a.lam0 = (const double*)lam0; a.s0 = (const double*)s0; a.lam0_lo = (const double*)lam0_lo; a.s0_lo = (const double*)s0_lo;
        a.warm_floor = warm_floor; a.warm_used = warm_used;
    }
    return qpx::api_ipm_range(a, stream, true);
}

int qpx_ipm_range(int dtype, int B, int n, int m, int q, const void* p, int64_t sp, const void* h, int64_t sh,
                  const void* b, int64_t sb, void* factors, int64_t sfac, double eps, int maxIter, int notImprovedLim,
                  int stall_policy, void* zhat, void* nu, void* lam, void* slack, int32_t* iters, int32_t* status,
                  void* best_resid, void* trace, const void* lower, int64_t slo, const void* gt1, void* lam_lo,
                  void* slack_lo, qpx_stream_t stream)
{
    return qpx_ipm_range_warm(dtype, B, n, m, q, p, sp, h, sh, b, sb, factors, sfac, eps, maxIter, notImprovedLim, stall_policy, zhat, nu, lam,
                              slack, iters, status, best_resid, trace, lower, slo, gt1, lam_lo, slack_lo, nullptr, nullptr, nullptr, nullptr, 1e-2,
                              nullptr, stream);
}

int qpx_backward_range(int dtype, int B, int n, int m, int q, void* factors, int64_t sfac, const void* zhat, const void* lam,
                       const void* slack, const void* nu, const void* dl_dz, void* dQ, void* dp, void* dG, void* dh, void* dA,
                       void* db, void* dx, void* dz, void* dy, int refine, const void* Q, int64_t sQ, const void* G, int64_t sG,
                       const void* A, int64_t sA, int32_t* status, const void* lam_lo, const void* slack_lo, qpx_stream_t stream)
{
    (void)Q; (void)sQ; (void)G; (void)sG; (void)A; (void)sA;        // (qpx_backward's refinement data: refine > 0 is not served)
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    if (!factors || !zhat || !lam || !slack || !lam_lo || !slack_lo || !dl_dz || (q > 0 && !nu)) return QPX_ERR_ARG;
    if (refine < 0) return QPX_ERR_ARG;
    if (refine > 0 || !qpx::range_served(dtype, n, m, q, B)) return QPX_ERR_UNSUPPORTED;
    qpx::KktArgs<double> a{};
    a.B = B; a.n = n; a.m = m; a.q = q; a.fac = (double*)factors; a.fac_stride = (size_t)sfac;
    a.zhat = (const double*)zhat; a.lam = (const double*)lam; a.slack = (const double*)slack; a.nu = (const double*)nu;
    a.lam_lo = (const double*)lam_lo; a.slack_lo = (const double*)slack_lo;
    a.dl_dz = (const double*)dl_dz;
    a.dQ = (double*)dQ; a.dp = (double*)dp; a.dG = (double*)dG; a.dh = (double*)dh; a.dA = (double*)dA; a.db = (double*)db;
    a.dx = (double*)dx; a.dz = (double*)dz; a.dy = (double*)dy;
    a.status = status;
    return qpx::api_backward_range(a, stream, true);
}

int qpx_elastic_supported(int dtype, int n, int m, int q)
{
    if (qpx::check_dims(dtype, 1, n, m, q) != QPX_OK) return 0;
    // (a small and a large batch cover both choices of the tile forms' waves per QP)
    return qpx::elastic_served(dtype, n, m, q, 1) && qpx::elastic_served(dtype, n, m, q, 1 << 20) ? 1 : 0;
}

int qpx_ipm_elastic(int dtype, int B, int n, int m, int q, const void* p, int64_t sp, const void* h, int64_t sh,
                    const void* b, int64_t sb, void* factors, int64_t sfac, double eps, int maxIter, int notImprovedLim,
                    int stall_policy, void* zhat, void* nu, void* lam, void* slack, int32_t* iters, int32_t* status,
                    void* best_resid, void* trace, const void* gamma, int64_t sgamma, const void* rho, int64_t srho,
                    const void* gt1, void* lam_t, void* slack_t, void* t, qpx_stream_t stream)
{
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    if (!p || !h || !gamma || !rho || !gt1 || !factors || !zhat || !lam || !slack || !lam_t || !slack_t || !t || !iters || !status ||
        !best_resid || (q > 0 && (!nu || !b)))
        return QPX_ERR_ARG;
    if (maxIter < 0 || stall_policy < 0 || stall_policy > 2 || sgamma < 0 || srho < 0) return QPX_ERR_ARG;
    if (!qpx::elastic_served(dtype, n, m, q, B)) return QPX_ERR_UNSUPPORTED;
    qpx::IpmArgs<double> a{};
    qpx::ipm_common_args(a, B, n, m, q, p, sp, h, sh, b, sb, factors, sfac, eps, maxIter, notImprovedLim, stall_policy, zhat, nu, lam, slack, iters,
                         status, best_resid, trace);
    a.gamma = (const double*)gamma; a.sgamma = sgamma; a.rho = (const double*)rho; a.srho = srho; a.gt1 = (const double*)gt1;
    a.lam_lo = (double*)lam_t; a.slack_lo = (double*)slack_t; a.tviol = (double*)t;
    return qpx::api_ipm_elastic(a, stream, true);
}

int qpx_soft_range_supported(int dtype, int n, int m, int q)
{
    if (qpx::check_dims(dtype, 1, n, m, q) != QPX_OK) return 0;
    // (a small and a large batch cover both choices of the tile forms' waves per QP)
    return qpx::soft_range_served(dtype, n, m, q, 1) && qpx::soft_range_served(dtype, n, m, q, 1 << 20) ? 1 : 0;
}

int qpx_ipm_soft_range(int dtype, int B, int n, int m, int q, const void* p, int64_t sp, const void* h, int64_t sh,
                       const void* b, int64_t sb, void* factors, int64_t sfac, double eps, int maxIter, int notImprovedLim,
                       int stall_policy, void* zhat, void* nu, void* lam, void* slack, int32_t* iters, int32_t* status,
                       void* best_resid, void* trace, const void* lower, int64_t slo, const void* gamma_u, int64_t sgamma_u,
                       const void* rho_u, int64_t srho_u, const void* gamma_l, int64_t sgamma_l, const void* rho_l,
                       int64_t srho_l, const void* gt1, void* lam_lo, void* slack_lo, void* lam_t, void* slack_t, void* lam_tl,
                       void* slack_tl, void* t, void* t_lo, qpx_stream_t stream)
{
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    if (!p || !h || !lower || !gamma_u || !rho_u || !gamma_l || !rho_l || !gt1 || !factors || !zhat || !lam || !slack || !lam_lo ||
        !slack_lo || !lam_t || !slack_t || !lam_tl || !slack_tl || !t || !t_lo || !iters || !status || !best_resid ||
        (q > 0 && (!nu || !b)))
        return QPX_ERR_ARG;
    if (maxIter < 0 || stall_policy < 0 || stall_policy > 2 || slo < 0 || sgamma_u < 0 || srho_u < 0 || sgamma_l < 0 || srho_l < 0)
        return QPX_ERR_ARG;
    if (!qpx::soft_range_served(dtype, n, m, q, B)) return QPX_ERR_UNSUPPORTED;
    qpx::IpmArgs<double> a{};
    qpx::ipm_common_args(a, B, n, m, q, p, sp, h, sh, b, sb, factors, sfac, eps, maxIter, notImprovedLim, stall_policy, zhat, nu, lam, slack, iters,
                         status, best_resid, trace);
    a.lower = (const double*)lower; a.slo = slo; a.gt1 = (const double*)gt1;
    a.gamma = (const double*)gamma_u; a.sgamma = sgamma_u; a.rho = (const double*)rho_u; a.srho = srho_u;
    a.gamma_lo = (const double*)gamma_l; a.sgamma_lo = sgamma_l; a.rho_lo = (const double*)rho_l; a.srho_lo = srho_l;
    a.lam_lo = (double*)lam_lo; a.slack_lo = (double*)slack_lo;
    a.lam_t = (double*)lam_t; a.slack_t = (double*)slack_t; a.lam_tl = (double*)lam_tl; a.slack_tl = (double*)slack_tl;
    a.tviol = (double*)t; a.tviol_lo = (double*)t_lo;
    return qpx::api_ipm_soft_range(a, stream, true);
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
    return dtype == QPX_F64
               ? qpx::api_polish<double>(B, n, m, q, Q, sQ, p, sp, G, sG, h, sh, A, sA, b, sb, factors, sfac, steps, refine, zhat, nu, lam, slack, best_resid, status, stream)
               : qpx::api_polish<float>(B, n, m, q, Q, sQ, p, sp, G, sG, h, sh, A, sA, b, sb, factors, sfac, steps, refine, zhat, nu, lam, slack, best_resid, status, stream);
}

int qpx_centre_supported(int dtype, int n, int m, int q)
{
    if (qpx::check_dims(dtype, 1, n, m, q) != QPX_OK) return 0;
    return qpx::centre_served(dtype, n, m, q) ? 1 : 0;
}

int qpx_centre(int dtype, int B, int n, int m, int q, const void* Q, int64_t sQ, const void* p, int64_t sp, const void* G,
               int64_t sG, const void* h, int64_t sh, const void* A, int64_t sA, const void* b, int64_t sb, void* factors,
               int64_t sfac, const void* kappa, int64_t skappa, double tol, int max_steps, void* zhat, void* nu, void* lam,
               void* slack, void* resid, int32_t* steps, int32_t* status, qpx_stream_t stream)
{
    const int e = qpx::check_dims(dtype, B, n, m, q);
    if (e) return e;
    if (!Q || !p || !G || !h || !factors || !zhat || !lam || !slack || (q > 0 && (!A || !b || !nu))) return QPX_ERR_ARG;
    if (!kappa || skappa < 0 || !(tol > 0.0) || max_steps < 1) return QPX_ERR_ARG;
    if (!qpx::centre_served(dtype, n, m, q)) return QPX_ERR_UNSUPPORTED;
    qpx::PolishArgs<double> a{};
    a.B = B; a.n = n; a.m = m; a.q = q; a.fac = (double*)factors; a.fac_stride = (size_t)sfac;
    a.Q = (const double*)Q; a.G = (const double*)G; a.A = (const double*)A; a.sQ = sQ; a.sG = sG; a.sA = sA;
    a.p = (const double*)p; a.h = (const double*)h; a.b = (const double*)b; a.sp = sp; a.sh = sh; a.sb = sb;
    a.zhat = (double*)zhat; a.nu = (double*)nu; a.lam = (double*)lam; a.slack = (double*)slack;
    a.steps = max_steps; a.refine = 0; a.best_resid = (double*)resid; a.status = status;
    a.kappa = (const double*)kappa; a.skappa = skappa; a.tol = tol; a.steps_out = steps;
    return qpx::api_centre(a, stream);
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

/* ---- scenario batches (DESIGN 4.15): B groups of K consecutive QPs, one factor blob per group ---- */

int qpx_group_supported(int dtype, int n, int m, int q) { return qpx::group_served(dtype, n, m, q) ? 1 : 0; }

int qpx_ipm_group(int dtype, int B, int K, int n, int m, int q, const void* p, int64_t sp, const void* h, int64_t sh,
                  const void* b, int64_t sb, void* factors, int64_t sfac, double eps, int maxIter, int notImprovedLim,
                  int stall_policy, void* zhat, void* nu, void* lam, void* slack, int32_t* iters, int32_t* status,
                  void* best_resid, void* trace, qpx_stream_t stream)
{
    if (K < 1 || B < 1 || (int64_t)B * K > 0x7fffffff) return QPX_ERR_ARG;
    const int e = qpx::check_dims(dtype, B * K, n, m, q);
    if (e) return e;
    if (!p || !h || !factors || !zhat || !lam || !slack || !iters || !status || !best_resid || (q > 0 && (!nu || !b))) return QPX_ERR_ARG;
    if (!qpx::group_served(dtype, n, m, q)) return QPX_ERR_UNSUPPORTED;
    return dtype != QPX_F32
               ? qpx::api_ipm<double>(B * K, n, m, q, p, sp, h, sh, b, sb, factors, sfac, eps, maxIter, notImprovedLim, stall_policy, zhat, nu, lam, slack, iters, status, best_resid, trace, stream, dtype == QPX_F32_WIDE,
                                      nullptr, nullptr, 0, nullptr, K)
               : qpx::api_ipm<float>(B * K, n, m, q, p, sp, h, sh, b, sb, factors, sfac, eps, maxIter, notImprovedLim, stall_policy, zhat, nu, lam, slack, iters, status, best_resid, trace, stream, 0,
                                     nullptr, nullptr, 1e-2, nullptr, K);
}

int qpx_backward_group(int dtype, int B, int K, int n, int m, int q, void* factors, int64_t sfac, const void* zhat,
                       const void* lam, const void* slack, const void* nu, const void* dl_dz, const void* dl_dlam,
                       const void* dl_dnu, void* dQ, void* dp, void* dG, void* dh, void* dA, void* db, void* dx, void* dz,
                       void* dy, int refine, const void* Q, int64_t sQ, const void* G, int64_t sG, const void* A, int64_t sA,
                       int32_t* status, qpx_stream_t stream)
{
    if (K < 1 || B < 1 || (int64_t)B * K > 0x7fffffff) return QPX_ERR_ARG;
    const int e = qpx::check_dims(dtype, B * K, n, m, q);
    if (e) return e;
    if (!factors || !zhat || !lam || !slack || (q > 0 && !nu)) return QPX_ERR_ARG;
    if (!dl_dz && !dl_dlam && !(q > 0 && dl_dnu)) return QPX_ERR_ARG;       // no cotangent at all
    if (dQ || dG || dA) return QPX_ERR_ARG;       // a group's matrix gradients are sums over its K QPs: dx, dz, dy and qpx_group_outer
    if (refine < 0) return QPX_ERR_ARG;
    if (refine > 0 || !qpx::group_served(dtype, n, m, q)) return QPX_ERR_UNSUPPORTED;
    (void)Q; (void)sQ; (void)G; (void)sG; (void)A; (void)sA;      // (refinement's data: refine is 0)
    if (dtype != QPX_F32)
        return qpx::api_backward<double>(dtype == QPX_F32_WIDE, B * K, n, m, q, factors, sfac, zhat, lam, slack, nu, dl_dz, dl_dlam, dl_dnu,
                                         nullptr, dp, nullptr, dh, nullptr, db, dx, dz, dy, 0, nullptr, 0, nullptr, 0, nullptr, 0, status, stream, K);
    return qpx::api_backward<float>(0, B * K, n, m, q, factors, sfac, zhat, lam, slack, nu, dl_dz, dl_dlam, dl_dnu, nullptr, dp, nullptr, dh,
                                    nullptr, db, dx, dz, dy, 0, nullptr, 0, nullptr, 0, nullptr, 0, status, stream, K);
}

size_t qpx_group_outer_workspace_elems(int dtype, int B, int K, int r, int c)
{
    if ((dtype != QPX_F32 && dtype != QPX_F64) || B < 1 || K < 1 || r < 1 || c < 1) return 0;
    const int tiles = ((r + 15) / 16) * ((c + 15) / 16), slab = qpx::group_slab(B, tiles);
    return slab > 1 ? (size_t)slab * tiles * 256 : 0;
}

int qpx_group_outer(int dtype, int B, int K, int r, int c, const void* u, const void* v, const void* w, const void* x,
                    double scale, void* out, void* ws, size_t ws_elems, qpx_stream_t stream)
{
    if (dtype != QPX_F32 && dtype != QPX_F64) return QPX_ERR_ARG;
    if (B < 1 || K < 1 || (int64_t)B * K > 0x7fffffff || r < 1 || c < 1 || !u || !out) return QPX_ERR_ARG;
    if ((!v && c != 1) || (!w) != (!x)) return QPX_ERR_ARG;       // as qpx_batch_outer
    return dtype == QPX_F64 ? qpx::api_group_outer<double>(B, K, r, c, u, v, w, x, scale, out, ws, ws_elems, stream)
                            : qpx::api_group_outer<float>(B, K, r, c, u, v, w, x, scale, out, ws, ws_elems, stream);
}

}  // extern "C"
