// qpx_kernels.h -- what every kernel family shares: wave-level reductions, the one-wave vector slots, the widening
// loads of QPX_F32_WIDE and the argument blocks of the launches (plain data, passed by value).
//
// (Rounds 1-4 also kept the round-1 WORKGROUP kernels here -- prefactor_body / ipm_body / kkt_body: one 256-thread workgroup
// per QP, packed Cholesky factors and substitutions in LDS or in the blob -- reachable through knob 1 only since the
// large-QP family took every size beyond the thread-grid / tile kernels in round 4 (3-6 x faster there, profiles/archive/r04b).
// Deleted in round 5; libqpx_hip_r04.so, archived beside the product, still holds them for A/Bs.)
#pragma once
#include "qpx_layout.h"
#include "qpx_platform.h"

// Phase timers of the profiling build (-DQPX_PROFILE, scripts/prof_phases.py): thread 0 of every
// workgroup accumulates shader-clock cycles per phase and writes 8 numbers per QP into `trace`.
#ifdef QPX_PROFILE
#define QPX_PROF_INIT long long qpx_prof_t = clock64(); long long qpx_prof_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define QPX_PROF(i) { const long long qpx_prof_n = clock64(); qpx_prof_acc[i] += qpx_prof_n - qpx_prof_t; qpx_prof_t = qpx_prof_n; }
#define QPX_PROF_DUMP(ptr, T) if (b.tid == 0 && (ptr)) { for (int qpx_i = 0; qpx_i < 8; ++qpx_i) (ptr)[qpx_i] = (T)qpx_prof_acc[qpx_i]; }
#else
#define QPX_PROF_INIT
#define QPX_PROF(i)
#define QPX_PROF_DUMP(ptr, T)
#endif

namespace qpx {

template <class T> struct Lim;
template <> struct Lim<float> {
    static QPX_DEV float inf() { return __builtin_huge_valf(); }
    static QPX_DEV float tiny() { return 1.17549435e-38f; }
};
template <> struct Lim<double> {
    static QPX_DEV double inf() { return __builtin_huge_val(); }
    static QPX_DEV double tiny() { return 2.2250738585072014e-308; }
};

// ------------------------------------------------------------------------------------------
// wave-level helpers (every lane of the calling wave takes part)

// Reductions over the 64 lanes; every lane gets the result.  Inside the four 16-lane rows with DPP
// moves, across the rows with four v_readlane broadcasts: ~25 VALU issues and no LDS traffic (the
// ds_bpermute butterfly these replace cost ~600 ticks per reduction on MI355X).
template <class T> QPX_DEV T wave_sum(const Block& b, T v)
{
    v += b.template xor16<1>(v);
    v += b.template xor16<2>(v);
    v += b.template xor16<7>(v);
    v += b.template xor16<15>(v);
    return (b.bcast(v, 0) + b.bcast(v, 16)) + (b.bcast(v, 32) + b.bcast(v, 48));
}
template <class T> QPX_DEV T min2_(T a, T c) { return (c < a) ? c : a; }
template <class T> QPX_DEV T max2_(T a, T c) { return (c > a) ? c : a; }
template <class T> QPX_DEV T wave_min(const Block& b, T v)
{
    v = min2_(v, b.template xor16<1>(v));
    v = min2_(v, b.template xor16<2>(v));
    v = min2_(v, b.template xor16<7>(v));
    v = min2_(v, b.template xor16<15>(v));
    return min2_(min2_(b.bcast(v, 0), b.bcast(v, 16)), min2_(b.bcast(v, 32), b.bcast(v, 48)));
}
template <class T> QPX_DEV T wave_max(const Block& b, T v)
{
    v = max2_(v, b.template xor16<1>(v));
    v = max2_(v, b.template xor16<2>(v));
    v = max2_(v, b.template xor16<7>(v));
    v = max2_(v, b.template xor16<15>(v));
    return max2_(max2_(b.bcast(v, 0), b.bcast(v, 16)), max2_(b.bcast(v, 32), b.bcast(v, 48)));
}

// A vector of length n is held by ONE wave as NS registers per lane: element i lives in
// slot i/64 of lane i%64.
template <int NS, class T> QPX_DEV void ld_slots(const Block& b, T (&x)[NS], const T* src, int n, T fill)
{
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int i = s * kWave + b.lane();
        x[s] = (i < n) ? src[i] : fill;
    }
}

// ------------------------------------------------------------------------------------------
// Arrays at the C boundary of a FLOAT64 kernel may be float32 (QPX_F32_WIDE in include/qpx.h: the caller keeps float32
// tensors, factors and arithmetic are float64; `io32` in the argument blocks below).  In<T> reads, put_ writes such an
// array through its declared pointer type; the branch is wave-uniform and sits outside every inner loop.  The float32
// kernels never set io32.
template <class T> struct In {
    const T* p;
    int f32;
    QPX_DEV In(const T* base, size_t off, int io32) : p(nullptr), f32(sizeof(T) == 8 ? io32 : 0)
    {
        if (base) p = f32 ? reinterpret_cast<const T*>(reinterpret_cast<const float*>(base) + off) : base + off;
    }
    QPX_DEV explicit operator bool() const { return p != nullptr; }
    QPX_DEV T operator[](size_t i) const { return f32 ? (T) reinterpret_cast<const float*>(p)[i] : p[i]; }
};
template <class T> QPX_DEV void put_(T* base, int io32, size_t i, T v)
{
    if (sizeof(T) == 8 && io32) reinterpret_cast<float*>(base)[i] = (float)v;
    else base[i] = v;
}

// ------------------------------------------------------------------------------------------
// Soft rows (qpx_pre_factor_soft): w (m), w_i = 1 / rho_i > 0 on a soft row, 0 on a hard one.  The blob of the
// softened QP is the hard one's with R_ii + w_i on the diagonal of R and the number of soft rows under the root of
// || G^T 1 ||.  soft_rows is the large-QP family's; the thread-grid / tile pre-factorisations call soft_blob at their very
// end, behind a block-uniform `if (a.w)`: by ONE wave, `acc` = || G^T 1 ||^2 as the kernel summed it (handed on in LDS).
template <class T> QPX_DEV T soft_rows(const Block& b, const In<T>& wg, int m)
{
    T cnt = T(0);
    for (int i = b.lane(); i < m; i += kWave) cnt += (wg[i] > T(0)) ? T(1) : T(0);
    return wave_sum(b, cnt);
}
// the diagonal of every image of R the blob holds (rows < m: the padding keeps its diagonal) and the scalar; true in every
// lane where an entry of w is negative or not finite (such an entry adds nothing)
template <class T> QPX_DEV bool soft_blob(const Block& b, const In<T>& wg, int m, T* F, const FacLayout& lay, bool wRg, bool wRw, bool wRm, T acc)
{
    bool bad = false;
    T cnt = T(0);
    for (int i = b.lane(); i < m; i += kWave) {
        const T w = wg[i];
        if (!(w >= T(0)) || !finite_(w)) bad = true;
        else if (w > T(0)) {
            cnt += T(1);
            if (wRg) F[lay.Rg + (size_t)(tri(i >> 4) + (i >> 4)) * 256 + (size_t)(17 * (i & 15))] += w;
            if (wRw) F[lay.Rw + (size_t)(tri(i >> 3) + (i >> 3)) * 64 + (size_t)(9 * (i & 7))] += w;
            if (wRm) F[lay.Rm + tile_image_index(i, i)] += w;
        }
    }
    cnt = wave_sum(b, cnt);
    if (b.lane() == 0) F[lay.scal] = sqrt_(acc + cnt);          // || G'^T 1 ||, G' = [G, -E]
    return b.any(bad);
}

// ------------------------------------------------------------------------------------------
// Which blob QP `qp` reads (IpmArgs / KktArgs::fac_group): its own, or -- scenario batches, DESIGN 4.15 -- the one its group of
// `group` consecutive QPs shares.  qp is the workgroup's index and group a kernel argument: a uniform division, once per launch
QPX_LAYOUT_HD int fac_index(int qp, int group) { return group > 1 ? (int)((unsigned)qp / (unsigned)group) : qp; }

// ------------------------------------------------------------------------------------------
// kernel argument blocks (plain data, passed by value)

template <class T> struct PrefactorArgs {
    int B, n, m, q;
    const T *Q, *G, *A;                   // batch-major, row-major; stride 0 = shared by the batch
    long long sQ, sG, sA;                 // batch strides in elements
    T* fac;
    size_t fac_stride;
    int* status;
    int images;                           // blob family / register images of R (qpx_layout.h: fac_layout)
    int io32 = 0;                         // T = double only: Q, G, A are float32 arrays (QPX_F32_WIDE)
    // matrix-core form (qpx_prefac.h) only: which tiles of K (pf_k) and of R (pf_r) each of the four waves computes, bit
    // t = tile (i, j), t = i (i + 1) / 2 + j -- a greedy balance the host works out once per launch (prefac_deal)
    unsigned pf_k[4] = {0, 0, 0, 0}, pf_r[4] = {0, 0, 0, 0};
    // soft rows (qpx_pre_factor_soft): w (B,m), float32 under io32, batch stride sw (0 = shared); NULL = qpx_pre_factor
    const T* w = nullptr;
    long long sw = 0;
};

template <class T> struct IpmArgs {
    int B, n, m, q;
    const T *p, *h, *b;                   // (B,n) (B,m) (B,q); stride 0 = shared by the batch
    long long sp, sh, sb;
    T* fac;
    size_t fac_stride;
    T eps;
    int maxIter, notImprovedLim, stall_policy;
    T *zhat, *nu, *lam, *slack;           // (B,n) (B,q) (B,m) (B,m)
    int *iters, *status;
    T* best_resid;
    T* trace;                             // optional [maxIter][B][3]: pri_resid, dual_resid, mu
    int images;                           // blob family the factors were written in (fac_layout)
    int io32 = 0;                         // T = double only: every array but `fac` is float32 (QPX_F32_WIDE)
    // warm start (qpx_ipm_warm; thread-grid / tile kernels only): lam0, s0 (B,m) dense, float32 under io32; NULL = the
    // reference's start point.  A QP whose 2 m entries are all finite enters the loop at z = max(lam0, warm_floor),
    // s = max(s0, warm_floor), pass 0; any other QP starts cold.  warm_used (B), optional: 1 / 0 per QP
    const T *lam0 = nullptr, *s0 = nullptr;
    T warm_floor = T(0);
    int* warm_used = nullptr;
    // two-sided rows (qpx_ipm_range; the forms of kIpmRangeRole only): lower (B,m), batch stride slo (0 = shared), -inf = a
    // one-sided row; gt1 (B) = || G^T e ||, e_i = 1 on the one-sided rows, NULL = 0; lam_lo, slack_lo (B,m): the lower side's
    // multipliers and slacks beside lam, slack (0 and +inf on a one-sided row)
    const T* lower = nullptr;
    long long slo = 0;
    const T* gt1 = nullptr;
    T *lam_lo = nullptr, *slack_lo = nullptr;
    // elastic rows (qpx_ipm_elastic; the forms of kIpmElasticRole only): gamma, rho (B,m), batch strides sgamma, srho (0 = shared),
    // +inf in either = a hard row; gt1 above (B) = sqrt(|| G^T 1 ||^2 + 4 k), k elastic rows; lam_lo, slack_lo above: the
    // multipliers and slacks of t >= 0 (0 and +inf on a hard row); tviol (B,m): t
    const T *gamma = nullptr, *rho = nullptr;
    long long sgamma = 0, srho = 0;
    T* tviol = nullptr;
    // soft two-sided rows (qpx_ipm_soft_range; the forms of kIpmSoftRangeRole only): lower, gamma, rho above (the upper side's
    // penalty), gamma_lo, rho_lo (B,m) the lower side's, batch strides sgamma_lo, srho_lo; lam_lo, slack_lo above: the lower
    // rows'; lam_t, slack_t, tviol / lam_tl, slack_tl, tviol_lo (B,m): multipliers, slacks and values of tu >= 0 / tl >= 0
    const T *gamma_lo = nullptr, *rho_lo = nullptr;
    long long sgamma_lo = 0, srho_lo = 0;
    T *lam_t = nullptr, *slack_t = nullptr, *lam_tl = nullptr, *slack_tl = nullptr, *tviol_lo = nullptr;
    // warm start of the range role (qpx_ipm_range_warm): the lower side's lam0_lo, s0_lo (B,m) dense beside lam0, s0 above.  A
    // QP is warm if lam0, s0 are finite on every row and lam0_lo, s0_lo on every row that is two-sided in THIS call (the
    // entries of a one-sided row are never read: a previous solve left 0 and +inf there); any other QP starts cold
    const T *lam0_lo = nullptr, *s0_lo = nullptr;
    // scenario batches (qpx_ipm_group): QP `qp` reads blob qp / fac_group -- fac_group consecutive QPs share one
    // factorisation; 0 or 1 = one blob per QP (or, with fac_stride 0, one for the batch).  Everything else stays per QP
    int fac_group = 0;
};

template <class T> struct KktArgs {
    int B, n, m, q;
    T* fac;
    size_t fac_stride;
    // general solve_kkt (batch.py:349-372): d (B,m), rx (B,n), rs, rz (B,m), ry (B,q); NULL = zeros
    const T *d, *rx, *rs, *rz, *ry;
    T *dx, *ds, *dz, *dy;
    // backward (qp.py:127-182): d is built from lam/slack, rx = dl_dz
    const T *zhat, *lam, *slack, *nu, *dl_dz;
    T *dQ, *dp, *dG, *dh, *dA, *db;       // backward: any of them may be NULL (gradient not wanted)
    int* status;
    int images;                           // blob family the factors were written in (fac_layout)
    // iterative refinement on the residual of the original KKT system (batch.py:244-270): steps, and the caller's
    // Q (B,n,n), G (B,m,n), A (B,q,n) with their batch strides; refine = 0 or Q = NULL: none
    int refine;
    const T *Q, *G, *A;
    long long sQ, sG, sA;
    int io32 = 0;                         // T = double only: every array but `fac` is float32 (QPX_F32_WIDE; refine = 0)
    // forward mode (qpx_jvp, kBackward = false only): d from lam / slack as in the backward, the right-hand side formed from
    // the tangents at (zhat, lam, nu) -- rx = 1/2 (tQ + tQ^T) zhat + tp + tG^T lam + tA^T nu, rs = 0, rz = tG zhat - th,
    // ry = tA zhat - tb --; outputs dx = dzhat, dz = dlam, ds = dslack, dy = dnu (any but dx may be NULL); d, rx .. ry unused
    int jvp = 0;
    const T *tQ = nullptr, *tp = nullptr, *tG = nullptr, *th = nullptr, *tA = nullptr, *tb = nullptr;   // NULL = zero
    long long stQ = 0, stp = 0, stG = 0, sth = 0, stA = 0, stb = 0;        // batch strides in elements (0 = shared)
    // backward with cotangents on the multipliers (qpx_backward_duals): rz = dl_dlam (B,m), ry = dl_dnu (B,q) beside
    // rx = dl_dz; NULL = zeros (and then dl_dz may be NULL too); rs stays zero
    const T *dl_dlam = nullptr, *dl_dnu = nullptr;
    // the multi-right-hand-side role (qpx_factor_solve_kkt_multi, kkt_multi_role): K > 0 right-hand sides per QP -- rx, rs, rz,
    // ry and dx, ds, dz, dy are (B, K, .), a QP's K vectors contiguous; one d (B, m) and one factorisation for all of them
    int K = 0;
    // the backward of two-sided rows (qpx_backward_range; the forms of kKktRangeRole only): the lower side's multipliers and
    // slacks (B,m) -- d = clamp(lam)/clamp(slack) + clamp(lam_lo)/clamp(slack_lo), lam - lam_lo in the outer products
    const T *lam_lo = nullptr, *slack_lo = nullptr;
    // scenario batches (qpx_backward_group): blob index = qp / fac_group, as IpmArgs::fac_group (kkt_mat_role only)
    int fac_group = 0;
};

// The finishing stage (qpx_polish, include/qpx.h): iterations of the reference's loop in the ORIGINAL variables
// (batch.py:92-198) on the residuals of the caller's data, started from a given iterate, best iterate kept
template <class T> struct PolishArgs {
    int B, n, m, q;
    T* fac;
    size_t fac_stride;
    int images;
    const T *Q, *G, *A;                   // the caller's problem data (B,n,n) (B,m,n) (B,q,n); stride 0 = shared
    long long sQ, sG, sA;
    const T *p, *h, *b;                   // (B,n) (B,m) (B,q)
    long long sp, sh, sb;
    T *zhat, *nu, *lam, *slack;           // in: the iterate to start from; out: the best iterate met
    int steps, refine;
    T* best_resid;                        // out, may be NULL: the reference's residual of the returned iterate (batch.py:103-107)
    int* status;
    // the centring role (qpx_centre, polish_centre_role; kPolishCentreRole forms only): kappa (B,m), batch stride skappa
    // (0 = shared); `steps` is max_steps, best_resid the stop test's residual of the returned iterate; steps_out (B), may be NULL
    const T* kappa = nullptr;
    long long skappa = 0;
    double tol = 0.0;
    int* steps_out = nullptr;
};

constexpr size_t kMaxLdsBytes = 160 * 1024;   // gfx950: 160 KiB of LDS per workgroup

QPX_LAYOUT_HD size_t max2(size_t a, size_t b) { return a > b ? a : b; }

// ------------------------------------------------------------------------------------------
// step length to the boundary for one QP (get_step, batch.py:210-213, as it behaves for a batch of one): min over blocking
// entries of -v/dv, or 1 when nothing blocks -- from the reciprocals rv = 1/v the caller already holds: the minimum of -v/dv
// is the reciprocal of the maximum of -dv/v, so the per-entry divisions become multiplications and
// one division remains (f64 division is a ~15-instruction sequence on gfx950).
template <int NS, class T>
QPX_DEV T step_to_boundary_rcp(const Block& b, const T (&rv)[NS], const T (&dv)[NS], int m)
{
    T t = T(0);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int i = s * kWave + b.lane();
        if (i < m && dv[s] < T(0)) t = max2_(t, -dv[s] * rv[s]);
    }
    t = wave_max(b, t);
    return (t > T(0)) ? T(1) / t : T(1);
}

}  // namespace qpx
