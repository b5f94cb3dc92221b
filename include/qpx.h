/*
 * qpx.h -- C ABI of libqpx_hip.so: the MI355X (gfx950) implementation of the one hot path of
 * locuslab/qpth, the dense batched primal-dual interior-point QP solver and its backward pass.
 *
 *     z* = argmin_z 1/2 z'Qz + p'z   s.t.  Gz <= h,  Az = b        (qpth/qp.py:32-42)
 *
 * Every entry point replaces one solver entry point of the reference (the seam that
 * qpth/qp.py:92-96,148-155 calls through):
 *
 *   qpx_pre_factor ........ qpth/solvers/pdipm/batch.py:375-429   pre_factor_kkt(Q, G, A)
 *   qpx_ipm ............... qpth/solvers/pdipm/batch.py:47-207    forward(Q,p,G,h,A,b,Q_LU,S_LU,R,...)
 *   qpx_forward ........... qpth/qp.py:92-96                       pre_factor_kkt + forward
 *   qpx_factor_solve_kkt .. qpth/solvers/pdipm/batch.py:435-470 + 349-372
 *                                                                  factor_kkt(S_LU,R,d); solve_kkt(...)
 *   qpx_backward .......... qpth/qp.py:127-182                     QPFunctionFn.backward (per-QP grads)
 *   qpx_backward_duals .... (no reference counterpart)            the same for a loss of (zhat, lam, nu): cotangents on the multipliers
 *   qpx_jvp ............... (no reference counterpart)            QPFunctionFn.jvp: forward mode, the adjoint of qpx_backward(_duals)
 *   qpx_ipm_warm .......... (no reference counterpart)            qpx_ipm entered at a previous solution's (lam, slacks)
 *   qpx_ipm_range_warm .... (no reference counterpart)            qpx_ipm_range entered at a previous solution's (lam, slacks, lam_lo, slacks_lo)
 *   qpx_factor_solve_kkt_multi  (no reference counterpart)       factor_kkt once, solve_kkt for K right-hand sides per QP: Jacobians
 *   qpx_backward2 ......... (no reference counterpart)            the second-order pass: the gradient of <W, qpx_backward's gradients>
 *   qpx_pre_factor_soft ... (no reference counterpart)            qpx_pre_factor with a quadratic penalty on the violation of chosen rows of G z <= h
 *
 * Conventions
 *   - dtype: QPX_F32 or QPX_F64: every `void*` array below has that element type; or QPX_F32_WIDE (see the enum).
 *   - All pointers are DEVICE pointers valid on `stream` (a hipStream_t).  The caller owns every
 *     buffer; the library never allocates or frees device memory.  Calls are stream-ordered and
 *     re-entrant: the only mutable state is the A/B knob of qpx_set_ipm_variant, which is per host
 *     thread (thread_local) and which nothing but measurements and tests should touch.
 *   - No call synchronises with the host, with ONE exception, in the large-QP family only (nz+neq+nineq > 208) when
 *     a batch of >= 96 QPs is worked on in two parts on two streams (the default there; knob bits 16..19 = 1 turns it
 *     off): the first call of a host thread on a device creates one side stream (kept for the thread's life) and
 *     checks ONCE per (side stream, caller stream) pair -- the last 8 pairs are remembered -- that the two really run
 *     side by side (HIP may deal both to one hardware queue: the parts would serialise, 2 x slower).  That check
 *     enqueues two 100-us delay kernels and waits for them on the host (~0.3 ms; it also waits for whatever the
 *     caller had queued on `stream` before).  It is skipped while `stream` is being captured into a graph and when
 *     the environment variable QPX_NO_STREAM_PROBE is set (then the first side stream is taken as it comes).
 *   - Arrays are dense, row-major, batch-major: Q (B,n,n), p (B,n), G (B,m,n), h (B,m),
 *     A (B,q,n), b (B,q).  A batch stride (in elements) of 0 means "one copy shared by the whole
 *     batch" (the reference's un-batched parameters, qpth/util.py:44-50).  q = 0: A, b unused.
 *   - `factors`: B * qpx_factor_elems(dtype,n,m,q) elements of scratch that carries the
 *     factorisations from qpx_pre_factor to qpx_ipm / qpx_factor_solve_kkt / qpx_backward
 *     (what the reference stashes on ctx as Q_LU, S_LU, R; qpth/qp.py:93).  Consumers take
 *     its batch stride `sfac` in elements: qpx_factor_elems(dtype,n,m,q), or 0 when Q, G, A are
 *     shared by the whole batch and were factored once with B = 1 (only if qpx_can_share_factors()).
 *   - `status`: int32[B], per-QP bit mask of QPX_ST_* written on the device; the functions
 *     themselves return 0 or a negative QPX_ERR_* launch/argument error and never throw.
 *   - Semantics of the IPM loop are those of the reference for a batch of one per QP; see
 *     `stall_policy` and DESIGN.md for the batch-global quirks of the reference this removes.
 */
#ifndef QPX_H
#define QPX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QPX_ABI_VERSION 8

/* QPX_F32_WIDE (ABI v4): the caller's arrays are float32, `factors` and all arithmetic are float64 -- every `void*`
 * array below except `factors` has float elements, `factors` holds qpx_factor_elems(QPX_F32_WIDE, ...) DOUBLES.  On
 * MI355X the float64 matrix-core kernels are as fast as the float32 thread-grid kernels and return the float64
 * solution of the float32 data (the float32 kernels iterate on products rounded to float32: ~1e-4 from it on the
 * reference's benchmark generator).  Served where the thread-grid / tile kernels run (nz+neq+nineq <= 208) and (v6) by
 * the large-QP family, else QPX_ERR_UNSUPPORTED; refine must be 0; qpx_batch_outer takes QPX_F32 for such a caller's
 * float32 vectors. */
enum { QPX_F32 = 0, QPX_F64 = 1, QPX_F32_WIDE = 2 };

enum {
    QPX_OK = 0,
    QPX_ERR_ARG = -1,          /* bad dtype / sizes / null pointer            */
    QPX_ERR_UNSUPPORTED = -2,  /* max(n,m,q) beyond what this build dispatches */
    QPX_ERR_LAUNCH = -3,       /* HIP launch error (see hipGetLastError)       */
    QPX_ERR_NO_DEVICE = -4
};

/* per-QP status bits */
enum {
    QPX_ST_Q_NOT_SPD = 1,      /* -> RuntimeError('Q is not SPD.')       qp.py:85          */
    QPX_ST_A_RANK = 2,         /* A Q^-1 A^T not factorable              batch.py:407       */
    QPX_ST_KKT_BREAKDOWN = 4,  /* factor_kkt failed, best iterate returned  batch.py:110-113 */
    QPX_ST_INACCURATE = 8,     /* best residual > 1 -> INACC_ERR warning   batch.py:141,205  */
    QPX_ST_MAXITER = 16,
    QPX_ST_NONFINITE = 32,
    QPX_ST_NOT_CENTRED = 64    /* qpx_centre ended with its residual above tol (last iterate returned) */
};

/* stall_policy of qpx_ipm: how `notImprovedLim` (batch.py:127-140, batch-global in the
 * reference) is applied per QP.  0 = never stop on stall; 1 = the reference's counter per QP
 * (identical to the reference for a batch of one); 2 = round-off-floor rule (default for B > 1). */
enum { QPX_STALL_OFF = 0, QPX_STALL_REFERENCE = 1, QPX_STALL_FLOOR = 2 };

typedef void* qpx_stream_t; /* hipStream_t */

int qpx_abi_version(void);
const char* qpx_strerror(int code);

/* elements (of dtype) of factor storage per QP (C2, f64: 27 100 = 217 KB; B = 65536, n = m = 64: 5.5 GB) */
size_t qpx_factor_elems(int dtype, int n, int m, int q);

/* largest max(n,m,q) this build can solve (1 024 since round 6; qpx_polish: 512, see qpx_polish_supported) */
int qpx_max_dim(void);
/* QPX_OK if (dtype, n, m, q) is served under the calling thread's knob, else the QPX_ERR_* the entry points would
 * return (QPX_F32_WIDE: QPX_ERR_UNSUPPORTED outside the thread-grid / tile kernels' sizes) */
int qpx_supported(int dtype, int n, int m, int q);
/* v6: which kernel family serves (dtype, n, m, q) under the calling thread's knob (or a negative QPX_ERR_*):
 * the thread-grid kernels, the float64 matrix-core tile kernels (nineq <= 112, nz+neq+nineq <= 208), or the large-QP
 * family (multi-kernel blocked Cholesky / GEMM path).  The host mirror uses it to decide where float32 tensors run in
 * float64 arithmetic (QPX_F32_WIDE: the last two).  (0 was the family of the round-1 workgroup kernels, deleted in v7.) */
enum { QPX_FAMILY_GRID = 1, QPX_FAMILY_TILE = 2, QPX_FAMILY_BIG = 3 };
int qpx_kernel_family(int dtype, int n, int m, int q);
/* v5: 1 if qpx_factor_solve_kkt / qpx_backward implement refine > 0 for this size and dtype (else they return
 * QPX_ERR_UNSUPPORTED when asked to): the in-kernel iterative refinement of KKTSolvers.IR_UNOPT, batch.py:244-270. */
int qpx_refine_supported(int dtype, int n, int m, int q);

/* tuning/A-B knob (per host thread): which kernel family runs.  0 (default) = automatic: the thread-grid /
 * matrix-core kernels (sweep pre-factorisation, register-resident LDL^T with in-place inverse factor)
 * whenever nz+neq+nineq <= 208, else the large-QP family (batched multi-kernel blocked Cholesky / MFMA GEMM path,
 * qpx_big.h -- BASELINE.json configs[3], nz = nineq = 500; equality constraints included since v6);
 * 3 = always the large-QP family.  (1 selected the round-1 workgroup kernels until v7: deleted, the value now means 0.)
 * Adding 256 / 512 / 1024 forces the 16x16-thread grid / the 8x8-thread grid / the matrix-core tile form
 * (f64, nineq <= 112) of the loop kernel, adding 2048 / 4096 / 8192 fixes the tile form's waves per QP
 * at 1 / 2 / 4 (four waves at 4 or 7 tile rows = the chain-wave form, which is the default there); by default the
 * library picks by dtype and size.  Bit 14 (16384): qpx_pre_factor by the symmetric sweep on the thread grid also
 * where its matrix-core form serves the size (float64 arithmetic, 33 <= nz + neq <= 112, nineq <= 112: a
 * factorisation of Q -- of [[Q, A^T], [A, 0]] -- + tile products, qpx_prefac.h; same blob).  (Bit 15, and bit 14 until v6, selected two round-3
 * forms -- a pre-factorisation by a sweep on matrix-core tiles and the four-wave tile kernels without their chain wave
 * -- that lost their A/Bs and were deleted.)
 * Large-QP family only: bits 16..19 = number of parts (1..4) the batch is split into, each part enqueued on a
 * stream of its own (the caller's + side streams forked from and joined back into it with events; the one host wait
 * this can involve is described under "Conventions"), 0 = automatic: two parts from 96 QPs up, else one, in
 * qpx_pre_factor, qpx_ipm / qpx_forward and qpx_polish; one part in qpx_factor_solve_kkt / qpx_backward (one factorisation +
 * one solve is too short a sequence to gain: profiles/r06q_backward_parts.txt), which take parts only from an explicit value; bits 20..24 = initial stagger between the side streams in units of 16 us; (bit 25 selected
 * the four-wave substitutions of round 3 until v7: retired with them); bit 26 = the mat-vec R z' in front of the factorisation
 * in the caller's stream (the round-3 order) instead of beside it on a helper stream; bit 27 =
 * diagonal blocks eliminated by one wave (the round-3 form) instead of four in the chain-wave form; bit 28 = on the
 * thread grid; bit 29 = no XCD-aware tile order.
 * The knob must not change between qpx_pre_factor and the calls that consume its factors (it selects the
 * layout of `factors` too: ask qpx_factor_elems after setting it).
 * Bits and values the library does not decode (retired knobs) are dropped, not stored: qpx_get_ipm_variant returns what
 * was understood, so set-then-get tells a script that its knob no longer exists.
 * Returns the previous value. */
int qpx_set_ipm_variant(int variant);
int qpx_get_ipm_variant(void);      /* the calling thread's current value */

/* May a batch whose Q, G, A are shared be served by ONE factor blob (qpx_pre_factor with B = 1, consumers
 * with sfac = 0)?  Yes for the thread-grid / tile kernels, which only read the blob; no for the large-QP family, which keeps
 * per-QP work matrices in it. */
int qpx_can_share_factors(int dtype, int n, int m, int q);

/* Measurement hook (bench.py): re-issues the largest GEMM of the large-QP pre-factorisation, R = Zt Zt^T, on the
 * blobs qpx_pre_factor wrote (idempotent: R is rewritten with the same values), as ONE launch on `stream`, so that
 * it can be bracketed by events on its own.  QPX_ERR_UNSUPPORTED when (dtype, n, m, q) is not served by that family. */
int qpx_big_gemm_r(int dtype, int B, int n, int m, int q, void* factors, qpx_stream_t stream);

/* pre_factor_kkt(Q, G, A).  status[i] = 0, or exactly QPX_ST_Q_NOT_SPD / QPX_ST_A_RANK for a QP whose factorisation broke
 * down; the blobs and status words of the other QPs of the batch are those of a batch without it, bit for bit.  The failed
 * QP's own blob: ALL ZEROS (every one of its qpx_factor_elems words) from the thread-grid / matrix-core kernels; from the
 * large-QP family unspecified -- the launches behind the failed diagonal block still run on it -- but for the failure bit
 * among its control words (BigCtrl: bcFail), which stops qpx_ipm on that QP.  (tests/prefac_checks.py pins all of it.) */
int qpx_pre_factor(int dtype, int B, int n, int m, int q,
                   const void* Q, int64_t sQ, const void* G, int64_t sG, const void* A, int64_t sA,
                   void* factors, int32_t* status, qpx_stream_t stream);

/* Soft inequality rows (additive after v8; QPX_ABI_VERSION stays 8):
 *     min 1/2 z'Qz + p'z + 1/2 sum_i rho_i t_i^2   s.t.  Gz <= h + t,  Az = b
 * pre-factored as the hard QP with two values of the blob changed -- R + diag(w) on the diagonal of every image of
 * R = G K G^T, and sqrt(|| G^T 1 ||^2 + #{i: w_i > 0}) for || G^T 1 || -- which is exactly the pre-factorisation of the
 * augmented QP in (z, t) condensed to the nineq rows.  w (B,m) of `dtype` (float32 under QPX_F32_WIDE), w_i = 1 / rho_i,
 * 0 = a hard row; sw: its batch stride in elements, 0 = shared by the batch; w == NULL is qpx_pre_factor itself, and an
 * all-zero w writes the same blob bit for bit.  Entries must be finite and >= 0: a QP with any other entry gets
 * QPX_ST_NONFINITE OR-ed into its status word.  Every consumer of the blob then serves the softened QP as it stands:
 * qpx_ipm(_warm) returns lam, the violation is t = w lam, and slack = h + t - G zhat; in qpx_backward(_duals) the
 * gradient with respect to w is -dz lam (dz: the KKT solution the call returns on request), in qpx_jvp a tangent tw
 * acts as th + tw lam.  NOT for refine > 0 or qpx_polish: they evaluate residuals from the caller's Q, G, A, i.e. of
 * the hard QP; the host refuses the combination. */
int qpx_pre_factor_soft(int dtype, int B, int n, int m, int q,
                        const void* Q, int64_t sQ, const void* G, int64_t sG, const void* A, int64_t sA,
                        const void* w, int64_t sw, void* factors, int32_t* status, qpx_stream_t stream);

/* forward(Q,p,G,h,A,b,Q_LU,S_LU,R,...): the PDIPM loop on pre-factored QPs.  Outputs in the
 * reference's return order x, y, z, s = zhat (B,n), nu (B,q), lam (B,m), slacks (B,m);
 * iters int32[B]; best_resid dtype[B]; trace: NULL or dtype[maxIter][B][3] = (pri_resid,
 * dual_resid, mu) per iteration (what verbose=1 prints, batch.py:115-117). */
int qpx_ipm(int dtype, int B, int n, int m, int q,
            const void* p, int64_t sp, const void* h, int64_t sh, const void* b, int64_t sb,
            void* factors, int64_t sfac, double eps, int maxIter, int notImprovedLim, int stall_policy,
            void* zhat, void* nu, void* lam, void* slack,
            int32_t* iters, int32_t* status, void* best_resid, void* trace, qpx_stream_t stream);

/* Additive after v8 (QPX_ABI_VERSION stays 8): qpx_ipm entered at a WARM START -- qpx_ipm's arguments plus lam0, s0 (B,m),
 * dense, of dtype like lam (float32 under QPX_F32_WIDE): the multipliers and slacks of a previous solution of a nearby batch.
 * Per QP: if all 2 m entries are finite the loop starts at z = max(lam0, warm_floor), s = max(s0, warm_floor), with
 * x = x0 - M^T z and nu = nu0 - W^T z implied by z (dual- and equality-feasible by construction): the reference's
 * start point (batch.py:61-87: one factorisation and one solve) is skipped and the passes begin at 0.  A QP with a NaN or an Inf
 * among its entries starts exactly as in qpx_ipm.  warm_used (int32[B], may be NULL): 1 where the warm entry was taken, else 0
 * (written only when lam0, s0 are given).  Stop rules, iters, status bits, trace and outputs: those of qpx_ipm; there is no new
 * status bit.  lam0 = s0 = NULL IS qpx_ipm; exactly one of them NULL, or a warm_floor that is not finite or <= 0:
 * QPX_ERR_ARG.  Served where qpx_warm_supported returns 1 under the calling thread's knob: the thread-grid / tile kernels
 * (nz+neq+nineq <= 208), all three dtypes; the large-QP family (its start point is a batch-wide launch sequence) returns
 * QPX_ERR_UNSUPPORTED when lam0, s0 are given. */
int qpx_warm_supported(int dtype, int n, int m, int q);
int qpx_ipm_warm(int dtype, int B, int n, int m, int q,
                 const void* p, int64_t sp, const void* h, int64_t sh, const void* b, int64_t sb,
                 void* factors, int64_t sfac, double eps, int maxIter, int notImprovedLim, int stall_policy,
                 void* zhat, void* nu, void* lam, void* slack,
                 int32_t* iters, int32_t* status, void* best_resid, void* trace,
                 const void* lam0, const void* s0, double warm_floor, int32_t* warm_used, qpx_stream_t stream);

/* qpx_pre_factor followed by qpx_ipm on the same stream */
int qpx_forward(int dtype, int B, int n, int m, int q,
                const void* Q, int64_t sQ, const void* p, int64_t sp,
                const void* G, int64_t sG, const void* h, int64_t sh,
                const void* A, int64_t sA, const void* b, int64_t sb,
                void* factors, double eps, int maxIter, int notImprovedLim, int stall_policy,
                void* zhat, void* nu, void* lam, void* slack,
                int32_t* iters, int32_t* status, void* best_resid, void* trace, qpx_stream_t stream);

/* factor_kkt(S_LU, R, d) then solve_kkt(Q_LU, d, G, A, S_LU, rx, rs, rz, ry) -> dx, ds, dz, dy.
 * d (B,m) > 0; rx (B,n), rs, rz (B,m), ry (B,q): NULL means zeros; dy may be NULL when q = 0.
 * refine > 0: that many steps of ITERATIVE REFINEMENT on the residual of the original KKT system
 * (qpth/solvers/pdipm/batch.py:228-270, kkt_resid_reg + solve_kkt_ir -- KKTSolvers.IR_UNOPT), evaluated with the
 * caller's Q (sQ), G (sG), A (sA) (batch strides in elements, 0 = shared); the factorisation is re-used, not repeated.
 * Implemented by the thread-grid / tile kernels (nz+neq+nineq <= 208, dtype QPX_F32 / QPX_F64): qpx_refine_supported.
 * Anywhere else refine > 0 returns QPX_ERR_UNSUPPORTED (v5; up to v4 the other kernel families ignored it). */
int qpx_factor_solve_kkt(int dtype, int B, int n, int m, int q, void* factors, int64_t sfac,
                         const void* d, const void* rx, const void* rs, const void* rz, const void* ry,
                         void* dx, void* ds, void* dz, void* dy,
                         int refine, const void* Q, int64_t sQ, const void* G, int64_t sG, const void* A, int64_t sA,
                         int32_t* status, qpx_stream_t stream);

/* QPFunctionFn.backward for given (zhat, lam, slacks, nu) -- from qpx_ipm or from any other
 * solver (qp.py:142-155) -- and dl_dz (B,n).  Per-QP gradients dQ (B,n,n), dp (B,n),
 * dG (B,m,n), dh (B,m), dA (B,q,n), db (B,q); each of the six may be NULL = "this gradient is not
 * wanted" (ctx.needs_input_grad): nothing is computed or written for it.  dx (B,n), dz (B,m),
 * dy (B,q): optional (NULL = skip) solution of the backward KKT system itself (qp.py:151-155), the
 * inputs of qpx_batch_outer.  refine, Q, G, A: as for qpx_factor_solve_kkt (0 / NULL: no refinement). */
int qpx_backward(int dtype, int B, int n, int m, int q, void* factors, int64_t sfac,
                 const void* zhat, const void* lam, const void* slack, const void* nu, const void* dl_dz,
                 void* dQ, void* dp, void* dG, void* dh, void* dA, void* db,
                 void* dx, void* dz, void* dy,
                 int refine, const void* Q, int64_t sQ, const void* G, int64_t sG, const void* A, int64_t sA,
                 int32_t* status, qpx_stream_t stream);

/* Additive after v8 (QPX_ABI_VERSION stays 8): qpx_backward for a loss l(zhat, lam, nu) that also depends on the MULTIPLIERS
 * -- qpx_backward's arguments plus the cotangents dl_dlam (B,m) and dl_dnu (B,q) of lam and nu, of dtype like dl_dz (float32
 * under QPX_F32_WIDE).  The same launch with the right-hand side (rx, rs, rz, ry) = (dl_dz, 0, dl_dlam, dl_dnu) in the solver's
 * convention K sol = -r, and the same six gradient formulas on the new (dx, dz, dy):
 *   dQ = 1/2 (dx zhat' + zhat dx'), dp = dx, dG = dz zhat' + lam dx', dh = -dz, dA = dy zhat' + nu dx', db = -dy.
 * Each of the three cotangents may be NULL = zero (dl_dnu is ignored when q = 0), but not all of them: QPX_ERR_ARG.  Exactly
 * the adjoint of qpx_jvp's (dzhat, dlam, dnu):
 *   <dl_dz, dzhat> + <dl_dlam, dlam> + <dl_dnu, dnu> = <dQ, tQ> + <dp, tp> + <dG, tG> + <dh, th> + <dA, tA> + <db, tb>  per QP.
 * There is no cotangent of the slacks (rs stays zero: ds = (-rs - dz) / d with d from 1e-10 to 1e8 loses eight digits;
 * DESIGN 4.5) -- a caller differentiates h - G zhat instead.  qpx_backward IS this call with dl_dlam = dl_dnu = NULL (and
 * dl_dz required); everything else -- outputs, refine, Q, G, A, status -- as for qpx_backward. */
int qpx_backward_duals(int dtype, int B, int n, int m, int q, void* factors, int64_t sfac,
                       const void* zhat, const void* lam, const void* slack, const void* nu,
                       const void* dl_dz, const void* dl_dlam, const void* dl_dnu,
                       void* dQ, void* dp, void* dG, void* dh, void* dA, void* db,
                       void* dx, void* dz, void* dy,
                       int refine, const void* Q, int64_t sQ, const void* G, int64_t sG, const void* A, int64_t sA,
                       int32_t* status, qpx_stream_t stream);

/* Additive after v8 (QPX_ABI_VERSION stays 8): FORWARD MODE of QPFunction -- the tangent of the solution at the given
 * (zhat, lam, slack, nu) along tangents tQ (B,n,n), tp (B,n), tG (B,m,n), th (B,m), tA (B,q,n), tb (B,q) of the six
 * parameters (each with its batch stride, 0 = shared; NULL = zero).  One KKT solve with the backward's matrix,
 * d = clamp(lam, 1e-8) / clamp(slack, 1e-8) (qp.py:148), and the solver's convention K sol = -r (batch.py:349-372) with
 *   rx = 1/2 (tQ + tQ^T) zhat + tp + tG^T lam + tA^T nu,   rs = 0,   rz = tG zhat - th,   ry = tA zhat - tb;
 * dzhat (B,n) = dx (required); dlam (B,m) = dz, dnu (B,q) = dy, dslack (B,m) = ds = -dlam / d: optional (NULL = skip).
 * Exactly the adjoint of qpx_backward: <dl_dz, dzhat> = <dQ, tQ> + <dp, tp> + <dG, tG> + <dh, th> + <dA, tA> + <db, tb>
 * per QP.  dtype QPX_F32, QPX_F64 or QPX_F32_WIDE (the tangents and outputs float32 then); refine, Q, G, A and the checks
 * as for qpx_backward (refine > 0 where qpx_refine_supported says so, else QPX_ERR_UNSUPPORTED); the large-QP family
 * refuses sfac = 0 with B > 1.  A breakdown of the factorisation ORs QPX_ST_KKT_BREAKDOWN into status. */
int qpx_jvp(int dtype, int B, int n, int m, int q, void* factors, int64_t sfac,
            const void* zhat, const void* lam, const void* slack, const void* nu,
            const void* tQ, int64_t stQ, const void* tp, int64_t stp, const void* tG, int64_t stG,
            const void* th, int64_t sth, const void* tA, int64_t stA, const void* tb, int64_t stb,
            void* dzhat, void* dlam, void* dnu, void* dslack,
            int refine, const void* Q, int64_t sQ, const void* G, int64_t sG, const void* A, int64_t sA,
            int32_t* status, qpx_stream_t stream);

/* Additive after v8 (QPX_ABI_VERSION stays 8): qpx_factor_solve_kkt for K RIGHT-HAND SIDES per QP in one launch -- T = R + diag(1/d)
 * is factored ONCE per QP (it depends on d alone), then the K solves run in blocks through the condensed inverse, each block
 * streaming the blob's matrices once.  What K calls of qpx_backward / qpx_factor_solve_kkt at one solution cost K
 * factorisations for: Jacobians of the solution, sensitivity analysis, per-sample gradients (qpth_amd/sensitivity.py).
 * d (B,m) > 0, one per QP.  rx (B,K,n), rs, rz (B,K,m), ry (B,K,q): a QP's K vectors contiguous, row-major; NULL = zeros, but
 * not all of them (ry is ignored when q = 0): QPX_ERR_ARG.  dx (B,K,n) required; ds, dz (B,K,m), dy (B,K,q): NULL = skip.
 * K >= 1 is a run-time argument; K = 1 IS qpx_factor_solve_kkt (refine = 0): the same kernel, the same bits.  sfac = 0 (shared factors) as
 * everywhere.  There is no refinement here.  Served where qpx_multi_supported returns 1 under the calling thread's knob: the
 * thread-grid / tile kernels (nz+neq+nineq <= 208), dtype QPX_F32, QPX_F64 or QPX_F32_WIDE; the large-QP family returns
 * QPX_ERR_UNSUPPORTED (call qpx_factor_solve_kkt K times there).  A breakdown of the factorisation ORs QPX_ST_KKT_BREAKDOWN
 * into status and returns zeros for dz, as the single solve does. */
int qpx_multi_supported(int dtype, int n, int m, int q);
int qpx_factor_solve_kkt_multi(int dtype, int B, int n, int m, int q, int K, void* factors, int64_t sfac,
                               const void* d, const void* rx, const void* rs, const void* rz, const void* ry,
                               void* dx, void* ds, void* dz, void* dy,
                               int32_t* status, qpx_stream_t stream);

/* Additive after v8 (QPX_ABI_VERSION stays 8): the SECOND-ORDER pass of the backward -- what torch.autograd.grad(...,
 * create_graph=True) differentiates.  At the solution (zhat, lam, slack, nu), with (dx, dz, dy) the KKT solution a call of
 * qpx_backward(_duals) returned for cotangents (dl_dz, dl_dlam, dl_dnu), and W_Q (B,n,n), W_p (B,n), W_G (B,m,n), W_h (B,m),
 * W_A (B,q,n), W_b (B,q) cotangents on that call's six gradients (each with its batch stride in elements, 0 = shared; NULL = zero):
 * the gradient of  psi = <W_Q, dQ> + <W_p, dp> + <W_G, dG> + <W_h, dh> + <W_A, dA> + <W_b, db>  per QP
 *   - with respect to (dl_dz, dl_dlam, dl_dnu): zdot (B,n) (required), lamdot (B,m), nudot (B,q) (NULL = skip) -- qpx_jvp's
 *     (dzhat, dlam, dnu) along W;
 *   - with respect to the six parameters: HQ (B,n,n), Hp (B,n), HG (B,m,n), Hh (B,m), HA (B,q,n), Hb (B,q), each NULL = not
 *     wanted: nothing is computed or written for it.
 * One launch, one factorisation of T = R + diag(1/d) per QP, two solves, the second right-hand side formed from the first
 * solution on the chip (DESIGN 4.9 has the closed form).  Second derivatives of a QP's solution exist only under strict
 * complementarity (no row with lam_i = s_i = 0).  No refinement.  dtype QPX_F64 or QPX_F32_WIDE (W, inputs and outputs float32
 * then), where qpx_backward2_supported returns 1 under the calling thread's knob: every form of the thread-grid / tile kernels
 * (nz+neq+nineq <= 208) that the default dispatch picks; QPX_F32, the large-QP family and the two-wave tile forms of the A/B
 * knob return QPX_ERR_UNSUPPORTED -- compose the pass from qpx_jvp and qpx_backward_duals there (qpth_amd/kkt.py:
 * KKTFactors.backward2).  A breakdown of the factorisation ORs QPX_ST_KKT_BREAKDOWN into status, as the single solve does. */
int qpx_backward2_supported(int dtype, int n, int m, int q);
int qpx_backward2(int dtype, int B, int n, int m, int q, void* factors, int64_t sfac,
                  const void* zhat, const void* lam, const void* slack, const void* nu,
                  const void* dx, const void* dz, const void* dy,
                  const void* W_Q, int64_t sWQ, const void* W_p, int64_t sWp, const void* W_G, int64_t sWG,
                  const void* W_h, int64_t sWh, const void* W_A, int64_t sWA, const void* W_b, int64_t sWb,
                  void* zdot, void* lamdot, void* nudot,
                  void* HQ, void* Hp, void* HG, void* Hh, void* HA, void* Hb,
                  int32_t* status, qpx_stream_t stream);

/* v6: the FINISHING STAGE as one kernel -- `steps` iterations of the reference's PDIPM loop in the original variables
 * (qpth/solvers/pdipm/batch.py:92-198: affine + centring-corrector Newton steps, step lengths batch.py:189-198) started
 * from the iterate (zhat, nu, lam, slack) the caller passes in, with the KKT residuals (batch.py:93-101) formed from the
 * caller's Q, p, G, h, A, b in float64 accumulation whatever dtype is, every KKT solve through the factors of
 * qpx_pre_factor and refined `refine` times on the residual of the original system (kkt_resid_reg / solve_kkt_ir,
 * batch.py:228-270 -- what forward(solver=KKTSolvers.IR_UNOPT) asks for).  The four arrays are overwritten with the BEST
 * iterate met (the reference's rule, batch.py:118-139: residual ||rx|| + ||rz|| + ||ry|| + nineq mu, strict <, NaN never
 * wins; the start iterate competes), best_resid (dtype[B], may be NULL) with its residual.  Served by every kernel
 * family since v7 (dtype QPX_F32 or QPX_F64; one kernel up to nz+neq+nineq = 208, the large-QP family's launch sequence
 * beyond, where `refine` must be 0: qpx_refine_supported, and up to max(n,m,q) = 512 only: its vectors live in LDS);
 * qpx_polish_supported says so; QPX_F32_WIDE and sizes beyond that: QPX_ERR_UNSUPPORTED.  Strides as everywhere: elements, 0 = shared by the batch. */
int qpx_polish_supported(int dtype, int n, int m, int q);
int qpx_polish(int dtype, int B, int n, int m, int q,
               const void* Q, int64_t sQ, const void* p, int64_t sp, const void* G, int64_t sG, const void* h, int64_t sh,
               const void* A, int64_t sA, const void* b, int64_t sb,
               void* factors, int64_t sfac, int steps, int refine,
               void* zhat, void* nu, void* lam, void* slack, void* best_resid,
               int32_t* status, qpx_stream_t stream);

/* Additive after v8 (QPX_ABI_VERSION stays 8): CENTRING -- Newton's method onto the point of the central path
 *   Q z + p + G^T lam + A^T nu = 0,   G z + s = h,   A z = b,   s_i lam_i = kappa_i   (s, lam > 0),
 * the minimiser of 1/2 z'Qz + p'z - sum_i kappa_i log(h_i - g_i'z) s.t. Az = b, started from the iterate (zhat, nu, lam, slack)
 * a loop launch returned, its (s, lam) first lifted row by row onto s_i lam_i >= kappa_i from below (s to kappa / lam, then
 * lam to kappa / s, neither denominator below sqrt(kappa): values only grow, and an entry that came in as 0 or not positive
 * becomes sqrt(kappa) -- the loop returns s = lam = 0 exactly on a weakly active row of a QP its start point solves).  One kernel, one workgroup per QP, the iterate in float64; per step: the
 * residuals rx, rz, ry from the caller's Q, p, G, h, A, b in float64 accumulation and rc_i = s_i lam_i - kappa_i, ONE
 * factorisation of R + diag(s/lam) and ONE solve through the factors of qpx_pre_factor -- solve_kkt(rx, rs, rz, ry) with
 * rs_i = lam_i - kappa_i / s_i --, the full step where it keeps s, lam > 0, else 0.99 of the step to the boundary.  A QP stops
 * when  res = max(||rx||_inf, ||rz||_inf, ||ry||_inf, max_i |rc_i| / kappa_i) <= tol  or after max_steps steps.  The four
 * arrays are overwritten with the LAST iterate, resid (dtype[B], may be NULL) with its res, steps (int32[B], may be NULL) with
 * the Newton steps taken.  kappa: (B,m) of dtype, batch stride skappa in elements, 0 = one (m) vector for the batch.
 * status: a kappa entry that is not finite and > 0 ORs QPX_ST_NONFINITE (nothing else is written for that QP but resid =
 * +inf, steps = 0); a breakdown of a factorisation ORs QPX_ST_KKT_BREAKDOWN and leaves the four arrays as they came in; a QP
 * that ends with res > tol (NaN included) ORs QPX_ST_NOT_CENTRED.
 * Served where the finishing stage is one kernel in float64 arithmetic: dtype QPX_F64 and nz+neq+nineq <= 208 under the
 * default knob (qpx_centre_supported); QPX_F32, QPX_F32_WIDE, the large-QP family: QPX_ERR_UNSUPPORTED.  NULL kappa, tol <= 0
 * (or NaN), max_steps < 1: QPX_ERR_ARG.  NOT for factors of qpx_pre_factor_soft: the residuals are those of the hard QP.
 * The derivative entry points serve the centred point as they stand (d = lam / s = kappa / s^2); the gradient with respect to
 * kappa_i is dz_i / lam_i, dz the inequality block of the backward's KKT solution. */
int qpx_centre_supported(int dtype, int n, int m, int q);
int qpx_centre(int dtype, int B, int n, int m, int q,
               const void* Q, int64_t sQ, const void* p, int64_t sp, const void* G, int64_t sG, const void* h, int64_t sh,
               const void* A, int64_t sA, const void* b, int64_t sb,
               void* factors, int64_t sfac, const void* kappa, int64_t skappa, double tol, int max_steps,
               void* zhat, void* nu, void* lam, void* slack, void* resid, int32_t* steps,
               int32_t* status, qpx_stream_t stream);

/* Additive after v8 (QPX_ABI_VERSION stays 8): TWO-SIDED inequality rows,  lower <= G z <= h  in nineq rows --
 * the QP a caller had to write as [G; -G] z <= [h; -lower] with 2 nineq rows.  The factors are those of qpx_pre_factor for
 * (Q, G, A): the doubled QP's Newton system collapses to the m x m system the loop already factors, with the diagonal
 * 1/(zu/su + zl/sl); the iterates, iteration counts and stop rule are those of qpx_ipm on the doubled QP.
 * qpx_ipm_range: qpx_ipm's arguments, then
 *   lower (B,m) of dtype, batch stride slo in elements (0 = one (m) vector for the batch); -inf = a ONE-SIDED row, as in qpx_ipm;
 *   gt1 (B) of dtype: || G^T e ||_2 per QP, e_i = 1 on the one-sided rows and 0 on the two-sided ones -- the doubled QP's
 *     || G'^T 1 || of the stop rule (batch.py:103-107) --, NULL = 0 (every row two-sided);
 *   lam_lo, slack_lo (B,m) of dtype, out: the multipliers and slacks of the rows  lower <= G z  beside lam, slack of  G z <= h;
 *     0 and +inf on a one-sided row.
 * status: a lower entry that is NaN, +inf or not below its h ORs QPX_ST_NONFINITE and the QP is left as after a failed
 * pre-factorisation: NaN in the outputs, iters = 0, best_resid = +inf.  trace as in qpx_ipm; mu is the doubled QP's (over
 * nineq + the number of two-sided rows).
 * qpx_backward_range: qpx_backward's arguments, then lam_lo, slack_lo (B,m) as qpx_ipm_range wrote them.  One launch: the
 * backward's KKT solve with d = clamp(lam)/clamp(slack) + clamp(lam_lo)/clamp(slack_lo) and lam - lam_lo where lam meets dx
 * in dG.  dz is v = dz_upper - dz_lower of the doubled QP's solution; the gradients with respect to the two bounds are
 *   dl/dh = -v du/(du + dl),   dl/dlower = -v dl/(du + dl),   du = clamp(lam)/clamp(slack), dl = clamp(lam_lo)/clamp(slack_lo)
 * (exactly 0 on a one-sided row), which the caller forms from dz; dh, if given, receives their sum -v.  refine must be 0.
 * Served in float64 arithmetic by the loop and backward forms the default dispatch picks, nz+neq+nineq <= 208
 * (qpx_range_supported); QPX_F32, QPX_F32_WIDE, the large-QP family and forms reachable through the A/B knob alone:
 * QPX_ERR_UNSUPPORTED.  No soft factors (qpx_pre_factor_soft) and no refinement in this role.
 * qpx_ipm_range_warm: qpx_ipm_range entered at a WARM START -- its arguments, then lam0, s0, lam0_lo, s0_lo (B,m),
 * dense, of dtype: lam, slack, lam_lo, slack_lo of a previous solution of a nearby batch; warm_floor, warm_used as in
 * qpx_ipm_warm.  Per QP: lam0, s0 are looked at on EVERY row, lam0_lo, s0_lo only on the rows that are two-sided in THIS call
 * (lower > -inf).  If all of those entries are finite the loop starts at zu = max(lam0, warm_floor), su = max(s0, warm_floor),
 * and on the two-sided rows zl = max(lam0_lo, warm_floor), sl = max(s0_lo, warm_floor), with x = x0 - M^T (zu - zl) implied
 * (dual- and equality-feasible for any such iterate); the start point is skipped and the passes begin at 0.  The lower
 * entries of a one-sided row are never read: the 0 and +inf a previous solve wrote there do not send the QP cold.  A row that
 * is two-sided now and carries 0 / +inf from a solve in which it was one-sided is not finite: that QP, as any QP with a NaN
 * or an Inf among the entries looked at, starts exactly as in qpx_ipm_range.  All four arrays NULL IS qpx_ipm_range (which is
 * this call with NULLs); some but not all of them given, or a warm_floor that is not finite or <= 0: QPX_ERR_ARG.
 * Served exactly where qpx_ipm_range is (qpx_range_warm_supported == qpx_range_supported for every argument and knob);
 * anything else is QPX_ERR_UNSUPPORTED, never a fall-through to a kernel without the role. */
int qpx_range_supported(int dtype, int n, int m, int q);
int qpx_range_warm_supported(int dtype, int n, int m, int q);
int qpx_ipm_range_warm(int dtype, int B, int n, int m, int q, const void* p, int64_t sp, const void* h, int64_t sh,
                       const void* b, int64_t sb, void* factors, int64_t sfac, double eps, int maxIter, int notImprovedLim,
                       int stall_policy, void* zhat, void* nu, void* lam, void* slack, int32_t* iters, int32_t* status,
                       void* best_resid, void* trace, const void* lower, int64_t slo, const void* gt1, void* lam_lo,
                       void* slack_lo, const void* lam0, const void* s0, const void* lam0_lo, const void* s0_lo,
                       double warm_floor, int32_t* warm_used, qpx_stream_t stream);
int qpx_ipm_range(int dtype, int B, int n, int m, int q, const void* p, int64_t sp, const void* h, int64_t sh,
                  const void* b, int64_t sb, void* factors, int64_t sfac, double eps, int maxIter, int notImprovedLim,
                  int stall_policy, void* zhat, void* nu, void* lam, void* slack, int32_t* iters, int32_t* status,
                  void* best_resid, void* trace, const void* lower, int64_t slo, const void* gt1, void* lam_lo,
                  void* slack_lo, qpx_stream_t stream);
int qpx_backward_range(int dtype, int B, int n, int m, int q, void* factors, int64_t sfac, const void* zhat, const void* lam,
                       const void* slack, const void* nu, const void* dl_dz, void* dQ, void* dp, void* dG, void* dh, void* dA,
                       void* db, void* dx, void* dz, void* dy, int refine, const void* Q, int64_t sQ, const void* G, int64_t sG,
                       const void* A, int64_t sA, int32_t* status, const void* lam_lo, const void* slack_lo, qpx_stream_t stream);

/* Additive after v8 (QPX_ABI_VERSION stays 8): ELASTIC inequality rows,
 *   min 1/2 z'Qz + p'z + sum_i ( gamma_i t_i + 1/2 rho_i t_i^2 )   s.t.  G z <= h + t,  t >= 0,  A z = b
 * -- the QP a caller had to write with nz + nineq variables and 2 nineq rows.  The factors are those of qpx_pre_factor for
 * (Q, G, A), the HARD QP's: the augmented QP's Newton system collapses to the m x m system the loop already factors, with the
 * diagonal s/lam + 1/(rho + lam_t/slack_t); the iterates, iteration counts and stop rule are those of qpx_ipm on the augmented QP.
 * qpx_ipm_elastic: qpx_ipm's arguments, then
 *   gamma, rho (B,m) of dtype, batch strides sgamma, srho in elements (0 = one (m) vector for the batch); a row with gamma = +inf
 *     or rho = +inf is a HARD row, as in qpx_ipm; otherwise gamma >= 0 and rho > 0;
 *   gt1 (B) of dtype: sqrt(|| G^T 1 ||^2 + 4 k) per QP, k its number of elastic rows -- the augmented QP's || G'^T 1 || of the
 *     stop rule (batch.py:103-107);
 *   lam_t, slack_t, t (B,m) of dtype, out: the multipliers and slacks of t >= 0 and t itself, beside lam, slack (= h + t - G z)
 *     of the rows; 0, +inf and 0 on a hard row.
 * status: a gamma entry that is NaN or negative, a rho entry that is NaN or not positive ORs QPX_ST_NONFINITE and the QP is left
 * as after a failed pre-factorisation: NaN in the outputs, iters = 0, best_resid = +inf.  trace as in qpx_ipm; mu is the
 * augmented QP's (over nineq + k).
 * The derivative entry points serve the solution as they stand, on the same factors, given lam and the EFFECTIVE slack
 *   slack_eff = clamp(lam) (1/du + 1/(rho + dt)),   du = clamp(lam)/clamp(slack), dt = clamp(lam_t)/clamp(slack_t)
 * (slack on a hard row; clamps at 1e-8); with dz the inequality block of their KKT solution, dl/dgamma = dz/(dt + rho) and
 * dl/drho = t dl/dgamma.  qpx_backward2 is NOT served that way.
 * Served in float64 arithmetic by the loop forms the default dispatch picks, nz+neq+nineq <= 208 (qpx_elastic_supported);
 * QPX_F32, QPX_F32_WIDE, the large-QP family and forms reachable through the A/B knob alone: QPX_ERR_UNSUPPORTED.  No warm
 * start and no soft factors (qpx_pre_factor_soft) in this role. */
int qpx_elastic_supported(int dtype, int n, int m, int q);
int qpx_ipm_elastic(int dtype, int B, int n, int m, int q, const void* p, int64_t sp, const void* h, int64_t sh,
                    const void* b, int64_t sb, void* factors, int64_t sfac, double eps, int maxIter, int notImprovedLim,
                    int stall_policy, void* zhat, void* nu, void* lam, void* slack, int32_t* iters, int32_t* status,
                    void* best_resid, void* trace, const void* gamma, int64_t sgamma, const void* rho, int64_t srho,
                    const void* gt1, void* lam_t, void* slack_t, void* t, qpx_stream_t stream);

/* Additive after v8 (QPX_ABI_VERSION stays 8): SOFT TWO-SIDED inequality rows,
 *   min 1/2 z'Qz + p'z + sum_i ( gu_i tu_i + 1/2 ru_i tu_i^2 + gl_i tl_i + 1/2 rl_i tl_i^2 )
 *   s.t.  l - tl <= G z <= h + tu,  tu, tl >= 0,  A z = b
 * -- the QP a caller had to write with nz + 2 nineq variables and 4 nineq rows.  The factors are those of qpx_pre_factor for
 * (Q, G, A), the HARD QP's: the augmented QP's Newton system collapses to the m x m system the loop already factors, with the
 * diagonal 1/(1/e_u + 1/e_l), e = s/lam + 1/(rho + lam_t/slack_t) on a soft side, s/lam on a hard one, 1/e_l = 0 on a one-sided
 * row; the iterates, iteration counts and stop rule are those of qpx_ipm on the augmented QP.
 * qpx_ipm_soft_range: qpx_ipm's arguments, then
 *   lower (B,m), batch stride slo (0 = one (m) vector): -inf = a one-sided row, otherwise lower < h strictly;
 *   gamma_u, rho_u, gamma_l, rho_l (B,m) with batch strides: the penalty of each side; gamma = +inf or rho = +inf makes that
 *     side HARD; otherwise gamma >= 0 and rho > 0.  The lower side's entries of a one-sided row are checked and otherwise unused;
 *   gt1 (B): sqrt(|| G^T e ||^2 + 4 (k_u + k_l)) per QP, e_i = 1 on one-sided rows and 0 on two-sided ones, k the number of soft
 *     sides -- the augmented QP's || G'^T 1 || of the stop rule;
 *   lam_lo, slack_lo: the lower rows' multipliers and slacks; lam_t, slack_t, t / lam_tl, slack_tl, t_lo: those of tu >= 0 /
 *     tl >= 0 and tu / tl themselves, all (B,m), out; an absent side reads 0, +inf and 0.
 * status: a NaN entry, a lower not below h, a negative gamma or a rho that is not positive ORs QPX_ST_NONFINITE and the QP is
 * left as after a failed pre-factorisation: NaN in the outputs, iters = 0, best_resid = +inf.  trace as in qpx_ipm; mu is the
 * augmented QP's (over all live complementarity pairs).
 * The backward is qpx_backward_range on the same factors, given lam, lam_lo and the EFFECTIVE slack of each side,
 *   slack_eff = clamp(lam) (clamp(slack)/clamp(lam) + 1/(rho + clamp(lam_t)/clamp(slack_t)))      (slack on a hard side).
 * Served in float64 arithmetic by the loop forms the default dispatch picks, nz+neq+nineq <= 208 (qpx_soft_range_supported);
 * QPX_F32, QPX_F32_WIDE, the large-QP family and forms reachable through the A/B knob alone: QPX_ERR_UNSUPPORTED.  No warm
 * start and no soft factors in this role. */
int qpx_soft_range_supported(int dtype, int n, int m, int q);
int qpx_ipm_soft_range(int dtype, int B, int n, int m, int q, const void* p, int64_t sp, const void* h, int64_t sh,
                       const void* b, int64_t sb, void* factors, int64_t sfac, double eps, int maxIter, int notImprovedLim,
                       int stall_policy, void* zhat, void* nu, void* lam, void* slack, int32_t* iters, int32_t* status,
                       void* best_resid, void* trace, const void* lower, int64_t slo, const void* gamma_u, int64_t sgamma_u,
                       const void* rho_u, int64_t srho_u, const void* gamma_l, int64_t sgamma_l, const void* rho_l,
                       int64_t srho_l, const void* gt1, void* lam_lo, void* slack_lo, void* lam_t, void* slack_t, void* lam_tl,
                       void* slack_tl, void* t, void* t_lo, qpx_stream_t stream);

/* Batch-MEAN of the gradient of a parameter that the whole batch shares (qp.py:159-177: the reference
 * forms B outer products and then `.mean(0)`): one contraction over the batch instead,
 *   out (r,c) = scale/B * sum_b ( u[b][r] v[b][c] + w[b][r] x[b][c] )        u, w: (B,r)  v, x: (B,c)
 * dQ: u = dx, v = zhat, w = zhat, x = dx, scale = 0.5;  dG: u = dz, v = zhat, w = lam, x = dx, scale = 1;
 * dA: u = dy, v = zhat, w = nu, x = dx.  `out` is (r,c) of dtype, overwritten.
 * v8: w == x == NULL: the second product is left out; v == NULL (c must be 1): v is a column of ones, i.e.
 *   out (r) = scale/B * sum_b u[b][r]  -- the `.mean(0)` of a shared VECTOR parameter's gradient (dp = mean dx,
 *   dh = -mean dz, db = -mean dy: qp.py:160-166,174-177), in the same fixed order of additions. */
int qpx_batch_outer(int dtype, int B, int r, int c, const void* u, const void* v, const void* w,
                    const void* x, double scale, void* out, void* ws, size_t ws_elems, qpx_stream_t stream);
/* v7: `ws` -- ws_elems elements of dtype, at least qpx_batch_outer_workspace_elems(dtype, B, r, c) -- lets a long batch be
 * contracted in TWO stages: partial tiles per chunk of the batch by many workgroups, then their sum in chunk order (fixed
 * order: bit-reproducible, no atomics).  NULL / too small / 0 elements needed: one workgroup per 16 x 16 tile of `out`
 * walks the whole batch, as before -- the same result up to the order of the additions. */
size_t qpx_batch_outer_workspace_elems(int dtype, int B, int r, int c);

/* v7: x = M^-1 r for B general k x k systems (Gaussian elimination with partial pivoting, one workgroup each).  M (B,k,k)
 * is destroyed, rhs (B,k) is overwritten by the solution; a singular M ORs QPX_ST_KKT_BREAKDOWN into status[b] (may be
 * NULL) and returns NaNs.  The host mirror's factor_solve_kkt_reg (qpth/solvers/pdipm/batch.py:273-310) with equality
 * constraints uses it for the neq x neq correction of the regularised (y, y) block. */
int qpx_dense_solve(int dtype, int B, int k, void* M, void* rhs, int32_t* status, qpx_stream_t stream);

/* ---- Scenario batches (additive in v8): B groups of K consecutive QPs.  A group shares (Q, G, A) and so ONE
 * factor blob -- `factors` holds B blobs, written by qpx_pre_factor(dtype, B, ...) -- while every per-QP array (p, h, b with
 * a non-zero stride, the outputs, iters, status, best_resid, trace) has B K rows: QP j = g K + k reads blob g.  `status` has
 * B K words too: the caller repeats the pre-factorisation's word of group g for its K QPs.
 *
 * qpx_group_supported: 1 exactly where qpx_can_share_factors is 1 (the kernels only read the blob) and a loop form and a
 * backward form serve the size under the calling thread's knob; 0 for the large-QP family. */
int qpx_group_supported(int dtype, int n, int m, int q);
/* qpx_ipm on the B K QPs (its arguments, its results bit for bit: the form is picked for B K QPs by qpx_ipm's rule and the
 * per-QP arithmetic is the same; only the blob's address differs).  sfac: the stride between GROUPS' blobs.  K < 1 or a NULL
 * that qpx_ipm refuses: QPX_ERR_ARG; a size without qpx_group_supported: QPX_ERR_UNSUPPORTED, before any launch. */
int qpx_ipm_group(int dtype, int B, int K, int n, int m, int q, const void* p, int64_t sp, const void* h, int64_t sh,
                  const void* b, int64_t sb, void* factors, int64_t sfac, double eps, int maxIter, int notImprovedLim,
                  int stall_policy, void* zhat, void* nu, void* lam, void* slack, int32_t* iters, int32_t* status,
                  void* best_resid, void* trace, qpx_stream_t stream);
/* qpx_backward_duals on the B K QPs: dp, dh, db are written per QP (B K rows, any may be NULL).  dQ, dG, dA must be NULL
 * (QPX_ERR_ARG otherwise): a group's matrix gradient is the SUM over its K QPs -- ask for dx, dz, dy (B K rows) and contract
 * them with qpx_group_outer.  refine must be 0 (Q, G, A are ignored); refine > 0 or an unsupported size:
 * QPX_ERR_UNSUPPORTED, before any launch. */
int qpx_backward_group(int dtype, int B, int K, int n, int m, int q, void* factors, int64_t sfac, const void* zhat,
                       const void* lam, const void* slack, const void* nu, const void* dl_dz, const void* dl_dlam,
                       const void* dl_dnu, void* dQ, void* dp, void* dG, void* dh, void* dA, void* db, void* dx, void* dz,
                       void* dy, int refine, const void* Q, int64_t sQ, const void* G, int64_t sG, const void* A, int64_t sA,
                       int32_t* status, qpx_stream_t stream);
/* The grouped mode of qpx_batch_outer: out (B,r,c),
 *   out[g] = scale * sum_{k < K} ( u[j][r] v[j][c] + w[j][r] x[j][c] ),  j = g K + k        u, w: (B K,r)  v, x: (B K,c)
 * (scale is NOT divided by anything; v, w, x NULL as for qpx_batch_outer).  dQ: u = dx, v = zhat, w = zhat, x = dx,
 * scale = 0.5; dG: u = dz, v = zhat, w = lam, x = dx; dA: u = dy, v = zhat, w = nu, x = dx.  Fixed order of additions, no
 * atomics: bit-reproducible.  B > 1 needs `ws`, at least qpx_group_outer_workspace_elems elements of dtype (QPX_ERR_ARG
 * otherwise); QPX_F32 / QPX_F64 only (a QPX_F32_WIDE caller passes QPX_F32, as for qpx_batch_outer). */
int qpx_group_outer(int dtype, int B, int K, int r, int c, const void* u, const void* v, const void* w, const void* x,
                    double scale, void* out, void* ws, size_t ws_elems, qpx_stream_t stream);
size_t qpx_group_outer_workspace_elems(int dtype, int B, int K, int r, int c);

#ifdef __cplusplus
}
#endif
#endif /* QPX_H */
