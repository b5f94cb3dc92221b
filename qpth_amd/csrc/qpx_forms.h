// qpx_forms.h -- which template instantiation ("form") of every launcher family exists: one X-macro list per family.
// The kernel translation units (qpx_hip_kernels.hip) instantiate from these lists and the dispatcher (qpx_api.inc, which
// includes this header itself) picks from them, on the GPU and in the host-thread emulator of the test tree alike: a new
// form is one entry here plus the rule in qpx_api.inc that picks it.  The order of a list is the order of the kernels in
// the code object.
#pragma once
#include <type_traits>

namespace qpx {

// The wave-0 phases of the large-QP family (launch_big_phase / _solve / _diag) hold a vector of the padded nineq in NS
// slots of 64 lanes: f(std::integral_constant<int, NS>) for the smallest of 1, 2, 4, 8, 16 that covers `ns` = big_pad(m) / kWave
template <class F> inline int big_ns_form(int ns, F&& f)
{
    if (ns <= 1) return f(std::integral_constant<int, 1>{});
    if (ns <= 2) return f(std::integral_constant<int, 2>{});
    if (ns <= 4) return f(std::integral_constant<int, 4>{});
    if (ns <= 8) return f(std::integral_constant<int, 8>{});
    return f(std::integral_constant<int, 16>{});
}

// Every KKT form exists in three roles: the solve, the backward (the launchers' kBw) and the solve for K right-hand sides
// in one launch (qpx_factor_solve_kkt_multi; qpx_grid.h: kkt_multi_role).  The third travels in the form's FIRST parameter,
// block / tile rows + kKktMultiRole: every launcher of the family -- the GPU's and the host-thread emulator's -- reaches it
// through the template it already has (kkt_grid_body / kkt_tile_body decode it).
constexpr int kKktMultiRole = 64;
// Right-hand sides per block of that role, every form: the products keep a block's accumulators (4 rows x RB in the row dots)
// beside the register-resident factor, and with eight every tile form but the seven-row chain-wave form and the larger
// float64 thread-grid forms spilled (6 .. 89 registers); at seven tile rows eight would also be the LDS of the second
// workgroup of a CU.  qpth_amd/kkt.py: MULTI_RHS_BLOCK.
constexpr int kKktMultiRB = 4;

// A fourth role, float64 arithmetic only: the second-order pass of the backward (qpx_backward2; qpx_grid.h: kkt_b2_role) -- two
// dependent solves behind one factorisation.  It travels like the third, block / tile rows + kKktB2Role, and exists for the
// forms of QPX_FORMS_KKT_B2_TILE / every thread-grid form below (the tile forms the dispatcher picks by default: the two-wave
// forms, reachable through the A/B knob alone, decline -- qpx_backward2_supported).
constexpr int kKktB2Role = 128;

// Every pre-factorisation form exists a second time for soft rows (qpx_pre_factor_soft): blocks / tile rows + kPrefacSoft in
// the form's FIRST parameter, as above (sweep_body / prefac_tile_body decode it).  The hard forms hold none of the soft
// rows' code: their registers are the ones they had without it.
constexpr int kPrefacSoft = 64;

// Every form of the one-kernel finishing stage exists a second time, float64 arithmetic only, as the CENTRING role
// (qpx_centre; qpx_grid.h: polish_centre_role): Newton steps onto the central-path point s_i lam_i = kappa_i.  Blocks / tile
// rows + kPolishCentreRole in the form's FIRST parameter, as above (polish_mat_body decodes it through PolishForm).  The
// finishing forms hold none of its code.
constexpr int kPolishCentreRole = 64;

// Two-sided rows l <= G z <= h (qpx_ipm_range, qpx_backward_range), float64 arithmetic only.  The loop forms of
// QPX_FORMS_IPM_RANGE_TILE / _GRID exist a second time as the RANGE role (qpx_grid.h: ipm_loop_role, kRange): blocks / tile
// rows + kIpmRangeRole in the form's FIRST parameter, as above (ipm_grid_body / ipm_tile_body decode it); the one-sided forms
// hold none of its code.  The backward of every KKT form the default dispatch picks has a range role too, block / tile rows +
// kKktRangeRole (kkt_grid_body / kkt_tile_body): d = d_upper + d_lower and lam_upper - lam_lower in the outer products.
constexpr int kIpmRangeRole = 64;
constexpr int kKktRangeRole = 256;

// Elastic rows G z <= h + t, t >= 0 with the penalty gamma't + 1/2 t'diag(rho)t (qpx_ipm_elastic), float64 arithmetic
// only.  The loop forms of QPX_FORMS_IPM_RANGE_TILE / _GRID exist a third time as the ELASTIC role (qpx_grid.h: ipm_loop_role,
// kElastic): blocks / tile rows + kIpmElasticRole in the form's FIRST parameter, decoded where the range role is; the one-sided
// and the range forms hold none of its code.  The backward has no such role: it runs on the hard factors with an effective
// slack the host forms.
constexpr int kIpmElasticRole = 128;

// Soft two-sided rows l - tl <= G z <= h + tu, tu, tl >= 0 with a penalty gamma t + 1/2 rho t^2 per side (qpx_ipm_soft_range;
// DESIGN 4.13), float64 arithmetic only: the composition of the two roles above.  The same loop forms exist a fourth time as the
// SOFT-RANGE role (qpx_grid.h: ipm_loop_role, kSoft): blocks / tile rows + kIpmSoftRangeRole in the form's FIRST parameter; the
// one-sided, range and elastic forms hold none of its code.  The backward runs in the range role (kKktRangeRole) with an
// effective slack per side the host forms.
constexpr int kIpmSoftRangeRole = kIpmRangeRole | kIpmElasticRole;

}  // namespace qpx

// thread-grid kernels: (blocks of 16 -- of 8 in the one-wave grid -- per side), (blocks, slots of 64 columns)
#define QPX_FORMS_SWEEP(X) X(1) X(2) X(4) X(7) X(8) X(10) X(13)
#define QPX_FORMS_IPM_GRID(X) \
    X(1, 1) X(1, 2) X(1, 4) X(2, 1) X(2, 2) X(2, 4) X(4, 1) X(4, 2) X(4, 4) X(7, 2) X(7, 4) X(10, 4) X(13, 4)
#define QPX_FORMS_IPM_GRID8(X) X(2, 1) X(2, 2) X(4, 1) X(4, 2) X(8, 1) X(8, 2) X(13, 2)
#define QPX_FORMS_KKT_GRID(X) X(1) X(2) X(4) X(7) X(10) X(13)                 // each as the KKT solve, as the backward and as the multi-right-hand-side solve
#define QPX_FORMS_POLISH_GRID(X) X(1) X(2) X(4) X(7) X(10) X(13)
// matrix-core tile kernels, f64: (tile rows, waves per QP, [slots,] chain-wave form)
#define QPX_FORMS_IPM_TILE(X)                                                                                    \
    X(1, 1, 1, false) X(1, 1, 2, false) X(1, 1, 4, false) X(2, 1, 1, false) X(2, 1, 2, false) X(2, 1, 4, false)  \
    X(4, 1, 1, false) X(4, 1, 2, false) X(4, 1, 4, false) X(4, 2, 1, false) X(4, 2, 2, false) X(4, 2, 4, false)  \
    X(7, 2, 2, false) X(7, 2, 4, false)                                                                          \
    X(7, 4, 2, true) X(7, 4, 4, true) X(4, 4, 1, true) X(4, 4, 2, true) X(4, 4, 4, true)
#define QPX_FORMS_KKT_TILE(X) \
    X(1, 1, false) X(2, 1, false) X(4, 1, false) X(4, 2, false) X(7, 2, false) X(7, 4, true) X(4, 4, true)   // each in the three roles, as above
#define QPX_FORMS_KKT_B2_TILE(X) X(1, 1, false) X(2, 1, false) X(4, 1, false) X(7, 4, true) X(4, 4, true)            // the second-order role (kKktB2Role)
#define QPX_FORMS_POLISH_TILE(X) X(1, 1, false) X(2, 1, false) X(4, 1, false) X(4, 4, true) X(7, 4, true)
// the range role of the loop (kIpmRangeRole): the forms the default dispatch picks, f64 -- (tile rows, waves, slots, chain) / (blocks, slots)
#define QPX_FORMS_IPM_RANGE_TILE(X)                                                                              \
    X(1, 1, 1, false) X(1, 1, 2, false) X(1, 1, 4, false) X(2, 1, 1, false) X(2, 1, 2, false) X(2, 1, 4, false)  \
    X(4, 1, 1, false) X(4, 1, 2, false) X(4, 1, 4, false)                                                        \
    X(7, 4, 2, true) X(7, 4, 4, true) X(4, 4, 1, true) X(4, 4, 2, true) X(4, 4, 4, true)
#define QPX_FORMS_IPM_RANGE_GRID(X) X(10, 4) X(13, 4)
// ... and of the backward (kKktRangeRole): the tile forms of the second-order role (the default dispatch's), every thread-grid form
#define QPX_FORMS_KKT_RANGE_TILE(X) QPX_FORMS_KKT_B2_TILE(X)
#define QPX_FORMS_PREFAC_TILE(X) X(4, false) X(7, false) X(4, true) X(7, true)    // (tile rows of nz + neq, with equalities)
