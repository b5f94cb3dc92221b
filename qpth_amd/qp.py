"""The autograd surface of the reference, unchanged: qpth/qp.py:13-183.

    QPFunction(eps=1e-12, verbose=0, notImprovedLim=3, maxIter=20,
               solver=QPSolvers.PDIPM_BATCHED, check_Q_spd=True)(Q, p, G, h, A, b) -> zhat (nBatch, nz)

solves a batch of QPs  z* = argmin 1/2 z'Qz + p'z  s.t. Gz <= h, Az = b  and is differentiable
in all six parameters.  Any subset of the parameters may be un-batched; an empty tensor
means "no such constraint" (qp.py:58-61).  The forward runs two HIP kernels
(pre_factor_kkt, PDIPM loop), the backward one (factor_kkt + solve_kkt + gradient outer
products); state crosses from forward to backward on ctx exactly as in the reference.
Forward mode (torch.autograd.forward_ad, which the reference does not support) is one more launch: QPFunctionFn.jvp solves
the backward's KKT system with the right-hand side formed from the input tangents (qpx_jvp).
QPFunction(duals=True) also returns the multipliers, differentiable in both modes: (zhat, nu, lam, slacks).
QPFunction(warm_start=ws) starts the loop at the previous call's (lam, slacks) kept in a qpth_amd.WarmStart.
QPFunction(...)(Q, p, G, h, A, b, rho) softens rows of G z <= h by a quadratic penalty, differentiable in rho too.
The backward is itself differentiable once: torch.autograd.grad(..., create_graph=True) and a second grad give Hessian-vector
products through the layer, one more launch with one factorisation and two solves (qpx_backward2).
QPFunction(...)(Q, p, G, h, A, b, kappa=kappa) returns the point of the CENTRAL PATH at kappa instead of the solution -- the
log-barrier smoothing of the QP, C-infinity in all parameters and in kappa; one more launch in the forward (qpx_centre).
QPFunction(...)(Q, p, G, h, A, b, lower=l) solves  l <= Gz <= h  in nineq rows -- not [G; -G] z <= [h; -l] in 2 nineq --, differentiable
in l as well: the loop's and the backward's range role, the same number of launches (qpx_ipm_range).
QPFunction(warm_start=rws)(Q, p, G, h, A, b, lower=l) with a qpth_amd.RangeWarmStart starts that loop at the previous call's
(lam, slacks, lam_lo, slacks_lo) (qpx_ipm_range_warm).
QPFunction(...)(Q, p, G, h, A, b, rho, l1=gamma) makes the rows ELASTIC: the exact penalty gamma't + 1/2 t'diag(rho)t on the violations
t >= 0 of Gz <= h + t, in nineq rows and nz variables -- not the augmented dense QP in (z, t) --, differentiable in gamma and rho:
the loop's elastic role on the hard QP's factors, the backward as it stands (qpx_ipm_elastic).
QPFunction(...)(Q, p, G, h, A, b, soft_range=SoftRange(lower, l1, rho)) composes the two: l - tl <= Gz <= h + tu with a penalty on
each side's violation, every row choosing its own kind, in nineq rows and nz variables -- not the augmented dense QP in (z, tu, tl)
with 4 nineq rows --, differentiable in the five fields: the loop's soft-range role, the range role's backward (qpx_ipm_soft_range,
DESIGN 4.13).
QPFunction(scenarios=K)(Q, p, G, h, A, b) solves every (Q, G, A) for K vectors (p, h, b) -- perturbed optimisers, scenario MPC,
sweeps -- with ONE factorisation per (Q, G, A) and the matrices' gradients summed per group on the matrix cores; the call
equals the existing one on the expanded batch (qpx_ipm_group).
"""
from enum import Enum

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from .kkt import KKTFactors, RangeWarmStart, SoftRange, _reduce_like, _rows, as_kappa, as_l1, as_lower, as_rho
from .solvers.pdipm import batch as pdipm_b
from .util import expandParam, extract_nBatch


class QPSolvers(Enum):
    PDIPM_BATCHED = 1
    CVXPY = 2


def _print_trace(res):
    tr = res.trace.cpu()
    iters = res.iters.cpu()
    for i in range(int(iters.max().item())):
        row = tr[i][iters > i]
        print('iter: {}, pri_resid: {:.5e}, dual_resid: {:.5e}, mu: {:.5e}'.format(
            i, row[:, 0].mean(), row[:, 1].mean(), row[:, 2].mean()))


def _nbatch(params, extras=()):
    """nBatch of a call: the six parameters' (extract_nBatch) or that of an extra input given per QP, (nBatch, nineq)"""
    nBatch = extract_nBatch(*params)
    for X in extras:
        if X is not None and X.dim() == 2:
            nBatch = max(nBatch, X.size(0))
    return nBatch


def _expand_params(params, nBatch):
    """-> (the six parameters broadcast over the batch, for each whether the batch shares it): expandParam of each"""
    Q, p, G, h, A, b = params
    Q, sQ = expandParam(Q, nBatch, 3)
    p, sp = expandParam(p, nBatch, 2)
    G, sG = expandParam(G, nBatch, 3)
    h, sh = expandParam(h, nBatch, 2)
    A, sA = expandParam(A, nBatch, 3)
    b, sb = expandParam(b, nBatch, 2)
    return (Q, p, G, h, A, b), (sQ, sp, sG, sh, sA, sb)


def _shared_flags(params):
    """for each of the six parameters as the caller gave them: does the batch share it (what expandParam answers, no views made)"""
    Q, p, G, h, A, b = params
    return (Q.dim() == 2 and Q.nelement() > 0, p.dim() == 1 and p.nelement() > 0, G.dim() == 2 and G.nelement() > 0,
            h.dim() == 1 and h.nelement() > 0, A.dim() == 2 and A.nelement() > 0, b.dim() == 1 and b.nelement() > 0)


def _neq_of(A):
    return A.size(-2) if A.nelement() > 0 else 0


def _without_A_b(grads, neq):
    """no equality constraints: no gradients for A and b"""
    return grads[:4] + (None, None) + grads[6:] if neq == 0 else grads


def _hard_factors(ctx, six, extras):
    """What the forwards of the three row-role nodes begin with: nBatch (an extra input given per QP counts), the six
    parameters broadcast over it, ctx.neq, and the factors of the HARD QP.  -> (nBatch, p, h, b, fac)"""
    nBatch = _nbatch(six, extras)
    (Q, p, G, h, A, b), _ = _expand_params(six, nBatch)
    ctx.neq = _neq_of(six[4])
    return nBatch, p, h, b, KKTFactors.build(Q, G, A, nBatch)


def _loop_epilogue(fac, res, check_Q_spd, verbose, inaccurate=True):
    """behind the launches of a forward: one small read-back -- the reference raises here too (qp.py:81-85, batch.py:379-386),
    and so does a bad entry of a row kind's extra inputs --, the trace, and the reference's warning (batch.py:141-142,205-206;
    `inaccurate`: the barrier-smoothed call has a check of its own instead)"""
    fac.raise_on_failure(check_Q_spd)
    if verbose == 1:
        _print_trace(res)
    if inaccurate and verbose >= 0 and not bool((res.best_resid <= 1.).all().item()):
        print(pdipm_b.INACC_ERR)


def _mark_duals(ctx, neq, nus, slacks):
    """duals=True: an output the loss does not use hands backward None instead of a tensor of zeros; slacks (and nu without
    equality constraints) are no differentiable outputs"""
    ctx.set_materialize_grads(False)
    if neq == 0:
        ctx.mark_non_differentiable(slacks, nus)
    else:
        ctx.mark_non_differentiable(slacks)


# The row kinds behind QPFunction's extra inputs.  kind: (label, way out, what exists in float64 arithmetic only, qpx_*_supported,
# refusals in the order they are checked).  A refusal: (the extra input or the option of the call that the kind does not combine
# with, the text of the message between label and way out).
_WITH_RHO = " together with rho (soft rows) is not served"
_WITH_KAPPA = " together with kappa (the barrier-smoothed QP) is not served"
_WITH_LOWER = " together with lower (two-sided rows) is not served"
_IN_HOLDER = " together with %s is not served: the SoftRange holder carries the bounds and penalties"
_DUALS = " with duals=True is not served (the multipliers are no outputs of this node)"
_WARM = " with warm_start is not served"
_WARM_ONE_SIDED = (" with warm_start=WarmStart() is not served: that holder has nothing for the lower side (pass a "
                   "qpth_amd.RangeWarmStart to warm-start this call)")
_REFINE = " with refine=%(refine)d is not served: pass refine=0 or refine=None"
_SOLVER = " is served by solver=QPSolvers.PDIPM_BATCHED only"
_ROW_KINDS = {
    "soft_range": ("qpth_amd: soft_range (soft two-sided rows)", "; write the augmented dense QP in (z, tu, tl) instead",
                   "soft-range role", "qpx_soft_range_supported",
                   (("rho", _IN_HOLDER % "rho"), ("kappa", _IN_HOLDER % "kappa"), ("lower", _IN_HOLDER % "lower"),
                    ("l1", _IN_HOLDER % "l1"), ("duals", _DUALS), ("warm_start", _WARM), ("refine", _REFINE), ("solver", _SOLVER))),
    "l1": ("qpth_amd: l1 (elastic rows)", "; write the augmented dense QP in (z, t) instead", "elastic role", "qpx_elastic_supported",
           (("kappa", _WITH_KAPPA), ("lower", _WITH_LOWER), ("warm_start", _WARM), ("refine", _REFINE), ("solver", _SOLVER))),
    "lower": ("qpth_amd: lower (two-sided rows)", "; write the rows as [G; -G] z <= [h; -lower] instead", "range role",
              "qpx_range_supported",
              (("rho", _WITH_RHO), ("kappa", _WITH_KAPPA), ("solver", _SOLVER), ("refine", _REFINE), ("duals", _DUALS),
               ("warm_start", _WARM_ONE_SIDED))),
    "kappa": ("qpth_amd: kappa (the barrier-smoothed QP)", "", "centring kernel", "qpx_centre_supported",
              (("rho", _WITH_RHO + ": the centring steps evaluate the residuals of the hard QP"), ("solver", _SOLVER),
               ("refine", " with refine=%(refine)d: the centring launch already iterates on the residuals of the caller's data; "
                          "pass refine=0 or refine=None"))),
}


_EXTRA_INPUTS = ("rho", "kappa", "lower", "l1")
_OPTIONS = ("duals", "warm_start", "refine", "solver")
assert all(name in _EXTRA_INPUTS + _OPTIONS for kind in _ROW_KINDS.values() for name, _ in kind[4])


def f64_arithmetic_serves(nz, nineq, neq, lib=None):
    """Sizes at which a float32 QP is solved in float64 ARITHMETIC (QPX_F32_WIDE, include/qpx.h: float32 tensors on the
    caller's side, float64 factors and arithmetic in the kernels, which widen on load and narrow on store): wherever
    the float64 matrix-core kernels serve the size -- the tile kernels (nineq <= 112, nz+neq+nineq <= 208) and, since
    round 4, the large-QP family.  On MI355X the f64 matrix-core loop is faster than the f32 thread-grid loop plus its
    finishing iterations, and its answer is the float64 solution of the float32 data.  The library is the authority
    (qpx_supported); without one the tile-kernel rule is returned."""
    if lib is not None:
        return lib.dll.qpx_kernel_family(_lib.QPX_F32_WIDE, nz, nineq, neq) in (_lib.FAMILY_TILE, _lib.FAMILY_BIG)
    return nineq <= 112 and nz + neq + nineq <= 208


def QPFunction(eps=1e-12, verbose=0, notImprovedLim=3,
               maxIter=20, solver=QPSolvers.PDIPM_BATCHED,
               check_Q_spd=True, refine=None, duals=False, warm_start=None, kappa_tol=1e-9, kappa_steps=20, scenarios=None):
    """Returns f(Q, p, G, h, A, b, rho=None, kappa=None, lower=None, l1=None, soft_range=None).  `refine`, `duals`, `warm_start`,
    `scenarios` and the inputs `rho`, `kappa`, `lower`, `l1` and `soft_range` are what the reference does not have.
    scenarios=K: a GROUPED batch -- B different (Q, G, A), each solved for K vectors (p, h, b): K noisy copies of
      p (perturbed optimisers, randomised smoothing), K disturbance realisations in h, b (scenario / robust MPC), sweeps and
      multi-starts.  Q, G, A: batched (B, ., .) or un-batched; p, h, b each (B, K, .), (B, .) (shared by that QP's K
      scenarios) or (.) (shared by all); the outputs are (B, K, .).  The call EQUALS the existing call on the expanded batch of
      B K QPs -- a batched X as X.repeat_interleave(K, 0), an un-batched X as itself, p, h, b flattened to (B K, .) -- in its
      values (the forward bit for bit), in every gradient convention (a batched matrix gets the sum over its K scenarios, a
      (B, .) vector likewise, an un-batched parameter the `.mean(0)` over all B K QPs) and in its errors (a bad Q in one
      group raises as the expanded call does).  What it saves: K - 1 of every K pre-factorisations and factor blobs, and the
      B K outer products per matrix gradient that autograd would add up again -- one contraction per group instead.
      duals=True is served, in reverse mode.  Where the kernels cannot share a blob (qpx_group_supported is 0: the large-QP
      family, nz + neq + nineq > 208) and for float32 inputs that run with finishing steps, the call builds the expanded
      batch itself: scenarios= works at every size, there only without the saving.  With Q, G, A all un-batched it is the
      existing one-blob path on B K QPs.  Not together with rho, kappa, lower, l1, soft_range, warm_start, refine > 0 or
      solver=QPSolvers.CVXPY: each a ValueError that names the expanded call as the way out.  Forward mode and
      create_graph=True: RuntimeError.  scenarios=None is the call as before: the same nodes and launches.
    soft_range: SOFT two-sided inequality rows, a qpth_amd.SoftRange(lower, l1, rho, l1_lower=None, rho_lower=None),
          min 1/2 z'Qz + p'z + sum_i ( l1_i tu_i + 1/2 rho_i tu_i^2 + l1_lower_i tl_i + 1/2 rho_lower_i tl_i^2 )
          s.t.  lower - tl <= Gz <= h + tu,  tu, tl >= 0,  Az = b:
      boxes, ranges and trust regions that may be violated at a price.  Each row decides its kind: lower_i = -inf makes it
      one-sided, l1 = +inf or rho = +inf on a side makes that side hard, so one call mixes hard, two-sided, elastic and
      soft two-sided rows.  The iterates, iteration counts and solution of the reference on the augmented QP in (z, tu, tl) --
      nz + 2 nineq variables, 4 nineq rows --, whose Newton system collapses to the nineq x nineq system the loop factors anyway,
      on the HARD QP's factors.  The fields: tensors of shape (nBatch, nineq), (nineq,) or (), or floats; lower < h strictly on
      every two-sided row, l1 >= 0, rho > 0 (the pure l1 penalty is not served); a bad entry raises ValueError from the
      forward.  Returns zhat; reverse mode gives gradients to the six parameters and to those of the five fields that are tensors
      requiring grad (un-batched ones reduced as l1 and rho are), exactly 0 on an absent or hard side.  float64 inputs at
      sizes the thread-grid / tile kernels serve (nz+neq+nineq <= 208) only; not together with rho, kappa, lower or l1 (the
      holder carries them), duals=True, warm_start, refine > 0, float32 inputs or an external solver: each a ValueError that
      names the augmented dense QP as the way out.  Forward mode and second derivatives: RuntimeError.  soft_range=None is the
      call as before: the same nodes and launches.
    l1: elastic inequality rows, together with rho,
          min 1/2 z'Qz + p'z + sum_i ( l1_i t_i + 1/2 rho_i t_i^2 )   s.t.  Gz <= h + t,  t >= 0,  Az = b,
      the EXACT penalty with a quadratic tail: where the hard QP is feasible and l1_i exceeds its multipliers the solution is the
      hard QP's with t = 0 exactly; elsewhere the QP stays feasible and the multipliers stay bounded (lam_i = l1_i + rho_i t_i on a
      violated row).  The iterates, iteration counts and solution of the reference on the augmented QP in (z, t) -- nz + nineq
      variables, 2 nineq rows --, whose Newton system collapses to the nineq x nineq system the loop factors anyway, on the HARD
      QP's factors.  l1 and rho: tensors of the other inputs' dtype and device, shape (nBatch, nineq), (nineq,) (shared by the
      batch) or () (one for every row), or Python floats; l1 >= 0, rho > 0, +inf in either = a hard row, so l1 = +inf everywhere
      is the six-input QP and l1 = 0 the soft rows of rho alone.  An l1 entry that is NaN or negative raises
      ValueError("l1 must be non-negative"), a rho entry that is NaN or not positive ValueError("rho must be positive"), from the
      forward.  l1 without rho raises ValueError: rho is the penalty's curvature, and the pure l1 penalty (rho = 0, a singular
      augmented Q) is not served.  Both are differentiable inputs, the seventh and eighth, in reverse and in forward mode
      (d loss / d l1 = dz / (dt + rho), d loss / d rho = t d loss / d l1 with dz the inequality block of the backward's KKT
      solution and dt = lam_t / s_t of the rows t >= 0: exactly 0 on a hard row); a shared one gets the `.mean(0)` convention,
      a scalar is summed over the rows as well.  duals=True returns (zhat, nu, lam, slacks), slacks = h + t - G zhat, as for the
      hard QP.  float64 inputs at sizes the thread-grid / tile kernels serve (nz+neq+nineq <= 208) only; not together with
      kappa, lower, warm_start, refine > 0, float32 inputs or solver=QPSolvers.CVXPY: each a ValueError from the call that names
      the augmented dense QP as the way out.  Second derivatives are not served: RuntimeError from the second grad.  l1=None is
      the call as before: the same nodes and launches.
    lower: two-sided inequality rows,
          min 1/2 z'Qz + p'z   s.t.  lower <= Gz <= h,  Az = b,
      box and range constraints in nineq rows: the iterates, iteration counts and solution of the reference on the doubled QP
      [G; -G] z <= [h; -lower], whose Newton system collapses to the nineq x nineq system the loop factors anyway -- the kernels'
      cost is cubic in the rows, and a doubled box on 100 variables leaves the register-resident kernels altogether.  A tensor
      of the other inputs' dtype and device, shape (nBatch, nineq) or (nineq,) (shared by the batch); -inf = a one-sided row,
      so lower = -inf everywhere is the six-input QP.  A seventh differentiable input in reverse mode (d loss / d lower is
      exactly 0 on a one-sided row); a shared lower gets the `.mean(0)` convention.  An entry that is NaN, +inf or not below
      its h raises ValueError("lower must be below h") from the forward.  float64 inputs at sizes the thread-grid / tile
      kernels serve (nz+neq+nineq <= 208) only; not together with rho, kappa, refine > 0, duals=True, a plain WarmStart, float32
      inputs or solver=QPSolvers.CVXPY: each a ValueError from the call that names the doubled call as the way out.  Forward
      mode and second derivatives are not served: RuntimeError.  lower=None is the call as before: the same nodes and launches.
      warm_start=qpth_amd.RangeWarmStart(), the SAME object on every step: the first call is cold, every later
      one enters the loop at the previous call's (lam, slacks, lam_lo, slacks_lo), floored at its `floor`; `used`, a holder of
      another batch and `clear()` as for WarmStart below.  A QP in which a row that was one-sided in the previous call is
      two-sided now starts cold.  The solution and the backward are those of the cold call to the solver's tolerance.  That
      holder without lower, or with rho, kappa, l1 or soft_range: ValueError.  After a LARGE step (0.1 on the box of the
      headline shape) a warm start can cost more passes than the start point, or stall: clear the holder then.
    kappa: the barrier-smoothed QP.  The call returns the point of the central path
          Q z + p + G'lam + A'nu = 0,  G z + s = h,  A z = b,  s_i lam_i = kappa_i   (s, lam > 0),
      the minimiser of 1/2 z'Qz + p'z - sum_i kappa_i log(h_i - g_i'z) s.t. Az = b, instead of the QP's solution: smooth in all
      parameters (no kinks, strict complementarity by construction, d = lam / s = kappa / s^2 well conditioned), and kappa -> 0
      recovers the hard QP.  A tensor of the other inputs' dtype and device, shape (nBatch, nineq), (nineq,) (shared by the
      batch) or () (one weight for every row), or a Python float; every entry finite and > 0, else ValueError("kappa must be
      positive") from the forward.  The forward is pre-factorisation, the PDIPM loop and one centring launch (Newton steps
      until max(|rx|, |rz|, |ry|, |s lam - kappa| / kappa) <= kappa_tol in max norms, kappa_steps at most; a QP that ends
      above kappa_tol prints one warning line when verbose >= 0).  With a Python float the loop runs to the tolerance
      max(eps, nineq * kappa) -- it stops about where mu reaches kappa, fewer iterations than the hard call; with a tensor it
      runs to the caller's eps: pass eps = nineq * kappa.min() to save those iterations.  kappa is a seventh differentiable
      input in reverse and in forward mode (d loss / d kappa_i = dz_i / lam_i, dz the inequality block of the backward's KKT
      solution); a shared kappa gets the `.mean(0)` convention, a scalar is summed over the rows as well.  duals=True,
      warm_start (the holder takes the centred lam, slacks) and second derivatives through create_graph=True work as for
      the hard QP -- with respect to the six parameters and the cotangents; the second-order gradient with respect to kappa
      itself is not offered (None), and the first-order gradient of kappa carries no graph.  float64 inputs at sizes the
      thread-grid / tile kernels serve (nz+neq+nineq <= 208) only; not together with rho, refine > 0, float32 inputs or
      solver=QPSolvers.CVXPY: each a ValueError from the call.  kappa=None is the call as before: the same nodes and launches.
    Second derivatives: under torch.autograd.grad(..., create_graph=True) the gradients carry a graph, and a second
      grad -- Hessian-vector products, gradient penalties, losses on -dE/dx, MAML-style outer loops -- runs the second-order
      pass: gradients flow to the first backward's cotangents (dl/dzhat, and dl/dlam, dl/dnu under duals=True) and to Q, p,
      G, h, A, b, un-batched parameters included.  They exist only under STRICT COMPLEMENTARITY: at a solution with a row
      where lam_i = s_i = 0 the solution map has a kink and the value returned is a one-sided one; rows with max(lam_i, s_i)
      below ~1e-3 already make it ill-conditioned.  Not served, each a RuntimeError from the second grad: soft rows (rho),
      refine > 0 (float32 inputs at sizes the float64 kernels do not serve run with refine=2 by default: pass refine=0), the
      external-solver path; and third derivatives (the second-order pass is once differentiable).  Without create_graph
      nothing changes: the same launches in the same order.
    rho: soft inequality rows,
          min 1/2 z'Qz + p'z + 1/2 sum_i rho_i t_i^2   s.t.  Gz <= h + t,  Az = b,
      solved in the kernels of the hard QP of the same (nz, nineq, neq) -- no augmented variables.  A tensor of the other
      inputs' dtype and device, shape (nBatch, nineq), (nineq,) (shared by the batch) or () (one penalty for every row), or
      a Python float; every entry > 0, +inf = a hard row.  A seventh differentiable input, in reverse and in forward mode;
      a shared rho gets the `.mean(0)` convention of the other shared parameters, a scalar is summed over the rows as
      well.  The violation is t = lam / rho, the returned slacks are h + t - G zhat.  Not with solver=QPSolvers.CVXPY and
      not with refine > 0 (both raise ValueError); a rho <= 0 or NaN raises ValueError("rho must be positive") from the
      forward.  rho=None is the hard QP, the six-input node as before.
    warm_start: a qpth_amd.WarmStart, the SAME object on every step of a training loop.  The first call is cold (the holder
      is empty); every later call enters the PDIPM loop at the previous call's (lam, slacks), floored at `ws.floor`, instead
      of the reference's start point, and needs about half the iterations while the parameters move by small steps (DESIGN
      4.7).  The holder then takes this call's lam, slacks (references, detached) and `ws.used`, int32 (nBatch,): 1 where the
      loop took the warm entry.  A holder of another (nBatch, nineq), dtype or device is ignored -- that call is cold -- and
      overwritten; sizes of the large-QP family (nz+neq+nineq > 208) always start cold (`ws.used` zeros).  The solution,
      backward, jvp and duals=True are those of the cold call to the solver's tolerance: they read the solution only.  The
      external-solver path (solver=QPSolvers.CVXPY) ignores the holder.  Under qpth_amd.dist.solve_sharded each rank's holder
      sees its own slice.
    duals=True: the call returns (zhat, nu, lam, slacks) -- the reference forward's order (batch.py:47-207) -- instead of
      zhat alone.  zhat, lam (nBatch, nineq) and nu (nBatch, neq) are differentiable in all six parameters, in reverse and in
      forward mode: a loss l(zhat, lam, nu) back-propagates through the same single backward launch, its KKT right-hand side
      (dl/dzhat, 0, dl/dlam, dl/dnu) (qpx_backward_duals).  slacks is returned NON-differentiable (a cotangent on
      it is numerically poor in this formulation, DESIGN 4.5: write h - G zhat where gradients through the slacks are
      needed); without equality constraints nu is an empty (nBatch, 0) tensor, non-differentiable too.  An output the loss
      does not use costs nothing: its cotangent reaches the kernel as NULL, not as zeros.
    `refine`, for float32 inputs:
      None (automatic) -- sizes the float64 tile kernels serve (f64_arithmetic_serves): the float64 kernels run on the
            float32 tensors (they widen on load and narrow results and gradients on store; the factors between
            forward and backward are float64); other sizes: as refine=2;
      0  -- the pure float32 kernels, nothing else (fastest at some sizes; the pre-computed products R = G Q^-1 G^T
            carry ~1e-2 relative error in float32 on the benchmark generator, so the loop kernel alone lands 20x
            further from the float64 answer than the reference's float32 run does);
      k > 0 -- the float32 kernels + k finishing Newton steps on the residuals of the ORIGINAL problem data
            (KKTFactors.polish -- the reference's KKTSolvers.IR_UNOPT idea, batch.py:244-270; each with one
            in-kernel refinement step per KKT solve, also applied to the backward solve).
    float64 inputs: None = 0.
    Memory: with refine=None a float32 batch in the large-QP family keeps a float64 factor blob (9.4 MB per QP at
    nz = nineq = 500, twice the float32 family's); a batch that only fits HBM with float32 factors should pass refine=2
    (float32 kernels + finishing iterations) or refine=0 explicitly."""
    def _forward(ctx, Q_, p_, G_, h_, A_, b_, rho_=None, kappa_=None, loop_eps=None):
        nBatch = _nbatch((Q_, p_, G_, h_, A_, b_), (rho_, kappa_))
        nineq, nz = G_.size(-2), G_.size(-1)
        neq = _neq_of(A_)
        # float32 data, float64 arithmetic (see QPFunction.__doc__)
        ctx.wide = (solver == QPSolvers.PDIPM_BATCHED and refine is None and Q_.dtype == torch.float32
                    and f64_arithmetic_serves(nz, nineq, neq, _lib.backend_for(Q_)))
        (Q, p, G, h, A, b), _ = _expand_params((Q_, p_, G_, h_, A_, b_), nBatch)

        assert(neq > 0 or nineq > 0)
        ctx.neq, ctx.nineq, ctx.nz = neq, nineq, nz

        if rho_ is not None:
            # soft rows: w = 1 / rho (0 = hard, rho = inf) into the pre-factorisation; ctx keeps rho as (nBatch | 1, nineq)
            if Q_.dtype == torch.float32 and refine is None and not ctx.wide:
                raise ValueError("qpth_amd: rho with float32 inputs at nz = %d, nineq = %d, neq = %d, where the float32 "
                                 "kernels would run with finishing steps on the residuals of the hard QP; pass refine=0 "
                                 "(or float64 inputs)" % (nz, nineq, neq))
            ctx.rho = _rows(rho_, nineq)
            w = ctx.rho.reciprocal()
        else:
            w = None

        if solver == QPSolvers.PDIPM_BATCHED:
            fac = KKTFactors.build(Q, G, A, nBatch, wide=ctx.wide, w=w)   # qp.py:93
            warm = warm_start.pair(nBatch, nineq, Q.dtype, Q.device) if warm_start is not None else None
            res = fac.ipm(p, h, b, eps if loop_eps is None else loop_eps, maxIter, notImprovedLim,
                          want_trace=(verbose == 1), warm=warm,
                          warm_floor=warm_start.floor if warm is not None else 1e-2)   # qp.py:94-96
            ctx.refine = (2 if Q.dtype == torch.float32 and not ctx.wide else 0) if refine is None else int(refine)
            if kappa_ is not None:
                # the smoothed QP: from the loop's iterate onto the central path at kappa, one more launch; ctx
                # keeps nothing of kappa but its rank: the derivatives read the centred (lam, slacks)
                res = fac.centre(p, h, b, res, _rows(kappa_, nineq), tol=kappa_tol, max_steps=kappa_steps)
            if ctx.refine > 0:
                # (the solves inside a finishing step are NOT refined: the step's own residuals are exact, and refining
                # the directions as well changes nothing in the answer -- C2 / C3 float32, two steps: the same error
                # distribution to three digits -- for 40 % more time per step; profiles/archive/r04f)
                res = fac.polish(p, h, b, res, steps=ctx.refine, refine=0)
            if warm_start is not None:
                warm_start.take(res)
            _loop_epilogue(fac, res, check_Q_spd, verbose, inaccurate=kappa_ is None)
            if kappa_ is not None:
                # one small read-back: a QP the kernel left untouched (resid = inf after 0 steps) had a bad kappa entry
                bad = ((res.centre_steps == 0) & torch.isinf(res.centre_resid)).any()
                off = ((res.status & _lib.ST_NOT_CENTRED) != 0).any()
                bad, off = torch.stack([bad, off]).tolist()
                if bad:
                    raise ValueError("kappa must be positive")
                if off and verbose >= 0:
                    print("qpth_amd warning: centring ended above kappa_tol = %g for some QPs (worst residual %.3e after at most "
                          "%d steps); raise kappa_steps" % (kappa_tol, float(res.centre_resid.max().item()), kappa_steps))
            ctx.fac = fac
            zhats, ctx.nus, ctx.lams, ctx.slacks = res.zhat, res.nu, res.lam, res.slacks
        elif solver == QPSolvers.CVXPY:
            # forward by an external CPU solver, backward by the HIP kernels (qp.py:97-120,142-143)
            from .solvers import external
            zhats, ctx.nus, ctx.lams, ctx.slacks = external.forward_batch(Q, p, G, h, A, b, neq)
            ctx.fac = None
            ctx.refine = 0 if refine is None else int(refine)
        else:
            assert False

        # (rho among the saved tensors: backward reads it there, under autograd's check for in-place changes; forward mode,
        # which runs inside this very call, reads ctx.rho)
        ctx.save_for_backward(zhats, Q_, p_, G_, h_, A_, b_, *(() if rho_ is None else (rho_,)))
        ctx.rho_dim = None if rho_ is None else rho_.dim()
        ctx.kappa_dim = None if kappa_ is None else kappa_.dim()
        # forward mode reads no saved_tensors: zhat as an attribute beside lam, s, nu (detached: no cycle through the
        # output's grad_fn), and on the external-solver path the matrices the factors are rebuilt from
        ctx.zhat = zhats.detach()
        ctx.QGA = (Q.detach(), G.detach(), A.detach(), nBatch) if ctx.fac is None else None
        if not duals:
            return zhats
        # the multipliers as outputs: ctx keeps detached aliases (no cycle through the outputs' grad_fn)
        nus, lams, slacks = ctx.nus, ctx.lams, ctx.slacks
        ctx.nus, ctx.lams, ctx.slacks = nus.detach(), lams.detach(), slacks.detach()
        _mark_duals(ctx, neq, nus, slacks)
        return zhats, nus, lams, slacks

    def _jvp(ctx, dQ, dp, dG, dh, dA, db, drho=None, dkappa=None):
        # forward mode: z' solves the backward's KKT system (same d, same factors) with the right-hand side formed from
        # the tangents on the device -- one launch, no host sync.  A None / empty tangent is zero.
        fac = ctx.fac
        if fac is None:                                          # external solver: the factors as backward builds them
            Q, G, A, nBatch = ctx.QGA
            fac = KKTFactors.build(Q, G, A, nBatch)
            fac.raise_on_failure(check_Q_spd)
        rf = 1 if (ctx.refine > 0 and fac.refine_ok) else 0
        if drho is not None:
            # w = 1 / rho enters the KKT rows like h times lam (G z - w lam + s = h): th + tw lam, tw = -trho / rho^2
            tw = -drho / (ctx.rho * ctx.rho)
            dh = tw * ctx.lams if dh is None else dh + tw * ctx.lams
        if dkappa is not None:
            # s lam = kappa linearised, divided by lam: the tangent of kappa enters the rows G z + s = h like -tkappa / lam on h
            th = -dkappa / ctx.lams
            dh = th if dh is None else dh + th
        if not duals:
            return fac.jvp(ctx.zhat, ctx.lams, ctx.slacks, ctx.nus, (dQ, dp, dG, dh, dA, db), refine=rf)
        # (z', nu', lam') from the same single launch; the slacks carry no tangent (non-differentiable)
        zt, lt, nt = fac.jvp(ctx.zhat, ctx.lams, ctx.slacks, ctx.nus, (dQ, dp, dG, dh, dA, db), refine=rf, want_duals=True)
        return zt, nt, lt, None

    class QPBackwardFn(Function):
        """The first backward as a node of its own: _backward goes through it when it runs with grad mode on, i.e. under
        torch.autograd.grad(..., create_graph=True), so that its gradients carry a graph.  forward is the launch _backward
        makes otherwise and also keeps the solution (dx, dz, dy) of the backward KKT system; backward is the second-order
        pass (KKTFactors.backward2): gradients flow to the incoming cotangents and to the six parameters.  It is
        once differentiable: third derivatives are not offered."""
        @staticmethod
        def forward(c, st, dl_dzhat, dl_dlam, dl_dnu, Q_, p_, G_, h_, A_, b_):
            out = st["fac"].backward(st["zhat"], st["lams"], st["slacks"], st["nus"], dl_dzhat, want=st["want"],
                                     shared=st["shared"], refine=st["refine"], dl_dlam=dl_dlam, dl_dnu=dl_dnu,
                                     want_dz=st["want_rho"], want_sol=True)
            c.st, c.sol = st, out[-1]
            c.set_materialize_grads(False)
            return out[:-1]

        @staticmethod
        @once_differentiable
        def backward(c, *W):
            st = c.st
            if st["unserved"]:
                raise RuntimeError("qpth_amd: second derivatives (create_graph=True) are not served %s" % st["unserved"])
            W, shared, nB = W[:6], st["shared"], st["nBatch"]
            if all(w is None for w in W):
                return (None,) * 10
            # a parameter the batch shares got the batch MEAN of its per-QP gradients: the per-QP cotangent is W / nBatch, and
            # its second-order gradient the SUM over the batch of the per-QP results
            Wq = [None if w is None else (w / nB if sh else w) for w, sh in zip(W, shared)]
            need = c.needs_input_grad
            (zd, ld, nd), H = st["fac"].backward2(st["zhat"], st["lams"], st["slacks"], st["nus"], c.sol, Wq, want=need[4:10])
            H = [None if x is None else (x.sum(0) if sh else x) for x, sh in zip(H, shared)]
            return (None, zd if need[1] else None, ld if need[2] else None, nd if need[3] else None) + tuple(H)

    def _backward(ctx, dl_dzhat, dl_dnu=None, dl_dlam=None, dl_dslacks=None):
        saved = ctx.saved_tensors
        zhats, leaves = saved[0], saved[1:7]
        nBatch = extract_nBatch(*leaves)
        shared = _shared_flags(leaves)
        neq = ctx.neq
        soft = ctx.rho_dim is not None
        smooth = ctx.kappa_dim is not None
        if dl_dzhat is None and dl_dlam is None and (dl_dnu is None or neq == 0):
            return (None,) * (7 if soft else 8 if smooth else 6)     # duals=True and no cotangent on any differentiable output

        fac = ctx.fac
        if fac is None:                                          # qp.py:142-143
            (Q, _, G, _, A, _), _ = _expand_params(leaves, nBatch)
            fac = KKTFactors.build(Q, G, A, nBatch)
            fac.raise_on_failure(check_Q_spd)

        # d = clamp(lams)/clamp(slacks), factor_kkt, solve_kkt(dl_dzhat, 0, 0, 0) -- with duals=True
        # solve_kkt(dl_dzhat, 0, dl_dlam, dl_dnu), each None where the loss does not use that output -- and the outer
        # products (qp.py:148-173) happen inside one kernel.  Only the gradients autograd asks for are
        # formed (ctx.needs_input_grad), and the `.mean(0)` of a parameter the batch shares
        # (qp.py:159-177) is taken inside KKTFactors.backward -- for Q, G, A as one contraction over
        # the batch instead of nBatch outer products.
        want = tuple(ctx.needs_input_grad[:6])
        want_rho = (soft or smooth) and ctx.needs_input_grad[6]     # (rho's gradient or kappa's: both read dz of the KKT solution)
        if torch.is_grad_enabled():
            # create_graph=True: the same launch inside a node whose backward is the second-order pass
            unserved = ("with soft rows (rho)" if soft else "with refine > 0 (refine=%d here)" % ctx.refine if ctx.refine > 0
                        else "on the external-solver path" if ctx.fac is None else None)
            st = dict(fac=fac, zhat=zhats.detach(), lams=ctx.lams, slacks=ctx.slacks, nus=ctx.nus, want=want,
                      shared=shared, refine=1 if (ctx.refine > 0 and fac.refine_ok) else 0,
                      want_rho=want_rho, nBatch=nBatch, unserved=unserved)
            grads = QPBackwardFn.apply(st, dl_dzhat, dl_dlam, dl_dnu if neq > 0 else None, *leaves)
        else:
            grads = fac.backward(zhats, ctx.lams, ctx.slacks, ctx.nus, dl_dzhat, want=want, shared=shared,
                                 refine=1 if (ctx.refine > 0 and fac.refine_ok) else 0,
                                 dl_dlam=dl_dlam, dl_dnu=dl_dnu if neq > 0 else None, want_dz=want_rho)
        if want_rho:
            grads, dz = grads[:6], grads[6]
        grads = _without_A_b(grads, neq)
        if smooth:
            dkappa = None
            if want_rho:
                # d loss / d kappa = dz / lam, reduced like drho; it carries no graph (second derivatives with respect
                # to kappa are not offered)
                dkappa = _reduce_like(dz.detach() / ctx.lams, ctx.kappa_dim)
            return grads + (dkappa, None)
        if not soft:
            return grads
        drho = None
        if want_rho:
            # dw = -dz lam, w = 1 / rho: drho = dz lam / rho^2 (0 on a hard row); shared: `.mean(0)`, a scalar summed over the rows
            rho = _rows(saved[7], ctx.nineq, detach=False)
            drho = _reduce_like(dz * ctx.lams / (rho * rho), ctx.rho_dim)
        return grads + (drho,)

    class QPFunctionFn(Function):
        @staticmethod
        def forward(ctx, Q_, p_, G_, h_, A_, b_):
            return _forward(ctx, Q_, p_, G_, h_, A_, b_)

        @staticmethod
        def jvp(ctx, dQ, dp, dG, dh, dA, db):
            return _jvp(ctx, dQ, dp, dG, dh, dA, db)

        @staticmethod
        def backward(ctx, dl_dzhat, dl_dnu=None, dl_dlam=None, dl_dslacks=None):
            return _backward(ctx, dl_dzhat, dl_dnu, dl_dlam, dl_dslacks)

    class QPSoftFunctionFn(Function):
        """the seven-input node: rho, the penalties of the soft rows, behind the six parameters"""
        @staticmethod
        def forward(ctx, Q_, p_, G_, h_, A_, b_, rho_):
            return _forward(ctx, Q_, p_, G_, h_, A_, b_, rho_)

        @staticmethod
        def jvp(ctx, dQ, dp, dG, dh, dA, db, drho):
            return _jvp(ctx, dQ, dp, dG, dh, dA, db, drho)

        @staticmethod
        def backward(ctx, dl_dzhat, dl_dnu=None, dl_dlam=None, dl_dslacks=None):
            return _backward(ctx, dl_dzhat, dl_dnu, dl_dlam, dl_dslacks)

    class QPSmoothFunctionFn(Function):
        """the node of the barrier-smoothed QP: kappa, the seventh differentiable input, behind the six parameters (and the loop's
        tolerance, a Python float or None, which is no tensor and gets no gradient)"""
        @staticmethod
        def forward(ctx, Q_, p_, G_, h_, A_, b_, kappa_, loop_eps):
            return _forward(ctx, Q_, p_, G_, h_, A_, b_, None, kappa_, loop_eps)

        @staticmethod
        def jvp(ctx, dQ, dp, dG, dh, dA, db, dkappa, _):
            return _jvp(ctx, dQ, dp, dG, dh, dA, db, None, dkappa)

        @staticmethod
        def backward(ctx, dl_dzhat, dl_dnu=None, dl_dlam=None, dl_dslacks=None):
            return _backward(ctx, dl_dzhat, dl_dnu, dl_dlam, dl_dslacks)

    class QPRangeFunctionFn(Function):
        """the node of two-sided rows: lower, the seventh differentiable input, behind the six parameters"""
        @staticmethod
        def forward(ctx, Q_, p_, G_, h_, A_, b_, lower_):
            nBatch, p, h, b, fac = _hard_factors(ctx, (Q_, p_, G_, h_, A_, b_), (lower_,))
            # (a RangeWarmStart: _gate let it through; the first call and a holder of another batch are cold)
            warm = warm_start.quad(nBatch, G_.size(-2), Q_.dtype, Q_.device) if warm_start is not None else None
            res = fac.ipm_range(p, h, lower_.detach(), b, eps, maxIter, notImprovedLim, want_trace=(verbose == 1), warm=warm,
                                warm_floor=warm_start.floor if warm is not None else 1e-2)
            if warm_start is not None:
                warm_start.take(res)
            _loop_epilogue(fac, res, check_Q_spd, verbose)
            ctx.fac = fac
            ctx.nus, ctx.lams, ctx.slacks, ctx.lams_lo, ctx.slacks_lo = res.nu, res.lam, res.slacks, res.lam_lo, res.slacks_lo
            ctx.save_for_backward(res.zhat, Q_, p_, G_, h_, A_, b_, lower_)
            return res.zhat

        @staticmethod
        def jvp(ctx, *tangents):
            raise RuntimeError("qpth_amd: forward mode is not served with two-sided rows (lower); write the rows as "
                               "[G; -G] z <= [h; -lower]")

        @staticmethod
        @once_differentiable
        def backward(ctx, dl_dzhat):
            zhats, *six, lower = ctx.saved_tensors
            grads = ctx.fac.backward_range(zhats, ctx.lams, ctx.slacks, ctx.lams_lo, ctx.slacks_lo, ctx.nus, dl_dzhat,
                                           want=tuple(ctx.needs_input_grad[:7]), shared=_shared_flags(six) + (lower.dim() == 1,))
            return _without_A_b(grads, ctx.neq)

    class QPElasticFunctionFn(Function):
        """the node of elastic rows: rho and l1, the seventh and eighth differentiable inputs, behind the six parameters (DESIGN
        4.12).  Forward: the hard QP's factors and the loop's elastic role; the derivatives run on the same factors, in the
        launches of the hard QP, given lam and the effective slack (KKTFactors.elastic_eff)."""
        @staticmethod
        def forward(ctx, Q_, p_, G_, h_, A_, b_, rho_, l1_):
            nineq = G_.size(-2)
            _, p, h, b, fac = _hard_factors(ctx, (Q_, p_, G_, h_, A_, b_), (rho_, l1_))
            gam, rho = _rows(l1_, nineq), _rows(rho_, nineq)
            res = fac.ipm_elastic(p, h, gam, rho, b, eps, maxIter, notImprovedLim, want_trace=(verbose == 1))
            _loop_epilogue(fac, res, check_Q_spd, verbose)
            ctx.fac = fac
            # a row is hard where either is +inf (the kernel's rule): rho = +inf there for the derivatives' formulas
            ctx.rho = torch.where(torch.isfinite(gam), rho, torch.full_like(rho, float("inf")))
            ctx.seff, ctx.dt = fac.elastic_eff(res.lam, res.slacks, res.lam_t, res.slacks_t, ctx.rho)
            ctx.t = res.t
            ctx.rho_dim, ctx.l1_dim = rho_.dim(), l1_.dim()
            ctx.zhat, ctx.nus, ctx.lams = res.zhat.detach(), res.nu.detach(), res.lam.detach()
            ctx.save_for_backward(Q_, p_, G_, h_, A_, b_, rho_, l1_)
            if not duals:
                return res.zhat
            _mark_duals(ctx, ctx.neq, res.nu, res.slacks)
            return res.zhat, res.nu, res.lam, res.slacks

        @staticmethod
        def jvp(ctx, dQ, dp, dG, dh, dA, db, drho, dl1):
            # the tangents of l1 and rho act on h: th -= (tl1 + t trho) / (dt + rho) (exactly nothing on a hard row)
            if drho is not None or dl1 is not None:
                th = (0 if dl1 is None else dl1) + (0 if drho is None else ctx.t * drho)
                th = -th / (ctx.dt + ctx.rho)
                dh = th if dh is None else dh + th
            if not duals:
                return ctx.fac.jvp(ctx.zhat, ctx.lams, ctx.seff, ctx.nus, (dQ, dp, dG, dh, dA, db))
            zt, lt, nt = ctx.fac.jvp(ctx.zhat, ctx.lams, ctx.seff, ctx.nus, (dQ, dp, dG, dh, dA, db), want_duals=True)
            return zt, nt, lt, None

        @staticmethod
        @once_differentiable
        def backward(ctx, dl_dzhat, dl_dnu=None, dl_dlam=None, dl_dslacks=None):
            neq = ctx.neq
            if dl_dzhat is None and dl_dlam is None and (dl_dnu is None or neq == 0):
                return (None,) * 8
            shared = _shared_flags(ctx.saved_tensors[:6])
            want_pen = ctx.needs_input_grad[6] or ctx.needs_input_grad[7]
            grads = ctx.fac.backward(ctx.zhat, ctx.lams, ctx.seff, ctx.nus, dl_dzhat, want=tuple(ctx.needs_input_grad[:6]),
                                     shared=shared, dl_dlam=dl_dlam, dl_dnu=dl_dnu if neq > 0 else None, want_dz=want_pen)
            drho = dl1 = None
            if want_pen:
                grads, dz = grads[:6], grads[6]
                # d loss / d l1 = dz / (dt + rho), d loss / d rho = t d loss / d l1; shared: `.mean(0)`, a scalar summed over the rows
                dgam = dz / (ctx.dt + ctx.rho)
                if ctx.needs_input_grad[7]:
                    dl1 = _reduce_like(dgam, ctx.l1_dim)
                if ctx.needs_input_grad[6]:
                    drho = _reduce_like(dgam * ctx.t, ctx.rho_dim)
            return _without_A_b(grads, neq) + (drho, dl1)

    class QPSoftRangeFunctionFn(Function):
        """the node of soft two-sided rows: lower, l1, rho, l1_lower, rho_lower behind the six parameters.  Forward:
        the hard QP's factors and the loop's soft-range role; backward: the range role's launch on the same factors with the
        effective slack of each side (KKTFactors.backward_soft_range)."""
        @staticmethod
        def forward(ctx, Q_, p_, G_, h_, A_, b_, *fields_):
            nineq = G_.size(-2)
            nBatch, p, h, b, fac = _hard_factors(ctx, (Q_, p_, G_, h_, A_, b_), fields_)
            lo, gu, ru, gl, rl = [_rows(X, nineq) for X in fields_]
            res = fac.ipm_soft_range(p, h, lo, gu, ru, gl, rl, b, eps, maxIter, notImprovedLim, want_trace=(verbose == 1))
            _loop_epilogue(fac, res, check_Q_spd, verbose)
            ctx.fac, ctx.res = fac, res
            # a side is hard where either of its penalties is +inf (the kernel's rule): rho = +inf there for the derivatives
            inf = torch.full((nBatch, nineq), float("inf"), dtype=Q_.dtype, device=Q_.device)
            ctx.rho_u = torch.where(torch.isfinite(gu), ru, inf)
            ctx.rho_l = torch.where(torch.isfinite(gl), rl, inf)
            ctx.dims = [X.dim() for X in fields_]
            ctx.save_for_backward(Q_, p_, G_, h_, A_, b_)
            return res.zhat

        @staticmethod
        def jvp(ctx, *tangents):
            raise RuntimeError("qpth_amd: forward mode is not served with soft two-sided rows (soft_range); write the augmented "
                               "dense QP in (z, tu, tl)")

        @staticmethod
        @once_differentiable
        def backward(ctx, dl_dzhat):
            grads = ctx.fac.backward_soft_range(ctx.res, ctx.rho_u, ctx.rho_l, dl_dzhat, want=tuple(ctx.needs_input_grad[:11]),
                                                shared=_shared_flags(ctx.saved_tensors))
            # an un-batched field: `.mean(0)`, a scalar summed over the rows as well (as l1 and rho of the elastic rows)
            five = tuple(None if g is None else _reduce_like(g, dim) for g, dim in zip(grads[6:], ctx.dims))
            return _without_A_b(grads[:6], ctx.neq) + five

    class QPScenarioFunctionFn(Function):
        """the node of a grouped batch (scenarios=K): Q_, G_, A_ as the caller gave them -- (B, ., .) or un-batched,
        at least one batched --, p_, h_, b_ flattened to (B K, .) or un-batched.  One blob per group; the loop and the backward
        run on B K QPs; a batched matrix's gradient comes back per group, summed over its scenarios."""
        @staticmethod
        def forward(ctx, Q_, p_, G_, h_, A_, b_):
            K = int(scenarios)
            B = max(X.size(0) for X in (Q_, G_, A_) if X.dim() == 3)
            nineq, nz, neq = G_.size(-2), G_.size(-1), _neq_of(A_)
            ctx.neq = neq
            wide = (refine is None and Q_.dtype == torch.float32
                    and f64_arithmetic_serves(nz, nineq, neq, _lib.backend_for(Q_)))
            fac = KKTFactors.build(Q_, G_, A_, B, wide=wide, scenarios=K)
            res = fac.ipm(p_, h_, b_, eps, maxIter, notImprovedLim, want_trace=(verbose == 1))
            _loop_epilogue(fac, res, check_Q_spd, verbose)
            ctx.fac = fac
            ctx.nus, ctx.lams, ctx.slacks = res.nu.detach(), res.lam.detach(), res.slacks.detach()
            ctx.save_for_backward(res.zhat, Q_, p_, G_, h_, A_, b_)
            if not duals:
                return res.zhat
            _mark_duals(ctx, neq, res.nu, res.slacks)
            return res.zhat, res.nu, res.lam, res.slacks

        @staticmethod
        def jvp(ctx, *tangents):
            raise RuntimeError("qpth_amd: forward mode is not served with scenarios=; call the expanded batch "
                               "(X.repeat_interleave(K, 0) for batched Q, G, A; p, h, b flattened) without scenarios=")

        @staticmethod
        @once_differentiable
        def backward(ctx, dl_dzhat, dl_dnu=None, dl_dlam=None, dl_dslacks=None):
            zhats, *six = ctx.saved_tensors
            neq = ctx.neq
            if dl_dzhat is None and dl_dlam is None and (dl_dnu is None or neq == 0):
                return (None,) * 6
            grads = ctx.fac.backward(zhats, ctx.lams, ctx.slacks, ctx.nus, dl_dzhat, want=tuple(ctx.needs_input_grad[:6]),
                                     shared=_shared_flags(six), dl_dlam=dl_dlam, dl_dnu=dl_dnu if neq > 0 else None)
            return _without_A_b(tuple(grads), neq)

    _EXPANDED = ("; call the expanded batch without scenarios= instead (X.repeat_interleave(K, 0) for batched Q, G, A; p, h, b "
                 "flattened to (B K, .))")

    def _apply_scenarios(Q, p, G, h, A, b, extras):
        """scenarios=K: the refusals, the shapes, then the one-blob path (nothing batched among Q, G, A), the expanded batch (a
        size or dtype the grouped kernels do not serve) or the grouped node; outputs (B, K, .)"""
        what = "qpth_amd: scenarios="
        for name, x in extras:
            if x is not None:
                raise ValueError(what + " together with %s is not served" % name + _EXPANDED)
        if warm_start is not None:
            raise ValueError(what + " with warm_start is not served" + _EXPANDED)
        if refine is not None and int(refine) > 0:
            raise ValueError(what + " with refine=%d is not served: pass refine=0 or refine=None" % int(refine) + _EXPANDED)
        if solver != QPSolvers.PDIPM_BATCHED:
            raise ValueError(what + " is served by solver=QPSolvers.PDIPM_BATCHED only" + _EXPANDED)
        if isinstance(scenarios, bool) or int(scenarios) != scenarios or int(scenarios) < 1:
            raise ValueError(what + "%r: the number of scenarios per (Q, G, A) must be a positive integer" % (scenarios,))
        K = int(scenarios)
        mats, vecs = ((Q, "Q"), (G, "G"), (A, "A")), ((p, "p"), (h, "h"), (b, "b"))
        sizes = [X.size(0) for X, _ in mats if X.dim() == 3] + [X.size(0) for X, _ in vecs if X.dim() in (2, 3)]
        B = sizes[0] if sizes else 1
        for X, name in mats:
            if X.nelement() > 0 and (X.dim() not in (2, 3) or (X.dim() == 3 and X.size(0) != B)):
                raise ValueError(what + "%d: %s has shape %s; expected (%d, ., .) or un-batched" % (K, name, tuple(X.shape), B))
        flat = []
        for X, name in vecs:
            if X.nelement() > 0:
                if X.dim() not in (1, 2, 3) or (X.dim() >= 2 and X.size(0) != B) or (X.dim() == 3 and X.size(1) != K):
                    raise ValueError(what + "%d: %s has shape %s; expected (%d, %d, .), (%d, .) or (.)"
                                     % (K, name, tuple(X.shape), B, K, B))
                if X.dim() == 2:              # shared by that QP's scenarios: materialised (small), autograd sums over them
                    X = X.unsqueeze(1).expand(B, K, X.size(-1))
                if X.dim() == 3:
                    X = X.reshape(B * K, X.size(-1))
            flat.append(X)
        p, h, b = flat
        batched = [X.dim() == 3 for X, _ in mats]
        if not any(batched):
            out = QPFunctionFn.apply(Q, p, G, h, A, b)                # one blob for all B K QPs, as without scenarios=
        else:
            lib = _lib.backend_for(Q)
            nineq, nz, neq = G.size(-2), G.size(-1), _neq_of(A)
            wide = refine is None and Q.dtype == torch.float32 and f64_arithmetic_serves(nz, nineq, neq, lib)
            code = _lib.QPX_F32_WIDE if wide else _lib._dtype_code(Q)
            finishing = Q.dtype == torch.float32 and refine is None and not wide       # (float32 kernels + finishing steps: per-QP data)
            if finishing or not lib.group_supported(code, nz, nineq, neq):
                Q, G, A = [X.repeat_interleave(K, 0) if X.dim() == 3 else X for X, _ in mats]
                out = QPFunctionFn.apply(Q, p, G, h, A, b)            # the expanded batch itself: no saving, the same answer
            else:
                out = QPScenarioFunctionFn.apply(Q, p, G, h, A, b)
        if torch.is_tensor(out):
            return out.reshape(B, K, out.size(-1)) if out.size(0) == B * K else out.unsqueeze(1).expand(B, K, out.size(-1))
        return tuple(X.reshape(B, K, X.size(-1)) if X.size(0) == B * K else X.unsqueeze(1).expand(B, K, X.size(-1)) for X in out)

    # the options of this QPFunction(...) that a row kind may refuse (_ROW_KINDS): is each one set?
    # (a RangeWarmStart is the range role's own holder: apply() has refused it everywhere else, the role does not refuse it)
    range_ws = isinstance(warm_start, RangeWarmStart)
    option_set = {"duals": bool(duals), "warm_start": warm_start is not None and not range_ws, "refine": refine is not None and int(refine) > 0,
                  "solver": solver != QPSolvers.PDIPM_BATCHED}

    def _gate(kind, Q, G, A, **given):
        """The refusals of one row kind (_ROW_KINDS), the first that applies: the other extra inputs (`given`) and the options of
        the call it does not combine with, in the kind's own order; then float64 inputs; then a size its role serves."""
        what, out, exists, symbol, refusals = _ROW_KINDS[kind]
        for name, text in refusals:
            if (given.get(name) is not None) if name in _EXTRA_INPUTS else option_set[name]:
                raise ValueError(what + text % {"refine": refine} + out)
        if Q.dtype != torch.float64:
            raise ValueError(what + " is served for float64 inputs only (the %s exists in float64 arithmetic), got %s"
                             % (exists, Q.dtype) + out)
        nineq, nz, neq = G.size(-2), G.size(-1), _neq_of(A)
        if not getattr(_lib.backend_for(Q).dll, symbol)(_lib.QPX_F64, nz, nineq, neq):
            raise ValueError(what + " is served up to nz + neq + nineq = 208 (the thread-grid / tile kernels, %s); "
                             "got nz = %d, nineq = %d, neq = %d" % (symbol, nz, nineq, neq) + out)

    def apply(Q, p, G, h, A, b, rho=None, kappa=None, lower=None, l1=None, soft_range=None):
        nineq = G.size(-2)
        if scenarios is not None:
            return _apply_scenarios(Q, p, G, h, A, b, (("rho", rho), ("kappa", kappa), ("lower", lower), ("l1", l1),
                                                       ("soft_range", soft_range)))
        if range_ws:
            with_ = [name for name, x in (("rho", rho), ("kappa", kappa), ("l1", l1), ("soft_range", soft_range)) if x is not None]
            if lower is None or with_:
                raise ValueError("qpth_amd: warm_start=RangeWarmStart() is the holder of two-sided rows (lower=) alone; got a call %s.  "
                                 "Pass a qpth_amd.WarmStart to the hard QP's call"
                                 % ("with " + ", ".join(with_) if with_ else "without lower"))
        if soft_range is not None:
            if not isinstance(soft_range, SoftRange):
                raise ValueError(_ROW_KINDS["soft_range"][0] + " must be a qpth_amd.SoftRange(lower, l1, rho, l1_lower=None, "
                                 "rho_lower=None), got %s" % type(soft_range).__name__)
            _gate("soft_range", Q, G, A, rho=rho, kappa=kappa, lower=lower, l1=l1)
            fields = soft_range.fields(Q, nineq, extract_nBatch(Q, p, G, h, A, b))
            return QPSoftRangeFunctionFn.apply(Q, p, G, h, A, b, *fields)
        if l1 is not None:
            if rho is None:
                raise ValueError(_ROW_KINDS["l1"][0] + " needs rho: rho is the penalty's curvature, gamma't + 1/2 t'diag(rho)t, and "
                                 "the pure l1 penalty (rho = 0, a singular augmented Q) is not served")
            _gate("l1", Q, G, A, kappa=kappa, lower=lower)
            nB = extract_nBatch(Q, p, G, h, A, b)
            return QPElasticFunctionFn.apply(Q, p, G, h, A, b, as_rho(rho, Q, nineq, nB), as_l1(l1, Q, nineq, nB))
        if lower is not None:
            _gate("lower", Q, G, A, rho=rho, kappa=kappa)
            return QPRangeFunctionFn.apply(Q, p, G, h, A, b, as_lower(lower, Q, nineq, extract_nBatch(Q, p, G, h, A, b)))
        if kappa is not None:
            _gate("kappa", Q, G, A, rho=rho)
            loop_eps = None if torch.is_tensor(kappa) else max(float(eps), nineq * float(kappa))
            kappa = as_kappa(kappa, Q, nineq, extract_nBatch(Q, p, G, h, A, b))
            return QPSmoothFunctionFn.apply(Q, p, G, h, A, b, kappa, loop_eps)
        if rho is None:
            return QPFunctionFn.apply(Q, p, G, h, A, b)
        if solver != QPSolvers.PDIPM_BATCHED:
            raise ValueError("qpth_amd: rho (soft inequality rows) is served by solver=QPSolvers.PDIPM_BATCHED only; with an "
                             "external solver, augment the QP with the violations t as variables")
        if refine is not None and int(refine) > 0:
            raise ValueError("qpth_amd: rho with refine=%d: refinement and the finishing steps evaluate residuals of the hard "
                             "QP; pass refine=0 (or refine=None with float64 inputs)" % int(refine))
        rho = as_rho(rho, Q, nineq, extract_nBatch(Q, p, G, h, A, b))
        return QPSoftFunctionFn.apply(Q, p, G, h, A, b, rho)
    return apply
