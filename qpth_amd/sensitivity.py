"""Many vector-Jacobian products at ONE solution of a batch of QPs: Jacobians of the solution and of the multipliers.

    sol = qpth_amd.sensitivity.solve(Q, p, G, h, A, b)        # the forward of QPFunction, state kept
    J = sol.jacobian(of=("z", "lam"), wrt=("p", "h"))         # J["z", "p"][b, i, j] = d zhat_i / d p_j
    g = sol.vjp_many(dl_dz=V)                                 # V (B, K, n): K cotangents per QP -> g["p"] (B, K, n), ...

`QPFunction`'s backward yields one product per launch, and every launch factors T = R + diag(1/d) again although the matrix
depends on the solution alone.  Here the K right-hand sides of a QP go through ONE launch and ONE factorisation
(KKTFactors.solve_kkt_many -> qpx_factor_solve_kkt_multi).  `torch.autograd.grad(..., is_grads_batched=True)` and
`torch.autograd.functional.jacobian(..., vectorize=True)` cannot do this: they hand backward a vmap-batched tensor without
storage, which has no pointer to give to a kernel.

An analysis interface, not an autograd node: every output is detached, and `QPFunction` itself is unchanged.
"""
import torch

from . import _lib
from .kkt import KKTFactors, RangeWarmStart, _rows, as_kappa, as_lower, as_rho
from .qp import _expand_params, _loop_epilogue, _neq_of, f64_arithmetic_serves
from .util import extract_nBatch

_VECTORS = ("p", "h", "b")
_MATRICES = ("Q", "G", "A")


class QPSolution:
    """What the forward of QPFunction leaves behind: zhat (B,n), nu (B,q), lam, slacks (B,m), the factors (KKTFactors) and
    the parameters expanded to the batch (`params`: Q, p, G, h, A, b; `shared`: which of them the batch shares)."""

    def __init__(self, fac, res, params, shared, refine, rho=None, rho_dim=None, lower=None, lower_shared=False):
        self.fac = fac
        # two-sided rows (solve(lower=...)): lower as (B | 1, m), the lower side's multipliers and slacks (0 and +inf on a one-sided row)
        self.lower, self.lower_shared = lower, lower_shared
        self.lam_lo, self.slacks_lo = (res.lam_lo, res.slacks_lo) if lower is not None else (None, None)
        self.rho, self.rho_dim = rho, rho_dim       # soft rows (solve(rho=...)): rho as (B | 1, m) and the caller's rho.dim()
        self.zhat, self.nu, self.lam, self.slacks = res.zhat, res.nu, res.lam, res.slacks
        self.params = dict(zip(("Q", "p", "G", "h", "A", "b"), params))
        self.shared = dict(zip(("Q", "p", "G", "h", "A", "b"), shared))
        self.refine = refine          # the backward's rule (qp.py): one in-kernel refinement step where the forward polished

    def _vjp_many_range(self, dl_dz, dl_dlam, dl_dlam_lo, dl_dnu):
        """The K-right-hand-side solve after solve(lower=...): the doubled QP's backward system collapsed onto the
        m x m launch.  With du = clamp(lam)/clamp(slacks), dl = clamp(lam_lo)/clamp(slacks_lo) (exactly 0 on a one-sided row),
        d = du + dl and the cotangents gu on lam, gl on lam_lo: solve with d and rz = (du gu - dl gl)/d for dx, v, dy; then
        dz_u = (du/d)(v + dl (gu + gl)), dz_l = (dl/d)(-v + du (gu + gl)), v = dz_u - dz_l.  The side with the SMALLER d is
        formed by its formula and the other from v (the larger side's formula is a difference of two numbers of size d times
        the cotangents): as the loop's range blocks choose.  -> dx, v, dz_u, dz_l, dy"""
        fac, q = self.fac, self.fac.q
        du = torch.clamp(self.lam, min=1e-8) / torch.clamp(self.slacks, min=1e-8)
        dl = torch.clamp(self.lam_lo, min=1e-8) / torch.clamp(self.slacks_lo, min=1e-8)
        d = du + dl
        rz = g = None
        if dl_dlam is not None or dl_dlam_lo is not None:
            K = (dl_dlam if dl_dlam is not None else dl_dlam_lo).shape[1]
            gu = fac._vecs(dl_dlam, K, fac.m, "dl_dlam") if dl_dlam is not None else None
            gl = fac._vecs(dl_dlam_lo, K, fac.m, "dl_dlam_lo") if dl_dlam_lo is not None else None
            num = (du.unsqueeze(1) * gu if gu is not None else 0) - (dl.unsqueeze(1) * gl if gl is not None else 0)
            rz = num / d.unsqueeze(1)
            g = (gu if gu is not None else 0) + (gl if gl is not None else 0)
        dx, _, v, dy = fac.solve_kkt_many(d, dl_dz, None, rz, dl_dnu if q else None)
        du_, dl_, d_ = du.unsqueeze(1), dl.unsqueeze(1), d.unsqueeze(1)
        upper_larger = (du_ >= dl_).expand_as(v)
        zl = (dl_ / d_) * ((du_ * g if g is not None else 0) - v)
        zu = (du_ / d_) * ((dl_ * g if g is not None else 0) + v)
        dz_u = torch.where(upper_larger, v + zl, zu)
        dz_l = torch.where(upper_larger, zl, zu - v)
        return dx, v, dz_u, dz_l, dy

    def vjp_many(self, dl_dz=None, dl_dlam=None, dl_dnu=None, want=_VECTORS, dl_dlam_lo=None):
        """K vector-Jacobian products per QP.  Cotangents dl_dz (B,K,n), dl_dlam (B,K,m), dl_dnu (B,K,q): None = zeros, pass
        at least one.  The backward's KKT system (qp.py:148-155), d = clamp(lam, 1e-8) / clamp(slacks, 1e-8), with the
        right-hand sides (dl_dz, 0, dl_dlam, dl_dnu), solved for all K in one launch (KKTFactors.solve_kkt_many).
        Returns a dict over `want` of K-stacked gradients: "p": dx (B,K,n), "h": -dz (B,K,m), "b": -dy (B,K,q), and the
        formulas of qpx_backward_duals for the matrices, "Q": 1/2 (dx zhat' + zhat dx') (B,K,n,n), "G": dz zhat' + lam dx'
        (B,K,m,n), "A": dy zhat' + nu dx' (B,K,q,n); after solve(rho=...), "rho": dz lam / rho^2 (B,K,m), 0 on a hard row
        (a shared rho: the mean over B, (K,m); a scalar rho: summed over the rows too, (K,)).  The matrix gradients are composed on the host by torch.einsum and are
        bound by memory traffic: B K n n elements each -- 41 MB for "Q" in float64 at B = 512, K = n = 100, written once
        and, for a shared parameter, read again by the mean.  A parameter the batch shares gets the reference's `.mean(0)`
        over B (qp.py:159-177)."""
        fac, q = self.fac, self.fac.q
        ranged = self.lower is not None
        known = _VECTORS + _MATRICES + (("rho",) if self.rho is not None else ()) + (("lower",) if ranged else ())
        bad = [w for w in want if w not in known]
        if bad:
            raise ValueError("qpth_amd: vjp_many: unknown parameter(s) %s; choose from %s%s"
                             % (bad, known, "" if self.rho is not None or ranged else " ('rho' after solve(rho=...), 'lower' after "
                                                                                    "solve(lower=...))"))
        if dl_dlam_lo is not None and not ranged:
            raise ValueError("qpth_amd: vjp_many: dl_dlam_lo is the cotangent of the lower side's multipliers: after solve(lower=...) only")
        if dl_dz is None and dl_dlam is None and dl_dlam_lo is None and (dl_dnu is None or q == 0):
            raise RuntimeError("qpth_amd: vjp_many needs at least one of dl_dz, dl_dlam, dl_dnu")
        zh, lam, nu = self.zhat, self.lam, self.nu
        if ranged:
            # "h": -dz_u, "lower": +dz_l (exactly 0 on a one-sided row), "G": v zhat' + (lam - lam_lo) dx'
            dx, dz, dz_u, dz_l, dy = self._vjp_many_range(dl_dz, dl_dlam, dl_dlam_lo, dl_dnu)
            lam = lam - self.lam_lo
        else:
            d = torch.clamp(self.lam, min=1e-8) / torch.clamp(self.slacks, min=1e-8)            # qp.py:148
            dx, _, dz, dy = fac.solve_kkt_many(d, dl_dz, None, dl_dlam, dl_dnu if q else None,
                                               refine=1 if (self.refine > 0 and fac.refine_ok) else 0)
            dz_u = dz
        B, K = dx.shape[:2]
        if dy is None:
            dy = dx.new_zeros(B, K, 0)

        def outer(u, v):                 # u (B,K,r), v (B,c) -> u_k v' (B,K,r,c)
            return torch.einsum("bkr,bc->bkrc", u, v)

        def outer_t(v, u):               # v (B,r), u (B,K,c) -> v u_k' (B,K,r,c)
            return torch.einsum("br,bkc->bkrc", v, u)

        out = {}
        for w in want:
            if w == "p":
                g = dx
            elif w == "h":
                g = -dz_u
            elif w == "lower":
                out[w] = (dz_l.mean(0) if self.lower_shared else dz_l).detach()
                continue
            elif w == "b":
                g = -dy
            elif w == "rho":
                g = dz * (lam / (self.rho * self.rho)).unsqueeze(1)
                g = (g if self.rho_dim == 2 else g.mean(0)) if self.rho_dim > 0 else g.mean(0).sum(-1)
                out[w] = g.detach()
                continue
            elif w == "Q":
                g = 0.5 * (outer(dx, zh) + outer_t(zh, dx))
            elif w == "G":
                g = outer(dz, zh) + outer_t(lam, dx)
            else:
                g = outer(dy, zh) + outer_t(nu, dx)
            out[w] = (g.mean(0) if self.shared[w] else g).detach()
        return out

    def jacobian(self, of=("z",), wrt=_VECTORS):
        """Jacobians of the solution -- and of the multipliers: `of` may add "lam" and "nu" -- with respect to the vector
        parameters in `wrt`, a dict keyed (of, wrt): J["z","p"] (B,n,n) with [b,i,j] = d zhat_i / d p_j, J["z","h"] (B,n,m),
        J["z","b"] (B,n,q), J["lam","h"] (B,m,m), ...; after solve(rho=...) with a per-QP or shared vector rho, "rho" too:
        J["z","rho"] (B,n,m).  vjp_many with identity cotangents: K = n (+ m + q) right-hand sides
        per QP, still one launch.  (The Jacobian with respect to a parameter the batch shares is the mean over the batch of
        the per-QP Jacobians, as vjp_many returns it.)"""
        fac = self.fac
        B, n, m, q = fac.B, fac.n, fac.m, fac.q
        of = tuple(of)
        ranged = self.lower is not None
        outputs = ("z", "lam", "lam_lo", "nu") if ranged else ("z", "lam", "nu")
        if not of or any(o not in outputs for o in of):
            raise ValueError("qpth_amd: jacobian: `of` is a non-empty subset of %s, got %s" % (outputs, of))
        vectors = _VECTORS + (("rho",) if self.rho_dim is not None and self.rho_dim > 0 else ()) + (("lower",) if ranged else ())
        if any(w not in vectors for w in wrt):
            raise ValueError("qpth_amd: jacobian: only the vector parameters %s are allowed in `wrt`, got %s" % (vectors, tuple(wrt)))
        sizes = {"z": n, "lam": m, "lam_lo": m, "nu": q}
        rows, K = {}, 0
        for o in outputs:
            if o in of and sizes[o] > 0:
                rows[o] = (K, K + sizes[o])
                K += sizes[o]
        dt, dev = self.zhat.dtype, self.zhat.device

        def identity_block(o):
            if o not in rows:
                return None
            c = torch.zeros(B, K, sizes[o], dtype=dt, device=dev)
            r0, r1 = rows[o]
            c[:, r0:r1] = torch.eye(sizes[o], dtype=dt, device=dev)
            return c

        g = self.vjp_many(identity_block("z"), identity_block("lam"), identity_block("nu"), want=tuple(wrt),
                          dl_dlam_lo=identity_block("lam_lo") if ranged else None)
        J = {}
        for o in of:
            r0, r1 = rows.get(o, (0, 0))
            for w in wrt:
                J[o, w] = g[w][..., r0:r1, :]
        return J


def solve(Q, p, G, h, A, b, eps=1e-12, maxIter=20, notImprovedLim=3, check_Q_spd=True, verbose=-1, warm_start=None, rho=None,
          kappa=None, kappa_tol=1e-9, kappa_steps=20, lower=None):
    """The forward of QPFunction(eps, verbose, notImprovedLim, maxIter, check_Q_spd)(Q, p, G, h, A, b) with its defaults for
    float32 (float64 arithmetic where f64_arithmetic_serves, else the float32 kernels + two finishing steps): un-batched
    parameters are broadcast, a Q that is not SPD raises.  Returns the QPSolution; nothing is recorded for autograd.
    warm_start: a qpth_amd.WarmStart, as for QPFunction(warm_start=...) -- the loop starts at the holder's (lam, slacks) and
    the holder takes this solve's.
    rho: soft inequality rows, as the seventh input of QPFunction's callable: (nBatch, nineq), (nineq,), () or a
    float, > 0, +inf = a hard row.  vjp_many(want=(..., "rho")) and jacobian(wrt=(..., "rho")) then differentiate in it.
    float32 inputs need a size that runs in float64 arithmetic (f64_arithmetic_serves): the finishing steps of the other
    sizes evaluate residuals of the hard QP.
    kappa: the barrier-smoothed QP, as QPFunction's `kappa`: (nBatch, nineq), (nineq,), () or a float, > 0.  The
    iterate is centred onto the central path at kappa (KKTFactors.centre, to kappa_tol in kappa_steps steps at most) before the
    state is kept, so jacobian() and vjp_many() are those of the smoothed map.  float64 inputs up to nz+neq+nineq = 208, not
    together with rho (ValueError).
    lower: two-sided rows lower <= G z <= h, as QPFunction's `lower`: (nBatch, nineq) or (nineq,), -inf = a
    one-sided row.  The solution keeps lam_lo, slacks_lo and lower; vjp_many takes dl_dlam_lo and want=(..., "lower"),
    jacobian of=(..., "lam_lo") and wrt=(..., "lower"), still one launch for all right-hand sides.  warm_start is then a
    qpth_amd.RangeWarmStart (a plain WarmStart there, or a RangeWarmStart without lower: ValueError).  float64 inputs at
    the range role's sizes; not together with rho or kappa (ValueError)."""
    if lower is not None:
        return _solve_range(Q, p, G, h, A, b, lower, eps, maxIter, notImprovedLim, check_Q_spd, verbose, warm_start, rho, kappa)
    if isinstance(warm_start, RangeWarmStart):
        raise ValueError("qpth_amd: warm_start=RangeWarmStart() is the holder of two-sided rows: pass lower=, or a qpth_amd.WarmStart")
    with torch.no_grad():
        nBatch = extract_nBatch(Q, p, G, h, A, b)
        nineq, nz = G.size(-2), G.size(-1)
        neq = _neq_of(A)
        assert(neq > 0 or nineq > 0)
        wide = Q.dtype == torch.float32 and f64_arithmetic_serves(nz, nineq, neq, _lib.backend_for(Q))
        rho_dim = None
        if rho is not None:
            rho = as_rho(rho, Q, nineq, nBatch)
            if Q.dtype == torch.float32 and not wide:
                raise ValueError("qpth_amd: rho with float32 inputs at a size the float32 kernels serve with finishing steps on the "
                                 "residuals of the hard QP; use float64 inputs, or QPFunction(refine=0)")
            rho_dim = rho.dim()
            rho = _rows(rho, nineq)
            nBatch = max(nBatch, rho.size(0))
        if kappa is not None:
            if rho is not None:
                raise ValueError("qpth_amd: kappa (the barrier-smoothed QP) together with rho (soft rows) is not served")
            if Q.dtype != torch.float64:
                raise ValueError("qpth_amd: kappa (the barrier-smoothed QP) is served for float64 inputs only, got %s" % Q.dtype)
            loop_eps = None if torch.is_tensor(kappa) else max(float(eps), nineq * float(kappa))
            kappa = _rows(as_kappa(kappa, Q, nineq, nBatch), nineq)
            nBatch = max(nBatch, kappa.size(0))
            eps = eps if loop_eps is None else loop_eps
        params, shared = _expand_params([X.detach() for X in (Q, p, G, h, A, b)], nBatch)
        Qe, pe, Ge, he, Ae, be = params
        fac = KKTFactors.build(Qe, Ge, Ae, nBatch, wide=wide, w=None if rho is None else rho.reciprocal())
        warm = warm_start.pair(nBatch, nineq, Q.dtype, Q.device) if warm_start is not None else None
        res = fac.ipm(pe, he, be, eps, maxIter, notImprovedLim, want_trace=(verbose == 1), warm=warm,
                      warm_floor=warm_start.floor if warm is not None else 1e-2)
        refine = 2 if (Q.dtype == torch.float32 and not wide) else 0
        if refine > 0:
            res = fac.polish(pe, he, be, res, steps=refine, refine=0)
        if kappa is not None:
            res = fac.centre(pe, he, be, res, kappa, tol=kappa_tol, max_steps=kappa_steps)      # (refuses unserved sizes)
        if warm_start is not None:
            warm_start.take(res)
        _loop_epilogue(fac, res, check_Q_spd, verbose, inaccurate=kappa is None)
        if kappa is not None:
            if bool(((res.centre_steps == 0) & torch.isinf(res.centre_resid)).any().item()):
                raise ValueError("kappa must be positive")
        return QPSolution(fac, res, params, shared, refine, rho, rho_dim)


def _solve_range(Q, p, G, h, A, b, lower, eps, maxIter, notImprovedLim, check_Q_spd, verbose, warm_start, rho, kappa):
    """solve(..., lower=lower): the hard QP's factors and the loop's range role (KKTFactors.ipm_range)"""
    for name, x in (("rho (soft rows)", rho), ("kappa (the barrier-smoothed QP)", kappa)):
        if x is not None:
            raise ValueError("qpth_amd: lower (two-sided rows) together with %s is not served" % name)
    if warm_start is not None and not isinstance(warm_start, RangeWarmStart):
        raise ValueError("qpth_amd: lower (two-sided rows) with warm_start=%s() is not served: that holder has nothing for the lower "
                         "side; pass a qpth_amd.RangeWarmStart" % type(warm_start).__name__)
    with torch.no_grad():
        nineq = G.size(-2)
        nBatch = extract_nBatch(Q, p, G, h, A, b)
        lower = as_lower(lower, Q, nineq, nBatch).detach()
        if lower.dim() == 2:
            nBatch = max(nBatch, lower.size(0))
        assert(nineq > 0)
        params, shared = _expand_params([X.detach() for X in (Q, p, G, h, A, b)], nBatch)
        Qe, pe, Ge, he, Ae, be = params
        fac = KKTFactors.build(Qe, Ge, Ae, nBatch)
        fac._require_role(*fac._RANGE)            # (dtype and sizes: the range role's own rule and message)
        warm = warm_start.quad(nBatch, nineq, Q.dtype, Q.device) if warm_start is not None else None
        res = fac.ipm_range(pe, he, lower, be, eps, maxIter, notImprovedLim, want_trace=(verbose == 1), warm=warm,
                            warm_floor=warm_start.floor if warm is not None else 1e-2)
        if warm_start is not None:
            warm_start.take(res)
        _loop_epilogue(fac, res, check_Q_spd, verbose)
        return QPSolution(fac, res, params, shared, 0, lower=_rows(lower, nineq), lower_shared=lower.dim() == 1)
