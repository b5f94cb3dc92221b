"""ctypes binding of the C ABI in include/qpx.h (libqpx_hip.so).

The product path is MI355X only: `hip()` loads qpth_amd/libqpx_hip.so (built by
`__graft_entry__.build()` / qpth_amd/csrc/build.sh) and FAILS LOUDLY when it is missing or
when tensors are not on a HIP device -- there is no CPU fallback anywhere in this package.

`QpxLib(path)` is the marshalling layer: torch tensors in, raw pointers + batch strides +
the current HIP stream out.  Tests additionally instantiate it over tests/emu's host-thread
emulation of the very same kernel bodies (`set_test_backend`), which exists so that the
GPU-less CI can exercise the host logic; nothing in the package selects it by itself.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_SO = os.path.join(_HERE, "libqpx_hip.so")

QPX_F32, QPX_F64, QPX_F32_WIDE = 0, 1, 2      # QPX_F32_WIDE: float32 arrays, float64 factors and arithmetic (include/qpx.h)
ST_Q_NOT_SPD, ST_A_RANK, ST_KKT_BREAKDOWN, ST_INACCURATE, ST_MAXITER, ST_NONFINITE = 1, 2, 4, 8, 16, 32
ST_NOT_CENTRED = 64                            # qpx_centre ended above its tolerance
STALL_OFF, STALL_REFERENCE, STALL_FLOOR = 0, 1, 2
FAMILY_GRID, FAMILY_TILE, FAMILY_BIG = 1, 2, 3

_vp, _i, _i64, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double

_SIGNATURES = {
    # name: (restype, argtypes)       -- must list every symbol include/qpx.h declares
    "qpx_abi_version": (_i, []),
    "qpx_strerror": (ctypes.c_char_p, [_i]),
    "qpx_factor_elems": (ctypes.c_size_t, [_i, _i, _i, _i]),
    "qpx_max_dim": (_i, []),
    "qpx_supported": (_i, [_i, _i, _i, _i]),
    "qpx_kernel_family": (_i, [_i, _i, _i, _i]),
    "qpx_refine_supported": (_i, [_i, _i, _i, _i]),
    "qpx_set_ipm_variant": (_i, [_i]),
    "qpx_get_ipm_variant": (_i, []),
    "qpx_can_share_factors": (_i, [_i, _i, _i, _i]),
    "qpx_big_gemm_r": (_i, [_i, _i, _i, _i, _i, _vp, _vp]),
    "qpx_pre_factor": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    "qpx_pre_factor_soft": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    "qpx_ipm": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _d, _i, _i, _i,
                     _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qpx_warm_supported": (_i, [_i, _i, _i, _i]),
    "qpx_ipm_warm": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _d, _i, _i, _i,
                          _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _d, _vp, _vp]),
    "qpx_forward": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64,
                         _vp, _i64, _vp, _d, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qpx_factor_solve_kkt": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                  _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
    "qpx_backward": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                          _vp, _vp, _vp, _vp, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
    "qpx_backward_duals": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                _vp, _vp, _vp, _vp, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
    "qpx_jvp": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64,
                     _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
    "qpx_multi_supported": (_i, [_i, _i, _i, _i]),
    "qpx_factor_solve_kkt_multi": (_i, [_i, _i, _i, _i, _i, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qpx_backward2_supported": (_i, [_i, _i, _i, _i]),
    "qpx_backward2": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                           _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64,
                           _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qpx_polish_supported": (_i, [_i, _i, _i, _i]),
    "qpx_polish": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64,
                        _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qpx_centre_supported": (_i, [_i, _i, _i, _i]),
    "qpx_centre": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64,
                        _vp, _i64, _vp, _i64, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qpx_range_supported": (_i, [_i, _i, _i, _i]),
    "qpx_ipm_range": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _d, _i, _i, _i,
                           _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "qpx_range_warm_supported": (_i, [_i, _i, _i, _i]),
    "qpx_ipm_range_warm": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _d, _i, _i, _i,
                                _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp,
                                _vp, _vp, _vp, _vp, _d, _vp, _vp]),
    "qpx_backward_range": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                _vp, _vp, _vp, _vp, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "qpx_elastic_supported": (_i, [_i, _i, _i, _i]),
    "qpx_ipm_elastic": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _d, _i, _i, _i,
                             _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "qpx_soft_range_supported": (_i, [_i, _i, _i, _i]),
    "qpx_ipm_soft_range": (_i, [_i, _i, _i, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _d, _i, _i, _i,
                                _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64,
                                _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qpx_batch_outer": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _d, _vp, _vp, ctypes.c_size_t, _vp]),
    "qpx_batch_outer_workspace_elems": (ctypes.c_size_t, [_i, _i, _i, _i]),
    "qpx_dense_solve": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "qpx_group_supported": (_i, [_i, _i, _i, _i]),
    "qpx_ipm_group": (_i, [_i, _i, _i, _i, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _d, _i, _i, _i,
                           _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qpx_backward_group": (_i, [_i, _i, _i, _i, _i, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                _vp, _vp, _vp, _vp, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
    "qpx_group_outer": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _d, _vp, _vp, ctypes.c_size_t, _vp]),
    "qpx_group_outer_workspace_elems": (ctypes.c_size_t, [_i, _i, _i, _i, _i]),
}
ABI_SYMBOLS = tuple(_SIGNATURES)


def _dtype_code(t):
    if t.dtype == torch.float64:
        return QPX_F64
    if t.dtype == torch.float32:
        return QPX_F32
    raise TypeError("qpth_amd supports float32 and float64 tensors, got %s" % t.dtype)


def _code(factors, wide):
    """dtype code of a call: QPX_F32_WIDE when the caller's arrays are float32 and `factors` is the float64 blob"""
    if wide:
        assert factors.dtype == torch.float64
        return QPX_F32_WIDE
    return _dtype_code(factors)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(t):
    if t.is_cuda:
        return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    return None


class Param:
    """A QP parameter as the kernels see it: dense trailing dims + a batch stride (0 = shared)."""

    def __init__(self, X, nbatch_dims):
        if X is None or X.nelement() == 0:
            self.t, self.stride = None, 0
            return
        if X.dim() == nbatch_dims:       # batched; an expand()ed view has stride 0 already
            if X.stride(0) == 0:
                X = X[0]
            else:
                X = X.contiguous()
                self.t, self.stride = X, (X.stride(0) if X.size(0) > 1 else 0)
                return
        self.t, self.stride = X.contiguous(), 0

    @property
    def ptr(self):
        return _ptr(self.t)


class QpxLib:
    def __init__(self, path, strict=True):
        """strict=False (scripts/ab_bench.py only): an older build of the library -- symbols it lacks are skipped and
        its ABI version is not checked; the product path always loads strictly."""
        if not os.path.exists(path):
            raise RuntimeError(
                "qpth_amd: %s is missing. Build the gfx950 extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or qpth_amd/csrc/build.sh). "
                "There is no CPU fallback." % path)
        self.path = path
        self.dll = ctypes.CDLL(path)
        for name, (res, args) in _SIGNATURES.items():
            if not strict and not hasattr(self.dll, name):
                continue
            fn = getattr(self.dll, name)       # AttributeError if a declared symbol is missing
            fn.restype, fn.argtypes = res, args
        if strict and self.dll.qpx_abi_version() != 8:
            raise RuntimeError("qpth_amd: ABI version mismatch in %s" % path)

    def check(self, code):
        if code != 0:
            raise RuntimeError("qpth_amd: %s (code %d)" % (self.dll.qpx_strerror(code).decode(), code))

    def factor_elems(self, dtype_code, n, m, q):
        return int(self.dll.qpx_factor_elems(dtype_code, n, m, q))

    # -- batch.py:375-429 ---------------------------------------------------------------
    def pre_factor(self, B, n, m, q, Q, G, A, factors, status, wide=False, w=None):
        """w (B,m) or (m,): soft rows, w = 1 / rho, 0 = hard (qpx_pre_factor_soft); without it the call is qpx_pre_factor
        itself, as before."""
        Qp, Gp, Ap = Param(Q, 3), Param(G, 3), Param(A, 3)
        if w is not None:
            wp = Param(w, 2)
            self.check(self.dll.qpx_pre_factor_soft(
                _code(factors, wide), B, n, m, q, Qp.ptr, Qp.stride, Gp.ptr, Gp.stride, Ap.ptr, Ap.stride,
                wp.ptr, wp.stride, _ptr(factors), _ptr(status), _stream(factors)))
            return
        self.check(self.dll.qpx_pre_factor(
            _code(factors, wide), B, n, m, q, Qp.ptr, Qp.stride, Gp.ptr, Gp.stride, Ap.ptr, Ap.stride,
            _ptr(factors), _ptr(status), _stream(factors)))

    # -- batch.py:47-207 ----------------------------------------------------------------
    def _ipm_call(self, fn, common, *more, wide=False):
        """one loop entry point `fn`: qpx_ipm's arguments -- every loop entry point begins with them; `common`, in the order
        unpacked below --, then `more` (what the entry point takes behind them, marshalled by the caller), then the stream"""
        (B, n, m, q, p, h, b, factors, sfac, eps, maxIter, notImprovedLim, stall_policy,
         zhat, nu, lam, slack, iters, status, best_resid, trace) = common
        pp, hp, bp = Param(p, 2), Param(h, 2), Param(b, 2)
        self.check(fn(
            _code(factors, wide), B, n, m, q, pp.ptr, pp.stride, hp.ptr, hp.stride, bp.ptr, bp.stride,
            _ptr(factors), int(sfac), float(eps), int(maxIter), int(notImprovedLim), int(stall_policy),
            _ptr(zhat), _ptr(nu), _ptr(lam), _ptr(slack), _ptr(iters), _ptr(status), _ptr(best_resid),
            _ptr(trace), *more, _stream(factors)))

    def ipm(self, B, n, m, q, p, h, b, factors, sfac, eps, maxIter, notImprovedLim, stall_policy,
            zhat, nu, lam, slack, iters, status, best_resid, trace=None, wide=False,
            lam0=None, s0=None, warm_floor=1e-2, warm_used=None):
        """lam0, s0 (B,m) dense: the warm start (qpx_ipm_warm); without them the call is qpx_ipm itself, as before."""
        common = (B, n, m, q, p, h, b, factors, sfac, eps, maxIter, notImprovedLim, stall_policy,
                  zhat, nu, lam, slack, iters, status, best_resid, trace)
        if lam0 is not None or s0 is not None:
            self._ipm_call(self.dll.qpx_ipm_warm, common, _ptr(lam0), _ptr(s0), float(warm_floor), _ptr(warm_used), wide=wide)
            return
        self._ipm_call(self.dll.qpx_ipm, common, wide=wide)

    # -- qp.py:92-96 ---------------------------------------------------------------------
    def forward(self, B, n, m, q, Q, p, G, h, A, b, factors, eps, maxIter, notImprovedLim,
                stall_policy, zhat, nu, lam, slack, iters, status, best_resid, trace=None, wide=False):
        Qp, Gp, Ap = Param(Q, 3), Param(G, 3), Param(A, 3)
        pp, hp, bp = Param(p, 2), Param(h, 2), Param(b, 2)
        self.check(self.dll.qpx_forward(
            _code(factors, wide), B, n, m, q, Qp.ptr, Qp.stride, pp.ptr, pp.stride, Gp.ptr, Gp.stride,
            hp.ptr, hp.stride, Ap.ptr, Ap.stride, bp.ptr, bp.stride, _ptr(factors), float(eps),
            int(maxIter), int(notImprovedLim), int(stall_policy), _ptr(zhat), _ptr(nu), _ptr(lam),
            _ptr(slack), _ptr(iters), _ptr(status), _ptr(best_resid), _ptr(trace), _stream(factors)))

    # -- batch.py:435-470 + 349-372 ------------------------------------------------------
    def factor_solve_kkt(self, B, n, m, q, factors, sfac, d, rx, rs, rz, ry, dx, ds, dz, dy, status,
                         refine=0, Q=None, G=None, A=None, wide=False):
        Qp, Gp, Ap = Param(Q, 3), Param(G, 3), Param(A, 3)
        self.check(self.dll.qpx_factor_solve_kkt(
            _code(factors, wide), B, n, m, q, _ptr(factors), int(sfac), _ptr(d), _ptr(rx), _ptr(rs), _ptr(rz),
            _ptr(ry), _ptr(dx), _ptr(ds), _ptr(dz), _ptr(dy), int(refine), Qp.ptr, Qp.stride, Gp.ptr, Gp.stride,
            Ap.ptr, Ap.stride, _ptr(status), _stream(factors)))

    # -- factor_kkt once, solve_kkt for K right-hand sides per QP (no reference counterpart) ------
    def factor_solve_kkt_multi(self, B, n, m, q, K, factors, sfac, d, rx, rs, rz, ry, dx, ds, dz, dy, status, wide=False):
        """rx .. ry, dx .. dy: (B, K, .) contiguous or None (zeros / not wanted; dx required)"""
        self.check(self.dll.qpx_factor_solve_kkt_multi(
            _code(factors, wide), B, n, m, q, int(K), _ptr(factors), int(sfac), _ptr(d), _ptr(rx), _ptr(rs), _ptr(rz),
            _ptr(ry), _ptr(dx), _ptr(ds), _ptr(dz), _ptr(dy), _ptr(status), _stream(factors)))

    # -- qp.py:127-182 --------------------------------------------------------------------
    def backward(self, B, n, m, q, factors, sfac, zhat, lam, slack, nu, dl_dz, dQ, dp, dG, dh, dA, db, status,
                 dx=None, dz=None, dy=None, refine=0, Q=None, G=None, A=None, wide=False, dl_dlam=None, dl_dnu=None):
        """Any of dQ..db may be None (gradient not wanted); dx, dz, dy: optional KKT solution outputs.
        dl_dlam (B,m), dl_dnu (B,q): cotangents of the multipliers (qpx_backward_duals; dl_dz may then be None).  Without
        them the call is qpx_backward itself, as before."""
        Qp, Gp, Ap = Param(Q, 3), Param(G, 3), Param(A, 3)
        if dl_dlam is not None or dl_dnu is not None or dl_dz is None:
            self.check(self.dll.qpx_backward_duals(
                _code(factors, wide), B, n, m, q, _ptr(factors), int(sfac), _ptr(zhat), _ptr(lam), _ptr(slack),
                _ptr(nu), _ptr(dl_dz), _ptr(dl_dlam), _ptr(dl_dnu), _ptr(dQ), _ptr(dp), _ptr(dG), _ptr(dh), _ptr(dA), _ptr(db),
                _ptr(dx), _ptr(dz), _ptr(dy), int(refine), Qp.ptr, Qp.stride, Gp.ptr, Gp.stride, Ap.ptr, Ap.stride,
                _ptr(status), _stream(factors)))
            return
        self.check(self.dll.qpx_backward(
            _code(factors, wide), B, n, m, q, _ptr(factors), int(sfac), _ptr(zhat), _ptr(lam), _ptr(slack),
            _ptr(nu), _ptr(dl_dz), _ptr(dQ), _ptr(dp), _ptr(dG), _ptr(dh), _ptr(dA), _ptr(db),
            _ptr(dx), _ptr(dz), _ptr(dy), int(refine), Qp.ptr, Qp.stride, Gp.ptr, Gp.stride, Ap.ptr, Ap.stride,
            _ptr(status), _stream(factors)))

    # -- two-sided rows lower <= G z <= h: the loop's and the backward's range role, float64
    def ipm_range(self, B, n, m, q, p, h, lower, gt1, b, factors, sfac, eps, maxIter, notImprovedLim, stall_policy,
                  zhat, nu, lam, slack, lam_lo, slack_lo, iters, status, best_resid, trace=None,
                  warm=None, warm_floor=1e-2, warm_used=None):
        """lower (B,m), (1,m) or (m,) (shared: batch stride 0), -inf = a one-sided row; gt1 (B,) = || G^T e || or None (0).
        warm = (lam0, s0, lam0_lo, s0_lo), (B,m) dense: the warm start (qpx_ipm_range_warm); without it the call is
        qpx_ipm_range itself, as before."""
        lp = Param(lower, 2)
        common = (B, n, m, q, p, h, b, factors, sfac, eps, maxIter, notImprovedLim, stall_policy,
                  zhat, nu, lam, slack, iters, status, best_resid, trace)
        if warm is not None:
            self._ipm_call(self.dll.qpx_ipm_range_warm, common,
                           lp.ptr, lp.stride, _ptr(gt1), _ptr(lam_lo), _ptr(slack_lo),
                           *[_ptr(w) for w in warm], float(warm_floor), _ptr(warm_used))
            return
        self._ipm_call(self.dll.qpx_ipm_range, common,
                       lp.ptr, lp.stride, _ptr(gt1), _ptr(lam_lo), _ptr(slack_lo))

    def backward_range(self, B, n, m, q, factors, sfac, zhat, lam, slack, lam_lo, slack_lo, nu, dl_dz, dQ, dp, dG, dA, db,
                       status, dx=None, dz=None, dy=None):
        """Any of dQ..db may be None (gradient not wanted); dz = v, from which the caller forms dh and dlower"""
        self.check(self.dll.qpx_backward_range(
            _dtype_code(factors), B, n, m, q, _ptr(factors), int(sfac), _ptr(zhat), _ptr(lam), _ptr(slack), _ptr(nu),
            _ptr(dl_dz), _ptr(dQ), _ptr(dp), _ptr(dG), None, _ptr(dA), _ptr(db), _ptr(dx), _ptr(dz), _ptr(dy), 0,
            None, 0, None, 0, None, 0, _ptr(status), _ptr(lam_lo), _ptr(slack_lo), _stream(factors)))

    # -- elastic rows G z <= h + t, t >= 0: the loop's elastic role, float64
    def ipm_elastic(self, B, n, m, q, p, h, gamma, rho, gt1, b, factors, sfac, eps, maxIter, notImprovedLim, stall_policy,
                    zhat, nu, lam, slack, lam_t, slack_t, t, iters, status, best_resid, trace=None):
        """gamma, rho (B,m), (1,m) or (m,) (shared: batch stride 0), +inf in either = a hard row; gt1 (B,) = || G'^T 1 ||"""
        gp, rp = Param(gamma, 2), Param(rho, 2)
        common = (B, n, m, q, p, h, b, factors, sfac, eps, maxIter, notImprovedLim, stall_policy,
                  zhat, nu, lam, slack, iters, status, best_resid, trace)
        self._ipm_call(self.dll.qpx_ipm_elastic, common,
                       gp.ptr, gp.stride, rp.ptr, rp.stride, _ptr(gt1), _ptr(lam_t), _ptr(slack_t), _ptr(t))

    # -- soft two-sided rows lower - tl <= G z <= h + tu: the loop's soft-range role, float64
    def ipm_soft_range(self, B, n, m, q, p, h, lower, gamma_u, rho_u, gamma_l, rho_l, gt1, b, factors, sfac, eps, maxIter,
                       notImprovedLim, stall_policy, zhat, nu, lam, slack, lam_lo, slack_lo, lam_t, slack_t, lam_tl, slack_tl,
                       t, t_lo, iters, status, best_resid, trace=None):
        """lower and the four penalty vectors (B,m), (1,m) or (m,) (shared: batch stride 0); -inf in lower = a one-sided row,
        +inf in a side's gamma or rho = a hard side; gt1 (B,) = || G'^T 1 ||"""
        lp, gu, ru, gl, rl = Param(lower, 2), Param(gamma_u, 2), Param(rho_u, 2), Param(gamma_l, 2), Param(rho_l, 2)
        common = (B, n, m, q, p, h, b, factors, sfac, eps, maxIter, notImprovedLim, stall_policy,
                  zhat, nu, lam, slack, iters, status, best_resid, trace)
        self._ipm_call(self.dll.qpx_ipm_soft_range, common,
                       lp.ptr, lp.stride, gu.ptr, gu.stride, ru.ptr, ru.stride, gl.ptr, gl.stride, rl.ptr, rl.stride, _ptr(gt1),
                       _ptr(lam_lo), _ptr(slack_lo), _ptr(lam_t), _ptr(slack_t), _ptr(lam_tl), _ptr(slack_tl), _ptr(t), _ptr(t_lo))

    # -- forward mode (QPFunctionFn.jvp): the tangent of the solution, one KKT solve with the backward's matrix
    def jvp(self, B, n, m, q, factors, sfac, zhat, lam, slack, nu, tQ, tp, tG, th, tA, tb, dzhat, status,
            dlam=None, dnu=None, dslack=None, refine=0, Q=None, G=None, A=None, wide=False):
        """tQ .. tb: any may be None (zero); un-batched, batch-1 and expanded tangents go in with batch stride 0 (Param)"""
        t = [Param(tQ, 3), Param(tp, 2), Param(tG, 3), Param(th, 2), Param(tA, 3), Param(tb, 2)]
        Qp, Gp, Ap = Param(Q, 3), Param(G, 3), Param(A, 3)
        self.check(self.dll.qpx_jvp(
            _code(factors, wide), B, n, m, q, _ptr(factors), int(sfac), _ptr(zhat), _ptr(lam), _ptr(slack), _ptr(nu),
            t[0].ptr, t[0].stride, t[1].ptr, t[1].stride, t[2].ptr, t[2].stride, t[3].ptr, t[3].stride,
            t[4].ptr, t[4].stride, t[5].ptr, t[5].stride, _ptr(dzhat), _ptr(dlam), _ptr(dnu), _ptr(dslack),
            int(refine), Qp.ptr, Qp.stride, Gp.ptr, Gp.stride, Ap.ptr, Ap.stride, _ptr(status), _stream(factors)))

    # -- the second-order pass of the backward: one launch, one factorisation, two dependent solves
    def backward2(self, B, n, m, q, factors, sfac, zhat, lam, slack, nu, dx, dz, dy, WQ, Wp, WG, Wh, WA, Wb,
                  zdot, lamdot, nudot, HQ, Hp, HG, Hh, HA, Hb, status, wide=False):
        """dx, dz, dy: the first backward's KKT solution, dense (B, .); WQ .. Wb: cotangents on its six gradients, any may be
        None (zero), shared ones go in with batch stride 0 (Param); lamdot, nudot, HQ .. Hb: any may be None (not wanted)"""
        t = [Param(WQ, 3), Param(Wp, 2), Param(WG, 3), Param(Wh, 2), Param(WA, 3), Param(Wb, 2)]
        self.check(self.dll.qpx_backward2(
            _code(factors, wide), B, n, m, q, _ptr(factors), int(sfac), _ptr(zhat), _ptr(lam), _ptr(slack), _ptr(nu),
            _ptr(dx), _ptr(dz), _ptr(dy),
            t[0].ptr, t[0].stride, t[1].ptr, t[1].stride, t[2].ptr, t[2].stride, t[3].ptr, t[3].stride,
            t[4].ptr, t[4].stride, t[5].ptr, t[5].stride, _ptr(zdot), _ptr(lamdot), _ptr(nudot),
            _ptr(HQ), _ptr(Hp), _ptr(HG), _ptr(Hh), _ptr(HA), _ptr(Hb), _ptr(status), _stream(factors)))

    # -- batch.py:92-198 in the original variables, as a finishing stage (KKTSolvers.IR_UNOPT, float32 refine=k)
    def polish(self, B, n, m, q, Q, p, G, h, A, b, factors, sfac, steps, refine, zhat, nu, lam, slack, best_resid, status):
        Qp, Gp, Ap = Param(Q, 3), Param(G, 3), Param(A, 3)
        pp, hp, bp = Param(p, 2), Param(h, 2), Param(b, 2)
        self.check(self.dll.qpx_polish(
            _dtype_code(factors), B, n, m, q, Qp.ptr, Qp.stride, pp.ptr, pp.stride, Gp.ptr, Gp.stride, hp.ptr, hp.stride,
            Ap.ptr, Ap.stride, bp.ptr, bp.stride, _ptr(factors), int(sfac), int(steps), int(refine),
            _ptr(zhat), _ptr(nu), _ptr(lam), _ptr(slack), _ptr(best_resid), _ptr(status), _stream(factors)))

    # -- Newton's method onto the central-path point s lam = kappa, from a loop launch's iterate
    def centre(self, B, n, m, q, Q, p, G, h, A, b, factors, sfac, kappa, tol, max_steps, zhat, nu, lam, slack, resid, steps, status):
        """kappa (B,m) or (m,) / (1,m) (shared: batch stride 0)"""
        Qp, Gp, Ap = Param(Q, 3), Param(G, 3), Param(A, 3)
        pp, hp, bp, kp = Param(p, 2), Param(h, 2), Param(b, 2), Param(kappa, 2)
        self.check(self.dll.qpx_centre(
            _dtype_code(factors), B, n, m, q, Qp.ptr, Qp.stride, pp.ptr, pp.stride, Gp.ptr, Gp.stride, hp.ptr, hp.stride,
            Ap.ptr, Ap.stride, bp.ptr, bp.stride, _ptr(factors), int(sfac), kp.ptr, kp.stride, float(tol), int(max_steps),
            _ptr(zhat), _ptr(nu), _ptr(lam), _ptr(slack), _ptr(resid), _ptr(steps), _ptr(status), _stream(factors)))

    # -- qp.py:159-177, the `.mean(0)` of a shared parameter's gradient as one contraction over the batch
    def batch_outer(self, u, v, w, x, scale, out):
        """v is None: the batch mean of u's columns times `scale` (out: (r,)); w, x None: one product only"""
        B, r = u.shape
        c = v.shape[1] if v is not None else 1
        code = _dtype_code(out)
        # long batches: partial tiles per batch chunk in a workspace, summed in chunk order by a second launch
        need = int(self.dll.qpx_batch_outer_workspace_elems(code, B, r, c))
        ws = torch.empty(need, dtype=out.dtype, device=out.device) if need else None
        self.check(self.dll.qpx_batch_outer(code, B, r, c, _ptr(u), _ptr(v), _ptr(w), _ptr(x),
                                            float(scale), _ptr(out), _ptr(ws), need, _stream(out)))


    # -- scenario batches: B groups of K consecutive QPs, one blob per group ----------------------
    def group_supported(self, dtype_code, n, m, q):
        return bool(self.dll.qpx_group_supported(dtype_code, n, m, q))

    def ipm_group(self, B, K, n, m, q, p, h, b, factors, sfac, eps, maxIter, notImprovedLim, stall_policy,
                  zhat, nu, lam, slack, iters, status, best_resid, trace=None, wide=False):
        """qpx_ipm_group: every per-QP tensor has B K rows (p, h, b may be shared: batch stride 0); `factors` holds B blobs"""
        pp, hp, bp = Param(p, 2), Param(h, 2), Param(b, 2)
        self.check(self.dll.qpx_ipm_group(
            _code(factors, wide), B, int(K), n, m, q, pp.ptr, pp.stride, hp.ptr, hp.stride, bp.ptr, bp.stride,
            _ptr(factors), int(sfac), float(eps), int(maxIter), int(notImprovedLim), int(stall_policy),
            _ptr(zhat), _ptr(nu), _ptr(lam), _ptr(slack), _ptr(iters), _ptr(status), _ptr(best_resid),
            _ptr(trace), _stream(factors)))

    def backward_group(self, B, K, n, m, q, factors, sfac, zhat, lam, slack, nu, dl_dz, dp, dh, db, status,
                       dx=None, dz=None, dy=None, wide=False, dl_dlam=None, dl_dnu=None):
        """qpx_backward_group: dp, dh, db per QP (any may be None); the matrices' gradients come from dx, dz, dy (group_outer)"""
        self.check(self.dll.qpx_backward_group(
            _code(factors, wide), B, int(K), n, m, q, _ptr(factors), int(sfac), _ptr(zhat), _ptr(lam), _ptr(slack),
            _ptr(nu), _ptr(dl_dz), _ptr(dl_dlam), _ptr(dl_dnu), None, _ptr(dp), None, _ptr(dh), None, _ptr(db),
            _ptr(dx), _ptr(dz), _ptr(dy), 0, None, 0, None, 0, None, 0, _ptr(status), _stream(factors)))

    def group_outer(self, K, u, v, w, x, scale, out):
        """out (B, r, c): out[g] = scale * sum over group g's K consecutive rows of (u^T v + w^T x); w, x None: one product"""
        BK, r = u.shape
        B, c = BK // int(K), v.shape[1]
        assert B * int(K) == BK and out.shape == (B, r, c) and out.is_contiguous()
        code = _dtype_code(out)
        need = int(self.dll.qpx_group_outer_workspace_elems(code, B, int(K), r, c))
        ws = torch.empty(need, dtype=out.dtype, device=out.device) if need else None
        self.check(self.dll.qpx_group_outer(code, B, int(K), r, c, _ptr(u), _ptr(v), _ptr(w), _ptr(x),
                                            float(scale), _ptr(out), _ptr(ws), need, _stream(out)))

    # -- the neq x neq correction of factor_solve_kkt_reg (batch.py:273-310): x = M^-1 r, M destroyed, r overwritten
    def dense_solve(self, M, rhs, status=None):
        B, k = rhs.shape
        assert M.shape == (B, k, k) and M.is_contiguous() and rhs.is_contiguous() and M.dtype == rhs.dtype
        self.check(self.dll.qpx_dense_solve(_dtype_code(rhs), B, k, _ptr(M), _ptr(rhs), _ptr(status), _stream(rhs)))
        return rhs


_HIP = None
_TEST_BACKEND = None


def hip():
    """The product backend: libqpx_hip.so.  Raises if it has not been built."""
    global _HIP
    if _HIP is None:
        _HIP = QpxLib(HIP_SO)
    return _HIP


def set_test_backend(lib):
    """tests/emu only: route calls to a QpxLib over the host-thread emulator (or None to undo)."""
    global _TEST_BACKEND
    _TEST_BACKEND = lib


def backend_for(t):
    """Backend that must execute work on tensor `t`.  CPU tensors are refused unless a test has
    explicitly installed the emulator."""
    if _TEST_BACKEND is not None:
        return _TEST_BACKEND
    if not t.is_cuda:
        raise RuntimeError(
            "qpth_amd runs on AMD Instinct GPUs only (got a %s tensor); there is no CPU fallback. "
            "Move Q, p, G, h, A, b to a HIP device." % t.device)
    return hip()
