"""Device-resident KKT factor state of one batch and the launches that use it.

`KKTFactors` is what the reference keeps as (Q_LU, S_LU, R) on ctx between forward and
backward (qpth/qp.py:93,150-155): here one HBM blob per QP written by qpx_pre_factor
(layout: qpth_amd/csrc/qpx_layout.h) plus the recorded `d` of factor_kkt.  When Q, G and A
are all shared by the batch (un-batched parameters, qpth/util.py:44-50) the blob is built
once and every workgroup reads the same copy.
"""
import contextlib
import threading

import numpy as np
import torch

from . import _lib

MULTI_RHS_BLOCK = 4      # right-hand sides per block of qpx_factor_solve_kkt_multi, every kernel form (csrc/qpx_forms.h: kKktMultiRB)

_STALL_POLICY = None     # None = automatic (reference counter for B == 1, floor rule otherwise)


def set_stall_policy(policy):
    """Override how `notImprovedLim` is applied per QP (see include/qpx.h); None = automatic."""
    global _STALL_POLICY
    assert policy in (None, _lib.STALL_OFF, _lib.STALL_REFERENCE, _lib.STALL_FLOOR)
    _STALL_POLICY = policy


def default_stall_policy(B):
    if _STALL_POLICY is not None:
        return _STALL_POLICY
    return _lib.STALL_REFERENCE if B == 1 else _lib.STALL_FLOOR


class IpmResult:
    __slots__ = ("zhat", "nu", "lam", "slacks", "iters", "status", "best_resid", "trace", "_warm_used",
                 "centre_resid", "centre_steps",         # these two: set by KKTFactors.centre only
                 "lam_lo", "slacks_lo",                  # ... these by KKTFactors.ipm_range only
                 "lam_t", "slacks_t", "t",               # ... these by KKTFactors.ipm_elastic and ipm_soft_range
                 "lam_tl", "slacks_tl", "t_lo")          # ... and these by KKTFactors.ipm_soft_range only

    @property
    def warm_used(self):
        """int32 (B,): 1 where the loop took the warm entry (KKTFactors.ipm(warm=...)).  A cold call has zeros here, made
        when first asked for: the cold path pays no launch for them."""
        if self._warm_used is None:
            self._warm_used = torch.zeros(self.iters.shape, dtype=torch.int32, device=self.iters.device)
        return self._warm_used


class WarmStart:
    """The (lam, slacks) of the previous solve of a batch, kept between calls so that the next solve of a nearby batch
    starts there (QPFunction(warm_start=ws), sensitivity.solve(warm_start=ws)):

        ws = qpth_amd.WarmStart()
        for step in range(steps):
            z = QPFunction(warm_start=ws)(Q, p, G, h, A, b)      # first call cold, every later one from the last solution

    A small holder: `lam`, `slacks` are the tensors the last forward produced (detached references, no copy), `used` the
    int32 (B,) tensor of that forward (1 where the loop took the warm entry; None before the first call), `floor` the
    value both are floored at on entry.  A holder whose tensors do not match the call -- another (B, nineq), dtype or
    device -- is ignored (that call is cold) and overwritten.  `clear()` empties it: the next call is cold."""

    def __init__(self, floor=1e-2):
        if not (floor > 0 and floor < float("inf")):
            raise ValueError("qpth_amd: WarmStart floor must be positive and finite, got %r" % (floor,))
        self.floor = float(floor)
        self.clear()

    def clear(self):
        self.lam = self.slacks = self.used = None

    def matches(self, B, m, dtype, device):
        return all(X is not None and tuple(X.shape) == (B, m) and X.dtype == dtype and X.device == device
                   for X in (self.lam, self.slacks))

    def take(self, res):
        """keep what a forward produced (KKTFactors.ipm's / polish's result)"""
        self.lam, self.slacks, self.used = res.lam.detach(), res.slacks.detach(), res.warm_used

    def pair(self, B, m, dtype, device):
        """(lam, slacks) for KKTFactors.ipm(warm=...), or None when the holder is empty or of another batch"""
        return (self.lam, self.slacks) if self.matches(B, m, dtype, device) else None


class RangeWarmStart:
    """WarmStart for two-sided rows, lower <= G z <= h: the (lam, slacks, lam_lo, slacks_lo) of the previous solve of a batch
    (QPFunction(warm_start=rws)(Q, p, G, h, A, b, lower=l), sensitivity.solve(..., lower=l, warm_start=rws)):

        rws = qpth_amd.RangeWarmStart()
        for step in range(steps):
            z = QPFunction(warm_start=rws)(Q, p, G, h, A, b, lower=l)      # first call cold, every later one warm

    A type of its own on purpose: a holder filled by a one-sided solve has nothing for the lower side, so handing a
    WarmStart to a call with `lower` (or this one to a call without) is an error, not a silent cold start.  `used`, `floor`,
    `clear()` and the rule for a holder of another (B, nineq), dtype or device are WarmStart's.  Which rows are two-sided may
    change between calls: a row that was one-sided in the previous solve and is two-sided now carries 0 / +inf on its lower
    side, and that QP starts cold (`used` says so); the other way round its lower entries are simply not read."""

    def __init__(self, floor=1e-2):
        if not (floor > 0 and floor < float("inf")):
            raise ValueError("qpth_amd: RangeWarmStart floor must be positive and finite, got %r" % (floor,))
        self.floor = float(floor)
        self.clear()

    def clear(self):
        self.lam = self.slacks = self.lam_lo = self.slacks_lo = self.used = None

    def matches(self, B, m, dtype, device):
        return all(X is not None and tuple(X.shape) == (B, m) and X.dtype == dtype and X.device == device
                   for X in (self.lam, self.slacks, self.lam_lo, self.slacks_lo))

    def take(self, res):
        """keep what a forward produced (KKTFactors.ipm_range's result)"""
        self.lam, self.slacks, self.lam_lo, self.slacks_lo = (res.lam.detach(), res.slacks.detach(), res.lam_lo.detach(),
                                                              res.slacks_lo.detach())
        self.used = res.warm_used

    def quad(self, B, m, dtype, device):
        """(lam, slacks, lam_lo, slacks_lo) for KKTFactors.ipm_range(warm=...), or None when the holder is empty or of another batch"""
        return (self.lam, self.slacks, self.lam_lo, self.slacks_lo) if self.matches(B, m, dtype, device) else None


def _batch_of(*params3):
    for X in params3:
        if X is not None and X.nelement() > 0 and X.dim() == 3:
            return X.size(0)
    return 1


def _is_shared(X, B):
    if X is None or X.nelement() == 0:
        return True
    return X.dim() == 2 or X.stride(0) == 0 or (B > 1 and X.size(0) == 1)


def _row_param(x, name, Q, nineq, nBatch, scalar_ok=True):
    """A per-row parameter as every entry point takes it: a tensor of Q's dtype and device, shape (nBatch, nineq), (nineq,) or
    -- scalar_ok -- (), or then a Python number (-> a 0-dim tensor).  Raises ValueError, naming it `name`, otherwise."""
    shapes = "(nBatch, %d), (%d,) or ()" % (nineq, nineq) if scalar_ok else "(nBatch, %d) or (%d,)" % (nineq, nineq)
    if not torch.is_tensor(x):
        if not scalar_ok:
            raise ValueError("qpth_amd: %s must be a tensor of shape %s" % (name, shapes))
        x = torch.tensor(float(x), dtype=Q.dtype, device=Q.device)
    if x.dtype != Q.dtype or x.device != Q.device:
        raise ValueError("qpth_amd: %s is %s on %s, the QP is %s on %s" % (name, x.dtype, x.device, Q.dtype, Q.device))
    if (x.dim() > 2 or (x.dim() == 0 and not scalar_ok) or (x.dim() >= 1 and x.size(-1) != nineq)
            or (x.dim() == 2 and nBatch > 1 and x.size(0) != nBatch)):
        raise ValueError("qpth_amd: %s has shape %s; expected %s" % (name, tuple(x.shape), shapes))
    return x


def as_rho(rho, Q, nineq, nBatch=1):
    """The penalties of the soft rows as every entry point takes them: a tensor of Q's dtype and device, shape
    (nBatch, nineq), (nineq,) or (), or a Python number (-> a 0-dim tensor).  Raises ValueError otherwise; the VALUES
    (> 0, +inf = a hard row) are checked by the pre-factorisation kernel (KKTFactors.raise_on_failure)."""
    return _row_param(rho, "rho", Q, nineq, nBatch)


def as_kappa(kappa, Q, nineq, nBatch=1):
    """The barrier weights of the smoothed QP as every entry point takes them, as as_rho: a tensor of Q's dtype
    and device, shape (nBatch, nineq), (nineq,) or (), or a Python number (-> a 0-dim tensor).  Raises ValueError otherwise;
    the VALUES (finite, > 0) are checked by the centring kernel."""
    return _row_param(kappa, "kappa", Q, nineq, nBatch)


def as_lower(lower, Q, nineq, nBatch=1):
    """The lower bounds of two-sided rows as every entry point takes them, as as_rho takes shapes: a tensor of Q's
    dtype and device, shape (nBatch, nineq) or (nineq,) (shared by the batch); -inf = a one-sided row.  Raises ValueError
    otherwise; the VALUES (below h, not NaN, not +inf) are checked by the loop kernel."""
    return _row_param(lower, "lower", Q, nineq, nBatch, scalar_ok=False)


def as_l1(l1, Q, nineq, nBatch=1):
    """The linear penalties of elastic rows as every entry point takes them, as as_rho: a tensor of Q's dtype and
    device, shape (nBatch, nineq), (nineq,) or (), or a Python number (-> a 0-dim tensor).  Raises ValueError otherwise; the
    VALUES (>= 0, +inf = a hard row) are checked by the loop kernel."""
    return _row_param(l1, "l1", Q, nineq, nBatch)


def _rows(x, nineq, detach=True):
    """a per-row parameter of any of its shapes as rows (nBatch | 1, nineq), detached"""
    if detach:
        x = x.detach()
    return x.expand(nineq).unsqueeze(0) if x.dim() < 2 else x


def _reduce_like(g, dim):
    """a per-QP gradient (nBatch, nineq) reduced to the shape of the caller's input of `dim` dimensions: `.mean(0)` below two
    (shared by the batch), summed over the rows as well at zero (a scalar)"""
    if dim < 2:
        g = g.mean(0)
    if dim == 0:
        g = g.sum()
    return g


class SoftRange:
    """The bounds and penalties of SOFT two-sided rows, the value of QPFunction(...)(..., soft_range=):
          min 1/2 z'Qz + p'z + sum_i ( l1_i tu_i + 1/2 rho_i tu_i^2 + l1_lower_i tl_i + 1/2 rho_lower_i tl_i^2 )
          s.t.  lower - tl <= Gz <= h + tu,  tu, tl >= 0,  Az = b.
    Each field is a tensor of shape (nBatch, nineq), (nineq,) (shared by the batch) or () (one for every row), or a Python
    float; l1_lower and rho_lower default to the upper side's l1 and rho.  lower = -inf makes a row one-sided; l1 = +inf or
    rho = +inf on a side makes that side hard.  Immutable; the tensors among the five fields that require grad are
    differentiable inputs of the call."""
    __slots__ = ("lower", "l1", "rho", "l1_lower", "rho_lower")

    def __init__(self, lower, l1, rho, l1_lower=None, rho_lower=None):
        for name, val in (("lower", lower), ("l1", l1), ("rho", rho), ("l1_lower", l1 if l1_lower is None else l1_lower),
                          ("rho_lower", rho if rho_lower is None else rho_lower)):
            if val is None:
                raise ValueError("qpth_amd: SoftRange needs %s" % name)
            object.__setattr__(self, name, val)

    def __setattr__(self, name, value):
        raise AttributeError("SoftRange is immutable")

    def __repr__(self):
        return "SoftRange(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)

    def fields(self, Q, nineq, nBatch=1):
        """the five fields as tensors of Q's dtype and device (a number -> a 0-dim tensor), shapes checked as as_rho does;
        the VALUES are checked by the loop kernel"""
        return [_row_param(getattr(self, name), "soft_range." + name, Q, nineq, nBatch) for name in self.__slots__]


class _PinnedPool:
    """Pinned int32 host buffers for the one small D2H copy behind a pre-factorisation (the per-QP status words).  A buffer
    belongs to exactly ONE KKTFactors from `take` until that object has read it (raise_on_failure) or dies; only then can
    another build() get it -- nothing is handed out twice however many builds are outstanding, and two host threads may
    build at once (autograd runs backward on threads of its own).  Allocating pinned memory per call would cost more than
    the kernels the asynchronous copy lets the host overlap, hence the free lists."""

    def __init__(self):
        self._lock = threading.Lock()
        self._free = {}
        self._pending = []          # (event, key, buffer): given up by their owner while the copy was still in flight

    @staticmethod
    def _done(ev):
        """True / False: the event has / has not completed; None: it cannot be asked (recorded inside a stream capture):
        the buffer behind it is dropped rather than handed out"""
        try:
            return bool(ev.query())
        except Exception:
            return None

    def take(self, device, count, may_allocate=True):
        key = (device.type, device.index, int(count))
        with self._lock:
            if self._pending:
                still = []
                for ev, k, buf in self._pending:
                    done = self._done(ev)
                    if done:
                        self._free.setdefault(k, []).append(buf)
                    elif done is not None:
                        still.append((ev, k, buf))
                self._pending = still
            lst = self._free.get(key)
            if lst:
                return key, lst.pop()
        if not may_allocate:
            return key, None
        return key, torch.zeros(count, dtype=torch.int32).pin_memory()

    def give(self, key, buf, event=None, keep=32):
        """event: the copy into `buf` may still be in flight -- the buffer is free once the event has completed"""
        with self._lock:
            done = True if event is None else self._done(event)
            if not done:
                if done is not None and len(self._pending) < keep:
                    self._pending.append((event, key, buf))
                return
            lst = self._free.setdefault(key, [])
            if len(lst) < keep:
                lst.append(buf)


_PINNED = _PinnedPool()


class KKTFactors:
    _entry_words = None      # (status and bad-entry words, event, messages) of a row role's launch, until raise_on_failure reads them

    @classmethod
    def build(cls, Q, G, A, nBatch=None, wide=False, w=None, scenarios=None):
        """pre_factor_kkt(Q, G, A)   (batch.py:375-429); enqueues one kernel, no host sync.
        scenarios=K: nBatch GROUPS of K consecutive QPs, a group sharing its (Q, G, A) and so one blob -- nBatch
        blobs are built, and everything behind build() works on nBatch K QPs: `B` is nBatch K, `status` has nBatch K words
        (a group's pre-factorisation word repeated for its K QPs), ipm / backward (duals' cotangents included) /
        raise_on_failure take and return nBatch K rows; backward hands a batched matrix's gradient back per GROUP, (nBatch, ., .),
        summed over the group's QPs.  Sizes of qpx_group_supported only (RuntimeError otherwise), no soft rows; the launches
        beside ipm and backward (solve_kkt, polish, centre, jvp, backward2, the row roles) are not served on such factors.
        Q, G, A all shared by the batch: the one-blob path on nBatch K QPs, as without scenarios.
        wide: float32 tensors, float64 factors and arithmetic (QPX_F32_WIDE, include/qpx.h): every later call on these
        factors takes and returns float32 tensors, the blob is float64.
        w (B, nineq), (1, nineq) or (nineq,), >= 0: soft rows -- the factors of the QP with the penalty 1/2 sum t_i^2 / w_i on
        the violation of G z <= h + t, w_i = 0 a hard row (qpx_pre_factor_soft).  Every launch on soft factors
        serves the softened QP; they have no refinement and no finishing stage (refine_ok, polish_ok are False: both
        would evaluate residuals of the hard QP).  A w per QP beside Q, G, A the batch shares means one blob per QP."""
        self = cls()
        self.soft = w is not None
        self.wide = bool(wide)
        if self.wide and Q.dtype != torch.float32:
            raise TypeError("qpth_amd: wide=True is for float32 tensors")
        B = nBatch if nBatch is not None else _batch_of(Q, G, A)
        self.K = None                 # scenarios per group, or None: one blob per QP / one for the batch
        if scenarios is not None:
            K = int(scenarios)
            if K < 1:
                raise ValueError("qpth_amd: scenarios must be a positive integer, got %r" % (scenarios,))
            if self.soft:
                raise ValueError("qpth_amd: scenarios= with soft rows (w / rho) is not served; build the expanded batch instead")
            if _is_shared(Q, B) and _is_shared(G, B) and _is_shared(A, B):
                B = B * K             # nothing is per group: the one-blob path on all the QPs
            else:
                self.K = K
        self.groups = B               # blobs when K is set
        self.B = B
        self.n = Q.size(-1)
        self.m = G.size(-2)
        self.q = A.size(-2) if (A is not None and A.nelement() > 0) else 0
        if G.size(-1) != self.n or Q.size(-2) != self.n or (self.q and A.size(-1) != self.n):
            raise RuntimeError("qpth_amd: inconsistent QP sizes Q%s G%s A%s" % (
                tuple(Q.shape), tuple(G.shape), tuple(A.shape) if A is not None else ()))
        for X, what in ((Q, "Q"), (G, "G"), (A if self.q else None, "A")):
            if X is None:
                continue
            if X.dtype != Q.dtype or X.device != Q.device:
                raise RuntimeError("qpth_amd: %s is %s on %s but Q is %s on %s (all of Q, p, G, h, A, b must share one "
                                   "dtype and one device)" % (what, X.dtype, X.device, Q.dtype, Q.device))
            if X.dim() not in (2, 3) or (X.dim() == 3 and X.size(0) not in (1, B)):
                raise RuntimeError("qpth_amd: %s has shape %s for a batch of %d" % (what, tuple(X.shape), B))
        if self.soft:
            if w.dtype != Q.dtype or w.device != Q.device:
                raise RuntimeError("qpth_amd: w (1 / rho) is %s on %s but Q is %s on %s" % (w.dtype, w.device, Q.dtype, Q.device))
            if tuple(w.shape) not in ((self.m,), (1, self.m), (B, self.m)):
                raise RuntimeError("qpth_amd: w (1 / rho) has shape %s, expected (%d, %d) or (%d,)" % (tuple(w.shape), B, self.m, self.m))
            w = w.detach()
        self.lib = _lib.backend_for(Q)
        self.dtype, self.device = Q.dtype, Q.device
        self.Q, self.G, self.A = Q, G, (A if self.q else None)     # the original data: iterative refinement evaluates residuals with it
        # the dtype code of every call on these factors (include/qpx.h)
        self.code = code = _lib.QPX_F32_WIDE if self.wide else (_lib.QPX_F64 if Q.dtype == torch.float64 else _lib.QPX_F32)
        self.elems = self.lib.factor_elems(code, self.n, self.m, self.q)
        # the A/B knob of the library is per host thread and selects the blob layout: remember the value the
        # factors are built under and re-apply it around every later call on them (autograd runs backward
        # on its own thread)
        self.variant = int(self.lib.dll.qpx_get_ipm_variant())
        # does the kernel family that serves this size refine KKT solves in the kernel (qpx_factor_solve_kkt(..., refine))?
        # (a pre-v5 build loaded non-strictly by scripts/ab_bench.py has no such symbol: it ignored `refine` where it could not refine)
        self.refine_ok = bool(self.lib.dll.qpx_refine_supported(code, self.n, self.m, self.q)) if hasattr(self.lib.dll, "qpx_refine_supported") else True
        # ... and does it have the finishing stage as a kernel (qpx_polish)?  Asked here, under the knob the factors are built
        # with: the answer depends on the calling thread's knob, and polish() may be reached from another thread
        pcode = _lib.QPX_F64 if Q.dtype == torch.float64 else _lib.QPX_F32
        self.polish_ok = (not self.wide and hasattr(self.lib.dll, "qpx_polish_supported")
                          and bool(self.lib.dll.qpx_polish_supported(pcode, self.n, self.m, self.q)))
        share_ok = bool(self.lib.dll.qpx_can_share_factors(code, self.n, self.m, self.q))
        self.shared = B > 1 and share_ok and _is_shared(Q, B) and _is_shared(G, B) and _is_shared(A, B)
        if self.K is not None:
            if not self.lib.group_supported(code, self.n, self.m, self.q):
                raise RuntimeError("qpth_amd: scenarios= is not served at nz = %d, nineq = %d, neq = %d (qpx_group_supported: the "
                                   "large-QP family keeps per-QP work matrices in the blob); build the expanded batch instead"
                                   % (self.n, self.m, self.q))
            self.refine_ok = self.polish_ok = False
            self.B = B * self.K
        if self.soft:
            self.refine_ok = self.polish_ok = False
            w_shared = w.dim() == 1 or w.stride(0) == 0 or (B > 1 and w.size(0) == 1)
            self.shared = self.shared and w_shared
            if not self.shared and w_shared:
                w = w.reshape(1, self.m)[:1].expand(B, self.m)      # per-QP blobs: the kernel reads it with batch stride 0
        self.w = w
        nblob = 1 if self.shared else B
        self.sfac = 0 if self.shared else self.elems
        self.blob = torch.empty(nblob * self.elems, dtype=torch.float64 if self.wide else Q.dtype, device=Q.device)
        self.status = torch.empty(B, dtype=torch.int32, device=Q.device)      # every pre-factorisation kernel writes it
        with self._knob():
            self.lib.pre_factor(nblob, self.n, self.m, self.q, Q, G, A if self.q else None, self.blob, self.status,
                                wide=self.wide, w=w)
        if self.shared:
            self.status[1:] = self.status[0]
        if self.K is not None:
            # a word per QP for the loop and the backward to OR their bits into: the group's, K times (the pinned copy below
            # reads `pre`, the groups' words as the kernel wrote them)
            pre = self.status
            # (repeat always materialises -- the kernels index raw words --, one copy kernel, no host sync: capturable)
            self.status = pre.unsqueeze(1).repeat(1, self.K).reshape(-1)
        # The reference raises on a bad Q / A from inside forward (qp.py:81-85, batch.py:379-386).  The two
        # status bits that matter are final once the pre-factorisation kernel has run, so the status words are
        # copied to pinned host memory right behind it and read (raise_on_failure) after the loop kernel
        # has been enqueued: the host waits for the pre-factorisation only, never for the IPM loop.
        self._pre_host = self._pre_event = self._pre_key = self._pre_bits = None
        if self.status.is_cuda:
            # one DMA of the per-QP status words, no reduction kernels in the stream.  (While the stream is being captured
            # into a graph the pool is left alone -- allocating pinned memory or asking an event would invalidate the
            # capture: the words stay on the device and raise_on_failure reads them from there.)
            if not torch.cuda.is_current_stream_capturing():
                self._pre_key, self._pre_host = _PINNED.take(self.device, nblob)
            if self._pre_host is not None:
                self._pre_host.copy_((pre if self.K is not None else self.status)[:nblob], non_blocking=True)
                self._pre_event = torch.cuda.Event()
                self._pre_event.record(torch.cuda.current_stream(self.device))
        # soft rows: a bad entry of w is the pre-factorisation's QPX_ST_NONFINITE, a bit the loop may set too -- where no
        # pinned copy holds the words as the pre-factorisation left them, a copy on the device does
        self._pre_soft = self.status[:nblob].clone() if (self.soft and self._pre_event is None) else None
        return self

    def _release_pinned(self, done):
        """the pinned buffer goes back to the pool: at once when the copy into it has completed (`done`), else behind its event"""
        host, key = self._pre_host, self._pre_key
        self._pre_host = self._pre_key = None
        if host is not None:
            _PINNED.give(key, host, None if done else self._pre_event)

    def __del__(self):
        try:
            if getattr(self, "_pre_host", None) is not None:
                self._release_pinned(False)
        except Exception:          # interpreter shutdown: nothing to give back to
            pass

    @contextlib.contextmanager
    def _knob(self):
        """around every launch on these factors: the library's A/B knob as it was when they were built, and THEIR
        device current (the launchers opt kernels into > 64 KiB of LDS per device and fork side streams from the
        current device's pool: tensors on cuda:1 while cuda:0 is current must not reach them that way)"""
        dll = self.lib.dll
        old = dll.qpx_set_ipm_variant(self.variant)
        guard = torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext()
        try:
            with guard:
                yield
        finally:
            dll.qpx_set_ipm_variant(old)

    # -- error surface of pre_factor_kkt / QPFunction (qp.py:81-85, batch.py:379-386) ------
    def raise_on_failure(self, check_Q_spd=False):
        mask = _lib.ST_Q_NOT_SPD | _lib.ST_A_RANK
        if self.soft:
            mask |= _lib.ST_NONFINITE
        bad_entry = None
        staged, self._entry_words = self._entry_words, None
        if staged is not None:
            # the row roles (ipm_range, ipm_elastic, ipm_soft_range): the words _stage_entry_checks copied in FRONT of the loop
            # launch -- the pre-factorisation's status and, per check and QP, whether an entry fails the loop's own test (formed
            # by torch operations): they stand in for the read-back of the pre-factorisation's words, and the host still never
            # waits for the loop
            host, ev, msgs = staged
            if ev is not None:
                ev.synchronize()
            words = host.cpu().numpy()
            self._pre_bits = int(np.bitwise_or.reduce(words[0]))      # (a later call reads these, not the pinned buffer)
            st = self._pre_bits & mask
            for row, msg in zip(words[1:], msgs):
                if row.any():
                    bad_entry = bad_entry or msg
            if self._pre_host is not None:
                self._release_pinned(False)
        elif self._pre_soft is not None:
            st = int(np.bitwise_or.reduce(self._pre_soft.cpu().numpy().reshape(-1))) & mask
        elif self._pre_event is not None:
            if self._pre_bits is None:         # first reading: wait for the copy, keep the bits, free the buffer
                self._pre_event.synchronize()
                self._pre_bits = int(np.bitwise_or.reduce(self._pre_host.numpy()))
                self._release_pinned(True)
            st = self._pre_bits & mask
        else:
            st = int(np.bitwise_or.reduce(self.status.cpu().numpy().reshape(-1))) & mask
        if st & _lib.ST_Q_NOT_SPD:
            if check_Q_spd:
                raise RuntimeError('Q is not SPD.')
            raise RuntimeError("""
qpth Error: Cannot perform LU factorization on Q.
Please make sure that your Q matrix is PSD and has
a non-zero diagonal.
""")
        if st & _lib.ST_A_RANK:
            raise RuntimeError("qpth_amd Error: A Q^-1 A^T is not positive definite; "
                               "the equality constraints must have full row rank.")
        if st & _lib.ST_NONFINITE:
            raise ValueError("rho must be positive")
        if bad_entry:
            raise ValueError(bad_entry)

    def _no_groups(self, bad=True, what=None):
        """scenario groups (build(scenarios=K)) have the loop and the backward: every other launch indexes the blob by QP"""
        if self.K is not None and bad:
            raise RuntimeError("qpth_amd: %s is not served on factors built with scenarios=%d (one blob per group of %d QPs); "
                               "build the factors of the expanded batch instead" % (what, self.K, self.K))

    def _no_refine_on_soft(self, refine, what):
        """refinement evaluates residuals from the caller's Q, G, A: of the HARD QP"""
        if self.soft and refine > 0:
            raise ValueError("qpth_amd: %s with refine=%d on factors with soft rows (w / rho): in-kernel refinement evaluates the "
                             "residuals of the hard QP; pass refine=0" % (what, refine))

    def _check(self, X, k, what, batched_ok=True):
        """The kernels index raw pointers: a tensor of another dtype, device or shape must never reach them (the
        reference fails inside bmm / baddbmm with a size or dtype error; here it would be an out-of-bounds read)."""
        if X.dtype != self.dtype or X.device != self.device:
            raise RuntimeError("qpth_amd: %s is %s on %s, the factors were built for %s on %s (all of Q, p, G, h, A, b "
                               "must share one dtype and one device)" % (what, X.dtype, X.device, self.dtype, self.device))
        shape = tuple(X.shape)
        if not (shape == (k,) or (batched_ok and shape in ((self.B, k), (1, k)))):
            raise RuntimeError("qpth_amd: %s has shape %s, expected (%d, %d) or (%d,)" % (what, shape, self.B, k, k))

    def _vec(self, X, k, what="vector"):
        """dense (B,k) contiguous tensor or None"""
        if X is None or X.nelement() == 0 or k == 0:
            return None
        self._check(X, k, what)
        if X.dim() == 1 or X.size(0) != self.B:
            X = X.reshape(1, k).expand(self.B, k)
        return X.contiguous()

    def _check_ph(self, p, h):
        self._check(p, self.n, "p")
        self._check(h, self.m, "h")

    def _check_b(self, b, b_required=True):
        """b_required: equality rows with an empty b are an error of their own (the loop's entry points; polish and centre
        leave an empty b to _check)"""
        if self.q:
            if b_required and (b is None or b.nelement() == 0):
                raise RuntimeError("qpth_amd: A has %d rows but b is empty" % self.q)
            self._check(b, self.q, "b")

    def _new_result(self, maxIter, want_trace, more=()):
        """an IpmResult for one loop launch: zhat, nu, lam, slacks, every field of `more` (B, nineq), iters, best_resid, the
        trace; `status` is the factors' own words"""
        B, dt, dev = self.B, self.dtype, self.device
        r = IpmResult()
        r.zhat = torch.empty(B, self.n, dtype=dt, device=dev)
        r.nu = torch.empty(B, self.q, dtype=dt, device=dev)
        r.lam = torch.empty(B, self.m, dtype=dt, device=dev)
        r.slacks = torch.empty(B, self.m, dtype=dt, device=dev)
        for name in more:
            setattr(r, name, torch.empty(B, self.m, dtype=dt, device=dev))
        r.iters = torch.empty(B, dtype=torch.int32, device=dev)                # written on every path of the loop kernels
        r.best_resid = torch.empty(B, dtype=dt, device=dev)
        r.trace = torch.full((maxIter, B, 3), float('nan'), dtype=dt, device=dev) if want_trace else None
        r.status = self.status
        r._warm_used = None
        return r

    def _stall(self, stall_policy):
        return default_stall_policy(self.B) if stall_policy is None else stall_policy

    # -- forward (batch.py:47-207) -------------------------------------------------------
    def ipm(self, p, h, b, eps=1e-12, maxIter=20, notImprovedLim=3, stall_policy=None, want_trace=False,
            warm=None, warm_floor=1e-2):
        """The IPM loop (batch.py:47-207), one kernel launch, no host sync.  `result.status` IS the factors'
        status array: the loop ORs its bits (breakdown, maxIter, inaccurate) into the pre-factorisation's,
        so repeated calls on the same factors accumulate them.
        warm = (lam0, s0), each (B, nineq): the loop starts at z = max(lam0, warm_floor), s = max(s0, warm_floor) instead
        of the reference's start point (qpx_ipm_warm), QP by QP where all entries are finite.
        `result.warm_used`, int32 (B,): 1 where it did.  Where the kernel family has no warm entry (qpx_warm_supported: the
        large-QP family) the call is the cold one and warm_used is zeros -- no error."""
        B, n, m, q = self.B, self.n, self.m, self.q
        r = self._new_result(maxIter, want_trace)
        kw = {}
        if self.K is not None:
            # scenario groups: the same loop kernel on the B QPs, QP j reading blob j // K
            self._no_groups(warm is not None, "ipm(warm=...)")
            self._check_ph(p, h)
            self._check_b(b)
            with self._knob():
                self.lib.ipm_group(self.groups, self.K, n, m, q, p, h, b if q else None, self.blob, self.sfac, eps, maxIter,
                                   notImprovedLim, self._stall(stall_policy), r.zhat, r.nu if q else None, r.lam, r.slacks,
                                   r.iters, self.status, r.best_resid, r.trace, wide=self.wide)
            return r
        if warm is not None:
            lam0, s0 = warm
            if not (warm_floor > 0 and warm_floor < float("inf")):
                raise ValueError("qpth_amd: warm_floor must be positive and finite, got %r" % (warm_floor,))
            self._check(lam0, m, "warm[0] (lam0)")
            self._check(s0, m, "warm[1] (s0)")
            with self._knob():
                served = bool(self.lib.dll.qpx_warm_supported(self.code, n, m, q))
            if served:
                r._warm_used = torch.empty(B, dtype=torch.int32, device=self.device)          # the kernel writes every QP's word
                kw = dict(lam0=self._vec(lam0, m, "warm[0] (lam0)"), s0=self._vec(s0, m, "warm[1] (s0)"),
                          warm_floor=warm_floor, warm_used=r._warm_used)
        self._check_ph(p, h)
        self._check_b(b)
        with self._knob():
            self.lib.ipm(B, n, m, q, p, h, b if q else None, self.blob, self.sfac, eps, maxIter, notImprovedLim,
                         self._stall(stall_policy), r.zhat, r.nu if q else None, r.lam, r.slacks, r.iters, self.status,
                         r.best_resid, r.trace, wide=self.wide, **kw)
        return r

    # -- what the float64 roles beside the hard loop share: range, elastic, soft range, centre ---------------
    def _role_ok(self, symbol):
        """does the role whose qpx_*_supported is `symbol` serve these factors (under the knob they were built with)?  float64
        tensors, the thread-grid / tile kernels' sizes (nz+neq+nineq <= 208), HARD factors"""
        if self.soft or self.wide or self.K is not None or self.dtype != torch.float64 or not hasattr(self.lib.dll, symbol):
            return False
        with self._knob():
            return bool(getattr(self.lib.dll, symbol)(_lib.QPX_F64, self.n, self.m, self.q))

    # per role what _require_role takes: its qpx_*_supported, the rows as the refusal names them, the way out
    _RANGE = ("qpx_range_supported", "two-sided rows (lower)", "Write the rows as [G; -G] z <= [h; -lower]")
    _ELASTIC = ("qpx_elastic_supported", "elastic rows (l1)", "Write the augmented dense QP in (z, t)")
    _SOFT_RANGE = ("qpx_soft_range_supported", "soft two-sided rows (soft_range)", "Write the augmented dense QP in (z, tu, tl)")

    def _require_role(self, symbol, rows, way_out):
        if not self._role_ok(symbol):
            raise ValueError("qpth_amd: %s are served for float64 tensors up to nz + neq + nineq = 208 under the default knob, on hard "
                             "factors; got %s, nz = %d, nineq = %d, neq = %d%s.  %s instead"
                             % (rows, str(self.dtype).replace("torch.", ""), self.n, self.m, self.q,
                                ", soft rows" if self.soft else "", way_out))

    def _stage_entry_checks(self, r, msgs, *bad):
        """In front of a row role's loop launch.  `r.status` becomes the status words of THIS launch: a copy of the
        pre-factorisation's that the loop ORs its bits into -- a bad entry's QPX_ST_NONFINITE stays with the launch that met it,
        the factors' own words never see it.  bad: per message of `msgs` a bool tensor (B | 1, nineq) or (nineq,), true where an
        entry fails the loop's own test.  One int32 word per test and QP, stacked under the factors' status words, is
        what raise_on_failure reads: copied to pinned memory here (no stream capture: there the words stay on the device and are
        read from it), so that the host never waits for the loop."""
        r.status = self.status.clone()
        words = torch.stack([self.status] + [x.any(-1).expand(self.B).to(torch.int32) for x in bad])
        if words.is_cuda and not torch.cuda.is_current_stream_capturing():
            host = torch.empty(words.shape, dtype=torch.int32, pin_memory=True)
            host.copy_(words, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._entry_words = (host, ev, msgs)
        else:
            self._entry_words = (words, None, msgs)

    # -- two-sided rows lower <= G z <= h ---------------------------------------
    def range_ok(self):
        """do qpx_ipm_range / qpx_backward_range serve these factors (under the knob they were built with)?  float64 tensors,
        the thread-grid / tile kernels' sizes (nz+neq+nineq <= 208), no soft rows"""
        return self._role_ok("qpx_range_supported")


    def gt1_of(self, lower, h):
        """|| G^T e ||_2 per QP, e = 1 on the one-sided rows (h - lower = +inf, the kernel's test): the doubled QP's
        || G'^T 1 || of the stop rule.  torch operations, no host sync; ONE number for the batch when G, h and lower are shared."""
        G = self.G
        if h.dim() == 2 and (h.size(0) == 1 or h.stride(0) == 0):
            h = h[0]
        # (broadcast: an h per QP beside a shared lower gives an e per QP -- the kernel's test row by row, also where
        # h - lower overflows to +inf for a finite lower)
        e = torch.isinf(h - lower).to(self.dtype)
        if G.dim() == 3 and (G.size(0) == 1 or G.stride(0) == 0):
            G = G[0]
        if e.dim() == 2 and (e.size(0) == 1 or e.stride(0) == 0):
            e = e[0]
        if G.dim() == 2 and e.dim() == 1:
            return torch.linalg.vector_norm(e @ G).reshape(1).expand(self.B).contiguous()
        g = torch.matmul(e.unsqueeze(-2), G).squeeze(-2)
        return torch.linalg.vector_norm(g, dim=-1).expand(self.B).contiguous()

    def ipm_range(self, p, h, lower, b, eps=1e-12, maxIter=20, notImprovedLim=3, stall_policy=None, want_trace=False,
                  warm=None, warm_floor=1e-2):
        """The IPM loop for  lower <= G z <= h  in nineq rows (qpx_ipm_range): the iterates of ipm() on the doubled QP
        [G; -G_F] z <= [h; -lower_F], one launch, no host sync.  lower (B, nineq), (1, nineq) or (nineq,); -inf = a one-sided
        row.  The result has lam, slacks of the rows G z <= h and lam_lo, slacks_lo of lower <= G z (0 and +inf on a one-sided
        row).  A lower entry that is NaN, +inf or not below its h: QPX_ST_NONFINITE in `status` (raise_on_failure).
        warm = (lam0, s0, lam0_lo, s0_lo), each (B, nineq): the loop starts at both sides' max(., warm_floor) instead of the
        start point (qpx_ipm_range_warm), QP by QP where lam0, s0 are finite on every row and lam0_lo, s0_lo on
        the rows that are two-sided in this call (a one-sided row's lower entries are not read).  `result.warm_used`, int32
        (B,): 1 where it did."""
        self._require_role(*self._RANGE)
        B, n, m, q = self.B, self.n, self.m, self.q
        kw = {}
        if warm is not None:
            if len(warm) != 4:
                raise ValueError("qpth_amd: ipm_range takes warm = (lam0, s0, lam0_lo, s0_lo), got %d entries" % len(warm))
            if not (warm_floor > 0 and warm_floor < float("inf")):
                raise ValueError("qpth_amd: warm_floor must be positive and finite, got %r" % (warm_floor,))
            names = ("warm[0] (lam0)", "warm[1] (s0)", "warm[2] (lam0_lo)", "warm[3] (s0_lo)")
            kw = dict(warm=[self._vec(X, m, name) for X, name in zip(warm, names)], warm_floor=warm_floor)
            if any(X is None for X in kw["warm"]):
                raise ValueError("qpth_amd: ipm_range(warm=...) needs all four of lam0, s0, lam0_lo, s0_lo")
        self._check_ph(p, h)
        self._check(lower, m, "lower")
        self._check_b(b)
        r = self._new_result(maxIter, want_trace, ("lam_lo", "slacks_lo"))
        if warm is not None:
            r._warm_used = kw["warm_used"] = torch.empty(B, dtype=torch.int32, device=self.device)    # the kernel writes every QP's word
        lo, hd = lower.detach(), h.detach()
        self._stage_entry_checks(r, ("lower must be below h",), ~(lo < hd))
        gt1 = self.gt1_of(lo, hd)
        with self._knob():
            self.lib.ipm_range(B, n, m, q, p, h, lower, gt1, b if q else None, self.blob, self.sfac, eps, maxIter,
                               notImprovedLim, self._stall(stall_policy), r.zhat, r.nu if q else None, r.lam, r.slacks, r.lam_lo,
                               r.slacks_lo, r.iters, r.status, r.best_resid, r.trace, **kw)
        return r

    def backward_range(self, zhat, lam, slacks, lam_lo, slacks_lo, nu, dl_dz, want=(True,) * 7, shared=(False,) * 7):
        """Gradients (dQ, dp, dG, dh, dA, db, dlower) of a loss on zhat for the rows lower <= G z <= h, as backward(): `want`
        and `shared` have a seventh entry for lower.  One launch (qpx_backward_range): the backward's KKT solve with
        d = du + dl, du = clamp(lam)/clamp(slacks), dl = clamp(lam_lo)/clamp(slacks_lo), and lam - lam_lo in dG; from its
        dz = v the two bounds' gradients dh = -v du/(du + dl), dlower = -v dl/(du + dl) (exactly 0 on a one-sided row) are
        elementwise operations here, as drho is."""
        self._require_role(*self._RANGE)
        B, n, m, q = self.B, self.n, self.m, self.q
        wh, wl, sh, sl = bool(want[3]), bool(want[6]), bool(shared[3]), bool(shared[6])
        # (dh is elementwise, below: the launch writes no dh and the tail has no shared-h contraction)
        want = self._wanted(want[:6])
        want[3] = False
        grads, (dx, dz, dy) = self._grad_buffers(want, shared, dz_too=wh or wl)
        dQ, dp, dG, _, dA, db = grads
        zh, lm, nv = self._vec(zhat, n, "zhat"), self._vec(lam, m, "lam"), self._vec(nu, q, "nu")
        ll, sll = self._vec(lam_lo, m, "lam_lo"), self._vec(slacks_lo, m, "slacks_lo")
        sk = self._vec(slacks, m, "slacks")
        gz = self._vec(dl_dz, n, "dl_dz")
        if gz is None:
            raise RuntimeError("qpth_amd: backward_range needs dl_dz")
        with self._knob():
            self.lib.backward_range(B, n, m, q, self.blob, self.sfac, zh, lm, sk, ll, sll, nv, gz, dQ, dp, dG, dA, db,
                                    self.status, dx, dz, dy)
            dQ, dp, dG, _, dA, db = self._shared_grads(grads, want, shared, (dx, dz, dy), zh, lm, nv, lam_lo=ll)
        dh = dlo = None
        if wh or wl:
            du = lm.clamp(min=1e-8) / sk.clamp(min=1e-8)
            dl = ll.clamp(min=1e-8) / sll.clamp(min=1e-8)
            share = dl / (du + dl)
            if wh:
                dh = dz * (share - 1.0)
                dh = dh.mean(0) if sh else dh
            if wl:
                dlo = -dz * share
                dlo = dlo.mean(0) if sl else dlo
        return dQ, dp, dG, dh, dA, db, dlo

    # -- elastic rows G z <= h + t, t >= 0, penalty gamma't + 1/2 t'diag(rho)t -----------
    def elastic_ok(self):
        """does qpx_ipm_elastic serve these factors (under the knob they were built with)?  float64 tensors, the thread-grid /
        tile kernels' sizes (nz+neq+nineq <= 208), HARD factors (rho enters the loop, not the pre-factorisation)"""
        return self._role_ok("qpx_elastic_supported")

    def gt1_elastic(self, gamma, rho):
        """sqrt(|| G^T 1 ||^2 + 4 k) per QP, k its elastic rows (gamma and rho finite, the kernel's test): the augmented QP's
        || G'^T 1 || of the stop rule.  torch operations, no host sync (gt1_of is the model)."""
        G = self.G
        if G.dim() == 3 and (G.size(0) == 1 or G.stride(0) == 0):
            G = G[0]
        g2 = G.sum(-2).square().sum(-1)
        k = (torch.isfinite(gamma) & torch.isfinite(rho)).to(self.dtype).sum(-1)
        return torch.sqrt(g2 + 4.0 * k).reshape(-1).expand(self.B).contiguous()

    def ipm_elastic(self, p, h, gamma, rho, b, eps=1e-12, maxIter=20, notImprovedLim=3, stall_policy=None, want_trace=False):
        """The IPM loop for  G z <= h + t, t >= 0  with the penalty  gamma't + 1/2 t'diag(rho)t  in nineq rows (qpx_ipm_elastic):
        the iterates of ipm() on the augmented QP in (z, t), one launch, no host sync.  gamma, rho (B, nineq), (1, nineq) or
        (nineq,); +inf in either = a hard row.  The result has lam, slacks (= h + t - G zhat) of the rows and lam_t, slacks_t, t
        of t >= 0 (0, +inf and 0 on a hard row).  A gamma entry that is NaN or negative, a rho entry that is NaN or not
        positive: QPX_ST_NONFINITE in `status` (raise_on_failure)."""
        self._require_role(*self._ELASTIC)
        B, n, m, q = self.B, self.n, self.m, self.q
        self._check_ph(p, h)
        self._check(gamma, m, "l1")
        self._check(rho, m, "rho")
        self._check_b(b)
        r = self._new_result(maxIter, want_trace, ("lam_t", "slacks_t", "t"))
        gamma, rho = gamma.detach(), rho.detach()
        self._stage_entry_checks(r, ("l1 must be non-negative", "rho must be positive"), ~(gamma >= 0), ~(rho > 0))
        gt1 = self.gt1_elastic(gamma, rho)
        with self._knob():
            self.lib.ipm_elastic(B, n, m, q, p, h, gamma, rho, gt1, b if q else None, self.blob, self.sfac, eps, maxIter,
                                 notImprovedLim, self._stall(stall_policy), r.zhat, r.nu if q else None, r.lam, r.slacks, r.lam_t,
                                 r.slacks_t, r.t, r.iters, r.status, r.best_resid, r.trace)
        return r

    @staticmethod
    def elastic_eff(lam, slacks, lam_t, slacks_t, rho):
        """(slack_eff, dt) of an elastic solution: the derivative entry points serve it on the hard factors given lam and
        slack_eff = clamp(lam) (1/du + 1/(rho + dt)), du = clamp(lam)/clamp(slacks), dt = clamp(lam_t)/clamp(slacks_t) (clamps at
        1e-8, qp.py:148) -- their d = clamp(lam)/clamp(slack_eff) is then the augmented QP's 1/(1/du + 1/(rho + dt)).  On a hard
        row (rho = +inf) slack_eff is clamp(slacks).  It is >= clamp(slacks), so the kernels' own clamp leaves it alone."""
        lc, sc = lam.clamp(min=1e-8), slacks.clamp(min=1e-8)
        dt = lam_t.clamp(min=1e-8) / slacks_t.clamp(min=1e-8)
        return sc + lc / (rho + dt), dt

    # -- soft two-sided rows lower - tl <= G z <= h + tu --------------------------------
    def soft_range_ok(self):
        """does qpx_ipm_soft_range serve these factors (under the knob they were built with)?  float64 tensors, the thread-grid /
        tile kernels' sizes (nz+neq+nineq <= 208), HARD factors"""
        return self._role_ok("qpx_soft_range_supported")

    def gt1_soft_range(self, h, lower, gamma_u, rho_u, gamma_l, rho_l):
        """sqrt(|| G^T e ||^2 + 4 (k_u + k_l)) per QP: e = 1 on the one-sided rows, k the soft sides (gamma and rho finite; a
        lower side on a two-sided row only) -- the augmented QP's || G'^T 1 || of the stop rule.  torch operations, no host sync."""
        g = self.gt1_of(lower, h)
        two = ~torch.isinf(h - lower)
        k = (torch.isfinite(gamma_u) & torch.isfinite(rho_u)).to(self.dtype) \
            + (two & torch.isfinite(gamma_l) & torch.isfinite(rho_l)).to(self.dtype)
        k = k.sum(-1).reshape(-1).expand(self.B)
        return torch.sqrt(g.square() + 4.0 * k).contiguous()

    def ipm_soft_range(self, p, h, lower, l1, rho, l1_lower, rho_lower, b, eps=1e-12, maxIter=20, notImprovedLim=3,
                       stall_policy=None, want_trace=False):
        """The IPM loop for  lower - tl <= G z <= h + tu, tu, tl >= 0  with the penalty  l1 t + 1/2 rho t^2  of each side in nineq
        rows (qpx_ipm_soft_range): the iterates of ipm() on the augmented QP in (z, tu, tl), one launch, no host sync.  The five
        vectors are (B, nineq), (1, nineq) or (nineq,).  The result has lam, slacks (upper rows), lam_lo, slacks_lo (lower rows),
        lam_t, slacks_t, t (tu >= 0) and lam_tl, slacks_tl, t_lo (tl >= 0); an absent side reads 0, +inf and 0.  A bad entry
        (NaN, lower not below h, l1 < 0, rho <= 0): QPX_ST_NONFINITE in `status` (raise_on_failure)."""
        self._require_role(*self._SOFT_RANGE)
        B, n, m, q = self.B, self.n, self.m, self.q
        lower, l1, rho, l1_lower, rho_lower = [x.detach() for x in (lower, l1, rho, l1_lower, rho_lower)]
        self._check_ph(p, h)
        for x, name in zip((lower, l1, rho, l1_lower, rho_lower), SoftRange.__slots__):
            self._check(x, m, name)
        self._check_b(b)
        r = self._new_result(maxIter, want_trace, ("lam_lo", "slacks_lo", "lam_t", "slacks_t", "lam_tl", "slacks_tl", "t", "t_lo"))
        hd = h.detach()
        self._stage_entry_checks(r, ("lower must be below h", "l1 must be non-negative", "rho must be positive",
                                     "l1_lower must be non-negative", "rho_lower must be positive"),
                                 ~(lower < hd), ~(l1 >= 0), ~(rho > 0), ~(l1_lower >= 0), ~(rho_lower > 0))
        gt1 = self.gt1_soft_range(hd, lower, l1, rho, l1_lower, rho_lower)
        with self._knob():
            self.lib.ipm_soft_range(B, n, m, q, p, h, lower, l1, rho, l1_lower, rho_lower, gt1, b if q else None, self.blob,
                                    self.sfac, eps, maxIter, notImprovedLim, self._stall(stall_policy), r.zhat,
                                    r.nu if q else None, r.lam, r.slacks, r.lam_lo, r.slacks_lo, r.lam_t, r.slacks_t, r.lam_tl,
                                    r.slacks_tl, r.t, r.t_lo, r.iters, r.status, r.best_resid, r.trace)
        return r

    def backward_soft_range(self, res, rho, rho_lower, dl_dz, want=(True,) * 11, shared=(False,) * 6):
        """Gradients (dQ, dp, dG, dh, dA, db, dlower, dl1, drho, dl1_lower, drho_lower) of a loss on zhat at the solution `res`
        of ipm_soft_range; rho, rho_lower (B, nineq) with +inf on every hard side (either of the side's penalties +inf).  No
        kernel of its own: qpx_backward_range on the same factors with the effective slack of each side (elastic_eff), so
        that its d is 1/e_u + 1/e_l, e = 1/d_side + 1/(rho + dt), and the true lam - lam_lo meets dx in dG.  From its dz = v
        the sides' shares give dh = -v_u, dlower = v_l (v_u = v (1/e_u)/d, v_l = -v (1/e_l)/d) and, per side,
        dl1 = v_side/(dt + rho), drho = t dl1: exactly 0 on a hard or absent side.  `shared` reduces the six parameters as
        backward() does; the five others come back per QP, (B, nineq), for the caller to reduce."""
        want = [bool(w) for w in want]
        pen = any(want[6:])
        seff_u, dtu = self.elastic_eff(res.lam, res.slacks, res.lam_t, res.slacks_t, rho)
        seff_l, dtl = self.elastic_eff(res.lam_lo, res.slacks_lo, res.lam_tl, res.slacks_tl, rho_lower)
        w7 = tuple(want[:3]) + (want[3] or pen,) + tuple(want[4:6]) + (pen,)
        sh = tuple(shared[:3]) + (shared[3] and not pen,) + tuple(shared[4:6]) + (False,)
        dQ, dp, dG, dh, dA, db, dlo = self.backward_range(res.zhat, res.lam, seff_u, res.lam_lo, seff_l, res.nu, dl_dz,
                                                          want=w7, shared=sh)
        out = [None] * 5
        if pen:
            if want[6]:
                out[0] = dlo
            if want[7] or want[8]:
                g = -dh / (dtu + rho)
                out[1] = g if want[7] else None
                out[2] = g * res.t if want[8] else None
            if want[9] or want[10]:
                g = dlo / (dtl + rho_lower)
                out[3] = g if want[9] else None
                out[4] = g * res.t_lo if want[10] else None
            if not want[3]:
                dh = None
            elif shared[3]:
                dh = dh.mean(0)
        return (dQ, dp, dG, dh, dA, db) + tuple(out)

    # -- factor_kkt + solve_kkt (batch.py:435-470, 349-372) ----------------------------------
    def solve_kkt(self, d, rx, rs, rz, ry, refine=0):
        """factor_kkt + solve_kkt; refine > 0: that many steps of iterative refinement on the residual of the original
        KKT system (batch.py:228-270, KKTSolvers.IR_UNOPT) inside the kernel, re-using the factorisation."""
        self._no_groups(True, "solve_kkt")
        self._no_refine_on_soft(refine, "solve_kkt")
        B, n, m, q = self.B, self.n, self.m, self.q
        dt, dev = self.dtype, self.device
        d = self._vec(d, m, "d")
        dx = torch.empty(B, n, dtype=dt, device=dev)
        ds = torch.empty(B, m, dtype=dt, device=dev)
        dz = torch.empty(B, m, dtype=dt, device=dev)
        dy = torch.empty(B, q, dtype=dt, device=dev) if q else None
        with self._knob():
            self.lib.factor_solve_kkt(B, n, m, q, self.blob, self.sfac, d, self._vec(rx, n, "rx"), self._vec(rs, m, "rs"),
                                      self._vec(rz, m, "rz"), self._vec(ry, q, "ry"), dx, ds, dz, dy, self.status,
                                      refine=refine, Q=self.Q, G=self.G, A=self.A, wide=self.wide)
        return dx, ds, dz, dy

    def _vecs(self, X, K, k, what):
        """dense (B,K,k) contiguous tensor or None: the K-stacked right-hand sides of solve_kkt_many"""
        if X is None or X.nelement() == 0 or k == 0:
            return None
        if X.dtype != self.dtype or X.device != self.device:
            raise RuntimeError("qpth_amd: %s is %s on %s, the factors were built for %s on %s"
                               % (what, X.dtype, X.device, self.dtype, self.device))
        if tuple(X.shape) != (self.B, K, k):
            raise RuntimeError("qpth_amd: %s has shape %s, expected (%d, %d, %d)" % (what, tuple(X.shape), self.B, K, k))
        return X.contiguous()

    def solve_kkt_many(self, d, rx, rs, rz, ry, refine=0):
        """factor_kkt ONCE + solve_kkt for K right-hand sides per QP: rx (B,K,n), rs, rz (B,K,m), ry (B,K,q), each None = zeros
        (not all of them); d (B,m) as for solve_kkt.  Returns (dx, ds, dz, dy) of shapes (B,K,.), dy None without equalities.
        One launch and one factorisation of T = R + diag(1/d) per QP (qpx_factor_solve_kkt_multi) where the thread-grid /
        tile kernels serve the size and refine == 0.  Otherwise -- the large-QP family (nz+neq+nineq > 208), refine > 0 --
        the same result costs K launches of solve_kkt on slices, each with a factorisation of its own.  No host sync."""
        self._no_groups(True, "solve_kkt_many")
        self._no_refine_on_soft(refine, "solve_kkt_many")
        B, n, m, q = self.B, self.n, self.m, self.q
        dt, dev = self.dtype, self.device
        given = [X for X in (rx, rs, rz, ry if q else None) if X is not None and X.nelement() > 0]
        if not given:
            raise RuntimeError("qpth_amd: solve_kkt_many needs at least one of rx, rs, rz, ry")
        if given[0].dim() != 3:
            raise RuntimeError("qpth_amd: right-hand sides of solve_kkt_many are (B, K, .), got %s" % (tuple(given[0].shape),))
        K = given[0].size(1)
        if K < 1:
            raise RuntimeError("qpth_amd: solve_kkt_many needs K >= 1 right-hand sides")
        d = self._vec(d, m, "d")
        rx, rs, rz, ry = self._vecs(rx, K, n, "rx"), self._vecs(rs, K, m, "rs"), self._vecs(rz, K, m, "rz"), self._vecs(ry, K, q, "ry")
        dx = torch.empty(B, K, n, dtype=dt, device=dev)
        ds = torch.empty(B, K, m, dtype=dt, device=dev)
        dz = torch.empty(B, K, m, dtype=dt, device=dev)
        dy = torch.empty(B, K, q, dtype=dt, device=dev) if q else None
        with self._knob():
            one_launch = refine == 0 and bool(self.lib.dll.qpx_multi_supported(self.code, n, m, q))
            if one_launch:
                self.lib.factor_solve_kkt_multi(B, n, m, q, K, self.blob, self.sfac, d, rx, rs, rz, ry, dx, ds, dz, dy,
                                                self.status, wide=self.wide)
        if not one_launch:
            for k in range(K):
                cut = [None if X is None else X[:, k] for X in (rx, rs, rz, ry)]
                out = self.solve_kkt(d, *cut, refine=refine)
                for dst, src in zip((dx, ds, dz, dy), out):
                    if dst is not None:
                        dst[:, k] = src
        return dx, ds, dz, dy

    # -- KKTSolvers.IR_UNOPT (batch.py:244-270) as a finishing stage --------------------------------
    def polish(self, p, h, b, res, steps=2, refine=0):
        """The finishing stage: `steps` iterations of the reference's PDIPM loop (batch.py:92-198: affine + centring-corrector)
        in the ORIGINAL variables (x, s, z, y), on residuals of the caller's data accumulated in float64, from the loop
        kernel's result; the best iterate is kept -- by the reference's residual ||rx|| + ||rz|| + ||ry|| + nineq mu,
        strict <, NaN never wins (batch.py:118-139) -- so a step that does not help cannot make the answer worse.  The
        loop kernel iterates on pre-computed products (R = G Q^-1 G^T, ...): in float32 their rounding error (cond(Q) ~
        1e6 on the benchmark generator) is a perturbation of the PROBLEM that no number of loop iterations removes;
        residuals against the original data do.  One C call (qpx_polish, include/qpx.h): one kernel where the thread-grid
        / tile kernels serve the size, a stream-ordered sequence of the large-QP family's launches beyond (v7).  No host
        sync.  (Rounds 2-4 composed this stage from torch operations on the host side for the sizes without a kernel;
        that version now lives in tests/polish_reference.py as the step-by-step reference of the kernels.)"""
        self._no_groups(True, "polish")
        if self.soft:
            raise ValueError("qpth_amd: no finishing stage (qpx_polish: KKTSolvers.IR_UNOPT, float32 refine=k) on factors with "
                             "soft rows (w / rho): its steps evaluate the residuals of the hard QP")
        if self.polish_ok:
            B, n, m, q = self.B, self.n, self.m, self.q
            self._check_ph(p, h)
            self._check_b(b, b_required=False)
            if not self.refine_ok:
                # the large-QP family has no refinement inside its KKT solves (qpx_refine_supported): the finishing steps
                # themselves run, their solves un-refined -- QPFunction(refine=k) never asks for more
                refine = 0
            for name in ("zhat", "lam", "slacks") + (("nu",) if q else ()):
                setattr(res, name, getattr(res, name).contiguous())
            with self._knob():
                self.lib.polish(B, n, m, q, self.Q, p, self.G, h, self.A if q else None, b if q else None, self.blob, self.sfac,
                                steps, refine, res.zhat, res.nu if q else None, res.lam, res.slacks, None, self.status)
            return res
        if self.wide:
            # float32 tensors in float64 arithmetic: the loop's answer already is the float64 solution of the data (DESIGN
            # 3.4), there is nothing for residuals in float64 to add; rounds 2-4 ran a host-composed stage here
            return res
        raise RuntimeError("qpth_amd: no finishing stage (qpx_polish: KKTSolvers.IR_UNOPT, float32 refine=k) for this size / dtype "
                           "under the current knob -- nz = %d, nineq = %d, neq = %d; it is served up to 512 per dimension "
                           "(qpx_polish_supported).  float32 tensors run in float64 arithmetic by default (refine=None)"
                           % (self.n, self.m, self.q))

    # -- the central-path point at a given kappa ------------------------------------------
    def centre_ok(self):
        """does qpx_centre serve these factors (under the knob they were built with)?  float64 tensors, the thread-grid /
        tile kernels' sizes (nz+neq+nineq <= 208), no soft rows"""
        return self._role_ok("qpx_centre_supported")

    def centre(self, p, h, b, res, kappa, tol=1e-9, max_steps=20):
        """Newton's method from the loop's result `res` onto the point of the central path
            Q z + p + G'lam + A'nu = 0,  G z + s = h,  A z = b,  s_i lam_i = kappa_i   (s, lam > 0)
        -- one launch (qpx_centre), no host sync: per step the residuals of the caller's data, one factorisation and one
        solve; a QP stops at max(|rx|, |rz|, |ry|, |s lam - kappa| / kappa) <= tol (max norms) or after max_steps steps.
        kappa: (B, nineq), (1, nineq) or (nineq,), every entry finite and > 0 (else QPX_ST_NONFINITE in `status`).  Returns
        `res`, its zhat, nu, lam, slacks overwritten, with `centre_resid` (B,) and `centre_steps` int32 (B,) added; a QP that
        ends above tol has _lib.ST_NOT_CENTRED in `res.status`.  backward, jvp, backward2 and solve_kkt_many serve the centred
        point as they stand; d loss / d kappa = dz / lam, dz of backward(want_dz=True)."""
        self._no_groups(True, "centre")
        if self.soft:
            raise ValueError("qpth_amd: no centring (qpx_centre) on factors with soft rows (w / rho): its steps evaluate the "
                             "residuals of the hard QP")
        if not self.centre_ok():
            raise ValueError("qpth_amd: centring (qpx_centre, kappa) is served for float64 tensors up to nz + neq + nineq = 208 "
                             "under the default knob; got %s, nz = %d, nineq = %d, neq = %d"
                             % (str(self.dtype).replace("torch.", "") + (" in float64 arithmetic" if self.wide else ""),
                                self.n, self.m, self.q))
        B, n, m, q = self.B, self.n, self.m, self.q
        self._check_ph(p, h)
        self._check_b(b, b_required=False)
        self._check(kappa, m, "kappa")
        for name in ("zhat", "lam", "slacks") + (("nu",) if q else ()):
            setattr(res, name, getattr(res, name).contiguous())
        res.centre_resid = torch.empty(B, dtype=self.dtype, device=self.device)
        res.centre_steps = torch.empty(B, dtype=torch.int32, device=self.device)
        with self._knob():
            self.lib.centre(B, n, m, q, self.Q, p, self.G, h, self.A if q else None, b if q else None, self.blob, self.sfac,
                            kappa, tol, max_steps, res.zhat, res.nu if q else None, res.lam, res.slacks,
                            res.centre_resid, res.centre_steps, self.status)
        return res

    # -- QPFunctionFn.jvp: forward mode ---------------------------------------------------------
    def jvp(self, zhat, lam, slacks, nu, tangents, refine=0, want_duals=False):
        """The tangent of the solution along `tangents` = (tQ, tp, tG, th, tA, tb) -- each None / empty (zero) or of its
        parameter's shape, batched, batch-1 or shared -- at the forward's (zhat, lam, slacks, nu): ONE KKT solve with the
        matrix the backward factors (d = clamp(lam) / clamp(slacks), qp.py:148), its right-hand side formed from the tangents
        inside the kernel (qpx_jvp, include/qpx.h).  Returns z' (B, n); want_duals: (z', lam', nu').  No host sync."""
        self._no_groups(True, "jvp")
        self._no_refine_on_soft(refine, "jvp")
        B, n, m, q = self.B, self.n, self.m, self.q
        dt, dev = self.dtype, self.device
        ts = []
        for X, shape, what in zip(tangents, ((n, n), (n,), (m, n), (m,), (q, n), (q,)), ("Q", "p", "G", "h", "A", "b")):
            if X is None or X.nelement() == 0 or (q == 0 and what in ("A", "b")):
                ts.append(None)
                continue
            if X.dtype != dt or X.device != dev:
                raise RuntimeError("qpth_amd: the tangent of %s is %s on %s, the factors were built for %s on %s"
                                   % (what, X.dtype, X.device, dt, dev))
            if tuple(X.shape) not in (shape, (1,) + shape, (B,) + shape):
                raise RuntimeError("qpth_amd: the tangent of %s has shape %s, expected %s, %s or %s"
                                   % (what, tuple(X.shape), shape, (1,) + shape, (B,) + shape))
            ts.append(X)
        dz = torch.empty(B, n, dtype=dt, device=dev)
        dl = torch.empty(B, m, dtype=dt, device=dev) if want_duals else None
        dn = torch.empty(B, q, dtype=dt, device=dev) if (want_duals and q) else None
        with self._knob():
            self.lib.jvp(B, n, m, q, self.blob, self.sfac, self._vec(zhat, n, "zhat"), self._vec(lam, m, "lam"),
                         self._vec(slacks, m, "slacks"), self._vec(nu, q, "nu"), *ts, dz, self.status, dlam=dl, dnu=dn,
                         refine=refine, Q=self.Q, G=self.G, A=self.A, wide=self.wide)
        return (dz, dl, dn) if want_duals else dz

    # -- QPFunctionFn.backward (qp.py:127-182) ------------------------------------------------
    def backward(self, zhat, lam, slacks, nu, dl_dz, want=(True,) * 6, shared=(False,) * 6, refine=0,
                 dl_dlam=None, dl_dnu=None, want_dz=False, want_sol=False):
        """Gradients (dQ, dp, dG, dh, dA, db) for the parameters `want` asks for (ctx.needs_input_grad;
        the others come back as None and cost nothing).  A parameter flagged in `shared` is one the whole
        batch shares: its gradient is returned already reduced to the reference's `.mean(0)` (qp.py:159-177)
        -- for the matrices by one contraction over the batch (qpx_batch_outer) instead of B outer products.
        dl_dlam (B, m), dl_dnu (B, q): cotangents of the multipliers lam*, nu* (None = zero; dl_dz may then be None too,
        but not all three): the same launch with the right-hand side (dl_dz, 0, dl_dlam, dl_dnu) -- qpx_backward_duals,
        the exact adjoint of jvp(..., want_duals=True).
        want_dz: a seventh value behind the six, dz (B, m) of the KKT solution as the launch wrote it -- the gradient with
        respect to the w of soft factors is -dz lam.
        want_sol: a last value behind those, (dx, dz, dy) -- the solution of the backward KKT system as the launch wrote it (dy
        None without equality constraints): what backward2 differentiates through."""
        self._no_refine_on_soft(refine, "backward")
        self._no_groups(refine > 0, "backward with refine=%d" % refine)
        B, n, m, q = self.B, self.n, self.m, self.q
        want = self._wanted(want)
        grads, (dx, dz, dy) = self._grad_buffers(want, shared, dz_too=want_dz, sol_too=want_sol)
        dQ, dp, dG, dh, dA, db = grads
        zh, lm, nv = self._vec(zhat, n, "zhat"), self._vec(lam, m, "lam"), self._vec(nu, q, "nu")
        gz, gl, gn = self._vec(dl_dz, n, "dl_dz"), self._vec(dl_dlam, m, "dl_dlam"), self._vec(dl_dnu, q, "dl_dnu")
        if gz is None and gl is None and gn is None:
            raise RuntimeError("qpth_amd: backward needs at least one of dl_dz, dl_dlam, dl_dnu")
        duals = {} if (gl is None and gn is None and gz is not None) else {"dl_dlam": gl, "dl_dnu": gn}
        if self.K is not None:
            # scenario groups: the same backward kernel, QP j reading blob j // K; a per-group matrix's gradient is the sum
            # over the group's QPs -- one grouped contraction each -- and a shared parameter's the mean over all B QPs as ever
            with self._knob():
                self.lib.backward_group(self.groups, self.K, n, m, q, self.blob, self.sfac, zh, lm,
                                        self._vec(slacks, m, "slacks"), nv, gz, dp, dh, db, self.status, dx, dz, dy,
                                        wide=self.wide, dl_dlam=gl, dl_dnu=gn)
                grads = self._group_grads(grads, want, shared, (dx, dz, dy), zh, lm, nv)
                grads = self._shared_grads(grads, want, shared, (dx, dz, dy), zh, lm, nv)
            out = tuple(grads) + ((dz,) if want_dz else ())
            return out + ((dx, dz, dy),) if want_sol else out
        with self._knob():
            self.lib.backward(B, n, m, q, self.blob, self.sfac, zh, lm, self._vec(slacks, m, "slacks"), nv,
                              gz, dQ, dp, dG, dh, dA, db, self.status, dx, dz, dy,
                              refine=refine, Q=self.Q, G=self.G, A=self.A, wide=self.wide, **duals)
            grads = self._shared_grads(grads, want, shared, (dx, dz, dy), zh, lm, nv)
        out = tuple(grads) + ((dz,) if want_dz else ())
        return out + ((dx, dz, dy),) if want_sol else out

    def _wanted(self, want):
        """the six `want` flags (Q, p, G, h, A, b) of a backward as a list of bools: none for A and b without equality constraints"""
        want = [bool(w) for w in want]
        if self.q == 0:
            want[4] = want[5] = False
        return want

    def _grad_buffers(self, want, shared, dz_too=False, sol_too=False):
        """What a backward launch writes, for six `want` (_wanted) and `shared` flags: ([dQ, dp, dG, dh, dA, db], (dx, dz, dy)),
        None where not asked for.  Per-QP gradients come out of the kernel as they are (dp = dx, dh = -dz, db = -dy:
        qp.py:157-166; the kernel writes the signs, no elementwise launches behind it); the KKT solution itself (dx, dz, dy) is
        only asked for when a batch-shared parameter needs it -- one contraction / mean over the batch, _shared_grads -- or the
        caller does (dz_too; sol_too: all three)."""
        B, n, m, q = self.B, self.n, self.m, self.q
        wQ, wp, wG, wh, wA, wb = want
        sQ, sp, sG, sh, sA, sb = shared[:6]

        def buf(flag, *shape):
            return torch.empty(*shape, dtype=self.dtype, device=self.device) if flag else None

        if self.K is not None:
            # scenario groups: the kernel writes no matrix gradient -- a batched matrix's is contracted per group from the KKT
            # solution (_group_grads), as a shared one's is over the batch
            sQ, sG, sA = sQ or wQ, sG or wG, sA or wA
        dQ = buf(wQ and not sQ, B, n, n)
        dG = buf(wG and not sG, B, m, n)
        dA = buf(wA and not sA, B, q, n)
        dp = buf(wp and not sp, B, n)
        dh = buf(wh and not sh, B, m)
        db = buf(wb and not sb, B, q)
        dx = buf((wp and sp) or (wQ and sQ) or (wG and sG) or (wA and sA) or sol_too, B, n)
        dz = buf((wh and sh) or (wG and sG) or dz_too or sol_too, B, m)
        dy = buf(q > 0 and ((wb and sb) or (wA and sA) or sol_too), B, q)
        return [dQ, dp, dG, dh, dA, db], (dx, dz, dy)

    def _group_grads(self, grads, want, shared, sol, zh, lm, nv):
        """Scenario groups: the gradients of the matrices each GROUP has of its own (wanted, not shared by the batch), (groups,
        ., .) -- the sum over the group's K QPs of the per-QP outer products (qp.py:167-173), one grouped contraction each
        (qpx_group_outer), in the order Q, G, A.  Called as _shared_grads is."""
        n, m, q, G, K = self.n, self.m, self.q, self.groups, self.K
        dt, dev = self.dtype, self.device
        dx, dz, dy = sol
        if want[0] and not shared[0]:
            grads[0] = torch.empty(G, n, n, dtype=dt, device=dev)
            self.lib.group_outer(K, dx, zh, zh, dx, 0.5, grads[0])
        if want[2] and not shared[2]:
            grads[2] = torch.empty(G, m, n, dtype=dt, device=dev)
            self.lib.group_outer(K, dz, zh, lm, dx, 1.0, grads[2])
        if want[4] and not shared[4]:
            grads[4] = torch.empty(G, q, n, dtype=dt, device=dev)
            self.lib.group_outer(K, dy, zh, nv, dx, 1.0, grads[4])
        return grads

    def _shared_grads(self, grads, want, shared, sol, zh, lm, nv, lam_lo=None):
        """The gradients of the parameters the batch shares, from the KKT solution `sol` a backward launch wrote: the
        reference's `.mean(0)` (qp.py:159-177) as one contraction over the batch each (qpx_batch_outer), in the order Q, G, A,
        p, h, b.  lam_lo: the range role's dG meets lam - lam_lo.  Returns `grads` with those entries filled in.  Called inside
        the caller's _knob() block, behind its launch (these launches too need the factors' device current)."""
        n, m, q = self.n, self.m, self.q
        dt, dev = self.dtype, self.device
        dx, dz, dy = sol
        sQ, sp, sG, sh, sA, sb = shared[:6]
        wQ, wp, wG, wh, wA, wb = want
        if wQ and sQ:
            grads[0] = torch.empty(n, n, dtype=dt, device=dev)
            self.lib.batch_outer(dx, zh, zh, dx, 0.5, grads[0])
        if wG and sG:
            grads[2] = torch.empty(m, n, dtype=dt, device=dev)
            self.lib.batch_outer(dz, zh, lm if lam_lo is None else lm - lam_lo, dx, 1.0, grads[2])
        if wA and sA:
            grads[4] = torch.empty(q, n, dtype=dt, device=dev)
            self.lib.batch_outer(dy, zh, nv, dx, 1.0, grads[4])
        # shared vectors: the same contraction with a column of ones (ABI v8) -- `.mean(0)` in a fixed order of
        # additions, the sign of qp.py:160-166 folded into the scale
        if wp and sp:
            grads[1] = torch.empty(n, dtype=dt, device=dev)
            self.lib.batch_outer(dx, None, None, None, 1.0, grads[1])
        if wh and sh:
            grads[3] = torch.empty(m, dtype=dt, device=dev)
            self.lib.batch_outer(dz, None, None, None, -1.0, grads[3])
        if wb and sb:
            grads[5] = torch.empty(q, dtype=dt, device=dev)
            self.lib.batch_outer(dy, None, None, None, -1.0, grads[5])
        return grads

    # -- the backward of the backward ------------------------------------------------
    def backward2_fused(self):
        """does qpx_backward2 serve these factors (under the knob they were built with)?"""
        if self.soft or self.K is not None or not hasattr(self.lib.dll, "qpx_backward2_supported"):
            return False
        with self._knob():
            return bool(self.lib.dll.qpx_backward2_supported(self.code, self.n, self.m, self.q))

    def backward2(self, zhat, lam, slacks, nu, sol, W, want=(True,) * 6, fused=None):
        """The second-order pass: for cotangents W = (W_Q, W_p, W_G, W_h, W_A, W_b) on the six PER-QP gradients a call of
        backward() returned -- each None (zero) or of its gradient's shape, batched (B, ...) or one for the whole batch -- and
        that call's KKT solution sol = (dx, dz, dy) (backward(want_sol=True)), the gradient of psi = sum_i <W_i, grad_i>
          - with respect to that call's cotangents (dl_dz, dl_dlam, dl_dnu): (zdot, lamdot, nudot), nudot None without
            equality constraints;
          - with respect to the six parameters, per QP: (HQ, Hp, HG, Hh, HA, Hb), None where `want` does not ask.
        Returns ((zdot, lamdot, nudot), (HQ, .., Hb)).  Two more solves with the matrix the backward factors (DESIGN 4.9 has
        the closed form).  fused=None: one launch with one factorisation (qpx_backward2) where the library serves these
        factors, else the COMPOSED path -- jvp(want_duals=True), elementwise and outer products in torch, backward(dl_dlam=,
        dl_dnu=): the large-QP family (nz+neq+nineq > 208), float32 kernels, forms the fused entry declines.  True / False
        force one or the other (True raises where the library declines).  Second derivatives of a QP's solution exist only
        under strict complementarity; soft factors and refinement are not served.  No host sync."""
        self._no_groups(True, "backward2")
        if self.soft:
            raise RuntimeError("qpth_amd: second derivatives are not served on factors with soft rows (w / rho)")
        B, n, m, q = self.B, self.n, self.m, self.q
        dt, dev = self.dtype, self.device
        dx, dz, dy = sol
        shapes = ((n, n), (n,), (m, n), (m,), (q, n), (q,))
        Ws = []
        for X, shape, what in zip(W, shapes, ("Q", "p", "G", "h", "A", "b")):
            if X is None or X.nelement() == 0 or (q == 0 and what in ("A", "b")):
                Ws.append(None)
                continue
            if X.dtype != dt or X.device != dev:
                raise RuntimeError("qpth_amd: the cotangent on the gradient of %s is %s on %s, the factors were built for %s on %s"
                                   % (what, X.dtype, X.device, dt, dev))
            if tuple(X.shape) not in (shape, (1,) + shape, (B,) + shape):
                raise RuntimeError("qpth_amd: the cotangent on the gradient of %s has shape %s, expected %s, %s or %s"
                                   % (what, tuple(X.shape), shape, (1,) + shape, (B,) + shape))
            Ws.append(X)
        want = [bool(w) for w in want]
        if q == 0:
            want[4] = want[5] = False
        zh, lm, sl, nv = self._vec(zhat, n, "zhat"), self._vec(lam, m, "lam"), self._vec(slacks, m, "slacks"), self._vec(nu, q, "nu")
        dx, dz, dy = self._vec(dx, n, "dx"), self._vec(dz, m, "dz"), self._vec(dy, q, "dy")
        if fused is None:
            fused = self.backward2_fused()
        elif fused and not self.backward2_fused():
            raise RuntimeError("qpth_amd: qpx_backward2 does not serve nz = %d, nineq = %d, neq = %d in this dtype under the "
                               "current knob (qpx_backward2_supported)" % (n, m, q))
        if fused:
            def buf(flag, *shape):
                return torch.empty(*shape, dtype=dt, device=dev) if flag else None
            zd, ld, nd = buf(True, B, n), buf(True, B, m), buf(q > 0, B, q)
            H = [buf(w, B, *shape) for w, shape in zip(want, shapes)]
            with self._knob():
                self.lib.backward2(B, n, m, q, self.blob, self.sfac, zh, lm, sl, nv, dx, dz, dy, *Ws, zd, ld, nd, *H,
                                   self.status, wide=self.wide)
            return (zd, ld, nd), tuple(H)
        # composed: step 1, forward mode along W
        zd, ld, nd = self.jvp(zh, lm, sl, nv, Ws, want_duals=True)
        # step 2, the cotangents on the solution (a None W is zero)
        WQ, Wp, WG, Wh, WA, Wb = [X if (X is None or X.dim() == len(sh) + 1) else X.unsqueeze(0) for X, sh in zip(Ws, shapes)]
        # (the closed form's g_z has G^T u, u = a lamdot, as well: by M (0, u, 0) = (G^T u, -u/d, 0) that term is the shift
        # ez = ez' - u of the solution for u/d added to g_lam, and HG, Hh need ez + u = ez' only -- as the kernel, no product with G)
        lc = lm.clamp(min=1e-8)
        u = dz / lc * ld
        gz = torch.zeros(B, n, dtype=dt, device=dev)
        gl = 2.0 * u * sl.clamp(min=1e-8) / lc               # a (G zdot + t_z) = u / d by row 2 of step 1, and u / d once more
        gn = torch.zeros(B, q, dtype=dt, device=dev) if q else None
        mv = lambda M_, x: torch.matmul(M_, x.unsqueeze(2)).squeeze(2)      # noqa: E731
        if WQ is not None:
            gz = gz + 0.5 * mv(WQ + WQ.transpose(1, 2), dx)
        if WG is not None:
            gz = gz + mv(WG.transpose(1, 2), dz)
            gl = gl + mv(WG, dx)
        if WA is not None:
            gz = gz + mv(WA.transpose(1, 2), dy)
            gn = gn + mv(WA, dx)
        # step 3, one more backward with cotangents on the multipliers, plus the direct terms
        H = list(self.backward(zh, lm, sl, nv, gz, want=want, dl_dlam=gl, dl_dnu=gn))
        o = lambda x, y: x.unsqueeze(2) * y.unsqueeze(1)                  # noqa: E731
        if want[0]:
            H[0] = H[0] + 0.5 * (o(dx, zd) + o(zd, dx))
        if want[2]:
            H[2] = H[2] + o(ld, dx) + o(dz, zd)
        if want[4]:
            H[4] = H[4] + o(nd, dx) + o(dy, zd)
        return (zd, ld, nd), tuple(H)
