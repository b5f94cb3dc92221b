"""qpth_amd -- MI355X-native drop-in for the hot path of locuslab/qpth: the batched
differentiable dense QP solver `QPFunction(...)(Q, p, G, h, A, b)` (qpth/qp.py:18-183) on
hand-written gfx950 HIP kernels (one QP per workgroup, KKT blocks in LDS).

    from qpth_amd.qp import QPFunction, QPSolvers
    zhat = QPFunction(verbose=-1)(Q, p, G, h, A, b)      # tensors on a HIP device
    J = qpth_amd.sensitivity.solve(Q, p, G, h, A, b).jacobian()   # d zhat / d (p, h, b), one launch (sensitivity.py)
    ws = qpth_amd.WarmStart(); QPFunction(warm_start=ws)(...)      # a training loop: each solve starts at the last one's (lam, slacks)
"""
from . import qp, sensitivity, solvers, util  # noqa: F401
from .qp import QPFunction, QPSolvers  # noqa: F401
from .kkt import RangeWarmStart, SoftRange, WarmStart, set_stall_policy  # noqa: F401

__version__ = "0.1.0"
