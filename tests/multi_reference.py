"""Float64 references of the multi-right-hand-side KKT solve (KKTFactors.solve_kkt_many, qpth_amd/sensitivity.py), shared by
tests/test_emu_multi.py and tests/test_gpu_multi.py: a dense solve of the full KKT matrix as full_kkt_tangent of
tests/test_emu_jvp.py builds it, on whatever device the tensors live on.

solve_kkt (batch.py:349-372) solves  [[Q, 0, G^T, A^T], [0, D, I, 0], [G, I, 0, 0], [A, 0, 0, 0]] (dx, ds, dz, dy) = -(rx, rs, rz, ry),
D = diag(d).  Without ds (D ds + dz = -rs), the second block row times d:
    [[Q, G^T, A^T], [D G, -I, 0], [A, 0, 0]] (dx, dz, dy) = -(rx, d rz - rs, ry),      ds = -rz - G dx."""
import torch

# every form of the kernels the dispatcher can pick (include/qpx.h, qpx_set_ipm_variant): the list of tests/test_emu_jvp.py,
# held equal to it by tests/test_emu_multi.py
KNOB_FORMS = (3, 256, 512, 1024 + 2048, 1024 + 4096, 1024 + 8192)


def ds_tol(tol, rs):
    """bound on ds = (-rs - dz) / d against ds = -rz - G dx of the dense solution.  rs None: `tol`, as every output.  With
    an rs, -rs - dz cancels where d is small (dz -> -rs as d -> 0): an error of dz of a few 2^-52 |dz| ~ 1e-15 .. 1e-14 is
    divided by d, which the backward's clamps keep >= ~1e-8 on the generator's solutions -- 1e-6 (solve_kkt's ds
    has the same property)"""
    return tol if rs is None else max(tol, 1e-6)


def kkt_matrix(Q, G, A, d):
    """(B, N, N) float64, N = n + m + q; Q (B,n,n), G (B,m,n), A (B,q,n) or None, d (B,m)"""
    Q, G, d = Q.double(), G.double(), d.double()
    B, m, n = G.shape
    q = A.shape[-2] if (A is not None and A.nelement()) else 0
    K = torch.zeros(B, n + m + q, n + m + q, dtype=torch.float64, device=Q.device)
    K[:, :n, :n] = Q
    K[:, :n, n:n + m] = G.transpose(1, 2)
    K[:, n:n + m, :n] = d.unsqueeze(2) * G
    K[:, n:n + m, n:n + m] = -torch.eye(m, dtype=torch.float64, device=Q.device)
    if q:
        K[:, :n, n + m:] = A.double().transpose(1, 2)
        K[:, n + m:, :n] = A.double()
    return K


def dense_solve_many(Q, G, A, d, rx, rs, rz, ry):
    """(dx, ds, dz, dy), each (B, K, .) float64, for K-stacked right-hand sides (B, K, .) (None = zeros)"""
    B, m, n = G.shape
    q = A.shape[-2] if (A is not None and A.nelement()) else 0
    Kn = next(X.shape[1] for X in (rx, rs, rz, ry) if X is not None)
    dev = Q.device

    def z(k):
        return torch.zeros(B, Kn, k, dtype=torch.float64, device=dev)

    rx, rs, rz = [z(k) if X is None else X.double() for X, k in ((rx, n), (rs, m), (rz, m))]
    ry = z(q) if (ry is None or q == 0) else ry.double()
    dd = d.double().unsqueeze(1)
    rhs = -torch.cat([rx, dd * rz - rs, ry], dim=2)                        # (B, K, N)
    x = torch.linalg.solve(kkt_matrix(Q, G, A, d), rhs.transpose(1, 2)).transpose(1, 2)
    dx, dz, dy = x[..., :n], x[..., n:n + m], x[..., n + m:]
    # ds from the third block row, G dx + ds = -rz: (-rs - dz) / d would divide a cancelling difference by d down to 1e-8
    # and make the reference's own ds good to eight digits only
    return dx, -rz - dx @ G.double().transpose(1, 2), dz, dy


def rel_many(a, ref):
    """(B, K) relative L2 errors of the K-stacked vectors a against ref"""
    a, ref = a.double(), ref.double()
    return (a - ref).norm(dim=2) / ref.norm(dim=2).clamp_min(1e-300)
