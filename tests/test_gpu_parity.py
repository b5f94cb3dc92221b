"""-m gpu: parity of the HIP path (through the C ABI, on a real MI355X) with the reference.

Three kinds of evidence, as the brief asks:
  1. golden vectors produced by the reference itself (tests/golden, make_golden.py);
  2. the oracle (CPU restatement, pinned to those vectors) on seeded inputs at sizes it
     finishes in seconds -- BASELINE.json configs C1..C3 and a C5 slice;
  3. size-independent properties at BASELINE.json's full sizes: KKT optimality of the returned
     (zhat, lam, nu, slacks), gradient consistency with finite differences of the solver, batch
     permutation equivariance, idempotence of a warm re-solve.
Tolerances are written where they are used; f64: 1e-6 relative unless noted (north star: 1e-4).
"""
import numpy as np
import pytest
import torch

import problems
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from qpth_amd import _lib
    _lib.hip()                              # the HIP extension must be the thing that runs
    assert _lib._TEST_BACKEND is None
    return torch.device("cuda:0")


def to_dev(arrs, dev, dtype=torch.float64, grad=True):
    out = []
    for x in arrs:
        x = np.asarray(x)
        t = torch.tensor(x, dtype=dtype, device=dev) if x.size else torch.empty(0, dtype=dtype, device=dev)
        if grad and t.nelement() > 0:
            t.requires_grad_(True)
        out.append(t)
    return out


def run_qpf(arrs, dl, dev, dtype=torch.float64, **kw):
    from qpth_amd.qp import QPFunction
    tq = to_dev(arrs, dev, dtype)
    z = QPFunction(verbose=-1, **kw)(*tq)
    z.backward(torch.tensor(np.asarray(dl), dtype=dtype, device=dev))
    torch.cuda.synchronize()
    return z.detach().cpu().numpy(), [t.grad.cpu().numpy() if t.grad is not None else None for t in tq]


def golden_inputs(g, dtype=np.float64):
    if "Q" in g:
        return [g[k] for k in ("Q", "p", "G", "h", "A", "b")]
    B, n, m, q, seed = [int(v) for v in g["shape"]]
    return list(problems.prof_qp(B, n, m, q, seed, dtype))


# ---------------------------------------------------------------- 1. golden vectors
@pytest.mark.parametrize("name", ["dl_dp", "dl_dG", "dl_dh", "dl_dA", "dl_db"])
def test_reference_gradient_problems(dev, name):
    g = load_golden("grads_" + name)
    z, grads = run_qpf(golden_inputs(g), g["dl_dz"], dev)
    assert rel_err(z, g["zhat"]).max() < TOL
    for k, gr in zip(("dQ", "dp", "dG", "dh", "dA", "db"), grads):
        if k in g:
            assert gr.shape == g[k].shape
            assert np.abs(gr - g[k]).max() <= TOL * max(1.0, np.abs(g[k]).max()), k


@pytest.mark.parametrize("name", ["c1_b8_n10_m5_f64", "c3s_b4_n20_m10_q4_f64", "c2s_b4_n100_m100_f64",
                                  "c3s_b4_n100_m50_q10_f64", "c5s_b6_n64_m64_f64",
                                  "broadcast_b5_n12_m9_q3", "unbatched_n12_m9_q3"])
def test_golden_batches(dev, name):
    g = load_golden(name)
    z, grads = run_qpf(golden_inputs(g), g["dl_dz"], dev)
    assert z.shape == g["zhat"].shape
    assert rel_err(z, g["zhat"]).max() < TOL
    for k, gr in zip(("dQ", "dp", "dG", "dh", "dA", "db"), grads):
        if k in g:
            assert gr.shape == g[k].shape, k
            assert np.abs(gr - g[k]).max() <= 10 * TOL * max(1.0, np.abs(g[k]).max()), k


def test_solver_entry_points_match_reference(dev):
    """pre_factor_kkt / factor_kkt / solve_kkt / forward, the seam of qp.py:92-96,148-155."""
    from qpth_amd.solvers.pdipm import batch as pdipm_b
    g = load_golden("kkt_solver")
    Q, p, G, h, A, b = to_dev([g[k] for k in ("Q", "p", "G", "h", "A", "b")], dev, grad=False)
    Qe, Ae = Q.unsqueeze(0).expand(2, 5, 5), A.unsqueeze(0).expand(2, 3, 5)
    d, rx, rs, rz, ry = to_dev([g[k] for k in ("d", "rx", "rs", "rz", "ry")], dev, grad=False)
    Q_LU, S_LU, R = pdipm_b.pre_factor_kkt(Qe, G, Ae)
    pdipm_b.factor_kkt(S_LU, R, d)
    outs = pdipm_b.solve_kkt(Q_LU, d, G, Ae, S_LU, rx, rs, rz, ry)
    for mine, key in zip(outs, ("dx", "ds", "dz", "dy")):
        assert np.allclose(mine.cpu().numpy(), g[key], rtol=1e-8, atol=1e-9), key
    g = load_golden("c3s_b4_n20_m10_q4_f64")
    Q, p, G, h, A, b = to_dev(golden_inputs(g), dev, grad=False)
    Q_LU, S_LU, R = pdipm_b.pre_factor_kkt(Q, G, A)
    x, y, z, s = pdipm_b.forward(Q, p, G, h, A, b, Q_LU, S_LU, R, verbose=-1)
    assert rel_err(x.cpu().numpy(), g["zhat"]).max() < TOL
    assert rel_err(y.cpu().numpy(), g["nu"]).max() < TOL
    assert rel_err(z.cpu().numpy(), g["lam"]).max() < 1e-5
    assert np.abs(s.cpu().numpy() - g["slacks"]).max() < 1e-6


# ---------------------------------------------------------------- accuracy options (batch.py:216-346) on the GPU
def test_solve_kkt_ir_and_full_solvers_match_the_reference(dev):
    """solve_kkt_ir (both call forms), factor_solve_kkt and the regularised full solve against the reference's
    factor_solve_kkt outputs (golden full_*, test.py:222-247)."""
    from qpth_amd.solvers.pdipm import batch as pdipm_b
    g = load_golden("kkt_solver")
    Q, G, A = to_dev([g[k] for k in ("Q", "G", "A")], dev, grad=False)
    Qe, Ae = Q.unsqueeze(0).expand(2, 5, 5), A.unsqueeze(0).expand(2, 3, 5)
    d, rx, rs, rz, ry = to_dev([g[k] for k in ("d", "rx", "rs", "rz", "ry")], dev, grad=False)
    D = torch.diag_embed(d)
    Q_LU, S_LU, R = pdipm_b.pre_factor_kkt(Qe, G, Ae)
    outs = {"handles": pdipm_b.solve_kkt_ir(Q_LU, d, G, Ae, S_LU, rx, rs, rz, ry, niter=1),
            "reference form": pdipm_b.solve_kkt_ir(Qe, D, G, Ae, rx, rs, rz, ry, niter=2),
            "factor_solve_kkt": pdipm_b.factor_solve_kkt(Qe, D, G, Ae, rx, rs, rz, ry)}
    for name, o in outs.items():
        for mine, key in zip(o, ("dx", "ds", "dz", "dy")):
            assert np.allclose(mine.cpu().numpy(), g["full_" + key], rtol=1e-8, atol=1e-9), (name, key)
            assert np.allclose(mine.cpu().numpy(), g[key], rtol=1e-8, atol=1e-9), (name, key)
    # the regularised solve with equality constraints (round 4), as the reference's solve_kkt_ir uses it (eps = 1e-7):
    # within 1e-5 of the un-regularised golden solution
    e5, e4 = torch.eye(5, dtype=torch.float64, device=dev), torch.eye(4, dtype=torch.float64, device=dev)
    for mine, key in zip(pdipm_b.factor_solve_kkt_reg(Qe + 1e-7 * e5, D + 1e-7 * e4, G, Ae, rx, rs, rz, ry, 1e-7), ("dx", "ds", "dz", "dy")):
        assert np.allclose(mine.cpu().numpy(), g["full_" + key], rtol=1e-5, atol=1e-5), key
    # regularised solve without equality constraints against a dense numpy solve of the same system
    B, n, m, eps = 4, 100, 100, 1e-3
    Qn, pn, Gn, hn, An, bn = problems.prof_qp(B, n, m, 0, seed=4)
    r = np.random.RandomState(2)
    dn, rxn, rsn, rzn = r.rand(B, m) + 0.1, r.randn(B, n), r.randn(B, m), r.randn(B, m)
    tQ, tG, td, trx, trs, trz = to_dev([Qn, Gn, dn, rxn, rsn, rzn], dev, grad=False)
    dx, ds, dz, dy = pdipm_b.factor_solve_kkt_reg(tQ, torch.diag_embed(td), tG, torch.empty(0, dtype=torch.float64, device=dev),
                                                  trx, trs, trz, None, eps)
    for i in range(B):
        K = np.zeros((n + 2 * m, n + 2 * m))
        K[:n, :n] = Qn[i]; K[:n, n + m:] = Gn[i].T
        K[n:n + m, n:n + m] = np.diag(dn[i]); K[n:n + m, n + m:] = np.eye(m)
        K[n + m:, :n] = Gn[i]; K[n + m:, n:n + m] = np.eye(m); K[n + m:, n + m:] = -eps * np.eye(m)
        sol = np.linalg.solve(K, -np.concatenate([rxn[i], rsn[i], rzn[i]]))
        for mine, ref in ((dx[i], sol[:n]), (ds[i], sol[n:n + m]), (dz[i], sol[n + m:])):
            assert np.abs(mine.cpu().numpy() - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("solver", ["LU_FULL", "LU_PARTIAL", "IR_UNOPT"])
@pytest.mark.parametrize("name", ["c3s_b4_n20_m10_q4_f64", "c2s_b4_n100_m100_f64", "c3s_b4_n100_m50_q10_f64"])
def test_forward_with_every_kkt_solver_matches_the_reference(dev, solver, name):
    """forward(..., solver=KKTSolvers.X) (batch.py:47-48) against the reference's golden vectors"""
    from qpth_amd.solvers.pdipm import batch as pdipm_b
    g = load_golden(name)
    Q, p, G, h, A, b = to_dev(golden_inputs(g), dev, grad=False)
    Q_LU, S_LU, R = pdipm_b.pre_factor_kkt(Q, G, A)
    x, y, z, s = pdipm_b.forward(Q, p, G, h, A, b, Q_LU, S_LU, R, verbose=-1, solver=getattr(pdipm_b.KKTSolvers, solver))
    assert rel_err(x.cpu().numpy(), g["zhat"]).max() < TOL
    assert rel_err(z.cpu().numpy(), g["lam"]).max() < 1e-5
    if y is not None:
        assert rel_err(y.cpu().numpy(), g["nu"]).max() < TOL


def test_refinement_is_refused_where_no_kernel_implements_it(dev):
    """refine > 0 on the large-QP family: QPX_ERR_UNSUPPORTED (ABI v5), not a silently un-refined answer; QPFunction's
    float32 finishing stage there runs with plain solves and keeps the best iterate."""
    from qpth_amd.solvers.pdipm import batch as pdipm_b
    B, n, m = 4, 300, 300
    arrs = problems.prof_qp(B, n, m, 0, seed=1)
    Q, p, G, h, A, b = to_dev(arrs, dev, grad=False)
    r = np.random.RandomState(0)
    d, rx, rs, rz = to_dev([r.rand(B, m) + 0.1, r.randn(B, n), r.randn(B, m), r.randn(B, m)], dev, grad=False)
    Q_LU, S_LU, R = pdipm_b.pre_factor_kkt(Q, G, A)
    assert not Q_LU.fac.refine_ok
    pdipm_b.solve_kkt(Q_LU, d, G, A, S_LU, rx, rs, rz, None)
    with pytest.raises(RuntimeError, match="not supported"):
        pdipm_b.solve_kkt_ir(Q_LU, d, G, A, S_LU, rx, rs, rz, None, niter=1)
    # (what the finishing stage achieves at these sizes is pinned against the oracle in
    # test_large_qp_accuracy_options_against_the_oracle)


def test_float32_is_as_close_to_f64_as_the_reference_f32(dev):
    """C1 in float32: the path runs float64 arithmetic on the float32 tensors (QPX_F32_WIDE), so its answer is the float64
    solution of the float32-ROUNDED data: within 1e-6 of the oracle on that data (float32 rounding of the output), and
    -- the rounding of the data itself moves the solution by 1.5e-5 here -- no further from the reference's float64
    answer than the reference's own float32 run (3.0e-5)."""
    from oracle import qp_oracle as orc
    g32, g64 = load_golden("c1_b8_n10_m5_f32"), load_golden("c1_b8_n10_m5_f64")
    arrs32 = golden_inputs(g32, np.float32)
    z, _ = run_qpf(arrs32, g32["dl_dz"], dev, dtype=torch.float32)
    x, y, lam, s, info = orc.OracleQP(*[np.asarray(a_, np.float64) for a_ in arrs32]).forward()
    assert rel_err(z, x).max() < 1e-6, rel_err(z, x).max()
    mine = rel_err(z, g64["zhat"]).max()
    ref = rel_err(g32["zhat"], g64["zhat"]).max()
    assert mine <= ref, (mine, ref)


# ---------------------------------------------------------------- 2. oracle, seeded inputs
@pytest.mark.parametrize("B,n,m,q,seed", [(8, 10, 5, 0, 3), (64, 100, 100, 0, 0), (64, 100, 50, 10, 1),
                                           (128, 64, 64, 0, 2), (16, 33, 70, 7, 4), (32, 2, 40, 0, 5),
                                           (3, 130, 90, 20, 6)])
def test_against_oracle(dev, B, n, m, q, seed):
    """z*, lam, nu, slacks and all gradients vs the oracle in reference (whole-batch) semantics."""
    from oracle import qp_oracle as orc
    Q, p, G, h, A, b = problems.prof_qp(B, n, m, q, seed)
    dl = np.random.RandomState(seed).randn(B, n)
    x, y, lam, s, grads, info = orc.qp_forward_backward(Q, p, G, h, A, b, dl_dz=dl)
    z, mine = run_qpf([Q, p, G, h, A, b], dl, dev)
    assert rel_err(z, x).max() < TOL
    for a_, r_, k in zip(mine, grads, ("dQ", "dp", "dG", "dh", "dA", "db")):
        if r_ is not None:
            assert np.abs(a_ - r_).max() <= 1e-5 * max(1.0, np.abs(r_).max()), k


def test_duals_against_oracle(dev):
    from oracle import qp_oracle as orc
    from qpth_amd.kkt import KKTFactors
    Q, p, G, h, A, b = problems.prof_qp(32, 100, 50, 10, 9)
    x, y, lam, s, info = orc.OracleQP(Q, p, G, h, A, b).forward()
    tQ, tp, tG, th, tA, tb = to_dev([Q, p, G, h, A, b], dev, grad=False)
    fac = KKTFactors.build(tQ, tG, tA)
    res = fac.ipm(tp, th, tb)
    torch.cuda.synchronize()
    assert int(res.status.max().item()) & 3 == 0
    assert rel_err(res.zhat.cpu().numpy(), x).max() < TOL
    assert rel_err(res.nu.cpu().numpy(), y).max() < TOL
    assert rel_err(res.lam.cpu().numpy(), lam).max() < 1e-5
    assert np.abs(res.slacks.cpu().numpy() - s).max() < 1e-6


# ---------------------------------------------------------------- 3. properties at full size
def kkt_residuals(Q, p, G, h, A, b, z, lam, nu, s):
    """solver-free optimality measures: stationarity, primal feasibility,
    dual feasibility, complementarity -- evaluated in torch on the device."""
    rx = torch.einsum("bij,bj->bi", Q, z) + p + torch.einsum("bmi,bm->bi", G, lam)
    if A.nelement():
        rx = rx + torch.einsum("bqi,bq->bi", A, nu)
        ry = torch.einsum("bqi,bi->bq", A, z) - b
    else:
        ry = torch.zeros(z.shape[0], 1, dtype=z.dtype, device=z.device)
    gz = torch.einsum("bmi,bi->bm", G, z) - h
    return (rx.norm(dim=1), torch.clamp(gz, min=0).norm(dim=1), ry.norm(dim=1),
            torch.clamp(-lam, min=0).norm(dim=1), (lam * gz).abs().sum(1), (gz + s).norm(dim=1))


@pytest.mark.parametrize("B,n,m,q", [(512, 100, 100, 0), (512, 100, 50, 10), (4096, 64, 64, 0)])
def test_full_size_optimality(dev, B, n, m, q):
    """BASELINE.json C2 / C3 / (a 4096-QP slab of) C5 at full per-QP size: every QP's answer
    satisfies the KKT conditions to round-off scale (the reference reaches ~1e-12)."""
    from qpth_amd.kkt import KKTFactors
    arrs = problems.prof_qp(B, n, m, q, seed=0)
    tQ, tp, tG, th, tA, tb = to_dev(arrs, dev, grad=False)
    fac = KKTFactors.build(tQ, tG, tA)
    res = fac.ipm(tp, th, tb)
    torch.cuda.synchronize()
    assert int(res.status.max().item()) & 7 == 0
    stat, pinf, einf, dinf, comp, slk = kkt_residuals(tQ, tp, tG, th, tA, tb, res.zhat, res.lam, res.nu, res.slacks)
    scale = (tp.norm(dim=1) + th.norm(dim=1)).max().item()
    for name, v, tol in (("stationarity", stat, 1e-8), ("primal", pinf, 1e-8), ("equality", einf, 1e-8),
                         ("dual sign", dinf, 1e-12), ("complementarity", comp, 1e-8), ("slack", slk, 1e-8)):
        assert v.max().item() < tol * scale, (name, v.max().item(), scale)
    assert res.iters.max().item() <= 20 and res.iters.float().mean().item() < 18


def test_full_size_matches_oracle_c2(dev):
    """The headline config (batch=512 nz=100 nineq=100) against the oracle: ~1 s of CPU."""
    from oracle import qp_oracle as orc
    Q, p, G, h, A, b = problems.prof_qp(512, 100, 100, 0, 0)
    dl = np.ones((512, 100))
    x, y, lam, s, grads, info = orc.qp_forward_backward(Q, p, G, h, A, b, dl_dz=dl)
    z, mine = run_qpf([Q, p, G, h, A, b], dl, dev)
    assert rel_err(z, x).max() < TOL                    # north star: 1e-4
    assert np.abs(mine[1] - grads[1]).max() <= 1e-5 * np.abs(grads[1]).max()
    assert np.abs(mine[0] - grads[0]).max() <= 1e-5 * np.abs(grads[0]).max()


def test_full_size_matches_oracle_c2_all_gradients(dev):
    """C2 at full size: every output and every gradient (dQ, dp, dG, dh) against the oracle."""
    from oracle import qp_oracle as orc
    Q, p, G, h, A, b = problems.prof_qp(512, 100, 100, 0, 1)
    dl = np.random.RandomState(1).randn(512, 100)
    x, y, lam, s, grads, info = orc.qp_forward_backward(Q, p, G, h, A, b, dl_dz=dl)
    z, mine = run_qpf([Q, p, G, h, A, b], dl, dev)
    assert rel_err(z, x).max() < TOL
    for k, a_, r_ in zip(("dQ", "dp", "dG", "dh"), mine, grads):
        assert np.abs(a_ - r_).max() <= 1e-5 * max(1.0, np.abs(r_).max()), k


def test_full_size_matches_oracle_c3_all_gradients(dev):
    """C3 at its full size (batch=512, nz=100, nineq=50, neq=10): every output and all six gradients against the oracle."""
    from oracle import qp_oracle as orc
    Q, p, G, h, A, b = problems.prof_qp(512, 100, 50, 10, 2)
    dl = np.random.RandomState(2).randn(512, 100)
    x, y, lam, s, grads, info = orc.qp_forward_backward(Q, p, G, h, A, b, dl_dz=dl)
    z, mine = run_qpf([Q, p, G, h, A, b], dl, dev)
    assert rel_err(z, x).max() < TOL
    for k, a_, r_ in zip(("dQ", "dp", "dG", "dh", "dA", "db"), mine, grads):
        assert np.abs(a_ - r_).max() <= 1e-5 * max(1.0, np.abs(r_).max()), k


def test_c5_shard_gradients_match_oracle(dev):
    """one GPU's share of C5 (8 192 QPs of nz = nineq = 64): gradients of every 32nd QP against the oracle"""
    from oracle import qp_oracle as orc
    B, n, m = 8192, 64, 64
    Q, p, G, h, A, b = problems.prof_qp(B, n, m, 0, 5)
    dl = np.random.RandomState(5).randn(B, n)
    z, mine = run_qpf([Q, p, G, h, A, b], dl, dev)
    sub = np.arange(0, B, 32)
    x, y, lam, s, grads, info = orc.qp_forward_backward(Q[sub], p[sub], G[sub], h[sub], A, b, dl_dz=dl[sub],
                                                         per_qp=True, stall_policy=1)
    assert rel_err(z[sub], x).max() < TOL
    for k, a_, r_ in zip(("dQ", "dp", "dG", "dh"), mine, grads):
        assert np.abs(a_[sub] - r_).max() <= 1e-5 * max(1.0, np.abs(r_).max()), k


def test_bench_table_rows_name_their_arithmetic(dev):
    """bench.py --table prof-gurobi (prof-gurobi.py:37-48,115-118): one JSON row per batch size, each saying which
    arithmetic the kernels ran"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--table", "prof-gurobi"],
                         capture_output=True, text=True, timeout=280, check=True).stdout
    rows = [json.loads(ln) for ln in out.splitlines() if ln.strip().startswith("{")]
    assert [r["nBatch"] for r in rows] == [1, 64, 128]
    for r in rows:
        assert r["table"] == "prof-gurobi" and r["arithmetic"] == "f64" and r["pre_factor_plus_forward_ms"] > 0


def test_full_size_matches_oracle_c4(dev):
    """BASELINE.json configs[3] at its full size (batch=128, nz=nineq=500): zhat, lam, slacks and all four
    gradients against the oracle (about 10 s of CPU).  Tolerances: zhat 1e-6 (north star 1e-4); multipliers and
    gradients 1e-5 of their scale."""
    from oracle import qp_oracle as orc
    from qpth_amd.kkt import KKTFactors
    B, n, m = 128, 500, 500
    Q, p, G, h, A, b = problems.prof_qp(B, n, m, 0, 0)
    dl = np.ones((B, n))
    x, y, lam, s, grads, info = orc.qp_forward_backward(Q, p, G, h, A, b, dl_dz=dl)
    z, mine = run_qpf([Q, p, G, h, A, b], dl, dev)
    assert rel_err(z, x).max() < TOL
    for k, a_, r_ in zip(("dQ", "dp", "dG", "dh"), mine, grads):
        assert np.abs(a_ - r_).max() <= 1e-5 * max(1.0, np.abs(r_).max()), k
    tQ, tp, tG, th, tA, tb = to_dev([Q, p, G, h, A, b], dev, grad=False)
    fac = KKTFactors.build(tQ, tG, tA)
    res = fac.ipm(tp, th, tb)
    torch.cuda.synchronize()
    assert int(res.status.max().item()) & 7 == 0
    assert np.abs(res.lam.cpu().numpy() - lam).max() < 1e-5 * max(1.0, np.abs(lam).max())
    assert np.abs(res.slacks.cpu().numpy() - s).max() < 1e-5 * max(1.0, np.abs(s).max())


def test_full_size_c4_float32_tensors(dev):
    """BASELINE.json configs[3] in float32 at its full size (the quoted C4-f32 rate had no parity test).
    Since round 4 float32 tensors run the large-QP family in float64 arithmetic (QPX_F32_WIDE: the pack kernels widen on
    load, outputs narrow on store), so the answer is the float64 solution of the float32 data: every QP within 1e-5
    of the oracle's float64 answer on the same (float32-rounded) data -- the gate of the C2 / C3 float32 test -- and
    the p-gradient within 1e-5 of its scale.  The float32 KERNELS (refine=2) are reported beside it as a distribution."""
    from oracle import qp_oracle as orc
    B, n, m = 128, 500, 500
    arrs32 = problems.prof_qp(B, n, m, 0, 0, np.float32)
    arrs64 = [np.asarray(a, np.float64) for a in arrs32]
    dl = np.ones((B, n))
    x, y, lam, s, grads, info = orc.qp_forward_backward(*arrs64, dl_dz=dl)
    z, mine = run_qpf(arrs32, dl.astype(np.float32), dev, dtype=torch.float32)
    assert z.dtype == np.float32
    err = rel_err(z, x)
    zk, _ = run_qpf(arrs32, dl.astype(np.float32), dev, dtype=torch.float32, refine=2)
    ek = rel_err(zk, x)
    print("C4 f32 rel err vs the f64 oracle: default (f64 arithmetic) median %.2e max %.2e | f32 kernels + 2 finishing steps median %.2e max %.2e"
          % (np.median(err), err.max(), np.median(ek), ek.max()))
    assert err.max() <= 1e-5, err.max()
    for k, a_, r_ in zip(("dQ", "dp", "dG", "dh"), mine, grads):
        assert a_.dtype == np.float32
        assert np.abs(a_ - r_).max() <= 1e-5 * max(1.0, np.abs(r_).max()), k
    assert np.median(ek) < 1e-3          # the float32 kernels: a distribution, not a gate (cond(Q) ~ 1e7 at nz = 500)


@pytest.mark.parametrize("B,n,m,q,seed", [(16, 300, 200, 50, 11), (8, 150, 400, 70, 12), (4, 500, 500, 100, 13)])
def test_large_qps_with_equality_constraints(dev, B, n, m, q, seed):
    """Equality constraints beyond nz+neq+nineq = 208 (VERDICT r3 missing #2: these ran the round-1 workgroup kernels):
    the large-QP family with the projected Zt (qpx_big.h), zhat, nu, lam, slacks and all six gradients against the
    oracle.  neq = 50 / 70 / 100: one and two blocks of 64 in the blocked solves with L11."""
    from oracle import qp_oracle as orc
    from qpth_amd import _lib
    from qpth_amd.kkt import KKTFactors
    assert _lib.hip().dll.qpx_kernel_family(_lib.QPX_F64, n, m, q) == _lib.FAMILY_BIG
    Q, p, G, h, A, b = problems.prof_qp(B, n, m, q, seed)
    dl = np.random.RandomState(seed).randn(B, n)
    x, y, lam, s, grads, info = orc.qp_forward_backward(Q, p, G, h, A, b, dl_dz=dl)
    z, mine = run_qpf([Q, p, G, h, A, b], dl, dev)
    assert rel_err(z, x).max() < TOL
    for k, a_, r_ in zip(("dQ", "dp", "dG", "dh", "dA", "db"), mine, grads):
        assert np.abs(a_ - r_).max() <= 1e-5 * max(1.0, np.abs(r_).max()), k
    tQ, tp, tG, th, tA, tb = to_dev([Q, p, G, h, A, b], dev, grad=False)
    fac = KKTFactors.build(tQ, tG, tA)
    res = fac.ipm(tp, th, tb)
    torch.cuda.synchronize()
    assert int(res.status.max().item()) & 7 == 0
    for name, a_, r_ in (("nu", res.nu, y), ("lam", res.lam, lam), ("slacks", res.slacks, s)):
        assert np.abs(a_.cpu().numpy() - r_).max() < 1e-5 * max(1.0, np.abs(r_).max()), name
    # the same QPs as float32 tensors (float64 arithmetic): the float64 answer of the rounded data
    # the same QPs as float32 tensors (float64 arithmetic, QPX_F32_WIDE): the float64 answer of the ROUNDED data -- every QP
    # within 1e-5 of the oracle on that data (the gate of the C4 float32 test), gradients within 1e-5 of their scale
    arrs32 = [np.asarray(a_, np.float32) for a_ in (Q, p, G, h, A, b)]
    x32, _, _, _, grads32, _ = orc.qp_forward_backward(*[np.asarray(a_, np.float64) for a_ in arrs32], dl_dz=dl.astype(np.float32).astype(np.float64))
    z32, mine32 = run_qpf(arrs32, dl.astype(np.float32), dev, dtype=torch.float32)
    e32 = rel_err(z32, x32)
    print("n=%d m=%d q=%d float32 tensors vs the f64 oracle on the rounded data: max rel err %.2e (on the f64 data: %.2e)"
          % (n, m, q, e32.max(), rel_err(z32, x).max()))
    assert z32.dtype == np.float32 and e32.max() <= 1e-5, e32.max()
    for k, a_, r_ in zip(("dQ", "dp", "dG", "dh", "dA", "db"), mine32, grads32):
        assert a_.dtype == np.float32
        assert np.abs(a_ - r_).max() <= 1e-5 * max(1.0, np.abs(r_).max()), k


@pytest.mark.parametrize("B,n,m,q,seed", [(4, 768, 768, 0, 21), (3, 600, 520, 40, 22), (2, 1000, 1024, 0, 23)])
def test_sizes_beyond_512_against_the_oracle(dev, B, n, m, q, seed):
    """Round 6: max(nz, nineq, neq) up to 1 024 (the reference has no cap, batch.py:375-470; until round 6 the library
    refused sizes beyond 512).  The large-QP family with sixteen vector slots per lane, substitution steps streamed in rounds
    of five blocks, sixteen blocks of the vector in the mat-vec's LDS: zhat, nu, lam, slacks and every gradient against the
    oracle (batch-of-one semantics), float64; and as float32 tensors in float64 arithmetic within 1e-5 of the oracle on the
    rounded data.  The finishing stage stops at 512 (its 23 vectors per QP in LDS) and says so."""
    from oracle import qp_oracle as orc
    from qpth_amd import _lib
    from qpth_amd.kkt import KKTFactors
    dll = _lib.hip().dll
    assert dll.qpx_max_dim() == 1024 and dll.qpx_kernel_family(_lib.QPX_F64, n, m, q) == _lib.FAMILY_BIG
    assert dll.qpx_supported(_lib.QPX_F64, 1025, 10, 0) == -2 and dll.qpx_polish_supported(_lib.QPX_F64, n, m, q) == 0
    Q, p, G, h, A, b = problems.prof_qp(B, n, m, q, seed)
    dl = np.random.RandomState(seed).randn(B, n)
    x, y, lam, s, grads, info = orc.qp_forward_backward(Q, p, G, h, A, b, dl_dz=dl, per_qp=True)
    z, mine = run_qpf([Q, p, G, h, A, b], dl, dev)
    assert rel_err(z, x).max() < TOL
    for k, a_, r_ in zip(("dQ", "dp", "dG", "dh", "dA", "db"), mine, grads):
        if r_ is not None and np.size(r_):
            assert np.abs(a_ - r_).max() <= 1e-5 * max(1.0, np.abs(r_).max()), k
    tQ, tp, tG, th, tA, tb = to_dev([Q, p, G, h, A, b], dev, grad=False)
    fac = KKTFactors.build(tQ, tG, tA)
    res = fac.ipm(tp, th, tb)
    torch.cuda.synchronize()
    assert int(res.status.max().item()) & 7 == 0
    for name, a_, r_ in (("lam", res.lam, lam), ("slacks", res.slacks, s)) + ((("nu", res.nu, y),) if q else ()):
        assert np.abs(a_.cpu().numpy() - r_).max() < 1e-5 * max(1.0, np.abs(r_).max()), name
    arrs32 = [np.asarray(a_, np.float32) for a_ in (Q, p, G, h, A, b)]
    x32 = orc.qp_forward_backward(*[np.asarray(a_, np.float64) for a_ in arrs32], dl_dz=dl, per_qp=True)[0]
    z32, _ = run_qpf(arrs32, dl.astype(np.float32), dev, dtype=torch.float32)
    e32 = rel_err(z32, x32)
    print("n=%d m=%d q=%d float32 tensors vs the f64 oracle on the rounded data: max rel err %.2e" % (n, m, q, e32.max()))
    assert z32.dtype == np.float32 and e32.max() <= 1e-5, e32.max()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("shape", [(8192, 10, 100), (8192, 100, 100), (700, 64, 64), (100, 3, 3)])
def test_batch_contraction_in_two_stages(dev, shape, dtype):
    """qpx_batch_outer at the shapes of shared-parameter gradients (dA 10 x 100 and dQ 100 x 100 at one GPU's share of C5,
    qp.py:159-177): two stages with the workspace (partial tiles per batch chunk, summed in chunk order -- twice: the same
    bits) and one stage without it, both against the float64 sum of outer products."""
    from qpth_amd import _lib
    B, r, c = shape
    g = torch.Generator().manual_seed(B + r)
    u, w = [torch.randn(B, r, dtype=dtype, generator=g).to(dev) for _ in range(2)]
    v, x = [torch.randn(B, c, dtype=dtype, generator=g).to(dev) for _ in range(2)]
    ref = (0.5 / B * (u.double().t() @ v.double() + w.double().t() @ x.double())).cpu()
    lib = _lib.hip()
    code = _lib.QPX_F64 if dtype == torch.float64 else _lib.QPX_F32
    need = int(lib.dll.qpx_batch_outer_workspace_elems(code, B, r, c))
    assert (need > 0) == (B > 256)
    outs = []
    for rep in range(2):
        out = torch.full((r, c), float("nan"), dtype=dtype, device=dev)
        lib.batch_outer(u, v, w, x, 0.5, out)
        outs.append(out.cpu())
    one = torch.full((r, c), float("nan"), dtype=dtype, device=dev)
    lib.check(lib.dll.qpx_batch_outer(code, B, r, c, u.data_ptr(), v.data_ptr(), w.data_ptr(), x.data_ptr(), 0.5,
                                      one.data_ptr(), None, 0, torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    tol = 1e-12 if dtype == torch.float64 else 2e-5
    for o in (outs[0], one.cpu()):
        assert (o.double() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


def test_large_qp_accuracy_options_against_the_oracle(dev):
    """the accuracy options beyond nz+neq+nineq = 208 were only compared with themselves.  At n=300
    m=200 q=50 (large-QP family): forward(solver=KKTSolvers.IR_UNOPT) in float64 against the oracle at the tolerances of
    the default path (zhat 1e-6, multipliers 1e-5 of their scale); QPFunction(refine=2) on float32 tensors (the float32
    kernels + two finishing iterations on float64 residuals of the caller's data) against the oracle's float64 answer
    on the rounded data: EVERY QP inside the north star's 1e-4 gate, median <= 1e-5 (measured on the kernel bodies: 2.6e-8 /
    3.3e-7 where the float32 loop alone, refine=0, leaves 2.3e-4 / 4.6e-4)."""
    from oracle import qp_oracle as orc
    from qpth_amd import _lib
    from qpth_amd.qp import QPFunction
    from qpth_amd.solvers.pdipm import batch as pdipm_b
    B, n, m, q = 8, 300, 200, 50
    assert _lib.hip().dll.qpx_kernel_family(_lib.QPX_F64, n, m, q) == _lib.FAMILY_BIG
    arrs = problems.prof_qp(B, n, m, q, 21)
    x, y, lam, s, info = orc.OracleQP(*arrs).forward()
    Q, p, G, h, A, b = to_dev(arrs, dev, grad=False)
    Q_LU, S_LU, R = pdipm_b.pre_factor_kkt(Q, G, A)
    xi, yi, zi, si = pdipm_b.forward(Q, p, G, h, A, b, Q_LU, S_LU, R, verbose=-1, solver=pdipm_b.KKTSolvers.IR_UNOPT)
    assert rel_err(xi.cpu().numpy(), x).max() < TOL
    for name, a_, r_ in (("nu", yi, y), ("lam", zi, lam), ("slacks", si, s)):
        assert np.abs(a_.cpu().numpy() - r_).max() < 1e-5 * max(1.0, np.abs(r_).max()), name
    arrs32 = [np.asarray(a_, np.float32) for a_ in arrs]
    x32 = orc.OracleQP(*[np.asarray(a_, np.float64) for a_ in arrs32]).forward()[0]
    t32 = to_dev(arrs32, dev, torch.float32, grad=False)
    z0 = QPFunction(verbose=-1, refine=0)(*t32).cpu().numpy()
    z2 = QPFunction(verbose=-1, refine=2)(*t32).cpu().numpy()
    e0, e2 = rel_err(z0, x32), rel_err(z2, x32)
    print("n=%d m=%d q=%d float32 kernels vs the f64 oracle on the rounded data: refine=0 median %.2e max %.2e | refine=2 median %.2e max %.2e"
          % (n, m, q, np.median(e0), e0.max(), np.median(e2), e2.max()))
    assert np.median(e2) <= 1e-5 and e2.max() <= 1e-4


def test_c5_shard_matches_oracle_and_kkt(dev):
    """One GPU's share of BASELINE.json configs[4] (65 536 QPs over 8 GPUs = 8 192 per GPU, nz=nineq=64):
    every 32nd QP against the oracle (256 QPs, batch-of-one semantics so that the subset is the same problem),
    and the KKT conditions of all 8 192."""
    from oracle import qp_oracle as orc
    from qpth_amd.kkt import KKTFactors
    B, n, m = 8192, 64, 64
    arrs = problems.prof_qp(B, n, m, 0, seed=5)
    tQ, tp, tG, th, tA, tb = to_dev(arrs, dev, grad=False)
    fac = KKTFactors.build(tQ, tG, tA)
    res = fac.ipm(tp, th, tb)
    torch.cuda.synchronize()
    assert int(res.status.max().item()) & 7 == 0
    stat, pinf, einf, dinf, comp, slk = kkt_residuals(tQ, tp, tG, th, tA, tb, res.zhat, res.lam, res.nu, res.slacks)
    scale = (tp.norm(dim=1) + th.norm(dim=1)).max().item()
    for name, v, tol in (("stationarity", stat, 1e-8), ("primal", pinf, 1e-8), ("dual sign", dinf, 1e-12),
                         ("complementarity", comp, 1e-8), ("slack", slk, 1e-8)):
        assert v.max().item() < tol * scale, (name, v.max().item(), scale)
    sub = slice(0, B, 32)
    Q, p, G, h, A, b = arrs
    x, y, lam, s, info = orc.OracleQP(Q[sub], p[sub], G[sub], h[sub], A, b).forward(per_qp=True, stall_policy=1)
    assert rel_err(res.zhat.cpu().numpy()[sub], x).max() < TOL
    assert np.abs(res.lam.cpu().numpy()[sub] - lam).max() < 1e-5 * max(1.0, np.abs(lam).max())


def test_c5_whole_batch_on_one_gpu(dev):
    """BASELINE.json configs[4] as ONE launch sequence on one GPU: all 65 536 QPs of nz = nineq = 64 (round 5 verified one
    GPU's share of 8 192; the round-end scaling run multiplies exactly this point).  Forward + p-gradient through the
    one-wave kernels at eight workgroups per CU: the KKT conditions of every QP, every 128th QP (512 of them) against the
    oracle with batch-of-one semantics, and the gradient of those against the oracle's."""
    from oracle import qp_oracle as orc
    from qpth_amd.kkt import KKTFactors
    B, n, m = 65536, 64, 64
    arrs = problems.prof_qp(B, n, m, 0, seed=8)
    tQ, tp, tG, th, tA, tb = to_dev(arrs, dev, grad=False)
    fac = KKTFactors.build(tQ, tG, tA)
    res = fac.ipm(tp, th, tb)
    ones = torch.ones(B, n, dtype=torch.float64, device=dev)
    dp = fac.backward(res.zhat, res.lam, res.slacks, res.nu, ones, want=(False, True, False, False, False, False))[1]
    torch.cuda.synchronize()
    assert int(res.status.max().item()) & 7 == 0
    stat, pinf, einf, dinf, comp, slk = kkt_residuals(tQ, tp, tG, th, tA, tb, res.zhat, res.lam, res.nu, res.slacks)
    scale = (tp.norm(dim=1) + th.norm(dim=1)).max().item()
    for name, v, tol in (("stationarity", stat, 1e-8), ("primal", pinf, 1e-8), ("dual sign", dinf, 1e-12),
                         ("complementarity", comp, 1e-8), ("slack", slk, 1e-8)):
        assert v.max().item() < tol * scale, (name, v.max().item(), scale)
    sub = slice(0, B, 128)
    Q, p, G, h, A, b = arrs
    dl = np.ones((len(range(0, B, 128)), n))
    x, y, lam, s, grads, info = orc.qp_forward_backward(Q[sub], p[sub], G[sub], h[sub], A, b, dl_dz=dl, per_qp=True, stall_policy=1)
    assert rel_err(res.zhat.cpu().numpy()[sub], x).max() < TOL
    assert np.abs(res.lam.cpu().numpy()[sub] - lam).max() < 1e-5 * max(1.0, np.abs(lam).max())
    assert np.abs(dp.cpu().numpy()[sub] - grads[1]).max() < 1e-5 * max(1.0, np.abs(grads[1]).max())


def test_c5_shape_beyond_8192_qps_runs_the_one_wave_form(dev):
    """The dispatcher switches the C5 shape (nz = nineq = 64: four tile rows) from the chain-wave form to one wave per QP
    beyond 512 QPs per launch (round 6; 8 192 until then -- qpx_api.inc: tile_waves; BASELINE.json configs[4] on ONE GPU is
    65 536), where the one-wave kernels keep eight workgroups on a CU (20 KB of LDS each: operand tiles in place of the
    panel's rows, S = W, the mat-vec scratch on the factorisation's).  VERDICT r3: only the <= 8 192 side was exercised at size.  9 216 QPs: every 36th against the oracle (batch-of-one semantics, so the
    subset is the same problem), the KKT conditions of all, and the p-gradient of the subset."""
    from oracle import qp_oracle as orc
    from qpth_amd.kkt import KKTFactors
    B, n, m = 9216, 64, 64
    arrs = problems.prof_qp(B, n, m, 0, seed=6)
    tQ, tp, tG, th, tA, tb = to_dev(arrs, dev, grad=False)
    fac = KKTFactors.build(tQ, tG, tA)
    res = fac.ipm(tp, th, tb)
    torch.cuda.synchronize()
    assert int(res.status.max().item()) & 7 == 0
    stat, pinf, einf, dinf, comp, slk = kkt_residuals(tQ, tp, tG, th, tA, tb, res.zhat, res.lam, res.nu, res.slacks)
    scale = (tp.norm(dim=1) + th.norm(dim=1)).max().item()
    for name, v, tol in (("stationarity", stat, 1e-8), ("primal", pinf, 1e-8), ("dual sign", dinf, 1e-12),
                         ("complementarity", comp, 1e-8), ("slack", slk, 1e-8)):
        assert v.max().item() < tol * scale, (name, v.max().item(), scale)
    sub = slice(0, B, 36)
    Q, p, G, h, A, b = arrs
    dl = np.ones((len(range(0, B, 36)), n))
    x, y, lam, s, grads, info = orc.qp_forward_backward(Q[sub], p[sub], G[sub], h[sub], A, b, dl_dz=dl, per_qp=True, stall_policy=1)
    assert rel_err(res.zhat.cpu().numpy()[sub], x).max() < TOL
    dQ, dp, dG, dh, dA, db = fac.backward(res.zhat, res.lam, res.slacks, res.nu, torch.ones(B, n, dtype=torch.float64, device=dev),
                                          want=(False, True, False, False, False, False))
    assert np.abs(dp.cpu().numpy()[sub] - grads[1]).max() <= 1e-5 * max(1.0, np.abs(grads[1]).max())


@pytest.mark.parametrize("name", ["f32pair_c2_b32_n100_m100", "f32pair_c3_b32_n100_m50_q10"])
def test_float32_error_distribution_matches_the_reference(dev, name):
    """f32 at the C2 / C3 sizes: the error of the HIP path against the reference's f64 answer, as a
    DISTRIBUTION, next to the reference's own f32-vs-f64 distribution on the same 32 QPs (the generator's Q has
    cond ~ 1.6e6, so f32 cannot meet the 1e-4 gate on every QP in either implementation: the reference's own
    max is 4.5e-4 at C2 and 5e-3 at C3).  Asserted: median within 10x, maximum within 4x of the reference's -- for
    the default (QPFunction(refine=None): float32 data, float64 arithmetic on the matrix cores at these sizes) and
    for the float32 kernels with two finishing steps (refine=2: iterations on the residuals of the original
    data, KKTFactors.polish); the float32 loop kernel alone (refine=0) is printed beside them."""
    g = load_golden(name)
    B, n, m, q, seed = [int(v) for v in g["shape"]]
    arrs = problems.prof_qp(B, n, m, q, seed, np.float32)
    z, _ = run_qpf(arrs, np.ones((B, n), np.float32), dev, dtype=torch.float32)
    zfast, _ = run_qpf(arrs, np.ones((B, n), np.float32), dev, dtype=torch.float32, refine=0)
    zpol, _ = run_qpf(arrs, np.ones((B, n), np.float32), dev, dtype=torch.float32, refine=2)
    pol = rel_err(zpol, g["zhat_f64"])
    assert z.dtype == np.float32
    mine = rel_err(z, g["zhat_f64"])
    fast = rel_err(zfast, g["zhat_f64"])
    ref = rel_err(g["zhat_f32"], g["zhat_f64"])
    print("%s f32 rel err vs f64 reference: default (f64 arithmetic) median %.2e max %.2e | f32 kernels + 2 finishing steps "
          "median %.2e max %.2e | f32 loop kernel alone (refine=0) median %.2e max %.2e | reference f32 median %.2e max %.2e"
          % (name, np.median(mine), mine.max(), np.median(pol), pol.max(), np.median(fast), fast.max(),
             np.median(ref), ref.max()))
    # the default path (float64 arithmetic on the float32 tensors) answers every QP far inside the north star's 1e-4
    assert mine.max() <= 1e-5, mine.max()
    # the float32 kernels + finishing steps: judged as a distribution, next to the reference's own float32 run
    assert np.median(pol) < 10 * np.median(ref), (np.median(pol), np.median(ref))
    assert pol.max() < max(4 * ref.max(), 1e-3), (pol.max(), ref.max())


@pytest.mark.parametrize("B,n,m,q,seed,shared", [(64, 100, 100, 0, 7, False), (64, 100, 50, 10, 8, False),
                                                  (256, 64, 64, 0, 9, False), (32, 12, 9, 3, 10, True)])
def test_float32_tensors_in_float64_arithmetic(dev, B, n, m, q, seed, shared):
    """QPX_F32_WIDE (the float32 default at the tile-kernel sizes): the float64 kernels read and write the float32
    tensors directly.  Forward and all gradients equal the float64 run on the same (float32-representable) data to
    float32 rounding; the factors kept between forward and backward are float64; with Q, G, A shared by the batch
    there is one factor blob and the gradients come out batch-mean reduced."""
    from qpth_amd.kkt import KKTFactors
    arrs32 = [np.asarray(a, np.float32) for a in problems.prof_qp(B, n, m, q, seed, np.float32)]
    if shared:
        arrs32 = [arrs32[0][0], arrs32[1], arrs32[2][0], arrs32[3] + 1.0, arrs32[4][0] if q else arrs32[4], arrs32[5]]
        z0 = np.random.RandomState(seed).randn(B, n).astype(np.float32)
        arrs32[3] = (z0 @ arrs32[2].T + np.random.RandomState(seed + 1).rand(B, m)).astype(np.float32)
        if q:
            arrs32[5] = (z0 @ arrs32[4].T).astype(np.float32)
    dl = np.random.RandomState(seed + 2).randn(B, n).astype(np.float32)
    z32, g32 = run_qpf(arrs32, dl, dev, dtype=torch.float32)
    z64, g64 = run_qpf([a.astype(np.float64) for a in arrs32], dl.astype(np.float64), dev)
    assert z32.dtype == np.float32 and z32.shape == z64.shape
    assert rel_err(z32, z64).max() < 1e-6
    for k, a_, b_ in zip(("dQ", "dp", "dG", "dh", "dA", "db"), g32, g64):
        assert (a_ is None) == (b_ is None), k
        if a_ is not None:
            assert a_.dtype == np.float32 and a_.shape == b_.shape, k
            assert np.abs(a_ - b_).max() <= 2e-5 * max(1.0, np.abs(b_).max()), (k, np.abs(a_ - b_).max(), np.abs(b_).max())
    tq = to_dev(arrs32, dev, torch.float32, grad=False)
    fac = KKTFactors.build(tq[0], tq[2], tq[4], nBatch=B, wide=True)
    assert fac.blob.dtype == torch.float64 and fac.shared == shared


@pytest.mark.parametrize("name", ["c3s_b4_n20_m10_q4_f64", "broadcast_b5_n12_m9_q3", "sudoku_b16_n64_m64_q40_f64"])
def test_backward_from_external_solutions(dev, name):
    """QPSolvers.CVXPY (qp.py:97-120,142-155): the forward is an EXTERNAL solver's (zhat, nu, lam, slacks) --
    here the reference's own, replayed from the golden file by a registered stub -- and the backward is ours:
    ctx.fac is None, the factors are rebuilt (qp.py:142-143) and qpx_backward runs on the given solution."""
    from qpth_amd.qp import QPFunction, QPSolvers
    from qpth_amd.solvers import external
    g = load_golden(name)
    arrs = [g[k] for k in ("Q", "p", "G", "h", "A", "b")]
    calls = []

    def replay(Q, p, G, h, A, b):
        i = len(calls)
        calls.append(i)
        return g["zhat"][i], (g["nu"][i] if g["nu"].shape[1] else None), g["lam"][i], g["slacks"][i]

    external.set_solver(replay)
    try:
        tq = to_dev(arrs, dev)
        z = QPFunction(verbose=-1, solver=QPSolvers.CVXPY)(*tq)
        z.backward(torch.tensor(g["dl_dz"], device=dev))
        torch.cuda.synchronize()
    finally:
        external.set_solver(None)
    assert len(calls) == g["zhat"].shape[0]
    assert np.array_equal(z.detach().cpu().numpy(), g["zhat"])
    for k, t in zip(("dQ", "dp", "dG", "dh", "dA", "db"), tq):
        if k in g:
            gr = t.grad.cpu().numpy()
            assert gr.shape == g[k].shape, k
            assert np.abs(gr - g[k]).max() <= 1e-5 * max(1.0, np.abs(g[k]).max()), k


@pytest.mark.parametrize("name,dtype", [("cls_b32_n2_m200_f64", torch.float64), ("cls_b32_n2_m200_f32", torch.float32),
                                        ("sudoku_b16_n64_m64_q40_f64", torch.float64)])
def test_shared_parameter_callers(dev, name, dtype):
    """The shapes the reference's own callers use, parameters shared by the batch exactly as the notebooks pass
    them (example-cls-layer.ipynb cell 3: Q, G, h shared, nz=2, nineq=200; example-sudoku.ipynb cell 10:
    Q = 0.1 I, G = -I, h = 0, A, b shared, nz=nineq=64, neq=40).  One factor blob for the whole batch; shared
    gradients are the batch mean (qp.py:159-177), formed by qpx_batch_outer."""
    from qpth_amd.kkt import KKTFactors
    g = load_golden(name)
    arrs = [g[k] for k in ("Q", "p", "G", "h", "A", "b")]
    f32 = dtype == torch.float32
    z, grads = run_qpf(arrs, g["dl_dz"], dev, dtype=dtype)
    ztol, gtol = (2e-3, 2e-2) if f32 else (1e-6, 1e-5)
    assert np.abs(z - g["zhat"]).max() < ztol * max(1.0, np.abs(g["zhat"]).max())
    for k, gr in zip(("dQ", "dp", "dG", "dh", "dA", "db"), grads):
        if k in g:
            assert gr.shape == g[k].shape, k
            assert np.abs(gr - g[k]).max() <= gtol * max(1.0, np.abs(g[k]).max()), k
    tq = to_dev(arrs, dev, dtype=dtype, grad=False)
    fac = KKTFactors.build(tq[0], tq[2], tq[4], nBatch=g["zhat"].shape[0])
    assert fac.shared and fac.blob.numel() == fac.elems          # factored once, not B times


def test_needs_input_grad_is_honoured(dev):
    """Only the gradients autograd asks for are computed (ctx.needs_input_grad -> NULL outputs of qpx_backward),
    and they equal the ones of a run that asks for everything."""
    from qpth_amd.qp import QPFunction
    arrs = problems.prof_qp(16, 30, 20, 4, seed=2)
    dl = np.random.RandomState(2).randn(16, 30)
    _, full = run_qpf(arrs, dl, dev)
    for only in (1, 3, 2):                                        # p only (bench.py's case), h only, G only
        tq = to_dev(arrs, dev, grad=False)
        tq[only].requires_grad_(True)
        z = QPFunction(verbose=-1)(*tq)
        z.backward(torch.tensor(dl, device=dev))
        for i, t in enumerate(tq):
            assert (t.grad is not None) == (i == only)
        assert np.array_equal(tq[only].grad.cpu().numpy(), full[only])


def test_hard_problems_raise_the_reference_warnings(dev, capsys):
    """An infeasible QP and one with cond(Q) ~ 1e12 on the GPU: the loop must terminate, flag what the reference
    flags (INACC_ERR printed when the best residual stays > 1, batch.py:141-142,205-206), and the residual it
    claims for the returned iterate (whose dual part is analytic in the condensed formulation: tau sigma_z
    ||G^T 1||) must bound the true stationarity error ||Q z + p + G^T lam|| of that iterate to within 10x."""
    from qpth_amd import _lib
    from qpth_amd.kkt import KKTFactors
    from qpth_amd.qp import QPFunction
    # (a) infeasible: z <= -1 and -z <= -1
    n = 6
    Q = np.eye(n)[None].repeat(3, 0)
    p = np.random.RandomState(0).randn(3, n)
    G = np.concatenate([np.eye(n), -np.eye(n)], 0)[None].repeat(3, 0)
    h = -np.ones((3, 2 * n))
    tq = to_dev([Q, p, G, h, np.zeros(0), np.zeros(0)], dev, grad=False)
    z = QPFunction(verbose=0)(*tq)
    torch.cuda.synchronize()
    assert "Returning an inaccurate and potentially incorrect solution" in capsys.readouterr().out
    fac = KKTFactors.build(tq[0], tq[2], tq[4])
    res = fac.ipm(tq[1], tq[3], tq[5])
    torch.cuda.synchronize()
    assert all(int(s) & _lib.ST_INACCURATE for s in res.status.tolist())
    assert torch.isfinite(res.zhat).all()
    # (b) ill-conditioned Q (cond 1e12), feasible: must solve, and the reported residual must be honest
    r = np.random.RandomState(1)
    B, n, m = 8, 40, 30
    U = np.linalg.qr(r.randn(B, n, n))[0]
    Q = np.einsum("bij,j,bkj->bik", U, np.logspace(-6, 6, n), U)
    G = r.randn(B, m, n); z0 = r.randn(B, n); h = np.einsum("bmn,bn->bm", G, z0) + r.rand(B, m)
    p = r.randn(B, n)
    tq = to_dev([Q, p, G, h, np.zeros(0), np.zeros(0)], dev, grad=False)
    fac = KKTFactors.build(tq[0], tq[2], tq[4])
    res = fac.ipm(tq[1], tq[3], tq[5], want_trace=True)
    torch.cuda.synchronize()
    assert int(res.status.max().item()) & 3 == 0
    stat = kkt_residuals(*tq, res.zhat, res.lam, res.nu, res.slacks)[0].cpu().numpy()
    claimed = res.best_resid.cpu().numpy()                       # pri + dual + nineq mu of the returned iterate
    floor = 1e-9 * float(np.abs(Q).max() * np.abs(res.zhat.cpu().numpy()).max() + np.abs(p).max())
    for t, a in zip(stat, claimed):
        assert t < 10 * max(a, floor), (t, a, floor)


def test_iterative_refinement_of_the_kkt_solve(dev):
    """solve_kkt_ir (batch.py:244-270) on the GPU: one in-kernel refinement step on the residual of the original KKT
    system (accumulated in float64) cuts the float32 residual by > 50x at the C2 size."""
    from qpth_amd.solvers.pdipm import batch as pdipm_b
    B, n, m, q = 64, 100, 100, 0
    Q, p, G, h, A, b = problems.prof_qp(B, n, m, q, seed=2, dtype=np.float32)
    r = np.random.RandomState(1)
    d = (r.rand(B, m) + 0.1).astype(np.float32)
    rx, rs, rz = [r.randn(B, k).astype(np.float32) for k in (n, m, m)]
    tq = to_dev([Q, G, d, rx, rs, rz], dev, dtype=torch.float32, grad=False)
    e = torch.empty(0, dtype=torch.float32, device=dev)
    Q_LU, S_LU, R = pdipm_b.pre_factor_kkt(tq[0], tq[1], e)
    outs = []
    for niter in (0, 1):
        dx, ds, dz, dy = pdipm_b.solve_kkt_ir(Q_LU, tq[2], tq[1], e, S_LU, tq[3], tq[4], tq[5], None, niter=niter)
        dx, ds, dz = [v.double().cpu().numpy() for v in (dx, ds, dz)]
        Q64, G64 = Q.astype(np.float64), G.astype(np.float64)
        e1 = np.einsum('bij,bj->bi', Q64, dx) + np.einsum('bmi,bm->bi', G64, dz) + rx
        e2 = d * ds + dz + rs
        e3 = np.einsum('bmi,bi->bm', G64, dx) + ds + rz
        outs.append(np.sqrt((e1 ** 2).sum(1) + (e2 ** 2).sum(1) + (e3 ** 2).sum(1)))
    print("KKT residual, float32, C2 size: refine 0 median %.2e, refine 1 median %.2e" % (np.median(outs[0]), np.median(outs[1])))
    assert np.median(outs[1]) < np.median(outs[0]) / 50


def test_batch_permutation_equivariance(dev):
    """QPs are independent units: permuting the batch permutes the answers bit for bit."""
    from qpth_amd.kkt import KKTFactors
    arrs = problems.prof_qp(96, 40, 30, 5, seed=11)
    tq = to_dev(arrs, dev, grad=False)
    perm = torch.randperm(96, device=dev)
    fac = KKTFactors.build(tq[0], tq[2], tq[4])
    r0 = fac.ipm(tq[1], tq[3], tq[5])
    fac1 = KKTFactors.build(tq[0][perm], tq[2][perm], tq[4][perm])
    r1 = fac1.ipm(tq[1][perm], tq[3][perm], tq[5][perm])
    assert torch.equal(r0.zhat[perm], r1.zhat)
    assert torch.equal(r0.lam[perm], r1.lam)


def test_gradients_match_finite_differences(dev):
    """central differences of 1/2||zhat - t||^2 through the HIP forward vs the HIP backward
    (the replacement for the reference's cvxpy+numdifftools checks)."""
    from qpth_amd.qp import QPFunction
    Q, p, G, h, A, b = problems.random_dense_qp(1, 8, 6, 2, seed=3)
    tgt = np.random.RandomState(0).randn(1, 8)

    def loss(params):
        t = to_dev(params, dev, grad=False)
        z = QPFunction(verbose=-1, eps=1e-14)(*t)
        return 0.5 * float(((z - torch.tensor(tgt, device=dev)) ** 2).sum().item())

    tq = to_dev([Q, p, G, h, A, b], dev)
    z = QPFunction(verbose=-1, eps=1e-14)(*tq)
    z.backward(z.detach() - torch.tensor(tgt, device=dev))
    base = [Q, p, G, h, A, b]
    eps = 1e-6
    for idx, name in ((1, "dp"), (3, "dh"), (5, "db"), (2, "dG"), (4, "dA")):
        g = tq[idx].grad.cpu().numpy()
        fd = np.zeros_like(base[idx])
        it = np.nditer(base[idx], flags=["multi_index"])
        for _ in it:
            mi = it.multi_index
            plus = [x.copy() for x in base]; plus[idx][mi] += eps
            minus = [x.copy() for x in base]; minus[idx][mi] -= eps
            fd[mi] = (loss(plus) - loss(minus)) / (2 * eps)
        assert np.abs(fd - g).max() < 1e-5 * max(1.0, np.abs(g).max()), name


# ---------------------------------------------------------------- edge cases
def test_edge_cases(dev):
    from qpth_amd.qp import QPFunction
    e = torch.empty(0, dtype=torch.float64, device=dev)
    # nineq = 1, nz = 1
    z = QPFunction(verbose=-1)(torch.ones(1, 1, 1, dtype=torch.float64, device=dev),
                               torch.tensor([[-2.0]], dtype=torch.float64, device=dev),
                               torch.ones(1, 1, 1, dtype=torch.float64, device=dev),
                               torch.tensor([[1.0]], dtype=torch.float64, device=dev), e, e)
    assert abs(z.item() - 1.0) < 1e-8                        # min 1/2 z^2 - 2z s.t. z <= 1
    # inactive constraints only: z* = -Q^-1 p
    Q, p, G, h, A, b = problems.random_dense_qp(4, 6, 3, 0, seed=1)
    h = h + 1e3
    tq = to_dev([Q, p, G, h, A, b], dev, grad=False)
    z = QPFunction(verbose=-1)(*tq)
    ref = -np.linalg.solve(Q, p[..., None])[..., 0]
    assert rel_err(z.cpu().numpy(), ref).max() < 1e-8
    # not SPD
    with pytest.raises(RuntimeError, match="Q is not SPD."):
        QPFunction(verbose=-1)(-torch.eye(3, dtype=torch.float64, device=dev).unsqueeze(0), tq[1][:1, :3],
                               tq[2][:1, :, :3], tq[3][:1], e, e)
    # size beyond this build
    with pytest.raises(RuntimeError, match="not supported"):
        QPFunction(verbose=-1)(torch.eye(1100, dtype=torch.float64, device=dev).unsqueeze(0),       # (round 6: the cap is 1 024, was 512)
                               torch.zeros(1, 1100, dtype=torch.float64, device=dev),
                               torch.ones(1, 1, 1100, dtype=torch.float64, device=dev),
                               torch.ones(1, 1, dtype=torch.float64, device=dev), e, e)


def test_large_qp_hbm_resident_path(dev):
    """nz = nineq = 200 (f64) exceeds 160 KiB of LDS: matrices are worked on in the HBM blob."""
    from oracle import qp_oracle as orc
    Q, p, G, h, A, b = problems.prof_qp(4, 200, 200, 0, 3)
    x, y, lam, s, info = orc.OracleQP(Q, p, G, h, A, b).forward()
    z, _ = run_qpf([Q, p, G, h, A, b], np.ones((4, 200)), dev)
    assert rel_err(z, x).max() < TOL


# ---------------------------------------------------------------- 4. every form of the loop kernel
# include/qpx.h, qpx_set_ipm_variant: 3 = the large-QP multi-kernel family forced at small sizes, +256 / +512 = 16x16 / 8x8
# thread grid, +1024 = matrix-core tiles with 1 / 2 / 4 waves per QP (+2048 / +4096 / +8192)
LOOP_FORMS = [3, 256, 512, 1024 + 2048, 1024 + 4096, 1024 + 8192]


@pytest.mark.parametrize("variant", LOOP_FORMS)
@pytest.mark.parametrize("shape", [(6, 12, 9, 3), (48, 100, 100, 0), (32, 40, 52, 5)])
def test_every_loop_kernel_form(dev, variant, shape):
    """The dispatcher picks one form per (dtype, size, batch); all of them must agree with the oracle."""
    from oracle import qp_oracle as orc
    from qpth_amd import _lib
    B, n, m, q = shape
    arrs = problems.prof_qp(B, n, m, q, seed=11)
    dl = np.random.RandomState(5).randn(B, n)
    xr, _, _, _, grads_ref, _ = orc.qp_forward_backward(*arrs, dl, per_qp=True, stall_policy=2)
    old = _lib.hip().dll.qpx_set_ipm_variant(variant)
    try:
        z, grads = run_qpf(arrs, dl, dev)
    finally:
        _lib.hip().dll.qpx_set_ipm_variant(old)
    assert rel_err(z, xr).max() < TOL
    for mine, ref in zip(grads, grads_ref):
        if ref is not None and mine is not None:
            assert np.abs(mine - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())


PREFAC_SWEEP = 1 << 14      # include/qpx.h, qpx_set_ipm_variant: pre_factor_kkt by the thread-grid sweep


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("shape", [(512, 100, 100), (64, 64, 64), (33, 112, 96), (16, 70, 50), (8, 49, 112), (1024, 100, 10),
                                   (512, 100, 50, 10), (64, 96, 96, 16), (33, 60, 70, 6), (16, 40, 30, 10), (8, 90, 40, 5), (16, 64, 64, 40), (8, 60, 30, 50),
                                   (16, 36, 40), (8, 30, 100, 10), (8, 33, 20)])      # 33 <= nz + neq <= 48: four tile rows, part padding
def test_matrix_core_prefactorisation_against_the_sweep(dev, shape, wide):
    """Round 4: pre_factor_kkt (batch.py:375-429) on the matrix cores (qpx_prefac.h; 33 <= nz + neq <= 112) writes the
    blob the symmetric sweep writes -- -K, M^T, || G^T 1 ||, the tile image of R with its zero padding -- at C2's full
    size and at the sizes that exercise its padding paths; float32 tensors in float64 arithmetic too."""
    from qpth_amd import _lib
    from qpth_amd import kkt as _dp
    B, n, m = shape[:3]
    q = shape[3] if len(shape) > 3 else 0            # neq > 0: the factorisation is of [[Q, A^T], [A, 0]], nz + neq <= 112
    rng = np.random.default_rng(n * 1000 + m)
    L = rng.standard_normal((B, n, n))
    dt = torch.float32 if wide else torch.float64
    Q = torch.tensor(L @ L.transpose(0, 2, 1) + 1e-2 * np.eye(n), dtype=dt, device=dev)
    G = torch.tensor(rng.standard_normal((B, m, n)), dtype=dt, device=dev)
    e = torch.tensor(rng.standard_normal((B, q, n)), dtype=dt, device=dev) if q else torch.empty(0, dtype=dt, device=dev)
    blobs = []
    for variant in (0, PREFAC_SWEEP):
        old = _lib.hip().dll.qpx_set_ipm_variant(variant)
        try:
            fac = _dp.KKTFactors.build(Q, G, e, wide=wide)
            fac.raise_on_failure()
            blobs.append(fac.blob.reshape(B, -1).cpu().numpy().copy())
        finally:
            _lib.hip().dll.qpx_set_ipm_variant(old)
    al = lambda x: (x + 3) & ~3
    nbt = [t for t in (1, 2, 4, 7) if (m + 15) // 16 <= t][0]
    regions, o = {}, 0
    for name, size in (("Kneg", n * n), ("MT", n * m), ("NTn", q * n), ("W", m * q), ("S11i", q * q)):
        if size:
            regions[name] = (o, size)
        o += al(size)
    regions["gt1"] = (o, 1)
    regions["Rm"] = (o + 12, nbt * (nbt + 1) // 2 * 256)
    for name, (off, ln) in regions.items():
        mine, ref = blobs[0][:, off:off + ln], blobs[1][:, off:off + ln]
        assert np.abs(mine - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), name
        if name == "Rm":
            assert ((ref == 0) == (mine == 0)).all()
    # K against numpy (neq = 0: the inverse of Q)
    if q == 0:
        K = -blobs[0][:, :n * n].reshape(B, n, n)
        Kr = np.linalg.inv(Q.double().cpu().numpy())
        assert np.abs(K - Kr).max() <= 1e-8 * np.abs(Kr).max()


def test_matrix_core_prefactorisation_reports_a_q_that_is_not_spd(dev):
    """a pivot that is not positive in any panel of the factorisation raises what the sweep raises (batch.py:382-386)"""
    from qpth_amd.qp import QPFunction
    Q, p, G, h, A, b = to_dev(problems.prof_qp(64, 100, 50, 0, seed=3), dev, grad=False)
    for row in (0, 37, 99):
        Qb = Q.clone()
        Qb[5, row, row] = -1.0
        with pytest.raises(RuntimeError, match="Cannot perform LU factorization on Q"):
            QPFunction(verbose=-1, check_Q_spd=False)(Qb, p, G, h, A, b)
    z = QPFunction(verbose=-1)(Q, p, G, h, A, b)
    assert torch.isfinite(z).all()
    # with equality constraints: which block's pivot failed decides the message (batch.py:382-386, 419-423)
    Q, p, G, h, A, b = to_dev(problems.prof_qp(64, 100, 50, 10, seed=3), dev, grad=False)
    Qb = Q.clone()
    Qb[7, 98, 98] = -1.0
    with pytest.raises(RuntimeError, match="Cannot perform LU factorization on Q"):
        QPFunction(verbose=-1, check_Q_spd=False)(Qb, p, G, h, A, b)
    Ab, bb = A.clone(), b.clone()
    Ab[9, 4] = 0
    bb[9, 4] = 0
    with pytest.raises(RuntimeError, match="full row rank"):
        QPFunction(verbose=-1)(Q, p, G, h, Ab, bb)


# ---------------------------------------------------------------- 5. the bench contract
def test_full_size_c2_second_seed(dev):
    """C2 at its full size, a second seed and a random dl_dz: every QP and every gradient against the oracle (the
    chain-wave loop kernel; its round-3 siblings -- the four-wave form without the chain wave and the pre-factorisation on
    matrix-core tiles -- were deleted in round 4)."""
    from oracle import qp_oracle as orc
    arrs = problems.prof_qp(512, 100, 100, 0, seed=2)
    dl = np.random.RandomState(3).randn(512, 100)
    xr, _, lamr, sr, grads_ref, _ = orc.qp_forward_backward(*arrs, dl, per_qp=True, stall_policy=2)
    z, grads = run_qpf(arrs, dl, dev)
    assert rel_err(z, xr).max() < TOL
    for mine, ref in zip(grads, grads_ref):
        if ref is not None and mine is not None:
            assert np.abs(mine - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("variant", LOOP_FORMS)
@pytest.mark.parametrize("name", ["c3s_b4_n20_m10_q4_f64", "c2s_b4_n100_m100_f64"])
def test_every_loop_kernel_form_against_the_reference(dev, variant, name):
    """The same forms against the REFERENCE's own outputs (golden vectors made by the unmodified reference, whole-batch
    semantics): test_every_loop_kernel_form above checks them against the oracle run with this library's per-QP stop
    rule, which is a cross-form check, not reference parity."""
    from qpth_amd import _lib
    g = load_golden(name)
    old = _lib.hip().dll.qpx_set_ipm_variant(variant)
    try:
        z, grads = run_qpf(golden_inputs(g), g["dl_dz"], dev)
    finally:
        _lib.hip().dll.qpx_set_ipm_variant(old)
    assert rel_err(z, g["zhat"]).max() < TOL
    for k, gr in zip(("dQ", "dp", "dG", "dh", "dA", "db"), grads):
        if k in g:
            assert np.abs(gr - g[k]).max() <= 10 * TOL * max(1.0, np.abs(g[k]).max()), k


def test_bench_prints_one_json_line_with_the_contract_fields(dev):
    """bench.py --full: one JSON line on stdout, the metric of BASELINE.json, the roofline object of the dominant
    kernel.  (Short run, no CPU baseline.)"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "3", "--warmup", "1",
                          "--no-cpu-baseline"], capture_output=True, text=True, timeout=280, check=True).stdout
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["metric"].startswith("QPs/sec (fwd+bwd) at batch=512 nz=100 nineq=100")
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["dtype"] == "f64" and d["vs_baseline"] is None
    assert d["value"] > 0 and abs(d["value"] - 512 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    rf = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in rf, key
    assert rf["bound"] in ("hbm", "mfma") and 0 < rf["frac"] < 1
    # the default command with --full also carries BASELINE.json's C3 and C4, timed the same way behind the headline
    side = d["extra"]["other_baseline_configs"]
    for key, B in (("c3", 512), ("c4", 128)):
        assert side[key]["value"] > 0 and abs(side[key]["value"] - B / (side[key]["ms_per_step"] * 1e-3)) < 1e-6 * side[key]["value"]


def test_plain_bench_times_its_steps_and_dumps_what_they_returned(dev, tmp_path):
    """bench.py without --full: the headline fields only, `steps` timed steps, and --dump-outputs writes the last step's
    zhat and dp -- the answer QPFunction gives on the same seeded C2 batch."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=280, check=True).stdout
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"].startswith("QPs/sec (fwd+bwd) at batch=512 nz=100 nineq=100")
    assert d["unit"] == "QPs/s" and d["higher_is_better"] is True and d["dtype"] == "f64" and d["steps"] == 7
    assert d["value"] > 0 and abs(d["value"] - 512 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    for key in ("roofline", "cpu_baseline", "extra", "kernel_ms", "first_20_steps_qps"):
        assert key not in d, key
    assert sorted(os.listdir(tmp_path)) == ["dp.npy", "zhat.npy"]
    z_dump, dp_dump = np.load(tmp_path / "zhat.npy"), np.load(tmp_path / "dp.npy")
    assert z_dump.dtype == np.float64 and z_dump.shape == (512, 100) and dp_dump.shape == (512, 100)
    from qpth_amd.qp import QPFunction
    tq = to_dev(problems.prof_qp(512, 100, 100, 0, seed=0), dev, grad=False)
    tq[1].requires_grad_(True)                              # p alone, as in bench.py's step
    zt = QPFunction(verbose=-1)(*tq)
    zt.backward(torch.ones_like(zt))
    z, dp = zt.detach().cpu().numpy(), tq[1].grad.cpu().numpy()
    assert rel_err(z_dump, z).max() < 1e-9
    assert np.abs(dp_dump - dp).max() <= 1e-9 * max(1.0, np.abs(dp).max())


def test_max_iter_and_eps_are_honoured(dev):
    """QPFunction(eps, maxIter) (qp.py:18-20): stop on maxIter (status bit, best iterate returned) and on
    best_resid < eps (batch.py:127-140)."""
    from qpth_amd import _lib
    from qpth_amd.kkt import KKTFactors
    arrs = problems.prof_qp(64, 100, 100, 0, seed=4)
    Q, p, G, h, A, b = to_dev(arrs, dev, grad=False)
    fac = KKTFactors.build(Q, G, A)
    full = fac.ipm(p, h, b)
    loose = fac.ipm(p, h, b, eps=1e-3)
    capped = fac.ipm(p, h, b, maxIter=3)
    torch.cuda.synchronize()
    assert int(capped.iters.max()) == 3
    assert all(int(s) & _lib.ST_MAXITER for s in capped.status.tolist())
    assert torch.isfinite(capped.zhat).all()
    assert int(loose.iters.max()) < int(full.iters.min())
    assert float(loose.best_resid.max()) < 1e-3
    assert rel_err(loose.zhat.cpu().numpy(), full.zhat.cpu().numpy()).max() < 1e-2


@pytest.mark.parametrize("name", ["edge_b3_n1_m1_q0", "edge_b2_n6_m4_q5", "edge_dup_b2_n8_m10_q0"])
def test_edge_shapes_match_the_reference(dev, name):
    """One variable / one constraint; neq = nz - 1; duplicated inequality rows (their multipliers and the
    gradients with respect to the duplicated rows are not unique: only z*, slacks and the other gradients
    are compared there)."""
    g = load_golden(name)
    arrs = [g[k] for k in ("Q", "p", "G", "h", "A", "b")]
    z, grads = run_qpf(arrs, g["dl_dz"], dev)
    assert rel_err(z, g["zhat"]).max() < TOL
    for k, gr in zip(("dQ", "dp", "dG", "dh", "dA", "db"), grads):
        if k in g and gr is not None and not ("dup" in name and k in ("dG", "dh")):
            assert np.abs(gr - g[k]).max() <= 1e-5 * max(1.0, np.abs(g[k]).max()), k


@pytest.mark.parametrize("B,n,m,q", [(64, 100, 100, 0), (32, 100, 50, 10), (24, 300, 200, 20), (128, 260, 260, 0)])
def test_launch_sequence_replays_from_a_captured_graph(dev, B, n, m, q):
    """The boundary is stream-ordered (include/qpx.h: every entry point enqueues on the caller's stream and returns; the
    large-QP family forks and joins its side streams with events): the launch sequence of pre-factorisation + PDIPM loop +
    backward is captured into ONE hipGraph and replayed on new data in the same buffers.  Asserted: the replay is bit-identical
    to the eager calls on the same data (same kernels, same order), for the tile kernels, the thread grid with equality
    constraints, the large-QP family with one part and with two parts on two streams (B >= 96)."""
    from qpth_amd.kkt import KKTFactors
    first = to_dev(problems.prof_qp(B, n, m, q, seed=21), dev, grad=False)
    second = to_dev(problems.prof_qp(B, n, m, q, seed=22), dev, grad=False)
    ones = torch.ones(B, n, dtype=torch.float64, device=dev)

    def run(Q, p, G, h, A, b):
        fac = KKTFactors.build(Q, G, A)
        res = fac.ipm(p, h, b)
        grads = fac.backward(res.zhat, res.lam, res.slacks, res.nu, ones)
        return [res.zhat, res.lam, res.slacks, res.iters, res.status] + [g for g in grads if g is not None]

    eager = [[t.clone() for t in run(*data)] for data in (first, second)]       # (also the warm-up: LDS opt-ins, side streams)
    torch.cuda.synchronize()
    static = [t.clone() for t in first]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(*static)
    for data, want in ((first, eager[0]), (second, eager[1]), (first, eager[0])):
        for s, t in zip(static, data):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        for got, exp in zip(outs, want):
            assert torch.equal(got, exp), (B, n, m, q)
    assert int(outs[4].max().item()) & 7 == 0


def test_large_qp_parts_on_a_caller_stream_among_many(dev):
    """The large-QP family runs a batch of >= 96 QPs as two parts, the second on a side stream of its own.  HIP deals streams to
    four hardware queues; the library checks once per caller stream that its side stream runs beside it and takes another one
    otherwise (qpx_hip_api.hip: runs_beside; profiles/r05p_stream_clash.txt).  Here: the same batch on torch's default stream and
    on streams created after several others had been used -- identical results whichever side stream was picked."""
    from qpth_amd.kkt import KKTFactors
    B, n, m = 96, 260, 260
    Q, p, G, h, A, b = to_dev(problems.prof_qp(B, n, m, 0, seed=23), dev, grad=False)

    def run():
        fac = KKTFactors.build(Q, G, A)
        res = fac.ipm(p, h, b)
        return res.zhat.clone(), res.lam.clone(), res.iters.clone()

    want = run()
    torch.cuda.synchronize()
    others = []
    for k in range(7):
        st = torch.cuda.Stream(dev)
        with torch.cuda.stream(st):
            torch.zeros(1024, device=dev).add_(1.0)
        others.append(st)
        caller = torch.cuda.Stream(dev)
        caller.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(caller):
            got = run()
        caller.synchronize()
        for g, w in zip(got, want):
            assert torch.equal(g, w), k
    assert int(want[2].max().item()) > 0
