#!/usr/bin/env python3
"""What n vector-Jacobian products at one solution cost, one process, HIP events: qpx_factor_solve_kkt_multi with K = nz
right-hand sides per QP (one launch, one factorisation) against K launches of qpx_backward asking only for dp, dh, db -- the
way to the same numbers without it -- at C2 (B = 512, nz = nineq = 100), B = 4096 at 64 / 64 and C3 (512, 100 / 50 / 10).

What is timed is the library call itself (ctypes marshalling + the launch) on outputs allocated once.  The K backward
launches are timed twice: enqueued back to back from the host (`loop_ms`), and captured once into a HIP graph -- a plain
chain, no parallel branches -- and replayed (`graph_ms`: no host time between the launches).  The ratio printed is against
the FASTER of the two.  Before timing, dx, dz, dy of the one launch are compared with dp, -dh, -db of the K launches.

    python scripts/bench_multi.py [--reps 5] [--rounds 3] [--out profiles/multi_rhs.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import problems  # noqa: E402
from qpth_amd.kkt import MULTI_RHS_BLOCK, KKTFactors  # noqa: E402

SHAPES = (("C2", 512, 100, 100, 0), ("B4096_64_64", 4096, 64, 64, 0), ("C3", 512, 100, 50, 10))


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for name, B, n, m, q in SHAPES:
        Q, p, G, h, A, b = [torch.tensor(x, device=dev) for x in problems.prof_qp(B, n, m, q, 0)]
        fac = KKTFactors.build(Q, G, A if q else None, B)
        r = fac.ipm(p, h, b)
        nu = r.nu if q else None
        K = n
        V = torch.eye(n, dtype=Q.dtype, device=dev).expand(B, n, n).contiguous()             # the cotangents of a Jacobian
        d = torch.clamp(r.lam, min=1e-8) / torch.clamp(r.slacks, min=1e-8)
        dx, dz = torch.empty(B, K, n, dtype=Q.dtype, device=dev), torch.empty(B, K, m, dtype=Q.dtype, device=dev)
        dy = torch.empty(B, K, q, dtype=Q.dtype, device=dev) if q else None
        dp, dh = torch.empty(K, B, n, dtype=Q.dtype, device=dev), torch.empty(K, B, m, dtype=Q.dtype, device=dev)
        db = torch.empty(K, B, q, dtype=Q.dtype, device=dev) if q else None
        gz = V.transpose(0, 1).contiguous()                                                    # (K, B, n): launch k's dl_dz

        def multi():
            fac.lib.factor_solve_kkt_multi(B, n, m, q, K, fac.blob, fac.sfac, d, V, None, None, None, dx, None, dz, dy, fac.status)

        def launches():
            for k in range(K):
                fac.lib.backward(B, n, m, q, fac.blob, fac.sfac, r.zhat, r.lam, r.slacks, nu, gz[k], None, dp[k], None, dh[k],
                                 None, db[k] if q else None, fac.status)

        multi()
        launches()
        torch.cuda.synchronize()
        err = max(float((dx.transpose(0, 1) - dp).norm() / dp.norm()), float((dz.transpose(0, 1) + dh).norm() / dh.norm()),
                  float((dy.transpose(0, 1) + db).norm() / db.norm()) if q else 0.0)
        assert err < 1e-8, err
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launches()                                                                         # warm-up on the capture stream
            with torch.cuda.graph(graph, stream=side):
                launches()
        torch.cuda.current_stream().wait_stream(side)
        graph.replay()
        torch.cuda.synchronize()
        t = {"multi_ms": [], "loop_ms": [], "graph_ms": []}
        for _ in range(args.rounds):                                                           # alternating rounds
            t["multi_ms"].append(timed(multi, args.reps))
            t["loop_ms"].append(timed(launches, args.reps))
            t["graph_ms"].append(timed(graph.replay, args.reps))
        med = {k: statistics.median(v) for k, v in t.items()}
        row = {"shape": name, "B": B, "nz": n, "nineq": m, "neq": q, "K": K, "rb": MULTI_RHS_BLOCK, "max_rel_diff": err,
               **{k: round(v, 4) for k, v in med.items()}, "rounds": {k: [round(x, 4) for x in v] for k, v in t.items()},
               "speedup": round(min(med["loop_ms"], med["graph_ms"]) / med["multi_ms"], 2)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
