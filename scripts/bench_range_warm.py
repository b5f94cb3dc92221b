#!/usr/bin/env python3
"""What the warm start of the range role buys (qpx_ipm_range_warm): the loop launch of two-sided rows (the library
call behind KKTFactors.ipm_range, on outputs allocated once) cold and warm, one process, HIP events, alternating rounds of
`reps` launches, medians -- the protocol of scripts/bench_warm.py.

Shapes: the box of scripts/bench_range.py (B = 512, nz = nineq = 100, G = I, every variable two-sided) and (100, 50, 10) with
every row two-sided (lower = h - 1 - rand, as bench_range's loop case).  The base problem is solved cold; the problem timed is
p + delta randn, h + delta rand, lower - delta rand (RandomState(7), drawn in that order) for delta in 0, 1e-3, 1e-2, 1e-1,
cold and from the base problem's (lam, slacks, lam_lo, slacks_lo).  Per cell: cold and warm ms, mean and max `iters` of both,
the number of QPs whose status word carries a failure bit (QPX_ST_KKT_BREAKDOWN | QPX_ST_INACCURATE | QPX_ST_NONFINITE) and of those that ended
above best_resid = 1e-6 -- a warm start far from the solution may stall (Limits): no cell is gated.

--parent PATH (libqpx_hip.so of the parent commit, loaded non-strictly): the cost of the change on the COLD path -- qpx_ipm_range
of the parent and of this build in alternating rounds on the same inputs, the parent's own max - min as the yardstick, and
whether the outputs are bit-identical.

    python scripts/bench_range_warm.py [--shapes box,C3] [--parent PATH] [--reps 20] [--rounds 5] [--out profiles/range_warm.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import problems  # noqa: E402
from bench_range import B, box, timed  # noqa: E402
from qpth_amd import _lib  # noqa: E402
from qpth_amd.kkt import KKTFactors, default_stall_policy  # noqa: E402

DELTAS = (0.0, 1e-3, 1e-2, 1e-1)
FLOOR = 1e-2
FAIL_BITS = _lib.ST_KKT_BREAKDOWN | _lib.ST_INACCURATE | _lib.ST_NONFINITE      # (QPX_ST_MAXITER is no failure at eps = 1e-12)


def c3():
    Q, p, G, h, A, b = problems.prof_qp(B, 100, 50, 10, 0)
    return Q, p, G, h, A, b, h - 1.0 - np.random.RandomState(2).rand(B, 50)             # h = G z0 + s0, s0 < 1: z0 stays inside


SHAPES = {"box": lambda: box(100), "C3": c3}


def perturbed(arrs, delta):
    Q, p, G, h, A, b, lower = arrs
    r = np.random.RandomState(7)
    p2 = p + delta * r.randn(*p.shape)
    h2 = h + delta * r.rand(*h.shape)
    return Q, p2, G, h2, A, b, lower - delta * r.rand(*lower.shape)


class Launch:
    """the range loop launch on factors of `arrs`, outputs allocated once; lib: the library the factors are built with"""

    def __init__(self, arrs, dev, lib=None):
        Q, self.p, G, self.h, A, self.b, self.lower = [torch.tensor(np.asarray(x), device=dev) if np.size(x) else None for x in arrs]
        self.B, self.m, self.n = G.shape
        self.q = A.shape[1] if A is not None else 0
        _lib.set_test_backend(lib)                 # (None: the product library)
        try:
            self.fac = KKTFactors.build(Q, G, A, self.B)
        finally:
            _lib.set_test_backend(None)
        new = lambda *s: torch.empty(*s, dtype=Q.dtype, device=dev)      # noqa: E731
        Bq, n, m, q = self.B, self.n, self.m, self.q
        self.zhat, self.nu, self.best = new(Bq, n), new(Bq, q) if q else None, new(Bq)
        self.sides = [new(Bq, m) for _ in range(4)]                      # lam, slacks, lam_lo, slacks_lo
        self.iters = torch.empty(Bq, dtype=torch.int32, device=dev)
        self.used = torch.empty(Bq, dtype=torch.int32, device=dev)
        self.status0 = self.fac.status.clone()
        self.status = self.status0.clone()
        self.gt1 = self.fac.gt1_of(self.lower, self.h)

    def __call__(self, warm=None):
        f = self.fac
        lam, slacks, lam_lo, slacks_lo = self.sides
        kw = dict(warm=warm, warm_floor=FLOOR, warm_used=self.used) if warm is not None else {}
        f.lib.ipm_range(self.B, self.n, self.m, self.q, self.p, self.h, self.lower, self.gt1, self.b, f.blob, f.sfac, 1e-12, 20, 3,
                        default_stall_policy(self.B), self.zhat, self.nu, lam, slacks, lam_lo, slacks_lo, self.iters, self.status,
                        self.best, **kw)

    def report(self, warm=None):
        """one launch on fresh status words: (mean iters, max iters, QPs with a failure bit, QPs above best_resid 1e-6, outputs)"""
        self.status.copy_(self.status0)
        self(warm)
        torch.cuda.synchronize()
        it = self.iters.cpu().numpy()
        failed = int(((self.status & FAIL_BITS) != 0).sum().item())
        above = int((~(self.best <= 1e-6)).sum().item())
        outs = [x.clone() for x in [self.zhat, self.nu] + self.sides if x is not None]
        return float(it.mean()), int(it.max()), failed, above, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--parent", default=None, help="libqpx_hip.so of the parent commit (optional): the cold path's cost")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    parent = _lib.QpxLib(os.path.abspath(args.parent), strict=False) if args.parent else None
    rows = []
    for name in args.shapes.split(","):
        base = SHAPES[name]()
        solve = Launch(base, dev)
        solve()
        torch.cuda.synchronize()
        warm = [x.clone() for x in solve.sides]
        if parent is not None:
            mine, par = Launch(base, dev), Launch(base, dev, lib=parent)
            same = all(torch.equal(x, y) for x, y in zip(mine.report()[4], par.report()[4])) and torch.equal(mine.iters, par.iters)
            t = {"parent": [], "this": []}
            for _ in range(args.rounds):
                t["parent"].append(timed(par, args.reps))
                t["this"].append(timed(mine, args.reps))
            med = {k: statistics.median(v) for k, v in t.items()}
            spread = max(t["parent"]) - min(t["parent"])
            row = {"shape": name, "what": "cold path, qpx_ipm_range: parent build / this build", "parent_ms": round(med["parent"], 5),
                   "this_ms": round(med["this"], 5), "parent_spread_ms": round(spread, 5),
                   "this_minus_parent_ms": round(med["this"] - med["parent"], 5),
                   "this_within_parent_spread": bool(med["this"] - med["parent"] <= spread), "bit_identical": bool(same),
                   "rounds": {k: [round(x, 5) for x in v] for k, v in t.items()}}
            rows.append(row)
            print(json.dumps(row), flush=True)
        for delta in DELTAS:
            run = Launch(perturbed(base, delta), dev)
            c_mean, c_max, c_fail, c_above, cold_out = run.report()
            w_mean, w_max, w_fail, w_above, warm_out = run.report(warm)
            used = int(run.used.sum().item())
            gap = float(((warm_out[0] - cold_out[0]).norm(dim=1) / cold_out[0].norm(dim=1)).max())
            t = {"cold": [], "warm": []}
            for _ in range(args.rounds):
                t["cold"].append(timed(run, args.reps))
                t["warm"].append(timed(lambda: run(warm), args.reps))
            med = {k: statistics.median(v) for k, v in t.items()}
            row = {"shape": name, "B": run.B, "nz": run.n, "nineq": run.m, "neq": run.q, "delta": delta, "floor": FLOOR,
                   "cold_ms": round(med["cold"], 5), "warm_ms": round(med["warm"], 5), "warm_over_cold": round(med["warm"] / med["cold"], 4),
                   "cold_iters_mean": round(c_mean, 3), "cold_iters_max": c_max, "warm_iters_mean": round(w_mean, 3), "warm_iters_max": w_max,
                   "cold_failed": c_fail, "warm_failed": w_fail, "cold_above_1e-6": c_above, "warm_above_1e-6": w_above,
                   "warm_used": used, "zhat_warm_vs_cold_max_rel": gap, "rounds": {k: [round(x, 5) for x in v] for k, v in t.items()}}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev), "reps": args.reps, "rounds": args.rounds, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
