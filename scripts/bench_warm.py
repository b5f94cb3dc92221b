#!/usr/bin/env python3
"""What the warm start of the PDIPM loop buys (qpx_ipm_warm): the loop launch (the library call behind
KKTFactors.ipm, on outputs allocated once) cold and warm, one process, HIP events, alternating rounds, at C2 (B = 512,
nz = nineq = 100), C3 (512, 100 / 50 / 10) and B = 4096 at 64 / 64.

The base problem is prof_qp(seed 0), solved cold; the problem timed is p + delta randn, h + delta rand (RandomState(7), p
first) for delta in 0, 1e-3, 1e-2, 1e-1, cold and from the base problem's (lam, slacks).  Per shape and delta: ms of both
(median over the rounds, every round kept), mean and max `iters` of both, and the ratio to hold the time against:
(warm passes) / (cold passes + 1) -- the cold start pays pass -1, one factorisation and one solve, on top of its iterations;
at B = 512 (two QPs per CU) the slowest QP bounds the launch, so the ratio of the MAX iters is given beside that of the means.

--parent PATH (libqpx_hip.so of the parent commit, loaded non-strictly as scripts/bench_backward_duals.py does): the cost
of the change on the COLD path -- qpx_ipm of the parent and of this build in alternating rounds on the same inputs, the
parent's own spread (max - min over its rounds) as the yardstick, and whether the outputs are bit-identical.

    python scripts/bench_warm.py [--shapes C2,C3,B4096_64_64] [--parent PATH] [--reps 20] [--rounds 5] [--out profiles/warm_start.json]
(a job script gives each shape a call of its own under `timeout`; --out appends to the rows of an existing file)
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
import problems  # noqa: E402
from qpth_amd import _lib  # noqa: E402
from qpth_amd.kkt import KKTFactors, default_stall_policy  # noqa: E402

SHAPES = {"C2": (512, 100, 100, 0), "C3": (512, 100, 50, 10), "B4096_64_64": (4096, 64, 64, 0)}
DELTAS = (0.0, 1e-3, 1e-2, 1e-1)
FLOOR = 1e-2


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def perturbed(arrs, delta):
    Q, p, G, h, A, b = arrs
    r = np.random.RandomState(7)
    return Q, p + delta * r.randn(*p.shape), G, h + delta * r.rand(*h.shape), A, b


class Launch:
    """the loop launch on factors of `arrs`, outputs allocated once; lib: the library the factors are built with"""

    def __init__(self, arrs, shape, dev, lib=None):
        B, n, m, q = shape
        self.shape = shape
        Q, self.p, G, self.h, A, self.b = [torch.tensor(x, device=dev) for x in arrs]
        _lib.set_test_backend(lib)                 # (None: the product library)
        try:
            self.fac = KKTFactors.build(Q, G, A if q else None, B)
        finally:
            _lib.set_test_backend(None)
        dt = Q.dtype
        self.out = [torch.empty(B, n, dtype=dt, device=dev), torch.empty(B, q, dtype=dt, device=dev) if q else None,
                    torch.empty(B, m, dtype=dt, device=dev), torch.empty(B, m, dtype=dt, device=dev),
                    torch.empty(B, dtype=torch.int32, device=dev)]
        self.best = torch.empty(B, dtype=dt, device=dev)
        self.used = torch.empty(B, dtype=torch.int32, device=dev)

    def __call__(self, warm=None):
        B, n, m, q = self.shape
        f = self.fac
        kw = dict(lam0=warm[0], s0=warm[1], warm_floor=FLOOR, warm_used=self.used) if warm is not None else {}
        f.lib.ipm(B, n, m, q, self.p, self.h, self.b if q else None, f.blob, f.sfac, 1e-12, 20, 3, default_stall_policy(B),
                  *self.out, f.status, self.best, **kw)

    def iters(self):
        torch.cuda.synchronize()
        it = self.out[4].cpu().numpy()
        return float(it.mean()), int(it.max())

    def outputs(self):
        torch.cuda.synchronize()
        return [x.clone() for x in self.out if x is not None]


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
        shape = SHAPES[name]
        B, n, m, q = shape
        base = problems.prof_qp(B, n, m, q, 0)
        solve = Launch(base, shape, dev)
        solve()
        lam0, s0 = solve.outputs()[-3:-1]
        if parent is not None:
            mine, par = Launch(base, shape, dev), Launch(base, shape, dev, lib=parent)
            mine(), par()
            same = all(torch.equal(x, y) for x, y in zip(mine.outputs(), par.outputs()))
            t = {"parent": [], "this": []}
            for _ in range(args.rounds):
                t["parent"].append(timed(par, args.reps))
                t["this"].append(timed(mine, args.reps))
            med = {k: statistics.median(v) for k, v in t.items()}
            spread = max(t["parent"]) - min(t["parent"])
            row = {"shape": name, "what": "cold path, qpx_ipm: parent build / this build", "parent_ms": round(med["parent"], 5),
                   "this_ms": round(med["this"], 5), "parent_spread_ms": round(spread, 5),
                   "this_minus_parent_ms": round(med["this"] - med["parent"], 5),
                   "this_within_parent_spread": bool(med["this"] - med["parent"] <= spread), "bit_identical": bool(same),
                   "rounds": {k: [round(x, 5) for x in v] for k, v in t.items()}}
            rows.append(row)
            print(json.dumps(row), flush=True)
        for delta in DELTAS:
            run = Launch(perturbed(base, delta), shape, dev)
            run()
            cold_out, cold_it = run.outputs(), run.iters()
            run(warm=(lam0, s0))
            warm_out, warm_it = run.outputs(), run.iters()
            assert bool((run.used == 1).all())
            gap = float(((warm_out[0] - cold_out[0]).norm(dim=1) / cold_out[0].norm(dim=1)).max())
            t = {"cold": [], "warm": []}
            for _ in range(args.rounds):
                t["cold"].append(timed(run, args.reps))
                t["warm"].append(timed(lambda: run(warm=(lam0, s0)), args.reps))
            med = {k: statistics.median(v) for k, v in t.items()}
            row = {"shape": name, "B": B, "nz": n, "nineq": m, "neq": q, "delta": delta, "floor": FLOOR,
                   "cold_ms": round(med["cold"], 5), "warm_ms": round(med["warm"], 5), "warm_over_cold": round(med["warm"] / med["cold"], 4),
                   "cold_iters_mean": round(cold_it[0], 3), "cold_iters_max": cold_it[1],
                   "warm_iters_mean": round(warm_it[0], 3), "warm_iters_max": warm_it[1],
                   "passes_ratio_mean": round(warm_it[0] / (cold_it[0] + 1), 4), "passes_ratio_max": round(warm_it[1] / (cold_it[1] + 1), 4),
                   "zhat_warm_vs_cold_max_rel": gap, "rounds": {k: [round(x, 5) for x in v] for k, v in t.items()}}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        old = []
        if os.path.exists(args.out):
            with open(args.out) as f:
                old = json.load(f).get("rows", [])
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev), "reps": args.reps, "rounds": args.rounds, "rows": old + rows}, f, indent=1)


if __name__ == "__main__":
    main()
