#!/usr/bin/env python3
"""What the second-order pass of the backward costs (qpx_backward2): one process, HIP events, alternating rounds,
at C2 (B = 512, nz = nineq = 100), C3 (512, 100 / 50 / 10) and B = 4096 at 64 / 64, on prof_qp(seed 0), float64:

  (a) the first-order backward alone (KKTFactors.backward, all six gradients);
  (b) the COMPOSED second-order pass, built from the entry points the parent has (KKTFactors.backward2(fused=False): qpx_jvp,
      the torch glue, qpx_backward_duals);
  (c) the fused entry (KKTFactors.backward2(fused=True): qpx_backward2, one launch, one factorisation).

Per shape: ms of each (median over the rounds, every round kept), the spread between the rounds of (a) (max - min), and
whether (c) is no slower than (b) beyond that spread.

--parent PATH (libqpx_hip.so of the parent commit, loaded non-strictly as scripts/bench_warm.py does): the cost of the change
on the FIRST-ORDER path -- (a) with the parent's library and with this build in alternating rounds on the same inputs, the
parent's own spread as the yardstick, and whether the gradients are bit-identical.

    python scripts/bench_backward2.py [--shapes C2,C3,B4096_64_64] [--parent PATH] [--reps 20] [--rounds 5] [--out profiles/backward2.json]
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
from qpth_amd.kkt import KKTFactors  # noqa: E402

SHAPES = {"C2": (512, 100, 100, 0), "C3": (512, 100, 50, 10), "B4096_64_64": (4096, 64, 64, 0)}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


class Solved:
    """factors, solution, a cotangent v and the first backward's solution of a shape; lib: the library the factors are built with"""

    def __init__(self, arrs, shape, dev, lib=None):
        B, n, m, q = shape
        Q, p, G, h, A, b = [torch.tensor(x, device=dev) for x in arrs]
        _lib.set_test_backend(lib)                 # (None: the product library)
        try:
            self.fac = KKTFactors.build(Q, G, A if q else None, B)
            self.r = self.fac.ipm(p, h, b if q else None)
        finally:
            _lib.set_test_backend(None)
        self.v = torch.tensor(np.random.RandomState(5).randn(B, n), device=dev)

    def backward(self, **kw):
        r = self.r
        return self.fac.backward(r.zhat, r.lam, r.slacks, r.nu, self.v, **kw)

    def backward2(self, sol, W, fused):
        r = self.r
        return self.fac.backward2(r.zhat, r.lam, r.slacks, r.nu, sol, W, fused=fused)


def rounds_of(fns, reps, rounds):
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, reps))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--parent", default=None, help="libqpx_hip.so of the parent commit (optional): the first-order path's cost")
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
        arrs = problems.prof_qp(B, n, m, q, 0)
        s = Solved(arrs, shape, dev)
        r = np.random.RandomState(9)
        W = [torch.tensor(r.randn(*sh), device=dev) if np.prod(sh) else None
             for sh in ((B, n, n), (B, n), (B, m, n), (B, m), (B, q, n), (B, q))]
        sol = s.backward(want_sol=True)[-1]
        assert s.fac.backward2_fused()
        f, c = s.backward2(sol, W, True), s.backward2(sol, W, False)
        gap = max(float(((a - e).flatten(1).norm(dim=1) / e.flatten(1).norm(dim=1)).max()) for a, e in zip(f[0] + f[1], c[0] + c[1]) if a is not None)
        t = rounds_of({"backward": s.backward, "composed": lambda: s.backward2(sol, W, False), "fused": lambda: s.backward2(sol, W, True)},
                      args.reps, args.rounds)
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = max(t["backward"]) - min(t["backward"])
        row = {"shape": name, "B": B, "nz": n, "nineq": m, "neq": q, "backward_ms": round(med["backward"], 5),
               "composed_ms": round(med["composed"], 5), "fused_ms": round(med["fused"], 5), "backward_spread_ms": round(spread, 5),
               "fused_over_composed": round(med["fused"] / med["composed"], 4),
               "fused_no_slower_than_composed": bool(med["fused"] - med["composed"] <= spread),
               "fused_vs_composed_max_rel": gap, "rounds": {k: [round(x, 5) for x in v] for k, v in t.items()}}
        rows.append(row)
        print(json.dumps(row), flush=True)
        if parent is not None:
            par = Solved(arrs, shape, dev, lib=parent)
            same = all(torch.equal(x, y) for x, y in zip(s.backward(), par.backward()) if x is not None)
            t = rounds_of({"parent": par.backward, "this": s.backward}, args.reps, args.rounds)
            med = {k: statistics.median(v) for k, v in t.items()}
            spread = max(t["parent"]) - min(t["parent"])
            row = {"shape": name, "what": "first-order backward: parent build / this build", "parent_ms": round(med["parent"], 5),
                   "this_ms": round(med["this"], 5), "parent_spread_ms": round(spread, 5),
                   "this_minus_parent_ms": round(med["this"] - med["parent"], 5),
                   "this_within_parent_spread": bool(med["this"] - med["parent"] <= spread), "bit_identical": bool(same),
                   "rounds": {k: [round(x, 5) for x in v] for k, v in t.items()}}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        old = []
        if os.path.exists(args.out):
            with open(args.out) as fh:
                old = json.load(fh).get("rows", [])
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(dev), "reps": args.reps, "rounds": args.rounds, "rows": old + rows}, fh, indent=1)


if __name__ == "__main__":
    main()
