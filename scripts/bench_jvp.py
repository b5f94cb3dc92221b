#!/usr/bin/env python3
"""Forward mode against reverse mode, one process, HIP events: the JVP launch (qpx_jvp: every tangent Q', p', G', h', A', b'
given, z' out) against the backward launch (qpx_backward: every gradient wanted) on the same factors and solution, at C2
(B = 512, nz = nineq = 100), C3 (512, 100 / 50 / 10) and B = 4096 at 64 / 64 (the one-wave tile form).  Both launches are
timed in alternating rounds of `reps` calls; the median round is reported.

    python scripts/bench_jvp.py [--reps 50] [--rounds 7] [--out profiles/jvp_vs_backward.json]
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
from qpth_amd.kkt import KKTFactors  # noqa: E402

SHAPES = (("C2", 512, 100, 100, 0), ("C3", 512, 100, 50, 10), ("B4096_64_64", 4096, 64, 64, 0))


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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for name, B, n, m, q in SHAPES:
        Q, p, G, h, A, b = [torch.tensor(x, device=dev) for x in problems.prof_qp(B, n, m, q, 0)]
        fac = KKTFactors.build(Q, G, A if q else None, B)
        r = fac.ipm(p, h, b)
        gen = torch.Generator(device=dev).manual_seed(1)
        tans = tuple(torch.randn(x.shape, generator=gen, dtype=x.dtype, device=dev) if x.nelement() else None
                     for x in (Q, p, G, h, A, b))
        ones = torch.ones(B, n, dtype=Q.dtype, device=dev)
        want = (True,) * 6

        def jvp():
            fac.jvp(r.zhat, r.lam, r.slacks, r.nu, tans)

        def bwd():
            fac.backward(r.zhat, r.lam, r.slacks, r.nu, ones, want=want)

        for _ in range(5):
            jvp()
            bwd()
        torch.cuda.synchronize()
        tj, tb = [], []
        for _ in range(args.rounds):
            tj.append(timed(jvp, args.reps))
            tb.append(timed(bwd, args.reps))
        j, w = statistics.median(tj), statistics.median(tb)
        row = {"shape": name, "B": B, "nz": n, "nineq": m, "neq": q, "jvp_ms": round(j, 5), "backward_ms": round(w, 5),
               "ratio": round(j / w, 3), "jvp_rounds_ms": [round(x, 5) for x in tj],
               "backward_rounds_ms": [round(x, 5) for x in tb]}
        rows.append(row)
        print("%-12s B=%5d n=%3d m=%3d q=%2d  jvp %.4f ms  backward %.4f ms  ratio %.3f" % (name, B, n, m, q, j, w, j / w),
              flush=True)
    out = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "rounds": args.rounds, "rows": rows}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
