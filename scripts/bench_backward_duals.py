#!/usr/bin/env python3
"""What the dual cotangents of the backward cost, one process, HIP events: the backward launch (every gradient wanted) at C2
(B = 512, nz = nineq = 100), C3 (512, 100 / 50 / 10) and B = 4096 at 64 / 64

  parent ........ qpx_backward of a PARENT build of the library (--parent <libqpx_hip.so of the commit before
                  qpx_backward_duals>; loaded non-strictly, as scripts/ab_bench.py does) -- same box, same process
  null .......... qpx_backward of this build: dl_dlam = dl_dnu = NULL, what every caller of QPFunction(duals=False) runs
  duals ......... qpx_backward_duals with dl_dz, dl_dlam and dl_dnu all present

timed in alternating rounds of `reps` calls.  What is timed is the library call itself (QpxLib.backward: ctypes marshalling + the
launch) on outputs allocated once -- no tensor allocation, no argument checks of KKTFactors in the interval.  Each is also
timed one launch at a time between two events with the device idle before it (`*_single_ms`, the median of `reps`): that
figure holds no host time at all, so a back-to-back figure close to it shows that the device, not the host, bounded the
rounds.  Per shape: every round, the median, and the parent's own spread (max - min
over its rounds) -- the yardstick for "null is no slower than the parent": boxes differ by ~6 %, so only this same-box A/B
counts.

    python scripts/bench_backward_duals.py [--parent PATH] [--reps 50] [--rounds 5] [--out profiles/backward_duals.json]
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
from qpth_amd import _lib  # noqa: E402
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
    ap.add_argument("--parent", default=None, help="libqpx_hip.so of the parent commit (optional)")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    parent = _lib.QpxLib(os.path.abspath(args.parent), strict=False) if args.parent else None
    rows = []
    for name, B, n, m, q in SHAPES:
        Q, p, G, h, A, b = [torch.tensor(x, device=dev) for x in problems.prof_qp(B, n, m, q, 0)]
        gen = torch.Generator(device=dev).manual_seed(1)
        gz, gl, gn = [torch.randn(B, k, generator=gen, dtype=Q.dtype, device=dev) for k in (n, m, q)]

        def prepare(lib):
            """factors and solution under `lib` (None: the product library) and the backward launch on them"""
            _lib.set_test_backend(lib)
            try:
                fac = KKTFactors.build(Q, G, A if q else None, B)
                r = fac.ipm(p, h, b)
            finally:
                _lib.set_test_backend(None)
            return fac, r

        def launcher(fac, r, **duals):
            """the raw library call on outputs allocated once (dQ, dp, dG, dh, dA, db)"""
            outs = [torch.empty(B, *s, dtype=Q.dtype, device=dev) if all(s) else None
                    for s in ((n, n), (n,), (m, n), (m,), (q, n), (q,))]
            nu = r.nu if q else None

            def go():
                fac.lib.backward(B, n, m, q, fac.blob, fac.sfac, r.zhat, r.lam, r.slacks, nu, gz, *outs, fac.status, **duals)
            return go, outs

        fac, r = prepare(None)
        null, null_outs = launcher(fac, r)
        duals, _ = launcher(fac, r, dl_dlam=gl, dl_dnu=gn if q else None)
        runs = {"null": null, "duals": duals}
        if parent is not None:
            pfac, pr = prepare(parent)                       # (KKTFactors remembers the library it was built with)
            par, par_outs = launcher(pfac, pr)
            runs = {"parent": par, **runs}
            par()
            null()
            same = all(torch.equal(x, y) for x, y in zip(par_outs, null_outs) if x is not None)
        for fn in runs.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                t[k].append(timed(fn, args.reps))
        row = {"shape": name, "B": B, "nz": n, "nineq": m, "neq": q}
        for k, v in t.items():
            row[k + "_ms"] = round(statistics.median(v), 5)
            row[k + "_rounds_ms"] = [round(x, 5) for x in v]
            # one launch at a time, the device idle before and waited for after: events around the launch alone
            single = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                single.append(timed(runs[k], 1))
            row[k + "_single_ms"] = round(statistics.median(single), 5)
        row["duals_over_null"] = round(row["duals_ms"] / row["null_ms"], 4)
        if parent is not None:
            spread = max(t["parent"]) - min(t["parent"])
            row["parent_spread_ms"] = round(spread, 5)
            row["null_minus_parent_ms"] = round(row["null_ms"] - row["parent_ms"], 5)
            row["null_over_parent"] = round(row["null_ms"] / row["parent_ms"], 4)
            row["null_within_parent_spread"] = bool(row["null_ms"] - row["parent_ms"] <= spread)
            row["null_bit_identical_to_parent"] = bool(same)
        rows.append(row)
        print("%-12s " % name + "  ".join("%s %.4f ms (single %.4f)" % (k, row[k + "_ms"], row[k + "_single_ms"]) for k in t)
              + ("  parent spread %.4f ms  null bit-identical %s" % (row["parent_spread_ms"], same) if parent is not None else ""),
              flush=True)
    out = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "rounds": args.rounds, "rows": rows}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
