#!/usr/bin/env python3
"""What the barrier-smoothed forward costs (qpx_centre): one process, HIP events, float64, prof_qp(seed 0) at
B = 512, nz = nineq = 100, kappa = 1e-3.

  GATE   the time of a qpx_centre launch per Newton step must not exceed the time of qpx_polish(steps=k, refine=0) per step
         by more than 5 % (tests/test_gpu_centre.py: step_times -- k steps each on the same factors and start iterate,
         alternating rounds, medians).  --parent PATH times the qpx_polish of the PARENT commit's libqpx_hip.so (loaded
         non-strictly, as scripts/bench_backward2.py does) beside this build's.
  RECORD the loop launch at eps = nineq * kappa against the default eps = 1e-12 (time and iterations), the centring launch
         as QPFunction runs it (time and Newton steps), and the hard forward for scale; the worst centring step count over
         the shapes and kappas of tests/test_gpu_centre.py (--steps: runs that file's forward cases).

    python scripts/bench_centre.py [--parent PATH] [--steps] [--out profiles/centre.json]
The exit status is 1 when the gate is missed."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import centre_checks as C  # noqa: E402
import problems  # noqa: E402
import test_gpu_centre as T  # noqa: E402
from qpth_amd import _lib  # noqa: E402
from qpth_amd.kkt import KKTFactors  # noqa: E402


def timed(fn, reps=10):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, n, m, kappa = 512, 100, 100, 1e-3
    out = {"device": torch.cuda.get_device_name(dev), "shape": {"B": B, "nz": n, "nineq": m, "neq": 0}, "kappa": kappa}
    c, p, rounds = T.step_times(dev, B, n, m, kappa)
    out["gate"] = {"centre_ms_per_step": round(c, 5), "polish_ms_per_step": round(p, 5), "ratio": round(c / p, 4), "limit": 1.05,
                   "met": bool(c <= 1.05 * p), "rounds": {k: [round(x, 5) for x in v] for k, v in rounds.items()}}
    if args.parent:
        parent = _lib.QpxLib(os.path.abspath(args.parent), strict=False)
        c2, p2, rounds = T.step_times(dev, B, n, m, kappa, polish_lib=parent)
        out["gate_parent_library"] = {"centre_ms_per_step": round(c2, 5), "parent_polish_ms_per_step": round(p2, 5), "ratio": round(c2 / p2, 4),
                                      "met": bool(c2 <= 1.05 * p2), "rounds": {k: [round(x, 5) for x in v] for k, v in rounds.items()}}
    # the record: the launches of the smoothed and of the hard forward
    Q, pp, G, h, A, b = C.on(problems.prof_qp(B, n, m, 0, seed=0), dev)
    fac = KKTFactors.build(Q, G, A, nBatch=B)
    kap = torch.full((m,), kappa, dtype=torch.float64, device=dev)
    rec = {}
    for name, eps in (("loop_eps_default", 1e-12), ("loop_eps_nineq_kappa", m * kappa)):
        r = fac.ipm(pp, h, b, eps)
        rec[name] = {"eps": eps, "ms": round(timed(lambda: fac.ipm(pp, h, b, eps)), 5),
                     "iterations_mean": round(float(r.iters.double().mean()), 3), "iterations_max": int(r.iters.max())}
    r = fac.ipm(pp, h, b, m * kappa)
    start = [x.clone() for x in (r.zhat, r.lam, r.slacks)]

    def centre():
        for x, s in zip((r.zhat, r.lam, r.slacks), start):
            x.copy_(s)
        fac.centre(pp, h, b, r, kap, tol=C.KAPPA_TOL, max_steps=C.KAPPA_STEPS)

    def copies():
        for x, s in zip((r.zhat, r.lam, r.slacks), start):
            x.copy_(s)

    t = timed(centre) - timed(copies)
    rec["centre_launch"] = {"tol": C.KAPPA_TOL, "ms": round(t, 5), "steps_mean": round(float(r.centre_steps.double().mean()), 3),
                            "steps_max": int(r.centre_steps.max()), "resid_max": float(r.centre_resid.max())}
    rec["smoothed_loop_plus_centre_ms"] = round(rec["loop_eps_nineq_kappa"]["ms"] + t, 5)
    rec["hard_loop_ms"] = rec["loop_eps_default"]["ms"]
    out["record"] = rec
    if args.steps:
        env = T.Env(dev)
        for shape, variant, kind in T.FORWARD:
            C.forward(env, shape, 1, kind, variant)
        out["centre_steps"] = {"cap": C.KAPPA_STEPS, "worst": int(C.measured["centre_steps worst"]),
                               "per_case": {k[len("centre_steps "):]: int(v) for k, v in C.measured.items()
                                            if k.startswith("centre_steps ") and k != "centre_steps worst"}}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0 if out["gate"]["met"] else 1


if __name__ == "__main__":
    sys.exit(main())
