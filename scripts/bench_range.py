#!/usr/bin/env python3
"""What two-sided rows cost and save (QPFunction(...)(Q, p, G, h, A, b, lower=l), qpx_ipm_range), one MI355X, float64,
one process, HIP events, medians of alternating rounds:

  the headline case ... B = 512, nz = nineq = 100, G = I: the box on all variables, fwd+bwd through QPFunction,
      range ......... lower=l: 100 rows, the seven-row chain-wave loop and backward
      doubled ....... what a caller had to write before: [I; -I] z <= [h; -l], 200 rows, nz + nineq = 300 > 208 -- the
                      large-QP family
      one_sided ..... the six-input call on the upper bounds alone (another QP: the cost of the 100-row kernels without the
                      range role's vector work, iteration counts differ)
  the loop alone ...... KKTFactors.ipm_range against KKTFactors.ipm on the same factors, (n, m, q) of the headline, of C3
      (100, 50, 10) and of (20, 170, 2), every row two-sided, per IPM iteration (launch time / mean iteration count)

and every figure tests/range_checks.py prints and asserts on (tests/test_gpu_range.py), measured on this device.

--headline FILE: a JSON {"parent": [...], "this": [...]} of bench.py's headline QPs/s, three runs of the parent build and
three of this one, alternating on the same box (a job script runs bench.py in both trees and writes the file); recorded with
the rule "this build's median lies inside the parent's min-max spread".  Exits non-zero when the range call is not faster
than the doubled-row call at the headline box.

    python scripts/bench_range.py [--reps 10] [--rounds 5] [--headline FILE] [--out profiles/range.json]
"""
import argparse
import contextlib
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
from qpth_amd.kkt import KKTFactors  # noqa: E402
from qpth_amd.qp import QPFunction  # noqa: E402

B = 512


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def on(arrs, dev):
    return [torch.tensor(np.asarray(x), device=dev) if np.size(x) else torch.empty(0, dtype=torch.float64, device=dev) for x in arrs]


def step_of(tensors, dev, lower=None):
    tq = on(tensors, dev)
    lo = None if lower is None else torch.tensor(lower, device=dev).requires_grad_(True)
    for t in tq:
        if t.nelement():
            t.requires_grad_(True)
    f = QPFunction(verbose=-1)

    def step():
        for t in tq:
            t.grad = None
        z = f(*tq) if lo is None else f(*tq, lower=lo)
        z.backward(torch.ones_like(z))
        return z
    return step


def alternate(steps, reps, rounds):
    t = {k: [] for k in steps}
    for fn in steps.values():
        fn()
    for _ in range(rounds):
        for k, fn in steps.items():
            t[k].append(timed(fn, reps))
    return t


def box(n, seed=0):
    """the headline generator's Q, p with the box z0 - [0.05, 0.55] <= z <= z0 + [0.05, 0.55] on all n variables"""
    Q, p, _, _, A, b = problems.prof_qp(B, n, n, 0, seed)
    r = np.random.RandomState(seed + 1)
    z0 = r.randn(B, n)
    G = np.broadcast_to(np.eye(n), (B, n, n)).copy()
    return Q, p, G, z0 + 0.05 + 0.5 * r.rand(B, n), A, b, z0 - 0.05 - 0.5 * r.rand(B, n)


def loop_case(dev, n, m, q, reps, rounds):
    Q, p, G, h, A, b = problems.prof_qp(B, n, m, q, 0)
    lower = h - 1.0 - np.random.RandomState(2).rand(B, m)             # h = G z0 + s0, s0 < 1: z0 stays inside
    Q, p, G, h, A, b, lower = on((Q, p, G, h, A, b, lower), dev)
    fac = KKTFactors.build(Q, G, A, B)
    res = {"range": fac.ipm_range(p, h, lower, b), "one_sided": fac.ipm(p, h, b)}
    its = {k: float(v.iters.double().mean().item()) for k, v in res.items()}
    t = alternate({"range": lambda: fac.ipm_range(p, h, lower, b), "one_sided": lambda: fac.ipm(p, h, b)}, reps, rounds)
    med = {k: statistics.median(v) for k, v in t.items()}
    per = {k: med[k] / its[k] for k in med}
    return {"shape": {"B": B, "nz": n, "nineq": m, "neq": q}, "loop_ms": {k: round(v, 5) for k, v in med.items()},
            "mean_iterations": {k: round(v, 3) for k, v in its.items()}, "ms_per_iteration": {k: round(v, 6) for k, v in per.items()},
            "range_over_one_sided_per_iteration": round(per["range"] / per["one_sided"], 4)}


def parity(dev):
    import range_checks as C
    import range_reference as R

    class Env:
        pass
    env = Env()
    env.dev = dev
    env.run = lambda variant=0: contextlib.nullcontext()
    for label in R.SHAPES:
        for sides in R.SIDES:
            C.check_reference_parity(env, label, sides)
    for label in ("t1b", "t4", "c4", "box", "g10"):
        C.check_one_sided_equivalence(env, label)
    C.check_trace_dual_resid(env)
    C.check_closed_form(env)
    C.check_adjoint_identity(env)
    return dict(sorted(C.measured.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--headline", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = 100
    Q, p, G, h, A, b, lower = box(n)
    G2, h2 = np.concatenate([G, -G], 1), np.concatenate([h, -lower], 1)
    steps = {"range": step_of((Q, p, G, h, A, b), dev, lower), "doubled": step_of((Q, p, G2, h2, A, b), dev),
             "one_sided": step_of((Q, p, G, h, A, b), dev)}
    gap = float((steps["range"]() - steps["doubled"]()).abs().max().item())
    t = alternate(steps, args.reps, args.rounds)
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {"device": torch.cuda.get_device_name(dev), "shape": {"B": B, "nz": n, "nineq": n, "neq": 0, "dtype": "f64", "G": "I"},
           "what": "fwd+bwd step through QPFunction, ms, median of the rounds (HIP events, %d steps per round)" % args.reps,
           "step_ms": {k: round(v, 5) for k, v in med.items()},
           "doubled_over_range": round(med["doubled"] / med["range"], 3),
           "range_faster_than_doubled": bool(med["range"] < med["doubled"]),
           "range_minus_one_sided_ms": round(med["range"] - med["one_sided"], 5),
           "max_abs_zhat_range_minus_doubled": gap,
           "rounds": {k: [round(x, 5) for x in v] for k, v in t.items()}}
    print(json.dumps(out), flush=True)
    out["loop_alone"] = [loop_case(dev, *s, args.reps, args.rounds) for s in ((100, 100, 0), (100, 50, 10), (20, 170, 2))]
    print(json.dumps(out["loop_alone"]), flush=True)
    out["parity_maxima"] = parity(dev)
    if args.headline:
        with open(args.headline) as f:
            hl = json.load(f)
        par, new = sorted(hl["parent"]), sorted(hl["this"])
        out["bench_headline_qps"] = {"parent": hl["parent"], "this": hl["this"], "this_median": statistics.median(new),
                                     "parent_spread": [par[0], par[-1]],
                                     "inside": bool(par[0] <= statistics.median(new) <= par[-1])}
        print(json.dumps(out["bench_headline_qps"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    # the reason for the feature: the range call must beat the doubled-row call at the headline box
    if not out["range_faster_than_doubled"]:
        sys.exit("bench_range: the range call (%.4f ms) is not faster than the doubled-row call (%.4f ms)" % (med["range"], med["doubled"]))


if __name__ == "__main__":
    main()
