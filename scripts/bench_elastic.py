#!/usr/bin/env python3
"""What elastic rows cost and save (QPFunction(...)(Q, p, G, h, A, b, rho, l1=gamma), qpx_ipm_elastic), one MI355X,
float64, one process, HIP events, medians of alternating rounds:

  the headline case ... B = 512, nz = nineq = 100, the headline generator's QP with every third h pulled below G z0 (rows end
                        violated), gamma in [0.2, 3.2], rho in [0.5, 4.5], fwd+bwd through QPFunction,
      elastic ....... l1=gamma: 100 rows and 100 variables, the seven-row chain-wave loop on the hard factors
      augmented ..... what a caller had to write before: the dense QP in (z, t), 200 variables and 200 rows -- the large-QP family
      soft .......... the positional-rho call on the same data (another QP: the quadratic penalty alone)
      hard .......... the six-input call on the headline generator's own (feasible) h (another QP again)
  the loop alone ...... KKTFactors.ipm_elastic against KKTFactors.ipm on the same factors, (n, m, q) of the headline, of C3
      (100, 50, 10) and of (20, 170, 2), every row elastic, per IPM iteration (launch time / mean iteration count)

and every figure tests/elastic_checks.py prints and asserts on (tests/test_gpu_elastic.py), measured on this device.

--headline FILE: a JSON {"parent": [...], "this": [...]} of bench.py's headline QPs/s, three runs of the parent build and
three of this one, alternating on the same box (a job script runs bench.py in both trees and writes the file); recorded with
the rule "this build's median lies inside the parent's min-max spread".  Exits non-zero when the l1= call is not faster than
the augmented dense call.

    python scripts/bench_elastic.py [--reps 10] [--rounds 5] [--headline FILE] [--out profiles/elastic.json]
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


def step_of(tensors, dev, nz=None):
    """fwd+bwd of QPFunction on six tensors, (six, rho) or (six, rho, gamma); nz: the loss reads the first nz entries of zhat"""
    tq = on(tensors, dev)
    for t in tq:
        if t.nelement():
            t.requires_grad_(True)
    f = QPFunction(verbose=-1)

    def step():
        for t in tq:
            t.grad = None
        z = f(*tq[:7], l1=tq[7]) if len(tq) == 8 else f(*tq)
        z = z if nz is None else z[:, :nz]
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


def penalties(m, seed):
    r = np.random.RandomState(seed)
    return 0.5 + 4.0 * r.rand(B, m), 0.2 + 3.0 * r.rand(B, m), 1.5 * r.rand(B, m) * (np.arange(m) % 3 == 0)


def augment_batch(Q, p, G, h, A, rho, gamma):
    """the augmented dense QP of a batch whose rows are all elastic (tests/elastic_reference.py: augment, batched)"""
    n, m = Q.shape[1], G.shape[1]
    Q2 = np.zeros((B, n + m, n + m))
    Q2[:, :n, :n] = Q
    Q2[:, n:, n:] = rho[:, :, None] * np.eye(m)
    eye = np.broadcast_to(np.eye(m), (B, m, m))
    G2 = np.concatenate([np.concatenate([G, -eye], 2), np.concatenate([np.zeros((B, m, n)), -eye], 2)], 1)
    A2 = np.concatenate([A, np.zeros((B, A.shape[1], m))], 2) if np.size(A) else A
    return Q2, np.concatenate([p, gamma], 1), G2, np.concatenate([h, np.zeros((B, m))], 1), A2


def loop_case(dev, n, m, q, reps, rounds):
    Q, p, G, h, A, b = problems.prof_qp(B, n, m, q, 0)
    rho, gamma, pull = penalties(m, 2)
    Q, p, G, h, A, b, he, rho, gamma = on((Q, p, G, h, A, b, h - pull, rho, gamma), dev)
    fac = KKTFactors.build(Q, G, A, B)
    res = {"elastic": fac.ipm_elastic(p, he, gamma, rho, b), "one_sided": fac.ipm(p, h, b)}
    its = {k: float(v.iters.double().mean().item()) for k, v in res.items()}
    t = alternate({"elastic": lambda: fac.ipm_elastic(p, he, gamma, rho, b), "one_sided": lambda: fac.ipm(p, h, b)}, reps, rounds)
    med = {k: statistics.median(v) for k, v in t.items()}
    per = {k: med[k] / its[k] for k in med}
    return {"shape": {"B": B, "nz": n, "nineq": m, "neq": q}, "loop_ms": {k: round(v, 5) for k, v in med.items()},
            "mean_iterations": {k: round(v, 3) for k, v in its.items()}, "ms_per_iteration": {k: round(v, 6) for k, v in per.items()},
            "elastic_over_one_sided_per_iteration": round(per["elastic"] / per["one_sided"], 4)}


def parity(dev):
    import elastic_checks as C
    import elastic_reference as R

    class Env:
        pass
    env = Env()
    env.dev = dev
    env.run = lambda variant=0: contextlib.nullcontext()
    for label in R.SHAPES:
        for kind in R.KINDS:
            C.check_reference_parity(env, label, kind)
            C.check_iteration_counts(env, label, kind, gated=False)
    for label in ("t1b", "t4", "c4", "c7", "g10"):
        C.check_hard_rows(env, label)
    for label, kind in C.TRACED:
        C.check_trace(env, label, kind)
    C.check_exactness(env, "t1b")
    C.check_exactness(env, "c4")
    C.check_gamma_zero(env)
    C.check_closed_form(env)
    C.check_adjoint_identity(env)
    C.check_duals(env)
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
    Q, p, G, h, A, b = problems.prof_qp(B, n, n, 0, 0)
    rho, gamma, pull = penalties(n, 1)
    he = h - pull
    steps = {"elastic": step_of((Q, p, G, he, A, b, rho, gamma), dev),
             "augmented": step_of(augment_batch(Q, p, G, he, A, rho, gamma) + (b,), dev, nz=n),
             "soft": step_of((Q, p, G, he, A, b, rho), dev), "hard": step_of((Q, p, G, h, A, b), dev)}
    gap = float((steps["elastic"]() - steps["augmented"]()).abs().max().item())
    t = alternate(steps, args.reps, args.rounds)
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {"device": torch.cuda.get_device_name(dev), "shape": {"B": B, "nz": n, "nineq": n, "neq": 0, "dtype": "f64"},
           "what": "fwd+bwd step through QPFunction, ms, median of the rounds (HIP events, %d steps per round)" % args.reps,
           "step_ms": {k: round(v, 5) for k, v in med.items()},
           "augmented_over_elastic": round(med["augmented"] / med["elastic"], 3),
           "elastic_faster_than_augmented": bool(med["elastic"] < med["augmented"]),
           "elastic_minus_soft_ms": round(med["elastic"] - med["soft"], 5),
           "elastic_minus_hard_ms": round(med["elastic"] - med["hard"], 5),
           "max_abs_zhat_elastic_minus_augmented": gap,
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
    # the reason for the feature: the l1= call must beat the augmented dense call at the headline shape
    if not out["elastic_faster_than_augmented"]:
        sys.exit("bench_elastic: the l1= call (%.4f ms) is not faster than the augmented dense call (%.4f ms)" % (med["elastic"], med["augmented"]))


if __name__ == "__main__":
    main()
