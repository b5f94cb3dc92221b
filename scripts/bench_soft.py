#!/usr/bin/env python3
"""What soft inequality rows cost (QPFunction(...)(Q, p, G, h, A, b, rho), qpx_pre_factor_soft): the fwd+bwd step
at the headline shape (B = 512, nz = nineq = 100, float64, prof_qp(seed 0)), one process, HIP events, alternating rounds:

  hard ........ QPFunction on the six parameters
  soft ........ the same with rho per QP (every fourth row hard, rho in [0.5, 5.5] on the others): the headline kernels
  augmented ... what a caller had to write before: the dense QP in (z, t), nz' = nz + 75, Q' = blkdiag(Q, diag rho),
                G' = [G, -E] -- nz' + nineq = 275 > 208, the large-QP family

and every figure tests/soft_checks.py prints and asserts on (tests/test_gpu_soft.py), measured on this device.

--headline FILE: a JSON {"parent": [...], "this": [...]} of bench.py's headline QPs/s, three runs of the parent build and
three of this one on the same box (a job script runs bench.py in both trees and writes the file); recorded with the rule
"the new median lies inside the parent's min-max spread widened by that spread once more".

    python scripts/bench_soft.py [--reps 10] [--rounds 5] [--headline FILE] [--out profiles/soft.json]
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
import soft_reference as S  # noqa: E402
from qpth_amd.qp import QPFunction  # noqa: E402

SHAPE = (512, 100, 100, 0)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def step_of(tensors, dev):
    tq = [torch.tensor(np.asarray(x), device=dev) if np.size(x) else torch.empty(0, dtype=torch.float64, device=dev) for x in tensors]
    for t in tq:
        if t.nelement():
            t.requires_grad_(True)
    f = QPFunction(verbose=-1)

    def step():
        for t in tq:
            t.grad = None
        z = f(*tq)
        z.backward(torch.ones_like(z))
    return step


def parity(dev):
    import soft_checks as C

    class Env:
        pass
    env = Env()
    env.dev = dev
    env.run = lambda variant=0: contextlib.nullcontext()
    for label in ("a", "b0", "b1", "d", "e"):
        C.check_reference_parity(env, label)
    for label in C.CASES:
        C.check_kkt_equivalence(env, label)
    for label in ("a", "b0", "b1"):
        C.check_stop_rule(env, label)
    C.check_adjoint_identity(env)
    C.check_infeasible_box(env)
    C.check_sensitivity(env)
    return dict(sorted(C.measured.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--headline", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, n, m, q = SHAPE
    Q, p, G, h, A, b = problems.prof_qp(B, n, m, q, 0)
    r = np.random.RandomState(1)
    rho = 0.5 + 5.0 * r.rand(B, m)
    rho[:, ::4] = np.inf
    aug = [S.augment(Q[i], p[i], G[i], h[i], A, b, rho[i])[0] for i in range(B)]
    aug = [np.stack([a[k] for a in aug]) if np.size(aug[0][k]) else aug[0][k] for k in range(6)]
    steps = {"hard": step_of((Q, p, G, h, A, b), dev), "soft": step_of((Q, p, G, h, A, b, rho), dev), "augmented": step_of(aug, dev)}
    t = {k: [] for k in steps}
    for fn in steps.values():
        fn()
    for _ in range(args.rounds):
        for k, fn in steps.items():
            t[k].append(timed(fn, args.reps))
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {"device": torch.cuda.get_device_name(dev), "shape": {"B": B, "nz": n, "nineq": m, "neq": q, "dtype": "f64"},
           "what": "fwd+bwd step through QPFunction, ms, median of the rounds (HIP events, %d steps per round)" % args.reps,
           "step_ms": {k: round(v, 5) for k, v in med.items()},
           "hard_spread_ms": round(max(t["hard"]) - min(t["hard"]), 5),
           "soft_minus_hard_ms": round(med["soft"] - med["hard"], 5),
           "augmented_over_soft": round(med["augmented"] / med["soft"], 3),
           "augmented_shape": {"nz": int(aug[0].shape[-1]), "nineq": m, "neq": q},
           "rounds": {k: [round(x, 5) for x in v] for k, v in t.items()}}
    print(json.dumps(out), flush=True)
    out["parity_maxima"] = parity(dev)
    if args.headline:
        with open(args.headline) as f:
            hl = json.load(f)
        par, new = sorted(hl["parent"]), sorted(hl["this"])
        spread = par[-1] - par[0]
        out["bench_headline_qps"] = {"parent": hl["parent"], "this": hl["this"], "this_median": statistics.median(new),
                                     "allowed": [par[0] - spread, par[-1] + spread],
                                     "inside": bool(par[0] - spread <= statistics.median(new) <= par[-1] + spread)}
        print(json.dumps(out["bench_headline_qps"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
