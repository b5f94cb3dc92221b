#!/usr/bin/env python3
"""What soft two-sided rows cost and save (QPFunction(...)(Q, p, G, h, A, b, soft_range=SoftRange(...)), qpx_ipm_soft_range;
DESIGN 4.13), one MI355X, float64, one process, HIP events, medians of alternating rounds:

  the headline case ... B = 512, nz = nineq = 100, the headline generator's QP with the band lower = h - (0.3 + U), pulled below
                        G z0 on the rows i % 6 == 0 and pushed above it on the rows i % 6 == 3, every row soft on both sides,
                        gamma in [0.2, 3.2], rho in [0.5, 4.5], fwd+bwd through QPFunction,
      soft_range ..... the new keyword: 100 rows and 100 variables, the seven-row chain-wave loop on the hard factors
      range .......... (a) the lower= call of the same shape on a feasible band (another QP: hard rows)
      elastic ........ (b) the rho, l1= call on the same h (another QP: no lower side)
      augmented ...... (c) what a caller had to write before: the dense QP in (z, tu, tl), 300 variables and 400 rows -- the
                       large-QP family

  the loop alone ...... KKTFactors.ipm_soft_range against KKTFactors.ipm_range and KKTFactors.ipm on the same factors, (n, m, q) of
      the headline, of C3 (100, 50, 10) and of (20, 170, 2), every row soft on both sides / hard two-sided on the feasible band /
      one-sided, per IPM iteration (launch time / mean iteration count; each call's small launches in front of the loop included)

and every figure tests/soft_range_checks.py prints and asserts on (tests/test_gpu_soft_range.py), measured on this device.
No time or quotient is gated.

    python scripts/bench_soft_range.py [--reps 10] [--rounds 5] [--out profiles/soft_range.json]
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
from qpth_amd import SoftRange  # noqa: E402
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


def step_of(tensors, dev, call, nz=None):
    """fwd+bwd of QPFunction; call(f, tensors) makes the forward; nz: the loss reads the first nz entries of zhat"""
    tq = on(tensors, dev)
    for t in tq:
        if t.nelement():
            t.requires_grad_(True)
    f = QPFunction(verbose=-1)

    def step():
        for t in tq:
            t.grad = None
        z = call(f, tq)
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


def augment_batch(Q, p, G, h, A, lower, gu, ru, gl, rl):
    """the augmented dense QP of a batch whose rows are all soft on both sides (tests/soft_range_reference.py: augment, batched)"""
    n, m = Q.shape[1], G.shape[1]
    Q2 = np.zeros((B, n + 2 * m, n + 2 * m))
    Q2[:, :n, :n] = Q
    Q2[:, n:n + m, n:n + m] = ru[:, :, None] * np.eye(m)
    Q2[:, n + m:, n + m:] = rl[:, :, None] * np.eye(m)
    eye, zm, zn = np.broadcast_to(np.eye(m), (B, m, m)), np.zeros((B, m, m)), np.zeros((B, m, n))
    G2 = np.concatenate([np.concatenate([G, -eye, zm], 2), np.concatenate([-G, zm, -eye], 2),
                         np.concatenate([zn, -eye, zm], 2), np.concatenate([zn, zm, -eye], 2)], 1)
    A2 = np.concatenate([A, np.zeros((B, A.shape[1], 2 * m))], 2) if np.size(A) else A
    return Q2, np.concatenate([p, gu, gl], 1), G2, np.concatenate([h, -lower, np.zeros((B, 2 * m))], 1), A2


def band(h0, m, seed):
    """the fixtures' recipe on the generator's h: (h, lower, width, gamma_u, rho_u, gamma_l, rho_l)"""
    r = np.random.RandomState(seed)
    gu, ru, gl, rl = 0.2 + 3.0 * r.rand(B, m), 0.5 + 4.0 * r.rand(B, m), 0.2 + 3.0 * r.rand(B, m), 0.5 + 4.0 * r.rand(B, m)
    width, pull = 0.3 + r.rand(B, m), 1.5 * r.rand(B, m)
    i = np.arange(m)
    h = np.where(i % 6 == 0, h0 - pull, h0)
    h = np.where(i % 6 == 3, h0 + pull + width, h)
    return h, h - width, width, gu, ru, gl, rl


def loop_case(dev, n, m, q, reps, rounds):
    Q, p, G, h0, A, b = problems.prof_qp(B, n, m, q, 0)
    h, lower, width, gu, ru, gl, rl = band(h0, m, 2)
    Q, p, G, h0, A, b, h, lower, lo0, gu, ru, gl, rl = on((Q, p, G, h0, A, b, h, lower, h0 - width, gu, ru, gl, rl), dev)
    fac = KKTFactors.build(Q, G, A, B)
    calls = {"soft_range": lambda: fac.ipm_soft_range(p, h, lower, gu, ru, gl, rl, b), "range": lambda: fac.ipm_range(p, h0, lo0, b),
             "one_sided": lambda: fac.ipm(p, h0, b)}
    its = {k: float(fn().iters.double().mean().item()) for k, fn in calls.items()}
    t = alternate(calls, reps, rounds)
    med = {k: statistics.median(v) for k, v in t.items()}
    per = {k: med[k] / its[k] for k in med}
    return {"shape": {"B": B, "nz": n, "nineq": m, "neq": q}, "loop_ms": {k: round(v, 5) for k, v in med.items()},
            "mean_iterations": {k: round(v, 3) for k, v in its.items()}, "ms_per_iteration": {k: round(v, 6) for k, v in per.items()},
            "soft_range_over_range_per_iteration": round(per["soft_range"] / per["range"], 4),
            "soft_range_over_one_sided_per_iteration": round(per["soft_range"] / per["one_sided"], 4)}


def parity(dev):
    import soft_range_checks as C
    import soft_range_reference as R

    class Env:
        pass
    env = Env()
    env.dev = dev
    env.run = lambda variant=0: contextlib.nullcontext()
    for label in R.SHAPES:
        for kind in R.KINDS:
            C.check_reference_parity(env, label, kind)
            C.check_iteration_counts(env, label, kind, gated=False)
    for label, kind in C.TRACED:
        C.check_trace(env, label, kind)
    for label in ("t1b", "c4", "c7"):
        C.check_hard_sides_are_the_range_call(env, label)
        C.check_no_lower_is_the_elastic_call(env, label)
        C.check_hard_one_sided_is_the_six_input_call(env, label)
    C.check_exactness(env, "t1b")
    C.check_exactness(env, "c4")
    for key in C.SLOT_SHAPES:
        C.check_augmented_call(env, key)
    return dict(sorted(C.measured.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = m = 100
    Q, p, G, h0, A, b = problems.prof_qp(B, n, m, 0, 0)
    h, lower, width, gu, ru, gl, rl = band(h0, m, 1)
    steps = {
        "soft_range": step_of((Q, p, G, h, A, b, lower, gu, ru, gl, rl), dev, lambda f, t: f(*t[:6], soft_range=SoftRange(*t[6:]))),
        "range": step_of((Q, p, G, h0, A, b, h0 - width), dev, lambda f, t: f(*t[:6], lower=t[6])),
        "elastic": step_of((Q, p, G, h, A, b, ru, gu), dev, lambda f, t: f(*t[:7], l1=t[7])),
        "augmented": step_of(augment_batch(Q, p, G, h, A, lower, gu, ru, gl, rl) + (b,), dev, lambda f, t: f(*t), nz=n),
    }
    gap = float((steps["soft_range"]() - steps["augmented"]()).abs().max().item())
    t = alternate(steps, args.reps, args.rounds)
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {"device": torch.cuda.get_device_name(dev), "shape": {"B": B, "nz": n, "nineq": m, "neq": 0, "dtype": "f64"},
           "what": "fwd+bwd step through QPFunction, ms, median of the rounds (HIP events, %d steps per round)" % args.reps,
           "step_ms": {k: round(v, 5) for k, v in med.items()},
           "augmented_over_soft_range": round(med["augmented"] / med["soft_range"], 3),
           "soft_range_over_range": round(med["soft_range"] / med["range"], 4),
           "soft_range_minus_range_ms": round(med["soft_range"] - med["range"], 5),
           "soft_range_minus_elastic_ms": round(med["soft_range"] - med["elastic"], 5),
           "max_abs_zhat_soft_range_minus_augmented": gap,
           "rounds": {k: [round(x, 5) for x in v] for k, v in t.items()}}
    print(json.dumps(out), flush=True)
    out["loop_alone"] = [loop_case(dev, *s, args.reps, args.rounds) for s in ((100, 100, 0), (100, 50, 10), (20, 170, 2))]
    print(json.dumps(out["loop_alone"]), flush=True)
    out["parity_maxima"] = parity(dev)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
