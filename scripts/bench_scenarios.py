#!/usr/bin/env python3
"""What scenario batches save (QPFunction(scenarios=K), qpx_ipm_group), one MI355X, float64, one process, HIP
events, medians of alternating rounds.  Per shape -- B groups of K scenarios --

      grouped ....... QPFunction(scenarios=K)(Q (B,.,.), p (B,K,.), ...): B blobs, the loop and the backward on B K QPs, the
                      matrices' gradients contracted per group
      expanded ...... what a caller had to write before: QPFunction()(Q.repeat_interleave(K, 0), p.reshape(B K, .), ...) --
                      B K pre-factorisations and blobs, B K outer products per matrix gradient, added up again by autograd

the fwd+bwd step through QPFunction (all six parameters require gradients), and through KKTFactors the three launch times of
each side -- pre-factorisation, loop, backward (the grouped one with its three contractions) -- and the bytes of the factor
blobs.  Shapes: 32 x 16 at nz = nineq = 100, 4096 x 16 at nz = nineq = 64, 2 x 256 at (100, 50, 10).  Also the grouped
contraction alone at each shape (dQ's, K = 16: one of a workgroup's sixteen waves has rows to add).

Exits non-zero when the grouped step is slower than the expanded one at any shape.

--headline FILE: a JSON {"parent": [...], "this": [...]} of bench.py's headline QPs/s, runs of the parent build and of this
one alternating on the same box; recorded with the rule "this build's median lies inside the parent's min-max spread".

    python scripts/bench_scenarios.py [--reps 5] [--rounds 5] [--headline FILE] [--out profiles/scenarios.json]
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
from qpth_amd.qp import QPFunction  # noqa: E402

SHAPES = [(32, 16, (100, 100, 0)), (4096, 16, (64, 64, 0)), (2, 256, (100, 50, 10))]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(steps, reps, rounds):
    t = {k: [] for k in steps}
    for fn in steps.values():
        fn()
    for _ in range(rounds):
        for k, fn in steps.items():
            t[k].append(timed(fn, reps))
    return t


def make(B, K, shape, dev, seed=0):
    """Q, G, A of B groups (the headline generator) and p, h, b of B K QPs, feasible by construction"""
    n, m, q = shape
    Q, _, G, _, A, _ = problems.prof_qp(B, n, m, q, seed)
    r = np.random.RandomState(seed + 1)
    z0, s0, p = r.randn(B, K, n), r.rand(B, K, m), r.randn(B, K, n)
    h = np.einsum("gmn,gkn->gkm", G, z0) + s0
    b = np.einsum("gqn,gkn->gkq", A, z0) if q else np.zeros(0)
    return [torch.tensor(x, device=dev) if np.size(x) else torch.empty(0, dtype=torch.float64, device=dev) for x in (Q, p, G, h, A, b)]


def step_of(six, K=None):
    six = [t.clone().requires_grad_(True) if t.nelement() else t for t in six]
    f = QPFunction(verbose=-1, scenarios=K)

    def step():
        for t in six:
            t.grad = None
        z = f(*six)
        z.backward(torch.ones_like(z))
        return z
    return step, six


def case(dev, B, K, shape, reps, rounds):
    n, m, q = shape
    Q, p, G, h, A, b = make(B, K, shape, dev)
    flat = [p.reshape(B * K, n), h.reshape(B * K, m), b.reshape(B * K, q) if q else b]
    exp = [Q.repeat_interleave(K, 0), flat[0], G.repeat_interleave(K, 0), flat[1], A.repeat_interleave(K, 0) if q else A, flat[2]]
    sg, tg = step_of([Q, p, G, h, A, b], K)
    se, te = step_of(exp)
    zg, ze = sg(), se()
    same = bool(torch.equal(zg.reshape(B * K, n), ze))
    gap = float((tg[0].grad - te[0].grad.reshape(B, K, n, n).sum(1)).abs().max() / te[0].grad.abs().max())
    t = alternate({"grouped": sg, "expanded": se}, reps, rounds)
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {"shape": {"groups": B, "scenarios": K, "nz": n, "nineq": m, "neq": q, "dtype": "f64"},
           "step_ms": {k: round(v, 5) for k, v in med.items()}, "expanded_over_grouped": round(med["expanded"] / med["grouped"], 4),
           "grouped_not_slower": bool(med["grouped"] <= med["expanded"]), "zhat_bitwise_equal": same, "dQ_max_rel_gap": gap,
           "rounds": {k: [round(x, 5) for x in v] for k, v in t.items()}}
    del sg, se, tg, te, zg, ze
    # the three launches of each side, through KKTFactors
    ones = torch.ones(B * K, n, dtype=torch.float64, device=dev)
    parts, blob = {}, {}
    for side, build in (("grouped", lambda: KKTFactors.build(Q, G, A, nBatch=B, scenarios=K)),
                        ("expanded", lambda: KKTFactors.build(exp[0], exp[2], exp[4]))):
        fac = build()
        res = fac.ipm(*flat)
        blob[side] = fac.blob.numel() * fac.blob.element_size()
        tt = alternate({"pre_factor": build, "loop": lambda: fac.ipm(*flat),
                        "backward": lambda: fac.backward(res.zhat, res.lam, res.slacks, res.nu, ones)}, reps, rounds)
        parts[side] = {k: round(statistics.median(v), 5) for k, v in tt.items()}
        if side == "grouped":
            dx = torch.randn(B * K, n, dtype=torch.float64, device=dev)
            dq = torch.empty(B, n, n, dtype=torch.float64, device=dev)
            lib = _lib.hip()
            parts[side]["contraction_dQ_alone"] = round(statistics.median(
                alternate({"c": lambda: lib.group_outer(K, dx, res.zhat, res.zhat, dx, 0.5, dq)}, reps, rounds)["c"]), 5)
        del fac, res
    out["launch_ms"], out["blob_bytes"] = parts, blob
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--headline", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev),
           "what": "fwd+bwd step through QPFunction, ms, median of %d alternating rounds (HIP events, %d steps per round); "
                   "launch_ms: the same through KKTFactors per launch" % (args.rounds, args.reps), "cases": []}
    for B, K, shape in SHAPES:
        out["cases"].append(case(dev, B, K, shape, args.reps, args.rounds))
        print(json.dumps(out["cases"][-1]), flush=True)
    if args.headline:
        with open(args.headline) as f:
            hl = json.load(f)
        par, new = sorted(hl["parent"]), sorted(hl["this"])
        out["bench_headline_qps"] = {"parent": hl["parent"], "this": hl["this"], "this_median": statistics.median(new),
                                     "parent_spread": [par[0], par[-1]], "inside": bool(par[0] <= statistics.median(new) <= par[-1])}
        print(json.dumps(out["bench_headline_qps"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    slow = [c["shape"] for c in out["cases"] if not c["grouped_not_slower"]]
    if slow:
        sys.exit("bench_scenarios: the grouped call is slower than the expanded call at %s" % slow)


if __name__ == "__main__":
    main()
