#!/usr/bin/env python3
"""The record of tests/loop_checks.py on the device: every check of tests/test_gpu_loop.py once (the iterates after k
iterations, iteration counts and trace at eps = 1e-8, the best iterate's bookkeeping, stall_policy = 0, float32 tensors in
float64 arithmetic, the one-wave form beyond 512 QPs -- every loop form of the A/B knob against oracle/qp_oracle, QP by QP)
and the range role's iterates (tests/range_checks.py), one MI355X.  Writes the worst figure per check and case beside its
gate, and the iteration counts at the default eps = 1e-12 of the library's default form and of the oracle (an observation:
the end game there is round-off, the counts are not gated).  Exits non-zero when a check fails, after the others have run.

    python scripts/check_loop.py [--out profiles/loop_trajectory.json]
"""
import argparse
import contextlib
import json
import os
import sys
import time
import traceback

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loop_checks as C  # noqa: E402
import range_checks as RC  # noqa: E402


class Env:
    def __init__(self):
        from qpth_amd import _lib
        self.lib = _lib.hip()
        self.dev = torch.device("cuda:0")

    @contextlib.contextmanager
    def run(self, variant=0):
        old = self.lib.dll.qpx_set_ipm_variant(int(variant))
        try:
            yield
        finally:
            self.lib.dll.qpx_set_ipm_variant(old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    env = Env()
    failed = []

    def run(check, *a):
        try:
            check(env, *a)
        except AssertionError:
            failed.append("%s%r" % (check.__name__, a))
            traceback.print_exc()

    t0 = time.time()
    for shape, form in C.CASES:
        run(C.check_iterates_after_k, shape, form)
        run(C.check_counts_and_trace, shape, form)
        run(C.check_best_iterate, shape, form)
        run(C.check_no_stall_counter, shape, form)
    for shape in C.SHAPES + [C.BIG]:
        run(C.record_counts, shape)
    for shape in C.WIDE_SHAPES:
        run(C.check_wide_iterates, shape)
    run(C.check_one_wave_beyond_512)
    for label in ("t1b", "t2", "t4", "c4", "box", "g10"):
        run(RC.check_iterates_after_k, label, "half")
    seconds = time.time() - t0

    def worst(prefix, src=C.measured):
        vals = [v for k, v in src.items() if k.startswith(prefix)]
        return max(vals) if vals else None

    out = {"device": torch.cuda.get_device_name(env.dev),
           "what": "tests/loop_checks.py on the device: worst figure per check over %d (shape, form) cases, then per case" % len(C.CASES),
           "gates": {"iterates": C.TOL, "best_resid_k": C.TOL, "best_resid_k_rel": C.TOL, "best_resid_k_rel_below_1e-3": None,
                     "trace": C.TOL, "trace_rel": C.TRACE_REL, "best_resid": 1e-12, "wide": C.TOL_WIDE,
                     "range_iterates": RC.TOL_REF},
           "worst": {"iterates": worst("iterates/"), "best_resid_k": worst("best_resid_k/"),
                     "best_resid_k_rel": worst("best_resid_k_rel/"),
                     "best_resid_k_rel_below_1e-3": worst("best_resid_k_rel_below_1e-3/"), "trace": worst("trace/"),
                     "trace_rel": worst("trace_rel/"), "best_resid": worst("best_resid/"), "wide": worst("wide/"),
                     "range_iterates": worst("iterates/", RC.measured)},
           "iterations_at_eps_1e-12_stall_policy_1": C.counts,
           "failed": failed, "seconds": round(seconds, 1),
           "measured": dict(sorted(C.measured.items())),
           "range_measured": {k: v for k, v in sorted(RC.measured.items()) if k.startswith("iterates/")}}
    print(json.dumps({k: out[k] for k in ("device", "gates", "worst", "failed", "seconds")}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if failed:
        sys.exit("check_loop: %d checks failed: %s" % (len(failed), ", ".join(failed)))


if __name__ == "__main__":
    main()
