#!/usr/bin/env python3
"""The record of tests/big_checks.py: every check of tests/test_gpu_big.py once on one MI355X (the large-QP family at 4 to 16
blocks of 64: the loop's path against oracle/qp_oracle, the KKT-solve kernels against the refined dense solve, the blob word by
word, the host forms -- parts, bits 26 and 29 -- bit for bit against the one-part default launch, bits 27 and 28 on the gates), or
with --emu the list of tests/test_emu_big.py on the host-thread emulator.  Writes every measured figure beside its gate and its
reference-side figure, which float64 gates the conditioning rule decided, whether each host form was bit for bit, and the CPU
seconds the references of each case took, under the key "MI355X" or "emulator" of the output file (the other key is kept).
Exits non-zero when a check fails, after the others have run.

    python scripts/check_big.py [--emu] [--out profiles/big_blocks.json]
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
import big_checks as C  # noqa: E402
from big_checks import K, L, P  # noqa: E402


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


class EmuEnv:
    dev = torch.device("cpu")

    @staticmethod
    @contextlib.contextmanager
    def run(variant=0):
        from emu.harness import emulated
        with emulated(256, variant):
            yield


def loop_gate(key):
    head = key.split("/")[0]
    return {"iterates": L.TOL, "best_resid_k": L.TOL, "best_resid_k_rel": L.TOL, "best_resid_k_rel_below_1e-3": None,
            "trace": L.TOL, "trace_rel": L.TRACE_REL, "best_resid": 1e-12, "wide": L.TOL_WIDE}[head]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--emu", action="store_true")
    args = ap.parse_args()
    env = EmuEnv() if args.emu else Env()
    failed = []

    def run(check, *a, **kw):
        try:
            return check(env, *a, **kw)
        except AssertionError:
            failed.append("%s%r" % (check.__name__, a))
            traceback.print_exc()

    t0 = time.time()
    shapes = C.UP_TO_FOUR_BLOCKS if args.emu else C.SHAPES
    forms = [(s, 0) for s in shapes] + ([] if args.emu else [(C.F32_SHAPE, f) for f in C.DIAG_FORMS])
    for shape, form in forms:
        run(C.check_iterates_after_k, shape, form)
        run(C.check_counts_and_trace, shape, form)
        run(C.check_best_iterate, shape, form)
        run(C.check_no_stall_counter, shape, form)
        run(C.check_solve, shape, form)
        run(C.check_backward, shape, form)
        run(C.check_jvp, shape, form)
        run(C.check_declined_roles, shape, form)
    if args.emu:
        run(C.check_iterates_after_k, C.NINE_BLOCKS)
        run(C.check_iterates_after_k, C.NINE_BLOCKS_LQ)
        run(C.check_counts_and_trace, C.NINE_BLOCKS)
        run(C.check_declined_roles, C.NINE_BLOCKS)
        run(C.check_solve, C.NINE_BLOCKS, kinds=("mid",))
    else:
        run(C.check_wide_iterates)
    run(C.check_f32)
    for shape in (C.UP_TO_FOUR_BLOCKS + [C.NINE_BLOCKS] if args.emu else C.BLOB_SHAPES):
        run(C.check_blob, shape)
    if not args.emu:
        for form in C.DIAG_FORMS:
            run(C.check_blob, C.F32_SHAPE, form)
    host = C.EMU_HOST if args.emu else C.HOST
    for shape, base, B in sorted({(s, base, B) for s, base, v, B in host}):
        run(C.check_default_launch, shape, base, B)
    for shape, base, variant, B in host:
        run(C.check_host_form, shape, base, variant, B)
    seconds = time.time() - t0

    figures = {}
    for k, v in L.measured.items():
        figures["loop/" + k] = {"measured": v, "gate": loop_gate(k)}
    for k, v in K.measured.items():
        figures["kkt/" + k] = {"measured": v, "gate": K.gates[k]}
    for k, v in P.measured.items():
        figures["prefac/" + k] = {"measured": v, "gate": P.gates[k], "reference_side": P.reference_side.get(k)}

    def worst(prefix):
        ks = [k for k in figures if k.startswith(prefix) and figures[k]["gate"]]
        if not ks:
            return None
        k = max(ks, key=lambda k: figures[k]["measured"] / figures[k]["gate"])
        return dict(figures[k], at=k)

    heads = sorted({"/".join(k.split("/")[:2]) + "/" for k in figures})
    out = {"device": "host-thread emulator" if args.emu else torch.cuda.get_device_name(env.dev),
           "what": "tests/big_checks.py: per check the worst figure relative to its gate, then every figure beside its gate (and, "
                   "for the blob, the plain float64 route's figure the gate rests on)",
           "worst": {h: worst(h) for h in heads},
           "kkt_reference_side": dict(sorted(K.reference_side.items())),
           "kkt_gates_decided_by_the_conditioning_rule": {"any": any(K.rule_decided.values()), "per_case": dict(sorted(K.rule_decided.items()))},
           "host_forms_bit_for_bit": dict(sorted(C.bitwise.items())),
           "reference_cpu_seconds": {k: round(v, 2) for k, v in sorted(C.ref_seconds.items())},
           "failed": failed, "seconds": round(seconds, 1),
           "figures": dict(sorted(figures.items()))}
    print(json.dumps({k: out[k] for k in ("device", "worst", "kkt_gates_decided_by_the_conditioning_rule", "host_forms_bit_for_bit",
                                          "failed", "seconds")}), flush=True)
    if args.out:
        both = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                both = json.load(f)
        both["emulator" if args.emu else "MI355X"] = out
        with open(args.out, "w") as f:
            json.dump(both, f, indent=1, sort_keys=True)
    if failed:
        sys.exit("check_big: %d checks failed: %s" % (len(failed), ", ".join(failed)))


if __name__ == "__main__":
    main()
