#!/usr/bin/env python3
"""The record of tests/kkt_checks.py on the device: every check of tests/test_gpu_kkt.py once (the plain solve, the backward
with its duals cotangents, forward mode with the adjoint identity, K right-hand sides, the second-order pass -- every KKT form
of the A/B knob against a dense solve refined in extended precision; the one-wave form beyond 512 QPs, shared factors, QPX_F32
on the thread-grid kernels, float32 tensors in float64 arithmetic), one MI355X.  Writes the worst figure per check and case
beside its gate, the forms that declined a role, whether K = 1 of the multi solve equalled the single solve bit for bit, and
the reference-side figures the gates rest on: the float64 and the float32 dense solve against the refined reference.  Exits
non-zero when a check fails, after the others have run.

    python scripts/check_kkt.py [--out profiles/kkt_roles.json]
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
import kkt_checks as C  # noqa: E402


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


def gate_table():
    """the gate of every figure: one entry per (check, arithmetic) where all its cases share it, else one per case"""
    groups = {}
    for k, g in C.gates.items():
        cls = "QPX_F32" if "/f32/" in k else "float32_tensors_in_float64_arithmetic" if "/wide/" in k else "float64"
        groups.setdefault("%s (%s)" % (k.split("/")[0], cls), {})[k] = g
    out = {}
    for name, per in sorted(groups.items()):
        if len(set(per.values())) == 1:
            out[name] = next(iter(per.values()))
        else:
            out.update(sorted(per.items()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    env = Env()
    failed, declined = [], {"multi": [], "backward2": []}

    def run(check, *a):
        try:
            return check(env, *a)
        except AssertionError:
            failed.append("%s%r" % (check.__name__, a))
            traceback.print_exc()

    t0 = time.time()
    for shape, form in C.CASES:
        run(C.check_solve, shape, form)
        run(C.check_backward, shape, form)
        run(C.check_jvp, shape, form)
        if run(C.check_multi, shape, form) is False:
            declined["multi"].append(C.tag(shape, form))
        else:
            run(C.check_multi_k1, shape, form)
        if run(C.check_backward2, shape, form) is False:
            declined["backward2"].append(C.tag(shape, form))
    run(C.check_one_wave_beyond_512)
    run(C.check_multi_k1, C.ONE_WAVE_SHAPE, 0, C.ONE_WAVE_B)
    for shape in C.SHARED_SHAPES:
        run(C.check_shared_factors, shape)
        run(C.check_multi_k1, shape, 0, C.B3, "shared")
    for shape in C.F32_SHAPES:
        run(C.check_f32_grid, shape)
    for shape in C.WIDE_SHAPES:
        run(C.check_wide, shape)
    seconds = time.time() - t0

    checks = sorted({k.split("/")[0] for k in C.measured})

    def worst(prefix, pick):
        """(figure, gate, case) of the check's worst figure relative to its gate among the cases `pick` keeps"""
        keys = [k for k in C.measured if k.split("/")[0] == prefix and pick(k)]
        if not keys:
            return None
        k = max(keys, key=lambda k: C.measured[k] / C.gates[k])
        return {"worst": C.measured[k], "gate": C.gates[k], "at": k.split("/", 1)[1]}

    f64 = lambda k: not k.endswith(("/f32/mid", "/wide/mid", "/wide/bwd"))      # noqa: E731
    out = {"device": torch.cuda.get_device_name(env.dev),
           "what": "tests/kkt_checks.py on the device: per check the worst figure (relative to its gate) over %d (shape, form) "
                   "cases and the cases beside them, by arithmetic; then every figure beside its gate" % len(C.CASES),
           "float64": {c: worst(c, f64) for c in checks},
           "float32_tensors_in_float64_arithmetic": {c: worst(c, lambda k: "/wide/" in k) for c in checks if worst(c, lambda k: "/wide/" in k)},
           "QPX_F32": {c: worst(c, lambda k: "/f32/" in k) for c in checks if worst(c, lambda k: "/f32/" in k)},
           "multi_k1_equals_the_single_solve_bitwise": {"all": all(C.k1_bitwise.values()),
                                                        "not_at": sorted(k for k, v in C.k1_bitwise.items() if not v)},
           "declined": declined,
           "reference_side": {"what": "an unrefined dense solve of check 1's system against the refined reference: dense64 = the "
                                      "float64 LU alone, dense32 = a float32 torch.linalg.solve (the QPX_F32 gates are "
                                      "max(1e-3, 100 x dense32)); worst, then per case",
                              "dense64_worst": max(v for k, v in C.reference_side.items() if k.startswith("dense64/")),
                              "dense32_worst": max(v for k, v in C.reference_side.items() if k.startswith("dense32/")),
                              "per_case": dict(sorted(C.reference_side.items()))},
           "failed": failed, "seconds": round(seconds, 1),
           "gates": gate_table(), "measured": dict(sorted(C.measured.items()))}
    above = [k for k, v in C.measured.items() if not v <= C.gates[k]]
    print(json.dumps({k: out[k] for k in ("device", "float64", "float32_tensors_in_float64_arithmetic", "QPX_F32",
                                          "multi_k1_equals_the_single_solve_bitwise", "failed", "seconds")}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if failed or above:
        sys.exit("check_kkt: %d checks failed: %s; above their gate: %s" % (len(failed), ", ".join(failed), ", ".join(above)))


if __name__ == "__main__":
    main()
