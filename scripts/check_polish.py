#!/usr/bin/env python3
"""The record of tests/polish_checks.py: every check of tests/test_gpu_polish.py once on one MI355X (`--emu`: of
tests/test_emu_polish.py on the host-thread emulator) -- the finishing stage's iterates after k steps and best_resid in every
form against the numpy step reference, the best-iterate rule on ill-centred starts, steps = 0, strides and shared factors, a
non-finite QP beside healthy ones, untouched memory, the error codes.  Writes, under "MI355X" (or "emulator") of the output
file and beside what the other run left there: per form of api_polish's rule the worst figure and its gate, every figure beside
its gate, the reference-side figures behind the gates that rest on a rule, and whether the rule decided.  Exits non-zero when
a check fails, after the others have run.

    python scripts/check_polish.py [--emu] [--out profiles/polish_steps.json]
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
import polish_checks as C  # noqa: E402


class GpuEnv:
    name = "MI355X"

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
    name = "emulator"
    dev = torch.device("cpu")

    @staticmethod
    @contextlib.contextmanager
    def run(variant=0):
        from emu.harness import emulated
        with emulated(256, variant):
            yield


def case_of(key):
    """"check/shape/knob[/f32][/...]" -> the key polish_checks.forms files the case's form under"""
    parts = key.split("/")[1:]
    if parts[0] == "rule":
        parts = parts[1:]
    for cut in range(len(parts), 1, -1):
        if "/".join(parts[:cut]) in C.forms:
            return "/".join(parts[:cut])
    return None


def per_form():
    out = {}
    for k, v in C.measured.items():
        c = case_of(k)
        form = C.forms[c] if c else "other"
        slot = out.setdefault(form, {})
        what = k.split("/")[0]
        if what not in slot or v / C.gates[k] > slot[what]["worst"] / slot[what]["gate"]:
            slot[what] = {"worst": v, "gate": C.gates[k], "at": k.split("/", 1)[1]}
    return dict(sorted(out.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--emu", action="store_true", help="the host-thread emulator instead of the GPU")
    args = ap.parse_args()
    env = EmuEnv() if args.emu else GpuEnv()
    failed = []

    def run(check, *a):
        try:
            return check(env, *a)
        except Exception:            # noqa: BLE001  (a RuntimeError of the ctypes layer is a failed check too)
            failed.append("%s%r" % (check.__name__, a))
            traceback.print_exc()

    t0 = time.time()
    cases = (C.EMU_CASES if args.emu else C.CASES) + C.F32_CASES
    for c in cases:
        run(C.check_steps, *c)
        run(C.check_zero_steps, *c)
    if not args.emu:
        run(C.check_one_wave_beyond_8192)
    for c in C.ILL:
        run(C.check_best_iterate_rule, *c)
    for shape in C.SHARED_SHAPES:
        run(C.check_unbatched_phb, shape)
        run(C.check_shared_factors, shape)
    run(C.check_unbatched_phb, C.SHARED_SHAPES[0], C.BIGK)
    run(C.check_big_refuses_shared_factors)
    for c in C.NAN_CASES:
        run(C.check_nan_beside_healthy, *c)
    for shape in C.SPARE_SHAPES:
        run(C.check_spare_rows, shape)
    run(C.check_supported_and_error_codes)
    seconds = time.time() - t0

    above = [k for k, v in C.measured.items() if not v <= C.gates[k]]
    mine = {"device": env.name if args.emu else torch.cuda.get_device_name(env.dev),
            "forms": per_form(),
            "forms_not_reached": sorted(set(C.ALL_FORMS) - set(C.forms.values())),
            "rule_decided": dict(sorted(C.rule_decided.items())),
            "reference_side": dict(sorted(C.reference_side.items())),
            "failed": failed, "above_their_gate": above, "seconds": round(seconds, 1),
            "gates": dict(sorted(C.gates.items())), "measured": dict(sorted(C.measured.items()))}
    print(json.dumps({k: mine[k] for k in ("device", "forms", "forms_not_reached", "failed", "above_their_gate", "seconds")}), flush=True)
    if args.out:
        out = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                out = json.load(f)
        out["what"] = ("tests/polish_checks.py: per form of api_polish's rule the worst figure (relative to its gate) of every check, "
                       "then every figure beside its gate; reference_side (per run: the float32 dense solve is the host library's): the numpy steps with the float64 LU alone (dense64) / a "
                       "float32 dense solve (dense32) against the refined reference -- the QPX_F32 gates are max(1e-3, 100 x "
                       "dense32), the gates of the ill-centred starts max(1e-6, 100 x dense64); rule_decided: did the second term decide")
        out["case_forms"] = dict(sorted(C.forms.items()))
        out[env.name] = mine
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if failed or above:
        sys.exit("check_polish: %d checks failed: %s; above their gate: %s" % (len(failed), ", ".join(failed), ", ".join(above)))


if __name__ == "__main__":
    main()
