#!/usr/bin/env python3
"""The record of tests/prefac_checks.py on the device: every check of tests/test_gpu_prefac.py once -- the factor blob of
qpx_pre_factor / qpx_pre_factor_soft in every form (the sweep at its seven block counts, the matrix-core form, the large-QP
family, the soft forms) against a dense reference refined in extended precision, word by word -- on one MI355X.  Writes the
worst figure per check relative to its gate, every figure beside its gate and beside the figure of the plain float64 (float32)
route the gate rests on, and the conditioning ladder per form and c.  Exits non-zero when a check fails, after the others have
run.  Blobs start as NaN, as under tests/conftest.py, so that a word nobody wrote shows.

    python scripts/check_prefac.py [--out profiles/prefac_blob.json] [--emulator]

--emulator: the same on the host-thread emulator (tests/emu; QPX_EMU_SO picks another build of it).
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
import prefac_checks as C  # noqa: E402


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


def poison_empty():
    real_empty = torch.empty

    def empty(*args, **kwargs):
        t = real_empty(*args, **kwargs)
        if t.is_floating_point() and t.numel():
            t.fill_(float("nan"))
        return t
    torch.empty = empty


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--emulator", action="store_true")
    args = ap.parse_args()
    env = EmuEnv() if args.emulator else Env()
    poison_empty()
    failed = []

    def run(check, *a):
        try:
            return check(env, *a)
        except Exception:
            failed.append("%s%r" % (check.__name__, a))
            traceback.print_exc()

    t0 = time.time()
    for shape, knob in C.CASES:
        run(C.check_blob, shape, knob)
    run(C.check_knob_512_writes_the_blob_of_knob_256)
    for shape, knob in C.COND_CASES:
        for c in C.COND_CS:
            run(C.check_conditioning, shape, knob, c)
    for shape in C.WIDE_SHAPES:
        run(C.check_wide, shape)
    for shape in C.F32_SHAPES:
        run(C.check_f32, shape)
    for shape, knob in C.SOFT_CASES:
        run(C.check_soft, shape, knob)
    for shape, knob in C.STRIDE_CASES:
        run(C.check_strides, shape, knob)
    for shape, knob in C.SHARED_CASES:
        run(C.check_shared, shape, knob)
    for shape, knob in (((65, 17, 0), C.BIGK), (C.BIG, 0)):
        run(C.check_large_family_refuses_sharing, shape, knob)
    for shape, knob, how in C.FAILURE_CASES:
        run(C.check_failure, shape, knob, how)
    seconds = time.time() - t0

    def worst(prefix):
        """the check's worst figure relative to its gate, with the plain route's figure at the same array"""
        keys = [k for k in C.measured if k.split("/")[0] == prefix]
        if not keys:
            return None
        k = max(keys, key=lambda k: C.measured[k] / C.gates[k])
        big = max(keys, key=lambda k: C.measured[k])
        return {"worst": C.measured[k], "gate": C.gates[k], "lapack": C.reference_side.get(k), "at": k.split("/", 1)[1],
                "largest": C.measured[big], "largest_at": big.split("/", 1)[1], "figures": len(keys)}

    ladder = {}
    for k, v in sorted(C.measured.items()):
        if k.startswith("cond/"):
            _, shape, knob, prob, name = k.split("/")
            ladder.setdefault("%s/%s" % (shape, knob), {}).setdefault(name, {})[prob] = {
                "measured": v, "lapack": C.reference_side[k], "gate": C.gates[k]}
    checks = sorted({k.split("/")[0] for k in C.measured})
    out = {"device": "host-thread emulator" if args.emulator else torch.cuda.get_device_name(env.dev),
           "what": "tests/prefac_checks.py: per check the worst figure relative to its gate (and the largest one) over its cases; "
                   "the conditioning ladder per form, array and c; then every figure beside its gate and the plain float64 "
                   "(QPX_F32: float32) route's figure the gate is max(floor, 100 x) of.  Bitwise and exact-zero assertions "
                   "(pads, soft rows, shared factors, failed QPs) have no figure: they hold or the check is listed as failed",
           "checks": {c: worst(c) for c in checks},
           "conditioning_ladder": ladder,
           "failed": failed, "seconds": round(seconds, 1),
           "figures": {k: {"measured": C.measured[k], "gate": C.gates[k], "lapack": C.reference_side.get(k)} for k in sorted(C.measured)}}
    above = [k for k, v in C.measured.items() if not v <= C.gates[k]]
    print(json.dumps({k: out[k] for k in ("device", "checks", "failed", "seconds")}, indent=1), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if failed or above:
        sys.exit("check_prefac: %d checks failed: %s; above their gate: %s" % (len(failed), ", ".join(failed), ", ".join(above)))


if __name__ == "__main__":
    main()
