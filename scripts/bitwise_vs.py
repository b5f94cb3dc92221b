#!/usr/bin/env python3
"""Are two builds of the library bit-identical in their results?

bitwise_vs.py a.so b.so [B n m q] [--device cpu|cuda:0] [--forms 0,3,256,...] [--ext] [--labels t1b,c4,...]

The plain call: forward (zhat, lam, slacks, nu, iters, status, best_resid, trace) and the p-gradient of both on the same
seeded inputs, compared with torch.equal (NaN entries equal).  --device cpu: CPU tensors through two builds of the emulator
library (tests/emu), as tests/emu/harness.py loads one.  --forms: under each of these qpx_set_ipm_variant knobs.  --ext: also
qpx_ipm_warm, qpx_ipm_range (with lam_lo, slack_lo) and qpx_ipm_elastic (with t) on that problem.  --labels: the range and
elastic problems of tests/range_reference.py / tests/elastic_reference.py with these labels, "half" and "all" (a label only
one of the two has is run for that one).  Exit status 1 if anything differs."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import problems  # noqa: E402
from qpth_amd import _lib  # noqa: E402
from qpth_amd.kkt import KKTFactors  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs=2)
ap.add_argument("dims", nargs="*", type=int)
ap.add_argument("--device", default="cuda:0")
ap.add_argument("--forms", default="0")
ap.add_argument("--ext", action="store_true")
ap.add_argument("--labels", default="")
args = ap.parse_args()
dev = torch.device(args.device)
if dev.type == "cpu":
    os.environ.setdefault("QPX_EMU_THREADS", "128")
libs = [_lib.QpxLib(os.path.abspath(x), strict=False) for x in args.libs]
FIELDS = ("zhat", "lam", "slacks", "nu", "iters", "status", "best_resid", "trace")


def on(arrs):
    return [torch.tensor(x, dtype=torch.float64, device=dev) if x.size else torch.empty(0, dtype=torch.float64, device=dev) for x in arrs]


def fields(res, extra=()):
    return {k: getattr(res, k).clone() for k in FIELDS + tuple(extra)}


def same(x, y):
    if x.dtype.is_floating_point:
        nx, ny = torch.isnan(x), torch.isnan(y)
        return torch.equal(nx, ny) and torch.equal(torch.where(nx, torch.zeros_like(x), x), torch.where(ny, torch.zeros_like(y), y))
    return torch.equal(x, y)


def both(form, Q, G, A, B, call):
    """call(fac) -> {name: tensor} under each library"""
    outs = []
    for lib in libs:
        _lib.set_test_backend(lib)
        old = lib.dll.qpx_set_ipm_variant(form)
        try:
            outs.append(call(KKTFactors.build(Q, G, A, B)))
            if dev.type == "cuda":
                torch.cuda.synchronize()
        finally:
            lib.dll.qpx_set_ipm_variant(old)
            _lib.set_test_backend(None)
    return outs


failed = 0


def report(what, outs):
    global failed
    if outs[0] is None:
        print("%-46s not served under this knob" % what, flush=True)
        return
    diff = [k for k in outs[0] if not same(outs[0][k], outs[1][k])]
    failed += bool(diff)
    print("%-46s %s vs %s: %s" % (what, os.path.basename(args.libs[0]), os.path.basename(args.libs[1]),
                                   "BIT-IDENTICAL" if not diff else "differ in " + ", ".join(diff)), flush=True)
    for k in diff:
        x, y = outs[0][k], outs[1][k]
        if x.dtype.is_floating_point:
            print("   %-10s max abs diff %.3e (max abs %.3e)" % (k, (x - y).nan_to_num().abs().max().item(), x.nan_to_num().abs().max().item()))
        else:
            print("   %-10s differs in %d of %d entries (by at most %d)" % (k, int((x != y).sum()), x.numel(), int((x - y).abs().max())))


def plain(form, B, n, m, q):
    tag = "B=%d n=%d m=%d q=%d form %d" % (B, n, m, q, form)
    Q, p, G, h, A, b = on(problems.prof_qp(B, n, m, q, 5))
    ones = torch.ones(B, n, dtype=Q.dtype, device=dev)

    def cold(fac):
        res = fac.ipm(p, h, b, want_trace=True)
        out = fields(res)
        out["dp"] = fac.backward(res.zhat, res.lam, res.slacks, res.nu, ones, want=(False, True, False, False, False, False))[1].clone()
        return out

    outs = both(form, Q, G, A, B, cold)
    report(tag, outs)
    if not args.ext:
        return
    c = outs[0]
    g = torch.Generator().manual_seed(7)
    u1, u2, u3 = [torch.rand(B, m, dtype=torch.float64, generator=g).to(dev) for _ in range(3)]
    hard = (torch.arange(m, device=dev) % 2 == 1).expand(B, m)
    inf = torch.full((B, m), float("inf"), dtype=torch.float64, device=dev)
    # warm: the cold solution, at a nearby p
    report(tag + " warm", both(form, Q, G, A, B, lambda fac: fields(fac.ipm(p * 1.01, h, b, want_trace=True, warm=(c["lam"], c["slacks"])), ("warm_used",))))
    probe = both(form, Q, G, A, B, lambda fac: {"r": torch.tensor(fac.range_ok()), "e": torch.tensor(fac.elastic_ok())})[0]
    # range: a band below h that the cold solution lies in, every second row one-sided
    Gz = torch.matmul(G, c["zhat"].unsqueeze(-1)).squeeze(-1)
    lower = torch.where(hard, -inf, torch.minimum(Gz, h) - 0.05 - 0.5 * u1)
    if bool(probe["r"]):
        report(tag + " range", both(form, Q, G, A, B, lambda fac: fields(fac.ipm_range(p, h, lower, b, want_trace=True), ("lam_lo", "slacks_lo"))))
    # elastic: h pulled below the solution on every third row, every second row hard
    gamma, rho = torch.where(hard, inf, 0.2 + 3.0 * u2), torch.where(hard, inf, 0.5 + 4.0 * u3)
    he = torch.where((torch.arange(m, device=dev) % 3 == 0).expand(B, m) & ~hard, Gz - 0.5 * u1, h)
    if bool(probe["e"]):
        report(tag + " elastic", both(form, Q, G, A, B, lambda fac: fields(fac.ipm_elastic(p, he, gamma, rho, b, want_trace=True), ("lam_t", "slacks_t", "t"))))


def labelled(form, label):
    import elastic_reference
    import range_reference
    for kind in ("half", "all"):
        if label in range_reference.SHAPES:
            Q, p, G, h, A, b, lower = on(range_reference.range_problem(label, kind))
            report("range %s/%s form %d" % (label, kind, form), both(form, Q, G, A, range_reference.SHAPES[label][0], lambda fac: fac.range_ok() and fields(
                fac.ipm_range(p, h, lower, b, want_trace=True), ("lam_lo", "slacks_lo")) or None))
        if label in elastic_reference.SHAPES:
            Q, p, G, h, A, b, rho, gamma = on(elastic_reference.elastic_problem(label, kind))
            report("elastic %s/%s form %d" % (label, kind, form), both(form, Q, G, A, elastic_reference.SHAPES[label][0], lambda fac: fac.elastic_ok() and fields(
                fac.ipm_elastic(p, h, gamma, rho, b, want_trace=True), ("lam_t", "slacks_t", "t")) or None))


for form in [int(x) for x in args.forms.split(",")]:
    if args.dims or not args.labels:
        plain(form, *(args.dims or [512, 100, 100, 0]))
    for label in [x for x in args.labels.split(",") if x]:
        labelled(form, label)
sys.exit(1 if failed else 0)
