"""The path of the hard-QP interior-point loop (KKTFactors.ipm, qpx_ipm) on the host-thread emulator: the iterates after k
iterations, the iteration counts, the per-iteration residuals and the best iterate's bookkeeping of every loop form the A/B
knob reaches, against oracle/qp_oracle QP by QP.  The checks, their problems, references and gates: tests/loop_checks.py;
tests/test_gpu_loop.py runs the same ones on the GPU."""
import contextlib

import pytest
import torch

import loop_checks as C
from emu.harness import emulated
from test_emu_parity import LOOP_FORMS


class Env:
    dev = torch.device("cpu")

    @staticmethod
    @contextlib.contextmanager
    def run(variant=0):
        with emulated(256, variant):
            yield


ENV = Env()
CASES = C.EMU_CASES
IDS = [C.tag(s, f) for s, f in CASES]


def test_the_forms_are_the_parity_tests_forms():
    assert C.LOOP_FORMS == LOOP_FORMS


@pytest.mark.parametrize("shape,form", CASES, ids=IDS)
def test_iterates_after_k_iterations(shape, form):
    C.check_iterates_after_k(ENV, shape, form)


@pytest.mark.parametrize("shape,form", CASES, ids=IDS)
def test_iteration_counts_and_trace(shape, form):
    C.check_counts_and_trace(ENV, shape, form)


@pytest.mark.parametrize("shape,form", CASES, ids=IDS)
def test_best_iterate_bookkeeping(shape, form):
    C.check_best_iterate(ENV, shape, form)


@pytest.mark.parametrize("shape,form", CASES, ids=IDS)
def test_stall_policy_0_runs_to_max_iter(shape, form):
    C.check_no_stall_counter(ENV, shape, form)


@pytest.mark.parametrize("shape", C.SHAPES + [C.BIG], ids=lambda s: C.tag(s))
def test_iteration_counts_at_the_default_eps_are_recorded(shape):
    C.record_counts(ENV, shape)


@pytest.mark.parametrize("shape", C.WIDE_SHAPES, ids=lambda s: C.tag(s))
def test_float32_tensors_in_float64_arithmetic(shape):
    C.check_wide_iterates(ENV, shape)
