"""Warm start and K-right-hand-side sensitivities of two-sided rows (KKTFactors.ipm_range(warm=...), qpx_ipm_range_warm,
QPFunction(warm_start=RangeWarmStart())(..., lower=l), sensitivity.solve(..., lower=l)) on the host-thread
emulator: the warm entry of the range role of every loop form the default dispatch picks, run by host threads.  The checks,
their problems, references and gates: tests/range_warm_checks.py; tests/test_gpu_range_warm.py runs the same ones on the GPU."""
import contextlib

import pytest
import torch

import range_checks as C
import range_reference as R
import range_warm_checks as RW
from emu.harness import emulated


class Env:
    dev = torch.device("cpu")

    @staticmethod
    @contextlib.contextmanager
    def run(variant=0):
        with emulated(256, variant):
            yield


ENV = Env()
CASES = [(label, sides) for label in R.SHAPES for sides in R.SIDES]
FORMS = [("t1b", 0), ("t4", C.ONE_WAVE), ("c4", 0), ("box", 0), ("g10", 0)]       # one-wave, chain-wave and thread-grid forms


def test_reference_alone():
    RW.check_reference_alone()


@pytest.mark.parametrize("label,sides", CASES)
def test_every_form(label, sides):
    RW.check_every_form(ENV, label, sides)


@pytest.mark.parametrize("label", ["t4", "c4"])
@pytest.mark.parametrize("sides", R.SIDES)
def test_every_form_one_wave(label, sides):
    RW.check_every_form(ENV, label, sides, C.ONE_WAVE)


@pytest.mark.parametrize("label,variant", FORMS + [("t4", 0)])
def test_lower_minus_inf_is_ipm_warm(label, variant):
    RW.check_one_sided_equivalence(ENV, label, variant)


@pytest.mark.parametrize("sides", R.SIDES)
@pytest.mark.parametrize("label,variant", FORMS)
def test_entry_state(label, variant, sides):
    RW.check_entry_state(ENV, label, sides, variant)


@pytest.mark.parametrize("label,variant", FORMS)
def test_per_qp_fallback(label, variant):
    RW.check_per_qp_fallback(ENV, label, variant)


def test_abi():
    RW.check_abi(ENV)


def test_qpfunction_three_step_loop():
    RW.check_qpfunction_loop(ENV)


def test_a_holder_of_another_batch_is_ignored_and_overwritten():
    RW.check_holder_of_another_batch(ENV)


def test_refusals():
    RW.check_refusals(ENV, pytest)


@pytest.mark.parametrize("label,sides", [c for c in CASES if c[0] in R.COUNTED])
def test_sensitivity_against_the_doubled_qp(label, sides):
    RW.check_sensitivity(ENV, label, sides)


def test_jacobian_z_lower_against_backward_calls():
    RW.check_jacobian_against_backward_calls(ENV)
