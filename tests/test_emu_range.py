"""Two-sided inequality rows (QPFunction(...)(Q, p, G, h, A, b, lower=l), KKTFactors.ipm_range / backward_range, qpx_ipm_range;
DESIGN 4.11) on the host-thread emulator: the range role of every loop form the default dispatch picks -- tile forms of one,
two, four and seven tile rows, one wave and chain-wave, the thread-grid forms of 10 and 13 blocks -- and of the backward, run
by host threads.  The checks, their problems, references and gates: tests/range_checks.py; tests/test_gpu_range.py runs the
same ones on the GPU."""
import contextlib

import pytest
import torch

import range_checks as C
import range_reference as R
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


@pytest.mark.parametrize("label,sides", CASES)
def test_reference_on_the_doubled_qp(label, sides):
    C.check_reference_parity(ENV, label, sides)


@pytest.mark.parametrize("label,sides", [c for c in CASES if c[0] in R.COUNTED])
def test_iteration_counts_of_the_doubled_qp(label, sides):
    C.check_iteration_counts(ENV, label, sides)


def test_trace_dual_resid_is_the_doubled_qps():
    C.check_trace_dual_resid(ENV)


@pytest.mark.parametrize("label", ["t1b", "t2", "t4", "c4", "box", "g10"])
def test_iterates_after_k_iterations_are_the_doubled_qps(label):
    C.check_iterates_after_k(ENV, label, "half")


@pytest.mark.parametrize("label", ["t1b", "t4", "c4", "box", "g10"])
def test_lower_minus_inf_is_the_six_input_call(label):
    C.check_one_sided_equivalence(ENV, label)


def test_closed_form_of_the_box():
    C.check_closed_form(ENV)


def test_gradcheck_over_seven_inputs():
    C.check_gradcheck(ENV)


def test_adjoint_identity_against_the_doubled_forward_mode():
    C.check_adjoint_identity(ENV)


def test_shared_lower_reductions():
    C.check_lower_reductions(ENV)


def test_abi_codes_and_range_supported():
    C.check_abi_codes(ENV)


def test_bad_lower():
    C.check_bad_lower(ENV, pytest)


def test_refusals():
    C.check_refusals(ENV, pytest)


def test_lower_none_is_the_six_input_call():
    C.check_lower_none_is_the_six_input_call(ENV)

# four tile rows with ONE wave per QP: what the default dispatch picks there beyond 512 QPs, reached through the A/B knob
@pytest.mark.parametrize("sides", R.SIDES)
def test_four_tile_rows_one_wave_reference(sides):
    C.check_reference_parity(ENV, "t4", sides, C.ONE_WAVE)


@pytest.mark.parametrize("sides", R.SIDES)
def test_four_tile_rows_one_wave_iteration_counts(sides):
    C.check_iteration_counts(ENV, "t4", sides, C.ONE_WAVE)


def test_four_tile_rows_one_wave_lower_minus_inf():
    C.check_one_sided_equivalence(ENV, "t4", C.ONE_WAVE)


@pytest.mark.parametrize("key", list(C.SLOT_SHAPES))
def test_slot_counts_against_the_doubled_call(key):
    C.check_doubled_call(ENV, key)


def test_four_tile_rows_one_wave_many_slots_against_the_doubled_call():
    C.check_doubled_call(ENV, "s44", "all", C.ONE_WAVE)


def test_four_tile_rows_one_wave_two_slots_reference():
    C.check_reference_parity(ENV, "c4", "all", C.ONE_WAVE)
