"""Soft two-sided inequality rows (QPFunction(...)(Q, p, G, h, A, b, soft_range=SoftRange(...)), KKTFactors.ipm_soft_range,
qpx_ipm_soft_range) on the host-thread emulator: the soft-range role of every loop form the default dispatch picks
-- tile forms of one, two, four and seven tile rows, one wave and chain-wave, the thread-grid forms of 10 and 13 blocks -- run
by host threads.  The checks, their problems, references and gates: tests/soft_range_checks.py;
tests/test_gpu_soft_range.py runs them on the GPU."""
import contextlib

import pytest
import torch

import soft_range_checks as C
import soft_range_reference as R
from emu.harness import emulated


class Env:
    dev = torch.device("cpu")

    @staticmethod
    @contextlib.contextmanager
    def run(variant=0):
        with emulated(256, variant):
            yield


ENV = Env()
CASES = [(label, kind) for label in R.SHAPES for kind in R.KINDS]
ROLE_SHAPES = ["t1b", "c4", "c7"]


@pytest.mark.parametrize("label,kind", CASES)
def test_reference_on_the_augmented_qp(label, kind):
    C.check_reference_parity(ENV, label, kind)


@pytest.mark.parametrize("label,kind", CASES)
def test_iteration_counts_of_the_augmented_qp(label, kind):
    C.check_iteration_counts(ENV, label, kind, gated=label in R.COUNTED)


@pytest.mark.parametrize("label,kind", C.TRACED + C.TRACED_OTHER_KIND)
def test_trace_is_the_augmented_qps(label, kind):
    C.check_trace(ENV, label, kind)


@pytest.mark.parametrize("label", ROLE_SHAPES)
def test_hard_sides_are_the_lower_call(label):
    C.check_hard_sides_are_the_range_call(ENV, label)


@pytest.mark.parametrize("label", ["t1b", "c7"])
def test_rho_inf_beside_a_finite_l1_is_a_hard_side(label):
    C.check_hard_sides_are_the_range_call(ENV, label, penalties=C.HARD_BY_RHO)


@pytest.mark.parametrize("label", ROLE_SHAPES)
def test_no_lower_is_the_l1_call(label):
    C.check_no_lower_is_the_elastic_call(ENV, label)


@pytest.mark.parametrize("label", ROLE_SHAPES)
def test_hard_one_sided_is_the_six_input_call(label):
    C.check_hard_one_sided_is_the_six_input_call(ENV, label)


@pytest.mark.parametrize("label", ["t1b", "c4"])
def test_exact_penalty_recovers_the_hard_range_qp(label):
    C.check_exactness(ENV, label)


def test_gradcheck_over_eleven_inputs():
    C.check_gradcheck(ENV)


@pytest.mark.parametrize("key", list(C.SLOT_SHAPES))
def test_slot_counts_against_the_augmented_call(key):
    C.check_augmented_call(ENV, key)


def test_abi_codes_and_soft_range_supported():
    C.check_abi_codes(ENV)


def test_bad_entries():
    C.check_bad_entries(ENV, pytest)


def test_refusals():
    C.check_refusals(ENV, pytest)


def test_shared_and_scalar_reductions():
    C.check_reductions(ENV)


def test_soft_range_none_is_the_old_call():
    C.check_none_is_the_old_call(ENV)


# four tile rows with ONE wave per QP: what the default dispatch picks there beyond 512 QPs, reached through the A/B knob
@pytest.mark.parametrize("kind", R.KINDS)
def test_four_tile_rows_one_wave_reference(kind):
    C.check_reference_parity(ENV, "t4", kind, C.ONE_WAVE)


@pytest.mark.parametrize("kind", R.KINDS)
def test_four_tile_rows_one_wave_iteration_counts(kind):
    C.check_iteration_counts(ENV, "t4", kind, C.ONE_WAVE)
