"""Elastic inequality rows (QPFunction(...)(Q, p, G, h, A, b, rho, l1=gamma), KKTFactors.ipm_elastic, qpx_ipm_elastic)
on the host-thread emulator: the elastic role of every loop form the default dispatch picks -- tile forms of one, two, four
and seven tile rows, one wave and chain-wave, the thread-grid forms of 10 and 13 blocks -- run by host threads.  The checks,
their problems, references and gates: tests/elastic_checks.py; tests/test_gpu_elastic.py runs the same ones on the GPU."""
import contextlib

import pytest
import torch

import elastic_checks as C
import elastic_reference as R
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


@pytest.mark.parametrize("label,kind", CASES)
def test_reference_on_the_augmented_qp(label, kind):
    C.check_reference_parity(ENV, label, kind)


@pytest.mark.parametrize("label,kind", CASES)
def test_iteration_counts_of_the_augmented_qp(label, kind):
    C.check_iteration_counts(ENV, label, kind, gated=label in R.COUNTED)


@pytest.mark.parametrize("label,kind", C.TRACED)
def test_trace_is_the_augmented_qps(label, kind):
    C.check_trace(ENV, label, kind)


@pytest.mark.parametrize("label", ["t1b", "c4"])
def test_exact_penalty_recovers_the_hard_qp(label):
    C.check_exactness(ENV, label)


@pytest.mark.parametrize("label", ["t1b", "t4", "c4", "c7", "g10"])
def test_l1_inf_is_the_six_input_call(label):
    C.check_hard_rows(ENV, label)


def test_l1_zero_is_the_soft_call():
    C.check_gamma_zero(ENV)


def test_closed_form():
    C.check_closed_form(ENV)


def test_gradcheck_over_eight_inputs():
    C.check_gradcheck(ENV)


def test_adjoint_identity_of_reverse_and_forward_mode():
    C.check_adjoint_identity(ENV)


def test_duals_cotangents_against_the_reference_solve():
    C.check_duals(ENV)


def test_shared_and_scalar_reductions():
    C.check_reductions(ENV)


def test_abi_codes_and_elastic_supported():
    C.check_abi_codes(ENV)


def test_bad_entries():
    C.check_bad_entries(ENV, pytest)


def test_refusals():
    C.check_refusals(ENV, pytest)


def test_l1_none_is_the_old_call():
    C.check_l1_none_is_the_old_call(ENV)


# four tile rows with ONE wave per QP: what the default dispatch picks there beyond 512 QPs, reached through the A/B knob
@pytest.mark.parametrize("kind", R.KINDS)
def test_four_tile_rows_one_wave_reference(kind):
    C.check_reference_parity(ENV, "t4", kind, C.ONE_WAVE)


@pytest.mark.parametrize("kind", R.KINDS)
def test_four_tile_rows_one_wave_iteration_counts(kind):
    C.check_iteration_counts(ENV, "t4", kind, C.ONE_WAVE)


def test_four_tile_rows_one_wave_l1_inf():
    C.check_hard_rows(ENV, "t4", C.ONE_WAVE)


@pytest.mark.parametrize("key", list(C.SLOT_SHAPES))
def test_slot_counts_against_the_augmented_call(key):
    C.check_augmented_call(ENV, key)


def test_four_tile_rows_one_wave_many_slots_against_the_augmented_call():
    C.check_augmented_call(ENV, "s44", "all", C.ONE_WAVE)


def test_four_tile_rows_one_wave_two_slots_reference():
    C.check_reference_parity(ENV, "c4", "all", C.ONE_WAVE)
