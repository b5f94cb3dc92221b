"""-m gpu: elastic inequality rows (QPFunction(...)(Q, p, G, h, A, b, rho, l1=gamma), qpx_ipm_elastic) on a real
MI355X, through libqpx_hip.so: the checks of tests/test_emu_elastic.py (tests/elastic_checks.py), same problems, references
and gates.  Batches of one or two QPs; a few seconds in all."""
import contextlib

import pytest
import torch

import elastic_checks as C
import elastic_reference as R

pytestmark = pytest.mark.gpu
CASES = [(label, kind) for label in R.SHAPES for kind in R.KINDS]


class Env:
    def __init__(self):
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from qpth_amd import _lib
        self.lib = _lib.hip()                   # the HIP extension must be the thing that runs
        assert _lib._TEST_BACKEND is None
        self.dev = torch.device("cuda:0")

    @contextlib.contextmanager
    def run(self, variant=0):
        old = self.lib.dll.qpx_set_ipm_variant(int(variant))
        try:
            yield
        finally:
            self.lib.dll.qpx_set_ipm_variant(old)


@pytest.fixture(scope="module")
def env():
    return Env()


@pytest.mark.parametrize("label,kind", CASES)
def test_reference_on_the_augmented_qp(env, label, kind):
    C.check_reference_parity(env, label, kind)


@pytest.mark.parametrize("label,kind", CASES)
def test_iteration_counts_of_the_augmented_qp(env, label, kind):
    C.check_iteration_counts(env, label, kind, gated=label in R.COUNTED)


@pytest.mark.parametrize("label,kind", C.TRACED)
def test_trace_is_the_augmented_qps(env, label, kind):
    C.check_trace(env, label, kind)


@pytest.mark.parametrize("label", ["t1b", "c4"])
def test_exact_penalty_recovers_the_hard_qp(env, label):
    C.check_exactness(env, label)


@pytest.mark.parametrize("label", ["t1b", "t4", "c4", "c7", "g10"])
def test_l1_inf_is_the_six_input_call(env, label):
    C.check_hard_rows(env, label)


def test_l1_zero_is_the_soft_call(env):
    C.check_gamma_zero(env)


def test_closed_form(env):
    C.check_closed_form(env)


def test_gradcheck_over_eight_inputs(env):
    C.check_gradcheck(env)


def test_adjoint_identity_of_reverse_and_forward_mode(env):
    C.check_adjoint_identity(env)


def test_duals_cotangents_against_the_reference_solve(env):
    C.check_duals(env)


def test_shared_and_scalar_reductions(env):
    C.check_reductions(env)


def test_abi_codes_and_elastic_supported(env):
    C.check_abi_codes(env)


def test_bad_entries(env):
    C.check_bad_entries(env, pytest)


def test_refusals(env):
    C.check_refusals(env, pytest)


def test_l1_none_is_the_old_call(env):
    C.check_l1_none_is_the_old_call(env)


# four tile rows with ONE wave per QP: what the default dispatch picks there beyond 512 QPs, reached through the A/B knob
@pytest.mark.parametrize("kind", R.KINDS)
def test_four_tile_rows_one_wave_reference(env, kind):
    C.check_reference_parity(env, "t4", kind, C.ONE_WAVE)


@pytest.mark.parametrize("kind", R.KINDS)
def test_four_tile_rows_one_wave_iteration_counts(env, kind):
    C.check_iteration_counts(env, "t4", kind, C.ONE_WAVE)


def test_four_tile_rows_one_wave_l1_inf(env):
    C.check_hard_rows(env, "t4", C.ONE_WAVE)


@pytest.mark.parametrize("key", list(C.SLOT_SHAPES))
def test_slot_counts_against_the_augmented_call(env, key):
    C.check_augmented_call(env, key)


def test_four_tile_rows_one_wave_many_slots_against_the_augmented_call(env):
    C.check_augmented_call(env, "s44", "all", C.ONE_WAVE)


def test_four_tile_rows_one_wave_two_slots_reference(env):
    C.check_reference_parity(env, "c4", "all", C.ONE_WAVE)
