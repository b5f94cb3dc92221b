"""-m gpu: soft two-sided inequality rows (QPFunction(...)(Q, p, G, h, A, b, soft_range=SoftRange(...)), qpx_ipm_soft_range;
DESIGN 4.13) on a real MI355X, through libqpx_hip.so: the checks of tests/test_emu_soft_range.py (tests/soft_range_checks.py),
same problems, references and gates -- every shape with the row kinds mixed, the headline shape and the four-row one-wave
form with every row soft.  Batches of one or two QPs; a few seconds in all."""
import contextlib

import pytest
import torch

import soft_range_checks as C
import soft_range_reference as R

pytestmark = pytest.mark.gpu
CASES = [(label, "mixed") for label in R.SHAPES] + [("c7", "all"), ("t4", "all")]
ROLE_SHAPES = ["t1b", "c4", "c7"]


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


@pytest.mark.parametrize("label", ROLE_SHAPES)
def test_hard_sides_are_the_lower_call(env, label):
    C.check_hard_sides_are_the_range_call(env, label)


def test_rho_inf_beside_a_finite_l1_is_a_hard_side(env):
    C.check_hard_sides_are_the_range_call(env, "t1b", penalties=C.HARD_BY_RHO)


@pytest.mark.parametrize("label", ROLE_SHAPES)
def test_no_lower_is_the_l1_call(env, label):
    C.check_no_lower_is_the_elastic_call(env, label)


@pytest.mark.parametrize("label", ROLE_SHAPES)
def test_hard_one_sided_is_the_six_input_call(env, label):
    C.check_hard_one_sided_is_the_six_input_call(env, label)


def test_exact_penalty_recovers_the_hard_range_qp(env):
    C.check_exactness(env, "t1b")


def test_gradcheck_over_eleven_inputs(env):
    C.check_gradcheck(env)


@pytest.mark.parametrize("key", list(C.SLOT_SHAPES))
def test_slot_counts_against_the_augmented_call(env, key):
    C.check_augmented_call(env, key)


def test_abi_codes_and_soft_range_supported(env):
    C.check_abi_codes(env)


def test_bad_entries(env):
    C.check_bad_entries(env, pytest)


def test_refusals(env):
    C.check_refusals(env, pytest)


def test_shared_and_scalar_reductions(env):
    C.check_reductions(env)


def test_soft_range_none_is_the_old_call(env):
    C.check_none_is_the_old_call(env)


# four tile rows with ONE wave per QP: what the default dispatch picks there beyond 512 QPs, reached through the A/B knob
def test_four_tile_rows_one_wave_reference(env):
    C.check_reference_parity(env, "t4", "mixed", C.ONE_WAVE)
