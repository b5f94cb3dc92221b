"""-m gpu: two-sided inequality rows (QPFunction(...)(Q, p, G, h, A, b, lower=l), qpx_ipm_range, qpx_backward_range; DESIGN
4.11) on a real MI355X, through libqpx_hip.so: the checks of tests/test_emu_range.py (tests/range_checks.py), same problems,
references and gates.  Batches of two or three QPs; a few seconds in all."""
import contextlib

import pytest
import torch

import range_checks as C
import range_reference as R

pytestmark = pytest.mark.gpu
CASES = [(label, sides) for label in R.SHAPES for sides in R.SIDES]


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


@pytest.mark.parametrize("label,sides", CASES)
def test_reference_on_the_doubled_qp(env, label, sides):
    C.check_reference_parity(env, label, sides)


@pytest.mark.parametrize("label,sides", [c for c in CASES if c[0] in R.COUNTED])
def test_iteration_counts_of_the_doubled_qp(env, label, sides):
    C.check_iteration_counts(env, label, sides)


def test_trace_dual_resid_is_the_doubled_qps(env):
    C.check_trace_dual_resid(env)


@pytest.mark.parametrize("label", ["t1b", "t2", "t4", "c4", "box", "g10"])
def test_iterates_after_k_iterations_are_the_doubled_qps(env, label):
    C.check_iterates_after_k(env, label, "half")


@pytest.mark.parametrize("label", ["t1b", "t4", "c4", "box", "g10"])
def test_lower_minus_inf_is_the_six_input_call(env, label):
    C.check_one_sided_equivalence(env, label)


def test_closed_form_of_the_box(env):
    C.check_closed_form(env)


def test_gradcheck_over_seven_inputs(env):
    C.check_gradcheck(env)


def test_adjoint_identity_against_the_doubled_forward_mode(env):
    C.check_adjoint_identity(env)


def test_shared_lower_reductions(env):
    C.check_lower_reductions(env)


def test_abi_codes_and_range_supported(env):
    C.check_abi_codes(env)


def test_bad_lower(env):
    C.check_bad_lower(env, pytest)


def test_refusals(env):
    C.check_refusals(env, pytest)


def test_lower_none_is_the_six_input_call(env):
    C.check_lower_none_is_the_six_input_call(env)

# four tile rows with ONE wave per QP: what the default dispatch picks there beyond 512 QPs, reached through the A/B knob
@pytest.mark.parametrize("sides", R.SIDES)
def test_four_tile_rows_one_wave_reference(env, sides):
    C.check_reference_parity(env, "t4", sides, C.ONE_WAVE)


@pytest.mark.parametrize("sides", R.SIDES)
def test_four_tile_rows_one_wave_iteration_counts(env, sides):
    C.check_iteration_counts(env, "t4", sides, C.ONE_WAVE)


def test_four_tile_rows_one_wave_lower_minus_inf(env):
    C.check_one_sided_equivalence(env, "t4", C.ONE_WAVE)


@pytest.mark.parametrize("key", list(C.SLOT_SHAPES))
def test_slot_counts_against_the_doubled_call(env, key):
    C.check_doubled_call(env, key)


def test_four_tile_rows_one_wave_many_slots_against_the_doubled_call(env):
    C.check_doubled_call(env, "s44", "all", C.ONE_WAVE)


def test_four_tile_rows_one_wave_two_slots_reference(env):
    C.check_reference_parity(env, "c4", "all", C.ONE_WAVE)
