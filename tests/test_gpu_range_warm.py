"""-m gpu: warm start and K-right-hand-side sensitivities of two-sided rows (KKTFactors.ipm_range(warm=...), qpx_ipm_range_warm,
QPFunction(warm_start=RangeWarmStart())(..., lower=l), sensitivity.solve(..., lower=l)) on a real MI355X, through
libqpx_hip.so: the checks of tests/test_emu_range_warm.py (tests/range_warm_checks.py), same problems, references and gates.
Batches of two or four QPs; the dense numpy references are the larger part of the run time."""
import contextlib

import pytest
import torch

import range_checks as C
import range_reference as R
import range_warm_checks as RW

pytestmark = pytest.mark.gpu
CASES = [(label, sides) for label in R.SHAPES for sides in R.SIDES]
FORMS = [("t1b", 0), ("t4", C.ONE_WAVE), ("c4", 0), ("box", 0), ("g10", 0)]       # one-wave, chain-wave and thread-grid forms


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
def test_every_form(env, label, sides):
    RW.check_every_form(env, label, sides)


@pytest.mark.parametrize("label", ["t4", "c4"])
@pytest.mark.parametrize("sides", R.SIDES)
def test_every_form_one_wave(env, label, sides):
    RW.check_every_form(env, label, sides, C.ONE_WAVE)


@pytest.mark.parametrize("label,variant", FORMS + [("t4", 0)])
def test_lower_minus_inf_is_ipm_warm(env, label, variant):
    RW.check_one_sided_equivalence(env, label, variant)


@pytest.mark.parametrize("sides", R.SIDES)
@pytest.mark.parametrize("label,variant", FORMS)
def test_entry_state(env, label, variant, sides):
    RW.check_entry_state(env, label, sides, variant)


@pytest.mark.parametrize("label,variant", FORMS)
def test_per_qp_fallback(env, label, variant):
    RW.check_per_qp_fallback(env, label, variant)


def test_abi(env):
    RW.check_abi(env)


def test_qpfunction_three_step_loop(env):
    RW.check_qpfunction_loop(env)


def test_a_holder_of_another_batch_is_ignored_and_overwritten(env):
    RW.check_holder_of_another_batch(env)


def test_refusals(env):
    RW.check_refusals(env, pytest)


@pytest.mark.parametrize("label,sides", [c for c in CASES if c[0] in R.COUNTED])
def test_sensitivity_against_the_doubled_qp(env, label, sides):
    RW.check_sensitivity(env, label, sides)


def test_jacobian_z_lower_against_backward_calls(env):
    RW.check_jacobian_against_backward_calls(env)
