"""-m gpu: soft inequality rows (QPFunction(...)(Q, p, G, h, A, b, rho), qpx_pre_factor_soft) on a real MI355X,
through libqpx_hip.so: the checks of tests/test_emu_soft.py (tests/soft_checks.py), same problems, references and gates.
Batches of two or three QPs; a few seconds in all."""
import contextlib

import pytest
import torch

import soft_checks as C

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("label", list(C.CASES))
def test_zero_w_leaves_the_blob_of_pre_factor(env, label):
    C.check_zero_w_blob(env, label)


def test_rho_none_is_the_six_input_call(env):
    C.check_rho_none_is_the_six_input_call(env)


def test_per_qp_w_on_shared_matrices_means_one_blob_per_qp(env):
    C.check_per_qp_w_on_shared_matrices(env)


@pytest.mark.parametrize("label", list(C.CASES))
def test_kkt_solve_equals_the_hard_solve_with_shifted_d(env, label):
    C.check_kkt_equivalence(env, label)


@pytest.mark.parametrize("label", ["a", "b0", "b1", "d", "e"])
def test_reference_on_the_augmented_qp(env, label):
    C.check_reference_parity(env, label)


@pytest.mark.parametrize("label", ["a", "b0", "b1"])
def test_stop_rule_of_the_augmented_qp(env, label):
    C.check_stop_rule(env, label)


def test_adjoint_identity_over_seven_inputs(env):
    C.check_adjoint_identity(env)


def test_gradcheck_over_seven_inputs(env):
    C.check_gradcheck(env)


def test_shared_and_scalar_rho_reductions(env):
    C.check_rho_reductions(env)


def test_infeasible_box(env):
    C.check_infeasible_box(env)


def test_duals_and_warm_start(env):
    C.check_warm_start(env)


def test_sensitivity_solve_with_rho(env):
    C.check_sensitivity(env)


def test_errors(env):
    C.check_errors(env, pytest)


def test_refinement_is_refused_on_soft_factors(env):
    C.check_refinement_is_refused_on_soft_factors(env, pytest)
