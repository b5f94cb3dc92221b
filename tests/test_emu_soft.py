"""Soft inequality rows (QPFunction(...)(Q, p, G, h, A, b, rho), KKTFactors.build(w=...), qpx_pre_factor_soft) on
the host-thread emulator: the kernel bodies of all three pre-factorisation paths -- the sweep, the matrix-core form, the
large-QP launch sequence -- run by host threads.  The checks, their problems, references and gates: tests/soft_checks.py;
tests/test_gpu_soft.py runs the same ones on the GPU."""
import contextlib

import pytest
import torch

import soft_checks as C
from emu.harness import emulated


class Env:
    dev = torch.device("cpu")

    @staticmethod
    @contextlib.contextmanager
    def run(variant=0):
        with emulated(256, variant):
            yield


ENV = Env()


@pytest.mark.parametrize("label", list(C.CASES))
def test_zero_w_leaves_the_blob_of_pre_factor(label):
    C.check_zero_w_blob(ENV, label)


def test_rho_none_is_the_six_input_call():
    C.check_rho_none_is_the_six_input_call(ENV)


def test_per_qp_w_on_shared_matrices_means_one_blob_per_qp():
    C.check_per_qp_w_on_shared_matrices(ENV)


@pytest.mark.parametrize("label", list(C.CASES))
def test_kkt_solve_equals_the_hard_solve_with_shifted_d(label):
    C.check_kkt_equivalence(ENV, label)


@pytest.mark.parametrize("label", ["a", "b0", "b1", "d", "e"])
def test_reference_on_the_augmented_qp(label):
    C.check_reference_parity(ENV, label)


@pytest.mark.parametrize("label", ["a", "b0", "b1"])
def test_stop_rule_of_the_augmented_qp(label):
    C.check_stop_rule(ENV, label)


def test_adjoint_identity_over_seven_inputs():
    C.check_adjoint_identity(ENV)


def test_gradcheck_over_seven_inputs():
    C.check_gradcheck(ENV)


def test_shared_and_scalar_rho_reductions():
    C.check_rho_reductions(ENV)


def test_infeasible_box():
    C.check_infeasible_box(ENV)


def test_duals_and_warm_start():
    C.check_warm_start(ENV)


def test_sensitivity_solve_with_rho():
    C.check_sensitivity(ENV)


def test_errors():
    C.check_errors(ENV, pytest)


def test_refinement_is_refused_on_soft_factors():
    C.check_refinement_is_refused_on_soft_factors(ENV, pytest)
