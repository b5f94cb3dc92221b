"""The KKT-solve kernels on the host-thread emulator: the plain solve, the backward with its duals cotangents, forward mode, K
right-hand sides and the second-order pass of every form the A/B knob reaches, against a dense solve refined in extended
precision.  The checks, their problems, references and gates: tests/kkt_checks.py; tests/test_gpu_kkt.py runs the same ones
on the GPU (and the one-wave form beyond 512 QPs, which is too long for fibres)."""
import contextlib

import pytest
import torch

import kkt_checks as C
from emu.harness import emulated
from test_emu_jvp import FORMS


class Env:
    dev = torch.device("cpu")

    @staticmethod
    @contextlib.contextmanager
    def run(variant=0):
        with emulated(256, variant):
            yield


ENV = Env()
CASES = C.EMU_CASES
IDS = [C.tag(s, f) for s, f in CASES]


def test_the_forms_are_the_knobs_forms():
    from qpth_amd.kkt import MULTI_RHS_BLOCK
    assert list(C.FORMS) == [0] + FORMS
    assert C.multi_ks() == (1, MULTI_RHS_BLOCK + 1, 2 * MULTI_RHS_BLOCK + 3)


@pytest.mark.parametrize("shape,form", CASES, ids=IDS)
def test_solve(shape, form):
    C.check_solve(ENV, shape, form)


@pytest.mark.parametrize("shape,form", CASES, ids=IDS)
def test_backward_with_duals_cotangents(shape, form):
    C.check_backward(ENV, shape, form)


@pytest.mark.parametrize("shape,form", CASES, ids=IDS)
def test_forward_mode_and_the_adjoint_identity(shape, form):
    C.check_jvp(ENV, shape, form)


@pytest.mark.parametrize("shape,form", CASES, ids=IDS)
def test_k_right_hand_sides(shape, form):
    C.check_multi(ENV, shape, form)


@pytest.mark.parametrize("shape,form", CASES, ids=IDS)
def test_k1_of_the_multi_solve_against_the_single_solve(shape, form):
    """bitwise: the dispatcher hands K = 1 to the single solve's kernel (tests/kkt_checks.py, check 4)"""
    C.check_multi_k1(ENV, shape, form)


@pytest.mark.parametrize("shape", C.SHARED_SHAPES, ids=lambda s: C.tag(s))
def test_k1_of_the_multi_solve_against_the_single_solve_shared_factors(shape):
    C.check_multi_k1(ENV, shape, 0, prob="shared")


@pytest.mark.parametrize("shape,form", CASES, ids=IDS)
def test_second_order_pass(shape, form):
    C.check_backward2(ENV, shape, form)


@pytest.mark.parametrize("shape", C.SHARED_SHAPES, ids=lambda s: C.tag(s))
def test_shared_factors_equal_the_expanded_batch_bitwise(shape):
    C.check_shared_factors(ENV, shape)


@pytest.mark.parametrize("shape", C.F32_SHAPES, ids=lambda s: C.tag(s))
def test_float32_thread_grid_kernels(shape):
    C.check_f32_grid(ENV, shape)


@pytest.mark.parametrize("shape", C.WIDE_SHAPES, ids=lambda s: C.tag(s))
def test_float32_tensors_in_float64_arithmetic(shape):
    C.check_wide(ENV, shape)
