"""-m gpu: the KKT-solve kernels on a real MI355X, through libqpx_hip.so: the checks of tests/test_emu_kkt.py
(tests/kkt_checks.py), same problems, references and gates, at every (shape, form) case -- where MFMA tile layouts, DPP
reductions, LDS aliasing and the wave roles are the real ones -- and the one-wave form that the default dispatch picks beyond
512 QPs.  Batches of three QPs (520 small ones in the one-wave case)."""
import contextlib

import pytest
import torch

import kkt_checks as C
from multi_reference import KNOB_FORMS

pytestmark = pytest.mark.gpu
IDS = [C.tag(s, f) for s, f in C.CASES]


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


def test_the_forms_are_the_knobs_forms():
    assert C.FORMS == (0,) + tuple(KNOB_FORMS)


@pytest.mark.parametrize("shape,form", C.CASES, ids=IDS)
def test_solve(env, shape, form):
    C.check_solve(env, shape, form)


@pytest.mark.parametrize("shape,form", C.CASES, ids=IDS)
def test_backward_with_duals_cotangents(env, shape, form):
    C.check_backward(env, shape, form)


@pytest.mark.parametrize("shape,form", C.CASES, ids=IDS)
def test_forward_mode_and_the_adjoint_identity(env, shape, form):
    C.check_jvp(env, shape, form)


@pytest.mark.parametrize("shape,form", C.CASES, ids=IDS)
def test_k_right_hand_sides(env, shape, form):
    C.check_multi(env, shape, form)


@pytest.mark.parametrize("shape,form", C.CASES, ids=IDS)
def test_k1_of_the_multi_solve_against_the_single_solve(env, shape, form):
    """bitwise: the dispatcher hands K = 1 to the single solve's kernel (tests/kkt_checks.py, check 4)"""
    C.check_multi_k1(env, shape, form)


@pytest.mark.parametrize("shape", C.SHARED_SHAPES, ids=lambda s: C.tag(s))
def test_k1_of_the_multi_solve_against_the_single_solve_shared_factors(env, shape):
    C.check_multi_k1(env, shape, 0, prob="shared")


def test_k1_of_the_multi_solve_against_the_single_solve_beyond_512_qps(env):
    C.check_multi_k1(env, C.ONE_WAVE_SHAPE, 0, B=C.ONE_WAVE_B)


@pytest.mark.parametrize("shape,form", C.CASES, ids=IDS)
def test_second_order_pass(env, shape, form):
    C.check_backward2(env, shape, form)


def test_one_wave_form_beyond_512_qps(env):
    C.check_one_wave_beyond_512(env)


@pytest.mark.parametrize("shape", C.SHARED_SHAPES, ids=lambda s: C.tag(s))
def test_shared_factors_equal_the_expanded_batch_bitwise(env, shape):
    C.check_shared_factors(env, shape)


@pytest.mark.parametrize("shape", C.F32_SHAPES, ids=lambda s: C.tag(s))
def test_float32_thread_grid_kernels(env, shape):
    C.check_f32_grid(env, shape)


@pytest.mark.parametrize("shape", C.WIDE_SHAPES, ids=lambda s: C.tag(s))
def test_float32_tensors_in_float64_arithmetic(env, shape):
    C.check_wide(env, shape)
