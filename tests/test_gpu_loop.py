"""-m gpu: the path of the hard-QP interior-point loop (KKTFactors.ipm, qpx_ipm) on a real MI355X, through libqpx_hip.so: the
checks of tests/test_emu_loop.py (tests/loop_checks.py), same problems, references and gates -- where MFMA tile layouts, DPP
reductions, LDS aliasing and the chain wave are the real ones -- and the one-wave form that the default dispatch picks
beyond 512 QPs.  Batches of two or three QPs (520 small ones in the one-wave case); a few seconds in all."""
import contextlib

import pytest
import torch

import loop_checks as C
from test_gpu_parity import LOOP_FORMS

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


def test_the_forms_are_the_parity_tests_forms():
    assert C.LOOP_FORMS == LOOP_FORMS


@pytest.mark.parametrize("shape,form", C.CASES, ids=IDS)
def test_iterates_after_k_iterations(env, shape, form):
    C.check_iterates_after_k(env, shape, form)


@pytest.mark.parametrize("shape,form", C.CASES, ids=IDS)
def test_iteration_counts_and_trace(env, shape, form):
    C.check_counts_and_trace(env, shape, form)


@pytest.mark.parametrize("shape,form", C.CASES, ids=IDS)
def test_best_iterate_bookkeeping(env, shape, form):
    C.check_best_iterate(env, shape, form)


@pytest.mark.parametrize("shape,form", C.CASES, ids=IDS)
def test_stall_policy_0_runs_to_max_iter(env, shape, form):
    C.check_no_stall_counter(env, shape, form)


@pytest.mark.parametrize("shape", C.SHAPES + [C.BIG], ids=lambda s: C.tag(s))
def test_iteration_counts_at_the_default_eps_are_recorded(env, shape):
    C.record_counts(env, shape)


@pytest.mark.parametrize("shape", C.WIDE_SHAPES, ids=lambda s: C.tag(s))
def test_float32_tensors_in_float64_arithmetic(env, shape):
    C.check_wide_iterates(env, shape)


def test_one_wave_form_beyond_512_qps(env):
    C.check_one_wave_beyond_512(env)
