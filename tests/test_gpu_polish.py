"""The finishing role of the finishing-stage kernels (qpx_polish) step by step on the MI355X: every check of
tests/polish_checks.py at all of its cases -- every form of QPX_FORMS_POLISH_TILE and QPX_FORMS_POLISH_GRID (the latter in both
dtypes) and the large-QP family -- against tests/polish_step_reference.py; the one-wave form at four tile rows, which
api_polish picks beyond 8192 QPs only, at B = 8200."""
import contextlib

import pytest
import torch

import polish_checks as C

pytestmark = pytest.mark.gpu
ids = lambda cases: [C.name(*c) for c in cases]      # noqa: E731


class Env:
    def __init__(self, dev):
        self.dev = dev

    @contextlib.contextmanager
    def run(self, variant=0):
        from qpth_amd import _lib
        dll = _lib.hip().dll
        old = dll.qpx_set_ipm_variant(variant)
        try:
            yield
        finally:
            dll.qpx_set_ipm_variant(old)


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "the -m gpu tests need an MI355X"
    return Env(torch.device("cuda:0"))


def test_the_case_list_reaches_every_form():
    got = {C.form_of(s, k, d, C.batch_of(s, k)) for s, k, d in C.CASES + C.F32_CASES}
    got.add(C.form_of(C.ONE_WAVE_SHAPE, 0, "f64", 2 * C.ONE_WAVE_REP))
    assert got == set(C.ALL_FORMS), sorted(set(C.ALL_FORMS) ^ got)


@pytest.mark.parametrize("shape,knob,dtype", C.CASES, ids=ids(C.CASES))
def test_iterates_after_k_steps(env, shape, knob, dtype):
    C.check_steps(env, shape, knob, dtype)


def test_one_wave_form_beyond_8192_qps(env):
    C.check_one_wave_beyond_8192(env)


@pytest.mark.parametrize("shape,knob,dtype", C.F32_CASES, ids=ids(C.F32_CASES))
def test_float32_kernels_after_k_steps(env, shape, knob, dtype):
    C.check_steps(env, shape, knob, dtype)


@pytest.mark.parametrize("kind,shape,knob,qp,expect", C.ILL, ids=[C.name(s, k, "f64", "-%s%d" % (kind, qp)) for kind, s, k, qp, _ in C.ILL])
def test_a_step_that_does_not_help_is_not_kept(env, kind, shape, knob, qp, expect):
    C.check_best_iterate_rule(env, kind, shape, knob, qp, expect)


@pytest.mark.parametrize("shape,knob,dtype", C.CASES + C.F32_CASES, ids=ids(C.CASES + C.F32_CASES))
def test_zero_steps_return_the_start(env, shape, knob, dtype):
    C.check_zero_steps(env, shape, knob, dtype)


@pytest.mark.parametrize("shape", C.SHARED_SHAPES, ids=lambda s: C.tag(s))
def test_unbatched_p_h_b(env, shape):
    C.check_unbatched_phb(env, shape)


def test_unbatched_p_h_b_in_the_large_family(env):
    C.check_unbatched_phb(env, C.SHARED_SHAPES[0], C.BIGK)


@pytest.mark.parametrize("shape", C.SHARED_SHAPES, ids=lambda s: C.tag(s))
def test_shared_factors(env, shape):
    C.check_shared_factors(env, shape)


def test_the_large_family_refuses_shared_factors(env):
    C.check_big_refuses_shared_factors(env)


@pytest.mark.parametrize("shape,knob", C.NAN_CASES, ids=[C.tag(s, k) for s, k in C.NAN_CASES])
def test_a_non_finite_qp_beside_healthy_ones(env, shape, knob):
    C.check_nan_beside_healthy(env, shape, knob)


@pytest.mark.parametrize("shape", C.SPARE_SHAPES, ids=lambda s: C.tag(s))
def test_spare_rows_are_untouched(env, shape):
    C.check_spare_rows(env, shape)


def test_supported_and_error_codes(env):
    C.check_supported_and_error_codes(env)
