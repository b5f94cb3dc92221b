"""The finishing role of the finishing-stage kernels (qpx_polish) step by step on the host-thread emulator: the iterates after
k steps, best_resid, the best-iterate rule, steps = 0, strides and shared factors, a non-finite QP beside healthy ones,
untouched memory and the error codes, in every form the emulator's case list reaches, against tests/polish_step_reference.py.
The checks, their starts, references and gates: tests/polish_checks.py; tests/test_gpu_polish.py runs the same ones on the GPU."""
import contextlib

import pytest
import torch

import polish_checks as C
from emu.harness import emulated


class Env:
    dev = torch.device("cpu")

    @staticmethod
    @contextlib.contextmanager
    def run(variant=0):
        with emulated(256, variant):
            yield


ENV = Env()
ids = lambda cases: [C.name(*c) for c in cases]      # noqa: E731


def test_the_case_list_reaches_every_form_but_the_gpu_only_one():
    got = {C.form_of(s, k, d, C.batch_of(s, k)) for s, k, d in C.EMU_CASES + C.F32_CASES}
    assert got == set(C.ALL_FORMS) - {"tile(4,1)"}, sorted(set(C.ALL_FORMS) - got)


@pytest.mark.parametrize("shape,knob,dtype", C.EMU_CASES, ids=ids(C.EMU_CASES))
def test_iterates_after_k_steps(shape, knob, dtype):
    C.check_steps(ENV, shape, knob, dtype)


@pytest.mark.parametrize("shape,knob,dtype", C.F32_CASES, ids=ids(C.F32_CASES))
def test_float32_kernels_after_k_steps(shape, knob, dtype):
    C.check_steps(ENV, shape, knob, dtype)


@pytest.mark.parametrize("kind,shape,knob,qp,expect", C.ILL, ids=[C.name(s, k, "f64", "-%s%d" % (kind, qp)) for kind, s, k, qp, _ in C.ILL])
def test_a_step_that_does_not_help_is_not_kept(kind, shape, knob, qp, expect):
    C.check_best_iterate_rule(ENV, kind, shape, knob, qp, expect)


@pytest.mark.parametrize("shape,knob,dtype", C.EMU_CASES + C.F32_CASES, ids=ids(C.EMU_CASES + C.F32_CASES))
def test_zero_steps_return_the_start(shape, knob, dtype):
    C.check_zero_steps(ENV, shape, knob, dtype)


@pytest.mark.parametrize("shape", C.SHARED_SHAPES, ids=lambda s: C.tag(s))
def test_unbatched_p_h_b(shape):
    C.check_unbatched_phb(ENV, shape)


def test_unbatched_p_h_b_in_the_large_family():
    C.check_unbatched_phb(ENV, C.SHARED_SHAPES[0], C.BIGK)


@pytest.mark.parametrize("shape", C.SHARED_SHAPES, ids=lambda s: C.tag(s))
def test_shared_factors(shape):
    C.check_shared_factors(ENV, shape)


def test_the_large_family_refuses_shared_factors():
    C.check_big_refuses_shared_factors(ENV)


@pytest.mark.parametrize("shape,knob", C.NAN_CASES, ids=[C.tag(s, k) for s, k in C.NAN_CASES])
def test_a_non_finite_qp_beside_healthy_ones(shape, knob):
    C.check_nan_beside_healthy(ENV, shape, knob)


@pytest.mark.parametrize("shape", C.SPARE_SHAPES, ids=lambda s: C.tag(s))
def test_spare_rows_are_untouched(shape):
    C.check_spare_rows(ENV, shape)


def test_supported_and_error_codes():
    C.check_supported_and_error_codes(ENV)
