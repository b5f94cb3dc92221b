"""Scenario batches (QPFunction(scenarios=K), KKTFactors.build(scenarios=K), qpx_ipm_group / qpx_backward_group /
qpx_group_outer) on the host-thread emulator: the grouped call against the library's own call on the expanded
batch.  The checks, their cases, references and gates: tests/scenario_checks.py; tests/test_gpu_scenarios.py runs the same
ones on the GPU, and there also the fallback at a large-QP size and the capture into a graph."""
import contextlib

import pytest
import torch

import scenario_checks as C
from emu.harness import emulated


class Env:
    dev = torch.device("cpu")

    @staticmethod
    @contextlib.contextmanager
    def run(variant=0):
        with emulated(256, variant):
            yield


ENV = Env()


# ---- 1. the forward is bitwise
@pytest.mark.parametrize("shape", C.FORM_SHAPES, ids=C.tag)
def test_forward_is_bitwise_in_every_form(shape):
    C.check_forward_bitwise(ENV, shape)


@pytest.mark.parametrize("B,K", [(2, 1), (1, 5)])
@pytest.mark.parametrize("shape", [(12, 9, 3), (20, 40, 4)], ids=C.tag)
def test_forward_one_scenario_and_one_group(shape, B, K):
    C.check_forward_bitwise(ENV, shape, B=B, K=K)


@pytest.mark.parametrize("shape", C.ONE_WAVE_SHAPES, ids=C.tag)
def test_forward_one_wave_tile_forms(shape):
    C.check_forward_bitwise(ENV, shape, knob=C.ONE_WAVE)


@pytest.mark.parametrize("wide", [False, True], ids=["f32", "f32_wide"])
def test_forward_float32(wide):
    C.check_forward_bitwise(ENV, (12, 9, 3), dtype=torch.float32, wide=wide)


# ---- 2. the backward
@pytest.mark.parametrize("duals", [False, True], ids=["dz", "duals"])
@pytest.mark.parametrize("shape", C.FORM_SHAPES, ids=C.tag)
def test_backward_against_the_expanded_batch(shape, duals):
    C.check_backward(ENV, shape, duals)


@pytest.mark.parametrize("shape", C.ONE_WAVE_SHAPES, ids=C.tag)
def test_backward_one_wave_tile_forms(shape):
    C.check_backward(ENV, shape, True, knob=C.ONE_WAVE)


@pytest.mark.parametrize("duals", [False, True], ids=["dz", "duals"])
@pytest.mark.parametrize("mixed", [False, True], ids=["bk", "mixed"])
@pytest.mark.parametrize("shape", [(12, 9, 3), (100, 100, 0)], ids=C.tag)
def test_qpfunction_equals_the_expanded_call(shape, mixed, duals):
    C.check_qpfunction_equals_expanded(ENV, shape, duals=duals, mixed=mixed)


@pytest.mark.parametrize("shape", [(6, 4, 2), (12, 9, 3)], ids=C.tag)
def test_against_the_oracle(shape):
    C.check_oracle(ENV, shape)


# ---- 3. the contraction alone
@pytest.mark.parametrize("K", C.OUTER_KS)
@pytest.mark.parametrize("rc", C.OUTER_SHAPES, ids=lambda rc: "%dx%d" % rc)
def test_group_outer_against_numpy(rc, K):
    C.check_outer(ENV, rc, K)


def test_group_outer_float32():
    C.check_outer(ENV, (12, 9), 17, dtype=torch.float32)


# ---- 4. one factorisation per group
def test_one_factorisation_per_group():
    C.check_one_factorisation_per_group(ENV)


def test_gradcheck_over_six_inputs():
    C.check_gradcheck(ENV)


def test_unbatched_matrices_take_the_one_blob_path():
    C.check_shared_matrices_take_the_one_blob_path(ENV)


# ---- 5. status
def test_a_bad_q_in_one_group():
    C.check_status(ENV)


# ---- 6. ABI and refusals (the fallback at a large-QP size runs on the GPU only: such a launch takes tens of seconds here)
def test_abi_codes_and_group_supported():
    C.check_abi(ENV)


def test_refusals():
    C.check_refusals(ENV)
