"""The pre-factorisation's factor blob on the host-thread emulator: every form -- the sweep at its seven block counts, the
matrix-core form, the large-QP family, the soft forms -- against a dense reference refined in extended precision, word by
word.  The checks, their cases, references and gates: tests/prefac_checks.py; tests/test_gpu_prefac.py runs the same ones on
the GPU (there every shape under knob 1 << 14 too)."""
import contextlib

import pytest
import torch

import prefac_checks as C
from emu.harness import emulated


class Env:
    dev = torch.device("cpu")

    @staticmethod
    @contextlib.contextmanager
    def run(variant=0):
        with emulated(256, variant):
            yield


ENV = Env()
ids = lambda cases: [C.tag(*c[:2]) + ("" if len(c) < 3 else "/%s%d" % c[2]) for c in cases]      # noqa: E731


def test_the_cases_reach_every_block_count_of_the_sweep_and_every_image():
    """the table of tests/prefac_checks.py says what it claims, in this module's own restatement of the layout"""
    R = C.R
    assert sorted({R.sweep_nb(sum(s)) for s, k in C.CASES if k == C.SWEEP or C.expected_family(s, k)[0] != C.FAMILY_BIG}) == [1, 2, 4, 7, 8, 10, 13]
    assert {(n + q) % 4 for n, m, q in C.SWEEP_GROUPS} == {0, 1, 2, 3} and all(R.sweep_nb(sum(s)) >= 10 for s in C.SWEEP_GROUPS)
    assert [R.wave_nb(s[1]) for s in C.RW_SHAPES] == [2, 4, 8, 13, 0]
    assert [R.grid_nb(s[1]) for s in C.RG_SHAPES] == [10, 13]
    assert {R.tile_nb(n + q) for n, m, q in C.MATRIX_CORE} == {4, 7}
    assert [R.LayoutBig(*s).NP // 64 for s in C.BIG_FORCED] == [1, 2, 3]


@pytest.mark.parametrize("shape,knob", C.CASES, ids=ids(C.CASES))
def test_every_word_of_the_blob(shape, knob):
    C.check_blob(ENV, shape, knob)


def test_knob_512_writes_the_blob_of_knob_256():
    C.check_knob_512_writes_the_blob_of_knob_256(ENV)


@pytest.mark.parametrize("c", C.COND_CS)
@pytest.mark.parametrize("shape,knob", C.COND_CASES, ids=ids(C.COND_CASES))
def test_conditioning_ladder(shape, knob, c):
    C.check_conditioning(ENV, shape, knob, c)


@pytest.mark.parametrize("shape", C.WIDE_SHAPES, ids=lambda s: C.tag(s))
def test_float32_tensors_in_float64_arithmetic(shape):
    C.check_wide(ENV, shape)


@pytest.mark.parametrize("shape", C.F32_SHAPES, ids=lambda s: C.tag(s))
def test_float32_blob(shape):
    C.check_f32(ENV, shape)


@pytest.mark.parametrize("shape,knob", C.SOFT_CASES, ids=ids(C.SOFT_CASES))
def test_soft_rows_change_the_diagonal_of_r_and_gt1_only(shape, knob):
    C.check_soft(ENV, shape, knob)


@pytest.mark.parametrize("shape,knob", C.STRIDE_CASES, ids=ids(C.STRIDE_CASES))
def test_unbatched_q_or_g_beside_a_batched_one(shape, knob):
    C.check_strides(ENV, shape, knob)


@pytest.mark.parametrize("shape,knob", C.SHARED_CASES, ids=ids(C.SHARED_CASES))
def test_shared_factors_are_qp_0_of_the_expanded_batch_bitwise(shape, knob):
    C.check_shared(ENV, shape, knob)


@pytest.mark.parametrize("shape,knob", [((65, 17, 0), C.BIGK), (C.BIG, 0)], ids=ids([((65, 17, 0), C.BIGK), (C.BIG, 0)]))
def test_large_family_refuses_sharing(shape, knob):
    C.check_large_family_refuses_sharing(ENV, shape, knob)


@pytest.mark.parametrize("shape,knob,how", C.FAILURE_CASES, ids=ids(C.FAILURE_CASES))
def test_a_failed_qp_leaves_its_neighbours_alone(shape, knob, how):
    C.check_failure(ENV, shape, knob, how)
