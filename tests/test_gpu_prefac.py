"""-m gpu: the pre-factorisation's factor blob on a real MI355X, through libqpx_hip.so: the checks of tests/test_emu_prefac.py
(tests/prefac_checks.py), same cases, references and gates -- where the matrix-core tile products, the DPP reductions of the
column sums and the LDS exchange of the four-pivot groups are the real ones.  One launch per case, batches of three QPs (two
in the large-QP family)."""
import contextlib

import pytest
import torch

import prefac_checks as C

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


ids = lambda cases: [C.tag(*c[:2]) + ("" if len(c) < 3 else "/%s%d" % c[2]) for c in cases]      # noqa: E731


@pytest.mark.parametrize("shape,knob", C.CASES, ids=ids(C.CASES))
def test_every_word_of_the_blob(env, shape, knob):
    C.check_blob(env, shape, knob)


def test_knob_512_writes_the_blob_of_knob_256(env):
    C.check_knob_512_writes_the_blob_of_knob_256(env)


@pytest.mark.parametrize("c", C.COND_CS)
@pytest.mark.parametrize("shape,knob", C.COND_CASES, ids=ids(C.COND_CASES))
def test_conditioning_ladder(env, shape, knob, c):
    C.check_conditioning(env, shape, knob, c)


@pytest.mark.parametrize("shape", C.WIDE_SHAPES, ids=lambda s: C.tag(s))
def test_float32_tensors_in_float64_arithmetic(env, shape):
    C.check_wide(env, shape)


@pytest.mark.parametrize("shape", C.F32_SHAPES, ids=lambda s: C.tag(s))
def test_float32_blob(env, shape):
    C.check_f32(env, shape)


@pytest.mark.parametrize("shape,knob", C.SOFT_CASES, ids=ids(C.SOFT_CASES))
def test_soft_rows_change_the_diagonal_of_r_and_gt1_only(env, shape, knob):
    C.check_soft(env, shape, knob)


@pytest.mark.parametrize("shape,knob", C.STRIDE_CASES, ids=ids(C.STRIDE_CASES))
def test_unbatched_q_or_g_beside_a_batched_one(env, shape, knob):
    C.check_strides(env, shape, knob)


@pytest.mark.parametrize("shape,knob", C.SHARED_CASES, ids=ids(C.SHARED_CASES))
def test_shared_factors_are_qp_0_of_the_expanded_batch_bitwise(env, shape, knob):
    C.check_shared(env, shape, knob)


@pytest.mark.parametrize("shape,knob", [((65, 17, 0), C.BIGK), (C.BIG, 0)], ids=ids([((65, 17, 0), C.BIGK), (C.BIG, 0)]))
def test_large_family_refuses_sharing(env, shape, knob):
    C.check_large_family_refuses_sharing(env, shape, knob)


@pytest.mark.parametrize("shape,knob,how", C.FAILURE_CASES, ids=ids(C.FAILURE_CASES))
def test_a_failed_qp_leaves_its_neighbours_alone(env, shape, knob, how):
    C.check_failure(env, shape, knob, how)
