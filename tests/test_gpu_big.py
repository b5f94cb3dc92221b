"""-m gpu: the large-QP family at its own sizes on a real MI355X, through libqpx_hip.so -- 4 to 16 blocks of 64, the batch in
parts on side streams, the knob's variant bits 26..29: every case of tests/big_checks.py (the table, the references and the
gates are there).  Most of each test is its CPU reference; the whole module (107 tests) is 17 s."""
import contextlib

import pytest
import torch

import big_checks as C

pytestmark = pytest.mark.gpu
ids = lambda shapes: [C.tag(s) for s in shapes]      # noqa: E731
HOST = C.HOST
HOST_IDS = ["%s/B%d/%#x" % (C.tag(s, base), B, v) for s, base, v, B in HOST]
DEFAULTS = sorted({(s, base, B) for s, base, v, B in HOST})
DIAG = [(C.F32_SHAPE, f) for f in C.DIAG_FORMS]
DIAG_IDS = [C.tag(s, f) for s, f in DIAG]


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


def test_the_table_reaches_the_block_counts_it_names():
    assert [tuple(x // 64 for x in (C.P.R.big_pad(n), C.P.R.big_pad(m), C.P.R.big_pad(q) if q else 0)) for n, m, q in C.SHAPES] == C.BLOCKS
    assert all(sum(s) > 208 for s in C.SHAPES)


# ---------------------------------------------------------------- 1. the loop's path
@pytest.mark.parametrize("shape", C.SHAPES, ids=ids(C.SHAPES))
def test_iterates_after_k_iterations(env, shape):
    C.check_iterates_after_k(env, shape)


@pytest.mark.parametrize("shape", C.SHAPES, ids=ids(C.SHAPES))
def test_iteration_counts_and_trace(env, shape):
    C.check_counts_and_trace(env, shape)


@pytest.mark.parametrize("shape", C.SHAPES, ids=ids(C.SHAPES))
def test_best_iterate_bookkeeping(env, shape):
    C.check_best_iterate(env, shape)


@pytest.mark.parametrize("shape", C.SHAPES, ids=ids(C.SHAPES))
def test_stall_policy_0_runs_to_max_iter(env, shape):
    C.check_no_stall_counter(env, shape)


def test_one_qp_stops_beside_a_running_one():
    C.check_one_qp_stops_beside_a_running_one()


def test_float32_tensors_in_float64_arithmetic(env):
    C.check_wide_iterates(env)


# ---------------------------------------------------------------- 2. the KKT-solve kernels
@pytest.mark.parametrize("shape", C.SHAPES, ids=ids(C.SHAPES))
def test_solve(env, shape):
    C.check_solve(env, shape)


@pytest.mark.parametrize("shape", C.SHAPES, ids=ids(C.SHAPES))
def test_backward_with_duals_cotangents(env, shape):
    C.check_backward(env, shape)


@pytest.mark.parametrize("shape", C.SHAPES, ids=ids(C.SHAPES))
def test_forward_mode_and_the_adjoint_identity(env, shape):
    C.check_jvp(env, shape)


@pytest.mark.parametrize("shape", C.SHAPES, ids=ids(C.SHAPES))
def test_k_right_hand_sides_and_the_second_order_pass_are_declined(env, shape):
    C.check_declined_roles(env, shape)


def test_float32_kernels(env):
    C.check_f32(env)


# ---------------------------------------------------------------- 3. every word of the blob
@pytest.mark.parametrize("shape", C.BLOB_SHAPES, ids=ids(C.BLOB_SHAPES))
def test_every_word_of_the_blob(env, shape):
    C.check_blob(env, shape)


# ---------------------------------------------------------------- the host forms
@pytest.mark.parametrize("shape,base,B", DEFAULTS, ids=["%s/B%d" % (C.tag(s, k), B) for s, k, B in DEFAULTS])
def test_one_part_default_launch_against_the_references(env, shape, base, B):
    C.check_default_launch(env, shape, base, B)


@pytest.mark.parametrize("shape,base,variant,B", HOST, ids=HOST_IDS)
def test_host_form_is_the_default_launch_bit_for_bit(env, shape, base, variant, B):
    C.check_host_form(env, shape, base, variant, B)


@pytest.mark.parametrize("shape,form", DIAG, ids=DIAG_IDS)
def test_other_diagonal_block_eliminations(env, shape, form):
    """bits 27 and 28: other arithmetic, so checks 1 to 3 on their own gates"""
    C.check_iterates_after_k(env, shape, form)
    C.check_counts_and_trace(env, shape, form)
    C.check_best_iterate(env, shape, form)
    C.check_no_stall_counter(env, shape, form)
    C.check_solve(env, shape, form)
    C.check_backward(env, shape, form)
    C.check_jvp(env, shape, form)
    C.check_blob(env, shape, form)
