"""The large-QP family at its own sizes on the host-thread emulator: what of tests/big_checks.py a fibre per GPU thread can do
in about 20 s per test -- the three shapes up to four blocks in full, the host forms at the batches up to 8 (here they only
guard the pointer offsets and part boundaries: the emulator runs streams one after the other), and at nine blocks the loop's
iterates, counts and trace, the KKT solve with the "mid" d and the blob.  tests/test_gpu_big.py runs every case on the GPU.
Measured: at most 23 s per test (the batch of 8 at (130, 70, 5)); the module, 50 tests, 380 s -- a launch of the large family
is 2.5 .. 4 s per QP in fibres; what was left to the GPU runner and the seconds that decided it: tests/big_checks.py."""
import contextlib

import pytest
import torch

import big_checks as C
from emu.harness import emulated


class Env:
    dev = torch.device("cpu")

    @staticmethod
    @contextlib.contextmanager
    def run(variant=0):
        with emulated(256, variant):
            yield


ENV = Env()
SHAPES = C.UP_TO_FOUR_BLOCKS
ids = lambda shapes: [C.tag(s) for s in shapes]      # noqa: E731
HOST = C.EMU_HOST
HOST_IDS = ["%s/B%d/%#x" % (C.tag(s, base), B, v) for s, base, v, B in HOST]
DEFAULTS = sorted({(s, base, B) for s, base, v, B in HOST})


def test_the_table_reaches_the_block_counts_it_names():
    big_pad = C.P.R.big_pad
    assert [tuple(x // 64 for x in (big_pad(n), big_pad(m), big_pad(q) if q else 0)) for n, m, q in C.SHAPES] == C.BLOCKS
    assert all(sum(s) > 208 for s in C.SHAPES)
    assert [C.part_lengths(B, parts) for parts, B in C.PARTS] == [[2, 3], [1, 2, 2], [1, 1, 1, 2], [16, 17], [16, 16, 16]]


# ---------------------------------------------------------------- 1. the loop's path
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_iterates_after_k_iterations(shape):
    C.check_iterates_after_k(ENV, shape)


@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_iteration_counts_and_trace(shape):
    C.check_counts_and_trace(ENV, shape)


@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_best_iterate_bookkeeping(shape):
    C.check_best_iterate(ENV, shape)


@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_stall_policy_0_runs_to_max_iter(shape):
    C.check_no_stall_counter(ENV, shape)


@pytest.mark.parametrize("shape", [C.NINE_BLOCKS, C.NINE_BLOCKS_LQ], ids=ids([C.NINE_BLOCKS, C.NINE_BLOCKS_LQ]))
def test_iterates_after_k_iterations_at_nine_blocks(shape):
    C.check_iterates_after_k(ENV, shape)


def test_iteration_counts_and_trace_at_nine_blocks():
    C.check_counts_and_trace(ENV, C.NINE_BLOCKS)


def test_one_qp_stops_beside_a_running_one():
    C.check_one_qp_stops_beside_a_running_one()


# ---------------------------------------------------------------- 2. the KKT-solve kernels
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_solve(shape):
    C.check_solve(ENV, shape)


@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_backward_with_duals_cotangents(shape):
    C.check_backward(ENV, shape)


@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_forward_mode_and_the_adjoint_identity(shape):
    C.check_jvp(ENV, shape)


@pytest.mark.parametrize("shape", SHAPES + [C.NINE_BLOCKS], ids=ids(SHAPES + [C.NINE_BLOCKS]))
def test_k_right_hand_sides_and_the_second_order_pass_are_declined(shape):
    C.check_declined_roles(ENV, shape)


def test_solve_at_nine_blocks():
    C.check_solve(ENV, C.NINE_BLOCKS, kinds=("mid",))


def test_float32_kernels():
    C.check_f32(ENV)


# ---------------------------------------------------------------- 3. every word of the blob
@pytest.mark.parametrize("shape", SHAPES + [C.NINE_BLOCKS], ids=ids(SHAPES + [C.NINE_BLOCKS]))
def test_every_word_of_the_blob(shape):
    C.check_blob(ENV, shape)


# ---------------------------------------------------------------- the host forms
@pytest.mark.parametrize("shape,base,B", DEFAULTS, ids=["%s/B%d" % (C.tag(s, k), B) for s, k, B in DEFAULTS])
def test_one_part_default_launch_against_the_references(shape, base, B):
    C.check_default_launch(ENV, shape, base, B)


@pytest.mark.parametrize("shape,base,variant,B", HOST, ids=HOST_IDS)
def test_host_form_is_the_default_launch_bit_for_bit(shape, base, variant, B):
    C.check_host_form(ENV, shape, base, variant, B)
