"""-m gpu: scenario batches on a real MI355X, through libqpx_hip.so: the checks of tests/test_emu_scenarios.py
(tests/scenario_checks.py), same cases, references and gates -- where the blob index is a scalar division in the kernel and
the grouped contraction runs on the matrix cores --, the fallback to the expanded batch at a large-QP size, and the launch
sequence build -> ipm -> backward -> group_outer captured into one graph."""
import contextlib

import pytest
import torch

import scenario_checks as C

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


# ---- 1. the forward is bitwise
@pytest.mark.parametrize("shape", C.FORM_SHAPES, ids=C.tag)
def test_forward_is_bitwise_in_every_form(env, shape):
    C.check_forward_bitwise(env, shape)


@pytest.mark.parametrize("B,K", [(2, 1), (1, 5)])
@pytest.mark.parametrize("shape", [(12, 9, 3), (20, 40, 4)], ids=C.tag)
def test_forward_one_scenario_and_one_group(env, shape, B, K):
    C.check_forward_bitwise(env, shape, B=B, K=K)


@pytest.mark.parametrize("shape", C.ONE_WAVE_SHAPES, ids=C.tag)
def test_forward_one_wave_tile_forms(env, shape):
    C.check_forward_bitwise(env, shape, knob=C.ONE_WAVE)


@pytest.mark.parametrize("wide", [False, True], ids=["f32", "f32_wide"])
def test_forward_float32(env, wide):
    C.check_forward_bitwise(env, (12, 9, 3), dtype=torch.float32, wide=wide)


# ---- 2. the backward
@pytest.mark.parametrize("duals", [False, True], ids=["dz", "duals"])
@pytest.mark.parametrize("shape", C.FORM_SHAPES, ids=C.tag)
def test_backward_against_the_expanded_batch(env, shape, duals):
    C.check_backward(env, shape, duals)


@pytest.mark.parametrize("shape", C.ONE_WAVE_SHAPES, ids=C.tag)
def test_backward_one_wave_tile_forms(env, shape):
    C.check_backward(env, shape, True, knob=C.ONE_WAVE)


@pytest.mark.parametrize("duals", [False, True], ids=["dz", "duals"])
@pytest.mark.parametrize("mixed", [False, True], ids=["bk", "mixed"])
@pytest.mark.parametrize("shape", [(12, 9, 3), (100, 100, 0)], ids=C.tag)
def test_qpfunction_equals_the_expanded_call(env, shape, mixed, duals):
    C.check_qpfunction_equals_expanded(env, shape, duals=duals, mixed=mixed)


@pytest.mark.parametrize("shape", [(6, 4, 2), (12, 9, 3)], ids=C.tag)
def test_against_the_oracle(env, shape):
    C.check_oracle(env, shape)


# ---- 3. the contraction alone
@pytest.mark.parametrize("K", C.OUTER_KS)
@pytest.mark.parametrize("rc", C.OUTER_SHAPES, ids=lambda rc: "%dx%d" % rc)
def test_group_outer_against_numpy(env, rc, K):
    C.check_outer(env, rc, K)


def test_group_outer_float32(env):
    C.check_outer(env, (12, 9), 17, dtype=torch.float32)


# ---- 4. one factorisation per group
def test_one_factorisation_per_group(env):
    C.check_one_factorisation_per_group(env)


def test_gradcheck_over_six_inputs(env):
    C.check_gradcheck(env)


def test_unbatched_matrices_take_the_one_blob_path(env):
    C.check_shared_matrices_take_the_one_blob_path(env)


# ---- 5. status
def test_a_bad_q_in_one_group(env):
    C.check_status(env)


# ---- 6. ABI, fallback and refusals
def test_abi_codes_and_group_supported(env):
    C.check_abi(env)


def test_fallback_at_a_large_qp_size_equals_the_expanded_call(env):
    C.check_fallback_equals_expanded(env)


def test_refusals(env):
    C.check_refusals(env)


# ---- 7. capture
def test_launch_sequence_replays_from_a_captured_graph(env):
    """build -> ipm -> backward -> group_outer at (100,100,0), B = 4, K = 3, captured into ONE graph and replayed on new data
    in the same buffers: bit-identical to the eager calls on the same data (as test_gpu_parity.py's test of the existing calls)"""
    from qpth_amd.kkt import KKTFactors
    shape, B, K = (100, 100, 0), 4, 3
    n = shape[0]
    first, second = [[t.clone() for t in sum((list(x) for x in C.tensors(env, shape, B, K, seed=s)[:2]), [])] for s in (21, 22)]
    ones = torch.ones(B * K, n, dtype=torch.float64, device=env.dev)

    def run(Q, G, A, p, h, b):
        fac = KKTFactors.build(Q, G, A, nBatch=B, scenarios=K)
        res = fac.ipm(p, h, b)
        grads = fac.backward(res.zhat, res.lam, res.slacks, res.nu, ones)
        return [res.zhat, res.lam, res.slacks, res.iters, res.status] + [g for g in grads if g is not None]

    eager = [[t.clone() for t in run(*data)] for data in (first, second)]       # (also the warm-up: LDS opt-ins)
    assert eager[0][5].shape == (B, n, n) and not torch.equal(eager[0][0], eager[1][0])
    torch.cuda.synchronize()
    static = [t.clone() for t in first]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(*static)
    for data, want in ((first, eager[0]), (second, eager[1]), (first, eager[0])):
        for s, t in zip(static, data):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        for got, exp in zip(outs, want):
            assert torch.equal(got, exp)
    assert int(outs[4].max().item()) & 7 == 0
