"""Batch sharding of QPFunction(duals=True) on CPU: world_size 2, gloo, the kernels in the host-thread emulator.
dist.solve_sharded with a callable that returns a tuple gathers every output; a loss of the local lam and nu back-propagates
on each rank and the shared parameter's gradient reduces to the global batch mean -- equal to the one-process run."""
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import problems
from test_dist_gloo import _free_port

B, N, M, NEQ = 4, 12, 9, 3


def _problem():
    arrs = list(problems.random_dense_qp(B, N, M, NEQ, seed=31))
    arrs[0] = arrs[0][0]                                  # Q shared by the batch
    r = np.random.RandomState(32)
    return [torch.tensor(x) for x in arrs], torch.tensor(r.randn(B, M)), torch.tensor(r.randn(B, NEQ))


def _run(tq, gl, gn, solve):
    from emu.harness import emulated
    Q = tq[0].clone().requires_grad_(True)
    p = tq[1].clone().requires_grad_(True)
    with emulated(64):
        local, full = solve(Q, p)
        z, nu, lam, sl = local
        lo = 0 if full is None else dist.get_rank() * (B // dist.get_world_size())
        ((lam * gl[lo:lo + lam.size(0)]).sum() + (nu * gn[lo:lo + nu.size(0)]).sum()).backward()
    return local, full, Q.grad, p.grad


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from qpth_amd import dist as qdist
    from qpth_amd.qp import QPFunction
    tq, gl, gn = _problem()
    local, full, dQ, dp = _run(tq, gl, gn, lambda Q, p: qdist.solve_sharded(QPFunction(verbose=-1, duals=True), Q, p, *tq[2:], B))
    assert isinstance(local, tuple) and len(full) == 4 and all(f.shape[0] == B for f in full)
    dQ = qdist.reduce_shared_grad(dQ, B // world, B)
    dist.all_reduce(dp, op=dist.ReduceOp.SUM)            # zero outside this rank's rows
    # the single-output callable is unchanged: (local zhat, full zhat)
    from emu.harness import emulated
    with emulated(64):
        z_local, z_full = qdist.solve_sharded(QPFunction(verbose=-1), *tq, B)
    assert torch.equal(z_full, full[0]) and torch.equal(z_local, local[0].detach())
    if rank == 0:
        np.savez(os.path.join(out_dir, "out.npz"), dQ=dQ.numpy(), dp=dp.numpy(), **{k: f.numpy() for k, f in zip(("z", "nu", "lam", "s"), full)})
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharding_with_duals(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    out = np.load(tmp_path / "out.npz")
    from qpth_amd.qp import QPFunction
    tq, gl, gn = _problem()
    local, _, dQ, dp = _run(tq, gl, gn, lambda Q, p: (QPFunction(verbose=-1, duals=True)(Q, p, *tq[2:]), None))
    for k, o in zip(("z", "nu", "lam", "s"), local):
        assert np.array_equal(out[k], o.detach().numpy()), k
    assert np.abs(out["dQ"] - dQ.numpy()).max() <= 1e-12 * max(1.0, dQ.abs().max().item())
    assert np.array_equal(out["dp"], dp.numpy())
