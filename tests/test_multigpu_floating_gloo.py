"""Floating bodies on several slabs, host logic on the CPU: gloo ranks of gpusph_amd.multigpu with the test-only oracle backend and
the floating-body rule in float64 (tests/floating_exact_ref.py, ExactOracleKernels).  Every rank sums the rows of the body particles
it owns into exact fixed-point limbs, the limbs are all-reduced, every rank rounds the sum once: one, two and three slabs must move
the cube, and with it every particle, with the same bits.  BuoyancyBox(0.05) has nine planes of cells of 0.1444 from -0.15 along every
axis: two slabs are cut at 0.572, three at 0.283 and 0.717.  The cube spans [0.3, 0.7] in x and y and [0.1, 0.5] in z, so two slabs
split along y (linearization xzy) and three along z (xyz) cut it; each is compared with the single domain of its own linearization
(the order of a particle's neighbours, and so its bits, follow the linearization), and the tests check on the ranks' own particles
that the body is on at least two of them, so that none can pass with the body on one rank.  Without the feature the exact_sums keyword does not exist."""
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from test_multigpu_gloo import ROOT, _free_port, _gather

STEPS = 12          # across the rebuild at iteration 10
FG_COMPUTE_FORCE, FG_MOVING_BOUNDARY = 0x08, 0x10


def _worker(rank, world, port, case, outdir):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ["OMP_NUM_THREADS"] = "2"
    import torch.distributed as dist
    from gpusph_amd import defs as D
    from gpusph_amd.problem import BuoyancyBox
    from gpusph_amd.multigpu import MultiGpuEngine, SlabPartition
    from floating_exact_ref import ExactOracleKernels
    assert (D.FG_COMPUTE_FORCE, D.FG_MOVING_BOUNDARY) == (FG_COMPUTE_FORCE, FG_MOVING_BOUNDARY)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    prob = BuoyancyBox(**case)
    arrs = prob.copy_to_array()
    part = SlabPartition(prob, world)
    n0 = int(part.local_mask(rank, arrs["hash"]).sum()) if world > 1 else len(arrs["hash"])
    # the body particles whose planes are this rank's own (its halo holds copies of others)
    c3 = (arrs["hash"] & D.CELLTYPE_BITMASK) // part.plane
    owned = (c3 >= part.lo[rank]) & (c3 < part.hi[rank]) & ((arrs["info"][:, 0] & FG_COMPUTE_FORCE) != 0)
    eng = MultiGpuEngine(prob, "cpu", rank, world, kernels=ExactOracleKernels(prob, int(n0 * 1.25) + 4096))
    assert eng.floating_exact
    for _ in range(STEPS):
        eng.step()
    out = eng.download_internal()
    state, slots = eng.floating_state(slots=True)
    np.savez(os.path.join(outdir, "r%d_of_%d.npz" % (rank, world)), n_local=eng.n_local, dt=eng.current_dt(), t=eng.time(),
             fstate=state, body_rows_at_start=int(owned.sum()),
             **{"slot_" + k: v for k, v in slots.items()}, **out)
    if world > 1:
        dist.barrier(); dist.destroy_process_group()


def _run(world, case, outdir):
    port = _free_port()
    if world == 1:
        _worker(0, 1, port, case, outdir)
    else:
        mp.spawn(_worker, args=(world, port, case, outdir), nprocs=world, join=True)


def _compare(tmp_path, case, worlds):
    for w in (1,) + tuple(worlds):
        _run(w, case, str(tmp_path))
    ids1, one, p1 = _gather(str(tmp_path), 1)
    s1 = p1[0]["fstate"]
    assert np.isfinite(s1).all() and s1[0, 2] > 0.3 + 1e-6 and np.abs(s1[0, 13:16]).max() > 0      # the cube rose under a force
    body = (one["info"][:, 0] & FG_COMPUTE_FORCE) != 0
    for w in worlds:
        idsN, many, pN = _gather(str(tmp_path), w)
        assert np.array_equal(ids1, idsN)            # every particle is owned by exactly one rank
        owners = [int(p["body_rows_at_start"]) for p in pN]
        assert sum(owners) == body.sum() and sum(1 for n in owners if n > 0) >= 2, owners      # the cut goes through the body
        now = [int(((p["info"][:, 0] & FG_COMPUTE_FORCE) != 0).sum()) for p in pN]
        assert sum(1 for n in now if n > 0) >= 2, now
        for k in ("pos", "vel", "forces"):
            assert np.array_equal(one[k].view(np.uint32), many[k].view(np.uint32)), (w, k)
        assert np.array_equal(one["hash"] & 0x3FFFFFFF, many["hash"] & 0x3FFFFFFF)
        for p in pN:
            assert float(p["dt"]) == float(p1[0]["dt"]) and float(p["t"]) == float(p1[0]["t"])
            assert np.array_equal(p["fstate"].view(np.uint64), s1.view(np.uint64)), w      # every rank holds the single domain's body
            for k in p1[0].files:
                if k.startswith("slot_"):
                    assert np.array_equal(p[k], p1[0][k]), (w, k)
            assert int(p["n_local"]) > len(p["pos"])      # every rank holds a halo
    return one, p1


@pytest.mark.parametrize("world,lin", [(2, "xzy"), (3, "xyz")])
def test_slabs_move_the_cube_with_the_bits_of_the_single_domain(tmp_path, world, lin):
    _compare(tmp_path, dict(deltap=0.05, linearization=lin, exact_sums=True), (world,))


def test_two_slabs_with_a_paddle_the_host_moves_beside_the_cube(tmp_path):
    """the paddle (the low-x wall slab, cut by the slab boundary as well) keeps the host callback on every rank"""
    one, _ = _compare(tmp_path, dict(deltap=0.05, linearization="xzy", exact_sums=True, paddle=True), (2,))
    pad = (one["info"][:, 0] & (FG_MOVING_BOUNDARY | FG_COMPUTE_FORCE)) == FG_MOVING_BOUNDARY
    assert pad.sum() > 50 and np.abs(one["vel"][pad, 0]).max() > 0


def test_several_slabs_ask_for_the_exact_sums():
    """the default sums in double are a single domain's: their bits depend on the order of the rows"""
    from gpusph_amd.problem import BuoyancyBox
    from gpusph_amd.multigpu import MultiGpuEngine
    with pytest.raises(NotImplementedError, match="exact body sums"):
        MultiGpuEngine(BuoyancyBox(deltap=0.1, linearization="xzy"), "cpu", 0, 2, kernels=object())
