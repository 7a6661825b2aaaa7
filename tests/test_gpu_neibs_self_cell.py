"""The fluid-segment scan of build_neibs_kernel (csrc/neibs_build.hip) exists twice: for the home cell (neighbour cell 13), where one
candidate is the particle itself and is left out by comparing `index - j0` with the candidate's number in its batch, and for the
other 26 cells, which carry no self test.  The lists must stay the oracle's, bit for bit (the pattern of
tests/test_gpu_parity.py::test_neibs_phase_bit_exact), where the self test matters most:

  clump    a cell of several hundred fluid particles: many batches of four candidates per home cell, the particle itself in the
           first batch, in a middle one and in the last one, at every position within a batch;
  single   a periodic lattice whose cells hold one particle each: the home cell's only candidate is the particle itself."""
import numpy as np
import pytest

import oracle_lib as ol
import tiling_overflow_cases as toc
from gpusph_amd import defs as D
from gpusph_amd.problem import PeriodicBox

pytestmark = pytest.mark.gpu

BATCH = 4      # NEIB_MLP: candidates per batch of the fluid segment


def _np(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def _build(prob):
    from gpusph_amd.engine import TimestepEngine
    eng = TimestepEngine(prob, device="cuda:0", clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs()
    eng.build_neibs()
    n = eng.n
    assert n == sim.n
    assert np.array_equal(_np(eng.hash, np.uint32)[:n], sim.hash[:n])
    assert np.array_equal(_np(eng.cellStart, np.uint32), sim.cs)
    assert np.array_equal(_np(eng.cellEnd, np.uint32), sim.ce)
    assert np.array_equal(_np(eng.pos)[:n].view(np.uint32), sim.pos[:n].view(np.uint32))
    info = eng.neibs_info()
    assert info.hasTooManyNeibs == -1 and sim.neibs_info.hasTooManyNeibs == -1
    assert info.numInteractions == sim.neibs_info.numInteractions
    nls = int(prob.simparams.neiblistsize)
    got = _np(eng.neibslist, np.uint16).reshape(nls, -1)
    want = np.asarray(sim.nl).reshape(nls, -1)
    assert got.shape == want.shape
    return eng, sim, n, got, want


def _home_cell_entries(column):
    """relative indices of the entries of neighbour cell 13 in the fluid section of one list"""
    out, cell = [], -1
    for d in column:
        d = int(d)
        if d == D.NEIBS_END:
            break
        if d >= D.CELLNUM_ENCODED:
            cell = (d >> D.CELLNUM_SHIFT) - 1
            d &= D.NEIBINDEX_MASK
        if cell == 13:
            out.append(d)
    return out


def _check_particles(picks, got, want, hash_, cs):
    for what, i in picks:
        assert np.array_equal(got[:, i], want[:, i]), "list of particle %d (%s of its cell) differs from the oracle's" % (i, what)
        rel = _home_cell_entries(got[:, i])
        own = i - int(cs[int(hash_[i]) & D.CELLTYPE_BITMASK])
        assert own not in rel, "particle %d (%s of its cell) lists itself" % (i, what)
        assert rel == sorted(set(rel)), "home-cell entries of particle %d out of order or repeated" % i


def test_home_cell_of_many_batches():
    prob = toc.clump()
    eng, sim, n, got, want = _build(prob)
    cells = sim.hash[:n].astype(np.int64) & D.CELLTYPE_BITMASK
    fluid = (sim.info[:n, 0] & 7) == D.PT_FLUID
    home = int(np.bincount(cells[fluid]).argmax())
    first, end = int(sim.cs[home]), int(sim.ce[home])
    members = np.flatnonzero(fluid & (cells == home))
    assert len(members) >= 3*BATCH and members[0] == first and members[-1] == first + len(members) - 1 < end
    print("clump: %d fluid particles in cell %d = %d batches" % (len(members), home, -(-len(members)//BATCH)))
    last = int(members[-1])
    mid0 = first + BATCH*(len(members)//(2*BATCH))      # first candidate of a middle batch
    picks = [("first", first), ("last", last)] + [("middle, candidate %d of its batch" % u, mid0 + u) for u in range(BATCH)] + \
        [("second", first + 1), ("last of the first batch", first + BATCH - 1), ("first of the last batch", first + BATCH*((len(members) - 1)//BATCH))]
    _check_particles(picks, got, want, sim.hash, sim.cs)
    assert len(_home_cell_entries(got[:, mid0])) >= 2*BATCH      # the clump is dense: the home cell fills whole batches of the list
    assert np.array_equal(got, want), "%d lists differ from the oracle's" % int((got != want).any(axis=0).sum())


def test_cells_of_a_single_particle():
    class Narrow(PeriodicBox):      # influence radius 0.98 dp: the cells are dp wide and hold the one lattice site each
        def set_deltap(self, dp):
            self.simparams.sfactor = 0.49
            super().set_deltap(dp)
    n3 = (12, 10, 9)
    prob = Narrow(n=n3, jitter=0.1, linearization="xzy")
    assert tuple(int(g) for g in prob.m_gridsize) == n3
    eng, sim, n, got, want = _build(prob)
    assert n == n3[0]*n3[1]*n3[2]
    assert np.array_equal(sim.ce[:n] - sim.cs[:n], np.ones(n, dtype=sim.cs.dtype)), "a cell with another number of particles than one"
    lengths = (want[:, :n] != D.NEIBS_END).argmin(axis=0)
    assert lengths.max() >= 2 and (lengths == 0).sum() < n//2      # jitter brings some lattice neighbours within 0.98 dp
    _check_particles([("only one", i) for i in (0, 1, n//2, n - 1)], got, want, sim.hash, sim.cs)
    for i in range(n):
        assert not _home_cell_entries(got[:, i])
    assert np.array_equal(got, want), "%d lists differ from the oracle's" % int((got != want).any(axis=0).sum())
