"""The CPU side of tests/grid_edge_cases.py: what the device tests of tests/test_gpu_grid_edge_cases.py take for granted is proven here on the
oracle, without a GPU.

Per case: the grid is the one the table names; every neighbour list fits; the length of every row's fluid section equals the
number of (particle, image) pairs within the influence radius counted without cells (tests/allpairs_ref.py over
grid_edge_cases.image_shifts: the reference's rule is the offsets -1 / 0 / +1 per axis, each wrapped on its own, the particle
itself skipped by index -- on one cell a particle meets its OWN images nowhere, and another particle through every image in reach);
in a perturbed state the oracle's forces and d(rho~)/dt equal the float64 image sum to 2e-5 of the field's scale; the table's
`usable` is what the tiling's limits say of the case (window_overflow, tile_cols_sides).

Measured (oracle against the float64 image sum, fraction of the field's largest entry; acceleration / d(rho~)/dt):
  one-cell 4.34e-6 / 2.73e-6    one-cell-wave 2.81e-6 / 1.65e-6    two-each 2.98e-6 / 2.23e-6    3x2x1 3.70e-6 / 2.20e-6
  3x2x1-zxy 3.59e-6 / 2.23e-6   3x1x2-yzx 3.06e-6 / 2.40e-6        1x3x2 2.73e-6 / 1.98e-6       slab-y 3.20e-6 / 1.13e-6
  slab-free 4.21e-6 / 1.13e-6   odd-5x3x1 4.68e-6 / 1.63e-6        rod-full 2.75e-6 / 1.78e-6    rod-over 2.78e-6 / 1.85e-6
Pairs on the Colagrossi threshold: 4 of 3.6 million in rod-over, none elsewhere; with gravity a quarter of the pairs have the switch
off.  Rows with a pair within 1e-6 of the influence radius: 20 of 47925 and 18 of 47952 in the rods (one of them 7e-8 inside it: the
list has it, the float64 count at R (1 - 1e-7) does not), none elsewhere."""
import functools

import numpy as np
import pytest

import allpairs_ref as ap
import grid_edge_cases as ge
import oracle_lib as ol
from forces_check import _perturb
from gpusph_amd import defs as D
from tiling_overflow_cases import section_lengths


RADIUS_BAND = 1e-6


@functools.lru_cache(maxsize=None)
def _built(name):
    prob = ge.problem(name)
    sim = ol.OracleSim(prob)
    sim.build_neibs()
    n = sim.n
    return prob, sim, prob.global_pos(sim.pos[:n], sim.hash[:n]), ap.consts(sim), ge.image_shifts(prob)


@pytest.mark.parametrize("name", list(ge.CASES))
def test_grid_lists_and_tiling_precondition(name):
    prob, sim, gp, k, shifts = _built(name)
    n = sim.n
    sp = prob.simparams
    assert tuple(int(v) for v in prob.m_gridsize) == ge.grid(name)
    assert n == int(np.prod(ge.CASES[name][0]["n"])) and sim.neibs_info.hasTooManyNeibs == -1
    assert len(shifts) == 3**bin(int(sp.periodicbound)).count("1")
    # lists: row by row as many entries as the image sum has neighbours.  The list build decides r < R in float32 on cell-local
    # positions (three roundings of lengths up to 0.3 per component: 5e-8 of absolute error, 4e-7 of R): a pair within RADIUS_BAND
    # of the radius may be on either side, the rows that have one are counted and must stay rare
    first = section_lengths(sim.nl, n, len(sim.pos), int(sp.neiblistsize), int(sp.neibboundpos), False)[0]
    inner = ap.neighbours(sim, gp, dict(k, R=k["R"]*(1 - RADIUS_BAND)), shifts=shifts)
    lo = np.array([len(nb) for nb in inner])
    hi = np.array([len(nb) for nb in ap.neighbours(sim, gp, dict(k, R=k["R"]*(1 + RADIUS_BAND)), shifts=shifts)])
    assert (lo <= first).all() and (first <= hi).all(), "rows differ: %s" % np.nonzero((first < lo) | (first > hi))[0][:8]
    print("%s: %d of %d rows with a pair within %g of the radius" % (name, (lo != hi).sum(), n, RADIUS_BAND))
    assert (lo != hi).sum() <= 1e-3*n
    assert lo.min() > 0 and first.max() <= ge.limits()["list"]
    multi = ge.image_pairs_beyond_one(inner)
    assert ge.multi_image(name) is None or (multi > 0) == ge.multi_image(name), multi
    if name == "one-cell":
        assert multi == n*(n - 1)          # every ordered pair
    # tiles: the allocation of the window columns, then the window itself
    need, have = ge.tile_cols_sides(prob)
    over, window, home = ge.window_overflow(prob, sim.hash, n)
    print("%s: tile_cols %d of %d words, largest window %d records, largest home column %d" % (name, need, have, window, home))
    if name == "rod-full":
        assert need == have
    if name == "rod-over":
        assert need == have + 1
    assert ge.usable(name) == int(need <= have and not over)


@pytest.mark.parametrize("name", ge.DEEP)
def test_stress_window_fits(name):
    """the tiled stress mode has a smaller window (TILE_WCAP_SPS1): the four SPS cases fit it too"""
    prob, sim, gp, k, shifts = _built(name)
    assert not ge.window_overflow(prob, sim.hash, sim.n, sps=True)[0]


@pytest.mark.parametrize("name", list(ge.CASES))
def test_oracle_forces_equal_the_float64_image_sum(name):
    prob, sim0, gp, k, shifts = _built(name)
    sim = ol.OracleSim(prob)
    sim.build_neibs()
    n = sim.n
    ge.perturb(sim)
    p = sim.o.p
    assert p.kerneltype == D.WENDLAND and p.densitydiffusiontype == D.COLAGROSSI and p.turbmodel == D.ARTIFICIAL
    f = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[0][:n].astype(np.float64)
    ref = ap.momentum_continuity(sim, gp, k, ge.wendland_F(k), shifts=shifts)
    acc, drt, amb = ref["acc"], ref["drt"], ref["amb"]
    ascale, dscale = np.abs(acc).max(), np.abs(drt).max()
    assert ascale > 10.0 and dscale > 1.0
    ea = np.abs(f[:, :3] - acc).max()/ascale
    ed = (np.abs(f[:, 3] - drt) - amb*(1 + 1e-6)).max()/dscale
    print("%s: acceleration %.2e, d(rho~)/dt %.2e of the scale; %d pairs, %d ambiguous, switch on / off %d / %d" %
          (name, ea, ed, ref["pairs"], ref["ambiguous"], ref["switch_on"], ref["switch_off"]))
    assert ea <= 2e-5 and ed <= 2e-5
    assert ref["ambiguous"] <= 0.01*ref["pairs"]
    if any(ge.CASES[name][0]["gravity"]):      # both branches of the switch, so g . r of an image is read on either side
        assert ref["switch_on"] > 0 and ref["switch_off"] > 0


def _by_id(sim, prob):
    n = sim.n
    ids = sim.info[:n, 2].astype(np.uint32) | (sim.info[:n, 3].astype(np.uint32) << 16)
    order = np.argsort(ids)
    return prob.global_pos(sim.pos[:n][order], sim.hash[:n][order]), prob.grid_pos_from_hash(sim.hash[:n][order])


@pytest.mark.parametrize("name", ge.DEEP)
def test_trajectory_crosses_faces_and_cells(name):
    """the twelve steps the device repeats, and the rebuild that the thirteenth would start with: with the mean velocity (4, -3, 2)
    and a rebuild every four steps particles leave through every periodic face and come back through the opposite one (calcHash
    has moved them: their global position has jumped by a box length), and change cell along every axis that has more than one.
    (The closing rebuild is there for z: at 2 m/s a particle has gone 0.29 dp when the last rebuild inside the run comes, and the
    jittered lattice keeps 0.3 dp from every face.)"""
    prob = ge.trajectory_problem(name)
    sim = ol.OracleSim(prob)
    _perturb(sim, None, 31)
    sim.build_neibs()
    x0, g0 = _by_id(sim, prob)
    for _ in range(ge.TRAJ_STEPS):
        sim.step()
    assert sim.iterations == ge.TRAJ_STEPS > 2*ge.TRAJ_REBUILD and np.isfinite(sim.vel[:sim.n]).all()      # rebuilds at 0, 4, 8
    sim.build_neibs()
    x1, g1 = _by_id(sim, prob)
    for a in range(3):
        moved = x1[:, a] - x0[:, a]
        wrapped = np.sign(moved) != np.sign(ge.MEAN_VELOCITY[a])      # nobody's velocity turns round: the noise is a tenth of the mean
        if int(prob.simparams.periodicbound) & (1 << a):
            assert wrapped.sum() > 0, "nobody crosses the periodic faces of axis %d" % a
            assert np.abs(np.abs(moved[wrapped]) - prob.m_size[a]).max() < 0.5*prob.m_cellsize[a]
        else:
            assert not wrapped.any()
        if prob.m_gridsize[a] > 1:
            assert (g1[:, a] != g0[:, a]).sum() > 0, "nobody changes cell along axis %d" % a
