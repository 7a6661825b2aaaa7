"""The forces tiles and the list build on grids of one to three cells per axis (tests/grid_edge_cases.py has the table and the reasons).

On such grids a cell stands in a tile's window several times, each copy at its own shift, and a pair interacts through several periodic
images; a wrong shift is a wrong force and no crash.  The tiled and the generic kernels share the helpers that make the shifts, so
next to the oracle (2e-5) and to each other they are held against a float64 sum over periodic images that knows no cells
(tests/allpairs_ref.py with grid_edge_cases.image_shifts) by the 4 x rule: the device may be at most four times as far from the
float64 value as the oracle is.  tests/test_grid_edge_cases.py proves on the CPU what is taken for granted here: the grids, that every
list fits, the oracle against the float64 sum, which cases the tiling can hold (`usable`), that the trajectories cross faces and cells.

Measured on an MI355X (profiles/grid_edge_cases.txt has every case): oracle / device from float64, acceleration
in m/s^2 of a scale of 60-110: one-cell 1.34e-4 / 1.40e-4, two-each 2.64e-4 / 2.64e-4, 3x2x1 1.68e-4 / 1.65e-4, slab-y 2.93e-4 / 2.91e-4,
rod-full 3.12e-4 / 2.99e-4; d(rho~)/dt in 1/s of a scale of 3-4: one-cell 7.2e-6 / 8.9e-6, two-each 1.37e-5 / 1.31e-5, rod-full 2.2e-5 / 3.0e-5.
Tiles usable == 1 in every case but one-cell-wave and rod-over."""
import numpy as np
import pytest

import allpairs_ref as ap
import grid_edge_cases as ge
import oracle_lib as ol
from forces_check import _check_neibs_and_forces, _engine, _np, _perturb, _within_4x, tiles_usable
from gpusph_amd import defs as D
from kernel_agreement import assert_forces_agree

pytestmark = pytest.mark.gpu

cases = pytest.mark.parametrize("name", list(ge.CASES))
deep = pytest.mark.parametrize("name", ge.DEEP)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _seed(name):
    return 70 + list(ge.CASES).index(name)


@cases
def test_lists_and_forces(name, monkeypatch):
    """a: hash, info, positions and lists bit-exact, forces and dt to 2e-5 against the oracle, tiled against generic, and the tiling
    usable exactly where the table says so (a case that passes because its tiling overflowed proves nothing).
    b: in the same state the device and the oracle against the float64 image sum, by the 4 x rule"""
    prob = ge.problem(name)
    assert tuple(int(v) for v in prob.m_gridsize) == ge.grid(name)
    eng, sim = _check_neibs_and_forces(prob, _seed(name), monkeypatch, usable=ge.usable(name))
    print("%s: tiles usable == %d" % (name, tiles_usable(eng)))
    n = eng.n
    f = _np(eng.forces)[:n]
    f_ref = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[0][:n]
    k = ap.consts(sim)
    ref = ap.momentum_continuity(sim, prob.global_pos(sim.pos[:n], sim.hash[:n]), k, ge.wendland_F(k), shifts=ge.image_shifts(prob),
                                 eos_rounding=True)      # _perturb's rho~ lies within 2e-3: pressures close enough for it to matter
    assert ref["ambiguous"] <= 0.01*ref["pairs"]
    _within_4x("%s acceleration" % name, f[:, :3], f_ref[:, :3], ref["acc"])
    drt = np.where(ref["amb"] > 0, np.nan, ref["drt"])      # a particle with a pair on the Colagrossi threshold has no single value
    _within_4x("%s d(rho~)/dt" % name, f[:, 3], f_ref[:, 3], drt)


@cases
def test_list_build_on_the_matrix_cores(name, monkeypatch):
    """c: SPHX_NEIBS_MFMA=1, lists and counters bit-exact (test_list_build_on_the_matrix_cores_bit_exact): the hand-over of the
    first / last cell of a periodic COORD1 to the general walk where those are one cell or two"""
    monkeypatch.setenv("SPHX_NEIBS_MFMA", "1")      # read when the context is created
    prob = ge.problem(name)
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs(); eng.build_neibs()
    n = eng.n
    assert n == sim.n and np.array_equal(_np(eng.hash, np.uint32)[:n], sim.hash[:n])
    assert np.array_equal(_np(eng.neibslist, np.uint16), sim.nl)
    info = eng.neibs_info()
    assert info.numInteractions == sim.neibs_info.numInteractions
    assert info.maxFluidBoundaryNeibs == sim.neibs_info.maxFluidBoundaryNeibs and info.hasTooManyNeibs == -1


def _calc_visc(eng, n):
    eng.k.calc_visc(eng.tau, eng.pos, eng.vel, eng.info, eng.hash, eng.cellStart, eng.neibslist, n, n, turbvisc=eng.turbvisc)
    return np.concatenate([_np(t)[:n] for t in eng.tau], axis=1), _np(eng.turbvisc)[:n].copy()


@deep
def test_sps(name, monkeypatch):
    """d: the forces with the SPS stress against the oracle and tiled against generic; sphx_calc_visc's tau and turbulent viscosity
    against orc_sps with the bars of test_gpu_kernel_axis.test_sps_stress.  The tiled stress mode is a forces instantiation of its
    own with a smaller window (TILE_WCAP_SPS1)"""
    import torch
    prob = ge.problem(name, viscosity="SPSVISC", kinematic_visc=1e-6)
    assert prob.simparams.turbmodel == D.SPS
    eng, sim = _check_neibs_and_forces(prob, 11, monkeypatch, usable=1)
    n = eng.n
    tau_ref, tv_ref = sim.o.sps(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, n)
    tau, tv = _calc_visc(eng, n)
    assert tiles_usable(eng) == 1
    scale = np.abs(tau_ref[:n]).max()
    assert scale > 0 and np.abs(tau).max() > 0 and (np.abs(tau_ref[:n]).max(axis=0) > 0).all()
    assert np.abs(tau - tau_ref[:n]).max() <= 2e-5*scale
    assert np.abs(tv - tv_ref[:n]).max() <= 2e-5*np.abs(tv_ref[:n]).max()
    monkeypatch.setenv("SPHX_DISABLE_TILES", "1")
    gen = _engine(prob, clobber_neibslist=True)
    gen.build_neibs()
    gen.vel[:n] = torch.from_numpy(sim.vel[:n]).to(gen.device)
    tau_g, tv_g = _calc_visc(gen, n)
    assert tiles_usable(gen) == 0
    monkeypatch.setenv("SPHX_DISABLE_TILES", "0")
    assert np.abs(tau_g - tau_ref[:n]).max() <= 2e-5*scale
    assert_forces_agree(tau, tau_g, what="SPS stress")
    assert_forces_agree(tv[:, None], tv_g[:, None], what="turbulent viscosity")


@deep
def test_filters_and_xsph(name):
    """e: Shepard and MLS bit-exact against the oracle (test_filters_bit_exact's state), and the XSPH rows of a forces pass"""
    import torch
    prob = ge.problem(name)
    prob.simparams.simflags |= D.ENABLE_XSPH
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs(); eng.build_neibs()
    n = eng.n
    assert n == sim.n and np.array_equal(_np(eng.hash, np.uint32)[:n], sim.hash[:n])
    rng = np.random.default_rng(3)
    vel = sim.vel.copy()
    vel[:, 3] += rng.uniform(-2e-3, 2e-3, size=len(vel)).astype(np.float32)
    vel[:, :3] += rng.uniform(-0.1, 0.1, size=(len(vel), 3)).astype(np.float32)
    sim.vel = vel
    eng.vel[:n] = torch.from_numpy(vel[:n]).to(eng.device)
    want = sim.o.xsph(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[:n]
    eng._forces(eng.pos, eng.vel, 1, 0)
    got = _np(eng.xsph)[:n]
    assert np.abs(want[:, :3]).max() > 1e-3
    assert np.array_equal(_bits(got), _bits(want)), "max |d xsph| = %g" % np.abs(got - want).max()
    for ftype in (D.SHEPARD_FILTER, D.MLS_FILTER):
        eng.vel[:n] = torch.from_numpy(vel[:n]).to(eng.device)
        ref = sim.o.filter(ftype, sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[:n]
        eng.apply_filter(ftype)
        out = _np(eng.vel)[:n]
        assert np.abs(ref[:, 3] - vel[:n, 3]).max() > 1e-4          # the filter does something to this state
        assert np.array_equal(_bits(out[:, :3]), _bits(ref[:, :3]))
        assert np.array_equal(_bits(out[:, 3]), _bits(ref[:, 3])), "filter %d: max |d rho~| = %g" % (ftype, np.abs(out[:, 3] - ref[:, 3]).max())


@deep
def test_trajectory(name):
    """f: twelve steps from _perturb's noise on the mean velocity (4, -3, 2), a rebuild every four steps, and the rebuild the
    thirteenth step would start with (tests/test_grid_edge_cases.py: by then particles have left through every periodic face,
    z included, and calcHash brings them back into the cell they left where the axis has one cell).  The trajectory bars of
    tests/test_gpu_parity.py: hash and info equal, positions 1e-6 of a cell per step, velocities 1e-3 of max |v|, rho~ 2e-6"""
    steps = ge.TRAJ_STEPS
    prob = ge.trajectory_problem(name)
    eng = _engine(prob)
    sim = ol.OracleSim(prob)
    _perturb(sim, eng, 31)
    for _ in range(steps):
        sim.step(); eng.step()
    assert tiles_usable(eng) == 1
    sim.build_neibs(); eng.build_neibs()
    assert tiles_usable(eng) == 1
    out = eng.download()
    n = eng.n
    assert n == sim.n and abs(eng.current_dt() - sim.dt) <= 1e-4*sim.dt
    assert np.array_equal(out["hash"], sim.hash[:n]) and np.array_equal(out["info"].reshape(-1, 4), sim.info[:n])
    assert np.abs(out["pos"][:, :3] - sim.pos[:n, :3]).max() <= 1e-6*float(min(prob.m_cellsize))*steps
    assert np.abs(out["vel"][:, :3] - sim.vel[:n, :3]).max() <= 1e-3*np.abs(sim.vel[:n, :3]).max()
    assert np.abs(out["vel"][:, 3] - sim.vel[:n, 3]).max() <= 2e-6
