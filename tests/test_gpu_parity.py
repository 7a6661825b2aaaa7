"""GPU parity: the HIP path, called through the C ABI, against the CPU oracle on identical inputs.

Bar (DESIGN.md "Parity"):
  * hash, sort permutation, sorted info, cellStart/End, reordered pos/vel, neighbour lists,
    neighbour counters, Euler update: BIT-EXACT;
  * forces / CFL / dt: relative tolerance 2e-5 of the largest |force| (fast v_log/v_exp/v_rcp
    path vs powf and IEEE division in the oracle), stated per test;
  * N-step trajectories (<= 25 steps, spanning re-sorts): positions 1e-6 of a cell per step, velocities
    1e-3 of max|v|, rho~ 1e-6 absolute.  The Tait EOS evaluates P = B((rho~+1)^7 - 1) with rho~ ~ 1e-3, i.e.
    with an inherent relative conditioning of ~1e-4 in fp32 whatever pow is used (the reference's own
    __powf included), so per-step force differences of 2e-5 accumulate to this level.
"""
import ctypes as C
import numpy as np
import pytest

import oracle_lib as ol
from gpusph_amd import defs as D
from gpusph_amd.problem import DamBreak3D

pytestmark = pytest.mark.gpu


def _engine(problem, **kw):
    import torch
    from gpusph_amd.engine import TimestepEngine
    assert torch.cuda.is_available()
    return TimestepEngine(problem, device="cuda:0", **kw)


def _np(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


CASES = [
    dict(deltap=0.04, obstacle=True),
    dict(deltap=0.03, obstacle=False, jitter=0.1),
    dict(deltap=0.025, obstacle=True, jitter=0.05, linearization="xzy"),
]


@pytest.mark.parametrize("case", CASES)
def test_neibs_phase_bit_exact(case):
    prob = DamBreak3D(**case)
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs()
    eng.build_neibs()
    n = eng.n
    assert n == sim.n
    assert np.array_equal(_np(eng.hash, np.uint32)[:n], sim.hash[:n])
    assert np.array_equal(_np(eng.info, np.uint16)[:n], sim.info[:n])
    assert np.array_equal(_np(eng.partindex, np.uint32)[:n], sim.partindex[:n])
    assert np.array_equal(_np(eng.cellStart, np.uint32), sim.cs)
    assert np.array_equal(_np(eng.cellEnd, np.uint32), sim.ce)
    assert np.array_equal(_np(eng.pos)[:n].view(np.uint32), sim.pos[:n].view(np.uint32))
    assert np.array_equal(_np(eng.vel)[:n].view(np.uint32), sim.vel[:n].view(np.uint32))
    assert np.array_equal(_np(eng.neibslist, np.uint16), sim.nl)
    info = eng.neibs_info()
    assert info.numInteractions == sim.neibs_info.numInteractions
    assert info.maxFluidBoundaryNeibs == sim.neibs_info.maxFluidBoundaryNeibs
    assert info.hasTooManyNeibs == -1


MFMA_CASES = {
    "dambreak-xzy": lambda: DamBreak3D(0.02, obstacle=True, jitter=0.05, linearization="xzy"),
    "dambreak-yzx": lambda: DamBreak3D(0.025, obstacle=True, jitter=0.1, linearization="yzx"),
    "dambreak-zxy": lambda: DamBreak3D(0.04, obstacle=True, jitter=0.1, linearization="zxy"),          # COORD1 = z: every lane goes to the general walk
    "lj-testpoints": lambda: DamBreak3D(0.03, boundary=D.LJ_BOUNDARY, jitter=0.1, linearization="yzx", testpoints=((0.5, 0.3, 0.1), (1.2, 0.33, 0.2))),
    "gaussian": lambda: DamBreak3D(0.04, kerneltype=D.GAUSSIAN, jitter=0.1, linearization="xzy"),      # cells of ~60 particles: rows beyond six tiles
    "periodic-xyz": lambda: __import__("gpusph_amd.problem", fromlist=["PeriodicBox"]).PeriodicBox(
        n=(14, 12, 11), linearization="xzy", velocity=(0.4, 0.3, -0.2)),                   # first / last cell of a periodic COORD1
    "dambreak-1M": lambda: DamBreak3D(DamBreak3D.deltap_for(1.0e6), obstacle=True, hydrostatic=False, jitter=0.05, linearization="xzy"),
}


@pytest.mark.parametrize("name", sorted(MFMA_CASES))
def test_list_build_on_the_matrix_cores_bit_exact(name, monkeypatch):
    """SPHX_NEIBS_MFMA=1: the distance tests of the list build as v_mfma_f32_32x32x2_f32 products with the reference's arithmetic
    inside the band where the product's verdict is not trusted (neibs_build.hip; off by default: measured slower than the general
    walk).  Every list entry, the counters and the section lengths behind the tile lists (a tiled forces pass on them agrees with
    the gather kernel) -- including the lanes the prepass hands to the general walk (COORD1 = z, periodic COORD1, long rows)."""
    monkeypatch.setenv("SPHX_NEIBS_MFMA", "1")      # read when the context is created
    prob = MFMA_CASES[name]()
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs(); eng.build_neibs()            # (the same inputs on both sides: the initial state, jittered)
    n = eng.n
    assert n == sim.n and np.array_equal(_np(eng.hash, np.uint32)[:n], sim.hash[:n])
    assert np.array_equal(_np(eng.neibslist, np.uint16), sim.nl)
    info = eng.neibs_info()
    assert info.numInteractions == sim.neibs_info.numInteractions
    assert info.maxFluidBoundaryNeibs == sim.neibs_info.maxFluidBoundaryNeibs and info.hasTooManyNeibs == -1


def test_many_inactive_particles_sort_without_a_quadratic_bin():
    """1e5 disabled particles (outflow, disableFreeSurfParts at scale): they all share the CELL_HASH_MAX bin.  The
    active prefix is bit-identical to the oracle's (hash, info, permutation, cells, lists), the tail holds exactly the
    disabled particles, and the rebuild does not take seconds (the in-bin rank is quadratic; big inactive bins skip it)"""
    import time
    import torch
    prob = DamBreak3D(DamBreak3D.deltap_for(5.0e5), obstacle=False, hydrostatic=False)
    n0 = prob.num_particles
    assert n0 > 400_000
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.step(); eng.step()                       # iteration 0 -> 1 (so that the next rebuild goes through calcHash)
    rng = np.random.default_rng(17)
    fluid_idx = np.nonzero((sim.info[:n0, 0] & 7) == 0)[0]          # calcHash re-hashes fluid particles (fixed boundaries keep theirs)
    kill = rng.choice(fluid_idx, size=100_000, replace=False)
    sim.pos[kill, 3] = np.nan
    eng.pos[torch.from_numpy(kill).to(eng.device), 3] = float("nan")
    sim.iterations = eng.iterations = prob.simparams.buildneibsfreq        # force a rebuild now
    torch.cuda.synchronize(); t0 = time.perf_counter()
    eng.build_neibs()
    torch.cuda.synchronize(); t_rebuild = time.perf_counter() - t0
    sim.build_neibs()
    n = eng.n
    assert n == sim.n == n0 - 100_000
    assert t_rebuild < 0.25, "rebuild took %.3f s" % t_rebuild
    assert np.array_equal(_np(eng.hash, np.uint32)[:n], sim.hash[:n])
    assert np.array_equal(_np(eng.info, np.uint16)[:n], sim.info[:n])
    assert np.array_equal(_np(eng.partindex, np.uint32)[:n], sim.partindex[:n])
    assert np.array_equal(_np(eng.cellStart, np.uint32), sim.cs) and np.array_equal(_np(eng.cellEnd, np.uint32), sim.ce)
    assert np.array_equal(_np(eng.pos)[:n].view(np.uint32), sim.pos[:n].view(np.uint32))
    assert np.array_equal(_np(eng.neibslist, np.uint16).reshape(-1, eng.alloc)[:, :n], sim.nl.reshape(-1, eng.alloc)[:, :n])
    tail = _np(eng.hash, np.uint32)[n:n0]
    assert (tail == 0xFFFFFFFF).all()
    ids = lambda info: info[:, 2].astype(np.uint32) | (info[:, 3].astype(np.uint32) << 16)
    assert np.array_equal(np.sort(ids(_np(eng.info, np.uint16)[n:n0])), np.sort(ids(sim.info[n:n0])))   # the same particles


@pytest.mark.parametrize("case", CASES[:2])
def test_forces_and_dt_tolerance(case):
    import torch
    prob = DamBreak3D(**case)
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs()
    eng.build_neibs()
    n = eng.n
    # give the particles some velocity / density perturbation so every term is exercised
    rng = np.random.default_rng(7)
    vel = sim.vel.copy()
    fluid = (sim.info[:, 0] & 7) == 0
    vel[fluid, :3] += rng.uniform(-0.3, 0.3, size=(fluid.sum(), 3)).astype(np.float32)
    vel[:, 3] += rng.uniform(0, 2e-3, size=len(vel)).astype(np.float32)
    sim.vel = vel
    eng.vel[:n] = torch.from_numpy(vel[:n]).to(eng.device)
    cof = 1 if prob.simparams.numforcesbodies else 0
    f_ref, cfl_ref, nb, rbf_ref, rbt_ref = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n,
                                                      compute_object_forces=cof, rb_count=prob.num_obstacle)
    dt_ref = sim.o.dtreduce(cfl_ref, nb, sim.sspeed_cfl)
    eng._forces(eng.pos, eng.vel, 1, 0)
    f = _np(eng.forces)[:n]
    scale = np.abs(f_ref[:, :3]).max()
    assert np.abs(f[:, :3] - f_ref[:n, :3]).max() <= 2e-5 * scale
    wscale = np.abs(f_ref[:, 3]).max()
    assert np.abs(f[:, 3] - f_ref[:n, 3]).max() <= 2e-5 * wscale + 1e-7
    # the CFL array is only ever max-reduced (dtreduce); the tiled kernel bins its maxima differently
    # from the reference's one-block-one-entry layout, so the contract is the maximum
    cfl = _np(eng.cfl)[:nb]
    assert abs(cfl.max() - cfl_ref[:nb].max()) <= 2e-5 * cfl_ref[:nb].max()
    dt = float(eng.d_dt_next.item())
    assert abs(dt - dt_ref) <= 2e-5 * dt_ref
    if prob.num_obstacle:
        rbf = _np(eng.rbforces)
        assert np.abs(rbf - rbf_ref).max() <= 2e-5 * max(np.abs(rbf_ref).max(), 1e-12)
        tf, tt = eng.reduce_rb_forces()
        assert np.allclose(tf, rbf_ref[:, :3].sum(axis=0, dtype=np.float64), rtol=1e-4, atol=1e-6 * np.abs(rbf_ref).max())


def test_euler_bit_exact():
    import torch
    prob = DamBreak3D(deltap=0.04, obstacle=True)
    eng = _engine(prob)
    sim = ol.OracleSim(prob)
    sim.build_neibs(); eng.build_neibs()
    n = eng.n
    rng = np.random.default_rng(3)
    forces = rng.normal(0, 5, size=(len(sim.pos), 4)).astype(np.float32)
    vel = sim.vel + rng.normal(0, 0.1, size=sim.vel.shape).astype(np.float32)
    eng.forces[:n] = torch.from_numpy(forces[:n]).to(eng.device)
    eng.vel[:n] = torch.from_numpy(vel[:n]).to(eng.device)
    dt = float(np.float32(3.1e-4))
    eng.d_dt.fill_(dt)
    for step, scale in ((1, 0.5), (2, 1.0)):
        pr, vr = sim.o.euler(sim.pos, vel, sim.info, sim.hash, forces, n, float(np.float32(dt) * np.float32(scale)), step)
        eng._euler(step, scale)
        assert np.array_equal(_np(eng.pos2)[:n].view(np.uint32), pr[:n].view(np.uint32))
        assert np.array_equal(_np(eng.vel2)[:n].view(np.uint32), vr[:n].view(np.uint32))


# Multi-step comparisons avoid sitting ON the Colagrossi switch: the diffusion term is applied only when
# |P_i - P_j| >= |rho_i g.r_ij| (forces_kernel.def:1933-1936), and a hydrostatic column satisfies this with
# EQUALITY up to rounding for every vertical pair, so which pairs diffuse is decided by the last bit of P
# (true of the reference's own __powf build as well).  Case A starts from rho~ = 0 with diffusion on, case B
# from the hydrostatic state with diffusion off; test_forces_and_dt_tolerance covers single evaluations.
# (case, steps, bound on the velocities in units of the largest, bound on rho~)
TRAJ = [
    (dict(deltap=0.04, obstacle=True, hydrostatic=False), 25, 1e-3, 2e-6),
    # BASELINE configs[0] as it is worded: DamBreak3D dp = 0.04, 100 steps.  The per-step differences (2e-5 of the forces, and a
    # Colagrossi pair decided differently now and then) add up over four times as many steps and ten rebuilds
    (dict(deltap=0.04, obstacle=True, hydrostatic=False), 100, 4e-3, 6e-5),
    (dict(deltap=0.03, obstacle=False, jitter=0.1, density_diffusion=D.DENSITY_DIFFUSION_NONE), 12, 1e-3, 2e-6),
]


@pytest.mark.parametrize("case,steps,vtol,rtol", TRAJ)
def test_n_steps_trajectory(case, steps, vtol, rtol):
    """config 1 style run (spans re-sorts): integer outputs exact while positions stay bit-close,
    floating fields within the stated tolerance."""
    prob = DamBreak3D(**case)
    eng = _engine(prob)
    sim = ol.OracleSim(prob)
    for _ in range(steps):
        sim.step()
        eng.step()
    out = eng.download()
    n = eng.n
    assert n == sim.n
    assert abs(eng.current_dt() - sim.dt) <= 1e-4 * sim.dt
    # same particles in the same slots (sort keys are integers; a flipped cell assignment would
    # show up here) -- allow a handful of cell-boundary flips caused by 1-ulp position differences
    same = (out["info"] == sim.info[:n]).all(axis=1)
    assert same.mean() > 0.999
    ids_g = out["info"][:, 2].astype(np.uint32) | (out["info"][:, 3].astype(np.uint32) << 16)
    ids_o = sim.info[:n, 2].astype(np.uint32) | (sim.info[:n, 3].astype(np.uint32) << 16)
    og = np.argsort(ids_g); oo = np.argsort(ids_o)
    gp = prob.global_pos(out["pos"][og], out["hash"][og])
    op = prob.global_pos(sim.pos[:n][oo], sim.hash[:n][oo])
    assert np.abs(gp - op).max() <= 1e-6 * prob.m_cellsize.min() * steps
    vscale = max(np.abs(sim.vel[:n, :3]).max(), 1e-3)
    assert np.abs(out["vel"][og][:, :3] - sim.vel[:n][oo][:, :3]).max() <= vtol * vscale
    assert np.abs(out["vel"][og][:, 3] - sim.vel[:n][oo][:, 3]).max() <= rtol


def test_full_size_properties():
    """BASELINE-size properties that need no oracle: sortedness, permutation, list symmetry."""
    prob = DamBreak3D(DamBreak3D.deltap_for(1.0e6), obstacle=True)
    eng = _engine(prob, clobber_neibslist=True)
    for _ in range(11):
        eng.step()
    n = eng.n
    h = _np(eng.hash, np.uint32)[:n]
    assert (np.diff(h.astype(np.int64)) >= 0).all()                       # sorted by cell
    pidx = np.sort(_np(eng.partindex, np.uint32)[:n])
    assert np.array_equal(pidx, np.arange(n, dtype=np.uint32))             # a permutation
    cs = _np(eng.cellStart, np.uint32); ce = _np(eng.cellEnd, np.uint32)
    occ = cs != 0xFFFFFFFF
    assert int((ce[occ] - cs[occ]).sum()) == n                             # cells partition the particles
    info = eng.neibs_info()
    assert info.hasTooManyNeibs == -1
    assert 0 < info.maxFluidBoundaryNeibs < 127
    out = eng.download()
    assert np.isfinite(out["pos"]).all() and np.isfinite(out["vel"]).all() and np.isfinite(out["forces"]).all()
    # the column starts hydrostatic: the mean vertical acceleration of the fluid lies between free fall and rest
    fluid = (out["info"][:, 0] & 7) == 0
    assert -9.81 < out["forces"][fluid, 2].mean() < 1.0
    dt = eng.current_dt()
    assert 0 < dt <= prob.simparams.dt * 1.0001


def _full_size_case(name):
    from gpusph_amd.problem import StillWater
    if name == "dambreak_1M":      # BASELINE configs[1]: DamBreak3D ~1 M particles, Wendland, artificial viscosity
        return DamBreak3D(DamBreak3D.deltap_for(1.0e6), obstacle=True, hydrostatic=False)
    if name == "dambreak_8M":      # the size BASELINE's per-GPU roofline target is quoted at
        return DamBreak3D(DamBreak3D.deltap_for(8.0e6), obstacle=True, hydrostatic=False)
    if name == "dambreak_32M":     # BASELINE configs[3], the bench workload itself (31.8 M particles on the one GPU)
        return DamBreak3D(DamBreak3D.deltap_for(32.0e6), obstacle=True, hydrostatic=False)
    if name == "stillwater_4M":    # BASELINE configs[2]: StillWater 4 M particles, SPS viscosity (engine_visc path), DYN walls
        return StillWater(StillWater.ppH_for(4.0e6), viscosity="SPSVISC")
    if name == "wavetank_8M":      # BASELINE configs[4]: WaveTank, moving paddle, planes + LJ box, SPS viscosity, 8 M particles
        from gpusph_amd.problem import WaveTank
        return WaveTank(0.005, paddle_tstart=0.0)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["dambreak_1M", "stillwater_4M", "dambreak_8M", "wavetank_8M", "dambreak_32M"])
def test_full_size_against_the_oracle(name):
    """BASELINE configs[1], configs[2], configs[3] (the bench workload) and the option set of configs[4] at their FULL sizes against the
    OpenMP oracle (seconds per step on the box's cores): neighbour phase bit-exact, one forces evaluation within 2e-5 of the largest
    force (incl. the SPS stress tensor for StillWater), then a 3-step trajectory with the usual tolerances (not at 32 M: the
    neighbour phase and the forces evaluation are what the bench times; three oracle steps there are minutes of CPU)."""
    import os
    import torch
    ol.lib().orc_set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
    prob = _full_size_case(name)
    assert prob.num_particles > {"dambreak_1M": 0.95e6, "stillwater_4M": 3.9e6, "dambreak_8M": 7.9e6, "wavetank_8M": 7.8e6, "dambreak_32M": 31.0e6}[name]
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs(); eng.build_neibs()
    n = eng.n
    assert n == sim.n
    assert np.array_equal(_np(eng.hash, np.uint32)[:n], sim.hash[:n])
    assert np.array_equal(_np(eng.info, np.uint16)[:n], sim.info[:n])
    assert np.array_equal(_np(eng.cellStart, np.uint32), sim.cs) and np.array_equal(_np(eng.cellEnd, np.uint32), sim.ce)
    assert np.array_equal(_np(eng.pos)[:n].view(np.uint32), sim.pos[:n].view(np.uint32))
    # every list of every particle (slot rows in slices: at 32 M the list is 8 GB on either side)
    rows = int(eng.sp.neiblistsize)
    dev_nl, ref_nl = eng.neibslist.view(rows, -1), np.asarray(sim.nl).reshape(rows, -1)
    for r0 in range(0, rows, 16):
        assert np.array_equal(_np(dev_nl[r0:r0 + 16], np.uint16), ref_nl[r0:r0 + 16]), "slots %d..%d" % (r0, r0 + 15)
    info = eng.neibs_info()
    assert info.numInteractions == sim.neibs_info.numInteractions and info.hasTooManyNeibs == -1
    # one forces evaluation on a perturbed state
    rng = np.random.default_rng(11)
    vel = sim.vel.copy()
    fluid = (sim.info[:, 0] & 7) == 0
    vel[fluid, :3] += rng.uniform(-0.2, 0.2, size=(int(fluid.sum()), 3)).astype(np.float32)
    vel[:, 3] += rng.uniform(0, 1e-3, size=len(vel)).astype(np.float32)
    sim.vel = vel
    eng.vel[:n] = torch.from_numpy(vel[:n]).to(eng.device)
    sps = prob.simparams.turbmodel == D.SPS
    tau_ref = sim.o.sps(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, n)[0] if sps else None
    f_ref, cfl_ref, nb, _, _ = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, tau=tau_ref,
                                            compute_object_forces=1 if prob.simparams.numforcesbodies else 0,
                                            rb_count=getattr(prob, "num_obstacle", 0))
    eng._forces(eng.pos, eng.vel, 1, 0)
    f = _np(eng.forces)[:n]
    scale = np.abs(f_ref[:n, :3]).max()
    err = np.abs(f[:, :3] - f_ref[:n, :3]).max()
    assert err <= 2e-5 * scale, "forces: %g of %g" % (err, scale)
    # d(rho~)/dt: the Colagrossi term is switched per pair by |P_i - P_j| >= |rho_i g.r_ij| (forces_kernel.def:1933-1936);
    # among ~6e7 pairs a few sit within an ulp of P of that threshold and the two powf implementations (device, glibc)
    # decide them differently.  Such a particle differs by ONE pair's diffusion term; everything else holds 2e-5
    dw = np.abs(f[:, 3] - f_ref[:n, 3])
    wscale = np.abs(f_ref[:n, 3]).max()
    flipped = dw > 2e-5 * wscale + 1e-7
    assert flipped.sum() <= max(2, int(3e-5 * n)), "%d particles beyond tolerance" % flipped.sum()
    if prob.simparams.densitydiffusiontype == D.COLAGROSSI:
        from kernel_agreement import colagrossi_flips_are_single_pairs
        assert dw.max() <= 1e-3 * wscale          # one pair's diffusion term, far below the field's scale
        colagrossi_flips_are_single_pairs(prob, sim, n, f[:, 3], f_ref[:n, 3], flipped)     # ... and exactly that: recomputed pair by pair
    else:
        assert not flipped.any()
    if sps:
        tau = np.concatenate([_np(t)[:n] for t in eng.tau], axis=1)
        assert np.abs(tau - tau_ref[:n]).max() <= 2e-5 * np.abs(tau_ref[:n]).max()
    if name == "dambreak_32M":
        return
    # three steps from the perturbed state
    for _ in range(3):
        sim.step(); eng.step()
    out = eng.download()
    assert abs(eng.current_dt() - sim.dt) <= 1e-4 * sim.dt
    assert np.array_equal(out["info"], sim.info[:n])
    assert np.abs(out["pos"][:, :3] - sim.pos[:n, :3]).max() <= 3e-6 * prob.m_cellsize.min()
    vscale = max(np.abs(sim.vel[:n, :3]).max(), 1e-3)
    assert np.abs(out["vel"][:, :3] - sim.vel[:n, :3]).max() <= 1e-4 * vscale
    assert np.abs(out["vel"][:, 3] - sim.vel[:n, 3]).max() <= 3e-6     # a flipped Colagrossi pair (see above) times 3 dt


def test_full_size_32M_tiled_equals_generic_and_invariants():
    """BASELINE configs[3] size (the bench workload, 31.8 M particles) through properties that need no oracle: the two
    independent HIP implementations of the forces pass (LDS-tiled, gather) agree to rounding (kernel_agreement.py) for every
    particle and in dt after a few steps and a neighbour rebuild; hash sorted, cells partition the particles, list within capacity"""
    import torch
    prob = DamBreak3D(DamBreak3D.deltap_for(32.0e6), obstacle=True)
    eng = _engine(prob, track_particle_count=False)
    for _ in range(11):            # crosses the rebuild at iteration 10
        eng.step()
    n = eng.n
    assert n > 31_000_000
    h = eng.hash[:n].to(torch.int64) & 0xFFFFFFFF
    assert bool((h[1:] >= h[:-1]).all())
    cs = eng.cellStart.to(torch.int64) & 0xFFFFFFFF; ce = eng.cellEnd.to(torch.int64) & 0xFFFFFFFF
    occ = cs != 0xFFFFFFFF
    assert int((ce[occ] - cs[occ]).sum().item()) == n
    info = eng.neibs_info()
    assert info.hasTooManyNeibs == -1 and 0 < info.maxFluidBoundaryNeibs < 127
    eng._forces(eng.pos, eng.vel, 1, 0)
    f_tiled = eng.forces[:n].clone(); dt_tiled = float(eng.d_dt_next.item())
    assert bool(torch.isfinite(f_tiled).all())
    own = eng.neibslist
    eng.neibslist = own.clone()    # a list this context did not build: the forces engine takes the generic kernel
    eng.forces.zero_()
    eng._forces(eng.pos, eng.vel, 1, 0)
    eng.neibslist = own
    from kernel_agreement import assert_forces_agree
    assert_forces_agree(f_tiled.cpu().numpy(), eng.forces[:n].cpu().numpy())
    assert abs(float(eng.d_dt_next.item()) - dt_tiled) <= 1e-5 * dt_tiled
    fluid = (eng.info[:n, 0].to(torch.int32) & 7) == 0
    az = f_tiled[fluid, 2].mean().item()
    assert -9.81 < az < 1.0


def test_against_committed_golden_fixture():
    """tests/golden/oracle_pipeline.npz (inputs + expected outputs, made by tests/golden/make_golden.py):
    the GPU path reproduces the committed integer outputs bit-for-bit and the floating ones within tolerance."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_pipeline.npz"))
    prob = DamBreak3D(float(g["deltap"]), obstacle=True, jitter=0.05, hydrostatic=False)
    arrs = prob.copy_to_array()
    assert np.array_equal(arrs["pos"].view(np.uint32), g["in_pos"].view(np.uint32))
    eng = _engine(prob, clobber_neibslist=True)
    eng.step()
    n = eng.n
    assert np.array_equal(_np(eng.hash, np.uint32)[:n], g["s1_hash"][:n])
    assert np.array_equal(_np(eng.info, np.uint16)[:n], g["s1_info"][:n])
    assert np.array_equal(_np(eng.partindex, np.uint32)[:n], g["s1_partindex"][:n])
    assert np.array_equal(_np(eng.cellStart, np.uint32), g["s1_cellStart"])
    assert np.array_equal(_np(eng.cellEnd, np.uint32), g["s1_cellEnd"])
    assert np.array_equal(_np(eng.neibslist, np.uint16), g["s1_neibs"])
    info = eng.neibs_info()
    assert info.numInteractions == int(g["s1_numInteractions"]) and info.maxFluidBoundaryNeibs == int(g["s1_maxneibs"])
    f = _np(eng.forces)[:n]
    scale = np.abs(g["s1_forces"][:, :3]).max()
    assert np.abs(f[:, :3] - g["s1_forces"][:n, :3]).max() <= 2e-5 * scale
    assert abs(eng.current_dt() - float(g["s1_dt"])) <= 2e-5 * float(g["s1_dt"])
    for _ in range(10):
        eng.step()
    out = eng.download()
    same = (out["info"] == g["s11_info"][:n]).all(axis=1)
    assert same.mean() > 0.999
    sel = same
    assert np.abs(out["vel"][sel][:, :3] - g["s11_vel"][:n][sel][:, :3]).max() <= 1e-3 * max(np.abs(g["s11_vel"][:, :3]).max(), 1e-3)


LJ_CASES = [dict(deltap=0.04, obstacle=True, jitter=0.2, hydrostatic=False, viscosity="KINEMATICVISC", kinematic_visc=0.05),
            dict(deltap=0.04, obstacle=True, jitter=0.2, hydrostatic=False, boundary=D.LJ_BOUNDARY),
            dict(deltap=0.04, obstacle=False, jitter=0.3, hydrostatic=False, boundary=D.LJ_BOUNDARY, walls="planes"),
            dict(deltap=0.04, obstacle=True, jitter=0.2, hydrostatic=False, boundary=D.MK_BOUNDARY),
            # two fluids in the tiled kernel (fluid number tag in the EOS row): Colagrossi between same-fluid pairs only,
            # per-fluid non-constant viscosity, LJ walls
            dict(deltap=0.04, obstacle=False, jitter=0.2, hydrostatic=False, two_fluids=True),
            dict(deltap=0.04, obstacle=True, jitter=0.2, hydrostatic=False, two_fluids=True, kinematic_visc=0.05,
                 viscosity=dict(rheologytype=D.NEWTONIAN, turbmodel=D.LAMINAR_FLOW, compvisc=D.KINEMATIC, avgop=D.HARMONIC,
                                is_const_visc=False)),
            dict(deltap=0.04, obstacle=False, jitter=0.2, hydrostatic=False, two_fluids=True, boundary=D.LJ_BOUNDARY,
                 density_diffusion=D.DENSITY_DIFFUSION_NONE),
            # SPS stress tensor rows in the LDS window (smaller window capacity): WaveTank's viscosity<SPSVISC>, and two fluids
            dict(deltap=0.04, obstacle=True, jitter=0.2, hydrostatic=False, viscosity="SPSVISC", kinematic_visc=1.0e-3),
            dict(deltap=0.03, obstacle=False, jitter=0.2, hydrostatic=True, viscosity="SPSVISC", kinematic_visc=1.0e-6, two_fluids=True),
            # Ferrari density diffusion in the tiled kernel (StillWater's default): DYN walls with a feedback body, two fluids + LJ
            dict(deltap=0.04, obstacle=True, jitter=0.2, hydrostatic=False, density_diffusion=D.FERRARI,
                 viscosity="DYNAMICVISC", kinematic_visc=3.0e-2),
            dict(deltap=0.04, obstacle=False, jitter=0.2, hydrostatic=False, two_fluids=True, boundary=D.LJ_BOUNDARY,
                 density_diffusion=D.FERRARI)]


@pytest.mark.parametrize("case", CASES + LJ_CASES)
def test_tiled_and_generic_kernels_agree(case, monkeypatch):
    """the LDS-tiled forces kernel and the generic gather kernel implement the same sum in the same order; the tiled one in
    the tile's frame of reference: agreement to rounding (kernel_agreement.py)"""
    import torch
    prob = DamBreak3D(**case)
    outs = []
    for disable in ("0", "1"):
        monkeypatch.setenv("SPHX_DISABLE_TILES", disable)
        eng = _engine(prob, clobber_neibslist=True)
        eng.build_neibs()
        n = eng.n
        rng = np.random.default_rng(11)
        vel = _np(eng.vel).copy()
        vel[:n, :3] += rng.uniform(-0.3, 0.3, size=(n, 3)).astype(np.float32)
        vel[:n, 3] += rng.uniform(0, 2e-3, size=n).astype(np.float32)
        eng.vel.copy_(torch.from_numpy(vel).to(eng.device))
        eng._forces(eng.pos, eng.vel, 1, 0)
        tau = np.concatenate([_np(t)[:n] for t in eng.tau], axis=1) if getattr(eng, "tau", None) else np.zeros((n, 6), np.float32)
        outs.append((_np(eng.forces)[:n].copy(), float(eng.d_dt_next.item()), _np(eng.rbforces).copy(), tau.copy()))
    from kernel_agreement import assert_forces_agree
    assert_forces_agree(outs[0][0], outs[1][0])
    assert abs(outs[0][1] - outs[1][1]) <= 1e-5 * outs[1][1]
    if np.abs(outs[1][2]).max() > 0:
        assert_forces_agree(outs[0][2], outs[1][2], what="rigid-body rows")
    # SPS: the stress mode of the tiled kernel (single fluid) and sps_kernel give the same tensor
    if np.abs(outs[1][3]).max() > 0:
        assert_forces_agree(outs[0][3], outs[1][3], what="SPS stress tensor")
    if case.get("viscosity") == "SPSVISC":
        assert np.abs(outs[0][3]).max() > 0


def test_multigpu_engine_world1_equals_single_engine():
    """HipKernels + MultiGpuEngine plumbing on the GPU: with one rank it is the single-GPU engine"""
    from gpusph_amd.multigpu import MultiGpuEngine
    prob = DamBreak3D(0.03, obstacle=True, jitter=0.05)
    a = _engine(prob)
    b = MultiGpuEngine(prob, "cuda:0", 0, 1)
    for _ in range(12):
        a.step(); b.step()
    n = a.n
    assert b.n_int == n
    assert np.array_equal(_np(a.pos)[:n].view(np.uint32), _np(b.pos)[:n].view(np.uint32))
    assert np.array_equal(_np(a.vel)[:n].view(np.uint32), _np(b.vel)[:n].view(np.uint32))
    assert a.current_dt() == b.current_dt()


_MG_CASES = {
    "default": (dict(), ()),
    "spsvisc+shepard": (dict(viscosity="SPSVISC", kinematic_visc=1.0e-6), ((0, 4),)),
    # StillWater's option set (laminar viscosity + Ferrari diffusion in the tiled stripes, MLS filter) and two fluids
    "dynamicvisc+ferrari+mls": (dict(viscosity="DYNAMICVISC", kinematic_visc=3.0e-2, density_diffusion=D.FERRARI), ((1, 4),)),
    "two-fluids": (dict(two_fluids=True), ()),
    # ENABLE_XSPH: the mean neighbourhood velocity of the particles next to the cut is formed from halo rows as well
    "xsph": (dict(xsph=True), ()),
    # the fidelity engines under the slab decomposition: sigma / densities exchanged after COMPUTE_DENSITY and the volumes with
    # the halo (SPH_GRENIER); the energy rate with the forces (internal energy); the stripes through the SPH_HA routing
    "grenier": (dict(obstacle=False, two_fluids=True, formulation=D.SPH_GRENIER, viscosity="DYNAMICVISC", density_diffusion=D.DENSITY_DIFFUSION_NONE), ()),
    "internal-energy": (dict(obstacle=False, internal_energy=True), ()),
    "sph-ha": (dict(obstacle=False, two_fluids=True, formulation=D.SPH_HA, density_diffusion=D.COLAGROSSI,
                    viscosity=dict(rheologytype=D.NEWTONIAN, turbmodel=D.LAMINAR_FLOW, compvisc=D.DYNAMIC, avgop=D.HARMONIC)), ()),
    # SA walls, density summation + dynamic gamma + Brezzi: every SA pass on the internal particles, then the halo import
    "sa-walls": (dict(problem="SABox", deltap=0.04, options="StillWaterSA", jitter=0.1), ()),
    # k-epsilon on SA walls: k, epsilon, eddy viscosity and Eulerian velocity with the halo, DKDE with the forces
    "sa-keps": (dict(problem="SABox", deltap=0.04, jitter=0.1, viscosity=dict(rheologytype=D.NEWTONIAN, turbmodel=D.KEPSILON)), ()),
}


def _mg_problem(kw):
    kw = dict(kw)
    if kw.pop("problem", None) == "SABox":
        from gpusph_amd.problem import SABox
        return SABox(**kw)
    xsph = kw.pop("xsph", False)
    prob = DamBreak3D(**{**dict(deltap=0.03, obstacle=True, jitter=0.05, linearization="xzy"), **kw})
    if xsph:
        prob.simparams.simflags |= D.ENABLE_XSPH
    return prob



def _mg_worker(rank, world, port, outdir, casename):
    import os, sys
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    from gpusph_amd.multigpu import MultiGpuEngine
    dist.init_process_group("gloo", rank=rank, world_size=world)      # one GPU on this box: RCCL needs one per rank
    kw, filters = _MG_CASES[casename]
    prob = _mg_problem(kw)
    eng = MultiGpuEngine(prob, "cuda:0", rank, world)
    for f in filters:
        eng.add_filter(*f)
    for _ in range(12):
        eng.step()
    torch.cuda.synchronize()
    out = eng.download_internal()
    np.savez(os.path.join(outdir, "g%d.npz" % rank), dt=eng.current_dt(), **out)
    dist.barrier(); dist.destroy_process_group()


@pytest.mark.parametrize("casename,kernels", [(c, "generic") for c in sorted(_MG_CASES)] + [("default", "tiled"), ("spsvisc+shepard", "tiled"), ("sa-walls", "tiled")])
def test_two_ranks_on_one_gpu_equal_single_domain(tmp_path, casename, kernels, monkeypatch):
    """the real HIP kernels under the slab decomposition (2 ranks sharing the one GPU of this box, host-staged
    gloo transport standing in for RCCL), including the overlapped edge-stripe / inner-stripe forces.
    With the gather kernels every particle sees the same arithmetic whatever the decomposition: bit-identical to the
    single-domain run.  The LDS-tiled kernels work in a frame per tile and the slabs tile differently, so there the two
    runs agree to rounding (12 steps: positions to 1e-6 of a cell per step, velocities to 1e-4 of the largest)."""
    import socket
    import torch.multiprocessing as mp
    monkeypatch.setenv("SPHX_DISABLE_TILES", "1" if kernels == "generic" else "0")     # read when a context is created; the workers inherit it
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_mg_worker, args=(2, port, str(tmp_path), casename), nprocs=2, join=True)
    kw, filters = _MG_CASES[casename]
    prob = _mg_problem(kw)
    ref = _engine(prob)
    for f in filters:
        ref.add_filter(*f)
    for _ in range(12):
        ref.step()
    n = ref.n
    parts = [np.load(str(tmp_path / ("g%d.npz" % r))) for r in range(2)]
    ids = np.concatenate([p["info"][:, 2].astype(np.uint32) | (p["info"][:, 3].astype(np.uint32) << 16) for p in parts])
    order = np.argsort(ids)
    rinfo = _np(ref.info, np.uint16)[:n]
    rid = rinfo[:, 2].astype(np.uint32) | (rinfo[:, 3].astype(np.uint32) << 16)
    ro = np.argsort(rid)
    assert np.array_equal(ids[order], rid[ro])
    if kernels == "tiled":
        cs = float(min(prob.m_cellsize))
        got = np.concatenate([p["pos"] for p in parts])[order]; want = _np(ref.pos)[:n][ro]
        assert np.array_equal(got[:, 3].view(np.uint32), want[:, 3].view(np.uint32))
        hg = np.concatenate([p["hash"] for p in parts])[order] if "hash" in parts[0] else None
        same_cell = np.ones(n, bool) if hg is None else (hg & 0x3FFFFFFF) == (_np(ref.hash, np.uint32)[:n][ro] & 0x3FFFFFFF)
        assert same_cell.mean() > 0.999        # a particle within rounding of a cell face may sit on either side of it
        assert np.abs(got[same_cell, :3] - want[same_cell, :3]).max() <= 12e-6 * cs
        got = np.concatenate([p["vel"] for p in parts])[order]; want = _np(ref.vel)[:n][ro]
        assert np.abs(got[:, :3] - want[:, :3]).max() <= 1e-4 * max(np.abs(want[:, :3]).max(), 1e-3)
        assert np.abs(got[:, 3] - want[:, 3]).max() <= 3e-6
        assert all(abs(float(p["dt"]) - ref.current_dt()) <= 1e-4 * ref.current_dt() for p in parts)
        return
    for k, t in (("pos", ref.pos), ("vel", ref.vel)):
        got = np.concatenate([p[k] for p in parts])[order]
        assert np.array_equal(got.view(np.uint32), _np(t)[:n][ro].view(np.uint32)), k
    assert all(float(p["dt"]) == ref.current_dt() for p in parts)
    if getattr(ref, "keps", False):
        for k in ("tke", "eps", "turbvisc", "eulervel"):
            got = np.concatenate([p[k] for p in parts])[order]
            assert np.array_equal(got.view(np.uint32), _np(ref.ke[k])[:n][ro].view(np.uint32)), k


# ---------------------------------------------------------------------------------------------
# The host side of the boundary: oracle/_ref/host/example_engines is built INSIDE the GPUSPH tree (hip_engines.h derives
# from the reference's own abstract engines, cudasimframework.cu answers the problems' SETUP_FRAMEWORK, buffers are the
# tree's BufferList with the HIPBuffer policy) and sends one worker's command stream through those interfaces, with the
# reference's blocking dtreduce.  It must leave bit-identical particles to the Python driver (same C-ABI calls,
# device-resident dt).  build() makes the binary where the tree is present; it travels with oracle/_ref.
def _cpp_case(name):
    from gpusph_amd.problem import StillWater, WaveTank
    if name == "dambreak":      # DamBreak3D.cu framework; obstacle with force feedback, Shepard filter, surface detection
        prob = DamBreak3D(deltap=0.04, obstacle=True, jitter=0.05, hydrostatic=False)
        return prob, "DamBreak3D", dict(rhodiff=D.COLAGROSSI, use_planes=0), [(D.SHEPARD_FILTER, 5)], 12
    if name == "wavetank":      # WaveTank.cu: SPSVISC + planes + LJ box + moving paddle + Shepard
        prob = WaveTank(0.06, paddle_tstart=0.0)
        return prob, "WaveTank", {}, [(D.SHEPARD_FILTER, 4)], 13
    if name == "dem":           # DEMExample.cu: LJ_BOUNDARY + terrain height map through setDEM + side planes
        from test_dem_oracle import dem_problem
        prob = dem_problem(0.04)
        prob.simparams.simflags &= ~D.ENABLE_REPACKING
        return prob, "DEMExample", dict(rhodiff=D.COLAGROSSI), [], 24
    if name == "stillwater":    # StillWater.cu: DYNAMICVISC + Ferrari + MLS, rebuild every 20
        prob = StillWater(8, jitter=0.05)
        return prob, "StillWater", dict(rhodiff=D.FERRARI, use_planes=0), [(D.MLS_FILTER, 3)], 22
    raise KeyError(name)


@pytest.mark.parametrize("name", ["dambreak", "wavetank", "stillwater", "dem"])
def test_cpp_adapters_match_python_engine(tmp_path, name):
    import os, subprocess
    import host_case as hc
    exe = hc.exe("example_engines")
    assert os.path.exists(exe), "oracle/_ref/host/example_engines is not built (make -C oracle host, needs the GPUSPH tree)"
    prob, framework, selectors, filters, steps = _cpp_case(name)
    eng = _engine(prob)
    for ft, fq in filters:
        eng.add_filter(ft, fq)
    arrs = prob.copy_to_array()
    case, state, fout = tmp_path / "case.txt", tmp_path / "state.bin", tmp_path / "out.bin"
    lines = hc.case_lines(prob, framework, **selectors) + hc.driver_lines(prob, eng, steps, filters=filters, final_surface=True)
    case.write_text("\n".join(lines) + "\n")
    hc.write_state(state, arrs)
    r = subprocess.run([exe, str(case), str(state), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    eng.run(steps)
    eng.postprocess(D.SURFACE_DETECTION)       # the driver runs the SURFACE_DETECTION engine before its dump
    ref = eng.download()
    if name == "dambreak":
        assert ((ref["info"].reshape(-1, 4)[:, 0] & D.FG_SURFACE) != 0).sum() > 20
    out = hc.read_out(fout)
    n2 = out["n"]
    assert n2 == eng.n
    assert np.float32(eng.current_dt()) == out["dt"] and eng.time() == out["t"]
    assert np.array_equal(out["info"], ref["info"].reshape(n2, 4)) and np.array_equal(out["hash"], ref["hash"])
    assert np.array_equal(out["pos"].view(np.uint32), ref["pos"].view(np.uint32))
    assert np.array_equal(out["vel"].view(np.uint32), ref["vel"].view(np.uint32))
    if name == "wavetank":      # the paddle really moved
        moved = np.abs(out["vel"][(out["info"][:, 0] & 7) == D.PT_BOUNDARY, :3]).max()
        assert moved > 1e-3


# ---------------------------------------------------------------------------------------------
# SPS turbulence: sphx_calc_visc (SPSstressMatrix, src/cuda/visc_kernel.cu:759-811) and the SPS term of the
# forces kernel (generic gather path) against the oracle.  fp32 tolerance 2e-5 of the largest entry.
@pytest.mark.parametrize("visc", [None, "SPSVISC"])
def test_sps_stress_and_forces_tolerance(visc):
    """SPS stress tensor + its divergence in the forces; "SPSVISC" = the framework's legacy selector (KINEMATICVISC + SPS:
    Newtonian laminar term with harmonic density averaging on top), None = the SPS term alone"""
    import torch
    from gpusph_amd import capi
    prob = DamBreak3D(deltap=0.04, obstacle=False, jitter=0.1, hydrostatic=False, viscosity=visc, kinematic_visc=0.02)
    prob.simparams.turbmodel = D.SPS
    dp = prob.m_deltap
    prob.physparams.smagfactor = float(np.float32((0.12 * dp) ** 2))              # src/GPUSPH.cc Smagorinsky set-up
    prob.physparams.kspsfactor = float(np.float32((2.0 / 3.0) * 0.0066 * dp * dp))
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs(); eng.build_neibs()
    n = eng.n
    rng = np.random.default_rng(11)
    vel = sim.vel.copy()
    fluid = (sim.info[:, 0] & 7) == 0
    vel[fluid, :3] += rng.uniform(-0.5, 0.5, size=(fluid.sum(), 3)).astype(np.float32)
    vel[:, 3] += rng.uniform(0, 2e-3, size=len(vel)).astype(np.float32)
    sim.vel = vel
    eng.vel[:n] = torch.from_numpy(vel[:n]).to(eng.device)
    tau_ref, tv_ref = sim.o.sps(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, n)
    A = eng.alloc
    tau = [torch.zeros((A, 2), dtype=torch.float32, device=eng.device) for _ in range(3)]
    tv = torch.zeros(A, dtype=torch.float32, device=eng.device)
    p = capi.ptr
    capi.check(eng.lib.sphx_calc_visc(eng.ctx.handle, p(tau[0]), p(tau[1]), p(tau[2]), p(tv), p(eng.pos), p(eng.vel),
                                      p(eng.info), p(eng.hash), p(eng.cellStart), p(eng.neibslist), n, n,
                                      eng.params.deltap, eng.params.slength, eng.params.influenceradius, eng._stream()))
    tau_gpu = np.concatenate([_np(t)[:n] for t in tau], axis=1)
    scale = np.abs(tau_ref[:n]).max()
    assert scale > 0
    assert np.abs(tau_gpu - tau_ref[:n]).max() <= 2e-5 * scale
    assert np.abs(_np(tv)[:n] - tv_ref[:n]).max() <= 2e-5 * np.abs(tv_ref[:n]).max()
    # forces with the SPS divergence term, fed with the ORACLE's tau on both sides
    f_ref, cfl_ref, nb, _, _ = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, tau=tau_ref)
    for k in range(3):
        tau[k][:n] = torch.from_numpy(np.ascontiguousarray(tau_ref[:n, 2 * k:2 * k + 2])).to(eng.device)
    nbl = C.c_uint32(0)
    eng._memset(eng.cfl, 0, eng._stream())
    capi.check(eng.lib.sphx_forces_basicstep(eng.ctx.handle, p(eng.forces), p(eng.cfl), None, None, p(eng.pos), p(eng.vel),
                                             p(eng.info), p(eng.hash), p(eng.cellStart), p(eng.neibslist),
                                             p(tau[0]), p(tau[1]), p(tau[2]), None, n, 0, n, eng.params.deltap,
                                             eng.params.slength, eng.params.dtadaptfactor, eng.params.influenceradius,
                                             0, D.SIMULATE, 1, eng.dt, 0, C.byref(nbl), eng._stream()))
    f = _np(eng.forces)[:n]
    fs = np.abs(f_ref[:, :3]).max()
    assert np.abs(f[:, :3] - f_ref[:n, :3]).max() <= 2e-5 * fs
    assert np.abs(f[:, 3] - f_ref[:n, 3]).max() <= 2e-5 * np.abs(f_ref[:, 3]).max() + 1e-7
    # without tau the call must be refused, not silently computed without the term
    with pytest.raises((capi.SphxError, capi.SphxInvalidArgument)):
        capi.check(eng.lib.sphx_forces_basicstep(eng.ctx.handle, p(eng.forces), p(eng.cfl), None, None, p(eng.pos),
                                                 p(eng.vel), p(eng.info), p(eng.hash), p(eng.cellStart), p(eng.neibslist),
                                                 None, None, None, None, n, 0, n, eng.params.deltap, eng.params.slength,
                                                 eng.params.dtadaptfactor, eng.params.influenceradius, 0, D.SIMULATE, 1,
                                                 eng.dt, 0, C.byref(nbl), eng._stream()))


# ---------------------------------------------------------------------------------------------
# density filters: sphx_filter_process vs the oracle.  filters.hip is compiled without FMA
# contraction, with IEEE division and sqrt and the reference's operation order: bit-exact for the polynomial kernels.
@pytest.mark.parametrize("ftype", [D.SHEPARD_FILTER, D.MLS_FILTER])
@pytest.mark.parametrize("case", [dict(deltap=0.04, obstacle=True, jitter=0.1, hydrostatic=False),
                                  dict(deltap=0.03, obstacle=False, jitter=0.05, linearization="xzy")])
def test_filters_bit_exact(ftype, case):
    import torch
    prob = DamBreak3D(**case)
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs(); eng.build_neibs()
    n = eng.n
    rng = np.random.default_rng(3)
    vel = sim.vel.copy()
    vel[:, 3] += rng.uniform(-2e-3, 2e-3, size=len(vel)).astype(np.float32)
    vel[:, :3] += rng.uniform(-0.1, 0.1, size=(len(vel), 3)).astype(np.float32)
    sim.vel = vel
    eng.vel[:n] = torch.from_numpy(vel[:n]).to(eng.device)
    ref = sim.o.filter(ftype, sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)
    eng.apply_filter(ftype)
    out = _np(eng.vel)[:n]
    assert np.array_equal(out[:, :3].view(np.uint32), ref[:n, :3].view(np.uint32))
    assert np.array_equal(out[:, 3].view(np.uint32), ref[:n, 3].view(np.uint32)), \
        "max |d rho~| = %g" % np.abs(out[:, 3] - ref[:n, 3]).max()
    # aliasing the two velocity buffers is refused
    from gpusph_amd import capi
    p = capi.ptr
    with pytest.raises((capi.SphxError, capi.SphxInvalidArgument)):
        capi.check(eng.lib.sphx_filter_process(eng.ctx.handle, int(ftype), p(eng.vel), p(eng.pos), p(eng.vel), p(eng.info),
                                               p(eng.hash), p(eng.cellStart), p(eng.neibslist), n, n,
                                               eng.params.slength, eng.params.influenceradius, eng._stream()))


def test_trajectory_with_shepard_filter():
    """WaveTank-style run: Shepard every 3 iterations (addFilter), 8 steps; same tolerances as TRAJ."""
    case = dict(deltap=0.04, obstacle=False, jitter=0.05, hydrostatic=False)
    prob = DamBreak3D(**case)
    eng = _engine(prob)
    eng.add_filter(D.SHEPARD_FILTER, 3)
    sim = ol.OracleSim(prob)
    sim.filters = [(D.SHEPARD_FILTER, 3)]
    steps = 8
    for _ in range(steps):
        sim.step(); eng.step()
    out = eng.download()
    n = eng.n
    assert n == sim.n
    assert np.array_equal(out["hash"], sim.hash[:n])
    cs = float(min(prob.m_cellsize))
    assert np.abs(out["pos"][:, :3] - sim.pos[:n, :3]).max() <= 1e-6 * cs * steps
    vmax = max(np.abs(sim.vel[:n, :3]).max(), 1e-6)
    assert np.abs(out["vel"][:, :3] - sim.vel[:n, :3]).max() <= 1e-3 * vmax
    assert np.abs(out["vel"][:, 3] - sim.vel[:n, 3]).max() <= 2e-6


# ---------------------------------------------------------------------------------------------
# LJ_BOUNDARY (Lennard-Jones repulsive boundary particles, generic forces kernel)
def test_lj_boundary_forces_and_trajectory():
    import torch
    case = dict(deltap=0.04, obstacle=False, jitter=0.2, hydrostatic=False, boundary=D.LJ_BOUNDARY)
    prob = DamBreak3D(**case)
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs(); eng.build_neibs()
    n = eng.n
    assert np.array_equal(_np(eng.neibslist, np.uint16).reshape(-1, eng.alloc)[:, :n],
                          sim.nl.reshape(-1, len(sim.pos))[:, :n])
    rng = np.random.default_rng(5)
    vel = sim.vel.copy()
    fluid = (sim.info[:, 0] & 7) == 0
    vel[fluid, :3] += rng.uniform(-0.3, 0.3, size=(fluid.sum(), 3)).astype(np.float32)
    vel[fluid, 3] += rng.uniform(0, 2e-3, size=fluid.sum()).astype(np.float32)
    sim.vel = vel
    eng.vel[:n] = torch.from_numpy(vel[:n]).to(eng.device)
    f_ref, cfl_ref, nb, _, _ = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)
    eng._forces(eng.pos, eng.vel, 1, 0)
    f = _np(eng.forces)[:n]
    scale = np.abs(f_ref[:, :3]).max()
    assert np.abs(f[:, :3] - f_ref[:n, :3]).max() <= 2e-5 * scale
    assert np.abs(f[:, 3] - f_ref[:n, 3]).max() <= 2e-5 * np.abs(f_ref[:, 3]).max() + 1e-7
    assert not np.any(f[~fluid[:n], :3])
    dt_ref = sim.o.dtreduce(cfl_ref, nb, sim.sspeed_cfl)
    assert abs(float(eng.d_dt_next.item()) - dt_ref) <= 2e-5 * dt_ref
    # a few full steps (the engine and the oracle both start again from the perturbed state)
    eng2 = _engine(prob); sim2 = ol.OracleSim(prob)
    steps = 6
    for _ in range(steps):
        sim2.step(); eng2.step()
    out = eng2.download()
    n2 = eng2.n
    assert np.array_equal(out["hash"], sim2.hash[:n2])
    cs = float(min(prob.m_cellsize))
    assert np.abs(out["pos"][:, :3] - sim2.pos[:n2, :3]).max() <= 1e-6 * cs * steps
    vmax = max(np.abs(sim2.vel[:n2, :3]).max(), 1e-6)
    assert np.abs(out["vel"][:, :3] - sim2.vel[:n2, :3]).max() <= 1e-3 * vmax
    assert np.abs(out["vel"][:, 3] - sim2.vel[:n2, 3]).max() <= 2e-6


def test_planes_forces_and_trajectory():
    """ENABLE_PLANES with LJ_BOUNDARY: plane repulsion in the finalize stage (sphx_set_planes)."""
    import torch
    prob = DamBreak3D(deltap=0.04, obstacle=False, jitter=0.3, hydrostatic=False, boundary=D.LJ_BOUNDARY, walls="planes")
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs(); eng.build_neibs()
    n = eng.n
    f_ref, cfl_ref, nb, _, _ = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)
    eng._forces(eng.pos, eng.vel, 1, 0)
    f = _np(eng.forces)[:n]
    scale = np.abs(f_ref[:, :3]).max()
    assert scale > 20.0                                          # the planes do push (|g| alone is 9.81)
    assert np.abs(f[:, :3] - f_ref[:n, :3]).max() <= 2e-5 * scale
    dt_ref = sim.o.dtreduce(cfl_ref, nb, sim.sspeed_cfl)
    assert abs(float(eng.d_dt_next.item()) - dt_ref) <= 2e-5 * dt_ref
    eng2 = _engine(prob); sim2 = ol.OracleSim(prob)
    steps = 6
    for _ in range(steps):
        sim2.step(); eng2.step()
    out = eng2.download()
    n2 = eng2.n
    assert np.array_equal(out["hash"], sim2.hash[:n2])
    cs = float(min(prob.m_cellsize))
    assert np.abs(out["pos"][:, :3] - sim2.pos[:n2, :3]).max() <= 1e-6 * cs * steps
    vmax = max(np.abs(sim2.vel[:n2, :3]).max(), 1e-6)
    assert np.abs(out["vel"][:, :3] - sim2.vel[:n2, :3]).max() <= 1e-3 * vmax


# ---------------------------------------------------------------------------------------------
# post-processing engines (vorticity, test points, free-surface detection): bit-exact vs the oracle
def test_postprocess_bit_exact():
    import torch
    pts = [(0.2, 0.3, 0.2), (0.25, 0.35, 0.1), (1.2, 0.3, 0.3)]
    prob = DamBreak3D(deltap=0.04, obstacle=True, jitter=0.1, hydrostatic=False, testpoints=pts)
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs(); eng.build_neibs()
    n = eng.n
    assert np.array_equal(_np(eng.neibslist, np.uint16).reshape(-1, eng.alloc)[:, :n],
                          sim.nl.reshape(-1, len(sim.pos))[:, :n])
    rng = np.random.default_rng(9)
    vel = sim.vel.copy()
    vel[:, :3] += rng.uniform(-0.4, 0.4, size=(len(vel), 3)).astype(np.float32)
    vel[:, 3] += rng.uniform(0, 2e-3, size=len(vel)).astype(np.float32)
    sim.vel = vel
    eng.vel[:n] = torch.from_numpy(vel[:n]).to(eng.device)
    # vorticity
    ref = sim.o.vorticity(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)
    out = _np(eng.postprocess(D.VORTICITY))
    assert np.array_equal(out.view(np.uint32), ref[:n].view(np.uint32))      # NaN rows included
    # surface detection (+ normals)
    ref_info, ref_nrm = sim.o.surface(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, normals=True)
    nrm = _np(eng.postprocess(D.SURFACE_DETECTION, normals=True))
    assert np.array_equal(_np(eng.info, np.uint16)[:n], ref_info[:n])
    assert ((ref_info[:n, 0] & D.FG_SURFACE) != 0).sum() > 100
    assert np.array_equal(nrm.view(np.uint32), ref_nrm[:n].view(np.uint32))
    # test points (last: it overwrites velocity rows)
    ref_vel = sim.o.testpoints(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)
    eng.postprocess(D.TESTPOINTS)
    got = _np(eng.vel)[:n]
    tp = (sim.info[:n, 0] & 7) == D.PT_TESTPOINT
    assert tp.sum() == 3
    assert np.array_equal(got[~tp].view(np.uint32), vel[:n][~tp].view(np.uint32))
    assert np.array_equal(got[tp, :3].view(np.uint32), ref_vel[:n][tp, :3].view(np.uint32))
    # pressure goes through powf: device libm vs glibc, 2 ulp
    assert np.abs(got[tp, 3] - ref_vel[:n][tp, 3]).max() <= 4e-7 * np.abs(ref_vel[:n][tp, 3]).max()


# ---------------------------------------------------------------------------------------------
# periodic boundaries (clampGridPos / calcGridHashPeriodic; the tiled kernel's wrapped window rows)
PERIODIC_CASES = [dict(n=(30, 24, 20), jitter=0.2, velocity=(5.0, -3.0, 2.0)),
                  dict(n=(26, 22, 18), jitter=0.15, velocity=(-4.0, 2.0, 6.0), periodic=D.PERIODIC_X | D.PERIODIC_Y,
                       linearization="xzy")]


@pytest.mark.parametrize("case", PERIODIC_CASES)
def test_periodic_neibs_forces_and_trajectory(case, monkeypatch):
    import torch
    from gpusph_amd.problem import PeriodicBox
    prob = PeriodicBox(deltap=0.05, **case)
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs(); eng.build_neibs()
    n = eng.n
    assert n == sim.n
    assert np.array_equal(_np(eng.hash, np.uint32)[:n], sim.hash[:n])
    assert np.array_equal(_np(eng.neibslist, np.uint16).reshape(-1, eng.alloc)[:, :n], sim.nl.reshape(-1, len(sim.pos))[:, :n])
    rng = np.random.default_rng(21)
    vel = sim.vel.copy()
    vel[:, :3] += rng.uniform(-0.3, 0.3, size=(len(vel), 3)).astype(np.float32)
    vel[:, 3] += rng.uniform(0, 2e-3, size=len(vel)).astype(np.float32)
    sim.vel = vel
    eng.vel[:n] = torch.from_numpy(vel[:n]).to(eng.device)
    f_ref, cfl_ref, nb, _, _ = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)
    eng._forces(eng.pos, eng.vel, 1, 0)
    f = _np(eng.forces)[:n]
    assert np.abs(f[:, :3] - f_ref[:n, :3]).max() <= 2e-5 * np.abs(f_ref[:, :3]).max()
    assert np.abs(f[:, 3] - f_ref[:n, 3]).max() <= 2e-5 * np.abs(f_ref[:, 3]).max() + 1e-7
    # tiled == generic on the same state
    monkeypatch.setenv("SPHX_DISABLE_TILES", "1")
    eng_g = _engine(prob, clobber_neibslist=True)
    eng_g.build_neibs()
    eng_g.vel[:n] = torch.from_numpy(vel[:n]).to(eng_g.device)
    eng_g._forces(eng_g.pos, eng_g.vel, 1, 0)
    from kernel_agreement import assert_forces_agree
    assert_forces_agree(f, _np(eng_g.forces)[:n])
    monkeypatch.setenv("SPHX_DISABLE_TILES", "0")
    # trajectory across two re-sorts: particles leave through one face and come back through the opposite one
    eng2 = _engine(prob); sim2 = ol.OracleSim(prob)
    steps = 22
    for _ in range(steps):
        sim2.step(); eng2.step()
    out = eng2.download()
    assert eng2.n == sim2.n == n
    assert np.array_equal(out["hash"], sim2.hash[:n]) and np.array_equal(out["info"].reshape(-1, 4), sim2.info[:n])
    cs = float(min(prob.m_cellsize))
    assert np.abs(out["pos"][:, :3] - sim2.pos[:n, :3]).max() <= 1e-6 * cs * steps
    vmax = np.abs(sim2.vel[:n, :3]).max()
    assert np.abs(out["vel"][:, :3] - sim2.vel[:n, :3]).max() <= 1e-3 * vmax
    assert np.abs(out["vel"][:, 3] - sim2.vel[:n, 3]).max() <= 2e-6


def test_against_committed_feature_fixture():
    """tests/golden/oracle_features.npz (SURVEY 8c fixtures iv, v and the widened rows): the HIP path against committed
    vectors, without the oracle in the loop -- SPS tau and forces, Shepard/MLS, vorticity, surface flags + normals, test
    points, moving-body Euler rows, LJ boundary particles with a feedback body, planes."""
    import os, torch
    from gpusph_amd import capi
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_features.npz"))
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    prob = DamBreak3D(float(g["a_deltap"]), obstacle=True, jitter=0.1, hydrostatic=False, testpoints=[(0.2, 0.3, 0.2), (0.3, 0.4, 0.1)])
    prob.simparams.turbmodel = D.SPS
    dp = prob.m_deltap
    prob.physparams.smagfactor = float(np.float32((0.12 * dp) ** 2))
    prob.physparams.kspsfactor = float(np.float32((2.0 / 3.0) * 0.0066 * dp * dp))
    eng = _engine(prob, clobber_neibslist=True)
    eng.build_neibs()
    n = eng.n
    vel = g["a_vel"]
    eng.vel[:n] = torch.from_numpy(vel[:n]).to(eng.device)
    p = capi.ptr
    A = eng.alloc
    tau = [torch.zeros((A, 2), dtype=torch.float32, device=eng.device) for _ in range(3)]
    tv = torch.zeros(A, dtype=torch.float32, device=eng.device)
    capi.check(eng.lib.sphx_calc_visc(eng.ctx.handle, p(tau[0]), p(tau[1]), p(tau[2]), p(tv), p(eng.pos), p(eng.vel), p(eng.info),
                                      p(eng.hash), p(eng.cellStart), p(eng.neibslist), n, n, eng.params.deltap, eng.params.slength,
                                      eng.params.influenceradius, eng._stream()))
    tau_gpu = np.concatenate([_np(t)[:n] for t in tau], axis=1)
    assert np.abs(tau_gpu - g["a_tau"][:n]).max() <= 2e-5 * np.abs(g["a_tau"]).max()
    # filters and post-processing: bit-exact
    for ftype, key in ((D.SHEPARD_FILTER, "a_shepard"), (D.MLS_FILTER, "a_mls")):
        eng.vel[:n] = torch.from_numpy(vel[:n]).to(eng.device)
        eng.apply_filter(ftype)
        assert np.array_equal(bits(_np(eng.vel)[:n]), bits(g[key][:n])), key
    eng.vel[:n] = torch.from_numpy(vel[:n]).to(eng.device)
    assert np.array_equal(bits(_np(eng.postprocess(D.VORTICITY))), bits(g["a_vorticity"][:n]))
    nrm = _np(eng.postprocess(D.SURFACE_DETECTION, normals=True))
    assert np.array_equal(_np(eng.info, np.uint16)[:n], g["a_surface_info"][:n]) and np.array_equal(bits(nrm), bits(g["a_normals"][:n]))
    eng.postprocess(D.TESTPOINTS)
    tp = (g["a_surface_info"][:n, 0] & 7) == D.PT_TESTPOINT
    got = _np(eng.vel)[:n]
    assert np.array_equal(bits(got[tp, :3]), bits(g["a_testpoints"][:n][tp, :3]))
    assert np.abs(got[tp, 3] - g["a_testpoints"][:n][tp, 3]).max() <= 4e-7 * np.abs(g["a_testpoints"][:n][tp, 3]).max() + 1e-12
    # moving-body Euler rows
    eng.vel[:n] = torch.from_numpy(vel[:n]).to(eng.device)
    rb = [np.ascontiguousarray(g[k], dtype=np.float32) for k in ("a_rb_trans", "a_rb_rot", "a_rb_lvel", "a_rb_avel")]   # keep alive
    capi.check(eng.lib.sphx_set_rb_motion(eng.ctx.handle, rb[0].ctypes.data, rb[1].ctypes.data, rb[2].ctypes.data, rb[3].ctypes.data, 1))
    eng.forces[:n] = torch.from_numpy(g["a_euler_forces"][:n]).to(eng.device)
    eng.d_dt.fill_(float(g["a_euler_dt"]))
    for step, scale in ((1, 0.5), (2, 1.0)):
        eng._euler(step, scale)
        assert np.array_equal(bits(_np(eng.pos2)[:n]), bits(g["a_euler%d_pos" % step][:n]))
        assert np.array_equal(bits(_np(eng.vel2)[:n]), bits(g["a_euler%d_vel" % step][:n]))
    # LJ boundary particles (+ feedback body) and planes
    for tag, kw in (("b", dict(obstacle=True, boundary=D.LJ_BOUNDARY)), ("c", dict(obstacle=False, boundary=D.LJ_BOUNDARY, walls="planes"))):
        prob = DamBreak3D(float(g["a_deltap"]), jitter=0.25, hydrostatic=False, **kw)
        eng = _engine(prob, clobber_neibslist=True)
        eng.build_neibs()
        n = eng.n
        assert np.array_equal(_np(eng.neibslist, np.uint16), g[tag + "_neibs"])
        eng.vel[:n] = torch.from_numpy(g[tag + "_vel"][:n]).to(eng.device)
        eng._forces(eng.pos, eng.vel, 1, 0)
        f, fr = _np(eng.forces)[:n], g[tag + "_forces"][:n]
        assert np.abs(f[:, :3] - fr[:, :3]).max() <= 2e-5 * np.abs(fr[:, :3]).max()
        assert abs(float(eng.d_dt_next.item()) - float(g[tag + "_dt"])) <= 2e-5 * float(g[tag + "_dt"])
        if prob.num_obstacle:
            assert np.abs(_np(eng.rbforces) - g[tag + "_rbforces"]).max() <= 2e-5 * max(np.abs(g[tag + "_rbforces"]).max(), 1e-12)


def test_against_committed_feature_fixture_2():
    """tests/golden/oracle_features2.npz: repacking run mode (bit-exact) and Newtonian viscosity cases against committed
    vectors, without the oracle in the loop"""
    import importlib.util, os, torch
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(here, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec); spec.loader.exec_module(mg)
    g = np.load(os.path.join(here, "oracle_features2.npz"))
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for tag, kind, make in mg.features2_cases():
        prob = make()
        eng = _engine(prob, clobber_neibslist=True)
        eng.build_neibs()
        n = eng.n
        vel = np.ascontiguousarray(g[tag + "_vel"])
        eng.vel[:n] = torch.from_numpy(vel[:n]).to(eng.device)
        fr = g[tag + "_forces"][:n]
        if kind == "repack":
            eng._forces(eng.pos, eng.vel, 1, 0, D.REPACK)
            assert np.array_equal(bits(_np(eng.forces)[:n]), bits(fr)), tag
            eng.d_dt.fill_(float(np.float32(1.3e-4)))
            eng._euler(1, 1.0, D.REPACK)
            assert np.array_equal(bits(_np(eng.pos2)[:n]), bits(g[tag + "_euler_pos"][:n]))
            assert np.array_equal(bits(_np(eng.vel2)[:n]), bits(g[tag + "_euler_vel"][:n]))
            tol = 1e-6
        else:
            eng._forces(eng.pos, eng.vel, 1, 0)
            f = _np(eng.forces)[:n]
            assert np.abs(f[:, :3] - fr[:, :3]).max() <= 2e-5 * np.abs(fr[:, :3]).max(), tag
            assert np.abs(f[:, 3] - fr[:, 3]).max() <= 1e-3 * np.abs(fr[:, 3]).max() + 1e-7, tag   # Colagrossi switch pairs (two fluids)
            tol = 2e-5
        assert abs(float(eng.d_dt_next.item()) - float(g[tag + "_dt"])) <= tol * float(g[tag + "_dt"]), tag


# ---------------------------------------------------------------------------------------------
# repacking run mode (run_mode = REPACK through the same basicstep entry points): no fast-math in this kernel, so
# the forces are BIT-EXACT against the oracle for the polynomial kernels; the CFL term holds a powf (sound speed)
# and is compared to 1e-6
def _repack_cases():
    from gpusph_amd.problem import PeriodicBox
    return [
        ("dambreak", lambda: DamBreak3D(deltap=0.04, obstacle=True, jitter=0.2, hydrostatic=True)),
        ("dambreak-cubic", lambda: DamBreak3D(deltap=0.05, obstacle=False, jitter=0.2, kerneltype=D.CUBICSPLINE)),
        ("dambreak-quadratic", lambda: DamBreak3D(deltap=0.05, obstacle=False, jitter=0.2, kerneltype=D.QUADRATIC)),
        ("periodic", lambda: PeriodicBox(deltap=0.05, n=(20, 16, 12), jitter=0.25, repacking=True)),
        ("lj-planes", lambda: DamBreak3D(deltap=0.04, obstacle=False, jitter=0.3, hydrostatic=False,
                                         boundary=D.LJ_BOUNDARY, walls="planes")),
    ]


@pytest.mark.parametrize("name", [c[0] for c in _repack_cases()])
def test_repack_forces_bit_exact(name):
    import torch
    prob = dict(_repack_cases())[name]()
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs(); eng.build_neibs()
    n = eng.n
    rng = np.random.default_rng(9)
    v = sim.vel.copy()
    v[:n, :3] = rng.uniform(-0.2, 0.2, size=(n, 3)).astype(np.float32)
    sim.vel = v
    eng.vel[: len(v)] = torch.from_numpy(v).to(eng.device)
    rb = getattr(prob, "num_obstacle", 0)
    f_ref, cfl_ref, nb, rbf_ref, rbt_ref = sim.o.repack_forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, rb_count=rb)
    eng.rbforces.fill_(1.0); eng.rbtorques.fill_(1.0)
    eng.forces.zero_()
    eng._forces(eng.pos, eng.vel, 1, 0, D.REPACK)
    f = _np(eng.forces)[:n]
    assert np.abs(f_ref[:n, :3]).max() > 1.0
    if name == "lj-planes":     # powf in the plane repulsion
        scale = np.abs(f_ref[:n, :3]).max()
        assert np.abs(f - f_ref[:n]).max() <= 2e-6 * scale
    else:
        assert np.array_equal(f.view(np.uint32), f_ref[:n].view(np.uint32))
    cfl = _np(eng.cfl)[:nb]
    np.testing.assert_allclose(cfl, cfl_ref[:nb], rtol=1e-6)
    dt_ref = sim.o.dtreduce(cfl_ref, nb, sim.sspeed_cfl)
    assert abs(float(eng.d_dt_next.item()) - dt_ref) <= 1e-6 * dt_ref
    if rb:
        assert not np.any(_np(eng.rbforces)[:rb]) and not np.any(_np(eng.rbtorques)[:rb])   # zeroed, like the oracle
        assert not np.any(rbf_ref[:rb]) and not np.any(rbt_ref[:rb])


def test_repack_euler_bit_exact_and_lid_removal():
    import torch
    from gpusph_amd import capi
    prob = DamBreak3D(deltap=0.04, obstacle=True, jitter=0.1, hydrostatic=True)
    eng = _engine(prob)
    sim = ol.OracleSim(prob)
    sim.build_neibs(); eng.build_neibs()
    n = eng.n
    rng = np.random.default_rng(10)
    f = rng.uniform(-50, 50, size=(len(sim.pos), 4)).astype(np.float32)
    v = sim.vel.copy()
    v[:n, :3] = rng.uniform(-0.5, 0.5, size=(n, 3)).astype(np.float32)
    sim.vel = v
    eng.vel[: len(v)] = torch.from_numpy(v).to(eng.device)
    eng.forces[: len(f)] = torch.from_numpy(f).to(eng.device)
    for step in (1, 2):
        dt = float(np.float32(eng.dt))
        p_ref, v_ref = sim.o.euler_repack(sim.pos, sim.vel, sim.info, sim.hash, f, n, dt, step)
        eng._euler(step, 1.0, D.REPACK)
        assert np.array_equal(_np(eng.pos2)[:n].view(np.uint32), p_ref[:n].view(np.uint32))
        assert np.array_equal(_np(eng.vel2)[:n].view(np.uint32), v_ref[:n].view(np.uint32))
    # the lid
    info = sim.info.copy()
    ptype = info[:n, 0] & 7
    info[np.where(ptype == 1)[0][:33], 0] |= D.FG_SURFACE
    info[np.where(ptype == 0)[0][:20], 0] |= D.FG_SURFACE
    pos_ref = sim.pos.copy()
    sim.o.disable_free_surf_parts(pos_ref, info, n)
    d_info = torch.from_numpy(info.view(np.int16)).to(eng.device)
    capi.check(eng.lib.sphx_disable_free_surf_parts(eng.ctx.handle, capi.ptr(eng.pos), capi.ptr(d_info), n, n, None))
    got = _np(eng.pos)[:n]
    assert np.array_equal(np.isnan(got[:, 3]), np.isnan(pos_ref[:n, 3])) and np.isnan(got[:, 3]).sum() == 33
    assert np.array_equal(got[:, :3].view(np.uint32), pos_ref[:n, :3].view(np.uint32))


@pytest.mark.parametrize("name", ["dambreak", "periodic"])
def test_repack_run_matches_oracle(name):
    """`--repack`: repack_maxiter iterations spanning a re-sort, lid removal, rebuild, state reset; then the simulation
    proper starts from the repacked particles."""
    prob = dict(_repack_cases())[name]()
    prob.simparams.repack_maxiter = 14
    eng = _engine(prob); sim = ol.OracleSim(prob)
    eng.repack(reset=False); sim.repack(reset=False)
    n = eng.n
    assert n == sim.n and eng.iterations == sim.iterations == 14
    out = eng.download()
    assert np.array_equal(out["hash"], sim.hash[:n])
    assert np.array_equal(out["info"], sim.info[:n])
    cs = float(min(prob.m_cellsize))
    assert np.abs(out["pos"][:, :3] - sim.pos[:n, :3]).max() <= 1e-6 * cs
    vmax = np.abs(sim.vel[:n, :3]).max()
    assert vmax > 0.05
    assert np.abs(out["vel"][:, :3] - sim.vel[:n, :3]).max() <= 1e-5 * vmax
    assert np.array_equal(out["vel"][:, 3], sim.vel[:n, 3])                     # density untouched
    assert abs(eng.time() - sim.t) <= 1e-6 * sim.t
    eng.repack(maxiter=0); sim.repack(maxiter=0)                                 # reset only
    assert eng.iterations == 0 and eng.time() == 0.0
    out = eng.download()
    assert not np.any(out["vel"][:, :3])
    np.testing.assert_allclose(out["vel"][:, 3], sim.vel[:n, 3], rtol=0, atol=2e-7)   # hydrostatic rho~ at the new positions
    for _ in range(3):
        eng.step(); sim.step()
    out = eng.download()
    assert np.abs(out["pos"][:, :3] - sim.pos[:n, :3]).max() <= 3e-6 * cs
    vmax = max(np.abs(sim.vel[:n, :3]).max(), 1e-6)
    assert np.abs(out["vel"][:, :3] - sim.vel[:n, :3]).max() <= 1e-3 * vmax


def test_repack_needs_the_framework_flag():
    from gpusph_amd import capi
    from gpusph_amd.problem import PeriodicBox
    prob = PeriodicBox(deltap=0.05, n=(12, 10, 9), jitter=0.1)       # ENABLE_REPACKING not set
    eng = _engine(prob)
    eng.build_neibs()
    with pytest.raises(capi.SphxInvalidArgument, match="ENABLE_REPACKING"):
        eng._forces(eng.pos, eng.vel, 1, 0, D.REPACK)
    with pytest.raises(ValueError, match="not enabled"):
        eng.repack()


def _fidelity_case(name):
    from gpusph_amd.problem import Poiseuille
    dp = DamBreak3D.deltap_for(1.0e6, obstacle=False)
    newt = dict(rheologytype=D.NEWTONIAN, turbmodel=D.LAMINAR_FLOW, compvisc=D.DYNAMIC, avgop=D.HARMONIC)
    if name == "grenier_1M":
        return DamBreak3D(dp, obstacle=False, two_fluids=True, formulation=D.SPH_GRENIER, viscosity="DYNAMICVISC",
                          density_diffusion=D.DENSITY_DIFFUSION_NONE)
    if name == "sph_ha_1M":
        return DamBreak3D(dp, obstacle=False, two_fluids=True, formulation=D.SPH_HA, viscosity=newt, density_diffusion=D.COLAGROSSI)
    if name == "internal_energy_1M":
        return DamBreak3D(dp, obstacle=False, internal_energy=True)
    if name == "papanastasiou_1M":
        return Poiseuille(100, rheology=D.PAPANASTASIOU)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["grenier_1M", "sph_ha_1M", "internal_energy_1M", "papanastasiou_1M"])
def test_fidelity_option_sets_at_one_million_particles(name):
    """the option sets of the fidelity engines at a million particles against the OpenMP oracle: three steps of the whole
    sequence (COMPUTE_DENSITY / CALC_VISC, forces, dt, Euler incl. volumes / energies) from a perturbed state"""
    import os
    import torch
    ol.lib().orc_set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
    prob = _fidelity_case(name)
    assert prob.num_particles > 0.9e6
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs(); eng.build_neibs()
    n = eng.n
    assert n == sim.n and np.array_equal(_np(eng.neibslist, np.uint16).reshape(-1, eng.alloc)[:, :n], sim.nl.reshape(-1, len(sim.pos))[:, :n])
    rng = np.random.default_rng(13)
    fluid = (sim.info[:n, 0] & 7) == 0
    sim.vel[:n, :3][fluid] += rng.uniform(-0.1, 0.1, size=(int(fluid.sum()), 3)).astype(np.float32)
    eng.vel[:n] = torch.from_numpy(sim.vel[:n]).to(eng.device)
    for _ in range(3):
        sim.step(); eng.step()
    out = eng.download()
    assert abs(eng.current_dt() - sim.dt) <= 1e-4 * sim.dt
    assert np.array_equal(out["info"], sim.info[:n])
    assert np.abs(out["pos"][:, :3] - sim.pos[:n, :3]).max() <= 3e-6 * prob.m_cellsize.min()
    vscale = max(np.abs(sim.vel[:n, :3]).max(), 1e-3)
    assert np.abs(out["vel"][:, :3] - sim.vel[:n, :3]).max() <= 1e-4 * vscale
    if name == "grenier_1M":
        np.testing.assert_allclose(out["vol"][:, 3], sim.vol[:n, 3], rtol=1e-5)
    if name == "internal_energy_1M":
        es = np.abs(sim.energy[:n]).max()
        assert es > 0 and np.abs(out["energy"] - sim.energy[:n]).max() <= 1e-3 * es
