"""One forces pass of a problem on the device against the oracle, and tiled against generic: the check that tests/test_gpu_options.py,
tests/test_gpu_tiling_overflow.py, tests/test_gpu_kernel_axis.py and tests/test_gpu_grid_edge_cases.py share, and the 4 x rule of the
last two.  TEST INFRASTRUCTURE; the callers carry the gpu mark."""
import numpy as np

import oracle_lib as ol
from gpusph_amd import defs as D


def _engine(problem, **kw):
    from gpusph_amd.engine import TimestepEngine
    return TimestepEngine(problem, device="cuda:0", **kw)


def _np(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def _perturb(sim, eng, seed):
    """eng = None: the oracle driver's side alone (CPU tests)"""
    rng = np.random.default_rng(seed)
    vel = sim.vel.copy()
    fluid = (sim.info[:, 0] & 7) == 0
    vel[fluid, :3] += rng.uniform(-0.3, 0.3, size=(fluid.sum(), 3)).astype(np.float32)
    vel[:, 3] += rng.uniform(0, 2e-3, size=len(vel)).astype(np.float32)
    sim.vel = vel
    if eng is not None:
        import torch
        eng.vel[:eng.n] = torch.from_numpy(vel[:eng.n]).to(eng.device)
    return vel


def _within_4x(what, gpu, orc, f64, weight=None):
    """the 4 x rule of tests/test_gpu_kernel_axis.py's docstring; returns (oracle's deviation, device's deviation) from the float64 value"""
    ok = np.isfinite(f64)
    w = 1.0 if weight is None else weight[ok]
    e_orc = float((np.abs(np.asarray(orc, dtype=np.float64)[ok] - f64[ok])*w).max())
    e_gpu = float((np.abs(np.asarray(gpu, dtype=np.float64)[ok] - f64[ok])*w).max())
    print("%s: |oracle - float64| = %.3g, |device - float64| = %.3g" % (what, e_orc, e_gpu))
    assert e_orc > 0 and np.isfinite(np.asarray(gpu)[ok]).all()
    assert e_gpu <= 4.0*e_orc, "%s: the device is %.3g from the float64 value, the oracle %.3g" % (what, e_gpu, e_orc)
    return e_orc, e_gpu


def tiles_usable(eng):
    """1: the last build of this context left a tiling the tiled kernels run on; 0: none, or one that overflowed.  Synchronises"""
    return int(eng.k.lib.sphx_dbg_tiles_usable(eng.k.ctx.handle))


def _check_neibs_and_forces(prob, seed, monkeypatch=None, tol=2e-5, switch_flips=0, kernels_ulp=0, usable=None):
    """usable: what sphx_dbg_tiles_usable has to say of the first engine's build -- 1: its pass below is the tiled kernels', 0: its
    tiling overflowed and the pass is the generic kernels' (the comparison with the generic context then compares the stand-by
    with the plain launch of the same kernel); None: not asked.  -> (the first engine, the oracle driver), both in the perturbed state"""
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs(); eng.build_neibs()
    n = eng.n
    assert n == sim.n
    if usable is not None:
        assert sim.neibs_info.hasTooManyNeibs == -1      # a pass over a list that did not fit is outside the contract
        eng.neibs_info()
        assert tiles_usable(eng) == usable
    assert np.array_equal(_np(eng.hash, np.uint32)[:n], sim.hash[:n])
    assert np.array_equal(_np(eng.info, np.uint16)[:n], sim.info[:n])
    assert np.array_equal(_np(eng.pos)[:n].view(np.uint32), sim.pos[:n].view(np.uint32))
    assert np.array_equal(_np(eng.neibslist, np.uint16).reshape(-1, eng.alloc)[:, :n], sim.nl.reshape(-1, len(sim.pos))[:, :n])
    vel = _perturb(sim, eng, seed)
    cof = 1 if prob.simparams.numforcesbodies else 0
    # turbulence<SPS>: the engine's pass runs CALC_VISC first; so does the oracle's driver (OracleSim.step)
    tau = sim.o.sps(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, n)[0] if prob.simparams.turbmodel == D.SPS else None
    f_ref, cfl_ref, nb, rbf_ref, _ = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n,
                                                compute_object_forces=cof, rb_count=prob.num_obstacle, tau=tau)
    eng._forces(eng.pos, eng.vel, 1, 0)
    f = _np(eng.forces)[:n]
    assert np.abs(f[:, :3] - f_ref[:n, :3]).max() <= tol * np.abs(f_ref[:, :3]).max()
    werr = np.abs(f[:, 3] - f_ref[:n, 3])
    wtol = tol * np.abs(f_ref[:, 3]).max() + 1e-7
    # the Colagrossi switch |P_i - P_j| >= |rho g.r| flips on the last bit of P for a pair sitting on it:
    # where a case is known to have such pairs a handful of particles may differ by ONE pair's diffusion term
    assert (werr > wtol).sum() <= switch_flips and werr.max() <= (1e-3 if switch_flips else tol) * np.abs(f_ref[:, 3]).max() + 1e-7
    dt_ref = sim.o.dtreduce(cfl_ref, nb, sim.sspeed_cfl, sim.max_kinvisc)
    assert abs(float(eng.d_dt_next.item()) - dt_ref) <= tol * dt_ref
    if monkeypatch is not None:      # same state through the other forces kernel
        import torch
        monkeypatch.setenv("SPHX_DISABLE_TILES", "1")
        eng_g = _engine(prob, clobber_neibslist=True)
        eng_g.build_neibs()
        eng_g.vel[:n] = torch.from_numpy(vel[:n]).to(eng_g.device)
        eng_g._forces(eng_g.pos, eng_g.vel, 1, 0)
        monkeypatch.setenv("SPHX_DISABLE_TILES", "0")
        fg = _np(eng_g.forces)[:n]
        from kernel_agreement import assert_forces_agree
        assert_forces_agree(f, fg)
    return eng, sim
