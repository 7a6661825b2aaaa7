"""Float64 ALL-PAIRS known answers for the headline option set (DamBreak3D as bench.py runs it: SPH_F1, Wendland, artificial
viscosity, Colagrossi density diffusion, DYN_BOUNDARY) and for the SPS stress tensor.

Whole-function parity of the pair loop is unpinned by reference outputs, so the restatement in
oracle/sph_oracle.c is held here by an evaluation that shares nothing with it: global float64 positions, neighbours by
distance (k-d tree -- no cells, no hash, no neighbour list, no list order), the formulas of the reference written from its
source text:
  continuity            m_j (v_ij . r_ij) F_ij                                        forces_kernel.def:2140-2151
  Colagrossi            - D c0 (rho_j/rho_i - 1) F_ij m_j, fluid neighbours of the same fluid, only where
                        |P_i - P_j| >= |g . r_ij| rho_i                               forces_kernel.def:1916-1952
  pressure              -(P_i/rho_i^2 + P_j/rho_j^2) m_j F_ij r_ij                     forces_kernel.def:2451-2466
  artificial viscosity  approaching pairs: (v.r) h alpha (c_i + c_j)/((r^2 + eps)(rho_i + rho_j)) m_j F_ij r_ij
                                                                                      visc_kernel.cu:74-85, forces_kernel.def:2748-2764
  who interacts         fluid <- fluid, fluid <- DYN boundary (no diffusion), DYN boundary <- fluid (continuity + diffusion;
                        momentum only with force feedback)                            forces_kernel.def:3565-3679
  finalize              drho~/dt = DrDt / rho0, gravity on fluid particles            forces_kernel.def:3212-3218,4032-4150
  SPS                   dv_a = -sum_j (v_i - v_j)_a r_ij F_ij m_j/rho_j over ALL neighbours, tau from it
                                                                                      visc_kernel.cu:307-407,759-811
The Colagrossi switch is decided by the last bits of P for pairs on its threshold; such pairs are identified (float64 margin
within a few float32 ulp of the pressures) and their term is allowed either way -- they are counted and must stay rare."""
import numpy as np
import pytest

import allpairs_ref as ap
import oracle_lib as ol
from gpusph_amd import defs as D
from gpusph_amd.problem import DamBreak3D


def _state(viscosity=None, seed=5):
    prob = DamBreak3D(0.025, obstacle=True, jitter=0.15, hydrostatic=True, viscosity=viscosity, kinematic_visc=1.0e-6)
    sim = ol.OracleSim(prob)
    sim.build_neibs()
    n = sim.n
    rng = np.random.default_rng(seed)
    # a sheared, converging velocity field plus noise (approaching and separating pairs), densities off the hydrostatic
    # profile by up to 0.4 % (so that most pairs are far from the diffusion threshold)
    gp = prob.global_pos(sim.pos[:n], sim.hash[:n])
    v = np.stack([0.8*np.sin(3.0*gp[:, 2]) - 0.5*gp[:, 0], 0.6*np.cos(2.0*gp[:, 0]) - 0.4*gp[:, 1],
                  0.3*gp[:, 0]*gp[:, 1] - 0.5*gp[:, 2]], axis=1) + rng.normal(0, 0.15, size=(n, 3))
    sim.vel[:n, :3] = v.astype(np.float32)
    sim.vel[:n, 3] += rng.uniform(-4e-3, 4e-3, size=n).astype(np.float32)
    return prob, sim, gp


_consts = ap.consts


def _wendland_F(k):
    """the headline kernel, as these two tests have always written it: F = (q - 2)^3 * 105 / (128 pi h^5)"""
    return lambda r: (r/k["h"] - 2.0)**3*k["fcoeff"]


def test_headline_option_set_equals_a_float64_all_pairs_evaluation():
    prob, sim, gp = _state()
    n = sim.n
    p = sim.o.p
    assert p.kerneltype == D.WENDLAND and p.densitydiffusiontype == D.COLAGROSSI and p.boundarytype == D.DYN_BOUNDARY
    assert p.turbmodel == D.ARTIFICIAL and p.sph_formulation == D.SPH_F1
    k = _consts(sim)
    assert k["gam"] == 7.0 and k["cpow"] == 3.0 and k["alpha"] > 0 and k["Dc"] > 0
    f = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[0][:n].astype(np.float64)

    ptype = sim.info[:n, 0] & 7
    fluid, bound = ptype == D.PT_FLUID, ptype == D.PT_BOUNDARY
    assert fluid.sum() > 3000 and bound.sum() > 3000, (fluid.sum(), bound.sum())
    # the float64 all-pairs sums (tests/allpairs_ref.py; the kernel function is its parameter)
    ref = ap.momentum_continuity(sim, gp, k, _wendland_F(k))
    acc, drt, amb, pairs, ambiguous = ref["acc"], ref["drt"], ref["amb"], ref["pairs"], ref["ambiguous"]

    # momentum equation: every fluid particle; walls without force feedback carry no acceleration
    ascale = np.abs(acc[fluid]).max()
    assert ascale > 50.0
    assert np.abs(f[fluid, :3] - acc[fluid]).max() <= 2e-5*ascale
    nofb = bound & ((sim.info[:n, 0] & D.FG_COMPUTE_FORCE) == 0)
    assert nofb.sum() > 0 and not f[nofb, :3].any()
    # continuity equation: fluid and wall particles; threshold pairs widen the bound of their two particles only
    dscale = np.abs(drt).max()
    assert dscale > 1.0
    err = np.abs(f[:, 3] - drt)
    assert (err <= 2e-5*dscale + amb*(1 + 1e-6)).all(), "drho/dt differs: %g of %g" % ((err - amb).max(), dscale)
    assert ambiguous <= 0.01*pairs, "too many pairs on the diffusion threshold to test anything: %d of %d" % (ambiguous, pairs)
    tight = amb == 0.0
    assert tight.mean() > 0.9 and np.abs(f[tight, 3] - drt[tight]).max() <= 2e-5*dscale
    # both branches of the switch and of the viscosity were exercised, on walls too
    assert np.abs(drt[bound]).max() > 0.05*dscale


def test_sps_stress_tensor_equals_a_float64_all_pairs_evaluation():
    prob, sim, gp = _state(viscosity="SPSVISC", seed=9)
    n = sim.n
    p = sim.o.p
    assert p.turbmodel == D.SPS
    k = _consts(sim)
    smag, ksps = float(p.smagfactor), float(p.kspsfactor)
    dp = float(prob.m_deltap)
    assert smag == pytest.approx((0.12*dp)**2, rel=1e-6) and ksps == pytest.approx((2*0.0066/3)*dp*dp, rel=1e-6)   # GPUSPH.cc:1542-1554
    tau, tv = sim.o.sps(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, n)
    ref, nu = ap.tau_all_pairs(sim, gp, k, smag, ksps, _wendland_F(k))
    scale = np.abs(ref).max(axis=0)
    assert (scale > 0).all() and np.abs(nu).max() > 0
    assert (np.abs(tau[:n] - ref) <= 2e-5*scale.max()).all(), np.abs(tau[:n] - ref).max(axis=0)/scale.max()
    assert np.abs(tv[:n] - nu).max() <= 2e-5*np.abs(nu).max()
    # walls get a stress from their fluid neighbours too (their rows are read by the fluid's forces pass)
    bound = (sim.info[:n, 0] & 7) == D.PT_BOUNDARY
    assert np.abs(ref[bound]).max() > 0.01*scale.max()

    # the consumer: forces with tau minus forces with tau = 0 is sum_j m_j F_ij (tau_i + tau_j) . r_ij for the pairs that carry
    # the momentum equation (forces_kernel.def:2777-2798)
    # (the stress of this coarse, gently sheared state is 1e-4 of the pressure term: scaled up so that the term stands above the
    # float32 rounding of the accelerations it is the difference of)
    tau = (tau*np.float32(1000.0)).astype(np.float32)
    f_tau = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, tau=tau)[0][:n].astype(np.float64)
    f_0 = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, tau=np.zeros_like(tau))[0][:n].astype(np.float64)
    term = f_tau[:, :3] - f_0[:, :3]
    assert np.array_equal(f_tau[:, 3], f_0[:, 3])
    fluid = (sim.info[:n, 0] & 7) == D.PT_FLUID
    want = ap.sps_divergence(sim, gp, k, tau, _wendland_F(k))
    ts = np.abs(want).max()
    fs = np.abs(f_0[fluid, :3]).max()
    assert ts > 0.1*fs
    # a difference of two float32 accelerations: their rounding adds to the bound of the term
    assert np.abs(term[fluid] - want[fluid]).max() <= 2e-5*ts + 1e-6*fs
