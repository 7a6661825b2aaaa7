"""The float64 restatement of the SPH_HA terms with SA walls (tests/sa_ha_ref.py), pinned without any kernel.

In exact arithmetic, for a SINGLE fluid whose fluid particles all have the mass rho0 deltap^3 (SABox's), the Hu & Adams forms reduce
to the SPH_F1 ones: V_a = m_a/rho_a, so P_a V_a^2/m_a = P_a m_a/rho_a^2 with m_a = m_b for fluid neighbours; the element term is
(P_a (m/rho_a)^2 + P_s (deltap^3 rho0/rho_s)^2) rho_s/(deltap^3 rho0)/m = (P_a/rho_a^2 + P_s/rho_s^2) rho_s; the density-summation
weight m_a theta_b/theta_a = m_a m_b/m_a = m_b for fluid and vertex neighbours alike (one rho0); and the Brezzi factor
2/(m_a (rho_a/m_a + rho_b/m_b)) = 2/(rho_a + rho_b) for fluid neighbours.  Only the vertex neighbours differ: in the forces (theta of
a vertex from its actual volume) and in Brezzi (vertices take part at all).  So on SABox(0.1, jitter 0.1) with perturbed densities
the restatement evaluated with "HA" is held against the UNCHANGED CPU oracle with SPH_F1 (which knows nothing of SPH_HA):
  forces              the fluid and element parts (at this size every fluid row has a vertex in reach, so instead of selecting
                      rows without one, the vertex part is taken in its F1 form -- after the whole F1 restatement, vertex part
                      included, has been held against the oracle);
  density summation   the whole pass: the new density from the HA volumic sum;
  Brezzi              the fluid-neighbour part.
Bound: 1e-5 of the largest magnitude of the pass (the project's float-against-float bound, tests/kernel_agreement.py); a row with
elements in reach gets, on top, what the float evaluation of |grad gamma_as| of its own elements (the oracle's) moves it by.  The
density summation is compared as the physical density rho the pass computes (rho~ = rho/rho0 - 1 is stored: its float32 resolution,
6e-8, is coarser than 1e-5 of its own magnitude).  The two-fluid coefficients are checked on a hand-worked set of particles."""
import numpy as np
import pytest

from gpusph_amd import defs as D
from gpusph_amd.problem import SABox, info_type
import sa_ha_ref as R
from sa_helpers import OracleSaSim

TOL = 1e-5


@pytest.fixture(scope="module")
def case():
    sim = OracleSaSim(SABox(0.1, jitter=0.1))
    p = sim.problem
    t = info_type(sim.info)
    rng = np.random.default_rng(41)
    vel = sim.vel.copy()
    noisy = (t == D.PT_FLUID) | (t == D.PT_BOUNDARY)
    vel[noisy, 3] += (0.02*rng.standard_normal(int(noisy.sum()))).astype(np.float32)
    g = p.global_pos(sim.pos, sim.hash)
    fl = t == D.PT_FLUID
    vel[fl, 0] = (0.05*g[fl, 2]/p.H).astype(np.float32)
    vel[fl, 2] = (0.02*g[fl, 0]/p.l).astype(np.float32)
    ref = R.ha_ref_of_state(p, sim.pos, sim.hash, sim.info, sim.vertices, sim.be)
    return sim, vel, ref, np.where(fl)[0]


def test_forces_fluid_and_element_parts_equal_the_f1_oracle(case):
    sim, vel, ref, fl = case
    o, n, p = sim.o, sim.n, sim.problem
    want, _, _ = o.forces_sa(sim.pos, vel, sim.info, sim.hash, sim.cs, sim.nl, sim.gg, sim.be, sim.vertpos, n, p.m_deltap)
    want = want[:n, :3].astype(np.float64)
    scale = np.abs(want[fl]).max()
    mass, gam = sim.pos[:, 3], sim.gg[:, 3]
    f1 = ref.forces("F1", vel, mass, gam)
    shift_f1 = ref.float32_shift(p, sim.pos, sim.hash, sim.be, sim.vertpos)
    ha = ref.forces("HA", vel, mass, gam)
    shift = ref.float32_shift(p, sim.pos, sim.hash, sim.be, sim.vertpos)
    wall = ref.has_element[fl]
    for name, got, sh in (("F1 restatement", f1["total"], shift_f1),
                          ("HA fluid + element parts with the F1 vertex part", ha["total"] - ha["vertex"] + f1["vertex"], shift)):
        err = np.abs(got - want)[fl].max(axis=1)
        allowance = np.abs(sh)[fl].max(axis=1)
        print("%s: worst row %.3g of the scale %.3g (rows without elements %.3g, %d of %d); allowance up to %.3g; with the oracle's float "
              "|grad gamma_as| in the place of the float64 one: %.3g" % (name, err.max()/scale, scale, err[~wall].max()/scale if (~wall).any() else 0.0,
                                                                         (~wall).sum(), len(fl), allowance.max()/scale,
                                                                         np.abs(got + sh - want)[fl].max()/scale))
        assert (err <= TOL*scale + allowance).all()
        assert (err[~wall] <= TOL*scale).all()
        # and two-sided: with the oracle's float value of every |grad gamma_as| in the place of the float64 one nothing is left
        assert np.abs(got + sh - want)[fl].max() <= TOL*scale
    # the parts are alive, and the vertex part is where the two formulations differ
    for k in ("fluid", "vertex", "element"):
        assert np.abs(ha[k][fl]).max() > 0.02*scale
    # (the element identity needs m = rho0 deltap^3 exactly; the state's masses are that product rounded to float32: 2^-24 of it)
    assert np.abs(ha["fluid"] - f1["fluid"])[fl].max() < 1e-9*scale and np.abs(ha["element"] - f1["element"])[fl].max() < 1e-6*scale
    # HA weighs the two pressures of a vertex pair by rho0/rho_v and rho_v/rho0 (theta_v from the ACTUAL volume): with the vertices near
    # their rest density that is a few 1e-4 of the scale here, well above the bound of this test
    assert np.abs(ha["vertex"] - f1["vertex"])[fl].max() > 20*TOL*scale


def _displaced(sim, fl):
    rng = np.random.default_rng(43)
    new = sim.pos.copy()
    new[fl, :3] += (0.02*sim.problem.m_deltap*rng.uniform(-1.0, 1.0, size=(len(fl), 3))).astype(np.float32)
    return new


def test_density_summation_equals_the_f1_oracle(case):
    sim, vel, ref, fl = case
    o, n, p = sim.o, sim.n, sim.problem
    new = _displaced(sim, fl)
    vs, gs = o.sa_density_sum(vel.copy(), sim.pos, new, vel, sim.gg, sim.be, sim.vertpos, sim.info, sim.hash, sim.cs, sim.nl, n)
    rho0 = float(p.physparams.rho0[0])
    want = (vs[fl, 3].astype(np.float64) + 1.0)*rho0
    vol, _, _ = ref.density_sum("HA", p.global_pos(new, sim.hash), sim.pos[:, 3])
    vol_f1, _, _ = ref.density_sum("F1", p.global_pos(new, sim.hash), sim.pos[:, 3])
    assert np.abs(vol - vol_f1)[fl].max() < 1e-9*np.abs(vol_f1[fl]).max()      # m_a theta_b/theta_a = m_b: fluid and vertex neighbours
    # the gamma terms are not the formulation's: gamma of the new state is the oracle's; a stored gamma of exactly 1 or 0.1 may have
    # been clamped AFTER the division (the quotient used the unclamped value): only rows without an element are taken then
    gnew = gs[fl, 3].astype(np.float64)
    usable = ~(((gnew == 1.0) | (gnew == np.float32(0.1))) & ref.has_element[fl])
    assert usable.sum() > 0.9*len(fl)
    rho_old = (vel[fl, 3].astype(np.float64) + 1.0)*rho0
    got = (sim.gg[fl, 3].astype(np.float64)*rho_old + vol[fl])/gnew
    scale = np.abs(want).max()
    err = np.abs(got - want)[usable]
    print("density summation: worst row %.3g of the largest density %.3g; the volumic sum is up to %.3g" % (err.max()/scale, scale, np.abs(vol[fl]).max()))
    assert np.abs(vol[fl]).max() > 1e-3*scale
    assert (err <= TOL*scale).all()


def test_brezzi_fluid_part_equals_the_f1_oracle(case):
    sim, vel, ref, fl = case
    o, n, p = sim.o, sim.n, sim.problem
    dt = float(np.float32(p.simparams.dt))
    _, f = o.sa_density_diffusion(sim.pos, vel, sim.gg, sim.info, sim.hash, sim.cs, sim.nl, n, dt)
    want = f[fl, 3].astype(np.float64)
    b = ref.brezzi("HA", vel, sim.pos[:, 3], sim.gg[:, 3], dt)
    scale = np.abs(want).max()
    err = np.abs(b["fluid"][fl] - want)
    print("Brezzi, fluid neighbours: worst row %.3g of the scale %.3g; the vertex part of HA is up to %.3g of it" % (err.max()/scale, scale, np.abs(b["vertex"][fl]).max()/scale))
    assert (err <= TOL*scale).all()
    assert np.abs(b["vertex"][fl]).max() > 0.02*scale
    assert not R.HaRef.brezzi(ref, "F1", vel, sim.pos[:, 3], sim.gg[:, 3], dt)["vertex"].any()


def test_two_fluid_coefficients_by_hand():
    """one fluid-0 particle a, one fluid-1 particle b, one vertex v (fluid 1, half a cell) and one element s (fluid 0), deltap = 0.1:
    every number below is worked out from the formulas of the issue, not from the module's code"""
    dp = 0.1
    ma, rhoa, rho0a, Pa = 4.0, 4040.0, 4000.0, 5000.0          # V_a = 4/4040
    mb, rhob, rho0b, Pb = 1.0, 990.0, 1000.0, -1200.0          # V_b = 1/990
    mv, rhov, rho0v, Pv = 0.5, 1010.0, 1000.0, 800.0           # V_v = 0.5/1010, theta_v (actual) = V_v/1e-3
    rhos, rho0s, Ps = 4100.0, 4000.0, 9000.0                   # Vr_s = 1e-3 * 4000/4100
    Va, Vb, Vv = 4.0/4040.0, 1.0/990.0, 0.5/1010.0
    # forces: fluid <- fluid, theta = 1 on both sides
    assert R.pair_pressure("HA", Pa, ma, rhoa, Pb, mb, rhob, False, dp) == pytest.approx((5000.0*Va**2 - 1200.0*Vb**2)/4.0, rel=1e-13)
    # fluid <- vertex: theta_v = V_v/deltap^3 = 0.49504950...
    tv = Vv/1e-3
    assert tv == pytest.approx(0.4950495049504950, rel=1e-12)
    assert R.pair_pressure("HA", Pa, ma, rhoa, Pv, mv, rhov, True, dp) == pytest.approx((5000.0*Va**2*tv + 800.0*Vv**2/tv)/4.0, rel=1e-13)
    # fluid <- element: theta_a = 1 (a fluid particle), Vr_a = V_a
    Vrs = 1e-3*4000.0/4100.0
    assert R.element_pressure("HA", Pa, ma, rhoa, Ps, rhos, rho0s, dp) == pytest.approx((5000.0*Va**2 + 9000.0*Vrs**2)/Vrs/4.0, rel=1e-13)
    # density summation: theta from the initial volumes: theta_a = (4/4000)/1e-3 = 1, theta_b = 1, theta_v = 0.5
    assert R.dsum_weight("HA", ma, rho0a, mb, rho0b, dp) == pytest.approx(4.0, rel=1e-13)          # NOT m_b = 1: the heavy particle sees its own mass
    assert R.dsum_weight("HA", ma, rho0a, mv, rho0v, dp) == pytest.approx(2.0, rel=1e-13)          # half a cell of it
    assert R.dsum_weight("HA", mb, rho0b, ma, rho0a, dp) == pytest.approx(1.0, rel=1e-13)
    assert R.dsum_weight("F1", ma, rho0a, mb, rho0b, dp) == 1.0
    # Brezzi: 2/(m_a (1/V_a + theta_b/(theta_a V_b))), theta from the initial volumes (vertex: 0.5)
    assert R.brezzi_factor("HA", ma, rhoa, mb, rhob, rho0b, False, dp) == pytest.approx(2.0/(4.0*(1010.0 + 990.0)), rel=1e-13)
    assert R.brezzi_factor("HA", ma, rhoa, mv, rhov, rho0v, True, dp) == pytest.approx(2.0/(4.0*(1010.0 + 0.5*2020.0)), rel=1e-13)
    assert R.brezzi_factor("F1", ma, rhoa, mb, rhob, rho0b, False, dp) == pytest.approx(2.0/5030.0, rel=1e-13)
    # and the F1 forms for the same particles differ from the HA ones once the masses differ
    assert R.pair_pressure("F1", Pa, ma, rhoa, Pb, mb, rhob, False, dp) == pytest.approx((5000.0/4040.0**2 - 1200.0/990.0**2)*1.0, rel=1e-13)
    assert abs(R.pair_pressure("HA", Pa, ma, rhoa, Pb, mb, rhob, False, dp)/R.pair_pressure("F1", Pa, ma, rhoa, Pb, mb, rhob, False, dp) - 1.0) > 0.1
