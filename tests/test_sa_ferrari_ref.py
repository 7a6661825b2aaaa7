"""The float64 restatement of the Ferrari diffusion term with SA walls (tests/sa_ferrari_ref.py) against answers it shares no
code with: zero for a uniform field, linear in the coefficient, the gravity correction cancelling a hydrostatic field, the cut
at r <= 1e-4 h.  The restatement is what the kernels' term is held to (tests/test_sa_ferrari_hostemu.py, tests/test_gpu_sa_ferrari.py)."""
import numpy as np
import pytest

from gpusph_amd import defs as D
from gpusph_amd.problem import SABox, info_type, make_particleinfo
from sa_ferrari_ref import FerrariRef


@pytest.fixture(scope="module")
def tank():
    p = SABox(0.1, jitter=0.1, options="Spheric2SA")
    ref = FerrariRef(p, p.parts.pos_global, p.parts.info, p.vertices, p.boundelements)
    return p, ref


def test_option_set_mirrors_spheric2sa(tank):
    p, ref = tank
    sp = p.simparams
    assert sp.densitydiffusiontype == D.FERRARI and sp.boundarytype == D.SA_BOUNDARY and sp.kerneltype == D.WENDLAND
    assert sp.simflags & D.ENABLE_GAMMA_QUADRATURE and not sp.simflags & D.ENABLE_DENSITY_SUM
    # densityDiffCoeff = 1e-3 ferrariLengthScale / deltap with Spheric2SA's 0.161 / 0.02715
    assert abs(sp.densityDiffCoeff - 1e-3*0.161/0.02715) < 1e-8 and abs(ref.xi - sp.densityDiffCoeff) < 1e-9
    k = SABox(0.1, options="Spheric2SA", viscosity="KEPSVISC").simparams
    assert k.turbmodel == D.KEPSILON and k.rheologytype == D.NEWTONIAN and k.densitydiffusiontype == D.FERRARI
    assert len(ref.fe_i) > 1000 and (ref.fe_gg > 0).sum() > 500 and len(ref.ff_i) > 500


def test_uniform_density_without_gravity_gives_zero(tank):
    p, ref = tank
    n = p.num_particles
    g = ref.g.copy()
    try:
        ref.g = np.zeros(3)
        fs, es, _ = ref.sums(np.full(n, 0.0123), p.parts.pos_global[:, 3], np.ones(n))
    finally:
        ref.g = g
    assert not fs.any() and not es.any()
    # ... and not because nothing is summed: gravity alone leaves both sums alive
    fs, es, _ = ref.sums(np.full(n, 0.0123), p.parts.pos_global[:, 3], np.ones(n))
    assert np.abs(fs).max() > 0 and np.abs(es).max() > 0


def test_linear_in_the_coefficient(tank):
    p, ref = tank
    n = p.num_particles
    rng = np.random.default_rng(5)
    rt = p.parts.vel[:, 3].astype(np.float64) + 0.02*rng.standard_normal(n)
    m = p.parts.pos_global[:, 3]
    a = ref.sums(rt, m, np.ones(n))
    b = ref.sums(rt, m, np.ones(n), xi=3.0*ref.xi)
    for x, y in zip(a, b):
        assert np.abs(x).max() > 0 and np.abs(y - 3.0*x).max() <= 1e-13*np.abs(y).max()


def test_gravity_correction_cancels_the_hydrostatic_gradient():
    """Fluid and elements at the problem's own hydrostatic densities: the term with g_corr against the same term with g_corr
    forced to zero, as the ratio of the root mean squares over a group of fluid particles (both sums together; gamma drops out of
    the ratio).  A tank deep enough to have particles with neither a wall nor the free surface in reach: deltap 0.05, H 0.45,
    jitter 0.1.  Measured: bulk 0.072 (30 particles), floor 0.022 (15), corner 0.020 (4); each is asserted with a factor of two.  (In the bulk the sum
    WITHOUT the correction is small itself: on a lattice the hydrostatic differences of opposite neighbours cancel, and only the jitter
    leaves something.)
    (What is left is the curvature of the Tait density profile over a kernel radius and, next to a wall, the elements' densities
    being the hydrostatic ones at their centroids.)"""
    p = SABox(0.05, H=0.45, jitter=0.1, options="Spheric2SA")
    n = p.num_particles
    g = p.parts.pos_global[:, :3]
    dp, R = p.m_deltap, p.simparams.influenceRadius
    fluid = info_type(p.parts.info) == D.PT_FLUID
    side = np.minimum.reduce([g[:, 0], p.l - g[:, 0], g[:, 1], p.w - g[:, 1]])
    groups = dict(
        bulk=fluid & (side > R + dp) & (g[:, 2] > R + dp) & (g[:, 2] < p.water_level - R),
        floor=fluid & (side > R + dp) & (g[:, 2] < 1.5*dp),
        corner=fluid & (g[:, 2] < 1.5*dp) & (np.minimum(g[:, 0], p.l - g[:, 0]) < 1.5*dp) & (np.minimum(g[:, 1], p.w - g[:, 1]) < 1.5*dp))
    rows = np.where(groups["bulk"] | groups["floor"] | groups["corner"])[0]
    ref = FerrariRef(p, p.parts.pos_global, p.parts.info, p.vertices, p.boundelements, only=rows)
    rt, m = p.parts.vel[:, 3].astype(np.float64), p.parts.pos_global[:, 3]
    with_g = sum(ref.sums(rt, m, np.ones(n))[:2])
    without = sum(ref.sums(rt, m, np.ones(n), gravity_correction=False)[:2])
    assert not ref.sums(rt, m, np.ones(n))[1][groups["bulk"]].any()      # the bulk has no element in reach
    measured = dict(bulk=0.072, floor=0.022, corner=0.020)
    for name, sel in groups.items():
        assert sel.sum() >= (4 if name == "corner" else 10), (name, sel.sum())
        ratio = np.sqrt((with_g[sel]**2).mean())/np.sqrt((without[sel]**2).mean())
        print("hydrostatic tank, %s (%d particles): with g_corr / without = %.3g" % (name, sel.sum(), ratio))
        assert ratio <= 2.0*measured[name], (name, ratio)


def test_particle_on_the_centroid_of_an_element_gets_nothing_from_it():
    """One fluid particle and one element: on the centroid r = 0 and within 1e-4 h of it the element term is exactly zero (and
    finite: no 0/0); just beyond the cut it is alive."""
    p = SABox(0.1, options="Spheric2SA")
    dp, h = p.m_deltap, p.simparams.slength
    corners = np.array([[0.3, 0.2, 0.0], [0.4, 0.2, 0.0], [0.4, 0.3, 0.0]])
    centroid = corners.mean(axis=0)
    info = make_particleinfo(np.array([D.PT_FLUID, D.PT_BOUNDARY, D.PT_VERTEX, D.PT_VERTEX, D.PT_VERTEX], dtype=np.uint16),
                             np.zeros(5, dtype=np.uint16), np.arange(5, dtype=np.uint32))
    vertices = np.zeros((5, 4), dtype=np.uint32); vertices[1, :3] = (2, 3, 4)
    be = np.zeros((5, 4)); be[1] = (0.0, 0.0, 1.0, 0.5*dp*dp)
    rt = np.array([0.03, 0.01, 0.0, 0.0, 0.0]); m = np.full(5, 1000.0*dp**3)
    got = {}
    for name, lift in (("on", 0.0), ("inside", 0.5e-4*h), ("beyond", 2e-4*h), ("away", 0.3*h)):
        pos = np.vstack([centroid + (0.0, 0.0, lift), centroid, corners])
        ref = FerrariRef(p, pos, info, vertices, be)
        fs, es, _ = ref.sums(rt, m, np.ones(5))
        assert np.isfinite(es).all() and not fs.any()
        assert len(ref.fe_i) == 1 and ref.fe_gg[0] > 0
        got[name] = es[0]
    assert got["on"] == 0.0 and got["inside"] == 0.0
    # straight above the centroid (r.n)/r = 1 at any height: just beyond the cut the term is as alive as further up
    assert abs(got["beyond"]) > 1e-4 and abs(got["away"]) > 1e-4
