"""Ferrari density diffusion in the continuity-equation form with SA walls (Spheric2SA's option set) on the CPU: the list
walker's own source (sa_bounds.hip's sa_forces_kernel, run by tests/hostemu one emulated thread after the other) against the
float64 all-pairs restatement of tests/sa_ferrari_ref.py, laminar and k-epsilon.  The state: SABox(0.1, jitter 0.1) as the
boundary conditions initialise it, then two per cent of seeded noise on the densities of fluid and elements and a sheared
velocity field, so that the continuity term and the diffusion term are of the same order.

The bound is the one tests/test_gpu_sa.py applies to the SA forces against the oracle: 1e-4 of the largest |force.w| of the
pass for every row, and for a row with boundary elements in reach twice what the float32 evaluation of |grad gamma_as| of ITS
elements in the reference's operation order (the CPU oracle's) moves the row by, on top (tests/sa_helpers.py
assert_wall_rows_no_farther_from_float64: tol * scale + 2 |oracle - float64|).  Measured here: without that allowance the worst
row of this tank is 3.9e-4 of the scale off -- four elements the support only grazes, whose float value is 4e-3 / m beside the
float64 one in the oracle's evaluation and in the walker's alike (an independent quadrature of the kernel over the elements sides
with float64); with the oracle's float values of |grad gamma_as| in the place of the float64 ones the worst row is 6e-6 of the
scale off.  (At this size every fluid particle has elements in reach.)"""
import ctypes as C

import numpy as np
import pytest

from gpusph_amd import capi, defs as D
from gpusph_amd.problem import SABox, info_type
from hostemu_lib import Emu
from sa_ferrari_ref import ferrari_ref_of_state, float32_shift
from sa_helpers import OracleSaSim

TOL = 1e-4


def _state(viscosity):
    """the oracle's initialised state of the tank, perturbed; the same for both runs of a case"""
    sim = OracleSaSim(SABox(0.1, jitter=0.1, options="Spheric2SA", viscosity=viscosity))
    p, n = sim.problem, sim.n
    t = info_type(sim.info)
    rng = np.random.default_rng(41)
    vel = sim.vel.copy()
    noisy = (t == D.PT_FLUID) | (t == D.PT_BOUNDARY)
    vel[noisy, 3] += (0.02*rng.standard_normal(int(noisy.sum()))).astype(np.float32)
    g = p.global_pos(sim.pos, sim.hash)
    fl = t == D.PT_FLUID
    vel[fl, 0] = (0.05*g[fl, 2]/p.H).astype(np.float32)      # du/dz
    vel[fl, 2] = (0.02*g[fl, 0]/p.l).astype(np.float32)
    return sim, vel


def _forces(sim, vel, diffusion, dsum=False):
    """force rows (and the k-epsilon rows) of the emulated walker for the option set with or without Ferrari diffusion"""
    p, n = sim.problem, sim.n
    q = SABox(0.1, jitter=0.1, options="Spheric2SA", viscosity="KEPSVISC" if sim.keps else "DYNAMICVISC")
    q.simparams.densitydiffusiontype = D.FERRARI if diffusion else D.DENSITY_DIFFUSION_NONE
    if dsum:
        q.simparams.simflags = (q.simparams.simflags | D.ENABLE_DENSITY_SUM) & ~D.ENABLE_GAMMA_QUADRATURE
    emu = Emu(q.sphx_params(n))
    P = emu.params
    out = np.zeros_like(sim.vel)
    d_cfl = np.zeros(n + 64, dtype=np.float32)      # one entry per block of particles: room to spare
    hnb = C.c_uint32(0)
    vp = [np.ascontiguousarray(v) for v in sim.vertpos]
    common = (n, 0, n, float(np.float32(p.m_deltap)), float(P.slength), float(P.dtadaptfactor), float(P.influenceradius))
    dkde = None
    try:
        if sim.keps:
            name = "sphx_forces_basicstep_sa_keps"
            fn = getattr(emu.lib, name)
            fn.restype, fn.argtypes = capi.SIGNATURES[name]
            dkde = np.zeros(3*len(sim.pos), dtype=np.float32)
            d_cflk = np.zeros_like(d_cfl)
            ke = sim.ke
            emu.call(name, out, d_cfl, None, d_cflk, dkde, sim.pos, vel, sim.info, sim.hash, sim.cs, sim.nl, sim.gg, sim.be, vp[0], vp[1], vp[2],
                     ke["tke"], ke["eps"], ke["turbvisc"], ke["eulervel"], *common, 5e-5, 0, D.SIMULATE, 1, 0.0, C.addressof(hnb), None)
        else:
            emu.call("sphx_forces_basicstep_sa", out, d_cfl, None, sim.pos, vel, sim.info, sim.hash, sim.cs, sim.nl, sim.gg, sim.be,
                     vp[0], vp[1], vp[2], *common, 0, D.SIMULATE, 1, 0.0, C.addressof(hnb), None)
    finally:
        emu.close()
    return out, dkde


@pytest.fixture(scope="module", params=["DYNAMICVISC", "KEPSVISC"])
def case(request):
    sim, vel = _state(request.param)
    ref = ferrari_ref_of_state(sim.problem, sim.pos, sim.hash, sim.info, sim.vertices, sim.be)
    return sim, vel, ref


def test_ferrari_part_of_the_walker_equals_the_restatement(case):
    """force.w(Ferrari) - force.w(no diffusion) of the walker's source against the float64 all-pairs sums.  Before the term was
    built the first call was refused ("density diffusion with SA_BOUNDARY: Brezzi with density summation only")."""
    sim, vel, ref = case
    n = sim.n
    with_d, _ = _forces(sim, vel, True)
    without, _ = _forces(sim, vel, False)
    fl = np.where(info_type(sim.info) == D.PT_FLUID)[0]
    fs, es, room = ref.sums(vel[:, 3], sim.pos[:, 3], sim.gg[:, 3])
    want = fs + es
    got = with_d[:, 3].astype(np.float64) - without[:, 3].astype(np.float64)
    scale = np.abs(with_d[fl, 3]).max()
    err = np.abs(got - want)[fl]
    wall = es[fl] != 0
    print("Ferrari part: max |restatement| %.3g (fluid sum %.3g, element sum %.3g) against max |force.w| %.3g; error max %.3g of the scale, "
          "rows without elements %.3g; %d of %d rows with elements in reach"
          % (np.abs(want[fl]).max(), np.abs(fs[fl]).max(), np.abs(es[fl]).max(), scale, err.max()/scale,
             err[~wall].max()/scale if (~wall).any() else 0.0, wall.sum(), len(fl)))
    # the term is no rounding-sized correction of the pass: a fifth of the largest force.w at least, both sums alive
    assert np.abs(want[fl]).max() > 0.2*scale and np.abs(fs[fl]).max() > 0.05*scale and np.abs(es[fl]).max() > 0.05*scale
    shift = float32_shift(ref, sim.problem, sim.pos, sim.hash, sim.be, sim.vertpos)
    allowance = 2.0*np.abs(shift)[fl]
    print("   largest allowance for float32 |grad gamma_as|: %.3g of the scale; error left when the oracle's float values stand in: %.3g"
          % (allowance.max()/scale, np.abs(got - want - shift)[fl].max()/scale))
    assert (err <= TOL*scale + allowance).all(), "worst row %g of the scale" % (err/scale).max()
    assert (err[~wall] <= TOL*scale).all()
    assert not got[info_type(sim.info) != D.PT_FLUID].any()


def test_nothing_else_in_the_pass_sees_the_term(case):
    sim, vel, ref = case
    with_d, dk1 = _forces(sim, vel, True)
    without, dk0 = _forces(sim, vel, False)
    assert np.array_equal(with_d[:, :3].view(np.uint32), without[:, :3].view(np.uint32))
    assert np.abs(with_d[:, :3]).max() > 0
    if sim.keps:
        assert np.array_equal(dk1.view(np.uint32), dk0.view(np.uint32)) and dk1.any()
    assert not np.array_equal(with_d[:, 3], without[:, 3])


def test_ferrari_with_density_summation_is_refused(case):
    sim, vel, ref = case
    with pytest.raises(RuntimeError, match="Ferrari density diffusion with SA_BOUNDARY.*not built with ENABLE_DENSITY_SUM"):
        _forces(sim, vel, True, dsum=True)
