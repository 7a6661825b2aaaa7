"""All four SPH kernel functions through every engine they reach on the device.

The kernel function is a compile-time axis of almost every pair loop (forces_pair.h, filters.hip, energy.hip, rheology.hip, granular.hip);
the rest of the suite launches it with a kernel other than Wendland in a handful of places.  Here every engine runs with the cubic
spline, the quadratic, the Wendland (the CONTROL of every test: if its row fails, the harness is wrong and not a kernel) and the
Gaussian kernel.  The Gaussian is the NARROW one of tests/kernel_axis.py (smoothing factor 1.0): the only Gaussian problem of the suite
whose tiling fits, so the only one that runs forces_tile_kernel<SPHX_GAUSSIAN, ...> and the Gaussian stress mode at all
(tests/test_kernel_axis_allpairs.py proves the fit on the CPU for every option set used here).

Bars: the oracle to 2e-5 of a field's largest entry for the forces, bit for bit for the filters and the post-processing with the
polynomial kernels (filters.hip keeps the reference's operation order).  The Gaussian's W and F go through expf, where the device's
libm and glibc differ in the last place: there the device and the oracle are both measured against the float64 all-pairs value of
tests/allpairs_ref.py and the device may be at most FOUR times as far from it as the oracle is -- both are float32 sums in the same
order, so they can differ only by expf ulps passed through the same conditioning; a wrong term is not within that.

Comparisons that are NOT made, because they would prove nothing: for the option sets `two-fluids-colagrossi` and `ferrari` with a kernel
other than Wendland, sphx_tiles_opts_forces sends the forces pass to the generic kernel whether tiles are enabled or not, so tiled against
generic would compare a kernel with itself (test_forces_matrix[<cubicspline|quadratic|gaussian>-<two-fluids-colagrossi|ferrari>])."""
import numpy as np
import pytest

import allpairs_ref as ap
import kernel_axis as ka
import oracle_lib as ol
from forces_check import _check_neibs_and_forces, _engine, _np, _within_4x, tiles_usable
from gpusph_amd import defs as D
from kernel_agreement import assert_forces_agree

pytestmark = pytest.mark.gpu

kernels = pytest.mark.parametrize("kernel", ka.KERNELS, ids=ka.kernel_id)
other_kernels = pytest.mark.parametrize("kernel", [k for k in ka.KERNELS if k != D.WENDLAND], ids=ka.kernel_id)
POLYNOMIAL = (D.CUBICSPLINE, D.QUADRATIC, D.WENDLAND)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _upload(eng, sim):
    import torch
    eng.vel[:sim.n] = torch.from_numpy(sim.vel[:sim.n]).to(eng.device)


def _pair(prob, seed, dv=0.4):
    """(engine, oracle driver, float64 positions, constants) after the list build, in the same perturbed state"""
    sim, gp, k = ka.oracle_state(prob, seed, dv)
    eng = _engine(prob, clobber_neibslist=True)
    eng.build_neibs()
    n = eng.n
    assert n == sim.n and np.array_equal(_np(eng.hash, np.uint32)[:n], sim.hash[:n])
    assert np.array_equal(_np(eng.neibslist, np.uint16).reshape(-1, eng.alloc)[:, :n], sim.nl.reshape(-1, len(sim.pos))[:, :n])
    _upload(eng, sim)
    return eng, sim, gp, k


def _W(kernel, k):
    return lambda r: ka.W64(kernel, r, k["h"])


def _F(kernel, k):
    return lambda r: ka.F64(kernel, r, k["h"])


# ---------------------------------------------------------------------------------------------------------------------------------
# forces matrix

@pytest.mark.parametrize("name", list(ka.OPTION_SETS))
@kernels
def test_forces_matrix(kernel, name, monkeypatch):
    """lists bit-exact, forces / d(rho~)/dt / dt to 2e-5 against the oracle, the tiled pass against the generic one -- for every
    option set of tests/kernel_axis.py.  The tiling is built for a superset of what the consumers take: usable == 1 in every case"""
    prob = ka.option_problem(kernel, name)
    tiled = ka.OPTION_SETS[name][1] or kernel == D.WENDLAND
    # not tiled: the pass is the generic kernel's with or without tiles; comparing the two contexts would compare it with itself
    eng, sim = _check_neibs_and_forces(prob, 60 + list(ka.OPTION_SETS).index(name), monkeypatch if tiled else None,
                                       switch_flips=3 if name == "two-fluids-colagrossi" else 0, usable=1)
    n = eng.n
    tau = None
    if prob.num_obstacle:      # the rows of the feedback body (BUFFER_RB_FORCES), to the bar of test_forces_and_dt_tolerance
        if prob.simparams.turbmodel == D.SPS:
            tau = sim.o.sps(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, n)[0]
        rbf_ref = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, compute_object_forces=1,
                               rb_count=prob.num_obstacle, tau=tau)[3]
        if ka.OPTION_SETS[name][0].get("near_body"):      # the body stands in reach of the fluid: rows of it carry forces (with LJ
            assert (np.abs(rbf_ref).max(axis=1) > 0).sum() >= 3      # walls only those within r0 = dp of a fluid particle: a handful)
        assert np.abs(_np(eng.rbforces) - rbf_ref).max() <= 2e-5*max(np.abs(rbf_ref).max(), 1e-12)
    if prob.simparams.turbmodel == D.SPS:      # the stress term is far above the bar in this state: the comparison above saw it
        tau = sim.o.sps(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, n)[0]
        with_tau = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, tau=tau)[0][:n, :3]
        without = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, tau=np.zeros_like(tau))[0][:n, :3]
        assert np.abs(with_tau - without).max() > 10*2e-5*np.abs(with_tau).max()
    if name == "xsph":      # the XSPH rows of the pass (filters.hip's xsph_kernel) against orc_xsph
        ref = sim.o.xsph(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[:n]
        got = _np(eng.xsph)[:n]
        fluid = (sim.info[:n, 0] & 7) == D.PT_FLUID
        assert np.abs(ref[fluid, :3]).max() > 1e-3 and not got[~fluid].any()
        if kernel in POLYNOMIAL:
            assert np.array_equal(_bits(got), _bits(ref))
        else:
            gp = prob.global_pos(sim.pos[:n], sim.hash[:n])
            k = ap.consts(sim)
            f64 = ap.xsph(sim, gp, k, _W(kernel, k))
            assert np.abs(ref[:, :3] - f64).max() <= 2e-5*np.abs(f64).max()
            _within_4x("XSPH", got[:, :3], ref[:, :3], f64)


# ---------------------------------------------------------------------------------------------------------------------------------
# SPS stress: sps_kernel and the tiled stress mode

def _calc_visc(eng, n):
    eng.k.calc_visc(eng.tau, eng.pos, eng.vel, eng.info, eng.hash, eng.cellStart, eng.neibslist, n, n, turbvisc=eng.turbvisc)
    return np.concatenate([_np(t)[:n] for t in eng.tau], axis=1), _np(eng.turbvisc)[:n].copy()


@pytest.mark.parametrize("name", ["spsvisc", "sps-alone"])
@kernels
def test_sps_stress(kernel, name, monkeypatch):
    """sphx_calc_visc: tau and the turbulent viscosity to 2e-5 against orc_sps from the tiled stress mode (usable == 1, one fluid),
    and the tiled mode against sps_kernel (tiles disabled)"""
    prob = ka.option_problem(kernel, name)
    eng, sim, gp, k = _pair(prob, 11, dv=0.5)
    n = eng.n
    eng.neibs_info()
    assert tiles_usable(eng) == 1
    tau_ref, tv_ref = sim.o.sps(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, n)
    tau, tv = _calc_visc(eng, n)
    scale = np.abs(tau_ref[:n]).max()
    assert scale > 0 and np.abs(tau).max() > 0 and (np.abs(tau_ref[:n]).max(axis=0) > 0).all()
    assert np.abs(tau - tau_ref[:n]).max() <= 2e-5*scale
    assert np.abs(tv - tv_ref[:n]).max() <= 2e-5*np.abs(tv_ref[:n]).max()
    monkeypatch.setenv("SPHX_DISABLE_TILES", "1")
    gen = _engine(prob, clobber_neibslist=True)
    gen.build_neibs()
    _upload(gen, sim)
    tau_g, tv_g = _calc_visc(gen, n)
    assert tiles_usable(gen) == 0
    monkeypatch.setenv("SPHX_DISABLE_TILES", "0")
    assert np.abs(tau_g - tau_ref[:n]).max() <= 2e-5*scale
    assert_forces_agree(tau, tau_g, what="SPS stress")
    assert_forces_agree(tv[:, None], tv_g[:, None], what="turbulent viscosity")


# ---------------------------------------------------------------------------------------------------------------------------------
# density filters

@pytest.mark.parametrize("fluids", [1, 2], ids=["one-fluid", "two-fluids"])
@pytest.mark.parametrize("ftype", [D.SHEPARD_FILTER, D.MLS_FILTER], ids=["shepard", "mls"])
@kernels
def test_filters(kernel, ftype, fluids):
    """Polynomial kernels: bit for bit (the bar test_filters_bit_exact states).  Gaussian: the 4 x rule against the float64 value.
    The two-fluid state is there for the constant the Gaussian W subtracts: a constant added to every weight cancels out of both
    filters where the density is uniform (with one fluid it moves rho~ by 1e-6, which is the rounding), and moves rho~ by 2e-4 --
    a hundred times the rule's room -- where neighbours of 1000 and 850 kg/m^3 meet.
    Measured on an MI355X, narrow Gaussian, max |rho~ - float64| of the oracle / of the device: Shepard 6.62e-7 / 6.62e-7 (two fluids
    6.59e-7 / 6.59e-7), MLS 1.03e-6 / 1.03e-6 (two fluids 9.77e-7 / 9.62e-7); also in DESIGN.md 4"""
    prob = ka.problem(kernel, obstacle=True, two_fluids=fluids == 2)
    eng, sim, gp, k = _pair(prob, 3, dv=0.1)
    n = eng.n
    ref = sim.o.filter(ftype, sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[:n]
    eng.apply_filter(ftype)
    out = _np(eng.vel)[:n]
    fluid = (sim.info[:n, 0] & 7) == D.PT_FLUID
    assert np.abs(ref[fluid, 3] - sim.vel[:n, 3][fluid]).max() > 1e-4          # the filter does something to this state
    assert np.array_equal(_bits(out[:, :3]), _bits(ref[:, :3]))
    if kernel in POLYNOMIAL:
        assert np.array_equal(_bits(out[:, 3]), _bits(ref[:, 3])), "max |d rho~| = %g" % np.abs(out[:, 3] - ref[:, 3]).max()
        return
    W = _W(kernel, k)
    if ftype == D.SHEPARD_FILTER:
        f64 = ap.shepard(sim, gp, k, W)
        assert np.array_equal(_bits(out[~fluid, 3]), _bits(ref[~fluid, 3]))      # the others keep their rho~: a copy
    else:
        # MLS rewrites every row.  Wall particles see fluid neighbours on one side only, or none: their moment matrix is singular
        # or close to it, and what its inverse makes of an expf ulp has no bar.  Rows with a condition number above 100 are left
        # out (every fluid row is far below: 10 at most); the polynomial kernels hold those rows' code path bit for bit
        f64, cond = ap.mls(sim, gp, k, W)
        f64[~(cond <= 100.0)] = np.nan
        assert cond[fluid].max() <= 100.0 and np.isfinite(f64[~fluid]).sum() > 100
    assert np.isfinite(f64[fluid]).all()
    _within_4x("Gaussian %s rho~" % ("Shepard" if ftype == D.SHEPARD_FILTER else "MLS"), out[:, 3], ref[:, 3], f64)


# ---------------------------------------------------------------------------------------------------------------------------------
# post-processing

def _flags_equal_off_threshold(what, got, ref, near, flagged):
    """flags equal to the oracle's except where the deciding comparison is within 1e-5 of its threshold in float64; those have to be
    under 1 % of the flagged particles (else the SEED of the case is to change, not this cap)"""
    assert flagged > 10 and near.sum() < 0.01*flagged, "%s: %d of %d flagged particles on the threshold" % (what, near.sum(), flagged)
    assert np.array_equal(got[~near], ref[~near]), what


@kernels
def test_postprocess(kernel):
    """vorticity, surface detection with normals, test points.  Polynomial kernels: bit for bit (test-point pressure: powf, 4e-7).
    Gaussian: float fields by the 4 x rule, flags equal off the threshold.  Measured on an MI355X, oracle / device from float64:
    vorticity 3.06e-6 / 3.06e-6, surface normal (times its length) 3.78e-6 for both, its Shepard sum 4.57e-7 for both, test-point
    velocity 3.63e-8 for both, test-point pressure 7.68e-3 / 7.66e-3 Pa; no particle of the 12 flagged ones on the threshold"""
    prob = ka.problem(kernel, obstacle=True, testpoints=ka.TESTPOINTS)
    eng, sim, gp, k = _pair(prob, 9)
    n = eng.n
    vel = sim.vel.copy()
    W, F = _W(kernel, k), _F(kernel, k)
    gauss = kernel == D.GAUSSIAN
    fluid = (sim.info[:n, 0] & 7) == D.PT_FLUID
    # vorticity
    ref = sim.o.vorticity(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[:n]
    out = _np(eng.postprocess(D.VORTICITY))
    assert np.abs(ref[fluid]).max() > 1.0
    if gauss:
        assert np.array_equal(np.isnan(out), np.isnan(ref))
        _within_4x("Gaussian vorticity", out, ref, ap.vorticity(sim, gp, k, F))
    else:
        assert np.array_equal(_bits(out), _bits(ref))      # NaN rows included
    # surface detection (+ normals)
    ref_info, ref_nrm = sim.o.surface(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, normals=True)
    nrm = _np(eng.postprocess(D.SURFACE_DETECTION, normals=True))
    got_info = _np(eng.info, np.uint16)[:n]
    flagged = int(((ref_info[:n, 0] & D.FG_SURFACE) != 0).sum())
    assert flagged > 10
    if gauss:
        f64, margin, length = ap.surface(sim, gp, k, W, F)
        _flags_equal_off_threshold("surface", got_info, ref_info[:n], ka.near_threshold(margin), flagged)
        assert np.array_equal(np.isnan(nrm), np.isnan(ref_nrm[:n]))
        _within_4x("Gaussian surface normal", nrm[:, :3], ref_nrm[:n, :3], f64[:, :3], weight=np.c_[length, length, length])
        _within_4x("Gaussian surface Shepard sum", nrm[:, 3], ref_nrm[:n, 3], f64[:, 3])
    else:
        assert np.array_equal(got_info, ref_info[:n])
        assert np.array_equal(_bits(nrm), _bits(ref_nrm[:n]))
    # test points (last: it overwrites velocity rows)
    ref_vel = sim.o.testpoints(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[:n]
    eng.postprocess(D.TESTPOINTS)
    got = _np(eng.vel)[:n]
    tp = (sim.info[:n, 0] & 7) == D.PT_TESTPOINT
    assert tp.sum() == 3 and (np.abs(ref_vel[tp]).max(axis=0) > 0).all()
    assert np.array_equal(_bits(got[~tp]), _bits(vel[:n][~tp]))
    if gauss:
        idx, f64 = ap.testpoints(sim, gp, k, W)
        assert np.array_equal(idx, np.where(tp)[0])
        _within_4x("Gaussian test-point velocity", got[tp, :3], ref_vel[tp, :3], f64[:, :3])
        _within_4x("Gaussian test-point pressure", got[tp, 3], ref_vel[tp, 3], f64[:, 3])
    else:
        assert np.array_equal(_bits(got[tp, :3]), _bits(ref_vel[tp, :3]))
        # pressure goes through powf: device libm vs glibc, 2 ulp
        assert np.abs(got[tp, 3] - ref_vel[tp, 3]).max() <= 4e-7*np.abs(ref_vel[tp, 3]).max()


@kernels
def test_interface_detection(kernel):
    """INTERFACE_DETECTION on the two-fluid column with the body: flags and normals as test_interface_detection_bit_exact has them
    for the polynomial kernels; the Gaussian by the 4 x rule, flags equal off the thresholds of the two cone tests.  Measured on an
    MI355X, oracle and device alike: normal (times its length) 4.11e-6, Shepard sum 5.81e-7 from float64; 12 + 28 flagged, none
    on a threshold"""
    prob = ka.problem(kernel, obstacle=True, two_fluids=True)
    eng, sim, gp, k = _pair(prob, 10)
    n = eng.n
    ref_info, ref_nrm = sim.o.interface(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, normals=True)
    nrm = _np(eng.postprocess(D.INTERFACE_DETECTION, normals=True))
    got = _np(eng.info, np.uint16)[:n]
    surf, intf = int(((ref_info[:n, 0] & D.FG_SURFACE) != 0).sum()), int(((ref_info[:n, 0] & D.FG_INTERFACE) != 0).sum())
    assert surf > 10 and intf > 10
    if kernel in POLYNOMIAL:
        assert np.array_equal(got, ref_info[:n])
        assert np.array_equal(_bits(nrm), _bits(ref_nrm[:n]))
        return
    f64, mfs, mif, length = ap.interface(sim, gp, k, _W(kernel, k), _F(kernel, k))
    near = ka.near_threshold(mfs) | ka.near_threshold(mif)
    _flags_equal_off_threshold("interface", got, ref_info[:n], near, surf + intf)
    assert np.array_equal(np.isnan(nrm), np.isnan(ref_nrm[:n]))
    f64[near] = np.nan          # which of the two normals such a particle stores is the rounding's to decide as well
    _within_4x("Gaussian interface normal", nrm[:, :3], ref_nrm[:n, :3], f64[:, :3], weight=np.c_[length, length, length])
    _within_4x("Gaussian interface Shepard sum", nrm[:, 3], ref_nrm[:n, 3], f64[:, 3])


# ---------------------------------------------------------------------------------------------------------------------------------
# energy rate

@kernels
def test_energy_rate(kernel):
    """forces_internal_energy on the plain option set, to the 3e-5 of tests/test_gpu_energy.py"""
    prob = ka.problem(kernel, obstacle=False, internal_energy=True)
    eng, sim, gp, k = _pair(prob, 9)
    n = eng.n
    dedt = np.zeros(len(sim.pos), dtype=np.float32)
    sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, dedt=dedt)
    eng.dedt.fill_(7.0)
    eng.k.forces_internal_energy(eng.dedt, eng.pos, eng.vel, eng.info, eng.hash, eng.cellStart, eng.neibslist, n, 0, n)
    got = _np(eng.dedt)[:n]
    scale = np.abs(dedt[:n]).max()
    assert scale > 0
    assert np.abs(got - dedt[:n]).max() <= 3e-5*scale
    assert np.abs(got[(sim.info[:n, 0] & 7) == D.PT_BOUNDARY]).max() > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the consumers of rheology.hip's kernel functions (gn_F / gn_W), for the kernels the rest of the suite never gives them

HA_VISC = dict(rheologytype=D.NEWTONIAN, turbmodel=D.LAMINAR_FLOW, compvisc=D.DYNAMIC, avgop=D.HARMONIC)
GN_CASES = {
    "sph-ha": dict(obstacle=False, two_fluids=True, formulation=D.SPH_HA, viscosity=HA_VISC),
    "monaghan": dict(obstacle=False, kinematic_visc=0.05, density_diffusion=D.DENSITY_DIFFUSION_NONE,
                     viscosity=dict(rheologytype=D.NEWTONIAN, turbmodel=D.LAMINAR_FLOW, viscmodel=D.MONAGHAN, compvisc=D.KINEMATIC,
                                    avgop=D.HARMONIC)),
    "papanastasiou": dict(obstacle=False, kinematic_visc=0.05,
                          viscosity=dict(rheologytype=D.PAPANASTASIOU, turbmodel=D.LAMINAR_FLOW, compvisc=D.KINEMATIC, avgop=D.HARMONIC)),
}


def _gn_problem(kernel, case):
    prob = ka.problem(kernel, **GN_CASES[case])
    if case == "papanastasiou":
        prob.physparams.set_yield_strength(0, 2.0)
    return prob


@pytest.mark.parametrize("case", list(GN_CASES))
@other_kernels
def test_rheology_kernels(kernel, case):
    """one SPH_HA forces pass, one MONAGHAN pass, one Papanastasiou effective-viscosity + forces pass on the dam-break mirror, with the
    bars of tests/test_gpu_rheology.py: forces 2e-5 of the largest component, effective viscosity 3e-5 relative"""
    import torch
    eng, sim, gp, k = _pair(_gn_problem(kernel, case), 21, dv=0.3)
    n = eng.n
    eff = None
    if case == "papanastasiou":
        eff, mx = sim.o.effective_visc(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)
        got_mx = eng.k.calc_effvisc(eng.effvisc, eng.pos, eng.vel, eng.info, eng.hash, eng.cellStart, eng.neibslist, n, n)
        np.testing.assert_allclose(_np(eng.effvisc)[:n], eff[:n], rtol=3e-5)
        assert got_mx == pytest.approx(mx, rel=3e-5)
        assert np.ptp(eff[:n]) > 0.05*eff[:n].max()                      # the field really varies
        eng.effvisc[:n].copy_(torch.from_numpy(eff[:n]).to(eng.device))      # forces on the oracle's viscosity field
        f = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, effvisc=eff)[0]
        eng.k.memset(eng.forces, 0); eng.k.memset(eng.cfl, 0)
        eng.k.forces_effvisc(eng.forces, eng.cfl, eng.pos, eng.vel, eng.info, eng.hash, eng.cellStart, eng.neibslist, eng.effvisc, n, 0, n, 0)
    else:
        f = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[0]
        eng._forces(eng.pos, eng.vel, 1, 0)
    gf = _np(eng.forces)[:n]
    scale = np.abs(f[:n, :3]).max()
    assert scale > 0
    assert np.abs(gf[:, :3] - f[:n, :3]).max() <= 2e-5*scale
    assert np.abs(gf[:, 3] - f[:n, 3]).max() <= 2e-5*np.abs(f[:n, 3]).max() + 1e-7
    # the viscous term these kernels carry matters at this bar
    if case != "sph-ha":
        sim.o.p.visccoeff[0] *= 0.5
        f2 = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, effvisc=None if eff is None else eff*np.float32(0.5))[0]
        assert np.abs(f2[:n, :3] - f[:n, :3]).max() > 10*2e-5*scale


def test_granular_jacobi_vectors_with_the_cubic_spline():
    """granular.hip reads gn_F / gn_W too: the wall pass and one build of the Jacobi vectors on the jittered LithostaticColumn with the
    cubic spline, against the float64 all-pairs restatement tests/granular_ref.py (which carries the kernel functions itself), to the
    bar of tests/test_gpu_granular.py"""
    import torch
    from test_gpu_granular import TOL, _Case, _dev
    c = _Case(kerneltype=D.CUBICSPLINE)
    ref, n, eng, K = c.ref, c.n, c.eng, c.eng.k
    assert c.pr.simparams.kerneltype == D.CUBICSPLINE and ref.interior.sum() > 100 and ref.is_wall.sum() > 100
    p0 = np.random.default_rng(5).uniform(0.0, 4000.0, size=eng.alloc).astype(np.float32)
    p = _dev(eng, p0)
    err = K.jacobi_wall_boundary_conditions(p, *c.state, n, n)
    got = _np(p)[:n]
    want, want_err = ref.wall_boundary_conditions(p0[:n])
    assert np.abs(got - want).max() <= TOL*np.abs(want).max()
    assert want_err > 0 and abs(err - want_err) <= TOL*np.abs(want).max()/ref.refpres_wall
    jac = torch.full((eng.alloc, 4), 7.0, dtype=torch.float32, device=eng.device)
    p = _dev(eng, p0)
    K.jacobi_build_vectors(jac, p, *c.state, n, n)
    j = _np(jac)[:n]
    Dv, Rx, B = ref.build_vectors(p0[:n])
    for name, got, w in (("D", j[:, 0], Dv), ("Rx", j[:, 1], Rx), ("B", j[:, 2], B)):
        assert np.abs(w).max() > 0
        assert np.abs(got[ref.active] - w[ref.active]).max() <= TOL*np.abs(w).max(), name


# ---------------------------------------------------------------------------------------------------------------------------------
# trajectory on the tiled path

@other_kernels
def test_trajectory(kernel):
    """12 steps from rho~ = 0 spanning a list rebuild, the tolerances of test_gpu_parity.TRAJ's 12-step case; the only place the narrow
    Gaussian's tiled kernel runs in sequence with the integrator"""
    steps, vtol, rtol = 12, 1e-3, 2e-6
    prob = ka.problem(kernel, obstacle=True)
    eng = _engine(prob)
    sim = ol.OracleSim(prob)
    for _ in range(steps):
        sim.step()
        eng.step()
    assert steps > prob.simparams.buildneibsfreq and tiles_usable(eng) == 1
    out = eng.download()
    n = eng.n
    assert n == sim.n
    assert abs(eng.current_dt() - sim.dt) <= 1e-4*sim.dt
    same = (out["info"] == sim.info[:n]).all(axis=1)
    assert same.mean() > 0.999
    ids_g = out["info"][:, 2].astype(np.uint32) | (out["info"][:, 3].astype(np.uint32) << 16)
    ids_o = sim.info[:n, 2].astype(np.uint32) | (sim.info[:n, 3].astype(np.uint32) << 16)
    og = np.argsort(ids_g); oo = np.argsort(ids_o)
    gp = prob.global_pos(out["pos"][og], out["hash"][og])
    op = prob.global_pos(sim.pos[:n][oo], sim.hash[:n][oo])
    assert np.abs(gp - op).max() <= 1e-6*prob.m_cellsize.min()*steps
    vscale = max(np.abs(sim.vel[:n, :3]).max(), 1e-3)
    assert np.abs(out["vel"][og][:, :3] - sim.vel[:n][oo][:, :3]).max() <= vtol*vscale
    assert np.abs(out["vel"][og][:, 3] - sim.vel[:n][oo][:, 3]).max() <= rtol
