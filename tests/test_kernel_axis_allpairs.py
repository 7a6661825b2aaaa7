"""The oracle on the KERNEL-FUNCTION axis, held by something that shares nothing with it (no GPU).

The device tests of tests/test_gpu_kernel_axis.py compare every engine with oracle/sph_oracle.c for all four kernel functions; here
the oracle's own pair sums are compared, per kernel, with float64 all-pairs evaluations (tests/allpairs_ref.py: k-d tree on global
positions, no cells or lists) whose W and F are tests/kernel_axis.py's W64 / F64 -- written from the reference's formulas, and held
themselves by the reference's recorded values, the unit integral, W' = r F and the cubic spline's continuity at its knot.
Also here: the precondition of the device tests, that the narrow Gaussian's tiling FITS for every option set they launch.

Bar of every pair sum: 2e-5 of the field's largest entry."""
import functools
import os

import numpy as np
import pytest

import allpairs_ref as ap
import kernel_axis as ka
import oracle_lib as ol
import tiling_overflow_cases as toc
from gpusph_amd import defs as D
from gpusph_amd.problem import DamBreak3D

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
kernels = pytest.mark.parametrize("kernel", ka.KERNELS, ids=ka.kernel_id)
TOL = 2e-5


# ---------------------------------------------------------------------------------------------------------------------------------
# W64 / F64 themselves

def _slope(fn, kernel, r, h):
    """r d/dr of W64 or F64 by a central difference (what a rounding of the argument r/h is multiplied by)"""
    d = 1e-6*r
    return r*(fn(kernel, r + d, h) - fn(kernel, r - d, h))/(2*d)


@kernels
def test_w64_f64_equal_the_references_recorded_values(kernel):
    """tests/golden/ref_kernels.npz holds W and F as the reference's own float32 code returns them.  W64 / F64 have to agree to the
    float32 rounding of that evaluation, 2 ulp: 2 ulp of the value -- for W of the kernel's peak where the value is smaller, since
    the polynomials sum terms of that size -- plus 2 ulp of the ARGUMENT r/h passed through the kernel's slope r dK/dr.  The second
    term is the rounding of the reference's `R = r/slength`, which is what decides the last digits where the kernel runs out
    ((2 - R)^3 at R = 1.9999 has lost three digits to it; exp(-R^2) at R = 3 carries 9 times the argument's relative error).  2 ulp of
    the value alone cannot be met there by ANY evaluation, the reference's float32 one included, and the recorded points are chosen
    to lie there."""
    g = np.load(os.path.join(GOLD, "ref_kernels.npz"))
    sel = g["kerneltype"] == kernel
    assert sel.sum() >= 100
    two_ulp = 2.0**-22
    worst_w = worst_f = 0.0
    for r, h, w_ref, f_ref in zip(g["r"][sel].astype(np.float64), g["slength"][sel].astype(np.float64),
                                  g["W"][sel].astype(np.float64), g["F"][sel].astype(np.float64)):
        w, f = float(ka.W64(kernel, r, h)), float(ka.F64(kernel, r, h))
        bw = two_ulp*(max(abs(w_ref), float(ka.W64(kernel, 0.0, h))) + abs(_slope(ka.W64, kernel, r, h)))
        bf = two_ulp*(abs(f_ref) + abs(_slope(ka.F64, kernel, r, h)))
        worst_w, worst_f = max(worst_w, abs(w - w_ref)/bw), max(worst_f, abs(f - f_ref)/bf)
        assert abs(w - w_ref) <= bw, (kernel, r/h, w, w_ref)
        assert abs(f - f_ref) <= bf, (kernel, r/h, f, f_ref)
    print("%s: worst |W64 - ref| %.2f of its bound, |F64 - ref| %.2f" % (ka.kernel_id(kernel), worst_w, worst_f))
    # and the bound is no licence: over most of the support it IS 2 ulp of the value to within a small factor
    q = g["r"][sel].astype(np.float64)/g["slength"][sel].astype(np.float64)
    mid = (q > 0.2) & (q < 1.2)
    assert mid.sum() > 20
    for r, h, f_ref in zip(g["r"][sel][mid].astype(np.float64), g["slength"][sel][mid].astype(np.float64), g["F"][sel][mid].astype(np.float64)):
        assert abs(float(ka.F64(kernel, r, h)) - f_ref) <= 8*two_ulp*abs(f_ref)


@kernels
def test_w64_integrates_to_one(kernel):
    h = 0.0375
    R = ka.radius(kernel)*h
    # Gauss-Legendre on each smooth piece (the cubic spline's knot at r = h is a panel boundary)
    x, wq = np.polynomial.legendre.leggauss(40)
    total = 0.0
    for a, b in ((0.0, h), (h, R)):
        r = 0.5*(b - a)*x + 0.5*(b + a)
        total += 0.5*(b - a)*(wq*4.0*np.pi*r*r*ka.W64(kernel, r, h)).sum()
    assert abs(total - 1.0) <= 1e-6, total


@kernels
def test_f64_is_the_derivative_of_w64_over_r(kernel):
    h = 0.0375
    q = np.linspace(0.05, ka.radius(kernel) - 0.05, 400)
    q = q[np.abs(q - 1.0) > 0.01]                # the cubic spline's second derivative jumps at its knot
    r = q*h
    d = 1e-5*h
    dW = (ka.W64(kernel, r + d, h) - ka.W64(kernel, r - d, h))/(2*d)
    F = ka.F64(kernel, r, h)
    assert np.abs(dW/r - F).max() <= 1e-6*np.abs(F).max()
    assert np.abs(dW/r/F - 1.0)[q < ka.radius(kernel) - 0.5].max() <= 1e-6


def test_cubic_spline_is_continuous_at_its_knot():
    h = 0.0375
    for fn in (ka.W64, ka.F64):
        below, above = float(fn(D.CUBICSPLINE, h*(1 - 1e-13), h)), float(fn(D.CUBICSPLINE, h*(1 + 1e-13), h))
        assert below != 0 and abs(below - above) <= 1e-11*abs(below)
    assert float(ka.W64(D.CUBICSPLINE, h, h)) == pytest.approx(0.25/(np.pi*h**3), rel=1e-14)
    assert float(ka.F64(D.CUBICSPLINE, h, h)) == pytest.approx(-3.0/(4.0*np.pi*h**5), rel=1e-14)


# ---------------------------------------------------------------------------------------------------------------------------------
# the narrow Gaussian fits the tiles

@pytest.mark.parametrize("name", sorted(ka.OPTION_SETS))
def test_the_narrow_gaussian_tiles_for_every_option_set(name):
    """what tests/test_tiling_overflow_cases.py proves of the overflow cases, the other way round: every list fits AND nothing of the
    tiling reaches a limit, so that `tiles_usable == 1` on the device is the tiled Gaussian kernels running"""
    lim = toc.limits()
    prob = ka.option_problem(D.GAUSSIAN, name)
    assert prob.simparams.sfactor == ka.NARROW_SFACTOR and prob.simparams.kernelradius == 3.0
    s = toc.survey(prob)
    print("%s: n = %d, longest fluid section %d, second %d, fullest home column %d, fullest window %d"
          % (name, s["n"], s["first"].max(), s["second"].max(), s["home"].max(), s["window"].max()))
    assert s["too_many"] == -1
    assert s["first"].max() <= lim["list"] and s["second"].max() <= lim["list"]
    assert s["home"].max() <= lim["pmax"]
    assert s["window"].max() <= lim["wcap_sps"]          # the tightest of the three window capacities
    assert 2500 <= s["n"] <= 6000


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle's pair sums per kernel against float64 all-pairs evaluations

@functools.lru_cache(maxsize=None)
def _state(kernel, viscosity=None, seed=5):
    """DamBreak3D with the body, jittered, hydrostatic, a sheared and converging velocity field plus noise, densities off the
    hydrostatic profile by up to 0.4 % (most pairs far from the Colagrossi threshold).  The Gaussian is the narrow one."""
    cls = toc.wide(DamBreak3D, ka.NARROW_SFACTOR) if kernel == D.GAUSSIAN else DamBreak3D
    prob = cls(0.04, obstacle=True, jitter=0.15, hydrostatic=True, kerneltype=kernel, viscosity=viscosity, kinematic_visc=1.0e-6)
    sim = ol.OracleSim(prob)
    sim.build_neibs()
    assert sim.neibs_info.hasTooManyNeibs == -1
    n = sim.n
    rng = np.random.default_rng(seed)
    gp = prob.global_pos(sim.pos[:n], sim.hash[:n])
    v = np.stack([0.8*np.sin(3.0*gp[:, 2]) - 0.5*gp[:, 0], 0.6*np.cos(2.0*gp[:, 0]) - 0.4*gp[:, 1],
                  0.3*gp[:, 0]*gp[:, 1] - 0.5*gp[:, 2]], axis=1) + rng.normal(0, 0.15, size=(n, 3))
    sim.vel[:n, :3] = v.astype(np.float32)
    sim.vel[:n, 3] += rng.uniform(-4e-3, 4e-3, size=n).astype(np.float32)
    k = ap.consts(sim)
    assert sim.o.p.kerneltype == kernel and k["R"] == pytest.approx(ka.radius(kernel)*k["h"], rel=1e-6)
    return prob, sim, gp, k


def _F(kernel, k):
    return lambda r: ka.F64(kernel, r, k["h"])


def _W(kernel, k):
    return lambda r: ka.W64(kernel, r, k["h"])


@kernels
def test_momentum_and_continuity_per_kernel(kernel):
    """the headline option set (tests/test_headline_allpairs.py) with each kernel function"""
    prob, sim, gp, k = _state(kernel)
    n = sim.n
    p = sim.o.p
    assert p.densitydiffusiontype == D.COLAGROSSI and p.boundarytype == D.DYN_BOUNDARY and p.turbmodel == D.ARTIFICIAL
    f = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[0][:n].astype(np.float64)
    ref = ap.momentum_continuity(sim, gp, k, _F(kernel, k))
    acc, drt, amb, fluid, bound = ref["acc"], ref["drt"], ref["amb"], ref["fluid"], ref["bound"]
    assert fluid.sum() > 500 and bound.sum() > 3000
    ascale = np.abs(acc[fluid]).max()
    assert ascale > 50.0
    aerr = np.abs(f[fluid, :3] - acc[fluid]).max()
    dscale = np.abs(drt).max()
    assert dscale > 1.0
    err = np.abs(f[:, 3] - drt)
    print("%s: momentum %.3g of %.3g, continuity %.3g of %.3g, %d of %d pairs on the Colagrossi threshold"
          % (ka.kernel_id(kernel), aerr/ascale, ascale, (err - amb).max()/dscale, dscale, ref["ambiguous"], ref["pairs"]))
    assert aerr <= TOL*ascale
    nofb = bound & ((sim.info[:n, 0] & D.FG_COMPUTE_FORCE) == 0)
    assert nofb.sum() > 0 and not f[nofb, :3].any()
    assert (err <= TOL*dscale + amb*(1 + 1e-6)).all(), "drho/dt differs: %g of %g" % ((err - amb).max(), dscale)
    assert ref["ambiguous"] <= 0.01*ref["pairs"]
    tight = amb == 0.0
    assert tight.mean() > 0.9 and np.abs(f[tight, 3] - drt[tight]).max() <= TOL*dscale
    assert np.abs(drt[bound]).max() > 0.05*dscale


@kernels
def test_sps_tensor_and_divergence_per_kernel(kernel):
    prob, sim, gp, k = _state(kernel, "SPSVISC", 9)
    n = sim.n
    p = sim.o.p
    assert p.turbmodel == D.SPS
    smag, ksps = float(p.smagfactor), float(p.kspsfactor)
    tau, tv = sim.o.sps(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, n)
    ref, nu = ap.tau_all_pairs(sim, gp, k, smag, ksps, _F(kernel, k))
    scale = np.abs(ref).max(axis=0)
    assert (scale > 0).all() and np.abs(nu).max() > 0
    print("%s: tau %.3g of %.3g, turbulent viscosity %.3g" % (ka.kernel_id(kernel), np.abs(tau[:n] - ref).max()/scale.max(),
                                                             scale.max(), np.abs(tv[:n] - nu).max()/np.abs(nu).max()))
    assert (np.abs(tau[:n] - ref) <= TOL*scale.max()).all()
    assert np.abs(tv[:n] - nu).max() <= TOL*np.abs(nu).max()
    bound = (sim.info[:n, 0] & 7) == D.PT_BOUNDARY
    assert np.abs(ref[bound]).max() > 0.01*scale.max()
    # the divergence term of the forces, as tests/test_headline_allpairs.py isolates it: forces with tau minus forces without
    tau = (tau*np.float32(1000.0)).astype(np.float32)
    f_tau = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, tau=tau)[0][:n].astype(np.float64)
    f_0 = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, tau=np.zeros_like(tau))[0][:n].astype(np.float64)
    term = f_tau[:, :3] - f_0[:, :3]
    fluid = (sim.info[:n, 0] & 7) == D.PT_FLUID
    want = ap.sps_divergence(sim, gp, k, tau, _F(kernel, k))
    ts = np.abs(want).max()
    fs = np.abs(f_0[fluid, :3]).max()
    assert ts > 0.1*fs
    # a difference of two float32 accelerations: their rounding adds to the bound of the term
    assert np.abs(term[fluid] - want[fluid]).max() <= TOL*ts + 1e-6*fs


@kernels
def test_shepard_per_kernel(kernel):
    """self term included, the Gaussian's subtracted constant included (W64 carries it).  The field the filter sums is the DENSITY
    sum m W / sum (m / rho) W: the bar is taken of it, and rho~ = rho / rho0 - 1 is compared as the difference it is"""
    prob, sim, gp, k = _state(kernel)
    n = sim.n
    out = sim.o.filter(D.SHEPARD_FILTER, sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[:n, 3].astype(np.float64)
    ref = ap.shepard(sim, gp, k, _W(kernel, k))
    fluid = np.isfinite(ref)
    moved = np.abs(ref[fluid] - sim.vel[:n, 3][fluid]).max()
    assert fluid.sum() > 500 and moved > 1e-3           # the filter does something to this state
    err = np.abs(out[fluid] - ref[fluid]).max()
    print("%s: Shepard rho~ differs by %.3g (relative density: of 1; largest |rho~| %.3g)" % (ka.kernel_id(kernel), err, np.abs(ref[fluid]).max()))
    assert err <= TOL*(1.0 + np.abs(ref[fluid]).max())
    assert np.array_equal(out[~fluid], sim.vel[:n, 3][~fluid].astype(np.float64))       # the others keep theirs


@kernels
def test_xsph_mean_velocity_per_kernel(kernel):
    prob, sim, gp, k = _state(kernel)
    n = sim.n
    out = sim.o.xsph(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[:n, :3].astype(np.float64)
    ref = ap.xsph(sim, gp, k, _W(kernel, k))
    scale = np.abs(ref).max()
    assert scale > 0.05
    print("%s: XSPH %.3g of %.3g" % (ka.kernel_id(kernel), np.abs(out - ref).max()/scale, scale))
    assert np.abs(out - ref).max() <= TOL*scale


@kernels
def test_vorticity_per_kernel(kernel):
    prob, sim, gp, k = _state(kernel)
    n = sim.n
    out = sim.o.vorticity(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[:n].astype(np.float64)
    ref = ap.vorticity(sim, gp, k, _F(kernel, k))
    fluid = np.isfinite(ref[:, 0])
    assert np.isnan(out[~fluid]).all() and fluid.sum() > 500
    scale = np.abs(ref[fluid]).max()
    assert scale > 1.0
    print("%s: vorticity %.3g of %.3g" % (ka.kernel_id(kernel), np.abs(out[fluid] - ref[fluid]).max()/scale, scale))
    assert np.abs(out[fluid] - ref[fluid]).max() <= TOL*scale


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 values the device tests measure the Gaussian against (MLS, surface and interface detection, test points): held here
# against the oracle for all four kernels, on the states the device tests use

@kernels
def test_mls_per_kernel(kernel):
    sim, gp, k = ka.oracle_state(ka.problem(kernel, obstacle=True), 3, dv=0.1)
    n = sim.n
    out = sim.o.filter(D.MLS_FILTER, sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[:n, 3].astype(np.float64)
    ref, cond = ap.mls(sim, gp, k, _W(kernel, k))
    ok = np.isfinite(ref)
    fluid = (sim.info[:n, 0] & 7) == D.PT_FLUID
    assert ok[fluid].mean() > 0.99 and np.abs(ref[ok & fluid] - sim.vel[:n, 3][ok & fluid]).max() > 1e-4
    # the correction vector is a solve: the sums' rounding is multiplied by the moment matrix's condition number
    err = np.abs(out[ok & fluid] - ref[ok & fluid])
    print("%s: MLS rho~ differs by %.3g, largest condition number %.3g" % (ka.kernel_id(kernel), err.max(), cond[ok & fluid].max()))
    assert (err <= TOL*(1.0 + np.abs(ref[ok & fluid]))*np.maximum(1.0, cond[ok & fluid]/100.0)).all()


@kernels
def test_filters_on_two_fluids_per_kernel(kernel):
    """the state in which the constant the Gaussian W subtracts shows in the filters: neighbours of two rest densities"""
    sim, gp, k = ka.oracle_state(ka.problem(kernel, obstacle=True, two_fluids=True), 3, dv=0.1)
    n = sim.n
    fluid = (sim.info[:n, 0] & 7) == D.PT_FLUID
    W = _W(kernel, k)
    for ftype, ref in ((D.SHEPARD_FILTER, ap.shepard(sim, gp, k, W)), (D.MLS_FILTER, ap.mls(sim, gp, k, W)[0])):
        out = sim.o.filter(ftype, sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[:n, 3].astype(np.float64)
        assert np.isfinite(ref[fluid]).all()
        assert np.abs(out[fluid] - ref[fluid]).max() <= TOL*(1.0 + np.abs(ref[fluid]).max())
    if kernel == D.GAUSSIAN:      # without the subtracted constant: two hundred times the rounding away
        wsub = float(np.exp(-9.0))*ka._gaussian_wcoeff(k["h"])
        moved = np.abs(ap.shepard(sim, gp, k, lambda r: W(r) + wsub)[fluid] - ap.shepard(sim, gp, k, W)[fluid]).max()
        assert moved > 1e-4


@kernels
def test_surface_and_testpoints_per_kernel(kernel):
    sim, gp, k = ka.oracle_state(ka.problem(kernel, obstacle=True, testpoints=ka.TESTPOINTS), 9)
    n = sim.n
    W, F = _W(kernel, k), _F(kernel, k)
    info, nrm = sim.o.surface(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, normals=True)
    ref, margin, length = ap.surface(sim, gp, k, W, F)
    fluid = np.isfinite(margin)
    flag = (info[:n, 0] & D.FG_SURFACE) != 0
    near = ka.near_threshold(margin)
    assert flag.sum() > 10 and near.sum() < 0.01*flag.sum()
    assert np.array_equal(flag[fluid & ~near], (margin <= 0)[fluid & ~near])
    # the pair sum is the normal BEFORE it is normalised (it nearly cancels inside the fluid): the unit normal's error, times that length
    err = (np.abs(nrm[:n][fluid].astype(np.float64) - ref[fluid])*np.c_[length, length, length, length*0 + 1][fluid]).max(axis=0)
    print("%s: surface normal differs by %.3g, Shepard sum by %.3g; %d flagged, %d on the threshold"
          % (ka.kernel_id(kernel), err[:3].max(), err[3], flag.sum(), near.sum()))
    assert err[:3].max() <= TOL*length[fluid].max() and err[3] <= TOL*np.abs(ref[fluid, 3]).max()
    tp, want = ap.testpoints(sim, gp, k, W)
    got = sim.o.testpoints(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)[:n][tp].astype(np.float64)
    assert len(tp) == 3 and (np.abs(want).max(axis=0) > 0).all()
    assert np.abs(got[:, :3] - want[:, :3]).max() <= TOL*np.abs(want[:, :3]).max()
    assert np.abs(got[:, 3] - want[:, 3]).max() <= TOL*np.abs(want[:, 3]).max()


@kernels
def test_interface_per_kernel(kernel):
    sim, gp, k = ka.oracle_state(ka.problem(kernel, obstacle=True, two_fluids=True), 10)
    n = sim.n
    info, nrm = sim.o.interface(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, normals=True)
    ref, mfs, mif, length = ap.interface(sim, gp, k, _W(kernel, k), _F(kernel, k))
    fluid = np.isfinite(mfs)
    surf, intf = (info[:n, 0] & D.FG_SURFACE) != 0, (info[:n, 0] & D.FG_INTERFACE) != 0
    near = ka.near_threshold(mfs) | ka.near_threshold(mif)
    assert surf.sum() > 10 and intf.sum() > 10 and near.sum() < 0.01*(surf.sum() + intf.sum())
    sure = fluid & ~near
    assert np.array_equal(surf[sure], (mfs <= 0)[sure]) and np.array_equal(intf[sure], ((mif <= 0) & (mfs > 0))[sure])
    err = (np.abs(nrm[:n][sure].astype(np.float64) - ref[sure])*np.c_[length, length, length, length*0 + 1][sure]).max(axis=0)
    print("%s: interface normal differs by %.3g, Shepard sum by %.3g; %d + %d flagged, %d on a threshold"
          % (ka.kernel_id(kernel), err[:3].max(), err[3], surf.sum(), intf.sum(), near.sum()))
    assert err[:3].max() <= TOL*length[sure].max() and err[3] <= TOL*np.abs(ref[sure, 3]).max()
