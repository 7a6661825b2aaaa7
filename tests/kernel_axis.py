"""The kernel-function axis (cubic spline, quadratic, Wendland, Gaussian) for tests/test_kernel_axis_allpairs.py (CPU) and
tests/test_gpu_kernel_axis.py (device).  TEST INFRASTRUCTURE, no GPU.

  problem(kernel, **opts)   the DamBreak3D every case of the axis is made from.  The Gaussian's radius is 3 h: at the default
                            smoothing factor 1.3 its lists (about 250 neighbours) overflow the 128 entries of a tile section and every
                            pass is the generic kernels' (tests/tiling_overflow_cases.py).  Here it is built with a smoothing factor
                            of 1.0 -- the NARROW Gaussian, whose tiling fits (test_kernel_axis_allpairs.py proves it per option set)
  W64 / F64                 the kernel and (1/r) dW/dr in float64, written from the reference's formulas (src/cuda/sph_core.cu:66-215)
                            and coefficients (src/cuda/forces.cu:274-309).  They share no code with oracle/sph_oracle.c or
                            gpusph_amd/params.py: that is their point."""
import math

import numpy as np

from gpusph_amd import defs as D
from gpusph_amd.problem import DamBreak3D

import tiling_overflow_cases as toc

KERNELS = [D.CUBICSPLINE, D.QUADRATIC, D.WENDLAND, D.GAUSSIAN]
KERNEL_NAMES = {D.CUBICSPLINE: "cubicspline", D.QUADRATIC: "quadratic", D.WENDLAND: "wendland", D.GAUSSIAN: "gaussian"}
NARROW_SFACTOR = 1.0
DELTAP = 0.05


def kernel_id(k):
    return KERNEL_NAMES[k]


def problem(kernel, near_body=False, **opts):
    """near_body: the feedback body stands next to the water column (its face 0.05 from the column's), within the kernel radius of
    the fluid.  Where DamBreak3D places it, half a metre downstream, its rows carry no force in the initial state at all"""
    cls = toc.wide(DamBreak3D, NARROW_SFACTOR) if kernel == D.GAUSSIAN else DamBreak3D
    if near_body:
        class NearBody(cls):
            OBSTACLE_XPOS = DamBreak3D.WATER_LENGTH + 0.05
        cls = NearBody
    return cls(DELTAP, jitter=0.1, hydrostatic=False, kerneltype=kernel, **opts)


# the option sets of the forces matrix (tests/test_gpu_kernel_axis.py); test_kernel_axis_allpairs.py proves for each that the narrow
# Gaussian's tiling fits.  name -> (constructor options, tiled: does sphx_tiles_opts_forces send a NON-Wendland pass to the tiles)
OPTION_SETS = {
    "artvisc-colagrossi-dyn-body": (dict(obstacle=True, near_body=True), True),
    "lj-body-no-diffusion": (dict(obstacle=True, near_body=True, boundary=D.LJ_BOUNDARY, density_diffusion=D.DENSITY_DIFFUSION_NONE), True),
    "mk": (dict(obstacle=True, boundary=D.MK_BOUNDARY), True),
    "dynamicvisc-no-diffusion": (dict(obstacle=True, viscosity="DYNAMICVISC", kinematic_visc=3e-2,
                                      density_diffusion=D.DENSITY_DIFFUSION_NONE), True),
    "spsvisc": (dict(obstacle=True, viscosity="SPSVISC"), True),
    "sps-alone": (dict(obstacle=True, sps_alone=True), True),
    "two-fluids-colagrossi": (dict(obstacle=False, two_fluids=True), False),
    "ferrari": (dict(obstacle=True, density_diffusion=D.FERRARI), False),
    "xsph": (dict(obstacle=True, xsph=True), True),
}


def option_problem(kernel, name):
    opts = dict(OPTION_SETS[name][0])
    sps_alone, xsph = opts.pop("sps_alone", False), opts.pop("xsph", False)
    prob = problem(kernel, **opts)
    if sps_alone:      # turbulence<SPS> on the inviscid fluid: the SPS term alone, with the factors GPUSPH.cc:1540-1556 derives
        prob.simparams.turbmodel = D.SPS
        dp = prob.m_deltap
        prob.physparams.smagfactor = float(np.float32((0.12*dp)**2))
        prob.physparams.kspsfactor = float(np.float32((2.0/3.0)*0.0066*dp*dp))
    if xsph:
        prob.simparams.simflags |= D.ENABLE_XSPH
    return prob


def radius(kernel):
    """the kernel's radius in units of h"""
    return 3.0 if kernel == D.GAUSSIAN else 2.0


def _gaussian_wcoeff(h):
    R = radius(D.GAUSSIAN)
    return 1.0/(h**3*(math.pi**1.5*math.erf(R) - (2.0/3.0)*math.exp(-R*R)*math.pi*R*(3.0 + 2.0*R*R)))


def W64(kernel, r, h):
    """W(r, h) in float64; r an array (or scalar) of distances within the kernel's radius"""
    r = np.asarray(r, dtype=np.float64)
    h = float(h)
    q = r/h
    if kernel == D.CUBICSPLINE:
        return np.where(q < 1.0, 1.0 - 1.5*q*q + 0.75*q*q*q, 0.25*(2.0 - q)**3)/(math.pi*h**3)
    if kernel == D.QUADRATIC:
        return (0.25*q*q - q + 1.0)*15.0/(16.0*math.pi*h**3)
    if kernel == D.WENDLAND:
        return (1.0 - 0.5*q)**4*(1.0 + 2.0*q)*21.0/(16.0*math.pi*h**3)
    if kernel == D.GAUSSIAN:
        return (np.exp(-q*q) - math.exp(-radius(kernel)**2))*_gaussian_wcoeff(h)
    raise ValueError(kernel)


def F64(kernel, r, h):
    """(1/r) dW/dr in float64"""
    r = np.asarray(r, dtype=np.float64)
    h = float(h)
    q = r/h
    if kernel == D.CUBICSPLINE:
        with np.errstate(divide="ignore", invalid="ignore"):
            outer = -(q - 2.0)**2/r
        return np.where(q < 1.0, (3.0*q - 4.0)/h, outer)*3.0/(4.0*math.pi*h**4)
    if kernel == D.QUADRATIC:
        return (q - 2.0)/r*15.0/(32.0*math.pi*h**4)
    if kernel == D.WENDLAND:
        return (q - 2.0)**3*105.0/(128.0*math.pi*h**5)
    if kernel == D.GAUSSIAN:
        return -np.exp(-q*q)*_gaussian_wcoeff(h)*2.0/(h*h)
    raise ValueError(kernel)


TESTPOINTS = [(0.2, 0.3, 0.2), (0.25, 0.35, 0.1), (1.2, 0.3, 0.3)]


def oracle_state(prob, seed, dv=0.4):
    """the oracle driver of `prob` after its list build, every velocity moved by up to dv and every rho~ raised by up to 2e-3 (the
    state of test_postprocess_bit_exact) -> (sim, global float64 positions, allpairs_ref.consts)"""
    import allpairs_ref as ap
    import oracle_lib as ol
    sim = ol.OracleSim(prob)
    sim.build_neibs()
    assert sim.neibs_info.hasTooManyNeibs == -1
    rng = np.random.default_rng(seed)
    vel = sim.vel.copy()
    vel[:, :3] += rng.uniform(-dv, dv, size=(len(vel), 3)).astype(np.float32)
    vel[:, 3] += rng.uniform(0, 2e-3, size=len(vel)).astype(np.float32)
    sim.vel = vel
    n = sim.n
    return sim, prob.global_pos(sim.pos[:n], sim.hash[:n]), ap.consts(sim)


def near_threshold(margin, tol=1e-5):
    """particles whose cone test (allpairs_ref._cone_margin) lies within tol of its threshold: their flag is the rounding's to decide"""
    return np.isfinite(margin) & (np.abs(margin) <= tol)
