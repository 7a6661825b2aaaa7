"""The rule floating bodies are integrated by (tests/floating_ref.py, the float64 restatement the kernels of csrc/floating.hip are
held to) against closed forms of its own discrete map, each to 1e-12 relative, and one whole run of the oracle with a floating
cube (BuoyancyBox).  Without the feature neither BuoyancyBox nor Problem.floating_bodies exists."""
import math

import numpy as np
import pytest

import floating_ref as fr
from gpusph_amd import defs as D
from gpusph_amd.bodies import FloatingBody, box_inertia, sphere_inertia
from gpusph_amd.problem import BuoyancyBox

REL = 1e-12
GRID = dict(origin=np.zeros(3), cellsize=np.full(3, 0.25), gridsize=np.array([8, 8, 8]), gravity=np.array([0.0, 0.0, -9.81]))
NOG = dict(GRID, gravity=np.zeros(3))
DT = float(np.float32(3.0e-4))


def _close(a, b, scale=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-300) if scale is None else scale
    assert np.abs(a - b).max() <= REL*scale, (a, b)


def _step(bodies, F=(0, 0, 0), T=(0, 0, 0), dt=DT):
    """one whole step with constant totals: the predictor's result is thrown away by the corrector"""
    tot = np.array([list(F) + list(T)]*len(bodies), dtype=np.float64)
    bodies.substep(1, tot, dt)
    return bodies.substep(2, tot, dt)


def test_free_fall_from_rest():
    # (x0 = 0: the closed form is then held relative to the distance fallen, not to where the body started)
    b = fr.RefBodies([FloatingBody(mass=3.0, inertia=np.array([1.0, 2.0, 3.0]))], GRID)
    g = GRID["gravity"]
    for n in range(1, 41):
        _step(b)
        _close(b.state[0, 7:10], n*DT*g)
        _close(b.state[0, 0:3], DT*DT*g*n*(n + 1)/2)
    assert np.array_equal(b.state[0, 3:7], [1.0, 0.0, 0.0, 0.0]) and not b.state[0, 10:13].any()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_constant_torque_about_a_principal_axis(axis):
    I = np.array([0.7, 1.1, 1.9])
    T = np.zeros(3); T[axis] = 2.5
    b = fr.RefBodies([FloatingBody(mass=1.0, inertia=I)], NOG)
    angle = 0.0
    for n in range(1, 31):
        _step(b, T=T)
        w = n*DT*T[axis]/I[axis]
        angle += DT*w                                      # the matching sum: every step turns by dt times the NEW rate
        _close(b.state[0, 10 + axis], w)
        q = b.state[0, 3:7]
        want = np.zeros(4); want[0] = math.cos(angle/2); want[1 + axis] = math.sin(angle/2)
        _close(q, want, scale=1.0)
        assert abs(2.0*math.atan2(q[1 + axis], q[0]) - angle) <= REL*max(angle, 1.0)


def test_torque_free_symmetric_top():
    """explicit Euler on Euler's equations: w3 stays, the transverse rate grows by (1 + (W dt)^2)^(1/2) per step"""
    I1, I3, w3 = 0.8, 1.7, 5.0
    W = (I3 - I1)*w3/I1
    b = fr.RefBodies([FloatingBody(mass=1.0, inertia=np.array([I1, I1, I3]), avel=np.array([0.3, -0.2, w3]))], NOG)
    wt0 = math.hypot(0.3, 0.2)
    for n in range(1, 41):
        _step(b)
        wb = fr.rotmat(b.state[0, 3:7]).T @ b.state[0, 10:13]
        _close(wb[2], w3)
        _close(math.hypot(wb[0], wb[1]), wt0*(1.0 + (W*DT)**2)**(n/2))
    assert (1.0 + (W*DT)**2)**20 - 1.0 > 1e3*REL              # the growth is far above the bound: a wrong sign or a missing 1/I shows
    for wrong in ((I1 - I3)*w3/I3, (I3 - I1)*w3):             # ... in the rate the closed form is made of
        assert abs((1.0 + (wrong*DT)**2)**20 - (1.0 + (W*DT)**2)**20) > 1e3*REL


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_spin_about_a_principal_axis_never_changes(axis):
    w = np.zeros(3); w[axis] = 7.0
    b = fr.RefBodies([FloatingBody(mass=1.0, inertia=np.array([0.7, 1.1, 1.9]), avel=w)], NOG)
    for _ in range(30):
        _step(b)
        assert np.array_equal(b.state[0, 10:13], w)


def test_unit_quaternion_and_orthonormal_step_rotation():
    rng = np.random.default_rng(5)
    q0 = rng.normal(size=4); q0 /= np.linalg.norm(q0)
    b = fr.RefBodies([FloatingBody(mass=2.0, inertia=np.array([0.5, 0.9, 1.3]), orientation=q0, avel=np.array([3.0, -8.0, 5.0]))], GRID)
    for _ in range(50):
        s = _step(b, F=rng.normal(size=3)*50, T=rng.normal(size=3)*20)
        q = b.state[0, 3:7]
        assert abs(float(q @ q) - 1.0) <= 4*2.0**-52
        R = s["rot"][0].reshape(3, 3).astype(np.float64)
        # nine floats rounded from an orthonormal matrix (each off by at most 2^-25): an entry of R R^T is off by at most
        # 2 sqrt(3) 2^-25 < 2 2^-24 in the first order; 6 2^-24 leaves room for the second
        assert np.abs(R @ R.T - np.eye(3)).max() <= 6*2.0**-24
        assert abs(np.linalg.det(R) - 1.0) <= 12*2.0**-24


def test_the_corrector_starts_from_the_saved_state():
    mk = lambda: fr.RefBodies([FloatingBody(mass=2.0, inertia=np.array([0.5, 0.9, 1.3]), crot=np.array([1.0, 1.0, 1.0]),
                                            lvel=np.array([0.1, 0.0, 0.2]), avel=np.array([1.0, 2.0, -1.0]))], GRID)
    a, b = mk(), mk()
    good = np.array([[3.0, -2.0, 40.0, 0.5, 0.25, -1.0]])
    a.substep(1, good, DT); a.substep(2, good, DT)
    b.substep(1, np.array([[1e30, -1e30, 1e25, 1e28, 1e28, -1e29]]), DT)
    assert np.abs(b.state[0, :fr.KEPT]).max() > 1e20
    b.substep(2, good, DT)
    assert np.array_equal(a.state.view(np.uint64), b.state.view(np.uint64))


def test_inertia_helpers_and_mass_by_density():
    m = 0.5*1000.0*0.4**3
    assert np.allclose(box_inertia(m, (0.4, 0.4, 0.4)), m*0.16/6.0, rtol=1e-15)
    assert np.allclose(box_inertia(12.0, (1.0, 2.0, 3.0)), [13.0, 10.0, 5.0], rtol=1e-15)
    assert np.allclose(sphere_inertia(5.0, 0.3), 0.4*5.0*0.09, rtol=1e-15)
    fb = FloatingBody(mass=2.0, inertia=box_inertia(2.0, (1.0, 1.0, 1.0))).set_mass_by_density(500.0, 1.0)
    assert fb.mass == 500.0 and np.allclose(fb.inertia, box_inertia(500.0, (1.0, 1.0, 1.0)), rtol=1e-15)


# ---- the whole run
@pytest.fixture(scope="module")
def run():
    pr = BuoyancyBox(deltap=0.05)
    sim = fr.FloatingOracleSim(pr)
    z = [sim.fl.state[0, 2]]
    for _ in range(12):
        sim.step()
        z.append(sim.fl.state[0, 2])
    return pr, sim, np.array(z)


def test_buoyancy_box_is_the_reference_problem():
    pr = BuoyancyBox(deltap=0.05)
    sp = pr.simparams
    assert (sp.kerneltype, sp.boundarytype, sp.rheologytype, sp.turbmodel) == (D.WENDLAND, D.DYN_BOUNDARY, D.INVISCID, D.ARTIFICIAL)
    assert sp.numbodies == 1 and sp.numforcesbodies == 1 and len(pr.floating_bodies) == 1
    fb = pr.floating_bodies[0]
    assert abs(fb.mass - 0.5*1000.0*0.4**3) < 1e-12 and np.array_equal(fb.crot, [0.5, 0.5, 0.3])
    info, g = pr.parts.info, pr.parts.pos_global
    body = (info[:, 0] & (D.FG_MOVING_BOUNDARY | D.FG_COMPUTE_FORCE)) == (D.FG_MOVING_BOUNDARY | D.FG_COMPUTE_FORCE)
    assert body.sum() == pr.num_obstacle == 9**3 - 3**3 and ((info[body, 0] & 7) == D.PT_BOUNDARY).all()
    assert 15000 <= len(info) <= 25000
    assert np.allclose(g[body, :3].mean(axis=0), [0.5, 0.5, 0.3], atol=1e-12)
    assert np.allclose(g[:, 3], 1000.0*pr.m_deltap**3)
    fluid = (info[:, 0] & 7) == D.PT_FLUID
    d = np.abs(g[fluid, :3] - np.array([0.5, 0.5, 0.3])).max(axis=1)
    assert d.min() >= 0.2 + 0.5*pr.dx - 1e-12 and g[fluid, 2].max() <= 0.6 + 1e-12
    ids = info[:, 2].astype(np.int64) | (info[:, 3].astype(np.int64) << 16)
    rows = ids[body] + int(pr.rb_firstindex[0])
    assert np.array_equal(np.sort(rows), np.arange(pr.num_obstacle)) and list(pr.rb_rowstart) == [0, pr.num_obstacle]
    empty = BuoyancyBox(deltap=0.05, fluid=False)
    assert empty.num_fluid == 0 and empty.num_obstacle == pr.num_obstacle
    both = BuoyancyBox(deltap=0.05, paddle=True)
    assert both.simparams.numbodies == 2 and both.num_paddle > 0 and both.moving_bodies_callback is not None
    pad = (both.parts.info[:, 0] & (D.FG_MOVING_BOUNDARY | D.FG_COMPUTE_FORCE)) == D.FG_MOVING_BOUNDARY
    assert pad.sum() == both.num_paddle and (both.parts.info[pad, 1] == 1).all() and (both.parts.pos_global[pad, 0] < 0).all()
    lj = BuoyancyBox(deltap=0.05, boundary=D.LJ_BOUNDARY)
    assert lj.layers == 1 and lj.num_obstacle == 9**3 - 7**3


def test_the_cube_is_pushed_up_across_a_rebuild(run):
    pr, sim, z = run
    assert sim.iterations == 12 and pr.simparams.buildneibsfreq == 10           # the lists were rebuilt at iteration 10
    rho0, g, side = 1000.0, 9.81, pr.SIDE
    first = sim.totals[0][0]
    ratio = first[2]/(rho0*g*side**3)
    print("net vertical fluid force on the cube at the first pass / (rho0 g side^3) = %.4f" % ratio)
    # a condition that catches a wrong sign, arm or mass, not a statement of SPH accuracy
    assert 0.5 <= ratio <= 2.0
    assert np.abs(first[[0, 1]]).max() <= 1e-3*abs(first[2])                     # the lattice is symmetric in x and y
    # half the density of water: the net acceleration of the first pass is upward, and every one of the steps lifts the cube
    # (how the rate changes over these 3.6 ms is the pressure wave's business: nothing is asserted about it)
    v = sim.fl.state[0, 9]
    assert first[2]/pr.floating_bodies[0].mass - g > 0
    assert v > 0 and (np.diff(z) > 0).all()
    assert np.isfinite(sim.pos).all() and np.isfinite(sim.vel).all()
    # the body's particles moved with it: their mean position is the centre of rotation (no rotation to speak of)
    body = (sim.info[:sim.n, 0] & D.FG_COMPUTE_FORCE) != 0
    gp = pr.global_pos(sim.pos[:sim.n][body], sim.hash[:sim.n][body])
    assert np.abs(gp.mean(axis=0) - sim.fl.state[0, 0:3]).max() <= 1e-6
