"""Host-side kinematics of moving bodies with prescribed motion: the part of ProblemCore::bodies_timestep
(src/ProblemCore.cc:484-610) that does not need the Chrono rigid-body solver (MB_MOVING and MB_FORCES_MOVING bodies).

Per integrator step the problem's `moving_bodies_callback(index, t0, t1, initial_kdata, kdata)` advances the body's
kinematic data from t0 to t1 and returns the translation `dx` (3) and the rotation matrix `dr` (3x3) of that interval;
the engines then receive, per body: translation, step rotation, linear and angular velocity, and the centre of rotation as
grid cell + cell-local position (calc_grid_and_local_pos).  On the predictor the interval is [t, t + dt/2] and the
kinematic data of time t are saved; on the corrector they are restored and the interval is [t, t + dt].

Floating bodies (MB_FLOATING) are described here (FloatingBody) and integrated on the device (csrc/floating.hip): they take the
body indices ahead of every other body, and MovingBodies leaves their rows of the tables alone (`first`)."""
import copy
from dataclasses import dataclass, field

import numpy as np


@dataclass
class KinematicData:
    """src/Object.h KinematicData subset: centre of rotation (global, double), linear and angular velocity"""
    crot: np.ndarray = field(default_factory=lambda: np.zeros(3))
    lvel: np.ndarray = field(default_factory=lambda: np.zeros(3))
    avel: np.ndarray = field(default_factory=lambda: np.zeros(3))


@dataclass
class FloatingBody:
    """What the device needs of a body that floats: mass, principal inertia (body axes), centre of rotation (global), orientation
    (unit quaternion w, x, y, z: body axes -> world axes), linear and angular velocity (world frame)"""
    mass: float = 1.0
    inertia: np.ndarray = field(default_factory=lambda: np.ones(3))
    crot: np.ndarray = field(default_factory=lambda: np.zeros(3))
    orientation: np.ndarray = field(default_factory=lambda: np.array([1.0, 0.0, 0.0, 0.0]))
    lvel: np.ndarray = field(default_factory=lambda: np.zeros(3))
    avel: np.ndarray = field(default_factory=lambda: np.zeros(3))

    def set_mass_by_density(self, density, volume):
        """Object::SetMass(dx, rho) through ProblemAPI<1>::setMassByDensity: mass = density * volume; the inertia scales with it"""
        m = float(density) * float(volume)
        self.inertia = np.asarray(self.inertia, dtype=np.float64) * (m / self.mass)
        self.mass = m
        return self


def box_inertia(mass, sides):
    """principal inertia of a homogeneous box about its centre (Cube::SetInertia, src/geometries/Cube.cc)"""
    lx, ly, lz = (float(v) for v in sides)
    return mass / 12.0 * np.array([ly * ly + lz * lz, lx * lx + lz * lz, lx * lx + ly * ly])


def sphere_inertia(mass, radius):
    """principal inertia of a homogeneous sphere (Sphere::SetInertia, src/geometries/Sphere.cc)"""
    return np.full(3, 0.4 * float(mass) * float(radius) ** 2)


class MovingBodies:
    def __init__(self, problem, centres, first=0):
        """`first`: bodies 0 .. first-1 float (the device moves them); the callback is asked about bodies first .. n-1 only and the
        rows of the floating bodies in what timestep() returns are never uploaded over the device's (sphx_floating_setup)"""
        self.problem = problem
        self.first = int(first)
        self.initial = [KinematicData(crot=np.array(c, dtype=np.float64)) for c in centres]
        self.kdata = copy.deepcopy(self.initial)
        self.storage = copy.deepcopy(self.initial)

    def __len__(self):
        return len(self.kdata)

    def grid_and_local(self, x):
        p = self.problem
        g = np.clip(np.floor((x - p.m_origin) / p.m_cellsize).astype(np.int64), 0, p.m_gridsize - 1)
        return g.astype(np.int32), (x - p.m_origin - (g + 0.5) * p.m_cellsize).astype(np.float32)

    def timestep(self, step, dt, t):
        """returns dict(trans (n,3) f32, rot (n,9) f32, lvel, avel, cg_grid (n,3) i32, cg_pos (n,3) f32)"""
        dt1 = dt / 2.0 if step == 1 else dt
        n = len(self)
        out = dict(trans=np.zeros((n, 3), np.float32), rot=np.zeros((n, 9), np.float32), lvel=np.zeros((n, 3), np.float32),
                   avel=np.zeros((n, 3), np.float32), cg_grid=np.zeros((n, 3), np.int32), cg_pos=np.zeros((n, 3), np.float32))
        for i in range(self.first, n):
            if step == 1:
                self.storage[i] = copy.deepcopy(self.kdata[i])
            else:
                self.kdata[i] = copy.deepcopy(self.storage[i])
            kd = self.kdata[i]
            dx, dr = self.problem.moving_bodies_callback(i, t, t + dt1, self.initial[i], kd)
            out["trans"][i] = np.asarray(dx, dtype=np.float64)
            out["rot"][i] = np.asarray(dr, dtype=np.float64).reshape(9)
            out["lvel"][i] = kd.lvel; out["avel"][i] = kd.avel
            out["cg_grid"][i], out["cg_pos"][i] = self.grid_and_local(kd.crot)
        return out
