"""Float64 restatement of the effective-pressure solver of the GRANULAR rheology and of its viscosity, for the tests of
gpusph_amd/csrc/granular.hip: all pairs within the influence radius instead of a neighbour list, dense numpy arrays, in the
manner of tests/test_headline_allpairs.py.  What is restated (paths in the GPUSPH tree):
  the four passes     jacobiFSBoundaryConditionsDevice, jacobiWallBoundaryConditionsDevice, jacobiBuildVectorsDevice,
                      jacobiUpdateEffPresDevice        src/cuda/visc_kernel.cu:813-1101
  the host loop       preparation, then build / update / wall pass / stop test
                      src/integrators/PredictorCorrectorIntegrator.cc:1046-1182, src/GPUSPH.cc:2295-2320
  the viscosity       viscShearTerm / clamp_visc<GRANULAR> behind the shear rate norm of effectiveViscDevice
                      src/cuda/visc_kernel.cu:529-579,655-708
Meant for a few thousand particles (the pair arrays are n x n).
"""
import math
import numpy as np

from gpusph_amd import defs as D


def _kernel(kerneltype, r, h):
    """W(r, h) and F(r, h) = (1/r) dW/dr (src/cuda/sph_core.cu:66-215) in float64; the Gaussian is left out (its coefficient
    depends on the truncation radius)"""
    R = r / h
    with np.errstate(divide="ignore", invalid="ignore"):
        if kerneltype == D.WENDLAND:
            W = (1 - 0.5 * R) ** 4 * (1 + 2 * R) * 21.0 / (16.0 * math.pi * h ** 3)
            F = (R - 2.0) ** 3 * 105.0 / (128.0 * math.pi * h ** 5)
        elif kerneltype == D.CUBICSPLINE:
            W = np.where(R < 1, 1 - 1.5 * R * R + 0.75 * R ** 3, 0.25 * (2 - R) ** 3) / (math.pi * h ** 3)
            F = np.where(R < 1, (-4 + 3 * R) / h, -(-2 + R) ** 2 / r) * 3.0 / (4.0 * math.pi * h ** 4)
        elif kerneltype == D.QUADRATIC:
            W = (0.25 * R * R - R + 1) * 15.0 / (16.0 * math.pi * h ** 3)
            F = (-2 + R) / r * 15.0 / (32.0 * math.pi * h ** 4)
        else:
            raise ValueError("kernel type not restated")
    return W, F


class GranularRef:
    """One state (positions, densities, flags) of a problem with the GRANULAR rheology.  `pos` are the cell-local float32 rows
    with their hashes as the device holds them; everything after that is float64."""

    def __init__(self, problem, pos, hashes, vel, info):
        sp, pp = problem.simparams, problem.physparams
        pp.update_visccoeff(sp)                                 # d_visccoeff, as make_sphx_params leaves it
        n = len(pos)
        self.n = n
        X = problem.global_pos(np.asarray(pos, dtype=np.float32), np.asarray(hashes))
        mass = np.asarray(pos, dtype=np.float32)[:, 3].astype(np.float64)
        self.active = np.isfinite(mass)
        d = X[:, None, :] - X[None, :, :]                       # r_ij = x_i - x_j
        for a, flag in enumerate((D.PERIODIC_X, D.PERIODIC_Y, D.PERIODIC_Z)):
            if sp.periodicbound & flag:
                L = float(problem.m_size[a])
                d[:, :, a] -= L * np.round(d[:, :, a] / L)
        self.d = d
        r = np.sqrt((d * d).sum(axis=2))
        self.h = float(np.float32(sp.slength))
        self.radius = float(np.float32(sp.influenceRadius))
        self.near = (r < self.radius) & ~np.eye(n, dtype=bool) & self.active[:, None] & self.active[None, :]
        flags = np.asarray(info).reshape(n, 4)[:, 0].astype(np.int64)
        self.fluid_num = (np.asarray(info).reshape(n, 4)[:, 1].astype(np.int64)) >> 12
        ptype = flags & 7
        self.is_fluid = ptype == D.PT_FLUID
        self.is_wall = (ptype == D.PT_BOUNDARY) & self.active
        sed = (flags & D.FG_SEDIMENT) != 0
        marked = (flags & (D.FG_SURFACE | D.FG_INTERFACE)) != 0
        self.sed_fluid = self.is_fluid & sed
        self.dirichlet = self.sed_fluid & marked & self.active
        self.interior_type = self.sed_fluid & ~marked           # by flags alone: how a NEIGHBOUR is sorted into Rx or B
        self.interior = self.interior_type & self.active        # the rows that are solved
        rho0 = np.array([float(np.float32(x)) for x in pp.rho0])
        self.rho0 = rho0
        self.c0 = np.array([float(np.float32(x)) for x in pp.sscoeff])
        self.rho = (np.asarray(vel, dtype=np.float32)[:, 3].astype(np.float64) + 1.0) * rho0[self.fluid_num]
        with np.errstate(invalid="ignore"):
            self.V = mass / self.rho
        W, F = _kernel(sp.kerneltype, r, self.h)
        V_j = np.where(self.active, self.V, 0.0)[None, :]
        self.VW = np.where(self.near, V_j * W, 0.0)
        self.VF = np.where(self.near, V_j * F, 0.0)
        self.g = np.array([float(np.float32(x)) for x in pp.gravity])
        self.delta_rho = rho0[0] if len(rho0) == 1 else abs(rho0[0] - rho0[1])
        self.deltap = float(np.float32(problem.m_deltap))
        self.refpres_wall = self.delta_rho * (self.c0[0] / 10.0) ** 2
        self.refpres_row = rho0[self.fluid_num] * self.c0[self.fluid_num] ** 2 / 100.0
        self.maxiter, self.backerr_max, self.residual_max = int(sp.jacobi_maxiter), float(np.float32(sp.jacobi_backerr)), float(np.float32(sp.jacobi_residual))
        # the pair coefficients of the two sums, masked once
        contributes = self.sed_fluid | (ptype == D.PT_BOUNDARY)
        self.C = np.where(self.interior[:, None] & contributes[None, :], self.VF, 0.0)
        self.C_rx = np.where(self.interior_type[None, :], self.C, 0.0)
        self.C_b = self.C - self.C_rx
        self.A = np.where(self.is_wall[:, None] & self.sed_fluid[None, :], self.VW, 0.0)
        self.Bw = self.delta_rho * (d @ self.g)                 # delta_rho g . r_ij
        self.pp, self.sp = pp, sp
        self.vel3 = np.asarray(vel, dtype=np.float32)[:, :3].astype(np.float64)

    # ---- the four passes; each returns a new pressure array (and what the pass reports)
    def fs_boundary_conditions(self, p):
        q = np.array(p, dtype=np.float64)
        q[self.dirichlet] = self.deltap * self.delta_rho * math.sqrt(float(self.g @ self.g))
        return q

    def wall_boundary_conditions(self, p):
        p = np.asarray(p, dtype=np.float64)
        rows = np.flatnonzero(self.is_wall)
        A = self.A[rows]
        num = np.maximum(A * (p[None, :] + self.Bw[rows]), 0.0).sum(axis=1)
        alpha = A.sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            new = np.where(alpha > 0, num / alpha, 0.0)
        err = np.where(alpha > 0, np.abs(new - p[rows]) / self.refpres_wall, 0.0)
        q = p.copy()
        q[rows] = new
        return q, float(err.max()) if len(rows) else 0.0

    def build_vectors(self, p):
        """(D, Rx, B) per row; zero on the rows that are not solved"""
        p = np.where(np.isfinite(p), np.asarray(p, dtype=np.float64), 0.0)
        return self.C.sum(axis=1), -(self.C_rx @ p), self.C_b @ p

    def update_effpres(self, p, Dv, Rx, B):
        rows = self.interior
        with np.errstate(divide="ignore", invalid="ignore"):
            new = (B - Rx) / Dv
            res = (Dv * new + Rx - B) / self.refpres_row
        q = np.array(p, dtype=np.float64)
        q[rows] = np.where(np.isnan(new[rows]), 0.0, new[rows])
        res = res[rows]
        res = res[~np.isnan(res)]
        return q, float(max(res.max(), 0.0)) if len(res) else 0.0

    def sweep(self, p):
        """one iteration of the loop: build, update, wall pass -> (pressures, backward error, residual)"""
        Dv, Rx, B = self.build_vectors(p)
        q, res = self.update_effpres(p, Dv, Rx, B)
        q, err = self.wall_boundary_conditions(q)
        return q, err, res

    def solve(self, p, maxiter=None, backerr=None, residual=None):
        """the host loop -> (pressures, h_jacobiCounter, backward error, residual) when the stop test fires"""
        maxiter = self.maxiter if maxiter is None else maxiter
        backerr = self.backerr_max if backerr is None else backerr
        residual = self.residual_max if residual is None else residual
        q = self.fs_boundary_conditions(p)
        q, _ = self.wall_boundary_conditions(q)
        counter = 0
        while True:
            q, err, res = self.sweep(q)
            if (err < backerr and res < residual) or counter > maxiter:
                return q, counter, err, res
            counter += 1

    # ---- the viscosity
    def shear_rate_norm(self):
        """S of effectiveViscDevice: the MIXED_TENSOR velocity gradient over every neighbour (fluid and boundary)"""
        w = self.VF                                              # V_j F_ij, zero beyond reach and for disabled particles
        dv = self.vel3[:, None, :] - self.vel3[None, :, :]
        grad = -np.einsum("ija,ijb,ij->iab", dv, self.d, w)      # grad[i][a][b] = -sum_j v_ij[a] r_ij[b] w_ij
        txx, tyy, tzz = grad[:, 0, 0], grad[:, 1, 1], grad[:, 2, 2]
        txy, txz, tyz = grad[:, 0, 1] + grad[:, 1, 0], grad[:, 0, 2] + grad[:, 2, 0], grad[:, 1, 2] + grad[:, 2, 1]
        return np.sqrt(2.0 * (txx * txx + tyy * tyy + tzz * tzz) + txy * txy + txz * txz + tyz * tyz)

    def effective_visc(self, effpres, old, S=None):
        """BUFFER_EFFVISC (KINEMATIC: mu_eff / rho) from `old`: non-fluid and disabled slots keep their value.  Pure fluid is
        Newtonian, sediment yields at tau_y / S; clamp(x, lo, hi) = max(lo, min(x, hi)) with a NaN lost in the min, so S = 0
        ends at the upper bound whether the pressure is positive (inf) or zero (0/0)"""
        pp = self.pp
        S = self.shear_rate_norm() if S is None else np.asarray(S, dtype=np.float64)
        visc = np.array([float(np.float32(x)) for x in pp.visccoeff])[self.fluid_num]
        sinpsi = np.array([float(np.float32(x)) for x in pp.sinpsi])[self.fluid_num]
        lim = float(np.float32(pp.limiting_kinvisc))
        rho0 = self.rho0[self.fluid_num]
        with np.errstate(divide="ignore", invalid="ignore"):
            tau_y = 2.0 * math.sqrt(3.0) * sinpsi / (3.0 - sinpsi) * np.asarray(effpres, dtype=np.float64)
            mu = np.where(self.sed_fluid, tau_y / S, visc)
        mu = np.where(visc != 0.0, mu, 0.0)
        mu = np.fmax(visc * rho0, np.fmin(mu, lim * rho0))       # fmin / fmax drop a NaN operand, like fminf / fmaxf
        out = np.array(old, dtype=np.float64)
        rows = self.is_fluid & self.active
        val = mu / self.rho if self.sp.compvisc == D.KINEMATIC else mu
        out[rows] = val[rows]
        return out
