"""All-pairs restatement of the post-processing of a run with SA_BOUNDARY -- test points, surface detection, vorticity
(src/cuda/post_process_kernel.cu:58-387 with boundarytype = SA_BOUNDARY) -- and of the wave-gage rule of GPUSPH::doWrite
(src/GPUSPH.cc:1565-1571,1649-1668,1688-1694), for the tests of those.  TEST INFRASTRUCTURE: no neighbour list, no cells, global
positions; it shares no code with the kernels, the oracle or the package beyond the problem's own arrays.

  test point   a = sum_j W(r) m_j/rho_j over FLUID and VERTEX particles with r < 2h; (v, P) = sum_j W m_j/rho_j (v_j, P(rho_j)) / a
               (and k, epsilon alike) for a > 1e-5, zeros otherwise
  surface      n = -sum_j F(r) V_j r_ij over fluid, boundary elements and vertices with r < 2h, n.w = W(0) V_i + sum_j W V_j;
               FG_SURFACE unless some neighbour has -(n.r_ij) > r |n| cos(cone), the cone of fluid or of non-fluid neighbours
  vorticity    sum_j F(r) m_j/rho_j (v_i - v_j) x r_ij over fluid neighbours
  gage         h > 0: sum z W2(r_xy, h) / sum W2 over surface particles with r_xy < 2h; h = 0: z of the nearest, first among equals

W = 21/(16 pi h^3) (1 - q/2)^4 (1 + 2q), F = (1/r) dW/dr = 105/(128 pi h^5) (q - 2)^3 (Wendland), W2 the 2D Wendland kernel.

dtype: the arithmetic of the sums.  float64 is the reference value; float32 (pair separations rounded to float32, everything after
in float32, numpy's order of summation) measures what single precision in SOME order does to the same sums: the tests bound the
device's distance from the float64 value by a multiple of the float32 evaluation's."""
import math

import numpy as np

from gpusph_amd import defs as D
from gpusph_amd.problem import info_type


class PostRef:
    def __init__(self, problem, pos_global, info, dtype=np.float64):
        sp, pp = problem.simparams, problem.physparams
        assert sp.kerneltype == D.WENDLAND
        self.dt = dt = np.dtype(dtype).type
        self.h = float(sp.slength)
        self.R = float(sp.influenceRadius)
        self.rho0, self.B, self.gam = float(pp.rho0[0]), float(pp.bcoeff[0]), float(pp.gammacoeff[0])
        self.pos = np.asarray(pos_global, dtype=np.float64)[:, :3]
        self.type = info_type(info)
        self.wc = dt(21.0/(16.0*math.pi*self.h**3))
        self.fc = dt(105.0/(128.0*math.pi*self.h**5))

    # ---- pieces
    def _pairs(self, rows, cols):
        """separations rows x cols: (d (nr, nc, 3), r (nr, nc), in reach and not the particle itself)"""
        d = (self.pos[rows][:, None, :] - self.pos[cols][None, :, :]).astype(self.dt)
        r = np.sqrt((d*d).sum(axis=2))
        reach = (r < self.dt(self.R)) & (np.asarray(rows)[:, None] != np.asarray(cols)[None, :])
        return d, r, reach

    def W(self, r):
        q = r/self.dt(self.h)
        t = self.dt(1) - q/self.dt(2)
        return self.wc*t*t*t*t*(self.dt(1) + self.dt(2)*q)

    def F(self, r):
        q = r/self.dt(self.h)
        t = q - self.dt(2)
        return self.fc*t*t*t

    def rho(self, rhotilde):
        return (np.asarray(rhotilde).astype(self.dt) + self.dt(1))*self.dt(self.rho0)

    def P(self, rhotilde):
        return self.dt(self.B)*(np.power(np.asarray(rhotilde).astype(self.dt) + self.dt(1), self.dt(self.gam)) - self.dt(1))

    # ---- the three kernels
    def testpoints(self, vel, mass, tke=None, eps=None):
        """-> (rows of the test points, (n_tp, 4) velocity and pressure, k, epsilon (or None), alpha)"""
        rows = np.where(self.type == D.PT_TESTPOINT)[0]
        cols = np.where((self.type == D.PT_FLUID) | (self.type == D.PT_VERTEX))[0]
        _, r, reach = self._pairs(rows, cols)
        vel = np.asarray(vel)
        w = np.where(reach, self.W(r)*np.asarray(mass)[cols].astype(self.dt)/self.rho(vel[cols, 3]), self.dt(0))
        alpha = w.sum(axis=1)
        fields = [vel[cols, 0], vel[cols, 1], vel[cols, 2], self.P(vel[cols, 3])]
        fields += [np.asarray(f)[cols] for f in (tke, eps) if f is not None]
        ok = alpha > self.dt(1e-5)
        out = [np.where(ok, (w*np.asarray(f).astype(self.dt)[None, :]).sum(axis=1)/np.where(ok, alpha, self.dt(1)), self.dt(0)) for f in fields]
        v4 = np.stack(out[:4], axis=1)
        extra = out[4:]
        return rows, v4, (extra[0] if tke is not None else None), (extra[-1] if eps is not None else None), alpha

    def surface(self, vel, mass, cosfluid=0.86, cosnonfluid=0.5):
        """-> (fluid rows, FG_SURFACE decision, unit normals with the Shepard sum in .w (n_fluid, 4), decision margin): the margin
        of a row is |criteria - r |n| cos| / (r |n|) of the neighbour that decides it, the one deepest inside its cone (a flagged
        row: the one closest to entering it) -- how far the decision is from turning over"""
        rows = np.where(self.type == D.PT_FLUID)[0]
        cols = np.where((self.type == D.PT_FLUID) | (self.type == D.PT_BOUNDARY) | (self.type == D.PT_VERTEX))[0]
        d, r, reach = self._pairs(rows, cols)
        vel = np.asarray(vel)
        vol = np.asarray(mass).astype(self.dt)/self.rho(vel[:, 3])
        rs = np.where(reach, r, self.dt(1))
        f = np.where(reach, self.F(rs)*vol[cols][None, :], self.dt(0))
        nrm = -(f[:, :, None]*d).sum(axis=1)
        nw = self.W(np.zeros(1, dtype=self.dt))[0]*vol[rows] + np.where(reach, self.W(rs)*vol[cols][None, :], self.dt(0)).sum(axis=1)
        ln = np.sqrt((nrm*nrm).sum(axis=1))
        crit = -(nrm[:, None, :]*d).sum(axis=2)
        cone = np.where(self.type[cols] == D.PT_FLUID, self.dt(cosfluid), self.dt(cosnonfluid))[None, :]
        lim = rs*ln[:, None]*cone
        # the decision of a row rests on the neighbour deepest inside its cone: s = (criteria - r |n| cos)/(r |n|), largest over the row
        s = np.where(reach, (crit - lim)/(rs*ln[:, None]), -np.inf).max(axis=1)
        flag = ~(s > 0)
        margin = np.abs(s)
        return rows, flag, np.concatenate([nrm/ln[:, None], nw[:, None]], axis=1), margin

    def vorticity(self, vel, mass):
        """-> (fluid rows, (n_fluid, 3))"""
        rows = np.where(self.type == D.PT_FLUID)[0]
        d, r, reach = self._pairs(rows, rows)
        vel = np.asarray(vel)
        rs = np.where(reach, r, self.dt(1))
        f = np.where(reach, self.F(rs)*(np.asarray(mass)[rows].astype(self.dt)/self.rho(vel[rows, 3]))[None, :], self.dt(0))
        u = (vel[rows, None, :3] - vel[None, rows, :3]).astype(self.dt)
        return rows, (f[:, :, None]*np.cross(u, d)).sum(axis=1)


def wendland2d(r, h):
    q = r/h
    t = 1.0 - q/2.0
    return 7.0/(4.0*math.pi*h*h)*t**4*(2.0*q + 1.0)


def gage_levels(pos_global, surface, gages):
    """the gage rule in float64: pos_global (n, 3), surface (n,) bool (active particles with FG_SURFACE), gages (g, 4): x, y, unused,
    smoothing length -> (z (g,), for the nearest-mode gages the two smallest r (g, 2), NaN elsewhere)"""
    p = np.asarray(pos_global, dtype=np.float64)[np.asarray(surface, dtype=bool)]
    gages = np.asarray(gages, dtype=np.float64).reshape(-1, 4)
    z = np.zeros(len(gages))
    two = np.full((len(gages), 2), np.nan)
    for k, (gx, gy, _, h) in enumerate(gages):
        r = np.sqrt((p[:, 0] - gx)**2 + (p[:, 1] - gy)**2)
        if h > 0:
            m = r < 2*h
            w = wendland2d(r[m], h)
            z[k] = (p[m, 2]*w).sum()/w.sum() if m.any() else np.nan
        elif len(r):
            i = int(np.argmin(r))          # the first of equals, as the strict < of the loop over the rows
            z[k] = p[i, 2]
            s = np.sort(r)
            two[k] = (s[0], s[1] if len(s) > 1 else np.inf)
    return z, two
