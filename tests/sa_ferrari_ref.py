"""Float64 restatement of the Ferrari density diffusion of the continuity equation with SA_BOUNDARY (compute_density_diffusion,
src/cuda/forces_kernel.def:1608-1705, the non-SPH_HA variants), for the tests of that term.  TEST INFRASTRUCTURE: all pairs, no
neighbour list, no cells, double precision, global positions; it shares no code with the kernels, the oracle or the package
beyond the problem's own arrays.

  fluid <- fluid      DrDt += xi m_j max(c_i, c_j) (rho_i - rho_j + g_corr)/rho_i / r (r.r) F(r)     r < 2h, 0 for r <= 1e-4 h
  fluid <- vertex     nothing
  fluid <- element    DrDt -= xi max(c_i, c_s) (rho_i - rho_s + g_corr)/r (r_is.n_s) |grad gamma_as|   r < 2h + deltap, 0 for r <= 1e-4 h
  g_corr = -(g.r_ij) rho0/c0^2;  both sums / gamma_i / rho0 are the Ferrari part of force.w

|grad gamma_as| is the closed form of src/cuda/gamma.cuh:248-370 in double precision (the project's float64 version of
tests/test_sa_wall_gamma.py, with the sum of the magnitudes of its cancelling terms as tests/sa_helpers.py keeps it: what a float32
evaluation of the same element can be off by, in whatever order it adds)."""
import math

import numpy as np

from gpusph_amd import defs as D
from gpusph_amd.problem import info_id, info_type


def grad_gamma_float64(ns, qv, q, h):
    """-> (|grad gamma_as|, sum of the magnitudes of the terms added up); ns unit normal, qv (3, 3) corners and q the particle,
    both relative to the element's position in units of h"""
    pas = float(ns @ q); a = abs(pas)
    if a >= 2:
        return 0.0, 0.0
    g = mag = tot = inside = tot_mag = 0.0
    for e in range(3):
        v0, v1 = qv[e], qv[(e + 1) % 3]
        t = (v0 - v1)/np.linalg.norm(v0 - v1)
        m = np.cross(ns, t); m /= np.linalg.norm(m)
        b = float(m @ (q - v0)); c = math.hypot(pas, b)
        s0, s1 = float(-(q - v0) @ t), float(-(q - v1) @ t)
        a1, a0 = math.atan2(s1, abs(b)), math.atan2(s0, abs(b))
        tot += math.copysign(a1 - a0, b); tot_mag += abs(a1) + abs(a0)
        if c < 2:
            lim = math.sqrt(4 - c*c)
            s0 = math.copysign(min(abs(s0), lim), s0); s1 = math.copysign(min(abs(s1), lim), s1)
            d0 = min(math.hypot(c, s0), 2.0); d1 = min(math.hypot(c, s1), 2.0)

            def pol(s, d):
                s2 = s*s
                terms = [3*a**4*(-420), 3*a**4*29*d, b**4*(-420), b**4*33*d, 2*a*a*(-210*8), 2*a*a*(-210*s2), 2*a*a*756*d, 2*a*a*19*s2*d,
                         4*336, 4*s2*s2*(-21), 4*s2*s2*2*d, 4*s2*28*(-5), 4*s2*28*3*d,
                         2*b*b*420*(-2), 2*b*b*420*d, 2*b*b*6*a*a*(-105), 2*b*b*6*a*a*8*d, 2*b*b*s2*(-140), 2*b*b*s2*13*d]
                return s*sum(terms), abs(s)*sum(abs(x) for x in terms)

            def angle(s, d):
                x, y = math.atan2(a*s, b*d), math.atan2(s, b)
                return x - y, abs(x) + abs(y)

            def lg(s, d):
                v = math.copysign(1, s)*math.acosh(max(d/max(c, 1e-7), 1.0))
                return v, abs(v)
            K = 5*b**6 + 21*b**4*(8 + a*a) + 35*b*b*a*a*(16 + a*a) + 35*a**4*(24 + a*a)
            (p1, mp1), (p0, mp0) = pol(s1, d1), pol(s0, d0)
            (g1, mg1), (g0, mg0) = angle(s1, d1), angle(s0, d0)
            (l1, ml1), (l0, ml0) = lg(s1, d1), lg(s0, d0)
            ca = 48*a**5*(28 + a*a)
            g += 0.00015542474911*(ca*(g1 - g0) + b*(p1 - p0 + 3*K*(l1 - l0)))
            mag += 0.00015542474911*(ca*(mg1 + mg0) + abs(b)*(mp1 + mp0 + 3*K*(ml1 + ml0)))
            inside += math.copysign(math.atan2(s1, abs(b)) - math.atan2(s0, abs(b)), b)
    w = 0.05968310365947*(1 - a/2)**5*(2 + 5*a + 4*a*a)
    return (g + (inside - tot)*w)/h, (mag + 2*tot_mag*w)/h


class FerrariRef:
    """The geometry of a state (who is in reach of whom, |grad gamma_as| of every fluid-element pair) evaluated once; the sums for
    any density field over it.  pos: global positions (n, 3); info, vertices, boundelements: the state's rows (vertices hold ids);
    only: the rows (fluid particles) to form the sums for, all of them by default -- their neighbours are everybody either way."""

    def __init__(self, problem, pos, info, vertices, boundelements, only=None):
        sp, pp = problem.simparams, problem.physparams
        self.h = h = float(sp.slength)
        self.R = float(sp.influenceRadius)
        self.dp = float(problem.m_deltap)
        self.rho0, self.c0 = float(pp.rho0[0]), float(pp.sscoeff[0])
        self.cpow = (float(pp.gammacoeff[0]) - 1.0)/2.0
        self.g = np.array(pp.gravity, dtype=np.float64)
        self.xi = float(np.float32(sp.densityDiffCoeff))
        pos = np.asarray(pos, dtype=np.float64)[:, :3]
        t = info_type(info)
        self.fluid = np.where(t == D.PT_FLUID)[0]
        self.seg = np.where(t == D.PT_BOUNDARY)[0]
        row_of_id = np.full(int(info_id(info).max()) + 1, -1, dtype=np.int64)
        row_of_id[info_id(info)] = np.arange(len(info))
        # fluid <- fluid, all pairs in reach: r, r.r F(r) with the Wendland F = 105/(128 pi h^5) (r/h - 2)^3
        pf = pos[self.fluid]
        d = pf[:, None, :] - pf[None, :, :]
        r = np.sqrt((d**2).sum(axis=2))
        np.fill_diagonal(r, np.inf)      # no particle is its own neighbour
        if only is not None:
            r[~np.isin(self.fluid, np.asarray(only))] = np.inf
        self.ff_i, self.ff_j = np.where(r < self.R)
        self.ff_r = r[self.ff_i, self.ff_j]
        self.ff_d = d[self.ff_i, self.ff_j]
        self.ff_F = 105.0/(128.0*math.pi*h**5)*(self.ff_r/h - 2.0)**3
        # fluid <- element
        ps = pos[self.seg]
        ns = np.asarray(boundelements, dtype=np.float64)[self.seg, :3]
        corners = pos[row_of_id[np.asarray(vertices)[self.seg, :3].astype(np.int64)]]      # (nseg, 3, 3)
        d = pf[:, None, :] - ps[None, :, :]
        r = np.sqrt((d**2).sum(axis=2))
        if only is not None:
            r[~np.isin(self.fluid, np.asarray(only))] = np.inf
        self.fe_i, self.fe_s = np.where(r < self.R + self.dp)
        self.fe_r = r[self.fe_i, self.fe_s]
        self.fe_d = d[self.fe_i, self.fe_s]
        self.fe_rn = (self.fe_d*ns[self.fe_s]).sum(axis=1)
        gg = np.empty((len(self.fe_i), 2))
        for k, (i, s) in enumerate(zip(self.fe_i, self.fe_s)):
            gg[k] = grad_gamma_float64(ns[s], (corners[s] - ps[s])/h, self.fe_d[k]/h, h)
        self.fe_gg, self.fe_mag = gg[:, 0], gg[:, 1]

    def sums(self, rhotilde, mass, gamma, xi=None, gravity_correction=True):
        """-> (fluid part, element part, room) of force.w per row of the state (zero for the rows that are not fluid particles);
        room: 2^-24 sum_s M_s |K_s| / gamma / rho0, the unit of what float32 rounding inside |grad gamma_as| moves the element part by"""
        xi = self.xi if xi is None else float(xi)
        rt = np.asarray(rhotilde, dtype=np.float64)
        rho = (rt + 1.0)*self.rho0
        c = self.c0*np.power(rt + 1.0, self.cpow)
        m = np.asarray(mass, dtype=np.float64)
        gam = np.asarray(gamma, dtype=np.float64)
        n = len(rt)
        gc = self.rho0/self.c0**2 if gravity_correction else 0.0
        I, J = self.fluid[self.ff_i], self.fluid[self.ff_j]
        on = self.ff_r > 1e-4*self.h
        term = xi*m[J]*np.maximum(c[I], c[J])*(rho[I] - rho[J] - (self.ff_d @ self.g)*gc)/rho[I]/self.ff_r*self.ff_r**2*self.ff_F
        fsum = np.zeros(n)
        np.add.at(fsum, I, np.where(on, term, 0.0))
        I, S = self.fluid[self.fe_i], self.seg[self.fe_s]
        on = self.fe_r > 1e-4*self.h
        K = np.where(on, -xi*np.maximum(c[I], c[S])*(rho[I] - rho[S] - (self.fe_d @ self.g)*gc)/np.where(on, self.fe_r, 1.0)*self.fe_rn, 0.0)
        self.last_K = K/gam[I]/self.rho0      # per fluid-element pair: what multiplies |grad gamma_as| in force.w
        esum, room = np.zeros(n), np.zeros(n)
        np.add.at(esum, I, K*self.fe_gg)
        np.add.at(room, I, 2.0**-24*np.abs(K)*self.fe_mag)
        f = self.fluid
        out = [np.zeros(n), np.zeros(n), np.zeros(n)]
        for o, v in zip(out, (fsum, esum, room)):
            o[f] = v[f]/gam[f]/self.rho0
        return tuple(out)


def ferrari_ref_of_state(problem, pos_local, hash_, info, vertices, boundelements, only=None):
    """FerrariRef of a (sorted) device or oracle state: cell-local positions + hashes -> global positions"""
    return FerrariRef(problem, problem.global_pos(np.asarray(pos_local), np.asarray(hash_)), info, vertices, boundelements, only=only)


def float32_shift(ref, problem, pos_local, hash_, boundelements, vertpos):
    """What a float32 evaluation of |grad gamma_as| does to the element part of the rows of the LAST ref.sums(...) call, measured on
    the CPU oracle's evaluation of the same elements (orc_grad_gamma_vp: the reference's operation order in float, which is not
    the kernels'): sum_s (g_oracle - g_float64) K_s per row.  For some positions -- an element that the support only grazes --
    the reference's float value of the closed form is several 1e-3 / h away from the float64 value (tests/test_sa_wall_gamma.py),
    by a jump that the last bit of the relative position decides; tests/test_gpu_sa.py grants a wall row twice that distance of
    its own elements on top of the plain tolerance, and so do the tests of this term.  The relative position is formed from the
    state's float32 rows as the kernels form it: the particle's cell-local position moved into the element's cell with one
    rounding, minus the element's."""
    import ctypes as C
    import oracle_lib as ol
    L = ol.lib()
    L.orc_grad_gamma_vp.restype = C.c_float
    L.orc_grad_gamma_vp.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    h = np.float32(ref.h)
    inv_h = np.float32(1.0)/h
    pos = np.asarray(pos_local, dtype=np.float32)
    be = np.ascontiguousarray(boundelements, dtype=np.float32)
    vp = [np.ascontiguousarray(v, dtype=np.float32) for v in vertpos]
    cell = problem.grid_pos_from_hash(np.asarray(hash_))
    csz = problem.m_cellsize.astype(np.float32).astype(np.float64)
    shift = np.zeros(len(pos))
    for k, (i, s) in enumerate(zip(ref.fluid[ref.fe_i], ref.seg[ref.fe_s])):
        if ref.last_K[k] == 0.0:
            continue
        own = (pos[i, :3].astype(np.float64) - (cell[s] - cell[i])*csz).astype(np.float32)      # fmaf(-(float)offset, cellsize, pos)
        q = ((own - pos[s, :3])*inv_h).astype(np.float32)
        g32 = float(L.orc_grad_gamma_vp(C.c_float(h), C.c_float(q[0]), C.c_float(q[1]), C.c_float(q[2]), be[s].ctypes.data_as(C.c_void_p),
                                        *[v[s].ctypes.data_as(C.c_void_p) for v in vp]))
        shift[i] += (g32 - ref.fe_gg[k])*ref.last_K[k]
    return shift
