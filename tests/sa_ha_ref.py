"""Float64 restatement of what formulation<SPH_HA> (Hu & Adams) changes in the three SA_BOUNDARY passes over the fluid particles,
for the tests of those terms (BiFluidPoiseuilleSA's option set: several fluids, density summation, laminar Newtonian or inviscid).
TEST INFRASTRUCTURE: all pairs, no neighbour list, no cells, double precision, global positions; it shares no code with the kernels,
the oracle or the package beyond the problem's own arrays and sa_ferrari_ref.grad_gamma_float64 (the closed form of |grad gamma_as|
in double).  Written from the reference's expressions (src/cuda/forces_kernel.def, src/cuda/density_sum_kernel.cu); formulation "F1"
is the form the project had before, kept here so that the identities between the two can be stated.

With V = m/rho the actual volume, theta = 1 for a fluid particle and (volume)/deltap^3 for a vertex, F the Wendland
F(r) = 105/(128 pi h^5) (r/h - 2)^3, W the Wendland kernel, a the fluid particle, b a fluid or vertex neighbour, s an element:

  (a) forces, r_ab < 2h, r_as < 2h + deltap; sums / gamma_a, + g                    (forces_kernel.def:2289-2355, 2395-2447)
      pressure  HA  -(P_a V_a^2 theta_b/theta_a + P_b V_b^2 theta_a/theta_b)/m_a F r_ab      theta of a vertex from its ACTUAL volume
                    +(P_a Vr_a^2 + P_s Vr_s^2)/Vr_s/m_a |grad gamma_as| n_s     Vr_a = m_a/rho_a/theta_a, Vr_s = deltap^3 rho0_s/rho_s
                F1  -(P_a/rho_a^2 + P_b/rho_b^2) m_b F r_ab,   +(P_a/rho_a^2 + P_s/rho_s^2) rho_s |grad gamma_as| n_s
      viscous   both formulations: MORRIS, +visc_avg(a, b) m_b/(rho_a rho_b) F (v_a - v_b);
                -2 avg(mu_a, mu_s)/max(|r_as.n_s|, deltap) |grad gamma_as| (v_as - (v_as.n_s) n_s)/rho_a
  (b) density summation, volumic sum over the neighbours in reach at step n        (density_sum_kernel.cu:206-322)
      sum_b w_ab (W(r_ab^{n+1}) [r^{n+1} < 2h] - W(r_ab^n)),  w_ab = m_b (F1),  m_a theta_b/theta_a with theta = (m/rho0)/deltap^3 from the
      INITIAL volumes of fluid and vertex particles alike (HA)
  (c) Brezzi diffusion / gamma_a / rho0_a                                          (forces_kernel.def:1766-1824)
      sum_b xi (C_ab (P_a - P_b) - g.r_ab) m_b/rho_b F dt 2 rho_a;  C_ab = 2/(rho_a + rho_b) over fluid b (F1),
      2/(m_a (1/V_a + theta_b/(theta_a V_b))) over fluid AND vertex b, theta from the initial volumes (1 for a fluid particle) (HA)"""
import math

import numpy as np

from gpusph_amd import defs as D
from gpusph_amd.problem import info_id, info_type
from sa_ferrari_ref import grad_gamma_float64


# ---- the coefficients of one pair, as scalars (the hand-worked test of tests/test_sa_ha_ref.py goes through these) ---------------
def pair_pressure(form, Pa, ma, rhoa, Pb, mb, rhob, b_is_vertex, dp):
    """what multiplies -F r_ab in the acceleration of a"""
    if form == "F1":
        return (Pa/rhoa**2 + Pb/rhob**2)*mb
    Va, Vb = ma/rhoa, mb/rhob
    ta, tb = 1.0, (Vb/dp**3 if b_is_vertex else 1.0)
    return (Pa*Va*Va*tb/ta + Pb*Vb*Vb*ta/tb)/ma


def element_pressure(form, Pa, ma, rhoa, Ps, rhos, rho0s, dp):
    """what multiplies +|grad gamma_as| n_s in the acceleration of a"""
    if form == "F1":
        return (Pa/rhoa**2 + Ps/rhos**2)*rhos
    Vra = ma/rhoa/1.0             # theta_a = 1: a is a fluid particle
    Vrs = dp**3*rho0s/rhos
    return (Pa*Vra*Vra + Ps*Vrs*Vrs)/Vrs/ma


def dsum_weight(form, ma, rho0a, mb, rho0b, dp):
    """the weight of W_ab in the density summation of a"""
    if form == "F1":
        return mb
    ta, tb = (ma/rho0a)/dp**3, (mb/rho0b)/dp**3
    return ma/ta*tb


def brezzi_factor(form, ma, rhoa, mb, rhob, rho0b, b_is_vertex, dp):
    """C_ab, what multiplies (P_a - P_b) in the Brezzi term"""
    if form == "F1":
        return 2.0/(rhoa + rhob)
    ta, tb = 1.0, ((mb/rho0b)/dp**3 if b_is_vertex else 1.0)
    Va, Vb = ma/rhoa, mb/rhob
    return 2.0/(ma*(1.0/Va + tb/(ta*Vb)))


class HaRef:
    """The geometry of a state (who is in reach of whom, |grad gamma_as| of every fluid-element pair) evaluated once; the sums of the
    three passes for any density / velocity field over it.  pos: global positions (n, 3) of step n; info, vertices, boundelements:
    the state's rows (vertices hold ids)."""

    def __init__(self, problem, pos, info, vertices, boundelements):
        self._read_params(problem, info)
        h = self.h
        self._geometry(np.asarray(pos, dtype=np.float64)[:, :3], info, vertices, boundelements, h)

    def for_problem(self, problem, info):
        """the same geometry (positions, types, elements) with the parameters and fluid numbers of another problem"""
        import copy
        other = copy.copy(self)
        other._read_params(problem, info)
        assert (other.h, other.R, other.dp) == (self.h, self.R, self.dp) and np.array_equal(info_type(info), self.types)
        return other

    def _read_params(self, problem, info):
        sp, pp = problem.simparams, problem.physparams
        P = problem.sphx_params(len(info))
        self.h = float(sp.slength)
        self.R = float(sp.influenceRadius)
        self.dp = float(problem.m_deltap)
        nf = int(P.numfluids)
        self.rho0 = np.array([float(P.rho0[f]) for f in range(nf)])
        self.B = np.array([float(P.bcoeff[f]) for f in range(nf)])
        self.gam_eos = np.array([float(P.gammacoeff[f]) for f in range(nf)])
        self.visc = np.array([float(P.visccoeff[f]) for f in range(nf)]) if sp.rheologytype != D.INVISCID else np.zeros(nf)
        self.newtonian = sp.rheologytype == D.NEWTONIAN
        self.kinematic = P.compvisc == D.KINEMATIC
        self.avgop = int(P.avgop)
        self.const_visc = bool(P.is_const_visc)
        # a non-constant kinematic viscosity is averaged as a dynamic one whose constness is re-derived (src/cuda/visc_avg.cu:170-190)
        self.rederived_const = (not (sp.simflags & D.ENABLE_MULTIFLUID)) and sp.rheologytype == D.NEWTONIAN and sp.turbmodel != D.KEPSILON
        self.g = np.array(pp.gravity, dtype=np.float64)
        self.xi = float(np.float32(sp.densityDiffCoeff))
        self.fnum = (np.asarray(info)[:, 1] >> 12).astype(np.int64)

    def _geometry(self, pos, info, vertices, boundelements, h):
        self.pos = pos
        self.n = len(pos)
        self.types = t = info_type(info).copy()
        self.fluid = np.where(t == D.PT_FLUID)[0]
        self.vert = np.where(t == D.PT_VERTEX)[0]
        self.seg = np.where(t == D.PT_BOUNDARY)[0]
        row_of_id = np.full(int(info_id(info).max()) + 1, -1, dtype=np.int64)
        row_of_id[info_id(info)] = np.arange(len(info))
        pf = pos[self.fluid]
        # fluid <- fluid and fluid <- vertex: pairs in reach at step n, as rows of the state
        self.pp = {}
        for name, rows in (("fluid", self.fluid), ("vertex", self.vert)):
            d = pf[:, None, :] - pos[rows][None, :, :]
            r = np.sqrt((d**2).sum(axis=2))
            if name == "fluid":
                np.fill_diagonal(r, np.inf)
            i, j = np.where(r < self.R)
            self.pp[name] = dict(I=self.fluid[i], J=rows[j], d=d[i, j], r=r[i, j])
        # fluid <- element
        ps = pos[self.seg]
        self.ns = ns = np.asarray(boundelements, dtype=np.float64)[self.seg, :3]
        corners = pos[row_of_id[np.asarray(vertices)[self.seg, :3].astype(np.int64)]]
        d = pf[:, None, :] - ps[None, :, :]
        r = np.sqrt((d**2).sum(axis=2))
        i, s = np.where(r < self.R + self.dp)
        self.fe_I, self.fe_S, self.fe_s = self.fluid[i], self.seg[s], s
        self.fe_d = d[i, s]
        gg = np.empty((len(i), 2))
        for k in range(len(i)):
            gg[k] = grad_gamma_float64(ns[s[k]], (corners[s[k]] - ps[s[k]])/h, self.fe_d[k]/h, h)
        self.fe_gg, self.fe_mag = gg[:, 0], gg[:, 1]
        self.fe_g32 = None
        # rows with an element that contributes (|grad gamma_as| != 0), with a vertex in reach
        self.has_element = np.zeros(self.n, dtype=bool); self.has_element[self.fe_I[self.fe_gg != 0]] = True
        self.has_vertex = np.zeros(self.n, dtype=bool); self.has_vertex[self.pp["vertex"]["I"]] = True

    # ---- equation of state, kernels
    def _state(self, vel, mass):
        rt = np.asarray(vel, dtype=np.float64)[:, 3]
        rho = (rt + 1.0)*self.rho0[self.fnum]
        P = self.B[self.fnum]*(np.power(rt + 1.0, self.gam_eos[self.fnum]) - 1.0)
        return rho, P, np.asarray(mass, dtype=np.float64), np.asarray(vel, dtype=np.float64)[:, :3]

    def F(self, r):
        return 105.0/(128.0*math.pi*self.h**5)*(r/self.h - 2.0)**3

    def W(self, r):
        q = r/self.h
        return 21.0/(16.0*math.pi*self.h**3)*(1.0 - 0.5*q)**4*(1.0 + 2.0*q)

    def _visc_pair(self, I, J, rho, m):
        """visc_avg(a, b) m_b / (rho_a rho_b) with the averaging of src/cuda/visc_avg.cu"""
        va, vb = self.visc[self.fnum[I]], self.visc[self.fnum[J]]
        if self.kinematic and self.const_visc:
            ra, rb = rho[I], rho[J]
            if self.avgop == D.ARITHMETIC:
                return va*m[J]*(ra + rb)/(ra*rb)
            if self.avgop == D.HARMONIC:
                return va*4*m[J]/(ra + rb)
            return va*2*m[J]/np.sqrt(ra*rb)
        const = self.const_visc
        if self.kinematic:
            va, vb, const = va*rho[I], vb*rho[J], self.rederived_const
        if const:
            avg2 = 2*va
        elif self.avgop == D.ARITHMETIC:
            avg2 = va + vb
        elif self.avgop == D.HARMONIC:
            avg2 = 4*va*vb/(va + vb)
        else:
            avg2 = 2*np.sqrt(va*vb)
        return m[J]*avg2/(rho[I]*rho[J])

    # ---- (a)
    def forces(self, form, vel, mass, gamma):
        """-> dict(fluid=, vertex=, element=) of (n, 3) contributions to force.xyz (already divided by gamma; pressure + viscous parts),
        total = their sum + g for the fluid rows; self.last_K: per fluid-element pair, what multiplies |grad gamma_as| in force.xyz"""
        rho, P, m, v = self._state(vel, mass)
        gam = np.asarray(gamma, dtype=np.float64)
        out = {}
        for name in ("fluid", "vertex"):
            q = self.pp[name]
            I, J = q["I"], q["J"]
            isv = name == "vertex"
            if form == "F1":
                c = (P[I]/rho[I]**2 + P[J]/rho[J]**2)*m[J]
            else:
                Va, Vb = m[I]/rho[I], m[J]/rho[J]
                tb = Vb/self.dp**3 if isv else np.ones(len(I))
                c = (P[I]*Va*Va*tb + P[J]*Vb*Vb/tb)/m[I]
            F = self.F(q["r"])
            term = -(c*F)[:, None]*q["d"]
            if self.newtonian:
                term = term + (self._visc_pair(I, J, rho, m)*F)[:, None]*(v[I] - v[J])
            acc = np.zeros((self.n, 3))
            np.add.at(acc, I, term)
            out[name] = acc/gam[:, None]
        I, S = self.fe_I, self.fe_S
        nrm = self.ns[self.fe_s]
        if form == "F1":
            c = (P[I]/rho[I]**2 + P[S]/rho[S]**2)*rho[S]
        else:
            Vra = m[I]/rho[I]
            Vrs = self.dp**3*self.rho0[self.fnum[S]]/rho[S]
            c = (P[I]*Vra*Vra + P[S]*Vrs*Vrs)/Vrs/m[I]
        K = c[:, None]*nrm
        if self.newtonian:
            vr = v[I] - v[S]
            vn = (vr*nrm).sum(axis=1)
            r_as = np.maximum(np.abs((self.fe_d*nrm).sum(axis=1)), self.dp)
            mua = self.visc[self.fnum[I]]*(rho[I] if self.kinematic else 1.0)
            mus = self.visc[self.fnum[S]]*(rho[S] if self.kinematic else 1.0)
            avg = 0.5*(mua + mus) if self.avgop == D.ARITHMETIC else (2*mua*mus/(mua + mus) if self.avgop == D.HARMONIC else np.sqrt(mua*mus))
            K = K - (2.0*avg/r_as/rho[I])[:, None]*(vr - vn[:, None]*nrm)
        self.last_K = K/gam[I][:, None]
        acc = np.zeros((self.n, 3))
        np.add.at(acc, I, self.last_K*self.fe_gg[:, None])
        out["element"] = acc
        tot = out["fluid"] + out["vertex"] + out["element"]
        tot[self.fluid] += self.g
        out["total"] = tot
        return out

    # ---- (b)
    def density_sum(self, form, new_pos, mass):
        """-> (volumic sum per row, sum of the magnitudes of its terms per row, number of its terms per row) for the new global
        positions new_pos (n, 3); the neighbours are those in reach at step n (the positions the geometry was made from)"""
        m = np.asarray(mass, dtype=np.float64)
        x1 = np.asarray(new_pos, dtype=np.float64)[:, :3]
        tot, mag, cnt = np.zeros(self.n), np.zeros(self.n), np.zeros(self.n)
        for name in ("fluid", "vertex"):
            q = self.pp[name]
            I, J = q["I"], q["J"]
            if form == "F1":
                w = m[J]
            else:
                ta = (m[I]/self.rho0[self.fnum[I]])/self.dp**3
                tb = (m[J]/self.rho0[self.fnum[J]])/self.dp**3
                w = m[I]/ta*tb
            r1 = np.sqrt(((x1[I] - x1[J])**2).sum(axis=1))
            W1 = np.where(r1 < self.R, self.W(r1), 0.0)
            W0 = self.W(q["r"])
            np.add.at(tot, I, w*(W1 - W0))
            np.add.at(mag, I, np.abs(w)*(W1 + W0))
            np.add.at(cnt, I, 2.0)
        return tot, mag, cnt

    # ---- (c)
    def brezzi(self, form, vel, mass, gamma, dt):
        """-> dict(fluid=, vertex=) of the parts of force.w of the Brezzi pass (divided by gamma and rho0), total = their sum"""
        rho, P, m, _ = self._state(vel, mass)
        gam = np.asarray(gamma, dtype=np.float64)
        out = {}
        for name in ("fluid", "vertex"):
            q = self.pp[name]
            I, J = q["I"], q["J"]
            acc = np.zeros(self.n)
            if name == "fluid" or form != "F1":
                if form == "F1":
                    C = 2.0/(rho[I] + rho[J])
                else:
                    tb = (m[J]/self.rho0[self.fnum[J]])/self.dp**3 if name == "vertex" else np.ones(len(I))
                    C = 2.0/(m[I]*(rho[I]/m[I] + tb*rho[J]/m[J]))
                term = self.xi*(C*(P[I] - P[J]) - q["d"] @ self.g)*m[J]/rho[J]*self.F(q["r"])*dt*2.0*rho[I]
                np.add.at(acc, I, term)
            out[name] = acc/gam/self.rho0[self.fnum]
        out["total"] = out["fluid"] + out["vertex"]
        return out

    # ---- what the float evaluation of |grad gamma_as| moves a row by
    def float32_shift(self, problem, pos_local, hash_, boundelements, vertpos):
        """(n, 3): sum_s (g_oracle - g_float64) K_s per row for the K_s of the LAST forces(...) call, g_oracle being the CPU oracle's float
        evaluation of the same element (orc_grad_gamma_vp: the reference's operation order), as sa_ferrari_ref.float32_shift measures it:
        the relative position is formed from the state's float32 rows as the kernels form it (the particle's cell-local position moved
        into the element's cell with one rounding, minus the element's).  The float values are kept: they depend on the geometry only."""
        if self.fe_g32 is None:
            import ctypes as C
            import oracle_lib as ol
            L = ol.lib()
            L.orc_grad_gamma_vp.restype = C.c_float
            L.orc_grad_gamma_vp.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            h = np.float32(self.h)
            inv_h = np.float32(1.0)/h
            pos = np.asarray(pos_local, dtype=np.float32)
            be = np.ascontiguousarray(boundelements, dtype=np.float32)
            vp = [np.ascontiguousarray(v, dtype=np.float32) for v in vertpos]
            cell = problem.grid_pos_from_hash(np.asarray(hash_))
            csz = problem.m_cellsize.astype(np.float32).astype(np.float64)
            g32 = np.zeros(len(self.fe_I))
            for k, (i, s) in enumerate(zip(self.fe_I, self.fe_S)):
                own = (pos[i, :3].astype(np.float64) - (cell[s] - cell[i])*csz).astype(np.float32)
                q = ((own - pos[s, :3])*inv_h).astype(np.float32)
                g32[k] = float(L.orc_grad_gamma_vp(C.c_float(h), C.c_float(q[0]), C.c_float(q[1]), C.c_float(q[2]), be[s].ctypes.data_as(C.c_void_p),
                                                   *[v[s].ctypes.data_as(C.c_void_p) for v in vp]))
            self.fe_g32 = g32
        shift = np.zeros((self.n, 3))
        np.add.at(shift, self.fe_I, (self.fe_g32 - self.fe_gg)[:, None]*self.last_K)
        return shift


def ha_ref_of_state(problem, pos_local, hash_, info, vertices, boundelements):
    """HaRef of a (sorted) device or oracle state: cell-local positions + hashes -> global positions"""
    return HaRef(problem, problem.global_pos(np.asarray(pos_local), np.asarray(hash_)), info, vertices, boundelements)
