"""Float64 ALL-PAIRS evaluations of the pair sums, with the kernel function as a parameter, for tests/test_headline_allpairs.py (the
Wendland kernel of the headline option set) and tests/test_kernel_axis_allpairs.py / tests/test_gpu_kernel_axis.py (all four
kernels).  TEST INFRASTRUCTURE, no GPU.

Nothing here is shared with oracle/sph_oracle.c: global float64 positions, neighbours by distance (k-d tree -- no cells, no hash, no
neighbour list, no list order), the formulas of the reference written from its source text (see tests/test_headline_allpairs.py for
the lines).  F and W are callables of the distance array: F(r) = (1/r) dW/dr, W(r) the kernel.  Who is whose neighbour follows the
lists of the DYN / LJ / MK boundary models: a fluid particle sees fluid and boundary particles, a boundary particle fluid ones only.
Periodic boxes (tests/grid_edge_cases.py): neighbours() and momentum_continuity() take the list of image shifts and sum over them."""
import itertools

import numpy as np
from scipy.spatial import cKDTree

from gpusph_amd import defs as D


def consts(sim):
    p = sim.o.p
    h = float(p.slength)
    return dict(h=h, rho0=float(p.rho0[0]), B=float(p.bcoeff[0]), gam=float(p.gammacoeff[0]), c0=float(p.sscoeff[0]),
                cpow=float(p.sspowercoeff[0]), g=np.array([p.gravity[0], p.gravity[1], p.gravity[2]], dtype=np.float64),
                alpha=float(p.artvisccoeff), eps=float(p.epsartvisc), Dc=float(p.densityDiffCoeff),
                fcoeff=105.0/(128.0*np.pi*h**5), R=float(p.influenceradius))


def _types(sim):
    n = sim.n
    ptype = sim.info[:n, 0] & 7
    return ptype == D.PT_FLUID, ptype == D.PT_BOUNDARY


def _image_pairs(gp, n, R, shifts):
    """-> (list of int64 arrays, list of (len, 3) float64 arrays): for every particle i below n the particles j != i with
    |x_i - x_j - s| < R for a shift s of `shifts`, once per such shift, and that shift.  shifts = None: the zero shift alone"""
    shifts = [np.zeros(3)] if shifts is None else [np.asarray(s, dtype=np.float64) for s in shifts]
    tree = cKDTree(gp)
    owner, other, shift = [], [], []
    for s in shifts:
        q = gp[:n] - s
        lens = tree.query_ball_point(q, R, return_length=True)
        if not lens.any():
            continue                               # an image out of everybody's reach
        j = np.fromiter(itertools.chain.from_iterable(tree.query_ball_point(q, R)), dtype=np.int64, count=int(lens.sum()))
        i = np.repeat(np.arange(n), lens)
        owner.append(i[j != i]); other.append(j[j != i]); shift.append(np.broadcast_to(s, (len(other[-1]), 3)))
    owner, other, shift = np.concatenate(owner), np.concatenate(other), np.concatenate(shift)
    # by particle; within a particle shift after shift, within a shift in the tree's order
    order = np.argsort(owner, kind="stable")
    cuts = np.cumsum(np.bincount(owner, minlength=n))[:-1]
    return np.split(other[order], cuts), np.split(shift[order], cuts)


def neighbours(sim, gp, k, fluid_only=False, shifts=None):
    """-> list of int64 arrays: the neighbours of every particle below sim.n within the influence radius, itself excluded.  Boundary
    particles see fluid ones only; test points see fluid ones only; nobody sees a test point.  shifts (float64 3-vectors, the periodic
    images of tests/grid_edge_cases.py): a neighbour is listed once per shift s with |x_i - x_j - s| within the radius"""
    n = sim.n
    fluid, bound = _types(sim)
    nbs_all = _image_pairs(gp, n, k["R"]*(1 - 1e-7), shifts)[0]
    out = []
    for i in range(n):
        nb = nbs_all[i]
        if len(nb):
            nb = nb[fluid[nb]] if (fluid_only or not fluid[i]) else nb[fluid[nb] | bound[nb]]
        out.append(nb)
    return out


def momentum_continuity(sim, gp, k, F, shifts=None, eos_rounding=False):
    """the headline option set (SPH_F1, artificial viscosity, Colagrossi diffusion, DYN_BOUNDARY, one fluid) -> dict(acc (n, 3),
    drt = d(rho~)/dt, amb = half the diffusion terms of the pairs on the Colagrossi threshold (the slack their particle gets), pairs,
    ambiguous, fluid, bound, switch_on, switch_off = fluid pairs off the threshold on either side of the switch).  shifts: as in
    neighbours(); r_ij = x_i - x_j - s is what enters F, v.r, g.r and the direction of the force.  eos_rounding: the threshold's band
    also takes in what float32 does to P on its way through the equation of state -- 1 + rho~ rounded to 2^-24 and raised to gamma
    moves P by gamma B 2^-24 (0.024 Pa for the water of the test problems, where the band of P's own last bits is 1e-4).  For
    states with rho~ inside a few 1e-3, whose pressure differences are small enough for pairs to land in between"""
    n = sim.n
    fluid, bound = _types(sim)
    m = sim.pos[:n, 3].astype(np.float64)
    v = sim.vel[:n, :3].astype(np.float64)
    ratio = sim.vel[:n, 3].astype(np.float64) + 1.0
    rho = ratio*k["rho0"]
    P = k["B"]*(ratio**k["gam"] - 1.0)
    c = k["c0"]*ratio**k["cpow"]
    # float32 rounding of P: what can move a pair across the Colagrossi threshold
    Pulp = np.spacing(np.abs(P).astype(np.float32)).astype(np.float64)*4.0 + 1e-30
    if eos_rounding:      # the rounding of 1 + rho~, and two ulp of powf's result, both times B
        Pulp = Pulp + (k["gam"] + 2.0)*k["B"]*ratio**k["gam"]*2.0**-23

    acc = np.zeros((n, 3)); drdt = np.zeros(n); amb = np.zeros(n)
    pairs = ambiguous = switch_on = switch_off = 0
    nbs_all, shs_all = _image_pairs(gp, n, k["R"]*(1 - 1e-7), shifts)
    for i in range(n):
        nb, sh = nbs_all[i], shs_all[i]
        if bound[i]:
            sh = sh[fluid[nb]]
            nb = nb[fluid[nb]]                     # DYN boundary particles list fluid neighbours only
        if not len(nb):
            continue
        d = gp[i] - gp[nb] - sh
        r2 = (d*d).sum(axis=1)
        r = np.sqrt(r2)
        Fr = F(r)
        vr = ((v[i] - v[nb])*d).sum(axis=1)
        mF = m[nb]*Fr
        cont = mF*vr
        nf = fluid[nb]
        margin = np.abs(P[i] - P[nb]) - np.abs((d @ k["g"])*rho[i])
        dterm = k["Dc"]*k["c0"]*(rho[nb]/rho[i] - 1.0)*mF
        on = nf & (margin >= 0.0)
        edge = nf & (np.abs(margin) <= Pulp[i] + Pulp[nb] + 1e-6*np.abs((d @ k["g"])*rho[i]))
        drdt[i] = cont.sum() - dterm[on & ~edge].sum()
        # threshold pairs: counted either way
        amb[i] = np.abs(dterm[edge]).sum()
        drdt[i] -= 0.5*dterm[edge].sum()
        pairs += int(nf.sum()); ambiguous += int(edge.sum())
        switch_on += int((on & ~edge).sum()); switch_off += int((nf & ~on & ~edge).sum())
        if fluid[i]:
            pg = P[i]/rho[i]**2 + P[nb]/rho[nb]**2
            visc = np.where(vr < 0.0, vr*k["h"]*k["alpha"]*(c[i] + c[nb])/((r2 + k["eps"])*(rho[i] + rho[nb])), 0.0)
            acc[i] = ((visc - pg)*mF) @ d + k["g"]
    return dict(acc=acc, drt=drdt/k["rho0"], amb=0.5*amb/k["rho0"], pairs=pairs, ambiguous=ambiguous, fluid=fluid, bound=bound,
                switch_on=switch_on, switch_off=switch_off)


def tau_all_pairs(sim, gp, k, smag, ksps, F):
    """SPS stress tensor (xx, xy, xz, yy, yz, zz) and turbulent viscosity of every particle"""
    n = sim.n
    m = sim.pos[:n, 3].astype(np.float64)
    v = sim.vel[:n, :3].astype(np.float64)
    rho = (sim.vel[:n, 3].astype(np.float64) + 1.0)*k["rho0"]
    fluid, bound = _types(sim)
    tree = cKDTree(gp)
    tau = np.zeros((n, 6)); nu = np.zeros(n)
    nbs_all = tree.query_ball_point(gp, k["R"]*(1 - 1e-7))
    for i in range(n):
        nb = np.array([j for j in nbs_all[i] if j != i], dtype=np.int64)
        if bound[i]:
            nb = nb[fluid[nb]]
        if not len(nb):
            continue
        d = gp[i] - gp[nb]
        r = np.sqrt((d*d).sum(axis=1))
        w = F(r)*m[nb]/rho[nb]
        dv = -((v[i] - v[nb])[:, :, None]*(d*w[:, None])[:, None, :]).sum(axis=0)     # dv[a][b] = d v_a / d x_b
        xx, yy, zz = dv[0, 0], dv[1, 1], dv[2, 2]
        xy, xz, yz = dv[0, 1] + dv[1, 0], dv[0, 2] + dv[2, 0], dv[1, 2] + dv[2, 1]
        S2 = 2.0*(xx*xx + yy*yy + zz*zz) + xy*xy + xz*xz + yz*yz
        S = np.sqrt(S2)
        nu[i] = smag*S
        divu = (2.0/3.0)*nu[i]*(xx + yy + zz)
        bl = ksps*S2
        tau[i] = [(2*nu[i]*xx - divu - bl)/rho[i], nu[i]*xy/rho[i], nu[i]*xz/rho[i],
                  (2*nu[i]*yy - divu - bl)/rho[i], nu[i]*yz/rho[i], (2*nu[i]*zz - divu - bl)/rho[i]]
    return tau, nu


def sps_divergence(sim, gp, k, tau, F):
    """sum_j m_j F_ij (tau_i + tau_j) . r_ij of every fluid particle, for the float32 tau the forces pass is fed with"""
    n = sim.n
    T = np.zeros((n, 3, 3))
    t64 = tau[:n].astype(np.float64)
    T[:, 0, 0], T[:, 0, 1], T[:, 0, 2], T[:, 1, 1], T[:, 1, 2], T[:, 2, 2] = t64.T
    T[:, 1, 0], T[:, 2, 0], T[:, 2, 1] = T[:, 0, 1], T[:, 0, 2], T[:, 1, 2]
    m = sim.pos[:n, 3].astype(np.float64)
    fluid = (sim.info[:n, 0] & 7) == D.PT_FLUID
    tree = cKDTree(gp)
    want = np.zeros((n, 3))
    for i in np.where(fluid)[0]:
        nb = np.array([j for j in tree.query_ball_point(gp[i], k["R"]*(1 - 1e-7)) if j != i], dtype=np.int64)
        d = gp[i] - gp[nb]
        r = np.sqrt((d*d).sum(axis=1))
        mF = m[nb]*F(r)
        want[i] = np.einsum("j,jab,jb->a", mF, T[i][None] + T[nb], d)
    return want


# ---------------------------------------------------------------------------------------------------------------------------------
# the sums that take W: density filters, XSPH, test points; and the gradient sums of the post-processing (vorticity, surface normal)

def _rho(sim, k):
    """physical density of every particle: rho0 of ITS fluid times (1 + rho~)"""
    n = sim.n
    p = sim.o.p
    fnum = (sim.info[:n, 1] >> 12).astype(np.int64)
    r0 = np.array([float(p.rho0[f]) for f in range(max(int(fnum.max()) + 1, 1))])
    return r0[fnum]*(sim.vel[:n, 3].astype(np.float64) + 1.0), r0[fnum]


def shepard(sim, gp, k, W, nbs=None):
    """Shepard-filtered rho~ of the fluid particles (NaN elsewhere): sum m_j W / sum (m_j / rho_j) W over the particle itself
    (W(0)) and its fluid and DYN-boundary neighbours; W carries the Gaussian's subtracted constant"""
    n = sim.n
    fluid, bound = _types(sim)
    m = sim.pos[:n, 3].astype(np.float64)
    rho, rho0 = _rho(sim, k)
    nbs = neighbours(sim, gp, k, fluid_only=sim.o.p.boundarytype != D.DYN_BOUNDARY) if nbs is None else nbs
    W0 = float(W(np.zeros(1))[0])
    out = np.full(n, np.nan)
    for i in np.where(fluid)[0]:
        nb = nbs[i]
        w = W(np.sqrt(((gp[i] - gp[nb])**2).sum(axis=1)))*m[nb]
        t1 = m[i]*W0 + w.sum()
        t2 = m[i]*W0/rho[i] + (w/rho[nb]).sum()
        out[i] = t1/t2/rho0[i] - 1.0
    return out


def mls(sim, gp, k, W, nbs=None):
    """MLS-filtered rho~ of every particle: the first row of the inverse of the 4 x 4 moment matrix sum (1, s) (1, s)^T W V_j
    (s = r_ij / h, self term W(0) V_i in its corner) applied to sum m_j W (1, r_ij)"""
    n = sim.n
    m = sim.pos[:n, 3].astype(np.float64)
    rho, rho0 = _rho(sim, k)
    nbs = neighbours(sim, gp, k, fluid_only=sim.o.p.boundarytype != D.DYN_BOUNDARY) if nbs is None else nbs
    W0 = float(W(np.zeros(1))[0])
    h = k["h"]
    out = np.full(n, np.nan)
    cond = np.zeros(n)
    for i in range(n):
        nb = nbs[i]
        d = gp[i] - gp[nb]
        w = W(np.sqrt((d*d).sum(axis=1)))
        q = np.concatenate([np.ones((len(nb), 1)), d/h], axis=1)
        M = np.einsum("j,ja,jb->ab", w*m[nb]/rho[nb], q, q)
        M[0, 0] += W0*m[i]/rho[i]
        cond[i] = np.linalg.cond(M)
        if not np.isfinite(cond[i]) or cond[i] > 1e6:
            continue
        B = np.linalg.solve(M, np.array([1.0, 0.0, 0.0, 0.0]))
        B[1:] /= h
        r = B[0]*W0*m[i] + ((B[0] + d @ B[1:])*w*m[nb]).sum()
        out[i] = r/rho0[i] - 1.0
    return out, cond


def xsph(sim, gp, k, W, nbs=None):
    """the XSPH row of the fluid particles: 2 * mean velocity = -2 sum_j m_j W (v_i - v_j)/(rho_i + rho_j) over FLUID neighbours"""
    n = sim.n
    fluid, _ = _types(sim)
    m = sim.pos[:n, 3].astype(np.float64)
    v = sim.vel[:n, :3].astype(np.float64)
    rho, _ = _rho(sim, k)
    nbs = neighbours(sim, gp, k, fluid_only=True) if nbs is None else nbs
    out = np.zeros((n, 3))
    for i in np.where(fluid)[0]:
        nb = nbs[i]
        w = W(np.sqrt(((gp[i] - gp[nb])**2).sum(axis=1)))*m[nb]/(rho[i] + rho[nb])
        out[i] = -2.0*(w[:, None]*(v[i] - v[nb])).sum(axis=0)
    return out


def vorticity(sim, gp, k, F, nbs=None):
    """sum_j (m_j / rho_j) F (v_i - v_j) x r_ij over the FLUID neighbours of fluid particles, NaN elsewhere"""
    n = sim.n
    fluid, _ = _types(sim)
    m = sim.pos[:n, 3].astype(np.float64)
    v = sim.vel[:n, :3].astype(np.float64)
    rho, _ = _rho(sim, k)
    nbs = neighbours(sim, gp, k, fluid_only=True) if nbs is None else nbs
    out = np.full((n, 3), np.nan)
    for i in np.where(fluid)[0]:
        nb = nbs[i]
        d = gp[i] - gp[nb]
        f = F(np.sqrt((d*d).sum(axis=1)))*m[nb]/rho[nb]
        out[i] = (f[:, None]*np.cross(v[i] - v[nb], d)).sum(axis=0)
    return out


def _cone_margin(normal, d, r, cos):
    """the largest (criteria - threshold)/threshold over the neighbours, criteria = -normal . r_ij and threshold = r |normal| cos of
    the cone test: <= 0 means that no neighbour lies in the cone (the particle is flagged); |.| small means that the flag hangs on
    the rounding of one comparison"""
    thr = r*np.sqrt((normal*normal).sum())*cos
    return ((-(d @ normal) - thr)/thr).max() if len(r) else -np.inf


def surface(sim, gp, k, W, F, cosf=0.86, cosn=0.5, nbs=None):
    """free-surface detection of the fluid particles -> (normal (n, 4): unit SPH normal and the Shepard sum sum V_j W with the self
    term, NaN elsewhere; margin (n,): _cone_margin, the flag is margin <= 0; length (n,) of the normal before it was normalised -- the
    pair sum itself, which nearly cancels inside the fluid: rounding of a unit normal is to be weighed with it)"""
    n = sim.n
    fluid, _ = _types(sim)
    m = sim.pos[:n, 3].astype(np.float64)
    rho, _ = _rho(sim, k)
    vol = m/rho
    nbs = neighbours(sim, gp, k) if nbs is None else nbs
    W0 = float(W(np.zeros(1))[0])
    normal = np.full((n, 4), np.nan); margin = np.full(n, np.nan); length = np.full(n, np.nan)
    for i in np.where(fluid)[0]:
        nb = nbs[i]
        d = gp[i] - gp[nb]
        r = np.sqrt((d*d).sum(axis=1))
        g = -((F(r)*vol[nb])[:, None]*d).sum(axis=0)
        margin[i] = _cone_margin(g, d, r, np.where(fluid[nb], cosf, cosn))
        length[i] = np.sqrt((g*g).sum())
        normal[i, :3] = g/length[i]
        normal[i, 3] = W0*vol[i] + (W(r)*vol[nb]).sum()
    return normal, margin, length


def interface(sim, gp, k, W, F, cosf=0.86, cosn=0.5, nbs=None):
    """interface detection of a multi-fluid state -> (normal (n, 4) as the kernel stores it: the interface normal for interface
    particles, else the free-surface normal; margin_fs, margin_if: FG_SURFACE is margin_fs <= 0, FG_INTERFACE is margin_if <= 0 <
    margin_fs; length as in surface()).  The second normal leaves out fluid neighbours of ANOTHER fluid"""
    n = sim.n
    fluid, _ = _types(sim)
    fnum = (sim.info[:n, 1] >> 12).astype(np.int64)
    m = sim.pos[:n, 3].astype(np.float64)
    rho, _ = _rho(sim, k)
    vol = m/rho
    nbs = neighbours(sim, gp, k) if nbs is None else nbs
    W0 = float(W(np.zeros(1))[0])
    normal = np.full((n, 4), np.nan); mfs = np.full(n, np.nan); mif = np.full(n, np.nan); length = np.full(n, np.nan)
    for i in np.where(fluid)[0]:
        nb = nbs[i]
        d = gp[i] - gp[nb]
        r = np.sqrt((d*d).sum(axis=1))
        cos = np.where(fluid[nb], cosf, cosn)
        own = (fnum[nb] == fnum[i]) | ~fluid[nb]
        Fr, Wv = F(r), W(r)*vol[nb]
        gfs = -(Fr[:, None]*d).sum(axis=0)*vol[i]
        gif = -(Fr[own][:, None]*d[own]).sum(axis=0)*vol[i]
        mfs[i] = _cone_margin(gfs, d, r, cos)
        mif[i] = _cone_margin(gif, d[own], r[own], cos[own])
        at_if = mif[i] <= 0 < mfs[i]
        g = gif if at_if else gfs
        length[i] = np.sqrt((g*g).sum())
        normal[i, :3] = g/length[i]
        normal[i, 3] = W0*vol[i] + (Wv[own].sum() if at_if else Wv.sum())
    return normal, mfs, mif, length


def testpoints(sim, gp, k, W):
    """Shepard-normalised velocity and pressure of the FLUID neighbours of every test point -> (rows of the test points, (n_tp, 4))"""
    n = sim.n
    p = sim.o.p
    fluid, _ = _types(sim)
    tp = np.where((sim.info[:n, 0] & 7) == D.PT_TESTPOINT)[0]
    fnum = (sim.info[:n, 1] >> 12).astype(np.int64)
    m = sim.pos[:n, 3].astype(np.float64)
    v = sim.vel[:n, :3].astype(np.float64)
    rho, rho0 = _rho(sim, k)
    B = np.array([float(p.bcoeff[f]) for f in range(int(fnum.max()) + 1)])[fnum]
    gam = np.array([float(p.gammacoeff[f]) for f in range(int(fnum.max()) + 1)])[fnum]
    P = B*((rho/rho0)**gam - 1.0)
    tree = cKDTree(gp)
    out = np.zeros((len(tp), 4))
    for a, i in enumerate(tp):
        nb = np.array([j for j in tree.query_ball_point(gp[i], k["R"]*(1 - 1e-7)) if j != i and fluid[j]], dtype=np.int64)
        w = W(np.sqrt(((gp[i] - gp[nb])**2).sum(axis=1)))*m[nb]/rho[nb]
        if w.sum() > 1e-5:
            out[a, :3] = (w[:, None]*v[nb]).sum(axis=0)/w.sum()
            out[a, 3] = (w*P[nb]).sum()/w.sum()
    return tp, out
