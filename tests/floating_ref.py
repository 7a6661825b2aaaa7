"""TEST REFERENCE ONLY: the rule floating bodies are integrated by (DESIGN.md "Floating bodies", csrc/floating.hip), restated in
numpy float64, and FloatingOracleSim, the oracle's whole-step driver with that rule where the reference calls Chrono.

Semi-implicit Euler on an unconstrained body.  State: centre of rotation x, orientation q (unit quaternion w, x, y, z; R(q) turns
body axes into world axes), linear velocity v, angular velocity w in the world frame; constants mass m, principal inertia I.  One
substep, dt1 = dt/2 in the predictor and dt in the corrector, formed in double from the float dt:
  1. step 1 saves (x, q, v, w) as the state of step n, step 2 starts from what was saved
  2. v' = v + dt1 (F/m + g)
  3. wb = R^T w, Tb = R^T T, wb' = wb + dt1 I^-1 (Tb - wb x (I wb)), w' = R wb'
  4. x' = x + dt1 v'
  5. q' = normalize(q * exp(dt1 wb'/2))
  6. slot of the rigid-body table, rounded to float: trans = x' - x, steprot = R(q' * q^-1), linearvel = v', angularvel = w',
     centre of the forces engine = grid cell / local position of x', centre of the integration engine = those of x
The arithmetic is written in the order of the kernel's, so that the two differ by the roundings of sin, cos and sqrt alone."""
import math

import numpy as np

import oracle_lib as ol

STATE = 19          # x 3, q 4, v 3, w 3, total force 3, total torque 3
KEPT = 13


def rotmat(q):
    w, x, y, z = (float(v) for v in q)
    return np.array([[1.0 - 2.0*(y*y + z*z), 2.0*(x*y - w*z), 2.0*(x*z + w*y)],
                     [2.0*(x*y + w*z), 1.0 - 2.0*(x*x + z*z), 2.0*(y*z - w*x)],
                     [2.0*(x*z - w*y), 2.0*(y*z + w*x), 1.0 - 2.0*(x*x + y*y)]], dtype=np.float64)


def qmul(a, b):
    return np.array([a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3],
                     a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2],
                     a[0]*b[2] - a[1]*b[3] + a[2]*b[0] + a[3]*b[1],
                     a[0]*b[3] + a[1]*b[2] - a[2]*b[1] + a[3]*b[0]], dtype=np.float64)


def advance(x, q, v, w, F, T, m, I, g, dt1):
    """steps 2-5 of the rule: (x', q', v', w') and the step rotation R(q' * q^-1)"""
    x, q, v, w, F, T, I, g = (np.asarray(a, dtype=np.float64) for a in (x, q, v, w, F, T, I, g))
    dt1 = float(dt1)
    R = rotmat(q)
    v1 = np.array([v[a] + dt1*(F[a]/m + g[a]) for a in range(3)])
    wb = np.array([R[0, a]*w[0] + R[1, a]*w[1] + R[2, a]*w[2] for a in range(3)])
    Tb = np.array([R[0, a]*T[0] + R[1, a]*T[1] + R[2, a]*T[2] for a in range(3)])
    Iw = I*wb
    gy = np.array([wb[1]*Iw[2] - wb[2]*Iw[1], wb[2]*Iw[0] - wb[0]*Iw[2], wb[0]*Iw[1] - wb[1]*Iw[0]])
    wb1 = np.array([wb[a] + dt1*((Tb[a] - gy[a])/I[a]) for a in range(3)])
    w1 = np.array([R[a, 0]*wb1[0] + R[a, 1]*wb1[1] + R[a, 2]*wb1[2] for a in range(3)])
    x1 = np.array([x[a] + dt1*v1[a] for a in range(3)])
    with np.errstate(invalid="ignore"):
        rate = math.sqrt(wb1[0]*wb1[0] + wb1[1]*wb1[1] + wb1[2]*wb1[2]) if np.isfinite(wb1).all() else float("nan")
        h = 0.5*dt1*rate
        sinc = 1.0 - h*h/6.0 if abs(h) < 1.0e-4 else (math.sin(h)/h if math.isfinite(h) else float("nan"))
        e = np.array([math.cos(h) if math.isfinite(h) else float("nan"), 0.5*dt1*sinc*wb1[0], 0.5*dt1*sinc*wb1[1], 0.5*dt1*sinc*wb1[2]])
        q1 = qmul(q, e)
        nq = np.sqrt(q1[0]*q1[0] + q1[1]*q1[1] + q1[2]*q1[2] + q1[3]*q1[3])
        q1 = q1/nq
        dR = rotmat(qmul(q1, np.array([q[0], -q[1], -q[2], -q[3]])))
    return x1, q1, v1, w1, dR


def grid_and_local(x, origin, cellsize, gridsize):
    """MovingBodies.grid_and_local (gpusph_amd/bodies.py); a non-finite x lands in cell 0 (fmax / fmin drop the NaN)"""
    x, origin, cellsize = (np.asarray(a, dtype=np.float64) for a in (x, origin, cellsize))
    rel = x - origin
    with np.errstate(invalid="ignore"):
        c = np.fmin(np.fmax(np.floor(rel/cellsize), 0.0), np.asarray(gridsize, dtype=np.float64) - 1.0)
        return c.astype(np.int32), (rel - (c + 0.5)*cellsize).astype(np.float32)


def device_grid(problem):
    """world origin, cell size and gravity as the library holds them (floats, widened), and the grid size"""
    f = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)
    return dict(origin=f(problem.m_origin), cellsize=f(problem.m_cellsize), gridsize=np.asarray(problem.m_gridsize, dtype=np.int64),
                gravity=f(problem.physparams.gravity))


class RefBodies:
    """the floating bodies of a problem under the rule: state [n, 19], saved [n, 13]"""

    def __init__(self, bodies, grid):
        self.grid = grid
        self.mass = np.array([float(b.mass) for b in bodies])
        self.inertia = np.array([np.asarray(b.inertia, dtype=np.float64) for b in bodies]).reshape(-1, 3)
        self.state = np.zeros((len(bodies), STATE))
        for k, b in enumerate(bodies):
            q = np.asarray(b.orientation, dtype=np.float64)
            n2 = float(q @ q)
            self.state[k, :KEPT] = np.concatenate([np.asarray(b.crot, dtype=np.float64), q if abs(n2 - 1.0) <= 1e-12 else q/math.sqrt(n2),
                                                   np.asarray(b.lvel, dtype=np.float64), np.asarray(b.avel, dtype=np.float64)])
        self.saved = self.state[:, :KEPT].copy()

    def __len__(self):
        return len(self.mass)

    def substep(self, step, totals, dt):
        """totals [n, 6] (force, torque about the forces engine's centre); dt the float time step.  -> the bodies' slots"""
        assert step in (1, 2)
        dt1 = 0.5*float(np.float32(dt)) if step == 1 else float(np.float32(dt))
        n, g = len(self), self.grid
        out = dict(trans=np.zeros((n, 3), np.float32), rot=np.zeros((n, 9), np.float32), lvel=np.zeros((n, 3), np.float32),
                   avel=np.zeros((n, 3), np.float32), cg_grid=np.zeros((n, 3), np.int32), cg_pos=np.zeros((n, 3), np.float32),
                   cg_grid_e=np.zeros((n, 3), np.int32), cg_pos_e=np.zeros((n, 3), np.float32))
        for b in range(n):
            if step == 1:
                self.saved[b] = self.state[b, :KEPT]
            s = self.saved[b]
            x, q, v, w = s[0:3], s[3:7], s[7:10], s[10:13]
            FT = np.asarray(totals[b], dtype=np.float64)
            x1, q1, v1, w1, dR = advance(x, q, v, w, FT[:3], FT[3:], self.mass[b], self.inertia[b], g["gravity"], dt1)
            self.state[b] = np.concatenate([x1, q1, v1, w1, FT])
            with np.errstate(invalid="ignore", over="ignore"):
                out["trans"][b] = x1 - x
                out["rot"][b] = dR.reshape(9)
                out["lvel"][b] = v1; out["avel"][b] = w1
            out["cg_grid"][b], out["cg_pos"][b] = grid_and_local(x1, g["origin"], g["cellsize"], g["gridsize"])
            out["cg_grid_e"][b], out["cg_pos_e"][b] = grid_and_local(x, g["origin"], g["cellsize"], g["gridsize"])
        return out


ULP = 2.0**-52
ROUNDINGS = 256     # the bound of check_state in ulps.  The longest chain of the rule ends in q': R(q) 5 roundings, wb 5, wb x (I wb) 4,
                    # the update 4, |wb'| 6, h 2, sin(h)/h 2, exp 3, the product 7, the norm 9, the division 1: about 50, under 100,
                    # with sin, cos and sqrt of the device within 2 ulps each on top


def check_totals(got, rbf, rbt, rowstart, where=""):
    """totals summed in double in any order against the exactly rounded sum: n additions of terms t_i are off by at most
    n 2^-52 sum|t_i|"""
    want = fsum_rows(rbf, rbt, rowstart)
    for b in range(len(rowstart) - 1):
        r0, r1 = int(rowstart[b]), int(rowstart[b + 1])
        rows = np.concatenate([rbf[r0:r1, :3], rbt[r0:r1, :3]], axis=1).astype(np.float64)
        bound = (r1 - r0)*ULP*np.abs(rows).sum(axis=0)
        err = np.abs(np.asarray(got[b], dtype=np.float64) - want[b])
        assert (err <= bound).all(), "%s body %d: totals off by %s, bound %s" % (where, b, err, bound)
    return want


def check_state(got, prev, totals, mass, inertia, gravity, dt1, where=""):
    """one body: got[19] against the rule applied to prev[13] and totals[6], each group to ROUNDINGS 2^-52 times the largest
    magnitude that enters it.  Returns the largest error / bound ratio"""
    got, prev, totals, I = (np.asarray(a, dtype=np.float64) for a in (got, prev, totals, inertia))
    x, q, v, w = prev[0:3], prev[3:7], prev[7:10], prev[10:13]
    x1, q1, v1, w1, _ = advance(x, q, v, w, totals[:3], totals[3:], mass, I, gravity, dt1)
    amax = lambda *a: max(float(np.abs(np.asarray(t, dtype=np.float64)).max()) for t in a)
    scales = dict(x=amax(x, x1, dt1*v1), q=1.0, v=amax(v, v1, dt1*totals[:3]/mass, dt1*np.asarray(gravity)),
                  w=amax(w, w1, dt1*totals[3:]/I.min(), dt1*amax(w)**2*I.max()/I.min()))
    worst = 0.0
    for name, sl, want in (("x", slice(0, 3), x1), ("q", slice(3, 7), q1), ("v", slice(7, 10), v1), ("w", slice(10, 13), w1)):
        bound = ROUNDINGS*ULP*max(scales[name], 1e-300)
        err = float(np.abs(got[sl] - want).max())
        assert err <= bound, "%s %s: off by %g, bound %g (%s vs %s)" % (where, name, err, bound, got[sl], want)
        worst = max(worst, err/bound)
    assert np.array_equal(got[13:19], totals), where
    return worst


def slots_from_states(prev, new, grid):
    """the slot the rule's doubles round to: prev[13] the state the substep started from, new[13] the one it made"""
    prev, new = np.asarray(prev, dtype=np.float64), np.asarray(new, dtype=np.float64)
    q, q1 = prev[3:7], new[3:7]
    dR = rotmat(qmul(q1, np.array([q[0], -q[1], -q[2], -q[3]])))
    cg, lp = grid_and_local(new[0:3], grid["origin"], grid["cellsize"], grid["gridsize"])
    cge, lpe = grid_and_local(prev[0:3], grid["origin"], grid["cellsize"], grid["gridsize"])
    return dict(trans=(new[0:3] - prev[0:3]).astype(np.float32), rot=dR.reshape(9).astype(np.float32), lvel=new[7:10].astype(np.float32),
                avel=new[10:13].astype(np.float32), cg_pos=lp, cg_pos_e=lpe, cg_grid=cg, cg_grid_e=cge)


def check_slot(got, want, where=""):
    """got / want: dicts of one body's slot; floats within one float ulp of the larger magnitude, cells equal"""
    for k in ("trans", "rot", "lvel", "avel", "cg_pos", "cg_pos_e"):
        a, b = np.asarray(got[k], dtype=np.float32).ravel(), np.asarray(want[k], dtype=np.float32).ravel()
        ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
        assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= ulp).all(), "%s %s: %s vs %s" % (where, k, a, b)
    for k in ("cg_grid", "cg_grid_e"):
        assert np.array_equal(np.asarray(got[k]).ravel(), np.asarray(want[k]).ravel()), "%s %s" % (where, k)


def fsum_rows(rbf, rbt, rowstart):
    """total force and torque per body, the exactly rounded sums of its float rows: [bodies, 6]"""
    nb = len(rowstart) - 1
    tot = np.zeros((nb, 6))
    for b in range(nb):
        r0, r1 = int(rowstart[b]), int(rowstart[b + 1])
        for k in range(3):
            tot[b, k] = math.fsum(rbf[r0:r1, k].astype(np.float64).tolist())
            tot[b, 3 + k] = math.fsum(rbt[r0:r1, k].astype(np.float64).tolist())
    return tot


class _Bodies:
    """what OracleSim.step asks of `bodies`: the bodies with prescribed motion (if any) behind the floating ones"""

    def __init__(self, n, moving):
        self.n, self.moving = n, moving

    def __len__(self):
        return self.n


class FloatingOracleSim(ol.OracleSim):
    """OracleSim with the floating bodies of the problem moved by the rule: MOVE_BODIES sums self.rbf / self.rbt per body with
    math.fsum, applies the rule, and writes both engines' centres in every substep as the device does."""

    def __init__(self, problem, allocated=None):
        super().__init__(problem, allocated)
        self.fl = RefBodies(problem.floating_bodies, device_grid(problem))
        self.rowstart = np.asarray(problem.rb_rowstart, dtype=np.int64)
        moving = self.bodies      # MovingBodies, when the problem has a callback
        if moving is not None:
            moving.first = len(self.fl)
        self.bodies = _Bodies(len(problem.rb_firstindex), moving)
        self.totals = []          # [bodies, 6] of every substep so far

    def _move_bodies(self, step, dt, t):
        p = self.o.p
        m = None
        if self.bodies.moving is not None:
            m = self.bodies.moving.timestep(step, dt, t)
            for b in range(len(self.fl), self.bodies.n):
                for a in range(3):
                    p.rbtrans[b][a] = float(m["trans"][b][a]); p.rblinearvel[b][a] = float(m["lvel"][b][a])
                    p.rbangularvel[b][a] = float(m["avel"][b][a])
                for a in range(9):
                    p.rbsteprot[b][a] = float(m["rot"][b][a])
        tot = fsum_rows(self.rbf, self.rbt, self.rowstart)
        self.totals.append(tot)
        s = self.fl.substep(step, tot, dt)
        for b in range(len(self.fl)):
            for a in range(3):
                p.rbtrans[b][a] = float(s["trans"][b][a]); p.rblinearvel[b][a] = float(s["lvel"][b][a])
                p.rbangularvel[b][a] = float(s["avel"][b][a])
                p.rbcgGridPos[b][a] = int(s["cg_grid"][b][a]); p.rbcgPos[b][a] = float(s["cg_pos"][b][a])
                p.rbcgGridPosE[b][a] = int(s["cg_grid_e"][b][a]); p.rbcgPosE[b][a] = float(s["cg_pos_e"][b][a])
            for a in range(9):
                p.rbsteprot[b][a] = float(s["rot"][b][a])
        self.last_slots = s
        # what OracleSim.step copies into the integration engine's centres behind the corrector: the floating bodies keep theirs
        # (the centre of step n, written above), the others get the callback's
        self._last_motion = dict(cg_grid=[[int(p.rbcgGridPosE[b][a]) for a in range(3)] for b in range(self.bodies.n)],
                                 cg_pos=[[float(p.rbcgPosE[b][a]) for a in range(3)] for b in range(self.bodies.n)])
        if m is not None:
            for b in range(len(self.fl), self.bodies.n):
                self._last_motion["cg_grid"][b] = [int(v) for v in m["cg_grid"][b]]
                self._last_motion["cg_pos"][b] = [float(v) for v in m["cg_pos"][b]]
