"""What tests/test_sa_postprocess_hostemu.py (the kernels' source on the CPU) and tests/test_gpu_sa_postprocess.py /
tests/test_gpu_wave_gages.py (the device) have in common: the probe tank, the fields the kernels are fed, and the comparisons
of their results with the float64 restatement tests/sa_postprocess_ref.py.  TEST INFRASTRUCTURE.

The bound of a comparison is not a number picked here.  It is 8 x the largest distance between a float32 numpy evaluation of the
restatement and its float64 evaluation over the same rows, and at least 1e-6 of the largest value compared: the margin covers the
order of the neighbour list instead of the rows' and the device's own W and powf."""
import numpy as np

from gpusph_amd import defs as D
from gpusph_amd.problem import SABox, SAProbeBox, info_type
from sa_postprocess_ref import PostRef, gage_levels

DP = 0.05
MARGIN = 1e-4          # rows of the surface decision with a float64 margin below this may be left out (at most 1 % of the fluid rows)


def probes(p):
    """bulk, one deltap off the floor, a corner, the free surface, above the water, outside the tank (in the margin of the domain)"""
    dp = p.m_deltap
    return np.array([[0.5*p.l, 0.5*p.w, 0.5*p.water_level], [0.5*p.l + 0.3*dp, 0.5*p.w, dp], [0.6*dp, 0.7*dp, 0.5*dp],
                     [0.4*p.l, 0.6*p.w, p.water_level - 0.5*dp], [0.5*p.l, 0.5*p.w, p.water_level + 3.2*dp], [-1.5*dp, 0.5*p.w, -1.5*dp]])


def gages_of(p):
    """smoothed gages (mid tank, near a wall, a wide one, over dry ground), nearest-mode gages (mid tank, near a corner)"""
    return [(0.31, 0.26, 0.08), (0.12, 0.4, 0.06), (0.3, 0.25, 0.5), (-5.0, -5.0, 0.08), (0.313, 0.262), (0.081, 0.093)]


def probe_box(jitter=0.0, viscosity="DYNAMICVISC", with_gages=True, **kw):
    p0 = SABox(DP, jitter=jitter, options="Spheric2SA", viscosity=viscosity, **kw)
    return SAProbeBox(DP, jitter=jitter, options="Spheric2SA", viscosity=viscosity, testpoints=probes(p0),
                      gages=gages_of(p0) if with_gages else (), **kw)


def fields(problem, gpos, info, vel0):
    """a sheared velocity on the fluid AND the vertices (what the SA test-point kernel adds), seeded density noise on everybody,
    k and epsilon fields: float32 rows for the state whose global positions are gpos"""
    t = info_type(info)
    n = len(t)
    vel = np.array(vel0, dtype=np.float32, copy=True)
    x, y, z = gpos[:, 0], gpos[:, 1], gpos[:, 2]
    carry = (t == D.PT_FLUID) | (t == D.PT_VERTEX)
    vel[carry, 0] = (0.05*z/problem.H + 0.01*np.sin(7.0*x))[carry]
    vel[carry, 1] = (0.02*x/problem.l)[carry]
    vel[carry, 2] = (-0.03*y/problem.w + 0.02*np.cos(9.0*z))[carry]
    ids = info[:, 2].astype(np.int64) | (info[:, 3].astype(np.int64) << 16)        # noise by particle id: the same in any row order
    noise = np.random.default_rng(5).standard_normal(int(ids.max()) + 1)
    vel[:, 3] += (0.01*noise[ids]).astype(np.float32)
    tke = (1e-3*(1.0 + 0.5*np.sin(5.0*x + 3.0*z))).astype(np.float32)
    eps = (5e-2*(1.0 + 0.3*np.cos(4.0*y))).astype(np.float32)
    return vel, tke, eps


class Restated:
    """the float64 and the float32 evaluation of the restatement on one state: gpos (n, 3) global, info, vel / tke / eps float32 rows"""

    def __init__(self, problem, gpos, info, vel, mass, tke=None, eps=None):
        self.r64 = PostRef(problem, gpos, info)
        self.r32 = PostRef(problem, gpos, info, dtype=np.float32)
        self.args = (vel, mass)
        self.tke, self.eps = tke, eps
        self.fluid_rows = np.where(info_type(info) == D.PT_FLUID)[0]

    @staticmethod
    def bound(v32, v64):
        return max(8.0*float(np.abs(np.asarray(v32, dtype=np.float64) - v64).max()), 1e-6*float(np.abs(v64).max()))

    def check(self, what, got, v32, v64, report):
        b = self.bound(v32, v64)
        err = float(np.abs(np.asarray(got, dtype=np.float64) - v64).max())
        report.append("%s: device %.3g, bound %.3g (float32 numpy %.3g; largest value %.3g)"
                      % (what, err, b, float(np.abs(np.asarray(v32, dtype=np.float64) - v64).max()), float(np.abs(v64).max())))
        print(report[-1])
        assert err <= b, report[-1]

    def testpoints(self, got_vel, got_tke=None, got_eps=None):
        """got_*: the rows of the state after the kernel"""
        report = []
        rows, a, ak, ae, alpha = self.r64.testpoints(*self.args, self.tke, self.eps)
        _, b, bk, be, _ = self.r32.testpoints(*self.args, self.tke, self.eps)
        assert (np.abs(alpha - 1e-5) > 1e-6).all()          # no probe sits on the threshold of the normalisation
        assert (alpha > 1e-5).sum() >= 4 and (alpha <= 1e-5).sum() >= 1
        self.check("test points, velocity", got_vel[rows, :3], b[:, :3], a[:, :3], report)
        self.check("test points, pressure", got_vel[rows, 3], b[:, 3], a[:, 3], report)
        assert not got_vel[rows][alpha <= 1e-5].any()
        if got_tke is not None:
            self.check("test points, k", got_tke[rows], bk, ak, report)
            self.check("test points, epsilon", got_eps[rows], be, ae, report)
            assert not got_tke[rows][alpha <= 1e-5].any() and not got_eps[rows][alpha <= 1e-5].any()
        return rows, report

    def surface(self, info_before, info_after, normals, cosf=0.86, cosn=0.5):
        report = []
        rows, flag, nrm, margin = self.r64.surface(*self.args, cosf, cosn)
        _, flag32, nrm32, _ = self.r32.surface(*self.args, cosf, cosn)
        firm = margin >= MARGIN
        assert (~firm).sum() <= 0.01*len(rows)
        got = (info_after[rows, 0] & D.FG_SURFACE) != 0
        report.append("FG_SURFACE: %d rows flagged of %d fluid rows; %d rows under the margin %g left out; float32 numpy flips %d"
                      % (flag.sum(), len(rows), (~firm).sum(), MARGIN, (flag32 != flag)[firm].sum()))
        print(report[-1])
        assert np.array_equal(got[firm], flag[firm]) and 20 < flag.sum() < len(rows)//2
        # nothing but FG_SURFACE of fluid rows changes
        other = np.ones(len(info_after), dtype=bool); other[rows] = False
        assert np.array_equal(info_after[other], info_before[other])
        assert np.array_equal(info_after[rows] & ~np.uint16(D.FG_SURFACE), info_before[rows] & ~np.uint16(D.FG_SURFACE))
        if normals is not None:
            self.check("surface normals (unit)", normals[rows, :3], nrm32[:, :3], nrm[:, :3], report)
            self.check("surface normals, Shepard sum", normals[rows, 3], nrm32[:, 3], nrm[:, 3], report)
            assert np.isnan(normals[other]).all()
        return rows, flag, report

    def vorticity(self, got):
        report = []
        rows, a = self.r64.vorticity(*self.args)
        _, b = self.r32.vorticity(*self.args)
        self.check("vorticity", got[rows], b, a, report)
        other = np.ones(len(got), dtype=bool); other[rows] = False
        assert np.isnan(got[other]).all()
        return report


def global_pos_f64(problem, pos_local, hash_):
    """the global position as the gage kernel forms it: float cell size and float world origin, widened to double"""
    g = problem.grid_pos_from_hash(np.asarray(hash_))
    cs = problem.m_cellsize.astype(np.float32).astype(np.float64)
    wo = problem.m_origin.astype(np.float32).astype(np.float64)
    return cs*(g + 0.5) + np.asarray(pos_local)[:, :3].astype(np.float64) + wo


def check_gages(problem, pos_local, hash_, info, gages, got, what=""):
    """the levels `got` of `gages` (g, 4) against the rule fed the state's own flags: 1e-12 relative with a smoothing length (double
    sums over a few hundred terms, only the order and FMA contraction differ), exact in nearest mode, NaN / 0 where empty"""
    gages = np.asarray(gages, dtype=np.float64).reshape(-1, 4)
    gp = global_pos_f64(problem, pos_local, hash_)
    surf = ((info[:, 0] & D.FG_SURFACE) != 0) & np.isfinite(np.asarray(pos_local)[:, 3])
    want, two = gage_levels(gp, surf, gages)
    assert got.dtype == np.float64 and got.shape == want.shape
    for k, g in enumerate(gages):
        if g[3] > 0:
            if np.isnan(want[k]):
                assert np.isnan(got[k]), (what, k)
            else:
                assert abs(got[k] - want[k]) <= 1e-12*abs(want[k]), (what, k, got[k], want[k])
        elif surf.any():
            assert two[k, 1] - two[k, 0] > 1e-9*two[k, 1], "gage %d has two nearest particles: move it" % k
            assert got[k] == want[k], (what, k, got[k], want[k])
        else:
            assert got[k] == 0.0
    print("gages %s: %s" % (what, " ".join("%.12g" % v for v in got)))
    return want
