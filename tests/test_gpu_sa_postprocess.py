"""Post-processing with SA walls on the GPU: test points (with k and epsilon in a k-epsilon run), surface detection and vorticity of
SAProbeBox(0.05, options="Spheric2SA") -- 2 297 particles and six probes: in the bulk, one deltap off the floor, in a corner, at
the free surface, above the water and outside the tank -- against the float64 all-pairs restatement (tests/sa_postprocess_ref.py).

Bounds (tests/sa_postprocess_cases.py): 8 x the largest distance between a float32 numpy evaluation of the restatement and its
float64 evaluation over the same rows, at least 1e-6 of the largest value; FG_SURFACE exactly on every fluid row whose float64
decision margin is at least 1e-4 (every row of both tanks).  Every comparison prints the device's distance next to its bound.
Measured on the MI355X (jitter 0 / 0.1), device distance (bound):
    vorticity                6.7e-8 (8.6e-7) / 8.6e-8 (9.1e-7)       of values up to 0.15
    surface normals, unit    2.0e-4 (9.9e-4) / 1.1e-5 (6.2e-5)       Shepard sum 9.3e-7 (4.6e-6) / 8.4e-7 (4.4e-6) of 1.85
    FG_SURFACE               equal on all 594 fluid rows, 63 / 50 flagged; no row under the margin, float32 numpy flips none
    test points, velocity    1.3e-8 (5.1e-8) / 3.3e-9 (5.2e-8)       of 0.05; pressure 0.010 (0.065) of 1.08e4 Pa
    test points, k, epsilon  2.8e-10 (2.5e-9), 1.3e-8 (6.5e-8)       (jitter 0.1, KEPSVISC)
Without the feature every SA post-process call raises SphxUnsupported."""
import numpy as np
import pytest

from gpusph_amd import capi, defs as D
from gpusph_amd.problem import DamBreak3D, SABox, info_type
from sa_helpers import assert_close_but_for_gamma_spikes, list_sections
import sa_postprocess_cases as cases

pytestmark = pytest.mark.gpu


def _np(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _engine(problem, **kw):
    import torch
    from gpusph_amd.engine import TimestepEngine
    assert torch.cuda.is_available()
    return TimestepEngine(problem, device="cuda:0", **kw)


def _tiles_usable(eng):
    return int(eng.k.lib.sphx_dbg_tiles_usable(eng.k.ctx.handle))


class _Case:
    """the probe tank on the device with its list built, the fields of tests/sa_postprocess_cases.py in its rows, the restatement"""

    def __init__(self, jitter, viscosity="DYNAMICVISC"):
        import torch
        self.eng = eng = _engine(cases.probe_box(jitter, viscosity))
        eng.build_neibs()
        self.n = n = eng.n
        self.pos, self.hash = _np(eng.pos)[:n].copy(), _np(eng.hash, np.uint32)[:n].copy()
        self.info = _np(eng.info)[:n].view(np.uint16).reshape(-1, 4).copy()
        self.gpos = eng.problem.global_pos(self.pos, self.hash)
        self.vel, self.tke, self.eps = cases.fields(eng.problem, self.gpos, self.info, _np(eng.vel)[:n])
        eng.vel[:n] = torch.from_numpy(self.vel).to(eng.device)
        if eng.keps:
            eng.ke["tke"][:n] = torch.from_numpy(self.tke).to(eng.device)
            eng.ke["eps"][:n] = torch.from_numpy(self.eps).to(eng.device)
        self.ref = cases.Restated(eng.problem, self.gpos, self.info, self.vel, self.pos[:, 3], self.tke, self.eps)


@pytest.fixture(scope="module", params=[0.0, 0.1])
def case(request):
    return _Case(request.param)


def test_list_of_the_test_point_rows_on_the_device(case):
    """the device's list of a test-point row holds exactly the fluid particles and the vertices within the influence radius (as sets,
    against brute force; a pair within rounding of the radius may fall on either side), and nobody lists a test point"""
    eng, n = case.eng, case.n
    p = eng.problem
    st = dict(problem=p, n=eng.alloc, nl=_np(eng.neibslist, np.uint16), hash=case.hash, cs=_np(eng.cellStart, np.uint32))
    t = info_type(case.info)
    R = float(np.float32(p.simparams.influenceRadius))
    rows = np.where(t == D.PT_TESTPOINT)[0]
    assert len(rows) == 6
    seen = 0
    for i in rows:
        fl, bd, vx = list_sections(st, i)
        r = np.sqrt(((case.gpos - case.gpos[i])**2).sum(axis=1))
        edge = np.abs(r - R) < 1e-6*R
        for got, typ in ((fl, D.PT_FLUID), (vx, D.PT_VERTEX)):
            want = set(np.where((t == typ) & (r < R) & ~edge)[0])
            assert want <= set(got) <= want | set(np.where((t == typ) & edge)[0]) and len(set(got)) == len(got)
            seen += len(got)
        assert all(t[j] == D.PT_BOUNDARY for j in bd)
    assert seen > 200
    for i in np.where(t != D.PT_TESTPOINT)[0][::23]:
        assert all(t[j] != D.PT_TESTPOINT for s in list_sections(st, i) for j in s)


def test_vorticity(case):
    case.ref.vorticity(_np(case.eng.postprocess(D.VORTICITY)))


def test_surface_detection(case):
    import torch
    eng, n = case.eng, case.n
    nrm = _np(eng.postprocess(D.SURFACE_DETECTION, normals=True))
    after = _np(eng.info)[:n].view(np.uint16).reshape(-1, 4).copy()
    case.ref.surface(case.info, after, nrm)
    eng.info[:n, 0] |= D.FG_SURFACE                     # stale flags are cleared; without the normals
    assert eng.postprocess(D.SURFACE_DETECTION) is None
    fl = info_type(case.info) == D.PT_FLUID
    assert np.array_equal(_np(eng.info)[:n].view(np.uint16).reshape(-1, 4)[fl], after[fl])
    eng.info[:n] = torch.from_numpy(case.info.view(np.int16)).to(eng.device)


def test_test_points(case):
    import torch
    eng, n = case.eng, case.n
    eng.postprocess(D.TESTPOINTS)
    got = _np(eng.vel)[:n].copy()
    rows, _ = case.ref.testpoints(got)
    other = np.ones(n, dtype=bool); other[rows] = False
    assert np.array_equal(_bits(got[other]), _bits(case.vel[other]))
    eng.vel[:n] = torch.from_numpy(case.vel).to(eng.device)


def test_test_points_of_the_k_epsilon_set():
    """viscosity="KEPSVISC": k and epsilon at the probes; the velocity rows are those of the call without the k-epsilon buffers, bit
    for bit"""
    import torch
    c = _Case(0.1, "KEPSVISC")
    eng, n = c.eng, c.n
    assert eng.keps
    eng.k.postprocess(D.TESTPOINTS, None, eng.vel, None, None, eng.pos, eng.vel, eng.info, eng.hash, eng.cellStart, eng.neibslist, n, 0.86, 0.5)
    plain = _np(eng.vel)[:n].copy()
    eng.vel[:n] = torch.from_numpy(c.vel).to(eng.device)
    eng.postprocess(D.TESTPOINTS)
    got, tke, eps = _np(eng.vel)[:n].copy(), _np(eng.ke["tke"])[:n].copy(), _np(eng.ke["eps"])[:n].copy()
    assert np.array_equal(_bits(got), _bits(plain))
    rows, _ = c.ref.testpoints(got, tke, eps)
    other = np.ones(n, dtype=bool); other[rows] = False
    assert np.array_equal(tke[other], c.tke[other]) and np.array_equal(eps[other], c.eps[other])


def test_still_refused(case):
    eng, n = case.eng, case.n
    with pytest.raises(capi.SphxUnsupported, match="INTERFACE_DETECTION"):
        eng.postprocess(D.INTERFACE_DETECTION)
    for ft in (D.SHEPARD_FILTER, D.MLS_FILTER):
        with pytest.raises(capi.SphxUnsupported, match="only LJ/DYN boundaries are built"):
            eng.apply_filter(ft)
    assert np.array_equal(_np(eng.info)[:n].view(np.uint16).reshape(-1, 4), case.info)


def _slosh(eng):
    import torch
    n, p = eng.n, eng.problem
    g = p.global_pos(_np(eng.pos)[:n], _np(eng.hash, np.uint32)[:n])
    fl = info_type(_np(eng.info)[:n].view(np.uint16).reshape(-1, 4)) == D.PT_FLUID
    v = _np(eng.vel)[:n].copy()
    v[fl, 0] = 0.3*np.sin(np.pi*g[fl, 0]/p.l)*(g[fl, 2]/p.H)
    v[fl, 2] = -0.15*np.cos(np.pi*g[fl, 0]/p.l)*(g[fl, 2]/p.H)
    eng.vel[:n] = torch.from_numpy(v.astype(np.float32)).to(eng.device)


def test_six_steps_with_and_without_probes():
    """probes are inert: the tank's own particles end where those of the SABox without probes end, to the trajectory tolerances of
    tests/test_gpu_sa.py (tiled against list walkers); both runs take the tiled window and the wall kernels in every step; the
    probes stay where they were put, and read a pressure after the run"""
    out = {}
    for probes in (True, False):
        p = cases.probe_box(0.1) if probes else SABox(cases.DP, jitter=0.1, options="Spheric2SA")
        p.simparams.buildneibsfreq = 4
        eng = _engine(p)
        _slosh(eng)
        usable = []
        for _ in range(6):
            eng.step()
            usable.append(_tiles_usable(eng))
        assert usable == [1]*6
        n = eng.n
        info = _np(eng.info)[:n].view(np.uint16).reshape(-1, 4)
        ids = info[:, 2].astype(np.int64) | (info[:, 3].astype(np.int64) << 16)
        gpos = p.global_pos(_np(eng.pos)[:n], _np(eng.hash, np.uint32)[:n])
        out[probes] = dict(ids=ids, t=info_type(info), gpos=gpos, vel=_np(eng.vel)[:n].copy(), gg=_np(eng.gradgamma)[:n].copy(),
                           dt=eng.current_dt(), cell=float(np.min(p.m_cellsize)), eng=eng, p=p)
    a, b = out[True], out[False]
    tank = a["t"] != D.PT_TESTPOINT
    oa, ob = np.argsort(a["ids"][tank]), np.argsort(b["ids"])
    assert np.array_equal(a["ids"][tank][oa], b["ids"][ob]) and (~tank).sum() == 6
    pa, pb = a["gpos"][tank][oa], b["gpos"][ob]
    va, vb = a["vel"][tank][oa], b["vel"][ob]
    assert np.isfinite(va).all() and np.isfinite(vb).all()
    vmax = np.abs(vb[:, :3]).max()
    assert vmax > 0.2
    assert_close_but_for_gamma_spikes(pa, pb, 2e-5, b["cell"], frac=0.002, spike=2.0, what="positions, with against without probes")
    assert_close_but_for_gamma_spikes(va[:, :3], vb[:, :3], 2e-4, vmax, frac=2e-3, spike=15.0, what="velocities, with against without probes")
    assert_close_but_for_gamma_spikes(va[:, 3], vb[:, 3], 2e-6, 1.0, frac=0.002, spike=4.0, what="densities, with against without probes")
    fl = b["t"][ob] == D.PT_FLUID
    assert np.abs(a["gg"][tank][oa][fl, 3] - b["gg"][ob][fl, 3]).max() < 2e-5
    assert abs(a["dt"] - b["dt"]) < 1e-4*b["dt"]
    # the probes did not move
    tp = np.where(~tank)[0]
    order = np.argsort(a["ids"][tp])
    assert np.abs(a["gpos"][tp][order] - cases.probes(a["p"])).max() < 1e-6
    eng = a["eng"]
    eng.postprocess(D.TESTPOINTS)
    pr = _np(eng.vel)[:eng.n][tp][order]
    rho_g_d = 1000.0*9.81*(a["p"].water_level - cases.probes(a["p"])[0, 2])
    assert 0.5*rho_g_d < pr[0, 3] < 1.5*rho_g_d and not pr[4].any()          # hydrostatic in the bulk, zeros above the water


def test_a_dyn_context_runs_the_kernels_it_ran():
    """DamBreak3D (DYN_BOUNDARY): surface detection and test points against the CPU oracle's non-SA kernels, bit for bit.  How this
    sees which instantiation was launched: the SA variants also walk the list from slot neibboundpos + 1 upwards as a vertex
    section; a DYN list has no such slot (the walker clamps to the last slot, where the boundary section begins), so an SA
    variant on this context would count the first boundary neighbours twice and lose bit equality"""
    import torch
    import oracle_lib as ol
    pts = [(0.2, 0.3, 0.2), (0.25, 0.35, 0.1), (1.2, 0.3, 0.3)]
    prob = DamBreak3D(deltap=0.05, obstacle=False, jitter=0.1, hydrostatic=False, testpoints=pts)
    assert prob.simparams.neibboundpos == prob.simparams.neiblistsize - 1
    eng = _engine(prob, clobber_neibslist=True)
    sim = ol.OracleSim(prob)
    sim.build_neibs(); eng.build_neibs()
    n = eng.n
    rng = np.random.default_rng(9)
    vel = sim.vel.copy()
    vel[:, :3] += rng.uniform(-0.4, 0.4, size=(len(vel), 3)).astype(np.float32)
    vel[:, 3] += rng.uniform(0, 2e-3, size=len(vel)).astype(np.float32)
    sim.vel = vel
    eng.vel[:n] = torch.from_numpy(vel[:n]).to(eng.device)
    ref_info, ref_nrm = sim.o.surface(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, normals=True)
    nrm = _np(eng.postprocess(D.SURFACE_DETECTION, normals=True))
    assert np.array_equal(_np(eng.info, np.uint16)[:n], ref_info[:n]) and ((ref_info[:n, 0] & D.FG_SURFACE) != 0).sum() > 10
    assert np.array_equal(_bits(nrm), _bits(ref_nrm[:n]))
    ref_vel = sim.o.testpoints(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n)
    eng.postprocess(D.TESTPOINTS)
    tp = info_type(sim.info[:n]) == D.PT_TESTPOINT
    assert tp.sum() == 3 and np.array_equal(_bits(_np(eng.vel)[:n][tp, :3]), _bits(ref_vel[:n][tp, :3]))
