"""Known answers of the float64 restatement tests/sa_postprocess_ref.py (test points, surface detection, vorticity with SA walls,
the wave-gage rule), which the device kernels are then held to (tests/test_gpu_sa_postprocess.py, tests/test_gpu_wave_gages.py),
the Python surface of the feature that needs no device, and the neighbour list of test-point rows of an SA mirror (the CPU oracle's
build) as sets against brute force."""
import numpy as np
import pytest

from gpusph_amd import capi, commonwriter, defs as D
from gpusph_amd.problem import DamBreak3D, SABox, SAProbeBox, WaveTank, info_type
from sa_postprocess_ref import PostRef, gage_levels, wendland2d

DP = 0.05


def probes(p):
    """bulk, one deltap off the floor, a corner, the free surface, above the water, outside the tank"""
    dp = p.m_deltap
    return np.array([[0.5*p.l, 0.5*p.w, 0.5*p.water_level], [0.5*p.l + 0.3*dp, 0.5*p.w, dp], [0.6*dp, 0.7*dp, 0.5*dp],
                     [0.4*p.l, 0.6*p.w, p.water_level - 0.5*dp], [0.5*p.l, 0.5*p.w, p.water_level + 3.2*dp], [-1.5*dp, 0.5*p.w, -1.5*dp]])


@pytest.fixture(scope="module")
def box():
    p = SABox(DP)
    return p, PostRef(p, p.parts.pos_global, p.parts.info)


def test_python_surface_of_the_feature():
    assert "sphx_wave_gages" in capi.SIGNATURES and "sphx_postprocess_testpoints_keps" in capi.SIGNATURES
    p0 = SABox(DP, options="Spheric2SA")
    p = SAProbeBox(DP, options="Spheric2SA", testpoints=probes(p0), gages=[(0.3, 0.25), (0.2, 0.2, 0.08)])
    n0 = p0.num_particles
    assert p.num_particles == n0 + 6 and p.num_testpoints == 6 and n0 == 2297
    assert (info_type(p.parts.info)[n0:] == D.PT_TESTPOINT).all()
    for k in ("pos_global", "vel", "info"):      # the tank's own rows are the SABox's
        assert np.array_equal(getattr(p.parts, k)[:n0], getattr(p0.parts, k))
    a = p.copy_to_array()
    assert all(len(a[k]) == n0 + 6 for k in ("pos", "vel", "info", "hash", "vertices", "boundelements", "gradgamma"))
    assert p.gages == [[0.3, 0.25, 0.0, 0.0], [0.2, 0.2, 0.0, 0.08]]
    assert SABox(DP).gages == [] and DamBreak3D(0.05).gages == [] and WaveTank(0.05).gages == []      # defaults untouched
    with pytest.raises(ValueError):
        SAProbeBox(DP, testpoints=[[9.0, 0.0, 0.0]])
    with pytest.raises(ValueError):
        p.add_gage(0.0, 0.0, -1.0)


def test_writer_layout():
    assert commonwriter.wave_gage_header(3) == "time\tzgage0\tzgage1\tzgage2\n"
    assert commonwriter.wave_gage_line(0.5, [0.3250000001234, float("nan"), 0.0]) == "0.5\t0.325\tnan\t0\n"
    assert commonwriter.wave_gage_line(1.0/3.0, [1.0e-5/3.0]) == "0.333333333\t3.33333333e-06\n"


def test_uniform_field_reads_back_at_every_test_point_with_fluid_in_reach():
    p0 = SABox(DP, jitter=0.1)
    p = SAProbeBox(DP, jitter=0.1, testpoints=probes(p0))
    ref = PostRef(p, p.parts.pos_global, p.parts.info)
    n = p.num_particles
    u = np.array([0.3, -0.2, 0.1])
    vel = np.zeros((n, 4)); vel[:, :3] = u; vel[:, 3] = 0.01
    k, e = np.full(n, 2.5e-3), np.full(n, 7.0e-2)
    rows, v4, tk, ep, alpha = ref.testpoints(vel, p.parts.pos_global[:, 3], k, e)
    assert list(rows) == list(range(n - 6, n))
    got = alpha > 1e-5
    # (the probe outside the tank, in the margin of the domain, has no fluid but the walls' vertices in reach: they carry the field too)
    assert list(got) == [True, True, True, True, False, True]
    P = ref.P(np.array([0.01]))[0]
    assert np.abs(v4[got, :3] - u).max() < 1e-13 and np.abs(v4[got, 3] - P).max() < 1e-9*P
    assert np.abs(tk[got] - 2.5e-3).max() < 1e-15 and np.abs(ep[got] - 7.0e-2).max() < 1e-14
    assert not v4[~got].any() and not tk[~got].any() and not ep[~got].any()      # nothing in reach: zeros
    assert 0.95 < alpha[0] < 1.05 and alpha[2] < 0.8*alpha[0]                    # the bulk has a full support, the corner has not


def test_vertices_count_at_a_test_point_near_a_wall():
    """what the SA instantiation adds: the probe one deltap off the floor reads the vertices' velocity too"""
    p0 = SABox(DP)
    p = SAProbeBox(DP, testpoints=probes(p0))
    ref = PostRef(p, p.parts.pos_global, p.parts.info)
    n = p.num_particles
    t = info_type(p.parts.info)
    vel = np.zeros((n, 4)); vel[t == D.PT_FLUID, 0] = 1.0          # the walls' vertices stand still
    _, v4, _, _, _ = ref.testpoints(vel, p.parts.pos_global[:, 3])
    assert abs(v4[0, 0] - 1.0) < 1e-13 and 0.5 < v4[1, 0] < 0.95 and 0.2 < v4[2, 0] < v4[1, 0]


def test_rigid_rotation(box):
    p, ref = box
    n = p.num_particles
    om = np.array([0.3, -0.5, 0.8])
    x = p.parts.pos_global[:, :3]
    vel = np.zeros((n, 4)); vel[:, :3] = np.cross(om, x - x.mean(axis=0))
    rows, vort = ref.vorticity(vel, p.parts.pos_global[:, 3])
    # sum_j F V_j (om x r) x r = (M - tr M) om with M = sum_j F V_j r (x) r, the SPH normalisation of a gradient: M = -1 for a full
    # support, so the bulk reads 2 om (the reference sums (v_i - v_j) x r_ij F: its sign convention), less where the support is cut
    dp = p.m_deltap
    g = x[rows]
    bulk = (np.abs(g[:, 0] - 0.5*p.l) < 1.1*dp) & (np.abs(g[:, 1] - 0.5*p.w) < 1.1*dp) & (np.abs(g[:, 2] - 0.15) < 1.1*dp)
    assert bulk.sum() >= 4
    ratio = vort[bulk]/(2.0*om)
    assert ((ratio > 0.94) & (ratio < 1.0)).all(), ratio          # + 2 om, a little short of it: the lattice sum for M is not quite -1
    full = np.ptp(ratio, axis=1) < 1e-9                            # rows whose support the floor does not cut: M is isotropic
    assert full.sum() >= 4 and np.abs(ratio[full] - ratio[full][0, 0]).max() < 1e-9 and 0.97 < ratio[full][0, 0] < 0.99


def test_surface_of_the_unjittered_tank_and_a_gage_over_it(box):
    p, ref = box
    n = p.num_particles
    rows, flag, nrm, margin = ref.surface(p.parts.vel, p.parts.pos_global[:, 3])
    z = p.parts.pos_global[rows, 2]
    top = np.abs(z - z.max()) < 1e-9
    assert top.sum() == 99
    assert not flag[~top].any()                 # no row below the top layer is flagged
    assert flag[top].sum() == 63                # the rest sit under the walls' non-fluid cone
    x = p.parts.pos_global[rows, :2]
    dp = p.m_deltap
    inner = (x[:, 0] > 1.5*dp) & (x[:, 0] < p.l - 1.5*dp) & (x[:, 1] > 1.5*dp) & (x[:, 1] < p.w - 1.5*dp)
    assert flag[top & inner].all() and not flag[top & ~inner].any()
    assert margin.min() > 1e-4
    assert np.abs(nrm[flag, 2]).min() > 0.99    # the flagged rows' normals point along z
    surf = np.zeros(n, dtype=bool); surf[rows[flag]] = True
    lev, two = gage_levels(p.parts.pos_global[:, :3], surf, [[0.3, 0.25, 0, 0.08], [0.31, 0.26, 0, 0.0], [0.3, 0.25, 0, 2.0]])
    assert np.abs(lev - z.max()).max() < 1e-12 and two[1, 1] > two[1, 0]
    # over dry ground: NaN with a smoothing length, 0 without a single surface particle
    lev, _ = gage_levels(p.parts.pos_global[:, :3], surf, [[-5.0, -5.0, 0, 0.08]])
    assert np.isnan(lev[0])
    lev, _ = gage_levels(p.parts.pos_global[:, :3], np.zeros(n, dtype=bool), [[0.3, 0.25, 0, 0.0], [0.3, 0.25, 0, 0.08]])
    assert lev[0] == 0.0 and np.isnan(lev[1])


def test_gage_rule_pieces():
    assert abs(wendland2d(0.0, 0.1) - 7.0/(4.0*np.pi*0.01)) < 1e-12 and wendland2d(0.2, 0.1) == 0.0
    pos = np.array([[0.0, 0.0, 1.0], [0.1, 0.0, 2.0], [-0.1, 0.0, 3.0], [0.0, 0.3, 9.0]])
    lev, two = gage_levels(pos, np.ones(4, dtype=bool), [[0.05, 0.0, 0, 0.0], [0.0, 0.0, 0, 0.1], [0.05, 0.0, 0, 0.1]])
    assert lev[0] == 1.0 and two[0, 0] == two[0, 1]                 # rows 0 and 1 are equally near: the lower row wins
    w = wendland2d(0.1, 0.1)
    assert abs(lev[1] - (1.0*wendland2d(0.0, 0.1) + 5.0*w)/(wendland2d(0.0, 0.1) + 2*w)) < 1e-14
    w0, w1 = wendland2d(0.05, 0.1), wendland2d(0.15, 0.1)
    assert abs(lev[2] - (1.0*w0 + 2.0*w0 + 3.0*w1)/(2*w0 + w1)) < 1e-14
    lev, _ = gage_levels(pos, np.array([False, True, False, False]), [[0.0, 0.0, 0, 0.0]])
    assert lev[0] == 2.0                                             # only flagged particles count


@pytest.mark.parametrize("jitter", [0.0, 0.1])
def test_margins_of_the_surface_decision(jitter):
    """the GPU test compares FG_SURFACE exactly on rows whose float64 margin is at least 1e-4: that is every row of both tanks, and a
    float32 evaluation flips none"""
    p = SABox(DP, jitter=jitter, options="Spheric2SA")
    out = {}
    for dt in (np.float64, np.float32):
        ref = PostRef(p, p.parts.pos_global, p.parts.info, dtype=dt)
        out[dt] = ref.surface(p.parts.vel, p.parts.pos_global[:, 3])
    assert (out[np.float64][3] < 1e-4).sum() == 0
    assert np.array_equal(out[np.float64][1], out[np.float32][1])
    assert 40 < out[np.float64][1].sum() < 110


@pytest.mark.parametrize("jitter", [0.0, 0.1])
def test_list_of_a_test_point_row_holds_its_fluid_and_vertex_neighbours(jitter):
    """No SA mirror had test-point rows before SAProbeBox: the list of such a row (the CPU oracle's build, which the device's list
    is bit-compared with in tests/test_gpu_sa_postprocess.py) holds exactly the fluid particles and the vertices within the
    influence radius, as sets, against brute force; every other row's list is the one of the tank without probes"""
    from sa_helpers import list_sections, sa_oracle_state
    p0 = SABox(DP, jitter=jitter, options="Spheric2SA")
    st0 = sa_oracle_state(p0)
    p = SAProbeBox(DP, jitter=jitter, options="Spheric2SA", testpoints=probes(p0))
    st = sa_oracle_state(p)
    n = st["n"]
    g = p.global_pos(st["pos"][:n], st["hash"][:n])
    t = info_type(st["info"][:n])
    R = float(np.float32(p.simparams.influenceRadius))
    rows = np.where(t == D.PT_TESTPOINT)[0]
    assert len(rows) == 6
    seen = 0
    for i in rows:
        fl, bd, vx = list_sections(st, i)
        r = np.sqrt(((g - g[i])**2).sum(axis=1))
        edge = np.abs(r - R) < 1e-6*R          # a pair within rounding of the radius may fall on either side
        for got, typ in ((fl, D.PT_FLUID), (vx, D.PT_VERTEX)):
            want = set(np.where((t == typ) & (r < R) & ~edge)[0])
            maybe = set(np.where((t == typ) & edge)[0])
            assert want <= set(got) <= want | maybe and len(set(got)) == len(got)
            seen += len(got)
        assert all(t[j] == D.PT_BOUNDARY for j in bd)
    assert seen > 200
    # nobody lists a test point, and the tank's own rows keep their lists
    ids = lambda s, rows_: (s["info"][rows_, 2].astype(np.uint32) | (s["info"][rows_, 3].astype(np.uint32) << 16))
    row0 = {int(v): k for k, v in enumerate(ids(st0, np.arange(st0["n"])))}
    for i in np.where(t != D.PT_TESTPOINT)[0][::37]:
        a = [sorted(int(v) for v in ids(st, np.array(s, dtype=np.int64))) for s in list_sections(st, i)]
        i0 = row0[int(ids(st, np.array([i]))[0])]
        b = [sorted(int(v) for v in ids(st0, np.array(s, dtype=np.int64))) for s in list_sections(st0, i0)]
        assert a == b
