"""Floating bodies on the device (csrc/floating.hip, sphx_floating_setup / _move / _state): the totals of the bodies' rows, the rule
against its float64 restatement (tests/floating_ref.py), determinism, host uploads that leave the device's slots alone, free fall,
a run beside the oracle, a step without a host read, HotFile resume, and what is refused.  BuoyancyBox(deltap=0.05) is 16 k
particles; every test takes seconds.  Without the feature the entry points and BuoyancyBox do not exist."""
import numpy as np
import pytest
import torch

import floating_ref as fr
import oracle_lib as ol
from gpusph_amd import capi, defs as D, hotfile
from gpusph_amd.bodies import FloatingBody, box_inertia
from gpusph_amd.problem import BuoyancyBox
from forces_check import _engine

pytestmark = pytest.mark.gpu
DP = 0.05


# ---- the kernels by themselves: HipKernels of a small problem, synthetic rows
@pytest.fixture(scope="module")
def small():
    return BuoyancyBox(deltap=0.1)


def _kernels(problem):
    from gpusph_amd.kernels import HipKernels
    return HipKernels(problem, len(problem.parts.info), "cuda:0")


def _bodies(n, rng):
    out = []
    for b in range(n):
        q = rng.normal(size=4)
        m = 20.0 + 10.0*b
        out.append(FloatingBody(mass=m, inertia=box_inertia(m, (0.4, 0.3 + 0.1*b, 0.5)), crot=np.array([0.5, 0.4, 0.3]) + 0.1*b,
                                orientation=q/np.linalg.norm(q), lvel=rng.normal(size=3)*0.3, avel=rng.normal(size=3)*2.0))
    return out


def _rows(n, rng, scale=5.0):
    """float rows of mixed sign and very mixed size; the fourth component is never part of a sum"""
    f = (rng.normal(size=(n, 4))*scale*10.0**rng.integers(-3, 3, size=(n, 1))).astype(np.float32)
    t = (rng.normal(size=(n, 4))*scale*10.0**rng.integers(-3, 3, size=(n, 1))).astype(np.float32)
    f[:, 3] = 1e30; t[:, 3] = -1e30
    return f, t


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.parametrize("counts", [(1,), (65,), (70000,), (16385, 300)])
def test_totals_against_fsum(small, counts):
    """n double additions of float terms in any order are within n 2^-52 sum|term| of the exactly rounded sum; 70 000 rows are more
    than four rounds of a body's 64 blocks, 16 385 one row more than one round"""
    rng = np.random.default_rng(sum(counts))
    K = _kernels(small)
    bodies = _bodies(len(counts), rng)
    rowstart = np.concatenate([[2], 2 + np.cumsum(counts)]).astype(np.uint32)
    rbf, rbt = _rows(int(rowstart[-1]) + 9, rng)
    rbf[int(rowstart[-1]):, :3] = 7e9                        # rows behind the last body: never counted
    K.floating_setup(bodies, rowstart)
    K.floating_move(_dev(rbf), _dev(rbt), 1, _dev(np.array([3e-4], dtype=np.float32)))
    state = K.floating_state()
    fr.check_totals(state[:, 13:19], rbf, rbt, rowstart, "counts %s" % (counts,))
    assert np.abs(state[:, 13:19]).max() < 1e9 and np.abs(state[:, 13:19]).min() > 0


def test_the_rule_against_its_float64_restatement(small):
    """steps 1, 2, 1 of two bodies: the device's state against the rule applied to the device's own totals, to 256 2^-52 of the
    largest magnitude entering each quantity (floating_ref.ROUNDINGS: about 50 roundings on the longest chain, sin, cos and sqrt
    within 2 ulps each); the float slot against float32 of the rule's doubles to one ulp"""
    rng = np.random.default_rng(3)
    K = _kernels(small)
    grid = fr.device_grid(small)
    bodies = _bodies(2, rng)
    rowstart = np.array([0, 1234, 3000], dtype=np.uint32)
    K.floating_setup(bodies, rowstart)
    ref = fr.RefBodies(bodies, grid)
    s0, slots0 = K.floating_state(slots=True)
    assert np.array_equal(s0[:, :13].view(np.uint64), ref.state[:, :13].view(np.uint64)) and not s0[:, 13:].any()
    assert np.array_equal(slots0["rot"], np.tile(np.eye(3, dtype=np.float32).ravel(), (2, 1))) and not slots0["trans"].any()
    worst = 0.0
    for step, dt in ((1, 3e-4), (2, 3e-4), (1, 2.5e-4)):
        rbf, rbt = _rows(3000, rng)
        prev = ref.state[:, :13].copy() if step == 1 else ref.saved.copy()
        K.floating_move(_dev(rbf), _dev(rbt), step, _dev(np.array([dt], dtype=np.float32)))
        state, slots = K.floating_state(slots=True)
        fr.check_totals(state[:, 13:19], rbf, rbt, rowstart)
        dt1 = 0.5*float(np.float32(dt)) if step == 1 else float(np.float32(dt))
        for b in range(2):
            worst = max(worst, fr.check_state(state[b], prev[b], state[b, 13:19], bodies[b].mass, bodies[b].inertia, grid["gravity"], dt1,
                                              "step %d body %d" % (step, b)))
            fr.check_slot({k: v[b] for k, v in slots.items()}, fr.slots_from_states(prev[b], state[b, :13], grid), "step %d body %d" % (step, b))
        ref.substep(step, state[:, 13:19], dt)
        ref.state[:, :13] = state[:, :13]
    print("largest error / bound of the device's state against the rule: %.3g" % worst)


def test_same_inputs_same_bits_and_another_bodys_rows_do_not_matter(small):
    rng = np.random.default_rng(7)
    bodies = _bodies(2, rng)
    rowstart = np.array([0, 20000, 41000], dtype=np.uint32)
    rbf, rbt = _rows(41000, rng)
    d_dt = _dev(np.array([3e-4], dtype=np.float32))
    got = []
    for variant in range(3):
        f, t = rbf.copy(), rbt.copy()
        if variant == 2:
            f[20000:], t[20000:] = _rows(21000, np.random.default_rng(8))
        K = _kernels(small)
        K.floating_setup(bodies, rowstart)
        for step in (1, 2):
            K.floating_move(_dev(f), _dev(t), step, d_dt)
        got.append(K.floating_state(slots=True))
    assert np.array_equal(got[0][0].view(np.uint64), got[1][0].view(np.uint64))
    assert np.array_equal(got[0][0][0].view(np.uint64), got[2][0][0].view(np.uint64)) and not np.array_equal(got[0][0][1], got[2][0][1])
    for k in got[0][1]:
        assert np.array_equal(got[0][1][k].view(np.uint32), got[1][1][k].view(np.uint32)), k
        assert np.array_equal(got[0][1][k][0].view(np.uint32), got[2][1][k][0].view(np.uint32)), k


# ---- whole runs
def _body_rows(info):
    return (info[:, 0] & D.FG_COMPUTE_FORCE) != 0


def _paddle_rows(info):
    return (info[:, 0] & (D.FG_MOVING_BOUNDARY | D.FG_COMPUTE_FORCE)) == D.FG_MOVING_BOUNDARY


def test_host_uploads_do_not_clobber_the_floating_slot():
    """a paddle the host moves (uploaded in every substep) beside a cube the device moves: after a step the cube's slot holds what
    the device made of its state, the paddle's rows are the oracle's bit for bit (they come from the host's slot through the Euler
    kernel), and ten steps move both"""
    pr = BuoyancyBox(deltap=DP, paddle=True)
    eng = _engine(pr); sim = fr.FloatingOracleSim(pr)
    grid = fr.device_grid(pr)
    before = eng.floating_state()[0, :13].copy()
    eng.step(); sim.step()
    state, slots = eng.floating_state(slots=True)
    fr.check_slot({k: v[0] for k, v in slots.items()}, fr.slots_from_states(before, state[0, :13], grid), "after a step")
    assert np.abs(slots["trans"][0]).max() > 0 and np.abs(slots["lvel"][0]).max() > 0
    for _ in range(9):
        eng.step(); sim.step()
    out = eng.download()
    n = eng.n
    assert n == sim.n and np.array_equal(out["hash"], sim.hash[:n]) and np.array_equal(out["info"], sim.info[:n])
    pad, body = _paddle_rows(out["info"]), _body_rows(out["info"])
    assert pad.sum() == pr.num_paddle and body.sum() == pr.num_obstacle
    assert np.array_equal(out["pos"][pad].view(np.uint32), sim.pos[:n][pad].view(np.uint32))      # rigid rows of the host's body: bit-exact
    assert np.array_equal(out["vel"][pad, :3].view(np.uint32), sim.vel[:n][pad, :3].view(np.uint32))
    g1 = pr.global_pos(out["pos"], out["hash"])
    g0 = pr.parts.pos_global[:, :3]
    ids = out["info"][:, 2].astype(np.int64) | (out["info"][:, 3].astype(np.int64) << 16)
    moved = g1 - g0[ids]
    assert moved[pad, 0].min() > 1e-6 and np.abs(moved[pad, 1:]).max() < 1e-7                      # the paddle slid along x
    assert moved[body, 2].min() > 1e-5                                                              # the cube rose
    fixed = ~(pad | body) & ((out["info"][:, 0] & 7) == D.PT_BOUNDARY)
    assert np.abs(moved[fixed]).max() < 1e-7
    assert abs(eng.floating_state()[0, 2] - sim.fl.state[0, 2]) < 1e-6


def test_without_floating_bodies_the_host_owns_every_slot():
    """a body with prescribed motion alone (WaveTank's paddle, body 0): its rows are the oracle's bit for bit, as before the
    feature -- the host's table reaches the device in one copy (held byte for byte on the host emulation,
    tests/test_floating_hostemu.py; the device's table has no reader without floating bodies)"""
    from gpusph_amd.problem import WaveTank
    pr = WaveTank(0.06, paddle_tstart=0.0)
    eng = _engine(pr); sim = ol.OracleSim(pr)
    for _ in range(3):
        eng.step(); sim.step()
    out = eng.download()
    n = eng.n
    pad = (out["info"][:, 0] & D.FG_MOVING_BOUNDARY) != 0
    assert pad.sum() > 50 and np.array_equal(out["pos"][pad].view(np.uint32), sim.pos[:n][pad].view(np.uint32))
    with pytest.raises(ValueError, match="no floating bodies"):
        eng.floating_state()
    with pytest.raises(capi.SphxInvalidArgument, match="no floating bodies"):
        eng.k.floating_move(eng.rbforces, eng.rbtorques, 1, eng.d_dt)


def test_free_fall_in_an_empty_box():
    """no fluid: the totals are zero and the cube falls by the closed form of the discrete map with the step's own dt,
    v_n = g sum dt_k, x_n = x0 + g sum_k dt_k (sum_{j<=k} dt_j); every particle of it sits at (p0 - c0) + c"""
    pr = BuoyancyBox(deltap=DP, fluid=False)
    eng = _engine(pr)
    g = float(np.float32(-9.81))
    c0 = np.array(pr.CENTRE)
    vz, z, steps = 0.0, c0[2], 10
    for _ in range(steps):
        dt = float(np.float32(eng.current_dt()))
        vz = vz + dt*g
        z = z + dt*vz
        eng.step()
    s = eng.floating_state()[0]
    assert not s[13:19].any()
    # ten additions each: within 1e-12 of the closed form
    assert abs(s[9] - vz) <= 1e-12*abs(vz) and abs(s[2] - z) <= 1e-12*abs(z) and abs(z - c0[2]) > 1e-5
    assert np.array_equal(s[[0, 1]], c0[:2]) and np.array_equal(s[3:7], [1.0, 0.0, 0.0, 0.0]) and not s[[7, 8, 10, 11, 12]].any()
    out = eng.download()
    body = _body_rows(out["info"])
    ids = out["info"][:, 2].astype(np.int64) | (out["info"][:, 3].astype(np.int64) << 16)
    want = pr.parts.pos_global[ids[body], :3] - c0 + s[0:3]
    got = pr.global_pos(out["pos"][body], out["hash"][body])
    ulp = float(np.spacing(np.float32(pr.m_cellsize.max())))
    assert np.abs(got - want).max() <= 2*ulp*steps
    assert np.array_equal(out["vel"][body, 2], np.full(body.sum(), np.float32(s[9])))


@pytest.mark.parametrize("boundary", [D.DYN_BOUNDARY, D.LJ_BOUNDARY])
def test_a_run_beside_the_oracle(boundary):
    """12 steps across a rebuild.  Fluid rows to the bounds test_body_with_prescribed_motion_trajectory uses.  The body: every forces
    pass is within 2e-5 max|F| per row of the oracle's (the bound the project asserts for the rows of BUFFER_FORCES, accelerations;
    max|F_row| is their largest so far), so a body row, which is that times the particle's mass m_p, within 2e-5 max|F_row| m_p, a
    total over `rows` rows within rows times that, the velocity after k substeps of at most dt within k dt rows 2e-5 max|F_row| m_p / M,
    doubled for the feedback of the body's motion on the forces, and the position within that times the elapsed time."""
    pr = BuoyancyBox(deltap=DP, boundary=boundary)
    eng = _engine(pr); sim = fr.FloatingOracleSim(pr)
    steps, M, rows, m_p = 12, pr.floating_bodies[0].mass, pr.num_obstacle, float(pr.parts.pos_global[0, 3])
    dtmax, frow, worst_v, worst_x = 0.0, 0.0, 0.0, 0.0
    for k in range(1, steps + 1):
        dtmax = max(dtmax, sim.dt)
        eng.step(); sim.step()
        frow = max(frow, float(np.abs(sim.forces[:sim.n, :3]).max()))
        s = eng.floating_state()[0]
        bound_v = 2*(2*k)*dtmax*(rows*2e-5*frow*m_p)/M
        dv, dx = np.abs(s[7:10] - sim.fl.state[0, 7:10]).max(), np.abs(s[0:3] - sim.fl.state[0, 0:3]).max()
        worst_v, worst_x = max(worst_v, dv/bound_v), max(worst_x, dx/(bound_v*sim.t))
        assert dv <= bound_v and dx <= bound_v*sim.t, (k, dv, dx, bound_v)
    print("boundary %d: body velocity / position against the oracle, largest error / bound: %.3g / %.3g" % (boundary, worst_v, worst_x))
    out = eng.download()
    n = eng.n
    assert n == sim.n and np.array_equal(out["hash"], sim.hash[:n]) and np.array_equal(out["info"], sim.info[:n])
    cs = float(min(pr.m_cellsize))
    assert np.abs(out["pos"][:, :3] - sim.pos[:n, :3]).max() <= 1e-6*cs*steps
    assert np.abs(out["vel"][:, :3] - sim.vel[:n, :3]).max() <= 1e-3*np.abs(sim.vel[:n, :3]).max()
    assert abs(eng.time() - sim.t) <= 1e-6*sim.t
    assert frow > 0 and abs(sim.fl.state[0, 2] - pr.CENTRE[2]) > 1e-5


def test_no_host_read_in_a_step(monkeypatch):
    """only floating bodies: three steps with every way of reading a tensor to the host and the library's synchronous entry points
    patched to raise"""
    pr = BuoyancyBox(deltap=DP)
    eng = _engine(pr, track_particle_count=False)

    def refuse(*a, **k):
        raise AssertionError("a step read from the device")
    for name in ("item", "cpu", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    for name in ("sphx_forces_dtreduce", "sphx_reduce_rb_forces", "sphx_floating_state", "sphx_neibs_getinfo", "sphx_device_synchronize",
                 "sphx_memcpy_d2h"):
        monkeypatch.setattr(eng.lib, name, refuse)
    monkeypatch.setattr(type(eng.k), "neibs_info", refuse)
    monkeypatch.setattr(type(eng), "reduce_rb_forces", refuse)
    monkeypatch.setattr(type(eng), "current_dt", refuse)
    for _ in range(3):
        eng.step()
    monkeypatch.undo()
    s = eng.floating_state()[0]
    assert eng.iterations == 3 and s[2] > pr.CENTRE[2] and np.isfinite(s).all()


def test_hotfile_resume_is_bit_identical(tmp_path):
    """6 steps, save, 6 more; a fresh engine resumed from the file and run for 6 steps gives the same bits.  (Lists every 3
    iterations, so that the save falls on a rebuild as in the other resume tests: a resumed run always starts with one.)"""
    def make():
        pr = BuoyancyBox(deltap=DP)
        pr.simparams.buildneibsfreq = 3
        return pr
    a = _engine(make())
    a.run(6)
    path = tmp_path / "hot.bin"
    a.save_hotfile(path)
    saved = a.floating_state()[0, :13].copy()
    hf = hotfile.read_hotfile(path)
    assert len(hf["bodies"]) == 1
    rec = hf["bodies"][0]
    assert rec["type"] == hotfile.MB_FLOATING and rec["numparts"] == a.problem.num_obstacle
    assert np.array_equal(np.array(rec["orientation"]), saved[3:7]) and abs(float(np.dot(saved[3:7], saved[3:7])) - 1.0) <= 4*2.0**-52
    assert np.array_equal(np.array(rec["crot"]), saved[0:3]) and np.array_equal(np.array(rec["lvel"]), saved[7:10])
    assert np.array_equal(np.array(rec["avel"]), saved[10:13]) and saved[2] > 0.3
    a.run(6)
    ref, ref_state = a.download(), a.floating_state()[0, :13].copy()
    b = _engine(make())
    b.load_hotfile(path)
    assert b.iterations == 6 and np.array_equal(b.floating_state()[0, :13].view(np.uint64), saved.view(np.uint64))
    b.run(6)
    out = b.download()
    assert b.n == a.n and b.current_dt() == a.current_dt()
    for k in ("pos", "vel", "info", "hash"):
        assert np.array_equal(np.asarray(out[k]).view(np.uint8), np.asarray(ref[k]).view(np.uint8)), k
    assert np.array_equal(b.floating_state()[0, :13].view(np.uint64), ref_state.view(np.uint64))


def test_refusals(small):
    from gpusph_amd.multigpu import MultiGpuEngine
    from gpusph_amd.problem import SABox
    pr = BuoyancyBox(deltap=0.1)
    with pytest.raises(NotImplementedError, match="single domain"):
        MultiGpuEngine(pr, "cuda:0", 0, 2)
    sa = SABox(0.05)
    sa.floating_bodies = list(pr.floating_bodies)
    sa.simparams.numforcesbodies = 1
    with pytest.raises(NotImplementedError, match="SA_BOUNDARY"):
        _engine(sa)
    for change, text in ((lambda p: setattr(p.simparams, "sph_formulation", D.SPH_GRENIER), "SPH_GRENIER"),
                         (lambda p: setattr(p.simparams, "rheologytype", D.GRANULAR), "GRANULAR")):
        bad = BuoyancyBox(deltap=0.1)
        change(bad)
        with pytest.raises(NotImplementedError, match=text):
            _engine(bad)
    two = BuoyancyBox(deltap=0.1)
    two.floating_bodies = two.floating_bodies*2               # more floating bodies than bodies whose forces are computed
    with pytest.raises(ValueError, match="numforcesbodies"):
        _engine(two)
    K = _kernels(small)
    K.floating_setup(_bodies(1, np.random.default_rng(1)), np.array([0, 10], dtype=np.uint32))
    rbf, rbt = (_dev(a) for a in _rows(10, np.random.default_rng(2)))
    d_dt = _dev(np.array([3e-4], dtype=np.float32))
    for step in (0, 3):
        with pytest.raises(capi.SphxInvalidArgument, match="step is 1"):
            K.floating_move(rbf, rbt, step, d_dt)
    with pytest.raises(capi.SphxInvalidArgument, match="too many bodies"):
        K.floating_setup(_bodies(17, np.random.default_rng(1)), np.arange(18, dtype=np.uint32))
    bad = _bodies(1, np.random.default_rng(1))
    bad[0].mass = 0.0
    with pytest.raises(capi.SphxInvalidArgument, match="mass"):
        K.floating_setup(bad, np.array([0, 10], dtype=np.uint32))
