"""floating.hip (the rigid-body dynamics of floating bodies) over its own source on the CPU (tests/hostemu), its kernels as teams of
fibres (their shuffles and the barrier are emulated), built with -DFLOAT_MAX_BLOCKS=4 so that the grid-stride loop runs several
rounds: the totals against math.fsum and the state against the float64 rule of tests/floating_ref.py, for row counts around the
wave and block sizes and above one round of the grid, two bodies with adjacent row ranges and the rows of a third body behind them,
a NaN row, steps 1, 2, 1; what a host upload leaves of the bodies' slots; the refusals of sphx_floating_setup.  This finds logic
errors (ranges, folds, the rule's terms, the merge of the two tables); the device build is held to the same in
tests/test_gpu_floating.py.  Without the feature the three entry points do not exist."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpusph_amd import capi
from gpusph_amd.bodies import FloatingBody, box_inertia
from gpusph_amd.problem import BuoyancyBox
import floating_ref as fr

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "hostemu")
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, "gpusph_amd", "csrc")
_SO = os.path.join(_EMU, "_build", "libsphx_emu_floating.so")
NAMES = ["sphx_create", "sphx_destroy", "sphx_set_constants", "sphx_last_error", "sphx_floating_setup", "sphx_floating_move",
         "sphx_floating_state", "sphx_set_rb_motion", "sphx_set_rb_cg", "sphx_set_rb_start"]
OK, INVALID = capi.SPHX_OK, capi.SPHX_ERR_INVALID
MAX_BLOCKS = 4
MAX_BODIES = 16
ONE_ROUND = MAX_BLOCKS*256          # rows one round of a body's blocks takes


def _build():
    sources = [os.path.join(_EMU, "emu_floating.cc"), os.path.join(_EMU, "hip", "hip_runtime.h"), os.path.join(_ROOT, "include", "sphx.h")] + \
        [os.path.join(_CSRC, f) for f in ("sphx_api.hip", "floating.hip", "floating.h", "diagnostics.h", "gages.h", "sphx_internal.h")]
    os.makedirs(os.path.dirname(_SO), exist_ok=True)
    if os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(s) for s in sources + [os.path.abspath(__file__)]):
        return _SO
    pat = re.compile(r'(\b\w+(?:<[^<>;()]*>)?)<<<(.+?), (\w+), 0, ([^>;]+?)>>>\(')
    out, n = pat.subn(lambda m: "SPHX_LAUNCH_WAVES(%s, %s, %s, %s, " % m.groups(), open(os.path.join(_CSRC, "floating.hip")).read())
    assert n == 3 and "<<<" not in out
    with open(os.path.join(_EMU, "_build", "floating_emu.inc"), "w") as f:
        f.write(out)
    cmd = ["g++", "-O1", "-g0", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes",
           "-DFLOAT_MAX_BLOCKS=%d" % MAX_BLOCKS,
           "-I" + _EMU, "-I" + os.path.join(_EMU, "_build"), "-I" + os.path.join(_ROOT, "include"), "-I" + _CSRC,
           "-o", _SO, os.path.join(_EMU, "emu_floating.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return _SO


def _table(raw):
    """RbParams (csrc/sphx_internal.h) from its bytes"""
    w = np.frombuffer(raw, dtype=np.uint32)
    o, out = 0, {}
    for name, per, dtype in (("cg_grid", 3, np.int32), ("cg_pos", 3, np.float32), ("cg_grid_e", 3, np.int32), ("cg_pos_e", 3, np.float32),
                             ("rbstart", 1, np.int32), ("trans", 3, np.float32), ("rot", 9, np.float32), ("lvel", 3, np.float32),
                             ("avel", 3, np.float32)):
        out[name] = w[o:o + MAX_BODIES*per].view(dtype).reshape(MAX_BODIES, per).copy()
        o += MAX_BODIES*per
    assert o == len(w)
    return out


class _Emu:
    def __init__(self):
        self.pr = BuoyancyBox(deltap=0.1)
        self.grid = fr.device_grid(self.pr)
        self.lib = C.CDLL(_build())
        for name in NAMES:
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = capi.SIGNATURES[name]
        self.lib.emu_rb_tables.restype = C.c_uint
        self.lib.emu_rb_tables.argtypes = [C.c_void_p]*4
        self.params = self.pr.sphx_params(len(self.pr.parts.info))

    def context(self, constants=True):
        h = C.c_void_p()
        assert self.lib.sphx_create(C.byref(h), 0) == OK
        if constants:
            assert self.lib.sphx_set_constants(h, C.byref(self.params)) == OK
        return h

    def err(self):
        return self.lib.sphx_last_error().decode()

    def setup_rc(self, h, bodies, rowstart, nf=None, drop=()):
        nf = len(bodies) if nf is None else nf
        col = lambda name, m: np.ascontiguousarray([np.asarray(getattr(b, name), dtype=np.float64).reshape(m) for b in bodies]).reshape(-1, m)
        arrs = [np.array([b.mass for b in bodies], dtype=np.float64), col("inertia", 3), col("crot", 3), col("orientation", 4),
                col("lvel", 3), col("avel", 3), np.ascontiguousarray(rowstart, dtype=np.uint32)]
        ptrs = [None if k in drop else a.ctypes.data for k, a in enumerate(arrs)]
        rc = self.lib.sphx_floating_setup(h, nf, *ptrs)
        return rc, ("" if rc == OK else self.err())

    def move(self, h, rbf, rbt, step, dt):
        d_dt = np.array([dt], dtype=np.float32)
        rc = self.lib.sphx_floating_move(h, rbf.ctypes.data, rbt.ctypes.data, step, d_dt.ctypes.data, None)
        return rc, ("" if rc == OK else self.err())

    def state(self, h, nf):
        state = np.full((nf, 19), -7.0)
        raw = np.zeros((nf, 30), dtype=np.float32)
        rc = self.lib.sphx_floating_state(h, state.ctypes.data, raw.ctypes.data, None)
        assert rc == OK, self.err()
        cells = raw[:, 24:].view(np.int32)
        return state, [dict(trans=raw[b, 0:3], rot=raw[b, 3:12], lvel=raw[b, 12:15], avel=raw[b, 15:18], cg_pos=raw[b, 18:21],
                            cg_pos_e=raw[b, 21:24], cg_grid=cells[b, 0:3], cg_grid_e=cells[b, 3:6]) for b in range(nf)]

    def tables(self, h):
        dev, host = np.zeros(1984, dtype=np.uint8), np.zeros(1984, dtype=np.uint8)
        assert self.lib.emu_rb_tables(h, dev.ctypes.data, host.ctypes.data, None) == 1984
        return dev, host


@pytest.fixture(scope="module")
def emu():
    return _Emu()


def _bodies(n, rng):
    out = []
    for b in range(n):
        q = rng.normal(size=4)
        m = 20.0 + 10.0*b
        out.append(FloatingBody(mass=m, inertia=box_inertia(m, (0.4, 0.3 + 0.1*b, 0.5)), crot=np.array([0.5, 0.4, 0.3]) + 0.1*b,
                                orientation=q/np.linalg.norm(q), lvel=rng.normal(size=3)*0.3, avel=rng.normal(size=3)*2.0))
    return out


def _rows(n, rng, scale=5.0):
    """float rows of mixed sign and very mixed size"""
    f = (rng.normal(size=(n, 4))*scale*10.0**rng.integers(-3, 3, size=(n, 1))).astype(np.float32)
    t = (rng.normal(size=(n, 4))*scale*10.0**rng.integers(-3, 3, size=(n, 1))).astype(np.float32)
    f[:, 3] = 1e30; t[:, 3] = -1e30          # the fourth component is never part of a sum
    return f, t


def _check_substep(emu, h, ref, bodies, rbf, rbt, rowstart, step, dt, where):
    nf = len(bodies)
    prev = ref.state[:, :fr.KEPT].copy() if step == 1 else ref.saved.copy()
    rc, msg = emu.move(h, rbf, rbt, step, dt)
    assert rc == OK, msg
    state, slots = emu.state(h, nf)
    fr.check_totals(state[:, 13:19], rbf, rbt, rowstart, where)
    dt1 = 0.5*float(np.float32(dt)) if step == 1 else float(np.float32(dt))
    for b in range(nf):
        fr.check_state(state[b], prev[b], state[b, 13:19], bodies[b].mass, bodies[b].inertia, emu.grid["gravity"], dt1, "%s body %d" % (where, b))
        fr.check_slot(slots[b], fr.slots_from_states(prev[b], state[b, :13], emu.grid), "%s body %d" % (where, b))
    # the reference carries the DEVICE's totals on, so that the next substep starts from comparable states
    ref.substep(step, state[:, 13:19], dt)
    for b in range(nf):
        ref.state[b, :fr.KEPT] = state[b, :fr.KEPT]
        if step == 1:
            ref.saved[b] = prev[b]
    return state


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4*ONE_ROUND + 5])
def test_row_counts(emu, n):
    """one body, rows [3, 3 + n): fewer rows than lanes, a wave, one more, more than a block, several rounds of the capped grid"""
    rng = np.random.default_rng(100 + n)
    assert n in (0, 1) or n == 64 or n % 64
    bodies = _bodies(1, rng)
    rbf, rbt = _rows(n + 7, rng)
    rowstart = np.array([3, 3 + n], dtype=np.uint32)
    h = emu.context()
    rc, msg = emu.setup_rc(h, bodies, rowstart)
    assert rc == OK, msg
    ref = fr.RefBodies(bodies, emu.grid)
    s1 = _check_substep(emu, h, ref, bodies, rbf, rbt, rowstart, 1, 2.5e-4, "n=%d step 1" % n)
    if n == 0:
        assert not s1[0, 13:19].any()
    emu.lib.sphx_destroy(h)


def test_same_inputs_same_bits_and_another_bodys_rows_do_not_matter(emu):
    rng = np.random.default_rng(7)
    bodies = _bodies(2, rng)
    rowstart = np.array([0, 700, 1500], dtype=np.uint32)
    rbf, rbt = _rows(1500, rng)
    got = []
    for variant in range(3):
        f, t = rbf.copy(), rbt.copy()
        if variant == 2:
            f[700:], t[700:] = _rows(800, np.random.default_rng(8))
        h = emu.context()
        assert emu.setup_rc(h, bodies, rowstart)[0] == OK
        for step in (1, 2):
            assert emu.move(h, f, t, step, 3e-4)[0] == OK
        got.append(emu.state(h, 2))
        emu.lib.sphx_destroy(h)
    assert np.array_equal(got[0][0].view(np.uint64), got[1][0].view(np.uint64))
    assert np.array_equal(got[0][0][0].view(np.uint64), got[2][0][0].view(np.uint64)) and not np.array_equal(got[0][0][1], got[2][0][1])
    for k in got[0][1][0]:
        assert np.array_equal(got[0][1][0][k], got[2][1][0][k]), k


def test_adjacent_ranges_a_third_body_a_nan_row_and_steps_1_2_1(emu):
    """two floating bodies whose row ranges touch (every row counts for its own body alone: the rows at the seam are huge and of
    opposite sign), the rows of a third, non-floating body behind them (never counted), then a NaN row in the second body"""
    rng = np.random.default_rng(21)
    bodies = _bodies(2, rng)
    n0, n1, n2 = ONE_ROUND + 77, 130, 50
    rowstart = np.array([0, n0, n0 + n1], dtype=np.uint32)
    rbf, rbt = _rows(n0 + n1 + n2, rng)
    rbf[n0 - 1, :3] = (4e6, -3e6, 2e6); rbf[n0, :3] = (-5e6, 1e6, 7e6)
    rbt[n0 - 1, :3] = (1e5, 2e5, -3e5); rbt[n0, :3] = (-2e5, 4e5, 6e5)
    rbf[n0 + n1:, :3] = 9e8; rbt[n0 + n1:, :3] = -9e8
    h = emu.context()
    assert emu.setup_rc(h, bodies, rowstart)[0] == OK
    ref = fr.RefBodies(bodies, emu.grid)
    before = ref.state[:, :13].copy()
    s = _check_substep(emu, h, ref, bodies, rbf, rbt, rowstart, 1, 3e-4, "step 1")
    assert abs(s[0, 13] - 4e6) < 1e5 and abs(s[1, 13] + 5e6) < 1e5 and np.abs(s[:, 13:19]).max() < 1e8
    f2, t2 = _rows(n0 + n1 + n2, rng)
    s2 = _check_substep(emu, h, ref, bodies, f2, t2, rowstart, 2, 3e-4, "step 2")
    # step 2 started from the state step 1 saved, not from where step 1 ended
    for b in range(2):
        fr.check_state(s2[b], before[b], s2[b, 13:19], bodies[b].mass, bodies[b].inertia, emu.grid["gravity"], float(np.float32(3e-4)), "from n")
    s3 = _check_substep(emu, h, ref, bodies, rbf, rbt, rowstart, 1, 2e-4, "step 1 again")
    assert not np.array_equal(s3[:, :3], s[:, :3])
    # one NaN row of the second body: its state is not finite any more, the first body's is, and nothing raises
    f2[n0 + 5, 1] = np.nan
    rc, msg = emu.move(h, f2, t2, 2, 2e-4)
    assert rc == OK, msg
    s4, slots = emu.state(h, 2)
    assert np.isfinite(s4[0]).all() and np.isnan(s4[1, 14]) and not np.isfinite(s4[1, :13]).all()
    assert np.isfinite(s4[1, [0, 2]]).all() and np.isnan(s4[1, 1])          # the force's y went into v_y and x_y alone
    assert (slots[1]["cg_grid"] >= 0).all() and (slots[1]["cg_grid"] < emu.grid["gridsize"]).all()
    emu.lib.sphx_destroy(h)


def test_host_uploads_leave_the_floating_slots_alone(emu):
    """bodies 0 and 1 float, body 2 is the host's: every setter marks the whole table for upload, and what reaches the device is
    body 2's slot and every body's rbstart; after sphx_floating_setup(0), and in a context that never had floating bodies, the
    device's table is the host's byte for byte"""
    rng = np.random.default_rng(33)
    bodies = _bodies(2, rng)
    rowstart = np.array([0, 100, 220], dtype=np.uint32)
    rbf, rbt = _rows(220, rng)
    h = emu.context()
    nb = 3

    def upload(seed):
        r = np.random.default_rng(seed)
        a = [r.normal(size=(nb, 3)).astype(np.float32), r.normal(size=(nb, 9)).astype(np.float32), r.normal(size=(nb, 3)).astype(np.float32),
             r.normal(size=(nb, 3)).astype(np.float32)]
        assert emu.lib.sphx_set_rb_motion(h, *[x.ctypes.data for x in a], nb) == OK
        gp, lp = r.integers(0, 5, size=(nb, 3)).astype(np.int32), r.normal(size=(nb, 3)).astype(np.float32)
        assert emu.lib.sphx_set_rb_cg(h, gp.ctypes.data, lp.ctypes.data, nb) == OK
        start = np.array([-5, -105, seed], dtype=np.int32)
        assert emu.lib.sphx_set_rb_start(h, start.ctypes.data, nb) == OK
        return dict(trans=a[0], rot=a[1], lvel=a[2], avel=a[3], cg_grid=gp, cg_pos=lp, cg_grid_e=gp, cg_pos_e=lp, rbstart=start.reshape(nb, 1))

    first = upload(1)
    dev, host = emu.tables(h)
    assert np.array_equal(dev, host)                         # no floating bodies yet: the one copy
    assert emu.setup_rc(h, bodies, rowstart)[0] == OK
    dev, host = emu.tables(h)
    assert np.array_equal(dev, host)                         # the bodies' first slots travel with the whole table
    t = _table(dev.tobytes())
    assert np.array_equal(t["rot"][0], np.eye(3, dtype=np.float32).ravel()) and not t["trans"][:2].any()
    assert np.array_equal(t["lvel"][1], np.asarray(bodies[1].lvel, dtype=np.float32)) and np.array_equal(t["trans"][2], first["trans"][2])
    assert emu.move(h, rbf, rbt, 1, 3e-4)[0] == OK
    mine = _table(emu.tables(h)[0].tobytes())
    assert mine["trans"][:2].any() and np.array_equal(mine["trans"][2], first["trans"][2])
    second = upload(2)                                       # stale values for bodies 0 and 1, new ones for body 2
    after = _table(emu.tables(h)[0].tobytes())
    for k in ("trans", "rot", "lvel", "avel", "cg_grid", "cg_pos", "cg_grid_e", "cg_pos_e"):
        assert np.array_equal(after[k][:2].view(np.uint32), mine[k][:2].view(np.uint32)), k
        assert np.array_equal(after[k][2].view(np.uint32), second[k][2].view(np.uint32)), k
        assert np.array_equal(after[k][3:].view(np.uint32), mine[k][3:].view(np.uint32)), k
    assert np.array_equal(after["rbstart"][:3], second["rbstart"])
    upload(3)                                                # pending when the next move comes: flushed first, the move's writes last
    assert emu.move(h, rbf, rbt, 2, 3e-4)[0] == OK
    state, slots = emu.state(h, 2)
    last = _table(emu.tables(h)[0].tobytes())
    for b in range(2):
        assert np.array_equal(last["trans"][b], slots[b]["trans"]) and np.array_equal(last["lvel"][b], state[b, 7:10].astype(np.float32))
    assert last["rbstart"][2, 0] == 3
    # the feature dropped: the host owns every slot again
    assert emu.setup_rc(h, [], np.zeros(1, dtype=np.uint32), nf=0, drop=range(7))[0] == OK
    upload(4)
    dev, host = emu.tables(h)
    assert np.array_equal(dev, host)
    rc, msg = emu.move(h, rbf, rbt, 1, 3e-4)
    assert rc == INVALID and "no floating bodies" in msg
    emu.lib.sphx_destroy(h)


def test_refusals(emu):
    rng = np.random.default_rng(5)
    good = _bodies(2, rng)
    rowstart = np.array([0, 10, 30], dtype=np.uint32)
    h = emu.context()

    def refused(bodies, rs, text, **kw):
        rc, msg = emu.setup_rc(h, bodies, rs, **kw)
        assert rc == INVALID and text in msg, (rc, msg)
        return msg

    seen = set()
    for field, value, text in (("mass", 0.0, "mass"), ("mass", -1.0, "mass"), ("mass", float("nan"), "mass"),
                               ("inertia", np.array([1.0, 0.0, 1.0]), "inertia"), ("inertia", np.array([1.0, 1.0, -2.0]), "inertia"),
                               ("orientation", np.zeros(4), "zero quaternion")):
        bad = _bodies(2, np.random.default_rng(5))
        setattr(bad[1], field, value)
        seen.add(refused(bad, rowstart, text))
    seen.add(refused(good, np.array([0, 10, 9], dtype=np.uint32), "rowstart decreases"))
    many = _bodies(MAX_BODIES + 1, rng)
    seen.add(refused(many, np.arange(MAX_BODIES + 2, dtype=np.uint32), "too many bodies"))
    seen.add(refused(good, rowstart, "negative", nf=-1))
    seen.add(refused(good, rowstart, "missing array", drop=(2,)))
    assert len(seen) == 7                                    # each refusal has a message of its own
    fresh = emu.context(constants=False)
    rc, msg = emu.setup_rc(fresh, good, rowstart)
    assert rc == INVALID and "constants not set" in msg
    emu.lib.sphx_destroy(fresh)
    # nothing was set up by a refused call
    rbf, rbt = _rows(30, rng)
    rc, msg = emu.move(h, rbf, rbt, 1, 3e-4)
    assert rc == INVALID and "no floating bodies" in msg
    assert emu.setup_rc(h, good, rowstart)[0] == OK
    for step in (0, 3, -1):
        rc, msg = emu.move(h, rbf, rbt, step, 3e-4)
        assert rc == INVALID and "step is 1" in msg
    d_dt = np.array([3e-4], dtype=np.float32)
    assert emu.lib.sphx_floating_move(h, None, rbt.ctypes.data, 1, d_dt.ctypes.data, None) == INVALID and "missing buffer" in emu.err()
    assert emu.lib.sphx_floating_move(h, rbf.ctypes.data, rbt.ctypes.data, 1, None, None) == INVALID and "missing buffer" in emu.err()
    emu.lib.sphx_destroy(h)
