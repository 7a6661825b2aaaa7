"""floating_exact.hip (the exactly rounded, order-free sums of a floating body's rows) over its own source on the CPU (tests/hostemu),
beside floating.hip whose rule it drives: the kernels as teams of fibres, built with -DFLOAT_MAX_BLOCKS=4 so that the grid-stride
loop runs several rounds.  The device's limbs against the format in Python integers (tests/floating_exact_ref.py), array-equal; the
totals against math.fsum bit for bit and against the known answers (the whole float range, ties, cancelling pairs, rows that are not
finite); the state against the float64 rule exactly as tests/test_floating_hostemu.py checks the default path; steps 1, 2, 1;
limbs of complementary subsets added in either order; the refusals.  This finds logic errors (limb indices, carries, signs, the
rounding); the device build is held to the same in tests/test_gpu_floating_exact.py.  Without the feature the two entry points do
not exist."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpusph_amd import capi
import floating_exact_ref as fx
import floating_ref as fr
import test_floating_hostemu as base

_EMU, _ROOT, _CSRC = base._EMU, base._ROOT, base._CSRC
_SO = os.path.join(_EMU, "_build", "libsphx_emu_floating_exact.so")
OK, INVALID = capi.SPHX_OK, capi.SPHX_ERR_INVALID
MAX_BLOCKS = 4
ONE_ROUND = MAX_BLOCKS*256
NAMES = base.NAMES + ["sphx_floating_limbs", "sphx_floating_move_limbs"]


def _build():
    sources = [os.path.join(_EMU, "emu_floating_exact.cc"), os.path.join(_EMU, "hip", "hip_runtime.h"), os.path.join(_ROOT, "include", "sphx.h")] + \
        [os.path.join(_CSRC, f) for f in ("sphx_api.hip", "floating.hip", "floating.h", "floating_exact.hip", "floating_exact.h",
                                          "diagnostics.h", "gages.h", "sphx_internal.h")]
    os.makedirs(os.path.dirname(_SO), exist_ok=True)
    if os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(s) for s in sources + [os.path.abspath(__file__)]):
        return _SO
    pat = re.compile(r'(\b\w+(?:<[^<>;()]*>)?)<<<(.+?), (\w+), 0, ([^>;]+?)>>>\(')
    for src, inc, launches in (("floating.hip", "floating_exact_emu_step.inc", 3), ("floating_exact.hip", "floating_exact_emu_sums.inc", 3)):
        out, n = pat.subn(lambda m: "SPHX_LAUNCH_WAVES(%s, %s, %s, %s, " % m.groups(), open(os.path.join(_CSRC, src)).read())
        assert n == launches and "<<<" not in out
        with open(os.path.join(_EMU, "_build", inc), "w") as f:
            f.write(out)
    cmd = ["g++", "-O1", "-g0", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes",
           "-DFLOAT_MAX_BLOCKS=%d" % MAX_BLOCKS,
           "-I" + _EMU, "-I" + os.path.join(_EMU, "_build"), "-I" + os.path.join(_ROOT, "include"), "-I" + _CSRC,
           "-o", _SO, os.path.join(_EMU, "emu_floating_exact.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return _SO


class _Emu(base._Emu):
    def __init__(self):
        from gpusph_amd.problem import BuoyancyBox
        self.pr = BuoyancyBox(deltap=0.1)
        self.grid = fr.device_grid(self.pr)
        self.lib = C.CDLL(_build())
        for name in NAMES:
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = capi.SIGNATURES[name]
        self.params = self.pr.sphx_params(len(self.pr.parts.info))

    def limbs(self, h, rbf, rbt, nf):
        out = np.full((nf, 6, capi.SPHX_FLOATING_LIMBS), -7.0)
        rc = self.lib.sphx_floating_limbs(h, rbf.ctypes.data, rbt.ctypes.data, out.ctypes.data, None)
        assert rc == OK, self.err()
        return out

    def move_limbs(self, h, limbs, step, dt):
        d_dt = np.array([dt], dtype=np.float32)
        limbs = np.ascontiguousarray(limbs, dtype=np.float64)
        rc = self.lib.sphx_floating_move_limbs(h, limbs.ctypes.data, step, d_dt.ctypes.data, None)
        return rc, ("" if rc == OK else self.err())

    def move(self, h, rbf, rbt, step, dt):
        """the exact path where test_floating_hostemu's _check_substep calls the default one"""
        return self.move_limbs(h, self.limbs(h, rbf, rbt, self.nf), step, dt)


@pytest.fixture(scope="module")
def emu():
    return _Emu()


def _start(emu, bodies, rowstart):
    h = emu.context()
    rc, msg = emu.setup_rc(h, bodies, rowstart)
    assert rc == OK, msg
    emu.nf = len(bodies)
    return h


def _exact_substep(emu, h, ref, bodies, rbf, rbt, rowstart, step, dt, where):
    """limbs array-equal to the format, totals bit-equal to math.fsum, then everything _check_substep asks of the default path"""
    got = emu.limbs(h, rbf, rbt, len(bodies))
    assert np.array_equal(got, fx.limbs(rbf, rbt, rowstart)), where
    state = base._check_substep(emu, h, ref, bodies, rbf, rbt, rowstart, step, dt, where)
    assert fx.same_bits(state[:, 13:19], fr.fsum_rows(rbf, rbt, rowstart)), where
    return state


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4*ONE_ROUND + 5])
def test_row_counts(emu, n):
    rng = np.random.default_rng(100 + n)
    bodies = base._bodies(1, rng)
    rbf, rbt = base._rows(n + 7, rng)
    rowstart = np.array([3, 3 + n], dtype=np.uint32)
    h = _start(emu, bodies, rowstart)
    ref = fr.RefBodies(bodies, emu.grid)
    s1 = _exact_substep(emu, h, ref, bodies, rbf, rbt, rowstart, 1, 2.5e-4, "n=%d step 1" % n)
    if n == 0:
        assert not s1[0, 13:19].any() and not np.signbit(s1[0, 13:19]).any()
    emu.lib.sphx_destroy(h)


def test_adjacent_ranges_a_third_body_and_steps_1_2_1(emu):
    rng = np.random.default_rng(21)
    bodies = base._bodies(2, rng)
    n0, n1, n2 = ONE_ROUND + 77, 130, 50
    rowstart = np.array([0, n0, n0 + n1], dtype=np.uint32)
    rbf, rbt = base._rows(n0 + n1 + n2, rng)
    rbf[n0 - 1, :3] = (4e6, -3e6, 2e6); rbf[n0, :3] = (-5e6, 1e6, 7e6)
    rbf[n0 + n1:, :3] = 7e9; rbt[n0 + n1:, :3] = -7e9
    h = _start(emu, bodies, rowstart)
    ref = fr.RefBodies(bodies, emu.grid)
    before = ref.state[:, :13].copy()
    s = _exact_substep(emu, h, ref, bodies, rbf, rbt, rowstart, 1, 3e-4, "step 1")
    f2, t2 = base._rows(n0 + n1 + n2, rng)
    s2 = _exact_substep(emu, h, ref, bodies, f2, t2, rowstart, 2, 3e-4, "step 2")
    for b in range(2):      # step 2 started from the state step 1 saved
        fr.check_state(s2[b], before[b], s2[b, 13:19], bodies[b].mass, bodies[b].inertia, emu.grid["gravity"], float(np.float32(3e-4)), "from n")
    s3 = _exact_substep(emu, h, ref, bodies, rbf, rbt, rowstart, 1, 2e-4, "step 1 again")
    assert not np.array_equal(s3[:, :3], s[:, :3])
    emu.lib.sphx_destroy(h)


@pytest.mark.parametrize("which", range(len(fx.KNOWN_BODIES)))
def test_known_answers(emu, which):
    """the whole float range, ties, pairs, rows that are not finite: limbs and totals against the reasoning's"""
    rng = np.random.default_rng(which)
    rbf, rbt, want = fx.known_rows(fx.KNOWN_BODIES[which], first=2, behind=3)
    rowstart = np.array([2, len(rbf) - 3], dtype=np.uint32)
    bodies = base._bodies(1, rng)
    h = _start(emu, bodies, rowstart)
    got = emu.limbs(h, rbf, rbt, 1)
    assert np.array_equal(got, fx.limbs(rbf, rbt, rowstart))
    assert emu.move_limbs(h, got, 1, 3e-4)[0] == OK
    state, _ = emu.state(h, 1)
    assert fx.same_bits(state[0, 13:19], want), (state[0, 13:19], want)
    emu.lib.sphx_destroy(h)


def test_subsets_added_in_either_order_move_the_body_with_the_same_bits(emu):
    rng = np.random.default_rng(9)
    bodies = base._bodies(2, rng)
    rowstart = np.array([1, 1200, 1500], dtype=np.uint32)
    rbf, rbt = base._rows(1500, rng)
    idx = np.arange(1500)

    def run(limbs):
        h = _start(emu, bodies, rowstart)
        assert emu.move_limbs(h, limbs(h), 1, 3e-4)[0] == OK
        out = emu.state(h, 2)
        emu.lib.sphx_destroy(h)
        return out

    whole = run(lambda h: emu.limbs(h, rbf, rbt, 2))
    for parts in ([idx < 700, idx >= 700], [idx % 2 == 0, idx % 2 == 1], [idx % 3 == 0, idx % 3 == 1, idx % 3 == 2]):
        for order in (parts, parts[::-1]):
            def limbs(h):
                total = np.zeros((2, 6, capi.SPHX_FLOATING_LIMBS))
                for keep in order:
                    f, t = rbf.copy(), rbt.copy()
                    f[~keep, :3] = 0.0; t[~keep, :3] = 0.0
                    total = total + emu.limbs(h, f, t, 2)
                return total
            got = run(limbs)
            assert np.array_equal(got[0].view(np.uint64), whole[0].view(np.uint64))
            for b in range(2):
                for k in whole[1][b]:
                    assert np.array_equal(got[1][b][k], whole[1][b][k]), k


def test_refusals(emu):
    rng = np.random.default_rng(5)
    rbf, rbt = base._rows(30, rng)
    out = np.zeros((2, 6, capi.SPHX_FLOATING_LIMBS))
    d_dt = np.array([3e-4], dtype=np.float32)
    L, M = emu.lib.sphx_floating_limbs, emu.lib.sphx_floating_move_limbs
    seen = set()

    def refused(rc, text):
        assert rc == INVALID and text in emu.err(), (rc, emu.err())
        seen.add(emu.err())

    fresh = emu.context(constants=False)
    refused(L(fresh, rbf.ctypes.data, rbt.ctypes.data, out.ctypes.data, None), "constants not set")
    refused(M(fresh, out.ctypes.data, 1, d_dt.ctypes.data, None), "constants not set")
    emu.lib.sphx_destroy(fresh)
    h = emu.context()
    refused(L(h, rbf.ctypes.data, rbt.ctypes.data, out.ctypes.data, None), "no floating bodies")
    refused(M(h, out.ctypes.data, 1, d_dt.ctypes.data, None), "no floating bodies")
    assert emu.setup_rc(h, base._bodies(2, rng), np.array([0, 10, 30], dtype=np.uint32))[0] == OK
    refused(L(h, None, rbt.ctypes.data, out.ctypes.data, None), "missing buffer")
    refused(L(h, rbf.ctypes.data, None, out.ctypes.data, None), "missing buffer")
    refused(L(h, rbf.ctypes.data, rbt.ctypes.data, None, None), "NULL d_limbs")
    for step in (0, 3, -1):
        refused(M(h, out.ctypes.data, step, d_dt.ctypes.data, None), "step is 1")
    refused(M(h, out.ctypes.data, 1, None, None), "missing buffer")
    refused(M(h, None, 1, d_dt.ctypes.data, None), "NULL d_limbs")
    # four refusals of the one, five of the other, each with a message of its own that names its entry point
    assert len(seen) == 9 and all(("sphx_floating_limbs" in m) != ("sphx_floating_move_limbs" in m) for m in seen)
    # the feature dropped: both refuse again
    assert emu.setup_rc(h, [], np.zeros(1, dtype=np.uint32), nf=0, drop=range(7))[0] == OK
    refused(L(h, rbf.ctypes.data, rbt.ctypes.data, out.ctypes.data, None), "no floating bodies")
    emu.lib.sphx_destroy(h)
