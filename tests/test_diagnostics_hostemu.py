"""diagnostics.hip (the save-time diagnostics: energies per fluid, the largest particle speed, the first particle without a finite
position) over its own source on the CPU (tests/hostemu), both kernels as teams of fibres (their shuffles and the barrier are
emulated), built with -DDIAG_MAX_BLOCKS=8 so that the grid-stride loop runs several rounds: against the float64 rule of
tests/diagnostics_ref.py to its derived bound, twice on one state, on part of the rows, on none and on one, without an energy
buffer, on a state whose answer can be counted, with inactive rows, NaN velocities and NaN positions, and with missing buffers.
This finds logic errors (classes, terms, folds, the cap of the grid); the device build is held to the same in
tests/test_gpu_save_diagnostics.py.  Without the feature sphx_save_diagnostics does not exist."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpusph_amd import capi, defs as D
from gpusph_amd.problem import DamBreak3D, info_type
import diagnostics_ref as ref

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "hostemu")
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, "gpusph_amd", "csrc")
_SO = os.path.join(_EMU, "_build", "libsphx_emu_diagnostics.so")
NAMES = ["sphx_create", "sphx_destroy", "sphx_set_constants", "sphx_last_error", "sphx_save_diagnostics"]
OK, INVALID = capi.SPHX_OK, capi.SPHX_ERR_INVALID
MAX_BLOCKS = 8


def _build():
    sources = [os.path.join(_EMU, "emu_diagnostics.cc"), os.path.join(_EMU, "hip", "hip_runtime.h"), os.path.join(_ROOT, "include", "sphx.h")] + \
        [os.path.join(_CSRC, f) for f in ("sphx_api.hip", "diagnostics.hip", "diagnostics.h", "gages.h", "sphx_internal.h")]
    os.makedirs(os.path.dirname(_SO), exist_ok=True)
    if os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(s) for s in sources + [os.path.abspath(__file__)]):
        return _SO
    pat = re.compile(r'(\b\w+(?:<[^<>;()]*>)?)<<<(.+?), (\w+), 0, ([^>;]+?)>>>\(')
    out, n = pat.subn(lambda m: "SPHX_LAUNCH_WAVES(%s, %s, %s, %s, " % m.groups(), open(os.path.join(_CSRC, "diagnostics.hip")).read())
    assert n == 2 and "<<<" not in out
    with open(os.path.join(_EMU, "_build", "diagnostics_emu.inc"), "w") as f:
        f.write(out)
    cmd = ["g++", "-O1", "-g0", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes",
           "-DDIAG_MAX_BLOCKS=%d" % MAX_BLOCKS,
           "-I" + _EMU, "-I" + os.path.join(_EMU, "_build"), "-I" + os.path.join(_ROOT, "include"), "-I" + _CSRC,
           "-o", _SO, os.path.join(_EMU, "emu_diagnostics.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return _SO


class _Case:
    def __init__(self):
        self.pr = pr = DamBreak3D(0.03, two_fluids=True, internal_energy=True, jitter=0.05)
        a = pr.copy_to_array()
        self.n = n = len(a["hash"])
        self.pos, self.info, self.hash = a["pos"], a["info"], a["hash"]
        rng = np.random.default_rng(11)
        self.vel = a["vel"].copy()
        self.vel[:, :3] = rng.uniform(-1.5, 1.5, size=(n, 3)).astype(np.float32)
        self.energy = rng.uniform(0.0, 40.0, size=n).astype(np.float32)
        self.lib = C.CDLL(_build())
        for name in NAMES:
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = capi.SIGNATURES[name]
        self.h = C.c_void_p()
        assert self.lib.sphx_create(C.byref(self.h), 0) == OK
        self.params = pr.sphx_params(n)
        assert self.lib.sphx_set_constants(self.h, C.byref(self.params)) == OK

    def rc(self, out, pos, vel, info, hash_, energy, n, h=None):
        conv = [a.ctypes.data if isinstance(a, np.ndarray) else a for a in (out, pos, vel, info, hash_, energy)]
        rc = self.lib.sphx_save_diagnostics(self.h if h is None else h, *conv, int(n), None)
        return rc, ("" if rc == OK else self.lib.sphx_last_error().decode())

    def run(self, pos=None, vel=None, energy="mine", n=None, info=None):
        pos = self.pos if pos is None else pos
        vel = self.vel if vel is None else vel
        info = self.info if info is None else info
        energy = self.energy if isinstance(energy, str) else energy
        n = self.n if n is None else n
        out = np.full(ref.DOUBLES, -7.0)
        rc, msg = self.rc(out, pos, vel, info, self.hash, energy, n)
        assert rc == OK, msg
        want = ref.rule(self.pr, pos[:n], vel[:n], info[:n], self.hash[:n], None if energy is None else energy[:n])
        return out, want


@pytest.fixture(scope="module")
def case():
    c = _Case()
    yield c
    c.lib.sphx_destroy(c.h)


def _classes(case, active=None):
    cls = np.where(info_type(case.info) == D.PT_FLUID, (case.info[:, 1] >> 12).astype(np.int64), D.MAX_FLUID_TYPES)
    if active is not None:
        cls = cls[active]
    return np.bincount(cls, minlength=ref.CLASSES)


def test_the_state_has_two_fluids_and_walls_and_needs_several_rounds(case):
    assert case.n == 16274
    counts = _classes(case)
    assert counts[0] > 500 and counts[1] > 500 and counts[D.MAX_FLUID_TYPES] > 500 and not counts[2:D.MAX_FLUID_TYPES].any()
    assert case.n > 3*MAX_BLOCKS*256


def test_against_the_rule_and_twice_the_same_bits(case):
    out, want = case.run()
    ref.check_out(out, want, "hostemu")
    assert (want["energy"][[0, 1, D.MAX_FLUID_TYPES]] != 0).all() and want["nan_row"] is None and want["max_speed"] > 1.5
    out2, _ = case.run()
    assert np.array_equal(out.view(np.uint64), out2.view(np.uint64))


@pytest.mark.parametrize("m", [0, 1, 63, 777, 2049, 11111])
def test_a_part_of_the_rows(case, m):
    """other grids and other partials: fewer blocks than the cap, a last wave that is not full, no row at all, one row"""
    assert m in (0, 1) or m % 64
    out, want = case.run(n=m)
    ref.check_out(out, want, "hostemu, rows [0, %d)" % m)
    assert int(want["rows"].sum()) == m
    if m == 0:
        assert not out[:ref.NANROW].any() and out[ref.NANROW] == ref.NO_ROW
        rc, msg = case.rc(out, None, None, None, None, None, 0)        # nothing is read
        assert rc == OK, msg


def test_without_an_energy_buffer(case):
    out, want = case.run(energy=None)
    ref.check_out(out, want, "hostemu, no energy buffer")
    full, _ = case.run()
    s, f = out[:ref.MAXSQ].reshape(-1, 4), full[:ref.MAXSQ].reshape(-1, 4)
    assert not s[:, 2].any() and f[[0, 1, D.MAX_FLUID_TYPES], 2].all()
    assert np.array_equal(s[:, [0, 1, 3]].view(np.uint64), f[:, [0, 1, 3]].view(np.uint64))


def test_counting_known_answer(case):
    """mass 1, velocity (1, 0, 0), energy 0.25: every sum is a count, exact in any order"""
    pos, vel = case.pos.copy(), case.vel.copy()
    pos[:, 3] = 1.0
    vel[:, :3] = (1.0, 0.0, 0.0)
    energy = np.full(case.n, 0.25, dtype=np.float32)
    out, want = case.run(pos=pos, vel=vel, energy=energy)
    s = out[:ref.MAXSQ].reshape(-1, 4)
    counts = _classes(case).astype(np.float64)
    assert np.array_equal(s[:, 3], counts) and counts.sum() == case.n
    assert np.array_equal(s[:, 0], 0.5*counts) and np.array_equal(s[:, 2], 0.25*counts)
    assert out[ref.MAXSQ] == 1.0 and np.sqrt(np.float32(out[ref.MAXSQ])) == np.float32(1.0) and out[ref.NANROW] == ref.NO_ROW
    ref.check_out(out, want, "hostemu, counting")


def test_inactive_rows_drop_out(case):
    pos, vel = case.pos.copy(), case.vel.copy()
    gone = np.array([0, 5, 640, 4097, case.n - 1])
    pos[gone, 3] = np.nan
    vel[gone[2], :3] = (50.0, -60.0, 70.0)                 # the largest velocity of all sits in an inactive row
    pos[gone[3], 0] = np.nan                               # ... and a NaN position in another: no sentinel for it
    out, want = case.run(pos=pos, vel=vel)
    ref.check_out(out, want, "hostemu, inactive rows")
    active = np.ones(case.n, dtype=bool); active[gone] = False
    assert np.array_equal(out[:ref.MAXSQ].reshape(-1, 4)[:, 3], _classes(case, active).astype(np.float64))
    assert np.sqrt(np.float32(out[ref.MAXSQ])) < 3.0 and out[ref.NANROW] == ref.NO_ROW and not np.isnan(out).any()


def test_nan_velocity_and_nan_positions(case):
    base, _ = case.run()
    vel = case.vel.copy()
    row = 1234
    vel[row, 1] = np.nan
    out, want = case.run(vel=vel)
    ref.check_out(out, want, "hostemu, NaN velocity")
    cls = int(np.nonzero(np.isnan(want["energy"][:, 0]))[0][0])
    s = out[:ref.MAXSQ].reshape(-1, 4)
    assert np.isnan(s[cls, 0]) and np.isnan(s[:, 0]).sum() == 1 and not np.isnan(s[:, 1:]).any()
    assert out[ref.MAXSQ] == base[ref.MAXSQ]               # fmax ignores the NaN
    pos = case.pos.copy()
    fl = np.nonzero((info_type(case.info) == D.PT_FLUID) & ((case.info[:, 1] >> 12) == 1))[0]
    a, b = int(fl[len(fl)//2]), int(fl[20])
    assert b < a
    pos[[a, b], 0] = np.nan
    out, want = case.run(pos=pos)
    ref.check_out(out, want, "hostemu, NaN positions")
    s = out[:ref.MAXSQ].reshape(-1, 4)
    assert out[ref.NANROW] == b and np.isnan(s[1, 1]) and np.isnan(s).sum() == 1


def test_missing_buffers_are_refused(case):
    out = np.zeros(ref.DOUBLES)
    args = [out, case.pos, case.vel, case.info, case.hash, case.energy]
    for k in range(5):
        a = list(args); a[k] = None
        rc, msg = case.rc(*a, case.n)
        assert rc == INVALID and "missing buffer" in msg, (k, rc, msg)
    fresh = C.c_void_p()
    assert case.lib.sphx_create(C.byref(fresh), 0) == OK
    rc, msg = case.rc(*args, case.n, h=fresh)
    assert rc == INVALID and "constants not set" in msg
    case.lib.sphx_destroy(fresh)
