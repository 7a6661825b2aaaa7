"""filters.hip (the post-processing engines) and gages.hip over their own source on the CPU (tests/hostemu), on the sorted state and
the neighbour list the CPU oracle builds for the probe tank: test points, surface detection and vorticity of an SA_BOUNDARY context
against the float64 restatement (tests/sa_postprocess_ref.py) to the bounds of tests/sa_postprocess_cases.py, the k-epsilon entry
point, the wave gages (the two reducing kernels as teams of fibres: their ballots and shuffles are emulated), and what is still refused.  This
finds logic errors (sections of the list, flags, sums, the folds of the gage partials); the device build is held to the same in
tests/test_gpu_sa_postprocess.py and tests/test_gpu_wave_gages.py.  The SA list build itself cannot run here (its general walk sits
under lane-dependent ballots, which the emulation refuses): the list of test-point rows is checked as sets on the oracle's build
(tests/test_sa_postprocess_ref.py) and on the device's (tests/test_gpu_sa_postprocess.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpusph_amd import capi, defs as D
from gpusph_amd.problem import DamBreak3D, info_type
from sa_helpers import sa_oracle_state
import sa_postprocess_cases as cases

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "hostemu")
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, "gpusph_amd", "csrc")
_SO = os.path.join(_EMU, "_build", "libsphx_emu_postprocess.so")
NAMES = ["sphx_create", "sphx_destroy", "sphx_set_constants", "sphx_last_error", "sphx_postprocess", "sphx_postprocess_testpoints_keps",
         "sphx_filter_process", "sphx_wave_gages", "sphx_wave_gages_finish"]
OK, INVALID, UNSUPPORTED = capi.SPHX_OK, capi.SPHX_ERR_INVALID, capi.SPHX_ERR_UNSUPPORTED


def _build():
    sources = [os.path.join(_EMU, "emu_postprocess.cc"), os.path.join(_EMU, "hip", "hip_runtime.h"), os.path.join(_ROOT, "include", "sphx.h")] + \
        [os.path.join(_CSRC, f) for f in ("sphx_api.hip", "filters.hip", "gages.hip", "sphx_internal.h", "neib_iter.h")]
    os.makedirs(os.path.dirname(_SO), exist_ok=True)
    if os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(s) for s in sources):
        return _SO
    pat = re.compile(r'(\b\w+(?:<[^<>;()]*>)?)<<<(.+?), (\w+), 0, ([^>;]+?)>>>\(')

    def launch(m):      # a block of whole waves that meet in wave operations: fibres; everything else is the plain serial launch
        if m.group(1) in ("gage_partials_kernel", "gage_fold_kernel"):
            return "SPHX_LAUNCH_WAVES(%s, %s, %s, %s, " % (m.group(1), m.group(2), m.group(3), m.group(4))
        return "SPHX_EMU_LAUNCH((%s), %s, %s, " % (m.group(1), m.group(2), m.group(3))
    for src in ("filters", "gages"):
        out, n = pat.subn(launch, open(os.path.join(_CSRC, src + ".hip")).read())
        assert n > 0 and "<<<" not in out
        with open(os.path.join(_EMU, "_build", src + "_emu.inc"), "w") as f:
            f.write(out)
    cmd = ["g++", "-O1", "-g0", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes",
           "-I" + _EMU, "-I" + os.path.join(_EMU, "_build"), "-I" + os.path.join(_ROOT, "include"), "-I" + _CSRC,
           "-o", _SO, os.path.join(_EMU, "emu_postprocess.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return _SO


class _Emu:
    def __init__(self, params):
        self.lib = C.CDLL(_build())
        for name in NAMES:
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = capi.SIGNATURES[name]
        self.h = C.c_void_p()
        assert self.lib.sphx_create(C.byref(self.h), 0) == OK
        self.params = params
        assert self.lib.sphx_set_constants(self.h, C.byref(params)) == OK

    def rc(self, name, *args):
        conv = [a.ctypes.data if isinstance(a, np.ndarray) else a for a in args]
        rc = getattr(self.lib, name)(self.h, *conv)
        return rc, ("" if rc == OK else self.lib.sphx_last_error().decode())

    def call(self, name, *args):
        rc, msg = self.rc(name, *args)
        assert rc == OK, msg

    def close(self):
        self.lib.sphx_destroy(self.h)


class _Case:
    def __init__(self, jitter, viscosity="DYNAMICVISC"):
        self.pr = pr = cases.probe_box(jitter, viscosity)
        st = sa_oracle_state(pr)
        self.n = n = st["n"]
        self.pos, self.info, self.hash, self.cs, self.nl = st["pos"], st["info"], st["hash"], st["cs"], st["nl"]
        self.gpos = pr.global_pos(self.pos[:n], self.hash[:n])
        self.vel, self.tke, self.eps = cases.fields(pr, self.gpos, self.info[:n], st["vel"][:n])
        self.emu = _Emu(pr.sphx_params(n))
        self.ref = cases.Restated(pr, self.gpos, self.info[:n], self.vel, self.pos[:n, 3], self.tke, self.eps)

    def post(self, pptype, vort=None, vel_inout=None, info_inout=None, normals=None, vel=None):
        n = self.n
        self.emu.call("sphx_postprocess", int(pptype), vort, vel_inout, info_inout, normals, self.pos, vel, self.info, self.hash, self.cs,
                      self.nl, n, n, 0.86, 0.5, None)


@pytest.fixture(scope="module", params=[0.0, 0.1])
def case(request):
    c = _Case(request.param)
    yield c
    c.emu.close()


def test_test_points(case):
    vel = case.vel.copy()
    case.post(D.TESTPOINTS, vel_inout=vel)
    rows, _ = case.ref.testpoints(vel)
    other = np.ones(case.n, dtype=bool); other[rows] = False
    assert np.array_equal(vel[other].view(np.uint32), case.vel[other].view(np.uint32))      # only the probes' rows are written
    # the k-epsilon entry point: the same velocity rows bit for bit, k and epsilon of the probes
    v2, tke, eps = case.vel.copy(), case.tke.copy(), case.eps.copy()
    n = case.n
    case.emu.call("sphx_postprocess_testpoints_keps", v2, tke, eps, case.pos, case.info, case.hash, case.cs, case.nl, n, n, None)
    assert np.array_equal(v2.view(np.uint32), vel.view(np.uint32))
    case.ref.testpoints(v2, tke, eps)
    assert np.array_equal(tke[other], case.tke[other]) and np.array_equal(eps[other], case.eps[other])


def test_surface_detection_and_gages(case):
    n = case.n
    info = case.info[:n].copy()
    normals = np.zeros((n, 4), dtype=np.float32)
    case.post(D.SURFACE_DETECTION, info_inout=info, normals=normals, vel=case.vel)
    case.ref.surface(case.info[:n], info, normals)
    info2 = case.info[:n].copy()
    info2[:, 0] |= D.FG_SURFACE                        # stale flags are cleared, and the normals are optional
    case.post(D.SURFACE_DETECTION, info_inout=info2, vel=case.vel)
    fl = info_type(info) == D.PT_FLUID
    assert np.array_equal(info2[fl], info[fl])
    # the gages on these flags
    g = np.array(case.pr.gages, dtype=np.float64)
    ng = len(g)
    part, z = np.zeros((ng, 4)), np.zeros(ng)
    case.emu.call("sphx_wave_gages", part, g, ng, case.pos, info, case.hash, n, None)
    case.emu.call("sphx_wave_gages_finish", z, part, g, ng, None)
    cases.check_gages(case.pr, case.pos[:n], case.hash[:n], info, g, z, "hostemu")
    assert (part[g[:, 3] <= 0, 2] == 1.0).all() and np.isnan(z[3])
    part2, z2 = np.zeros((ng, 4)), np.zeros(ng)
    case.emu.call("sphx_wave_gages", part2, g, ng, case.pos, info, case.hash, n, None)
    case.emu.call("sphx_wave_gages_finish", z2, part2, g, ng, None)
    assert np.array_equal(part.view(np.uint64), part2.view(np.uint64)) and np.array_equal(z.view(np.uint64), z2.view(np.uint64))
    # a part of the rows (another grid, other partials): the rule on those rows; no flagged row at all: NaN / 0
    m = n//3
    case.emu.call("sphx_wave_gages", part, g, ng, case.pos, info, case.hash, m, None)
    case.emu.call("sphx_wave_gages_finish", z, part, g, ng, None)
    keep = g[:, 3] > 0
    cases.check_gages(case.pr, case.pos[:m], case.hash[:m], info[:m], g[keep], z[keep], "hostemu, a third of the rows")
    case.emu.call("sphx_wave_gages", part, g, ng, case.pos, case.info, case.hash, n, None)
    case.emu.call("sphx_wave_gages_finish", z, part, g, ng, None)
    assert np.isnan(z[g[:, 3] > 0]).all() and not z[g[:, 3] <= 0].any()


def test_gage_ties_inactive_rows_and_the_cap(case):
    """two flagged rows at the same distance of a nearest-mode gage: the lower row; an inactive flagged row does not count; 64 gages
    run, 65 are refused"""
    n = case.n
    fl = np.where(info_type(case.info[:n]) == D.PT_FLUID)[0]
    a, b = int(fl[10]), int(fl[400])
    info = case.info[:n].copy()
    info[[a, b], 0] |= D.FG_SURFACE
    gp = cases.global_pos_f64(case.pr, case.pos[:n], case.hash[:n])
    mid = 0.5*(gp[a] + gp[b])
    g = np.array([[mid[0], mid[1], 0.0, 0.0], [gp[b, 0], gp[b, 1], 0.0, 0.0], [mid[0], mid[1], 0.0, 10.0]])
    part, z = np.zeros((3, 4)), np.zeros(3)
    case.emu.call("sphx_wave_gages", part, g, 3, case.pos, info, case.hash, n, None)
    case.emu.call("sphx_wave_gages_finish", z, part, g, 3, None)
    ra, rb = np.hypot(*(gp[a, :2] - mid[:2])), np.hypot(*(gp[b, :2] - mid[:2]))
    want = gp[a, 2] if ra <= rb else gp[b, 2]
    assert z[0] == want and part[0, 3] == (a if ra <= rb else b) and z[1] == gp[b, 2] and part[1, 1] == 0.0
    pos = case.pos.copy()
    pos[b, 3] = np.nan
    case.emu.call("sphx_wave_gages", part, g, 3, pos, info, case.hash, n, None)
    case.emu.call("sphx_wave_gages_finish", z, part, g, 3, None)
    assert z[0] == gp[a, 2] and z[1] == gp[a, 2] and abs(z[2] - gp[a, 2]) < 1e-15      # (z W / W of the one particle left)
    many = np.tile(g[2], (65, 1))
    part, z = np.zeros((65, 4)), np.zeros(65)
    case.emu.call("sphx_wave_gages", part, many, 64, case.pos, info, case.hash, n, None)
    case.emu.call("sphx_wave_gages_finish", z, part, many, 64, None)
    assert np.abs(z[:64] - z[0]).max() == 0.0 and abs(z[0] - 0.5*(gp[a, 2] + gp[b, 2])) < 1e-9
    rc, msg = case.emu.rc("sphx_wave_gages", part, many, 65, case.pos, info, case.hash, n, None)
    assert rc == INVALID and "SPHX_MAX_GAGES" in msg


def test_vorticity(case):
    vort = np.zeros((case.n, 3), dtype=np.float32)
    case.post(D.VORTICITY, vort=vort, vel=case.vel)
    case.ref.vorticity(vort)


def test_still_refused(case):
    n = case.n
    info = case.info[:n].copy()
    rc, msg = case.emu.rc("sphx_postprocess", int(D.INTERFACE_DETECTION), None, None, info, None, case.pos, case.vel, case.info, case.hash,
                          case.cs, case.nl, n, n, 0.86, 0.5, None)
    assert rc == UNSUPPORTED and "INTERFACE_DETECTION" in msg and "SA_BOUNDARY" in msg
    assert np.array_equal(info, case.info[:n])
    out = np.zeros_like(case.vel)
    P = case.emu.params
    for ft in (D.SHEPARD_FILTER, D.MLS_FILTER):
        rc, msg = case.emu.rc("sphx_filter_process", int(ft), out, case.pos, case.vel, case.info, case.hash, case.cs, case.nl, n, n,
                              float(P.slength), float(P.influenceradius), None)
        assert rc == UNSUPPORTED and msg == "sphx_filter_process: only LJ/DYN boundaries are built"


def test_a_dyn_context_runs_the_kernels_it_ran(oracle_built):
    """DamBreak3D (DYN_BOUNDARY) with test points through the same entry point against the CPU oracle's non-SA post-processing, bit
    for bit (host libm on both sides here): the SA instantiations are chosen by the context's boundary type, a context without SA
    walls keeps the kernels it had (on the device: tests/test_gpu_parity.py test_postprocess_bit_exact)"""
    import oracle_lib as ol
    pts = [(0.2, 0.3, 0.2), (0.25, 0.35, 0.1), (1.2, 0.3, 0.3)]
    pr = DamBreak3D(deltap=0.05, obstacle=False, jitter=0.1, hydrostatic=False, testpoints=pts)
    sim = ol.OracleSim(pr)
    sim.build_neibs()
    n = sim.n
    rng = np.random.default_rng(9)
    vel = sim.vel.copy()
    vel[:, :3] += rng.uniform(-0.4, 0.4, size=(len(vel), 3)).astype(np.float32)
    vel[:, 3] += rng.uniform(0, 2e-3, size=len(vel)).astype(np.float32)
    emu = _Emu(pr.sphx_params(len(sim.pos)))
    tail = (sim.hash, sim.cs, sim.nl, n, n, 0.86, 0.5, None)
    vort = np.zeros((len(sim.pos), 3), dtype=np.float32)
    emu.call("sphx_postprocess", int(D.VORTICITY), vort, None, None, None, sim.pos, vel, sim.info, *tail)
    assert np.array_equal(vort[:n].view(np.uint32), sim.o.vorticity(sim.pos, vel, sim.info, sim.hash, sim.cs, sim.nl, n)[:n].view(np.uint32))
    info, nrm = sim.info.copy(), np.zeros((len(sim.pos), 4), dtype=np.float32)
    emu.call("sphx_postprocess", int(D.SURFACE_DETECTION), None, None, info, nrm, sim.pos, vel, sim.info, *tail)
    ref_info, ref_nrm = sim.o.surface(sim.pos, vel, sim.info, sim.hash, sim.cs, sim.nl, n, normals=True)
    assert np.array_equal(info[:n], ref_info[:n]) and ((info[:n, 0] & D.FG_SURFACE) != 0).sum() > 10
    assert np.array_equal(nrm[:n].view(np.uint32), ref_nrm[:n].view(np.uint32))
    got = vel.copy()
    emu.call("sphx_postprocess", int(D.TESTPOINTS), None, got, None, None, sim.pos, None, sim.info, *tail)
    want = sim.o.testpoints(sim.pos, vel, sim.info, sim.hash, sim.cs, sim.nl, n)
    tp = info_type(sim.info[:n]) == D.PT_TESTPOINT
    assert tp.sum() == 3 and np.array_equal(got[:n][tp].view(np.uint32), want[:n][tp].view(np.uint32))
    assert np.array_equal(got[:n][~tp].view(np.uint32), vel[:n][~tp].view(np.uint32))
    rc, msg = emu.rc("sphx_postprocess_testpoints_keps", got, vort, vort, sim.pos, sim.info, sim.hash, sim.cs, sim.nl, n, n, None)
    assert rc == INVALID and "SA_BOUNDARY" in msg
    emu.close()
