"""granular.hip over its own source on the CPU (tests/hostemu): the four passes of the effective-pressure solver against the
float64 restatement, and the fused solve against the loop over the passes, bit for bit.  This finds logic errors (flags, list
sections, sums, the counter, the two pressure arrays); the device build is held to the same in tests/test_gpu_granular.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpusph_amd import capi, defs as D
from gpusph_amd.problem import LithostaticColumn
import oracle_lib as ol
from granular_ref import GranularRef

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "hostemu")
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, "gpusph_amd", "csrc")
_SO = os.path.join(_EMU, "_build", "libsphx_emu_granular.so")
NAMES = ["sphx_create", "sphx_destroy", "sphx_set_constants", "sphx_last_error", "sphx_set_granular",
         "sphx_jacobi_fs_boundary_conditions", "sphx_jacobi_wall_boundary_conditions", "sphx_jacobi_build_vectors",
         "sphx_jacobi_update_effpres", "sphx_jacobi_solve"]


def _build():
    sources = [os.path.join(_EMU, "emu_granular.cc"), os.path.join(_EMU, "hip", "hip_runtime.h"), os.path.join(_ROOT, "include", "sphx.h")] + \
        [os.path.join(_CSRC, f) for f in ("sphx_api.hip", "granular.hip", "sphx_internal.h", "neib_iter.h")]
    os.makedirs(os.path.dirname(_SO), exist_ok=True)
    if os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(s) for s in sources):
        return _SO
    text = open(os.path.join(_CSRC, "granular.hip")).read()
    pat = re.compile(r'(\b\w+)<<<(.+?), (\w+), 0, ([^>;]+?)>>>\(')

    def launch(m):      # a block of one thread has no wave to meet: the plain serial launch
        if m.group(3) == "1":
            return "SPHX_EMU_LAUNCH((%s), %s, %s, " % (m.group(1), m.group(2), m.group(3))
        return "SPHX_LAUNCH_WAVES(%s, %s, %s, %s, " % (m.group(1), m.group(2), m.group(3), m.group(4))
    out, n = pat.subn(launch, text)
    assert n > 0 and "<<<" not in out
    with open(os.path.join(_EMU, "_build", "granular_emu.inc"), "w") as f:
        f.write(out)
    cmd = ["g++", "-O1", "-g0", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes",
           "-I" + _EMU, "-I" + os.path.join(_EMU, "_build"), "-I" + os.path.join(_ROOT, "include"), "-I" + _CSRC,
           "-o", _SO, os.path.join(_EMU, "emu_granular.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return _SO


class _Emu:
    def __init__(self, problem, n):
        self.lib = C.CDLL(_build())
        for name in NAMES:
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = capi.SIGNATURES[name]
        self.h = C.c_void_p()
        self._check(self.lib.sphx_create(C.byref(self.h), 0))
        self.params = problem.sphx_params(n)
        sinpsi = (C.c_float * 4)(*[float(np.float32(x)) for x in list(problem.physparams.sinpsi) + [0.0] * (4 - len(problem.physparams.sinpsi))])
        sp = problem.simparams
        self._check(self.lib.sphx_set_granular(self.h, sinpsi, int(sp.jacobi_maxiter), float(np.float32(sp.jacobi_backerr)),
                                               float(np.float32(sp.jacobi_residual))))
        self._check(self.lib.sphx_set_constants(self.h, C.byref(self.params)))

    def _check(self, rc):
        if rc != capi.SPHX_OK:
            raise RuntimeError("emulated libsphx: rc %d: %s" % (rc, self.lib.sphx_last_error().decode()))

    def call(self, name, *args):
        conv = [a.ctypes.data if isinstance(a, np.ndarray) else a for a in args]
        self._check(getattr(self.lib, name)(self.h, *conv))

    def close(self):
        self.lib.sphx_destroy(self.h)


class _Case:
    """a sorted state of the column with its neighbour list (the oracle's), a few particles disabled afterwards"""

    def __init__(self, **kw):
        self.pr = LithostaticColumn(0.05, jitter=0.15, **kw)
        sim = ol.OracleSim(self.pr)
        sim.build_neibs()
        n = self.n = sim.n
        self.pos, self.vel, self.info, self.hash, self.cs, self.nl = sim.pos.copy(), sim.vel, sim.info, sim.hash, sim.cs, sim.nl
        self.effpres0 = np.ascontiguousarray(self.pr.effpres0[sim.partindex][:n])
        rng = np.random.default_rng(99)
        self.pos[rng.choice(n, size=9, replace=False), 3] = np.nan        # disabled behind the list build: still in the lists
        self.ref = GranularRef(self.pr, self.pos[:n], self.hash[:n], self.vel[:n], self.info[:n])
        self.emu = _Emu(self.pr, len(self.pos))
        self.deltap = float(np.float32(self.pr.m_deltap))

    def state(self):
        return (self.pos, self.vel, self.info, self.hash, self.cs, self.nl)

    def loop(self, p):
        """preparation and the loop through the four entry points, the stop test on the host"""
        e, n, sp = self.emu, self.n, self.pr.simparams
        p = p.copy()
        jac = np.zeros((len(self.pos), 4), dtype=np.float32)
        err, res = C.c_float(0), C.c_float(0)
        e.call("sphx_jacobi_fs_boundary_conditions", p, self.pos, self.info, n, n, self.deltap, None)
        e.call("sphx_jacobi_wall_boundary_conditions", p, C.byref(err), *self.state(), n, n, self.deltap, None)
        counter = 0
        while True:
            e.call("sphx_jacobi_build_vectors", jac, p, *self.state(), n, n, None)
            e.call("sphx_jacobi_update_effpres", p, C.byref(res), jac, self.info, n, n, None)
            e.call("sphx_jacobi_wall_boundary_conditions", p, C.byref(err), *self.state(), n, n, self.deltap, None)
            if (err.value < np.float32(sp.jacobi_backerr) and res.value < np.float32(sp.jacobi_residual)) or counter > sp.jacobi_maxiter:
                return p, counter, err.value, res.value
            counter += 1

    def solve(self, p):
        p = p.copy()
        it, err, res = C.c_uint32(0), C.c_float(0), C.c_float(0)
        self.emu.call("sphx_jacobi_solve", p, *self.state(), self.n, self.n, self.deltap, C.byref(it), C.byref(err), C.byref(res), None)
        return p, it.value, err.value, res.value


@pytest.fixture(scope="module")
def case():
    c = _Case()
    yield c
    c.emu.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_passes_against_the_restatement(case):
    c, ref, n = case, case.ref, case.n
    rng = np.random.default_rng(5)
    p0 = rng.uniform(0.0, 4000.0, size=len(c.pos)).astype(np.float32)
    tol = 2e-5
    # Dirichlet rows
    p = p0.copy()
    c.emu.call("sphx_jacobi_fs_boundary_conditions", p, c.pos, c.info, n, n, c.deltap, None)
    want = ref.fs_boundary_conditions(p0[:n])
    assert ref.dirichlet.sum() > 100 and np.abs(p[:n] - want).max() <= tol * want.max()
    assert np.array_equal(_bits(p[:n][~ref.dirichlet]), _bits(p0[:n][~ref.dirichlet]))
    # wall rows
    p = p0.copy()
    err = C.c_float(0)
    c.emu.call("sphx_jacobi_wall_boundary_conditions", p, C.byref(err), *c.state(), n, n, c.deltap, None)
    want, want_err = ref.wall_boundary_conditions(p0[:n])
    assert np.abs(p[:n] - want).max() <= tol * np.abs(want).max()
    assert np.array_equal(_bits(p[:n][~ref.is_wall]), _bits(p0[:n][~ref.is_wall]))
    assert abs(err.value - want_err) <= tol * np.abs(want).max() / ref.refpres_wall
    # the vectors
    jac = np.full((len(c.pos), 4), 7.0, dtype=np.float32)
    c.emu.call("sphx_jacobi_build_vectors", jac, p0, *c.state(), n, n, None)
    Dv, Rx, B = ref.build_vectors(p0[:n])
    for got, w in ((jac[:n, 0], Dv), (jac[:n, 1], Rx), (jac[:n, 2], B)):
        assert np.abs(got[ref.active] - w[ref.active]).max() <= tol * np.abs(w).max()
    assert np.isnan(jac[:n, 3][ref.active]).all() and not jac[:n][~ref.active].any()
    assert not jac[:n, :3][ref.active & ~ref.interior].any() and (jac[:n, 0][ref.interior] != 0).all()
    # the update
    p = p0.copy()
    res = C.c_float(0)
    c.emu.call("sphx_jacobi_update_effpres", p, C.byref(res), jac, c.info, n, n, None)
    want, _ = ref.update_effpres(p0[:n], Dv, Rx, B)
    assert np.abs(p[:n] - want).max() <= tol * np.abs(want).max()
    assert np.array_equal(_bits(p[:n][~ref.interior]), _bits(p0[:n][~ref.interior]))
    # the residual is what rounding leaves of D p + Rx - B: half an ulp of each of the three terms and of the quotient
    bound = (4 * 2.0 ** -24 * (np.abs(Rx) + np.abs(B)) / ref.refpres_row)[ref.interior].max()
    assert 0.0 <= res.value <= bound


@pytest.mark.parametrize("which", ["converging", "cap", "no sediment"])
def test_fused_solve_gives_the_bits_of_the_loop(case, which):
    c = case
    if which == "no sediment":
        c = _Case(sediment_layers=0, water_layers=5)
        assert not c.ref.interior.any() and not c.ref.sed_fluid.any()
    sp = c.pr.simparams
    keep = (sp.jacobi_maxiter, sp.jacobi_backerr)
    if which == "cap":
        sp.jacobi_maxiter = 3
    if which == "converging":
        sp.jacobi_backerr = 3e-3      # the same path in fewer sweeps: the emulation runs every lane as a fibre
    try:
        sinpsi = (C.c_float * 4)(0, 0.5, 0, 0)
        c.emu._check(c.emu.lib.sphx_set_granular(c.emu.h, sinpsi, int(sp.jacobi_maxiter), float(np.float32(sp.jacobi_backerr)),
                                                 float(np.float32(sp.jacobi_residual))))
        p0 = np.zeros(len(c.pos), dtype=np.float32)
        p0[:c.n] = 0.0 if which != "no sediment" else c.effpres0
        want = c.loop(p0)
        got = c.solve(p0)
    finally:
        sp.jacobi_maxiter, sp.jacobi_backerr = keep
        if c is not case:
            c.emu.close()
    print(which, "counter %d backward error %g residual %g" % want[1:])
    assert got[1:] == want[1:]
    assert np.array_equal(_bits(got[0]), _bits(want[0]))
    if which == "cap":
        assert want[1] == 4
    if which == "converging":
        assert 3 < want[1] < 2000
    if which == "no sediment":
        assert want[1:] == (0, 0.0, 0.0)
