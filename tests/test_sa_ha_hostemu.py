"""formulation<SPH_HA> with SA walls (BiFluidPoiseuilleSA's option set) on the CPU: the list walkers' own source (sa_bounds.hip's
sa_forces_kernel, sa_density_sum_kernel, sa_density_diffusion_kernel, run by tests/hostemu one emulated thread after the other)
against the float64 all-pairs restatement of tests/sa_ha_ref.py on SATwoFluidBox(0.1, jitter 0.1): two fluids of densities 4000 and
1000, one layer of each.  The state: as the boundary conditions initialise it (OracleSaSim: neighbour phase, gamma, segment and
vertex conditions -- none of which depends on the formulation), then two per cent of seeded noise on the densities of fluid and
elements and a sheared velocity field.

Bound, as in tests/test_sa_ferrari_hostemu.py: 1e-4 of the largest magnitude of the pass for every row, and for a row with boundary
elements in reach twice what the float32 evaluation of |grad gamma_as| of ITS elements in the reference's operation order moves
the row by, on top.  The volumic sum of the density summation and the Brezzi pass have no element term: no allowance at all.  (The
volumic sum is the difference of two float32 sums that nearly cancel -- the displacement is 0.02 deltap; measured here, the worst
row is 2.7e-5 of the largest |sum| off, a tenth of what 2 N roundings of the partial sums could do at worst; the pass's result,
the new density, is held to 1e-4 of itself as well.)

The same three passes with ONE fluid (SABox with formulation<SPH_HA> against SPH_F1, both through the emulated library) to the
identities of tests/test_sa_ha_ref.py, 1e-5 of the scale (float against float): the passes agree but for the vertex neighbours,
and there they differ by what the restatement's vertex parts say.

All of it fails before SPH_HA + SA_BOUNDARY was built: sphx_set_constants refused the option set ("SPH_HA is built for DYN_BOUNDARY
and LAMINAR_FLOW")."""
import ctypes as C
import os

import numpy as np
import pytest

from gpusph_amd import defs as D
from gpusph_amd.problem import SABox, SATwoFluidBox, info_type
from hostemu_lib import Emu
import sa_ha_ref as R
from sa_helpers import OracleSaSim

TOL = 1e-4
TOL_ID = 1e-5


def perturbed(sim):
    """two per cent of seeded density noise on fluid and elements and a sheared velocity on the initialised state"""
    p = sim.problem
    t = info_type(sim.info)
    rng = np.random.default_rng(41)
    vel = sim.vel.copy()
    noisy = (t == D.PT_FLUID) | (t == D.PT_BOUNDARY)
    vel[noisy, 3] += (0.02*rng.standard_normal(int(noisy.sum()))).astype(np.float32)
    g = p.global_pos(sim.pos, sim.hash)
    fl = t == D.PT_FLUID
    vel[fl, 0] = (0.05*g[fl, 2]/p.H).astype(np.float32)
    vel[fl, 2] = (0.02*g[fl, 0]/p.l).astype(np.float32)
    return vel


def displaced(sim, amount=0.02):
    """the fluid particles moved by a seeded `amount` deltap (cell-local positions against the hashes of step n, as the Euler step
    leaves them)"""
    fl = info_type(sim.info) == D.PT_FLUID
    rng = np.random.default_rng(43)
    new = sim.pos.copy()
    new[fl, :3] += (amount*sim.problem.m_deltap*rng.uniform(-1.0, 1.0, size=(int(fl.sum()), 3))).astype(np.float32)
    return new


class EmuRun:
    """the three passes of a problem's option set through the emulated library on the arrays of an OracleSaSim"""

    def __init__(self, problem, sim):
        self.sim, self.n = sim, sim.n
        self.emu = Emu(problem.sphx_params(sim.n))
        self.P = self.emu.params
        self.dp = float(np.float32(problem.m_deltap))
        self.vp = [np.ascontiguousarray(v) for v in sim.vertpos]

    def close(self):
        self.emu.close()

    def forces(self, vel):
        s, n, P = self.sim, self.n, self.P
        out = np.zeros_like(s.vel)
        cfl = np.zeros(n + 64, dtype=np.float32)
        cflg = np.zeros(2*n + 128, dtype=np.float32)      # BUFFER_CFL_GAMMA: per particle, then per block
        hnb = C.c_uint32(0)
        self.emu.call("sphx_forces_basicstep_sa", out, cfl, cflg, s.pos, vel, s.info, s.hash, s.cs, s.nl, s.gg, s.be, self.vp[0], self.vp[1],
                      self.vp[2], n, 0, n, self.dp, float(P.slength), float(P.dtadaptfactor), float(P.influenceradius), 0, D.SIMULATE, 1, 0.0,
                      C.addressof(hnb), None)
        return out

    def density_sum(self, vel, new_pos):
        """-> (new velocity rows, new gamma rows, the volumic sum the walker leaves in FORCES.w)"""
        s, n, P = self.sim, self.n, self.P
        nv, ng = vel.copy(), np.zeros_like(s.gg)
        scratch = np.zeros_like(s.vel)
        self.emu.call("sphx_sa_density_sum", nv, ng, scratch, s.pos, new_pos, vel, s.gg, s.be, self.vp[0], self.vp[1], self.vp[2], s.info, s.hash,
                      s.cs, s.nl, n, n, 0.0, 1, 0.0, 5e-5, self.dp, float(P.slength), float(P.influenceradius), None)
        return nv, ng, scratch[:, 3].copy()

    def brezzi(self, vel, dt):
        s, n, P = self.sim, self.n, self.P
        f = np.zeros_like(s.vel)
        self.emu.call("sphx_sa_compute_density_diffusion", f, s.pos, vel, s.gg, s.info, s.hash, s.cs, s.nl, n, n, self.dp, float(P.slength),
                      float(P.influenceradius), float(np.float32(dt)), None)
        return f[:, 3].copy()


def check_forces(got, ref, vel, mass, gam, fl, shift_args, what=""):
    """force.xyz rows `got` against the restatement, componentwise; prints the worst row with and without allowance"""
    want = ref.forces("HA", vel, mass, gam)
    shift = ref.float32_shift(*shift_args)
    scale = np.abs(got[fl, :3]).max()
    err = np.abs(got[:, :3].astype(np.float64) - want["total"])[fl]
    allowance = 2.0*np.abs(shift)[fl]
    wall = ref.has_element[fl]
    over = (err - allowance).max(axis=1)
    print("%sforces: scale %.3g; parts fluid %.3g vertex %.3g element %.3g of it; worst row %.3g of the scale without allowance, %.3g beyond "
          "its allowance (largest %.3g), rows with no element in reach (%d of %d) %.3g; left with the oracle's float |grad gamma_as|: %.3g"
          % (what, scale, np.abs(want["fluid"][fl]).max()/scale, np.abs(want["vertex"][fl]).max()/scale, np.abs(want["element"][fl]).max()/scale,
             err.max()/scale, over.max()/scale, allowance.max()/scale, (~wall).sum(), len(fl), err[~wall].max()/scale if (~wall).any() else 0.0,
             np.abs(got[:, :3] - want["total"] - shift)[fl].max()/scale))
    assert (err <= TOL*scale + allowance).all(), "worst row %g of the scale beyond its allowance" % (over.max()/scale)
    assert (err[~wall] <= TOL*scale).all()
    return want, scale


def check_density_sum(fw, nv, ng, ref, vel, new_global, mass, old_gam, fl, rho0_of_row, what=""):
    vol, mag, cnt = ref.density_sum("HA", new_global, mass)
    scale = np.abs(fw[fl]).max()
    err = np.abs(fw.astype(np.float64) - vol)[fl]
    room = cnt[fl]*2.0**-24*mag[fl]
    print("%sdensity summation: largest |volumic sum| %.3g (largest sum of magnitudes %.3g, up to %d terms); worst row %.3g of it "
          "(2 N 2^-24 of the magnitudes would be up to %.3g)" % (what, scale, mag[fl].max(), cnt[fl].max(), err.max()/scale, room.max()/scale))
    assert (err <= TOL*scale).all()
    # the pass's result: rho = (gamma_old rho_old + sum)/gamma_new with the row's own rho0; gamma_new is the pass's own (a stored
    # value of exactly 1 or 0.1 may have been clamped after the division: rows with elements in reach are left out then)
    gnew = ng[fl, 3].astype(np.float64)
    usable = ~(((gnew == 1.0) | (gnew == np.float32(0.1))) & ref.has_element[fl])
    assert usable.sum() > 0.9*len(fl)
    r0 = rho0_of_row[fl]
    rho_old = (vel[fl, 3].astype(np.float64) + 1.0)*r0
    want = (old_gam[fl].astype(np.float64)*rho_old + vol[fl])/gnew
    got = (nv[fl, 3].astype(np.float64) + 1.0)*r0
    e2 = (np.abs(got - want)/np.abs(want))[usable]
    print("   new density: worst row %.3g of its own density" % e2.max())
    assert (e2 <= TOL).all()
    return vol, scale


def check_brezzi(got, ref, vel, mass, gam, dt, fl, what=""):
    want = ref.brezzi("HA", vel, mass, gam, dt)
    scale = np.abs(got[fl]).max()
    err = np.abs(got.astype(np.float64) - want["total"])[fl]
    print("%sBrezzi: scale %.3g; parts fluid %.3g vertex %.3g of it; worst row %.3g of the scale"
          % (what, scale, np.abs(want["fluid"][fl]).max()/scale, np.abs(want["vertex"][fl]).max()/scale, err.max()/scale))
    assert (err <= TOL*scale).all()
    return want, scale


@pytest.fixture(scope="module")
def two_fluids():
    p = SATwoFluidBox(0.1, jitter=0.1)
    sim = OracleSaSim(p)
    vel = perturbed(sim)
    ref = R.ha_ref_of_state(p, sim.pos, sim.hash, sim.info, sim.vertices, sim.be)
    run = EmuRun(p, sim)
    yield p, sim, vel, ref, run
    run.close()


def test_the_tank_has_two_fluids_side_by_side(two_fluids):
    p, sim, vel, ref, run = two_fluids
    t = info_type(sim.info)
    f = sim.info[:, 1] >> 12
    fl = t == D.PT_FLUID
    assert (f[fl] == 0).sum() >= 20 and (f[fl] == 1).sum() >= 20
    for kind in (D.PT_BOUNDARY, D.PT_VERTEX):
        assert (f[t == kind] == 0).any() and (f[t == kind] == 1).any()
    q = ref.pp["fluid"]
    assert (f[q["I"]] != f[q["J"]]).sum() > 100          # pairs across the interface
    m = sim.pos[:, 3]
    assert np.allclose(m[fl & (f == 0)], 4000.0*p.m_deltap**3, rtol=1e-6) and np.allclose(m[fl & (f == 1)], 1000.0*p.m_deltap**3, rtol=1e-6)
    P = run.P
    assert P.sph_formulation == D.SPH_HA and P.boundarytype == D.SA_BOUNDARY and P.numfluids == 2 and P.compvisc == D.DYNAMIC and P.avgop == D.HARMONIC
    assert P.simflags == D.ENABLE_MULTIFLUID | D.ENABLE_DTADAPT | D.ENABLE_DENSITY_SUM and P.densitydiffusiontype == D.BREZZI


def test_forces_walker_against_the_restatement(two_fluids):
    p, sim, vel, ref, run = two_fluids
    fl = np.where(info_type(sim.info) == D.PT_FLUID)[0]
    got = run.forces(vel)
    want, scale = check_forces(got, ref, vel, sim.pos[:, 3], sim.gg[:, 3], fl, (p, sim.pos, sim.hash, sim.be, sim.vertpos))
    for k in ("fluid", "vertex", "element"):
        assert np.abs(want[k][fl]).max() > 0.02*scale
    assert not got[info_type(sim.info) != D.PT_FLUID].any()
    # the formulation matters here: the F1 form of the same state is far away
    f1 = ref.forces("F1", vel, sim.pos[:, 3], sim.gg[:, 3])["total"]
    assert np.abs(f1 - want["total"])[fl].max() > 0.05*scale


def test_density_sum_walker_against_the_restatement(two_fluids):
    p, sim, vel, ref, run = two_fluids
    fl = np.where(info_type(sim.info) == D.PT_FLUID)[0]
    new = displaced(sim)
    nv, ng, fw = run.density_sum(vel, new)
    rho0 = np.asarray(p.physparams.rho0)[sim.info[:, 1] >> 12]
    vol, scale = check_density_sum(fw, nv, ng, ref, vel, p.global_pos(new, sim.hash), sim.pos[:, 3], sim.gg[:, 3], fl, rho0)
    f1, _, _ = ref.density_sum("F1", p.global_pos(new, sim.hash), sim.pos[:, 3])
    assert np.abs(f1 - vol)[fl].max() > 0.05*scale
    # wall rows: gamma copied, density untouched
    w = info_type(sim.info) != D.PT_FLUID
    assert np.array_equal(ng[w].view(np.uint32), sim.gg[w].view(np.uint32)) and np.array_equal(nv[w].view(np.uint32), vel[w].view(np.uint32))


def test_brezzi_walker_against_the_restatement(two_fluids):
    p, sim, vel, ref, run = two_fluids
    fl = np.where(info_type(sim.info) == D.PT_FLUID)[0]
    dt = float(np.float32(p.simparams.dt))
    got = run.brezzi(vel, dt)
    want, scale = check_brezzi(got, ref, vel, sim.pos[:, 3], sim.gg[:, 3], dt, fl)
    assert np.abs(want["fluid"][fl]).max() > 0.02*scale and np.abs(want["vertex"][fl]).max() > 0.02*scale
    assert not got[info_type(sim.info) != D.PT_FLUID].any()


def single_fluid_problem(formulation):
    p = SABox(0.1, jitter=0.1)
    p.simparams.sph_formulation = formulation
    return p


def test_one_fluid_ha_equals_f1_but_for_the_vertices():
    """the identities of tests/test_sa_ha_ref.py through the emulated library"""
    p1, pa = single_fluid_problem(D.SPH_F1), single_fluid_problem(D.SPH_HA)
    sim = OracleSaSim(p1)
    vel = perturbed(sim)
    # the vertices near their rest density weigh the two forms alike to a few 1e-4: some noise on them makes the difference plain
    vx = info_type(sim.info) == D.PT_VERTEX
    vel[vx, 3] += (0.02*np.random.default_rng(47).standard_normal(int(vx.sum()))).astype(np.float32)
    ref = R.ha_ref_of_state(p1, sim.pos, sim.hash, sim.info, sim.vertices, sim.be)
    fl = np.where(info_type(sim.info) == D.PT_FLUID)[0]
    mass, gam = sim.pos[:, 3], sim.gg[:, 3]
    new = displaced(sim)
    dt = float(np.float32(p1.simparams.dt))
    out = {}
    for name, p in (("F1", p1), ("HA", pa)):
        run = EmuRun(p, sim)
        try:
            out[name] = (run.forces(vel), run.density_sum(vel, new), run.brezzi(vel, dt))
        finally:
            run.close()
    # forces: HA - F1 is the difference of the vertex parts
    f_ha, f_f1 = out["HA"][0][:, :3].astype(np.float64), out["F1"][0][:, :3].astype(np.float64)
    rh, r1 = ref.forces("HA", vel, mass, gam), ref.forces("F1", vel, mass, gam)
    scale = np.abs(f_f1[fl]).max()
    dv = rh["vertex"] - r1["vertex"]
    err = np.abs((f_ha - f_f1) - dv)[fl]
    print("one fluid, forces: HA - F1 is up to %.3g of the scale %.3g; it differs from the restatement's vertex part by %.3g of the scale"
          % (np.abs(f_ha - f_f1)[fl].max()/scale, scale, err.max()/scale))
    assert (err <= TOL_ID*scale).all()
    assert np.abs(dv[fl]).max() > 1e-3*scale and np.abs(f_ha - f_f1)[fl].max() > 1e-3*scale
    # density summation: the same density
    rho0 = float(p1.physparams.rho0[0])
    d_ha, d_f1 = (out["HA"][1][0][fl, 3].astype(np.float64) + 1.0)*rho0, (out["F1"][1][0][fl, 3].astype(np.float64) + 1.0)*rho0
    print("one fluid, density summation: HA against F1 %.3g of the largest density" % (np.abs(d_ha - d_f1).max()/d_f1.max()))
    assert (np.abs(d_ha - d_f1) <= TOL_ID*d_f1.max()).all()
    assert np.array_equal(out["HA"][1][1].view(np.uint32), out["F1"][1][1].view(np.uint32))          # gamma: not the formulation's
    # Brezzi: HA - F1 is the vertex part
    b_ha, b_f1 = out["HA"][2].astype(np.float64), out["F1"][2].astype(np.float64)
    bv = ref.brezzi("HA", vel, mass, gam, dt)["vertex"]
    scale = np.abs(b_f1[fl]).max()
    err = np.abs((b_ha - b_f1) - bv)[fl]
    print("one fluid, Brezzi: HA - F1 is up to %.3g of the scale %.3g; it differs from the restatement's vertex part by %.3g of the scale"
          % (np.abs(b_ha - b_f1)[fl].max()/scale, scale, err.max()/scale))
    assert (err <= TOL_ID*scale).all()
    assert np.abs(bv[fl]).max() > 0.02*scale


def _refused(**change):
    p = SATwoFluidBox(0.1)
    for k, v in change.items():
        setattr(p.simparams, k, v)
    p.physparams.rheologytype = p.simparams.rheologytype
    return p.sphx_params(p.num_particles)


BASE = D.ENABLE_MULTIFLUID | D.ENABLE_DTADAPT | D.ENABLE_DENSITY_SUM
REFUSALS = [
    ("continuity equation", dict(simflags=D.ENABLE_MULTIFLUID | D.ENABLE_DTADAPT), "continuity equation is not built"),
    ("gamma quadrature", dict(simflags=BASE | D.ENABLE_GAMMA_QUADRATURE), "ENABLE_GAMMA_QUADRATURE is not built"),
    ("Ferrari", dict(densitydiffusiontype=D.FERRARI), "Ferrari density diffusion is not built"),
    ("k-epsilon", dict(turbmodel=D.KEPSILON), "k-epsilon model is not built"),
    ("open boundaries", dict(simflags=BASE | D.ENABLE_INLET_OUTLET), "open boundaries are not built"),
    ("moving bodies", dict(simflags=BASE | D.ENABLE_MOVING_BODIES), "moving bodies are not built"),
    ("repacking", dict(simflags=BASE | D.ENABLE_REPACKING), "repacking is not built"),
    ("GRANULAR", dict(rheologytype=D.GRANULAR), "GRANULAR rheology .LithostaticSA. is not built"),
]


@pytest.mark.parametrize("change,message", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_set_constants_refuses_what_is_not_built(change, message):
    from gpusph_amd import capi
    with pytest.raises(RuntimeError, match="rc %d: sphx: SPH_HA with SA_BOUNDARY: .*%s" % (capi.SPHX_ERR_UNSUPPORTED, message)):
        Emu(_refused(**change))


@pytest.mark.parametrize("diffusion", [D.BREZZI, D.DENSITY_DIFFUSION_NONE])
def test_the_accepted_set_runs_over_an_empty_range(diffusion):
    p = SATwoFluidBox(0.1, density_diffusion=diffusion)
    emu = Emu(p.sphx_params(p.num_particles))
    P = emu.params
    try:
        a = np.zeros((4, 4), dtype=np.float32)
        b = np.zeros((4, 4), dtype=np.float32)
        u = np.zeros(16, dtype=np.uint32)
        v2 = np.zeros((4, 2), dtype=np.float32)
        nl = np.zeros(4*P.neiblistsize, dtype=np.uint16)
        hnb = C.c_uint32(7)
        dp, h, R_ = float(np.float32(p.m_deltap)), float(P.slength), float(P.influenceradius)
        emu.call("sphx_forces_basicstep_sa", a, a[:, 0].copy(), np.zeros(16, np.float32), a, a, u, u, u, nl, a, a, v2, v2, v2, 0, 0, 0, dp, h,
                 float(P.dtadaptfactor), R_, 0, D.SIMULATE, 1, 0.0, C.addressof(hnb), None)
        assert hnb.value == 0
        emu.call("sphx_sa_density_sum", a, b, a, a, a, a, a, a, v2, v2, v2, u, u, u, nl, 0, 0, 0.0, 1, 0.0, 5e-5, dp, h, R_, None)
        if diffusion == D.BREZZI:
            emu.call("sphx_sa_compute_density_diffusion", a, a, a, a, u, u, u, nl, 0, 0, dp, h, R_, 1e-4, None)
        else:
            with pytest.raises(RuntimeError, match="built for Brezzi diffusion with density summation"):
                emu.call("sphx_sa_compute_density_diffusion", a, a, a, a, u, u, u, nl, 0, 0, dp, h, R_, 1e-4, None)
        with pytest.raises(RuntimeError, match="SPH_HA needs deltap"):
            emu.call("sphx_sa_density_sum", a, b, a, a, a, a, a, a, v2, v2, v2, u, u, u, nl, 0, 0, 0.0, 1, 0.0, 5e-5, 0.0, h, R_, None)
    finally:
        emu.close()


def test_more_than_one_domain_is_refused():
    from gpusph_amd.multigpu import MultiGpuEngine
    with pytest.raises(NotImplementedError, match="SPH_HA with SA_BOUNDARY is built for a single domain"):
        MultiGpuEngine(SATwoFluidBox(0.1), "cpu", 0, 2)


import host_case as hc      # noqa: E402

_FRAMEWORK_CHECK = {}


def _framework_check(case, tmp_root):
    """framework_check of THIS checkout's gpusph_amd/host/problem_setup.h on a case file -> its JSON.  The program build() left under
    oracle/_ref/host is taken if it knows the framework; one that was built from an older problem_setup.h (a copy of oracle/_ref that
    travelled with another build) answers "unknown framework case": then the same recipe (oracle/Makefile, target framework_check)
    builds the program from this checkout into a temporary directory, once, where the GPUSPH tree is present -- the test never
    passes on a program that does not hold the expression under test, and never skips because of a stale one."""
    import json
    import subprocess
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(hc.ROOT, "gpusph_amd") + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    exe = _FRAMEWORK_CHECK.get("exe", hc.exe("framework_check"))
    r = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=120, env=env)
    if r.returncode != 0 and "unknown framework case" in r.stderr and "exe" not in _FRAMEWORK_CHECK:
        out = os.path.join(str(tmp_root), "host")
        exe = os.path.join(out, "framework_check")
        m = subprocess.run(["make", "-s", "-C", os.path.join(hc.ROOT, "oracle"), exe, "HOUT=" + out], capture_output=True, text=True, timeout=900)
        if m.returncode != 0 and not os.path.isdir(os.environ.get("REF", "/root/reference")):
            pytest.skip("oracle/_ref/host/framework_check predates this framework and the GPUSPH tree is absent: nothing to build it from")
        assert m.returncode == 0, "oracle/_ref/host/framework_check predates this framework and could not be rebuilt:\n" + m.stdout + m.stderr
        _FRAMEWORK_CHECK["exe"] = exe
        r = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout)


@pytest.mark.skipif(not os.path.exists(os.path.join(hc.HOST_DIR, "framework_check")),
                    reason="oracle/_ref/host not built (build() makes it where the GPUSPH tree is present)")
@pytest.mark.parametrize("rhodiff", [D.BREZZI, D.DENSITY_DIFFUSION_NONE])
def test_bifluid_poiseuille_sa_framework_and_constants(tmp_path, tmp_path_factory, rhodiff):
    """the framework BiFluidPoiseuilleSA's own SETUP_FRAMEWORK expression builds against the SATwoFluidBox mirror: options and every
    uploaded constant.  The reference's problem is periodic in x and y; the mirror is a closed tank, so the periodicity is put on
    for the comparison (no particle of the tank uses it)."""
    from test_intree_boundary import assert_options, assert_params
    prob = SATwoFluidBox(0.05, density_diffusion=rhodiff)
    prob.simparams.periodicbound = D.PERIODIC_X | D.PERIODIC_Y
    case = tmp_path / "case.txt"
    case.write_text("\n".join(hc.case_lines(prob, "BiFluidPoiseuilleSA", rhodiff=rhodiff)) + "\n")
    if "tmp" not in _FRAMEWORK_CHECK:
        _FRAMEWORK_CHECK["tmp"] = tmp_path_factory.mktemp("framework_check")
    out = _framework_check(case, _FRAMEWORK_CHECK["tmp"])
    assert_options(out, prob.simparams)
    o = out["options"]
    assert o["sph_formulation"] == D.SPH_HA and o["boundarytype"] == D.SA_BOUNDARY and o["is_const_visc"] == 0
    assert o["simflags"] == D.ENABLE_MULTIFLUID | D.ENABLE_DTADAPT | D.ENABLE_DENSITY_SUM and o["densitydiffusiontype"] == rhodiff
    assert (o["compvisc"], o["viscmodel"], o["viscavgop"]) == (D.DYNAMIC, D.MORRIS, D.HARMONIC)
    assert out["engines"]["bc"] == 1
    assert_params(out, prob, prob.num_particles)
