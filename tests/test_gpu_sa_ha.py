"""formulation<SPH_HA> with SA walls (BiFluidPoiseuilleSA's option set) on the GPU: the three list walkers on the device against
the float64 restatement (tests/sa_ha_ref.py) and against the host emulation of their own source, the tiling switch, one fluid
against SPH_F1, and whole steps of the SATwoFluidBox mirror.

The tank is SATwoFluidBox(0.05, jitter 0.1): 594 fluid particles of 2297, fluid 0 (rho0 = 4000) below fluid 1 (1000), rows next
to one, two and three walls (a vertex in a corner has gamma = 1/8).  The single-pass tests put the interface between the fourth
and the fifth of the six layers (interface = 0.225): with the default, half the depth, only the third layer of fluid 0 -- 35 rows --
is out of reach of every boundary element, and these tests ask for 50 such rows per fluid.  The runs use the default.
Bounds of the single-pass comparisons as in tests/test_sa_ha_hostemu.py; before SPH_HA + SA_BOUNDARY was built every test here
failed at sphx_set_constants."""
import types

import numpy as np
import pytest

from gpusph_amd import defs as D
from gpusph_amd.problem import SABox, SATwoFluidBox, info_id, info_type
import sa_ha_ref as R
from test_sa_ha_hostemu import EmuRun, TOL, TOL_ID, check_brezzi, check_density_sum, check_forces, displaced, perturbed

pytestmark = pytest.mark.gpu
KW = dict(deltap=0.05, jitter=0.1)


def _np(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _engine(problem, tiles, monkeypatch):
    """SPHX_DISABLE_TILES is read when a context is created"""
    import torch
    from gpusph_amd.engine import TimestepEngine
    assert torch.cuda.is_available()
    monkeypatch.setenv("SPHX_DISABLE_TILES", "0" if tiles else "1")
    # clobber_neibslist: the slots behind a section's end marker hold what the allocation held before; with the list cleared before
    # every build two engines of the same state have the same list to the bit (these tests compare them)
    return TimestepEngine(problem, device="cuda:0", clobber_neibslist=True)


def _tiles_usable(eng):
    return int(eng.k.lib.sphx_dbg_tiles_usable(eng.k.ctx.handle))


def _initialised(problem, tiles, monkeypatch):
    eng = _engine(problem, tiles, monkeypatch)
    eng.build_neibs()
    eng.sa_boundary_conditions(0)
    return eng


def _state(eng):
    """the engine's sorted state as the arrays of an OracleSaSim (what perturbed / displaced / EmuRun take); the list has the
    engine's stride, so the arrays keep the allocation's length"""
    n = eng.n
    s = types.SimpleNamespace(problem=eng.problem, n=n)
    s.pos, s.vel, s.gg, s.be = _np(eng.pos).copy(), _np(eng.vel).copy(), _np(eng.gradgamma).copy(), _np(eng.boundelements).copy()
    s.info = _np(eng.info).view(np.uint16).reshape(-1, 4).copy()
    s.hash = _np(eng.hash, np.uint32).copy()
    s.cs = _np(eng.cellStart, np.uint32).copy()
    s.nl = _np(eng.neibslist, np.uint16).copy()
    s.vertices = _np(eng.vertices, np.uint32).copy()
    s.vertpos = [_np(v).copy() for v in eng.vertpos]
    assert len(s.pos) == n, "these tests take an engine allocated for exactly its particles"
    return s


class DeviceRun:
    """the three passes of the engine's option set on the device, with the signatures of EmuRun"""

    def __init__(self, eng):
        self.eng = eng

    def _up(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.eng.device)

    def forces(self, vel):
        e, k, n = self.eng, self.eng.k, self.eng.n
        v = self._up(vel)
        k.memset(e.cfl, 0); k.memset(e.forces, 0)
        k.forces_sa(e.forces, e.cfl, e.pos, v, e.info, e.hash, e.cellStart, e.neibslist, e.gradgamma, e.boundelements, e.vertpos, n, 0, n, 0,
                    cfl_gamma=e.cfl_gamma)
        return _np(e.forces)[:n].copy()

    def density_sum(self, vel, new_pos):
        import torch
        e, k, n = self.eng, self.eng.k, self.eng.n
        v, p1 = self._up(vel), self._up(new_pos)
        nv, ng = v.clone(), torch.zeros_like(e.gradgamma)
        k.memset(e.forces, 0)
        k.sa_density_sum(nv, ng, e.forces, e.pos, p1, v, e.gradgamma, e.boundelements, e.vertpos, e.info, e.hash, e.cellStart, e.neibslist, n, n)
        return _np(nv)[:n].copy(), _np(ng)[:n].copy(), _np(e.forces)[:n, 3].copy()

    def brezzi(self, vel, dt):
        e, k, n = self.eng, self.eng.k, self.eng.n
        v = self._up(vel)
        k.memset(e.forces, 0)
        k.sa_density_diffusion(e.forces, e.pos, v, e.gradgamma, e.info, e.hash, e.cellStart, e.neibslist, n, n, float(np.float32(dt)))
        return _np(e.forces)[:n, 3].copy()


_CASE = {}


def _case(monkeypatch):
    """the tank of the single-pass tests, its perturbed state, the device's rows of the three passes and the restatement's geometry,
    once for the module"""
    if not _CASE:
        p = SATwoFluidBox(interface=0.225, **KW)
        eng = _initialised(p, True, monkeypatch)
        assert _tiles_usable(eng) == 0      # nothing of SPH_HA is tiled, whatever the switch says
        s = _state(eng)
        vel, new = perturbed(s), displaced(s)
        dt = float(np.float32(p.simparams.dt))
        run = DeviceRun(eng)
        _CASE.update(p=p, s=s, vel=vel, new=new, dt=dt, forces=run.forces(vel), dsum=run.density_sum(vel, new), brezzi=run.brezzi(vel, dt),
                     ref=R.ha_ref_of_state(p, s.pos, s.hash, s.info, s.vertices, s.be))
    return types.SimpleNamespace(**_CASE)


def test_the_three_passes_against_the_restatement(monkeypatch):
    c = _case(monkeypatch)
    p, s, ref = c.p, c.s, c.ref
    t = info_type(s.info)
    f = s.info[:, 1] >> 12
    fl = np.where(t == D.PT_FLUID)[0]
    # --- the inputs are not degenerate
    free = ~ref.has_element[fl]
    for k in (0, 1):
        assert (free & (f[fl] == k)).sum() >= 50, "fluid %d: %d rows with no element in reach" % (k, (free & (f[fl] == k)).sum())
    q = ref.pp["fluid"]
    other = np.zeros(len(s.info), dtype=bool); other[q["I"][f[q["I"]] != f[q["J"]]]] = True
    assert other[fl].sum() >= 50
    g = p.global_pos(s.pos, s.hash)
    dp = p.m_deltap
    near = (g[:, 0] < 1.5*dp).astype(int) + (g[:, 0] > p.l - 1.5*dp) + (g[:, 1] < 1.5*dp) + (g[:, 1] > p.w - 1.5*dp) + (g[:, 2] < 1.5*dp)
    for walls in (1, 2, 3):
        assert (near[fl] == walls).sum() >= 4
    assert np.abs(s.gg[t == D.PT_VERTEX, 3] - 0.125).min() < 5e-3
    # --- forces
    want, scale = check_forces(c.forces, ref, c.vel, s.pos[:, 3], s.gg[:, 3], fl, (p, s.pos, s.hash, s.be, s.vertpos), "device ")
    for k in ("fluid", "vertex", "element"):
        assert np.abs(want[k][fl]).max() >= 0.02*scale
    assert not c.forces[t != D.PT_FLUID].any()
    # --- density summation
    nv, ng, fw = c.dsum
    rho0 = np.asarray(p.physparams.rho0)[f]
    check_density_sum(fw, nv, ng, ref, c.vel, p.global_pos(c.new, s.hash), s.pos[:, 3], s.gg[:, 3], fl, rho0, "device ")
    # --- Brezzi
    wb, sb = check_brezzi(c.brezzi, ref, c.vel, s.pos[:, 3], s.gg[:, 3], c.dt, fl, "device ")
    assert np.abs(wb["fluid"][fl]).max() >= 0.02*sb and np.abs(wb["vertex"][fl]).max() >= 0.02*sb


def test_device_against_the_host_emulation_of_the_same_source(monkeypatch):
    c = _case(monkeypatch)
    s = c.s
    fl = np.where(info_type(s.info) == D.PT_FLUID)[0]
    emu = EmuRun(c.p, s)
    try:
        ef, (ev, eg, ew), eb = emu.forces(c.vel), emu.density_sum(c.vel, c.new), emu.brezzi(c.vel, c.dt)
    finally:
        emu.close()
    nv, ng, fw = c.dsum
    for name, got, want in (("forces", c.forces[fl, :3], ef[fl, :3]), ("volumic sum", fw[fl], ew[fl]), ("Brezzi", c.brezzi[fl], eb[fl]),
                            ("new density", (nv[fl, 3].astype(np.float64) + 1.0), (ev[fl, 3].astype(np.float64) + 1.0)),
                            ("new gamma", ng[fl, 3], eg[fl, 3])):      # (grad gamma, the closed form through two math libraries, is not the formulation's)
        scale = np.abs(want).max()
        err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
        print("%s: device against emulation %.3g of the scale %.3g" % (name, err/scale, scale))
        assert err <= 1e-5*scale, name


def test_the_tiling_switch_changes_nothing(monkeypatch):
    c = _case(monkeypatch)
    eng = _initialised(SATwoFluidBox(interface=0.225, **KW), False, monkeypatch)
    assert _tiles_usable(eng) == 0
    s = _state(eng)
    assert np.array_equal(_bits(s.pos), _bits(c.s.pos)) and np.array_equal(s.nl, c.s.nl) and np.array_equal(_bits(s.gg), _bits(c.s.gg))
    run = DeviceRun(eng)
    assert np.array_equal(_bits(run.forces(c.vel)), _bits(c.forces))
    for a, b in zip(run.density_sum(c.vel, c.new), c.dsum):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(run.brezzi(c.vel, c.dt)), _bits(c.brezzi))
    assert _tiles_usable(eng) == 0


def test_one_fluid_ha_against_f1_on_the_device(monkeypatch):
    """the identities of tests/test_sa_ha_ref.py on the device, walker against walker: the passes agree but for the vertex
    neighbours, and there the forces (and Brezzi) DIFFER, by what the restatement's vertex parts say"""
    c = _case(monkeypatch)
    out = {}
    for name, form in (("F1", D.SPH_F1), ("HA", D.SPH_HA)):
        p = SABox(**KW)
        p.simparams.sph_formulation = form
        eng = _initialised(p, False, monkeypatch)
        s = _state(eng)
        if name == "F1":
            vel = perturbed(s)
            vx = info_type(s.info) == D.PT_VERTEX      # noise on the vertices too: near their rest density the two forms weigh them alike
            vel[vx, 3] += (0.02*np.random.default_rng(47).standard_normal(int(vx.sum()))).astype(np.float32)
            new, dt, s1, p1 = displaced(s), float(np.float32(p.simparams.dt)), s, p
        else:
            assert np.array_equal(_bits(s.pos), _bits(s1.pos)) and np.array_equal(s.nl, s1.nl)
        run = DeviceRun(eng)
        out[name] = (run.forces(vel), run.density_sum(vel, new), run.brezzi(vel, dt))
    s = s1
    assert np.array_equal(_bits(s.pos[:, :3]), _bits(c.s.pos[:, :3]))      # the same lattice and jitter: the geometry is evaluated once
    ref = c.ref.for_problem(p1, s.info)
    fl = np.where(info_type(s.info) == D.PT_FLUID)[0]
    mass, gam = s.pos[:, 3], s.gg[:, 3]
    f_ha, f_f1 = out["HA"][0][:, :3].astype(np.float64), out["F1"][0][:, :3].astype(np.float64)
    dv = ref.forces("HA", vel, mass, gam)["vertex"] - ref.forces("F1", vel, mass, gam)["vertex"]
    scale = np.abs(f_f1[fl]).max()
    err = np.abs((f_ha - f_f1) - dv)[fl]
    novert = ~ref.has_vertex[fl]
    print("one fluid, forces: HA - F1 up to %.3g of the scale %.3g; beside the restatement's vertex part %.3g; %d rows with no vertex in reach: %.3g"
          % (np.abs(f_ha - f_f1)[fl].max()/scale, scale, err.max()/scale, novert.sum(), np.abs(f_ha - f_f1)[fl][novert].max()/scale))
    assert (err <= TOL_ID*scale).all()
    assert novert.sum() >= 50 and (np.abs(f_ha - f_f1)[fl][novert] <= TOL_ID*scale).all()
    assert np.abs(f_ha - f_f1)[fl][~novert].max() > 1e-3*scale and np.abs(dv[fl]).max() > 1e-3*scale
    rho0 = float(p1.physparams.rho0[0])
    d_ha, d_f1 = (out["HA"][1][0][fl, 3].astype(np.float64) + 1.0)*rho0, (out["F1"][1][0][fl, 3].astype(np.float64) + 1.0)*rho0
    print("one fluid, density summation: HA against F1 %.3g of the largest density" % (np.abs(d_ha - d_f1).max()/d_f1.max()))
    assert (np.abs(d_ha - d_f1) <= TOL_ID*d_f1.max()).all()
    assert np.array_equal(_bits(out["HA"][1][1]), _bits(out["F1"][1][1]))
    b_ha, b_f1 = out["HA"][2].astype(np.float64), out["F1"][2].astype(np.float64)
    bv = ref.brezzi("HA", vel, mass, gam, dt)["vertex"]
    scale = np.abs(b_f1[fl]).max()
    err = np.abs((b_ha - b_f1) - bv)[fl]
    print("one fluid, Brezzi: HA - F1 up to %.3g of the scale %.3g; beside the restatement's vertex part %.3g" % (np.abs(b_ha - b_f1)[fl].max()/scale, scale, err.max()/scale))
    assert (err <= TOL_ID*scale).all() and np.abs(bv[fl]).max() > 0.02*scale


def _slosh(eng):
    import torch
    n, p = eng.n, eng.problem
    g = p.global_pos(_np(eng.pos)[:n], _np(eng.hash, np.uint32)[:n])
    fl = info_type(_np(eng.info)[:n].view(np.uint16).reshape(-1, 4)) == D.PT_FLUID
    v = _np(eng.vel)[:n].copy()
    v[fl, 0] = 0.3*np.sin(np.pi*g[fl, 0]/p.l)*(g[fl, 2]/p.H)
    v[fl, 2] = -0.3*np.cos(np.pi*g[fl, 0]/p.l)*(g[fl, 2]/p.H)*0.5
    eng.vel[:n] = torch.from_numpy(v.astype(np.float32)).to(eng.device)


def _wall_rows_by_id(eng):
    n = eng.n
    info = _np(eng.info)[:n].view(np.uint16).reshape(-1, 4)
    w = info_type(info) != D.PT_FLUID
    order = np.argsort(info_id(info)[w])
    return _bits(_np(eng.pos)[:n][w][order]), _np(eng.hash, np.uint32)[:n][w][order]


@pytest.mark.parametrize("diffusion", [D.BREZZI, D.DENSITY_DIFFUSION_NONE], ids=["Brezzi", "no diffusion"])
def test_eight_steps_across_a_list_rebuild(diffusion, monkeypatch):
    p = SATwoFluidBox(density_diffusion=diffusion, **KW)
    p.simparams.buildneibsfreq = 4
    eng = _engine(p, True, monkeypatch)
    _slosh(eng)
    eng.build_neibs()
    walls0 = _wall_rows_by_id(eng)
    for _ in range(8):
        eng.step()
        assert _tiles_usable(eng) == 0
    n = eng.n
    assert np.isfinite(_np(eng.pos)[:n]).all() and np.isfinite(_np(eng.vel)[:n]).all() and np.isfinite(_np(eng.gradgamma)[:n]).all()
    dt = eng.current_dt()
    assert 0 < dt < 1e-2
    walls1 = _wall_rows_by_id(eng)
    assert np.array_equal(walls0[0], walls1[0]) and np.array_equal(walls0[1], walls1[1])
    speed = np.sqrt((_np(eng.vel)[:n, :3]**2).sum(axis=1)).max()
    print("eight steps: dt %.3g, largest speed %.3g" % (dt, speed))
    assert speed > 0.05


def test_brezzi_damps_density_noise_in_a_tank_at_rest(monkeypatch):
    """What the term is for (the pattern of test_gpu_sa_ferrari.py test_diffusion_damps_density_noise_in_a_tank_at_rest): a stratified
    tank at rest with 1e-3 of seeded density noise, 20 steps, with Brezzi and without: the rms deviation of the fluid's density from
    the hydrostatic one ends lower with the diffusion."""
    import torch
    rms = {}
    for diffusion in (D.BREZZI, D.DENSITY_DIFFUSION_NONE):
        eng = _engine(SATwoFluidBox(density_diffusion=diffusion, **KW), True, monkeypatch)
        n, p = eng.n, eng.problem
        fl = info_type(_np(eng.info)[:n].view(np.uint16).reshape(-1, 4)) == D.PT_FLUID
        v = _np(eng.vel)[:n].copy()
        hyd0 = v[fl, 3].copy()
        v[fl, 3] += (1e-3*np.random.default_rng(7).standard_normal(int(fl.sum()))).astype(np.float32)
        eng.vel[:n] = torch.from_numpy(v).to(eng.device)
        start = np.sqrt(((v[fl, 3] - hyd0)**2).mean())
        for _ in range(20):
            eng.step()
        g = p.global_pos(_np(eng.pos)[:n], _np(eng.hash, np.uint32)[:n])
        info = _np(eng.info)[:n].view(np.uint16).reshape(-1, 4)
        fl = info_type(info) == D.PT_FLUID
        rho = _np(eng.vel)[:n][fl, 3]
        assert np.isfinite(rho).all()
        rms[diffusion] = (np.sqrt(((rho - p.initial_density(g[fl]))**2).mean()), start)
    print("rms deviation from the hydrostatic density after 20 steps: Brezzi %.4g, no diffusion %.4g (seeded %.4g)"
          % (rms[D.BREZZI][0], rms[D.DENSITY_DIFFUSION_NONE][0], rms[D.BREZZI][1]))
    assert rms[D.BREZZI][0] < rms[D.DENSITY_DIFFUSION_NONE][0]


def test_stratified_tank_stays_at_rest(monkeypatch):
    """20 steps from rest: no fluid particle crosses the interface by more than deltap/2, and the largest speed stays below one per
    cent of c0 (a physical sanity bound: the design Mach number is 0.1)"""
    p = SATwoFluidBox(**KW)
    eng = _engine(p, True, monkeypatch)
    for _ in range(20):
        eng.step()
    n = eng.n
    info = _np(eng.info)[:n].view(np.uint16).reshape(-1, 4)
    fl = info_type(info) == D.PT_FLUID
    f = info[:, 1] >> 12
    z = p.global_pos(_np(eng.pos)[:n], _np(eng.hash, np.uint32)[:n])[:, 2]
    vel = _np(eng.vel)[:n]
    assert np.isfinite(z).all() and np.isfinite(vel).all()
    over0 = (z[fl & (f == 0)] - p.interface).max()
    under1 = (p.interface - z[fl & (f == 1)]).max()
    speed = np.sqrt((vel[fl, :3]**2).sum(axis=1)).max()
    c0 = float(p.physparams.sscoeff[0])
    print("stratified tank after 20 steps: fluid 0 up to %.3g deltap above the interface, fluid 1 up to %.3g deltap below; "
          "largest speed %.3g = %.3g c0" % (over0/p.m_deltap, under1/p.m_deltap, speed, speed/c0))
    assert over0 <= 0.5*p.m_deltap and under1 <= 0.5*p.m_deltap
    assert speed < 0.01*c0
