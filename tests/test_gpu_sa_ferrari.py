"""Ferrari density diffusion in the continuity-equation form with SA walls (Spheric2SA's option set) on the GPU, through the three
ways the SA forces pass runs: the list walker against the float64 all-pairs restatement (tests/sa_ferrari_ref.py), the tiled window
+ the one-element-per-lane wall kernel against the walker, whole steps of both, and what the term is for.

The tank is SABox(0.05, jitter 0.1): 594 fluid particles of 2297, with rows next to one, two and three walls (a vertex in a
corner has gamma = 1/8), rows at the free surface and rows with no boundary element in reach; the tiling engages at this size
(as in tests/test_gpu_sa.py).  Bound of the single-pass comparisons, as in tests/test_sa_ferrari_hostemu.py: 1e-4 of the largest
|force.w| of the pass, plus, for a row with elements in reach, twice what the float evaluation of |grad gamma_as| of its own
elements in the reference's operation order moves the row by."""
import numpy as np
import pytest

from gpusph_amd import defs as D
from gpusph_amd.problem import SABox, SAPaddleBox, info_type
from sa_ferrari_ref import ferrari_ref_of_state, float32_shift
from sa_helpers import assert_close_but_for_gamma_spikes

pytestmark = pytest.mark.gpu
TOL = 1e-4
KW = dict(deltap=0.05, jitter=0.1, options="Spheric2SA")


def _np(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _problem(cls=SABox, diffusion=True, viscosity="DYNAMICVISC", **kw):
    p = cls(viscosity=viscosity, **dict(KW, **kw))
    if not diffusion:      # the same framework line without densitydiffusion<FERRARI>
        p.simparams.densitydiffusiontype = D.DENSITY_DIFFUSION_NONE
    return p


def _engine(problem, tiles, monkeypatch, **kw):
    """SPHX_DISABLE_TILES is read when a context is created"""
    import torch
    from gpusph_amd.engine import TimestepEngine
    assert torch.cuda.is_available()
    monkeypatch.setenv("SPHX_DISABLE_TILES", "0" if tiles else "1")
    return TimestepEngine(problem, device="cuda:0", **kw)


def _tiles_usable(eng):
    return int(eng.k.lib.sphx_dbg_tiles_usable(eng.k.ctx.handle))


def _initialised(problem, tiles, monkeypatch):
    eng = _engine(problem, tiles, monkeypatch)
    eng.build_neibs()
    assert _tiles_usable(eng) == (1 if tiles else 0)      # which kernels run: no silent fall-back either way
    eng.sa_boundary_conditions(0)
    return eng


def _perturbed(eng, vertex_noise=0.0):
    """two per cent of seeded density noise on fluid and elements and a sheared velocity field on the state the boundary
    conditions initialised; vertex_noise: on top, noise on the densities of the VERTICES alone"""
    n, p = eng.n, eng.problem
    info = _np(eng.info)[:n].view(np.uint16).reshape(-1, 4)
    t = info_type(info)
    vel = _np(eng.vel)[:n].copy()
    rng = np.random.default_rng(41)
    noisy = (t == D.PT_FLUID) | (t == D.PT_BOUNDARY)
    vel[noisy, 3] += (0.02*rng.standard_normal(int(noisy.sum()))).astype(np.float32)
    g = p.global_pos(_np(eng.pos)[:n], _np(eng.hash, np.uint32)[:n])
    fl = t == D.PT_FLUID
    vel[fl, 0] = (0.05*g[fl, 2]/p.H).astype(np.float32)
    vel[fl, 2] = (0.02*g[fl, 0]/p.l).astype(np.float32)
    if vertex_noise:
        vx = t == D.PT_VERTEX
        vel[vx, 3] += (vertex_noise*np.random.default_rng(43).standard_normal(int(vx.sum()))).astype(np.float32)
    return vel


def _forces(eng, vel):
    """one forces pass of the engine's option set on the given velocity / density rows -> (force rows, k-epsilon rows)"""
    import torch
    n, k = eng.n, eng.k
    eng.vel[:n] = torch.from_numpy(vel).to(eng.device)
    k.memset(eng.cfl, 0)
    if eng.keps:
        k.memset(eng.cfl_keps, 0); k.memset(eng.dkde, 0)
        k.forces_sa_keps(eng.forces, eng.cfl, eng.cfl_keps, eng.dkde, eng.pos, eng.vel, eng.info, eng.hash, eng.cellStart, eng.neibslist,
                         eng.gradgamma, eng.boundelements, eng.vertpos, eng.ke, n, 0, n, 0)
        return _np(eng.forces)[:n].copy(), _np(eng.dkde)[:n].copy()
    k.forces_sa(eng.forces, eng.cfl, eng.pos, eng.vel, eng.info, eng.hash, eng.cellStart, eng.neibslist, eng.gradgamma,
                eng.boundelements, eng.vertpos, n, 0, n, 0)
    return _np(eng.forces)[:n].copy(), None


_REF = {}


def _restatement(eng):
    """the float64 geometry of the tank (every fluid-element pair's |grad gamma_as|), evaluated once for the module: every engine
    of these tests starts from the same sorted state"""
    n = eng.n
    pos, hash_ = _np(eng.pos)[:n].copy(), _np(eng.hash, np.uint32)[:n].copy()
    if "ref" not in _REF:
        info = _np(eng.info)[:n].view(np.uint16).reshape(-1, 4).copy()
        _REF.update(pos=pos, hash=hash_, info=info, ref=ferrari_ref_of_state(
            eng.problem, pos, hash_, info, _np(eng.vertices, np.uint32)[:n], _np(eng.boundelements)[:n]))
    assert np.array_equal(_bits(pos), _bits(_REF["pos"])) and np.array_equal(hash_, _REF["hash"])
    return _REF["ref"], _REF["info"]


def _allowance(ref, eng):
    n = eng.n
    return 2.0*np.abs(float32_shift(ref, eng.problem, _np(eng.pos)[:n], _np(eng.hash, np.uint32)[:n], _np(eng.boundelements)[:n],
                                    [_np(v)[:n] for v in eng.vertpos]))


@pytest.mark.parametrize("viscosity", ["DYNAMICVISC", "KEPSVISC"])
def test_walker_against_the_restatement(viscosity, monkeypatch):
    """force.w(Ferrari) - force.w(no diffusion) of sa_forces_kernel<KEPS> on the device against the float64 sums; force.xyz and
    the k-epsilon rows do not see the term"""
    eng = _initialised(_problem(viscosity=viscosity), False, monkeypatch)
    ref, info = _restatement(eng)
    vel = _perturbed(eng)
    with_d, dk1 = _forces(eng, vel)
    gam = _np(eng.gradgamma)[:eng.n, 3].copy()
    mass = _np(eng.pos)[:eng.n, 3].copy()
    off = _initialised(_problem(viscosity=viscosity, diffusion=False), False, monkeypatch)
    without, dk0 = _forces(off, vel)
    t = info_type(info)
    fl = np.where(t == D.PT_FLUID)[0]
    # the tank has what the issue asks for: a corner (vertex gamma 1/8, fluid rows that see three walls), the free surface, the bulk
    g = eng.problem.global_pos(_REF["pos"], _REF["hash"])
    dp, pr = eng.problem.m_deltap, eng.problem
    near = (g[:, 0] < 1.5*dp).astype(int) + (g[:, 0] > pr.l - 1.5*dp) + (g[:, 1] < 1.5*dp) + (g[:, 1] > pr.w - 1.5*dp) + (g[:, 2] < 1.5*dp)
    assert np.abs(gam[t == D.PT_VERTEX] - 0.125).min() < 5e-3 and (near[fl] == 3).sum() >= 4 and gam[fl].min() < 0.9
    assert (g[fl, 2] > eng.problem.water_level - 0.8*eng.problem.m_deltap).sum() > 50
    fs, es, _ = ref.sums(vel[:, 3], mass, gam)
    allowance = _allowance(ref, eng)[fl]
    assert 50 < (es[fl] == 0).sum() < len(fl) - 50
    want = fs + es
    got = with_d[:, 3].astype(np.float64) - without[:, 3]
    scale = np.abs(with_d[fl, 3]).max()
    err = np.abs(got - want)[fl]
    away = es[fl] == 0
    print("%s: Ferrari part max %.3g of max |force.w| %.3g; error: rows without elements %.3g of the scale, rows with %.3g (allowance up to %.3g)"
          % (viscosity, np.abs(want[fl]).max(), scale, err[away].max()/scale, err[~away].max()/scale, allowance.max()/scale))
    assert np.abs(fs[fl]).max() > 0.05*scale and np.abs(es[fl]).max() > 0.02*scale
    assert (err[away] <= TOL*scale).all()
    assert (err <= TOL*scale + allowance).all(), "worst row %g of the scale" % (err/scale).max()
    assert np.array_equal(_bits(with_d[:, :3]), _bits(without[:, :3])) and np.abs(with_d[fl, :3]).max() > 0
    assert not with_d[t != D.PT_FLUID].any()
    if viscosity == "KEPSVISC":
        assert np.array_equal(_bits(dk1), _bits(dk0)) and dk1.any()


def test_tiled_window_and_wall_kernel_against_the_walker(monkeypatch):
    """the Ferrari part as forces_tile_kernel<.., DIFF_FERRARI> + sa_forces_wall_kernel form it against the walker's, laminar; and a
    perturbation of the VERTEX densities alone moves it in neither path (the vertex section stands where the tile lists have
    their boundary section: those rows run with the diffusion switched off)"""
    part, part_v, full = {}, {}, {}
    for tiles in (True, False):
        on = _initialised(_problem(), tiles, monkeypatch)
        off = _initialised(_problem(diffusion=False), tiles, monkeypatch)
        vel, vel_v = _perturbed(on), _perturbed(on, vertex_noise=0.02)
        f_on, f_off = _forces(on, vel)[0], _forces(off, vel)[0]
        part[tiles] = f_on[:, 3].astype(np.float64) - f_off[:, 3]
        full[tiles] = f_on
        part_v[tiles] = _forces(on, vel_v)[0][:, 3].astype(np.float64) - _forces(off, vel_v)[0][:, 3]
        if tiles:
            ref, info = _restatement(on)
            allowance = _allowance(ref, on)
    fl = np.where(info_type(info) == D.PT_FLUID)[0]
    scale = np.abs(full[False][fl, 3]).max()
    err = np.abs(part[True] - part[False])[fl]
    print("tiled + wall kernel against the walker, Ferrari part: worst row %.3g of the scale (allowance up to %.3g)"
          % (err.max()/scale, allowance[fl].max()/scale))
    assert np.abs(part[False][fl]).max() > 0.2*scale
    assert (err <= TOL*scale + allowance[fl]).all(), "worst row %g of the scale" % (err/scale).max()
    away = allowance[fl] == 0
    assert away.sum() > 50 and (err[away] <= TOL*scale).all()
    for tiles in (True, False):
        moved = np.abs(part_v[tiles] - part[tiles])[fl]
        print("vertex densities perturbed, %s: the Ferrari part moves by %.3g of the scale" % ("tiled" if tiles else "walker", moved.max()/scale))
        assert (moved <= TOL*scale).all()


def _slosh(eng):
    import torch
    n, p = eng.n, eng.problem
    g = p.global_pos(_np(eng.pos)[:n], _np(eng.hash, np.uint32)[:n])
    fl = info_type(_np(eng.info)[:n].view(np.uint16).reshape(-1, 4)) == D.PT_FLUID
    v = _np(eng.vel)[:n].copy()
    v[fl, 0] = 0.3*np.sin(np.pi*g[fl, 0]/p.l)*(g[fl, 2]/p.H)
    v[fl, 2] = -0.15*np.cos(np.pi*g[fl, 0]/p.l)*(g[fl, 2]/p.H)
    eng.vel[:n] = torch.from_numpy(v.astype(np.float32)).to(eng.device)
    return fl


def test_six_steps_through_both_paths_across_a_rebuild(monkeypatch):
    """the laminar set from a sloshing start, tiled against list walkers, to the trajectory tolerances of
    tests/test_gpu_sa.py test_sa_tiled_kernels_agree_with_the_list_walkers; the list is rebuilt before the fifth step"""
    out = {}
    for tiles in (True, False):
        p = _problem()
        p.simparams.buildneibsfreq = 4
        eng = _engine(p, tiles, monkeypatch)
        fl = _slosh(eng)
        usable = []
        for _ in range(6):
            eng.step()
            usable.append(_tiles_usable(eng))
        assert usable == [1 if tiles else 0]*6
        n = eng.n
        out[tiles] = (_np(eng.pos)[:n].copy(), _np(eng.vel)[:n].copy(), _np(eng.gradgamma)[:n].copy(), _np(eng.hash, np.uint32)[:n].copy(),
                      eng.current_dt(), fl, float(np.min(p.m_cellsize)))
    (pos_t, vel_t, gg_t, hash_t, dt_t, fl, cell), (pos_w, vel_w, gg_w, hash_w, dt_w, _, _) = out[True], out[False]
    assert np.isfinite(vel_t).all() and np.isfinite(vel_w).all() and np.array_equal(hash_t, hash_w)
    vmax = np.abs(vel_w[:, :3]).max()
    assert vmax > 0.2
    assert_close_but_for_gamma_spikes(pos_t[:, :3], pos_w[:, :3], 2e-5, cell, frac=0.002, spike=2.0, what="positions, tiled against list walkers (Ferrari)")
    assert_close_but_for_gamma_spikes(vel_t[:, :3], vel_w[:, :3], 2e-4, vmax, frac=2e-3, spike=15.0, what="velocities, tiled against list walkers (Ferrari)")
    assert_close_but_for_gamma_spikes(vel_t[:, 3], vel_w[:, 3], 2e-6, 1.0, frac=0.002, spike=4.0, what="densities, tiled against list walkers (Ferrari)")
    assert np.abs(gg_t[fl, 3] - gg_w[fl, 3]).max() < 2e-5
    assert abs(dt_t - dt_w) < 1e-4*dt_w


def test_six_steps_of_the_k_epsilon_set(monkeypatch):
    eng = _engine(_problem(viscosity="KEPSVISC"), True, monkeypatch)
    _slosh(eng)
    for _ in range(6):
        eng.step()
    n = eng.n
    assert np.isfinite(_np(eng.pos)[:n]).all() and np.isfinite(_np(eng.vel)[:n]).all()
    assert all(np.isfinite(_np(t)[:n]).all() for t in eng.ke.values()) and 0 < eng.current_dt() < 1e-2


def test_six_steps_with_a_moving_wall(monkeypatch):
    """SAPaddleBox with the option: the flap's rows follow the prescribed motion bit for bit (against the oracle's sequence after
    the first step, which both take with the problem's initial dt: from the second on the diffusion changes the densities and so
    the time step the motion is integrated with), the walls at rest keep their rows, everything stays finite"""
    from sa_helpers import OracleSaSim
    mk = lambda: _problem(SAPaddleBox)
    sim, eng = OracleSaSim(mk()), _engine(mk(), True, monkeypatch)
    assert eng.sa_moving
    n = sim.n
    sim.step(); eng.step()
    info = _np(eng.info)[:n].view(np.uint16).reshape(-1, 4)
    assert np.array_equal(info, sim.info[:n])
    moving = (info[:, 0] & D.FG_MOVING_BOUNDARY) != 0
    t = info_type(info)
    seg = moving & (t == D.PT_BOUNDARY)
    rest = ~moving & (t != D.PT_FLUID)
    pos0 = sim.st["pos"][:n].copy()
    assert np.array_equal(_bits(_np(eng.pos)[:n][moving, :3]), _bits(sim.pos[:n][moving, :3]))
    assert np.array_equal(_bits(_np(eng.boundelements)[:n][seg]), _bits(sim.be[:n][seg]))
    rest_pos, rest_be = _np(eng.pos)[:n][rest].copy(), _np(eng.boundelements)[:n][rest & (t == D.PT_BOUNDARY)].copy()
    assert np.array_equal(_bits(rest_pos), _bits(pos0[rest]))
    for _ in range(5):
        eng.step()
    gp, gv, gb = _np(eng.pos)[:n], _np(eng.vel)[:n], _np(eng.boundelements)[:n]
    assert np.isfinite(gp).all() and np.isfinite(gv).all() and np.isfinite(_np(eng.gradgamma)[:n][t != D.PT_BOUNDARY]).all()
    assert np.array_equal(_bits(gp[rest]), _bits(rest_pos)) and np.array_equal(_bits(gb[rest & (t == D.PT_BOUNDARY)]), _bits(rest_be))
    assert gb[seg, 2].max() < -1e-3 and np.abs(np.linalg.norm(gb[seg, :3], axis=1) - 1.0).max() < 1e-5      # the flap did turn
    assert np.abs(gv[t == D.PT_FLUID, :3]).max() > 0


def test_diffusion_damps_density_noise_in_a_tank_at_rest(monkeypatch):
    """What the term is for: a hydrostatic tank with seeded density noise, 20 steps, with Ferrari and with DENSITY_DIFFUSION_NONE
    on the same build: the rms deviation of the fluid's density from the hydrostatic one ends lower with the diffusion."""
    import torch
    rms = {}
    for diffusion in (True, False):
        eng = _engine(_problem(diffusion=diffusion), True, monkeypatch)
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
    print("rms deviation from the hydrostatic density after 20 steps: Ferrari %.4g, no diffusion %.4g (seeded %.4g)"
          % (rms[True][0], rms[False][0], rms[True][1]))
    assert rms[True][0] < rms[False][0]
