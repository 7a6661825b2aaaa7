"""The GRANULAR rheology on the GPU (granular.hip, the GRANULAR branches of rheology.hip, the step driver) against the float64
all-pairs restatement tests/granular_ref.py and, for the forces, the CPU oracle: the four passes of the effective-pressure solver,
the fused solve against the loop over the passes, the viscosity, the forces with the central particle's viscosity, the re-sort
of BUFFER_EFFPRES and whole steps of the LithostaticColumn."""
import numpy as np
import pytest

from gpusph_amd import defs as D
from gpusph_amd.problem import LithostaticColumn, info_id, info_type
import oracle_lib as ol
from granular_ref import GranularRef

pytestmark = pytest.mark.gpu

TOL = 2e-5      # the project's bar for fp32 neighbour sums (tests/test_gpu_rheology.py)


def _engine(problem, **kw):
    import torch
    from gpusph_amd.engine import TimestepEngine
    assert torch.cuda.is_available()
    return TimestepEngine(problem, device="cuda:0", **kw)


def _np(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


class _Case:
    """the jittered column after its first list build, nine particles disabled behind the build (they are still in the lists)"""

    def __init__(self, disable=9, **kw):
        self.pr = LithostaticColumn(0.05, jitter=0.15, **kw)
        eng = self.eng = _engine(self.pr, clobber_neibslist=True)
        eng.build_neibs()
        n = self.n = eng.n
        if disable:
            pos = _np(eng.pos)
            pos[np.random.default_rng(99).choice(n, size=disable, replace=False), 3] = np.nan
            eng.pos.copy_(_dev(eng, pos))
        self.ref = GranularRef(self.pr, _np(eng.pos)[:n], _np(eng.hash, np.uint32)[:n], _np(eng.vel)[:n], _np(eng.info, np.uint16)[:n])
        self.state = (eng.pos, eng.vel, eng.info, eng.hash, eng.cellStart, eng.neibslist)
        self.maxiter = self.pr.simparams.jacobi_maxiter

    def loop(self, p):
        """preparation and the loop through the four entry points, the stop test on the host with the reference's two reads"""
        import torch
        K, n, sp, eng = self.eng.k, self.n, self.pr.simparams, self.eng
        jac = torch.zeros((eng.alloc, 4), dtype=torch.float32, device=eng.device)
        K.jacobi_fs_boundary_conditions(p, eng.pos, eng.info, n, n)
        K.jacobi_wall_boundary_conditions(p, *self.state, n, n)
        counter = 0
        while True:
            K.jacobi_build_vectors(jac, p, *self.state, n, n)
            res = K.jacobi_update_effpres(p, jac, eng.info, n, n)
            err = K.jacobi_wall_boundary_conditions(p, *self.state, n, n)
            if (err < np.float32(sp.jacobi_backerr) and res < np.float32(sp.jacobi_residual)) or counter > self.maxiter:
                return counter, err, res
            counter += 1

    def set_solver(self, maxiter=None):
        """jacobi_maxiter of the library's solve and of loop()"""
        sp = self.pr.simparams
        self.maxiter = sp.jacobi_maxiter if maxiter is None else maxiter
        self.eng.k.set_granular(self.pr.physparams.sinpsi, self.maxiter, sp.jacobi_backerr, sp.jacobi_residual)


@pytest.fixture(scope="module")
def case():
    return _Case()


def _fixed_point_check(ref, p, sp):
    """the field is a near-fixed-point of the float64 operator: one restated sweep moves it by no more than the stop thresholds
    times their reference pressures, plus the fp32 bar"""
    q, _, _ = ref.sweep(np.asarray(p, dtype=np.float64))
    rows = ref.interior | ref.is_wall
    moved = np.abs(q - p)[rows].max()
    bound = sp.jacobi_backerr * ref.refpres_wall + sp.jacobi_residual * ref.refpres_row.max() + TOL * np.abs(p).max()
    print("one restated sweep moves the field by %.4g Pa (bound %.4g, largest pressure %.1f)" % (moved, bound, np.abs(p).max()))
    assert moved <= bound
    assert np.array_equal(q[~rows], np.asarray(p, dtype=np.float64)[~rows])


def test_passes_against_the_restatement(case):
    import torch
    c, ref, n, eng, K = case, case.ref, case.n, case.eng, case.eng.k
    assert n % 64 and ref.interior.sum() % 64 and ref.is_wall.sum() % 64 and (~ref.active).sum() == 9
    rng = np.random.default_rng(5)
    p0 = rng.uniform(0.0, 4000.0, size=eng.alloc).astype(np.float32)
    # Dirichlet rows
    p = _dev(eng, p0)
    K.jacobi_fs_boundary_conditions(p, eng.pos, eng.info, n, n)
    got, want = _np(p)[:n], ref.fs_boundary_conditions(p0[:n])
    assert ref.dirichlet.sum() > 100 and np.abs(got - want).max() <= TOL * want.max()
    assert np.array_equal(_bits(got[~ref.dirichlet]), _bits(p0[:n][~ref.dirichlet]))
    # wall rows and their backward error
    p = _dev(eng, p0)
    err = K.jacobi_wall_boundary_conditions(p, *c.state, n, n)
    got = _np(p)[:n]
    want, want_err = ref.wall_boundary_conditions(p0[:n])
    print("wall pass: largest difference %.3g of %.1f, backward error %.6g vs %.6g" % (np.abs(got - want).max(), np.abs(want).max(), err, want_err))
    assert np.abs(got - want).max() <= TOL * np.abs(want).max()
    assert np.array_equal(_bits(got[~ref.is_wall]), _bits(p0[:n][~ref.is_wall]))
    assert want_err > 0 and abs(err - want_err) <= TOL * np.abs(want).max() / ref.refpres_wall
    # the vectors
    jac = torch.full((eng.alloc, 4), 7.0, dtype=torch.float32, device=eng.device)
    p = _dev(eng, p0)
    K.jacobi_build_vectors(jac, p, *c.state, n, n)
    j = _np(jac)[:n]
    Dv, Rx, B = ref.build_vectors(p0[:n])
    for name, got, w in (("D", j[:, 0], Dv), ("Rx", j[:, 1], Rx), ("B", j[:, 2], B)):
        print("%s: largest difference %.3g of %.4g" % (name, np.abs(got[ref.active] - w[ref.active]).max(), np.abs(w).max()))
        assert np.abs(got[ref.active] - w[ref.active]).max() <= TOL * np.abs(w).max()
    assert np.isnan(j[:, 3][ref.active]).all() and not j[~ref.active].any()
    assert not j[:, :3][ref.active & ~ref.interior].any() and (j[:, 0][ref.interior] != 0).all()
    assert np.array_equal(_bits(_np(p)), _bits(p0)) and (_np(jac)[n:] == 7.0).all()
    # the update and its residual
    res = K.jacobi_update_effpres(p, jac, eng.info, n, n)
    got = _np(p)[:n]
    want, _ = ref.update_effpres(p0[:n], Dv, Rx, B)
    assert np.abs(got - want).max() <= TOL * np.abs(want).max()
    assert np.array_equal(_bits(got[~ref.interior]), _bits(p0[:n][~ref.interior]))
    # the residual is what rounding leaves of D p + Rx - B: half an ulp of each of the three terms and of the quotient
    bound = (4 * 2.0 ** -24 * (np.abs(Rx) + np.abs(B)) / ref.refpres_row)[ref.interior].max()
    print("residual %.3g, rounding bound %.3g" % (res, bound))
    assert 0.0 <= res <= bound


def test_granular_viscosity(case):
    import torch
    c, ref, n, eng, K = case, case.ref, case.n, case.eng, case.eng.k
    pr = c.pr
    dp = pr.m_deltap
    X = pr.global_pos(_np(eng.pos)[:n], _np(eng.hash, np.uint32)[:n])
    rng = np.random.default_rng(17)
    vel0 = _np(eng.vel).copy()
    vel = vel0.copy()
    # a sheared, perturbed flow above z = 5.5 dp; everything below (floor included) at rest, so that the rows of the lowest
    # sediment layers see no relative velocity at all: S = 0 exactly, in fp32 as in float64
    moving = X[:, 2] > 5.5 * dp
    vel[:n, 0] = np.where(moving, 40.0 * (X[:, 2] - 5.5 * dp), 0.0)
    vel[:n, :3] += np.where(moving[:, None], rng.uniform(-0.3, 0.3, size=(n, 3)), 0.0).astype(np.float32)
    p = rng.uniform(50.0, 1000.0, size=eng.alloc).astype(np.float32)      # yield stresses on both sides of both bounds at S ~ 40 / s
    still = ref.sed_fluid & (X[:, 2] < 2.6 * dp)
    p[:n][still & (info_id(_np(eng.info, np.uint16)[:n]) % 2 == 0)] = 0.0      # S = 0 with p = 0 next to S = 0 with p > 0
    old = rng.uniform(1.0, 2.0, size=eng.alloc).astype(np.float32)
    try:
        eng.vel.copy_(_dev(eng, vel))
        ref2 = GranularRef(pr, _np(eng.pos)[:n], _np(eng.hash, np.uint32)[:n], vel[:n], _np(eng.info, np.uint16)[:n])
        S = ref2.shear_rate_norm()
        effvisc = _dev(eng, old)
        mx = K.calc_effvisc_granular(effvisc, _dev(eng, p), *c.state, n, n)
    finally:
        eng.vel.copy_(_dev(eng, vel0))
    got = _np(effvisc)
    want = ref2.effective_visc(p[:n], old[:n], S)
    rows = ref.is_fluid & ref.active
    np.testing.assert_allclose(got[:n][rows], want[rows], rtol=3e-5)
    # boundary slots, disabled particles and the rows beyond the range keep what they held
    assert np.array_equal(_bits(got[:n][~rows]), _bits(old[:n][~rows])) and np.array_equal(_bits(got[n:]), _bits(old[n:]))
    assert (~rows).sum() > 300
    pp = pr.physparams
    hi = np.float32(pp.limiting_kinvisc) * ref.rho0[ref.fluid_num] / ref.rho
    lo = np.array(pp.visccoeff)[ref.fluid_num] * ref.rho0[ref.fluid_num] / ref.rho
    zero = rows & still & (S == 0.0)
    assert (zero & (p[:n] > 0)).sum() > 20 and (zero & (p[:n] == 0)).sum() > 20
    np.testing.assert_allclose(got[:n][zero], hi[zero], rtol=3e-5)                 # inf and 0/0 both end at the upper bound
    inside = rows & ref.sed_fluid & (want > 1.01 * lo) & (want < 0.99 * hi)
    assert inside.sum() > 50 and (rows & ref.sed_fluid & (want >= 0.99 * hi)).sum() > 50 and (rows & ref.sed_fluid & (want <= 1.01 * lo)).sum() > 10
    # the pure fluid is Newtonian, clamped like the rest (the reference's lower bound is visccoeff rho0 with the DYNAMIC viscosity
    # in visccoeff, which lies above the viscosity itself)
    water = rows & ~ref.sed_fluid
    newtonian = np.array(pp.visccoeff)[0] / ref.rho
    np.testing.assert_allclose(got[:n][water], np.maximum(lo, np.minimum(newtonian, hi))[water], rtol=3e-5)
    assert mx == pytest.approx(want[rows].max(), rel=3e-5)


def test_forces_take_the_central_viscosity():
    """four values of the viscosity dealt out by particle id: row i of the GRANULAR forces is the oracle's row i for a UNIFORM
    field of i's value (the oracle reads the neighbour's viscosity, as the generalized Newtonian rheologies do)"""
    kw = dict(jitter=0.15)
    eng = _engine(LithostaticColumn(0.05, **kw), clobber_neibslist=True)
    eng.build_neibs()
    opr = LithostaticColumn(0.05, **kw)
    opr.simparams.rheologytype = opr.physparams.rheologytype = D.BINGHAM
    sim = ol.OracleSim(opr)
    sim.build_neibs()
    n = sim.n
    assert eng.n == n and np.array_equal(_np(eng.hash, np.uint32)[:n], sim.hash[:n])
    rng = np.random.default_rng(3)
    fluid = info_type(sim.info[:n]) == D.PT_FLUID
    sim.vel[:n, :3][fluid] += rng.uniform(-0.3, 0.3, size=(fluid.sum(), 3)).astype(np.float32)
    eng.vel[:n].copy_(_dev(eng, sim.vel[:n]))
    values = np.array([1e-3, 2e-3, 5e-3, 1e-2], dtype=np.float32)
    which = info_id(sim.info[:n]) % 4
    field = np.zeros(len(sim.pos), dtype=np.float32)
    field[:n] = values[which]
    eng.effvisc[:n].copy_(_dev(eng, field[:n]))
    K = eng.k
    K.memset(eng.forces, 0); K.memset(eng.cfl, 0)
    K.forces_effvisc(eng.forces, eng.cfl, eng.pos, eng.vel, eng.info, eng.hash, eng.cellStart, eng.neibslist, eng.effvisc, n, 0, n, 0)
    gf = _np(eng.forces)[:n]
    uniform = [sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, effvisc=np.full(len(sim.pos), v, dtype=np.float32))[0][:n]
               for v in values]
    want = np.stack(uniform)[which, np.arange(n)]
    scale = np.abs(want[:, :3]).max()
    print("forces: largest difference %.3g of %.4g" % (np.abs(gf[:, :3] - want[:, :3]).max(), scale))
    assert np.abs(gf[:, :3] - want[:, :3]).max() <= TOL * scale
    assert np.abs(gf[:, 3] - want[:, 3]).max() <= TOL * np.abs(want[:, 3]).max() + 1e-7
    # ... and not the per-neighbour result of the same field
    per_neib = sim.o.forces(sim.pos, sim.vel, sim.info, sim.hash, sim.cs, sim.nl, n, effvisc=field)[0][:n]
    assert np.abs(gf[:, :3] - per_neib[:, :3]).max() > 100 * TOL * scale


@pytest.mark.parametrize("which", ["converging", "cap", "no sediment"])
def test_fused_solve_gives_the_bits_of_the_loop(case, which):
    import torch
    c = case if which != "no sediment" else _Case(disable=0, sediment_layers=0, water_layers=5)
    eng, n = c.eng, c.n
    if which == "no sediment":
        assert not c.ref.interior.any() and not c.ref.sed_fluid.any()
    c.set_solver(maxiter=3 if which == "cap" else None)
    try:
        p0 = torch.zeros(eng.alloc, dtype=torch.float32, device=eng.device)
        p_loop = p0.clone()
        want = c.loop(p_loop)
        p_solve = p0.clone()
        got = eng.k.jacobi_solve(p_solve, *c.state, n, n)
    finally:
        c.set_solver()
    print(which, "counter %d backward error %g residual %g" % want)
    assert got == want
    assert np.array_equal(_bits(_np(p_solve)), _bits(_np(p_loop)))
    sp = c.pr.simparams
    if which == "cap":
        assert want[0] == 4
    elif which == "converging":
        assert 100 < want[0] < sp.jacobi_maxiter and want[1] < sp.jacobi_backerr and want[2] < sp.jacobi_residual
        _fixed_point_check(c.ref, _np(p_solve)[:n], sp)
    else:
        assert want == (0, 0.0, 0.0) and not _np(p_solve).any()


def test_build_neibs_carries_effpres_with_its_particle():
    eng = _engine(LithostaticColumn(0.05, jitter=0.15))
    n = len(eng.problem.parts.info)
    rng = np.random.default_rng(8)
    p = rng.uniform(0.0, 4000.0, size=n).astype(np.float32)
    eng.effpres[:n].copy_(_dev(eng, p))
    ids = info_id(_np(eng.info, np.uint16)[:n])
    before = np.empty(n, dtype=np.uint32); before[ids] = _bits(p)
    eng.build_neibs()
    assert eng.n == n
    ids2 = info_id(_np(eng.info, np.uint16)[:n])
    assert not np.array_equal(ids, ids2)                        # the build did re-sort
    after = np.empty(n, dtype=np.uint32); after[ids2] = _bits(_np(eng.effpres)[:n])
    assert np.array_equal(before, after)


def test_steps_of_the_tilted_column():
    """twelve steps (a rebuild at the eleventh) with gravity tilted by 0.1 rad, below the friction angle of 30 degrees"""
    pr = LithostaticColumn(0.05, jitter=0.05, tilt=0.1)
    eng = _engine(pr)
    for _ in range(12):
        eng.step()
    sp = pr.simparams
    assert set(eng.jacobi_iterations) == {"init", "predictor", "corrector"}
    print("counters of the last solves", eng.jacobi_iterations, "largest", eng.jacobi_max_iterations)
    assert eng.jacobi_max_iterations < sp.jacobi_maxiter
    for err, res in eng.jacobi_last.values():
        assert err < sp.jacobi_backerr and res < sp.jacobi_residual
    out = eng.download()
    n = eng.n
    assert n == pr.num_particles and np.isfinite(out["pos"]).all() and np.isfinite(out["vel"]).all()
    ref = GranularRef(pr, out["pos"], out["hash"], out["vel"], out["info"])
    _fixed_point_check(ref, out["effpres"], sp)
    assert out["effpres"][ref.interior].min() > 0


def _params(**change):
    pr = LithostaticColumn(0.05)
    for k, v in change.items():
        setattr(pr.simparams, k, v)
    return pr.sphx_params(pr.num_particles)


@pytest.mark.parametrize("change", [dict(boundarytype=D.SA_BOUNDARY, neibboundpos=125), dict(boundarytype=D.LJ_BOUNDARY), dict(sph_formulation=D.SPH_F1),
                                    dict(simflags=D.ENABLE_DTADAPT), dict(simflags=D.ENABLE_DTADAPT | D.ENABLE_MULTIFLUID | D.ENABLE_XSPH),
                                    dict(simflags=D.ENABLE_DTADAPT | D.ENABLE_MULTIFLUID | D.ENABLE_MOVING_BODIES)],
                         ids=["SA", "LJ", "SPH_F1", "single fluid", "XSPH", "moving bodies"])
def test_set_constants_refuses_the_unbuilt_combinations(change):
    from gpusph_amd import capi
    ctx = capi.Context(0)
    try:
        ctx.set_constants(_params())                      # the built set
        with pytest.raises(capi.SphxUnsupported):
            ctx.set_constants(_params(**change))
    finally:
        ctx.close()
