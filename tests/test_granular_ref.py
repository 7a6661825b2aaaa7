"""CPU-side checks of the GRANULAR rheology: the float64 restatement the GPU tests are held to (tests/granular_ref.py) against
its own known answer, the LithostaticColumn set-up, and the new entry points in the cross-compiled library and its binding."""
import numpy as np

from gpusph_amd import capi, defs as D
from gpusph_amd.problem import LithostaticColumn, info_type
from granular_ref import GranularRef

NEW_SYMBOLS = ("sphx_set_granular", "sphx_jacobi_fs_boundary_conditions", "sphx_jacobi_wall_boundary_conditions",
               "sphx_jacobi_build_vectors", "sphx_jacobi_update_effpres", "sphx_jacobi_solve", "sphx_calc_effvisc_granular")


def test_library_exports_the_granular_entry_points():
    lib = capi.load()
    for name in NEW_SYMBOLS:
        assert name in capi.SIGNATURES, "python binding lacks %s" % name
        assert hasattr(lib, name), "libsphx.so does not export %s" % name


def test_column_layout():
    pr = LithostaticColumn(0.05, jitter=0.1)
    info = pr.parts.info
    flags = info[:, 0]
    ptype = info_type(info)
    sed = (flags & D.FG_SEDIMENT) != 0
    interface = (flags & D.FG_INTERFACE) != 0
    n = pr.num_particles
    interior = (ptype == D.PT_FLUID) & sed & ~interface
    # the counts the GPU tests rely on: none of them a multiple of the wave size
    assert (n, int(interior.sum()), int((ptype == D.PT_BOUNDARY).sum())) == (1458, 486, 324)
    assert all(c % 64 for c in (n, int(interior.sum()), int((ptype == D.PT_BOUNDARY).sum())))
    assert sed.sum() == 8 * 81 and (sed & interface).sum() == 2 * 81 and not (interface & ~sed).any()
    assert np.array_equal((info[:, 1] >> 12)[sed], np.ones(sed.sum(), dtype=np.uint16)) and not (info[:, 1] >> 12)[~sed].any()
    arrs = pr.copy_to_array()
    g = 9.81
    z0 = LithostaticColumn(0.05).parts.pos_global[:, 2]      # the lattice heights
    want = np.where(sed, pr.delta_rho * g * (pr.m_deltap + pr.zi - z0), 0.0)
    np.testing.assert_allclose(arrs["effpres"], want, rtol=1e-6)
    sp = pr.sphx_params(n)
    assert (sp.rheologytype, sp.sph_formulation, sp.boundarytype, sp.avgop, sp.compvisc) == \
        (D.GRANULAR, D.SPH_HA, D.DYN_BOUNDARY, D.HARMONIC, D.KINEMATIC) and sp.simflags & D.ENABLE_MULTIFLUID
    tilted = LithostaticColumn(0.05, tilt=0.2)
    assert np.allclose(tilted.physparams.gravity, (9.81 * np.sin(0.2), 0.0, -9.81 * np.cos(0.2)))


def test_restatement_finds_the_lithostatic_profile():
    """Unjittered column from a zero field (Lithostatic.inc's default): below the two layers that hold the Dirichlet value
    delta_rho g dp the converged field is the lithostatic line delta_rho g (dp + z_top - z), z_top the lower of those layers.
    The discrete operator is not exact next to them (the rows there miss the water's share of their kernel support and see the
    upper Dirichlet layer, which is off the line).  Measured in float64: 326 iterations, largest deviation 9.995 Pa of 3063 Pa,
    in the row below the Dirichlet layers; held here with a margin of two."""
    pr = LithostaticColumn(0.05, lithostatic_init=False)
    arrs = pr.copy_to_array()
    ref = GranularRef(pr, arrs["pos"], arrs["hash"], arrs["vel"], arrs["info"])
    p, iterations, err, res = ref.solve(arrs["effpres"])
    assert 0 < iterations < pr.simparams.jacobi_maxiter
    assert err < pr.simparams.jacobi_backerr and res < pr.simparams.jacobi_residual
    z = pr.parts.pos_global[:, 2]
    g = float(np.linalg.norm(pr.physparams.gravity))
    line = pr.delta_rho * g * (pr.m_deltap + pr.z_dirichlet - z)
    dev = np.abs(p[ref.interior] - line[ref.interior]).max()
    print("iterations %d, deviation from the lithostatic line %.4f Pa of %.1f" % (iterations, dev, line[ref.interior].max()))
    assert dev <= 2 * 9.995
    assert dev > 0.5      # ... and it is the discrete answer, not the line copied
    # (the restatement takes g and dp as the float32 values the device gets: 6e-8 each)
    np.testing.assert_allclose(p[ref.dirichlet], pr.delta_rho * g * pr.m_deltap, rtol=1e-6)
    # uniform in every layer: the column has no side walls
    for k in range(1, 9):
        layer = np.isclose(z, k * pr.m_deltap) & ref.sed_fluid
        assert np.ptp(p[layer]) <= 1e-9 * p[layer].max()
    # one more sweep moves nothing beyond the thresholds
    q, err2, _ = ref.sweep(p)
    assert err2 < pr.simparams.jacobi_backerr
    assert np.abs(q - p)[ref.interior].max() <= 1e-3 * line[ref.interior].max()


def test_restatement_counter_semantics():
    """JACOBI_STOP_CRITERION (src/GPUSPH.cc:2300-2321): the counter is raised after a failed test and the cap is `counter >
    maxiter`, so a solve that never converges runs maxiter + 2 sweeps and leaves the counter at maxiter + 1"""
    pr = LithostaticColumn(0.05, lithostatic_init=False, columns=(7, 7), sediment_layers=5, water_layers=2)
    arrs = pr.copy_to_array()
    ref = GranularRef(pr, arrs["pos"], arrs["hash"], arrs["vel"], arrs["info"])
    sweeps = []
    orig = ref.sweep
    ref.sweep = lambda p: (sweeps.append(1), orig(p))[1]
    _, counter, _, _ = ref.solve(arrs["effpres"], maxiter=3)
    assert counter == 4 and len(sweeps) == 5
    # nothing to solve: one sweep, both maxima zero, counter 0
    water = LithostaticColumn(0.05, columns=(7, 7), sediment_layers=0, water_layers=5)
    a = water.copy_to_array()
    r0 = GranularRef(water, a["pos"], a["hash"], a["vel"], a["info"])
    p, counter, err, res = r0.solve(a["effpres"])
    assert (counter, err, res) == (0, 0.0, 0.0) and not p.any()
