"""What the SA_BOUNDARY entry points of sa_bounds.hip that choose between the tiled window, the one-element-per-lane wall kernels and
the list walker REFUSE, and in which words: a table of (entry point, option set, what is wrong with the call) -> (return code,
message), through the host-emulated library (tests/hostemu).  The table was recorded before these entry points were folded onto
shared implementations and holds unchanged after: a caller that matches on a message, or an option-set check that moved behind
another one, shows here.  Every call is made over an empty range (no kernel runs): a call that is not refused returns SPHX_OK."""
import numpy as np
import pytest

from gpusph_amd import capi
from gpusph_amd import defs as D
from gpusph_amd.params import SphxParams
from gpusph_amd.problem import SABox

OK, INVALID, UNSUPPORTED = capi.SPHX_OK, capi.SPHX_ERR_INVALID, capi.SPHX_ERR_UNSUPPORTED

# the arguments of each entry point behind the context, in the order of include/sphx.h
_DSUM_TAIL = ["vertPos0", "vertPos1", "vertPos2", "info", "hash", "cellStart", "neibsList", "numParticles", "particleRangeEnd"]
ARGS = {
    "sphx_sa_density_sum": ["newVel", "newGGam", "forces", "oldPos", "newPos", "oldVel", "oldGGam", "boundElements"] + _DSUM_TAIL +
                           ["dt", "step", "t", "epsilon", "deltap", "slength", "influenceradius", "stream"],
    "sphx_sa_density_sum_moving": ["newVel", "newGGam", "forces", "oldPos", "newPos", "oldVel", "oldGGam", "oldBoundElements",
                                   "newBoundElements"] + _DSUM_TAIL + ["stream"],
    "sphx_sa_density_sum_io": ["newVel", "newGGam", "forces", "oldPos", "newPos", "oldVel", "oldEulerVel", "oldGGam",
                               "boundElements"] + _DSUM_TAIL + ["dt", "stream"],
    "sphx_sa_density_sum_io_moving": ["newVel", "newGGam", "forces", "oldPos", "newPos", "oldVel", "oldEulerVel", "oldGGam",
                                      "oldBoundElements", "newBoundElements"] + _DSUM_TAIL + ["dt", "stream"],
    "sphx_sa_compute_density_diffusion": ["forces", "pos", "vel", "gGam", "info", "hash", "cellStart", "neibsList", "numParticles",
                                          "particleRangeEnd", "deltap", "slength", "influenceradius", "dt", "stream"],
    "sphx_sa_compute_density_diffusion_io": ["forces", "pos", "vel", "gGam", "boundElements", "vertPos0", "vertPos1", "vertPos2", "info",
                                             "hash", "cellStart", "neibsList", "numParticles", "particleRangeEnd", "deltap", "dt",
                                             "stream"],
    "sphx_forces_basicstep_sa": ["forces", "cfl", "cflGamma", "pos", "vel", "info", "hash", "cellStart", "neibsList", "gGam",
                                 "boundElements", "vertPos0", "vertPos1", "vertPos2", "numParticles", "fromParticle", "toParticle",
                                 "deltap", "slength", "dtadaptfactor", "influenceradius", "cflOffset", "run_mode", "step", "dt",
                                 "h_numBlocks", "stream"],
    "sphx_forces_basicstep_sa_io": ["forces", "cfl", "cflGamma", "pos", "vel", "eulerVel", "info", "hash", "cellStart", "neibsList",
                                    "gGam", "boundElements", "vertPos0", "vertPos1", "vertPos2", "numParticles", "fromParticle",
                                    "toParticle", "deltap", "cflOffset", "h_numBlocks", "stream"],
    "sphx_sa_integrate_gamma": ["newGGam", "oldGGam", "newPos", "boundElements", "vertPos0", "vertPos1", "vertPos2", "info", "hash",
                                "cellStart", "neibsList", "numParticles", "particleRangeEnd", "dt", "step", "t", "epsilon", "slength",
                                "influenceradius", "run_mode", "stream"],
}
ENTRIES = list(ARGS)
DSUMS = ENTRIES[:4]
_SCALARS = {"numParticles", "particleRangeEnd", "fromParticle", "toParticle", "cflOffset", "dt", "step", "t", "epsilon", "deltap",
            "slength", "influenceradius", "dtadaptfactor", "run_mode", "stream"}


def _option_sets():
    """the uploaded constants of the option sets the entry points tell apart (the flags are what they look at, so one tank's
    constants with other flags stand for the problems that have them)"""
    prob = SABox(0.1)
    base = prob.sphx_params(prob.num_particles)
    def variant(**kw):
        p = SphxParams.from_buffer_copy(bytes(base))
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    f = int(base.simflags)
    quad = (f & ~D.ENABLE_DENSITY_SUM) | D.ENABLE_GAMMA_QUADRATURE
    return {
        "solid": variant(),                                                                         # StillWaterSA
        "moving": variant(simflags=f | D.ENABLE_MOVING_BODIES),                                     # SAPaddleBox
        "io": variant(simflags=f | D.ENABLE_INLET_OUTLET),                                          # SAChannelIO
        "io_moving": variant(simflags=f | D.ENABLE_INLET_OUTLET | D.ENABLE_MOVING_BODIES),          # SAChannelIOFlap
        "quadrature": variant(simflags=quad, densitydiffusiontype=D.DENSITY_DIFFUSION_NONE),        # StillWaterRepackSA
        "keps": variant(turbmodel=D.KEPSILON, is_const_visc=0),
        "solid_no_brezzi": variant(densitydiffusiontype=D.DENSITY_DIFFUSION_NONE),
        "io_no_brezzi": variant(simflags=f | D.ENABLE_INLET_OUTLET, densitydiffusiontype=D.DENSITY_DIFFUSION_NONE),
        "dyn_boundary": variant(boundarytype=D.DYN_BOUNDARY, densitydiffusiontype=D.DENSITY_DIFFUSION_NONE),
    }


@pytest.fixture(scope="module")
def emus():
    from hostemu_lib import Emu
    made = {name: Emu(p) for name, p in _option_sets().items()}
    yield made
    for e in made.values():
        e.close()


def _call(emu, entry, **change):
    """the entry point over an empty range with every buffer present and distinct, but for `change`: name=None (a missing buffer),
    name="other name" (the same buffer twice) or name=value (a scalar)"""
    bufs = {n: np.zeros(16, dtype=np.float32) for n in ARGS[entry] if n not in _SCALARS}
    vals = {"slength": float(emu.params.slength), "influenceradius": float(emu.params.influenceradius), "run_mode": D.SIMULATE,
            "stream": None}
    conv = []
    for n in ARGS[entry]:
        v = change.get(n, bufs.get(n, vals.get(n, 0)))
        if isinstance(v, str):
            v = bufs[v]
        conv.append(v.ctypes.data if isinstance(v, np.ndarray) else v)
    assert len(conv) + 1 == len(capi.SIGNATURES[entry][1])
    rc = getattr(emu.lib, entry)(emu.h, *conv)
    return rc, ("" if rc == OK else emu.lib.sphx_last_error().decode())


# (entry point, option set, what is changed in the call) -> (return code, message)
TABLE = [
    ('sphx_sa_density_sum', 'solid', {}, (OK, '')),
    ('sphx_sa_density_sum', 'moving', {}, (INVALID, 'sphx_sa_density_sum: with ENABLE_MOVING_BODIES the boundary elements are double buffered: call sphx_sa_density_sum_moving')),
    ('sphx_sa_density_sum', 'io', {}, (OK, '')),
    ('sphx_sa_density_sum', 'io_moving', {}, (INVALID, 'sphx_sa_density_sum: with ENABLE_MOVING_BODIES the boundary elements are double buffered: call sphx_sa_density_sum_moving')),
    ('sphx_sa_density_sum', 'quadrature', {}, (INVALID, 'sphx_sa_density_sum: needs ENABLE_DENSITY_SUM with dynamic gamma')),
    ('sphx_sa_density_sum_moving', 'solid', {}, (INVALID, 'sphx_sa_density_sum_moving: the uploaded option set has no ENABLE_MOVING_BODIES (call sphx_sa_density_sum)')),
    ('sphx_sa_density_sum_moving', 'moving', {}, (OK, '')),
    ('sphx_sa_density_sum_moving', 'io', {}, (INVALID, 'sphx_sa_density_sum_moving: the uploaded option set has no ENABLE_MOVING_BODIES (call sphx_sa_density_sum)')),
    ('sphx_sa_density_sum_moving', 'io_moving', {}, (INVALID, 'sphx_sa_density_sum_moving: with ENABLE_INLET_OUTLET as well the pass reads the Eulerian velocities: call sphx_sa_density_sum_io_moving')),
    ('sphx_sa_density_sum_moving', 'quadrature', {}, (INVALID, 'sphx_sa_density_sum_moving: needs ENABLE_DENSITY_SUM with dynamic gamma')),
    ('sphx_sa_density_sum_io', 'solid', {}, (OK, '')),
    ('sphx_sa_density_sum_io', 'moving', {}, (OK, '')),
    ('sphx_sa_density_sum_io', 'io', {}, (OK, '')),
    ('sphx_sa_density_sum_io', 'io_moving', {}, (OK, '')),
    ('sphx_sa_density_sum_io', 'quadrature', {}, (OK, '')),
    ('sphx_sa_density_sum_io_moving', 'solid', {}, (INVALID, 'sphx_sa_density_sum_io_moving: the uploaded option set has not both ENABLE_INLET_OUTLET and ENABLE_MOVING_BODIES')),
    ('sphx_sa_density_sum_io_moving', 'moving', {}, (INVALID, 'sphx_sa_density_sum_io_moving: the uploaded option set has not both ENABLE_INLET_OUTLET and ENABLE_MOVING_BODIES')),
    ('sphx_sa_density_sum_io_moving', 'io', {}, (INVALID, 'sphx_sa_density_sum_io_moving: the uploaded option set has not both ENABLE_INLET_OUTLET and ENABLE_MOVING_BODIES')),
    ('sphx_sa_density_sum_io_moving', 'io_moving', {}, (OK, '')),
    ('sphx_sa_density_sum_io_moving', 'quadrature', {}, (INVALID, 'sphx_sa_density_sum_io_moving: the uploaded option set has not both ENABLE_INLET_OUTLET and ENABLE_MOVING_BODIES')),
    ('sphx_sa_density_sum', 'dyn_boundary', {}, (INVALID, 'density_sum called without SA_BOUNDARY')),
    ('sphx_sa_density_sum_moving', 'dyn_boundary', {}, (INVALID, 'density_sum called without SA_BOUNDARY')),
    ('sphx_sa_density_sum_io', 'dyn_boundary', {}, (INVALID, 'density_sum called without SA_BOUNDARY')),
    ('sphx_sa_density_sum_io_moving', 'dyn_boundary', {}, (INVALID, 'density_sum called without SA_BOUNDARY')),
    ('sphx_sa_compute_density_diffusion', 'dyn_boundary', {}, (INVALID, 'compute_density_diffusion called without SA_BOUNDARY')),
    ('sphx_sa_compute_density_diffusion_io', 'dyn_boundary', {}, (INVALID, 'compute_density_diffusion called without SA_BOUNDARY')),
    ('sphx_forces_basicstep_sa', 'dyn_boundary', {}, (INVALID, 'forces basicstep (SA) called without SA_BOUNDARY')),
    ('sphx_forces_basicstep_sa_io', 'dyn_boundary', {}, (INVALID, 'forces called without SA_BOUNDARY')),
    ('sphx_sa_integrate_gamma', 'dyn_boundary', {}, (INVALID, 'integrate_gamma called without SA_BOUNDARY')),
    ('sphx_forces_basicstep_sa', 'keps', {}, (INVALID, 'sphx_forces_basicstep_sa: the KEPSILON forces read k, epsilon, the eddy viscosity and the Eulerian velocity: call sphx_forces_basicstep_sa_keps')),
    ('sphx_forces_basicstep_sa', 'solid', {'run_mode': D.REPACK}, (UNSUPPORTED, 'sphx_forces_basicstep_sa: repacking with dynamic gamma (its CFL condition) is not built; ENABLE_GAMMA_QUADRATURE is')),
    ('sphx_forces_basicstep_sa', 'quadrature', {'run_mode': D.REPACK}, (OK, '')),
    ('sphx_forces_basicstep_sa', 'solid', {'run_mode': 7}, (INVALID, 'sphx_forces_basicstep_sa: invalid run mode')),
    ('sphx_forces_basicstep_sa', 'solid', {'fromParticle': 2, 'toParticle': 1}, (INVALID, 'sphx_forces_basicstep_sa: empty range')),
    ('sphx_forces_basicstep_sa', 'solid', {'cfl': None}, (INVALID, 'sphx_forces_basicstep_sa: ENABLE_DTADAPT needs the CFL buffer')),
    ('sphx_forces_basicstep_sa', 'solid', {'slength': 1.0}, (INVALID, 'sphx_forces_basicstep_sa: slength / influenceradius differ from the uploaded constants')),
    ('sphx_forces_basicstep_sa_io', 'io', {}, (OK, '')),
    ('sphx_forces_basicstep_sa_io', 'keps', {}, (UNSUPPORTED, 'sphx_sa_io: open boundaries with k-epsilon are not built')),
    ('sphx_forces_basicstep_sa_io', 'io', {'fromParticle': 2, 'toParticle': 1}, (INVALID, 'sphx_forces_basicstep_sa_io: invalid particle range')),
    ('sphx_forces_basicstep_sa_io', 'io', {'toParticle': 1}, (INVALID, 'sphx_forces_basicstep_sa_io: invalid particle range')),
    ('sphx_sa_compute_density_diffusion', 'solid', {}, (OK, '')),
    ('sphx_sa_compute_density_diffusion', 'solid_no_brezzi', {}, (UNSUPPORTED, 'sphx_sa_compute_density_diffusion: built for Brezzi diffusion with density summation')),
    ('sphx_sa_compute_density_diffusion', 'quadrature', {}, (UNSUPPORTED, 'sphx_sa_compute_density_diffusion: built for Brezzi diffusion with density summation')),
    ('sphx_sa_compute_density_diffusion', 'solid', {'influenceradius': 1.0}, (INVALID, 'sphx_sa_compute_density_diffusion: slength / influenceradius differ from the uploaded constants')),
    ('sphx_sa_compute_density_diffusion_io', 'io', {}, (OK, '')),
    ('sphx_sa_compute_density_diffusion_io', 'io_no_brezzi', {}, (UNSUPPORTED, 'sphx_sa_compute_density_diffusion_io: built for Brezzi diffusion with density summation')),
    ('sphx_sa_compute_density_diffusion_io', 'keps', {}, (UNSUPPORTED, 'sphx_sa_io: open boundaries with k-epsilon are not built')),
    ('sphx_sa_integrate_gamma', 'quadrature', {}, (OK, '')),
    ('sphx_sa_integrate_gamma', 'solid', {}, (UNSUPPORTED, 'sphx_sa_integrate_gamma: dynamic gamma (transport equation) is not built; ENABLE_GAMMA_QUADRATURE is')),
    ('sphx_sa_integrate_gamma', 'quadrature', {'newGGam': 'oldGGam'}, (INVALID, 'sphx_sa_integrate_gamma: in-place use is not supported')),
    ('sphx_sa_integrate_gamma', 'quadrature', {'slength': 1.0}, (INVALID, 'sphx_sa_integrate_gamma: slength / influenceradius differ from the uploaded constants')),
    ('sphx_sa_density_sum', 'solid', {'newGGam': 'oldGGam'}, (INVALID, 'sphx_sa_density_sum: gamma is double buffered')),
    ('sphx_sa_density_sum', 'solid', {'slength': 1.0}, (INVALID, 'sphx_sa_density_sum: slength / influenceradius differ from the uploaded constants')),
    ('sphx_sa_density_sum_moving', 'moving', {'newGGam': 'oldGGam'}, (INVALID, 'sphx_sa_density_sum_moving: gamma and the boundary elements are double buffered')),
    ('sphx_sa_density_sum_moving', 'moving', {'newBoundElements': 'oldBoundElements'}, (INVALID, 'sphx_sa_density_sum_moving: gamma and the boundary elements are double buffered')),
    ('sphx_sa_density_sum_io', 'io', {'newGGam': 'oldGGam'}, (OK, '')),
    ('sphx_sa_density_sum_io', 'keps', {}, (UNSUPPORTED, 'sphx_sa_io: open boundaries with k-epsilon are not built')),
    ('sphx_sa_density_sum_io_moving', 'io_moving', {'newGGam': 'oldGGam'}, (INVALID, 'sphx_sa_density_sum_io_moving: gamma and the boundary elements are double buffered')),
    ('sphx_sa_density_sum_io_moving', 'io_moving', {'newBoundElements': 'oldBoundElements'}, (INVALID, 'sphx_sa_density_sum_io_moving: gamma and the boundary elements are double buffered')),
    ('sphx_sa_density_sum', 'solid', {'neibsList': None}, (INVALID, 'sphx_sa_density_sum: missing buffer')),
    ('sphx_sa_density_sum_moving', 'moving', {'neibsList': None}, (INVALID, 'sphx_sa_density_sum_moving: missing buffer')),
    ('sphx_sa_density_sum_io', 'io', {'neibsList': None}, (INVALID, 'sphx_sa_density_sum_io: missing buffer')),
    ('sphx_sa_density_sum_io_moving', 'io_moving', {'neibsList': None}, (INVALID, 'sphx_sa_density_sum_io_moving: missing buffer')),
    ('sphx_sa_compute_density_diffusion', 'solid', {'neibsList': None}, (INVALID, 'sphx_sa_compute_density_diffusion: missing buffer')),
    ('sphx_sa_compute_density_diffusion_io', 'io', {'neibsList': None}, (INVALID, 'sphx_sa_compute_density_diffusion_io: missing buffer')),
    ('sphx_forces_basicstep_sa', 'solid', {'neibsList': None}, (INVALID, 'sphx_forces_basicstep_sa: missing buffer')),
    ('sphx_forces_basicstep_sa_io', 'io', {'neibsList': None}, (INVALID, 'sphx_forces_basicstep_sa_io: missing buffer')),
    ('sphx_sa_integrate_gamma', 'quadrature', {'neibsList': None}, (INVALID, 'sphx_sa_integrate_gamma: missing buffer')),
    ('sphx_sa_density_sum_io', 'io', {'oldEulerVel': None}, (INVALID, 'sphx_sa_density_sum_io: missing buffer')),
    ('sphx_sa_density_sum_moving', 'moving', {'newBoundElements': None}, (INVALID, 'sphx_sa_density_sum_moving: missing buffer')),
    ('sphx_forces_basicstep_sa_io', 'io', {'eulerVel': None}, (INVALID, 'sphx_forces_basicstep_sa_io: missing buffer')),
    ('sphx_sa_compute_density_diffusion_io', 'io', {'vertPos2': None}, (INVALID, 'sphx_sa_compute_density_diffusion_io: missing buffer')),
]


@pytest.mark.parametrize("entry,options,change,want", TABLE, ids=["%s-%s-%s" % (e, o, "-".join("%s=%s" % kv for kv in c.items()) or "plain") for e, o, c, _ in TABLE])
def test_refusal(emus, entry, options, change, want):
    assert _call(emus[options], entry, **change) == want


def test_the_table_covers_what_it_says():
    have = {(e, o) for e, o, c, _ in TABLE if not c}
    four = ("solid", "moving", "io", "io_moving")
    assert all((e, o) in have for e in DSUMS for o in four)                       # every density summation under every option set
    assert all((e, "dyn_boundary") in have for e in ENTRIES)                      # no entry point without SA_BOUNDARY
    assert all(any(e == e2 and None in c.values() for e2, _, c, _ in TABLE) for e in ENTRIES)      # a missing buffer, each
    assert all(want[0] != OK or not want[1] for *_, want in TABLE)
