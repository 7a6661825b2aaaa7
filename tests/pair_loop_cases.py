"""The runs that tests/test_gpu_pair_loop_bits.py compares and tests/golden/make_pair_loop_golden.py records: the plain tiled forces
pass (Wendland kernel, artificial viscosity, one fluid, Colagrossi diffusion: pair_interact_pk in csrc/forces_tile.h) of a small dam
break under four gravities.  TEST INFRASTRUCTURE; needs a device.

The pass has two instantiations: one for a gravity along z, whose g.r is the one product g_z r_z, and one for any gravity.  The host
chooses at every launch; sphx_dbg_forces_general_gravity keeps a context on the second."""
import hashlib

import numpy as np

from gpusph_amd.problem import DamBreak3D

GRAVITIES = {
    "down": (0.0, 0.0, -9.81),
    "up": (0.0, 0.0, 9.81),
    "along-y": (0.0, -9.81, 0.0),
    "oblique": (3.0, -2.0, -9.0),
}
ALONG_Z = ("down", "up")
STEPS = 12          # a rebuild at step 10
SEED = 11
EVERY = 16          # rows kept in the fixture for diagnosis
ARRAYS = ("forces", "pos", "vel")


def problem(case):
    prob = DamBreak3D(0.03, obstacle=True, hydrostatic=False)
    prob.physparams.gravity = tuple(float(g) for g in GRAVITIES[case])
    return prob


def gravity_path(eng, force_general=None):
    """-> 1: a tiled plain pass of this context takes the instantiation for a gravity along z, 0: the one for any gravity.
    force_general True / False: first keep the context on the general one / let the host choose again"""
    on = -1 if force_general is None else int(bool(force_general))
    return int(eng.k.lib.sphx_dbg_forces_general_gravity(eng.k.ctx.handle, on))


def run(case, force_general=False, path=True):
    """one forces pass on the perturbed initial state, then STEPS steps -> dict: forces1 / pos1 / vel1 / dt1 after the pass,
    forces12 / pos12 / vel12 / dt12 after the steps, path (see gravity_path; None when path is False: a library without the entry)"""
    import torch
    from gpusph_amd.engine import TimestepEngine
    from forces_check import tiles_usable
    from test_gpu_tiling_overflow import _perturb
    eng = TimestepEngine(problem(case), device="cuda:0", clobber_neibslist=True)
    out = {"path": None}
    if path:
        out["path"] = gravity_path(eng, force_general)
    eng.build_neibs()
    assert eng.neibs_info().hasTooManyNeibs == -1
    assert tiles_usable(eng) == 1
    _perturb(eng, SEED)
    eng._forces(eng.pos, eng.vel, 1, 0)
    n = eng.n
    for k in ARRAYS:
        out[k + "1"] = getattr(eng, k)[:n].cpu().numpy().copy()
    out["dt1"] = float(eng.d_dt_next.item())
    for _ in range(STEPS):
        eng.step()
    torch.cuda.synchronize()
    assert tiles_usable(eng) == 1 and eng.n == n
    for k in ARRAYS:
        out[k + "12"] = getattr(eng, k)[:n].cpu().numpy().copy()
    out["dt12"] = float(eng.d_dt_next.item())
    return out


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def record(case, res):
    """what the fixture holds of one run: key -> array"""
    rec = {}
    for stage in ("1", "12"):
        for k in ARRAYS:
            a = res[k + stage]
            rec["%s/sha256_%s%s" % (case, k, stage)] = digest(a)
            rec["%s/rows_%s%s" % (case, k, stage)] = a[::EVERY].copy()
        rec["%s/dt%s" % (case, stage)] = np.float64(res["dt" + stage])
    rec["%s/n" % case] = np.int64(len(res["forces1"]))
    return rec
