"""The rule of the save-time diagnostics (gpusph_amd/csrc/diagnostics.hip, include/sphx.h sphx_save_diagnostics) in numpy, for
tests/test_diagnostics_hostemu.py (the kernels' source on the CPU) and tests/test_gpu_save_diagnostics.py (the device).  TEST
INFRASTRUCTURE.

Per active row (finite pos.w), with the global position gp of sa_postprocess_cases.global_pos_f64 and m = (double)pos.w:
    kinetic   = m (double)((vx vx + vy vy + vz vz)/2)      the bracket in float32, left to right
    potential = -m (gp.x gx + gp.y gy + gp.z gz)           in float64, left to right, g the float32 gravity widened
    internal  = m (double)e_int                            0 without an energy buffer
into the class fluid_num (fluid particles) or MAX_FLUID_TYPES (everybody else), summed with math.fsum: the correctly rounded sum.

The terms are bit-identical to the kernel's (no FMA contraction on either side), so only the order of the sum differs.  Any order of
summing n terms is within (n - 1) 2^-53 sum|term| of the exact sum to first order; the tests allow (n + 8) 2^-52 sum|term|, n the
number of rows of the class: derived, not measured.  The row counts, the largest speed and the first row without a finite position
are held exactly."""
import math

import numpy as np

from gpusph_amd import defs as D
from gpusph_amd.problem import info_type
from sa_postprocess_cases import global_pos_f64

CLASSES = D.MAX_FLUID_TYPES + 1
MAXSQ = 4*CLASSES               # the layout of sphx_save_diagnostics' result (include/sphx.h)
NANROW = MAXSQ + 1
DOUBLES = MAXSQ + 4
NO_ROW = 4294967296.0


def rule(problem, pos, vel, info, hash_, energy=None):
    """-> dict(energy [CLASSES, 3] float64, abs [CLASSES, 3] the sums of |term|, rows [CLASSES] int, max_speed float32, nan_row int or None)"""
    pos, vel = np.asarray(pos, dtype=np.float32), np.asarray(vel, dtype=np.float32)
    info = np.asarray(info).view(np.uint16).reshape(-1, 4)
    n = len(pos)
    out = dict(energy=np.zeros((CLASSES, 3)), abs=np.zeros((CLASSES, 3)), rows=np.zeros(CLASSES, dtype=np.int64),
               max_speed=np.float32(0.0), nan_row=None)
    if not n:
        return out
    with np.errstate(all="ignore"):
        gp = global_pos_f64(problem, pos, hash_)
        active = np.isfinite(pos[:, 3])
        m = pos[:, 3].astype(np.float64)
        sq = vel[:, 0]*vel[:, 0] + vel[:, 1]*vel[:, 1] + vel[:, 2]*vel[:, 2]
        assert sq.dtype == np.float32
        g = np.asarray(problem.physparams.gravity, dtype=np.float32).astype(np.float64)
        terms = np.zeros((n, 3))
        terms[:, 0] = m*(sq/np.float32(2)).astype(np.float64)
        terms[:, 1] = -m*(gp[:, 0]*g[0] + gp[:, 1]*g[1] + gp[:, 2]*g[2])
        if energy is not None:
            terms[:, 2] = m*np.asarray(energy, dtype=np.float32).astype(np.float64)
        cls = np.where(info_type(info) == D.PT_FLUID, (info[:, 1] >> 12).astype(np.int64), D.MAX_FLUID_TYPES)
        for c in range(CLASSES):
            rows = active & (cls == c)
            out["rows"][c] = int(rows.sum())
            for k in range(3):
                t = terms[rows, k]
                out["energy"][c, k] = math.fsum(t) if np.isfinite(t).all() else np.nan
                out["abs"][c, k] = math.fsum(np.abs(t)) if np.isfinite(t).all() else np.nan
        if active.any():
            out["max_speed"] = np.float32(np.fmax.reduce(np.sqrt(sq[active]), initial=np.float32(0.0)))      # fmax ignores NaN
        bad = active & ~np.isfinite(gp).all(axis=1)
        if bad.any():
            out["nan_row"] = int(np.nonzero(bad)[0][0])
    return out


def check_sums(got_energy, got_rows, want, what=""):
    """the energies [CLASSES, 3] to (n + 8) 2^-52 sum|term| per class, NaN where the rule's is; the row counts exactly"""
    got_energy = np.asarray(got_energy, dtype=np.float64)
    assert got_energy.shape == (CLASSES, 3)
    assert np.array_equal(np.asarray(got_rows).astype(np.int64), want["rows"]), (what, got_rows, want["rows"])
    worst = 0.0
    for c in range(CLASSES):
        for k in range(3):
            w, a = want["energy"][c, k], want["abs"][c, k]
            if np.isnan(w):
                assert np.isnan(got_energy[c, k]), (what, c, k, got_energy[c, k])
                continue
            bound = (want["rows"][c] + 8)*2.0**-52*a
            err = abs(got_energy[c, k] - w)
            if a > 0:
                worst = max(worst, err/(2.0**-52*a))
            assert err <= bound, (what, c, k, got_energy[c, k], w, err, bound)
    print("diagnostics %s: rows %s, worst error %.3g x 2^-52 sum|term|" % (what, want["rows"].tolist(), worst))


def check_out(out, want, what=""):
    """the raw result of sphx_save_diagnostics (DOUBLES float64) against the rule"""
    out = np.asarray(out, dtype=np.float64)
    assert out.shape == (DOUBLES,)
    s = out[:MAXSQ].reshape(CLASSES, 4)
    check_sums(s[:, :3], s[:, 3], want, what)
    assert np.array_equal(s[:, 3], want["rows"].astype(np.float64))
    maxsq = out[MAXSQ]
    assert np.float64(np.float32(maxsq)) == maxsq                        # a float, widened
    got_speed = np.sqrt(np.float32(maxsq))
    assert got_speed.view(np.uint32) == want["max_speed"].view(np.uint32), (what, got_speed, want["max_speed"])
    assert out[NANROW] == (NO_ROW if want["nan_row"] is None else float(want["nan_row"])), (what, out[NANROW], want["nan_row"])
    assert not out[NANROW + 1:].any()
