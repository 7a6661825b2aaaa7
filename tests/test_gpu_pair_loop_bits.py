"""The plain tiled forces pass has a second instantiation for a gravity along z (pair_interact_pk in csrc/forces_tile.h: g.r as the one
product g_z r_z instead of a multiply and two FMAs).  It may change no bit:

  a. a context on it against a context kept on the instantiation for any gravity (sphx_dbg_forces_general_gravity), for gravity
     down and up: forces, the next time step, and positions, velocities, forces and time step after 12 steps (a rebuild at step 10);
  b. gravities with an x or y component take the instantiation for any gravity, and are held to the oracle like the option tests;
  c. every run against tests/golden/pair_loop_parent.npz, which tests/golden/make_pair_loop_golden.py recorded on the device with
     the library of the commit before the second instantiation existed: digests of the arrays, equality demanded.

The problem is DamBreak3D at deltap 0.03 with the obstacle, the seeded perturbation of tests/test_gpu_tiling_overflow.py, a tiling that
is usable (asserted in every run).  No tolerance anywhere in a. and c."""
import functools
import os

import numpy as np
import pytest

import pair_loop_cases as plc
from forces_check import _check_neibs_and_forces

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_loop_parent.npz")


@functools.lru_cache(maxsize=None)
def _run(case, force_general):
    return plc.run(case, force_general=force_general)


def _differing(a, b):
    return ", ".join("%s %d of %d words" % (k, int((a[k].view(np.uint32) != b[k].view(np.uint32)).sum()), a[k].size)
                     for k in a if isinstance(a[k], np.ndarray) and not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)))


@pytest.mark.parametrize("case", plc.ALONG_Z)
def test_gravity_along_z_against_any_gravity(case):
    z, general = _run(case, False), _run(case, True)
    assert z["path"] == 1 and general["path"] == 0
    f = z["forces1"]
    assert np.isfinite(f).all() and np.abs(f[:, :3]).max() > 0 and np.abs(f[:, 3]).max() > 0
    assert np.abs(z["pos12"] - z["pos1"]).max() > 0      # the steps moved something
    for stage in ("1", "12"):
        for k in plc.ARRAYS:
            assert np.array_equal(z[k + stage].view(np.uint32), general[k + stage].view(np.uint32)), \
                "after %s: %s" % ("one pass" if stage == "1" else "%d steps" % plc.STEPS, _differing(z, general))
        assert z["dt" + stage] == general["dt" + stage]


@pytest.mark.parametrize("case", [c for c in plc.GRAVITIES if c not in plc.ALONG_Z])
def test_other_gravities_take_the_general_pass(case):
    assert _run(case, False)["path"] == 0
    eng, _ = _check_neibs_and_forces(plc.problem(case), 51, usable=1)
    assert plc.gravity_path(eng) == 0


def test_minus_zero_counts_as_zero():
    from gpusph_amd.engine import TimestepEngine
    prob = plc.problem("down")
    prob.physparams.gravity = (-0.0, -0.0, -9.81)
    assert plc.gravity_path(TimestepEngine(prob, device="cuda:0", clobber_neibslist=True)) == 1


@pytest.mark.parametrize("case", list(plc.GRAVITIES))
def test_against_the_commit_before(case):
    gold = np.load(GOLDEN)
    runs = [("as chosen", _run(case, False))]
    if case in plc.ALONG_Z:
        runs.append(("kept on any gravity", _run(case, True)))
    for what, res in runs:
        rec = plc.record(case, res)
        assert int(gold[case + "/n"]) == len(res["forces1"])
        for key in sorted(rec):
            if "/rows_" in key or key.endswith("/n"):
                continue
            if "/dt" in key:
                assert float(rec[key]) == float(gold[key]), "%s, %s: %r | %r" % (what, key, float(rec[key]), float(gold[key]))
                continue
            if not np.array_equal(rec[key], gold[key]):
                rows = key.replace("sha256_", "rows_")
                a, b = rec[rows].view(np.uint32), gold[rows].view(np.uint32)
                bad = np.flatnonzero((a != b).any(axis=1))
                err = np.abs(rec[rows].astype(np.float64) - gold[rows].astype(np.float64)).max()
                pytest.fail("%s, %s: digest differs; of the %d rows kept, %d differ (first: row %s), largest difference %g"
                            % (what, key, len(a), len(bad), plc.EVERY*int(bad[0]) if len(bad) else "-", err))
