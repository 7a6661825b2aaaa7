"""TEST REFERENCE ONLY: the fixed-point accumulator of csrc/floating_exact.hip (include/sphx.h, SPHX_FLOATING_LIMBS) in plain Python
integers, its rounding through Fraction, and ExactOracleKernels, the CPU test backend with floating bodies under the rule of
tests/floating_ref.py, so that gpusph_amd.multigpu runs floating bodies on several gloo ranks without a GPU.

The format: the sum of float rows is N 2^-149 with an integer N (a float is an integer multiple of 2^-149).  Per body and component
13 doubles, all integer-valued: limbs l_0 .. l_9 with N = sum l_k 2^(32 k), canonical when 0 <= l_k < 2^32 for k < 9 and
l_9 = floor(N / 2^288) (signed); then the counts of NaN rows, +Inf rows and -Inf rows, which never enter N."""
import math
from fractions import Fraction

import numpy as np
import torch

import floating_ref as fr
from oracle_kernels import OracleKernels

LIMBS, SLOTS = 10, 13
SCALE = 1 << 149


def limbs_of(values):
    """float rows of one component -> the 13 canonical slots as Python ints"""
    n, nan, pinf, ninf = 0, 0, 0, 0
    for v in np.asarray(values, dtype=np.float32).astype(np.float64).tolist():
        if math.isnan(v):
            nan += 1
        elif math.isinf(v):
            pinf, ninf = pinf + (v > 0), ninf + (v < 0)
        else:
            num, den = v.as_integer_ratio()      # int(Fraction(v) 2^149): den is a power of two up to 2^149
            assert SCALE % den == 0
            n += num*(SCALE//den)
    return [(n >> (32*k)) & 0xFFFFFFFF for k in range(LIMBS - 1)] + [n >> (32*(LIMBS - 1)), nan, pinf, ninf]


def limbs(rbf, rbt, rowstart):
    """[bodies, 6, 13] float64: what sphx_floating_limbs writes for these rows"""
    nb = len(rowstart) - 1
    out = np.zeros((nb, 6, SLOTS))
    for b in range(nb):
        r0, r1 = int(rowstart[b]), int(rowstart[b + 1])
        for k in range(3):
            for c, rows in ((k, rbf), (3 + k, rbt)):
                ints = limbs_of(rows[r0:r1, k])
                out[b, c] = ints
                assert [int(v) for v in out[b, c]] == ints      # every slot is exact in a double
    return out


def round_slots(slots):
    """13 integer-valued slots (canonical or sums of canonical ones) -> the exactly rounded total"""
    ints = [int(v) for v in slots]
    assert all(float(i) == float(v) for i, v in zip(ints, slots))
    nan, pinf, ninf = ints[LIMBS:]
    if nan or (pinf and ninf):
        return float("nan")
    if pinf or ninf:
        return float("inf") if pinf else float("-inf")
    n = sum(l << (32*k) for k, l in enumerate(ints[:LIMBS]))
    return float(Fraction(n, SCALE))      # Fraction -> float rounds to nearest, ties to even


def round_limbs(arr):
    """[bodies, 6, 13] -> [bodies, 6]"""
    arr = np.asarray(arr, dtype=np.float64)
    return np.array([[round_slots(arr[b, c]) for c in range(arr.shape[1])] for b in range(arr.shape[0])]).reshape(arr.shape[0], arr.shape[1])


def same_bits(a, b):
    """equal as bit patterns, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


class ExactOracleKernels(OracleKernels):
    """OracleKernels with the floating-body interface of HipKernels: the rows summed with math.fsum (floating_move) or through the
    limbs (floating_limbs / floating_move_limbs), the rule of floating_ref.RefBodies, the bodies' slots written into the oracle's
    parameter block in every substep as the device writes its table.  Host uploads leave the floating bodies' slots alone."""

    def floating_setup(self, bodies, rowstart):
        self.num_floating = len(bodies)
        self.fl_rowstart = np.asarray(rowstart, dtype=np.int64)
        self.fl = fr.RefBodies(bodies, fr.device_grid(self._problem))
        g = self.fl.grid
        slots = dict(trans=np.zeros((len(bodies), 3), np.float32), rot=np.tile(np.eye(3, dtype=np.float32).ravel(), (len(bodies), 1)),
                     lvel=self.fl.state[:, 7:10].astype(np.float32), avel=self.fl.state[:, 10:13].astype(np.float32))
        cells = [fr.grid_and_local(self.fl.state[b, 0:3], g["origin"], g["cellsize"], g["gridsize"]) for b in range(len(bodies))]
        slots["cg_grid"] = slots["cg_grid_e"] = np.array([c[0] for c in cells])
        slots["cg_pos"] = slots["cg_pos_e"] = np.array([c[1] for c in cells])
        self._write_slots(slots)

    def _write_slots(self, s):
        p = self.op
        for b in range(self.num_floating):
            for a in range(3):
                p.rbtrans[b][a] = float(s["trans"][b][a]); p.rblinearvel[b][a] = float(s["lvel"][b][a])
                p.rbangularvel[b][a] = float(s["avel"][b][a])
                p.rbcgGridPos[b][a] = int(s["cg_grid"][b][a]); p.rbcgPos[b][a] = float(s["cg_pos"][b][a])
                p.rbcgGridPosE[b][a] = int(s["cg_grid_e"][b][a]); p.rbcgPosE[b][a] = float(s["cg_pos_e"][b][a])
            for a in range(9):
                p.rbsteprot[b][a] = float(s["rot"][b][a])
        self.fl_slots = s

    def _others(self, m):
        """the rows of a host upload that reach the table: the bodies behind the floating ones"""
        nf = getattr(self, "num_floating", 0)
        return {k: v[nf:] for k, v in m.items()}, nf

    def set_body_motion(self, m, forces_cg):
        rest, nf = self._others(m)
        p = self.op
        for i in range(len(rest["trans"])):
            b = nf + i
            for a in range(3):
                p.rbtrans[b][a] = float(rest["trans"][i][a]); p.rblinearvel[b][a] = float(rest["lvel"][i][a])
                p.rbangularvel[b][a] = float(rest["avel"][i][a])
                if forces_cg:
                    p.rbcgGridPos[b][a] = int(rest["cg_grid"][i][a]); p.rbcgPos[b][a] = float(rest["cg_pos"][i][a])
            for a in range(9):
                p.rbsteprot[b][a] = float(rest["rot"][i][a])

    def set_body_cg_integration(self, m):
        rest, nf = self._others(m)
        p = self.op
        for i in range(len(rest["trans"])):
            for a in range(3):
                p.rbcgGridPosE[nf + i][a] = int(rest["cg_grid"][i][a]); p.rbcgPosE[nf + i][a] = float(rest["cg_pos"][i][a])

    def floating_limbs(self, rbforces, rbtorques, out):
        out.copy_(torch.from_numpy(limbs(rbforces.numpy(), rbtorques.numpy(), self.fl_rowstart)))

    def floating_move_limbs(self, summed, step, d_dt):
        self._write_slots(self.fl.substep(step, round_limbs(summed.numpy()), float(d_dt[0])))

    def floating_move(self, rbforces, rbtorques, step, d_dt):
        self._write_slots(self.fl.substep(step, fr.fsum_rows(rbforces.numpy(), rbtorques.numpy(), self.fl_rowstart), float(d_dt[0])))

    def floating_state(self, slots=False):
        state = self.fl.state.copy()
        return (state, {k: np.array(v).copy() for k, v in self.fl_slots.items()}) if slots else state


# ---- rows whose exactly rounded sum is known by reasoning (and, where finite, is math.fsum's): name -> (float32 rows, the sum)
TINY, BIG = 2.0**-149, float(np.finfo(np.float32).max)
NAN, INF = float("nan"), float("inf")
KNOWN = {
    # the whole float range in one sum: where FLT_MAX cancels the 2^-149 must survive
    "range_cancels": ([BIG, TINY, -BIG], TINY),
    "range_cancels_negative": ([-BIG, -TINY, BIG, -TINY], -2*TINY),
    "range_keeps_big": ([BIG, TINY], BIG),
    "range_three_big": ([BIG, BIG, -TINY, BIG], 3*BIG),          # 3 FLT_MAX - 2^-149 rounds to 3 FLT_MAX, far inside the doubles
    "range_all_tiny": ([TINY]*5 + [-TINY]*2, 3*TINY),
    # ties at 53 bits: to even, and the smallest float below the tie decides
    "tie_down": ([1.0, 2.0**-53], 1.0),
    "tie_broken": ([1.0, 2.0**-53, TINY], 1.0 + 2.0**-52),
    "tie_down_negative": ([-1.0, -2.0**-53], -1.0),
    "tie_broken_negative": ([-1.0, -2.0**-53, -TINY], -(1.0 + 2.0**-52)),
    "tie_up_to_even": ([1.0, 2.0**-52, 2.0**-53], 1.0 + 2.0**-51),
    "tie_below": ([1.0, 2.0**-53, -TINY], 1.0),
    # pairs x, -x: exactly +0.0
    "pairs": ([3.25, -3.25, BIG, -BIG, TINY, -TINY, -3*2.0**-70, 3*2.0**-70], 0.0),
    "nothing_but_zeros": ([0.0, -0.0, 0.0], 0.0),
    # rows that are not finite
    "a_nan": ([1.0, NAN, 2.0], NAN),
    "plus_inf": ([1.0, INF, -BIG, INF], INF),
    "minus_inf": ([-INF, BIG, BIG], -INF),
    "both_infs": ([INF, 5.0, -INF], NAN),
    "nan_and_inf": ([INF, NAN], NAN),
}


def known_rows(names, first=0, behind=0):
    """six KNOWN cases as the six components of one body: rbf, rbt [first + n + behind, 4] float32 with the body in rows
    [first, first + n), short cases padded with +0.0 rows, the rows around the body and the fourth component never to be counted;
    and the six sums"""
    assert len(names) == 6
    n = max(len(KNOWN[k][0]) for k in names)
    rbf = np.zeros((first + n + behind, 4), dtype=np.float32); rbt = np.zeros_like(rbf)
    rbf[:first, :3] = 7e9; rbt[:first, :3] = -7e9
    rbf[first + n:, :3] = 7e9; rbt[first + n:, :3] = -7e9
    rbf[:, 3] = 1e30; rbt[:, 3] = -1e30
    for c, name in enumerate(names):
        rows = np.array(KNOWN[name][0], dtype=np.float32)
        assert np.array_equal(rows.astype(np.float64), np.array(KNOWN[name][0]), equal_nan=True), name      # the rows are floats
        (rbf if c < 3 else rbt)[first:first + len(rows), c % 3] = rows
    return rbf, rbt, np.array([KNOWN[k][1] for k in names])


KNOWN_BODIES = [("range_cancels", "range_keeps_big", "range_three_big", "range_cancels_negative", "range_all_tiny", "pairs"),
                ("tie_down", "tie_broken", "tie_down_negative", "tie_broken_negative", "tie_up_to_even", "tie_below"),
                ("a_nan", "plus_inf", "minus_inf", "both_infs", "nan_and_inf", "nothing_but_zeros")]
