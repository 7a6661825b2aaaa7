"""The exact body sums' format in plain Python (tests/floating_exact_ref.py), the known answer every other test of
csrc/floating_exact.hip leans on: its rounding against math.fsum bit for bit, on random rows of very mixed size and on rows whose
sum is known by reasoning (the whole float range, ties at 53 bits, cancelling pairs, rows that are not finite); canonical form;
and the property the feature rests on: the limbs of any permutation and of any split into two or three parts add up, slot by slot,
to arrays that round to the same bits.  No GPU."""
import math

import numpy as np
import pytest

import floating_exact_ref as fx
import floating_ref as fr


def _rows(n, rng, scale=5.0):
    f = (rng.normal(size=(n, 4))*scale*10.0**rng.integers(-3, 3, size=(n, 1))).astype(np.float32)
    t = (rng.normal(size=(n, 4))*scale*10.0**rng.integers(-3, 3, size=(n, 1))).astype(np.float32)
    f[:, 3] = 1e30; t[:, 3] = -1e30
    return f, t


@pytest.mark.parametrize("name", sorted(fx.KNOWN))
def test_known_answers(name):
    rows, want = fx.KNOWN[name]
    slots = fx.limbs_of(rows)
    assert all(0 <= l < 2**32 for l in slots[:9]) and abs(slots[9]) < 2**21 and all(c >= 0 for c in slots[10:])
    got = fx.round_slots(np.array(slots, dtype=np.float64))
    assert fx.same_bits(got, want), (got, want)
    if math.isfinite(want):
        assert fx.same_bits(math.fsum(rows), want) and not any(slots[10:])
    else:
        assert sum(slots[10:]) == sum(1 for v in rows if not math.isfinite(v))


def test_random_rows_against_fsum_and_the_canonical_form():
    rng = np.random.default_rng(11)
    rowstart = np.array([3, 403, 1000], dtype=np.uint32)
    rbf, rbt = _rows(1010, rng)
    rbf[1000:, :3] = 7e9
    L = fx.limbs(rbf, rbt, rowstart)
    assert L.shape == (2, 6, 13) and np.array_equal(L, np.floor(L)) and not L[:, :, 10:].any()
    assert (L[:, :, :9] >= 0).all() and (L[:, :, :9] < 2.0**32).all() and (np.abs(L[:, :, 9]) < 2.0**21).all()
    assert (L[:, :, 9] == -1).any() and (L[:, :, 9] == 0).any()      # negative sums: the top limb is the floor
    assert fx.same_bits(fx.round_limbs(L), fr.fsum_rows(rbf, rbt, rowstart))
    # the integer itself: limbs back to N, N 2^-149 against the sum of the rows as fractions
    from fractions import Fraction
    n = sum(int(l) << (32*k) for k, l in enumerate(L[1, 4, :10]))
    assert Fraction(n, 1 << 149) == sum(Fraction(float(v)) for v in rbt[403:1000, 1])


def _zeroed(a, keep):
    out = a.copy()
    out[~keep, :3] = 0.0
    return out


@pytest.mark.parametrize("case", ["random", "range", "ties", "nonfinite"])
def test_permutations_and_splits_round_to_the_same_bits(case):
    rng = np.random.default_rng(5)
    if case == "random":
        rbf, rbt = _rows(301, rng)
    else:
        rbf, rbt, _ = fx.known_rows(fx.KNOWN_BODIES[("range", "ties", "nonfinite").index(case)])
        rbf, rbt = np.tile(rbf, (3, 1)), np.tile(rbt, (3, 1))       # several rows of each kind, so that every part of a split has some
    n = len(rbf)
    rowstart = np.array([0, n], dtype=np.uint32)
    whole = fx.limbs(rbf, rbt, rowstart)
    want = fx.round_limbs(whole)
    perm = rng.permutation(n)
    assert np.array_equal(fx.limbs(rbf[perm], rbt[perm], rowstart), whole)      # the same integer: the same canonical limbs
    idx = np.arange(n)
    for parts in ([idx < n//2, idx >= n//2], [idx % 2 == 0, idx % 2 == 1], [idx % 3 == 0, idx % 3 == 1, idx % 3 == 2],
                  [idx < n//3, (idx >= n//3) & (idx < 2*n//3), idx >= 2*n//3], [rng.random(n) < 0.3]):
        if len(parts) == 1:
            parts = [parts[0], ~parts[0]]
        each = [fx.limbs(_zeroed(rbf, keep), _zeroed(rbt, keep), rowstart) for keep in parts]
        for order in (each, each[::-1]):
            total = np.zeros_like(whole)
            for e in order:
                total = total + e
            assert fx.same_bits(fx.round_limbs(total), want)
    if case in ("random", "range", "ties"):
        assert fx.same_bits(want, fr.fsum_rows(rbf, rbt, rowstart))
