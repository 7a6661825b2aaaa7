"""The preconditions of tests/test_gpu_tiling_overflow.py, proved on the CPU oracle: every case of tests/tiling_overflow_cases.py has a
neighbour list that FITS (a forces pass over one that did not is outside the contract) and a tiling that cannot -- by the trigger the
case is there for.  The limits are read from the sources, so that a change of them fails here and not silently on the device."""
import pytest

import tiling_overflow_cases as toc


def test_limits_are_the_ones_the_cases_were_made_for():
    assert toc.limits() == dict(list=128, pmax=640, wcap=2876, wcap_sps1=2156, wcap_sps=1720)


@pytest.mark.parametrize("case", sorted(toc.CASES))
def test_tiling_overflows_and_the_list_does_not(case):
    lim = toc.limits()
    prob = toc.CASES[case]()
    s = toc.survey(prob)
    first, second, home, window = s["first"], s["second"], s["home"], s["window"]
    long_rows = int(((first > lim["list"]) | (second > lim["list"])).sum())
    print("%s: n = %d, list %d/%d, hasTooManyNeibs %d, rows with a section > %d: %d (longest fluid section %d, second %d), "
          "largest home column %d, largest window %d"
          % (case, s["n"], s["listsize"][0], s["listsize"][1], s["too_many"], lim["list"], long_rows, first.max(), second.max(),
             home.max(), window.max()))
    assert s["too_many"] == -1, "a neighbour list of this case does not fit: no forces pass may run on it"
    sps = prob.simparams.turbmodel == toc.D.SPS
    wcap = (lim["wcap_sps"] if prob.physparams.numFluids() > 1 else lim["wcap_sps1"]) if sps else lim["wcap"]
    if case == "clump":      # build_tiles_kernel's trigger: one cell holds the clump, and a list entry can still index it
        assert home.max() > lim["pmax"] and prob.clumped > lim["pmax"]
        assert home.max() <= 2047
    else:                    # tile_lists_kernel's trigger ...
        assert long_rows > 0
    if case.startswith("wide"):      # ... and that one alone
        assert home.max() <= lim["pmax"] and window.max() <= wcap


def test_the_unclumped_problem_tiles():
    """the other state of the recovery test: nothing of it reaches a limit"""
    lim = toc.limits()
    s = toc.survey(toc.unclumped())
    assert s["too_many"] == -1
    assert max(s["first"].max(), s["second"].max()) <= lim["list"]
    assert s["home"].max() <= lim["pmax"]
