"""What the one-domain records of tests/test_driver_trace.py do not see (tests/driver_trace.py says what each record holds):
rank 0 of two domains with its halo exchanges, reductions and host reads in one call list, or the driver's refusal of an option set
that is built for a single domain; and the host's reads of device words during the one-domain runs.  Not one exchange, reduction or
host read more per step than the records have: each of them is a wait of the step on another device or on the host."""
import json

import pytest

import driver_trace as dt

REFUSED = {"satwofluidbox": ["NotImplementedError", "SPH_HA with SA_BOUNDARY is built for a single domain"],
           "lithostatic_column": ["NotImplementedError", "the GRANULAR rheology is built for a single domain"]}


def _want(name):
    with open(dt.golden_path(name)) as f:
        return json.load(f)


def test_the_cases_on_two_ranks():
    assert set(dt.RANKS2_CASE_NAMES) >= {"dambreak", "dambreak_sps_xsph_shepard", "wavetank", "internal_energy", "grenier",
                                         "sabox_stillwater", "sabox_spheric2", "spheric2_keps", "sapaddlebox", "sachannelio",
                                         "sachannelioflap", "satwofluidbox", "lithostatic_column"}


@pytest.mark.parametrize("case", dt.RANKS2_CASE_NAMES)
def test_rank_0_of_two_equals_the_record(case):
    want = _want("ranks2_" + case)
    got = dt.record_ranks2(case)
    if case in REFUSED:
        assert got == {"refused": REFUSED[case]} == want
        return
    names = [c[0] for c in got["calls"]]
    assert names.count("transport.exchange") > 0 and names.count("transport.allreduce_min") == dt.STEPS
    # the forces pass took its two-stripe branch: the edge stripe [3n/4, n) first, then [0, 3n/4)
    stripes = [c[1][-3:-1] for c in got["calls"] if c[0].startswith("forces") and c[0] != "forces_internal_energy"]
    assert stripes and all(a[0] > 0 and b == [0, a[0]] for a, b in zip(stripes[::2], stripes[1::2]))
    for i, (a, b) in enumerate(zip(got["calls"], want["calls"])):
        assert a == b, "%s, call %d" % (case, i)
    assert got == want


@pytest.mark.parametrize("case", dt.CASE_NAMES)
def test_host_reads_equal_the_record(case):
    assert dt.host_reads(case) == _want("host_reads")[case]


def test_host_reads_of_a_plain_run():
    """three steps of a dam break with a re-sort every second step read the particle count twice and nothing else"""
    assert _want("host_reads")["dambreak"]["steps"] == [["host.item", ["new_num+0[1]"], {}]] * 2
