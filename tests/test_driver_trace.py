"""The driver's command sequence per option set equals the records under tests/golden/driver_trace (tests/driver_trace.py says
what a record holds): the backend calls of three steps across a second re-sort with the allocation behind every tensor argument,
the halo state in its order, the HotFile set and its count, the keys of download(), and which allocation every attribute names at
the end.  The records were taken from the driver as it stood before the buffer table (gpusph_amd/multigpu.py, BUFFERS)."""
import json

import pytest

import driver_trace as dt


@pytest.mark.parametrize("case", dt.CASE_NAMES)
def test_driver_trace_equals_the_record(case):
    with open(dt.golden_path(case)) as f:
        want = json.load(f)
    got = dt.record(case)
    by_method = got.pop("halo_state_method", got["halo_state"])      # (a driver from before the table has no halo_state())
    assert by_method == got["halo_state"]
    for where in ("steps", "repack"):
        g, w = (got, want) if where == "steps" else (got.get("repack"), want.get("repack"))
        if w is None:
            assert g is None
            continue
        for i, (a, b) in enumerate(zip(g["calls"], w["calls"])):
            assert a == b, "%s, call %d of %s" % (case, i, where)
        assert len(g["calls"]) == len(w["calls"])
        assert g["attributes"] == w["attributes"]
    assert got == want
