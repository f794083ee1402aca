"""CPU: what every array-marshalling Context method hands to the C library, on numpy inputs, against the transcripts recorded from the
binding as it stood before the marshalling was folded into one place (tests/golden/B1_binding_calls_host.json, written by
tests/tools/binding_recorder.py).  Argument order, scalar types and values, which input, output or converted copy each pointer is,
the shape and dtype of every output, the want_* wiring and the nbad pass-through must all come out the same."""
import json
import os

import pytest

from tests.tools import binding_recorder as br

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "B1_binding_calls_host.json")
COMPUTE = lambda calls: [c for c in calls if c[0] not in br.QUIET]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def recorded():
    return br.record_all()


def test_case_list_is_the_golden_one(golden, recorded):
    assert sorted(recorded) == sorted(golden)
    assert len(recorded) > 120


def test_transcripts_match_the_parent(golden, recorded):
    bad = [k for k in sorted(golden) if k not in br.LINE_SURF_CASES["host"] and recorded[k] != golden[k]]
    assert not bad, "\n".join("%s:\n  now    %s\n  golden %s" % (k, recorded[k], golden[k]) for k in bad[:5])


def test_host_calls_never_set_a_stream(recorded):
    assert not [k for k, v in recorded.items() if any(c[0] == "ibs_set_stream" for c in v["calls"])]


def test_errors_reach_no_compute_call(recorded):
    errs = [k for k, v in recorded.items() if br.is_error(v["result"])]
    assert len(errs) >= 20
    assert not [k for k in errs if COMPUTE(recorded[k]["calls"])]


@pytest.mark.parametrize("case", br.LINE_SURF_CASES["host"])
def test_line_surf_is_range_checked_on_host_arrays(golden, recorded, case):
    """the one deliberate difference: the parent left an out-of-range host line_surf of the VJP and the tangent to the library"""
    assert COMPUTE(golden[case]["calls"])
    assert recorded[case] == dict(calls=[], result="IbsError: line_surf out of range")


def test_the_real_library_is_back():
    from ibs_amd import _lib
    with br.stand_in() as fake:
        assert _lib.lib() is fake
    assert not isinstance(_lib._LIB, br.StandIn)
