"""GPU: the transcripts of tests/test_binding_calls_cpu.py on torch.cuda inputs (tests/golden/B1_binding_calls_device.json, recorded on
an MI355X from the binding as it stood before the marshalling was folded into one place).  The library is the recorder's stand-in: no
kernel runs.  Inputs and outputs resolve by data_ptr(); an uploaded temporary or a resident table copy is "tmp" (what such
temporaries hold stays with the numerical GPU tests)."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "B1_binding_calls_device.json")
# the parent had already set the stream when it refused an in-out array of the re-close; the refusal now comes before any call
RECLOSE_REFUSALS = ("reclose_scan/error-cert-dtype", "reclose_scan/error-cert-missing", "reclose_scan/error-lam-not-contiguous")


def _compute(calls):
    from tests.tools import binding_recorder as br
    return [c for c in calls if c[0] not in br.QUIET]


@pytest.fixture(scope="module")
def br():
    from tests.tools import binding_recorder
    return binding_recorder


@pytest.fixture(scope="module")
def device():
    import torch
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def recorded(br, device):
    return br.record_all(device)


def test_transcripts_match_the_parent(br, golden, recorded):
    assert sorted(recorded) == sorted(golden) and len(recorded) > 140
    skip = br.LINE_SURF_CASES["device"] + RECLOSE_REFUSALS
    bad = [k for k in sorted(golden) if k not in skip and recorded[k] != golden[k]]
    assert not bad, "\n".join("%s:\n  now    %s\n  golden %s" % (k, recorded[k], golden[k]) for k in bad[:5])


def test_line_surf_is_checked_against_the_surface_count_of_tabs(br, golden, recorded):
    """the one deliberate difference: a host line_surf is checked against the n_surf the library is given -- that of `tabs`, here
    twice the tables' own -- where the parent checked fieldline_geometry against len(tables.s) whatever `tabs` held"""
    (case,) = br.LINE_SURF_CASES["device"]
    assert golden[case] == dict(calls=[], result="IbsError: line_surf out of range")
    calls = _compute(recorded[case]["calls"])
    assert [c[0] for c in calls] == ["ibs_fieldline_geometry_f64"] and calls[0][1][1] == "i:8"
    for k in ("fieldline_geometry/tabs-host-lines-beyond", "fieldline_geometry_vjp/tabs-host-lines-beyond"):
        assert recorded[k] == dict(calls=[], result="IbsError: line_surf out of range")


@pytest.mark.parametrize("case", RECLOSE_REFUSALS)
def test_a_refused_in_out_array_reaches_no_library_call(golden, recorded, case):
    assert [c[0] for c in golden[case]["calls"]] == ["ibs_set_stream"]
    assert recorded[case] == dict(calls=[], result=golden[case]["result"])


def test_errors_reach_no_library_call(br, recorded):
    errs = [k for k, v in recorded.items() if br.is_error(v["result"])]
    assert len(errs) >= 25
    assert not [k for k in errs if recorded[k]["calls"]]


def test_mixing_numpy_and_device_arrays_is_refused(recorded):
    for k in ("mixed/solve_gcf", "mixed/gamma_scan"):
        assert recorded[k] == dict(calls=[], result="IbsError: mixing host (numpy) and device (torch.cuda) arrays in one call is "
                                                    "not supported")


@pytest.mark.parametrize("side_stream", [False, True])
def test_every_compute_call_follows_one_set_stream_of_the_current_stream(br, device, side_stream):
    import contextlib
    import torch
    s = torch.cuda.Stream(device) if side_stream else None
    n_compute = 0
    with br.stand_in(True) as fake, (torch.cuda.stream(s) if side_stream else contextlib.nullcontext()):
        want = torch.cuda.current_stream(device).cuda_stream
        assert (want != 0) == side_stream
        ctx = br.ibs_amd.Context(0)
        d = br.make_data(device)
        for name, method, args, kw, inout in br.cases(d, device):
            rec = br.run_case(ctx, fake, method, args, kw, inout)
            host_call = [c for c in rec["calls"] if c[1][-1] == "i:1" and c[0] not in br.QUIET]       # (mem = host: the mixed-sigma case)
            if br.is_error(rec["result"]) or host_call:
                assert not fake.streams, name
                continue
            calls = [c[0] for c in rec["calls"] if c[0] != "ibs_set_option"]
            assert (calls or method == "upload_tables_rows") and len(calls) % 2 == 0, (name, calls)
            assert all(c == "ibs_set_stream" for c in calls[0::2]) and not any(c in br.QUIET for c in calls[1::2]), (name, calls)
            assert fake.streams == [want] * (len(calls) // 2), (name, fake.streams, want)
            n_compute += len(calls) // 2
        ctx.close()
    assert n_compute > 120
    if side_stream:
        torch.cuda.synchronize(device)
