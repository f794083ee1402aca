"""GPU: the transcripts of tests/test_modes_cpu.py on torch.cuda inputs.  The library is the recorder's stand-in: no kernel runs.
A device call hands over the caller's own tensors and the outputs it returns, as the host call hands over contiguous float64 arrays:
so the device transcript of every case is its host transcript (tests/golden/B2_modes_calls_host.json) with mem = 0 in place of 1,
torch outputs in place of numpy ones, and one ibs_set_stream of the current stream before the compute call; errors and mixed
host / device arrays reach no library call at all."""
import json

import pytest

pytestmark = pytest.mark.gpu


def as_device(host):
    """the device transcript a host transcript of these methods corresponds to"""
    def result(r):
        if isinstance(r, dict):
            return {k: result(v) for k, v in r.items()}
        return r.replace("numpy:", "torch:", 1) if isinstance(r, str) and r.startswith("numpy:") else r
    calls = []
    for sym, args in host["calls"]:
        assert args[-1] == "i:1"
        calls += [["ibs_set_stream", ["handle", "stream"]], [sym, args[:-1] + ["i:0"]]]
    return dict(calls=calls, result=result(host["result"]))


def test_device_transcripts_are_the_host_ones():
    import torch
    from tests import test_modes_cpu as tm
    dev = torch.device("cuda:0")
    with open(tm.GOLDEN) as fh:
        golden = json.load(fh)
    rec = tm.record(dev)
    mixed = sorted(k for k in rec if k.startswith("mixed/"))
    assert sorted(k for k in rec if k not in mixed) == sorted(golden) and len(mixed) == 3
    bad = [k for k in sorted(golden) if rec[k] != as_device(golden[k])]
    assert not bad, "\n".join("%s:\n  now    %s\n  wanted %s" % (k, rec[k], as_device(golden[k])) for k in bad[:5])
    for k in mixed:
        assert rec[k] == dict(calls=[], result="IbsError: mixing host (numpy) and device (torch.cuda) arrays in one call is not supported"), rec[k]
    assert not [k for k, v in rec.items() if tm.br.is_error(v["result"]) and v["calls"]]
