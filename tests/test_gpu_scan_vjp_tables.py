"""GPU: the fused scan VJP composed with the geometry's VJP -- BallooningScan.smooth_max on wout-derived tables (the golden fixtures
tests/test_gpu_geometry_vjp.py loads) against a central difference with the geometry recomputed -- and the device transcripts of
Context.gamma_scan_vjp against tests/golden/B3_scan_vjp_calls_host.json."""
import json
import os

import numpy as np
import pytest

import ibs_amd

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
S = np.array([0.6, 0.9])
N, NALPHA, NTHETA0, BETA = 131, 3, 3, 20.0


@pytest.fixture(scope="module")
def ctx():
    c = ibs_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wout():
    return dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz")))


def test_smooth_max_of_the_coarse_table_and_its_table_gradient(ctx, wout):
    """7. 2 surfaces, nalpha = 3, ntheta0 = 3, N = 131, beta = 20: the value inside max - log(9) / beta <= value <= max and equal to
    objective.smooth_max of the scan's own coarse table; tab_mn_bar contracted with a random table direction (each entry of tab_mn
    times a standard normal) against the central difference of the value with the geometry recomputed from tab_mn +- 1e-4 direction
    on the host path: within 1e-4 of |gradient| (the bar of tests/test_gpu_vjp.py (e) for differences that recompute the geometry)"""
    import torch
    from ibs_amd.objective import smooth_max
    dev = torch.device("cuda:0")
    th = ibs_amd.theta_grid(N)
    tabs = ibs_amd.SurfaceTables.from_wout(wout, S)
    scan = ibs_amd.BallooningScan(ctx, None, th, S, nalpha=NALPHA, ntheta0=NTHETA0, tables=tabs, device=dev, surf_index=np.arange(2))
    r = scan.smooth_max(BETA)
    value, top = r["value"].cpu().numpy(), r["max"].cpu().numpy()
    assert value.shape == top.shape == (2,)
    assert (value <= top).all() and (value >= top - np.log(NALPHA * NTHETA0) / BETA).all(), (value, top)
    coarse = scan.coarse()
    assert np.abs(smooth_max(coarse, BETA) - value).max() <= 1e-12 and np.abs(coarse.reshape(2, -1).max(1) - top).max() <= 1e-12
    assert tuple(r["tab_mn_bar"].shape) == tabs.tab_mn.shape and tuple(r["tab_nyq_bar"].shape) == tabs.tab_nyq.shape
    assert tuple(r["scal_bar"].shape) == (2, 6)
    for k in ("tab_mn_bar", "tab_nyq_bar", "scal_bar"):
        assert torch.isfinite(r[k]).all() and r[k].abs().max() > 0, k
    dirn = np.random.default_rng(23).standard_normal(tabs.tab_mn.shape) * tabs.tab_mn
    h = float(th[1] - th[0])
    surf, alphas = np.repeat(np.arange(2, dtype=np.int32), NALPHA), np.tile(scan.alpha_scan, 2)

    def value_at(eps):
        t = ibs_amd.SurfaceTables.from_wout(wout, S)
        t.tab_mn += eps * dirn
        geo = ctx.fieldline_geometry(t, surf, alphas, th)
        gam = ctx.gamma_scan(h, *[geo["geo"][k] for k in range(7)], geo["dPdrho"], scan.theta0_scan)["gam"]
        return smooth_max(gam.reshape(2, NALPHA, NTHETA0), BETA)
    assert np.abs(value_at(0.0) - value).max() <= 1e-12
    step = 1e-4
    fd = (value_at(step) - value_at(-step)) / (2 * step)
    an = (r["tab_mn_bar"].cpu().numpy() * dirn).sum(axis=(1, 2))
    print("smooth_max: value", value, "max", top, "analytic", an, "central difference", fd, "rel", np.abs(an - fd) / np.abs(an))
    assert (np.abs(an - fd) <= 1e-4 * np.abs(an)).all(), (an, fd)


def test_smooth_max_needs_tables_and_a_device(ctx):
    th = ibs_amd.theta_grid(N)
    scan = ibs_amd.BallooningScan(ctx, lambda s, a: None, th, S, nalpha=NALPHA, ntheta0=NTHETA0)
    with pytest.raises(ibs_amd.IbsError):
        scan.smooth_max(BETA)


def as_device(host):
    """the device transcript a host transcript of this method corresponds to"""
    def result(r):
        if isinstance(r, dict):
            return {k: result(v) for k, v in r.items()}
        return r.replace("numpy:", "torch:", 1) if isinstance(r, str) and r.startswith("numpy:") else r
    calls = []
    for sym, args in host["calls"]:
        assert args[-1] == "i:1"
        args = ["tmp" if a.startswith("bcast:") else a for a in args]          # (a scalar sigma is expanded on the device)
        calls += [["ibs_set_stream", ["handle", "stream"]], [sym, args[:-1] + ["i:0"]]]
    return dict(calls=calls, result=result(host["result"]))


def test_device_transcripts_are_the_host_ones():
    """Context.gamma_scan_vjp on torch.cuda inputs under the recorder's stand-in library (no kernel runs): every case is its host
    transcript of B3 with mem = 0, torch outputs and one ibs_set_stream before the compute call; errors and mixed host / device
    arrays reach no library call"""
    import torch
    from tests import test_scan_vjp_cpu as ts
    dev = torch.device("cuda:0")
    with open(ts.GOLDEN) as fh:
        golden = json.load(fh)
    rec = ts.record(dev)
    mixed = sorted(k for k in rec if k.startswith("mixed/"))
    assert sorted(k for k in rec if k not in mixed) == sorted(golden) and len(mixed) == 2
    bad = [k for k in sorted(golden) if rec[k] != as_device(golden[k])]
    assert not bad, "\n".join("%s:\n  now    %s\n  wanted %s" % (k, rec[k], as_device(golden[k])) for k in bad[:5])
    for k in mixed:
        assert rec[k] == dict(calls=[], result="IbsError: mixing host (numpy) and device (torch.cuda) arrays in one call is not supported"), rec[k]
    assert not [k for k, v in rec.items() if ts.br.is_error(v["result"]) and v["calls"]]
