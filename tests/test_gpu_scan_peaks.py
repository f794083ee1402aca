"""GPU: k_scan_peaks (ibs_scan_peaks_f64) against ibs_amd.pick_starts, exactly, on host and device pointers; slot 0 against
ibs_surface_argmax_pack_f64 + ibs_scan_starts_f64; the two-bump lines on the device; and the drivers' n_starts on the NCSX tables of
tests/golden/G8_*."""
import os

import numpy as np
import pytest

from tests import scan_peaks_cases as pc
from tests.helpers import OracleContext

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
# 63 / 64 / 65 entries on a wave edge, 272 just past a 256-thread block, several entries per thread
SHAPES = ((1, 1), (1, 5), (5, 1), (7, 9), (8, 8), (5, 13), (16, 17), (24, 15), (40, 33))
N_SURFS = (1, 3, 365)
TOL = 1e-8            # the project's FP64 tolerance for refined maxima


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.close()


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def run_peaks(ctx, tabs, K, device, n_bad0=5):
    """every output of Context.scan_peaks as numpy, with n_bad preset to n_bad0 (the call adds to it)"""
    n, na, nt = tabs.shape
    al, t0 = pc.grids(na, nt)
    nb = np.full(1, n_bad0, dtype=np.int32)
    args = (up(al), up(t0), up(tabs), K, up(nb)) if device else (al, t0, tabs, K, nb)
    r = ctx.scan_peaks(*args, want_sigma0=True, want_index=True, want_found=True)
    assert r["n_bad"] is args[4]
    r = {k: (v.cpu().numpy() if device else v) for k, v in r.items()}
    r["n_bad"] = int(r["n_bad"][0]) - n_bad0
    return r


def same(got, ref, msg, rows=slice(None)):
    for k in ("start", "peak", "sigma0"):
        assert np.array_equal(pc.bits(got[k][rows]), pc.bits(ref[k][rows])), (msg, k)
    assert np.array_equal(got["index"][rows], ref["index"][rows]) and np.array_equal(got["n_found"][rows], ref["n_found"][rows]), msg


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_kernel_equals_pick_starts(ctx, shape):
    """starts, values and shifts bit for bit, indices, n_found and the n_bad increment, for every value family, K and n_surf, on
    host and on device pointers; the healthy surfaces beside a NaN one keep their bits; a second call and the reversed order of
    the surfaces give the same bits per surface"""
    na, nt = shape
    multi = 0
    for K in pc.STARTS:
        normal_dev = None
        for fam in pc.FAMILIES:
            tabs = pc.family(fam, max(N_SURFS), na, nt, 77)          # (one seed: "nan_mixed" is "normal" with two surfaces overwritten)
            ref = pc.pick_all(tabs, K)
            multi += int((ref["n_found"] > 1).sum())
            for n in N_SURFS:
                sub = {k: v[:n] for k, v in ref.items() if k != "n_bad"}         # (the result of a surface does not depend on n_surf)
                sub["n_bad"] = int(ref["bad"][:n].sum())
                for device in (False, True):
                    got = run_peaks(ctx, tabs[:n], K, device)
                    msg = (shape, K, fam, n, "device" if device else "host")
                    same(got, sub, msg)
                    assert got["n_bad"] == sub["n_bad"], (msg, got["n_bad"], sub["n_bad"])
            assert sub["n_bad"] == ref["n_bad"]
            full = run_peaks(ctx, tabs, K, True)
            same(run_peaks(ctx, tabs, K, True), full, (shape, K, fam, "again"))
            rev = run_peaks(ctx, tabs[::-1], K, True)
            same({k: (v[::-1] if k != "n_bad" else v) for k, v in rev.items()}, full, (shape, K, fam, "reversed"))
            if fam == "normal":
                normal_dev = full
            if fam == "nan_mixed":
                healthy = np.array([j for j in range(len(tabs)) if np.isfinite(tabs[j]).all()])
                assert len(healthy) == len(tabs) - (2 if na * nt > 1 else 1) and ref["n_bad"] == 1
                same(full, normal_dev, (shape, K, "healthy surfaces beside NaN ones"), healthy)
    if na * nt > 9:
        assert multi > 100, multi


@pytest.mark.parametrize("shape", ((1, 1), (7, 9), (8, 8), (16, 17), (24, 15)), ids=lambda s: "%dx%d" % s)
def test_slot_0_is_the_existing_pair(ctx, shape):
    """K = 1: start, sigma0 and the n_bad increment of scan_peaks equal surface_argmax_pack followed by scan_starts, bitwise"""
    import torch
    na, nt = shape
    al, t0 = pc.grids(na, nt)
    for fam in pc.FAMILIES:
        tabs = pc.family(fam, 365, na, nt, 78)
        d = up(tabs)
        nb = torch.zeros(1, dtype=torch.int32, device=d.device)
        st, sg = ctx.scan_starts(up(al), up(t0), ctx.surface_argmax_pack(d.view(365, -1)), nb, want_sigma0=True)
        got = run_peaks(ctx, tabs, 1, True)
        assert np.array_equal(pc.bits(got["start"][:, 0]), pc.bits(st.cpu().numpy())), (shape, fam)
        assert np.array_equal(pc.bits(got["sigma0"][:, 0]), pc.bits(sg.cpu().numpy())), (shape, fam)
        assert got["n_bad"] == int(nb.item()) == (1 if fam == "nan_mixed" else 0), (shape, fam)


def test_two_bump_lines_on_the_device(ctx):
    """the 7 x 3 table of the two-bump surface (tests/test_scan_peaks_cpu.py) from ctx.gamma_scan on the device: the peaks are nodes
    (1, 0) and (4, 0), and the starts those of pick_starts on the oracle's table"""
    import ibs_amd
    N = 131
    th = np.linspace(-4 * np.pi, 4 * np.pi, N)
    h = th[1] - th[0]
    al, t0 = pc.grids(7, 3)
    geo = pc.two_bump_fieldlines(th, al)(0.5, al)
    dP = -0.5 * np.mean((geo[:, 2] - geo[:, 7]) * geo[:, 0] ** 2, axis=1)
    geo7 = [np.ascontiguousarray(geo[:, k]) for k in range(7)]
    dev = ctx.gamma_scan(h, *[up(a) for a in geo7], up(dP), up(t0))["gam"]
    r = ctx.scan_peaks(up(al), up(t0), dev.view(1, 7, 3), 2, want_index=True, want_found=True)
    ref = ibs_amd.pick_starts(OracleContext().gamma_scan(h, *geo7, dP, t0)["gam"], al, t0, 2)
    assert np.array_equal(r["index"].cpu().numpy(), [[3, 12]]) and np.array_equal(ref["index"], [3, 12])
    assert np.array_equal(r["start"].cpu().numpy()[0], ref["start"]) and int(r["n_found"].item()) == 2 and int(r["n_bad"].item()) == 0
    assert np.abs(r["peak"].cpu().numpy()[0] - ref["peak"]).max() < TOL


# ---- the drivers on the NCSX tables
N_DRV = 513
SVALS3 = np.array([0.5, 0.7, 0.9])
GRID = dict(nalpha=8, ntheta0=5)


def wout_ncsx():
    return dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz")))


def driver(ctx, svals, **kw):
    import torch
    import ibs_amd
    th = np.linspace(-4 * np.pi, 4 * np.pi, N_DRV)
    tabs = ibs_amd.SurfaceTables.from_wout(wout_ncsx(), svals)
    return ibs_amd.BallooningScan(ctx, None, th, svals, tables=tabs, device=torch.device("cuda:0"), **GRID, **kw)


def rows_of(scan):
    rows, bad = scan.device_rows()
    assert float(bad.item()) == 0.0
    return rows.cpu().numpy()


def check_multi(ctx, svals, K, **kw):
    """n_starts = K against n_starts = 1 and against refine_batched + final_solve_device from the same starts, slot by slot"""
    one = driver(ctx, svals, **kw)
    r1 = rows_of(one)
    multi = driver(ctx, svals, n_starts=K, **kw)
    rk = rows_of(multi)
    cand = multi.last_candidates.cpu().numpy()
    pk = {k: v.cpu().numpy() for k, v in multi.last_peaks.items()}
    n = len(svals)
    assert cand.shape == (n, K, 3) and pk["index"].shape == pk["value"].shape == (n, K) and pk["n_found"].shape == (n,)
    assert np.array_equal(rk[:, 2], cand[:, :, 2].max(axis=1))
    best = np.argmax(cand[:, :, 2], axis=1)                                # (first maximum: slot 0 wins ties)
    assert np.array_equal(rk, cand[np.arange(n), best])
    assert (rk[:, 2] >= r1[:, 2] - TOL).all(), (rk[:, 2], r1[:, 2])
    assert (pk["n_found"] >= 1).all() and (pk["index"] >= 0).all()
    pad = np.arange(K)[None, :] >= pk["n_found"][:, None]
    assert np.array_equal(pk["index"][pad], np.broadcast_to(pk["index"][:, :1], (n, K))[pad])
    nt = len(one.theta0_scan)
    worst = 0.0
    for k in range(K):
        starts = np.stack([one.alpha_scan[pk["index"][:, k] // nt], one.theta0_scan[pk["index"][:, k] % nt]], axis=1)
        sg = 1.3 * np.abs(pk["value"][:, k]) + 0.05 if one.nearest else None
        xo, fo, rounds = one.refine_batched(starts, sigma0=sg)
        gam = one.final_solve_device(xo)
        worst = max(worst, float(np.abs(gam - cand[:, k, 2]).max()))
    print("multi-start figures: %s K=%d  gam(K) - gam(1) per surface: %s; n_found %s; worst |candidate - refine_batched| %.2e" % (
        kw or "max/reference", K, " ".join("%.3e" % x for x in rk[:, 2] - r1[:, 2]), pk["n_found"], worst))
    assert worst < TOL, worst
    return r1, rk


def test_one_start_takes_the_old_path_bitwise(ctx):
    plain = rows_of(driver(ctx, SVALS3))
    one = driver(ctx, SVALS3, n_starts=1)
    assert np.array_equal(pc.bits(plain), pc.bits(rows_of(one))) and one.last_candidates is None and one.last_peaks is None
    # without the refinement n_starts > 1 returns slot 0: the rows of one start
    multi = driver(ctx, SVALS3, n_starts=3)
    r0 = multi.device_rows(refine=False)[0].cpu().numpy()
    assert np.array_equal(pc.bits(r0), pc.bits(driver(ctx, SVALS3).device_rows(refine=False)[0].cpu().numpy()))
    assert tuple(multi.last_candidates.shape) == (3, 3, 3)


def test_three_starts_on_three_surfaces(ctx):
    check_multi(ctx, SVALS3, 3)
    t, a, g = driver(ctx, SVALS3, n_starts=3).run()
    assert np.isfinite(g).all() and g.shape == (3,)


@pytest.mark.parametrize("kw", (dict(eigenpair="nearest"), dict(jac="exact"), dict(jac="exact_tangent")),
                         ids=("nearest", "exact", "exact_tangent"))
def test_three_starts_in_the_host_driven_modes(ctx, kw):
    check_multi(ctx, SVALS3[1:], 3, **kw)


def test_all_candidates_are_certified(ctx):
    """certify=True with n_starts = 2: the coarse tables and the final solves of ALL candidates are certified and counted"""
    one = driver(ctx, SVALS3[1:], certify=True)
    r1 = one.local_rows()
    two = driver(ctx, SVALS3[1:], certify=True, n_starts=2)
    r2 = two.local_rows()
    n, per = 2, GRID["nalpha"] * GRID["ntheta0"]
    assert one.last_certificate == dict(checked=n * per + n, reclosed=one.last_certificate["reclosed"], failed=0)
    assert two.last_certificate["checked"] == n * per + 2 * n and two.last_certificate["failed"] == 0
    assert (r2[:, 2] >= r1[:, 2] - TOL).all() and tuple(two.last_candidates.shape) == (2, 2, 3)


def test_adjoint_step_with_two_starts(ctx):
    import torch
    import ibs_amd
    import bench
    dev = torch.device("cuda:0")
    w0 = wout_ncsx()
    wouts = [w0] + bench.emulated_equilibria(w0)[0][1:3]
    steps = np.array([1.0, 1e-3, 2e-3])
    f_other = np.array([0.8, 0.81, 0.82])
    th = np.linspace(-4 * np.pi, 4 * np.pi, N_DRV)
    kw = dict(gamma_thresh=-2.0e-4, prefac=50.0, **GRID)
    one = ibs_amd.AdjointStep(ctx, th, SVALS3[1:], dev, **kw).run(wouts, f_other, steps)
    two = ibs_amd.AdjointStep(ctx, th, SVALS3[1:], dev, n_starts=2, **kw).run(wouts, f_other, steps)
    assert sorted(one) == sorted(two) and two["gam"].shape == (3, 2)
    assert (two["gam"] >= one["gam"] - TOL).all(), (two["gam"], one["gam"])
    assert np.isfinite(two["f0"]).all() and np.isfinite(two["dfobj"]).all() and np.isfinite(two["fobj"])
