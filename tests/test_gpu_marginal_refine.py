"""GPU: the objective of the margin's refinement (ibs_marginal_obj_w_grad_f64, csrc/ibs_marginal_points.hip) against the CPU
restatement tests/marginal_points_oracle.py, against ibs_marginal_scan_f64 on the centre line, and the drivers built on it
(BallooningScan.marginal(refine=True), AdjointStep.marginal).

Bounds: |s* - s*_oracle| <= 4 u with u = N eps normT / kappa from the oracle's vector (tests/test_gpu_marginal.py's bound);
|val s*_oracle + 1| <= 4 u / s*_oracle + 4e-16; dscale and jac 1e-9 relative to max(1, |.|), the project's bar for Hellmann-Feynman
sums (s* is homogeneous of degree 1 in g and -1 in c, so rows a few eps apart move d s* / d alpha by a few eps s* / del_alpha ~
1e-13); dPdrho 1e-13 relative.  The measured worst cases are printed (and written to the file named by IBS_MARGINAL_REFINE_REPORT, if
set: profiles/marginal_refine_tests.txt)."""
import os

import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from tests import marginal_oracle as mo
from tests import marginal_points_oracle as mpo
from tests.helpers import synthetic_fieldlines

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
DEL = 0.004
# the lane edge, the vector-chunk edge N - 2 = 383 / 385, the count-chunk edge 767 / 769, and three count chunks
LENGTHS = (67, 69, 129, 385, 387, 769, 771, 2307)
POINTS = ((0.3, 0.0, 0.0), (0.3, 1.1, 0.4), (0.3, np.pi, 0.5 * np.pi), (0.9, 0.0, 0.5 * np.pi), (0.9, 1.1, 0.0), (0.9, np.pi, 0.4))
SVALS = np.array([0.6, 0.9])
KEYS = ("val", "jac", "scale", "dscale", "dPdrho", "info")
_REPORT = []


def report(line):
    print("marginal-refine figures:", line)
    _REPORT.append(line)
    path = os.environ.get("IBS_MARGINAL_REFINE_REPORT")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(_REPORT) + "\n")


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.close()


def triples(N, pts=POINTS):
    """(h, geo (n, 3, 8, N), theta0 (n,)) of synthetic points (s, alpha, theta0)"""
    th = bo.theta_grid(N)
    fl = synthetic_fieldlines(th)
    geo = np.stack([fl(s, np.array([a - 0.5 * DEL, a, a + 0.5 * DEL])) for s, a, _ in pts])
    return th[1] - th[0], geo, np.array([t for _, _, t in pts])


def rel(a, b):
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def check_against_oracle(name, r, ref):
    """the module docstring's bars; returns the report line"""
    assert r["nbad"] == 0 and not (r["info"] >> 16).any(), (name, r["info"] >> 16)
    assert np.isfinite(ref["scale"]).all() and (ref["u"] > 0).all(), name
    err = np.abs(r["scale"] - ref["scale"]) / ref["u"]
    ev = np.abs(r["val"] * ref["scale"] + 1)
    e_ds, e_j = rel(r["dscale"], ref["dscale"]), rel(r["jac"], ref["jac"])
    e_dP = float((np.abs(r["dPdrho"] - ref["dPdrho"]) / np.abs(ref["dPdrho"])).max())
    line = ("%-18s points %d  max |s - s_oracle| / u %.2e  |val s + 1| %.1e  dscale err %.1e  jac err %.1e  dPdrho rel %.1e  passes %.1f"
            % (name, len(err), err.max(), ev.max(), e_ds, e_j, e_dP, (r["info"] & 0xffff).mean()))
    report(line)
    assert (err <= 4).all(), (name, err)
    assert (ev <= 4 * ref["u"] / ref["scale"] + 4e-16).all(), (name, ev)
    assert e_ds <= 1e-9 and e_j <= 1e-9, (name, e_ds, e_j)
    assert e_dP <= 1e-13, (name, e_dP)


@pytest.fixture(scope="module")
def solved(ctx):
    """every synthetic length solved once on the GPU and by the oracle; shared, unchanged, by the tests below"""
    res = {}
    for N in LENGTHS:
        h, geo, t0 = triples(N)
        res[N] = dict(h=h, geo=geo, t0=t0, gpu=ctx.marginal_obj_w_grad(h, geo, t0, DEL, want_info=True), ref=mpo.points(h, geo, t0, DEL))
    return res


@pytest.mark.parametrize("N", LENGTHS)
def test_entry_point_against_the_oracle(solved, N):
    s = solved[N]
    check_against_oracle("synthetic N=%d" % N, s["gpu"], s["ref"])


def g8_tables():
    import ibs_amd
    return ibs_amd.SurfaceTables.from_wout(dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz"))), SVALS)


@pytest.fixture(scope="module")
def real(ctx):
    """G8 tables, 2 surfaces, N = 969, four (alpha, theta0) per surface: the triples from the geometry kernel, resident on the device"""
    import torch
    dev = torch.device("cuda:0")
    N = 969
    th = np.linspace(-4 * np.pi, 4 * np.pi, N)
    pts = [(k, a, t) for k in range(2) for a, t in ((0.0, 0.0), (0.9, 0.3), (2.0, 1.0), (np.pi, 0.5 * np.pi))]
    al = np.array([[a - 0.5 * DEL, a, a + 0.5 * DEL] for _, a, _ in pts]).reshape(-1)
    r = ctx.fieldline_geometry(g8_tables(), np.repeat([k for k, _, _ in pts], 3), al, th, device=dev)
    geo = r["geo"].view(8, len(pts), 3, N).permute(1, 2, 0, 3).contiguous()
    t0 = torch.from_numpy(np.array([t for _, _, t in pts])).to(dev)
    out = ctx.marginal_obj_w_grad(th[1] - th[0], geo, t0, DEL, want_info=True)
    out = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}
    out["nbad"] = int((((out["info"] >> 16) & 3) != 0).sum())
    return dict(h=th[1] - th[0], geo=geo.cpu().numpy(), t0=t0.cpu().numpy(), gpu=out)


def test_real_geometry_against_the_oracle(real):
    check_against_oracle("G8 N=969", real["gpu"], mpo.points(real["h"], real["geo"], real["t0"], DEL))


def test_consistency_with_marginal_scan(ctx, solved, real):
    """at every point scale equals ibs_marginal_scan_f64 on the centre line at that theta0 (fed the entry point's own dPdrho) BITWISE:
    the rows are formed with the same arithmetic and solved by the same marginal_one.  The theta0 component of dscale is held to
    1e-13 relative to max(1, |.|): k_marginal_points forms the three sums in k_marginal_scan's order, so bitwise equality is expected,
    but the two kernels are compiled separately and the compiler's contraction of the closing expression has not been compared on a
    GPU; the measured difference is printed"""
    for name, s in [("synthetic N=%d" % N, solved[N]) for N in (129, 387, 771)] + [("G8 N=969", real)]:
        r = s["gpu"]
        centre = [np.ascontiguousarray(s["geo"][:, 1, k]) for k in range(7)]
        sc = ctx.marginal_scan(s["h"], *centre, r["dPdrho"], s["t0"], want_grad=True)
        d = np.arange(len(s["t0"]))
        e_s = np.abs(r["scale"] - sc["scale"][d, d]).max()
        e_t = float((np.abs(r["dscale"][:, 1] - sc["dscale_dtheta0"][d, d]) / np.maximum(1.0, np.abs(r["dscale"][:, 1]))).max())
        report("%-18s against marginal_scan on the centre line: max |delta scale| %.1e  dscale_dtheta0 rel %.1e" % (name, e_s, e_t))
        assert (r["scale"] == sc["scale"][d, d]).all(), (name, r["scale"], sc["scale"][d, d])
        assert e_t <= 1e-13, (name, r["dscale"][:, 1], sc["dscale_dtheta0"][d, d])


def test_status(ctx):
    """dPdrho = 0: bit 8, scale = inf, val = 0, zero gradient, not counted; a NaN in the centre line: bit 1, everything NaN, counted; a
    NaN in the right line only: bit 1 with val and scale kept and NaN gradients -- and no flag at all without a gradient"""
    h, geo, t0 = triples(129, POINTS[1:2])
    clean = ctx.marginal_obj_w_grad(h, geo, t0, DEL, want_info=True)
    assert clean["nbad"] == 0 and int(clean["info"][0] >> 16) == 0 and np.isfinite(clean["scale"][0])
    flat = geo.copy()
    flat[:, :, 7] = flat[:, :, 2]                            # gbdrift = cvdrift: dPdrho = 0, c = 0
    r = ctx.marginal_obj_w_grad(h, flat, t0, DEL, want_info=True)
    assert r["nbad"] == 0 and int(r["info"][0] >> 16) == 256
    assert np.isinf(r["scale"][0]) and r["scale"][0] > 0 and r["val"][0] == 0.0 and r["dPdrho"][0] == 0.0
    assert (r["jac"] == 0).all() and (r["dscale"] == 0).all()
    bad = geo.copy()
    bad[0, 1, 0, 40] = np.nan                                # the centre line's bmag
    r = ctx.marginal_obj_w_grad(h, bad, t0, DEL, want_info=True)
    assert r["nbad"] == 1 and int(r["info"][0] >> 16) == 2
    assert all(np.isnan(r[k]).all() for k in ("val", "jac", "scale", "dscale", "dPdrho"))
    side = geo.copy()
    side[0, 2, 4, 40] = np.nan                               # the right line's gds2
    r = ctx.marginal_obj_w_grad(h, side, t0, DEL, want_info=True)
    assert r["nbad"] == 1 and int(r["info"][0] >> 16) == 2
    assert r["val"][0] == clean["val"][0] and r["scale"][0] == clean["scale"][0] and r["dPdrho"][0] == clean["dPdrho"][0]
    assert np.isnan(r["jac"]).all() and np.isnan(r["dscale"]).all()
    r = ctx.marginal_obj_w_grad(h, side, t0, DEL, want_grad=False, want_info=True)
    assert r["nbad"] == 0 and int(r["info"][0] >> 16) == 0 and "jac" not in r and "dscale" not in r
    assert abs(r["scale"][0] - clean["scale"][0]) <= 4 * mpo.points(h, geo, t0, DEL, False)["u"][0]


def test_repeatability(ctx):
    """one point against 300 copies, host pointers against device pointers: bitwise equal on every output"""
    import torch
    h, geo, t0 = triples(387, POINTS[1:2])
    one = ctx.marginal_obj_w_grad(h, geo, t0, DEL, want_info=True)
    many = ctx.marginal_obj_w_grad(h, np.tile(geo, (300, 1, 1, 1)), np.tile(t0, 300), DEL, want_info=True)
    for k in KEYS:
        assert np.isfinite(one[k]).all() and (many[k] == one[k][0]).all(), k
    dev = torch.device("cuda:0")
    d = ctx.marginal_obj_w_grad(h, torch.from_numpy(np.tile(geo, (300, 1, 1, 1))).to(dev), torch.from_numpy(np.tile(t0, 300)).to(dev),
                                DEL, want_info=True)
    for k in KEYS:
        assert (d[k].cpu().numpy() == many[k]).all(), k
    assert ctx.last_launch()[0] == "ibs::k_marginal_points"


def test_scan_driver_refined_margin_on_ncsx_tables(ctx):
    """BallooningScan.marginal(refine=True) on the G8 tables (2 surfaces, 8 x 5 coarse grid, N = 969), the device-resident branch and
    the tables-on-host branch: they agree (scale 1e-8 relative, location 1e-4); in each scale <= coarse_scale and scale is within 4 u of
    mo.solve at the returned point; refine=False is bitwise what marginal() returns, and index / table stay the coarse ones"""
    import time
    import torch
    import ibs_amd
    N = 969
    th = np.linspace(-4 * np.pi, 4 * np.pi, N)
    tabs = g8_tables()
    kw = dict(nalpha=8, ntheta0=5)
    dev_scan = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs, device=torch.device("cuda:0"), **kw)
    host_scan = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs, **kw)
    out = {}
    for name, scan in (("device", dev_scan), ("host", host_scan)):
        coarse = scan.marginal()
        again = scan.marginal(refine=False)
        assert set(coarse) == set(again) == {"scale", "alpha", "theta0", "index", "table"}
        for key in coarse:
            assert np.array_equal(coarse[key], again[key]), (name, key)
        t = time.perf_counter()
        res = out[name] = scan.marginal(refine=True)
        ms = (time.perf_counter() - t) * 1e3
        assert np.array_equal(res["index"], coarse["index"]) and np.array_equal(res["table"], coarse["table"])
        assert np.array_equal(res["coarse_scale"], coarse["scale"])
        assert np.array_equal(res["start"], np.stack([coarse["alpha"], coarse["theta0"]], axis=1))
        for k, s in enumerate(SVALS):
            ln = host_scan.fieldlines(s, np.array([res["alpha"][k]]))[0]
            q = mo.solve(host_scan.h, *mo.line_gc(bo.dPdrho_of(ln[2], ln[7], ln[0]), *ln[:7], res["theta0"][k]))
            assert res["scale"][k] <= res["coarse_scale"][k], (name, k, res["scale"][k], res["coarse_scale"][k])
            assert abs(res["scale"][k] - q["scale"]) <= 4 * q["u"], (name, k, res["scale"][k], q["scale"], q["u"])
            assert abs(res["dPdrho"][k] - bo.dPdrho_of(ln[2], ln[7], ln[0])) <= 1e-12 * abs(res["dPdrho"][k])
        report("G8 N=969 marginal(refine=True), %s branch: s* %s (coarse %s) at alpha %s theta0 %s; evals %s tasks %s rounds %d; %.1f ms "
               "with the coarse scan" % (name, res["scale"], res["coarse_scale"], res["alpha"], res["theta0"], res["evals"], res["task"],
                                         res["rounds"], ms))
    d, hst = out["device"], out["host"]
    assert (np.abs(d["scale"] - hst["scale"]) <= 1e-8 * np.abs(hst["scale"])).all(), (d["scale"], hst["scale"])
    assert np.abs(d["alpha"] - hst["alpha"]).max() < 1e-4 and np.abs(d["theta0"] - hst["theta0"]).max() < 1e-4


def test_adjoint_step_marginal(ctx):
    """AdjointStep.marginal on the three equilibria of tests/test_gpu_exact_refine.py's AdjointStep test (base, scaled pressure, a
    perturbed boundary mode), N = 969: every equilibrium's rows equal a separate BallooningScan.marginal(refine=True) on that
    equilibrium's tables BITWISE, and dscale follows from those rows.  Bitwise is the one that holds, and it needs the same table
    values on both sides: the tables are that equilibrium's rows of the step's table set (SurfaceTables.from_wouts = frame() + fill(),
    checked here to be what AdjointStep holds), and the rounds' geometry runs in one form whatever the batch (scan.MARGINAL_GEO_LPP).
    SurfaceTables.from_wout builds the same tables through other products (1e-15 relative apart, measured 4e-15), and a minimiser
    that stops on ftol 5e-11 / gtol 2e-8 carries such a difference into its end point: against from_wout's tables the rows agree
    to the bars of tests/test_gpu_exact_refine.py's AdjointStep test (1e-8 relative in scale, 1e-4 in location; measured 4e-12 in
    scale and 8e-9 in alpha), asserted here as well"""
    import torch
    import ibs_amd
    import bench
    dev = torch.device("cuda:0")
    wout0 = dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz")))
    scaled = dict(wout0)
    scaled["pres"] = np.asarray(wout0["pres"], dtype=np.float64) * 50.0
    wouts = [wout0, scaled, bench.emulated_equilibria(wout0)[0][1]]
    steps = np.array([1.0, 1e-3, 2e-3])
    th = ibs_amd.theta_grid_for(11, 11)
    assert len(th) == 969
    step = ibs_amd.AdjointStep(ctx, th, SVALS, dev, nalpha=8, ntheta0=5)
    out = step.marginal(wouts, steps)
    assert set(out) == {"scale", "alpha", "theta0", "dscale"} and set(step.marginal(wouts)) == {"scale", "alpha", "theta0"}
    kw = dict(nalpha=8, ntheta0=5, device=dev)
    step_tabs = ibs_amd.SurfaceTables.from_wouts(wouts, SVALS)        # the table set of the step: frame() + fill(), as AdjointStep builds it
    for name in ("tab_mn", "tab_nyq", "scal"):
        assert np.array_equal(getattr(step_tabs, name), getattr(step._frame, name)), name
    worst, worst_own = 0.0, np.zeros(3)
    for q, w in enumerate(wouts):
        m = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=step_tabs, surf_index=[2 * q, 2 * q + 1], **kw).marginal(refine=True)
        for key in ("scale", "alpha", "theta0"):
            worst = max(worst, float(np.abs(out[key][q] - m[key]).max()))
            assert np.array_equal(out[key][q], m[key]), (q, key, out[key][q], m[key])
        own = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=ibs_amd.SurfaceTables.from_wout(w, SVALS), **kw).marginal(refine=True)
        worst_own = np.maximum(worst_own, [np.abs(out[key][q] / own[key] - 1).max() if key == "scale" else np.abs(out[key][q] - own[key]).max()
                                           for key in ("scale", "alpha", "theta0")])
    report("AdjointStep.marginal, 3 equilibria x 2 surfaces: max |row - BallooningScan.marginal row on the step's tables| %.1e (bitwise); "
           "against from_wout's tables: scale %.1e relative, alpha %.1e, theta0 %.1e; scale %s" % ((worst,) + tuple(worst_own) + (out["scale"].ravel(),)))
    assert worst_own[0] <= 1e-8 and worst_own[1] < 1e-4 and worst_own[2] < 1e-4, worst_own
    assert np.array_equal(out["dscale"], (out["scale"][1:] - out["scale"][0]) / steps[1:, None])


def test_option_default_yields_to_the_callers_override(ctx):
    """Context.option_default, which pins the form of the rounds' geometry step: the option holds inside the block and is back at the
    context's default after it; an override the caller set through set_option stands inside the block and after it.  The form is read
    off the geometry kernel's name (6 lines of 969 points: eight lanes per point by batch size)"""
    import torch
    tabs, th = g8_tables(), np.linspace(-4 * np.pi, 4 * np.pi, 969)

    def form():
        ctx.fieldline_geometry(tabs, np.zeros(6, dtype=np.int32), np.linspace(0.0, 1.0, 6), th, device=torch.device("cuda:0"))
        return ctx.last_launch()[0]
    try:
        assert form() == "ibs::k_geo_rows<1, 8, 12>"
        with ctx.option_default("geo_lpp", 1):
            assert form() == "ibs::k_geo_rows<1, 1, 12>"
        assert form() == "ibs::k_geo_rows<1, 8, 12>"
        ctx.set_option("geo_lpp", 2)
        with ctx.option_default("geo_lpp", 1):
            assert form() == "ibs::k_geo_rows<1, 2, 12>"
        assert form() == "ibs::k_geo_rows<1, 2, 12>"
        ctx.set_option("geo_lpp", None)
        assert form() == "ibs::k_geo_rows<1, 8, 12>"
    finally:
        ctx.set_option("geo_lpp", None)
