"""GPU: the one-wave theta0 scan with the diagonal scaling s carried from set-up (k_gamma_scan<double, M>) and with the half-grid
means formed by the one rule of csrc/ibs_half_grid.hpp (every form).

Shapes: grid lengths on the chunk and ownership edges of the resident form -- N = 131 (M = 3, one lane with a last row), 193
(M = 3, 63 lanes), 195 (M = 4, one lane), 449 (M = 7, 63 lanes), 451 (M = 8, one lane), 513 (M = 8, 63 lanes) -- on two lines x
four theta0 (two surfaces of one line each).  The geometry is the first two golden NCSX lines (tests/golden/G3_ncsx_lines.npz),
interpolated onto the shorter grids as in tests/test_gpu_scan_resident.py.

 (a) resident against lean (scan_resident 1 / 0): gam, lam, info, pack, X, dX, d gam / d theta0 carry the same bits.
 (b) against tests/golden/scan_parent_rows.npz -- gam, lam, info of exactly these scans, recorded on the GPU from the library of the
     commit before the rule was written down: lam and info are equal (set-up's arithmetic is what the compiler made of it then);
     gam moves at rounding level, because the eigenvector is now scaled with set-up's s instead of a second rounding of it.
 (c) gam and lam against the C oracle, within what tests/test_gpu_scan_resident.py holds this kernel to (check_scan).
 (d) GAM_BOUND: the largest |gam - recorded gam| measured on these shapes and on the 1,024 solves of the bench batch was
     MEASURED_DGAM (docs/EXPERIMENTS.md R6.18), times 8: one more row of rounding in each of the Simpson sums.
"""
import functools
import os

import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from oracle import c_oracle as co
from tests.test_gpu_edge_lengths import check_scan, scan_norm_a

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
SIZES = [131, 193, 195, 449, 451, 513]
N_LINES, N_SURF = 2, 2
THETA0 = np.array([0.0, 0.4, 0.8, 1.2])
MEASURED_DGAM = 7.43e-18
GAM_BOUND = 8.0 * MEASURED_DGAM


def rows_per_lane(N):
    return (N - 2 + 63) // 64


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.reset_options()
    c.close()


@functools.lru_cache(maxsize=None)
def inputs(N):
    """(h, the seven geometry arrays (N_LINES, N), dPdrho) of the golden lines on the N-point grid"""
    g3 = np.load(os.path.join(G, "G3_ncsx_lines.npz"))
    geo, th513, th = g3["geo_513"][:N_LINES], bo.theta_grid(513), bo.theta_grid(N)
    if N != 513:
        geo = np.stack([np.stack([np.interp(th, th513, ln[k]) for k in range(8)]) for ln in geo])
    a = tuple(np.ascontiguousarray(geo[:, k, :]) for k in range(7))
    assert (a[0] > 0).all() and (np.abs(a[1]) > 0).all()
    return float(th[1] - th[0]), a, np.ascontiguousarray(g3["dPdrho_513"][:N_LINES])


@functools.lru_cache(maxsize=None)
def reference(N):
    """the C oracle on the same systems, once per length: ref tuple of check_scan (no X, no theta0 derivative)"""
    h, a, dP = inputs(N)
    gam_c, lam_c, _ = co.gamma_scan(h, *a, dP, THETA0)
    return gam_c, lam_c, None, None, None, scan_norm_a(h, np.stack(a, axis=1), dP, THETA0)


@functools.lru_cache(maxsize=None)
def parent_rows():
    return np.load(os.path.join(G, "scan_parent_rows.npz"))


def scan_both(ctx, N):
    """the scan with every output, and the fused scan + argmax, under scan_resident = 1 and = 0: [resident, lean] as numpy dicts"""
    import torch
    import ibs_amd
    dev = torch.device("cuda:0")
    h, a, dP = inputs(N)
    geo = [torch.from_numpy(x).to(dev) for x in a]
    dP_d, t0 = torch.from_numpy(dP).to(dev), torch.from_numpy(THETA0).to(dev)
    M, out = rows_per_lane(N), []
    try:
        for res, name in ((1, "ibs::k_gamma_scan<double, %d>" % M), (0, "ibs::k_gamma_scan_lean<double, %d>" % M)):
            ctx.set_option("scan_resident", res)
            r = ctx.gamma_scan(h, *geo, dP_d, t0, want_X=True, want_dtheta0=True, want_info=True)
            assert ctx.last_launch()[0] == name, (N, res, ctx.last_launch())
            plan = ibs_amd.ScanPlan(ctx, h, geo, dP_d, t0, N_SURF)
            plan.scan_argmax()
            torch.cuda.synchronize()
            assert ctx.last_launch()[0] == name, (N, res, ctx.last_launch())
            d = {k: r[k].cpu().numpy() for k in ("gam", "lam", "info", "X", "dX", "dgam_dtheta0")}
            d.update(pack=plan.pack.cpu().numpy(), plan_gam=plan.gam.cpu().numpy(), plan_lam=plan.lam.cpu().numpy())
            out.append(d)
    finally:
        ctx.set_option("scan_resident", None)
    return out


@pytest.mark.parametrize("N", SIZES)
def test_scaling_carried_from_set_up(ctx, N):
    res, lean = scan_both(ctx, N)
    assert not ((res["info"] >> 16) & 3).any(), (N, res["info"] >> 16)
    # (a) the two forms
    for k in ("gam", "lam", "info", "pack", "X", "dX", "dgam_dtheta0", "plan_gam", "plan_lam"):
        assert res[k].shape == lean[k].shape and np.array_equal(res[k], lean[k]), (N, k, float(np.abs(res[k] - lean[k]).max()))
    assert np.array_equal(res["plan_gam"].reshape(res["gam"].shape), res["gam"])
    # (b) the recorded rows of the commit before
    rec = parent_rows()
    d_gam = float(np.abs(res["gam"] - rec["gam_%d" % N]).max())
    print("scan scaling figures: N=%d  max |gam - recorded gam| = %.2e  (bound %.2e)" % (N, d_gam, GAM_BOUND))
    assert np.array_equal(res["lam"], rec["lam_%d" % N]), (N, np.abs(res["lam"] - rec["lam_%d" % N]).max())
    assert np.array_equal(res["info"], rec["info_%d" % N]), N
    assert d_gam <= GAM_BOUND, (N, d_gam)
    # (c) the C oracle
    check_scan(N, "scaling carried", dict(gam=res["gam"], lam=res["lam"]), reference(N))
