"""CPU: the restatement the GPU tests of the certificate compare against (tests/certify_oracle.py) -- the mapping of raw systems onto
geometry arrays, ||A||, the tolerance and the cert rule on the near-degenerate fixtures --, the argument checks of the new entry points
(which come before any device use), the driver options, and the kernels' resource use."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ibs_amd
from ibs_amd import _lib
from oracle import ballooning_oracle as bo
from oracle import c_oracle as co
from tests import certify_oracle as cz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")
G = os.path.join(os.path.dirname(__file__), "golden")
IBS_ERR_ARG, IBS_ERR_UNSUPPORTED = -1, -3
NEW = ("ibs_geo_sturm_count_f64", "ibs_gamma_scan_certify_f64", "ibs_gamma_points_certify_f64", "ibs_gamma_scan_reclose_f64",
       "ibs_gamma_points_reclose_f64")


def _ulp_err(a, b):
    return np.abs(a - b) / np.spacing(np.abs(b))


def test_mapping_reproduces_the_rows_to_4_ulp():
    """(g, c, f) -> geometry arrays -> host-folded rows at theta0 = 0: G10 and 64 systems of the rough family (iid per point inside
    the NCSX_op envelopes, BASELINE configs[4]), every entry within 4 ulp"""
    d = np.load(os.path.join(G, "G10_rough_pair_1025.npz"))
    rng = np.random.default_rng(5)
    N = 513
    gr = np.exp(rng.uniform(np.log(0.01), np.log(50.0), (64, N))); cr = rng.uniform(-2.5, 3.5, (64, N))
    fr = np.exp(rng.uniform(np.log(0.2), np.log(3e3), (64, N)))
    for g, c, f in ((d["g"][None], d["c"][None], d["f"][None]), (gr, cr, fr)):
        for planes in (0.0, 1e-3):
            geo7, dP = cz.gcf_to_geometry(g, c, f, th0_planes=planes)
            g2, c2, f2 = cz.fold_rows(geo7, dP, np.array([0.0]))
            assert max(_ulp_err(g2, g).max(), _ulp_err(c2, c).max(), _ulp_err(f2, f).max()) <= 4
            if planes:                        # the planes are there, and leave the rows positive at theta0 > 0
                g3, _, f3 = cz.fold_rows(geo7, dP, np.array([0.3]))
                assert (g3 > g2).all() and (f3 > 0).all()


def test_rule_on_mapped_g10():
    """the near-degenerate pair of G10 survives the mapping: lam_max moves by a few eps, the rule gives 0 at lam_max (0 above
    lam + tol, 1 above lam - tol) and bit 0 at the lam_2 that round 5 returned"""
    d = np.load(os.path.join(G, "G10_rough_pair_1025.npz"))
    N = 1025
    h = 8 * np.pi / (N - 1)
    geo7, dP = cz.gcf_to_geometry(d["g"], d["c"], d["f"])
    g, c, f = cz.fold_rows(geo7, dP, np.array([0.0]))
    lam_max = float(d["lam_max"])
    assert lam_max == 0.002708194851508614
    tol = cz.tolerance(h, g, c, f)[0]
    assert abs(co.lam_batch(h, g, c, f)[0] - lam_max) < 1e-3 * tol
    assert co.count_above_batch(h, g, c, f, np.array([lam_max + tol]))[0] == 0
    assert co.count_above_batch(h, g, c, f, np.array([lam_max - tol]))[0] == 1
    assert cz.cert_rule(h, g, c, f, np.array([lam_max]))[0] == 0
    assert cz.cert_rule(h, g, c, f, np.array([float(d["lam_returned_round5"])]))[0] == cz.NOT_MAX
    assert cz.cert_rule(h, g, c, f, np.array([lam_max + 10 * tol]))[0] == cz.NO_EIG
    assert cz.cert_rule(h, g, c, f, np.array([np.nan]))[0] == cz.UNCHECKED
    l2 = cz.second_eigenvalue(h, g[0], c[0], f[0], lam_max, tol)
    assert abs(l2 - float(d["lam_returned_round5"])) < tol


def test_salpha_pair_is_decidable():
    """shat = 2, alpha = 6, theta0 = 0, N = 513: the top two eigenvalues are a few 1e-9 ||A|| apart -- at least 2 tol, so that
    lam_2 + tol < lam_max - tol and a certificate tells them apart; and the geometry form of the line gives the same rows"""
    N = 513
    th = bo.theta_grid(N)
    h = th[1] - th[0]
    g, c = bo.salpha_gc(th, 2.0, 6.0, 0.0)
    l1, l2 = cz.dense_top_two(h, g, c, g)
    tol = cz.tolerance(h, g[None], c[None], g[None])[0]
    assert l1 - l2 >= 2 * tol, (l1, l2, tol)
    assert l1 - l2 < 1e-2, (l1, l2)                      # (near-degenerate on the scale of the spectrum)
    assert abs(co.lam_batch(h, g[None], c[None], g[None])[0] - l1) < tol
    assert cz.cert_rule(h, g[None], c[None], g[None], np.array([l2]))[0] == cz.NOT_MAX
    geo7, dP = cz.salpha_geometry(th, [2.0], [6.0])
    g2, c2, f2 = cz.fold_rows(geo7, dP, np.array([0.0]))
    assert np.abs(g2[0] - g).max() <= 4 * np.spacing(np.abs(g).max()) and np.abs(c2[0] - c).max() <= 4 * np.spacing(np.abs(c).max())
    assert np.array_equal(g2, f2)


def test_arguments_are_checked_before_any_device_work():
    """every new entry point: null context, a null required argument, ld < N: IBS_ERR_ARG; the N rule: IBS_ERR_UNSUPPORTED (the count
    accepts even N).  The checks come before the context is touched, so a zeroed buffer stands for it where no GPU is present."""
    lib = _lib.lib()
    names = re.findall(r"\b(ibs_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "ibs.h")).read())
    for n in NEW:
        assert n in names and n in _lib.SYMBOLS
    buf = C.create_string_buffer(1 << 16)
    p = C.cast(buf, C.c_void_p)
    geo = [p] * 7
    fns = {
        "count": lambda ctx, n, ld, a, b: lib.ibs_geo_sturm_count_f64(ctx, 1, 1, n, 0.05, *geo, ld, p, p, a, b, 0),
        "cscan": lambda ctx, n, ld, a, b: lib.ibs_gamma_scan_certify_f64(ctx, 1, 1, n, 0.05, *geo, ld, p, p, a, 0.0, b, 0),
        "cpts": lambda ctx, n, ld, a, b: lib.ibs_gamma_points_certify_f64(ctx, 1, n, 0.05, *geo, ld, p, p, a, 0.0, b, 0),
        "rscan": lambda ctx, n, ld, a, b: lib.ibs_gamma_scan_reclose_f64(ctx, 1, 1, n, 0.05, *geo, ld, p, p, 0.0, a, b, p, None, None, 0),
        "rpts": lambda ctx, n, ld, a, b: lib.ibs_gamma_points_reclose_f64(ctx, 1, n, 0.05, *geo, ld, p, p, 0.0, a, b, p, None, None, 0),
    }
    N = 513
    for key, fn in fns.items():
        assert fn(None, N, N, p, p) == IBS_ERR_ARG and b"null" in lib.ibs_last_error(), key
        assert fn(p, N, N, None, p) == IBS_ERR_ARG and b"null" in lib.ibs_last_error(), key
        assert fn(p, N, N, p, None) == IBS_ERR_ARG and b"null" in lib.ibs_last_error(), key
        assert fn(p, N, N - 1, p, p) == IBS_ERR_ARG, key
        for n in (65, 65538, 65539):
            assert fn(p, n, n, p, p) == IBS_ERR_UNSUPPORTED, (key, n)
        if key != "count":
            assert fn(p, 512, 512, p, p) == IBS_ERR_UNSUPPORTED, key
    assert lib.ibs_geo_sturm_count_f64(p, 1, 1, 513, 0.0, *geo, 513, p, p, p, p, 0) == IBS_ERR_ARG      # h
    assert lib.ibs_geo_sturm_count_f64(p, 1, 1, 513, 0.05, None, *geo[1:], 513, p, p, p, p, 0) == IBS_ERR_ARG


def test_driver_options():
    """certify=True with eigenpair="nearest" is refused; the flag defaults to False and leaves no trace on the objects"""
    th = bo.theta_grid(129)
    with pytest.raises(ValueError):
        ibs_amd.BallooningScan(None, lambda s, a: None, th, [0.5], eigenpair="nearest", certify=True)
    with pytest.raises(ValueError):
        ibs_amd.AdjointStep(None, th, [0.5], "cpu", eigenpair="nearest", certify=True)
    sc = ibs_amd.BallooningScan(None, lambda s, a: None, th, [0.5])
    assert sc.certify is False and sc.last_certificate is None and sc._certify_kw() == {}
    assert ibs_amd.BallooningScan(None, lambda s, a: None, th, [0.5], certify=True)._certify_kw() == dict(certify=True)
    for name in ("geo_sturm_count", "certify_scan", "certify_points", "reclose_scan", "reclose_points"):
        assert callable(getattr(ibs_amd.Context, name))
    assert callable(ibs_amd.BallooningScan.mode_count)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_certify_kernels_have_no_scratch():
    """the four forms of k_geo_certify and k_geo_reclose (csrc/ibs_certify.hip) compile for gfx950 with ScratchSize 0"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "ibs_certify.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    name, scratch = None, {}
    for line in r.stderr.split("\n"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    kern = {k: v for k, v in scratch.items() if "k_geo_" in k}
    assert len(kern) == 5 and all(v == 0 for v in kern.values()), scratch
