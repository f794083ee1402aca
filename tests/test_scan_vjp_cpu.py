"""CPU: the host side of the fused scan VJP (ibs_gamma_scan_vjp_f64, Context.gamma_scan_vjp, objective.smooth_max) -- the argument
rule of the entry point without a GPU, the one-point pullback of csrc/ibs_scan_pullback.hpp compiled for the host against the
analytic Jacobian-transpose of a numpy restatement of the fold, smooth_max on CPU tensors, the marshalling of Context.gamma_scan_vjp
against tests/golden/B3_scan_vjp_calls_host.json (transcripts of the recorder's stand-in library: tests/tools/binding_recorder.py),
and that the two kernels compile for gfx950 without scratch."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ibs_amd
from ibs_amd import _lib
from tests.test_cabi import header_prototypes
from tests.tools import binding_recorder as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "B3_scan_vjp_calls_host.json")
IBS_ERR_ARG, IBS_ERR_UNSUPPORTED = -1, -3
NAME = "ibs_gamma_scan_vjp_f64"
P, D, I32, I64 = C.c_void_p, C.c_double, C.c_int32, C.c_int64


def test_entry_point_row_and_argument_rule():
    """the row of _lib.SYMBOLS against the header; then, through ctypes on a zeroed buffer standing for the context (the checks come
    before the context is touched): a null context, a null required array, all three bars null or ld < N -> IBS_ERR_ARG;
    N in {512, 65, 65539} -> IBS_ERR_UNSUPPORTED"""
    row = [P, I32, I32, I32, D, *([P] * 7), I64, P, P, P, P, P, P, P, P, P, P, I32]
    assert _lib.SYMBOLS[NAME] == (C.c_int, row)
    protos = header_prototypes()
    assert NAME in protos and len(protos[NAME][1]) == len(row)
    txt = open(os.path.join(ROOT, "include", "ibs.h")).read()
    assert "Nothing upstream corresponds" in txt[txt.index("Exact vector-Jacobian product of the whole table"):txt.index("int " + NAME)]
    lib = _lib.lib()
    buf = C.create_string_buffer(1 << 16)
    p = C.cast(buf, C.c_void_p)
    N = 513

    def call(ctx=p, n=N, ld=None, geo=None, dP=p, t0=p, sigma=None, gbar=p, bars=(p, p, p)):
        geo = [p] * 7 if geo is None else geo
        return lib.ibs_gamma_scan_vjp_f64(ctx, 1, 1, n, 0.05, *geo, n if ld is None else ld, dP, t0, sigma, gbar, *bars, None, None, None, 0)

    assert call(ctx=None) == IBS_ERR_ARG and b"null" in lib.ibs_last_error()
    for k in range(7):
        assert call(geo=[None if i == k else p for i in range(7)]) == IBS_ERR_ARG and b"null" in lib.ibs_last_error(), k
    for kw in (dict(dP=None), dict(t0=None), dict(gbar=None), dict(bars=(None, None, None))):
        assert call(**kw) == IBS_ERR_ARG and b"null" in lib.ibs_last_error(), kw
    assert call(ld=N - 1) == IBS_ERR_ARG
    for n in (512, 65, 65539):
        assert call(n=n) == IBS_ERR_UNSUPPORTED, n
        assert call(n=n, bars=(None, None, p)) == IBS_ERR_UNSUPPORTED, n


# ---- csrc/ibs_scan_pullback.hpp on the host
PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "ibs_scan_pullback.hpp"

// in: n records of 12 doubles (g_bar c_bar f_bar | the seven values | mdP | theta0); out: n records of 2 x 8 doubles (the seven bars |
// dP_bar): one call on zeros, then two calls ADDED to a start of (1, 2, ..., 8), less that start and halved -- the += is checked too
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) return 2;
  std::vector<double> in;
  double rec[12];
  while (std::fread(rec, sizeof(double), 12, fp) == 12) in.insert(in.end(), rec, rec + 12);
  std::fclose(fp);
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  for (size_t p = 0; p < in.size() / 12; ++p) {
    const double* r = &in[12 * p];
    double once[8] = {0, 0, 0, 0, 0, 0, 0, 0}, twice[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    ibs::scan_pullback_point(r[0], r[1], r[2], r + 3, r[10], r[11], once, once[7]);
    ibs::scan_pullback_point(r[0], r[1], r[2], r + 3, r[10], r[11], twice, twice[7]);
    ibs::scan_pullback_point(r[0], r[1], r[2], r + 3, r[10], r[11], twice, twice[7]);
    double res[16];
    for (int k = 0; k < 8; ++k) { res[k] = once[k]; res[8 + k] = 0.5 * (twice[k] - (k + 1)); }
    std::fwrite(res, sizeof(double), 16, out);
  }
  std::fclose(out);
  return 0;
}
"""


def fold_numpy(v, dP, th0):
    """(g, c, f) of one grid point: ball_scan.py:267-268 and utils.py:1560-1562 as the reference writes them"""
    bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22 = v
    cv = cvdrift + th0 * cvdrift0
    gd = gds2 + 2 * th0 * gds21 + th0 ** 2 * gds22
    gp = np.abs(gradpar)
    return gp * gd / bmag, -1 * dP * cv * 1 / (gp * bmag), gd / bmag ** 2 * 1 / (gp * bmag)


def jacobian_numpy(v, dP, th0):
    """d (g, c, f) / d (the seven values, dPdrho) of fold_numpy, (3, 8), differentiated by hand from the closed forms g = |gradpar| gd /
    bmag, c = -dP cv / (|gradpar| bmag), f = gd / (|gradpar| bmag^3) -- logarithmic derivatives, not the kernel's chain of temporaries"""
    bmag, gradpar = v[0], v[1]
    g, c, f = fold_numpy(v, dP, th0)
    gp, sg = np.abs(gradpar), np.sign(gradpar)
    J = np.zeros((3, 8))
    J[0, 0], J[1, 0], J[2, 0] = -g / bmag, -c / bmag, -3 * f / bmag
    J[0, 1], J[1, 1], J[2, 1] = sg * g / gp, -sg * c / gp, -sg * f / gp
    J[1, 2] = -dP / (gp * bmag); J[1, 3] = th0 * J[1, 2]
    for k, w in ((4, 1.0), (5, 2 * th0), (6, th0 ** 2)):
        J[0, k] = w * gp / bmag
        J[2, k] = w / (gp * bmag ** 3)
    J[1, 7] = -(v[2] + th0 * v[3]) / (gp * bmag)
    return J


def pullback_points():
    rng = np.random.default_rng(2718)
    n = 256
    bars = rng.standard_normal((n, 3))
    v = np.empty((n, 7))
    v[:, 0] = rng.uniform(0.5, 2.0, n)                                   # bmag
    v[:, 1] = rng.uniform(0.3, 1.5, n) * np.where(np.arange(n) % 3 == 1, -1.0, 1.0)     # gradpar, a third of them negative
    v[:, 2:4] = rng.standard_normal((n, 2))                              # cvdrift, cvdrift0
    v[:, 4] = rng.uniform(0.5, 3.0, n); v[:, 5] = rng.standard_normal(n); v[:, 6] = rng.uniform(0.5, 2.0, n)
    dP = -rng.uniform(0.2, 3.0, n)
    th0 = rng.uniform(-1.5, 1.5, n)
    th0[::5] = 0.0                                                      # theta0 = 0: the theta0 planes receive exactly 0
    th0[1::16] = 0.5                                                    # dyadic
    return bars, v, dP, th0


def test_pullback_header_on_the_host(tmp_path):
    """ibs::scan_pullback_point, compiled by the host compiler alone (no HIP types in the header), on 256 random points -- gradpar < 0
    on a third of them, theta0 = 0 on a fifth -- against J^T (g_bar, c_bar, f_bar), J the hand-derived Jacobian of the numpy fold.
    The pullback is a handful of multiplies and at most four added terms per component: every component is held to 1e-14 of the
    sum of the magnitudes of its terms, sum_i |J_ik| |bar_i| (= |component| wherever its terms share a sign: the error of any
    floating-point sum scales with the terms, not with what is left of them after cancellation; measured: 4.1e-16 of that sum at
    worst, and 2e-14 of |component| alone on the one of the 2,048 components whose terms cancel most).  J itself is checked against
    central differences of the fold first.  The results are ADDED: two calls on a non-zero start give twice one call."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    bars, v, dP, th0 = pullback_points()
    n = len(bars)
    # the reference's own check: central differences of the fold, step 1e-6, 1e-8 of the largest entry of J's column
    for p in range(0, n, 17):
        J = jacobian_numpy(v[p], dP[p], th0[p])
        for k in range(8):
            x = np.r_[v[p], dP[p]]
            e = np.zeros(8); e[k] = 1e-6 * max(1.0, abs(x[k]))
            fd = (np.array(fold_numpy((x + e)[:7], (x + e)[7], th0[p])) - np.array(fold_numpy((x - e)[:7], (x - e)[7], th0[p]))) / (2 * e[k])
            assert np.abs(fd - J[:, k]).max() <= 1e-8 * max(np.abs(J[:, k]).max(), 1.0), (p, k, fd, J[:, k])
    src, exe, fin, fout = (str(tmp_path / s) for s in ("pullback.cpp", "pullback", "in.bin", "out.bin"))
    with open(src, "w") as fh:
        fh.write(PROGRAM)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, src, "-o", exe], check=True)
    np.concatenate([bars, v, -dP[:, None], th0[:, None]], axis=1).astype(np.float64).tofile(fin)
    subprocess.run([exe, fin, fout], check=True)
    got = np.fromfile(fout, dtype=np.float64).reshape(n, 16)
    once, twice = got[:, :8], got[:, 8:]
    worst = 0.0
    for p in range(n):
        J = jacobian_numpy(v[p], dP[p], th0[p])
        ref = J.T @ bars[p]
        scale = np.abs(J).T @ np.abs(bars[p])
        err = np.abs(once[p] - ref)
        assert (err <= 1e-14 * scale).all(), (p, once[p], ref, err / np.maximum(scale, 1e-300))
        worst = max(worst, (err / np.maximum(scale, 1e-300)).max())
        assert (np.abs(twice[p] - ref) <= 1e-14 * scale + 8 * 2.3e-16).all(), (p, twice[p], ref)      # (the start values 1 .. 8 round once)
        if th0[p] == 0.0:
            assert once[p, 3] == 0.0 and once[p, 5] == 0.0 and once[p, 6] == 0.0, (p, once[p])
    neg = v[:, 1] < 0
    assert neg.sum() > 50 and (th0 == 0.0).sum() > 40
    assert worst > 0.0          # (the two evaluations are different programs: they do not agree to the last bit everywhere)


# ---- objective.smooth_max
def test_smooth_max_bounds_and_gradcheck():
    """max - log(n) / beta <= value <= max over the last two axes, on numpy arrays and CPU tensors alike (the same numbers), and
    torch.autograd.gradcheck; beta <= 0 is refused"""
    import torch
    from ibs_amd.objective import smooth_max
    rng = np.random.default_rng(5)
    gam = rng.standard_normal((4, 3, 5)) * 0.3
    gam[1] = 0.125                                            # a flat table: the value is the maximum itself
    for beta in (0.5, 20.0, 400.0):
        val = smooth_max(gam, beta)
        top = gam.reshape(4, -1).max(1)
        assert val.shape == (4,)
        assert (val <= top + 1e-15).all() and (val >= top - np.log(15) / beta - 1e-15).all(), (beta, val, top)
        assert abs(val[1] - 0.125) <= 1e-15
        tv = smooth_max(torch.from_numpy(gam), beta)
        assert isinstance(tv, torch.Tensor) and np.abs(tv.numpy() - val).max() <= 1e-14
    assert smooth_max(gam[0], 20.0).shape == ()
    t = torch.from_numpy(gam[:2]).clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a: smooth_max(a, 20.0), (t,))
    for beta in (0.0, -1.0, float("nan")):
        with pytest.raises(ibs_amd.IbsError):
            smooth_max(gam, beta)


# ---- the binding of Context.gamma_scan_vjp
def scan_vjp_cases(d, device=None):
    """[(case name, method, args, kwargs)]; device: the torch.device of d, or None for the host cases"""
    h = 0.09
    scan = (*d["scan7"], d["dP"], d["t0_scan"])
    gbar = d["gam_scan"]
    m = "gamma_scan_vjp"
    out = []
    for tag, kw in br._subsets(("want_info",)):
        out.append(("%s/%s" % (m, tag), m, (h, *scan, gbar), kw))
    out.append((m + "/sigma-array-info", m, (h, *scan, gbar), dict(sigma=d["sig_scan"], want_info=True)))
    out.append((m + "/sigma-scalar", m, (h, *scan, gbar), dict(sigma=0.37)))
    for want in (("geo",), ("dPdrho",), ("theta0",), ("geo", "theta0"), ["theta0", "dPdrho"]):
        out.append(("%s/want-%s" % (m, "+".join(want)), m, (h, *scan, gbar), dict(want=want)))
    out.append((m + "/error-want-empty", m, (h, *scan, gbar), dict(want=())))
    out.append((m + "/error-want-name", m, (h, *scan, gbar), dict(want=("geo", "alpha"))))
    out.append((m + "/error-want-str", m, (h, *scan, gbar), dict(want="geo")))
    out.append((m + "/error-shape-1d", m, (h, *[a[0] for a in d["scan7"]], d["dP"], d["t0_scan"], gbar), {}))
    out.append((m + "/error-shape-geo", m, (h, d["scan7"][0], d["scan7"][1][:1], *d["scan7"][2:], d["dP"], d["t0_scan"], gbar), {}))
    out.append((m + "/error-shape-dP", m, (h, *d["scan7"], d["dP"][:1], d["t0_scan"], gbar), {}))
    out.append((m + "/error-shape-theta0", m, (h, *d["scan7"], d["dP"], d["sig_scan"], gbar), {}))
    out.append((m + "/error-shape-gam_bar", m, (h, *scan, gbar[:, :2]), {}))
    if device is not None:
        host = d["np"]
        out.append(("mixed/gam_bar", m, (h, *scan, host["gam_scan"]), {}))
        out.append(("mixed/dPdrho", m, (h, *d["scan7"], host["dP"], d["t0_scan"], gbar), {}))
    return out


def record(device=None):
    with br.stand_in(device is not None) as fake:
        ctx = ibs_amd.Context(0)
        d = br.make_data(device)
        out = {name: br.run_case(ctx, fake, method, args, kw) for name, method, args, kw in scan_vjp_cases(d, device)}
        ctx.close()
    return out


@pytest.fixture(scope="module")
def recorded():
    return record()


def test_transcripts_match_the_golden(recorded):
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    assert sorted(recorded) == sorted(golden) and len(golden) >= 17
    bad = [k for k in sorted(golden) if recorded[k] != golden[k]]
    assert not bad, "\n".join("%s:\n  now    %s\n  golden %s" % (k, recorded[k], golden[k]) for k in bad[:5])


def test_what_the_transcripts_say(recorded):
    """independent of the golden file: one compute call in prototype order, the outputs' shapes, nbad passed through, the entries
    not wanted null in the call and None in the result"""
    r = recorded["gamma_scan_vjp/sigma-array-info"]
    (sym, a), = r["calls"]
    assert sym == NAME
    assert a == ["handle", "i:2", "i:3", "i:67", "f:0.09", *["in:%s" % k for k in br.GEO7], "i:67", "in:dPdrho", "in:theta0", "in:sigma",
                 "in:gam_bar", "out:geo_bar:(7, 2, 67):float64", "out:dPdrho_bar:(2,):float64", "out:theta0_bar:(2, 3):float64",
                 "out:gam:(2, 3):float64", "out:lam:(2, 3):float64", "out:info:(2, 3):int32", "i:1"]
    assert r["result"]["nbad"] == br.NBAD
    (sym, a), = recorded["gamma_scan_vjp/plain"]["calls"]
    assert a[15] == "null" and a[-2] == "null"
    (sym, a), = recorded["gamma_scan_vjp/sigma-scalar"]["calls"]
    assert a[15] == "bcast:sigma:6"
    (sym, a), = recorded["gamma_scan_vjp/want-theta0"]["calls"]
    assert a[17:20] == ["null", "null", "out:theta0_bar:(2, 3):float64"]
    res = recorded["gamma_scan_vjp/want-theta0"]["result"]
    assert res["geo_bar"] is None and res["dPdrho_bar"] is None and res["theta0_bar"].startswith("numpy:(2, 3)")
    (sym, a), = recorded["gamma_scan_vjp/want-dPdrho"]["calls"]
    assert a[17:20] == ["null", "out:dPdrho_bar:(2,):float64", "null"]
    assert recorded["gamma_scan_vjp/want-theta0+dPdrho"]["calls"][0][1][17:20] == ["null", "out:dPdrho_bar:(2,):float64",
                                                                                   "out:theta0_bar:(2, 3):float64"]
    assert not [k for k, v in recorded.items() if any(c[0] == "ibs_set_stream" for c in v["calls"])]


def test_errors_reach_no_compute_call(recorded):
    errs = [k for k, v in recorded.items() if br.is_error(v["result"])]
    assert sorted(errs) == sorted(k for k in recorded if "/error-" in k) and len(errs) == 8
    assert not [k for k in errs if recorded[k]["calls"]]
    for k in errs:
        assert recorded[k]["result"].startswith("IbsError: gamma_scan_vjp: "), recorded[k]


# ---- the kernels
def test_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """csrc/ibs_scan_vjp.hip: k_scan_vjp_points<true>, <false> and k_scan_vjp_reduce compile for gfx950 with ScratchSize 0, and the
    points kernel keeps the long path's LDS (eight blocks per CU)"""
    hipcc = shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-DIBS_WITH_F32", "-Wno-unused-value",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "ibs_scan_vjp.hip"), "-o",
                        str(tmp_path / "scan_vjp.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    res = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for key in ("ScratchSize [bytes/lane]", "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                res.setdefault(name, {})[key] = int(m.group(1))
    pts = [k for k in res if "k_scan_vjp_points" in k]
    red = [k for k in res if "k_scan_vjp_reduce" in k]
    assert len(pts) == 2 and len(red) == 1, sorted(res)
    for k in pts + red:
        assert res[k]["ScratchSize [bytes/lane]"] == 0, (k, res[k])
    for k in pts:
        assert res[k]["LDS Size [bytes/block]"] * 8 <= 160 * 1024, (k, res[k])
