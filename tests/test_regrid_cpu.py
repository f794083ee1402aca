"""CPU: the regrid of utils.py:1565-1576 as csrc/ibs_regrid.hpp states it, against numpy; the new entry points' exports and argument
checks; the regrid kernels' resources.

A stand-alone C++ program (host compiler only, no GPU, no sanitizer) runs the header over the five grids of tests/regrid_cases.py x
N in {67, 131, 257, 2051} and s-alpha rows g, c, f (shat = 0.8, alpha = 1.2, theta0 = 0, 0.7, 1.5):
  nodes, half nodes and h are bit for bit np.linspace, (tu[:-1] + tu[1:]) / 2 and np.diff(...)[2];
  every interval index is np.interp's and lies in [0, N - 2] -- in that range also for rows with a NaN, a decreasing pair and equal
  neighbours, which regrid_row_ok refuses;
  every interpolated value is within 4 eps (|fp_k| + |fp_{k+1}|) of np.interp.  The bound is derived: the value is one difference, one
  quotient, one product and one sum, each rounded once, and |slope dx| <= |fp_k| + |fp_{k+1}|.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ibs_amd
from ibs_amd import _lib
from tests import regrid_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")
LIB = os.path.join(ROOT, "ideal-ballooning-solver_amd", "lib", "libibs_hip.so")
NAMES = ["ibs_regrid_rows_f64", "ibs_assemble_gcf_theta_f64", "ibs_gamma_scan_theta_f64", "ibs_gamma_points_theta_f64"]
NS = (67, 131, 257, 2051)
ERR_ARG, ERR_UNSUPPORTED = -1, -3

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "ibs_regrid.hpp"

// in:  n_cases, then per case N, lo, hi, theta[N], g[N], c[N], f[N]
// out: per case ok, h, nodes[N], half[N-1], k[N], kh[N-1], g_u[N], gh[N-1], c_u[N], f_u[N]
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::FILE* fi = std::fopen(argv[1], "rb");
  std::FILE* fo = std::fopen(argv[2], "wb");
  if (!fi || !fo) return 2;
  double head;
  if (std::fread(&head, sizeof(double), 1, fi) != 1) return 2;
  for (int cs = 0; cs < (int)head; ++cs) {
    double p[3];
    if (std::fread(p, sizeof(double), 3, fi) != 3) return 2;
    const int N = (int)p[0];
    const double lo = p[1], hi = p[2];
    std::vector<double> in((size_t)4 * N);
    if (std::fread(in.data(), sizeof(double), in.size(), fi) != in.size()) return 2;
    const double *th = in.data(), *g = th + N, *c = g + N, *f = c + N;
    const double step = ibs::regrid_step(lo, hi, N);
    std::vector<double> out;
    out.push_back(ibs::regrid_row_ok(th, N, lo, hi) ? 1.0 : 0.0);
    out.push_back(ibs::regrid_spacing(N, lo, hi));
    std::vector<int> k(N), kh(N - 1);
    for (int j = 0; j < N; ++j) out.push_back(ibs::regrid_node(j, N, lo, hi, step));
    for (int j = 0; j < N - 1; ++j) out.push_back(ibs::regrid_half_node(j, N, lo, hi, step));
    for (int j = 0; j < N; ++j) { k[j] = ibs::regrid_interval(th, N, ibs::regrid_node(j, N, lo, hi, step)); out.push_back(k[j]); }
    for (int j = 0; j < N - 1; ++j) { kh[j] = ibs::regrid_interval(th, N, ibs::regrid_half_node(j, N, lo, hi, step)); out.push_back(kh[j]); }
    auto at = [&](const double* fp, int kk, double x) { return ibs::regrid_value(x, th[kk], th[kk + 1], fp[kk], fp[kk + 1]); };
    for (int j = 0; j < N; ++j) out.push_back(at(g, k[j], ibs::regrid_node(j, N, lo, hi, step)));
    for (int j = 0; j < N - 1; ++j) out.push_back(at(g, kh[j], ibs::regrid_half_node(j, N, lo, hi, step)));
    for (int j = 0; j < N; ++j) out.push_back(at(c, k[j], ibs::regrid_node(j, N, lo, hi, step)));
    for (int j = 0; j < N; ++j) out.push_back(at(f, k[j], ibs::regrid_node(j, N, lo, hi, step)));
    if (std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) return 2;
  }
  std::fclose(fi);
  std::fclose(fo);
  return 0;
}
"""


def cases():
    """(label, valid, theta, lo, hi, g, c, f): the good grids, then broken copies of the random grid at N = 131"""
    out = []
    for N in NS:
        for kind in rc.KINDS:
            th = rc.grid(kind, N)
            for t0 in (0.0, 0.7, 1.5):
                out.append(("%s N=%d theta0=%g" % (kind, N, t0), True, th, th[0], th[-1], *rc.salpha_rows(th, theta0=t0)))
    th = rc.grid("random", 131)
    rows = rc.salpha_rows(th)
    for label, edit in (("nan", lambda t: t.__setitem__(40, np.nan)), ("inf", lambda t: t.__setitem__(40, np.inf)),
                        ("decreasing", lambda t: t.__setitem__(slice(60, 62), t[60:62][::-1].copy())),
                        ("equal", lambda t: t.__setitem__(90, t[89])), ("all nan", lambda t: t.__setitem__(slice(None), np.nan)),
                        ("reversed", lambda t: t.__setitem__(slice(None), t[::-1].copy()))):
        bad = th.copy()
        edit(bad)
        out.append((label, False, bad, th[0], th[-1], *rows))
    off = th.copy()
    off[-1] += 1e-9                      # still increasing, but the end point is off the window
    out.append(("end off the window", False, off, th[0], th[-1], *rows))
    return out


@pytest.fixture(scope="module")
def header_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("regrid")
    cs = cases()
    data, res = tmp / "in.bin", tmp / "out.bin"
    with open(data, "wb") as fp:
        np.array([float(len(cs))]).tofile(fp)
        for _, _, th, lo, hi, g, c, f in cs:
            np.array([float(len(th)), lo, hi]).tofile(fp)
            for a in (th, g, c, f):
                np.ascontiguousarray(a, dtype=np.float64).tofile(fp)
    src, exe = tmp / "regrid_check.cpp", tmp / "regrid_check"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, str(src), "-o", str(exe)])
    p = subprocess.run([str(exe), str(data), str(res)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    flat = np.fromfile(res)
    out, o = [], 0
    for _, _, th, *_ in cs:
        N = len(th)
        sizes = dict(ok=1, h=1, nodes=N, half=N - 1, k=N, kh=N - 1, g=N, gh=N - 1, c=N, f=N)
        d = {}
        for name, n in sizes.items():
            d[name] = flat[o:o + n]
            o += n
        out.append(d)
    assert o == len(flat)
    return cs, out


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def test_nodes_half_nodes_and_h_are_numpy_bit_for_bit(header_run):
    cs, out = header_run
    for (label, valid, th, lo, hi, *_), d in zip(cs, out):
        N = len(th)
        tu = np.linspace(lo, hi, N)
        half = (tu[:-1] + tu[1:]) / 2
        assert same_bits(d["nodes"], tu), label
        assert same_bits(d["half"], half), label
        assert same_bits(d["h"], [np.diff(half)[2]]), label


def test_interval_indices_stay_in_range_on_any_row(header_run):
    cs, out = header_run
    n_bad = 0
    for (label, valid, th, lo, hi, *_), d in zip(cs, out):
        N = len(th)
        for key in ("k", "kh"):
            k = d[key]
            assert np.all(k == np.round(k)) and k.min() >= 0 and k.max() <= N - 2, (label, key, k.min(), k.max())
        assert bool(d["ok"][0]) == valid, label
        n_bad += not valid
        if valid:
            tu = np.linspace(lo, hi, N)
            assert np.array_equal(d["k"], rc.interval(th, tu)), label
            assert np.array_equal(d["kh"], rc.interval(th, (tu[:-1] + tu[1:]) / 2)), label
    assert n_bad == 7


def test_values_are_np_interp_within_the_derived_bound(header_run):
    cs, out = header_run
    worst = 0.0
    for (label, valid, th, lo, hi, g, c, f), d in zip(cs, out):
        if not valid:
            continue
        h, tu, half, gu, gh, cu, fu = rc.regrid_numpy(th, g, c, f)
        for got, ref, fp, x in ((d["g"], gu, g, tu), (d["gh"], gh[:-1], g, half), (d["c"], cu, c, tu), (d["f"], fu, f, tu)):
            bound = rc.interp_bound(th, fp, x)
            err = np.abs(got - ref)
            assert np.all(err <= bound), (label, float((err / np.maximum(bound, 1e-300)).max()))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        if label.startswith("hits"):                                  # the x == xp[k] branch returns the sample itself
            assert same_bits(d["g"][::2], g[::2]), label
    print("largest error over the bound: %.3f" % worst)


# ---- plumbing ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("nm") is None, reason="needs nm")
def test_library_exports_the_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    with open(os.path.join(ROOT, "include", "ibs.h")) as fh:
        header = fh.read()
    for name in NAMES:
        assert name in names and name in _lib.SYMBOLS and "int %s(" % name in header, name


def test_python_interface_exists():
    for m in ("regrid_rows", "assemble_gcf_theta", "gamma_scan_theta", "gamma_points_theta"):
        assert callable(getattr(ibs_amd.Context, m, None)), m
    assert callable(getattr(ibs_amd, "gamma_ball_full_many", None))


def _entry(name):
    """call(ctx=..., N=..., ld=..., theta_ld=..., lo=..., hi=..., null=()) of one entry point on small host arrays"""
    lib = _lib.lib()
    fn = getattr(lib, name)
    n, nt0 = 2, 3

    def call(ctx, N=67, ld=None, theta_ld=0, lo=-1.0, hi=1.0, null=()):
        ld = N if ld is None else ld
        a = {k: np.ones((n, max(N, 2))) for k in ("g", "c", "f", "b", "gp", "cv", "cv0", "g2", "g21", "g22")}
        a.update(th=np.linspace(lo if np.isfinite(lo) else -1.0, hi if np.isfinite(hi) else 1.0, max(N, 2)), dP=np.ones(n), t0=np.zeros(nt0),
                 o1=np.zeros((n * nt0, max(N, 2))), o2=np.zeros((n * nt0, max(N, 2))), o3=np.zeros((n * nt0, max(N, 2))),
                 o4=np.zeros((n * nt0, max(N, 2))), gam=np.zeros(n * nt0))
        p = lambda k: None if k in null else C.c_void_p(a[k].ctypes.data)
        geo = [p(k) for k in ("b", "gp", "cv", "cv0", "g2", "g21", "g22")]
        head = [p("th"), theta_ld, lo, hi]
        if name == "ibs_regrid_rows_f64":
            return fn(ctx, n, N, *head, p("g"), p("c"), p("f"), ld, p("o1"), p("o2"), p("o3"), p("o4"), ld, None, None, _lib.MEM_HOST)
        if name == "ibs_assemble_gcf_theta_f64":
            return fn(ctx, n, nt0, N, *head, *geo, ld, p("dP"), p("t0"), 0, p("o1"), p("o2"), p("o3"), p("o4"), None, None, _lib.MEM_HOST)
        if name == "ibs_gamma_scan_theta_f64":
            return fn(ctx, n, nt0, N, *head, *geo, ld, p("dP"), p("t0"), p("gam"), None, None, None, None, _lib.MEM_HOST)
        return fn(ctx, n, N, *head, *geo, ld, p("dP"), p("t0"), p("gam"), None, None, None, None, _lib.MEM_HOST)
    return lib, call


REQUIRED = {"ibs_regrid_rows_f64": ("th", "g", "o1", "o2"),
            "ibs_assemble_gcf_theta_f64": ("th", "b", "gp", "cv", "cv0", "g2", "g21", "g22", "dP", "t0", "o1", "o2", "o3", "o4"),
            "ibs_gamma_scan_theta_f64": ("th", "b", "gp", "cv", "cv0", "g2", "g21", "g22", "dP", "t0"),
            "ibs_gamma_points_theta_f64": ("th", "b", "gp", "cv", "cv0", "g2", "g21", "g22", "dP", "t0")}


@pytest.mark.parametrize("name", NAMES)
def test_argument_errors_need_no_gpu(name):
    """every argument check comes before the context is touched: a placeholder block of memory stands in for it"""
    lib, call = _entry(name)
    fake = C.create_string_buffer(1 << 16)
    assert call(None) == ERR_ARG and b"null context" in lib.ibs_last_error()
    for k in REQUIRED[name]:
        assert call(fake, null=(k,)) == ERR_ARG, k
    assert call(fake, ld=66) == ERR_ARG
    for theta_ld in (66, 1, -67):                                  # neither 0 nor >= N
        assert call(fake, theta_ld=theta_ld) == ERR_ARG and b"theta_ld" in lib.ibs_last_error(), theta_ld
    for lo, hi in ((np.nan, 1.0), (-1.0, np.inf), (-np.inf, 1.0), (1.0, 1.0), (2.0, 1.0)):
        assert call(fake, lo=lo, hi=hi) == ERR_ARG and b"window" in lib.ibs_last_error(), (lo, hi)
    for bad_N in (512, 68, 65, 65539):                             # even, even, below 66, above 65,537
        assert call(fake, N=bad_N) == ERR_UNSUPPORTED, bad_N
    if name == "ibs_regrid_rows_f64":                              # c / c_u and f / f_u come in pairs
        assert call(fake, null=("c",)) == ERR_ARG and call(fake, null=("o4",)) == ERR_ARG
        assert b"pairs" in lib.ibs_last_error()


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_regrid_kernels_have_no_scratch():
    """k_regrid_rows<LDS> and k_assemble_regrid<LDS> (csrc/ibs_regrid.hip): four kernels, ScratchSize 0 for gfx950"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "ibs_regrid.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    name, scratch = None, {}
    for line in r.stderr.split("\n"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    kern = {k: v for k, v in scratch.items() if "k_regrid_rows" in k or "k_assemble_regrid" in k}
    assert len(kern) == 4 and all(v == 0 for v in kern.values()), scratch
