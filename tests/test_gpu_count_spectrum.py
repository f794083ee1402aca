"""GPU: Sturm counts deep inside, below and above the spectrum, on rows given in other units (tests/edge_cases.py: count_batch; every
expected count confirmed by two CPU methods in tests/test_count_spectrum_cpu.py, where the sweep's lane arithmetic is restated).

The rest of the suite asks ibs_sturm_count_f64 only for counts at 0 and next to lam_max, on (g, c, f) of order 1 to 1e3.  The
prefix-product sweep k_sturm_count runs an un-normalised recurrence inside a lane; with one renormalisation per chunk its 32 rows per
lane at N = 2049 overflowed once (g, c) were 4096 times larger, and counts came back wrong without a status.  Here every form of
the count runs three families (s-alpha, the moving well, iid rows inside the configs[4] envelopes) at eleven shifts each -- the
midpoints of gaps at least 16 N^2 eps ||A|| wide below the 1st, 2nd, 3rd, 8th, 64th, (n/4)-th, (n/2)-th, (3n/4)-th and (n-1)-th
largest eigenvalue, one shift below the spectrum and one above it -- with (g, c) scaled by 2^-40 ... 2^40 and once f by 2^20.

Bounds: counts are exact, no allowance.  The raw solves are a guard on the same rows: lam within 4 N eps ||A|| of the C oracle on the
scaled rows, gam within 1e-8 2^(k - m) (the suite's bound carried by the exact factor the growth rate scales with), X within 1e-6,
status 0.  The FP32 entry point is left out: its range is a separate question."""
import numpy as np
import pytest

from oracle import c_oracle as co
from tests import certify_oracle as cz
from tests import edge_cases as ec
from tests.test_gpu_edge_lengths import up_to_sign
from tests.test_gpu_lane_edges import forms_of, run_with

pytestmark = pytest.mark.gpu

EPS = ec.EPS
PAD = 70
FEW = [6, 12, 31]          # the second call of 3 systems: s-alpha at n / 2, the well at its 2nd eigenvalue, the rough rows below the spectrum


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.close()


def scale_id(s):
    return "gc2^%d_f2^%d" % s


@pytest.mark.parametrize("scale", ec.COUNT_SCALES, ids=scale_id)
@pytest.mark.parametrize("N", ec.COUNT_N_GPU)
def test_counts_across_the_spectrum_and_input_magnitudes(ctx, N, scale):
    """ibs_sturm_count_f64 in every form legal at the length (0: by size, 1: prefix-product sweep, N <= 2050; 2: division form, lanes as
    systems; 3: division form, one wave per system), one call of 70 systems (the 33 of count_batch repeated) and one of 3 (both sides
    of the n_sys >= 64 switch of long grids): equal to the expected counts"""
    k, m = scale
    M = ec.rows_per_lane(N)
    short = N <= 2050
    kernels = {1: "ibs::k_sturm_count<double, %d>" % M, 2: "ibs::k_sturm_count_div", 3: "ibs::k_sturm_count_long"}
    h, g, c, f, shift, want = ec.count_batch(N, k, m)
    assert len(want) == 33
    try:
        for idx in (np.arange(PAD) % 33, np.array(FEW)):
            n = len(idx)
            gi, ci, fi, si, wi = (np.ascontiguousarray(a[idx]) for a in (g, c, f, shift, want))
            for form in ([0, 1] if short else [0]) + [2, 3]:
                ctx.set_option("sturm_form", form if form else None)
                got = np.asarray(ctx.sturm_count(h, gi, ci, fi, si))
                name = ctx.last_launch()[0]
                bad = np.nonzero(got != wi)[0]
                print("count-spectrum: N=%d (g, c) 2^%d f 2^%d form %d, %d systems, %s: %d wrong %s"
                      % (N, k, m, form, n, name, len(bad), [(int(idx[j]), int(got[j]), int(wi[j])) for j in bad[:6]]))
                assert name == kernels[form or (1 if short else (2 if n >= 64 else 3))], (N, n, form, name)
                assert np.array_equal(got, wi), (N, scale, n, form, [(int(idx[j]), int(got[j]), int(wi[j])) for j in bad[:12]])
    finally:
        ctx.set_option("sturm_form", None)


@pytest.mark.parametrize("scale", ec.COUNT_SCALES_GEO, ids=scale_id)
@pytest.mark.parametrize("N", ec.COUNT_N_GEO)
def test_geometry_fed_counts_across_the_spectrum(ctx, N, scale):
    """ibs_geo_sturm_count_f64 on the same 33 systems written as geometry arrays (certify_oracle.gcf_to_geometry: B = 1, gradpar =
    sqrt(g / f), gds2 = g / gradpar, cvdrift = c gradpar; the powers of two are even, so the square root carries them exactly), one
    line per system at theta0 = 0.  The device rows differ from (g, c, f) by roundings of a few ulp per row, far inside the gaps."""
    k, m = scale
    h, g, c, f, shift, want = ec.count_batch(N, k, m)
    geo7, dP = cz.gcf_to_geometry(g, c, f)
    cnt = np.asarray(ctx.geo_sturm_count(h, *geo7, dP, np.zeros(1), shift.reshape(-1, 1))).reshape(-1)
    assert "k_geo_certify<0" in ctx.last_launch()[0]
    bad = np.nonzero(cnt != want)[0]
    print("count-spectrum: geometry-fed N=%d (g, c) 2^%d: %d wrong" % (N, k, len(bad)))
    assert np.array_equal(cnt, want), (N, scale, [(int(j), int(cnt[j]), int(want[j])) for j in bad[:12]])


_SOLVE_REF = {}


def solve_reference(N, k, m):
    """the s-alpha and the well rows of a length at a scale with the C oracle's (gam, lam, X) on the SCALED rows and the scaled ||A||"""
    if (N, k, m) not in _SOLVE_REF:
        cases = ec.count_cases(N)
        h = cases["salpha"][0]
        g, c, f = (np.stack(r) for r in zip(*[ec.scaled_rows(*cases[fam][1], k, m) for fam in ("salpha", "well")]))
        gam, lam, _ = co.solve_gcf_batch(h, g, c, f)
        X = np.stack([co.solve_gcf(h, g[j], c[j], f[j])[2] for j in range(2)])
        _SOLVE_REF[N, k, m] = (h, g, c, f, gam, lam, X, ec.norm_a(h, g, c, f))
    return _SOLVE_REF[N, k, m]


@pytest.mark.parametrize("scale", ec.COUNT_SCALES, ids=scale_id)
@pytest.mark.parametrize("N", ec.COUNT_N_GEO)
def test_raw_solves_on_scaled_rows(ctx, N, scale):
    """ibs_solve_gcf_f64 on the s-alpha and the well rows at every scale: the default form, gcf_direct = 1, and force_p = 32 where
    the length admits it"""
    k, m = scale
    h, g, c, f, gam_o, lam_o, X_o, nA = solve_reference(N, k, m)
    forms = [t for t in forms_of(N) if t[0] in ("default", "gcf_direct=1", "force_p=32")]
    assert len(forms) == (3 if 32 in ec.lanes_allowed(N) else 2)
    for tag, opts, name, P in forms:
        r, got = run_with(ctx, opts, lambda: ctx.solve_gcf(h, g, c, f, want_X=True, want_info=True))
        assert got == name, (N, tag, got, name)
        st = np.asarray(r["info"]) >> 16
        for j, fam in enumerate(("salpha", "well")):
            X = np.asarray(r["X"][j])
            e_lam = abs(float(r["lam"][j]) - lam_o[j]) / (N * EPS * nA[j])
            e_gam = abs(float(r["gam"][j]) - gam_o[j]) / 2.0 ** (k - m)
            e_X = float(np.abs(up_to_sign(X, X_o[j]) * X - X_o[j]).max())
            print("count-spectrum: solve N=%d (g, c) 2^%d f 2^%d %s %s  |dlam| = %.2f N eps ||A||  |dgam| = %.1e 2^(k-m)  |dX| = %.1e  status %d"
                  % (N, k, m, tag, fam, e_lam, e_gam, e_X, st[j]))
            assert e_lam <= 4.0, (N, scale, tag, fam, "lam", e_lam)
            assert e_gam < 1e-8, (N, scale, tag, fam, "gam", e_gam)
            assert e_X < 1e-6, (N, scale, tag, fam, "X", e_X)
            assert st[j] == 0, (N, scale, tag, fam, "status", st[j])
