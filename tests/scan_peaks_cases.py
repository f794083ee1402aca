"""Shared by tests/test_scan_peaks_cpu.py and tests/test_gpu_scan_peaks.py: the coarse tables the peak selection is tried on, the
two-bump field-line family, and a loop over ibs_amd.pick_starts for a batch of surfaces.  Never imported by the product path."""
import numpy as np

import ibs_amd

STARTS = (1, 2, 5, 16)


def grids(na, nt):
    """the scan grids of ball_scan.py:225-226"""
    return np.linspace(0.0, np.pi, na), np.linspace(0.0, 0.5 * np.pi, nt)


def hand_tables():
    """{name: table}: the hand-written cases of the rule"""
    nan = np.nan
    corner = np.array([[5.0, 4.0, 3.0], [4.0, 3.0, 2.0], [3.0, 2.0, 1.0]])            # one peak, at index 0
    plateau = np.array([[0.0, 0.0, 0.0, 0.0, 0.0],
                        [0.0, 2.0, 2.0, 0.0, 0.0],
                        [0.0, 2.0, 2.0, 0.0, 1.0],                                    # (the lower level: a plateau of ones)
                        [0.0, 0.0, 0.0, 1.0, 1.0]])
    equal = np.zeros((5, 7)) - 1.0
    equal[3, 5] = equal[0, 0] = equal[1, 3] = 0.5                                      # three separated peaks of one value
    with_nan = np.array([[1.0, nan, 3.0, nan],
                         [nan, nan, nan, nan],
                         [2.0, nan, nan, 0.5],
                         [nan, 4.0, nan, nan]])
    return {
        "corner": corner, "plateau": plateau, "equal": equal, "nan": with_nan,
        "zero": np.zeros((4, 3)), "all_nan": np.full((3, 4), nan),
        "1xn": np.array([[1.0, 3.0, 2.0, 2.0, 5.0, 5.0, 0.0]]), "nx1": np.array([[2.0], [1.0], [1.0], [3.0], [-1.0], [0.0]]),
        "1x1": np.array([[0.25]]), "1x1_zero": np.array([[0.0]]), "negative": -1.0 - np.arange(12.0).reshape(3, 4),
    }


def family(name, n_surf, na, nt, seed):
    """(n_surf, na, nt) tables of a value family"""
    rng = np.random.default_rng(seed)
    if name == "normal":
        return rng.normal(size=(n_surf, na, nt))
    if name == "ints":                                  # ties everywhere
        return rng.integers(0, 4, size=(n_surf, na, nt)).astype(np.float64)
    if name == "zero":
        return np.zeros((n_surf, na, nt))
    if name == "monotone":                              # one peak, in the last corner; every second surface descends instead
        t = np.arange(na * nt, dtype=np.float64).reshape(na, nt) * 1e-3 - 0.01
        return np.stack([t if k % 2 == 0 else -t for k in range(n_surf)])
    if name == "nan_mixed":                             # healthy surfaces, one with scattered NaN, one all NaN
        t = rng.normal(size=(n_surf, na, nt))
        t[n_surf // 2] = np.nan
        mask = rng.random(size=(na, nt)) < 0.3
        mask.flat[-1] = na * nt > 1                     # (at least one NaN where the table has room, and one finite entry always)
        mask.flat[0] = False
        t[n_surf - 1][mask] = np.nan
        return t
    raise KeyError(name)


FAMILIES = ("normal", "ints", "zero", "monotone", "nan_mixed")


def pick_all(tabs, K):
    """ibs_amd.pick_starts over a batch -> dict(start (n, K, 2), peak, sigma0 (n, K), index (n, K) int32, n_found, bad (n,) int32, n_bad)"""
    n, na, nt = tabs.shape
    al, t0 = grids(na, nt)
    rs = [ibs_amd.pick_starts(t, al, t0, K) for t in tabs]
    out = {k: np.stack([r[k] for r in rs]) for k in ("start", "peak", "sigma0", "index")}
    out["n_found"] = np.array([r["n_found"] for r in rs], dtype=np.int32)
    out["bad"] = np.array([r["n_bad"] for r in rs], dtype=np.int32)       # per surface
    out["n_bad"] = int(out["bad"].sum())
    return out


def bits(a):
    """float64 array -> its bit patterns (NaN == NaN, -0.0 != 0.0)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def two_bump_fieldlines(theta, alpha_scan):
    """tests/helpers.synthetic_fieldlines with gradpar = 1 and two bumps in alpha: a broad one on node 1 of alpha_scan and a narrow,
    higher one half way between nodes 4 and 5 -- the coarse table ranks the narrow basin second, its crest holds the maximum"""
    theta = np.asarray(theta)
    a1, a2 = alpha_scan[1], 0.5 * (alpha_scan[4] + alpha_scan[5])

    def fieldlines(s, alphas):
        out = []
        for a in np.atleast_1d(alphas):
            shat = 0.4 + 1.2 * s
            am = (0.5 + 0.8 * s) * (1 + 0.30 * np.exp(-((a - a1) / 0.5) ** 2) + 0.55 * np.exp(-((a - a2) / 0.25) ** 2))
            lam0 = shat * theta - am * np.sin(theta)
            bmag = 1 + 0.1 * s * np.cos(theta)
            gradpar = np.ones_like(theta)
            gds2 = 1 + lam0 ** 2
            gds21 = -shat * lam0
            gds22 = np.full_like(theta, shat ** 2)
            cvdrift = am * (np.cos(theta) + np.sin(theta) * lam0)
            cvdrift0 = -am * shat * np.sin(theta)
            gbdrift = cvdrift - 2.0 / bmag ** 2          # => dPdrho = -1
            out.append(np.stack([bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, gbdrift]))
        return np.stack(out)

    return fieldlines
