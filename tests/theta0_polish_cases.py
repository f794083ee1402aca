"""Cases of the theta0 polish (csrc/ibs_theta0_polish.hpp): field lines whose growth rate peaks between the nodes of a theta0 grid or
on the edge of the box, the CPU oracle's gam on them, and hand-written rows for the peak rule.  Test-only."""
import functools

import numpy as np

from oracle import ballooning_oracle as bo


def shifted_fieldlines(theta, phi):
    """tests/helpers.synthetic_fieldlines with the secular term shifted by phi: lam0 = shat (theta - phi) - am sin(theta), which moves
    the crest of gam(theta0) to about theta0 = -phi.  Returns fieldlines(s, alphas) -> (nalpha, 8, N)."""
    theta = np.asarray(theta)

    def fieldlines(s, alphas):
        out = []
        for a in np.atleast_1d(alphas):
            shat = 0.4 + 1.2 * s
            am = (0.5 + 0.8 * s) * (1 + 0.35 * np.cos(a - 0.9) + 0.1 * np.cos(2 * a))
            lam0 = shat * (theta - phi) - am * np.sin(theta)
            bmag = 1 + 0.1 * s * np.cos(theta)
            gradpar = np.ones_like(theta) * (1.0 + 0.05 * np.cos(a))
            gds2 = 1 + lam0 ** 2
            gds21 = -shat * lam0
            gds22 = np.full_like(theta, shat ** 2)
            cvdrift = am * (np.cos(theta) + np.sin(theta) * lam0)
            cvdrift0 = -am * shat * np.sin(theta)
            gbdrift = cvdrift - 2.0 / bmag ** 2          # => dPdrho = -1
            out.append(np.stack([bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, gbdrift]))
        return np.stack(out)

    return fieldlines


# (s, alpha, phi): four crests inside the box [0, pi / 2], then two maxima on its edges (theta0 = 0 and theta0 = pi / 2)
INTERIOR = [(0.5, 0.3, -0.2), (0.5, 0.3, -0.05), (0.9, 1.0, -0.6), (0.5, 2.0, -1.5)]
EDGE = [(0.5, 0.3, 0.23), (0.5, 2.0, -1.65)]
CASES = INTERIOR + EDGE
GRIDS = (5, 15)


def theta0_grid(n):
    return np.linspace(0.0, 0.5 * np.pi, n)


@functools.lru_cache(maxsize=None)
def case_line(N, case):
    """(theta, line (8, N), dPdrho) of one case"""
    s, alpha, phi = case
    theta = bo.theta_grid(N)
    line = shifted_fieldlines(theta, phi)(s, [alpha])[0]
    return theta, line, bo.dPdrho_of(line[2], line[7], line[0])


def case_lines(N, cases=CASES):
    """(h, geo7: seven (n, N) arrays, dPdrho (n,)) of the cases, as Context.gamma_scan takes them"""
    lines = np.stack([case_line(N, c)[1] for c in cases])
    theta = bo.theta_grid(N)
    return theta[1] - theta[0], [np.ascontiguousarray(lines[:, k]) for k in range(7)], np.array([case_line(N, c)[2] for c in cases])


def oracle_gam(N, case, t0):
    """the CPU oracle's growth rate of the case's line at theta0 = t0"""
    theta, line, dP = case_line(N, case)
    cv, gd = bo.fold_theta0(float(t0), line[2], line[3], line[4], line[5], line[6])
    return float(bo.gamma_ball_full(dP, theta, line[0], line[1], cv, gd)[0])


@functools.lru_cache(maxsize=None)
def oracle_row(N, case, n_theta0):
    return np.array([oracle_gam(N, case, t) for t in theta0_grid(n_theta0)])


def dense_max(N, case, lo, hi, n=801):
    """the maximum of n oracle samples of [lo, hi]"""
    return max(oracle_gam(N, case, t) for t in np.linspace(lo, hi, n))


def bracket(theta0, row, node):
    """the bracket rule: [theta0[node - 1], theta0[node + 1]], cut to the node where the row ends or the neighbour is NaN"""
    lo = theta0[node - 1] if node > 0 and not np.isnan(row[node - 1]) else theta0[node]
    hi = theta0[node + 1] if node + 1 < len(row) and not np.isnan(row[node + 1]) else theta0[node]
    return float(lo), float(hi)


nan = float("nan")
# (row, K = 4 expectation: node, n_found) -- written out by hand from the rule
HAND_ROWS = [
    ([1.0, 3.0, 2.0, 5.0, 4.0], [3, 1, 3, 3], 2),                    # two peaks, ranked by value
    ([2.0, 2.0, 2.0, 2.0], [0, 0, 0, 0], 1),                           # plateau: the smallest index alone
    ([1.0, 4.0, 1.0, 4.0, 1.0], [1, 3, 1, 1], 2),                      # tie between peaks: index ascending; peaks two apart share a bracket end
    ([3.0, nan, 3.0], [0, 2, 0, 0], 2),                                # NaN neighbours never beat
    ([nan, 1.0, nan, 0.5, nan], [1, 3, 1, 1], 2),
    ([nan, nan, nan], [-1, -1, -1, -1], 0),                            # all NaN
    ([7.0], [0, 0, 0, 0], 1),                                          # length 1
    ([1.0, 2.0], [1, 1, 1, 1], 1),                                     # length 2
    ([2.0, 2.0], [0, 0, 0, 0], 1),
    ([5.0, 1.0, 4.0, 1.0, 3.0, 1.0, 2.0, 1.0, 6.0], [8, 0, 2, 4], 4),  # more peaks than slots
    ([1.0, 2.0, 2.0, 1.0, -np.inf, 0.0], [1, 5, 1, 1], 2),             # plateau inside, -inf is a value
]
