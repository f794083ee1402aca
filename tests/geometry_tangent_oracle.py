"""CPU oracle for the alpha-tangent of the field-line geometry.  TEST INFRASTRUCTURE ONLY.

The tangent comes from torch.autograd.functional.jvp through tests/geometry_vjp_oracle.forward with the all-ones direction in
line_alpha: every line depends on its own alpha only, so one forward-mode pass gives d/d alpha of every line at once.
"""
import numpy as np
import torch

from tests import geometry_vjp_oracle as vo


def dalpha(xm, xn, xm_nyq, xn_nyq, tab_mn, tab_nyq, scal, line_surf, line_alpha, theta, reverse_modes=False):
    """(geo (8, n_lines, N), geo_da (8, n_lines, N), dPdrho (n_lines,), dPdrho_da (n_lines,)) as numpy: the forward and its derivative
    in each line's alpha.  reverse_modes: sum the Fourier series in the opposite mode order."""
    al = torch.as_tensor(np.asarray(line_alpha, dtype=np.float64))
    f = lambda a: vo.forward(xm, xn, xm_nyq, xn_nyq, tab_mn, tab_nyq, scal, line_surf, a, theta, reverse_modes)
    (geo, dP), (geo_da, dP_da) = torch.autograd.functional.jvp(f, al, torch.ones_like(al))
    return geo.numpy(), geo_da.numpy(), dP.numpy(), dP_da.numpy()


def rows(geo, theta0, dPdrho=None):
    """(g, c, f) of lines geo (8, n, N) at theta0 (n,) (ball_scan.py:267-268, utils.py:1560-1562), dPdrho from the lines unless given"""
    th0 = np.asarray(theta0, dtype=np.float64)[:, None]
    if dPdrho is None:
        dPdrho = -0.5 * np.mean((geo[2] - geo[7]) * geo[0] ** 2, axis=1)
    dP = np.asarray(dPdrho)[:, None]
    B, gp = geo[0], np.abs(geo[1])
    d = geo[4] + 2 * th0 * geo[5] + th0 ** 2 * geo[6]
    return gp / B * d, -dP * (geo[2] + th0 * geo[3]) / (gp * B), d / (gp * B ** 3)


def rows_dalpha(geo, geo_da, theta0):
    """the alpha-derivative of rows(geo, theta0) at fixed dPdrho, from the tangent planes geo_da"""
    th0 = np.asarray(theta0, dtype=np.float64)[:, None]
    dP = (-0.5 * np.mean((geo[2] - geo[7]) * geo[0] ** 2, axis=1))[:, None]
    B, gp = geo[0], np.abs(geo[1])
    dB, dgp = geo_da[0], np.sign(geo[1]) * geo_da[1]
    d = geo[4] + 2 * th0 * geo[5] + th0 ** 2 * geo[6]
    dd = geo_da[4] + 2 * th0 * geo_da[5] + th0 ** 2 * geo_da[6]
    cv, dcv = geo[2] + th0 * geo[3], geo_da[2] + th0 * geo_da[3]
    g_a = (dgp / B - gp * dB / B ** 2) * d + gp / B * dd
    inv = 1.0 / (gp * B)
    dinv = -inv ** 2 * (dgp * B + gp * dB)
    c_a = -dP * (dcv * inv + cv * dinv)
    f_a = dd * inv / B ** 2 + d * (dinv / B ** 2 - 2 * inv * dB / B ** 3)
    return g_a, c_a, f_a
