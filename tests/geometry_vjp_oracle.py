"""CPU oracle for the vector-Jacobian product of the field-line geometry.  TEST INFRASTRUCTURE ONLY.

A torch (CPU, float64) restatement of oracle/geometry_oracle.fieldline_geometry (the reference's vmec_fieldlines,
utils.py:359-720) for many lines on many surfaces, whose VJP comes from torch.autograd.  The root theta_vmec of
utils.py:391-416 is found by Newton without gradient; one more Newton step with a detached denominator then carries the
implicit-function derivative: at the root the step's value is zero and its derivative is -dF / F_theta.
"""
import numpy as np
import torch

MU0 = 4 * np.pi * 1.0e-7


def _t(a):
    return a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=torch.float64)


def forward(xm, xn, xm_nyq, xn_nyq, tab_mn, tab_nyq, scal, line_surf, line_alpha, theta, reverse_modes=False):
    """(geo (8, n_lines, N), dPdrho (n_lines,)) as torch tensors; tab_mn (n_surf, 6, mnmax), tab_nyq (n_surf, 7, mnmax_nyq),
    scal (n_surf, 6) = s iota d_iota_d_s d_pressure_d_s phiedge Aminor_p, line_alpha (n_lines,): differentiable in all four.
    reverse_modes: sum the Fourier series in the opposite mode order (the order-of-summation spread of the oracle)."""
    xm, xn, xmq, xnq, theta = (_t(a) for a in (xm, xn, xm_nyq, xn_nyq, theta))
    tab_mn, tab_nyq, scal, alpha = (_t(a) for a in (tab_mn, tab_nyq, scal, line_alpha))
    if reverse_modes:
        xm, xn, xmq, xnq = xm.flip(0), xn.flip(0), xmq.flip(0), xnq.flip(0)
        tab_mn, tab_nyq = tab_mn.flip(2), tab_nyq.flip(2)
    js = torch.as_tensor(np.asarray(line_surf), dtype=torch.long)
    mn = tab_mn[js]; nq = tab_nyq[js]; sc = scal[js]                       # per line
    s, iota, diota, dp, phiedge, L = (sc[:, k, None] for k in range(6))
    tp = theta[None, :]
    phi = (tp - alpha[:, None]) / iota                                     # utils.py:373 (phi_center = 0)
    lmns = mn[:, 2]                                                        # (n_lines, mnmax)

    def lam_and_dt(tv, ph, lm):
        ang = xm[None, :, None] * tv[:, None, :] - xn[None, :, None] * ph[:, None, :]
        return (lm[:, :, None] * torch.sin(ang)).sum(1), (lm[:, :, None] * xm[None, :, None] * torch.cos(ang)).sum(1)

    with torch.no_grad():                                                  # utils.py:391-416: the root itself
        tv = tp.expand_as(phi).clone()
        for _ in range(60):
            lam, lam_t = lam_and_dt(tv, phi, lmns)
            step = (tv + lam - tp) / (1 + lam_t)
            tv = tv - step
            if float(step.abs().max()) < 1e-15 * max(1.0, float(tv.abs().max())):
                break
        _, lam_t = lam_and_dt(tv, phi, lmns)
    lam, _ = lam_and_dt(tv, phi, lmns)                                     # differentiable in phi and lmns at fixed tv
    tv = tv - (tv + lam - tp) / (1 + lam_t)                                # implicit-function derivative
    ang = xm[None, :, None] * tv[:, None, :] - xn[None, :, None] * phi[:, None, :]
    ca, sa = torch.cos(ang), torch.sin(ang)
    S = lambda coef, trig: (coef[:, :, None] * trig).sum(1)
    R = S(mn[:, 0], ca); R_s = S(mn[:, 3], ca)
    R_t = -S(mn[:, 0] * xm, sa); R_p = S(mn[:, 0] * xn, sa)                # utils.py:432-435
    Z_s = S(mn[:, 4], sa); Z_t = S(mn[:, 1] * xm, ca); Z_p = -S(mn[:, 1] * xn, ca)      # utils.py:437-440
    l_s = S(mn[:, 5], sa); l_t = S(mn[:, 2] * xm, ca); l_p = -S(mn[:, 2] * xn, ca)      # utils.py:442-444
    ang = xmq[None, :, None] * tv[:, None, :] - xnq[None, :, None] * phi[:, None, :]
    ca, sa = torch.cos(ang), torch.sin(ang)
    sqg = S(nq[:, 0], ca); modB = S(nq[:, 1], ca); B_s = S(nq[:, 2], ca)
    B_t = -S(nq[:, 1] * xmq, sa); B_p = S(nq[:, 1] * xnq, sa)              # utils.py:458-462
    Bsup_phi = S(nq[:, 3], ca); Bsub_s = S(nq[:, 4], sa); Bsub_t = S(nq[:, 5], ca); Bsub_p = S(nq[:, 6], ca)   # utils.py:464-468
    etf = -phiedge / (2 * np.pi)                                           # utils.py:474
    sgn = torch.sign(etf).detach()
    Bref = 2 * sgn * etf / (L * L); sq = torch.sqrt(s)                     # utils.py:654-665 (|etf| = sgn etf)
    shat = (-2 * s / iota) * diota                                         # utils.py:316
    sp, cp = torch.sin(phi), torch.cos(phi)
    X_t = R_t * cp; X_p = R_p * cp - R * sp; X_s = R_s * cp                # utils.py:483-489
    Y_t = R_t * sp; Y_p = R_p * sp + R * cp; Y_s = R_s * sp
    gs = torch.stack([Y_t * Z_p - Z_t * Y_p, Z_t * X_p - X_t * Z_p, X_t * Y_p - Y_t * X_p]) / sqg   # utils.py:492-500
    gt = torch.stack([Y_p * Z_s - Z_p * Y_s, Z_p * X_s - X_p * Z_s, X_p * Y_s - Y_p * X_s]) / sqg   # utils.py:502-504
    gp = torch.stack([Y_s * Z_t - Z_s * Y_t, Z_s * X_t - X_s * Z_t, X_s * Y_t - Y_s * X_t]) / sqg   # utils.py:506-508
    gpsi = gs * etf                                                        # utils.py:515-517
    ls = l_s - phi * diota
    galpha = ls * gs + (1 + l_t) * gt + (-iota + l_p) * gp                 # utils.py:520-538
    BxgB_alpha = (Bsub_s * B_t * (l_p - iota) + Bsub_t * B_p * ls + Bsub_p * B_s * (1 + l_t)
                  - Bsub_p * B_t * ls - Bsub_t * B_s * (l_p - iota) - Bsub_s * B_p * (1 + l_t)) / sqg   # utils.py:603-618
    BxgB_psi = (Bsub_t * B_p - Bsub_p * B_t) / sqg * etf                   # utils.py:646-650
    bmag = modB / Bref                                                     # utils.py:678
    gradpar = L * (iota * Bsup_phi) / modB                                 # utils.py:469, 679
    gds2 = (galpha * galpha).sum(0) * L * L * s                            # utils.py:682
    gds21 = (galpha * gpsi).sum(0) * shat / Bref                           # utils.py:683
    gds22 = (gpsi * gpsi).sum(0) * shat * shat / (L * L * Bref * Bref * s)  # utils.py:684-689
    gbdrift = -1.0 * 2 * Bref * L * L * sq * BxgB_alpha / (modB * modB * modB) * sgn        # utils.py:692-702
    gbdrift0 = -1.0 * BxgB_psi * 2 * shat / (modB * modB * modB * sq) * sgn                 # utils.py:704-711
    cvdrift = gbdrift - 2 * Bref * L * L * sq * MU0 * dp * sgn / (etf * modB * modB)        # utils.py:714-718
    geo = torch.stack([bmag, gradpar, cvdrift, gbdrift0, gds2, gds21, gds22, gbdrift])
    dPdrho = -0.5 * ((cvdrift - gbdrift) * bmag * bmag).mean(1)            # ball_scan.py:262
    return geo, dPdrho


def vjp(xm, xn, xm_nyq, xn_nyq, tab_mn, tab_nyq, scal, line_surf, line_alpha, theta, geo_bar, dPdrho_bar=None,
        reverse_modes=False):
    """dict(tab_mn_bar, tab_nyq_bar, scal_bar, alpha_bar) as numpy: the cotangents of the four inputs for the cotangents
    geo_bar (8, n_lines, N) and, optionally, dPdrho_bar (n_lines,)."""
    leaves = [torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=True) for a in (tab_mn, tab_nyq, scal, line_alpha)]
    geo, dP = forward(xm, xn, xm_nyq, xn_nyq, leaves[0], leaves[1], leaves[2], line_surf, leaves[3], theta, reverse_modes)
    f = (geo * _t(geo_bar)).sum()
    if dPdrho_bar is not None:
        f = f + (dP * _t(dPdrho_bar)).sum()
    g = torch.autograd.grad(f, leaves)
    return dict(zip(("tab_mn_bar", "tab_nyq_bar", "scal_bar", "alpha_bar"), (x.numpy() for x in g)))


def numpy_forward(modes, tab_mn, tab_nyq, scal, line_surf, line_alpha, theta):
    """(geo (8, n_lines, N), dPdrho (n_lines,)) from oracle/geometry_oracle.fieldline_geometry, line by line, on the packed arrays
    (modes: mapping with xm, xn, xm_nyq, xn_nyq; phiedge and Aminor_p are per-surface scalars here, one each there)"""
    from oracle import geometry_oracle as go
    out = []
    for js, al in zip(np.asarray(line_surf), np.asarray(line_alpha)):
        d = {k: np.asarray(modes[k], dtype=np.float64) for k in ("xm", "xn", "xm_nyq", "xn_nyq")}
        for k, name in enumerate(go.NAMES_MN):
            d[name] = tab_mn[:, k]
        for k, name in enumerate(go.NAMES_NYQ):
            d[name] = tab_nyq[:, k]
        d["s"], d["iota"], d["d_iota_d_s"], d["d_pressure_d_s"] = scal[:, 0], scal[:, 1], scal[:, 2], scal[:, 3]
        d["phiedge"], d["Aminor_p"] = float(scal[js, 4]), float(scal[js, 5])
        out.append(go.fieldline_geometry(d, int(js), [float(al)], theta)[0])
    geo = np.stack(out, axis=1)
    return geo, -0.5 * np.mean((geo[2] - geo[7]) * geo[0] ** 2, axis=1)


def packed(d):
    """(tab_mn, tab_nyq, scal) from a dict of per-surface vectors by name (tests/golden/G8_surface_tables.npz)"""
    from oracle import geometry_oracle as go
    n = len(d["s"])
    return (np.stack([d[k] for k in go.NAMES_MN], axis=1), np.stack([d[k] for k in go.NAMES_NYQ], axis=1),
            np.stack([d["s"], d["iota"], d["d_iota_d_s"], d["d_pressure_d_s"], np.full(n, float(d["phiedge"])),
                      np.full(n, float(d["Aminor_p"]))], axis=1))
