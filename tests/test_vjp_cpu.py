"""CPU: the restatement of the exact gam / lam vector-Jacobian product (tests/vjp_oracle.py) against central differences of the
oracle's own gam and lam along smooth random directions in the (g, c, f) rows.  It is the yardstick of the kernel test
(tests/test_gpu_vjp.py), so it has to be the derivative of what the oracle computes: s-alpha and synthetic field lines at four grid
lengths, lam_max's eigenpair, and one interior eigenpair (the eigenvalue nearest 0.42 on a strongly driven line)."""
import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from tests import vjp_oracle as vo
from tests.helpers import synthetic_fieldlines


def salpha_rows(N, dP=-1.0):
    th = bo.theta_grid(N)
    g, c = bo.salpha_gc(th, 1.0, 0.8, 0.1)
    return th, g, -dP * c, g.copy()


def synthetic_rows(N):
    th = bo.theta_grid(N)
    ln = synthetic_fieldlines(th)(0.5, [0.3])[0]
    dP = bo.dPdrho_of(ln[2], ln[7], ln[0])
    cv, gd = bo.fold_theta0(0.2, ln[2], ln[3], ln[4], ln[5], ln[6])
    g, c, f = bo.gcf(dP, ln[0], ln[1], cv, gd)
    return th, g, c, f


def directional(th, g, c, f, sigma, seed):
    """(analytic, central-difference) derivative of gam (step 1e-6) and of lam (step 1e-5) along one smooth random direction"""
    rng = np.random.default_rng(seed)
    dg, dc, df = vo.smooth_direction(rng, th, g), vo.smooth_direction(rng, th, np.abs(c).max()), vo.smooth_direction(rng, th, f)
    gam, lam, X = vo.eigenpair(th, g, c, f, sigma)
    out = []
    for k, (gb_, lb_, t) in enumerate(((1.0, 0.0, 1e-6), (0.0, 1.0, 1e-5))):
        gb, cb, fb = vo.gcf_vjp(th, g, c, f, lam, X, gam_bar=gb_, lam_bar=lb_)
        an = gb @ dg + cb @ dc + fb @ df
        p = vo.eigenpair(th, g + t * dg, c + t * dc, f + t * df, sigma)[k]
        m = vo.eigenpair(th, g - t * dg, c - t * dc, f - t * df, sigma)[k]
        out.append((an, (p - m) / (2 * t)))
    return out


@pytest.mark.parametrize("N", [129, 257, 513, 969])
@pytest.mark.parametrize("kind", ["salpha", "synthetic"])
def test_restated_vjp_matches_central_differences(kind, N):
    th, g, c, f = salpha_rows(N) if kind == "salpha" else synthetic_rows(N)
    (ga, gf), (la, lf) = directional(th, g, c, f, None, N)
    assert abs(ga - gf) <= 1e-6 * abs(ga), (ga, gf)
    assert abs(la - lf) <= 1e-5 * abs(la), (la, lf)


def test_restated_vjp_interior_eigenpair():
    """the eigenvalue nearest 0.42 of an s-alpha line driven by dPdrho = -4 lies below lam_max: the same formulas hold"""
    from tests.nearest_oracle import dense_nearest
    th, g, c, f = salpha_rows(513, dP=-4.0)
    assert dense_nearest(th, g, c, f, 0.42)["idx"] >= 1
    (ga, gf), (la, lf) = directional(th, g, c, f, 0.42, 7)
    assert abs(ga - gf) <= 1e-6 * abs(ga), (ga, gf)
    assert abs(la - lf) <= 1e-5 * abs(la), (la, lf)


def test_restated_vjp_is_invariant_to_eigenvector_scale():
    """X enters through quotients only: any nonzero scale and either sign give the same rows"""
    th, g, c, f = synthetic_rows(257)
    gam, lam, X = vo.eigenpair(th, g, c, f)
    a = vo.gcf_vjp(th, g, c, f, lam, X, 0.7, -0.3)
    b = vo.gcf_vjp(th, g, c, f, lam, -3.5 * X, 0.7, -0.3)
    for u, v in zip(a, b):
        assert np.abs(u - v).max() <= 1e-10 * np.abs(u).max()


def test_vjp_entry_point_and_module_are_declared():
    """the C ABI declares ibs_solve_gcf_vjp_f64 and the binding resolves it; ibs_amd.autograd exists, and `import ibs_amd` still
    does not import torch"""
    import os
    import subprocess
    import sys
    import ibs_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "ibs.h")) as fh:
        assert "int ibs_solve_gcf_vjp_f64(" in fh.read()
    assert "ibs_solve_gcf_vjp_f64" in ibs_amd.SYMBOLS
    assert hasattr(ibs_amd.Context, "solve_gcf_vjp")
    code = ("import sys; sys.path.insert(0, %r); import ibs_amd; assert 'torch' not in sys.modules; "
            "import importlib.util; assert importlib.util.find_spec('ibs_amd.autograd') is not None" % root)
    subprocess.check_call([sys.executable, "-c", code])


def test_exact_gradient_entry_points_validate_their_arguments():
    """the autograd layer and the drop-in factory refuse unknown modes before any device work"""
    import ibs_amd
    from ibs_amd import autograd as iag
    z = np.zeros((1, 129))
    with pytest.raises(ValueError):
        iag.solve_gcf(0.1, z, z, z, eigenpair="bogus")
    with pytest.raises(ValueError):
        iag.solve_gcf(0.1, z, z, z, eigenpair="nearest")                  # no sigma
    with pytest.raises(ValueError):
        ibs_amd.make_obj_w_grad(lambda *a: None, jac="bogus")
    with pytest.raises(ValueError):
        ibs_amd.make_obj_w_grad(lambda *a: None, jac="exact", eigenpair="bogus")
    with pytest.raises(ibs_amd.IbsError):
        ibs_amd.Context.solve_gcf_vjp(None, 0.1, z, z, z, np.zeros(1), z)    # neither cotangent
