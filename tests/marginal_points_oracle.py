"""CPU restatement of ibs_marginal_obj_w_grad_f64 (the objective of the margin's refinement in (alpha, theta0)), from the pieces of
tests/marginal_oracle.py: the centre line's rows, mo.solve, mo.grad_rows, the theta0 tangent, and the side lines' rows through
mo.line_gc with each line's own bo.dPdrho_of.  MarginalPointsOracleContext lets BallooningScan.marginal(refine=True) run without a
GPU.  Test infrastructure only."""
import numpy as np

from oracle import ballooning_oracle as bo
from tests import marginal_oracle as mo


def point(h, geo3, t0, del_alpha=0.004, want_grad=True):
    """one point: geo3 (3, 8, N) = the lines alpha - del_alpha / 2, alpha, alpha + del_alpha / 2.  dict(val = -1 / s*, scale, dPdrho,
    u (0 with scale = inf), info[, jac (2,), dscale (2,) = (d s* / d alpha, d s* / d theta0)])"""
    dP = [bo.dPdrho_of(ln[2], ln[7], ln[0]) for ln in geo3]
    g, c = mo.line_gc(dP[1], *geo3[1][:7], t0)
    r = mo.solve(h, g, c)
    out = dict(val=0.0 - r["mu"], scale=r["scale"], dPdrho=dP[1], u=r.get("u", 0.0), info=0)
    if r["X"] is None:
        out.update(info=256 << 16, val=0.0)
        if want_grad:
            out.update(jac=np.zeros(2), dscale=np.zeros(2))
        return out
    if want_grad:
        gb, cb = mo.grad_rows(h, r)
        c_ln = geo3[1]
        gt, ct = mo.theta0_tangent(c_ln[0], c_ln[1], c_ln[3], c_ln[5], c_ln[6], dP[1], t0)
        gl, cl = mo.line_gc(dP[0], *geo3[0][:7], t0)
        gr, cr = mo.line_gc(dP[2], *geo3[2][:7], t0)
        ds = np.array([float(np.sum(gb * (gr - gl) + cb * (cr - cl))) / del_alpha, float(np.sum(gb * gt + cb * ct))])
        out.update(dscale=ds, jac=ds / r["scale"] ** 2)
    return out


def points(h, geo, theta0, del_alpha=0.004, want_grad=True):
    """the batch: geo (n, 3, 8, N), theta0 (n,) -> dict of arrays (val, scale, dPdrho, u, info[, jac, dscale])"""
    rs = [point(h, geo[k], float(theta0[k]), del_alpha, want_grad) for k in range(len(geo))]
    out = {key: np.array([r[key] for r in rs]) for key in ("val", "scale", "dPdrho", "u")}
    out["info"] = np.array([r["info"] for r in rs], dtype=np.int32)
    if want_grad:
        out.update(jac=np.array([r["jac"] for r in rs]).reshape(len(rs), 2), dscale=np.array([r["dscale"] for r in rs]).reshape(len(rs), 2))
    return out


class MarginalPointsOracleContext(mo.MarginalOracleContext):
    """MarginalOracleContext + marginal_obj_w_grad (host arrays); n_point_evals counts the points evaluated"""
    n_point_evals = 0

    def marginal_obj_w_grad(self, h, geo, theta0, del_alpha=0.004, want_grad=True, want_info=False):
        r = points(h, np.asarray(geo), np.asarray(theta0), del_alpha, want_grad)
        self.n_point_evals += len(r["val"])
        out = dict(val=r["val"], scale=r["scale"], dPdrho=r["dPdrho"], nbad=0)
        if want_grad:
            out.update(jac=r["jac"], dscale=r["dscale"])
        if want_info:
            out.update(info=r["info"])
        return out
