"""Per-equilibrium scan driver: the build's counterpart of ball_scan.py:190-386.

One process per GPU.  Surfaces are sharded over ranks (surface r goes to rank r % world, the
`mpi.group` <-> surface mapping of ball_scan.py:172, 251-252); every rank scans its surfaces on
its GPU, refines the per-surface maximum, and one all-gather (RCCL on GPUs, gloo in CPU tests)
replaces the three comm_lead.Gather calls of ball_scan.py:345-347.  No data-path collective
exists besides that gather.

Geometry is produced on the host by the caller (SIMSOPT/VMEC stay untouched, BASELINE north_star):
`fieldlines(s, alphas)` must return an array (len(alphas), 8, N) in the order
bmag, gradpar_theta_pest, cvdrift, cvdrift0, gds2, gds21, gds22, gbdrift -- e.g. a thin wrapper
around the reference's own utils.vmec_fieldlines (ball_scan.py:251-261).
"""
import numpy as np

from ._lib import IbsError
from .solver import CLUSTER_BIT, MAX_ROW_STARTS

GEO_ORDER = ("bmag", "gradpar_theta_pest", "cvdrift", "cvdrift0", "gds2", "gds21", "gds22", "gbdrift")


def shard_surfaces(n_surf, rank, world):
    """indices of the surfaces owned by `rank` (round-robin)"""
    return list(range(rank, n_surf, world))


def pick_start(gam_table, alpha_scan, theta0_scan):
    """ball_scan.py:279-295: start point of the refinement from the coarse table (first maximum on ties;
    an all-zero table starts from (0, 0) with sigma0 = 0.05)."""
    if not np.all(np.isfinite(gam_table)):
        raise IbsError("coarse table holds %d non-finite growth rates (invalid geometry?)"
                       % int(np.sum(~np.isfinite(gam_table))))
    m = np.max(gam_table)
    if m == 0.0:
        return 0.0, 0.0, 0.05, None
    idx = np.where(gam_table == m)
    i, j = int(idx[0][0]), int(idx[1][0])
    return float(alpha_scan[i]), float(theta0_scan[j]), 1.3 * abs(float(gam_table[i, j])) + 0.05, (i, j)


MAX_STARTS = 16


def check_n_starts(n_starts):
    ok = isinstance(n_starts, (int, np.integer)) and not isinstance(n_starts, bool)
    if not ok or not 1 <= n_starts <= MAX_STARTS:
        raise ValueError("n_starts must be an integer in [1, %d], not %r" % (MAX_STARTS, n_starts))
    return int(n_starts)


def pick_starts(gam_table, alpha_scan, theta0_scan, n_starts):
    """the n_starts best local maxima ("peaks") of a coarse table (n_alpha, n_theta0) as the starts of a multi-start refinement:
    the rule of ibs_scan_peaks_f64 (csrc/ibs_scan_peaks.hpp) in numpy, and that kernel's oracle.
    A neighbour w of entry v beats it if w > v, or w == v and w has the smaller row-major index; a NaN never beats anything.  An
    entry is a peak if it is not NaN and none of its up to eight neighbours (i +- 1, j +- 1) inside the table beats it -- no
    wrap-around: alpha in [0, pi] and theta0 in [0, pi / 2] are a box, as in the refinement's bounds.  Peaks rank by value
    descending, ties by index ascending, so the first maximum of the table is peak 0.
    Slot 0 is pick_start's: start (alpha[i], theta0[j]), sigma0 = 1.3 |gam| + 0.05; a maximum of exactly 0 starts at (0, 0) with
    sigma0 = 0.05 (ball_scan.py:279-282); one that is not finite (or a table of NaN) is counted in n_bad -- where pick_start
    raises -- and starts at (0, 0).  In the last two cases n_found = 0 and every slot repeats slot 0.  Slots 1 .. n_starts - 1 are
    the next peaks in rank, each with its own start, value, index and sigma0 = 1.3 |peak| + 0.05; with fewer peaks than slots
    n_found is the number found and the remaining slots repeat slot 0.
    Returns dict(start (n_starts, 2), peak (n_starts,), index int32 (n_starts,): row-major, -1 where the start is no node,
    sigma0 (n_starts,), n_found, n_bad)."""
    K = check_n_starts(n_starts)
    tab = np.asarray(gam_table, dtype=np.float64)
    na, nt = tab.shape
    idx = np.arange(na * nt, dtype=np.int64).reshape(na, nt)
    pv = np.full((na + 2, nt + 2), np.nan); pv[1:-1, 1:-1] = tab
    pi = np.full((na + 2, nt + 2), -1, dtype=np.int64); pi[1:-1, 1:-1] = idx
    beaten = np.isnan(tab)
    with np.errstate(invalid="ignore"):
        for di in (0, 1, 2):
            for dj in (0, 1, 2):
                if (di, dj) != (1, 1):
                    w, iw = pv[di:di + na, dj:dj + nt], pi[di:di + na, dj:dj + nt]
                    beaten |= (w > tab) | ((w == tab) & (iw < idx))          # (the NaN frame never beats: both comparisons are false)
    flat = tab.reshape(-1)
    peaks = np.nonzero(~beaten.reshape(-1))[0]
    picks = peaks[np.lexsort((peaks, -flat[peaks]))][:K]
    m = float(flat[picks[0]]) if len(picks) else float("nan")
    ok = bool(np.isfinite(m))
    node = ok and m != 0.0
    nf = len(picks) if node else 0
    out = dict(start=np.zeros((K, 2)), peak=np.full(K, m), index=np.full(K, -1, dtype=np.int32), sigma0=np.full(K, 0.05),
               n_found=nf, n_bad=0 if ok else 1)
    for k in range(K if node else 0):
        e = int(picks[k if k < nf else 0])
        v = float(flat[e])
        out["start"][k] = alpha_scan[e // nt], theta0_scan[e % nt]
        out["peak"][k], out["index"][k], out["sigma0"][k] = v, e, 1.3 * abs(v) + 0.05       # ball_scan.py:289, 295
    return out


POLISH_MAX_EVAL = 64
NODE_RETURNED_BIT, MAX_EVAL_BIT, ONE_SIDED_BIT = 1 << 10, 1 << 11, 1 << 12
_GOLD = 0.3819660112501051          # (3 - sqrt 5) / 2


def row_peaks(gam, K):
    """the K best peaks of every row of gam (n_rows, n_theta0) (or of one row): the rule of ibs_row_peaks_f64 and of the kernel behind
    ibs_theta0_polish_f64 (csrc/ibs_theta0_polish.hpp) in numpy -- pick_starts' rule in one dimension.  Entry j is a peak if it is
    not NaN and neither neighbour inside the row beats it (w beats v if w > v, or w == v and w has the smaller index; a NaN never
    beats anything); peaks rank by value descending, ties by index ascending.  Returns (node int32 (n_rows, K), n_found int32
    (n_rows,)): slot k holds peak k, slots from n_found on repeat slot 0, a row without a finite entry has n_found = 0 and node -1."""
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= MAX_ROW_STARTS:
        raise ValueError("K must be an integer in [1, %d], not %r" % (MAX_ROW_STARTS, K))
    tab = np.atleast_2d(np.asarray(gam, dtype=np.float64))
    n_rows, nt = tab.shape
    idx = np.arange(nt)
    node = np.full((n_rows, K), -1, dtype=np.int32)
    n_found = np.zeros(n_rows, dtype=np.int32)
    pad = np.full((n_rows, nt + 2), np.nan); pad[:, 1:-1] = tab
    with np.errstate(invalid="ignore"):
        left, right = pad[:, :-2], pad[:, 2:]
        beaten = np.isnan(tab) | (left >= tab) | (right > tab)        # (the left neighbour has the smaller index: it wins ties)
    for r in range(n_rows):
        peaks = idx[~beaten[r]]
        picks = peaks[np.lexsort((peaks, -tab[r, peaks]))][:K]
        n_found[r] = len(picks)
        if len(picks):
            node[r] = picks[0]
            node[r, :len(picks)] = picks
    return node, n_found


def polish_theta0(f, theta0, row, node, xtol=1e-5, max_eval=32):
    """gam maximised over theta0 about node `node` of the coarse row `row` (values of f at the nodes theta0): the state machine of
    csrc/ibs_theta0_polish.hpp (ibs_theta0_polish_init / _step / _result, and every wave of ibs_theta0_polish_f64) restated in
    pure Python, statement by statement, so that it asks f for the same points bit for bit.  f(theta0) -> gam, or (gam, status).
    Bracket [theta0[node - 1], theta0[node + 1]], cut to the node where the row ends or the neighbour is NaN (exactly one side cut:
    status bit 12; zero length: the node, no evaluation).  Brent's bounded search on the absolute tolerance xtol, seeded with the
    three known values (one-sided: first the golden point next to the node); it stops on |x - m| <= 2 xtol - (b - a) / 2 or after
    max_eval evaluations (bit 11).  A value that is not finite, or that comes with status bit 0 or 1 (a failed evaluation), counts as -inf.  The result is the best evaluated point only if its
    value is strictly greater than the node's, else the node with the row's value (bit 10).
    Returns dict(theta0, gam, n_eval, status, points: the requested theta0 in order)."""
    theta0 = np.asarray(theta0, dtype=np.float64)
    row = np.asarray(row, dtype=np.float64)
    n, j = len(theta0), int(node)
    if not (0 <= j < n) or not (xtol > 0 and np.isfinite(xtol)) or not 1 <= max_eval <= POLISH_MAX_EVAL or np.isnan(row[j]):
        raise ValueError("polish_theta0: node in [0, n), a gam at the node, xtol > 0 and max_eval in [1, %d] required" % POLISH_MAX_EVAL)
    if not (np.all(np.isfinite(theta0)) and np.all(np.diff(theta0) > 0)):
        raise ValueError("polish_theta0: theta0 must be finite and strictly increasing")
    has_lo = j > 0 and not np.isnan(row[j - 1])
    has_hi = j + 1 < n and not np.isnan(row[j + 1])
    xn, fn = float(theta0[j]), float(row[j])
    a = float(theta0[j - 1]) if has_lo else xn
    b = float(theta0[j + 1]) if has_hi else xn
    s = dict(a=a, b=b, x=xn, fx=fn, w=xn, fw=fn, v=xn, fv=fn, d=0.0, e=0.0, n_eval=0, status=0)
    points = []
    tol1, tol2 = float(xtol), 2.0 * float(xtol)

    def propose():
        """Brent's next point, or None when the search is over"""
        if s["n_eval"] >= max_eval:
            s["status"] |= MAX_EVAL_BIT
            return None
        a, b, x, w, v = s["a"], s["b"], s["x"], s["w"], s["v"]
        fx, fw, fv = s["fx"], s["fw"], s["fv"]
        xm = 0.5 * (a + b)
        if abs(x - xm) <= tol2 - 0.5 * (b - a):
            return None
        parab, d = False, 0.0
        with np.errstate(all="ignore"):
            if abs(s["e"]) > tol1:
                r = np.float64(x - w) * np.float64(fx - fv)
                q = np.float64(x - v) * np.float64(fx - fw)
                p = np.float64(x - v) * q - np.float64(x - w) * r
                q = 2.0 * (q - r)
                if q > 0.0:
                    p = -p
                q = abs(q)
                etemp = s["e"]
                if abs(p) < abs(0.5 * q * etemp) and p > q * (a - x) and p < q * (b - x):
                    d = float(p / q)
                    u = x + d
                    if u - a < tol2 or b - u < tol2:
                        d = tol1 if xm >= x else -tol1
                    parab = True
                    s["e"] = s["d"]
        if not parab:
            s["e"] = a - x if x >= xm else b - x
            d = _GOLD * s["e"]
        s["d"] = d
        s["n_eval"] += 1
        return x + d if abs(d) >= tol1 else (x + tol1 if d > 0.0 else x - tol1)

    def value(u):
        points.append(u)
        r = f(u)
        g, st = r if isinstance(r, tuple) else (r, 0)
        s["status"] |= int(st) & 3
        g = float(g)
        return g if np.isfinite(g) and not int(st) & 3 else -np.inf

    u = None
    if b > a:
        if has_lo and has_hi:
            flo, fhi = float(row[j - 1]), float(row[j + 1])
            lo_better = flo >= fhi
            s["w"], s["fw"] = (a, flo) if lo_better else (b, fhi)
            s["v"], s["fv"] = (b, fhi) if lo_better else (a, flo)
            s["d"] = s["e"] = b - a
            u = propose()
        else:
            s["status"] |= ONE_SIDED_BIT
            s["v"], s["fv"] = (b, float(row[j + 1])) if has_hi else (a, float(row[j - 1]))
            u = a + _GOLD * (b - a) if has_hi else b - _GOLD * (b - a)
            s["n_eval"] = 1
            fu = value(u)
            s["x"], s["fx"] = u, fu
            s["d"] = s["e"] = b - a
            u = propose()
    while u is not None:
        fu = value(u)
        x = s["x"]
        if fu >= s["fx"]:
            if u >= x:
                s["a"] = x
            else:
                s["b"] = x
            s["v"], s["fv"], s["w"], s["fw"], s["x"], s["fx"] = s["w"], s["fw"], x, s["fx"], u, fu
        else:
            if u < x:
                s["a"] = u
            else:
                s["b"] = u
            if fu >= s["fw"] or s["w"] == x:
                s["v"], s["fv"], s["w"], s["fw"] = s["w"], s["fw"], u, fu
            elif fu >= s["fv"] or s["v"] == x or s["v"] == s["w"]:
                s["v"], s["fv"] = u, fu
        u = propose()
    better = s["fx"] > fn
    return dict(theta0=s["x"] if better else xn, gam=s["fx"] if better else fn, n_eval=s["n_eval"],
                status=s["status"] | (0 if better else NODE_RETURNED_BIT), points=points)


def gather_rows_tensor(local, n_surf, rank, world, dist, ctx=None):
    """ONE all-gather of per-surface rows held as a torch tensor (device tensor: RCCL, in-stream; CPU tensor: gloo).
    ctx: a Context that holds a native communicator (Context.comm_init): the collective is then issued by the library
    itself (ibs_comm_allgather_f64) instead of torch.distributed.
    local: (n_local, k) rows of the surfaces shard_surfaces(n_surf, rank, world) lists.  Returns (n_surf, k) in surface
    order on every rank (replaces the three comm_lead.Gather of ball_scan.py:345-347)."""
    import torch
    k = local.shape[1]
    if world == 1:
        return local.clone()
    n_max = (n_surf + world - 1) // world
    pad = torch.full((n_max, k), float("nan"), dtype=local.dtype, device=local.device)
    pad[: local.shape[0]] = local
    out = torch.empty((world * n_max, k), dtype=local.dtype, device=local.device)
    if ctx is not None and getattr(ctx, "_comm_world", 0) == world and local.is_cuda:
        ctx.allgather(pad, out)
    else:
        dist.all_gather_into_tensor(out, pad)
    # row of surface j: rank j % world, slot j // world
    j = torch.arange(n_surf, device=local.device)
    return out[(j % world) * n_max + j // world]


def gather_surfaces(local, n_surf, rank, world, dist=None, device=None, ctx=None):
    """all-gather of per-surface rows.  local: (n_local, k) rows of the surfaces shard_surfaces() lists.
    Returns (n_surf, k) on every rank (replaces ball_scan.py:345-347)."""
    local = np.asarray(local, dtype=np.float64)
    if world == 1:
        return local.copy()
    import torch
    t = torch.from_numpy(np.ascontiguousarray(local))
    if device is not None:
        t = t.to(device)
    return gather_rows_tensor(t, n_surf, rank, world, dist, ctx).cpu().numpy()


EIGENPAIRS = ("max", "nearest")
# upstream's shifts (eigenpair="nearest"): the coarse scan (ball_scan.py:230, 269) and the final solve (ball_scan.py:337, the
# default of gamma_ball_full); the refinement's is 1.3 |gam| + 0.05 of the surface's coarse maximum (ball_scan.py:289, 295)
SIGMA_COARSE = 1.0
SIGMA_FINAL = 0.42


def first_unstable(t_stable, t_unstable, lo_unstable, t_lo):
    """The envelope of BallooningScan.local_eq_boundary over (alpha, theta0): from t_stable, t_unstable (n, nalpha, n_theta0, n_fixed,
    max_cross) and lo_unstable (n, nalpha, n_theta0, n_fixed) the smallest t = (t_stable + t_unstable) / 2 of a crossing from stable
    to unstable (t_stable < t_unstable) of any line of the surface, +inf where there is none, t_lo where a line is unstable at t_lo.
    Returns (n, n_fixed)."""
    t_stable, t_unstable = np.asarray(t_stable), np.asarray(t_unstable)
    up = t_stable < t_unstable                              # (NaN beyond n_cross: False)
    first = np.where(up, 0.5 * (t_stable + t_unstable), np.inf).min(axis=(1, 2, 4), initial=np.inf)
    return np.where((np.asarray(lo_unstable) > 0).any(axis=(1, 2)), float(t_lo), first)


def local_eq_first_up(t_stable, t_unstable, lo_unstable, t_lo):
    """T of every ray of a local_eq_boundary result, with no reduction -- the per-ray form of what first_unstable reduces (the rule:
    csrc/ibs_local_eq_boundary_polish.hpp): from t_stable, t_unstable (..., max_cross) and lo_unstable (...) the first-stability
    parameter t_lo where the ray is unstable at t_lo, else the smallest (t_stable + t_unstable) / 2 of a crossing from stable to
    unstable (t_stable < t_unstable; of a ray that starts stable that is crossing 0), else +inf; NaN for an invalid ray
    (lo_unstable < 0).  t_lo: a scalar, or an array that broadcasts against lo_unstable.  Returns (...)."""
    t_stable, t_unstable, lo = np.asarray(t_stable, dtype=np.float64), np.asarray(t_unstable, dtype=np.float64), np.asarray(lo_unstable)
    up = t_stable < t_unstable                              # (NaN beyond n_cross: False)
    first = np.where(up, 0.5 * (t_stable + t_unstable), np.inf).min(axis=-1, initial=np.inf)
    return np.where(lo < 0, np.nan, np.where(lo > 0, np.asarray(t_lo, dtype=np.float64), first))


def polish_first_up(boundary, theta0, t_row, node, t_lo, xtol=1e-5, max_eval=32):
    """T minimised over theta0 about node `node` of the coarse row t_row (T at the nodes theta0) of ONE (line, ray family): the rule of
    csrc/ibs_local_eq_boundary_polish.hpp restated in Python, so that it asks for the same points bit for bit as every wave of
    ibs_local_eq_boundary_polish_f64.  boundary(theta0) -> (t_stable, t_unstable, lo_unstable, status) of the family's ray at that
    theta0 with max_cross = 1 (scalars; status = info >> 16 of Context.local_eq_boundary).  f = -T = -local_eq_first_up(...) is
    maximised by polish_theta0 unchanged on the row -t_row; an evaluation with status bit 0 or 1 is a failed one.  The addition: a node
    with T = t_lo is returned at once (no evaluation, bit 10).  Where the node itself is returned one more evaluation at the node, not
    counted in n_eval, supplies the ends.  Status bit 1 gives NaN outputs and lo_unstable -1.
    Returns dict(theta0, t, t_stable, t_unstable, lo_unstable, n_eval, status, points: the theta0 of the search in order)."""
    theta0 = np.asarray(theta0, dtype=np.float64)
    row = np.asarray(t_row, dtype=np.float64)
    j, nan = int(node), float("nan")
    xn, Tn = float(theta0[j]), float(row[j])
    if Tn == t_lo:
        return dict(theta0=xn, t=Tn, t_stable=nan, t_unstable=nan, lo_unstable=1, n_eval=0, status=NODE_RETURNED_BIT, points=[])
    seen, extra = {}, [0]

    def f(u):
        ts, tu, lo, st = boundary(u)
        seen[u] = (float(ts), float(tu), int(lo))
        extra[0] |= int(st) & 8
        return -float(local_eq_first_up(np.array([ts]), np.array([tu]), lo, t_lo)), int(st)

    r = polish_theta0(f, theta0, -row, j, xtol=xtol, max_eval=max_eval)
    status = r["status"] | extra[0]
    if status & NODE_RETURNED_BIT:
        ts, tu, lo, st = boundary(xn)
        status |= int(st) & 11
        x, t, ts, tu, lo = xn, Tn, float(ts), float(tu), int(lo)
    else:
        x, t = r["theta0"], -r["gam"]
        ts, tu, lo = seen[x]
    if status & 2:
        x = t = ts = tu = nan
        lo = -1
    return dict(theta0=x, t=t, t_stable=ts, t_unstable=tu, lo_unstable=lo, n_eval=r["n_eval"], status=status, points=r["points"])


def check_eigenpair(eigenpair):
    if eigenpair not in EIGENPAIRS:
        raise ValueError("eigenpair must be 'max' or 'nearest', not %r" % (eigenpair,))
    return eigenpair


# lanes per grid point of the geometry kernel in the rounds of marginal(refine=True) (option "geo_lpp"; BallooningScan._marginal_points)
MARGINAL_GEO_LPP = 1

JACS = ("reference", "exact", "exact_tangent")


class JacError(IbsError, ValueError):
    """an unknown jac value: an IbsError that is, like the drivers' other option errors (eigenpair, certify), a ValueError as well"""


def check_jac(jac):
    if jac not in JACS:
        raise JacError("jac must be 'reference', 'exact' or 'exact_tangent', not %r" % (jac,))
    return jac


MARGINAL_JACS = ("reference", "exact_tangent")


def check_marginal_jac(jac):
    if jac not in MARGINAL_JACS:
        raise JacError("the margin's jac must be 'reference' or 'exact_tangent', not %r" % (jac,))
    return jac


def _host(a):
    """a device tensor or a host array as numpy"""
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _flagged(info, any_bit=False):
    """which solves of the info words (sweeps | status << 16; numpy or a device tensor, no synchronisation) failed: status bits 0-1
    (iteration cap, invalid data) for every call whose higher bits are informational (a tie, a cluster, an infinite margin, the
    polish's bits 10-12); any_bit: the lam_max scan and its points have no informational bit, so any status bit fails them."""
    status = info >> 16
    return (status if any_bit else status & 3) != 0


def _check_flags(message, info, any_bit=False):
    """raise IbsError(message % (flagged[, total])) if a solve of the info words failed (one synchronisation for a device tensor)"""
    nbad = int(_host(_flagged(info, any_bit).sum()))
    if nbad:
        raise IbsError(message % (nbad, int(np.prod(info.shape)))[:message.count("%d")])


BOX_LO, BOX_HI = np.array([0.0, 0.0]), np.array([np.pi, 0.5 * np.pi])      # ball_scan.py:311


def _lockstep(evaluate, x0, active, maxiter, ftol, gtol):
    """The host-driven L-BFGS-B of ball_scan.py:307-314 for n points at once: one optimizer state per point (csrc/ibs_lbfgsb2.hpp
    through the C ABI ibs_lbfgsb2_*), advanced in lockstep.  Every round calls evaluate(idx, x[idx]) -> numpy (val (m,), jac (m, 2))
    ONCE, idx being exactly the still-running points in increasing order, then steps each of them; a point's trajectory does not
    depend on the points beside it.  x0 (n, 2) is clipped to the box; points that are not `active` are neither moved nor evaluated.
    Returns dict(x (n, 2), f (n,): the objective at the last accepted iterate, NaN where nothing was evaluated, evals int32 (n,),
    task int32 (n,): the task codes of lbfgsb.TASKS, 10 where nothing was evaluated, rounds = the largest evals)."""
    import ctypes as C
    from . import _lib
    lib = _lib.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)
    x = np.clip(np.asarray(x0, dtype=np.float64).reshape(-1, 2), BOX_LO, BOX_HI)
    n = len(x)
    states = [C.create_string_buffer(lib.ibs_lbfgsb2_state_bytes()) for _ in range(n)]
    for k in range(n):
        lib.ibs_lbfgsb2_init(states[k], p(x[k]), p(BOX_LO), p(BOX_HI), float(ftol), float(gtol), int(maxiter), 20)
    active = np.array(active, dtype=bool)
    f, evals, task = np.full(n, np.nan), np.zeros(n, dtype=np.int32), np.full(n, 10, dtype=np.int32)
    rounds = 0
    while active.any():
        idx = np.nonzero(active)[0]
        val, jac = evaluate(idx, x[idx])
        rounds += 1
        evals[idx] += 1
        for q, k in enumerate(idx):
            gk = np.ascontiguousarray(jac[q], dtype=np.float64)
            if not lib.ibs_lbfgsb2_step(states[k], float(val[q]), p(gk), p(x[k])):
                active[k] = False
    for k in np.nonzero(evals)[0]:
        fk = C.c_double(0.0); cnt = np.zeros(5, dtype=np.int32)
        lib.ibs_lbfgsb2_result(states[k], p(x[k]), C.byref(fk), p(cnt))
        f[k], task[k] = fk.value, cnt[2]
    return dict(x=x, f=f, evals=evals, task=task, rounds=rounds)


class BallooningScan:
    """Coarse (alpha, theta0) scan -> argmax -> L-BFGS-B refinement -> final solve, per surface.
    eigenpair="max" (the default): every stage returns lam_max's eigenpair (the physical growth rate).  eigenpair="nearest":
    every stage returns the eigenpair nearest upstream's shift, as ball_scan.py's eigs(A, 1, sigma=sigma0) does (utils.py:1597):
    sigma = 1.0 in the coarse scan, 1.3 |gam| + 0.05 of the surface's coarse maximum in the refinement, 0.42 in the final solve.
    The two agree wherever lam_max lies below the shifts; on strongly driven surfaces they differ.
    jac="reference" (the default): the refinement runs on upstream's Hellmann-Feynman gradient (utils.py:1676-1680, 1721-1725), which
    puts gam in place of lam and is 0.1-5 % off the gam it comes with.  jac="exact": it runs on the exact derivative of that gam,
    batched on the device (ibs_obj_w_grad_exact_f64), for either eigenpair; the coarse scan and the final solve are the same.
    That derivative is exact in theta0 and, in alpha, the reference's central difference of the rows over del_alpha (three lines per
    point).  jac="exact_tangent" (tables= and device= required, else IbsError: upstream's callback has no tangent): exact in alpha as
    well, from ONE line per point -- every round is one forward geometry launch, one alpha-tangent launch
    (ibs_fieldline_geometry_dalpha_f64) and one point launch (ibs_obj_w_grad_exact_tangent_f64); del_alpha plays no part.
    certify=True (eigenpair="max" only; "nearest" already runs in division form with its a-priori bound: ValueError): every eigenvalue
    of the coarse scan's table is certified by a division-form Sturm count pair at lam +- 4 N eps ||A|| and re-closed in division form
    where the pair refuses it (Context.certify_scan / reclose_scan), the per-surface maximum is then taken again from the table
    (surface_argmax_pack), and the final solves are certified and re-closed the same way.  The solves inside the refinement's objective
    are NOT certified: they only steer the optimizer, and the final solve at its end point is what is reported.  The counts of the
    last run are in .last_certificate = dict(checked, reclosed, failed); failed > 0 raises IbsError.  certify=False (the default)
    adds no call and no keyword to any call.
    n_starts=K > 1: every surface is refined from the K best peaks of its coarse table (pick_starts / ibs_scan_peaks_f64: local
    maxima over the eight neighbours, ranked by value; slot 0 is the first maximum, upstream's one start) and the best refined
    candidate is reported, slot 0 winning ties -- a narrow basin whose crest lies between nodes can rank below the first maximum in
    the table and still hold the surface's maximum.  All n K points run through the refinement and the final solve in one batch; a
    surface with fewer than K peaks repeats slot 0 in the remaining slots (duplicated work, never preferred by the first-maximum
    rule).  .last_candidates (n_own, K, 3) = (theta0, alpha, gam) of every slot and .last_peaks = dict(index, value (n_own, K),
    n_found (n_own,)) describe the last run (device tensors on the device path, not synchronised).  n_starts changes two steps of
    device_rows() only: how the starts are picked and how the rows are selected from the candidates.
    theta0_polish=True (tables= and device= only, n_starts=1, eigenpair="max"; else ValueError): after the coarse scan every line's
    growth rate is maximised over theta0 between the nodes (Context.theta0_polish, one call with one slot per line, on the lines
    the scan staged: no geometry launch), and every surface's refinement starts from its best polished (alpha_i, theta0*) in place of
    the best node; refine=False rows report that point and its value.  .last_envelope holds that call's outputs (device tensors).
    Every mode runs the one sequence of device_rows(); tools/bitwise_vs_parent.py --parent-scan compares a rewrite of this file with
    the one it replaces, Context call by Context call and bit by bit."""

    def __init__(self, ctx, fieldlines, theta, rho_arr, nalpha=24, ntheta0=15, del_alpha=0.004,
                 rank=0, world=1, dist=None, gather_device=None, tables=None, device=None, surf_index=None, eigenpair="max",
                 jac="reference", certify=False, n_starts=1, theta0_polish=False):
        """fieldlines: host geometry callable (see module docstring), or None together with
        tables=SurfaceTables (row F1): then the geometry is produced on `device` by the HIP geometry kernel and consumed
        there -- coarse scan, per-surface maximum, start points, refinement and final solve all stay in HBM and ONE small
        copy returns the rows.  surf_index[k] = index of surface k (of rho_arr) in `tables`; default: the surface of
        tables.s nearest to rho_arr[k].  Table sets that hold several equilibria (SurfaceTables.from_wouts: s repeats
        per equilibrium) need the explicit index.
        eigenpair: "max" or "nearest" (anything else raises ValueError); jac: "reference", "exact" or "exact_tangent" (see the class
        docstring; anything else raises IbsError, which is a ValueError too); n_starts: an integer in [1, 16] (else ValueError)."""
        self.n_starts = check_n_starts(n_starts)
        self.last_candidates = self.last_peaks = None
        self.theta0_polish = bool(theta0_polish)
        self.last_envelope = self.last_marginal_envelope = None
        if self.theta0_polish:
            if tables is None or device is None:
                raise ValueError("theta0_polish=True runs on the resident path: tables= and device= are required")
            if self.n_starts != 1:
                raise ValueError("theta0_polish=True takes n_starts=1")
            if eigenpair == "nearest":
                raise ValueError("theta0_polish=True maximises lam_max's growth rate: eigenpair='nearest' is not supported")
        self.eigenpair = check_eigenpair(eigenpair)
        self.nearest = eigenpair == "nearest"
        self.jac = check_jac(jac)
        self.tangent = jac == "exact_tangent"
        self.exact = jac == "exact" or self.tangent        # (the host-driven refinement on ibs_obj_w_grad_exact*_f64)
        if self.tangent and (tables is None or device is None):
            raise IbsError("jac='exact_tangent' needs tables= and device=: a host geometry callable has no alpha-tangent")
        self.certify = bool(certify)
        if self.certify and self.nearest:
            raise ValueError("certify=True applies to eigenpair='max': eigenpair='nearest' runs in division form with its a-priori bound")
        self.last_certificate = None
        self.ctx = ctx
        self.tables = tables
        self.device = device
        self._resident = {}
        if tables is not None:
            fieldlines = self._device_fieldlines_host
        self.fieldlines = fieldlines
        self.theta = np.asarray(theta, dtype=np.float64)
        self.h = float((self.theta[-1] - self.theta[0]) / (len(self.theta) - 1))
        self.rho_arr = np.asarray(rho_arr, dtype=np.float64)               # ball_scan.py:197
        self.alpha_scan = np.linspace(0, np.pi, nalpha)                    # ball_scan.py:226
        self.theta0_scan = np.linspace(0.0, 0.5 * np.pi, ntheta0)          # ball_scan.py:225
        self.del_alpha = del_alpha
        self.rank, self.world, self.dist, self.gather_device = rank, world, dist, gather_device
        self._native_gather = world > 1 and getattr(ctx, "_comm_world", 0) == world
        self.own = shard_surfaces(len(self.rho_arr), rank, world)
        if tables is not None:
            if surf_index is None:
                surf_index = [int(np.argmin(np.abs(tables.s - r))) for r in self.rho_arr]
            self.surf_index = np.asarray(surf_index, dtype=np.int32)
            if self.surf_index.shape != self.rho_arr.shape or (len(self.surf_index) and (
                    self.surf_index.min() < 0 or self.surf_index.max() >= len(tables.s))):
                raise IbsError("surf_index must give one table index in [0, %d) per surface" % len(tables.s))

    def _own_surf(self):
        """table indices of the surfaces this rank owns"""
        return self.surf_index[np.asarray(self.own, dtype=np.int64)] if len(self.own) else np.zeros(0, dtype=np.int32)

    def _device_fieldlines_host(self, s, alphas):
        """geometry kernel behind the host-callable interface (used by the final solve / tests)"""
        js = int(np.argmin(np.abs(self.tables.s - s)))
        alphas = np.atleast_1d(np.asarray(alphas, dtype=np.float64))
        r = self.ctx.fieldline_geometry(self.tables, [js] * len(alphas), alphas, self.theta)
        return np.ascontiguousarray(np.transpose(r["geo"], (1, 0, 2)))

    @property
    def _on_device(self):
        """the resident path: geometry by the HIP kernel from `tables`, consumed on `device`"""
        return self.tables is not None and self.device is not None

    def _coarse_lines(self, want_t0=True):
        """The lines of the coarse alpha grid of the owned surfaces (at least one), surface-major, in the memory kind of the path --
        device tensors on the resident path (ONE geometry launch), numpy from the fieldlines callback: dict(geo: the 8 planes
        ((8, n_lines, N) resident, (n_lines, 8, N) callback), geo7: the seven planes a solve takes, dP (ball_scan.py:262 with the
        callback), t0: the coarse theta0 grid, and the host maps surf (resident only: the table index) and alpha of every line).
        want_t0=False: no t0 and no upload of it (the local-equilibrium calls fold at their own theta0).  device_rows() does not
        come here: its lines are chunk ranges of the cached device maps of _resident_inputs(), between two marks of its phase timer."""
        na, n = len(self.alpha_scan), len(self.own)
        alpha = np.tile(self.alpha_scan, n)
        if not self._on_device:
            geo = np.concatenate([np.asarray(self.fieldlines(self.rho_arr[k], self.alpha_scan)) for k in self.own], axis=0)
            dP = -0.5 * np.mean((geo[:, 2] - geo[:, 7]) * geo[:, 0] ** 2, axis=1)   # ball_scan.py:262
            return dict(geo=geo, geo7=[np.ascontiguousarray(geo[:, k]) for k in range(7)], dP=dP, t0=self.theta0_scan, alpha=alpha)
        surf = np.repeat(self._own_surf(), na)
        r = self.ctx.fieldline_geometry(self.tables, surf, alpha, self.theta, device=self.device)
        lines = dict(geo=r["geo"], geo7=[r["geo"][k] for k in range(7)], dP=r["dPdrho"], surf=surf, alpha=alpha)
        if want_t0:
            import torch
            lines["t0"] = torch.from_numpy(self.theta0_scan).to(self.device)
        return lines

    def _line_sigma(self, surf):
        """sigma = sign(-phiedge) of the surface of every line (surf: table indices), the sign the local-equilibrium fold takes"""
        return np.sign(-np.asarray(self.tables.scal)[surf, 4])

    # -- A5: coarse scan of the surfaces this rank owns, one launch
    def coarse(self):
        na, nt = len(self.alpha_scan), len(self.theta0_scan)
        if not self.own:
            self._coarse_cert = np.zeros(0, dtype=np.int32)
            return np.zeros((0, na, nt))
        ln = self._coarse_lines()
        # device-pointer calls are asynchronous and return no count of flagged systems: there the info words are read
        kw = dict(want_info=True) if self._on_device else {}
        if self.nearest:
            out = self.ctx.gamma_scan_nearest(self.h, *ln["geo7"], ln["dP"], ln["t0"], SIGMA_COARSE, **kw)
        else:
            out = self.ctx.gamma_scan(self.h, *ln["geo7"], ln["dP"], ln["t0"], **kw, **self._certify_kw())
        if self._on_device:
            _check_flags("%d of %d coarse-scan solves were flagged (status word != 0: invalid data or iteration cap)", out["info"],
                         any_bit=not self.nearest)
        elif out.get("nbad", 0):
            raise IbsError("%d coarse-scan solves were flagged (status word != 0: invalid data or iteration cap)" % out["nbad"])
        if self.certify:
            self._coarse_cert = out["cert"]
        return _host(out["gam"]).reshape(len(self.own), na, nt)

    def _certify_kw(self):
        """keyword of the solver calls: nothing at all without certify"""
        return dict(certify=True) if self.certify else {}

    # -- unstable modes on the coarse grid of the surfaces this rank owns, one launch
    def mode_count(self, shift=0.0):
        """the number of eigenvalues above `shift` of every (alpha, theta0) of the coarse grid, int (n_own, nalpha, ntheta0)
        (Context.geo_sturm_count: at shift 0 the number of unstable modes, bishop_ball_s-alpha.py:110-115 for real field lines)"""
        na, nt = len(self.alpha_scan), len(self.theta0_scan)
        if not self.own:
            return np.zeros((0, na, nt), dtype=np.int32)
        ln = self._coarse_lines()
        cnt = self.ctx.geo_sturm_count(self.h, *ln["geo7"], ln["dP"], ln["t0"], shift)
        return _host(cnt).reshape(len(self.own), na, nt)

    # -- the s-alpha picture of the owned surfaces: shear and pressure variations of every line of the alpha grid, two launches
    def local_eq(self, eps, p, theta0=None, shift=0.0, count_only=False):
        """gam, lam_max and the number of eigenvalues above `shift` of every line of the alpha grid of every owned surface under the
        relative changes eps (n_eps,) of the surface's global shear and the factors p (n_p,) on its pressure gradient, folded at
        theta0 (n_theta0,; default: the coarse theta0 grid), by the rule of operators.local_eq_fold with centre = alpha, sigma =
        sign(-phiedge) of the tables and no ps row -- the geometry re-evaluated with d_iota_d_s (1 + eps) and d_pressure_d_s p, at
        frozen local shear on the pressure axis.  Resident path only (tables= and device=, else ValueError): ONE geometry launch and
        ONE Context.local_eq_scan call.  Returns numpy dict(gam, lam, count (n_own, nalpha, n_theta0, n_eps, n_p), gam_max, unstable
        (n_own, n_eps, n_p) = the envelope over (alpha, theta0): the largest gam and "some line has an eigenvalue above shift";
        theta0, eps, p).  count_only=True: count and unstable alone, no eigenvalue is computed.  Flagged solves raise IbsError."""
        if not self._on_device:
            raise ValueError("local_eq() runs on the resident path: tables= and device= are required")
        eps = np.atleast_1d(np.asarray(eps, dtype=np.float64))
        p = np.atleast_1d(np.asarray(p, dtype=np.float64))
        t0 = self.theta0_scan if theta0 is None else np.atleast_1d(np.asarray(theta0, dtype=np.float64))
        na, n = len(self.alpha_scan), len(self.own)
        shape = (n, na, len(t0), len(eps), len(p))
        var = np.stack([a.ravel() for a in np.meshgrid(t0, eps, p, indexing="ij")], axis=1)
        keys = ("count",) if count_only else ("gam", "lam", "count")
        res = dict(theta0=t0, eps=eps, p=p)
        if n:
            ln = self._coarse_lines(want_t0=False)
            out = self.ctx.local_eq_scan(self.theta[0], self.h, ln["geo"], ln["dP"], ln["alpha"], self._line_sigma(ln["surf"]), var, shift=shift,
                                         count_only=count_only, want_info=True)
            _check_flags("%d of %d local-equilibrium solves were flagged (status bits 0-1: iteration cap or invalid data)", out["info"])
            res.update({k: out[k].cpu().numpy().reshape(shape) for k in keys})
        else:
            res.update({k: np.zeros(shape, dtype=np.int32 if k == "count" else np.float64) for k in keys})
        res["unstable"] = (res["count"] > 0).any(axis=(1, 2))
        if not count_only:
            res["gam_max"] = res["gam"].max(axis=(1, 2))
        return res

    # -- the boundaries of that picture: marginal pressure factor (or shear change) of every line of the alpha grid, two launches
    def local_eq_boundary(self, fixed, t_range, theta0=None, axis="p", shift=0.0, max_cross=4, xtol=1e-12):
        """Where every line of the alpha grid of every owned surface crosses the stability boundary ("an eigenvalue above `shift`")
        along one axis of the (eps, p) plane of local_eq(), closed on the device (Context.local_eq_boundary).
            axis="p":   fixed = the relative shear changes eps (n_fixed,), t_range = (p_lo, p_hi): a ray runs along the pressure factor
                        p at each eps -- the marginal pressure gradient at each shear
            axis="eps": fixed = the pressure factors p (n_fixed,), t_range = (eps_lo, eps_hi): a ray runs along eps at each p
        with the rule of local_eq (centre = alpha, sigma = sign(-phiedge), no ps row), folded at theta0 (n_theta0,; default: the coarse
        theta0 grid); the ray parameter t IS the running coordinate.  Resident path only (tables= and device=, else ValueError): ONE
        geometry launch and ONE boundary call.  Returns numpy dict(t_stable, t_unstable, t (n_own, nalpha, n_theta0, n_fixed,
        max_cross), NaN beyond n_cross; n_cross, lo_unstable, info (n_own, nalpha, n_theta0, n_fixed); first_unstable (n_own,
        n_fixed) = the envelope over (alpha, theta0): the smallest t at which any line of the surface crosses from stable to unstable,
        +inf where none does, t_lo where some line is unstable at t_lo already -- the surface's first-stability limit; theta0, fixed,
        t_range, axis).  A crossing is a change of verdict between two of 64 equidistant nodes of t_range: a tangency and two
        crossings between one pair of nodes are missed.  Flagged systems (status bits 0-1) raise IbsError."""
        if not self._on_device:
            raise ValueError("local_eq_boundary() runs on the resident path: tables= and device= are required")
        return self._local_eq_boundary(fixed, t_range, theta0, axis, shift, max_cross, xtol)[0]

    def _local_eq_boundary(self, fixed, t_range, theta0, axis, shift, max_cross, xtol):
        """local_eq_boundary() on the resident path -> (its dict, the coarse lines it ran on (None without an owned surface), the ray
        families (n_fixed, 7) of local_eq_boundary_envelope: the rays of one theta0 with entry 0 zeroed)"""
        if axis not in ("p", "eps"):
            raise ValueError("axis must be 'p' or 'eps', not %r" % (axis,))
        fixed = np.atleast_1d(np.asarray(fixed, dtype=np.float64))
        t_lo, t_hi = (float(v) for v in t_range)
        t0 = self.theta0_scan if theta0 is None else np.atleast_1d(np.asarray(theta0, dtype=np.float64))
        na, n = len(self.alpha_scan), len(self.own)
        shape = (n, na, len(t0), len(fixed))
        tt, ff = (a.ravel() for a in np.meshgrid(t0, fixed, indexing="ij"))
        zero, one = np.zeros_like(ff), np.ones_like(ff)
        cols = (tt, ff, zero, zero, one) if axis == "p" else (tt, zero, ff, one, zero)
        rays = np.stack([*cols, np.full_like(ff, t_lo), np.full_like(ff, t_hi)], axis=1)
        res = dict(theta0=t0, fixed=fixed, t_range=(t_lo, t_hi), axis=axis)
        if n:
            ln = self._coarse_lines(want_t0=False)
            out = self.ctx.local_eq_boundary(self.theta[0], self.h, ln["geo"], ln["dP"], ln["alpha"], self._line_sigma(ln["surf"]), rays, shift=shift,
                                             max_cross=max_cross, xtol=xtol, want_info=True)
            _check_flags("%d of %d local-equilibrium boundary systems were flagged (status bits 0-1: pass cap or invalid data)",
                         out["info"])
            res.update({k: out[k].cpu().numpy().reshape(shape + (max_cross,)) for k in ("t_stable", "t_unstable", "t")})
            res.update({k: out[k].cpu().numpy().reshape(shape) for k in ("n_cross", "lo_unstable", "info")})
        else:
            res.update({k: np.full(shape + (max_cross,), np.nan) for k in ("t_stable", "t_unstable", "t")})
            res.update({k: np.zeros(shape, dtype=np.int32) for k in ("n_cross", "lo_unstable", "info")})
        res["first_unstable"] = first_unstable(res["t_stable"], res["t_unstable"], res["lo_unstable"], t_lo)
        fam = rays[:len(fixed)].copy()
        fam[:, 0] = 0.0
        return res, (ln if n else None), fam

    # -- the boundaries minimised over theta0 between the nodes: the coarse boundary call, then one polish call on the same lines
    def local_eq_boundary_envelope(self, fixed, t_range, theta0=None, axis="p", shift=0.0, n_starts=1, xtol=1e-12, xtol_theta0=1e-5,
                                   max_eval=32):
        """local_eq_boundary(fixed, t_range, theta0, axis, shift, xtol=xtol) with every line's first-stability parameter T = the first
        crossing from stable to unstable (local_eq_first_up) then MINIMISED over theta0 between the nodes of the theta0 grid
        (Context.local_eq_boundary_polish; the rule: polish_first_up): the envelope over theta0 that the boundary of an s-alpha picture
        is by convention, at the coarse alpha values.  Resident path only (tables= and device=, else ValueError): ONE geometry launch,
        ONE boundary call for the coarse rows and ONE polish call about the n_starts <= 4 best nodes of every (line, fixed value) row.
        Returns local_eq_boundary's dict plus theta0_env, t_env (n_own, nalpha, n_fixed, n_starts), node, n_eval, lo_unstable_env int32 of
        that shape, n_found (n_own, nalpha, n_fixed); first_unstable_env (n_own, n_fixed) = the smallest t_env over (alpha, slot) of every
        surface, t_lo where some line is unstable at t_lo, +inf where none crosses -- never above first_unstable; at (n_own, n_fixed, 2) =
        (alpha, theta0*) of the attaining slot, the first in (alpha, slot) order.  Wherever no slot beat its node t_env is the coarse
        call's T.  Flagged systems (status bits 0-1) raise IbsError."""
        if not self._on_device:
            raise ValueError("local_eq_boundary_envelope() runs on the resident path: tables= and device= are required")
        if isinstance(n_starts, bool) or not isinstance(n_starts, (int, np.integer)) or not 1 <= n_starts <= MAX_ROW_STARTS:
            raise ValueError("n_starts must be an integer in [1, %d], not %r" % (MAX_ROW_STARTS, n_starts))
        K = int(n_starts)
        res, ln, fam = self._local_eq_boundary(fixed, t_range, theta0, axis, shift, 4, xtol)
        t0, t_lo = res["theta0"], res["t_range"][0]
        na, n, nf = len(self.alpha_scan), len(self.own), len(res["fixed"])
        slots = (n, na, nf, K)
        if n:
            T = local_eq_first_up(res["t_stable"], res["t_unstable"], res["lo_unstable"], t_lo)      # (n, nalpha, n_theta0, n_fixed)
            t_row = np.ascontiguousarray(np.moveaxis(T, 2, 3)).reshape(n * na, nf, len(t0))
            out = self.ctx.local_eq_boundary_polish(self.theta[0], self.h, ln["geo"], ln["dP"], ln["alpha"], self._line_sigma(ln["surf"]), fam,
                                                    t0, t_row, shift=shift, xtol=xtol, n_starts=K, xtol_theta0=xtol_theta0,
                                                    max_eval=max_eval, want_info=True)
            _check_flags("%d of %d slots of the local-equilibrium boundary envelope were flagged (status bits 0-1: pass cap or invalid data)",
                         out["info"])
            env = {k: _host(out[k]).reshape(slots) for k in ("theta0", "t", "node", "n_eval", "lo_unstable")}
            n_found = _host(out["n_found"]).reshape(n, na, nf)
        else:
            env = dict(theta0=np.zeros(slots), t=np.zeros(slots), node=np.zeros(slots, np.int32), n_eval=np.zeros(slots, np.int32),
                       lo_unstable=np.zeros(slots, np.int32))
            n_found = np.zeros((n, na, nf), np.int32)
        flat = np.moveaxis(np.where(np.isnan(env["t"]), np.inf, env["t"]), 2, 1).reshape(n, nf, na * K)
        arg = flat.argmin(axis=2)                                               # (first minimum in (alpha, slot) order)
        rows, cols = np.arange(n)[:, None], np.arange(nf)[None, :]
        th_at = np.moveaxis(env["theta0"], 2, 1).reshape(n, nf, na * K)[rows, cols, arg]
        res.update(theta0_env=env["theta0"], t_env=env["t"], node=env["node"], n_eval=env["n_eval"], lo_unstable_env=env["lo_unstable"],
                   n_found=n_found, first_unstable_env=flat[rows, cols, arg], at=np.stack([self.alpha_scan[arg // K], th_at], axis=2))
        return res

    # -- the first-stability limit of that picture with its exact derivatives: the boundary call, then one point launch and one geometry VJP
    def local_eq_boundary_sensitivity(self, fixed, t_range, theta0=None, axis="p", shift=0.0, theta0_polish=False):
        """first_unstable of local_eq_boundary(fixed, t_range, theta0, axis, shift) for every owned surface and fixed value, with its exact
        derivatives with respect to the fixed value, the shift and the surface's own tables.  Resident path only (tables= and device=,
        else ValueError).  The derivatives are taken at the (alpha, theta0) of the coarse grid that ATTAINS the minimum (the first one in
        (alpha, theta0, crossing) order): the envelope over a DISCRETE set of lines, C1 only where the attaining line does not switch.
        There t* solves lam_max(t*) = shift on that line and the implicit-function rule gives d t* / d (.) = -lam_(.) / lam_t, with the
        derivatives of lam_max from one point launch (autograd.local_eq_lam, ibs_local_eq_grad_f64) on a fresh geometry launch in which
        every (surface, fixed value) works on its own copy of the surface's tables, and one geometry-VJP launch.  The rule is
        local_eq()'s: frozen local shear on the pressure axis, no ps row.  lam_max must be simple; a near-tangency shows as a small
        dlam_dt.  Where some line is unstable at t_lo already, or none crosses, the derivatives are zero and mask is False.
        theta0_polish=True: the limit is first_unstable_env of local_eq_boundary_envelope(fixed, t_range, theta0, axis, shift) and the
        derivatives are taken at its polished (alpha, theta0*) = `at` in place of the best node; at an interior theta0* the envelope
        theorem holds in theta0 (d t* / d theta0 = 0 there), so the derivatives are those of the envelope over theta0 at that alpha.  The
        dict is then local_eq_boundary_envelope's plus the keys below.
        Returns local_eq_boundary's dict plus numpy mask (bool), alpha, theta0_at, lam_at, dlam_dt, dfirst_dfixed, dfirst_dshift: (n_own,
        n_fixed); and device tensors tab_mn_bar (n_own, n_fixed, 6, mnmax), tab_nyq_bar (n_own, n_fixed, 7, mnmax_nyq), scal_bar (n_own,
        n_fixed, 6) = d first_unstable / d tables, in the layout of marginal_sensitivity per fixed value (SurfaceTables.pullback carries
        them to the wout arrays)."""
        import torch
        from . import autograd as iag
        if not self._on_device:
            raise ValueError("local_eq_boundary_sensitivity() runs on the resident path: tables= and device= are required")
        dev, own = self.device, self._own_surf()
        if theta0_polish:
            res = self.local_eq_boundary_envelope(fixed, t_range, theta0=theta0, axis=axis, shift=shift)
            t0, fx = res["theta0"], res["fixed"]
            n, nf, na = len(own), len(fx), len(self.alpha_scan)
            best, al_at, th_at = res["first_unstable_env"], res["at"][:, :, 0], res["at"][:, :, 1]
            mask = np.isfinite(best) & ~(res["lo_unstable"] > 0).any(axis=(1, 2)) & ~(res["lo_unstable_env"] > 0).any(axis=(1, 3))
        else:
            res = self.local_eq_boundary(fixed, t_range, theta0=theta0, axis=axis, shift=shift)
            t0, fx = res["theta0"], res["fixed"]
            n, nf, na = len(own), len(fx), len(self.alpha_scan)
            cand = np.where(res["t_stable"] < res["t_unstable"], res["t"], np.inf)      # (n, nalpha, n_theta0, n_fixed, max_cross)
            flat = np.moveaxis(cand, 3, 1).reshape(n, nf, -1)
            arg = flat.argmin(axis=2) if flat.shape[2] else np.zeros((n, nf), dtype=np.int64)
            ia, it, _ = np.unravel_index(arg, (na, len(t0), cand.shape[4]))
            best = flat.min(axis=2, initial=np.inf)
            mask = np.isfinite(best) & ~(res["lo_unstable"] > 0).any(axis=(1, 2))
            al_at, th_at = self.alpha_scan[ia], t0[it]
        out = {k: np.zeros((n, nf)) for k in ("alpha", "theta0_at", "lam_at", "dlam_dt", "dfirst_dfixed", "dfirst_dshift")}
        d = self.ctx._device_tables(self.tables, dev)
        bars = [torch.zeros((n, nf) + tuple(d[k].shape[1:]), dtype=torch.float64, device=dev) for k in (4, 5, 6)]
        q, k = np.nonzero(mask)
        if len(q):
            al, th0, ts = al_at[q, k], th_at[q, k], best[q, k]
            var = np.stack([th0, fx[k], ts] if axis == "p" else [th0, ts, fx[k]], axis=1)
            idx = torch.from_numpy(own[q].astype(np.int64)).to(dev)
            tm, tq, sc = (d[j][idx].clone().requires_grad_(True) for j in (4, 5, 6))
            pts = torch.arange(len(q), dtype=torch.int32, device=dev)
            geo, dP = iag.fieldline_geometry(self.tables, pts, torch.from_numpy(np.ascontiguousarray(al)).to(dev), self._resident_inputs()["th"],
                                             tab_mn=tm, tab_nyq=tq, scal=sc, ctx=self.ctx)
            v = torch.from_numpy(var).to(dev).requires_grad_(True)
            lam = iag.local_eq_lam(self.theta[0], self.h, geo, dP, al, self._line_sigma(own[q]), pts, v, ctx=self.ctx)
            lam.sum().backward()
            lv = v.grad.cpu().numpy()
            lam_t, lam_f = (lv[:, 2], lv[:, 1]) if axis == "p" else (lv[:, 1], lv[:, 2])
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = 1.0 / lam_t
            out["alpha"][q, k], out["theta0_at"][q, k], out["lam_at"][q, k], out["dlam_dt"][q, k] = al, th0, lam.detach().cpu().numpy(), lam_t
            out["dfirst_dfixed"][q, k], out["dfirst_dshift"][q, k] = -lam_f * inv, inv
            w = torch.from_numpy(-inv).to(dev)
            for bar, x in zip(bars, (tm, tq, sc)):
                bar[torch.from_numpy(q).to(dev), torch.from_numpy(k).to(dev)] = x.grad * w.reshape((-1,) + (1,) * (x.grad.dim() - 1))
        res.update(out, mask=mask, tab_mn_bar=bars[0], tab_nyq_bar=bars[1], scal_bar=bars[2])
        return res

    # -- every line's growth rate maximised over theta0 between the nodes of the coarse grid, two launches
    def envelope(self, n_starts=1, xtol=1e-5, max_eval=32):
        """gam_env(alpha) = max over theta0 of gam(alpha, theta0) of every line of the coarse grid: the coarse scan, then
        Context.theta0_polish about the n_starts <= 4 best peaks of every line's row (Brent between the nodes on the staged line:
        no geometry launch beyond the coarse scan's).  Returns numpy dict(theta0, gam, node, n_eval (n_own, nalpha, n_starts),
        n_found (n_own, nalpha), surface (n_own, 3) = (theta0*, alpha, gam) of the best slot of every surface, first maximum in
        (alpha, slot) order).  gam is never below the coarse row, so surface[:, 2] bounds the coarse maximum from above.
        eigenpair="nearest" is refused (ValueError): that mode's gam is not lam_max's.  Flagged solves (status bits 0-1) raise."""
        if self.nearest:
            raise ValueError("envelope() maximises lam_max's growth rate: eigenpair='nearest' is not supported")
        if isinstance(n_starts, bool) or not isinstance(n_starts, (int, np.integer)) or not 1 <= n_starts <= MAX_ROW_STARTS:
            raise ValueError("n_starts must be an integer in [1, %d], not %r" % (MAX_ROW_STARTS, n_starts))
        K = int(n_starts)
        if not self.own:
            return self._envelope_rows(None, K, ("theta0", "gam"), "gam", "gam")
        ln = self._coarse_lines()
        sc = self.ctx.gamma_scan(self.h, *ln["geo7"], ln["dP"], ln["t0"], want_info=True)
        out = self.ctx.theta0_polish(self.h, *ln["geo7"], ln["dP"], ln["t0"], sc["gam"], n_starts=K, xtol=xtol, max_eval=max_eval,
                                     lam=sc["lam"], want_info=True)
        nbad = int(_flagged(_host(sc["info"]), any_bit=True).sum()) + int(_flagged(_host(out["info"])).sum())
        if nbad:
            raise IbsError("%d solves of the envelope were flagged (status bits 0-1: iteration cap or invalid data)" % nbad)
        return self._envelope_rows(out, K, ("theta0", "gam"), "gam", "gam")

    def _envelope_rows(self, out, K, keys, rank, value):
        """the result of a theta0 polish call `out` with K slots per line of the coarse grid (None: no owned surface) as numpy:
        out's float arrays `keys`, node and n_eval as (n_own, nalpha, K), n_found (n_own, nalpha), and surface (n_own, 3) = (theta0*,
        alpha, out[value]) of the slot with the largest out[rank] of every surface (NaN ranks last), first maximum in (alpha, slot)
        order"""
        n, na = len(self.own), len(self.alpha_scan)
        if out is None:
            z = np.zeros((0, na, K))
            return dict({k: z.copy() for k in keys}, node=z.astype(np.int32), n_eval=z.astype(np.int32),
                        n_found=np.zeros((0, na), np.int32), surface=np.zeros((0, 3)))
        res = {k: _host(out[k]).reshape(n, na, K) for k in keys + ("node", "n_eval")}
        res["n_found"] = _host(out["n_found"]).reshape(n, na)
        flat = np.where(np.isnan(res[rank]), -np.inf, res[rank]).reshape(n, na * K)
        best = np.argmax(flat, axis=1)                                           # (first maximum)
        rows = np.arange(n)
        res["surface"] = np.stack([res["theta0"].reshape(n, -1)[rows, best], self.alpha_scan[best // K],
                                   res[value].reshape(n, -1)[rows, best]], axis=1)
        return res

    # -- the top of the spectrum on the coarse grid of the surfaces this rank owns, one launch
    def modes(self, n_modes):
        """the n_modes largest eigenvalues and their growth rates of every (alpha, theta0) of the coarse grid (Context.gamma_scan_modes,
        1 <= n_modes <= 16): dict(lam, gam, cluster), each (n_own, nalpha, ntheta0, n_modes), mode 0 = lam_max's; cluster (bool): a
        neighbouring eigenvalue lies within 4 N eps ||A|| -- lam holds, gam is the quotient of some vector of the cluster.  The modes
        mode_count() counts: (lam > 0).sum(-1) == min(n_modes, mode_count()).  Flagged solves (status bits 0-1) raise IbsError."""
        na, nt = len(self.alpha_scan), len(self.theta0_scan)
        if not self.own:
            z = np.zeros((0, na, nt, int(n_modes)))
            return dict(lam=z, gam=z.copy(), cluster=z.astype(bool))
        ln = self._coarse_lines()
        out = self.ctx.gamma_scan_modes(self.h, *ln["geo7"], ln["dP"], ln["t0"], n_modes, want_info=True)
        out = {k: _host(out[k]) for k in ("lam", "gam", "info")}
        _check_flags("%d of %d modes of the coarse grid were flagged (status bits 0-1: iteration cap or invalid data)", out["info"])
        shape = (len(self.own), na, nt, -1)
        return dict(lam=out["lam"].reshape(shape), gam=out["gam"].reshape(shape),
                    cluster=(((out["info"] >> 16) & CLUSTER_BIT) != 0).reshape(shape))

    # -- marginal stability on the coarse grid of the surfaces this rank owns, one launch
    def _marginal_coarse(self):
        """the coarse table of marginal(): dict(tab (n_own, nalpha, ntheta0) numpy, and -- for the calls that follow on the same lines
        -- geo7, dP, t0 and the scan's mu in the memory kind of the path: device tensors or numpy)"""
        na, nt = len(self.alpha_scan), len(self.theta0_scan)
        if not self.own:
            return dict(tab=np.zeros((0, na, nt)))
        ln = self._coarse_lines()
        if self._on_device:
            out = self.ctx.marginal_scan(self.h, *ln["geo7"], ln["dP"], ln["t0"], want_info=True)
            _check_flags("%d of %d marginal-stability solves were flagged (status bits 0-1: iteration cap or invalid data)", out["info"])
        else:
            out = self.ctx.marginal_scan(self.h, *ln["geo7"], ln["dP"], ln["t0"])
            if out.get("nbad", 0):
                raise IbsError("%d marginal-stability solves were flagged (status bits 0-1: iteration cap or invalid data)" % out["nbad"])
        return dict(tab=_host(out["scale"]).reshape(len(self.own), na, nt), geo7=ln["geo7"], dP=ln["dP"], t0=ln["t0"], mu=out["mu"])

    def _marginal_envelope(self, co, K, xtol, max_eval):
        """marginal_envelope() on the coarse scan co (_marginal_coarse): the one polish call and its per-surface best slot"""
        keys = ("theta0", "mu", "scale")
        if not self.own:
            return self._envelope_rows(None, K, keys, "mu", "scale")
        out = self.ctx.marginal_theta0_polish(self.h, *co["geo7"], co["dP"], co["t0"], co["mu"], n_starts=K, xtol=xtol,
                                              max_eval=max_eval, want_info=True)
        _check_flags("%d solves of the margin's envelope were flagged (status bits 0-1: iteration cap or invalid data)",
                     _host(out["info"]))
        return self._envelope_rows(out, K, keys, "mu", "scale")

    # -- every line's margin maximised over theta0 between the nodes of the coarse grid, two launches
    def marginal_envelope(self, n_starts=1, xtol=1e-5, max_eval=32):
        """mu_env(alpha) = max over theta0 of mu(alpha, theta0) = 1 / s* of every line of the coarse grid, i.e. the line's smallest
        critical scale: the coarse Context.marginal_scan, then Context.marginal_theta0_polish about the n_starts <= 4 best peaks of
        every line's row of mu (Brent between the nodes on the lines the scan read: no geometry launch beyond the coarse scan's), on
        the resident path or with the fieldlines callback.  Returns numpy dict(theta0, mu, scale, node, n_eval (n_own, nalpha,
        n_starts), n_found (n_own, nalpha), surface (n_own, 3) = (theta0*, alpha, s*) of the best slot of every surface, first
        maximum of mu in (alpha, slot) order).  mu is never below the coarse row, so surface[:, 2] is never above the coarse minimum
        of s*.  Flagged solves (status bits 0-1) raise; scale = inf is a result."""
        if isinstance(n_starts, bool) or not isinstance(n_starts, (int, np.integer)) or not 1 <= n_starts <= MAX_ROW_STARTS:
            raise ValueError("n_starts must be an integer in [1, %d], not %r" % (MAX_ROW_STARTS, n_starts))
        return self._marginal_envelope(self._marginal_coarse(), int(n_starts), xtol, max_eval)

    def marginal(self, refine=False, maxiter=30, ftol=5.0e-11, gtol=2.0e-8, jac="reference", n_starts=1, theta0_polish=False):
        """per owned surface, the smallest critical scale s* of dPdrho over the coarse (alpha, theta0) grid and where it sits
        (Context.marginal_scan): dict(scale (n_own,), alpha, theta0, index (n_own, 2) = (i_alpha, i_theta0) of the first minimum,
        table (n_own, nalpha, ntheta0)).  s* < 1: some line of the surface is unstable now; s* scales dPdrho at FIXED geometry
        arrays, so away from 1 it is a local margin.  Raises IbsError on status bits 0-1.
        refine=True: every surface's minimum is refined in (alpha, theta0) from that grid node, as run() refines the growth rate:
        -mu = -1 / s* (finite where no scale makes a line unstable) is minimised over [0, pi] x [0, pi/2] by the L-BFGS-B state
        machines (ibs_lbfgsb2_*) in lockstep, every round ONE batched geometry step + ONE Context.marginal_obj_w_grad launch for the
        surfaces still running, and one more launch at the refined points fills the result.  scale, alpha, theta0 are then the
        refined ones (index and table stay the coarse ones) and the dict gains coarse_scale (n_own,), start (n_own, 2), dscale
        (n_own, 2) = (d s* / d alpha, d s* / d theta0) at the refined point, dPdrho (n_own,) of the refined line, evals (n_own,),
        task (n_own,) = the L-BFGS-B task codes (lbfgsb.TASKS) and rounds.  A surface's refinement does not depend on the surfaces
        refined beside it (the rounds' geometry runs in one form of the geometry kernel: MARGINAL_GEO_LPP).  A surface whose coarse table is all +inf stays at its
        start point with scale = inf and no evaluation (its gradient is 0).
        jac="reference" (the default): the rounds take d s* / d alpha from the del_alpha difference of the rows, three lines per point
        (ibs_marginal_obj_w_grad_f64).  jac="exact_tangent" (tables= and device= required, else
        IbsError; any other value is refused): d s* / d alpha is the derivative, from ONE line per point -- every round is one forward
        geometry launch (in the same pinned form), one alpha-tangent launch (ibs_fieldline_geometry_dalpha_f64) and one point launch
        (ibs_marginal_obj_w_grad_tangent_f64); the dict has the same keys and dscale is then exact in both variables, so the refined
        point is a stationary point of the s* returned (marginal_sensitivity()).  Either mode leaves its (alpha, theta0) per owned
        surface on the object for marginal_sensitivity().
        n_starts=K > 1 (refine=True; K <= 16, else ValueError): every surface is refined from the K best peaks of its table of mu =
        1 / s* (pick_starts' rule: Context.scan_peaks on the resident path, the numpy rule with the callback; slot 0 is the first
        maximum of mu) -- a basin whose crest lies between nodes can rank below the first minimum in the table and still hold the
        surface's margin.  The distinct slots of all surfaces run through the same lockstep loop and ONE final launch; slots from
        n_found on copy slot 0 and are not evaluated; a table whose maximum mu is 0 stays at scale = inf with no evaluation.  The
        winner is the smallest refined scale, slot 0 on ties: scale, alpha, theta0, start, dscale, dPdrho are the winner's, and the
        dict gains candidates (n_own, K, 3) = (scale, alpha, theta0) of every slot and n_found (n_own,); evals and task are then
        (n_own, K).  With refine=False the starts are not used.
        theta0_polish=True (n_starts=1, else ValueError): every line's mu is first maximised over theta0 between the nodes
        (marginal_envelope's polish call on the lines of the coarse scan, one slot per line) and every surface starts at the crest
        of its best line -- marginal_envelope's `surface` -- in place of the best node; refine=False reports that point.  The
        envelope is left in .last_marginal_envelope.
        The calls every combination of these options makes are held to those of the file's previous version by
        tools/bitwise_vs_parent.py --parent-scan."""
        tangent = check_marginal_jac(jac) == "exact_tangent"
        K = check_n_starts(n_starts)
        if theta0_polish and K != 1:
            raise ValueError("theta0_polish=True takes n_starts=1")
        if tangent and not self._on_device:
            raise IbsError("marginal(jac='exact_tangent') needs tables= and device=: a host geometry callable has no alpha-tangent")
        na, nt = len(self.alpha_scan), len(self.theta0_scan)
        co = self._marginal_coarse()
        tab = co["tab"]
        flat = tab.reshape(len(tab), -1)
        k = np.argmin(flat, axis=1) if len(tab) else np.zeros(0, dtype=np.int64)
        ia, it = k // nt, k % nt
        res = dict(scale=flat[np.arange(len(tab)), k], alpha=self.alpha_scan[ia], theta0=self.theta0_scan[it],
                   index=np.stack([ia, it], axis=1), table=tab)
        if theta0_polish:
            env = self.last_marginal_envelope = self._marginal_envelope(co, 1, 1e-5, 32)
            crest = dict(res, scale=env["surface"][:, 2].copy(), alpha=env["surface"][:, 1].copy(), theta0=env["surface"][:, 0].copy())
            if refine:
                res = dict(self._marginal_refine(crest, maxiter, ftol, gtol, tangent), coarse_scale=res["scale"])
            else:
                res = crest
        elif refine and K > 1:
            res = self._marginal_refine_multi(res, co, K, maxiter, ftol, gtol, tangent)
        elif refine:
            res = self._marginal_refine(res, maxiter, ftol, gtol, tangent)
        self._last_marginal_points = np.stack([res["alpha"], res["theta0"]], axis=1).astype(np.float64).reshape(len(tab), 2)
        return res

    # -- the margin's objective at X[q] = (alpha, theta0) of owned surface own_idx[q], all at once: one geometry step (the three
    # lines of every point: the geometry kernel on `device`, staged through the host without one, or the host callable) and one
    # ibs_marginal_obj_w_grad_f64 launch; numpy out.  tangent (jac="exact_tangent"): from ONE line per point -- the points' own
    # lines, their alpha-tangent, then one ibs_marginal_obj_w_grad_tangent_f64 launch
    def _marginal_points(self, own_idx, X, tangent=False):
        # the geometry kernel picks its form from the size of the batch, and the forms differ in the last bits of the rows: left to
        # that, a surface's trajectory (and its refined point, to 1e-10) would depend on how many others run beside it.  One form
        # for every round (pinned) makes the refinement of a surface the same in any batch, bit for bit
        if self.tables is not None:
            geo, geo_da, t0 = self._point_lines(self._own_surf()[own_idx], X, tangent, pinned=True)
        else:
            d = self.del_alpha
            geo = np.stack([np.asarray(self.fieldlines(self.rho_arr[self.own[k]], np.array([a - 0.5 * d, a, a + 0.5 * d])))
                            for a, k in zip(X[:, 0], own_idx)])
            t0 = np.ascontiguousarray(X[:, 1])
        if tangent:
            out = self.ctx.marginal_obj_w_grad_tangent(self.h, geo, geo_da, t0, want_grad=True, want_info=True)
        else:
            out = self.ctx.marginal_obj_w_grad(self.h, geo, t0, self.del_alpha, want_grad=True, want_info=True)
        out = {key: _host(v) for key, v in out.items() if key != "nbad"}
        bad = _flagged(out["info"]) | ~np.isfinite(out["val"]) | ~np.isfinite(out["jac"]).all(axis=1)
        if bad.any():
            raise IbsError("%d of %d marginal-stability solves of the refinement were flagged (status bits 0-1: iteration cap or "
                           "invalid data) or gave a non-finite objective" % (int(bad.sum()), len(own_idx)))
        return out

    def _point_lines(self, surf, X, tangent, pinned=False):
        """the lines of a batch of points X[q] = (alpha, theta0) on the surfaces of table index surf[q], by the geometry kernel: ->
        (geo, geo_da, t0) on `device` (numpy where the scan has tables but no device).  tangent False: the three lines at alpha -
        del_alpha / 2, alpha, alpha + del_alpha / 2 of every point, geo (n, 3, 8, N), geo_da None.  tangent True: the point's own
        line, geo (8, n, N), and its alpha-tangent planes geo_da.  pinned: the forward launch runs in the geometry kernel's form
        MARGINAL_GEO_LPP whatever the size of the batch."""
        import contextlib
        n, N, d = len(surf), len(self.theta), self.del_alpha
        form = self.ctx.option_default("geo_lpp", MARGINAL_GEO_LPP) if pinned else contextlib.nullcontext()
        geo_da = None
        if tangent:
            surf, al = np.ascontiguousarray(surf), np.ascontiguousarray(X[:, 0])
            with form:
                geo = self.ctx.fieldline_geometry(self.tables, surf, al, self.theta, device=self.device)["geo"]
            geo_da = self.ctx.fieldline_geometry_dalpha(self.tables, surf, al, self.theta, device=self.device)["geo_da"]
        else:
            al = np.stack([X[:, 0] - 0.5 * d, X[:, 0], X[:, 0] + 0.5 * d], axis=1).reshape(-1)
            with form:
                geo = self.ctx.fieldline_geometry(self.tables, np.repeat(surf, 3), al, self.theta, device=self.device)["geo"]
            if self.device is not None:
                geo = geo.view(8, n, 3, N).permute(1, 2, 0, 3).contiguous()
            else:
                geo = np.ascontiguousarray(geo.reshape(8, n, 3, N).transpose(1, 2, 0, 3))
        t0 = np.ascontiguousarray(X[:, 1])
        if self.device is not None:
            import torch
            t0 = torch.from_numpy(t0).to(self.device)
        return geo, geo_da, t0

    def _marginal_refine(self, res, maxiter, ftol, gtol, tangent=False):
        """the lockstep loop of refine_batched on the margin's objective, from the first minimum of every coarse table"""
        n = len(self.own)
        start = np.stack([res["alpha"], res["theta0"]], axis=1).astype(np.float64).reshape(n, 2)
        # (an all-inf table: mu = 0 with a zero gradient all around the start)
        r = self._marginal_refine_points(np.arange(n), start, np.isfinite(res["scale"]), maxiter, ftol, gtol, tangent)
        return dict(res, coarse_scale=res["scale"], start=start, alpha=r["x"][:, 0].copy(), theta0=r["x"][:, 1].copy(), evals=r["evals"],
                    task=r["task"], rounds=r["rounds"], scale=r["scale"], dscale=r["dscale"], dPdrho=r["dPdrho"])

    def _marginal_refine_points(self, own_idx, start, active, maxiter, ftol, gtol, tangent):
        """the loop itself on n points: point q belongs to owned surface own_idx[q] (repeats allowed) and starts at start[q]; points
        that are not `active` are not moved.  Every round is one `points` call on the points still running, and one more on all n
        fills dict(x (n, 2), evals, task (n,), rounds, scale, dscale, dPdrho)."""
        def evaluate(idx, X):
            r = self._marginal_points(own_idx[idx], X, tangent)
            return r["val"], r["jac"]
        r = _lockstep(evaluate, start, active, maxiter, ftol, gtol)
        out = dict(x=r["x"], evals=r["evals"], task=r["task"], rounds=r["rounds"])
        if len(own_idx):
            fin = self._marginal_points(own_idx, r["x"], tangent)
            out.update(scale=fin["scale"], dscale=fin["dscale"], dPdrho=fin["dPdrho"])
        else:
            out.update(scale=np.zeros(0), dscale=np.zeros((0, 2)), dPdrho=np.zeros(0))
        return out

    def _marginal_refine_multi(self, res, co, K, maxiter, ftol, gtol, tangent):
        """marginal(refine=True, n_starts=K > 1): the starts from the K best peaks of every surface's table of mu, all distinct slots of
        all surfaces through _marginal_refine_points at once, the winner per surface"""
        n, na, nt = len(self.own), len(self.alpha_scan), len(self.theta0_scan)
        start, n_found = np.zeros((n, K, 2)), np.zeros(n, dtype=np.int32)
        if n and self._on_device:
            import torch
            pk = self.ctx.scan_peaks(torch.from_numpy(self.alpha_scan).to(self.device), co["t0"], co["mu"].reshape(n, na, nt), K,
                                     want_found=True)
            start, n_found = pk["start"].cpu().numpy(), pk["n_found"].cpu().numpy()
        else:
            mu = np.asarray(co["mu"]).reshape(n, na, nt) if n else np.zeros((0, na, nt))
            for q in range(n):
                ps = pick_starts(mu[q], self.alpha_scan, self.theta0_scan, K)
                start[q], n_found[q] = ps["start"], ps["n_found"]
        run = np.maximum(n_found, 1)                                   # (a table whose maximum mu is 0: one point, not evaluated)
        own_idx = np.repeat(np.arange(n), run)
        slot = np.concatenate([np.arange(m) for m in run]) if n else np.zeros(0, dtype=np.int64)
        x0 = start[own_idx, slot].reshape(len(own_idx), 2)
        r = self._marginal_refine_points(own_idx, x0, n_found[own_idx] > 0, maxiter, ftol, gtol, tangent)
        cand, evals, task = np.zeros((n, K, 3)), np.zeros((n, K), dtype=np.int32), np.full((n, K), 10, dtype=np.int32)
        point = np.zeros((n, K), dtype=np.int64)                       # the point behind every slot: padded slots copy slot 0
        first = np.concatenate([[0], np.cumsum(run)[:-1]]) if n else np.zeros(0, dtype=np.int64)
        for q in range(n):
            point[q] = first[q]
            point[q, :run[q]] = first[q] + np.arange(run[q])
        if n:
            cand = np.stack([r["scale"][point], r["x"][point, 0], r["x"][point, 1]], axis=2)
            evals, task = r["evals"][point], r["task"][point]
        win = point[np.arange(n), np.argmin(cand[:, :, 0], axis=1)] if n else np.zeros(0, dtype=np.int64)      # (slot 0 on ties)
        return dict(res, coarse_scale=res["scale"], start=x0[win], alpha=r["x"][win, 0].copy(),
                    theta0=r["x"][win, 1].copy(), evals=evals, task=task, rounds=r["rounds"], scale=r["scale"][win], dscale=r["dscale"][win],
                    dPdrho=r["dPdrho"][win], candidates=cand, n_found=n_found)

    # -- jac="exact": val and the exact gradient at a batch of points (numpy or device tensors in, numpy out); sigma None = lam_max's pair
    # (geo_da: the alpha-tangent planes of jac="exact_tangent", geo then being the (8, n, N) planes of the points' own lines)
    def _obj_exact(self, geo, t0, sigma, geo_da=None):
        from .solver import EXACT_VJP_SHIFT, vjp_status_message
        if geo_da is not None:
            val, jac, r = self.ctx.obj_w_grad_exact_tangent(self.h, geo, geo_da, t0, sigma=sigma, want_info=True)
        else:
            val, jac, r = self.ctx.obj_w_grad_exact(self.h, geo, t0, self.del_alpha, sigma=sigma, want_info=True)
        val, jac = _host(val), _host(jac)
        vst = (_host(r["info"]) >> EXACT_VJP_SHIFT) & 3
        if np.any(vst):
            raise IbsError(vjp_status_message(int(np.sum(vst & 1)), int(np.sum(vst >> 1))))
        bad = ~(np.isfinite(val) & np.isfinite(jac).all(axis=1))
        if bad.any():
            raise IbsError("%d objective solves of the refinement were flagged (invalid data or iteration cap)" % int(bad.sum()))
        return val, jac

    # -- A6: objective with gradient at one point of one surface (utils.py:1632-1728); sigma0: the shift of eigenpair="nearest"
    def obj_w_grad(self, x, s, sigma0=None):
        a, t0 = float(x[0]), float(x[1])
        d = self.del_alpha
        if self.tangent:
            js = np.array([int(np.argmin(np.abs(self.tables.s - s)))], dtype=np.int32)
            val, jac = self.batched_obj_w_grad(js, np.array([[a, t0]]), None if sigma0 is None else np.array([float(sigma0)]))
            return float(val[0]), np.asarray(jac[0], dtype=np.float64)
        geo = np.asarray(self.fieldlines(s, np.array([a - 0.5 * d, a, a + 0.5 * d])))
        if self.exact:
            val, jac = self._obj_exact(geo[None], np.array([t0]), float(sigma0) if self.nearest else None)
        elif self.nearest:
            val, jac = self.ctx.obj_w_grad_nearest(self.h, geo[None], np.array([t0]), float(sigma0), d)
            if not (np.isfinite(val[0]) and np.all(np.isfinite(jac[0]))):
                raise IbsError("the objective's solve at (alpha, theta0) = (%g, %g) was flagged (invalid data or iteration cap)" % (a, t0))
        else:
            val, jac = self.ctx.obj_w_grad(self.h, geo[None], np.array([t0]), d)
        return float(val[0]), np.asarray(jac[0], dtype=np.float64)

    # -- A7: refinement + final solve (ball_scan.py:305-339); sigma0: the refinement's shift of eigenpair="nearest" (pick_start)
    def refine(self, s, a0, t0, sigma0=None):
        from scipy.optimize import minimize
        res = minimize(self.obj_w_grad, x0=(a0, t0), args=(s, sigma0) if self.nearest else (s,), jac=True,
                       bounds=((0.0, np.pi), (0.0, 0.5 * np.pi)),
                       options={"ftol": 5.0e-11, "gtol": 2.0e-08, "maxiter": 30})
        a, t = float(res.x[0]), float(res.x[1])
        geo = np.asarray(self.fieldlines(s, np.array([a])))[0]
        dP = -0.5 * np.mean((geo[2] - geo[7]) * geo[0] ** 2)
        if self.nearest:
            r = self.ctx.gamma_points_nearest(self.h, *[geo[k][None] for k in range(7)], np.array([dP]), np.array([t]), SIGMA_FINAL)
            if r.get("nbad", 0):
                raise IbsError("the final solve at (alpha, theta0) = (%g, %g) was flagged (invalid data or iteration cap)" % (a, t))
            return t, a, float(np.asarray(r["gam"])[0]), res
        r = self.ctx.gamma_scan(self.h, *[geo[k][None] for k in range(7)], np.array([dP]), np.array([t]), **self._certify_kw())
        if self.certify:
            self._count_certificate(r["cert"])
        return t, a, float(np.asarray(r["gam"])[0, 0]), res

    # -- F2: all owned surfaces refined in lockstep; every evaluation of every surface is ONE batched launch
    def batched_obj_w_grad(self, surf_idx, X, sigma=None):
        """objective and gradient at X[k] = (alpha, theta0) of surface surf_idx[k] for all k at once
        (device geometry for the 3 n lines, then the fused obj_w_grad kernel; eigenpair="nearest": the eigenpair nearest
        sigma[k], ibs_obj_w_grad_nearest_f64; jac="exact": ibs_obj_w_grad_exact_f64, for either eigenpair; jac="exact_tangent": the
        geometry of the n lines themselves by the row kernels, their alpha-tangent, then ibs_obj_w_grad_exact_tangent_f64).
        Returns (val (n,), jac (n, 2))."""
        import torch
        geo, geo_da, t0 = self._point_lines(surf_idx, X, self.tangent)
        sg = torch.from_numpy(np.ascontiguousarray(sigma, dtype=np.float64)).to(self.device) if self.nearest else None
        if self.exact:
            return self._obj_exact(geo, t0, sg, geo_da=geo_da)
        if self.nearest:
            val, jac = self.ctx.obj_w_grad_nearest(self.h, geo, t0, sg, self.del_alpha)
        else:
            val, jac = self.ctx.obj_w_grad(self.h, geo, t0, self.del_alpha)
        return val.cpu().numpy(), jac.cpu().numpy()

    def refine_batched(self, starts, maxiter=30, ftol=5.0e-11, gtol=2.0e-8, sigma0=None, surf_idx=None):
        """the per-surface L-BFGS-B of ball_scan.py:307-314 (same bounds, tolerances and iteration cap) for every owned
        surface at once, driven from the host (_lockstep): every round ONE batched geometry + objective launch for the surfaces
        still running.  The host-driven form of refine_device(), which it is tested against.
        starts: (n, 2); sigma0 (n,): the shifts of eigenpair="nearest"; surf_idx (n,): the table index of every point's surface
        (None: point k lies on owned surface k -- with it n points need not be n surfaces: the multi-start refinement).
        Returns (x_opt (n, 2), f_opt (n,) = -gam, rounds); jac="exact*" leaves the evaluations per point in ._batched_evals."""
        surf = self._own_surf() if surf_idx is None else np.ascontiguousarray(surf_idx, dtype=np.int32)

        def evaluate(idx, X):
            if not self.nearest:
                return self.batched_obj_w_grad(surf[idx], X)
            f, g = self.batched_obj_w_grad(surf[idx], X, np.asarray(sigma0)[idx])
            if not (np.all(np.isfinite(f)) and np.all(np.isfinite(g))):
                raise IbsError("%d objective solves of the refinement were flagged (invalid data or iteration cap)"
                               % int(np.sum(~(np.isfinite(f) & np.isfinite(g).all(axis=1)))))
            return f, g
        r = _lockstep(evaluate, np.asarray(starts, dtype=np.float64).reshape(len(surf), 2), np.ones(len(surf), dtype=bool), maxiter,
                      ftol, gtol)
        if self.exact:
            self._batched_evals = r["evals"]   # evaluations per surface of this call (diagnostic)
        return r["x"], r["f"], r["rounds"]

    def refine_device(self, starts, maxiter=30, ftol=5.0e-11, gtol=2.0e-8):
        """the same maximisation with the L-BFGS-B state machines on the device as well (ibs_refine_f64): no host
        round trip per evaluation.  Returns (x_opt (n, 2), f_opt (n,) = -gam, evaluations per surface (n,)).
        f_opt is the objective at the optimizer's last accepted iterate (scipy's res.fun); run() re-evaluates gam at
        x_opt like ball_scan.py:322-339 does."""
        surf = self._own_surf()
        xo, fo, ne, _ = self.ctx.refine(self.tables, surf, np.asarray(starts, dtype=np.float64).reshape(len(surf), 2),
                                        self.theta, self.del_alpha, maxiter, ftol, gtol, device=self.device)
        return xo, fo, ne

    def final_solve_device(self, xo):
        """gam at the refined (alpha, theta0) of every owned surface: the final geometry + solve of ball_scan.py:322-339
        (the value the reference stores; the optimizer's own f is the value at its last ACCEPTED iterate, which after a
        collapsed line search is the same point, after a maxiter stop as well).  ONE field line per point
        (ibs_gamma_points_f64): no tangent lines, no gradient sums."""
        import torch
        xo = np.asarray(xo, dtype=np.float64).reshape(-1, 2)
        r = self.ctx.fieldline_geometry(self.tables, self._own_surf(), np.ascontiguousarray(xo[:, 0]), self.theta, device=self.device)
        t0 = torch.from_numpy(np.ascontiguousarray(xo[:, 1])).to(self.device)
        if self.nearest:
            out = self.ctx.gamma_points_nearest(self.h, *[r["geo"][k] for k in range(7)], r["dPdrho"], t0, SIGMA_FINAL)
        else:
            out = self.ctx.gamma_points(self.h, *[r["geo"][k] for k in range(7)], r["dPdrho"], t0, **self._certify_kw())
        return out["gam"].cpu().numpy()

    # -- the whole per-surface worker of ball_scan.py:248-339 for the owned surfaces, resident in HBM
    def _resident_inputs(self):
        """device copies of what does not change between optimizer iterations: line -> (surface, alpha) tables of the coarse
        scan, the grids, the point -> surface map of the refinement"""
        import torch
        K = self.n_starts
        key = (tuple(self.own), str(self.device)) + ((K,) if K > 1 else ())
        if self._resident.get("key") != key:
            dev, na = self.device, len(self.alpha_scan)
            own = self._own_surf()
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            self._resident = dict(key=key, surf=t(np.repeat(own, na).astype(np.int32)), al=t(np.tile(self.alpha_scan, len(own))),
                                  th=t(self.theta), t0=t(self.theta0_scan), alpha=t(self.alpha_scan), pt_surf=t(own.astype(np.int32)),
                                  n_bad=torch.zeros(1, dtype=torch.int32, device=dev))
            if K > 1:          # (the point -> surface map of the multi-start refinement: K consecutive points per surface)
                self._resident["pt_surf_k"] = self._resident["pt_surf"].repeat_interleave(K)
        return self._resident

    def device_rows(self, refine=True, phases=None, chunks=None, fill=None):
        """(theta0*, alpha*, gam) of the owned surfaces as an (n_own, 3) DEVICE tensor + a device scalar counting what went
        wrong (flagged solves, non-finite maxima).  The one sequence of every mode: per chunk geometry -> coarse stage
        (_coarse_stage: the scan, certified and re-closed with certify=True) -> pick (_pick_starts: n_starts points per surface),
        then refinement of all n_own n_starts points (ibs_refine_f64 on device pointers; the host-driven refine_batched for
        eigenpair="nearest", jac="exact*" and N > 2050, which ibs_refine_f64 does not cover) -> final geometry + solve, one line per
        point -> select (n_starts > 1: every surface's best candidate, slot 0 on ties, by ibs_surface_argmax_pack_f64 and a device
        gather; .last_candidates, .last_peaks) -> bookkeeping.  Nothing returns to the host in between beyond what the host-driven
        refinement does; bad counts the flagged solves of ALL candidates and a non-finite coarse maximum once per surface.
        refine=False: the coarse pick itself (slot 0).  The stages by mode:
        eigenpair="max": coarse scan with the fused per-surface first maximum (ibs_gamma_scan_argmax_f64) -> start points on the
        device (ibs_scan_starts_f64) -> L-BFGS-B per surface on the device -> final solve (ibs_gamma_points_f64); any status bit
        fails a solve.
        eigenpair="nearest": the coarse scan with the eigenpair nearest 1.0 (ibs_gamma_scan_nearest_f64) -> per-surface first
        maximum (ibs_surface_argmax_pack_f64) -> start points and each surface's shift 1.3 |max| + 0.05 (ibs_scan_starts_f64) ->
        the host-driven L-BFGS-B (refine_batched: one geometry + ibs_obj_w_grad_nearest_f64 launch per round) -> final geometry +
        ibs_gamma_points_nearest_f64 at 0.42.  A solve counts as failed on status bits 0-1 only (bit 5, a tie, is informational).
        jac="exact": the refinement is the host-driven one as well, for either eigenpair (ibs_refine_f64 has no exact form): one
        geometry + ibs_obj_w_grad_exact_f64 launch per round; everything else as above.  jac="exact_tangent": the same loop with one
        geometry, one alpha-tangent and one ibs_obj_w_grad_exact_tangent_f64 launch per round, on one line per point.
        chunks: optional list of (c0, c1) ranges of owned surfaces: the coarse part (geometry, scan, starts) runs chunk by chunk,
        and fill(c0, c1) -- if given -- is called on the host before a chunk's launches (AdjointStep: the tables of the next
        equilibria are computed and uploaded while the GPU works on the previous ones).
        phases: optional dict filled with per-phase milliseconds (HIP events; adds one synchronisation at the end)."""
        import time
        import torch
        ctx, dev = self.ctx, self.device
        n = len(self.own)
        if n == 0:
            return torch.empty((0, 3), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)
        res = self._resident_inputs()
        na, K = len(self.alpha_scan), self.n_starts
        ev = {}

        def mark(name):
            if phases is not None:
                e = torch.cuda.Event(enable_timing=True); e.record(); ev.setdefault(name, []).append(e)
        res["n_bad"].zero_()
        chunks = chunks or [(0, n)]
        bad = res["n_bad"][0] * 0
        self._cert_dev = torch.zeros(3, dtype=torch.float64, device=dev) if self.certify else None
        t_fill = 0.0
        pk = {}                            # the picks of all owned surfaces: start, peak[, sigma0][, index, n_found][, the envelope]
        for c0, c1 in chunks:
            if fill is not None:
                t0 = time.perf_counter(); fill(c0, c1); t_fill += time.perf_counter() - t0
            mark("g0")
            geo = ctx.fieldline_geometry(self.tables, res["surf"][c0 * na:c1 * na], res["al"][c0 * na:c1 * na], res["th"], device=dev)
            mark("g1")
            g7 = [geo["geo"][k] for k in range(7)]
            sc = self._coarse_stage(g7, geo["dPdrho"], c1 - c0)
            bad = bad + _flagged(sc["info"], any_bit=not self.nearest).sum()
            picked = self._pick_starts(sc, g7, geo["dPdrho"], c1 - c0)
            mark("s1")
            for key, v in picked.items():
                if len(chunks) == 1:       # (one chunk: its tensors as they are, no copy)
                    pk[key] = v
                else:
                    per = len(v) // (c1 - c0)                  # rows per surface: 1, or nalpha for the envelope's
                    if key not in pk:
                        pk[key] = torch.empty((n * per,) + v.shape[1:], dtype=v.dtype, device=dev)
                    pk[key][c0 * per:c1 * per] = v
        if "env_info" in pk:               # (theta0_polish: the envelope's rows are per line)
            bad = bad + _flagged(pk["env_info"]).sum()
            self.last_envelope = {key[4:]: v for key, v in pk.items() if key.startswith("env_")}
        if K > 1:
            self.last_peaks = dict(index=pk["index"], value=pk["peak"], n_found=pk["n_found"])
        start, peak = pk["start"], pk["peak"]
        mark("r0")
        if refine:
            pts, pt_surf = start.view(n * K, 2), res["pt_surf_k" if K > 1 else "pt_surf"]
            if self.nearest or self.exact or len(self.theta) > 2050:
                # ibs_refine_f64 has no nearest-sigma and no exact form, and holds the register-resident evaluation kernel (N <= 2050):
                # there the same L-BFGS-B state machines run on the host (ibs_lbfgsb2_*) and every round is ONE batched geometry +
                # objective launch for the points still running (refine_batched: the form refine_device is tested against)
                xh, fh, rounds = self.refine_batched(pts.cpu().numpy(), sigma0=pk["sigma0"].view(-1).cpu().numpy() if self.nearest else None,
                                                     surf_idx=np.repeat(self._own_surf(), K) if K > 1 else None)
                xo = torch.from_numpy(xh).to(dev); ne = self._batched_evals if self.exact else None
            else:
                xo, fo, ne, rounds = ctx.refine_device(self.tables, pt_surf, pts, res["th"], self.del_alpha)
            mark("r1")
            xa, xt = xo[:, 0].contiguous(), xo[:, 1].contiguous()
            gf = ctx.fieldline_geometry(self.tables, pt_surf, xa, res["th"], device=dev)
            g7 = [gf["geo"][k] for k in range(7)]
            if self.nearest:
                fin = ctx.gamma_points_nearest(self.h, *g7, gf["dPdrho"], xt, SIGMA_FINAL, want_info=True)
            else:
                fin = ctx.gamma_points(self.h, *g7, gf["dPdrho"], xt, want_info=True, **self._certify_kw())
                if self.certify:
                    self._cert_dev = self._cert_dev + self._cert_counts(fin["cert"])
            bad = bad + _flagged(fin["info"], any_bit=not self.nearest).sum()
            cand = torch.stack([xt, xa, fin["gam"]], dim=1)
            self.last_refine = dict(n_evals=ne, rounds=rounds)
        else:
            mark("r1")
            cand = torch.stack([start[..., 1], start[..., 0], peak], dim=-1)
        if K > 1:                          # select: the best refined candidate of every surface; unrefined, the first maximum
            cand = self.last_candidates = cand.view(n, K, 3)
            if refine:
                best = ctx.surface_argmax_pack(fin["gam"].view(n, K))[:, 1]
                best = torch.where(best < K, best, torch.zeros_like(best)).to(torch.int64)  # (no finite candidate: slot 0, and bad > 0)
                rows = torch.gather(cand, 1, best.view(n, 1, 1).expand(n, 1, 3)).reshape(n, 3)
            else:
                rows = cand[:, 0].contiguous()
        else:
            rows = cand
        bad = bad + res["n_bad"][0]
        self._last_rows = rows             # (sensitivity()'s default points)
        mark("f1")
        if phases is not None:
            torch.cuda.synchronize()
            span = lambda a, b: sum(x.elapsed_time(y) for x, y in zip(ev[a], ev[b]))
            phases["geometry_ms"] = span("g0", "g1"); phases["scan_argmax_ms"] = span("g1", "s1")
            phases["refine_ms"] = span("r0", "r1"); phases["final_solve_ms"] = span("r1", "f1")
            if fill is not None:
                phases["host_tables_ms"] = t_fill * 1e3
                phases["coarse_chunks"] = len(chunks)
        return rows, bad.to(torch.float64)

    def _coarse_stage(self, g7, dP, m):
        """the coarse scan of a chunk of m surfaces on its lines' planes g7, dP: dict(gam, lam, info[, pack]) on the device.  max: the
        scan with the fused per-surface first maximum (pack); certify=True certifies the table's eigenvalues and re-closes them in
        place -- the pack is then stale and dropped -- and adds the counts to ._cert_dev.  nearest: the scan at SIGMA_COARSE."""
        ctx, t0 = self.ctx, self._resident["t0"]
        if self.nearest:
            return ctx.gamma_scan_nearest(self.h, *g7, dP, t0, SIGMA_COARSE, want_info=True)
        sc = ctx.gamma_scan_argmax(self.h, g7, dP, t0, m)
        if self.certify:
            cert = ctx.certify_scan(self.h, *g7, dP, t0, sc["lam"])
            ctx.reclose_scan(self.h, *g7, dP, t0, cert, sc["lam"], sc["gam"])
            self._cert_dev = self._cert_dev + self._cert_counts(cert)
            del sc["pack"]
        return sc

    def _pick_starts(self, sc, g7, dP, m):
        """the refinement's starts of a chunk of m surfaces from its coarse scan sc: dict(start, peak[, sigma0 in nearest mode]) on
        the device.  n_starts = 1: start (m, 2), peak (m,) from the per-surface first maximum (the scan's fused pack, else
        ibs_surface_argmax_pack_f64 over the table) by ibs_scan_starts_f64; theta0_polish moves every surface's start to the crest of
        its best line (ibs_theta0_polish_f64, whose outputs ride along as env_*).  n_starts = K > 1: start (m, K, 2), peak (m, K),
        index, n_found of the K best peaks (ibs_scan_peaks_f64 on the table: the scan kernel is that of K = 1, so that slot 0 has
        that run's bits).  Either way a non-finite maximum is counted once per surface in the resident n_bad."""
        ctx, res, K = self.ctx, self._resident, self.n_starts
        na, nt = len(self.alpha_scan), len(self.theta0_scan)
        if K > 1:
            pk = ctx.scan_peaks(res["alpha"], res["t0"], sc["gam"].view(m, na, nt), K, n_bad=res["n_bad"], want_sigma0=self.nearest,
                                want_index=True, want_found=True)
            return {key: pk[key] for key in ("start", "peak", "index", "n_found") + (("sigma0",) if self.nearest else ())}
        pack = sc["pack"] if "pack" in sc else ctx.surface_argmax_pack(sc["gam"].view(m, -1))
        if self.nearest:
            st, sg = ctx.scan_starts(res["alpha"], res["t0"], pack, res["n_bad"], want_sigma0=True)
            return dict(start=st, peak=pack[:, 0], sigma0=sg)
        st, gm = ctx.scan_starts(res["alpha"], res["t0"], pack, res["n_bad"]), pack[:, 0]
        if not self.theta0_polish:
            return dict(start=st, peak=gm)
        # every line's crest between the nodes; the surface's start is the first maximum of gam_env over its lines
        import torch
        env = ctx.theta0_polish(self.h, *g7, dP, res["t0"], sc["gam"], lam=sc["lam"], want_info=True)
        ge = torch.nan_to_num(env["gam"].view(m, na), nan=-float("inf"))
        top = ge.max(dim=1).values
        col = torch.arange(na, device=self.device).expand_as(ge)
        first = torch.where(ge == top[:, None], col, na).min(dim=1).values.clamp(max=na - 1)
        ok = torch.isfinite(top) & (top != 0.0)                              # (else the start scan_starts gave: (0, 0))
        t_star = env["theta0"].view(m, na).gather(1, first[:, None])[:, 0]
        st = torch.where(ok[:, None], torch.stack([res["alpha"][first], t_star], dim=1), st)
        return dict({"env_" + key: v for key, v in env.items() if key != "nbad"}, start=st, peak=torch.where(ok, top, gm))

    def sensitivity(self, points=None, eigenpair=None):
        """exact derivatives of every owned surface's gam at ONE point (alpha, theta0) of that surface, with respect to the point and
        to the surface's own tables.  tables= + device= scans only.  points (n_own, 2) = (alpha, theta0); None: the rows of the last
        local_rows() / device_rows() / run().  eigenpair None: this scan's mode ("nearest": the eigenpair nearest SIGMA_FINAL, as in
        the final solve).  One geometry launch, one solve (autograd.growth_rate), one rows-VJP (ibs_solve_gcf_vjp_f64) and one
        geometry-VJP launch (ibs_fieldline_geometry_vjp_f64) in which every surface's point works on its own copy of the surface's
        tables, so that the cotangents stay per point.  Returns device tensors dict(gam, dgam_dalpha, dgam_dtheta0: (n_own,);
        tab_mn_bar (n_own, 6, mnmax), tab_nyq_bar (n_own, 7, mnmax_nyq), scal_bar (n_own, 6))."""
        import torch
        from . import autograd as iag
        if not self._on_device:
            raise IbsError("sensitivity() needs a scan built with tables= and device=")
        mode = self.eigenpair if eigenpair is None else check_eigenpair(eigenpair)
        dev, own = self.device, self._own_surf()
        n = len(own)
        if points is None:
            rows = getattr(self, "_last_rows", None)
            if rows is None or rows.shape[0] != n:
                raise IbsError("sensitivity(): no points given and no rows of an earlier run on this object")
            al, t0 = rows[:, 1].detach().clone(), rows[:, 0].detach().clone()
        else:
            pts = np.asarray(points, dtype=np.float64).reshape(n, 2)
            al, t0 = (torch.from_numpy(np.ascontiguousarray(pts[:, k])).to(dev) for k in (0, 1))
        d = self.ctx._device_tables(self.tables, dev)
        idx = torch.from_numpy(own.astype(np.int64)).to(dev)
        tm, tq, sc = (d[k][idx].clone().requires_grad_(True) for k in (4, 5, 6))
        al.requires_grad_(True); t0.requires_grad_(True)
        geo, dP = iag.fieldline_geometry(self.tables, torch.arange(n, dtype=torch.int32, device=dev), al, self._resident_inputs()["th"],
                                         tab_mn=tm, tab_nyq=tq, scal=sc, ctx=self.ctx)
        gam = iag.growth_rate(self.h, *geo[:7], dP, t0[:, None], eigenpair=mode, sigma=SIGMA_FINAL if mode == "nearest" else None,
                              ctx=self.ctx)
        gam.sum().backward()
        return dict(gam=gam.detach().reshape(n), dgam_dalpha=al.grad, dgam_dtheta0=t0.grad, tab_mn_bar=tm.grad, tab_nyq_bar=tq.grad,
                    scal_bar=sc.grad)

    def smooth_max(self, beta):
        """objective.smooth_max of every owned surface's WHOLE coarse (alpha, theta0) table and its exact gradient with respect to
        the surface's own tables: an aggregate that sees a maximum that jumps, where sensitivity() is a statement at one frozen
        point.  tables= + device= scans only; the eigenpair is this scan's (eigenpair="nearest": the one nearest SIGMA_COARSE, as in
        the coarse scan).  Each owned surface gets its own differentiable copies of tab_mn, tab_nyq, scal and all nalpha coarse
        lines of the surface index that copy: one geometry launch, one autograd.gamma_scan (the scan kernel forward,
        ibs_gamma_scan_vjp_f64 backward), smooth_max, one backward through ibs_fieldline_geometry_vjp_f64.  Returns device tensors
        dict(value, max: (n_own,); tab_mn_bar (n_own, 6, mnmax), tab_nyq_bar (n_own, 7, mnmax_nyq), scal_bar (n_own, 6)) =
        d value / d tables; SurfaceTables.pullback carries them to the wout arrays, as after sensitivity()."""
        import torch
        from . import autograd as iag
        from .objective import smooth_max
        if not self._on_device:
            raise IbsError("smooth_max() needs a scan built with tables= and device=")
        dev, own = self.device, self._own_surf()
        n, na = len(own), len(self.alpha_scan)
        res = self._resident_inputs()
        d = self.ctx._device_tables(self.tables, dev)
        idx = torch.from_numpy(own.astype(np.int64)).to(dev)
        tm, tq, sc = (d[k][idx].clone().requires_grad_(True) for k in (4, 5, 6))
        line_surf = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(na)
        geo, dP = iag.fieldline_geometry(self.tables, line_surf, res["al"], res["th"], tab_mn=tm, tab_nyq=tq, scal=sc, ctx=self.ctx)
        gam = iag.gamma_scan(self.h, *geo[:7], dP, res["t0"], eigenpair=self.eigenpair, sigma=SIGMA_COARSE if self.nearest else None,
                             ctx=self.ctx)
        tab = gam.reshape(n, na, -1)
        value = smooth_max(tab, beta)
        value.sum().backward()
        return dict(value=value.detach(), max=tab.detach().reshape(n, -1).max(dim=1).values if n else value.detach(),
                    tab_mn_bar=tm.grad, tab_nyq_bar=tq.grad, scal_bar=sc.grad)

    def marginal_sensitivity(self, points=None):
        """exact derivatives of every owned surface's critical scale s* at ONE point (alpha, theta0) of that surface, with respect to
        the point and to the surface's own tables.  tables= + device= scans only.  points (n_own, 2) = (alpha, theta0); None: the
        points of the last marginal() on this object (IbsError if there is none).  One geometry launch (in the pinned form of the
        refinement's rounds), one alpha-tangent launch, one point launch with the cotangent planes (ibs_marginal_obj_w_grad_tangent_f64)
        and one geometry-VJP launch (ibs_fieldline_geometry_vjp_f64) in which every surface's point works on its own copy of the
        surface's tables, so that the cotangents stay per point.  s* is an eigenvalue of the discrete pencil: the derivatives are
        those of the scale returned.  At a point refined with marginal(refine=True, jac="exact_tangent") that is interior to the box,
        dscale_dalpha = dscale_dtheta0 = 0 and the table cotangents are d (min s*) / d tables by the envelope theorem.  A surface with
        scale = inf has zero derivatives; status bits 0-1 raise IbsError.  The frozen-geometry caveat of marginal() applies.
        Returns device tensors dict(scale, dscale_dalpha, dscale_dtheta0, dPdrho: (n_own,); tab_mn_bar (n_own, 6, mnmax), tab_nyq_bar
        (n_own, 7, mnmax_nyq), scal_bar (n_own, 6))."""
        import torch
        from . import autograd as iag
        if not self._on_device:
            raise IbsError("marginal_sensitivity() needs a scan built with tables= and device=")
        dev, own = self.device, self._own_surf()
        n = len(own)
        if points is None:
            pts = getattr(self, "_last_marginal_points", None)
            if pts is None or pts.shape[0] != n:
                raise IbsError("marginal_sensitivity(): no points given and no marginal() on this object before")
        else:
            pts = np.asarray(points, dtype=np.float64).reshape(n, 2)
        al, t0 = (torch.from_numpy(np.ascontiguousarray(pts[:, k])).to(dev) for k in (0, 1))
        d = self.ctx._device_tables(self.tables, dev)
        idx = torch.from_numpy(own.astype(np.int64)).to(dev)
        tm, tq, sc = (d[k][idx].clone().requires_grad_(True) for k in (4, 5, 6))
        th = self._resident_inputs()["th"]
        with self.ctx.option_default("geo_lpp", MARGINAL_GEO_LPP):
            geo, _ = iag.fieldline_geometry(self.tables, torch.arange(n, dtype=torch.int32, device=dev), al, th, tab_mn=tm, tab_nyq=tq,
                                            scal=sc, ctx=self.ctx)
        gda = self.ctx.fieldline_geometry_dalpha(self.tables, own, np.ascontiguousarray(pts[:, 0]), self.theta, device=dev)["geo_da"]
        scale, dscale, dP = iag.marginal_points_full(self.h, geo, gda, t0, ctx=self.ctx)
        scale.sum().backward()
        return dict(scale=scale.detach(), dscale_dalpha=dscale[:, 0].contiguous(), dscale_dtheta0=dscale[:, 1].contiguous(), dPdrho=dP,
                    tab_mn_bar=tm.grad, tab_nyq_bar=tq.grad, scal_bar=sc.grad)

    @staticmethod
    def _cert_counts(cert):
        """(checked, reclosed, failed) of a device tensor of cert words, as a device tensor"""
        import torch
        return torch.stack([torch.full((), float(cert.numel()), dtype=torch.float64, device=cert.device),
                            (cert == 8).sum().to(torch.float64), ((cert & 7) != 0).sum().to(torch.float64)])

    def _count_certificate(self, cert):
        """host-side paths: add a call's cert words to .last_certificate"""
        c = np.asarray(cert.cpu().numpy() if hasattr(cert, "cpu") else cert)
        if self.last_certificate is None:          # (refine() called on its own, outside local_rows)
            self.last_certificate = dict(checked=0, reclosed=0, failed=0)
        lc = self.last_certificate
        lc["checked"] += int(c.size); lc["reclosed"] += int(np.sum(c == 8)); lc["failed"] += int(np.sum((c & 7) != 0))

    def _raise_uncertified(self):
        if self.last_certificate["failed"]:
            raise IbsError("%d of %d eigenvalues could not be certified (cert bits 0-2 after the re-close)"
                           % (self.last_certificate["failed"], self.last_certificate["checked"]))

    def _multi_start_rows(self, tabs, refine):
        """the callback path for n_starts = K > 1: pick_starts on every coarse table, self.refine from each of the n_found distinct
        starts (at least one), the best refined candidate by the first-maximum rule (slot 0 wins ties); the slots beyond n_found
        repeat slot 0's candidate without running it again.  refine=False: slot 0, the rows of n_starts = 1.  Fills
        .last_candidates and .last_peaks (numpy)."""
        K = self.n_starts
        rows, cands = [], np.zeros((len(self.own), K, 3))
        peaks = dict(index=np.zeros((len(self.own), K), dtype=np.int32), value=np.zeros((len(self.own), K)),
                     n_found=np.zeros(len(self.own), dtype=np.int32))
        for q, (k, tab) in enumerate(zip(self.own, tabs)):
            pick_start(tab, self.alpha_scan, self.theta0_scan)           # (raises on a table with non-finite growth rates)
            ps = pick_starts(tab, self.alpha_scan, self.theta0_scan, K)
            peaks["index"][q], peaks["value"][q], peaks["n_found"][q] = ps["index"], ps["peak"], ps["n_found"]
            for j in range(max(1, ps["n_found"])):
                (a0, t0), sigma0 = ps["start"][j], ps["sigma0"][j]
                if refine:
                    t, a, gam, _ = self.refine(self.rho_arr[k], float(a0), float(t0), float(sigma0) if self.nearest else None)
                else:
                    t, a, gam = float(t0), float(a0), float(ps["peak"][j])
                cands[q, j] = t, a, gam
            cands[q, max(1, ps["n_found"]):] = cands[q, 0]
            rows.append(tuple(cands[q, int(np.argmax(cands[q, :, 2])) if refine else 0]))
        self.last_candidates, self.last_peaks = cands, peaks
        return rows

    def local_rows(self, refine=True):
        """(theta0*, alpha*, gam) of the surfaces this rank owns, (n_own, 3): coarse scan -> argmax -> refinement -> final
        solve (ball_scan.py:248-339), no collective"""
        if self.certify:
            self.last_certificate = dict(checked=0, reclosed=0, failed=0)
        if self._on_device:
            import torch
            rows, bad = self.device_rows(refine)
            if not len(self.own):
                return rows.cpu().numpy().reshape(0, 3)
            # the one copy (and synchronisation): the rows, the count of what went wrong and, with certify, the certificate counts
            host = torch.cat([rows.reshape(-1), bad.reshape(1)] + ([self._cert_dev] if self.certify else [])).cpu().numpy()
            if self.certify:
                self.last_certificate = dict(checked=int(host[-3]), reclosed=int(host[-2]), failed=int(host[-1]))
                host = host[:-3]
            if host[-1] != 0 or not np.all(np.isfinite(host[:-1])):
                raise IbsError("%d solves of this rank's scan were flagged or produced non-finite growth rates (status word != 0: "
                               "invalid data or iteration cap)" % int(host[-1]))
            if self.certify:
                self._raise_uncertified()
            return host[:-1].reshape(len(self.own), 3)
        tabs = self.coarse()
        rows = []
        if self.certify:
            self._count_certificate(self._coarse_cert)
        for k, tab in zip(self.own, tabs if self.n_starts == 1 else ()):
            a0, t0, sigma0, ij = pick_start(tab, self.alpha_scan, self.theta0_scan)
            if refine:
                t, a, gam, _ = self.refine(self.rho_arr[k], a0, t0, sigma0 if self.nearest else None)
            else:
                t, a, gam = t0, a0, float(np.max(tab))
            rows.append((t, a, gam))
        if self.n_starts > 1:
            rows = self._multi_start_rows(tabs, refine)
        if self.certify:
            self._raise_uncertified()
        return np.array(rows, dtype=np.float64).reshape(len(self.own), 3)

    def run(self, refine=True):
        """returns (theta0_arr, alpha_arr, gam_arr), each (nsurfs,), identical on every rank.
        Every rank takes part in the ONE gather whatever happens on its own shard: a rank-local failure of ANY kind (flagged
        solves, non-finite tables, a geometry producer that raises, an out-of-memory error of the framework) travels through
        the collective as NaN rows and is raised on EVERY rank afterwards -- a rank that raised before the gather would
        leave the others waiting in it."""
        err = None
        try:
            local = self.local_rows(refine)
        except Exception as e:             # (re-raised after the gather, whatever it is)
            err = e
            local = np.full((len(self.own), 3), np.nan)
        # one decision for every gather of this object, the same on every rank: the library's own communicator when the
        # context holds one for this world (Context.comm_init is all-or-none over the ranks), else torch.distributed
        full = gather_surfaces(local, len(self.rho_arr), self.rank, self.world, self.dist, self.gather_device,
                               self.ctx if self._native_gather else None)
        if err is not None:
            raise err
        if self.world > 1 and not np.all(np.isfinite(full)):
            bad = sorted(set(int(j) % self.world for j in np.nonzero(~np.isfinite(full).all(axis=1))[0]))
            raise IbsError("surface rows of rank(s) %s are not finite: the scan failed there (see that rank's error)" % bad)
        return full[:, 0], full[:, 1], full[:, 2]


# -- A8 / F4: on-disk history contract of ball_scan.py:359-384 (consumed by sims_runner_*.py:198-199, 300-306)
def append_history(path, dof_idx, iter0, gam_arr, theta0_arr, alpha_arr):
    import os
    out = {}
    for name, row in (("ball_gam", gam_arr), ("ball_theta0", theta0_arr), ("ball_alpha", alpha_arr)):
        fn = os.path.join(path, "%s%d.npy" % (name, int(dof_idx)))
        old = np.load(fn, allow_pickle=True)
        if iter0 == 0:
            new = np.delete(np.append(old, row), 0)        # ball_scan.py:369-375: replace the placeholder
        else:
            new = np.vstack((old, row))                    # ball_scan.py:376-379
        np.save(fn, new)
        out[name] = new
    return out
