"""Call transcripts of the Python binding: what every Context method hands to the C library, without a GPU kernel.

stand_in() replaces _lib._LIB by an object that answers the names of _lib.SYMBOLS, checks every call against the symbol's argument
types and records it.  run_case() resolves every argument of every recorded call to

    i:<int>  f:<float>  s:<bytes>          a scalar passed by value
    null  handle  ref  buf  stream          a null pointer, the context handle, a byref() / string buffer, ibs_set_stream's stream
    in:<name>  inout:<name>                 the caller's own array, by address
    copy:<name>:<dtype>                     a converted copy of the caller's array, by its full contents (host calls)
    bcast:<name>:<k>                        a scalar of the caller broadcast to (at least) k float64 values (host calls)
    out:<name>:<shape>:<dtype>              the array the method returned under that name, by address
    empty                                   a pointer whose count argument, just before it, is 0
    tmp                                     device calls only: an uploaded temporary or a resident table copy

and fails on a pointer that is none of these.  It uses the public methods and _lib._LIB only, so it runs unchanged on any version of
solver.py:  python tests/tools/binding_recorder.py host|device OUT.json [--solver PATH/solver.py]  writes the golden transcripts
tests/golden/B1_binding_calls_{host,device}.json (from the parent commit's solver.py when a refactor is to be pinned).
"""
import contextlib
import ctypes as C
import importlib.util
import inspect
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import ibs_amd                      # noqa: E402
from ibs_amd import _lib            # noqa: E402
from ibs_amd._lib import IbsError   # noqa: E402

HANDLE = 0x1B5C0DE0
NBAD = 7                            # what every compute call returns: visible wherever a method passes nbad / rounds through
QUIET = ("ibs_create", "ibs_destroy", "ibs_set_stream", "ibs_set_option", "ibs_synchronize")
SCALAR_OR_ARRAY = ("sigma", "shift", "gam_bar", "lam_bar")
N, N_SYS, N_LINES, N_T0, N_PTS = 67, 3, 2, 3, 2


class RecorderError(AssertionError):
    pass


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _readable_ranges():
    out = []
    with open("/proc/self/maps") as fh:
        for line in fh:
            span, perm = line.split()[:2]
            if perm[0] == "r":
                lo, hi = (int(v, 16) for v in span.split("-"))
                if out and out[-1][1] == lo:
                    out[-1][1] = hi
                else:
                    out.append([lo, hi])
    return out


class StandIn:
    """stands in for the loaded library: answers the names of _lib.SYMBOLS only"""

    def __init__(self, device=False):
        self.device = device
        self.calls = None           # a list while a case is being recorded
        self.n_calls = 0
        self._copies = []

    def __getattr__(self, name):
        if name.startswith("__") or name not in _lib.SYMBOLS:
            raise AttributeError(name)
        fn = lambda *args: self._call(name, args)
        self.__dict__[name] = fn
        return fn

    def _call(self, name, args):
        argtypes = _lib.SYMBOLS[name][1]
        if len(args) != len(argtypes):
            raise RecorderError("%s: %d arguments for %d" % (name, len(args), len(argtypes)))
        for k, (a, t) in enumerate(zip(args, argtypes)):
            try:
                t.from_param(a)
            except (TypeError, C.ArgumentError) as e:
                raise RecorderError("%s: argument %d (%r) is not a %s: %s" % (name, k, a, t.__name__, e))
        self.n_calls += 1
        if name == "ibs_create":
            args[0]._obj.value = HANDLE
        if name == "ibs_last_error":
            return b"stand-in"
        if self.calls is not None:
            self.calls.append((name, self._raw(name, args)))
        return 0 if name in QUIET else NBAD

    def _raw(self, name, args):
        ranges = None
        raw = []
        for k, a in enumerate(args):
            if isinstance(a, bool):
                raise RecorderError("%s: argument %d is a bool" % (name, k))
            if a is None:
                raw.append("null")
            elif isinstance(a, int):
                raw.append("i:%d" % a)
            elif isinstance(a, float):
                raw.append("f:%r" % a)
            elif isinstance(a, bytes):
                raw.append("s:" + a.decode())
            elif isinstance(a, C.c_void_p):
                if name == "ibs_set_stream" and k == 1:
                    raw.append(("stream", a.value or 0))
                elif a.value is None:
                    raw.append("null")
                elif a.value == HANDLE:
                    raw.append("handle")
                else:
                    if ranges is None and not self.device:
                        ranges = _readable_ranges()
                    raw.append(("p", a.value, None if self.device else self._copy_of(a.value, ranges)))
            elif isinstance(a, C.Array):
                raw.append("buf")
            else:
                raw.append("ref")               # byref(...)
        return raw

    def _copy_of(self, addr, ranges):
        """the converted copy or broadcast scalar of the caller whose bytes stand at addr"""
        for label, data in self._copies:
            n = len(data)
            if any(lo <= addr and addr + n <= hi for lo, hi in ranges) and C.string_at(addr, min(n, 8)) == data[:8] \
                    and C.string_at(addr, n) == data:
                return label
        return None

    def begin(self, named):
        self.calls = []
        self._copies = []
        if self.device:
            return
        for name, v in named.items():
            if isinstance(v, (int, float)):
                for k in (6, 3, 2, 1):
                    self._copies.append(("bcast:%s:%d" % (name, k), np.full(k, float(v)).tobytes()))
            elif not _is_torch(v):
                a = np.asarray(v)
                for dt in sorted((np.float64, np.int32, np.float32), key=lambda d: np.dtype(d) != a.dtype):
                    if a.size:
                        self._copies.append(("copy:%s:%s" % (name, np.dtype(dt).name), np.ascontiguousarray(a, dtype=dt).tobytes()))

    def end(self):
        calls, self.calls = self.calls, None
        return calls


@contextlib.contextmanager
def stand_in(device=False):
    saved = _lib._LIB
    fake = _lib._LIB = StandIn(device)
    try:
        yield fake
    finally:
        _lib._LIB = saved


def _addr(a):
    return a.data_ptr() if _is_torch(a) else a.ctypes.data


def _is_array(v):
    return isinstance(v, np.ndarray) or (_is_torch(v) and hasattr(v, "data_ptr"))


def _named_inputs(bound):
    named = {}
    for name, v in bound.items():
        if hasattr(v, "tab_mn"):
            for k in ("xm", "xn", "xm_nyq", "xn_nyq", "tab_mn", "tab_nyq", "scal", "rows_mn", "rows_nyq"):
                named["%s.%s" % (name, k)] = getattr(v, k)
        elif _is_array(v):
            named[name] = v
        elif isinstance(v, (list, tuple)) and v and all(_is_array(e) for e in v):
            for k, e in enumerate(v):
                named["%s.%d" % (name, k)] = e
        elif isinstance(v, (list, tuple)) and v and all(isinstance(e, (int, float)) for e in v):
            named[name] = v
        elif name in SCALAR_OR_ARRAY and isinstance(v, (int, float)) and not isinstance(v, bool):
            named[name] = v
    return named


def _named_outputs(ret, prefix=""):
    if isinstance(ret, dict):
        ret = sorted(ret.items())
    elif isinstance(ret, tuple):
        ret = list(enumerate(ret))
    elif _is_array(ret):
        return {prefix or "ret": ret}
    else:
        return {}
    out = {}
    for k, v in ret:
        out.update(_named_outputs(v, "%s%s%s" % (prefix, "." if prefix else "", k)))
    return out


def _describe(ret):
    if isinstance(ret, dict):
        return {k: _describe(v) for k, v in sorted(ret.items())}
    if isinstance(ret, tuple):
        return [_describe(v) for v in ret]
    if _is_array(ret):
        return "%s:%s:%s" % ("torch" if _is_torch(ret) else "numpy", tuple(ret.shape), str(ret.dtype).replace("torch.", ""))
    return ret if ret is None or isinstance(ret, (int, float, str)) else repr(ret)


def is_error(result):
    """the case raised: its transcript must hold no compute call"""
    return isinstance(result, str) and not result.startswith(("numpy:", "torch:"))


def run_case(ctx, fake, method, args, kwargs, inout=()):
    """calls ctx.<method> under the stand-in -> dict(calls=[[symbol, [argument, ...]], ...], result=...); the raw stream handles of
    the ibs_set_stream calls are left in fake.streams"""
    bound = inspect.signature(getattr(ctx, method)).bind(*args, **kwargs)
    bound.apply_defaults()
    named = _named_inputs(bound.arguments)
    fake.begin(named)
    ret = None
    try:
        ret = getattr(ctx, method)(*args, **kwargs)
        result = _describe(ret)
    except IbsError as e:
        result = "IbsError: %s" % e
    except RecorderError:
        fake.end()
        raise
    except Exception as e:                                    # (a shape that does not unpack: the type is the record)
        result = type(e).__name__
    raw_calls = fake.end()
    ins = {_addr(v): k for k, v in named.items() if _is_array(v)}
    outs = {_addr(v): (k, v) for k, v in _named_outputs(ret).items() if not _is_torch(v) or v.is_cuda}
    fake.streams = []
    calls = []
    for sym, raw in raw_calls:
        res = []
        for k, a in enumerate(raw):
            if isinstance(a, str):
                res.append(a)
            elif a[0] == "stream":
                fake.streams.append(a[1])
                res.append("stream")
            elif a[1] in ins:
                res.append(("inout:" if ins[a[1]] in inout else "in:") + ins[a[1]])
            elif a[1] in outs:
                name, v = outs[a[1]]
                res.append("out:%s:%s:%s" % (name, tuple(v.shape), str(v.dtype).replace("torch.", "")))
            elif a[2] is not None:
                res.append(a[2])
            elif k and res[-1] == "i:0":
                res.append("empty")
            elif fake.device:
                res.append("tmp")
            else:
                raise RecorderError("%s.%s: argument %d of %s is a pointer to nothing the case knows" % (method, sym, k, sym))
        calls.append([sym, res])
    return dict(calls=calls, result=result)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
GEO7 = ("bmag", "gradpar", "cvdrift", "cvdrift0", "gds2", "gds21", "gds22")


def make_data(device=None):
    """the smallest shapes the library accepts: N = 67, 3 systems, 2 lines x 3 theta0, 2 points; tables of G8.  device: a
    torch.device -> every array a tensor there (the numpy originals stay under "np")"""
    # (every scalar that is broadcast has a value of its own among the cases: a broadcast is recognised by its contents)
    rng = np.random.default_rng(20261)
    r = lambda *shape: rng.uniform(0.5, 1.5, shape)
    d = dict(g=r(N_SYS, N), c=r(N_SYS, N), f=r(N_SYS, N), gh=r(N_SYS, N), X=r(N_SYS, N), dX=r(N_SYS, N), lam=r(N_SYS), gam=r(N_SYS),
             sig_sys=r(N_SYS), gbar_sys=r(N_SYS), lbar_sys=r(N_SYS), g_p=r(N_SYS, N), c_p=r(N_SYS, N), f_p=r(N_SYS, N),
             scan7=[r(N_LINES, N) for _ in GEO7], dP=r(N_LINES), t0_scan=r(N_T0), sig_scan=r(N_LINES, N_T0), lam_scan=r(N_LINES, N_T0),
             gam_scan=r(N_LINES, N_T0), X_scan=r(N_LINES, N_T0, N), dX_scan=r(N_LINES, N_T0, N),
             t0_pts=r(N_PTS), sig_pts=r(N_PTS), lam_pts=r(N_PTS), gam_pts=r(N_PTS), X_pts=r(N_PTS, N), dX_pts=r(N_PTS, N),
             geo4=r(N_PTS, 3, 8, N), geoT=r(8, N_PTS, N), geoD=r(8, N_PTS, N), geo_bar=r(8, N_LINES, N), dP_bar=r(N_LINES),
             line_alpha=r(N_LINES), theta=np.linspace(-np.pi, np.pi, N), starts=r(N_PTS, 2), gam_surf=r(3, 6),
             alpha_scan=r(N_LINES), pack=r(3, 2))
    d["cert_scan"] = np.full((N_LINES, N_T0), 1, dtype=np.int32)
    d["cert_pts"] = np.full((N_PTS,), 2, dtype=np.int32)
    d["line_surf"] = np.array([1, 0], dtype=np.int32)
    d["n_bad"] = np.zeros(1, dtype=np.int32)
    d["g32"] = np.asfortranarray(r(N_SYS, N).astype(np.float32))          # float32 and not contiguous
    host = dict(d)
    if device is not None:
        import torch
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        d = {k: ([up(a) for a in v] if isinstance(v, list) else up(v)) for k, v in d.items()}
        d["g32"] = up(np.ascontiguousarray(host["g32"].T)).t()
    d["np"] = host
    d["tables"] = ibs_amd.SurfaceTables.from_arrays(dict(np.load(os.path.join(ROOT, "tests", "golden", "G8_surface_tables.npz"))))
    d["tables_fresh"] = ibs_amd.SurfaceTables.from_arrays(dict(np.load(os.path.join(ROOT, "tests", "golden", "G8_surface_tables.npz"))))
    if device is not None:
        t = d["tables"]
        d["tabs"] = tuple(up(np.concatenate([a, a])) for a in (t.tab_mn, t.tab_nyq, t.scal))      # twice the surfaces of `tables`
    return d


def _subsets(names):
    """all off, each alone, all on"""
    sets = [()] + [(n,) for n in names] + ([tuple(names)] if len(names) > 1 else [])
    return [("-".join(s) or "plain", {n: (n in s) for n in names}) for s in sets]


def cases(d, device=None):
    """[(case name, method, args, kwargs, in-out names)]; device: the torch.device of d, or None for the host cases"""
    h = 0.09
    out = []

    def add(name, method, *args, inout=(), **kw):
        out.append((name, method, args, kw, inout))

    g, c, f = d["g"], d["c"], d["f"]
    scan = (*d["scan7"], d["dP"], d["t0_scan"])
    pts = (*d["scan7"], d["dP"], d["t0_pts"])
    bad4, badT = d["geo4"][:, :2], d["geoT"][:7]
    # ---- raw systems
    for tag, kw in _subsets(("want_X", "want_info")):
        add("solve_gcf/" + tag, "solve_gcf", h, g, c, f, **kw)
        add("solve_gcf/gh-" + tag, "solve_gcf", h, g, c, f, gh=d["gh"], **kw)
        add("solve_gcf_nearest/" + tag, "solve_gcf_nearest", h, g, c, f, d["sig_sys"], **kw)
        add("gamma_points_nearest/" + tag, "gamma_points_nearest", h, *pts, d["sig_pts"], **kw)
    add("solve_gcf/no-gam", "solve_gcf", h, g, c, f, want_gam=False)
    add("solve_gcf/one-system-X", "solve_gcf", h, g[:1], c[:1], f[:1], want_X=True)
    add("solve_gcf/f32", "solve_gcf", h, d["g32"], d["g32"], d["g32"], dtype=np.float32, want_gam=False)
    add("solve_gcf/f32-noncontiguous-to-f64", "solve_gcf", h, d["g32"], c, f)
    add("solve_gcf_nearest/scalar-sigma-gh", "solve_gcf_nearest", h, g, c, f, 0.37, gh=d["gh"])
    add("gamma_points_nearest/scalar-sigma", "gamma_points_nearest", h, *pts, 0.42)
    for tag, kw in (("gam_bar", dict(gam_bar=d["gbar_sys"])), ("lam_bar", dict(lam_bar=d["lbar_sys"])),
                    ("both", dict(gam_bar=d["gbar_sys"], lam_bar=d["lbar_sys"])), ("scalars-info", dict(gam_bar=1.37, lam_bar=0.2531, want_info=True))):
        add("solve_gcf_vjp/" + tag, "solve_gcf_vjp", h, g, c, f, d["lam"], d["X"], **kw)
    add("solve_gcf_vjp/error-none", "solve_gcf_vjp", h, g, c, f, d["lam"], d["X"])
    # ---- marginal stability
    for tag, kw in _subsets(("want_X", "want_grad", "want_info")):
        add("marginal_gcf/" + tag, "marginal_gcf", h, g, c, **kw)
    for tag, kw in _subsets(("want_grad", "want_info")):
        add("marginal_scan/" + tag, "marginal_scan", h, *scan, **kw)
        add("marginal_obj_w_grad/" + tag, "marginal_obj_w_grad", h, d["geo4"], d["t0_pts"], del_alpha=0.01, **kw)
    for tag, kw in _subsets(("want_grad", "want_geo_bar", "want_info")):
        add("marginal_obj_w_grad_tangent/" + tag, "marginal_obj_w_grad_tangent", h, d["geoT"], d["geoD"], d["t0_pts"], **kw)
    add("marginal_obj_w_grad_tangent/no-geo_da", "marginal_obj_w_grad_tangent", h, d["geoT"], None, d["t0_pts"], want_grad=False)
    add("marginal_obj_w_grad_tangent/error-geo_da-required", "marginal_obj_w_grad_tangent", h, d["geoT"], None, d["t0_pts"])
    add("marginal_obj_w_grad_tangent/error-shape", "marginal_obj_w_grad_tangent", h, badT, d["geoD"], d["t0_pts"])
    add("marginal_obj_w_grad_tangent/error-shape-da", "marginal_obj_w_grad_tangent", h, d["geoT"], badT, d["t0_pts"])
    add("marginal_obj_w_grad/error-shape", "marginal_obj_w_grad", h, bad4, d["t0_pts"])
    # ---- scans and points
    for tag, kw in _subsets(("want_X", "want_dtheta0", "want_info")):
        add("gamma_scan/" + tag, "gamma_scan", h, *scan, **kw)
        add("gamma_points/" + tag, "gamma_points", h, *pts, **kw)
    add("gamma_scan/warm", "gamma_scan", h, *scan, lam_guess=d["lam_scan"], guess_width=0.5, want_info=True)
    add("gamma_scan/certify", "gamma_scan", h, *scan, certify=True)
    add("gamma_scan/certify-X", "gamma_scan", h, *scan, certify=True, want_X=True, want_info=True)
    add("gamma_points/certify", "gamma_points", h, *pts, certify=True)
    add("gamma_points/certify-X", "gamma_points", h, *pts, certify=True, want_X=True)
    for tag, kw in _subsets(("want_info",)):
        add("gamma_scan_nearest/" + tag, "gamma_scan_nearest", h, *scan, d["sig_scan"], **kw)
        add("obj_w_grad/" + tag, "obj_w_grad", h, d["geo4"], d["t0_pts"], **kw)
        add("obj_w_grad_nearest/" + tag, "obj_w_grad_nearest", h, d["geo4"], d["t0_pts"], d["sig_pts"], **kw)
        add("obj_w_grad_exact/" + tag, "obj_w_grad_exact", h, d["geo4"], d["t0_pts"], **kw)
        add("obj_w_grad_exact/sigma-" + tag, "obj_w_grad_exact", h, d["geo4"], d["t0_pts"], sigma=d["sig_pts"], **kw)
        add("obj_w_grad_exact_tangent/" + tag, "obj_w_grad_exact_tangent", h, d["geoT"], d["geoD"], d["t0_pts"], **kw)
        add("obj_w_grad_exact_tangent/sigma-" + tag, "obj_w_grad_exact_tangent", h, d["geoT"], d["geoD"], d["t0_pts"], sigma=0.63, **kw)
    add("gamma_scan_nearest/scalar-sigma", "gamma_scan_nearest", h, *scan, 1.0)
    add("obj_w_grad_nearest/scalar-sigma", "obj_w_grad_nearest", h, d["geo4"], d["t0_pts"], 0.61, del_alpha=0.01)
    add("obj_w_grad_exact/scalar-sigma", "obj_w_grad_exact", h, d["geo4"], d["t0_pts"], sigma=0.62, del_alpha=0.01)
    for m in ("obj_w_grad", "obj_w_grad_exact"):
        add(m + "/error-shape", m, h, bad4, d["t0_pts"])
    add("obj_w_grad_nearest/error-shape", "obj_w_grad_nearest", h, bad4, d["t0_pts"], 0.61)
    add("obj_w_grad_exact_tangent/error-shape", "obj_w_grad_exact_tangent", h, d["geoT"], badT, d["t0_pts"])
    # ---- counts, certificates, re-close
    add("hf_grad", "hf_grad", d["X"], d["dX"], f, d["g_p"], d["c_p"], d["f_p"], d["gam"])
    add("sturm_count", "sturm_count", h, g, c, f, d["sig_sys"])
    add("sturm_count/exact", "sturm_count", h, g, c, f, d["sig_sys"], exact=True)
    add("geo_sturm_count/default-shift", "geo_sturm_count", h, *scan)
    add("geo_sturm_count/scalar-shift", "geo_sturm_count", h, *scan, shift=0.29)
    add("geo_sturm_count/array-shift", "geo_sturm_count", h, *scan, shift=d["sig_scan"])
    add("certify_scan", "certify_scan", h, *scan, d["lam_scan"])
    add("certify_scan/tol", "certify_scan", h, *scan, d["lam_scan"], tol_factor=8.0)
    add("certify_points", "certify_points", h, *pts, d["lam_pts"])
    add("certify_points/error-theta0", "certify_points", h, *scan, d["lam_pts"])
    io = ("cert", "lam", "gam", "X", "dX")
    add("reclose_scan", "reclose_scan", h, *scan, d["cert_scan"], d["lam_scan"], d["gam_scan"], inout=io)
    add("reclose_scan/X-dX", "reclose_scan", h, *scan, d["cert_scan"], d["lam_scan"], d["gam_scan"], d["X_scan"], d["dX_scan"],
        tol_factor=8.0, inout=io)
    add("reclose_points", "reclose_points", h, *pts, d["cert_pts"], d["lam_pts"], d["gam_pts"], inout=io)
    add("reclose_points/X-dX", "reclose_points", h, *pts, d["cert_pts"], d["lam_pts"], d["gam_pts"], d["X_pts"], d["dX_pts"], inout=io)
    add("reclose_points/error-theta0", "reclose_points", h, *scan, d["cert_pts"], d["lam_pts"], d["gam_pts"], inout=io)
    add("reclose_scan/error-cert-missing", "reclose_scan", h, *scan, None, d["lam_scan"], d["gam_scan"], inout=io)
    add("reclose_scan/error-cert-dtype", "reclose_scan", h, *scan, d["lam_scan"], d["lam_scan"], d["gam_scan"], inout=io)
    add("reclose_scan/error-lam-not-contiguous", "reclose_scan", h, *scan, d["cert_scan"], d["X_scan"][:, :, 0], d["gam_scan"], inout=io)
    add("surface_argmax", "surface_argmax", d["gam_surf"])
    # ---- table-fed
    tb, ls, la, th = d["tables"], d["line_surf"], d["line_alpha"], d["theta"]
    kd = {} if device is None else dict(device=device)
    lines = [("", (ls, la, th))]
    if device is not None:
        lines.append(("host-lines-", tuple(d["np"][k] for k in ("line_surf", "line_alpha", "theta"))))
    else:
        lines.append(("list-lines-", ([1, 0], [0.25, 0.5], th)))
    oob = np.array([0, len(tb.s)], dtype=np.int32)
    la_h, th_h = d["np"]["line_alpha"], d["np"]["theta"]
    for ltag, ln in lines:
        add("fieldline_geometry/" + ltag + "rows", "fieldline_geometry", tb, *ln, **kd)
        add("fieldline_geometry/" + ltag + "no-rows", "fieldline_geometry", tb, *ln, use_rows=False, **kd)
        add("fieldline_geometry_dalpha/" + ltag + "plain", "fieldline_geometry_dalpha", tb, *ln, **kd)
        for want in (("tab_mn", "tab_nyq", "scal", "alpha"), ("tab_mn",), ("tab_nyq",), ("scal",), ("alpha",), ("scal", "alpha")):
            add("fieldline_geometry_vjp/" + ltag + "-".join(want), "fieldline_geometry_vjp", tb, *ln, d["geo_bar"], want=want, **kd)
        add("fieldline_geometry_vjp/" + ltag + "dPdrho_bar", "fieldline_geometry_vjp", tb, *ln, d["geo_bar"], d["dP_bar"], **kd)
    add("fieldline_geometry_vjp/error-want", "fieldline_geometry_vjp", tb, ls, la, th, d["geo_bar"], want=("beta",), **kd)
    add("fieldline_geometry_vjp/error-want-empty", "fieldline_geometry_vjp", tb, ls, la, th, d["geo_bar"], want=(), **kd)
    add("fieldline_geometry_vjp/error-geo_bar-shape", "fieldline_geometry_vjp", tb, ls, la, th, d["geo_bar"][:7], **kd)
    add("fieldline_geometry/line_surf-out-of-range", "fieldline_geometry", tb, oob, la_h, th_h, **kd)
    add("fieldline_geometry_vjp/line_surf-out-of-range", "fieldline_geometry_vjp", tb, oob, la_h, th_h, d["geo_bar"], **kd)
    add("fieldline_geometry_dalpha/line_surf-out-of-range", "fieldline_geometry_dalpha", tb, oob, la_h, th_h, **kd)
    pt_surf = np.array([1, 0], dtype=np.int32)
    add("refine", "refine", tb, pt_surf, d["np"]["starts"], th_h, **kd)
    add("refine/options", "refine", tb, [0, 1], d["np"]["starts"], th_h, del_alpha=0.01, maxiter=5, ftol=1e-9, gtol=1e-7, **kd)
    add("refine/error-starts", "refine", tb, pt_surf, d["np"]["starts"][:1], th_h, **kd)
    add("refine/error-pt_surf-out-of-range", "refine", tb, oob, d["np"]["starts"], th_h, **kd)
    if device is not None:
        # tabs brings its own surface count (twice the tables'): an index that only `tabs` holds, and one beyond both
        in_tabs = np.array([0, len(tb.s)], dtype=np.int32)
        beyond = np.array([0, 2 * len(tb.s)], dtype=np.int32)
        add("fieldline_geometry/tabs", "fieldline_geometry", tb, ls, la, th, tabs=d["tabs"], **kd)
        add("fieldline_geometry/tabs-host-lines-in-tabs", "fieldline_geometry", tb, in_tabs, la_h, th_h, tabs=d["tabs"], **kd)
        add("fieldline_geometry/tabs-host-lines-beyond", "fieldline_geometry", tb, beyond, la_h, th_h, tabs=d["tabs"], **kd)
        add("fieldline_geometry_vjp/tabs", "fieldline_geometry_vjp", tb, ls, la, th, d["geo_bar"], tabs=d["tabs"], **kd)
        add("fieldline_geometry_vjp/tabs-host-lines-beyond", "fieldline_geometry_vjp", tb, beyond, la_h, th_h, d["geo_bar"],
            tabs=d["tabs"], **kd)
        add("refine_device", "refine_device", tb, ls, d["starts"], th)
        add("refine_device/options", "refine_device", tb, ls, d["starts"], th, del_alpha=0.01, maxiter=5, ftol=1e-9, gtol=1e-7)
        add("gamma_scan_argmax", "gamma_scan_argmax", h, d["scan7"], d["dP"], d["t0_scan"], 2)
        add("gamma_scan_argmax/error-host", "gamma_scan_argmax", h, d["np"]["scan7"], d["np"]["dP"], d["np"]["t0_scan"], 2)
        add("scan_starts", "scan_starts", d["alpha_scan"], d["t0_scan"], d["pack"], d["n_bad"])
        add("scan_starts/sigma0", "scan_starts", d["alpha_scan"], d["t0_scan"], d["pack"], d["n_bad"], want_sigma0=True)
        add("surface_argmax_pack", "surface_argmax_pack", d["gam_surf"])
        add("upload_tables_rows/first-use", "upload_tables_rows", d["tables_fresh"], device, 0, 2)
        add("upload_tables_rows/again", "upload_tables_rows", d["tables_fresh"], device, 2, 4)
        add("surface_argmax_pack/error-host", "surface_argmax_pack", d["np"]["gam_surf"])
        add("mixed/solve_gcf", "solve_gcf", h, g, d["np"]["c"], f)
        add("mixed/gamma_scan", "gamma_scan", h, *d["scan7"], d["np"]["dP"], d["t0_scan"])
        add("mixed/solve_gcf_nearest-sigma", "solve_gcf_nearest", h, d["np"]["g"], d["np"]["c"], d["np"]["f"], d["sig_sys"])
    else:
        add("gamma_scan_argmax/error-host", "gamma_scan_argmax", h, d["scan7"], d["dP"], d["t0_scan"], 2)
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


# the one deliberate change of the marshalling refactor: line_surf is range-checked whenever it arrives as a host array, against the
# n_surf handed to the library.  Transcripts written before it differ in exactly these cases.
LINE_SURF_CASES = {
    "host": ("fieldline_geometry_vjp/line_surf-out-of-range", "fieldline_geometry_dalpha/line_surf-out-of-range"),
    "device": ("fieldline_geometry/tabs-host-lines-in-tabs",),
}


def load_solver(path):
    """another version of solver.py as a submodule of the installed package"""
    spec = importlib.util.spec_from_file_location("ibs_amd._solver_under_test", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def record_all(device=None, solver=None):
    """{case name: transcript} of every case, on a fresh Context of `solver` (default: the package's own)"""
    solver = solver or ibs_amd.solver
    with stand_in(device is not None) as fake:
        ctx = solver.Context(0)
        d = make_data(device)
        out = {}
        for name, method, args, kw, inout in cases(d, device):
            out[name] = run_case(ctx, fake, method, args, kw, inout)
        ctx.close()
    return out


if __name__ == "__main__":
    mode, dest = sys.argv[1], sys.argv[2]
    solver = load_solver(sys.argv[sys.argv.index("--solver") + 1]) if "--solver" in sys.argv else None
    dev = None
    if mode == "device":
        import torch
        dev = torch.device("cuda:0")
    rec = record_all(dev, solver)
    with open(dest, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("%d cases, %d library calls -> %s" % (len(rec), sum(len(v["calls"]) for v in rec.values()), dest))
