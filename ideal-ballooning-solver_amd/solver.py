"""Host-side handle on the HIP solver: one Context per process/GPU.

Accepts numpy arrays (host memory: staged by the library) or torch CUDA tensors (device memory:
zero-copy, asynchronous on the torch current stream).  Mirrors the reference operators'
argument meaning; see operators.py for the exact drop-in signatures.
"""
import contextlib
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import MEM_DEVICE, MEM_HOST, IbsError, check


class VjpStatusWarning(UserWarning):
    """solve_gcf_vjp flagged systems: status bit 1 (the pair is not an eigenpair of its rows, or invalid data: NaN rows) or status bit 0
    (a pivot of the adjoint solve fell below pivmin and was replaced: the rows may be inaccurate)"""


def vjp_status_message(n_pivot, n_bad):
    return ("solve_gcf_vjp: %d system(s) with a replaced pivot in the adjoint solve (status bit 0: rows may be inaccurate), %d not an "
            "eigenpair of their rows or with invalid data (status bit 1: NaN rows)" % (n_pivot, n_bad))


# ibs_obj_w_grad_exact_f64: (info >> EXACT_VJP_SHIFT) & 3 = the status of its adjoint solve in solve_gcf_vjp's convention (bit 0 a replaced
# pivot, bit 1 refused), i.e. status bits 6 and 7 of the info word
EXACT_VJP_SHIFT = 16 + 6

# spectrum mode (ibs_*_modes_f64): modes per system at most, and the informational status bit of a clustered mode (info >> 16)
MAX_MODES = 16
CLUSTER_BIT = 1 << 9
# ibs_solve_gcf_modes_basis_f64: the mode's vector is a member of its cluster's Ritz basis; the cluster continues below the last mode
BASIS_BIT, OPEN_CLUSTER_BIT = 1 << 13, 1 << 14
# multi-start refinement (ibs_scan_peaks_f64): starts per surface at most
MAX_STARTS = 16
MAX_ROW_STARTS = 4      # ibs_theta0_polish_f64: start slots per line


def _is_torch(x):
    return type(x).__module__.startswith("torch")




_F64, _F32, _I32 = np.dtype(np.float64), np.dtype(np.float32), np.dtype(np.int32)
_NULL = C.c_void_p(None)
_NO_ROWS = np.zeros((0, 2), np.int32)
_TORCH_DTYPES = {}


def _torch_dtype(dtype):
    if not _TORCH_DTYPES:
        import torch
        _TORCH_DTYPES.update({_F64: torch.float64, _F32: torch.float32, _I32: torch.int32})
    return _TORCH_DTYPES[dtype]


class _Args:
    """one library call of a Context: inputs and outputs are declared in the order of the C prototype (each declaration returns the
    pointer to pass), call() makes the call, result() returns the outputs.  The memory kind of the call is that of its first array
    (all numpy or all torch-cuda); device=...: a call on that device whatever comes first, host arrays go up with upload=True."""

    def __init__(self, ctx, dtype=_F64, device=None, host=False):
        self.ctx = ctx
        self.dtype = np.dtype(dtype)
        self.mem = MEM_HOST if host else None if device is None else MEM_DEVICE
        self.ref = device       # the torch device of a device call: where outputs are allocated and whose current stream is used
        self.keep = []          # converted copies, uploads and outputs: alive during the call
        self.temps = []         # device temporaries the (asynchronous) call reads: alive until the context's next such call
        self.outs = {}

    def _set(self, mem):
        if self.mem is None:
            self.mem = mem
        elif self.mem != mem:
            raise IbsError("mixing host (numpy) and device (torch.cuda) arrays in one call is not supported")

    def inp(self, x, dtype=None, upload=False):
        """pointer to x as a contiguous array of dtype (default: the call's); None -> a null pointer"""
        if x is None:
            return _NULL
        dtype = self.dtype if dtype is None else dtype
        if _is_torch(x):
            if not x.is_cuda:
                raise IbsError("torch tensors must live on the GPU (got %s)" % x.device)
            td = _torch_dtype(dtype)
            if x.dtype != td or not x.is_contiguous():
                x = x.to(td).contiguous()
                self.temps.append(x)
            self._set(MEM_DEVICE)
            if self.ref is None:
                self.ref = x.device
            self.keep.append(x)
            return C.c_void_p(x.data_ptr())
        a = np.ascontiguousarray(x, dtype=dtype)
        if upload and self.mem == MEM_DEVICE:
            import torch
            t = torch.from_numpy(a).to(self.ref)
            self.temps.append(t)
            return C.c_void_p(t.data_ptr())
        self._set(MEM_HOST)
        self.keep.append(a)
        return C.c_void_p(a.ctypes.data)

    def rows(self, x, shape):
        """a scalar-or-array input (sigma, shift, gam_bar, lam_bar) as float64 of `shape` in the memory kind of the call"""
        if x is None:
            return _NULL
        if self.mem == MEM_DEVICE:
            import torch
            t = torch.as_tensor(x, dtype=torch.float64, device=self.ref)
            return self.inp(t.expand(shape).contiguous() if t.dim() == 0 else t.reshape(shape))
        a = np.asarray(x.detach().cpu().numpy() if _is_torch(x) else x, dtype=np.float64)
        return self.inp(np.broadcast_to(a, shape) if a.ndim == 0 else a.reshape(shape))

    def geo(self, h, geo7, dPdrho, theta0, points=False):
        """the leading arguments of a geometry-fed entry point: seven (n_lines, N) arrays, dPdrho (n_lines,) and theta0 --
        (n_theta0,) of a scan, one per line of a points call -> (arguments up to theta0, shape of one output, N)"""
        n_lines, N = geo7[0].shape
        shape = (n_lines,) if points else (n_lines, int(theta0.shape[0]))
        return [*shape, N, float(h), *[self.inp(a) for a in geo7], N, self.inp(dPdrho), self.inp(theta0)], shape, N

    def lines(self, line_surf, line_alpha, theta, n_surf, what="line_surf"):
        """(line_surf, line_alpha, theta) as int32 / float64 / float64 in the memory kind of the call: resident tensors pass through
        (the geometry kernel clamps the surface index itself), host arrays are uploaded for a device call; a host line_surf is
        range-checked against the n_surf the library is given"""
        if not _is_torch(line_surf):
            line_surf = np.ascontiguousarray(line_surf, dtype=np.int32)
            if line_surf.size and (line_surf.min() < 0 or line_surf.max() >= n_surf):
                raise IbsError("%s out of range" % what)
        return self.inp(line_surf, _I32, True), self.inp(line_alpha, _F64, True), self.inp(theta, _F64, True)

    def tables(self, tables, tabs=None, use_rows=True):
        """the table arguments of a table-fed entry point -> (n_surf, [n_surf, mnmax, mnmax_nyq, seven table pointers], [n_rows,
        rows, n_rows_nyq, rows_nyq, dn, dn_nyq]); a device call reads the copies resident on its device (uploaded once and kept ON
        the tables object: a cache keyed by id(tables) would hand a later object that re-uses the id the previous object's tables),
        with `tabs` = (tab_mn, tab_nyq, scal) in place of the last three"""
        if self.mem == MEM_DEVICE:
            dev = self.ctx._device_tables(tables, self.ref)
            seven, rows = (dev[:7] if tabs is None else dev[:4] + list(tabs)), dev[7:]
        else:
            tabs = None         # (device calls only)
            seven = (tables.xm, tables.xn, tables.xm_nyq, tables.xn_nyq, tables.tab_mn, tables.tab_nyq, tables.scal)
            rows = (tables.rows_mn, tables.rows_nyq) if use_rows else (_NO_ROWS, _NO_ROWS)
        n_surf = len(tables.s) if tabs is None else int(tabs[2].shape[0])
        nr = (len(tables.rows_mn), len(tables.rows_nyq)) if use_rows else (0, 0)
        return (n_surf, [n_surf, len(tables.xm), len(tables.xm_nyq), *[self.inp(a) for a in seven]],
                [nr[0], self.inp(rows[0], _I32), nr[1], self.inp(rows[1], _I32), float(tables.dn_mn), float(tables.dn_nyq)])

    def out(self, name, shape, dtype=None, want=True):
        """pointer to a new array the call fills, returned under `name`; want=False: a null pointer and no entry"""
        if not want:
            return _NULL
        dtype = self.dtype if dtype is None else dtype
        if self.mem == MEM_DEVICE:
            import torch
            t = self.outs[name] = torch.empty(shape, dtype=_torch_dtype(dtype), device=self.ref)
            return C.c_void_p(t.data_ptr())
        a = self.outs[name] = np.empty(shape, dtype=dtype)
        return C.c_void_p(a.ctypes.data)

    def inout(self, what, name, a, dtype, optional=False):
        """pointer to the caller's own array, which the call updates in place: it must already be what the library reads"""
        if a is None:
            if optional:
                return _NULL
            raise IbsError("%s: %s is required" % (what, name))
        if _is_torch(a):
            ok = a.is_cuda and a.is_contiguous() and a.dtype == _torch_dtype(dtype)
        else:
            ok = isinstance(a, np.ndarray) and a.flags.c_contiguous and a.flags.writeable and a.dtype == dtype
        if not ok:
            raise IbsError("%s: %s is updated in place and must be a contiguous %s array" % (what, name, dtype.name))
        return self.inp(a, dtype)

    def call(self, name, *args, mem=True):
        """ibs_<name>(handle, *args[, mem]) on the current torch stream of a device call -> its checked return value"""
        ctx = self.ctx
        if self.mem == MEM_DEVICE:
            ctx._stream_from_torch(self.ref)
            if self.temps:
                ctx._keep = self.temps
        fn = getattr(ctx._lib, name)
        return check(fn(ctx._h, *args, self.mem) if mem else fn(ctx._h, *args), name)

    def result(self, nbad=None):
        """dict of the wanted outputs[, nbad]"""
        if nbad is not None:
            self.outs["nbad"] = nbad
        return self.outs


def _refine_views(buf, n):
    """the packed result of ibs_refine_f64, 4 n float64 words = x_opt (n, 2) | f_opt (n,) | n_evals (n,) int32 in the rest: one
    buffer, so that a device call's results come back in one copy"""
    i32 = np.int32 if isinstance(buf, np.ndarray) else _torch_dtype(_I32)
    return buf[:2 * n].reshape(n, 2), buf[2 * n:3 * n], buf[3 * n:].view(i32)[:n]


def _device_key(device):
    """'cuda:<index>' for every spelling of one device (torch.device('cuda'), 'cuda', 'cuda:0', a tensor's .device): the
    key of the resident copies a table set keeps per device, so that an upload under one spelling is found under another"""
    import torch
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return str(d)


class Context:
    def __init__(self, device=0):
        self._lib = _lib.lib()
        self._h = C.c_void_p(None)
        check(self._lib.ibs_create(C.byref(self._h), int(device)), "ibs_create")
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._comm_world = 0
            self._lib.ibs_destroy(self._h)
            self._h = C.c_void_p(None)

    __del__ = close

    def _stream_from_torch(self, ref):
        """the library works on the current torch stream of ref's device (ref: a tensor or a torch.device)"""
        import torch
        self._lib.ibs_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(getattr(ref, "device", ref)).cuda_stream))

    def synchronize(self):
        check(self._lib.ibs_synchronize(self._h), "ibs_synchronize")

    # ---- native RCCL all-gather (include/ibs.h: ibs_comm_*) -------------------------------------------------
    def comm_init(self, dist, rank, world):
        """create this rank's RCCL communicator inside the library; the unique id travels through `dist`
        (any initialised torch.distributed backend).  Collective over all ranks."""
        import torch
        # (IBS_RCCL_LIB: another library with RCCL's five entry points -- the shared-memory stand-in tests/cabi/fake_rccl.c lets the
        #  multi-rank code run on a one-GPU box, where RCCL refuses two ranks on one device)
        rccl = os.environ.get("IBS_RCCL_LIB") or os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        # every rank takes part in the same collectives of `dist` whatever fails locally (a rank that raised before the
        # broadcast would leave the others waiting in it): load, id, broadcast, agreement, and only then ncclCommInitRank
        ident = C.create_string_buffer(128)
        problem = None
        try:
            check(self._lib.ibs_comm_load(rccl.encode() if os.path.exists(rccl) else None), "ibs_comm_load")
            if rank == 0:
                check(self._lib.ibs_comm_unique_id(ident), "ibs_comm_unique_id")
        except IbsError as e:
            problem = str(e)
        box = [ident.raw if (rank == 0 and problem is None) else None]
        if world > 1:
            dist.broadcast_object_list(box, src=0)
            seen = [None] * world
            dist.all_gather_object(seen, problem)
        else:
            seen = [problem]
        if box[0] is None or any(p is not None for p in seen):
            raise IbsError("native RCCL communicator not available on every rank: %s" % ([p for p in seen if p] or ["no id from rank 0"])[0])
        ident = C.create_string_buffer(box[0], 128)
        check(self._lib.ibs_comm_init(self._h, ident, int(rank), int(world)), "ibs_comm_init")
        self._comm_world = int(world)

    def allgather(self, send, recv):
        """recv (world * n,) <- every rank's send (n,): float64 CUDA tensors, asynchronous on the current torch stream"""
        self._stream_from_torch(send)
        check(self._lib.ibs_comm_allgather_f64(self._h, C.c_void_p(send.data_ptr()), C.c_void_p(recv.data_ptr()),
                                               send.numel()), "ibs_comm_allgather_f64")

    def allgather_start(self, send, recv, slot=0, then_wait=-1, same_stream=False, host_wait=None):
        """the same gather on the communicator's own stream, ordered after the work enqueued so far on the current torch
        stream: later launches do not wait for it.  comm_wait(slot) before `send` / `recv` are reused or read;
        then_wait >= 0 does comm_wait(then_wait) in the same call; host_wait = s instead waits for slot s on the host
        (no stream operation; for callers that run several slots ahead).  same_stream: the context's stream is already
        the current torch stream (the call follows a launch of this context)."""
        if host_wait is not None:
            then_wait = -2 - int(host_wait)
        if not same_stream:
            self._stream_from_torch(send)
        check(self._lib.ibs_comm_allgather_start_f64(self._h, C.c_void_p(send.data_ptr()), C.c_void_p(recv.data_ptr()),
                                                     send.numel(), int(slot), int(then_wait)), "ibs_comm_allgather_start_f64")

    def comm_wait(self, slot=-1):
        """order the context's stream after the overlapped gather of `slot` (default: all pending); the host does not block"""
        check(self._lib.ibs_comm_wait(self._h, int(slot)), "ibs_comm_wait")

    def comm_destroy(self):
        self._comm_world = 0            # gathers go back to torch.distributed
        check(self._lib.ibs_comm_destroy(self._h), "ibs_comm_destroy")

    def last_launch(self):
        """(kernel name as rocprofv3 prints it, waves of the launch) of the solver / geometry kernel this thread launched last"""
        buf = C.create_string_buffer(96)
        nb, nt = _lib._I64(0), _lib._I32(0)
        self._lib.ibs_last_launch(buf, 96, C.byref(nb), C.byref(nt))
        return buf.value.decode(), int(nb.value) * int(nt.value) // 64

    def set_option(self, name, value):
        """diagnostic override of a dispatch heuristic of this context (include/ibs.h: ibs_set_option);
        value None = back to the context's default"""
        check(self._lib.ibs_set_option(self._h, name.encode(), float("nan") if value is None else float(value)),
              "ibs_set_option")
        mine = self.__dict__.setdefault("_options", {})      # what the caller holds overridden (option_default() leaves those alone)
        if name == "all":
            mine.clear()
        elif value is None:
            mine.pop(name, None)
        elif name != "forget_rows":
            mine[name] = float(value)

    @contextlib.contextmanager
    def option_default(self, name, value):
        """`name` = value inside the block unless the caller holds the option overridden through set_option (then theirs stands);
        afterwards the option is back at the context's default"""
        if name in self.__dict__.get("_options", {}):
            yield
            return
        self.set_option(name, value)
        try:
            yield
        finally:
            self.set_option(name, None)

    def reset_options(self):
        self.set_option("all", None)


    # ---- raw (g, c, f) systems --------------------------------------------------------------
    def solve_gcf(self, h, g, c, f, want_X=False, want_info=False, dtype=np.float64, gh=None, want_gam=True):
        """g, c, f: (n_sys, N).  Returns dict(lam, gam[, X, dX][, info]).  gh (n_sys, N) optional half-grid g
        (first N-1 columns used): see ibs_solve_gcfh_f64.  float32: with want_gam / want_X the systems are widened to
        FP64 inside the solver (FP32 in HBM only); want_gam=False and no X = the all-FP32 kernel, eigenvalues only."""
        ar = _Args(self, dtype)
        n_sys, N = g.shape
        name = "ibs_solve_gcfh_f64" if gh is not None else "ibs_solve_gcf_f64" if ar.dtype == _F64 else "ibs_solve_gcf_f32"
        half = () if gh is None else (ar.inp(gh),)
        rc = ar.call(name, n_sys, N, float(h), ar.inp(g), *half, ar.inp(c), ar.inp(f), N, ar.out("lam", (n_sys,)),
                     ar.out("gam", (n_sys,), want=want_gam), ar.out("X", (n_sys, N), want=want_X), ar.out("dX", (n_sys, N), want=want_X),
                     ar.out("info", (n_sys,), _I32, want_info))
        out = ar.result(rc)
        out.setdefault("gam", None)
        return out

    def solve_gcf_nearest(self, h, g, c, f, sigma, gh=None, want_X=False, want_info=False):
        """the eigenpair NEAREST sigma (ibs_solve_gcf_nearest_f64: what utils.py:1597's eigs(A, 1, sigma=sigma0) returns).
        g, c, f (and gh, optional half-grid g as in solve_gcf): (n_sys, N); sigma: a scalar or (n_sys,).
        Returns dict(lam, idx, gam[, X, dX][, info], nbad): idx = the number of eigenvalues above lam (0 = lam_max, -1 = invalid
        data); info status bit 5 = the two eigenvalues about sigma are equally near within 4 N eps ||A|| (the larger is returned)."""
        ar = _Args(self)
        n_sys, N = g.shape
        rc = ar.call("ibs_solve_gcf_nearest_f64", n_sys, N, float(h), ar.inp(g), ar.inp(gh), ar.inp(c), ar.inp(f), N,
                     ar.rows(sigma, (n_sys,)), ar.out("lam", (n_sys,)), ar.out("idx", (n_sys,), _I32), ar.out("gam", (n_sys,)),
                     ar.out("X", (n_sys, N), want=want_X), ar.out("dX", (n_sys, N), want=want_X), ar.out("info", (n_sys,), _I32, want_info))
        return ar.result(rc)

    @staticmethod
    def _n_modes(n_modes):
        ok = isinstance(n_modes, (int, float, np.integer, np.floating)) and not isinstance(n_modes, bool)
        if not ok or int(n_modes) != n_modes or not 1 <= n_modes <= MAX_MODES:
            raise IbsError("n_modes must be an integer in [1, %d], not %r" % (MAX_MODES, n_modes))
        return int(n_modes)

    def solve_gcf_modes(self, h, g, c, f, n_modes, gh=None, want_X=False, want_info=False, basis=False):
        """the n_modes LARGEST eigenpairs of every system (ibs_solve_gcf_modes_f64), 1 <= n_modes <= 16: g, c, f (and gh, optional
        half-grid g as in solve_gcf): (n_sys, N).  Returns dict(lam, gam[, X, dX][, info], nbad): lam, gam, info (n_sys, n_modes),
        mode 0 = lam_max and the eigenvalues descending; X, dX (n_sys, n_modes, N), the entry of largest magnitude +1.  info
        status bit 9 (CLUSTER_BIT, per mode, informational): a neighbouring eigenvalue lies within 4 N eps ||A|| -- lam holds, the
        vector is some vector of the cluster's invariant subspace and gam its quotient.
        basis=True (ibs_solve_gcf_modes_basis_f64): the members of every cluster get an F-orthonormal Ritz basis of the cluster
        (status bits BASIS_BIT, OPEN_CLUSTER_BIT; include/ibs.h); X and dX are always returned, and cluster_first (n_sys, n_modes)
        int32, the first mode of every mode's cluster (its own index where it is in none).  Everything else as with basis=False, bit
        for bit."""
        K = self._n_modes(n_modes)
        if len(g.shape) != 2:
            raise IbsError("solve_gcf_modes: g must be (n_sys, N), not %s" % (tuple(g.shape),))
        n_sys, N = g.shape
        for name, a in (("c", c), ("f", f), ("gh", gh)):
            if a is not None and tuple(a.shape) != (n_sys, N):
                raise IbsError("solve_gcf_modes: %s must be (%d, %d) like g, not %s" % (name, n_sys, N, tuple(a.shape)))
        ar = _Args(self)
        if basis:
            rc = ar.call("ibs_solve_gcf_modes_basis_f64", n_sys, N, float(h), ar.inp(g), ar.inp(gh), ar.inp(c), ar.inp(f), N, K,
                         ar.out("lam", (n_sys, K)), ar.out("gam", (n_sys, K)), ar.out("X", (n_sys, K, N)), ar.out("dX", (n_sys, K, N)),
                         ar.out("cluster_first", (n_sys, K), _I32), ar.out("info", (n_sys, K), _I32, want_info))
            return ar.result(rc)
        rc = ar.call("ibs_solve_gcf_modes_f64", n_sys, N, float(h), ar.inp(g), ar.inp(gh), ar.inp(c), ar.inp(f), N, K,
                     ar.out("lam", (n_sys, K)), ar.out("gam", (n_sys, K)), ar.out("X", (n_sys, K, N), want=want_X),
                     ar.out("dX", (n_sys, K, N), want=want_X), ar.out("info", (n_sys, K), _I32, want_info))
        return ar.result(rc)

    def solve_gcf_vjp(self, h, g, c, f, lam, X, gam_bar=None, lam_bar=None, want_info=False):
        """exact vector-Jacobian product of gam and lam in the rows (ibs_solve_gcf_vjp_f64): g, c, f, X (n_sys, N), lam (n_sys,), the
        eigenpair any simple one of the rows (solve_gcf's or solve_gcf_nearest's); gam_bar, lam_bar (n_sys,) or scalars, either may be
        None (= 0), not both.  Returns dict(g_bar, c_bar, f_bar[, info], nbad) with rows (n_sys, N); a system whose (lam, X) is not
        an eigenpair of its rows (or whose data are invalid) gets status bit 1 and NaN rows."""
        if gam_bar is None and lam_bar is None:
            raise IbsError("solve_gcf_vjp: gam_bar and lam_bar are both None")
        ar = _Args(self)
        n_sys, N = g.shape
        rc = ar.call("ibs_solve_gcf_vjp_f64", n_sys, N, float(h), ar.inp(g), ar.inp(c), ar.inp(f), N, ar.inp(lam), ar.inp(X),
                     ar.rows(gam_bar, (n_sys,)), ar.rows(lam_bar, (n_sys,)), ar.out("g_bar", (n_sys, N)), ar.out("c_bar", (n_sys, N)),
                     ar.out("f_bar", (n_sys, N)), ar.out("info", (n_sys,), _I32, want_info))
        return ar.result(rc)

    # ---- marginal stability -----------------------------------------------------------------
    def marginal_gcf(self, h, g, c, want_X=False, want_grad=False, want_info=False):
        """the critical scale s* of c at fixed g (ibs_marginal_gcf_f64): the factor by which the pressure gradient of a line may be
        scaled, at fixed geometry arrays, before the line goes unstable; s* < 1 = unstable now.  g, c: (n_sys, N).
        Returns dict(scale, mu = 1 / s*[, X, gam0][, g_bar, c_bar][, info], nbad): X the marginal mode (zero ends, largest entry +1),
        gam0 its FD4 / Simpson quotient (O(h^2) from 0), g_bar / c_bar = d s* / d g, d s* / d c (n_sys, N).  info status bit 8: no
        c_j > 0, scale = inf and mu = 0 (not counted in nbad)."""
        ar = _Args(self)
        n_sys, N = g.shape
        rc = ar.call("ibs_marginal_gcf_f64", n_sys, N, float(h), ar.inp(g), ar.inp(c), N, ar.out("scale", (n_sys,)), ar.out("mu", (n_sys,)),
                     ar.out("X", (n_sys, N), want=want_X), ar.out("gam0", (n_sys,), want=want_X), ar.out("g_bar", (n_sys, N), want=want_grad),
                     ar.out("c_bar", (n_sys, N), want=want_grad), ar.out("info", (n_sys,), _I32, want_info))
        return ar.result(rc)

    def marginal_scan(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, want_grad=False, want_info=False):
        """the critical scale of dPdrho of every (line, theta0), at fixed geometry arrays (ibs_marginal_scan_f64): arrays as in
        gamma_scan.  Returns dict(scale, mu[, dscale_dtheta0, dscale_ddPdrho][, info], nbad) shaped (n_lines, n_theta0);
        dPdrho_crit = scale * dPdrho[:, None]."""
        ar = _Args(self)
        head, shape, N = ar.geo(h, (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22), dPdrho, theta0)
        rc = ar.call("ibs_marginal_scan_f64", *head, ar.out("scale", shape), ar.out("mu", shape),
                     ar.out("dscale_dtheta0", shape, want=want_grad), ar.out("dscale_ddPdrho", shape, want=want_grad),
                     ar.out("info", shape, _I32, want_info))
        return ar.result(rc)

    def marginal_theta0_polish(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, mu, n_starts=1, xtol=1e-5,
                               max_eval=32, node=None, want_scale=True, want_info=False, want_found=True):
        """mu = 1 / s* of every line maximised over theta0 between the nodes of its coarse row (ibs_marginal_theta0_polish_f64; the
        rule: scan.row_peaks and scan.polish_theta0): about the n_starts <= 4 best peaks of mu[line], or about the nodes the caller
        names.  Arrays as in marginal_scan, any odd N in [66, 65537]; theta0 (n_theta0,): finite and strictly increasing; mu (n_lines,
        n_theta0): marginal_scan's mu on these lines; node int32 (n_lines, n_starts), optional: the nodes to polish about (-1 = skip
        the slot) instead of the row's own peaks.
        Returns dict(theta0, mu (n_lines, n_starts)[, scale = s* at theta0: bitwise marginal_scan's there], node, n_eval int32
        (n_lines, n_starts)[, info int32: multisection passes | status << 16][, n_found int32 (n_lines,)], nbad): mu is never below
        the coarse row; status bit 8 = the returned point has scale = inf (mu = 0), bit 10 = the node itself was returned, bit 11 =
        max_eval reached, bit 12 = one-sided bracket.  Slots from n_found on repeat slot 0; a row without a finite entry gives NaN."""
        K = int(n_starts)
        if K != n_starts or not 1 <= K <= MAX_ROW_STARTS:
            raise IbsError("n_starts must be an integer in [1, %d], not %r" % (MAX_ROW_STARTS, n_starts))
        geo = (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22)
        shape = (int(geo[0].shape[0]), int(theta0.shape[0]))
        if tuple(mu.shape) != shape:
            raise IbsError("marginal_theta0_polish: mu must be %s, not %s" % (shape, tuple(mu.shape)))
        slots = (shape[0], K)
        if node is not None and tuple(node.shape) != slots:
            raise IbsError("marginal_theta0_polish: node must be %s, not %s" % (slots, tuple(node.shape)))
        ar = _Args(self)
        head, _, N = ar.geo(h, geo, dPdrho, theta0)
        rc = ar.call("ibs_marginal_theta0_polish_f64", *head, ar.inp(mu), ar.inp(node, _I32), K, float(xtol), int(max_eval),
                     ar.out("theta0", slots), ar.out("mu", slots), ar.out("scale", slots, want=want_scale), ar.out("node", slots, _I32),
                     ar.out("n_eval", slots, _I32), ar.out("info", slots, _I32, want_info), ar.out("n_found", (shape[0],), _I32, want_found))
        return ar.result(rc)

    # ---- local-equilibrium scan -------------------------------------------------------------
    def local_eq_scan(self, theta_lo, h, geo, dPdrho, centre, sigma, var, ps=None, shift=0.0, count_only=False, want_info=False):
        """gam, lam_max and the number of eigenvalues above `shift` of every line under the variations var of its surface's shear and
        pressure gradient (ibs_local_eq_scan_f64; the rule: operators.local_eq_fold).  geo (8, n_lines, N): fieldline_geometry's
        output on the uniform grid theta_lo + j h; dPdrho, centre (= alpha of such lines), sigma (= sign(-phiedge), +-1) (n_lines,);
        var (n_var, 3) = (theta0, eps, p); ps (n_lines, N), optional.  The memory kind is geo's; the small arrays may be numpy either
        way.  count_only=True: the count alone, no eigenvalue is computed (the stable / unstable diagram).
        Returns dict([gam, lam, ]count int32[, info int32], nbad) shaped (n_lines, n_var).  A line with non-finite data, a sigma
        that is not +-1 or a non-finite triple gives status 2, NaN gam and lam and count -1 on those systems alone."""
        eight, n_lines, N = geo.shape
        if eight != 8:
            raise IbsError("geo must be (8, n_lines, N)")
        n_var = int(var.shape[0])
        if tuple(var.shape) != (n_var, 3):
            raise IbsError("var must be (n_var, 3) = (theta0, eps, p)")
        if ps is not None and tuple(ps.shape) != (n_lines, N):
            raise IbsError("ps must be (n_lines, N) = %s, not %s" % ((n_lines, N), tuple(ps.shape)))
        ar = _Args(self)
        shape = (n_lines, n_var)
        pgeo = ar.inp(geo)
        rc = ar.call("ibs_local_eq_scan_f64", n_lines, n_var, N, float(theta_lo), float(h), pgeo, N, ar.inp(dPdrho, upload=True),
                     ar.inp(centre, upload=True), ar.inp(sigma, upload=True), ar.inp(ps, upload=True), N, ar.inp(var, upload=True),
                     float(shift), ar.out("gam", shape, want=not count_only), ar.out("lam", shape, want=not count_only),
                     ar.out("count", shape, _I32), ar.out("info", shape, _I32, want_info))
        return ar.result(rc)

    # ---- local-equilibrium boundaries --------------------------------------------------------
    def local_eq_boundary(self, theta_lo, h, geo, dPdrho, centre, sigma, rays, ps=None, shift=0.0, max_cross=4, xtol=1e-12,
                          want_nodes=False, want_info=False):
        """The parameters t at which every line crosses the stability boundary ("an eigenvalue above `shift`") along the rays
        (n_ray, 7) = (theta0, eps0, p0, d_eps, d_p, t_lo, t_hi) in the (eps, p) plane of the local-equilibrium rule
        (ibs_local_eq_boundary_f64; triples of a ray: operators.local_eq_ray_triples), closed on the device to xtol (t_hi - t_lo).
        The other arguments are local_eq_scan's.  A crossing is a change of verdict between two of the 64 nodes
        operators.local_eq_ray_nodes(rays); the first max_cross (1 .. 4) in increasing t are closed and returned.
        Returns dict(t_stable, t_unstable, t = their mean (n_lines, n_ray, max_cross), NaN beyond n_cross; n_cross, lo_unstable = the
        verdict at t_lo, int32 (n_lines, n_ray)[; node_count int32 (n_lines, n_ray, 64) = the counts at the nodes][; info], nbad).
        info: bits 0-15 passes over the rows; status (info >> 16) bit 0 pass cap, 1 invalid system (NaN, n_cross -1: non-finite line
        data, g or f <= 0 on the ray, sigma not +-1, a non-finite ray or t_lo >= t_hi), 2 more than max_cross crossings, 3 the
        bracket's ends became neighbours in FP64 before xtol was met.  A tangency and two crossings between one pair of nodes are
        missed: narrow the range or split the ray."""
        eight, n_lines, N = geo.shape
        if eight != 8:
            raise IbsError("geo must be (8, n_lines, N)")
        n_ray = int(rays.shape[0])
        if tuple(rays.shape) != (n_ray, 7):
            raise IbsError("rays must be (n_ray, 7) = (theta0, eps0, p0, d_eps, d_p, t_lo, t_hi)")
        if ps is not None and tuple(ps.shape) != (n_lines, N):
            raise IbsError("ps must be (n_lines, N) = %s, not %s" % ((n_lines, N), tuple(ps.shape)))
        max_cross = int(max_cross)
        ar = _Args(self)
        shape = (n_lines, n_ray)
        pgeo = ar.inp(geo)
        cross = shape + (max(max_cross, 0),)
        rc = ar.call("ibs_local_eq_boundary_f64", n_lines, n_ray, N, float(theta_lo), float(h), pgeo, N, ar.inp(dPdrho, upload=True),
                     ar.inp(centre, upload=True), ar.inp(sigma, upload=True), ar.inp(ps, upload=True), N, ar.inp(rays, upload=True),
                     float(shift), max_cross, float(xtol), ar.out("t_stable", cross), ar.out("t_unstable", cross),
                     ar.out("n_cross", shape, _I32), ar.out("lo_unstable", shape, _I32),
                     ar.out("node_count", shape + (64,), _I32, want_nodes), ar.out("info", shape, _I32, want_info))
        res = ar.result(rc)
        res["t"] = 0.5 * (res["t_stable"] + res["t_unstable"])
        return res

    def local_eq_boundary_polish(self, theta_lo, h, geo, dPdrho, centre, sigma, rays, theta0, t_row, ps=None, shift=0.0, xtol=1e-12,
                                 n_starts=1, xtol_theta0=1e-5, max_eval=32, want_info=True):
        """The first-stability parameter T of every (line, ray family) minimised over theta0 between the nodes theta0 (n_theta0,) of
        the coarse row t_row (n_lines, n_ray, n_theta0) = T at the nodes (ibs_local_eq_boundary_polish_f64; the rule:
        scan.local_eq_first_up and scan.polish_first_up).  A family is a ray of local_eq_boundary whose entry 0 is replaced by the
        theta0 under evaluation; every evaluation is local_eq_boundary(max_cross=1) at that theta0, bit for bit.  t_row: +inf where a
        node has no crossing, t_lo where it is unstable at t_lo, NaN where it is not to be used.  The other arguments are
        local_eq_boundary's; n_starts <= 4 slots per row, xtol_theta0 absolute, max_eval <= 64.
        Returns dict(theta0, t, t_stable, t_unstable (n_lines, n_ray, n_starts); node, n_eval, lo_unstable[, info] int32 of that shape;
        n_found int32 (n_lines, n_ray), nbad).  t is never above the node's T.  Status (info >> 16) bits 0-1 are failures (bit 1: NaN
        outputs), bit 3 and bits 10 (the node itself is returned), 11 (max_eval reached), 12 (one-sided bracket) informational."""
        K = int(n_starts)
        if K != n_starts or not 1 <= K <= MAX_ROW_STARTS:
            raise IbsError("n_starts must be an integer in [1, %d], not %r" % (MAX_ROW_STARTS, n_starts))
        eight, n_lines, N = geo.shape
        if eight != 8:
            raise IbsError("geo must be (8, n_lines, N)")
        n_ray, n_theta0 = int(rays.shape[0]), int(theta0.shape[0])
        if tuple(rays.shape) != (n_ray, 7):
            raise IbsError("rays must be (n_ray, 7) = (-, eps0, p0, d_eps, d_p, t_lo, t_hi)")
        if ps is not None and tuple(ps.shape) != (n_lines, N):
            raise IbsError("ps must be (n_lines, N) = %s, not %s" % ((n_lines, N), tuple(ps.shape)))
        if tuple(t_row.shape) != (n_lines, n_ray, n_theta0):
            raise IbsError("local_eq_boundary_polish: t_row must be %s, not %s" % ((n_lines, n_ray, n_theta0), tuple(t_row.shape)))
        ar = _Args(self)
        slots = (n_lines, n_ray, K)
        pgeo = ar.inp(geo)
        rc = ar.call("ibs_local_eq_boundary_polish_f64", n_lines, n_ray, N, float(theta_lo), float(h), pgeo, N, ar.inp(dPdrho, upload=True),
                     ar.inp(centre, upload=True), ar.inp(sigma, upload=True), ar.inp(ps, upload=True), N, ar.inp(rays, upload=True),
                     n_theta0, ar.inp(theta0, upload=True), ar.inp(t_row, upload=True), float(shift), float(xtol), K, float(xtol_theta0),
                     int(max_eval), ar.out("theta0", slots), ar.out("t", slots), ar.out("t_stable", slots), ar.out("t_unstable", slots),
                     ar.out("node", slots, _I32), ar.out("n_eval", slots, _I32), ar.out("lo_unstable", slots, _I32),
                     ar.out("info", slots, _I32, want_info), ar.out("n_found", (n_lines, n_ray), _I32))
        return ar.result(rc)

    # ---- local-equilibrium gradients --------------------------------------------------------
    def local_eq_grad(self, theta_lo, h, geo, dPdrho, centre, sigma, line_of, var, ps=None, want_grad=True, want_geo_bar=False,
                      want_info=False):
        """lam_max and gam at the points (line_of[k], theta0, eps, p) of the local-equilibrium rule with the exact derivatives of lam_max
        (ibs_local_eq_grad_f64; numpy: operators.local_eq_lam_grad).  geo, dPdrho, centre, sigma, ps: local_eq_scan's; line_of int32
        (n_pts,): the line of each point; var (n_pts, 3) = (theta0, eps, p).  The memory kind is geo's; the small arrays may be numpy.
        Returns dict(lam, gam (n_pts,)[, dlam (n_pts, 4) = d lam / d (theta0, eps, p, dPdrho)][, geo_bar (8, n_pts, N) = d lam / d (the
        eight arrays of the point's line)][, info], nbad).  want_grad=False and want_geo_bar=False: no mode is kept, lam and gam are
        local_eq_scan's bits.  A point with status bit 0 or 1 (line_of out of range included) is NaN in every output."""
        eight, n_lines, N = geo.shape
        if eight != 8:
            raise IbsError("geo must be (8, n_lines, N)")
        n_pts = int(var.shape[0])
        if tuple(var.shape) != (n_pts, 3) or tuple(line_of.shape) != (n_pts,):
            raise IbsError("var must be (n_pts, 3) = (theta0, eps, p) and line_of (n_pts,)")
        if ps is not None and tuple(ps.shape) != (n_lines, N):
            raise IbsError("ps must be (n_lines, N) = %s, not %s" % ((n_lines, N), tuple(ps.shape)))
        ar = _Args(self)
        pgeo = ar.inp(geo)
        rc = ar.call("ibs_local_eq_grad_f64", n_lines, n_pts, N, float(theta_lo), float(h), pgeo, N, ar.inp(dPdrho, upload=True),
                     ar.inp(centre, upload=True), ar.inp(sigma, upload=True), ar.inp(ps, upload=True), N, ar.inp(line_of, _I32, True),
                     ar.inp(var, upload=True), ar.out("lam", (n_pts,)), ar.out("gam", (n_pts,)), ar.out("dlam", (n_pts, 4), want=want_grad),
                     ar.out("geo_bar", (8, n_pts, N), want=want_geo_bar), N, ar.out("info", (n_pts,), _I32, want_info))
        return ar.result(rc)

    def local_eq_boundary_grad(self, theta_lo, h, geo, dPdrho, centre, sigma, rays, ps=None, shift=0.0, max_cross=4, xtol=1e-12,
                               want_geo_bar=False, want_nodes=False):
        """local_eq_boundary with the derivatives of every returned crossing t*: ONE local_eq_boundary call, the crossings gathered on
        the host at t = the midpoint of the closed bracket, ONE local_eq_grad call at those points, and the implicit-function rule
        on lam_max(t*) = shift with lam_t = d_eps lam_eps + d_p lam_p:
            d t* / d (theta0, eps0, p0, shift, dPdrho) = (-lam_theta0, -lam_eps, -lam_p, 1, -lam_dP) / lam_t.
        Returns local_eq_boundary's dict (info included) plus lam_at, dlam_dt (n_lines, n_ray, max_cross) and dt (n_lines, n_ray,
        max_cross, 5), NaN beyond n_cross, in the memory kind of geo; grad_nbad = local_eq_grad's flagged points; with
        want_geo_bar also pts int (n_cross_total, 3) = the (line, ray, crossing) of every gathered point and dt_geo (8, n_cross_total,
        N) = d t* / d (the eight arrays of that line) = -geo_bar / lam_t.  dlam_dt is returned so that the caller can judge a
        near-tangency: lam_t = 0 gives inf or NaN by arithmetic."""
        b = self.local_eq_boundary(theta_lo, h, geo, dPdrho, centre, sigma, rays, ps=ps, shift=shift, max_cross=max_cross, xtol=xtol,
                                   want_nodes=want_nodes, want_info=True)
        on_dev = _is_torch(geo)
        host = (lambda a: a.detach().cpu().numpy()) if on_dev else np.asarray
        nc, t = host(b["n_cross"]), host(b["t"])
        rays_h = np.asarray(host(rays) if _is_torch(rays) else rays, dtype=np.float64)
        shape = t.shape
        il, ir, ic = np.nonzero(np.arange(shape[2])[None, None, :] < nc[:, :, None])
        tt = t[il, ir, ic]
        var = np.stack([rays_h[ir, 0], rays_h[ir, 1] + tt * rays_h[ir, 3], rays_h[ir, 2] + tt * rays_h[ir, 4]], axis=1).reshape(-1, 3)
        lam_at, dlam_dt, dt = np.full(shape, np.nan), np.full(shape, np.nan), np.full(shape + (5,), np.nan)
        b["grad_nbad"] = 0
        pts = np.stack([il, ir, ic], axis=1)
        dt_geo = None
        if len(tt):
            g = self.local_eq_grad(theta_lo, h, geo, dPdrho, centre, sigma, il.astype(np.int32), var, ps=ps, want_geo_bar=want_geo_bar)
            b["grad_nbad"] = g["nbad"]
            dl = host(g["dlam"])
            lt = rays_h[ir, 3] * dl[:, 1] + rays_h[ir, 4] * dl[:, 2]
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = 1.0 / lt
                lam_at[il, ir, ic], dlam_dt[il, ir, ic] = host(g["lam"]), lt
                dt[il, ir, ic] = np.stack([-dl[:, 0] * inv, -dl[:, 1] * inv, -dl[:, 2] * inv, inv, -dl[:, 3] * inv], axis=1)
            if want_geo_bar:
                if on_dev:
                    import torch
                    dt_geo = g["geo_bar"] * torch.from_numpy(-inv).to(g["geo_bar"].device)[None, :, None]
                else:
                    dt_geo = g["geo_bar"] * (-inv)[None, :, None]
        if on_dev:
            import torch
            lam_at, dlam_dt, dt = (torch.from_numpy(a).to(geo.device) for a in (lam_at, dlam_dt, dt))
        b.update(lam_at=lam_at, dlam_dt=dlam_dt, dt=dt)
        if want_geo_bar:
            if dt_geo is None:
                N = int(geo.shape[2])
                dt_geo = geo.new_zeros((8, 0, N)) if on_dev else np.zeros((8, 0, N))
            b.update(pts=pts, dt_geo=dt_geo)
        return b

    @staticmethod
    def _three_lines(geo):
        n_pts, three, eight, N = geo.shape
        if three != 3 or eight != 8:
            raise IbsError("geo must be (n_pts, 3, 8, N)")
        return n_pts, N

    def marginal_obj_w_grad(self, h, geo, theta0, del_alpha=0.004, want_grad=True, want_info=False):
        """the objective of the margin's refinement in (alpha, theta0) (ibs_marginal_obj_w_grad_f64): geo (n_pts, 3, 8, N) -- the
        lines alpha - del_alpha / 2, alpha, alpha + del_alpha / 2 --, theta0 (n_pts,).  Returns dict(val = -1 / s*, scale = s*,
        dPdrho (the centre line's)[, jac = dscale / s*^2, dscale = (d s* / d alpha, d s* / d theta0): (n_pts, 2)][, info], nbad).
        want_grad=False: the side lines are not read and no mode is formed.  info status bit 8: scale = inf, val = 0, jac = dscale = 0
        (not counted in nbad); bits 0-1: NaN outputs -- or, where only a side line held invalid data, NaN jac and dscale alone."""
        n_pts, N = self._three_lines(geo)
        ar = _Args(self)
        rc = ar.call("ibs_marginal_obj_w_grad_f64", n_pts, N, float(h), ar.inp(geo), N, ar.inp(theta0), float(del_alpha),
                     ar.out("val", (n_pts,)), ar.out("jac", (n_pts, 2), want=want_grad), ar.out("scale", (n_pts,)),
                     ar.out("dscale", (n_pts, 2), want=want_grad), ar.out("dPdrho", (n_pts,)), ar.out("info", (n_pts,), _I32, want_info))
        return ar.result(rc)

    def marginal_obj_w_grad_tangent(self, h, geo, geo_da, theta0, want_grad=True, want_geo_bar=False, want_info=False):
        """marginal_obj_w_grad with the derivative in alpha exact as well, from ONE line per point (ibs_marginal_obj_w_grad_tangent_f64):
        geo, geo_da (8, n_pts, N) as fieldline_geometry and fieldline_geometry_dalpha return them for the same lines, theta0 (n_pts,);
        no del_alpha.  geo_da may be None with want_grad=False.  Returns dict(val = -1 / s*, scale = s*, dPdrho[, jac = dscale / s*^2,
        dscale = (d s* / d alpha, d s* / d theta0): (n_pts, 2)][, geo_bar (8, n_pts, N) = d scale / d geo, the dependence through the
        line's own dPdrho included: the cotangent to hand to fieldline_geometry_vjp][, info], nbad).  want_grad=False and
        want_geo_bar=False: no mode is formed.  Status bits as marginal_obj_w_grad; geo_bar is zero with bit 8 and NaN with a failed
        solve, and kept where only geo_da held invalid data (bit 1, NaN jac and dscale)."""
        eight, n_pts, N = geo.shape
        if eight != 8 or (geo_da is not None and tuple(geo_da.shape) != (8, n_pts, N)):
            raise IbsError("geo and geo_da must both be (8, n_pts, N)")
        if geo_da is None and want_grad:
            raise IbsError("geo_da is required with want_grad")
        ar = _Args(self)
        rc = ar.call("ibs_marginal_obj_w_grad_tangent_f64", n_pts, N, float(h), ar.inp(geo), ar.inp(geo_da), N, ar.inp(theta0),
                     ar.out("val", (n_pts,)), ar.out("jac", (n_pts, 2), want=want_grad), ar.out("scale", (n_pts,)),
                     ar.out("dscale", (n_pts, 2), want=want_grad), ar.out("dPdrho", (n_pts,)),
                     ar.out("geo_bar", (8, n_pts, N), want=want_geo_bar), ar.out("info", (n_pts,), _I32, want_info))
        return ar.result(rc)

    def gamma_scan_nearest(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, sigma, want_info=False):
        """the coarse scan of ball_scan.py:248-273 with the eigenpair nearest sigma, as upstream (sigma = 1.0 there: ball_scan.py:230);
        ibs_gamma_scan_nearest_f64.  Geometry arrays (n_lines, N); dPdrho (n_lines,); theta0 (n_theta0,); sigma a scalar or
        (n_lines, n_theta0).  Returns dict(gam, lam, idx[, info], nbad) shaped (n_lines, n_theta0)."""
        ar = _Args(self)
        head, shape, N = ar.geo(h, (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22), dPdrho, theta0)
        rc = ar.call("ibs_gamma_scan_nearest_f64", *head, ar.rows(sigma, shape), ar.out("gam", shape), ar.out("lam", shape),
                     ar.out("idx", shape, _I32), ar.out("info", shape, _I32, want_info))
        return ar.result(rc)

    def gamma_scan_modes(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, n_modes, want_info=False):
        """the n_modes largest eigenvalues and growth rates of every (line, theta0) of a coarse scan (ibs_gamma_scan_modes_f64), arrays
        as in gamma_scan, 1 <= n_modes <= 16.  Returns dict(gam, lam[, info], nbad) shaped (n_lines, n_theta0, n_modes), mode 0 =
        lam_max; status bit 9 (CLUSTER_BIT) as in solve_gcf_modes.  No eigenfunctions."""
        K = self._n_modes(n_modes)
        geo7 = (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22)
        if len(bmag.shape) != 2:
            raise IbsError("gamma_scan_modes: the seven geometry arrays must be (n_lines, N), not %s" % (tuple(bmag.shape),))
        n_lines, N = bmag.shape
        for a in geo7[1:]:
            if tuple(a.shape) != (n_lines, N):
                raise IbsError("gamma_scan_modes: the seven geometry arrays must all be (%d, %d), not %s" % (n_lines, N, tuple(a.shape)))
        if tuple(dPdrho.shape) != (n_lines,) or len(theta0.shape) != 1:
            raise IbsError("gamma_scan_modes: dPdrho must be (%d,) and theta0 (n_theta0,)" % n_lines)
        ar = _Args(self)
        head, shape, N = ar.geo(h, geo7, dPdrho, theta0)
        rc = ar.call("ibs_gamma_scan_modes_f64", *head, K, ar.out("gam", shape + (K,)), ar.out("lam", shape + (K,)),
                     ar.out("info", shape + (K,), _I32, want_info))
        return ar.result(rc)

    def gamma_scan_vjp(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, gam_bar, sigma=None,
                       want=("geo", "dPdrho", "theta0"), want_info=False):
        """exact vector-Jacobian product of the whole growth-rate table of a coarse scan (ibs_gamma_scan_vjp_f64): arrays as in
        gamma_scan, gam_bar (n_lines, n_theta0) the cotangent of gam; sigma None: lam_max's eigenpair, else a scalar or
        (n_lines, n_theta0): the eigenpair nearest it.  want: which of "geo", "dPdrho", "theta0" to return, at least one.
        Returns dict(geo_bar (7, n_lines, N) in the order of the arguments, dPdrho_bar (n_lines,), theta0_bar (n_lines, n_theta0):
        per system -- a caller whose lines share theta0 sums over the lines --, gam, lam[, info], nbad); entries not wanted are
        None.  gam and lam are the division-form solve's own.  A system with gam_bar == 0 contributes exactly 0; a non-zero
        cotangent on a failed solve (status bits 0-1), a refused adjoint (status bit 7) or a non-finite gam_bar (sets bit 1) makes
        the rows and dPdrho_bar of its line and its own theta0_bar NaN.  EXACT_VJP_SHIFT moves info's status to solve_gcf_vjp's
        two bits."""
        geo7 = (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22)
        if len(bmag.shape) != 2:
            raise IbsError("gamma_scan_vjp: the seven geometry arrays must be (n_lines, N), not %s" % (tuple(bmag.shape),))
        n_lines, N = bmag.shape
        for a in geo7[1:]:
            if tuple(a.shape) != (n_lines, N):
                raise IbsError("gamma_scan_vjp: the seven geometry arrays must all be (%d, %d), not %s" % (n_lines, N, tuple(a.shape)))
        if tuple(dPdrho.shape) != (n_lines,) or len(theta0.shape) != 1:
            raise IbsError("gamma_scan_vjp: dPdrho must be (%d,) and theta0 (n_theta0,)" % n_lines)
        if tuple(gam_bar.shape) != (n_lines, int(theta0.shape[0])):
            raise IbsError("gamma_scan_vjp: gam_bar must be (%d, %d), not %s" % (n_lines, theta0.shape[0], tuple(gam_bar.shape)))
        want = tuple(want)
        if not want or any(w not in ("geo", "dPdrho", "theta0") for w in want):
            raise IbsError("gamma_scan_vjp: want must name at least one of 'geo', 'dPdrho', 'theta0', not %r" % (want,))
        ar = _Args(self)
        head, shape, N = ar.geo(h, geo7, dPdrho, theta0)
        rc = ar.call("ibs_gamma_scan_vjp_f64", *head, ar.rows(sigma, shape), ar.inp(gam_bar),
                     ar.out("geo_bar", (7, n_lines, N), want="geo" in want), ar.out("dPdrho_bar", (n_lines,), want="dPdrho" in want),
                     ar.out("theta0_bar", shape, want="theta0" in want), ar.out("gam", shape), ar.out("lam", shape),
                     ar.out("info", shape, _I32, want_info))
        for k in ("geo_bar", "dPdrho_bar", "theta0_bar"):
            ar.outs.setdefault(k, None)
        return ar.result(rc)

    # ---- geometry x theta0 scan ---------------------------------------------------------------
    def gamma_scan(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0,
                   want_X=False, want_dtheta0=False, want_info=False, lam_guess=None, guess_width=None, certify=False):
        """geometry arrays: (n_lines, N); dPdrho: (n_lines,); theta0: (n_theta0,).
        Returns dict(gam, lam[, X, dX][, dgam_dtheta0]) shaped (n_lines, n_theta0[, N]).
        certify=True: every lam is then certified by a division-form Sturm count pair at lam +- 4 N eps ||A|| (certify_scan), a system
        that fails is solved again in division form (reclose_scan: lam, gam, X, dX replaced; dgam_dtheta0 is not), and out["cert"]
        (int32: 0 = certified, 8 = re-closed and certified, bits 0-2 = open, see certify_scan) and out["ncert_failed"] (host arrays
        only) are added.  certify=False makes today's calls only."""
        geo = (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22)
        if certify:
            out = self.gamma_scan(h, *geo, dPdrho, theta0, want_X=want_X, want_dtheta0=want_dtheta0, want_info=want_info,
                                  lam_guess=lam_guess, guess_width=guess_width)
            out["cert"] = self.certify_scan(h, *geo, dPdrho, theta0, out["lam"])
            out["ncert_failed"] = self.reclose_scan(h, *geo, dPdrho, theta0, out["cert"], out["lam"], out["gam"], out.get("X"),
                                                    out.get("dX"))
            return out
        ar = _Args(self)
        head, shape, N = ar.geo(h, geo, dPdrho, theta0)
        warm = () if lam_guess is None else (ar.inp(lam_guess), float(guess_width))
        rc = ar.call("ibs_gamma_scan_f64" if lam_guess is None else "ibs_gamma_scan_warm_f64", *head, *warm, ar.out("gam", shape),
                     ar.out("lam", shape), ar.out("X", shape + (N,), want=want_X), ar.out("dX", shape + (N,), want=want_X),
                     ar.out("dgam_dtheta0", shape, want=want_dtheta0), ar.out("info", shape, _I32, want_info))
        return ar.result(rc)

    def gamma_scan_argmax(self, h, geo7, dPdrho, theta0, n_surf):
        """coarse scan + per-surface first maximum in ONE C call on device tensors (ibs_gamma_scan_argmax_f64; replaces
        ball_scan.py:248-295 for all surfaces at once).  geo7: seven (n_lines, N) tensors, lines surface-major.
        Returns dict(gam, lam (n_lines, n_theta0), pack (n_surf, 2) = (max, first row-major index), info)."""
        ar = _Args(self)
        head, shape, N = ar.geo(h, geo7, dPdrho, theta0)
        if ar.mem != MEM_DEVICE:
            raise IbsError("gamma_scan_argmax takes device tensors")
        ar.call("ibs_gamma_scan_argmax_f64", *head, int(n_surf), ar.out("gam", shape), ar.out("lam", shape), ar.out("pack", (n_surf, 2)),
                ar.out("info", shape, _I32), mem=False)
        return ar.result()

    def gamma_points(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0,
                     want_X=False, want_dtheta0=False, want_info=False, certify=False):
        """one (line, theta0) pair per point (ibs_gamma_points_f64: the final solve of ball_scan.py:322-339 for many
        surfaces at once).  geometry arrays (n_pts, N); dPdrho, theta0 (n_pts,).  Returns dict(gam, lam[, X, dX][, ...]).
        certify=True: as in gamma_scan (certify_points, reclose_points; out["cert"], out["ncert_failed"])."""
        geo = (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22)
        if certify:
            out = self.gamma_points(h, *geo, dPdrho, theta0, want_X=want_X, want_dtheta0=want_dtheta0, want_info=want_info)
            out["cert"] = self.certify_points(h, *geo, dPdrho, theta0, out["lam"])
            out["ncert_failed"] = self.reclose_points(h, *geo, dPdrho, theta0, out["cert"], out["lam"], out["gam"], out.get("X"),
                                                      out.get("dX"))
            return out
        ar = _Args(self)
        head, shape, N = ar.geo(h, geo, dPdrho, theta0, points=True)
        rc = ar.call("ibs_gamma_points_f64", *head, ar.out("gam", shape), ar.out("lam", shape), ar.out("X", shape + (N,), want=want_X),
                     ar.out("dX", shape + (N,), want=want_X), ar.out("dgam_dtheta0", shape, want=want_dtheta0),
                     ar.out("info", shape, _I32, want_info))
        return ar.result(rc)

    # ---- lines on a non-uniform theta grid (include/ibs.h: ibs_regrid_rows_f64 and the *_theta_f64 entry points) -------------
    @staticmethod
    def _theta_window(theta, window):
        """(theta_lo, theta_hi) as host floats: `window`, or the two end values of theta (of its first row: all lines share the window).
        The library takes them as host scalars, so for a device tensor this is one small copy to the host."""
        if window is not None:
            lo, hi = window
            return float(lo), float(hi)
        first = theta if len(theta.shape) == 1 else theta[0]
        return float(first[0]), float(first[-1])

    @staticmethod
    def _theta_rows(what, theta, n_rows, N):
        """theta_ld of a grid argument: (N,) = one shared grid (0), (n_rows, N) = one row each (N)"""
        shape = tuple(theta.shape)
        if shape == (N,):
            return 0
        if shape == (n_rows, N):
            return N
        raise IbsError("%s: theta must be (%d,) or (%d, %d), not %s" % (what, N, n_rows, N, shape))

    def _theta_call(self, first):
        """the call object of a theta entry point: its memory kind is that of the data arrays; a host theta goes up with them"""
        return _Args(self, device=first.device, host=False) if _is_torch(first) else _Args(self, host=True)

    def regrid_rows(self, theta, g, c=None, f=None, window=None, want_info=False):
        """raw rows on a non-uniform grid -> the uniform grid of the same window, as utils.py:1565-1576 (ibs_regrid_rows_f64): g (and c,
        f, each optional) (n_sys, N) on theta, (N,) shared or (n_sys, N).  Returns dict(h, g, gh, c, f[, info], nbad): h the spacing
        and (g, gh, c, f) the rows to hand to solve_gcf(h, g, c, f, gh=gh) / solve_gcf_nearest / solve_gcf_modes; c / f None where not
        given.  window=None reads the two end values of theta (a small copy to the host for a device tensor); a row that is not an
        increasing grid on the window gives NaN rows and status bit 1 (counted in nbad)."""
        n_sys, N = g.shape
        ld_t = self._theta_rows("regrid_rows", theta, n_sys, N)
        lo, hi = self._theta_window(theta, window)
        ar = self._theta_call(g)
        h = C.c_double(0.0)
        rc = ar.call("ibs_regrid_rows_f64", n_sys, N, ar.inp(theta, upload=True), ld_t, lo, hi, ar.inp(g), ar.inp(c), ar.inp(f), N,
                     ar.out("g", (n_sys, N)), ar.out("gh", (n_sys, N)), ar.out("c", (n_sys, N), want=c is not None),
                     ar.out("f", (n_sys, N), want=f is not None), N, C.byref(h), ar.out("info", (n_sys,), _I32, want_info))
        out = ar.result(rc)
        out.setdefault("c", None)
        out.setdefault("f", None)
        out["h"] = h.value
        return out

    def assemble_gcf_theta(self, theta, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, points=False,
                           window=None, want_info=False):
        """the regridded rows of every (line, theta0) system of geometry on a non-uniform grid (ibs_assemble_gcf_theta_f64): g, c, f are
        formed at the samples and interpolated, as upstream.  Arrays (n_lines, N), dPdrho (n_lines,), theta (N,) or (n_lines, N);
        theta0 (n_theta0,), or with points=True (n_lines,): one per line.  Returns dict(h, g, gh, c, f[, info], nbad), the rows shaped
        (n_lines, n_theta0, N) -- (n_lines, N) with points=True.  window as in regrid_rows."""
        geo7 = (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22)
        n_lines, N = bmag.shape
        ld_t = self._theta_rows("assemble_gcf_theta", theta, n_lines, N)
        lo, hi = self._theta_window(theta, window)
        shape = (n_lines,) if points else (n_lines, int(theta0.shape[0]))
        ar = self._theta_call(bmag)
        h = C.c_double(0.0)
        rc = ar.call("ibs_assemble_gcf_theta_f64", n_lines, 1 if points else shape[1], N, ar.inp(theta, upload=True), ld_t, lo, hi,
                     *[ar.inp(a) for a in geo7], N, ar.inp(dPdrho), ar.inp(theta0), 1 if points else 0,
                     ar.out("g", shape + (N,)), ar.out("gh", shape + (N,)), ar.out("c", shape + (N,)), ar.out("f", shape + (N,)),
                     C.byref(h), ar.out("info", shape, _I32, want_info))
        out = ar.result(rc)
        out["h"] = h.value
        return out

    def _theta_composed(self, what, points, theta, geo7, dPdrho, theta0, want_X, want_info, window, eigenpair, sigma, n_modes):
        """eigenpair="nearest" / n_modes=K of the theta scans: assemble_gcf_theta, then the raw solver with gh, reshaped"""
        if eigenpair not in ("max", "nearest"):
            raise IbsError("%s: eigenpair must be 'max' or 'nearest', not %r" % (what, eigenpair))
        if n_modes is not None and eigenpair == "nearest":
            raise IbsError("%s: n_modes and eigenpair='nearest' exclude each other" % what)
        if eigenpair == "nearest" and sigma is None:
            raise IbsError("%s: eigenpair='nearest' needs sigma" % what)
        rows = self.assemble_gcf_theta(theta, *geo7, dPdrho, theta0, points=points, window=window, want_info=True)
        shape, N = tuple(rows["g"].shape[:-1]), rows["g"].shape[-1]
        n_sys = int(np.prod(shape))
        g, gh, c, f = (rows[k].reshape(n_sys, N) for k in ("g", "gh", "c", "f"))
        if n_modes is not None:
            K = self._n_modes(n_modes)
            r = self.solve_gcf_modes(rows["h"], g, c, f, K, gh=gh, want_X=want_X, want_info=want_info)
            tail = (K,)
        else:
            r = self.solve_gcf_nearest(rows["h"], g, c, f, sigma, gh=gh, want_X=want_X, want_info=want_info)
            tail = ()
        out = {k: (v.reshape(shape + tail + ((N,) if k in ("X", "dX") else ())) if k != "nbad" else v) for k, v in r.items()}
        out["h"] = rows["h"]
        return out

    def gamma_scan_theta(self, theta, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, want_X=False,
                         want_info=False, window=None, eigenpair="max", sigma=None, n_modes=None):
        """gamma_scan for geometry on a NON-UNIFORM theta grid (ibs_gamma_scan_theta_f64): every line is regridded as upstream does
        (utils.py:1565-1576) and solved with the half-grid row, on the device.  theta (N,) shared or (n_lines, N); arrays (n_lines, N);
        dPdrho (n_lines,); theta0 (n_theta0,).  Returns dict(gam, lam[, X, dX][, info], nbad) shaped (n_lines, n_theta0[, N]).
        window=None reads the two end values of theta -- for a device tensor a small copy to the host; pass window=(lo, hi) to avoid
        it.  A line whose row is not an increasing grid on the window gives NaN and status bit 1.
        eigenpair="nearest" (with sigma, a scalar or (n_lines, n_theta0)) and n_modes=K are compositions: assemble_gcf_theta, then
        solve_gcf_nearest / solve_gcf_modes with gh; their dicts, reshaped to (n_lines, n_theta0[, K][, N])."""
        geo7 = (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22)
        if eigenpair != "max" or n_modes is not None:
            return self._theta_composed("gamma_scan_theta", False, theta, geo7, dPdrho, theta0, want_X, want_info, window, eigenpair,
                                        sigma, n_modes)
        return self._theta_scan("ibs_gamma_scan_theta_f64", False, theta, geo7, dPdrho, theta0, want_X, want_info, window)

    def gamma_points_theta(self, theta, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, want_X=False,
                           want_info=False, window=None, eigenpair="max", sigma=None, n_modes=None):
        """gamma_points on a non-uniform grid (ibs_gamma_points_theta_f64: the final solve of ball_scan.py:322-339 for many lines at
        once): line i at its own theta0[i]; theta (N,) or (n_pts, N).  Returns dict(gam, lam[, X, dX][, info], nbad) shaped (n_pts[, N]):
        the bits gamma_scan_theta gives at the same (line, theta0).  window, eigenpair, sigma and n_modes as in gamma_scan_theta."""
        geo7 = (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22)
        if eigenpair != "max" or n_modes is not None:
            return self._theta_composed("gamma_points_theta", True, theta, geo7, dPdrho, theta0, want_X, want_info, window, eigenpair,
                                        sigma, n_modes)
        return self._theta_scan("ibs_gamma_points_theta_f64", True, theta, geo7, dPdrho, theta0, want_X, want_info, window)

    def _theta_scan(self, name, points, theta, geo7, dPdrho, theta0, want_X, want_info, window):
        n_lines, N = geo7[0].shape
        ld_t = self._theta_rows(name, theta, n_lines, N)
        lo, hi = self._theta_window(theta, window)
        shape = (n_lines,) if points else (n_lines, int(theta0.shape[0]))
        ar = self._theta_call(geo7[0])
        rc = ar.call(name, *shape, N, ar.inp(theta, upload=True), ld_t, lo, hi, *[ar.inp(a) for a in geo7], N, ar.inp(dPdrho),
                     ar.inp(theta0), ar.out("gam", shape), ar.out("lam", shape), ar.out("X", shape + (N,), want=want_X),
                     ar.out("dX", shape + (N,), want=want_X), ar.out("info", shape, _I32, want_info))
        return ar.result(rc)

    def scan_starts(self, alpha_scan, theta0_scan, pack, n_bad, want_sigma0=False):
        """start points (n_surf, 2) = (alpha, theta0) of the refinement from the per-surface maxima `pack`, on the device
        (ibs_scan_starts_f64; ball_scan.py:279-295).  All arguments device tensors; n_bad: int32 tensor of one element that
        accumulates the number of surfaces whose maximum is not finite.  want_sigma0: returns (start, sigma0 (n_surf,)) with
        the refinement's shift of every surface, 1.3 |max| + 0.05 (0.05 for an all-zero table: ball_scan.py:282, 289)."""
        ar = _Args(self, device=pack.device)
        n_surf = pack.shape[0]
        ar.call("ibs_scan_starts_f64", n_surf, alpha_scan.shape[0], theta0_scan.shape[0], ar.inp(alpha_scan), ar.inp(theta0_scan),
                ar.inp(pack), ar.out("start", (n_surf, 2)), ar.out("sigma0", (n_surf,), want=want_sigma0),
                ar.inout("scan_starts", "n_bad", n_bad, _I32), mem=False)
        return (ar.outs["start"], ar.outs["sigma0"]) if want_sigma0 else ar.outs["start"]

    @staticmethod
    def _n_starts(n_starts):
        ok = isinstance(n_starts, (int, float, np.integer, np.floating)) and not isinstance(n_starts, bool)
        if not ok or int(n_starts) != n_starts or not 1 <= n_starts <= MAX_STARTS:
            raise IbsError("n_starts must be an integer in [1, %d], not %r" % (MAX_STARTS, n_starts))
        return int(n_starts)

    def scan_peaks(self, alpha_scan, theta0_scan, gam, n_starts, n_bad=None, want_sigma0=False, want_index=False, want_found=False):
        """the n_starts best peaks of every surface's coarse table and the starts of a multi-start refinement from them
        (ibs_scan_peaks_f64; the rule: scan.pick_starts), 1 <= n_starts <= 16.  gam: (n_surf, n_alpha, n_theta0) -- numpy arrays or
        device tensors, like the grids.  Returns dict(start (n_surf, n_starts, 2) = (alpha, theta0), peak (n_surf, n_starts)[, sigma0
        (n_surf, n_starts) = 1.3 |peak| + 0.05][, index int32 (n_surf, n_starts): row-major, -1 where the start is (0, 0)][, n_found
        int32 (n_surf,)], n_bad): slot 0 is the first maximum with the start of scan_starts, slots beyond n_found repeat it.
        n_bad: int32 array of one element in the call's memory kind, which accumulates the number of surfaces whose maximum is not
        finite (None: a zeroed one is made); it is returned under "n_bad"."""
        K = self._n_starts(n_starts)
        na, nt = int(alpha_scan.shape[0]), int(theta0_scan.shape[0])
        if len(gam.shape) != 3 or tuple(gam.shape[1:]) != (na, nt):
            raise IbsError("scan_peaks: gam must be (n_surf, %d, %d), not %s" % (na, nt, tuple(gam.shape)))
        n_surf = int(gam.shape[0])
        ar = _Args(self)
        head = [ar.inp(alpha_scan), ar.inp(theta0_scan), ar.inp(gam)]
        if n_bad is None:
            if ar.mem == MEM_DEVICE:
                import torch
                n_bad = torch.zeros(1, dtype=torch.int32, device=ar.ref)
            else:
                n_bad = np.zeros(1, dtype=np.int32)
        ar.call("ibs_scan_peaks_f64", n_surf, na, nt, K, *head, ar.out("start", (n_surf, K, 2)), ar.out("peak", (n_surf, K)),
                ar.out("index", (n_surf, K), _I32, want_index), ar.out("sigma0", (n_surf, K), want=want_sigma0),
                ar.out("n_found", (n_surf,), _I32, want_found), ar.inout("scan_peaks", "n_bad", n_bad, _I32))
        ar.outs["n_bad"] = n_bad
        return ar.outs

    def theta0_polish(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, gam, n_starts=1, xtol=1e-5,
                      max_eval=32, lam=None, node=None, want_lam=False, want_info=False, want_found=True):
        """gam of every line maximised over theta0 between the nodes of its coarse row (ibs_theta0_polish_f64; the rule:
        scan.row_peaks and scan.polish_theta0): about the n_starts <= 4 best peaks of gam[line], or about the nodes the caller names.
        geometry arrays (n_lines, N), odd N <= 2050; dPdrho (n_lines,); theta0 (n_theta0,): finite and strictly increasing; gam
        (n_lines, n_theta0): the coarse table of gamma_scan on these lines; lam, same shape, optional: warm starts; node int32
        (n_lines, n_starts), optional: the nodes to polish about (-1 = skip the slot) instead of the row's own peaks.
        Returns dict(theta0, gam (n_lines, n_starts), node, n_eval int32 (n_lines, n_starts)[, lam][, info int32: sweeps | status << 16]
        [, n_found int32 (n_lines,)], nbad): gam is never below the coarse row; status bit 10 = the node itself was returned, bit 11 =
        max_eval reached, bit 12 = one-sided bracket.  Slots from n_found on repeat slot 0; a row without a finite entry gives NaN."""
        K = int(n_starts)
        if K != n_starts or not 1 <= K <= MAX_ROW_STARTS:
            raise IbsError("n_starts must be an integer in [1, %d], not %r" % (MAX_ROW_STARTS, n_starts))
        geo = (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22)
        shape = (int(geo[0].shape[0]), int(theta0.shape[0]))
        for name, t in (("gam", gam), ("lam", lam)):
            if t is not None and tuple(t.shape) != shape:
                raise IbsError("theta0_polish: %s must be %s, not %s" % (name, shape, tuple(t.shape)))
        slots = (shape[0], K)
        if node is not None and tuple(node.shape) != slots:
            raise IbsError("theta0_polish: node must be %s, not %s" % (slots, tuple(node.shape)))
        ar = _Args(self)
        head, _, N = ar.geo(h, geo, dPdrho, theta0)
        rc = ar.call("ibs_theta0_polish_f64", *head, ar.inp(gam), ar.inp(lam), ar.inp(node, _I32), K, float(xtol), int(max_eval),
                     ar.out("theta0", slots), ar.out("gam", slots), ar.out("lam", slots, want=want_lam), ar.out("node", slots, _I32),
                     ar.out("n_eval", slots, _I32), ar.out("info", slots, _I32, want_info), ar.out("n_found", (shape[0],), _I32, want_found))
        return ar.result(rc)

    def obj_w_grad(self, h, geo, theta0, del_alpha=0.004, want_info=False):
        """geo: (n_pts, 3, 8, N) -- lines (alpha-d/2, alpha, alpha+d/2) x (bmag, gradpar, cvdrift, cvdrift0,
        gds2, gds21, gds22, gbdrift); theta0: (n_pts,).  Returns (val (n_pts,), jac (n_pts, 2)) with the
        sign convention of utils.py:1728: val = -gam, jac = (-dgam/dalpha, -dgam/dtheta0)."""
        n_pts, N = self._three_lines(geo)
        ar = _Args(self)
        ar.call("ibs_obj_w_grad_f64", n_pts, N, float(h), ar.inp(geo), N, ar.inp(theta0), float(del_alpha), ar.out("val", (n_pts,)),
                ar.out("jac", (n_pts, 2)), ar.out("info", (n_pts,), _I32, want_info))
        return tuple(ar.outs.values())

    @staticmethod
    def _val_jac(ar, want_info):
        """(val, jac) or, with want_info, (val, jac, dict of the other outputs)"""
        out = ar.outs
        val, jac = out.pop("val"), out.pop("jac")
        return (val, jac, out) if want_info else (val, jac)

    def obj_w_grad_nearest(self, h, geo, theta0, sigma, del_alpha=0.004, want_info=False):
        """obj_w_grad with the eigenpair NEAREST sigma (ibs_obj_w_grad_nearest_f64: utils.py:1632-1728 as the refinement of
        ball_scan.py:305-314 runs it, sigma = 1.3 |gam| + 0.05).  geo (n_pts, 3, 8, N), theta0 (n_pts,), sigma a scalar or (n_pts,).
        Returns (val, jac) or, with want_info, (val, jac, dict(lam, idx, info)); a failed solve gives NaN val and jac."""
        n_pts, N = self._three_lines(geo)
        ar = _Args(self)
        ar.call("ibs_obj_w_grad_nearest_f64", n_pts, N, float(h), ar.inp(geo), N, ar.inp(theta0), ar.rows(sigma, (n_pts,)),
                float(del_alpha), ar.out("val", (n_pts,)), ar.out("jac", (n_pts, 2)), ar.out("lam", (n_pts,), want=want_info),
                ar.out("idx", (n_pts,), _I32, want_info), ar.out("info", (n_pts,), _I32, want_info))
        return self._val_jac(ar, want_info)

    def obj_w_grad_exact(self, h, geo, theta0, del_alpha=0.004, sigma=None, want_info=False):
        """obj_w_grad with the EXACT gradient of the gam it returns (ibs_obj_w_grad_exact_f64: utils.py:1632-1728 with the exact
        derivative in place of the Hellmann-Feynman formulas of utils.py:1676-1680 / 1721-1725), batched on the device.
        geo (n_pts, 3, 8, N), theta0 (n_pts,); sigma None: lam_max's eigenpair, else a scalar or (n_pts,): the eigenpair nearest it.
        Returns (val, jac) or, with want_info, (val, jac, dict(gam, lam, idx, info)).  A failed solve (status bits 0-1) gives NaN
        val and jac; an adjoint that refuses the pair (status bit 7) NaN jac alone; bit 6 (a replaced pivot of the adjoint solve) is
        informational.  EXACT_VJP_SHIFT moves info's status to solve_gcf_vjp's two bits."""
        n_pts, N = self._three_lines(geo)
        ar = _Args(self)
        ar.call("ibs_obj_w_grad_exact_f64", n_pts, N, float(h), ar.inp(geo), N, ar.inp(theta0), ar.rows(sigma, (n_pts,)),
                float(del_alpha), ar.out("val", (n_pts,)), ar.out("jac", (n_pts, 2)), ar.out("gam", (n_pts,), want=want_info),
                ar.out("lam", (n_pts,), want=want_info), ar.out("idx", (n_pts,), _I32, want_info), ar.out("info", (n_pts,), _I32, want_info))
        return self._val_jac(ar, want_info)

    def obj_w_grad_exact_tangent(self, h, geo, geo_da, theta0, sigma=None, want_info=False):
        """obj_w_grad_exact with the derivative in alpha exact as well, from ONE line per point (ibs_obj_w_grad_exact_tangent_f64):
        geo, geo_da (8, n_pts, N) as fieldline_geometry and fieldline_geometry_dalpha return them for the same lines, theta0 (n_pts,);
        no del_alpha.  sigma, the return values and the status bits are obj_w_grad_exact's; val, jac[:, 1] and the info dict are the
        bits obj_w_grad_exact gives on the same centre line."""
        eight, n_pts, N = geo.shape
        if eight != 8 or tuple(geo_da.shape) != (8, n_pts, N):
            raise IbsError("geo and geo_da must both be (8, n_pts, N)")
        ar = _Args(self)
        ar.call("ibs_obj_w_grad_exact_tangent_f64", n_pts, N, float(h), ar.inp(geo), ar.inp(geo_da), N, ar.inp(theta0),
                ar.rows(sigma, (n_pts,)), ar.out("val", (n_pts,)), ar.out("jac", (n_pts, 2)), ar.out("gam", (n_pts,), want=want_info),
                ar.out("lam", (n_pts,), want=want_info), ar.out("idx", (n_pts,), _I32, want_info), ar.out("info", (n_pts,), _I32, want_info))
        return self._val_jac(ar, want_info)

    def gamma_points_nearest(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, sigma,
                             want_X=False, want_info=False):
        """gamma_points with the eigenpair NEAREST sigma (ibs_gamma_points_nearest_f64: the final solve of ball_scan.py:322-339,
        sigma = 0.42 there).  Geometry arrays (n_pts, N); dPdrho, theta0 (n_pts,); sigma a scalar or (n_pts,).
        Returns dict(gam, lam, idx[, X, dX][, info], nbad)."""
        ar = _Args(self)
        head, shape, N = ar.geo(h, (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22), dPdrho, theta0, points=True)
        rc = ar.call("ibs_gamma_points_nearest_f64", *head, ar.rows(sigma, shape), ar.out("gam", shape), ar.out("lam", shape),
                     ar.out("idx", shape, _I32), ar.out("X", shape + (N,), want=want_X), ar.out("dX", shape + (N,), want=want_X),
                     ar.out("info", shape, _I32, want_info))
        return ar.result(rc)

    # ---- table-fed: field-line geometry, its derivatives, the refinement --------------------------
    def fieldline_geometry(self, tables, line_surf, line_alpha, theta, device=None, use_rows=True, tabs=None):
        """geometry of the field lines (tables.s[line_surf[i]], line_alpha[i]) on the grid theta (row F1).
        Returns dict(geo=(8, n_lines, N), dPdrho=(n_lines,)); geo[0..6] + dPdrho feed gamma_scan directly.
        device=None: numpy in / numpy out (staged);  device=torch.device(...): results stay in HBM.
        tabs (device calls): (tab_mn, tab_nyq, scal) device tensors to use in place of the tables' resident copies, for any
        number of surfaces (ibs_amd.autograd.fieldline_geometry); the mode tables stay those of `tables`."""
        n_lines, N = len(line_surf), len(theta)
        ar = _Args(self, device=device, host=device is None)
        n_surf, head, rows = ar.tables(tables, tabs, use_rows)
        pls, pla, pth = ar.lines(line_surf, line_alpha, theta, n_surf)
        ar.call("ibs_fieldline_geometry_f64", *head, n_lines, pls, pla, N, pth, N, ar.out("geo", (8, n_lines, N)),
                ar.out("dPdrho", (n_lines,)), *rows)
        return ar.result()

    def fieldline_geometry_vjp(self, tables, line_surf, line_alpha, theta, geo_bar, dPdrho_bar=None, device=None,
                               want=("tab_mn", "tab_nyq", "scal", "alpha"), tabs=None):
        """vector-Jacobian product of fieldline_geometry (ibs_fieldline_geometry_vjp_f64): cotangents geo_bar (8, n_lines, N)
        and, optionally, dPdrho_bar (n_lines,) -> dict(tab_mn_bar (n_surf, 6, mnmax), tab_nyq_bar (n_surf, 7, mnmax_nyq),
        scal_bar (n_surf, 6), alpha_bar (n_lines,)); entries not named in `want` are None.  Exact: the root solve of
        utils.py:391-416 by the implicit-function theorem.  Sums run in a fixed order: repeatable bit for bit.
        device=None: numpy in / numpy out (staged);  device=torch.device(...): device tensors in, device tensors out.
        tabs: as in fieldline_geometry."""
        want = set(want)
        if not want or not want <= {"tab_mn", "tab_nyq", "scal", "alpha"}:
            raise IbsError("want must name at least one of tab_mn, tab_nyq, scal, alpha")
        n_lines, N = len(line_surf), len(theta)
        if tuple(geo_bar.shape) != (8, n_lines, N):
            raise IbsError("geo_bar must be (8, n_lines, N)")
        ar = _Args(self, device=device, host=device is None)
        n_surf, head, _ = ar.tables(tables, tabs)
        pls, pla, pth = ar.lines(line_surf, line_alpha, theta, n_surf)
        shapes = dict(tab_mn=(n_surf, 6, head[1]), tab_nyq=(n_surf, 7, head[2]), scal=(n_surf, 6), alpha=(n_lines,))
        ar.call("ibs_fieldline_geometry_vjp_f64", *head, n_lines, pls, pla, N, pth, N, ar.inp(geo_bar), ar.inp(dPdrho_bar),
                *[ar.out(k + "_bar", shape, want=k in want) for k, shape in shapes.items()])
        return {k + "_bar": ar.outs.get(k + "_bar") for k in shapes}

    def fieldline_geometry_dalpha(self, tables, line_surf, line_alpha, theta, device=None):
        """alpha-tangent of fieldline_geometry (ibs_fieldline_geometry_dalpha_f64): dict(geo_da=(8, n_lines, N)), the derivative of the
        eight arrays of every line in its own alpha -- the derivative in place of the central difference of utils.py:1641-1646 /
        1683-1718.  dPdrho does not depend on alpha and has no tangent.  One lane per grid point: a line alone gives its batch bits.
        device=None: numpy in / numpy out (staged);  device=torch.device(...): numpy or device tensors in, a device tensor out."""
        n_lines, N = len(line_surf), len(theta)
        ar = _Args(self, device=device, host=device is None)
        n_surf, head, _ = ar.tables(tables)
        pls, pla, pth = ar.lines(line_surf, line_alpha, theta, n_surf)
        ar.call("ibs_fieldline_geometry_dalpha_f64", *head, n_lines, pls, pla, N, pth, N, ar.out("geo_da", (8, n_lines, N)))
        return ar.result()

    def _device_tables(self, tables, device, filled=True):
        """the surface/mode/row tables of `tables` resident on `device` (uploaded once, cached on the object); filled=False leaves
        tab_mn, tab_nyq and scal empty on creation, for a row-wise upload"""
        import torch
        cache = tables.__dict__.setdefault("_device_copies", {})
        key = _device_key(device)
        if key not in cache:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            big = up if filled else (lambda a: torch.empty(a.shape, dtype=torch.float64, device=device))
            cache[key] = [up(tables.xm), up(tables.xn), up(tables.xm_nyq), up(tables.xn_nyq), big(tables.tab_mn), big(tables.tab_nyq),
                          big(tables.scal), up(tables.rows_mn), up(tables.rows_nyq)]
            # (a caching allocator may hand these rows the addresses of a freed table set: the library's verdict on device-resident
            #  rows is keyed by address and size)
            self.set_option("forget_rows", 1)
        return cache[key]

    def upload_tables_rows(self, tables, device, r0, r1):
        """(re)upload the surfaces r0 .. r1 - 1 of `tables` into its resident device copies (allocated on first use);
        asynchronous on the current torch stream when the host arrays are page-locked (SurfaceTables.frame(pinned=True)).
        For callers that fill a frame piece by piece while earlier pieces are already being worked on."""
        import torch
        dev = self._device_tables(tables, device, filled=False)
        pinned = getattr(tables, "_pinned", {})
        for k, name in ((4, "tab_mn"), (5, "tab_nyq"), (6, "scal")):
            src = pinned[name] if name in pinned else torch.from_numpy(getattr(tables, name))
            dev[k][r0:r1].copy_(src[r0:r1], non_blocking=True)

    def _refine(self, ar, tables, n, pt_surf, starts, n_theta, theta, del_alpha, maxiter, ftol, gtol):
        """the one call of ibs_refine_f64 -> (packed result buffer, rounds)"""
        _, head, rows = ar.tables(tables)
        pout = ar.out("packed", (4 * n,)).value or 0
        rounds = ar.call("ibs_refine_f64", *head, *rows, n, ar.inp(pt_surf, _I32, True), ar.inp(starts, _F64, True), n_theta,
                         ar.inp(theta, _F64, True), float(del_alpha), int(maxiter), float(ftol), float(gtol), C.c_void_p(pout),
                         C.c_void_p(pout + 16 * n), C.c_void_p(pout + 24 * n))
        return ar.outs["packed"], rounds

    def refine(self, tables, pt_surf, starts, theta, del_alpha=0.004, maxiter=30, ftol=5.0e-11, gtol=2.0e-8, device=None):
        """maximise gam over (alpha, theta0) from starts (n, 2) on surfaces tables.s[pt_surf] -- the whole
        quasi-Newton loop runs on the device (ibs_refine_f64; replaces ball_scan.py:305-314).
        Returns (x_opt (n, 2), f_opt (n,) = -gam, n_evals (n,), rounds) as numpy."""
        ps = np.ascontiguousarray(pt_surf, dtype=np.int32)
        st = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 2)
        th = np.ascontiguousarray(theta, dtype=np.float64)
        n = len(ps)
        if st.shape[0] != n:
            raise IbsError("starts must be (len(pt_surf), 2)")
        if ps.size and (ps.min() < 0 or ps.max() >= len(tables.s)):
            raise IbsError("pt_surf out of range")
        ar = _Args(self, device=device, host=device is None)
        if device is not None:
            # the grid and the point -> surface map rarely change between calls: their device copies are kept on the tables
            # object, keyed by content; the start points go up in one copy, the results come back in one
            import torch
            cache = tables.__dict__.setdefault("_refine_inputs", {})
            key = (_device_key(device), th.tobytes(), ps.tobytes())
            if key not in cache:
                cache.clear()
                cache[key] = (torch.from_numpy(ps).to(device), torch.from_numpy(th).to(device))
            ps, th = cache[key]
        out, rounds = self._refine(ar, tables, n, ps, st, len(th), th, del_alpha, maxiter, ftol, gtol)
        xo, fo, ne = _refine_views(out if device is None else out.cpu(), n)
        return (xo, fo, ne, rounds) if device is None else (xo.numpy(), fo.numpy(), ne.numpy().copy(), rounds)

    def refine_device(self, tables, d_pt_surf, d_start, d_theta, del_alpha=0.004, maxiter=30, ftol=5.0e-11, gtol=2.0e-8):
        """refine() on device tensors, results left in HBM: d_pt_surf (n,) int32, d_start (n, 2), d_theta (N,) float64.
        Returns (x_opt (n, 2), f_opt (n,) = -gam, n_evals (n,) int32, rounds); the tensors are stream-ordered on the
        current torch stream (include/ibs.h: ibs_refine_f64 with device pointers)."""
        n = int(d_pt_surf.shape[0])
        out, rounds = self._refine(_Args(self, device=d_start.device), tables, n, d_pt_surf, d_start, int(d_theta.shape[0]), d_theta,
                                   del_alpha, maxiter, ftol, gtol)
        return (*_refine_views(out, n), rounds)

    def refine_stats(self):
        """(evaluations, forward sweeps, rounds needed, rounds enqueued) of the last refine() call of this context"""
        out = np.zeros(4, dtype=np.int64)
        check(self._lib.ibs_refine_stats(self._h, C.c_void_p(out.ctypes.data)), "ibs_refine_stats")
        return tuple(int(v) for v in out)

    def hf_grad(self, X, dX, f, g_p, c_p, f_p, gam):
        """Hellmann-Feynman d(gam)/dp for caller-built tangents (utils.py:1676-1680, 1721-1725).
        X, dX, f, g_p, c_p, f_p: (n_sys, N); gam: (n_sys,) -> jac (n_sys,)"""
        ar = _Args(self)
        n_sys, N = X.shape
        ar.call("ibs_hf_grad_f64", n_sys, N, *[ar.inp(a) for a in (X, dX, f, g_p, c_p, f_p)], N, ar.inp(gam), ar.out("jac", (n_sys,)))
        return ar.outs["jac"]

    def sturm_count(self, h, g, c, f, shift, exact=False):
        """eigenvalues of (T, F) above shift[i] per system (ibs_sturm_count_f64).  exact=True: the division-form kernel (lanes as
        systems: a few eps ||A||, any N, ~5 TB/s in big batches) instead of the prefix-product sweep (N <= 2050: ~6 TB/s, exact for
        ~N eps ||A|| on smooth and up to ~N^2 eps ||A|| on iid-random coefficients: within that distance of an eigenvalue it can be
        off by one).  Without it the library picks by size (include/ibs.h: ibs_sturm_count_f64)."""
        if exact:
            self.set_option("sturm_form", 2)
            try:
                return self.sturm_count(h, g, c, f, shift)
            finally:
                self.set_option("sturm_form", None)
        ar = _Args(self)
        n_sys, N = g.shape
        ar.call("ibs_sturm_count_f64", n_sys, N, float(h), ar.inp(g), ar.inp(c), ar.inp(f), N, ar.inp(shift), ar.out("count", (n_sys,), _I32))
        return ar.outs["count"]

    # ---- geometry-fed Sturm count, count-pair certificate and re-close (ibs_certify.hip) ------
    def geo_sturm_count(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, shift=0.0):
        """eigenvalues above shift for every (line, theta0) of a geometry-fed scan (ibs_geo_sturm_count_f64: the number of unstable
        modes at shift 0, bishop_ball_s-alpha.py:110-115 for real field lines).  Arrays as in gamma_scan; shift a scalar or
        (n_lines, n_theta0).  Returns int32 (n_lines, n_theta0).  Even N is accepted."""
        ar = _Args(self)
        head, shape, N = ar.geo(h, (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22), dPdrho, theta0)
        ar.call("ibs_geo_sturm_count_f64", *head, ar.rows(shift, shape), ar.out("count", shape, _I32))
        return ar.outs["count"]

    @staticmethod
    def _one_theta0_per_point(points, geo7, theta0):
        if points and int(theta0.shape[0]) != geo7[0].shape[0]:
            raise IbsError("theta0 must hold one value per point (%d), got %d" % (geo7[0].shape[0], int(theta0.shape[0])))

    def _certify(self, points, h, geo7, dPdrho, theta0, lam, tol_factor):
        self._one_theta0_per_point(points, geo7, theta0)
        ar = _Args(self)
        head, shape, N = ar.geo(h, geo7, dPdrho, theta0, points)
        ar.call("ibs_gamma_points_certify_f64" if points else "ibs_gamma_scan_certify_f64", *head, ar.inp(lam), float(tol_factor),
                ar.out("cert", shape, _I32))
        return ar.outs["cert"]

    def certify_scan(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, lam, tol_factor=0.0):
        """count-pair certificate of the eigenvalues lam (n_lines, n_theta0) of a geometry-fed scan (ibs_gamma_scan_certify_f64): with
        tol = tol_factor N eps ||A|| (tol_factor <= 0: 4) the division-form Sturm counts must read 0 above lam + tol and >= 1 above
        lam - tol.  Returns cert, int32 (n_lines, n_theta0): 0 = certified; bit 0 = lam is not the largest eigenvalue; bit 1 = no
        eigenvalue at lam; bit 2 = not checked (lam not finite or invalid data)."""
        return self._certify(False, h, (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22), dPdrho, theta0, lam, tol_factor)

    def certify_points(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, lam, tol_factor=0.0):
        """certify_scan for the points of gamma_points: theta0, lam (n_pts,) -> cert (n_pts,) (ibs_gamma_points_certify_f64)"""
        return self._certify(True, h, (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22), dPdrho, theta0, lam, tol_factor)

    def _reclose(self, points, h, geo7, dPdrho, theta0, cert, lam, gam, X, dX, tol_factor):
        self._one_theta0_per_point(points, geo7, theta0)
        ar = _Args(self)
        head, shape, N = ar.geo(h, geo7, dPdrho, theta0, points)
        return ar.call("ibs_gamma_points_reclose_f64" if points else "ibs_gamma_scan_reclose_f64", *head, float(tol_factor),
                       ar.inout("reclose", "cert", cert, _I32), ar.inout("reclose", "lam", lam, _F64), ar.inout("reclose", "gam", gam, _F64),
                       ar.inout("reclose", "X", X, _F64, optional=True), ar.inout("reclose", "dX", dX, _F64, optional=True))

    def reclose_scan(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, cert, lam, gam, X=None, dX=None,
                     tol_factor=0.0):
        """re-close of the systems certify_scan refused (ibs_gamma_scan_reclose_f64), IN PLACE: every system whose cert has bit 0 or
        1 is solved again in division form and certified again; on success its lam, gam (X, dX) are replaced and its cert becomes 8,
        else it keeps its bits; all other entries stay untouched bit for bit.  cert int32, lam, gam (n_lines, n_theta0), X, dX
        (n_lines, n_theta0, N) optional: contiguous arrays of exactly those types.  Device tensors: nothing is read back, returns 0;
        numpy arrays: returns the number of systems that still carry bit 0 or 1."""
        return self._reclose(False, h, (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22), dPdrho, theta0, cert, lam, gam, X, dX,
                             tol_factor)

    def reclose_points(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, cert, lam, gam, X=None, dX=None,
                       tol_factor=0.0):
        """reclose_scan for the points of gamma_points (ibs_gamma_points_reclose_f64): cert, lam, gam (n_pts,), X, dX (n_pts, N)"""
        return self._reclose(True, h, (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22), dPdrho, theta0, cert, lam, gam, X, dX,
                             tol_factor)

    def surface_argmax_pack(self, gam):
        """gam: device tensor (n_surf, n_per_surf) -> pack (n_surf, 2) = (max, first row-major index) on the device
        (ibs_surface_argmax_pack_f64; ball_scan.py:283-288), the input of scan_starts."""
        ar = _Args(self)
        n_surf, n_per = gam.shape
        pgam = ar.inp(gam)
        if ar.mem != MEM_DEVICE:
            raise IbsError("surface_argmax_pack takes a device tensor")
        ar.call("ibs_surface_argmax_pack_f64", n_surf, n_per, pgam, ar.out("pack", (n_surf, 2)), mem=False)
        return ar.outs["pack"]

    def surface_argmax(self, gam):
        """gam: (n_surf, n_per_surf) -> (idx int32 (n_surf,), val (n_surf,)); first index on ties (ball_scan.py:283-288)."""
        ar = _Args(self)
        n_surf, n_per = gam.shape
        ar.call("ibs_surface_argmax_f64", n_surf, n_per, ar.inp(gam), ar.out("idx", (n_surf,), _I32), ar.out("val", (n_surf,)))
        return ar.outs["idx"], ar.outs["val"]


_DEFAULT = {}


def default_context(device=0):
    if device not in _DEFAULT:
        _DEFAULT[device] = Context(device)
    return _DEFAULT[device]


class ScanPlan:
    """Pre-marshalled geometry x theta0 scan + per-surface argmax on device-resident tensors: one
    optimizer iteration's worth of work is two kernel launches and no allocation.
    (Counterpart of the per-surface body of ball_scan.py:248-295.)

    geometry tensors: (n_lines, N) torch.cuda float64, lines ordered surface-major
    (n_lines = n_surf * n_alpha).  Results live in .gam (n_lines, n_theta0), .lam, .best_val (n_surf,),
    .best_idx (n_surf,) -- index into the flattened (alpha, theta0) table of the surface; both are views of
    .pack (n_surf, 2) float64, the buffer the per-surface all-gather sends."""

    def __init__(self, ctx, h, geo7, dPdrho, theta0, n_surf, want_dtheta0=False, n_pack=2):
        import torch
        self.ctx = ctx
        self.lib = ctx._lib
        t64 = torch.float64
        self.geo = [g.to(t64).contiguous() for g in geo7]
        dev = self.geo[0].device
        self.dP = dPdrho.to(t64).contiguous()
        self.t0 = theta0.to(t64).contiguous()
        n_lines, N = self.geo[0].shape
        n_t0 = self.t0.shape[0]
        if n_lines % n_surf:
            raise IbsError("n_lines=%d is not a multiple of n_surf=%d" % (n_lines, n_surf))
        self.n_lines, self.N, self.n_t0, self.n_surf = n_lines, N, n_t0, n_surf
        self.gam = torch.empty((n_lines, n_t0), dtype=t64, device=dev)
        self.lam = torch.empty((n_lines, n_t0), dtype=t64, device=dev)
        self.dth0 = torch.empty((n_lines, n_t0), dtype=t64, device=dev) if want_dtheta0 else None
        self.info = torch.empty((n_lines, n_t0), dtype=torch.int32, device=dev)
        # (lam_max, flat index) per surface; n_pack buffers so that the all-gather of one step can still be reading its
        # buffer while later steps' argmax write the others (argmax(slot))
        self.packs = [torch.empty((n_surf, 2), dtype=t64, device=dev) for _ in range(max(1, int(n_pack)))]
        self.pack = self.packs[0]
        self.best_val = self.pack[:, 0]
        self.best_idx = self.pack[:, 1]
        ctx._stream_from_torch(self.geo[0])
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)
        self._scan_args = (ctx._h, n_lines, n_t0, N, float(h), *[p(g) for g in self.geo], N, p(self.dP), p(self.t0),
                           p(self.gam), p(self.lam), C.c_void_p(None), C.c_void_p(None), p(self.dth0), p(self.info),
                           MEM_DEVICE)
        self._amax_args = [(ctx._h, n_surf, (n_lines // n_surf) * n_t0, p(self.gam), p(pk)) for pk in self.packs]
        self._fused_args = [(ctx._h, n_lines, n_t0, N, float(h), *[p(g) for g in self.geo], N, p(self.dP), p(self.t0), n_surf,
                             p(self.gam), p(self.lam), p(pk), p(self.info)) for pk in self.packs]

    def _use_current_stream(self):
        # the Context's stream is shared mutable state: launch on the caller's CURRENT torch stream, like every other
        # Context call (a plan used under torch.cuda.stream(s) must be ordered against that stream's tensors)
        import torch
        self.lib.ibs_set_stream(self.ctx._h, C.c_void_p(torch.cuda.current_stream(self.gam.device).cuda_stream))

    def scan(self):
        self._use_current_stream()
        rc = self.lib.ibs_gamma_scan_f64(*self._scan_args)
        if rc < 0:
            check(rc, "ibs_gamma_scan_f64")

    def argmax(self, slot=0):
        self._use_current_stream()
        rc = self.lib.ibs_surface_argmax_pack_f64(*self._amax_args[slot])
        if rc < 0:
            check(rc, "ibs_surface_argmax_pack_f64")

    def scan_argmax(self, slot=0):
        """scan + per-surface first maximum in one C call (ibs_gamma_scan_argmax_f64: one kernel launch for small batches)"""
        self._use_current_stream()
        rc = self.lib.ibs_gamma_scan_argmax_f64(*self._fused_args[slot])
        if rc < 0:
            check(rc, "ibs_gamma_scan_argmax_f64")

    def __call__(self):
        self.scan_argmax()
