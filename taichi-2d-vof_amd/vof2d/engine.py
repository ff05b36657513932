"""Thin object wrapper over one C-ABI handle (include/vof2d.h).

An Engine is one strip of the grid (the full domain when row_lo = 0 and
row_hi = nx+1).  It owns nothing but the handle; every method is one call
through the ABI.  `api` is an `_abi.Api`; the product passes the HIP library's
(`_lib.hip_api()`), tests may pass the oracle's.
"""
import ctypes as C

import numpy as np

from . import _abi

NP_DTYPE = {_abi.VOF_F64: np.float64, _abi.VOF_F32: np.float32}
DTYPE_CODE = {"f64": _abi.VOF_F64, "float64": _abi.VOF_F64, "fp64": _abi.VOF_F64,
              "f32": _abi.VOF_F32, "float32": _abi.VOF_F32, "fp32": _abi.VOF_F32}


class VofError(RuntimeError):
    pass


def dtype_code(dtype):
    if isinstance(dtype, str):
        return DTYPE_CODE[dtype.lower()]
    if dtype in (_abi.VOF_F64, _abi.VOF_F32) and not isinstance(dtype, type):
        return int(dtype)
    return {np.dtype(np.float64): _abi.VOF_F64, np.dtype(np.float32): _abi.VOF_F32}[np.dtype(dtype)]


def criterion_code(criterion):
    return {"abs": _abi.VOF_RESID_ABS, "rel": _abi.VOF_RESID_REL}[criterion]


def _due(nsteps, every):   # the records a vof_step_<verb> call owes: one per whole group (0 for arguments the library refuses)
    return max(nsteps, 0) // every if every >= 1 else 0


def make_desc(api, nx, ny, dtype="f64", coord_cast="f32", rows=None, own=None, jacobi_iters=10,
              device=-1, flags=0, **consts):
    """vof_desc_default + overrides.  rows=(row_lo,row_hi), own=(own_lo,own_hi)."""
    d = _abi.Desc()
    rc = api.desc_default(C.byref(d), int(nx), int(ny), dtype_code(dtype))
    if rc != 0:
        raise VofError("vof_desc_default(%d, %d) failed: %s" % (nx, ny, _abi.ERRNAMES.get(rc, rc)))
    if coord_cast not in ("f32", "none"):
        raise ValueError("coord_cast must be 'f32' or 'none'")
    d.coord_cast_f32 = 1 if coord_cast == "f32" else 0
    if rows is not None:
        d.row_lo, d.row_hi = int(rows[0]), int(rows[1])
        d.own_lo = max(1, d.row_lo)
        d.own_hi = min(int(nx), d.row_hi)
    if own is not None:
        d.own_lo, d.own_hi = int(own[0]), int(own[1])
    d.jacobi_iters = int(jacobi_iters)
    d.device = int(device)
    d.flags = int(flags)
    for k, v in consts.items():
        if k not in ("Lx", "Ly", "rho_l", "rho_g", "nu_l", "nu_g", "sigma", "gx", "gy", "dt"):
            raise TypeError("unknown constant %r" % k)
        setattr(d, k, float(v))
    return d


class Engine:
    def __init__(self, api, desc, stream=None):
        self.api = api
        self.desc = desc
        self._h = _abi.H()
        rc = api.create(C.byref(desc), C.c_void_p(stream) if stream else None, C.byref(self._h))
        if rc != 0:
            self._h = None
            raise VofError("vof_create failed: %s" % _abi.ERRNAMES.get(rc, rc))
        self.nx, self.ny = desc.nx, desc.ny
        self.row_lo, self.row_hi = desc.row_lo, desc.row_hi
        self.own_lo, self.own_hi = desc.own_lo, desc.own_hi
        self.nrows = self.row_hi - self.row_lo + 1
        self.np_dtype = NP_DTYPE[desc.dtype]

    # -- plumbing ---------------------------------------------------------
    @property
    def handle(self):
        return self._h

    def _ck(self, rc, what):
        if rc != 0:
            msg = self.api.last_error(self._h) if self._h else b""
            raise VofError("%s%s failed: %s %s" % (self.api.prefix, what, _abi.ERRNAMES.get(rc, rc),
                                                   (msg or b"").decode(errors="replace")))

    def close(self):
        if self._h:
            self.api.destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- reference verbs (2dvof.py kernels) --------------------------------
    def set_init_F(self, ic):
        self._ck(self.api.set_init_F(self._h, int(ic)), "set_init_F")

    def set_scene(self, shapes, samples=8, clear=True):
        """vof_set_scene: paints the shapes (a list of records of vof2d/scene.py, or the array of scene.pack) into F on the
        rows this handle stores, samples x samples sample points a cell, in list order; clear=True empties the domain first,
        clear=False paints over the F that is there.  Returns the summary as a dict keyed by scene.SUMMARY."""
        from . import scene
        recs = scene.pack(shapes)
        summ = (C.c_double * _abi.VOF_SCENE_SUM_N)()
        self._ck(self.api.set_scene(self._h, recs.ctypes.data_as(C.POINTER(C.c_double)) if len(recs) else None, len(recs),
                                    scene.check_samples(samples), _abi.VOF_SCENE_CLEAR if clear else 0, summ), "set_scene")
        return scene.summary_of(list(summ))

    def set_BC(self):
        self._ck(self.api.set_BC(self._h), "set_BC")

    def cal_nu_rho(self):
        self._ck(self.api.cal_nu_rho(self._h), "cal_nu_rho")

    def get_normal_young(self):
        self._ck(self.api.get_normal_young(self._h), "get_normal_young")

    def advect_upwind(self):
        self._ck(self.api.advect_upwind(self._h), "advect_upwind")

    def solve_p_jacobi(self, n=1):
        self._ck(self.api.solve_p_jacobi(self._h, int(n)), "solve_p_jacobi")

    def update_uv(self):
        self._ck(self.api.update_uv(self._h), "update_uv")

    def fct_x_sweep(self):
        self._ck(self.api.fct_x_sweep(self._h), "fct_x_sweep")

    def fct_y_sweep(self):
        self._ck(self.api.fct_y_sweep(self._h), "fct_y_sweep")

    def solve_VOF_rudman(self, istep):
        self._ck(self.api.solve_VOF_rudman(self._h, int(istep)), "solve_VOF_rudman")

    def post_process_f(self):
        self._ck(self.api.post_process_f(self._h), "post_process_f")

    def step(self, nsteps=1):
        self._ck(self.api.step(self._h, int(nsteps)), "step")

    def step_phase(self, phase):
        self._ck(self.api.step_phase(self._h, int(phase)), "step_phase")

    @property
    def istep(self):
        v = C.c_int64()
        self._ck(self.api.get_istep(self._h, C.byref(v)), "get_istep")
        return v.value

    @istep.setter
    def istep(self, value):
        self._ck(self.api.set_istep(self._h, int(value)), "set_istep")

    # -- extensions ---------------------------------------------------------
    def solve_p_residual(self, tol, max_iters, check_every=10):
        it, res = C.c_int32(), C.c_double()
        self._ck(self.api.solve_p_residual(self._h, float(tol), int(max_iters), int(check_every),
                                           C.byref(it), C.byref(res)), "solve_p_residual")
        return it.value, res.value

    def solve_p(self, tol, max_iters, check_every=10, criterion="abs"):
        """vof_solve_p: sweeps until the residual (\"abs\": max|p_new - p|; \"rel\": that over
        max(max|p_new|, tiny)) is <= tol; returns (sweeps done, residual).  Same defaults as
        StripSolver.solve_p and vof_solve_p_residual (absolute criterion, a check every 10 sweeps)."""
        crit = criterion_code(criterion)
        it, res = C.c_int32(), C.c_double()
        self._ck(self.api.solve_p(self._h, float(tol), int(max_iters), int(check_every), crit,
                                  C.byref(it), C.byref(res)), "solve_p")
        return it.value, res.value

    def solve_p_cg(self, tol, max_iters, check_every=10, criterion="abs", build_rhs=True):
        """vof_solve_p_cg: conjugate gradients on the pressure equation until max|z| (\"abs\"; \"rel\": over
        max(max|p|, tiny)) is <= tol, z = what one more Jacobi sweep would change beyond the drift constant;
        returns (iterations done, residual, drift)."""
        crit = criterion_code(criterion)
        it, res, drift = C.c_int32(), C.c_double(), C.c_double()
        self._ck(self.api.solve_p_cg(self._h, float(tol), int(max_iters), int(check_every), crit,
                                     1 if build_rhs else 0, C.byref(it), C.byref(res), C.byref(drift)), "solve_p_cg")
        return it.value, res.value, drift.value

    def solve_p_mg(self, tol, max_cycles, check_every=1, criterion="abs", build_rhs=True):
        """vof_solve_p_mg: V-cycles of geometric multigrid on the equation of solve_p_cg, same residual and stopping
        rule; returns (cycles done, residual, drift).  Knobs (set_param): mg_nu, mg_levels."""
        crit = criterion_code(criterion)
        it, res, drift = C.c_int32(), C.c_double(), C.c_double()
        self._ck(self.api.solve_p_mg(self._h, float(tol), int(max_cycles), int(check_every), crit,
                                     1 if build_rhs else 0, C.byref(it), C.byref(res), C.byref(drift)), "solve_p_mg")
        return it.value, res.value, drift.value

    def step_mg(self, nsteps, cycles, criterion="rel"):
        """vof_step_mg: nsteps time steps whose pressure solve is `cycles` V-cycles of solve_p_mg's cycle, warm-started
        from p; returns (residual of the last step, worst residual of the call, the istep it belongs to).  One read-back,
        at the end.  Knobs (set_param): mg_nu, mg_levels, mg_graph, mg_coarse_block."""
        crit = criterion_code(criterion)
        last, worst, at = C.c_double(), C.c_double(), C.c_int64()
        self._ck(self.api.step_mg(self._h, int(nsteps), int(cycles), crit, C.byref(last), C.byref(worst), C.byref(at)), "step_mg")
        return last.value, worst.value, at.value

    def diagnostics(self):
        """vof_diagnostics: one fixed-order pass over F, u, v on the owned interior cells; the raw row as a dict keyed by
        diag.NAMES (a strip's value is its partial: diag.combine; the physical quantities: diag.derive)."""
        from . import diag
        row = (C.c_double * _abi.VOF_DIAG_N)()
        self._ck(self.api.diagnostics(self._h, row), "diagnostics")
        return diag.raw_of(list(row))

    def step_diag(self, nsteps, every, mg_cycles=0, criterion="rel"):
        """vof_step_diag: nsteps steps (of vof_step; of vof_step_mg with mg_cycles >= 1), a row of diagnostics recorded on
        the device behind every `every` of them, one read-back at the end; returns the (rows, VOF_DIAG_N) float64 array."""
        crit = criterion_code(criterion)
        rows = _due(int(nsteps), int(every))
        out = np.zeros((rows, _abi.VOF_DIAG_N), dtype=np.float64)
        done = C.c_int64()
        self._ck(self.api.step_diag(self._h, int(nsteps), int(every), int(mg_cycles), crit,
                                    out.ctypes.data_as(C.POINTER(C.c_double)) if rows else None, rows, C.byref(done)), "step_diag")
        return out[:done.value]

    def interface(self, eps=1e-6):
        """vof_interface: one PLIC segment per mixed cell (eps < F < 1 - eps) of the owned interior rows, reconstructed and
        compacted on the device in ascending (i, j) order; returns (rows, summary): an (n, VOF_IFACE_N) float64 array (the
        slots: vof2d/interface.py) and the summary as a dict keyed by interface.SUMMARY.  One call with the capacity the
        last call needed (plus a margin); a second one if the list has outgrown it."""
        from . import interface
        summ = (C.c_double * _abi.VOF_IFACE_SUM_N)()
        rows = self._sized_rows("_iface_cap", 0, _abi.VOF_IFACE_N, summ, _abi.VOF_IFACE_SUM_SEGMENTS, "interface",
                                lambda ptr, cap: self.api.interface(self._h, float(eps), ptr, cap, summ))
        return rows, interface.summary_of(list(summ))

    def curvature(self, eps=1e-6):
        """vof_curvature: one row per mixed cell with an orientation -- the cells and the order of interface() at the same eps --
        holding the height-function curvature, whether its three columns span the interface, the axis, the solver's own CSF
        curvature at the cell, the slope and F; whole-domain handles only.  Returns (rows, summary): an (n, VOF_CURV_N) float64
        array (the slots: vof2d/curvature.py) and the summary as a dict keyed by curvature.SUMMARY.  One call with the capacity
        the last call needed (plus a margin); a second one if the list has outgrown it."""
        from . import curvature
        summ = (C.c_double * _abi.VOF_CURV_SUM_N)()
        rows = self._sized_rows("_curv_cap", 0, _abi.VOF_CURV_N, summ, _abi.VOF_CURV_SUM_ROWS, "curvature",
                                lambda ptr, cap: self.api.curvature(self._h, float(eps), ptr, cap, summ))
        return rows, curvature.summary_of(list(summ))

    def energy(self):
        """vof_energy: the energy budget in one fixed-order pass over F, u, v, p -- face kinetic energy, density moments, the
        interface measure and the power of every term of the momentum predictor; whole-domain handles only.  The raw row as a
        dict keyed by energy.NAMES (the physical quantities: energy.derive)."""
        from . import energy
        row = (C.c_double * _abi.VOF_ENERGY_N)()
        self._ck(self.api.energy(self._h, row), "energy")
        return energy.raw_of(list(row))

    def step_energy(self, nsteps, every, mg_cycles=0, criterion="rel"):
        """vof_step_energy: nsteps steps (of vof_step; of vof_step_mg with mg_cycles >= 1), a row of the energy budget recorded on
        the device behind every `every` of them, one read-back at the end; returns the (rows, VOF_ENERGY_N) float64 array."""
        crit = criterion_code(criterion)
        rows = _due(int(nsteps), int(every))
        out = np.zeros((rows, _abi.VOF_ENERGY_N), dtype=np.float64)
        done = C.c_int64()
        self._ck(self.api.step_energy(self._h, int(nsteps), int(every), int(mg_cycles), crit,
                                      out.ctypes.data_as(C.POINTER(C.c_double)) if rows else None, rows, C.byref(done)), "step_energy")
        return out[:done.value]

    def blobs(self, phase="liquid", threshold=0.5, labels=False):
        """vof_blobs: the connected pieces of the liquid (F >= threshold) or of the gas (F < threshold) on the owned interior
        rows, labelled and measured on the device; returns (rows, summary[, labels]): an (n, VOF_BLOB_N) float64 array in
        ascending order of the blobs' first cells (the slots: vof2d/blobs.py), the summary as a dict keyed by blobs.SUMMARY
        and, if asked for, the (owned interior rows, ny) int32 array of blob indices (-1: not a member).  One call with the
        capacity the last call needed (plus a margin); a second one if the list has outgrown it."""
        from . import blobs
        summ = (C.c_double * _abi.VOF_BLOB_SUM_N)()
        nrows = max(min(self.own_hi, self.nx) - max(self.own_lo, 1) + 1, 0)
        lab = np.empty((nrows, self.ny), dtype=np.int32) if labels else None
        rows = self._sized_rows("_blobs_cap", 16, _abi.VOF_BLOB_N, summ, _abi.VOF_BLOB_SUM_BLOBS, "blobs",
                                lambda ptr, cap: self.api.blobs(self._h, blobs.PHASES[phase], float(threshold), ptr, cap,
                                                                lab.ctypes.data_as(C.POINTER(C.c_int32)) if labels else None,
                                                                lab.nbytes if labels else 0, summ))
        out = (rows, blobs.summary_of(list(summ)))
        return out + (lab,) if labels else out

    def tracers_set(self, xy):
        """vof_tracers_set: replaces the handle's tracers by the (n, 2) positions xy (physical x, y inside the closed domain) and
        zeroes TIME; an empty array clears the set."""
        a = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        self._ck(self.api.tracers_set(self._h, a.ctypes.data_as(C.POINTER(C.c_double)) if len(a) else None, len(a)), "tracers_set")

    def tracers_advance(self, time):
        """vof_tracers_advance: one midpoint-rule advance of every tracer by `time` on the current u, v (enqueues only)."""
        self._ck(self.api.tracers_advance(self._h, float(time)), "tracers_advance")

    def tracers(self, rows=True):
        """vof_tracers_get: (rows, summary): the (COUNT, VOF_TRACER_N) float64 array of X, Y, U, V, F in the order the tracers were
        given (the slots: vof2d/tracers.py) and the summary as a dict keyed by tracers.SUMMARY.  rows=False reads the summary
        alone and returns (None, summary)."""
        from . import tracers
        summ = (C.c_double * _abi.VOF_TRACER_SUM_N)()
        if not rows:
            self._ck(self.api.tracers_get(self._h, None, 0, summ), "tracers_get")
            return None, tracers.summary_of(list(summ))
        out = self._sized_rows("_tracers_cap", 0, _abi.VOF_TRACER_N, summ, _abi.VOF_TRACER_SUM_COUNT, "tracers_get",
                               lambda ptr, cap: self.api.tracers_get(self._h, ptr, cap, summ))
        return out, tracers.summary_of(list(summ))

    def step_tracers(self, nsteps, every=1, mg_cycles=0, criterion="rel", snap_every=0):
        """vof_step_tracers: nsteps steps (of vof_step; of vof_step_mg with mg_cycles >= 1), the tracers advanced by every * dt
        behind every `every` of them, a snapshot of all rows recorded on the device behind every snap_every-th advance
        (0: none), one read-back at the end; returns the (snapshots, COUNT, VOF_TRACER_N) float64 array."""
        crit = criterion_code(criterion)
        nsteps, every, snap_every = int(nsteps), int(every), int(snap_every)
        due = _due(_due(nsteps, every), snap_every)
        count = int(self.tracers(rows=False)[1]["COUNT"]) if due else 0
        out = np.zeros((due, count, _abi.VOF_TRACER_N), dtype=np.float64)
        done = C.c_int64()
        self._ck(self.api.step_tracers(self._h, nsteps, every, int(mg_cycles), crit, snap_every,
                                       out.ctypes.data_as(C.POINTER(C.c_double)) if due else None, due, C.byref(done)), "step_tracers")
        return out[:done.value]

    def depths(self):
        """vof_depths: one pass over F on the owned interior cells; returns (depth_i, depth_j, top, summary): the sums of F
        along j per owned row and along the owned i per column (float64), the largest j with F >= 0.5 per owned row (int32,
        0: none) and the summary as a dict keyed by gauges.DEPTH_SUMMARY (a strip's value is its partial: gauges.combine;
        the physical quantities: gauges.derive)."""
        from . import gauges
        rows = max(min(self.own_hi, self.nx) - max(self.own_lo, 1) + 1, 0)
        di, dj, top = np.empty(rows, dtype=np.float64), np.empty(self.ny, dtype=np.float64), np.empty(rows, dtype=np.int32)
        summ = (C.c_double * _abi.VOF_DEPTH_SUM_N)()
        self._ck(self.api.depths(self._h, di.ctypes.data_as(C.POINTER(C.c_double)) if rows else None, rows, dj.ctypes.data_as(C.POINTER(C.c_double)), self.ny,
                                 top.ctypes.data_as(C.POINTER(C.c_int32)) if rows else None, rows, summ), "depths")
        return di, dj, top, gauges.depth_summary_of(list(summ))

    def gauges_set(self, xy):
        """vof_gauges_set: replaces the handle's gauges by the (n, 2) positions xy (physical x, y inside the closed domain) and
        zeroes RECORDS; an empty array clears the set."""
        a = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        self._ck(self.api.gauges_set(self._h, a.ctypes.data_as(C.POINTER(C.c_double)) if len(a) else None, len(a)), "gauges_set")

    def gauges_get(self, rows=True):
        """vof_gauges_get: (rows, summary): the (COUNT, VOF_GAUGE_N) float64 array of X, Y, U, V, F, P, DEPTH, TOP in the order
        the gauges were given (the slots: vof2d/gauges.py) and the summary as a dict keyed by gauges.SUMMARY.  rows=False
        reads the summary alone and returns (None, summary)."""
        from . import gauges
        summ = (C.c_double * _abi.VOF_GAUGE_SUM_N)()
        if not rows:
            self._ck(self.api.gauges_get(self._h, None, 0, summ), "gauges_get")
            return None, gauges.summary_of(list(summ))
        out = self._sized_rows("_gauges_cap", 0, _abi.VOF_GAUGE_N, summ, _abi.VOF_GAUGE_SUM_COUNT, "gauges_get",
                               lambda ptr, cap: self.api.gauges_get(self._h, ptr, cap, summ))
        return out, gauges.summary_of(list(summ))

    def step_gauges(self, nsteps, every=1, mg_cycles=0, criterion="rel"):
        """vof_step_gauges: nsteps steps (of vof_step; of vof_step_mg with mg_cycles >= 1), a record of every gauge taken on
        the device behind every `every` of them, one read-back at the end; returns the (records, COUNT, VOF_GAUGE_N)
        float64 array."""
        crit = criterion_code(criterion)
        nsteps, every = int(nsteps), int(every)
        due = _due(nsteps, every)
        count = int(self.gauges_get(rows=False)[1]["COUNT"]) if due else 0
        out = np.zeros((due, count, _abi.VOF_GAUGE_N), dtype=np.float64)
        done = C.c_int64()
        self._ck(self.api.step_gauges(self._h, nsteps, every, int(mg_cycles), crit,
                                      out.ctypes.data_as(C.POINTER(C.c_double)) if due else None, due, C.byref(done)), "step_gauges")
        return out[:done.value]

    def dye_set(self, arr):
        """vof_dye_set: replaces the handle's dye by the (nx+2, ny+2) array arr, ghost cells included, stored as given;
        None releases it."""
        if arr is None:
            self._ck(self.api.dye_set(self._h, None, 0), "dye_set")
            return
        a = np.ascontiguousarray(arr, dtype=self.np_dtype)
        if a.shape != (self.nx + 2, self.ny + 2):
            raise ValueError("dye: expected shape %s, got %s" % ((self.nx + 2, self.ny + 2), a.shape))
        self._ck(self.api.dye_set(self._h, a.ctypes.data_as(C.c_void_p), a.nbytes), "dye_set")

    def dye_get(self):
        """vof_dye_get: the dye as an (nx+2, ny+2) array of the handle's dtype."""
        out = np.empty((self.nx + 2, self.ny + 2), dtype=self.np_dtype)
        self._ck(self.api.dye_get(self._h, out.ctypes.data_as(C.c_void_p), out.nbytes), "dye_get")
        return out

    def dye_advance(self):
        """vof_dye_advance: one transport of the dye (both FCT sweeps in the order of the handle's istep, post_process_f, the
        boundary condition of F) on the current u, v (enqueues only)."""
        self._ck(self.api.dye_advance(self._h), "dye_advance")

    def dye_stats(self):
        """vof_dye_stats: one fixed-order pass over the dye, F, u, v on the interior cells; the raw row as a dict keyed by
        dye.NAMES (the physical quantities: dye.derive)."""
        from . import dye
        row = (C.c_double * _abi.VOF_DYE_N)()
        self._ck(self.api.dye_stats(self._h, row), "dye_stats")
        return dye.raw_of(list(row))

    def step_dye(self, nsteps, every=0, mg_cycles=0, criterion="rel"):
        """vof_step_dye: nsteps times one step (of vof_step; of vof_step_mg with mg_cycles >= 1) and one advance of the dye, a
        row of statistics recorded on the device behind every `every`-th step (0: none), one read-back at the end; returns
        the (rows, VOF_DYE_N) float64 array."""
        crit = criterion_code(criterion)
        nsteps, every = int(nsteps), int(every)
        rows = _due(nsteps, every)
        out = np.zeros((rows, _abi.VOF_DYE_N), dtype=np.float64)
        done = C.c_int64()
        self._ck(self.api.step_dye(self._h, nsteps, every, int(mg_cycles), crit,
                                   out.ctypes.data_as(C.POINTER(C.c_double)) if rows else None, rows, C.byref(done)), "step_dye")
        return out[:done.value]

    def set_frame_lut(self, table=None):
        """vof_frame_set_lut: replaces the handle's colour table by the (258, 3) uint8 array (frames.lut samples matplotlib's
        maps into one); None restores the default."""
        if table is None:
            self._ck(self.api.frame_set_lut(self._h, None), "frame_set_lut")
            return
        t = np.ascontiguousarray(table, dtype=np.uint8)
        if t.shape != (_abi.VOF_FRAME_LUT_ROWS, 3):
            raise ValueError("frame lut: expected shape (%d, 3), got %s" % (_abi.VOF_FRAME_LUT_ROWS, t.shape))
        self._ck(self.api.frame_set_lut(self._h, t.ctypes.data_as(C.POINTER(C.c_uint8))), "frame_set_lut")

    def frame(self, quantity="F", bx=1, by=None, lo=0.0, hi=0.0, contour=False, symmetric=False, rgb=True, means=False):
        """vof_frame: the quantity box-averaged over bx x by cells per pixel and coloured on the device; returns (rgb, means,
        summary): the (ph, pw, 3) uint8 picture (top of the domain first), the (pw, ph) float64 means (each None unless asked
        for) and the summary as a dict keyed by frames.SUMMARY.  lo == hi: the range of the picture."""
        from . import frames
        s = frames.spec(quantity, bx, by, lo, hi, contour, symmetric)
        pw, ph = frames.shape(self.nx, self.ny, min(max(s.bx, 1), self.nx), min(max(s.by, 1), self.ny))
        img = np.empty((ph, pw, 3), dtype=np.uint8) if rgb else None
        mean = np.empty((pw, ph), dtype=np.float64) if means else None
        summ = (C.c_double * _abi.VOF_FRAME_SUM_N)()
        self._ck(self.api.frame(self._h, C.byref(s), img.ctypes.data_as(C.POINTER(C.c_uint8)) if rgb else None, img.nbytes if rgb else 0,
                                mean.ctypes.data_as(C.POINTER(C.c_double)) if means else None, mean.size if means else 0, summ), "frame")
        return img, mean, frames.summary_of(list(summ))

    def step_frames(self, nsteps, every, quantity="F", bx=1, by=None, lo=0.0, hi=0.0, contour=False, symmetric=False, mg_cycles=0, criterion="rel"):
        """vof_step_frames: nsteps steps (of vof_step; of vof_step_mg with mg_cycles >= 1), a frame rendered on the device
        behind every `every` of them, one read-back at the end; returns (pictures, summaries): the (frames, ph, pw, 3) uint8
        array and a list of dicts keyed by frames.SUMMARY."""
        from . import frames
        crit = criterion_code(criterion)
        nsteps, every = int(nsteps), int(every)
        due = _due(nsteps, every)
        s = frames.spec(quantity, bx, by, lo, hi, contour, symmetric)
        pw, ph = frames.shape(self.nx, self.ny, min(max(s.bx, 1), self.nx), min(max(s.by, 1), self.ny))
        out = np.zeros((due, ph, pw, 3), dtype=np.uint8)
        summ = np.zeros((due, _abi.VOF_FRAME_SUM_N), dtype=np.float64)
        done = C.c_int64()
        self._ck(self.api.step_frames(self._h, nsteps, every, int(mg_cycles), crit, C.byref(s), out.ctypes.data_as(C.POINTER(C.c_uint8)) if due else None,
                                      summ.ctypes.data_as(C.POINTER(C.c_double)) if due else None, due, C.byref(done)), "step_frames")
        return out[:done.value], [frames.summary_of(list(r)) for r in summ[:done.value]]

    def stats_begin(self, mask=3, level=0.5):
        """vof_stats_begin: allocates and clears the accumulator planes of the groups in `mask` (stats.MOMENTS | stats.ENVELOPE, or
        a sequence of group names); a cell counts as wet in a sample if its clamped F is >= level.  mask 0 releases them."""
        from . import stats
        self._ck(self.api.stats_begin(self._h, stats.mask_of(mask), float(level)), "stats_begin")

    def stats_sample(self):
        """vof_stats_sample: one sample of the fields as they are into the planes (enqueues only)."""
        self._ck(self.api.stats_sample(self._h), "stats_sample")

    def stats_plane(self, slot):
        """vof_stats_get: one plane (a slot number or a name of stats.PLANES) as an (nx, ny) float64 array indexed [i-1, j-1]."""
        from . import stats
        out = np.empty((self.nx, self.ny), dtype=np.float64)
        self._ck(self.api.stats_get(self._h, stats.slot_of(slot), out.ctypes.data_as(C.POINTER(C.c_double)), out.size), "stats_get")
        return out

    def stats_summary(self):
        """vof_stats_summary: the summary as a dict keyed by stats.SUMMARY."""
        from . import stats
        summ = (C.c_double * _abi.VOF_STATS_SUM_N)()
        self._ck(self.api.stats_summary(self._h, summ), "stats_summary")
        return stats.summary_of(list(summ))

    def step_stats(self, nsteps, every, mg_cycles=0, criterion="rel"):
        """vof_step_stats: nsteps steps (of vof_step; of vof_step_mg with mg_cycles >= 1), a sample taken on the device behind every
        `every` of them; nothing is read back.  Returns the number of samples taken."""
        done = C.c_int64()
        self._ck(self.api.step_stats(self._h, int(nsteps), int(every), int(mg_cycles), criterion_code(criterion), C.byref(done)), "step_stats")
        return done.value

    def _sized_rows(self, cap_attr, first_cap, width, summ, count_slot, what, call):
        """The rows of a verb that fills at most `cap` of them and reports in summ[count_slot] how many there are:
        call(rows pointer, cap) with the capacity the last call needed (plus a margin), once more if the list has outgrown it."""
        cap = getattr(self, cap_attr, first_cap)
        while True:
            rows = np.empty((cap, width), dtype=np.float64)
            self._ck(call(rows.ctypes.data_as(C.POINTER(C.c_double)) if cap else None, cap), what)
            n = int(summ[count_slot])
            if n <= cap:
                break
            cap = n + n // 8 + 16
        setattr(self, cap_attr, cap)
        return rows[:n].copy()

    def jacobi_sweeps_norms(self, n, build_rhs=True):
        """(max|p_new - p|, max|p_new|) of the last of n sweeps over the owned rows."""
        upd, pm = C.c_double(), C.c_double()
        self._ck(self.api.jacobi_sweeps_norms(self._h, int(n), 1 if build_rhs else 0, C.byref(upd), C.byref(pm)),
                 "jacobi_sweeps_norms")
        return upd.value, pm.value

    def jacobi_sweeps_residual(self, n, build_rhs=True):
        res = C.c_double()
        self._ck(self.api.jacobi_sweeps_residual(self._h, int(n), 1 if build_rhs else 0, C.byref(res)),
                 "jacobi_sweeps_residual")
        return res.value

    # -- fields -------------------------------------------------------------
    def get(self, name, rows=None):
        g0, g1 = (self.row_lo, self.row_hi) if rows is None else rows
        out = np.empty((g1 - g0 + 1, self.ny + 2), dtype=self.np_dtype)
        self._ck(self.api.get_rows(self._h, name.encode(), int(g0), int(g1),
                                   out.ctypes.data_as(C.c_void_p), out.nbytes), "get_rows(%s)" % name)
        return out

    def set(self, name, arr, rows=None):
        g0, g1 = (self.row_lo, self.row_hi) if rows is None else rows
        a = np.ascontiguousarray(arr, dtype=self.np_dtype)
        if a.shape != (g1 - g0 + 1, self.ny + 2):
            raise ValueError("field %s rows %d..%d: expected shape %s, got %s" %
                             (name, g0, g1, (g1 - g0 + 1, self.ny + 2), a.shape))
        self._ck(self.api.set_rows(self._h, name.encode(), int(g0), int(g1),
                                   a.ctypes.data_as(C.c_void_p), a.nbytes), "set_rows(%s)" % name)

    def vis_field(self, which):
        """rgb_buf of get_vof_field / get_u_field / get_v_field / get_vnorm_field (2dvof.py:458-486)."""
        out = np.empty((2 * self.nx, 2 * self.ny), dtype=self.np_dtype)
        self._ck(self.api.get_vis_field(self._h, which.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes),
                 "get_vis_field(%s)" % which)
        return out

    def interp_velocity(self):
        """V of interp_velocity (2dvof.py:488-492): (nx+2, ny+2, 2)."""
        out = np.empty((self.nx + 2, self.ny + 2, 2), dtype=self.np_dtype)
        self._ck(self.api.interp_velocity(self._h, out.ctypes.data_as(C.c_void_p), out.nbytes), "interp_velocity")
        return out

    def field_view(self, name):
        """(device base pointer, pitch, col0, nrows) -- element (i, j) at
        base + ((i-row_lo)*pitch + col0 + j) * itemsize."""
        base, pitch, col0, nrows = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int64()
        self._ck(self.api.field_view(self._h, name.encode(), C.byref(base), C.byref(pitch),
                                     C.byref(col0), C.byref(nrows)), "field_view(%s)" % name)
        return base.value, pitch.value, col0.value, nrows.value

    def copy_rows_from(self, src, name, g0, g1):
        self._ck(self.api.copy_rows(self._h, src._h, name.encode(), int(g0), int(g1)), "copy_rows")

    def regrid_from(self, src, plic=True, eps=1e-6, summary=True):
        """vof_regrid: F, u, v, p of the engine src carried onto this one's grid (finer or coarser by integer factors, or the
        same; either dtype), the boundary conditions applied, istep taken over; asynchronous unless the summary is asked for.
        Returns the summary as a dict keyed by regrid.SUMMARY, or None."""
        from . import regrid
        summ = (C.c_double * _abi.VOF_REGRID_SUM_N)() if summary else None
        self._ck(self.api.regrid(self._h, src._h, _abi.VOF_REGRID_PLIC if plic else 0, float(eps), summ), "regrid")
        return regrid.summary_of(list(summ)) if summary else None

    # -- scalars --------------------------------------------------------------
    def set_param(self, name, value):
        self._ck(self.api.set_param(self._h, name.encode(), float(value)), "set_param(%s)" % name)

    def get_param(self, name):
        v = C.c_double()
        self._ck(self.api.get_param(self._h, name.encode(), C.byref(v)), "get_param(%s)" % name)
        return v.value

    def get_counter(self, name):
        v = C.c_int64()
        self._ck(self.api.get_counter(self._h, name.encode(), C.byref(v)), "get_counter(%s)" % name)
        return v.value

    # -- sync / timing ----------------------------------------------------------
    # -- strips over RCCL, inside the library (include/vof2d.h "strips over RCCL") ------
    def comm_init(self, uid, rank, world, loopback=False):
        buf = C.create_string_buffer(bytes(uid), _abi.VOF_COMM_ID_BYTES)
        self._ck(self.api.comm_init(self._h, buf, int(rank), int(world),
                                    _abi.VOF_COMM_LOOPBACK if loopback else 0), "comm_init")

    def comm_exchange(self, mask):
        self._ck(self.api.comm_exchange(self._h, int(mask)), "comm_exchange")

    def step_exchange(self, nsteps=1, overlap=1):
        """overlap: 0 = one exchange after the step, 1 = per field as soon as final, 3 = p, u, v in one
        group after the first sweep, 4 = fused transport on the edge bands first, one group for all
        four fields under the transport of the other rows, 5 = the pair kernels of the single GPU (k_jacobi_pair, k_tm)
        with u*, v*, rhs, F, p exchanged once per step (include/vof2d.h)."""
        self._ck(self.api.step_exchange(self._h, int(nsteps), int(overlap)), "step_exchange")

    def step_tm_piece(self, piece):
        """The kernels of one piece of an overlap-mode-5 call without the exchange: 0 = the first step's k_momentum,
        1 = one middle step (k_jacobi_pair, k_tm), 2 = the last step (k_jacobi_tb x 2, k_transport)."""
        self._ck(self.api.step_tm_piece(self._h, int(piece)), "step_tm_piece")

    def comm_allreduce_max(self, value):
        v = C.c_double(float(value))
        self._ck(self.api.comm_allreduce_max(self._h, C.byref(v)), "comm_allreduce_max")
        return v.value

    def comm_info(self):
        """(RCCL version code, 1 if step_exchange replays captured graphs)."""
        ver, gr = C.c_int32(), C.c_int32()
        self._ck(self.api.comm_info(self._h, C.byref(ver), C.byref(gr)), "comm_info")
        return ver.value, gr.value

    def comm_destroy(self):
        self._ck(self.api.comm_destroy(self._h), "comm_destroy")

    def sync(self):
        self._ck(self.api.sync(self._h), "sync")

    def timer_start(self):
        self._ck(self.api.timer_start(self._h), "timer_start")

    def timer_stop(self):
        ms = C.c_float()
        self._ck(self.api.timer_stop(self._h, C.byref(ms)), "timer_stop")
        return ms.value

    def profile_steps(self, nsteps, reset=True):
        """In-situ per-kernel profile of nsteps fused steps: {kernel: (avg_us, launches)}."""
        if reset:
            self._ck(self.api.reset_profile(self._h), "reset_profile")
        self._ck(self.api.profile_steps(self._h, int(nsteps)), "profile_steps")
        out = {}
        for k in ("k_momentum", "k_set_bc", "k_jacobi", "k_jacobi_tb", "k_correct", "k_fct_x", "k_fct_y",
                  "k_transport", "k_normals", "k_kappa", "k_predictor", "k_rhs", "k_jacobi_pair", "k_tm", "k_tm_uv",
                  "k_cg_apply", "k_cg_update", "k_cg_residual", "k_cg_finish",
                  "k_mg_smooth", "k_mg_restrict", "k_mg_prolong", "k_mg_coarse_block"):
            us, n = C.c_double(), C.c_int64()
            if self.api.get_profile(self._h, k.encode(), C.byref(us), C.byref(n)) != 0:
                continue   # a kernel this build of the library does not have
            if n.value:
                out[k] = (us.value, n.value)
        return out

    def time_jacobi(self, n):
        ms = C.c_float()
        self._ck(self.api.time_jacobi(self._h, int(n), C.byref(ms)), "time_jacobi")
        return ms.value


def selftest_division(api, dtype, n, seed):
    """vof_selftest_division: (a, b, q) arrays with q = the kernels' exact division of a by b."""
    dt = np.float64 if dtype_code(dtype) == _abi.VOF_F64 else np.float32
    a, b, q = (np.empty(n, dt) for _ in range(3))
    rc = api.selftest_division(dtype_code(dtype), n, seed, a.ctypes.data, b.ctypes.data, q.ctypes.data)
    if rc != 0:
        raise VofError("vof_selftest_division failed: %s" % _abi.ERRNAMES.get(rc, rc))
    return a, b, q


def comm_unique_id(api):
    """vof_comm_get_unique_id: the VOF_COMM_ID_BYTES one rank creates and every rank passes to comm_init."""
    buf = C.create_string_buffer(_abi.VOF_COMM_ID_BYTES)
    rc = api.comm_get_unique_id(buf)
    if rc != 0:
        raise VofError("vof_comm_get_unique_id failed: %s (is librccl.so.1 loadable?)" % _abi.ERRNAMES.get(rc, rc))
    return buf.raw

