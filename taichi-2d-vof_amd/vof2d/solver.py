"""VOF2D -- the reference's program interface, object-shaped.

2dvof.py exposes module-global ``ti.field`` objects (``F.to_numpy()``,
``x.from_numpy()``; :44,:46,:535,:565), a 0-D field ``sigma[None]`` (:28-29)
and zero-argument kernels (``set_BC()``, ``advect_upwind()`` ...; :498,:513-528).
VOF2D keeps those names and meanings; each call is one C-ABI call into the HIP
library.  ``step(n)`` runs the solver part of the main loop (:506-528) with
the fused kernel schedule.
"""
import numpy as np

from . import _abi
from ._lib import hip_api
from .engine import Engine, make_desc

FIELD_NAMES = ("F", "u", "v", "p", "u_star", "v_star", "mx", "my", "kappa", "rho", "nu", "rhs")


class Field:
    """Stand-in for a ``ti.field`` of shape (nx+2, ny+2): to_numpy / from_numpy / [i, j]."""

    def __init__(self, eng, name):
        self._eng, self.name = eng, name
        self.shape = (eng.nrows, eng.ny + 2)
        self.dtype = eng.np_dtype

    def to_numpy(self):
        return self._eng.get(self.name)

    def from_numpy(self, arr):
        self._eng.set(self.name, arr)

    def __getitem__(self, idx):
        i, j = idx
        return self._eng.get(self.name, rows=(int(i), int(i)))[0, int(j)]


class _Sigma:
    """sigma[None] of 2dvof.py:28-29."""

    def __init__(self, eng):
        self._eng = eng

    def __getitem__(self, key):
        return self._eng.get_param("sigma")

    def __setitem__(self, key, value):
        self._eng.set_param("sigma", float(value))


class VOF2D:
    def __init__(self, nx=200, ny=200, dtype="f32", coord_cast="f32", jacobi_iters=10, device=-1,
                 use_graph=True, stream=None, api=None, **consts):
        """Defaults are the reference's shipped problem (2dvof.py:9,19-20): 200x200, f32."""
        self.api = api if api is not None else hip_api()
        flags = 0 if use_graph else _abi.VOF_FLAG_NO_GRAPH
        self.desc = make_desc(self.api, nx, ny, dtype, coord_cast, jacobi_iters=jacobi_iters, device=device,
                              flags=flags, **consts)
        self.eng = Engine(self.api, self.desc, stream=stream)
        self.nx, self.ny = nx, ny
        self.imin, self.jmin, self.imax, self.jmax = 1, 1, nx, ny  # :37-40
        for name in FIELD_NAMES:
            setattr(self, name, Field(self.eng, name))
        self.sigma = _Sigma(self.eng)
        self.dt = self.eng.get_param("dt")
        self.dx, self.dy = self.eng.get_param("dx"), self.eng.get_param("dy")
        self.dxi, self.dyi = self.eng.get_param("dxi"), self.eng.get_param("dyi")

    # reference verbs ------------------------------------------------------
    def set_init_F(self, ic):
        self.eng.set_init_F(ic)

    def set_scene(self, shapes, samples=8, clear=True):
        """An initial state painted from shapes on the device (vof_set_scene; the shapes: vof2d/scene.py); the summary as a dict."""
        return self.eng.set_scene(shapes, samples, clear)

    def set_BC(self):
        self.eng.set_BC()

    def cal_nu_rho(self):
        self.eng.cal_nu_rho()

    def get_normal_young(self):
        self.eng.get_normal_young()

    def advect_upwind(self):
        self.eng.advect_upwind()

    def solve_p_jacobi(self, n=1):
        self.eng.solve_p_jacobi(n)

    def solve_p_cg(self, tol, max_iters, check_every=10, criterion="abs", build_rhs=True):
        return self.eng.solve_p_cg(tol, max_iters, check_every, criterion, build_rhs)

    def solve_p_mg(self, tol, max_cycles, check_every=1, criterion="abs", build_rhs=True):
        return self.eng.solve_p_mg(tol, max_cycles, check_every, criterion, build_rhs)

    def update_uv(self):
        self.eng.update_uv()

    def fct_x_sweep(self):
        self.eng.fct_x_sweep()

    def fct_y_sweep(self):
        self.eng.fct_y_sweep()

    def solve_VOF_rudman(self, istep=None):
        self.eng.solve_VOF_rudman(self.istep if istep is None else istep)

    def post_process_f(self):
        self.eng.post_process_f()

    # display fields (2dvof.py:458-492) -------------------------------------------
    def get_vof_field(self):
        return self.eng.vis_field("vof")

    def get_u_field(self):
        return self.eng.vis_field("u")

    def get_v_field(self):
        return self.eng.vis_field("v")

    def get_vnorm_field(self):
        return self.eng.vis_field("vnorm")

    def interp_velocity(self):
        return self.eng.interp_velocity()

    # main loop --------------------------------------------------------------
    def step(self, nsteps=1):
        self.eng.step(nsteps)

    def step_mg(self, nsteps, cycles, criterion="rel"):
        """nsteps steps with `cycles` multigrid V-cycles each instead of the sweeps (vof_step_mg):
        (last residual, worst residual, its step)."""
        return self.eng.step_mg(nsteps, cycles, criterion)

    def diagnostics(self):
        """The raw row of vof_diagnostics as a dict (vof2d/diag.py: NAMES, derive)."""
        return self.eng.diagnostics()

    def interface(self, eps=1e-6):
        """The interface as PLIC segments, extracted on the device (vof_interface): (rows, summary), vof2d/interface.py."""
        return self.eng.interface(eps)

    def curvature(self, eps=1e-6):
        """Height-function curvature of every mixed cell beside the solver's own, on the device (vof_curvature): (rows, summary), vof2d/curvature.py."""
        return self.eng.curvature(eps)

    def energy(self):
        """The raw row of vof_energy as a dict (vof2d/energy.py: NAMES, derive, rates)."""
        return self.eng.energy()

    def blobs(self, phase="liquid", threshold=0.5, labels=False):
        """Droplets or bubbles labelled and measured on the device (vof_blobs): (rows, summary[, labels]), vof2d/blobs.py."""
        return self.eng.blobs(phase, threshold, labels)

    def tracers_set(self, xy):
        """Give the handle a set of passive tracers at the (n, 2) physical positions xy (vof_tracers_set; vof2d/tracers.py: lattice, seed)."""
        self.eng.tracers_set(xy)

    def tracers_advance(self, time):
        """Move every tracer by `time` with the current u, v (vof_tracers_advance)."""
        self.eng.tracers_advance(time)

    def tracers(self, rows=True):
        """The tracers' rows X, Y, U, V, F and the summary (vof_tracers_get): (rows, summary), vof2d/tracers.py."""
        return self.eng.tracers(rows)

    def step_tracers(self, nsteps, every=1, mg_cycles=0, criterion="rel", snap_every=0):
        """nsteps steps with the tracers advanced every `every` of them and snapshots recorded on the device (vof_step_tracers)."""
        return self.eng.step_tracers(nsteps, every, mg_cycles, criterion, snap_every)

    def depths(self):
        """Both marginals of F, the top of the liquid per row and the front on the floor from one pass on the device (vof_depths):
        (depth_i, depth_j, top, summary), vof2d/gauges.py."""
        return self.eng.depths()

    def gauges_set(self, xy):
        """Give the handle fixed sensors at the (n, 2) physical positions xy (vof_gauges_set)."""
        self.eng.gauges_set(xy)

    def gauges_get(self, rows=True):
        """What the gauges read now: rows X, Y, U, V, F, P, DEPTH, TOP and the summary (vof_gauges_get): (rows, summary), vof2d/gauges.py."""
        return self.eng.gauges_get(rows)

    def step_gauges(self, nsteps, every=1, mg_cycles=0, criterion="rel"):
        """nsteps steps with a record of every gauge taken on the device every `every` steps (vof_step_gauges)."""
        return self.eng.step_gauges(nsteps, every, mg_cycles, criterion)

    def dye_set(self, arr):
        """Give the handle a dye: an (nx+2, ny+2) marker field carried by the transport of F (vof_dye_set; None releases it; vof2d/dye.py: box)."""
        self.eng.dye_set(arr)

    def dye_get(self):
        """The dye as an (nx+2, ny+2) array (vof_dye_get)."""
        return self.eng.dye_get()

    def dye_advance(self):
        """One transport of the dye with the current u, v and the step parity of istep (vof_dye_advance)."""
        self.eng.dye_advance()

    def dye_stats(self):
        """The raw row of vof_dye_stats as a dict (vof2d/dye.py: NAMES, derive)."""
        return self.eng.dye_stats()

    def step_dye(self, nsteps, every=0, mg_cycles=0, criterion="rel"):
        """nsteps steps, the dye moved behind each, a row of its statistics recorded on the device every `every` steps (vof_step_dye)."""
        return self.eng.step_dye(nsteps, every, mg_cycles, criterion)

    def set_frame_lut(self, table=None):
        """Give the handle a colour table for its frames: (258, 3) uint8, vof2d/frames.py: lut (vof_frame_set_lut; None: the grey ramp)."""
        self.eng.set_frame_lut(table)

    def frame(self, quantity="F", bx=1, by=None, lo=0.0, hi=0.0, contour=False, symmetric=False, rgb=True, means=False):
        """A picture of F, U, V, SPEED, P, VORT or DYE rendered on the device, bx x by cells per pixel (vof_frame): (rgb, means, summary),
        vof2d/frames.py."""
        return self.eng.frame(quantity, bx, by, lo, hi, contour, symmetric, rgb, means)

    def step_frames(self, nsteps, every, quantity="F", bx=1, by=None, lo=0.0, hi=0.0, contour=False, symmetric=False, mg_cycles=0, criterion="rel"):
        """nsteps steps with such a picture rendered on the device every `every` steps (vof_step_frames): (pictures, summaries)."""
        return self.eng.step_frames(nsteps, every, quantity, bx, by, lo, hi, contour, symmetric, mg_cycles, criterion)

    def stats_begin(self, mask=3, level=0.5):
        """Start (or clear) per-cell statistics over the run: running sums of F, u, v and their products, envelopes, wet time and
        arrival step (vof_stats_begin; mask 0 releases them; vof2d/stats.py: PLANES, derive)."""
        self.eng.stats_begin(mask, level)

    def stats_sample(self):
        """One sample of the current state into the statistics (vof_stats_sample)."""
        self.eng.stats_sample()

    def stats_plane(self, slot):
        """One accumulator plane as an (nx, ny) float64 array (vof_stats_get)."""
        return self.eng.stats_plane(slot)

    def stats_summary(self):
        """The summary of the statistics as a dict (vof_stats_summary; vof2d/stats.py: SUMMARY)."""
        return self.eng.stats_summary()

    def step_stats(self, nsteps, every, mg_cycles=0, criterion="rel"):
        """nsteps steps with a sample taken on the device every `every` steps (vof_step_stats): the samples taken."""
        return self.eng.step_stats(nsteps, every, mg_cycles, criterion)

    def step_diag(self, nsteps, every, mg_cycles=0, criterion="rel"):
        """nsteps steps with a row of diagnostics recorded on the device every `every` steps (vof_step_diag)."""
        return self.eng.step_diag(nsteps, every, mg_cycles, criterion)

    def step_energy(self, nsteps, every, mg_cycles=0, criterion="rel"):
        """nsteps steps with a row of the energy budget recorded on the device every `every` steps (vof_step_energy)."""
        return self.eng.step_energy(nsteps, every, mg_cycles, criterion)

    @property
    def istep(self):
        return self.eng.istep

    @istep.setter
    def istep(self, v):
        self.eng.istep = v

    def regrid(self, nx, ny, dtype=None, plic=True, eps=1e-6, **consts):
        """A new VOF2D of nx x ny cells on the same device that carries this one's state (vof_regrid): finer or coarser by
        integer factors of at most regrid.MAX_FACTOR, or the same grid in the other dtype.  The constants are copied;
        `consts` overrides them (dt, the material constants; Lx and Ly must stay).  F of a mixed cell's children comes from
        the cell's PLIC line unless plic=False.  The summary of the call is left in `.regrid_summary` of the new solver."""
        from . import regrid
        from .engine import dtype_code
        regrid.factors(self.nx, self.ny, nx, ny)   # (ValueError in front of any allocation)
        d = self.desc
        kw = {k: getattr(d, k) for k in ("Lx", "Ly", "rho_l", "rho_g", "nu_l", "nu_g", "sigma", "gx", "gy", "dt")}
        kw["sigma"] = self.eng.get_param("sigma")
        kw.update(consts)
        new = VOF2D(nx, ny, dtype=d.dtype if dtype is None else dtype_code(dtype), coord_cast="f32" if d.coord_cast_f32 else "none",
                    jacobi_iters=d.jacobi_iters, device=d.device, use_graph=not (d.flags & _abi.VOF_FLAG_NO_GRAPH), api=self.api, **kw)
        new.regrid_summary = new.eng.regrid_from(self.eng, plic=plic, eps=eps)
        return new

    def step_verbs(self, nsteps=1):
        """The main loop of 2dvof.py:506-528 written verb by verb (literal schedule)."""
        for _ in range(nsteps):
            self.istep = self.istep + 1
            self.cal_nu_rho()
            self.get_normal_young()
            self.advect_upwind()
            self.set_BC()
            self.solve_p_jacobi(self.desc.jacobi_iters)
            self.update_uv()
            self.set_BC()
            self.solve_VOF_rudman(self.istep)
            self.post_process_f()
            self.set_BC()

    def sync(self):
        self.eng.sync()

    @property
    def courant_violations(self):
        return self.eng.get_counter("courant_violations")

    def state(self, names=("F", "u", "v", "p")):
        return {n: self.eng.get(n) for n in names}

    def close(self):
        self.eng.close()
