"""The command line of 2dvof.py on the HIP library: argument parsing and the main loop.

Same flags as /root/reference/2dvof.py:11-17 (`-ic {1,2,3}`, `-s`), same banner (:95-99), same
per-100-step status line (:533-557), same `output/NNNNNN-f.png` naming and plot (:563-571), same
`output/` and `data/` directories (:500-501).  The Taichi GUI is replaced by a headless loop.

`run(args, api=None, comm=None)` is the whole program for one rank; `2dvof.py` calls it with the
HIP library (the only engine the product has).  Tests hand it another object with the same C ABI
and a torch.distributed (gloo) carrier to exercise the multi-rank host logic without a GPU.
"""
import argparse
import os
import sys

import numpy as np

STATE = ("F", "u", "v", "p")


def build_parser():
    parser = argparse.ArgumentParser(
        description="2-D VOF solver (drop-in command line of taichi-2d-vof's 2dvof.py on MI355X)")
    # 1 - Dam Break; 2 - Rising Bubble; 3 - Droping liquid          (2dvof.py:12-14)
    parser.add_argument('-ic', type=int, choices=[1, 2, 3], default=1)
    parser.add_argument('-s', action='store_true')
    ext = parser.add_argument_group("extensions (the reference hard-codes these at :9, :19-20, :521 and loops until 'q')")
    ext.add_argument('--nx', type=int, default=200)
    ext.add_argument('--ny', type=int, default=200)
    ext.add_argument('--dtype', choices=['f32', 'f64'], default='f32', help='field precision (default f32 = ti.f32, :9)')
    ext.add_argument('--coord-cast', choices=['f32', 'none'], default='f32',
                     help='keep / drop the .astype(np.float32) of the mesh coordinates (:43, :45)')
    ext.add_argument('--steps', type=int, default=0, help='stop after N steps (default 0: run until Ctrl-C, like the reference)')
    ext.add_argument('--dt', type=float, default=None, help='time step (default 4e-6, :33)')
    ext.add_argument('--jacobi-iters', type=int, default=10, help='pressure sweeps per step (reference: 10, :521)')
    ext.add_argument('--gpus', type=int, default=1,
                     help='row strips over N GPUs of this node, one process per GPU, halo exchange over RCCL '
                          '(started by this command itself, or by torch.distributed.run)')
    ext.add_argument('--verbs', action='store_true',
                     help='call the kernels one by one exactly as the main loop :513-528 does, instead of the fused '
                          'vof_step() schedule (same results, more HBM traffic; one GPU)')
    ext.add_argument('--jacobi-tol', type=float, default=0.0,
                     help='residual-terminated pressure solve instead of the fixed sweep count, capped by --jacobi-max '
                          '(with --gpus N the two norms are all-reduced over the strips)')
    ext.add_argument('--jacobi-max', type=int, default=2000)
    ext.add_argument('--jacobi-crit', choices=['abs', 'rel'], default='abs',
                     help='abs: max|p_new-p| <= tol (default); rel: max|p_new-p| / max|p_new| <= tol (vof_solve_p)')
    ext.add_argument('--pressure-solver', choices=['jacobi', 'cg', 'mg'], default='jacobi',
                     help='what --jacobi-tol runs: Jacobi sweeps (default, vof_solve_p), conjugate gradients (cg, vof_solve_p_cg) '
                          'or geometric multigrid (mg, vof_solve_p_mg) on the same equation; --jacobi-max caps the iterations '
                          '(cg) or V-cycles (mg), --jacobi-crit as for the sweeps; one GPU')
    ext.add_argument('--mg-cycles', type=int, default=0, metavar='K',
                     help='with --pressure-solver mg and without --jacobi-tol: every step runs K V-cycles (K >= 1), warm-started '
                          'from the previous p, inside the fused step (vof_step_mg); --jacobi-crit is the criterion of the '
                          'residual the status line reports; one GPU')
    ext.add_argument('--mg-coarse', choices=['block', 'launches'], default='block',
                     help='with --mg-cycles: the coarsest-level solve of a cycle as one workgroup (block, default; where that '
                          'level is small enough) or as the launches of vof_solve_p_mg')
    ext.add_argument('--device', type=int, default=0, help='HIP device ordinal (one GPU; with --gpus N rank r takes device r)')
    ext.add_argument('--vis', type=int, choices=[0, 1, 2, 3, 4], default=0,
                     help='what the reference GUI would display (SPACE cycles it there, :508-509): 0 VOF, 1 u, 2 v, '
                          '3 |velocity|, 4 velocity vectors; saved as output/NNNNNN-vis.png with -s (one GPU)')
    ext.add_argument('--save-every', type=int, default=0, metavar='N',
                     help='write data/NNNNNNNN.npz (F, u, v, p with ghost cells, istep) every N steps: the use the '
                          "reference's data/ directory (:501) was made for")
    ext.add_argument('--diag-every', type=int, default=None, metavar='N',
                     help='every N steps append a row to data/diagnostics.csv: liquid volume, centroid, kinetic energy, max and '
                          'rms divergence of u, v, max |u|, max |v|, CFL number, min and max F, reduced on the device '
                          '(vof_step_diag; with --jacobi-tol, --verbs or --gpus N vof_diagnostics at the multiples of N); the '
                          'status line then reports volume, div_max and cfl')
    ext.add_argument('--interface-every', type=int, default=None, metavar='N',
                     help='every N steps write data/interface_NNNNNN.npy -- the interface as one PLIC segment per mixed cell, '
                          'rows of i, j, x0, y0, x1, y1, nx, ny extracted on the device (vof_interface) -- and append istep, '
                          'segments, degenerate, length to data/interface.csv; with -s the VOF frame draws the segments')
    ext.add_argument('--blobs-every', type=int, default=None, metavar='N',
                     help='every N steps append one line per blob to data/blobs.csv -- istep, blob, cells, volume, xc, yc, uc, vc, '
                          'imin, imax, jmin, jmax of every connected piece of the phase, labelled and measured on the device (vof_blobs)')
    ext.add_argument('--blobs-phase', choices=('liquid', 'gas'), default='liquid',
                     help='the phase whose pieces --blobs-every lists: liquid (F >= T, droplets) or gas (F < T, bubbles)')
    ext.add_argument('--blobs-threshold', type=float, default=0.5, metavar='T', help='the F that separates the phases for --blobs-every, in (0, 1)')
    ext.add_argument('--tracers', type=int, default=0, metavar='N',
                     help='about N passive tracer particles on a regular lattice, moved with the flow on the device (vof_step_tracers); one GPU')
    ext.add_argument('--tracers-phase', choices=('liquid', 'gas', 'all'), default='liquid',
                     help='which lattice points become tracers: those that start in the liquid (F >= 0.5, default), in the gas, or all')
    ext.add_argument('--tracers-every', type=int, default=1, metavar='K',
                     help='advance the tracers by K dt every K steps (default 1: every step)')
    ext.add_argument('--tracers-save-every', type=int, default=None, metavar='M',
                     help='every M steps write data/tracers_NNNNNN.npy -- rows of x, y, u, v, F per tracer, in the order they were seeded '
                          '(vof_tracers_get) -- and append istep, time, count, lost, in_liquid to data/tracers.csv')
    ext.add_argument('--gauge', action='append', default=[], metavar='X,Y',
                     help='a fixed sensor at the physical position X,Y inside the closed domain (repeatable): u, v, F, p sampled there, the '
                          'liquid depth over the floor and the top of the liquid at X, read on the device (vof_gauges_*); one GPU')
    ext.add_argument('--gauges-file', default=None, metavar='FILE', help='more gauges, one `x y` per line (# starts a comment)')
    ext.add_argument('--gauges-every', type=int, default=None, metavar='N',
                     help='every N steps append one line per gauge to data/gauges.csv: istep, gauge, x, y, u, v, f, p, depth, top '
                          '(vof_step_gauges; with --jacobi-tol, --verbs, --mg-cycles, --diag-every or --tracers vof_gauges_get at the multiples of N)')
    ext.add_argument('--depths-every', type=int, default=None, metavar='N',
                     help='every N steps write data/depths_NNNNNN.npy -- rows of x_i, liquid depth over the floor in metres, top j of the '
                          'liquid per grid row, from one pass over F on the device (vof_depths) -- and append istep, front_lo, front_hi, '
                          'top, volume to data/depths.csv; works with --gpus N')
    ext.add_argument('--dye-box', action='append', default=[], metavar='X0,X1,Y0,Y1',
                     help='a dye: a marker field equal to F inside the physical box [X0, X1] x [Y0, Y1] (decided at the cell centres; repeatable, '
                          'the boxes are joined) and 0 elsewhere, carried by the transport of F behind every step on the device (vof_step_dye); one GPU')
    ext.add_argument('--dye-file', default=None, metavar='FILE.npy', help='the dye as an (nx+2, ny+2) array, ghost cells included, instead of boxes')
    ext.add_argument('--dye-every', type=int, default=None, metavar='N',
                     help='every N steps append a row to data/dye.csv: amount, centroid, mean, variance, share outside the liquid, the '
                          "dye's velocity, min and max of the dye and max(C - F), reduced on the device")
    ext.add_argument('--dye-save-every', type=int, default=None, metavar='M', help='every M steps write the dye to data/dye_NNNNNN.npy')
    ext.add_argument('--frames-every', type=int, default=None, metavar='N',
                     help='every N steps write output/frame_NNNNNN.png (named by istep) -- a picture rendered on the device: box averages, a '
                          'colour table, 8-bit RGB, three bytes a pixel copied out (vof_frame) -- and append istep, time, lo, hi, nan_pixels '
                          'to data/frames.csv; needs no matplotlib with --frame-cmap grey; one GPU')
    ext.add_argument('--frame', default='F:0:1', metavar='QUANTITY[:LO:HI]',
                     help='what a frame shows: F, U, V, SPEED, P, VORT or DYE, over the fixed range LO..HI; without a range the range of each '
                          'picture, symmetric about zero for U, V and VORT (default F:0:1)')
    ext.add_argument('--frame-block', type=int, default=None, metavar='K',
                     help='K x K cells per pixel (default: the smallest K that keeps the longer side within 1024 pixels)')
    ext.add_argument('--frame-cmap', default=None, metavar='NAME',
                     help="the colour map, one of matplotlib's or `grey` (default Blues for F and DYE, coolwarm for U, V, VORT, plasma for SPEED, P)")
    ext.add_argument('--frame-contour', action='store_true', help='mark the interface (the 0.5 level of the box-averaged F) on the frames')
    ext.add_argument('--stats-every', type=int, default=None, metavar='N',
                     help='every N steps take one sample of per-cell statistics on the device (vof_stats_sample): running sums of F, u, v and '
                          'their products, the envelopes of F and of the speed, the wet time and the step the front first arrived; works beside '
                          '--diag-every, --dye-*, --frames-every, --gauges-every, --tracers and --mg-cycles; one GPU.  With --resume the '
                          'statistics start anew: the planes are not part of a checkpoint')
    ext.add_argument('--stats', default='MOMENTS,ENVELOPE', metavar='GROUPS',
                     help='the groups --stats-every keeps, comma-separated: MOMENTS (means, variances, Reynolds stress, liquid-phase velocity), '
                          'ENVELOPE (max F, max speed, wet fraction, arrival time); default both')
    ext.add_argument('--stats-level', type=float, default=0.5, metavar='L', help='a cell counts as wet in a sample if its clamped F is >= L, in (0, 1] (default 0.5)')
    ext.add_argument('--stats-from', type=int, default=0, metavar='STEP', help='no sample before that step (to skip a spin-up)')
    ext.add_argument('--stats-save-every', type=int, default=None, metavar='M',
                     help='every M steps, and at the end of the run, write data/stats_NNNNNN.npz -- the raw planes, the sample count N and the '
                          'derived arrays -- and append a line of the summary to data/stats.csv (default: at the end of the run only)')
    ext.add_argument('--resume', default=None, metavar='FILE', help='continue from a file written by --save-every')
    return parser


def parse_frame(text):
    """(quantity, lo, hi) of a --frame value QUANTITY[:LO:HI]; lo == hi == 0.0 without a range.  ValueError with the reason."""
    from . import frames
    parts = text.split(':')
    name = parts[0].upper()
    if name not in frames.QUANTITIES:
        raise ValueError("--frame: %r is not one of %s" % (parts[0], ', '.join(frames.QUANTITIES)))
    if len(parts) == 1:
        return name, 0.0, 0.0
    if len(parts) != 3:
        raise ValueError("--frame needs QUANTITY or QUANTITY:LO:HI, not %r" % text)
    try:
        lo, hi = float(parts[1]), float(parts[2])
    except ValueError:
        raise ValueError("--frame %s: LO and HI must be numbers" % text)
    if not (lo < hi and abs(lo) != float('inf') and abs(hi) != float('inf')):
        raise ValueError("--frame %s: needs finite LO < HI" % text)
    return name, lo, hi


def dye_conflicts(args):
    """The options a dye cannot be combined with, each with the reason ('' where there is none): its steps are those of
    vof_step_dye, one call that steps and moves the dye on the device."""
    dye = bool(args.dye_box or args.dye_file or args.dye_every is not None or args.dye_save_every is not None)
    if not dye:
        return ''
    for on, name, why in ((args.gpus > 1, "--gpus N", "the dye's sweeps on a strip would need their own halo exchanges"),
                          (args.verbs, "--verbs", "the verb-by-verb loop has no place for the dye's transport"),
                          (args.jacobi_tol > 0.0, "--jacobi-tol", "the residual-terminated loop runs verb by verb"),
                          (args.diag_every is not None, "--diag-every", "vof_step_diag and vof_step_dye are two stepping loops"),
                          (bool(args.tracers), "--tracers", "vof_step_tracers and vof_step_dye are two stepping loops"),
                          (args.gauges_every is not None, "--gauges-every", "vof_step_gauges and vof_step_dye are two stepping loops")):
        if on:
            return "the dye options (--dye-box, --dye-file, --dye-every, --dye-save-every) cannot be combined with %s: %s" % (name, why)
    return ''


def parse_dye_boxes(specs):
    """[(x0, x1, y0, y1)] of the --dye-box values."""
    out = []
    for spec in specs:
        try:
            x0, x1, y0, y1 = (float(t) for t in spec.split(','))
        except ValueError:
            raise SystemExit("--dye-box needs X0,X1,Y0,Y1 (four numbers), not %r" % spec)
        if not (x0 <= x1 and y0 <= y1):
            raise SystemExit("--dye-box %s: needs X0 <= X1 and Y0 <= Y1" % spec)
        out.append((x0, x1, y0, y1))
    return out


def parse_args(argv=None):
    """build_parser().parse_args plus the combinations argparse cannot express."""
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.diag_every is not None and args.diag_every < 1:
        parser.error("--diag-every needs N >= 1")
    if args.interface_every is not None and args.interface_every < 1:
        parser.error("--interface-every needs N >= 1")
    if args.blobs_every is not None and args.blobs_every < 1:
        parser.error("--blobs-every needs N >= 1")
    if not 0.0 < args.blobs_threshold < 1.0:
        parser.error("--blobs-threshold needs 0 < T < 1")
    if args.tracers < 0:
        parser.error("--tracers needs N >= 0")
    if args.tracers_every < 1:
        parser.error("--tracers-every needs K >= 1")
    if args.tracers_save_every is not None and args.tracers_save_every < 1:
        parser.error("--tracers-save-every needs M >= 1")
    if args.tracers_save_every is not None and not args.tracers:
        parser.error("--tracers-save-every writes the tracers of --tracers N: pass that too")
    if args.tracers and args.gpus > 1:
        parser.error("--tracers runs on one GPU (a tracer would leave a strip's rows): drop --gpus")
    if args.gauges_every is not None and args.gauges_every < 1:
        parser.error("--gauges-every needs N >= 1")
    if args.depths_every is not None and args.depths_every < 1:
        parser.error("--depths-every needs N >= 1")
    if (args.gauge or args.gauges_file or args.gauges_every is not None) and args.gpus > 1:
        parser.error("--gauge, --gauges-file and --gauges-every run on one GPU (a gauge reads rows a strip may not hold): drop --gpus, "
                     "or use --depths-every, which works on strips")
    if args.gauges_every is not None and not (args.gauge or args.gauges_file or args.resume):
        parser.error("--gauges-every records the gauges of --gauge X,Y / --gauges-file FILE: pass at least one")
    if args.dye_every is not None and args.dye_every < 1:
        parser.error("--dye-every needs N >= 1")
    if args.dye_save_every is not None and args.dye_save_every < 1:
        parser.error("--dye-save-every needs M >= 1")
    if args.dye_box and args.dye_file:
        parser.error("--dye-box and --dye-file both give the dye: pass one of them")
    if (args.dye_every is not None or args.dye_save_every is not None) and not (args.dye_box or args.dye_file or args.resume):
        parser.error("--dye-every and --dye-save-every report the dye of --dye-box X0,X1,Y0,Y1 / --dye-file FILE.npy: pass one")
    if dye_conflicts(args):
        parser.error(dye_conflicts(args))
    if args.frames_every is not None:
        if args.frames_every < 1:
            parser.error("--frames-every needs N >= 1")
        if args.gpus > 1:
            parser.error("--frames-every runs on one GPU (frames over row strips are not built): drop --gpus")
        if args.frame_block is not None and args.frame_block < 1:
            parser.error("--frame-block needs K >= 1")
        try:
            name = parse_frame(args.frame)[0]
        except ValueError as e:
            parser.error(str(e))
        if name == "DYE" and not (args.dye_box or args.dye_file or args.resume):
            parser.error("--frame DYE shows the dye of --dye-box X0,X1,Y0,Y1 / --dye-file FILE.npy: pass one")
    if args.stats_every is not None:
        from . import stats as stats_mod
        if args.stats_every < 1:
            parser.error("--stats-every needs N >= 1")
        if args.gpus > 1:
            parser.error("--stats-every runs on one GPU (statistics over row strips are not built): drop --gpus")
        if args.stats_save_every is not None and args.stats_save_every < 1:
            parser.error("--stats-save-every needs M >= 1")
        if not 0.0 < args.stats_level <= 1.0:
            parser.error("--stats-level needs 0 < L <= 1")
        if args.stats_from < 0:
            parser.error("--stats-from needs STEP >= 0")
        try:
            if not stats_mod.mask_of(args.stats):
                raise ValueError("--stats names no group")
        except ValueError as e:
            parser.error("--stats: %s" % e)
    elif args.stats_save_every is not None:
        parser.error("--stats-save-every writes the statistics of --stats-every N: pass that too")
    if args.mg_cycles != 0:
        if args.mg_cycles < 1:
            parser.error("--mg-cycles needs K >= 1")
        if args.pressure_solver != "mg":
            parser.error("--mg-cycles counts the V-cycles of --pressure-solver mg: pass that solver, not %s" % args.pressure_solver)
        if args.jacobi_tol > 0.0:
            parser.error("--mg-cycles fixes the work of a step, --jacobi-tol ends it on a residual: pass one of them")
        if args.gpus > 1:
            parser.error("--mg-cycles runs on one GPU (the levels and sums of a strip would span its neighbours): drop --gpus")
        return args
    if args.pressure_solver in ("cg", "mg"):
        if not args.jacobi_tol > 0.0:
            parser.error("--pressure-solver %s needs a tolerance: pass --jacobi-tol T (> 0)" % args.pressure_solver)
        if args.gpus > 1:
            parser.error("--pressure-solver %s runs on one GPU (its sums are not reduced over strips): drop --gpus" % args.pressure_solver)
    return args


def numerics_of(args, dt):
    """What, besides the fields, decides how a run continues: a checkpoint resumed with other values of these is
    a different run, not a continuation."""
    num = {"dt": float(dt), "jacobi_iters": int(args.jacobi_iters), "coord_cast": str(args.coord_cast),
           "jacobi_tol": float(args.jacobi_tol), "jacobi_max": int(args.jacobi_max) if args.jacobi_tol > 0.0 else 0,
           "jacobi_crit": str(args.jacobi_crit) if args.jacobi_tol > 0.0 else ""}
    if getattr(args, "pressure_solver", "jacobi") in ("cg", "mg"):   # (only then: checkpoints of sweep runs resume as before)
        num["pressure_solver"] = str(args.pressure_solver)
    if getattr(args, "mg_cycles", 0) > 0:   # (only then, as above)
        num["mg_cycles"] = int(args.mg_cycles)
        num["mg_coarse"] = str(args.mg_coarse)
    return num


def save_state(path, fields, istep, nx, ny, dtype, ic, courant=0, numerics=None):
    tmp = path + ".tmp.npz"
    extra = {"num_" + k: np.array(v) for k, v in (numerics or {}).items()}
    np.savez(tmp, istep=np.int64(istep), nx=np.int64(nx), ny=np.int64(ny), dtype=np.array(dtype), ic=np.int64(ic),
             courant_violations=np.int64(courant), **extra, **fields)
    os.replace(tmp, path)


def load_state(path, nx, ny, dtype, numerics=None):
    """(fields, istep, courant_violations).  Refuses a file of another grid / precision, and one written with other
    numerics (dt, sweep count, coordinate cast, residual criterion) than this run's: the tests promise an exact
    continuation.  Files from before the numerics were recorded are accepted as they are."""
    z = np.load(path, allow_pickle=False)
    if (int(z["nx"]), int(z["ny"]), str(z["dtype"])) != (nx, ny, dtype):
        raise SystemExit("--resume: %s holds a %dx%d %s run, this one is %dx%d %s" %
                         (path, int(z["nx"]), int(z["ny"]), str(z["dtype"]), nx, ny, dtype))
    for k, v in (numerics or {}).items():
        key = "num_" + k
        if key in z.files and z[key].item() != v:
            raise SystemExit("--resume: %s was written with %s = %r, this run has %r (pass the same value to continue it)" %
                             (path, k.replace("_", "-"), z[key].item(), v))
    if numerics is not None and any(k.startswith("num_") for k in z.files):
        # (recorded only by conjugate-gradient and multigrid runs, so that files of sweep runs look as they always did)
        have = str(z["num_pressure_solver"]) if "num_pressure_solver" in z.files else "jacobi"
        want = numerics.get("pressure_solver", "jacobi")
        if have != want:
            raise SystemExit("--resume: %s was written with pressure-solver = %r, this run has %r (pass the same value to continue it)" %
                             (path, have, want))
        # (... and only by runs with a fixed cycle count)
        for k, none in (("mg_cycles", 0), ("mg_coarse", "")):
            have = z["num_" + k].item() if "num_" + k in z.files else none
            want = numerics.get(k, none)
            if have != want:
                raise SystemExit("--resume: %s was written with %s = %r, this run has %r (pass the same value to continue it)" %
                                 (path, k.replace("_", "-"), have, want))
    return {f: z[f] for f in STATE}, int(z["istep"]), int(z["courant_violations"]) if "courant_violations" in z.files else 0


class _Single:
    """One GPU: the VOF2D mirror of the reference's fields and kernels."""

    def __init__(self, args, api):
        from .solver import VOF2D
        consts = {} if args.dt is None else {"dt": args.dt}
        self.sim = VOF2D(args.nx, args.ny, dtype=args.dtype, coord_cast=args.coord_cast, device=args.device,
                         jacobi_iters=args.jacobi_iters, api=api, **consts)
        self.eng, self.rank, self.args = self.sim.eng, 0, args
        self.base_courant = 0
        self.mg_worst = (0.0, 0)                     # worst residual of --mg-cycles steps since the last report, its step
        self.diag_every = getattr(args, "diag_every", None) or 0
        # the fused steps record their rows on the device (vof_step_diag); the Python loops ask at the multiples of N
        self.diag_in_advance = bool(self.diag_every) and not (args.jacobi_tol > 0.0 or args.verbs)
        self.diag_rows = []
        if getattr(args, "mg_cycles", 0) > 0 and args.mg_coarse == "block":
            self.eng.set_param("mg_coarse_block", 1)
        # --tracers: advanced by K dt every K steps; `tr_pending` steps have been taken since the last advance (a stop of the
        # main loop may fall between two); TIME and the lost tracers of the run a checkpoint came from are carried beside the handle's
        self.tr_every = args.tracers_every if getattr(args, "tracers", 0) else 0
        self.tr_pending = 0
        self.tr_time0 = 0.0
        self.tr_lost0 = 0
        # --gauges-every: the plain fused steps take their records on the device (vof_step_gauges); every other loop is cut at
        # the multiples of N and asks there (vof_gauges_get)
        self.gauges_every = getattr(args, "gauges_every", None) or 0
        self.gauges_in_advance = bool(self.gauges_every) and not (args.jacobi_tol > 0.0 or args.verbs or self.diag_in_advance
                                                                  or getattr(args, "mg_cycles", 0) > 0 or self.tr_every)
        self.gauge_recs = []                         # (istep, rows) not yet written
        # a dye (--dye-box / --dye-file): every step is a step of vof_step_dye, the rows of --dye-every recorded on the device
        self.dye_on = False
        self.dye_every = getattr(args, "dye_every", None) or 0
        self.dye_rows = []                           # raw rows not yet written

    def set_dye(self, C):
        self.eng.dye_set(C)
        self.dye_on = True

    def dye(self):
        return self.eng.dye_get()

    def take_dye(self):
        rows, self.dye_rows = self.dye_rows, []
        return rows

    def _advance_dye(self, n):
        """n steps of vof_step_dye with a row at every multiple of N: no rows up to the first multiple (a resumed run may start
        anywhere), then one call for the rest."""
        from . import dye
        N, K, crit = self.dye_every, getattr(self.args, "mg_cycles", 0), self.args.jacobi_crit
        head = min(n, -self.sim.istep % N) if N else n
        if head:
            self.sim.step_dye(head, 0, K, crit)
            if N and self.sim.istep % N == 0:
                self.dye_rows.append(self.eng.dye_stats())
        if n - head:
            self.dye_rows += [dye.raw_of(r) for r in self.sim.step_dye(n - head, N, K, crit)]

    def set_gauges(self, xy):
        self.eng.gauges_set(xy)

    def save_gauges(self, path, istep):
        rows, _ = self.eng.gauges_get()
        tmp = path + ".tmp.npz"
        np.savez(tmp, xy=rows[:, :2], istep=np.int64(istep))
        os.replace(tmp, path)

    def record_gauges(self):
        self.gauge_recs.append((self.sim.istep, self.eng.gauges_get()[0]))

    def take_gauges(self):
        recs, self.gauge_recs = self.gauge_recs, []
        return recs

    def depths(self):
        return self.eng.depths()

    def _advance_gauges(self, n):
        """n fused steps with a record at every multiple of N: plain steps up to the first multiple (a resumed run may start
        anywhere), then one vof_step_gauges for the rest."""
        N = self.gauges_every
        head = min(n, -self.sim.istep % N)
        if head:
            self.sim.step(head)
            if self.sim.istep % N == 0:
                self.record_gauges()
        if n - head:
            first = self.sim.istep
            recs = self.sim.step_gauges(n - head, N)
            self.gauge_recs += [(first + (r + 1) * N, rows) for r, rows in enumerate(recs)]

    def init(self, ic):
        self.sim.set_init_F(ic)

    def seed_tracers(self):
        from . import tracers
        return len(tracers.seed(self.eng, self.args.tracers, self.args.tracers_phase))

    def tracer_rows(self):
        """(rows, summary) with TIME and the counts continued over a resume."""
        rows, summ = self.eng.tracers()
        summ = dict(summ, TIME=self.tr_time0 + summ["TIME"], COUNT=summ["COUNT"] + self.tr_lost0, LOST=summ["LOST"] + self.tr_lost0)
        return rows, summ

    def save_tracers(self, path, istep):
        rows, summ = self.tracer_rows()
        tmp = path + ".tmp.npz"
        np.savez(tmp, xy=rows[:, :2], time=np.float64(summ["TIME"]), istep=np.int64(istep), pending=np.int64(self.tr_pending), lost=np.int64(summ["LOST"]))
        os.replace(tmp, path)

    def load_tracers(self, path, istep):
        """The tracers of a checkpoint, if `path` holds those of step `istep`: the positions that are not lost (a lost tracer stays
        counted), TIME, the steps owed to the next advance.  False: there is nothing to restore, seed anew."""
        if not os.path.exists(path):
            return False
        z = np.load(path, allow_pickle=False)
        if int(z["istep"]) != istep:
            return False
        xy = z["xy"]
        self.eng.tracers_set(xy[~np.isnan(xy[:, 0])])
        self.tr_time0, self.tr_lost0, self.tr_pending = float(z["time"]), int(z["lost"]), int(z["pending"]) % self.tr_every
        return True

    def load(self, fields, istep, courant=0):
        for f in STATE:
            self.eng.set(f, fields[f])
        self.eng.istep = istep
        self.base_courant = courant                  # (the device counter restarts at zero)

    def advance(self, n):
        """n steps; with --tracers the tracers are advanced by K dt behind every K-th step counted from where they were seeded,
        wherever the main loop stops in between."""
        K = self.tr_every
        if not K:
            return self._advance(n)
        a = self.args
        fused = not (a.jacobi_tol > 0.0 or self.diag_in_advance or getattr(a, "mg_cycles", 0) > 0 or a.verbs)
        dt = self.eng.get_param("dt")
        while n > 0:
            if self.tr_pending == 0 and n >= K and fused:
                m = n // K * K
                self.eng.step_tracers(m, K)          # (groups of K steps and an advance each, enqueued in one call)
            else:
                m = min(n, K - self.tr_pending)
                self._advance(m)
                self.tr_pending += m
                if self.tr_pending == K:
                    self.eng.tracers_advance(float(K) * dt)
                    self.tr_pending = 0
            n -= m

    def _advance(self, n):
        a, sim = self.args, self.sim
        if a.jacobi_tol > 0.0:
            for _ in range(n):   # main loop :513-528 with the residual-terminated solve (extension)
                sim.istep = sim.istep + 1
                sim.cal_nu_rho(); sim.get_normal_young(); sim.advect_upwind(); sim.set_BC()
                if a.pressure_solver == "cg":
                    sim.solve_p_cg(a.jacobi_tol, a.jacobi_max, 10, a.jacobi_crit)
                elif a.pressure_solver == "mg":
                    sim.solve_p_mg(a.jacobi_tol, a.jacobi_max, 1, a.jacobi_crit)
                else:
                    self.eng.solve_p(a.jacobi_tol, a.jacobi_max, 10, a.jacobi_crit)
                sim.update_uv(); sim.set_BC()
                sim.solve_VOF_rudman(sim.istep); sim.post_process_f(); sim.set_BC()
        elif self.dye_on:
            self._advance_dye(n)
        elif self.diag_in_advance:
            self._advance_diag(n)
        elif self.gauges_in_advance:
            self._advance_gauges(n)
        elif getattr(a, "mg_cycles", 0) > 0:
            self._step_mg(n)
        elif a.verbs:
            sim.step_verbs(n)
        else:
            sim.step(n)

    def _step_mg(self, n):
        _, worst, at = self.sim.step_mg(n, self.args.mg_cycles, self.args.jacobi_crit)
        if not worst <= self.mg_worst[0]:
            self.mg_worst = (worst, at)

    def _advance_diag(self, n):
        """n fused steps with a row at every multiple of N: plain steps up to the first multiple (a resumed run may start
        anywhere), then one vof_step_diag for the rest."""
        from . import diag
        N, K = self.diag_every, getattr(self.args, "mg_cycles", 0)
        head = min(n, -self.sim.istep % N)
        if head:
            self._step_mg(head) if K > 0 else self.sim.step(head)
            if self.sim.istep % N == 0:
                self.diag_rows.append(self.eng.diagnostics())
        if n - head:
            # (with --mg-cycles the rows replace the residual record of vof_step_mg: the status line reports div_max)
            rows = self.sim.step_diag(n - head, N, K, self.args.jacobi_crit)
            self.diag_rows += [diag.raw_of(r) for r in rows]

    def record_diag(self):
        self.diag_rows.append(self.eng.diagnostics())

    def interface(self):
        return self.eng.interface()

    def blobs(self):
        return self.eng.blobs(self.args.blobs_phase, self.args.blobs_threshold)

    def take_diag(self):
        rows, self.diag_rows = self.diag_rows, []
        return rows

    def report(self):
        """What the status line adds for this run ('' for most), and a fresh start of whatever it accumulates."""
        if getattr(self.args, "mg_cycles", 0) <= 0 or self.diag_in_advance or self.dye_on:
            return ''
        worst, at = self.mg_worst
        self.mg_worst = (0.0, 0)
        return f' Worst {self.args.jacobi_crit} residual after {self.args.mg_cycles} V-cycles: {worst:8.2e} (step {at}).'

    def full(self, name):
        return self.eng.get(name)

    def courant(self):
        return self.base_courant + self.sim.courant_violations

    def close(self):
        self.sim.sync()
        self.sim.close()


class _Strips:
    """N GPUs: this rank's row strip (vof2d/strips.py); rank 0 gathers what it writes to disk."""

    def __init__(self, args, api, comm, rank, world):
        from .strips import StripSolver
        consts = {} if args.dt is None else {"dt": args.dt}
        self.s = StripSolver(args.nx, args.ny, args.dtype, ic=args.ic, coord_cast=args.coord_cast,
                             jacobi_iters=args.jacobi_iters, rank=rank, world=world, device=rank, api=api,
                             comm=comm, dist=getattr(comm, "dist", None), **consts)
        self.eng, self.rank, self.world, self.args = self.s.eng, rank, world, args
        self.base_courant = 0
        self.diag_every = getattr(args, "diag_every", None) or 0
        self.diag_in_advance = False
        self.diag_rows = []

    def init(self, ic):
        pass                                         # StripSolver ran set_init_F on its strip

    def load(self, fields, istep, courant=0):
        lo, hi = self.s.rows
        for f in STATE:
            self.eng.set(f, fields[f][lo:hi + 1])   # every rank reads the file: owned rows and halos alike
        self.eng.istep = istep
        self.base_courant = courant                  # (the device counters restart at zero)

    def advance(self, n):
        a = self.args
        if a.jacobi_tol <= 0.0:
            self.s.step(n)
            return
        e = self.eng
        for _ in range(n):   # main loop :513-528, verb by verb on the extended strip, with the residual-terminated solve
            e.istep = e.istep + 1
            e.cal_nu_rho(); e.get_normal_young(); e.advect_upwind(); e.set_BC()
            # (StripSolver.solve_p: the sweeps of a check in batches the deep halo of p covers, p exchanged after every
            # batch, both norms all-reduced (MAX) -- same sweep counts and residuals as vof_solve_p on one domain)
            self.s.solve_p(a.jacobi_tol, a.jacobi_max, 10, a.jacobi_crit)
            e.update_uv(); e.set_BC()
            e.solve_VOF_rudman(e.istep); e.post_process_f(); e.set_BC()
            self.s.exchange()                         # F, u, v, p: the 8 rows the step consumed are well inside the halo

    def depths(self):
        return self.s.depths()                       # (collective: rank 0 holds the domain's profile, the others None)

    def record_diag(self):
        self.diag_rows.append(self.s.diagnostics())   # (collective: every rank holds the combined row, rank 0 writes it)

    def interface(self):
        return self.s.interface()                    # (collective: rank 0 holds the domain's list, the others None)

    def blobs(self):
        return self.s.blobs(self.args.blobs_phase, self.args.blobs_threshold)   # (collective, likewise)

    def take_diag(self):
        rows, self.diag_rows = self.diag_rows, []
        return rows

    def report(self):
        return ''

    def full(self, name):
        return self.s.gather(name)                   # rank 0: (nx+2, ny+2); others: None

    def courant(self):
        parts = self.s.comm.gather_object(int(self.eng.get_counter("courant_violations")))
        return self.base_courant + sum(parts) if self.rank == 0 else 0

    def close(self):
        self.s.barrier()
        self.s.close()


def run(args, api=None, comm=None, rank=None, world=None, out=None):
    """The program of one rank.  api: the C-ABI object (default: the HIP library; there is no other
    engine in the product).  comm / rank / world: the process group when several ranks run."""
    say = out if out is not None else (lambda *a: print(*a, flush=True))
    if world is None:
        env_world = int(os.environ.get("WORLD_SIZE", 1))
        if args.gpus == 1 and env_world > 1:
            # e.g. torchrun without --gpus: every rank would run the whole problem on device 0 and race on output/, data/
            raise SystemExit("started under a launcher with WORLD_SIZE = %d but --gpus is 1: pass --gpus %d (row strips), "
                             "or start a single process" % (env_world, env_world))
        world = env_world if args.gpus > 1 else 1
    if rank is None:
        rank = int(os.environ.get("RANK", 0)) if world > 1 else 0
    if world > 1 and (args.verbs or args.vis):
        raise SystemExit("--verbs and --vis run on one GPU (drop --gpus)")
    if world > 1 and args.pressure_solver in ("cg", "mg"):
        raise SystemExit("--pressure-solver %s runs on one GPU (drop --gpus)" % args.pressure_solver)
    if world > 1 and getattr(args, "mg_cycles", 0) > 0:
        raise SystemExit("--mg-cycles runs on one GPU (drop --gpus)")
    if world > 1 and world != args.gpus:
        raise SystemExit("--gpus %d but the launcher started %d ranks" % (args.gpus, world))
    if api is None:
        from ._lib import hip_api
        api = hip_api()
    if world > 1:
        if comm is None:
            from .comms import EnvComm
            comm = EnvComm()
        drv = _Strips(args, api, comm, rank, world)
    else:
        drv = _Single(args, api)
    eng = drv.eng
    nx, ny, dt = args.nx, args.ny, eng.get_param("dt")
    rho_l, rho_g = eng.get_param("rho_l"), eng.get_param("rho_g")
    nu_l, nu_g = eng.get_param("nu_l"), eng.get_param("nu_g")
    gy, sigma = eng.get_param("gy"), eng.get_param("sigma")
    Lx, Ly = eng.get_param("Lx"), eng.get_param("Ly")
    lead = rank == 0

    if lead:
        say(f'>>> A VOF solver written in HIP for MI355X; Press Ctrl-C to exit.')
        say(f'>>> Grid resolution: {nx} x {ny}, dt = {dt:4.2e}' + (f', {world} row strips' if world > 1 else ''))
        say(f'>>> Density ratio: {rho_l / rho_g : 4.2f}, gravity : {gy : 4.2f}, sigma : {sigma : 4.2f}')
        say(f'>>> Viscosity ratio: {nu_l / nu_g : 4.2f}')

    istep = 0
    nstep = 100  # Interval to update output                       (2dvof.py:497)
    drv.init(args.ic)
    if lead:
        os.makedirs('output', exist_ok=True)  # Make dir for output                 (:500)
        os.makedirs('data', exist_ok=True)    # Make dir for data save               (:501)
    numerics = numerics_of(args, dt)
    if args.resume:
        fields, istep, warn0 = load_state(args.resume, nx, ny, args.dtype, numerics)
        drv.load(fields, istep, warn0)
        if lead:
            say(f'>>> Resumed from {args.resume} at step {istep}.')

    # passive tracers (vof_tracers_*): seeded from the initial F, or restored beside the checkpoint
    tracers_on = bool(getattr(args, "tracers", 0)) and world == 1
    tr_save = (getattr(args, "tracers_save_every", None) or 0) if tracers_on else 0
    tr_path = 'data/tracers.csv'
    if tracers_on:
        from . import tracers as tracers_mod
        state = os.path.join(os.path.dirname(os.path.abspath(args.resume)), 'tracers_state.npz') if args.resume else None
        if state and drv.load_tracers(state, istep):
            say(f'>>> Tracers restored from {state}.')
        else:
            say(f'>>> {drv.seed_tracers()} tracers seeded ({args.tracers_phase}).')
        if tr_save and not (args.resume and os.path.exists(tr_path) and os.path.getsize(tr_path) > 0):
            with open(tr_path, 'w') as f:
                f.write(tracers_mod.CSV_HEADER + '\n')

    # fixed sensors (vof_gauges_*): from the command line, or the set beside the checkpoint
    gauges_every = (getattr(args, "gauges_every", None) or 0) if world == 1 else 0
    gauges_on, gauges_path = False, 'data/gauges.csv'
    if world == 1 and (getattr(args, "gauge", None) or getattr(args, "gauges_file", None) or gauges_every):
        from . import gauges as gauges_mod
        xy = gauges_mod.parse_positions(args.gauge, args.gauges_file)
        state = os.path.join(os.path.dirname(os.path.abspath(args.resume)), 'gauges_state.npz') if args.resume else None
        if not len(xy) and state and os.path.exists(state):
            xy = np.load(state, allow_pickle=False)["xy"]
            say(f'>>> Gauges restored from {state}.')
        if not len(xy):
            raise SystemExit("--gauges-every: no gauges given and none beside the checkpoint (--gauge X,Y, --gauges-file FILE)")
        drv.set_gauges(xy)
        gauges_on = True
        say(f'>>> {len(xy)} gauges set.')
        if gauges_every and not (args.resume and os.path.exists(gauges_path) and os.path.getsize(gauges_path) > 0):
            with open(gauges_path, 'w') as f:
                f.write(gauges_mod.GAUGES_CSV_HEADER + '\n')
    stop_at_gauges = bool(gauges_every) and not drv.gauges_in_advance

    # a dye (vof_dye_*): seeded from F inside the boxes, read from a file, or restored beside the checkpoint
    dye_every = getattr(args, "dye_every", None) or 0
    dye_save = getattr(args, "dye_save_every", None) or 0
    dye_on, dye_path = False, 'data/dye.csv'
    if getattr(args, "dye_box", None) or getattr(args, "dye_file", None) or dye_every or dye_save:
        from . import dye as dye_mod
        if dye_conflicts(args) or world > 1:
            raise SystemExit(dye_conflicts(args) or "the dye options run on one GPU (drop --gpus)")
        if not hasattr(api, "step_dye"):
            raise SystemExit("the dye options need the dye verbs of the HIP library (vof_dye_*, vof_step_dye): this backend has none")
        state = os.path.join(os.path.dirname(os.path.abspath(args.resume)), 'dye_state.npz') if args.resume else None
        # (a resumed run continues the dye it saved, whatever boxes the command line repeats: they describe step 0)
        if state and os.path.exists(state) and int(np.load(state, allow_pickle=False)["istep"]) == istep:
            C = np.load(state, allow_pickle=False)["C"]
            say(f'>>> Dye restored from {state}.')
        elif args.dye_file:
            C = np.load(args.dye_file, allow_pickle=False)
            if C.shape != (nx + 2, ny + 2):
                raise SystemExit("--dye-file: %s holds an array of shape %s, the dye is (nx+2, ny+2) = %s" % (args.dye_file, C.shape, (nx + 2, ny + 2)))
        elif args.dye_box:
            C = dye_mod.boxes(drv.full("F"), eng.get_param("dx"), eng.get_param("dy"), parse_dye_boxes(args.dye_box))
        else:
            raise SystemExit("--dye-every / --dye-save-every: no dye given and none of this step beside the checkpoint (--dye-box X0,X1,Y0,Y1, --dye-file FILE.npy)")
        drv.set_dye(C)
        dye_on = True
        say(f'>>> Dye set: {float(np.asarray(C, dtype=np.float64)[1:-1, 1:-1].sum()) * eng.get_param("dx") * eng.get_param("dy"):.6e} m^2.')
        if dye_every and not (args.resume and os.path.exists(dye_path) and os.path.getsize(dye_path) > 0):
            with open(dye_path, 'w') as f:
                f.write(','.join(('istep', 'time') + dye_mod.DERIVED) + '\n')

    # the free-surface profile (vof_depths) is read between calls, like the interface
    depths_every = getattr(args, "depths_every", None) or 0
    depths_path = 'data/depths.csv'
    if depths_every:
        from . import gauges as gauges_mod
        if lead and not (args.resume and os.path.exists(depths_path) and os.path.getsize(depths_path) > 0):
            with open(depths_path, 'w') as f:
                f.write(gauges_mod.DEPTHS_CSV_HEADER + '\n')

    # pictures rendered on the device (vof_frame) are taken between calls too: three bytes a pixel leave the device
    frames_every = (getattr(args, "frames_every", None) or 0) if world == 1 else 0
    frames_path = 'data/frames.csv'
    if frames_every:
        from . import frames as frames_mod
        if not hasattr(api, "frame"):
            raise SystemExit("--frames-every needs the frame verbs of the HIP library (vof_frame): this backend has none")
        fq, flo, fhi = parse_frame(args.frame)
        block = args.frame_block or frames_mod.default_block(nx, ny)
        cmap = args.frame_cmap or frames_mod.DEFAULT_CMAP[fq]
        eng.set_frame_lut(None if cmap in ("grey", "gray") else frames_mod.lut(cmap))
        frame_kw = dict(quantity=fq, bx=block, by=block, lo=flo, hi=fhi, contour=bool(args.frame_contour), symmetric=flo == fhi and fq in frames_mod.SIGNED)
        os.makedirs('output', exist_ok=True)
        if not (args.resume and os.path.exists(frames_path) and os.path.getsize(frames_path) > 0):
            with open(frames_path, 'w') as f:
                f.write('istep,time,lo,hi,nan_pixels\n')

    # per-cell statistics over the run (vof_stats_*): a sample only enqueues, so it is taken between the calls of whatever loop steps
    stats_every = (getattr(args, "stats_every", None) or 0) if world == 1 else 0
    stats_save = getattr(args, "stats_save_every", None) or 0
    stats_from = getattr(args, "stats_from", 0)
    stats_path, stats_saved_at = 'data/stats.csv', -1
    if stats_every:
        from . import stats as stats_mod
        if not hasattr(api, "stats_sample"):
            raise SystemExit("--stats-every needs the statistics verbs of the HIP library (vof_stats_*): this backend has none")
        stats_mask = stats_mod.mask_of(args.stats)
        eng.stats_begin(stats_mask, args.stats_level)
        say(f'>>> Statistics begun: {", ".join(g for g, b in stats_mod.GROUPS.items() if stats_mask & b)}, a sample every {stats_every} steps'
            + (f' from step {stats_from} on' if stats_from else '') + (' (they start anew: not part of a checkpoint).' if args.resume else '.'))
        if not (args.resume and os.path.exists(stats_path) and os.path.getsize(stats_path) > 0):
            with open(stats_path, 'w') as f:
                f.write(','.join(('istep', 'time') + tuple(k.lower() for k in stats_mod.SUMMARY)) + '\n')

    def save_stats(k):
        """data/stats_NNNNNN.npz: the raw planes, N and the derived arrays; a line of the summary to data/stats.csv."""
        summ = eng.stats_summary()
        planes = {p: eng.stats_plane(p) for p in stats_mod.planes_of(stats_mask)}
        tmp = 'data/stats_%06d.tmp.npz' % k
        np.savez(tmp, N=np.int64(summ["SAMPLES"]), istep=np.int64(k), mask=np.int64(stats_mask), level=np.float64(args.stats_level), **planes,
                 **stats_mod.derive(planes, summ["SAMPLES"], dt))
        os.replace(tmp, 'data/stats_%06d.npz' % k)
        with open(stats_path, 'a') as f:
            f.write(','.join([str(k), repr(k * dt)] + [repr(float(summ[c])) for c in stats_mod.SUMMARY]) + '\n')

    diag_every = drv.diag_every
    stop_at_diag = bool(diag_every) and not drv.diag_in_advance
    diag_last = None
    if diag_every and lead:
        from . import diag
        dx, dy = eng.get_param("dx"), eng.get_param("dy")
        diag_path = 'data/diagnostics.csv'
        if not (args.resume and os.path.exists(diag_path) and os.path.getsize(diag_path) > 0):
            with open(diag_path, 'w') as f:      # the header once; a resumed run appends to what is there
                f.write(','.join(('istep', 'time') + diag.DERIVED) + '\n')

    # the interface is read between calls (vof_interface records nothing in advance): every step loop is cut at the multiples of N
    iface_every = getattr(args, "interface_every", None) or 0
    iface_last = None
    iface_path = 'data/interface.csv'
    if iface_every and lead and not (args.resume and os.path.exists(iface_path) and os.path.getsize(iface_path) > 0):
        with open(iface_path, 'w') as f:
            f.write('istep,segments,degenerate,length\n')

    def write_diag(rows):
        """Append the rows (raw dicts) to data/diagnostics.csv; returns the derived values of the last one."""
        last = None
        with open(diag_path, 'a') as f:
            for raw in rows:
                last = diag.derive(raw, dx, dy, dt, nx, ny)
                k = int(raw["ISTEP"])
                f.write(','.join([str(k), repr(k * dt)] + [repr(float(last[c])) for c in diag.DERIVED]) + '\n')
        return last

    # ... and so are the blobs (vof_blobs)
    blobs_every = getattr(args, "blobs_every", None) or 0
    blobs_path = 'data/blobs.csv'
    if blobs_every and lead:
        from . import blobs as blobs_mod
        if not (args.resume and os.path.exists(blobs_path) and os.path.getsize(blobs_path) > 0):
            with open(blobs_path, 'w') as f:
                f.write(blobs_mod.CSV_HEADER + '\n')

    def next_stop(i):
        n = nstep - i % nstep
        if stop_at_diag:
            n = min(n, diag_every - i % diag_every)
        if iface_every:
            n = min(n, iface_every - i % iface_every)
        if blobs_every:
            n = min(n, blobs_every - i % blobs_every)
        if args.save_every:
            n = min(n, args.save_every - i % args.save_every)
        if tr_save:
            n = min(n, tr_save - i % tr_save)
        if stop_at_gauges:
            n = min(n, gauges_every - i % gauges_every)
        if depths_every:
            n = min(n, depths_every - i % depths_every)
        if dye_save:
            n = min(n, dye_save - i % dye_save)
        if frames_every:
            n = min(n, frames_every - i % frames_every)
        if stats_every and i + stats_every - i % stats_every >= stats_from:
            n = min(n, stats_every - i % stats_every)
        if stats_save:
            n = min(n, stats_save - i % stats_save)
        if args.steps:
            n = min(n, args.steps - i)
        return n

    try:
        while args.steps == 0 or istep < args.steps:
            n = next_stop(istep)
            drv.advance(n)
            istep += n
            if diag_every:
                if stop_at_diag and istep % diag_every == 0:
                    drv.record_diag()
                rows = drv.take_diag()
                if lead and rows:
                    diag_last = write_diag(rows)
            if iface_every and istep % iface_every == 0:
                iface_last = drv.interface()
                if lead:
                    seg, summ = iface_last
                    np.save('data/interface_%06d.npy' % istep, seg)
                    with open(iface_path, 'a') as f:
                        f.write('%d,%d,%d,%r\n' % (istep, summ["SEGMENTS"], summ["DEGENERATE"], float(summ["LENGTH"])))
            if blobs_every and istep % blobs_every == 0:
                found = drv.blobs()
                if lead:
                    with open(blobs_path, 'a') as f:
                        f.writelines(line + '\n' for line in blobs_mod.csv_lines(found[0], istep, eng.get_param("dx"), eng.get_param("dy")))
            if tr_save and istep % tr_save == 0:
                rows, summ = drv.tracer_rows()
                np.save('data/tracers_%06d.npy' % istep, rows)
                with open(tr_path, 'a') as f:
                    f.write(tracers_mod.csv_line(dict(summ, ISTEP=istep)) + '\n')
            if gauges_every:
                if stop_at_gauges and istep % gauges_every == 0:
                    drv.record_gauges()
                recs = drv.take_gauges()
                if recs:
                    with open(gauges_path, 'a') as f:
                        for k, rows in recs:
                            f.writelines(line + '\n' for line in gauges_mod.gauges_csv_lines(k, rows))
            if depths_every and istep % depths_every == 0:
                prof = drv.depths()
                if lead:
                    d = gauges_mod.derive(prof[0], prof[3], eng.get_param("dx"), eng.get_param("dy"))
                    np.save('data/depths_%06d.npy' % istep, np.stack([d["x"], d["depth"], prof[2].astype(np.float64)], axis=1))
                    with open(depths_path, 'a') as f:
                        f.write(gauges_mod.depths_csv_line(dict(prof[3], ISTEP=istep), eng.get_param("dx"), eng.get_param("dy")) + '\n')
            if dye_on:
                rows = drv.take_dye()
                if rows:
                    with open(dye_path, 'a') as f:
                        for raw in rows:
                            d, k = dye_mod.derive(raw, eng.get_param("dx"), eng.get_param("dy")), int(raw["ISTEP"])
                            f.write(','.join([str(k), repr(k * dt)] + [repr(float(d[c])) for c in dye_mod.DERIVED]) + '\n')
                if dye_save and istep % dye_save == 0:
                    np.save('data/dye_%06d.npy' % istep, drv.dye())
            if frames_every and istep % frames_every == 0:
                rgb, _, fs = eng.frame(**frame_kw)
                frames_mod.write_png('output/frame_%06d.png' % istep, rgb)
                with open(frames_path, 'a') as f:
                    f.write('%d,%r,%r,%r,%d\n' % (istep, istep * dt, fs["LO"], fs["HI"], fs["NAN_PIXELS"]))
            if stats_every:
                if istep % stats_every == 0 and istep >= stats_from:
                    eng.stats_sample()
                if stats_save and istep % stats_save == 0:
                    save_stats(istep)
                    stats_saved_at = istep
            if args.save_every and istep % args.save_every == 0:
                if dye_on:                                          # (beside the checkpoint, whose format stays as it is)
                    np.savez('data/dye_state.tmp.npz', C=drv.dye(), istep=np.int64(istep))
                    os.replace('data/dye_state.tmp.npz', 'data/dye_state.npz')
                fields = {f: drv.full(f) for f in STATE}
                warn = drv.courant()
                if lead:
                    save_state('data/%08d.npz' % istep, fields, istep, nx, ny, args.dtype, args.ic, warn, numerics)
                if tracers_on:
                    drv.save_tracers('data/tracers_state.npz', istep)   # (beside the checkpoint, whose format stays as it is)
                if gauges_on:
                    drv.save_gauges('data/gauges_state.npz', istep)
            if (istep % nstep) == 0:  # Output data every <nstep> steps            (:530)
                warn = drv.courant()
                extra = drv.report()
                Fnp = drv.full("F") if args.s else None
                if args.s and iface_every and istep % iface_every != 0:
                    iface_last = drv.interface()      # (the frame shows the interface of its own step)
                if not lead:
                    continue
                from .vis import OPTIONS, save_display
                say(f'>>> Number of steps:{istep:<5d}, Time:{istep*dt:5.2e} sec. Displaying {OPTIONS[args.vis][0]}.'
                    + extra
                    + (f' Volume: {diag_last["volume"]:.6e}, max|div u|: {diag_last["div_max"]:8.2e}, CFL: {diag_last["cfl"]:8.2e}.' if diag_last else '')
                    + (f' [{warn} Courant warnings]' if warn else ''))
                if args.s:
                    import matplotlib
                    matplotlib.use('Agg')
                    import matplotlib.pyplot as plt
                    count = istep // nstep - 1
                    if world == 1:   # what gui.set_image / gui.arrows show in the reference (:531-559), as a file
                        save_display(f'output/{count:06d}-vis.png', drv.sim, args.vis)
                    fx, fy = 5, Ly / Lx * 5
                    plt.figure(figsize=(fx, fy))
                    plt.axis('off')
                    plt.contourf(Fnp.T, cmap=plt.cm.Blues)
                    if iface_every:
                        from .vis import draw_segments
                        draw_segments(plt.gca(), iface_last[0], eng.get_param("dx"), eng.get_param("dy"))
                    plt.savefig(f'output/{count:06d}-f.png')
                    plt.close()
    except KeyboardInterrupt:
        pass
    if stats_every and stats_saved_at != eng.istep:
        save_stats(eng.istep)                                       # the end of the run
    drv.close()
    return 0


def main(script, argv=None):
    """Entry of 2dvof.py: parse; with --gpus N and no launcher around us become the launcher
    (vof2d/launch.py: a GPU-free parent and N fresh workers, never a re-exec of a process that
    touched the GPU); otherwise run this rank."""
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(argv)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1:
        from .launch import spawn_ranks, under_launcher
        if not under_launcher():
            return spawn_ranks(script, argv, args.gpus)
    return run(args)
