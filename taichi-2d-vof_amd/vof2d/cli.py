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
from types import SimpleNamespace

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
    ext.add_argument('--energy-every', type=int, default=None, metavar='N',
                     help='every N steps append a row to data/energy.csv: kinetic, potential and surface energy, their sum, and the rate at '
                          'which viscosity, the upwind advection, gravity, surface tension and the pressure gradient feed the kinetic energy -- '
                          'the momentum predictor\'s own terms evaluated face by face in double and reduced on the device (vof_energy); one GPU')
    ext.add_argument('--interface-every', type=int, default=None, metavar='N',
                     help='every N steps write data/interface_NNNNNN.npy -- the interface as one PLIC segment per mixed cell, '
                          'rows of i, j, x0, y0, x1, y1, nx, ny extracted on the device (vof_interface) -- and append istep, '
                          'segments, degenerate, length to data/interface.csv; with -s the VOF frame draws the segments')
    ext.add_argument('--curvature-every', type=int, default=None, metavar='N',
                     help='every N steps write data/curvature_NNNNNN.npy -- one row per mixed cell, in the order of --interface-every: '
                          'i, j, kappa (height functions), valid, axis, kappa_csf (the solver\'s own), hp, f, computed on the device '
                          '(vof_curvature) -- and append istep, rows, degenerate, valid, the valid share, mean, rms, min and max of both '
                          'curvatures to data/curvature.csv; one GPU')
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
    ext.add_argument('--scene', default=None, metavar='FILE.json',
                     help='the initial state: the shapes of FILE.json (rect, box, disc, ellipse, halfplane, triangle, polygon, each liquid or '
                          'gas; vof2d/scene.py) painted in list order over an empty domain on the device (vof_set_scene), in place of -ic; '
                          'works with --gpus N; not with --resume (a checkpoint holds its own state)')
    ext.add_argument('--scene-over-ic', action='store_true', help='paint the scene over the state of -ic instead of an empty domain')
    ext.add_argument('--scene-samples', type=int, default=None, metavar='S',
                     help="sample points per cell and axis, 1, 2, 4, 8 or 16 (default: the file's \"samples\", 8 without one)")
    ext.add_argument('--resume', default=None, metavar='FILE', help='continue from a file written by --save-every')
    ext.add_argument('--regrid-from', default=None, metavar='FILE',
                     help='start from a file written by --save-every on ANOTHER grid (finer or coarser by integer factors of at most 16) or in '
                          'the other precision: its state is carried onto this run\'s --nx x --ny on the device (vof_regrid), the step count '
                          'with it; the numerics of the file (dt ...) are not enforced, differences are reported; one GPU; not with '
                          '--resume, --scene or --gpus N')
    ext.add_argument('--regrid-no-plic', action='store_true',
                     help='with --regrid-from: the cells of a refined mixed cell copy its F (default: their F comes from the cell\'s PLIC line)')
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


def load_scene(args):
    """(records, samples) of --scene FILE.json with --scene-samples applied; SystemExit with the reason where the file cannot be used."""
    from . import scene
    try:
        recs, samples = scene.load(args.scene)
        if args.scene_samples is not None:
            samples = scene.check_samples(args.scene_samples)
    except OSError as e:
        raise SystemExit("--scene %s: cannot be read: %s" % (args.scene, e.strerror or e))
    except ValueError as e:                          # (a JSON syntax error is one too)
        raise SystemExit("--scene %s: %s" % (args.scene, e))
    return recs, samples


def parse_args(argv=None):
    """build_parser().parse_args plus the combinations argparse cannot express."""
    parser = build_parser()
    args = parser.parse_args(argv)
    args.scene_shapes = None
    if args.scene is not None:
        if args.resume:
            raise SystemExit("--scene cannot be combined with --resume: a checkpoint holds the state the run continues from, "
                             "and a scene would paint over it (drop one of them)")
        args.scene_shapes, args.scene_samples = load_scene(args)
    elif args.scene_over_ic or args.scene_samples is not None:
        parser.error("--scene-over-ic and --scene-samples belong to --scene FILE.json: pass that too")
    if args.regrid_from is not None:
        for on, name, why in ((bool(args.resume), "--resume", "a checkpoint of this grid is continued as it is"),
                              (args.scene is not None, "--scene", "the file holds the state the run starts from, and a scene would paint over it"),
                              (args.gpus > 1, "--gpus N", "vof_regrid works on whole-domain handles")):
            if on:
                raise SystemExit("--regrid-from cannot be combined with %s: %s (drop one of them)" % (name, why))
    elif args.regrid_no_plic:
        parser.error("--regrid-no-plic belongs to --regrid-from FILE: pass that too")
    def at_least_1(*options):                        # (in this order: the first refusal is the one reported)
        for opt in options:
            if getattr(args, opt + "_every") is not None and getattr(args, opt + "_every") < 1:
                parser.error("--%s-every needs N >= 1" % opt)
    at_least_1("diag", "interface", "blobs", "curvature", "energy")
    if args.curvature_every is not None and args.gpus > 1:
        parser.error("--curvature-every runs on one GPU (curvature over row strips is not built): drop --gpus")
    if args.energy_every is not None and args.gpus > 1:
        parser.error("--energy-every runs on one GPU (the energy budget over row strips is not built): drop --gpus")
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
    at_least_1("gauges", "depths")
    if (args.gauge or args.gauges_file or args.gauges_every is not None) and args.gpus > 1:
        parser.error("--gauge, --gauges-file and --gauges-every run on one GPU (a gauge reads rows a strip may not hold): drop --gpus, "
                     "or use --depths-every, which works on strips")
    if args.gauges_every is not None and not (args.gauge or args.gauges_file or args.resume):
        parser.error("--gauges-every records the gauges of --gauge X,Y / --gauges-file FILE: pass at least one")
    at_least_1("dye")
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

    def record_gauges(self):
        self.gauge_recs.append((self.sim.istep, self.eng.gauges_get()[0]))

    def depths(self):
        return self.eng.depths()

    def init(self, ic):
        self.sim.set_init_F(ic)

    def paint_scene(self, shapes, samples, clear):
        """(PAINTED, MIXED) of the scene painted on the device."""
        summ = self.sim.set_scene(shapes, samples, clear)
        return int(summ["PAINTED"]), int(summ["MIXED"])

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

    def regrid_from(self, path, plic, numerics):
        """--regrid-from: a temporary solver of the file's grid and precision takes the file's state, vof_regrid carries it onto
        this run's, the temporary is freed.  Returns (istep, the summary, (nx, ny, dtype) of the file, the numerics the file
        recorded with other values as {name: (file's, this run's)})."""
        from . import regrid
        from .solver import VOF2D
        a = self.args
        try:
            z = np.load(path, allow_pickle=False)
            snx, sny, sdtype, istep = int(z["nx"]), int(z["ny"]), str(z["dtype"]), int(z["istep"])
            fields = {f: z[f] for f in STATE}
        except (OSError, KeyError, ValueError) as e:
            raise SystemExit("--regrid-from %s: not a file written by --save-every: %s" % (path, e))
        try:
            regrid.factors(snx, sny, a.nx, a.ny)
        except ValueError as e:
            raise SystemExit("--regrid-from: %s holds a %dx%d run, this one is %dx%d: %s" % (path, snx, sny, a.nx, a.ny, e))
        differ = {k: (z["num_" + k].item(), v) for k, v in numerics.items() if "num_" + k in z.files and z["num_" + k].item() != v}
        tmp = VOF2D(snx, sny, dtype=sdtype, coord_cast=a.coord_cast, device=a.device, jacobi_iters=a.jacobi_iters, api=self.sim.api)
        try:
            for f in STATE:
                tmp.eng.set(f, fields[f])
            tmp.istep = istep
            summ = self.eng.regrid_from(tmp.eng, plic=plic)
        finally:
            tmp.close()
        self.base_courant = int(z["courant_violations"]) if "courant_violations" in z.files else 0
        return istep, summ, (snx, sny, sdtype), differ

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
        K, crit = getattr(a, "mg_cycles", 0), a.jacobi_crit
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
            from . import dye
            N = self.dye_every
            self._advance_recording(n, N, lambda m: sim.step_dye(m, 0, K, crit), lambda: self.dye_rows.append(self.eng.dye_stats()),
                                    lambda m: self.dye_rows.extend(dye.raw_of(r) for r in sim.step_dye(m, N, K, crit)))
        elif self.diag_in_advance:
            # (with --mg-cycles the rows of vof_step_diag replace the residual record of vof_step_mg: the status line reports div_max)
            from . import diag
            N = self.diag_every
            self._advance_recording(n, N, self._step_mg if K > 0 else sim.step, self.record_diag,
                                    lambda m: self.diag_rows.extend(diag.raw_of(r) for r in sim.step_diag(m, N, K, crit)))
        elif self.gauges_in_advance:
            N = self.gauges_every

            def rest(m):                             # (record r of the call belongs to step first + (r + 1) N)
                first = sim.istep
                self.gauge_recs += [(first + (r + 1) * N, rows) for r, rows in enumerate(sim.step_gauges(m, N))]
            self._advance_recording(n, N, sim.step, self.record_gauges, rest)
        elif K > 0:
            self._step_mg(n)
        elif a.verbs:
            sim.step_verbs(n)
        else:
            sim.step(n)

    def _step_mg(self, n):
        _, worst, at = self.sim.step_mg(n, self.args.mg_cycles, self.args.jacobi_crit)
        if not worst <= self.mg_worst[0]:
            self.mg_worst = (worst, at)

    def _advance_recording(self, n, N, plain, ask, rest):
        """n steps with a record at every multiple of N: plain(head) for the steps up to the first multiple (a resumed run may start
        anywhere) and ask() once there, then rest(n - head), one device call that records on the device.  N = 0: plain steps alone."""
        head = min(n, -self.sim.istep % N) if N else n
        if head:
            plain(head)
            if N and self.sim.istep % N == 0:
                ask()
        if n - head:
            rest(n - head)

    def record_diag(self):
        self.diag_rows.append(self.eng.diagnostics())

    def interface(self):
        return self.eng.interface()

    def blobs(self):
        return self.eng.blobs(self.args.blobs_phase, self.args.blobs_threshold)

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

    def paint_scene(self, shapes, samples, clear):
        """Every rank paints its strip from the same list; rank 0 holds the domain's (PAINTED, MIXED), the others (0, 0)."""
        summ = self.s.set_scene(shapes, samples, clear)
        parts = self.s.comm.gather_object((int(summ["PAINTED"]), int(summ["MIXED"])))
        return (sum(p[0] for p in parts), sum(p[1] for p in parts)) if self.rank == 0 else (0, 0)

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
    if world > 1 and getattr(args, "energy_every", None):
        raise SystemExit("--energy-every runs on one GPU (the energy budget over row strips is not built): drop --gpus")
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
    lead = rank == 0

    if lead:
        say(f'>>> A VOF solver written in HIP for MI355X; Press Ctrl-C to exit.')
        say(f'>>> Grid resolution: {nx} x {ny}, dt = {dt:4.2e}' + (f', {world} row strips' if world > 1 else ''))
        say(f'>>> Density ratio: {rho_l / rho_g : 4.2f}, gravity : {gy : 4.2f}, sigma : {sigma : 4.2f}')
        say(f'>>> Viscosity ratio: {nu_l / nu_g : 4.2f}')

    istep = 0
    drv.init(args.ic)
    if getattr(args, "scene_shapes", None) is not None:
        painted, mixed = drv.paint_scene(args.scene_shapes, args.scene_samples, not args.scene_over_ic)
        if lead:
            say(f'>>> Scene {args.scene}: {len(args.scene_shapes)} shapes, {args.scene_samples} x {args.scene_samples} samples a cell, '
                f'painted {painted} cells, {mixed} of them mixed.')
    if lead:
        os.makedirs('output', exist_ok=True)  # Make dir for output                 (:500)
        os.makedirs('data', exist_ok=True)    # Make dir for data save               (:501)
    numerics = numerics_of(args, dt)
    if args.resume:
        fields, istep, warn0 = load_state(args.resume, nx, ny, args.dtype, numerics)
        drv.load(fields, istep, warn0)
        if lead:
            say(f'>>> Resumed from {args.resume} at step {istep}.')
    if getattr(args, "regrid_from", None):
        if world > 1:
            raise SystemExit("--regrid-from runs on one GPU (drop --gpus)")
        istep, summ, (snx, sny, sdtype), differ = drv.regrid_from(args.regrid_from, not args.regrid_no_plic, numerics)
        how = {1: "refined", -1: "coarsened", 0: "copied"}[int(summ["DIR"])]
        say(f'>>> Regridded from {args.regrid_from} ({snx} x {sny} {sdtype}) at step {istep}: {how} by ({int(summ["RX"])}, {int(summ["RY"])}), '
            f'{int(summ["PLIC_CELLS"])} cells from a PLIC line ({int(summ["DEGENERATE"])} mixed cells without an orientation); '
            f'volume {summ["F_SRC"] / (snx * sny):.12g} -> {summ["F_DST"] / (nx * ny):.12g} of the domain.')
        if differ:
            say('>>> Numerics that differ from the file\'s (not enforced): ' + ', '.join(f'{k.replace("_", "-")} {a!r} -> {b!r}' for k, (a, b) in sorted(differ.items())))

    # every recording option is one recorder (vof2d/recorders.py); the loop steps to the nearest stop any of them asks for
    from . import recorders
    recs = recorders.recorders_of(args, drv, world)
    ctx = SimpleNamespace(args=args, api=api, drv=drv, eng=eng, world=world, lead=lead, say=say, istep=istep, nx=nx, ny=ny, dt=dt,
                          dx=eng.get_param("dx"), dy=eng.get_param("dy"), numerics=numerics, recorders=recs, diag_last=None, iface_last=None)
    for r in recs:
        r.setup(ctx)
    try:
        while args.steps == 0 or istep < args.steps:
            n = recorders.next_stop(recs, istep, args.steps)
            drv.advance(n)
            istep += n
            for r in recs:
                r.after(istep)
    except KeyboardInterrupt:
        pass
    for r in recs:
        r.end()                                      # (the statistics of the whole run)
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
