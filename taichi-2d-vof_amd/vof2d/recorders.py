"""The recording options of the command line (vof2d/cli.py), one small object each.

A recorder has five concerns and nothing more: `setup` (refusals, what is restored beside a checkpoint, the CSV header once),
`next_stop` (how many steps until it next needs the main loop to stop, or None), `after` (what it does at a stop), `checkpoint`
(what it saves beside a checkpoint) and `end` (the end of the run).  `cli.run` builds the list with `recorders_of`, steps to the
nearest stop (`next_stop` of the list) and calls every recorder's `after` in the order of the list: that order fixes the order of
the device calls and of the lines in the files.  `run` below is what cli.run hands to every setup: a namespace of args, api, drv,
eng, world, lead, say, the step the run starts from, the grid, the numerics, the list itself and what the status line reports.
"""
import os

import numpy as np

from . import blobs, cli, curvature, diag, dye, energy, frames, gauges, stats, tracers

NSTEP = 100  # Interval to update output                       (2dvof.py:497)


def header_once(path, header, resume):
    """Start `path` with its header -- unless a resumed run finds the file there and not empty: it appends to what is there."""
    if not (resume and os.path.exists(path) and os.path.getsize(path) > 0):
        with open(path, 'w') as f:
            f.write(header + '\n')


def append(path, lines):
    with open(path, 'a') as f:
        f.writelines(line + '\n' for line in lines)


def csv_row(k, dt, values, columns):
    """istep, time and the columns of `values`, as the CSV files of the derived rows hold them."""
    return ','.join([str(k), repr(k * dt)] + [repr(float(values[c])) for c in columns])


def beside(resume, name):
    """`name` beside the checkpoint a run resumes from (None: not a resumed run)."""
    return os.path.join(os.path.dirname(os.path.abspath(resume)), name) if resume else None


def due(i, N):
    return bool(N) and i % N == 0


class Recorder:
    path = header = None                             # the CSV file it appends to and that file's first line

    def __init__(self, every=0, save=0, stop=True, on=None, start=0):
        """A record every `every` steps from step `start` on -- the main loop stops for it unless stop is False: the stepping call
        records it on the device --, something saved every `save` steps (0: never, both).  on: whether the options ask for it at all."""
        self.every, self.save, self.stop, self.start = every, save, stop, start
        self.periods = tuple((N, first) for N, first in ((every if stop else 0, start), (save, 0)) if N)
        self.on = bool(every or save) if on is None else bool(on)

    def setup(self, run):
        self.run = run
        if run.lead and self.header:
            header_once(self.path, self.header, run.args.resume)

    def next_stop(self, i):
        return min((max(i + N - i % N, -(-first // N) * N) - i for N, first in self.periods), default=None)   # (the next multiple of N from `first` on)

    def after(self, i=None):
        pass

    checkpoint = end = after                         # nothing at a stop, beside a checkpoint or at the end of the run, by default


def next_stop(recorders, i, steps=0):
    """The steps from step i to the nearest stop any recorder asks for (the display always asks), or to the last step of --steps."""
    n = min(s for s in (r.next_stop(i) for r in recorders) if s is not None)
    return min(n, steps - i) if steps else n


class Diag(Recorder):
    """--diag-every.  The fused steps record their rows on the device (vof_step_diag); the Python loops are asked at the multiples of N."""
    path, header = 'data/diagnostics.csv', ','.join(('istep', 'time') + diag.DERIVED)

    def after(self, i):
        run = self.run
        if self.stop and due(i, self.every):
            run.drv.record_diag()
        rows, run.drv.diag_rows = run.drv.diag_rows, []
        if run.lead and rows:
            derived = [diag.derive(raw, run.dx, run.dy, run.dt, run.nx, run.ny) for raw in rows]
            append(self.path, (csv_row(int(raw["ISTEP"]), run.dt, d, diag.DERIVED) for raw, d in zip(rows, derived)))
            run.diag_last = derived[-1]              # (the status line reports it)


class Energy(Recorder):
    """--energy-every: the energy budget (vof_energy) is read between calls, like the interface; one GPU (cli.run refuses strips)."""
    path, header = 'data/energy.csv', ','.join(('istep', 'time') + energy.DERIVED)

    def setup(self, run):
        if not hasattr(run.api, "energy"):
            raise SystemExit("--energy-every needs the energy verb of the HIP library (vof_energy): this backend has none")
        super().setup(run)
        eng = run.eng
        self.consts = (eng.get_param("gx"), eng.get_param("gy"), eng.get_param("sigma"))

    def after(self, i):
        if due(i, self.every):
            run = self.run
            append(self.path, [csv_row(i, run.dt, energy.derive(run.eng.energy(), run.dx, run.dy, *self.consts), energy.DERIVED)])


class Interface(Recorder):
    """--interface-every: the interface is read between calls (vof_interface records nothing in advance)."""
    path, header = 'data/interface.csv', 'istep,segments,degenerate,length'

    def after(self, i):
        if due(i, self.every):
            self.run.iface_last = self.run.drv.interface()   # (collective on strips: rank 0 holds the domain's list, the others None)
            if self.run.lead:
                seg, summ = self.run.iface_last
                np.save('data/interface_%06d.npy' % i, seg)
                append(self.path, ['%d,%d,%d,%r' % (i, summ["SEGMENTS"], summ["DEGENERATE"], float(summ["LENGTH"]))])


class Curvature(Recorder):
    """--curvature-every: the curvature rows (vof_curvature) are read between calls, like the interface; one GPU."""
    path, header = 'data/curvature.csv', curvature.CSV_HEADER

    def setup(self, run):
        if not hasattr(run.api, "curvature"):
            raise SystemExit("--curvature-every needs the curvature verb of the HIP library (vof_curvature): this backend has none")
        super().setup(run)

    def after(self, i):
        if due(i, self.every):
            rows, summ = self.run.eng.curvature()
            np.save('data/curvature_%06d.npy' % i, rows)
            append(self.path, [curvature.csv_line(summ)])


class Blobs(Recorder):
    """--blobs-every: ... and so are the blobs (vof_blobs)."""
    path, header = 'data/blobs.csv', blobs.CSV_HEADER

    def after(self, i):
        if due(i, self.every):
            found = self.run.drv.blobs()
            if self.run.lead:
                append(self.path, blobs.csv_lines(found[0], i, self.run.dx, self.run.dy))


class Tracers(Recorder):
    """--tracers: passive tracers (vof_tracers_*), seeded from the initial F or restored beside the checkpoint; drv.advance moves them."""
    path, header = 'data/tracers.csv', tracers.CSV_HEADER

    def setup(self, run):
        self.run = run
        state = beside(run.args.resume, 'tracers_state.npz')
        if state and run.drv.load_tracers(state, run.istep):
            run.say(f'>>> Tracers restored from {state}.')
        else:
            run.say(f'>>> {len(tracers.seed(run.eng, run.args.tracers, run.args.tracers_phase))} tracers seeded ({run.args.tracers_phase}).')
        if self.save:
            super().setup(run)

    def after(self, i):
        if due(i, self.save):
            rows, summ = self.run.drv.tracer_rows()
            np.save('data/tracers_%06d.npy' % i, rows)
            append(self.path, [tracers.csv_line(dict(summ, ISTEP=i))])

    def checkpoint(self, i):
        self.run.drv.save_tracers('data/tracers_state.npz', i)


class Gauges(Recorder):
    """--gauge, --gauges-file, --gauges-every: fixed sensors (vof_gauges_*), from the command line or the set beside the checkpoint.
    The plain fused steps take their records on the device (vof_step_gauges); every other loop is asked at the multiples of N."""
    path, header = 'data/gauges.csv', gauges.GAUGES_CSV_HEADER

    def setup(self, run):
        self.run = run
        xy = gauges.parse_positions(run.args.gauge, run.args.gauges_file)
        state = beside(run.args.resume, 'gauges_state.npz')
        if not len(xy) and state and os.path.exists(state):
            xy = np.load(state, allow_pickle=False)["xy"]
            run.say(f'>>> Gauges restored from {state}.')
        if not len(xy):
            raise SystemExit("--gauges-every: no gauges given and none beside the checkpoint (--gauge X,Y, --gauges-file FILE)")
        run.eng.gauges_set(xy)
        run.say(f'>>> {len(xy)} gauges set.')
        if self.every:
            super().setup(run)

    def after(self, i):
        drv = self.run.drv
        if self.stop and due(i, self.every):
            drv.record_gauges()
        recs, drv.gauge_recs = drv.gauge_recs, []
        for k, rows in recs:
            append(self.path, gauges.gauges_csv_lines(k, rows))

    def checkpoint(self, i):
        np.savez('data/gauges_state.npz.tmp.npz', xy=self.run.eng.gauges_get()[0][:, :2], istep=np.int64(i))
        os.replace('data/gauges_state.npz.tmp.npz', 'data/gauges_state.npz')


class Depths(Recorder):
    """--depths-every: the free-surface profile (vof_depths) is read between calls, like the interface."""
    path, header = 'data/depths.csv', gauges.DEPTHS_CSV_HEADER

    def after(self, i):
        run = self.run
        if due(i, self.every):
            prof = run.drv.depths()                  # (collective on strips: rank 0 holds the domain's profile)
            if run.lead:
                d = gauges.derive(prof[0], prof[3], run.dx, run.dy)
                np.save('data/depths_%06d.npy' % i, np.stack([d["x"], d["depth"], prof[2].astype(np.float64)], axis=1))
                append(self.path, [gauges.depths_csv_line(dict(prof[3], ISTEP=i), run.dx, run.dy)])


class Dye(Recorder):
    """--dye-*: a dye (vof_dye_*), seeded from F inside the boxes, read from a file, or restored beside the checkpoint.  drv.advance
    records the rows of --dye-every on the device (vof_step_dye); the loop stops for --dye-save-every alone."""
    path, header = 'data/dye.csv', ','.join(('istep', 'time') + dye.DERIVED)

    def setup(self, run):
        self.run = run
        args, nx, ny = run.args, run.nx, run.ny
        if cli.dye_conflicts(args) or run.world > 1:
            raise SystemExit(cli.dye_conflicts(args) or "the dye options run on one GPU (drop --gpus)")
        if not hasattr(run.api, "step_dye"):
            raise SystemExit("the dye options need the dye verbs of the HIP library (vof_dye_*, vof_step_dye): this backend has none")
        state = beside(args.resume, 'dye_state.npz')
        # (a resumed run continues the dye it saved, whatever boxes the command line repeats: they describe step 0)
        if state and os.path.exists(state) and int(np.load(state, allow_pickle=False)["istep"]) == run.istep:
            C = np.load(state, allow_pickle=False)["C"]
            run.say(f'>>> Dye restored from {state}.')
        elif args.dye_file:
            C = np.load(args.dye_file, allow_pickle=False)
            if C.shape != (nx + 2, ny + 2):
                raise SystemExit("--dye-file: %s holds an array of shape %s, the dye is (nx+2, ny+2) = %s" % (args.dye_file, C.shape, (nx + 2, ny + 2)))
        elif args.dye_box:
            C = dye.boxes(run.drv.full("F"), run.dx, run.dy, cli.parse_dye_boxes(args.dye_box))
        else:
            raise SystemExit("--dye-every / --dye-save-every: no dye given and none of this step beside the checkpoint (--dye-box X0,X1,Y0,Y1, --dye-file FILE.npy)")
        run.eng.dye_set(C)
        run.drv.dye_on = True                        # (from here on every step is one of vof_step_dye)
        run.say(f'>>> Dye set: {float(np.asarray(C, dtype=np.float64)[1:-1, 1:-1].sum()) * run.dx * run.dy:.6e} m^2.')
        if self.every:
            super().setup(run)

    def after(self, i):
        run = self.run
        rows, run.drv.dye_rows = run.drv.dye_rows, []
        if rows:
            append(self.path, (csv_row(int(raw["ISTEP"]), run.dt, dye.derive(raw, run.dx, run.dy), dye.DERIVED) for raw in rows))
        if due(i, self.save):
            np.save('data/dye_%06d.npy' % i, run.eng.dye_get())

    def checkpoint(self, i):                         # (beside the checkpoint, whose format stays as it is)
        np.savez('data/dye_state.tmp.npz', C=self.run.eng.dye_get(), istep=np.int64(i))
        os.replace('data/dye_state.tmp.npz', 'data/dye_state.npz')


class Frames(Recorder):
    """--frames-every: pictures rendered on the device (vof_frame) are taken between calls too: three bytes a pixel leave the device."""
    path, header = 'data/frames.csv', 'istep,time,lo,hi,nan_pixels'

    def setup(self, run):
        args = run.args
        if not hasattr(run.api, "frame"):
            raise SystemExit("--frames-every needs the frame verbs of the HIP library (vof_frame): this backend has none")
        fq, flo, fhi = cli.parse_frame(args.frame)
        block = args.frame_block or frames.default_block(run.nx, run.ny)
        cmap = args.frame_cmap or frames.DEFAULT_CMAP[fq]
        run.eng.set_frame_lut(None if cmap in ("grey", "gray") else frames.lut(cmap))
        self.kw = dict(quantity=fq, bx=block, by=block, lo=flo, hi=fhi, contour=bool(args.frame_contour), symmetric=flo == fhi and fq in frames.SIGNED)
        os.makedirs('output', exist_ok=True)
        super().setup(run)

    def after(self, i):
        if due(i, self.every):
            rgb, _, fs = self.run.eng.frame(**self.kw)
            frames.write_png('output/frame_%06d.png' % i, rgb)
            append(self.path, ['%d,%r,%r,%r,%d' % (i, i * self.run.dt, fs["LO"], fs["HI"], fs["NAN_PIXELS"])])


class Stats(Recorder):
    """--stats-*: per-cell statistics over the run (vof_stats_*): a sample only enqueues, so it is taken between the calls of whatever
    loop steps, at the multiples of N from step `start` (--stats-from) on."""
    path, header = 'data/stats.csv', ','.join(('istep', 'time') + tuple(k.lower() for k in stats.SUMMARY))
    saved_at = -1

    def setup(self, run):
        args = run.args
        if not hasattr(run.api, "stats_sample"):
            raise SystemExit("--stats-every needs the statistics verbs of the HIP library (vof_stats_*): this backend has none")
        self.mask = stats.mask_of(args.stats)
        run.eng.stats_begin(self.mask, args.stats_level)
        run.say(f'>>> Statistics begun: {", ".join(g for g, b in stats.GROUPS.items() if self.mask & b)}, a sample every {self.every} steps'
                + (f' from step {self.start} on' if self.start else '') + (' (they start anew: not part of a checkpoint).' if args.resume else '.'))
        super().setup(run)

    def write(self, k):
        """data/stats_NNNNNN.npz: the raw planes, the sample count N and the derived arrays; a line of the summary to data/stats.csv."""
        run = self.run
        summ = run.eng.stats_summary()
        planes = {p: run.eng.stats_plane(p) for p in stats.planes_of(self.mask)}
        tmp = 'data/stats_%06d.tmp.npz' % k
        np.savez(tmp, N=np.int64(summ["SAMPLES"]), istep=np.int64(k), mask=np.int64(self.mask), level=np.float64(run.args.stats_level), **planes,
                 **stats.derive(planes, summ["SAMPLES"], run.dt))
        os.replace(tmp, 'data/stats_%06d.npz' % k)
        append(self.path, [csv_row(k, run.dt, summ, stats.SUMMARY)])
        self.saved_at = k

    def after(self, i):
        if due(i, self.every) and i >= self.start:
            self.run.eng.stats_sample()
        if due(i, self.save):
            self.write(i)

    def end(self):
        if self.saved_at != self.run.eng.istep:
            self.write(self.run.eng.istep)


class Checkpoint(Recorder):
    """--save-every: data/NNNNNNNN.npz, and beside it whatever the other recorders keep for a resumed run."""

    def after(self, i):
        run = self.run
        if due(i, self.every):
            fields = {f: run.drv.full(f) for f in cli.STATE}
            warn = run.drv.courant()
            if run.lead:
                cli.save_state('data/%08d.npz' % i, fields, i, run.nx, run.ny, run.args.dtype, run.args.ic, warn, run.numerics)
            for r in run.recorders:
                r.checkpoint(i)


class Display(Recorder):
    """The status line every NSTEP steps (:530) and, with -s, the pictures the reference GUI would show."""

    def after(self, i):
        run, args, drv, iface_every = self.run, self.run.args, self.run.drv, getattr(self.run.args, "interface_every", None) or 0
        if not due(i, NSTEP):
            return
        warn = drv.courant()
        extra = drv.report()
        Fnp = drv.full("F") if args.s else None
        if args.s and iface_every and i % iface_every != 0:
            run.iface_last = drv.interface()          # (the frame shows the interface of its own step)
        if not run.lead:
            return
        from .vis import OPTIONS, save_display
        last = run.diag_last
        run.say(f'>>> Number of steps:{i:<5d}, Time:{i*run.dt:5.2e} sec. Displaying {OPTIONS[args.vis][0]}.'
                + extra
                + (f' Volume: {last["volume"]:.6e}, max|div u|: {last["div_max"]:8.2e}, CFL: {last["cfl"]:8.2e}.' if last else '')
                + (f' [{warn} Courant warnings]' if warn else ''))
        if args.s:
            import matplotlib
            matplotlib.use('Agg')
            import matplotlib.pyplot as plt
            count = i // NSTEP - 1
            if run.world == 1:   # what gui.set_image / gui.arrows show in the reference (:531-559), as a file
                save_display(f'output/{count:06d}-vis.png', drv.sim, args.vis)
            fx, fy = 5, run.eng.get_param("Ly") / run.eng.get_param("Lx") * 5
            plt.figure(figsize=(fx, fy))
            plt.axis('off')
            plt.contourf(Fnp.T, cmap=plt.cm.Blues)
            if iface_every:
                from .vis import draw_segments
                draw_segments(plt.gca(), run.iface_last[0], run.dx, run.dy)
            plt.savefig(f'output/{count:06d}-f.png')
            plt.close()


def recorders_of(args, drv, world):
    """The recorders the options ask for, in the order they act at a stop.  The energy budget, curvature, tracers, gauges, frames and statistics run on one GPU;
    strips get the rest (the dye refuses them)."""
    opt = lambda name: getattr(args, name, None) or 0
    one = world == 1
    every = [Diag(drv.diag_every, stop=not drv.diag_in_advance), Energy(opt("energy_every")), Interface(opt("interface_every")), Curvature(opt("curvature_every") if one else 0), Blobs(opt("blobs_every")),
             Tracers(save=opt("tracers_save_every"), on=one and opt("tracers")),
             Gauges(opt("gauges_every"), stop=not getattr(drv, "gauges_in_advance", False), on=one and (opt("gauge") or opt("gauges_file") or opt("gauges_every"))),
             Depths(opt("depths_every")),
             Dye(opt("dye_every"), opt("dye_save_every"), stop=False, on=opt("dye_box") or opt("dye_file") or opt("dye_every") or opt("dye_save_every")),
             Frames(opt("frames_every") if one else 0), Stats(opt("stats_every"), opt("stats_save_every"), on=one and opt("stats_every"), start=getattr(args, "stats_from", 0)),
             Checkpoint(args.save_every), Display(NSTEP)]
    return [r for r in every if r.on]
