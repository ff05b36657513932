"""The scheduling of the command line on the CPU, without a library: where the main loop stops (the recorders' next-stop rule as a
pure function of the options) and how _Single cuts n steps into plain steps, one question and one recording device call."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

from vof2d import _abi, cli, recorders

GRID = ["--nx", "16", "--ny", "16"]
EVERY = (None, 1, 3, 4, 7, 100)
# option -> what else the command line must carry for parse_args to take it
PERIODS = {"--diag-every": [], "--interface-every": [], "--blobs-every": [], "--tracers-save-every": ["--tracers", "10"],
           "--gauges-every": ["--gauge", "0.1,0.1"], "--depths-every": [], "--dye-save-every": ["--dye-box", "0,1,0,1"], "--frames-every": [],
           "--stats-every": [], "--stats-save-every": [], "--save-every": []}
NO_DYE = ("--diag-every", "--tracers-save-every", "--gauges-every")     # (cli.dye_conflicts)


def draws():
    """One option alone at every value, then random combinations; each with the two `in advance` flags of the driver."""
    rng = random.Random(20)
    for opt in PERIODS:
        for n in EVERY[1:]:
            yield {opt: n, **({"--stats-every": 4} if opt == "--stats-save-every" else {})}, False, False
    for _ in range(30):
        chosen = {opt: rng.choice(EVERY) for opt in PERIODS}
        for opt in NO_DYE if rng.random() < 0.5 else ("--dye-save-every",):
            chosen[opt] = None
        if chosen["--stats-every"] is None:
            chosen["--stats-save-every"] = None
        yield {k: v for k, v in chosen.items() if v is not None}, rng.random() < 0.5, rng.random() < 0.5


def stops_made(recs, start, steps, limit):
    """The steps at which the loop of cli.run stops, from `start` on (an endless run is followed up to `limit`)."""
    i, made = start, []
    while i < (steps or limit):
        n = recorders.next_stop(recs, i, steps)
        assert n >= 1
        i += n
        made.append(i)
    return [k for k in made if k <= (steps or limit)]


def test_the_loop_stops_exactly_where_a_recorder_is_due():
    cases = 0
    for chosen, diag_ahead, gauges_ahead in draws():
        for stats_from in (0, 5, 9) if "--stats-every" in chosen else (0,):
            argv = GRID + ["--stats-from", str(stats_from)]
            for opt, n in chosen.items():
                argv += [opt, str(n)] + PERIODS[opt]
            args = cli.parse_args(argv)
            drv = SimpleNamespace(diag_every=args.diag_every or 0, diag_in_advance=diag_ahead, gauges_in_advance=gauges_ahead)
            recs = recorders.recorders_of(args, drv, 1)
            # the periods the loop must stop for: every option's but those recorded in advance by the stepping call, and the display's
            periods = [n for opt, n in chosen.items() if opt != "--stats-every" and not (opt == "--diag-every" and diag_ahead)
                       and not (opt == "--gauges-every" and gauges_ahead)] + [100]
            severy = chosen.get("--stats-every")
            for steps in (0, 23):
                for start in range(31):
                    limit = start + 105                                   # (past the display's first stop)
                    want = [i for i in range(start + 1, (steps or limit) + 1)
                            if any(i % n == 0 for n in periods) or (severy and i % severy == 0 and i >= stats_from) or i == steps]
                    assert stops_made(recs, start, steps, limit) == want, (argv, diag_ahead, gauges_ahead, steps, start)
                    cases += 1
    assert cases > 4000


def test_on_strips_the_one_gpu_recorders_stay_out():
    args = cli.parse_args(GRID + ["--diag-every", "3", "--interface-every", "4", "--blobs-every", "5", "--depths-every", "6", "--save-every", "7"])
    args.frames_every, args.stats_every, args.tracers, args.gauges_every = 2, 2, 10, 2   # (parse_args refuses them with --gpus N)
    drv = SimpleNamespace(diag_every=3, diag_in_advance=False)
    names = [type(r).__name__ for r in recorders.recorders_of(args, drv, 2)]
    assert names == ["Diag", "Interface", "Blobs", "Depths", "Checkpoint", "Display"]
    names = [type(r).__name__ for r in recorders.recorders_of(args, SimpleNamespace(diag_every=3, diag_in_advance=True, gauges_in_advance=False), 1)]
    assert names == ["Diag", "Interface", "Blobs", "Tracers", "Gauges", "Depths", "Frames", "Stats", "Checkpoint", "Display"]


# ---------------------------------------------------------------------------- _Single._advance_recording
CALLS = (3, 7, 10, 1, 3, 8)
# (stub, istep at the call, steps) with N = 4, written out from the three methods this one replaced (_advance_diag, _advance_gauges,
# _advance_dye: head = min(n, -istep % N) plain steps, a question if they end on a multiple of N, one recording call for the rest)
FROM_0 = [("rest", 0, 3),                                              # 3: on a multiple, nothing to lead in
          ("plain", 3, 1), ("ask", 4, 0), ("rest", 4, 6),              # 7: 1 to the multiple, asked there, 6 in one call
          ("plain", 10, 2), ("ask", 12, 0), ("rest", 12, 8),           # 10
          ("rest", 20, 1),                                             # 1
          ("plain", 21, 3), ("ask", 24, 0),                            # 3: ends on the multiple, nothing left
          ("rest", 24, 8)]                                             # 8
FROM_2 = [("plain", 2, 2), ("ask", 4, 0), ("rest", 4, 1),              # 3
          ("plain", 5, 3), ("ask", 8, 0), ("rest", 8, 4),              # 7
          ("rest", 12, 10),                                            # 10
          ("plain", 22, 1),                                            # 1: short of the multiple, no question
          ("plain", 23, 1), ("ask", 24, 0), ("rest", 24, 2),           # 3
          ("plain", 26, 2), ("ask", 28, 0), ("rest", 28, 6)]           # 8
RECORDED_AT = [4, 8, 12, 16, 20, 24, 28, 32]                           # (either way: every multiple of 4 up to the last step)


def bare_single(start, **flags):
    """A _Single without a library: the attributes _advance reads, a `sim` and an `eng` that note their calls."""
    drv = object.__new__(cli._Single)
    calls = []
    sim = SimpleNamespace(istep=start)

    def stepper(name, rows_of=None):
        def call(n, every=0, *rest):
            calls.append((name if every or rows_of is None else name + "0", sim.istep, n))
            first, sim.istep = sim.istep, sim.istep + n
            return rows_of(first, n // every) if rows_of and every else []
        return call

    def table(width):
        def rows(first, count):
            a = np.zeros((count, width))
            a[:, 0] = [first + (r + 1) * 4 for r in range(count)]     # ISTEP leads both tables
            return a
        return rows
    sim.step = stepper("step")
    sim.step_mg = lambda n, K, crit: (stepper("step_mg")(n), (0.0, 0.0, 0))[1]
    sim.step_diag = stepper("step_diag", table(_abi.VOF_DIAG_N))
    sim.step_dye = stepper("step_dye", table(_abi.VOF_DYE_N))
    sim.step_gauges = stepper("step_gauges", lambda first, count: ["rows"] * count)
    ask = lambda name, value: lambda: (calls.append((name, sim.istep, 0)), value())[1]
    eng = SimpleNamespace(diagnostics=ask("diagnostics", lambda: {"ISTEP": float(sim.istep)}), dye_stats=ask("dye_stats", lambda: {"ISTEP": float(sim.istep)}),
                          gauges_get=ask("gauges_get", lambda: ("rows", {})))
    drv.sim, drv.eng, drv.mg_worst = sim, eng, (0.0, 0)
    drv.args = SimpleNamespace(jacobi_tol=0.0, verbs=False, mg_cycles=flags.pop("mg_cycles", 0), jacobi_crit="rel")
    drv.dye_on = drv.diag_in_advance = drv.gauges_in_advance = False
    drv.dye_every = drv.diag_every = drv.gauges_every = 4
    drv.dye_rows, drv.diag_rows, drv.gauge_recs = [], [], []
    for k, v in flags.items():
        setattr(drv, k, v)
    return drv, calls


@pytest.mark.parametrize("start,want", [(0, FROM_0), (2, FROM_2)])
def test_advance_recording_with_three_stubs(start, want):
    drv, calls = bare_single(start)

    def stub(name):
        def call(n=0):
            calls.append((name, drv.sim.istep, n))
            drv.sim.istep += n
        return call
    for n in CALLS:
        drv._advance_recording(n, 4, stub("plain"), stub("ask"), stub("rest"))
    assert calls == want and drv.sim.istep == start + 32


ROLES = {  # role -> (the flag of _Single that selects it, the engine calls behind plain / ask / rest, where the records gather)
    "diag": (dict(diag_in_advance=True), {"plain": "step", "ask": "diagnostics", "rest": "step_diag"}, "diag_rows"),
    "diag-mg": (dict(diag_in_advance=True, mg_cycles=2), {"plain": "step_mg", "ask": "diagnostics", "rest": "step_diag"}, "diag_rows"),
    "gauges": (dict(gauges_in_advance=True), {"plain": "step", "ask": "gauges_get", "rest": "step_gauges"}, "gauge_recs"),
    "dye": (dict(dye_on=True), {"plain": "step_dye0", "ask": "dye_stats", "rest": "step_dye"}, "dye_rows"),   # (its head: vof_step_dye with every = 0)
}


@pytest.mark.parametrize("role", list(ROLES))
@pytest.mark.parametrize("start,want", [(0, FROM_0), (2, FROM_2)])
def test_each_role_makes_the_calls_of_the_method_it_had(role, start, want):
    flags, names, kept = ROLES[role]
    drv, calls = bare_single(start, **flags)
    for n in CALLS:
        drv._advance(n)
    assert calls == [(names[stub], istep, n) for stub, istep, n in want]
    got = getattr(drv, kept)
    assert [int(r[0] if role == "gauges" else r["ISTEP"]) for r in got] == RECORDED_AT   # (gauges: tagged first + (r + 1) N by the host)


def test_dye_without_rows_takes_plain_steps_alone():
    drv, calls = bare_single(3, dye_on=True, dye_every=0)
    drv._advance(9)
    assert calls == [("step_dye0", 3, 9)] and drv.dye_rows == []
