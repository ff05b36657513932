"""The fixed script of calls behind tests/test_state_trace_gpu.py and tests/golden/make_state_trace.py: every transition of the
handle's state (runtime/state.h: the step prologue and epilogue, a field written from outside, the phases) and of the launch
context (the plan's geometry, the rhs array of k_tm, the stream of the chains) is crossed once, on the forms the knobs force.

After every call the library's F, u, v, p (and u*, v*, rhs behind a step) are compared == with the oracle's, where the oracle
has the entry point; the tuple of counters, istep and -- for vof_profile_steps -- the launches per kernel make one row of the trace.
A call the oracle lacks (vof_step_mg) leaves a digest of the four fields in its row instead, and hands its fields to the oracle.
Reading a field settles the handle (ghost cells, a predictor formed ahead): the calls marked "quiet" are followed by the row only, so
that the next batch finds the handle as the last one left it (counter tm_chained_batches).
"""
import hashlib

import numpy as np

from util import STATE, diff_report, engine

SCRATCH = ("u_star", "v_star", "rhs")
COUNTERS = ("tm_steps", "tm_chained_batches", "pair_launches", "halves_steps", "tb_plan_active")

TM = {"fuse_tm": 1, "jacobi_pair": 1, "overlap_halves": 0}
SQUARE = {"Lx": 24 / 256.0, "Ly": 40 / 256.0}     # dx == dy == 1 / 256 exactly: k_jacobi_pair wants square cells (jacobi_pair_ok)
CASES = {
    # k_tm + k_jacobi_pair (tm_eligible needs nx >= 16), and k_tm over k_jacobi_tb launches
    "tm_pair_f64": dict(nx=24, ny=40, dtype="f64", knobs=TM, kw=SQUARE),
    "tm_pair_f32": dict(nx=24, ny=40, dtype="f32", knobs=TM, kw=SQUARE),
    "tm_tb_f64": dict(nx=24, ny=40, dtype="f64", knobs=dict(TM, jacobi_tb_general=1), kw=SQUARE),
    "tm_tb_f32": dict(nx=24, ny=40, dtype="f32", knobs=dict(TM, jacobi_tb_general=1), kw=SQUARE),
    # the smallest nx at which a two-step batch runs as chains: nx / 2 - 32 >= 64 (halves_eligible, K = 2, ten sweeps)
    "chains_f64": dict(nx=200, ny=72, dtype="f64", knobs={"fuse_tm": 0, "overlap_halves": 1}),
    "plain_f64": dict(nx=24, ny=40, dtype="f64", knobs={"fuse_tm": 0, "overlap_halves": 0}),
    "two_kernel_f64": dict(nx=24, ny=40, dtype="f64", knobs={"fuse_tm": 0, "overlap_halves": 0, "fuse_transport": 0, "virtual_ghosts": 0}),
}

SCRIPT = (
    ("step", 1),                       # the eager, non-lean step after set_init_F
    ("step", 2),
    ("step", 5),
    ("step", 16 + 3),
    ("verb", "cal_nu_rho"),            # a reader
    ("step", 2, "quiet"),
    ("step", 2, "quiet"),              # ... chained to the batch before it
    ("step", 3),
    ("verb", "get_normal_young"),      # writes mx, my
    ("step", 2),
    ("verb", "update_uv"),             # writes u, v: one eager step follows
    ("step", 3),
    ("verb", "post_process_f"),        # writes F
    ("step", 2),
    ("verb", "fct_x_sweep"),           # swaps F with its twin: the graphs go
    ("step", 4),
    ("set", "u", 11),
    ("step", 2),
    ("set", "F", 12),
    ("step", 4, "quiet"),
    ("setrows", "F", 5, 8, 13),
    ("step", 2),
    ("setrows", "v", 3, 4, 14),
    ("step", 3),
    ("setrows", "mx", 2, 6, 15),
    ("step", 2, "quiet"),
    ("istep", 1),                      # the other parity
    ("step", 4),
    ("tiny_p", 31),                    # a ring of tiny pressure values: the launches report it, the next step's planner plans for it
    ("step", 1),
    ("step", 1),
    ("step", 2),
    ("phases",),
    ("step", 2, "quiet"),
    ("profile", 2),
    ("profile", 5),
    ("step", 2),
    ("knob", "jacobi_tb_adapt", 0),
    ("step", 16 + 3),
    ("knob", "jacobi_tb_adapt", 1),
    ("knob", "solve_pairs", 1),
    ("step", 2, "quiet"),
    ("sweeps", 20),                    # vof_solve_p_jacobi(20): ten sweeps per launch where the pair kernel applies
    ("step", 2, "quiet"),
    ("scratch",),                      # get("rhs") with the next step's predictor formed ahead
    ("step", 2, "quiet"),
    ("step_mg", 3, 2),
    ("step", 3),
    ("step", 2, "quiet"),
    ("step_mg", 2, 1),
    ("step", 2),
)


def digest(e, names=STATE):
    return {f: hashlib.sha256(np.ascontiguousarray(e.get(f)).tobytes()).hexdigest()[:16] for f in names}


def row_of(e, **extra):
    return dict(counters=[int(e.get_counter(c)) for c in COUNTERS], istep=int(e.istep), **extra)


def noise(seed, x, f):
    rng = np.random.default_rng(seed)
    x = x.astype(np.float64)
    if f == "F":
        return np.clip(x + 0.3 * rng.standard_normal(x.shape) * (rng.random(x.shape) < 0.1), 0, 1)
    return x + 0.01 * rng.standard_normal(x.shape)


def differ(a, b, names):
    return [diff_report(x, y, n) for n in names for x, y in [(a.get(n), b.get(n))] if not np.array_equal(x, y)]


def run_case(hip_api, oracle_api, case):
    """The script on the library and on the oracle; the trace (one row per call).  Raises AssertionError at the first call after
    which a field of the library differs from the oracle's."""
    spec = CASES[case]
    a = engine(hip_api, spec["nx"], spec["ny"], spec["dtype"], "f32", ic=1, **spec.get("kw", {}))
    b = engine(oracle_api, spec["nx"], spec["ny"], spec["dtype"], "f32", ic=1, **spec.get("kw", {}))
    trace = []
    try:
        for k, v in spec["knobs"].items():
            a.set_param(k, v)
        for n, op in enumerate(SCRIPT):
            names, extra = STATE, {}
            if op[0] == "step":
                a.step(op[1]); b.step(op[1])
                names = STATE + SCRATCH
            elif op[0] == "verb":
                for e in (a, b):
                    if op[1] == "update_uv":
                        e.cal_nu_rho()
                    getattr(e, op[1])()
            elif op[0] == "set":
                x = noise(op[2], b.get(op[1]), op[1])
                for e in (a, b):
                    e.set(op[1], x)
            elif op[0] == "setrows":
                rows = (op[2], op[3])
                x = noise(op[4], b.get(op[1], rows), op[1])
                for e in (a, b):
                    e.set(op[1], x, rows)
            elif op[0] == "tiny_p":
                nx, ny = spec["nx"], spec["ny"]
                rng = np.random.default_rng(op[1])
                i, j = np.meshgrid(np.arange(nx + 2), np.arange(ny + 2), indexing="ij")
                r = np.hypot(i - 0.5 * nx, j - 0.45 * ny)
                x = b.get("p").astype(np.float64)
                band = (r > 0.15 * min(nx, ny)) & (r < 0.4 * min(nx, ny))
                x[band] = (1e-290 if spec["dtype"] == "f64" else 1e-32) * rng.uniform(0.01, 50.0, size=int(band.sum()))
                x[r <= 0.15 * min(nx, ny)] = 0.0
                for e in (a, b):
                    e.set("p", x)
            elif op[0] == "istep":
                for e in (a, b):
                    e.istep = e.istep + op[1]
            elif op[0] == "phases":
                for ph in (0, 1, 2):
                    a.step_phase(ph)
                    if ph < 2:
                        trace.append(row_of(a, op="phase %d" % ph))
                b.step(1)
            elif op[0] == "profile":
                extra["profile"] = {k: int(v[1]) for k, v in sorted(a.profile_steps(op[1]).items())}
                b.step(op[1])
            elif op[0] == "knob":
                a.set_param(op[1], op[2])
            elif op[0] == "sweeps":
                for e in (a, b):
                    e.cal_nu_rho()
                    e.solve_p_jacobi(op[1])
            elif op[0] == "scratch":
                names = ("rhs",) + STATE + SCRATCH
            elif op[0] == "step_mg":     # (the oracle has no multigrid: the library's fields go to both sides)
                a.step_mg(op[1], op[2])
                extra["digest"] = digest(a)
                for f in STATE:
                    x = a.get(f)
                    for e in (a, b):
                        e.set(f, x)
                b.istep = a.istep
            else:
                raise ValueError(op)
            trace.append(row_of(a, op=" ".join(str(x) for x in op), **extra))
            assert a.istep == b.istep, (case, n, op, a.istep, b.istep)
            if "quiet" not in op:
                msgs = differ(a, b, names)
                assert not msgs, "%s, call %d %r: %s" % (case, n, op, " ; ".join(msgs))
        return trace
    finally:
        a.close(); b.close()


# ---- one emulated two-strip case: device copies stand in for the send / recv groups (as the strip fuzz of test_fuzz_gpu.py does)
STRIPS = dict(nx=40, ny=24, dtype="f64", iters=10, owns=((1, 20), (21, 40)))


def run_strips(hip_api):
    """Two strips driven through vof_step_phase and vof_step_tm_piece beside the single domain; the trace of the strips.  Raises
    AssertionError where an owned row of a strip differs from the single domain's."""
    from vof2d.strips import stored_rows
    nx, ny, dtype, iters, owns = (STRIPS[k] for k in ("nx", "ny", "dtype", "iters", "owns"))
    W = iters + 8                     # VOF_HALO_ROWS (include/vof2d.h)
    full = engine(hip_api, nx, ny, dtype, "f32", ic=1, jacobi_iters=iters)
    strips = [engine(hip_api, nx, ny, dtype, "f32", ic=1, jacobi_iters=iters, rows=stored_rows(nx, o, W), own=o) for o in owns]
    trace = []

    def trade(fields, D=W):
        lo_s, hi_s = strips
        edge = owns[0][1]
        for f in fields:
            lo_s.copy_rows_from(hi_s, f, edge + 1, edge + D)
            hi_s.copy_rows_from(lo_s, f, edge + 1 - D, edge)

    def check(what):
        for k, s in enumerate(strips):
            trace.append(row_of(s, op="%s, strip %d" % (what, k)))
            g0, g1 = (0, owns[0][1]) if k == 0 else (owns[1][0], nx + 1)
            for f in STATE:
                x, y = s.get(f, (g0, g1)), full.get(f, (g0, g1))
                assert np.array_equal(x, y), "%s, strip %d: %s" % (what, k, diff_report(x, y, f))

    def phased(n):
        for _ in range(n):
            for ph, fields in ((0, ("p",)), (1, ("u", "v")), (2, ("F",))):
                for s in strips:
                    s.step_phase(ph)
                trade(fields)

    def pieces(n):
        for s in strips:
            s.step_tm_piece(0)
        trade(SCRATCH)
        for _ in range(n - 1):
            for s in strips:
                s.step_tm_piece(1)
            trade(("rhs", "p"))
            trade(("F", "u_star", "v_star"), 8)     # (what a middle step of overlap mode 5 ships: runtime/comm.h, kTmReachRows)
        for s in strips:
            s.step_tm_piece(2)
        trade(STATE)

    try:
        for s in strips:
            s.step(1)
        trade(STATE)
        full.step(1)
        check("step 1")
        phased(2); full.step(2)
        check("two phased steps")
        pieces(4); full.step(4)
        check("four steps in pieces")
        for e in strips + [full]:
            e.get_normal_young()      # (leaves its normals in mx, my: the second u*, v* pair of the middle steps)
        pieces(3); full.step(3)
        check("three steps in pieces")
        phased(1); full.step(1)
        check("a phased step")
        x = noise(21, full.get("u"), "u")
        full.set("u", x)
        for s in strips:
            s.set("u", x[s.row_lo:s.row_hi + 1])
        for s in strips:
            s.step(1)
        trade(STATE)
        full.step(1)
        check("a step after set u")
        pieces(2); full.step(2)
        check("two steps in pieces")
        return trace
    finally:
        full.close()
        for s in strips:
            s.close()
