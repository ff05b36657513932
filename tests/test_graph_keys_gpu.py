"""Captured graphs are replayed only against the field views they were captured with (runtime/views.h: every key carries the
orientation of all four pairs -- F / twin, p / pt, (u*, v*) / (mx, my), rhs / kappa).  Each script below moves a view between two
replays of one kind of graph -- an odd number of middle steps of vof_step_tm_piece leaves u*, v* in the mx, my arrays and, where
k_jacobi_pair runs an odd number of times per step, p in pt -- and holds the fields, after every call, == to a side that replays
nothing: the oracle, the single domain beside two strips, a twin with mg_graph = 0.  Small grids with square cells, so that
k_jacobi_pair applies (jacobi_pair_ok) and nx >= 16 (the pieces)."""
import pytest

import _state_trace as st
from util import STATE, assert_fields_same, engine

EVERYTHING = STATE + st.SCRATCH
PLAIN = {"fuse_tm": 0, "overlap_halves": 0}
DTYPES = ("f64", "f32")


def pieces(e, middle):
    """middle + 1 steps of a strip call, piece by piece: the head, `middle` middle steps, the last step."""
    for piece in (0,) + (1,) * middle + (2,):
        e.step_tm_piece(piece)


def pair(hip_api, other_api, dtype, knobs, **kw):
    a = engine(hip_api, 24, 40, dtype, "f32", ic=1, **dict(st.SQUARE, **kw))
    b = engine(other_api, 24, 40, dtype, "f32", ic=1, **dict(st.SQUARE, **kw))
    for k, v in knobs.items():
        a.set_param(k, v)
    return a, b


# ---- 1. the views moved under the batch graphs of a full domain
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,middle,form,iters",
                         # (an even number of middle steps: the control -- every view is back where it was)
                         [(d, m, f, 10) for d in DTYPES for f in ("tm", "plain") for m in ((1, 3), (2, 4))] +
                         [("f64", (1, 3), "tm", 20)],      # p swapped twice per middle step, u*, v* once
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_batch_graphs_behind_moved_views(hip_api, oracle_api, dtype, middle, form, iters):
    a, o = pair(hip_api, oracle_api, dtype, st.TM if form == "tm" else PLAIN, jacobi_iters=iters)
    try:
        n = 0

        def both(what, steps, call):
            nonlocal n
            call(a)
            o.step(steps)
            n += 1
            assert a.istep == o.istep
            assert_fields_same(a, o, EVERYTHING, ctx="%s %s, %d sweeps, call %d (%s), step %d" % (form, dtype, iters, n, what, a.istep))

        both("step 1", 1, lambda e: e.step(1))
        both("step 4", 4, lambda e: e.step(4))
        both("pieces, %d middle" % middle[0], middle[0] + 1, lambda e: pieces(e, middle[0]))
        both("step 4", 4, lambda e: e.step(4))
        both("pieces, %d middle" % middle[1], middle[1] + 1, lambda e: pieces(e, middle[1]))
        both("step 4", 4, lambda e: e.step(4))
    finally:
        a.close(); o.close()


# ---- 2. ... and under the step graphs of two strips (device copies stand in for the send / recv groups, as in _state_trace.run_strips)
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_step_graphs_of_strips_behind_moved_views(hip_api, dtype):
    from vof2d.strips import stored_rows
    nx, ny, iters, owns = (st.STRIPS[k] for k in ("nx", "ny", "iters", "owns"))
    W = iters + 8                     # VOF_HALO_ROWS (include/vof2d.h)
    kw = dict(Lx=nx / 256.0, Ly=ny / 256.0, jacobi_iters=iters)     # square cells
    full = engine(hip_api, nx, ny, dtype, "f32", ic=1, **kw)
    strips = [engine(hip_api, nx, ny, dtype, "f32", ic=1, rows=stored_rows(nx, o, W), own=o, **kw) for o in owns]

    def trade(fields, D=W):
        lo_s, hi_s = strips
        edge = owns[0][1]
        for f in fields:
            lo_s.copy_rows_from(hi_s, f, edge + 1, edge + D)
            hi_s.copy_rows_from(lo_s, f, edge + 1 - D, edge)

    def check(what):
        for k, s in enumerate(strips):
            rows = (0, owns[0][1]) if k == 0 else (owns[1][0], nx + 1)
            assert_fields_same(s, full, STATE, rows, ctx="%s, %s, strip %d, step %d" % (what, dtype, k, s.istep))

    def steps(what):
        for r in range(3):
            for s in strips:
                s.step(1)
            trade(STATE)
            full.step(1)
            check("%s, round %d" % (what, r))

    def one_middle(what):
        for s in strips:
            s.step_tm_piece(0)
        trade(st.SCRATCH)
        for s in strips:
            s.step_tm_piece(1)
        trade(("rhs", "p"))
        trade(("F", "u_star", "v_star"), 8)     # (what a middle step of overlap mode 5 ships: runtime/comm.h, kTmReachRows)
        for s in strips:
            s.step_tm_piece(2)
        trade(STATE)
        full.step(2)
        check(what)

    try:
        for s in strips:
            s.step(1)
        trade(STATE)
        full.step(1)
        check("step 1")
        one_middle("pieces")
        steps("steps behind one middle step")
        one_middle("pieces again")
        steps("steps behind two middle steps")
    finally:
        full.close()
        for s in strips:
            s.close()


# ---- 3. the graph of a V-cycle and the step graphs of vof_step_mg, against a twin that launches every kernel itself
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_mg_graphs_behind_moved_views_and_past_the_cap(hip_api, dtype):
    a, b = pair(hip_api, hip_api, dtype, {})
    b.set_param("mg_graph", 0)
    try:
        n = 0

        def both(what, call):
            nonlocal n
            ra, rb = call(a), call(b)
            n += 1
            assert ra == rb and a.istep == b.istep, (what, ra, rb)
            assert_fields_same(a, b, EVERYTHING, ctx="%s, call %d (%s), step %d" % (dtype, n, what, a.istep))

        solve = lambda e: e.solve_p_mg(0.0, 3)
        both("solve_p_mg", solve)
        both("step 1", lambda e: e.step(1))      # (the pieces want the first step after set_init_F behind them)
        both("pieces, one middle step", lambda e: pieces(e, 1))
        both("solve_p_mg", solve)
        both("step 2", lambda e: e.step(2))
        both("solve_p_mg", solve)
        for c in list(range(1, 19)) + [1]:      # (more cycle counts than a kind keeps graphs for: the oldest go, on the device)
            both("step_mg(2, %d)" % c, lambda e: e.step_mg(2, c))
    finally:
        a.close(); b.close()


# ---- 4. the phase graphs
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_phase_graphs_behind_moved_views(hip_api, oracle_api, dtype):
    a, o = pair(hip_api, oracle_api, dtype, {})
    try:
        n = 0

        def both(what, on_a, on_o):
            nonlocal n
            on_a(a)
            on_o(o)
            n += 1
            assert a.istep == o.istep
            assert_fields_same(a, o, EVERYTHING, ctx="%s, call %d (%s), step %d" % (dtype, n, what, a.istep))

        def phases(e):
            for ph in (0, 1, 2):
                e.step_phase(ph)

        both("phases", phases, lambda e: e.step(1))
        for verb in ("fct_x_sweep", "fct_y_sweep", "fct_x_sweep"):      # (F is left in its twin)
            both(verb, lambda e: getattr(e, verb)(), lambda e: getattr(e, verb)())
        both("phases behind the sweeps", phases, lambda e: e.step(1))
        both("pieces, one middle step", lambda e: pieces(e, 1), lambda e: e.step(2))
        both("phases behind the pieces", phases, lambda e: e.step(1))
    finally:
        a.close(); o.close()
