"""The kernels of kernels/cg.h and kernels/mg.h held BIT FOR BIT to the order-exact restatement tests/_solver_bits_np.py
(which tests/test_solver_bits.py judges on the CPU first), through vof_solve_p_cg and vof_solve_p_mg with a negative
tolerance -- never met, so exactly N iterations / K cycles run.

Every case compares the whole of p (ghost ring included) as unsigned integers, the returned count, and the bits of the
returned residual and drift.  No cell is excluded and there is no tolerance.  The grids are the smallest at which each
mechanism of the kernels exists (the tables of the cases say which); the fields are seeded random ones of the size of the
real ones (max|p| 1e3, rhs of the size dxi2 p), plus one oracle-built state per family.
"""
import numpy as np
import pytest

import _reduce_np as red
import _solver_bits_np as sb
from test_cg_solve import oracle_problem
from util import engine

pytestmark = pytest.mark.gpu

RECT = {"Lx": 0.1, "Ly": 0.13}


def bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def fbits(x):
    return int(np.float64(x).view(np.uint64))


def random_fields(e, seed):
    """p with max|p| of some 1e3 and rhs of the size dxi2 p, ghost ring included, finite in both field types; pt (the
    other ping-pong array of multigrid's finest level) likewise: its interior must be written before it is read."""
    rng = np.random.default_rng(seed)
    shape, dt = (e.nx + 2, e.ny + 2), e.np_dtype
    scale = max(e.get_param("dxi2"), e.get_param("dyi2"))
    p = rng.uniform(-1e3, 1e3, shape).astype(dt)
    rhs = (scale * rng.uniform(-1e3, 1e3, shape)).astype(dt)
    pt = rng.uniform(-1e3, 1e3, shape).astype(dt)
    assert np.isfinite(p).all() and np.isfinite(rhs).all()
    return p, rhs, pt


def assert_same_bits(ctx, p, got, want):
    """got = (count, residual, drift) of the library with its p; want = (p, count, residual, drift) of the restatement."""
    q, itq, resq, cq = want
    it, res, c = got
    print("%s: library %d, %.17g, drift %.17g | restatement %d, %.17g, drift %.17g" % (ctx, it, res, c, itq, resq, cq))
    a, b = bits(p), bits(q)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        i, j = bad[0]
        pytest.fail("%s: p differs in %d of %d cells, first at (%d, %d): library %r (%#x), restatement %r (%#x); rows %d..%d, columns %d..%d" %
                    (ctx, len(bad), a.size, i, j, p[i, j], int(a[i, j]), q[i, j], int(b[i, j]), bad[:, 0].min(), bad[:, 0].max(),
                     bad[:, 1].min(), bad[:, 1].max()))
    assert it == itq, ctx
    assert fbits(res) == fbits(resq), "%s: residual %r vs %r" % (ctx, res, resq)
    assert fbits(c) == fbits(cq), "%s: drift %r vs %r" % (ctx, c, cq)


# ---------------------------------------------------------------------------------------------------- conjugate gradients
def run_cg(api, nx, ny, dtype, N, every=None, rows=None, kw=None, fields=None, seed=0):
    e = engine(api, nx, ny, dtype, "f32", **(kw or {}))
    if rows is not None:
        e.set_param("rows_per_wave", rows)
    R = int(e.get_param("rows_per_wave"))
    assert R == (rows if rows is not None else 2)
    p0, rhs = fields if fields is not None else random_fields(e, seed)[:2]
    e.set("p", p0)
    e.set("rhs", rhs)
    every = N if every is None else every
    got = e.solve_p_cg(-1.0, N, every, "rel", build_rhs=False)
    p = e.get("p")
    assert np.array_equal(bits(e.get("rhs")), bits(rhs))
    want = sb.cg_solve(p0, rhs, e.get_param("dxi2"), e.get_param("dyi2"), -1.0, N, every, "rel", R)
    e.close()
    ctx = "cg %dx%d %s N %d every %d R %d %s" % (nx, ny, dtype, N, every, R, kw or "")
    assert_same_bits(ctx, p, got, want)
    return p0, p, got


#   grid          type  rows_per_wave  constants    why
CG_CASES = [
    (8, 6, "f64", None, None),        # one wave, 61 idle lanes, every cell next to a wall
    (33, 17, "f64", None, None),      # odd extents: the last chunk is a single row
    (33, 17, "f64", 1, None),
    (33, 17, "f64", 3, None),
    (33, 17, "f32", None, None),
    (33, 17, "f32", 1, None),
    (33, 17, "f32", 3, None),
    (40, 130, "f64", None, None),     # two column tiles, the second holding 2 columns: the edge-lane direction crosses j = 128 | 129
    (40, 129, "f64", None, None),     # ... holding 1
    (24, 256, "f64", None, None),     # a tile filled exactly
    (24, 257, "f64", None, None),     # a third tile of one column
    (80, 50, "f64", None, RECT),      # dxi2 != dyi2
    (96, 130, "f32", None, None),
]


@pytest.mark.parametrize("N", [1, 2, 5])
@pytest.mark.parametrize("nx,ny,dtype,rows,kw", CG_CASES)
def test_cg_iterations_bit_for_bit(hip_api, nx, ny, dtype, rows, kw, N):
    run_cg(hip_api, nx, ny, dtype, N, rows=rows, kw=kw, seed=1000 * nx + ny)


@pytest.mark.parametrize("nx,blocks", [(1025, 257), (1024, 256)])
def test_cg_more_partials_than_folding_threads(hip_api, nx, blocks):
    """R1 = 2: 513 chunks x 2 tiles = 1026 waves = 257 blocks, more than the 256 folding threads of k_cg_finish (1024 rows:
    exactly 256); the k_cg_apply launch, R2 = 4, has 129."""
    assert red.blocks(nx, 130, 2) == blocks and red.blocks(1025, 130, 4) == 129
    run_cg(hip_api, nx, 130, "f64", 3, seed=nx)


def test_cg_check_interval_keeps_the_direction(hip_api):
    """N = 7 with a check every 3: the iterations run 3 + 3 + 1, through the non-restart CG_FIN_RESID (beta from the
    recomputed residual, the direction kept)."""
    run_cg(hip_api, 40, 130, "f64", 7, every=3, seed=7)


def test_cg_on_an_oracle_built_state(hip_api):
    e, p0, rhs = oracle_problem(hip_api, 96, 130, "f64", 2, 3)
    e.close()
    run_cg(hip_api, 96, 130, "f64", 5, fields=(p0, rhs))


def test_cg_stop_word(hip_api):
    """rhs = 0 and p constant: dot(s, q) = 0, the stop word is set, p is untouched, the count reported is N, the residual 0.
    With a constant rhs instead, whatever the restatement says happens is the expectation."""
    nx, ny, N = 33, 17, 5
    p0 = np.full((nx + 2, ny + 2), 731.25)
    p0_, p, (it, res, drift) = run_cg(hip_api, nx, ny, "f64", N, fields=(p0, np.zeros_like(p0)))
    assert np.array_equal(bits(p), bits(p0)) and it == N and res == 0.0
    run_cg(hip_api, nx, ny, "f64", N, fields=(p0, np.full_like(p0, 7.5e7)))


# ---------------------------------------------------------------------------------------------------- multigrid
def run_mg(api, nx, ny, dtype, K, knobs=None, kw=None, fields=None, seed=0):
    knobs = knobs or {}
    e = engine(api, nx, ny, dtype, "f32", **(kw or {}))
    for k, v in knobs.items():
        e.set_param(k, v)
    R = int(e.get_param("rows_per_wave"))
    nu, levels = knobs.get("mg_nu", 2), knobs.get("mg_levels", -1)
    block = e.get_param("mg_coarse_block") == 1
    assert block == sb.block_in_effect(nx, ny, levels, knobs.get("mg_coarse_block", 0))
    p0, rhs, pt0 = fields if fields is not None else random_fields(e, seed)
    e.set("p", p0)
    e.set("rhs", rhs)
    e.set("pt", pt0)
    got = e.solve_p_mg(-1.0, K, K, "rel", build_rhs=False)
    p = e.get("p")
    assert np.array_equal(bits(e.get("rhs")), bits(rhs))
    want = sb.mg_solve(p0, rhs, e.get_param("dxi2"), e.get_param("dyi2"), -1.0, K, K, "rel", R, nu, levels, block, pt0)
    e.close()
    ctx = "mg %dx%d %s K %d %s %s levels %s block %d" % (nx, ny, dtype, K, knobs, kw or "", sb.level_sizes(nx, ny, levels), block)
    assert_same_bits(ctx, p, got, want)
    return block


BLOCK = {"mg_coarse_block": 1}
#   grid            type   knobs               constants   why
MG_CASES = [
    (8, 8, "f64", {}, None),                  # two levels, coarsest 4x4
    (16, 24, "f64", {}, None),                # 16x24, 8x12, 4x6: unequal extents
    (64, 64, "f64", {}, None),                # five levels
    (64, 64, "f64", BLOCK, None),
    (64, 64, "f32", {}, None),
    (64, 64, "f32", BLOCK, None),
    (96, 130, "f64", {}, None),               # coarsest 48x65 by launches, own_drift on a level whose ny is odd; fine level two tiles
    (16, 260, "f64", {}, None),               # 16x260 (three tiles, the last of 4 columns), 8x130 (two tiles, the second of 2), 4x65
    (16, 260, "f64", BLOCK, None),            # ... whose 6 x 67 cells with the ring fit the block kernel
    (64, 64, "f64", {"mg_nu": 1}, None),      # odd nu: the correction is added to the other ping-pong array
    (64, 64, "f64", {"mg_nu": 3}, None),
    (64, 64, "f64", {"mg_levels": 1}, None),  # the grid itself through the CG arrays of the solve, own_drift false
    (64, 64, "f64", {"mg_levels": 2}, None),  # ends on level 1, the largest level the coarse work arrays are sized for
    (64, 64, "f64", {"mg_levels": 3}, None),
    (30, 28, "f64", {"mg_levels": 1, "mg_coarse_block": 1}, None),   # depth 1 in the block kernel: 32 x 30 cells with the ring
    (80, 50, "f64", {}, RECT),                # rectangular cells, coarsest 40x25 by launches
]


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("nx,ny,dtype,knobs,kw", MG_CASES)
def test_mg_cycles_bit_for_bit(hip_api, nx, ny, dtype, knobs, kw, K):
    block = run_mg(hip_api, nx, ny, dtype, K, knobs, kw, seed=1000 * nx + ny)
    assert block == (knobs.get("mg_coarse_block", 0) == 1)      # (every case that sets the knob is eligible for it)


@pytest.mark.parametrize("graph", [0, 1])
def test_mg_captured_cycle_and_launches_against_the_restatement(hip_api, graph):
    run_mg(hip_api, 64, 64, "f64", 2, {"mg_graph": graph}, seed=64)


@pytest.mark.parametrize("nx,ny,ic,knobs", [(96, 130, 2, {}), (64, 64, 1, BLOCK)])
def test_mg_on_an_oracle_built_state(hip_api, nx, ny, ic, knobs):
    e, p0, rhs = oracle_problem(hip_api, nx, ny, "f64", ic, 3)
    e.close()
    run_mg(hip_api, nx, ny, "f64", 2, knobs, fields=(p0, rhs, np.zeros_like(p0)))
