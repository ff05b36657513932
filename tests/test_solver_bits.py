"""The order-exact restatement of the CG and multigrid kernels (tests/_solver_bits_np.py), judged on the CPU before it
judges the kernels (tests/test_solver_bits_gpu.py): on ORACLE right-hand sides its solves must land where the textbook
restatements (tests/_cg_np.py, tests/_mg_np.py) land, within the distances the project already measured between two
solves of one problem and uses in test_agrees_with_the_restatement of tests/test_cg_solve_gpu.py / test_mg_solve_gpu.py.
"""
import functools

import numpy as np
import pytest

import _cg_np as cg
import _mg_np as mg
import _reduce_np as red
import _solver_bits_np as sb
from test_cg_solve import oracle_problem

CAP = 40


@functools.lru_cache(maxsize=None)
def _problem(api, nx, ny, ic):
    e, p0, rhs = oracle_problem(api, nx, ny, "f64", ic, 3)
    for a in (p0, rhs):
        a.setflags(write=False)
    return p0, rhs, e.get_param("dxi2"), e.get_param("dyi2")


def distance(p, q):
    d = (p[1:-1, 1:-1] - p[1:-1, 1:-1].mean()) - (q[1:-1, 1:-1] - q[1:-1, 1:-1].mean())
    return float(np.abs(d).max())


@pytest.mark.parametrize("nx,ny,ic,measured", [(64, 64, 1, 5.0e-5), (96, 130, 2, 1.6e-4)])
def test_order_exact_cg_lands_where_the_textbook_one_does(oracle_api, nx, ny, ic, measured):
    p0, rhs, cx, cy = _problem(oracle_api, nx, ny, ic)
    cap, every = 10 * max(nx, ny), 10
    q, itq, resq, cq = cg.cg_solve(p0, rhs, cx, cy, 1e-8, cap, every, "rel")
    p, it, res, c = sb.cg_solve(p0, rhs, cx, cy, 1e-8, cap, every, "rel")
    print("%dx%d ic %d: order-exact %d iterations (%.3e), textbook %d (%.3e), distance %.3e (bound 4 x %.1e)" %
          (nx, ny, ic, it, res, itq, resq, distance(p, q), measured))
    assert res <= 1e-8 and resq <= 1e-8
    assert abs(it - itq) <= every
    assert distance(p, q) <= 4 * measured
    assert abs(c - cq) <= cg.allowance(p)
    assert np.array_equal(p[0], p0[0]) and np.array_equal(p[:, -1], p0[:, -1])      # the ghost ring is nobody's to write


@pytest.mark.parametrize("nx,ny,ic,measured", [(64, 64, 1, 7.2e-5), (96, 130, 2, 2.3e-5)])
def test_order_exact_multigrid_lands_where_the_textbook_one_does(oracle_api, nx, ny, ic, measured):
    p0, rhs, cx, cy = _problem(oracle_api, nx, ny, ic)
    q, itq, resq, cq = mg.mg_solve(p0, rhs, cx, cy, 1e-8, CAP, 1, "rel")
    p, it, res, c = sb.mg_solve(p0, rhs, cx, cy, 1e-8, CAP, 1, "rel")
    print("%dx%d ic %d: order-exact %d cycles (%.3e), textbook %d (%.3e), distance %.3e (bound 4 x %.1e)" %
          (nx, ny, ic, it, res, itq, resq, distance(p, q), measured))
    assert res <= 1e-8 and resq <= 1e-8
    assert abs(it - itq) <= 1
    assert distance(p, q) <= 4 * measured
    assert abs(c - cq) <= cg.allowance(p)


@pytest.mark.parametrize("nx,ny,ic", [(64, 64, 1), (48, 80, 2)])
def test_block_order_and_launch_order_take_the_same_number_of_cycles(oracle_api, nx, ny, ic):
    """The claim in the docstring of test_block_kernel_converges_like_the_launches (tests/test_step_mg_gpu.py)."""
    p0, rhs, cx, cy = _problem(oracle_api, nx, ny, ic)
    assert sb.block_in_effect(nx, ny, -1, 1)
    a = sb.mg_solve(p0, rhs, cx, cy, 1e-8, CAP, 1, "rel", block=False)
    b = sb.mg_solve(p0, rhs, cx, cy, 1e-8, CAP, 1, "rel", block=True)
    print("%dx%d ic %d: launches %d cycles (%.3e), block %d (%.3e), distance %.3e" % (nx, ny, ic, a[1], a[2], b[1], b[2], distance(a[0], b[0])))
    assert a[2] <= 1e-8 and b[2] <= 1e-8 and 0 < a[1] <= CAP
    assert a[1] == b[1]
    assert a[3] == b[3]                                  # the drift is formed before the orders part


def test_block_rule_and_depths():
    assert sb.level_sizes(16, 260) == [(16, 260), (8, 130), (4, 65)] and sb.block_in_effect(16, 260, -1, 1)
    assert sb.level_sizes(96, 130) == [(96, 130), (48, 65)] and not sb.block_in_effect(96, 130, -1, 1)
    assert sb.level_sizes(64, 64, 2) == [(64, 64), (32, 32)] and not sb.block_in_effect(64, 64, 2, 1)
    assert sb.level_sizes(64, 64, 1) == [(64, 64)] and sb.level_sizes(64, 64, 3)[-1] == (16, 16)
    assert sb.block_in_effect(30, 28, 1, 1) and not sb.block_in_effect(30, 28, 1, 0) and sb.block_in_effect(30, 30, 1, 1) and not sb.block_in_effect(30, 32, 1, 1)
    assert sb.level_sizes(64, 64) == mg.hierarchy(64, 64) and sb.level_sizes(48, 80, 2) == mg.hierarchy(48, 80, 2)


def test_fixed_order_with_more_partials_than_folding_threads():
    """257 block partials into 256 folding threads, against a two-level fold written out by hand: thread 0 takes partials
    0 and 256, every other thread its one, then the tree s = 128 ... 1."""
    rng = np.random.default_rng(11)
    nrows, ny, R = 1025, 130, 2                          # 513 chunks x 2 tiles = 1026 waves = 257 blocks (256 at 1024 rows)
    assert red.blocks(nrows, ny, R) == 257 and red.blocks(1024, ny, R) == 256 and red.blocks(nrows, ny, 2 * R) == 129
    t = rng.standard_normal((nrows, ny)) * 10.0 ** rng.integers(-6, 7, (nrows, ny))
    part = []
    for b in range(257):
        waves = []
        for wv in range(4 * b, 4 * b + 4):
            ch, tj = wv // 2, wv % 2
            lanes = np.zeros(64)
            if ch < 513:
                for r in range(ch * R, min(ch * R + R, nrows)):
                    for lane in range(64):
                        for q in range(2):
                            j = tj * 128 + lane * 2 + q
                            if j < ny:
                                lanes[lane] += t[r, j]
            s = 32
            while s:
                lanes[:64 - s] = lanes[:64 - s] + lanes[s:64]
                s >>= 1
            waves.append(lanes[0])
        part.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    thread = [0.0 + part[k] for k in range(256)]
    thread[0] = thread[0] + part[256]
    s = 128
    while s:
        for k in range(s):
            thread[k] = thread[k] + thread[k + s]
        s >>= 1
    got = red.fixed_order(t, R, 256)
    assert np.float64(got).view(np.uint64) == np.float64(thread[0]).view(np.uint64), (got, thread[0])


def test_finish_guards_and_the_stop_word():
    """The scalar logic of k_cg_finish, mode by mode, on hand-made sums."""
    sc = sb.new_scalars()
    sb.finish(sc, sb.FIN_SUMB, 6.0, sum_ap=-3.0)
    assert sc["C"] == -2.0 and sc["SUMB"] == 6.0
    sc["STOP"], sc["RZ_OLD"] = 1.0, -4.0
    sb.finish(sc, sb.FIN_RESID, -8.0, 0.5, 2.0, restart=1)
    assert sc["STOP"] == 0.0 and sc["BETA"] == 0.0 and (sc["RZ"], sc["MAXZ"], sc["MAXP"]) == (-8.0, 0.5, 2.0)
    sb.finish(sc, sb.FIN_RESID, -8.0, 0.5, 2.0, restart=0)
    assert sc["BETA"] == 2.0 and sc["STOP"] == 0.0
    sc["RZ_OLD"] = 0.0
    sb.finish(sc, sb.FIN_RESID, -8.0, 0.5, 2.0, restart=0)
    assert sc["BETA"] == 0.0
    sb.finish(sc, sb.FIN_APPLY, -16.0)
    assert sc["ALPHA"] == 0.5 and sc["SQ"] == -16.0 and sc["STOP"] == 0.0
    sb.finish(sc, sb.FIN_UPDATE, -2.0, 0.25, 3.0)
    assert (sc["RZ_OLD"], sc["RZ"], sc["BETA"], sc["MAXZ"], sc["MAXP"]) == (-8.0, -2.0, 0.25, 0.25, 3.0)
    sb.finish(sc, sb.FIN_APPLY, 0.0)                     # nothing to divide by
    assert sc["ALPHA"] == 0.0 and sc["STOP"] == 1.0
    before = dict(sc)
    sb.finish(sc, sb.FIN_UPDATE, -1.0, 9.0, 9.0)         # behind the stop word: a no-op
    sb.finish(sc, sb.FIN_APPLY, -1.0)
    assert sc == before
    sc["STOP"] = 0.0
    sb.finish(sc, sb.FIN_UPDATE, float("nan"), 1.0, 1.0)
    assert sc["BETA"] == 0.0 and sc["STOP"] == 1.0
    sc["STOP"] = 0.0
    sb.finish(sc, sb.FIN_APPLY, float("inf"))
    assert sc["ALPHA"] == 0.0 and sc["STOP"] == 1.0


def test_a_constant_p_with_no_right_hand_side_stops_at_once():
    p0 = np.full((10, 8), 3.25)
    p, it, res, c = sb.cg_solve(p0, np.zeros_like(p0), 4096.0, 4096.0, -1.0, 5, 5, "rel")
    assert it == 5 and res == 0.0 and c == 0.0 and np.array_equal(p.view(np.uint64), p0.view(np.uint64))
    p, it, res, c = sb.mg_solve(p0, np.zeros_like(p0), 4096.0, 4096.0, -1.0, 2, 2, "rel")
    assert it == 2 and res == 0.0 and np.array_equal(p.view(np.uint64), p0.view(np.uint64))
