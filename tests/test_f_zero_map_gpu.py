"""k_tm's zero maps (kernels/fused_tm.h): one word per (interior row, k_tm tile column) of F and of its twin says
"these cells are +0 bit for bit", written by the wave that stores the segment; the interior transport march drops the F load of a row
whose three source words stand and the F'' store of a zero segment whose destination word stands.  Nothing a caller can read may
change: knob f_zero_map 1 == 0 == the CPU oracle, value for value, and no flag may ever stand over a cell that is not a zero
(counter fzmap_wrong) -- in particular after F was written by anything that keeps no map (FieldState::fzmap_stale, runtime/state.h).

The grid, 64 x 352: even ny selects the buffer-store form; k_tm's tile columns start at c0 = -7, 105, 217, 329, so tiles 1 and 2 are
interior ones, each with an edge tile beside it; fuse_tm 1, tm_rows 8, tm_taper 0 give interior chunks and chunk seams at rows
16 / 17, 24 / 25, ...  Checkpoints 1, 2, 3, 8, 9, 24, 40 mix batches of 8 and 2 steps with single steps; 17, 32 and 40 end on a batch,
where the flags stand and the counters look at them (behind a single step the maps are stale and both counters read 0).
"""
import numpy as np
import pytest

from util import STATE, assert_fields_same, engine

NX, NY = 64, 352
CHECKPOINTS = (1, 2, 3, 8, 9, 17, 24, 32, 40)
ON_A_BATCH = (17, 32, 40)                            # reached by a batch of 8: the maps are not stale there
TILE_W, TILE_H, TILE_STRIDE = 128, 8, 112            # TmGeom<2> of vof2d_device.h
NTF = (NY + TILE_STRIDE - 1) // TILE_STRIDE
KNOBS = (("fuse_tm", 1), ("tm_rows", 8), ("tm_taper", 0))
COURANT = 0.25


def _hip(api, dtype, zero_map, ic=None):
    e = engine(api, NX, NY, dtype, "f32", ic=ic)
    for k, v in KNOBS:
        e.set_param(k, v)
    e.set_param("f_zero_map", zero_map)
    return e


def _segments_zero(F):
    """[row 1 .. nx, tile]: the columns the tile stores in that row are all +0 bit for bit."""
    bits = F.view(np.uint64 if F.dtype == np.float64 else np.uint32)
    out = np.zeros((NX, NTF), dtype=bool)
    for tj in range(NTF):
        c0 = 1 - TILE_H + tj * TILE_STRIDE
        jlo, jhi = max(1, c0 + TILE_H), min(NY, c0 + TILE_W - TILE_H - 1)
        out[:, tj] = (bits[1:NX + 1, jlo:jhi + 1] == 0).all(axis=1)
    return out


def _blobs(e):
    """Liquid blobs whose edges lie on the tile seams (columns 112 / 113, 119 / 120, 224 / 225) and on the chunk seams (rows 16 / 17,
    24 / 25), in a uniform flow of Courant number 0.25 in both directions: the interface crosses both kinds of seam within 40 steps."""
    dt_np = e.np_dtype
    F = np.zeros((NX + 2, NY + 2), dtype=dt_np)
    F[10:17, 100:113] = 1.0
    F[25:31, 120:225] = 1.0
    u = np.zeros_like(F)
    v = np.zeros_like(F)
    u[2:NX + 1, 1:NY + 1] = COURANT * e.get_param("dx") / e.get_param("dt")
    v[1:NX + 1, 2:NY + 1] = COURANT * e.get_param("dy") / e.get_param("dt")
    e.set("F", F)
    e.set("u", u)
    e.set("v", v)


def _start(e, case):
    if case == "blobs":
        _blobs(e)
    else:
        e.set_init_F(int(case[2:]))


def test_blobs_turn_zero_segments_into_nonzero_ones(oracle_api):
    """The precondition of the blob case, on the CPU: segments that start all-zero must become non-zero on the way (the flags of
    the maps have to fall), at least ten of them."""
    b = engine(oracle_api, NX, NY, "f64", "f32")
    _blobs(b)
    zero0 = _segments_zero(b.get("F"))
    fell = np.zeros_like(zero0)
    for st in CHECKPOINTS:
        b.step(st - b.istep)
        fell |= zero0 & ~_segments_zero(b.get("F"))
    assert int(fell.sum()) >= 10, int(fell.sum())
    assert fell[16:, :].any() and fell[:, 2].any()      # ... behind the chunk seam 16 / 17 and in the tile right of column 224 / 225


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", ["ic1", "ic2", "ic3", "blobs"])
def test_zero_map_changes_no_value(hip_api, oracle_api, case, dtype):
    on, off, ora = _hip(hip_api, dtype, 1), _hip(hip_api, dtype, 0), engine(oracle_api, NX, NY, dtype, "f32")
    for e in (on, off, ora):
        _start(e, case)
    flagged = []
    for st in CHECKPOINTS:
        for e in (on, off, ora):
            e.step(st - e.istep)
        assert_fields_same(on, ora, STATE, ctx="%s %s f_zero_map 1 vs oracle, step %d" % (case, dtype, st))
        assert_fields_same(off, ora, STATE, ctx="%s %s f_zero_map 0 vs oracle, step %d" % (case, dtype, st))
        assert on.get_counter("fzmap_wrong") == 0, "step %d" % st
        flagged.append(on.get_counter("fzmap_flagged"))
        assert flagged[-1] <= int(_segments_zero(ora.get("F")).sum())
        if case in ("ic1", "blobs") and st in ON_A_BATCH:
            assert flagged[-1] > 0, (st, flagged)      # ... so fzmap_wrong == 0 above looked at that many segments
    print("fzmap_flagged at the checkpoints:", flagged)
    assert on.get_counter("tm_steps") >= 28 and off.get_counter("tm_steps") >= 28
    assert off.get_counter("fzmap_flagged") == 0
    assert on.get_counter("courant_violations") == ora.get_counter("courant_violations")
    if case in ("ic1", "blobs"):
        assert max(flagged) > 0, flagged


def _write_set(on, ora, other):
    F = ora.get("F")
    F[40:48, 130:201] = 1.0
    on.set("F", F)
    ora.set("F", F)


def _write_set_rows(on, ora, other):
    rows = ora.get("F", rows=(40, 47))
    rows[:, 130:201] = 1.0
    on.set("F", rows, rows=(40, 47))
    ora.set("F", rows, rows=(40, 47))


def _write_init(on, ora, other):
    on.set_init_F(2)
    ora.set_init_F(2)


def _write_scene(on, ora, other):
    from vof2d import scene
    on.set_scene([scene.disc(0.07, 0.05, 0.012)], samples=4, clear=False)
    ora.set("F", on.get("F"))


def _write_rudman(on, ora, other):
    on.solve_VOF_rudman(on.istep)
    ora.solve_VOF_rudman(ora.istep)


def _write_copy_rows(on, ora, other):
    on.copy_rows_from(other, "F", 40, 47)
    ora.set("F", other.get("F", rows=(40, 47)), rows=(40, 47))


WRITES = {"set": _write_set, "set_rows": _write_set_rows, "set_init_F": _write_init, "set_scene": _write_scene,
          "solve_VOF_rudman": _write_rudman, "copy_rows": _write_copy_rows}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("before", [6, 7])
@pytest.mark.parametrize("how", list(WRITES))
def test_a_write_from_outside_clears_the_maps(hip_api, oracle_api, how, before, dtype):
    """A dam-break stepped `before` steps, then F changed under the flags by something that keeps no map -- liquid where the maps say
    gas --, then six steps more: still the oracle's values, and no flag over a cell that is not zero.  before = 7 is the eager first
    step and three batches of two, so that the flags stand when the write comes (6 ends on a single step, which clears them itself)."""
    on, ora = _hip(hip_api, dtype, 1, ic=1), engine(oracle_api, NX, NY, dtype, "f32", ic=1)
    other = _hip(hip_api, dtype, 1, ic=2) if how == "copy_rows" else None
    for e in (on, ora):
        e.step(1)
        e.step(before - 1)
    if before == 7:
        flagged = on.get_counter("fzmap_flagged")
        assert flagged > 0 and on.get_counter("fzmap_wrong") == 0
        assert _segments_zero(ora.get("F"))[39:47, 1].all()      # rows 40 .. 47 of tile 1: gas, about to be written
    WRITES[how](on, ora, other)
    assert_fields_same(on, ora, ("F",), ctx="%s %s: F after the write" % (how, dtype))
    for e in (on, ora):
        e.step(6)
    assert_fields_same(on, ora, STATE, ctx="%s %s: six steps after the write" % (how, dtype))
    assert on.get_counter("fzmap_wrong") == 0
    for e in (on, ora):
        e.step(4)                                                # ... and on, ending in batches: the flags stand again
    assert_fields_same(on, ora, STATE, ctx="%s %s: ten steps after the write" % (how, dtype))
    assert on.get_counter("fzmap_wrong") == 0


@pytest.mark.gpu
def test_default_follows_the_gas_share_and_changing_sides_recaptures(hip_api):
    """f_zero_map = -1 (the default) at 4096^2, the smallest grid measured to gain: a dam-break (5/6 gas) runs with the maps, the same
    handle as a rising bubble (2 % gas) without -- its batch graphs are captured again --, and as a dam-break once more (F emptied
    first: set_init_F 1 only adds its liquid, like the reference) with them; a handle with the knob at 0 holds the same values throughout."""
    from util import same, diff_report
    n = 4096
    a, b = engine(hip_api, n, n, "f64", "f32"), engine(hip_api, n, n, "f64", "f32")
    b.set_param("f_zero_map", 0)
    for phase, (ic, with_maps) in enumerate(((1, True), (2, False), (1, True))):
        for e in (a, b):
            if phase == 2:
                e.set("F", np.zeros((n + 2, n + 2)))
            e.set_init_F(ic)
            e.step(1)
            e.step(34)
        assert a.get_counter("tm_steps") == b.get_counter("tm_steps") > 0
        flagged = a.get_counter("fzmap_flagged")
        assert (flagged > 100000) == with_maps and (with_maps or flagged == 0), (phase, ic, flagged, a.get_param("gas_share"))
        assert a.get_counter("fzmap_wrong") == 0 and b.get_counter("fzmap_flagged") == 0
        for f in STATE:
            x, y = a.get(f), b.get(f)
            assert same(x, y), "phase %d ic %d: %s" % (phase, ic, diff_report(x, y, f))
            del x, y


@pytest.mark.gpu
def test_a_view_of_F_ends_the_maps(hip_api, oracle_api):
    """vof_field_view hands out a pointer the caller may write through at any time, unseen by the handle: after a view of F the handle
    keeps no maps (its batches are captured again without them), and a view of another field changes nothing."""
    on, ora = _hip(hip_api, "f64", 1, ic=1), engine(oracle_api, NX, NY, "f64", "f32", ic=1)
    for e in (on, ora):
        e.step(1)
        e.step(8)
    on.field_view("p")
    assert on.get_counter("fzmap_flagged") > 0
    on.field_view("F")
    for e in (on, ora):
        e.step(16)
    assert on.get_counter("fzmap_flagged") == 0 and on.get_counter("tm_steps") == 24
    assert_fields_same(on, ora, STATE, ctx="after a view of F")
