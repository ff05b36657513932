"""k_tm's rows as segments (kernels/row_segments.h, L::tm_chunk_rows): a launch cuts its rows into a body and up to three tail
segments of shorter chunks, handed out in order.  Which rows a pair takes never changes a value -- every cell is computed from
the same operands whatever the chunking --, so what can break is the bookkeeping: the pair -> (segment, chunk, rows) mapping, the
pair count, ragged last chunks, chunks shorter than the marches' pipeline (12 transport rows around a chunk, the momentum wave
five behind), the interior predicate at segment boundaries.  Taper on == taper off == the oracle, value for value."""
import pytest

from util import STATE, assert_fields_same, engine

TM_ROWS = 12
STEPS = 20      # one eager step, then batch graphs of 16 and 2 steps and a single step
GRIDS = ((160, 240), (97, 250))    # the odd nx gives ragged last chunks; ny even: the buffer-store forms run


def layouts(nx):
    """name -> (knobs of the tail: (first row, chunk rows) of up to three segments; segments that hold rows)"""
    return {
        # the column interface of the dam (rows <= nx / 3) crosses the first boundary, its row interface lies in the 7-row chunks
        "body-7-3": (((nx // 4 + 1, 7), (nx // 2 + 1, 3)), 3),
        "last-row-alone": (((nx, 5),), 2),
        "second-of-four-empty": (((nx // 3, 7), (nx // 3, 5), (2 * nx // 3, 3)), 3),
    }


def pair_form(api, nx, ny, dtype, ic, tail=None, tm_rows=TM_ROWS):
    e = engine(api, nx, ny, dtype, "f32", ic=ic)
    e.set_param("overlap_halves", 0)
    e.set_param("fuse_tm", 1)
    e.set_param("jacobi_pair", 1)
    e.set_param("tm_rows", tm_rows)
    if tail is None:
        e.set_param("tm_taper", 0)
    else:
        for k, (at, rows) in enumerate(tail):
            e.set_param("tm_tail_at%d" % (k + 1), at)
            e.set_param("tm_tail_rows%d" % (k + 1), rows)
        e.set_param("tm_taper", 1)
    return e


_reference = {}


def reference(hip_api, oracle_api, nx, ny, dtype, ic):
    """the oracle and the untapered pair form after STEPS steps, computed once per case and left alone"""
    key = (nx, ny, dtype, ic)
    if key not in _reference:
        o = engine(oracle_api, nx, ny, dtype, "f32", ic=ic)
        off = pair_form(hip_api, nx, ny, dtype, ic)
        for e in (o, off):
            e.step(STEPS)
        assert off.get_counter("tm_steps") == STEPS - 2 and off.get_counter("tm_segments") == 1
        _reference[key] = (o, off)
    return _reference[key]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["body-7-3", "last-row-alone", "second-of-four-empty"])
@pytest.mark.parametrize("ic", [1, 2])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_tail_segments_change_no_value(hip_api, oracle_api, nx, ny, dtype, ic, layout):
    tail, used = layouts(nx)[layout]
    o, off = reference(hip_api, oracle_api, nx, ny, dtype, ic)
    a = pair_form(hip_api, nx, ny, dtype, ic, tail)
    a.step(STEPS)
    ctx = "%s %dx%d ic %d, %s, step %d" % (dtype, nx, ny, ic, layout, STEPS)
    assert a.get_counter("tm_steps") == STEPS - 2, ctx        # k_tm ran: every step but the eager first and the single last
    assert a.get_counter("tm_segments") == used, ctx
    assert_fields_same(a, off, STATE, ctx="taper on / off, " + ctx)       # (whole arrays: ghost rows and columns included)
    assert_fields_same(a, o, STATE, ctx="taper on / oracle, " + ctx)
    assert_fields_same(off, o, STATE, ctx="taper off / oracle, " + ctx)
    assert a.get_counter("courant_violations") == off.get_counter("courant_violations") == o.get_counter("courant_violations"), ctx
    a.close()


@pytest.mark.gpu
def test_rule_changes_no_value_at_two_rounds(hip_api):
    """The layout by the rule on a full domain whose launch runs more than one residency round (2048^2: 2432 pairs of 16-row chunks
    for 1536 slots), against taper off.  tm_taper = -1, the default, keeps one segment there -- the rule asks for body chunks of at
    least 28 rows, and the sweep it was set from lost 1 % at 2048^2 --; -2 is the same cut without that condition: a body and three
    tail segments."""
    n = 2048
    engines = {}
    for taper in (0, -1, -2):
        e = pair_form(hip_api, n, n, "f64", 1, tm_rows=0)
        e.set_param("tm_taper", taper)
        e.step(4)
        assert e.get_counter("tm_steps") == 2, taper
        engines[taper] = e
    assert engines[0].get_counter("tm_segments") == 1 and engines[-1].get_counter("tm_segments") == 1
    assert engines[-2].get_counter("tm_segments") == 4
    for taper in (-1, -2):
        assert_fields_same(engines[taper], engines[0], STATE, ctx="tm_taper %d / off, %d^2 step 4" % (taper, n))
        assert engines[taper].get_counter("courant_violations") == engines[0].get_counter("courant_violations")
