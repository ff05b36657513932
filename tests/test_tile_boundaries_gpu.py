"""Grids whose ny sits on and one past a multiple of every marching kernel's tile stride (runtime: the tile geometry of
vof2d_device.h decides how many tiles a launch gets; one too few leaves the last columns unwritten).  Strides with two
columns per lane: k_jacobi_pair 108, k_transport / k_fct_y / k_tm 112, k_jacobi_tb<5> 116 (square cells) and 120
(general), k_momentum and k_jacobi_tb<2> 124.  Even and odd ny: the buffer-store and the global-store forms.
Bar: value-for-value equality (IEEE ==) with the CPU oracle."""
import functools

import pytest

from util import STATE, assert_fields_same, engine

pytestmark = pytest.mark.gpu

NX, STEPS = 64, 24
NYS = (108, 109, 112, 113, 116, 117, 120, 121, 124, 125, 216, 217)
LX = 0.0625          # dx = 2^-10 exactly, so Ly = ny * 2^-10 gives dy == dx bit for bit
FORMS = {"plain": {"fuse_tm": 0, "overlap_halves": 0}, "pairs": {"fuse_tm": 1, "jacobi_pair": 2, "batch_steps": 4}}


def extent(ny, square):
    return {"Lx": LX, "Ly": ny * LX / NX if square else 2 * LX}


@functools.lru_cache(maxsize=None)
def oracle_fields(oracle_api, ny, dtype, square):
    o = engine(oracle_api, NX, ny, dtype, "f32", ic=2, **extent(ny, square))
    o.step(STEPS)
    return {f: o.get(f) for f in STATE}


class Fields:
    """The oracle's fields after STEPS steps, offered like an engine to assert_fields_same."""

    def __init__(self, fields):
        self.fields = fields

    def get(self, name, rows=None):
        assert rows is None
        return self.fields[name]


@pytest.mark.parametrize("square", [True, False], ids=["square", "general"])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ny", NYS)
def test_steps_on_stride_boundaries(hip_api, oracle_api, ny, dtype, form, square):
    e = engine(hip_api, NX, ny, dtype, "f32", ic=2, **extent(ny, square))
    for k, v in FORMS[form].items():
        e.set_param(k, v)
    assert (e.get_param("dx") == e.get_param("dy")) == square
    e.step(STEPS)
    assert_fields_same(e, Fields(oracle_fields(oracle_api, ny, dtype, square)), STATE,
                       ctx="%dx%d %s %s %s" % (NX, ny, dtype, form, "square" if square else "general"))
    tm_steps, pair_launches = e.get_counter("tm_steps"), e.get_counter("pair_launches")
    if form == "plain":
        assert tm_steps == 0 and pair_launches == 0
    else:
        assert tm_steps > 0
        # (k_jacobi_pair needs square cells; elsewhere the batches run the general k_jacobi_tb<5>)
        assert pair_launches > 0 if square else pair_launches == 0


def test_solve_p_jacobi_on_a_stride_boundary(hip_api, oracle_api, dtype="f64"):
    """Seven sweeps through the verbs at ny = 125 (one past k_jacobi_tb<2>'s stride of 124): one launch of five sweeps,
    one of two."""
    a, b = (engine(api, NX, 125, dtype, "f32", ic=2) for api in (hip_api, oracle_api))
    for e in (a, b):
        e.step(3)
        e.cal_nu_rho()
        e.get_normal_young()
        e.advect_upwind()
        e.set_BC()
        e.solve_p_jacobi(7)
    assert_fields_same(a, b, STATE + ("u_star", "v_star"), ctx="solve_p_jacobi(7), 64x125 %s" % dtype)
