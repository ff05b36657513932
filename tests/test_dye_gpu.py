"""vof_dye_set / _get / _advance / _stats and vof_step_dye on the GPU (include/vof2d.h).

Two judges.  A dye seeded equal to F must stay equal to F byte for byte, ghost cells included: that ties k_dye to the
transport of F and through it to the golden reference runs.  Any other dye is held, step by step and byte for byte, to the
twin oracle state of tests/_dye_np.py: the NumPy oracle's solve_VOF_rudman, post_process_f, set_BC with F := C and u, v,
istep read back from the device.  The statistics are held bit for bit to the order-exact restatement of the same module.

Shapes: nx = 64 (16 chunks of 4 rows by the rule; knob fctx_corr_rows = 25: chunks of 25, 25 and 14 rows); ny = 112 and 113,
on and one past the column stride of k_dye (TransportGeom<2>::STRIDE = 112 for both precisions: one tile, and two whose
second stores a single column), even and odd; square cells (Ly = Lx ny / nx) and rectangular ones; 24 steps: both parities.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _dye_np as ynp
from _interface_np import diag_chunk_rows
from test_step_mg_gpu import FIELDS, assert_same_state
from util import engine
from vof2d import _abi, dye
from vof2d.engine import VofError

pytestmark = pytest.mark.gpu
DP = C.POINTER(C.c_double)
NP = {"f64": np.float64, "f32": np.float32}
STEPS = 24


def square(nx, ny):
    return {"Lx": 0.1, "Ly": 0.1 * ny / nx}


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def where_differs(a, b):
    bits = np.uint64 if a.itemsize == 8 else np.uint32
    bad = np.argwhere(a.view(bits) != b.view(bits))
    if not len(bad):
        return "no cell differs"
    i, j = bad[0]
    return "%d cells differ, first at [%d,%d]: %r vs %r; rows %d..%d cols %d..%d" % (len(bad), i, j, a[i, j], b[i, j], bad[:, 0].min(), bad[:, 0].max(),
                                                                                      bad[:, 1].min(), bad[:, 1].max())


def dyes(e, kind, seed=0):
    """The dyes of the oracle tests, finite everywhere."""
    F = e.get("F")
    rng = np.random.default_rng(seed)
    T = F.dtype.type
    if kind == "box":        # the upper half of whatever liquid there is, and a box in the gas (all zero: the zero-row paths)
        Lx, Ly = e.get_param("Lx"), e.get_param("Ly")
        return dye.box(F, e.get_param("dx"), e.get_param("dy"), 0.0, Lx, 0.3 * Ly, Ly)
    if kind == "random":     # anything in [0, 1], runs of exact 0 and 1 along both directions, random ghost values
        Cd = rng.uniform(0.0, 1.0, F.shape).astype(T)
        Cd[5:20, :] = T(0)
        Cd[30:36, 10:60] = T(1)
        Cd[:, 70:90] = T(0)
        Cd[40:50, 95:] = T(1)
        ring = np.ones(F.shape, bool)
        ring[1:-1, 1:-1] = False
        Cd[ring] = rng.uniform(0.0, 1.0, int(ring.sum())).astype(T)
        return Cd
    if kind == "subnormal":  # f64: columns up to 56 below the smallest normal number, the others so small that their fluxes (x u dt) are
        Cd = rng.uniform(0.0, 1.0, F.shape)
        Cd[:, :57] *= 2.0 ** -1030
        Cd[:, 57:] *= 2.0 ** -1000
        Cd[10:20, :] = 0.0
        assert T is np.float64 and 0 < Cd[:, :57].max() < np.finfo(np.float64).tiny < Cd[:, 57:].max()
        return Cd
    raise ValueError(kind)


def flow(hip_api, nx, ny, dtype, ic, warm=30, flags=0, **kw):
    e = engine(hip_api, nx, ny, dtype, "f32", ic=ic, flags=flags, **kw)
    if warm:
        e.step(warm)
    return e


# ---------------------------------------------------------------------------- invariance: a dye equal to F stays F
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("ic", [1, 2, 3])
def test_a_dye_seeded_with_F_stays_F(hip_api, ic, dtype):
    a, b = (engine(hip_api, 64, 113, dtype, "f32", ic=ic) for _ in range(2))
    a.dye_set(a.get("F"))
    assert a.step_dye(STEPS).shape == (0, _abi.VOF_DYE_N)
    b.step(STEPS)
    Cd, F = a.dye_get(), a.get("F")
    ctx = "64x113 %s ic %d" % (dtype, ic)
    assert same_bytes(Cd, F), ctx + ": " + where_differs(Cd, F)
    assert_same_state(a, b, ctx + ": step_dye(24) against vof_step(24) on a twin")
    assert a.istep == STEPS and not np.array_equal(F, engine(hip_api, 64, 113, dtype, "f32", ic=ic).get("F"))


# ---------------------------------------------------------------------------- the twin oracle state, step by step
ORACLE = [(64, 112, "f64", 1, "box", True, 0), (64, 113, "f64", 3, "random", False, 0), (64, 112, "f32", 2, "random", False, 25),
          (64, 113, "f32", 3, "box", True, 0), (64, 113, "f64", 2, "subnormal", True, 25), (64, 112, "f64", 3, "random", True, 25)]


@pytest.mark.parametrize("nx,ny,dtype,ic,kind,sq,rows", ORACLE)
def test_the_dye_equals_the_twin_oracle_state_step_by_step(hip_api, nx, ny, dtype, ic, kind, sq, rows):
    kw = square(nx, ny) if sq else {}
    a, b = (flow(hip_api, nx, ny, dtype, ic, **kw) for _ in range(2))
    for e in (a, b):
        if rows:
            e.set_param("fctx_corr_rows", rows)          # chunks of 25, 25, 14 rows
    C0 = dyes(a, kind)
    a.dye_set(C0); b.dye_set(C0)
    assert same_bytes(a.dye_get(), C0)                   # stored as given, ghost cells included
    twin = ynp.Twin(C0, NP[dtype], "f32", **kw)
    ctx = "%dx%d %s ic %d %s dye%s" % (nx, ny, dtype, ic, kind, ", chunks of %d rows" % rows if rows else "")
    for k in range(STEPS):
        a.step_dye(1)
        want = twin.advance(a.get("u"), a.get("v"), a.istep)
        got = a.dye_get()
        assert same_bytes(got, want), "%s, step %d (istep %d): %s" % (ctx, k + 1, a.istep, where_differs(got, want))
    assert kind == "subnormal" or not np.array_equal(got[1:-1, 1:-1], C0[1:-1, 1:-1]), ctx + ": the dye has not moved"
    assert got.min() >= 0 and got.max() <= 1
    # one call of 24 steps is the 24 single calls
    b.step_dye(STEPS)
    assert same_bytes(b.dye_get(), got), ctx + ": step_dye(24) against 24 calls: " + where_differs(b.dye_get(), got)
    assert_same_state(a, b, ctx)


# ---------------------------------------------------------------------------- routes
def test_both_routes_graphs_or_not_and_the_twin_array_give_the_same_bytes(hip_api):
    nx, ny, dtype, ic = 64, 113, "f64", 3
    ref = flow(hip_api, nx, ny, dtype, ic)
    C0 = dyes(ref, "random", seed=5)
    ref.dye_set(C0)
    assert ref.get_param("dye_fused") == 1.0
    ref.step_dye(7)
    want, F = ref.dye_get(), ref.get("F")
    # the two sweep kernels and the post kernel of the parent schedule
    two = flow(hip_api, nx, ny, dtype, ic)
    two.set_param("dye_fused", 0)
    two.dye_set(C0)
    two.step_dye(7)
    assert same_bytes(two.dye_get(), want), "dye_fused = 0: " + where_differs(two.dye_get(), want)
    # the knob flipped between the steps
    mix = flow(hip_api, nx, ny, dtype, ic)
    mix.dye_set(C0)
    for k in range(7):
        mix.set_param("dye_fused", k & 1)
        mix.step_dye(1)
    assert same_bytes(mix.dye_get(), want) and same_bytes(mix.get("F"), F)
    # eager launches
    eager = flow(hip_api, nx, ny, dtype, ic, flags=_abi.VOF_FLAG_NO_GRAPH)
    eager.dye_set(C0)
    eager.step_dye(7)
    assert same_bytes(eager.dye_get(), want) and same_bytes(eager.get("F"), F)
    assert_same_state(eager, ref, "VOF_FLAG_NO_GRAPH")
    # an odd number of single advances, then step_dye: the dye sits in the other array of the pair when the steps come
    for e in (ref, two):
        for _ in range(3):
            e.dye_advance()
    odd = ref.dye_get()
    assert same_bytes(two.dye_get(), odd) and not same_bytes(odd, want)
    twin = ynp.Twin(want, NP[dtype], "f32")
    for _ in range(3):
        twin.advance(ref.get("u"), ref.get("v"), ref.istep)
    assert same_bytes(odd, twin.C), where_differs(odd, twin.C)
    ref.step_dye(5)                                        # one call; the other handle step by step, with the oracle beside it
    for _ in range(5):
        two.step_dye(1)
        twin.advance(two.get("u"), two.get("v"), two.istep)
    assert same_bytes(ref.dye_get(), twin.C), where_differs(ref.dye_get(), twin.C)
    assert same_bytes(two.dye_get(), twin.C)
    mix.step(5)                                            # a vof_step leaves the dye alone, and the dye calls left F alone
    assert same_bytes(ref.get("F"), mix.get("F")) and same_bytes(mix.dye_get(), want)


def test_multigrid_steps_equal_the_loop(hip_api):
    a, b = (flow(hip_api, 64, 64, "f64", 1, warm=10) for _ in range(2))
    C0 = dyes(a, "box")
    a.dye_set(C0); b.dye_set(C0)
    rows = a.step_dye(9, 3, 2, "rel")
    want = []
    for k in range(9):
        b.step_mg(1, 2, "rel")
        b.dye_advance()
        if (k + 1) % 3 == 0:
            want.append(b.dye_stats())
    assert rows.shape == (3, _abi.VOF_DYE_N) and [dye.raw_of(r) for r in rows] == want
    assert same_bytes(a.dye_get(), b.dye_get())
    assert_same_state(a, b, "step_dye(9, 3, K = 2) against the loop")
    c = flow(hip_api, 64, 64, "f64", 1, warm=10)
    c.step_mg(9, 2, "rel")
    assert_same_state(a, c, "step_dye(9, 3, K = 2) against vof_step_mg(9)")


# ---------------------------------------------------------------------------- non-interference
def test_the_dye_and_the_other_step_verbs_leave_each_other_alone(hip_api):
    a, b = (flow(hip_api, 64, 113, "f64", 3, warm=4) for _ in range(2))
    C0 = dyes(a, "random", seed=9)
    a.dye_set(C0)
    a.gauges_set([[0.01, 0.02], [0.05, 0.06]]); b.gauges_set([[0.01, 0.02], [0.05, 0.06]])
    a.dye_advance(); b.step(0)
    ra, rb = a.step_diag(6, 3), b.step_diag(6, 3)
    assert ra.tobytes() == rb.tobytes()
    a.step_dye(3, 1); b.step(3)
    a.dye_stats()
    ga, gb = a.step_gauges(4, 2), b.step_gauges(4, 2)
    assert ga.tobytes() == gb.tobytes()
    a.dye_advance(); a.dye_advance()
    a.step(17); b.step(17)                                  # (batch graphs on both)
    assert_same_state(a, b, "dye calls interleaved with vof_step, vof_step_diag, vof_step_gauges")
    # a step verb leaves the dye where it was; so do vof_set_init_F and vof_set_field
    before = a.dye_get()
    a.step(3); a.step_diag(2, 1); a.step_gauges(2, 1)
    a.set("p", a.get("p")); a.set_init_F(2)
    assert same_bytes(a.dye_get(), before)
    a.dye_set(None)
    with pytest.raises(VofError, match="VOF_ESTATE"):
        a.dye_get()
    a.dye_set(C0)
    assert same_bytes(a.dye_get(), C0)


# ---------------------------------------------------------------------------- the statistics
@pytest.mark.parametrize("nx,ny,dtype,ic", [(64, 113, "f64", 3), (33, 17, "f32", 2), (96, 130, "f64", 1)])
def test_rows_equal_the_restatement_bit_for_bit(hip_api, nx, ny, dtype, ic):
    e = flow(hip_api, nx, ny, dtype, ic, warm=12)
    Cd = e.get("F") * np.random.default_rng(1).uniform(0.0, 1.25, (nx + 2, ny + 2)).astype(NP[dtype])
    e.dye_set(Cd)
    R = diag_chunk_rows(nx, ny)
    ctx = "%dx%d %s ic %d" % (nx, ny, dtype, ic)

    def hold(raw, where):
        Cn, F, u, v = e.dye_get(), e.get("F"), e.get("u"), e.get("v")
        terms, ext, cells = ynp.restate(Cn, F, u, v)
        ynp.check(raw, terms, ext, cells, istep=e.istep, ctx=ctx + " " + where, say=print, R=R)
        return ynp.row_in_kernel_order(Cn, F, u, v, R, e.istep)

    raw = e.dye_stats()
    hold(raw, "vof_dye_stats")
    assert raw["MAX_EXCESS"] > 0 and raw["SUM_CU"] != 0 and raw == e.dye_stats()          # the same state gives the same bits
    rows = e.step_dye(6, 2)
    assert rows.shape == (3, _abi.VOF_DYE_N) and [r[dye.ISTEP] for r in rows] == [14.0, 16.0, 18.0]
    want = hold(dye.raw_of(rows[-1]), "the last row of vof_step_dye")
    assert rows[-1].tobytes() == want.tobytes() and rows[-1].tobytes() == np.array([e.dye_stats()[k] for k in dye.NAMES] + [0.0] * 4).tobytes()
    # rows r of a call are what vof_dye_stats yields behind the same steps on a twin
    a, b = (flow(hip_api, nx, ny, dtype, ic, warm=12) for _ in range(2))
    a.dye_set(Cd); b.dye_set(Cd)
    rows = a.step_dye(5, 2)
    want = []
    for k in range(5):
        b.step(1); b.dye_advance()
        if k & 1:
            want.append(b.dye_stats())
    assert [dye.raw_of(r) for r in rows] == want and a.istep == 17


def test_a_nan_cell_reads_as_infinite_extrema_and_nan_sums(hip_api):
    e = flow(hip_api, 64, 64, "f64", 1, warm=3)
    Cd = e.get("F")
    Cd[20, 30] = np.nan
    e.dye_set(Cd)
    raw = e.dye_stats()
    assert raw["MAX_C"] == math.inf and raw["MIN_C"] == -math.inf and raw["MAX_EXCESS"] == math.inf
    assert all(math.isnan(raw[k]) for k in ynp.SUMS) and raw["CELLS"] == 64 * 64 and raw["ISTEP"] == 3


# ---------------------------------------------------------------------------- refusals
def test_refusals_leave_the_handle_and_the_dye_alone(hip_api):
    e = flow(hip_api, 64, 64, "f64", 1, warm=2)
    api, h, EINVAL, ESTATE, REL = hip_api, e.handle, _abi.VOF_EINVAL, _abi.VOF_ESTATE, _abi.VOF_RESID_REL
    out = np.zeros((4, _abi.VOF_DYE_N))
    op, done = out.ctypes.data_as(DP), C.c_int64(-1)
    buf = np.zeros((66, 66))
    bp = buf.ctypes.data_as(C.c_void_p)
    # no dye yet
    assert api.dye_advance(h) == ESTATE and api.dye_get(h, bp, buf.nbytes) == ESTATE and api.dye_stats(h, op) == ESTATE
    assert api.step_dye(h, 2, 1, 0, REL, op, 4, C.byref(done)) == ESTATE and e.istep == 2 and done.value == -1
    assert api.dye_set(h, None, 0) == 0                      # nothing to release: fine
    C0 = dyes(e, "box")
    e.dye_set(C0)
    before = {n: e.get(n) for n in FIELDS}
    # sizes and pointers
    assert api.dye_set(h, bp, buf.nbytes - 8) == EINVAL and api.dye_set(h, bp, 0) == EINVAL and api.dye_set(h, None, 8) == EINVAL
    assert api.dye_get(h, bp, buf.nbytes + 8) == EINVAL and api.dye_get(h, None, buf.nbytes) == EINVAL and api.dye_stats(h, None) == EINVAL
    #            nsteps every K crit out cap
    for args in ((4, -1, 0, REL, op, 4), (-1, 1, 0, REL, op, 4), (4, 1, 0, REL, None, 4), (4, 1, 0, REL, op, 3), (4, 1, -1, REL, op, 4), (4, 1, 2, 7, op, 4)):
        assert api.step_dye(h, *args, C.byref(done)) == EINVAL, args
    assert done.value == -1 and not out.any() and e.istep == 2 and same_bytes(e.dye_get(), C0)
    assert all(np.array_equal(e.get(n), before[n]) for n in FIELDS)
    # every == 0 records nothing and needs no out; a bad criterion does not matter without multigrid steps
    assert api.step_dye(h, 1, 0, 0, 7, None, 0, C.byref(done)) == 0 and done.value == 0 and e.istep == 3
    assert api.step_dye(h, 0, 1, 0, REL, None, 0, C.byref(done)) == 0 and done.value == 0 and e.istep == 3
    # a phased step in progress
    kept = e.dye_get()
    e.step_phase(0)
    for call in (e.dye_advance, e.dye_get, e.dye_stats, lambda: e.step_dye(2), lambda: e.dye_set(C0)):
        with pytest.raises(VofError, match="VOF_ESTATE"):
            call()
    e.step_phase(1); e.step_phase(2)
    assert same_bytes(e.dye_get(), kept) and e.istep == 4
    # a strip
    s = engine(hip_api, 128, 128, "f64", "f32", ic=1, rows=(0, 80), own=(1, 60))
    fields = {n: s.get(n) for n in FIELDS}
    for call in (lambda: s.dye_set(np.zeros((130, 130))), s.dye_advance, s.dye_get, s.dye_stats, lambda: s.step_dye(2)):
        with pytest.raises(VofError, match="VOF_ESTATE") as err:
            call()
        assert "whole domain" in str(err.value)
    assert s.istep == 0 and all(np.array_equal(s.get(n), fields[n]) for n in FIELDS)


# ---------------------------------------------------------------------------- the command line
def test_cli_writes_the_dye_files_and_resumes(hip_api, tmp_path, monkeypatch):
    import os

    from vof2d import cli
    monkeypatch.chdir(tmp_path)
    base = ["-ic", "3", "--nx", "64", "--ny", "64", "--dtype", "f64", "--dye-box", "0,0.1,0.05,0.1", "--dye-every", "4", "--dye-save-every", "10", "--depths-every", "10"]
    lines = []
    assert cli.run(cli.parse_args(base + ["--steps", "20", "--save-every", "20"]), api=hip_api, world=1, rank=0,
                   out=lambda *a: lines.append(" ".join(str(x) for x in a))) == 0
    assert any("Dye set" in ln for ln in lines)
    e = engine(hip_api, 64, 64, "f64", "f32", ic=3)
    dx, dy, dt = e.get_param("dx"), e.get_param("dy"), e.get_param("dt")
    e.dye_set(dye.box(e.get("F"), dx, dy, 0.0, 0.1, 0.05, 0.1))
    rows = e.step_dye(20, 4)
    text = open(os.path.join("data", "dye.csv")).read().strip().split("\n")
    assert text[0] == ",".join(("istep", "time") + dye.DERIVED) and len(text) == 6
    for r, line in zip(rows, text[1:]):
        d, k = dye.derive(dye.raw_of(r), dx, dy), int(r[dye.ISTEP])
        assert line == ",".join([str(k), repr(k * dt)] + [repr(float(d[c])) for c in dye.DERIVED])
    assert same_bytes(np.load(os.path.join("data", "dye_000020.npy")), e.dye_get()) and os.path.exists(os.path.join("data", "dye_000010.npy"))
    assert os.path.exists(os.path.join("data", "depths_000020.npy"))
    z = np.load(os.path.join("data", "dye_state.npz"))
    assert int(z["istep"]) == 20 and same_bytes(z["C"], e.dye_get())
    # resumed: the dye beside the checkpoint goes on
    assert cli.run(cli.parse_args(base + ["--steps", "28", "--resume", "data/00000020.npz"]), api=hip_api, world=1, rank=0, out=lambda *a: None) == 0
    e.step_dye(8)
    assert same_bytes(np.load(os.path.join("data", "dye_state.npz"))["C"], z["C"])     # (no --save-every: untouched)
    text = open(os.path.join("data", "dye.csv")).read().strip().split("\n")
    assert len(text) == 8 and text[-1].split(",")[0] == "28"
    d = dye.derive(e.dye_stats(), dx, dy)
    assert text[-1] == ",".join(["28", repr(28 * dt)] + [repr(float(d[c])) for c in dye.DERIVED])
