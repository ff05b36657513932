"""vof_energy and vof_step_energy on the GPU (include/vof2d.h).

vof_energy is held to the NumPy restatement of tests/_energy_np.py applied to the fields read back: ISTEP, CELLS and the maximum with ==,
every sum against math.fsum of the restated terms within n 2^-52 fsum(|t|) (derived in tests/_diag_np.py, not measured) AND, bit for bit,
against the restated order of the reduction with the handle's chunk length.  vof_step_energy is held to its definition, bit for bit: the
loop "step `every` steps; vof_energy" on a twin.  Every figure is printed before it is asserted.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import _curvature_np as cnp
import _energy_np as enp
import _interface_np as inp
import _reduce_np as rnp
from test_step_mg_gpu import FIELDS, assert_same_state
from util import GOLDEN, engine
from vof2d import _abi, energy
from vof2d.engine import VofError

pytestmark = pytest.mark.gpu

TM_GRID = (2048, 2048, "f32", 2)          # vof_step batches its steady-state steps in the k_tm form here (tests/test_step_mg_gpu.py)


def restated(e):
    return enp.restate(e.get("F"), e.get("u"), e.get("v"), e.get("p"), enp.params_of(e))


def hold_to_restatement(e, ctx, bits=True):
    raw = e.energy()
    R = inp.diag_chunk_rows(e.nx, e.ny) if bits else None
    enp.check(raw, restated(e), istep=e.istep, ctx=ctx, say=print, R=R)
    assert len(raw) == len(energy.NAMES)
    return raw


def vec(raw):
    return np.array([raw[k] for k in energy.NAMES] + [0.0] * (_abi.VOF_ENERGY_N - len(energy.NAMES)))


# ---------------------------------------------------------------------------- equal to the restatement
@pytest.mark.parametrize("nx,ny", [(3, 3), (3, 200)])
def test_the_least_rows(hip_api, nx, ny):
    """Three rows: one chunk of two rows and one of one; 3 x 200 has a second column tile.  Random fields: every face and sum is live."""
    e = engine(hip_api, nx, ny, "f64", "f32", ic=1)
    rng = np.random.default_rng(nx * 1000 + ny)
    e.set("F", rng.choice([0.0, 1.0, 0.25, 0.75], size=(nx + 2, ny + 2)))
    for n in ("u", "v", "p"):
        e.set(n, rng.standard_normal((nx + 2, ny + 2)))
    raw = hold_to_restatement(e, "%dx%d f64 random" % (nx, ny))
    assert raw["CELLS"] == nx * ny and raw["KE_U"] > 0 and raw["KE_V"] > 0 and raw["MAX_ACC_SIGMA"] > 0


def test_a_ragged_tile_33x17_f64(hip_api):
    e = engine(hip_api, 33, 17, "f64", "f32", ic=2)
    for upto in (0, 1, 20):
        e.step(upto - e.istep)
        raw = hold_to_restatement(e, "33x17 f64 ic 2 step %d" % upto)
    assert raw["KE_V"] > 0 and raw["P_SIGMA"] != 0 and raw["SUM_GRADF"] > 0


def test_a_second_tile_of_two_columns_96x130_f64(hip_api):
    e = engine(hip_api, 96, 130, "f64", "f32", ic=3, Lx=0.1, Ly=0.13)
    assert e.get_param("dxi") != e.get_param("dyi")
    for upto in (0, 1, 20):
        e.step(upto - e.istep)
        raw = hold_to_restatement(e, "96x130 f64 ic 3 step %d" % upto)
    assert raw["P_GRAV"] != 0 and raw["P_PRES"] != 0


def test_more_partials_than_folding_threads_f64(hip_api):
    """1100 x 130: the rule gives 2-row chunks, so the windows restart every two rows; 550 chunks x 2 tiles = 1100 waves = 275 blocks,
    so threads 0 .. 18 of k_row_finish fold two partials each."""
    nx, ny = 1100, 130
    R = inp.diag_chunk_rows(nx, ny)
    assert R == 2 and rnp.blocks(nx, ny, R) == 275 > 256
    e = engine(hip_api, nx, ny, "f64", "f32", ic=3)
    for upto in (0, 1):
        e.step(upto - e.istep)
        hold_to_restatement(e, "%dx%d f64 ic 3 step %d" % (nx, ny, upto))


@pytest.mark.parametrize("ic", [1, 2, 3])
def test_200_f32_after_0_1_and_50_steps(hip_api, ic):
    e = engine(hip_api, 200, 200, "f32", "f32", ic=ic)
    for upto in (0, 1, 50):
        e.step(upto - e.istep)
        raw = hold_to_restatement(e, "200x200 f32 ic %d step %d" % (ic, upto))
        assert raw["CELLS"] == 200 * 200 and raw["SUM_RHO"] > 0
    assert raw["KE_U"] > 0 and raw["KE_V"] > 0 and raw["P_GRAV"] != 0 and raw["P_VISC"] != 0


def test_a_disc_across_a_tile_seam_and_a_chunk_boundary(hip_api):
    """140 x 260 f64, a painted disc: the faces that gather kappa lie on both sides of the columns 128 | 129 (two wave tiles) and of the rows
    70 | 71 (two chunks of two rows), and the stencils of the gather reach across both."""
    nx, ny = 140, 260
    e = engine(hip_api, nx, ny, "f64", "f32", ic=1)
    dx, dy = e.get_param("dx"), e.get_param("dy")
    F = cnp.disc(nx, ny, dx, dy, 70.5 * dx, 128.5 * dy, 30.3 * dx)
    R = inp.diag_chunk_rows(nx, ny)
    crossed = (F[1:-1, 1:-1] != F[:-2, 1:-1]) | (F[1:-1, 1:-1] != F[1:-1, :-2])        # cells with a face the interface crosses
    assert R == 2 and crossed[:, 127].any() and crossed[:, 128].any()                    # columns 128 and 129
    assert 70 % R == 0 and crossed[69].any() and crossed[70].any()                       # rows 70 (ends a chunk) and 71 (starts one)
    assert crossed[69, :128].any() and crossed[69, 128:].any() and crossed[70, :128].any() and crossed[70, 128:].any()
    rng = np.random.default_rng(7)
    e.set("F", F)
    for n in ("u", "v", "p"):
        e.set(n, rng.standard_normal((nx + 2, ny + 2)))
    raw = hold_to_restatement(e, "140x260 f64 disc")
    assert raw["P_SIGMA"] != 0 and raw["MAX_ACC_SIGMA"] > 0
    print("SUM_GRADF dx dy %r beside the perimeter 2 pi r %r" % (raw["SUM_GRADF"] * dx * dy, 2 * math.pi * 30.3 * dx))       # (a figure, not a check)


# ---------------------------------------------------------------------------- random states
def random_state(rng, nx, ny):
    """F from patches of 0, 1 and mixed values; u, v, p random."""
    F = np.zeros((nx + 2, ny + 2))
    for _ in range(int(rng.integers(1, 6))):
        i0, j0 = int(rng.integers(0, nx + 2)), int(rng.integers(0, ny + 2))
        i1, j1 = i0 + int(rng.integers(1, nx + 2)), j0 + int(rng.integers(1, ny + 2))
        kind = int(rng.integers(0, 3))
        F[i0:i1, j0:j1] = (0.0, 1.0)[kind] if kind < 2 else rng.random((min(i1, nx + 2) - i0, min(j1, ny + 2) - j0))
    return F, rng.standard_normal((nx + 2, ny + 2)), rng.standard_normal((nx + 2, ny + 2)), 100.0 * rng.standard_normal((nx + 2, ny + 2))


def test_thirty_random_states(hip_api):
    rng = np.random.default_rng(20240521)
    for case in range(30):
        nx, ny = int(rng.integers(3, 41)), int(rng.integers(3, 141))
        dtype = ("f64", "f32")[case % 2]
        e = engine(hip_api, nx, ny, dtype, "f32", ic=1)
        for n, a in zip(("F", "u", "v", "p"), random_state(rng, nx, ny)):
            e.set(n, a.astype(np.float32 if dtype == "f32" else np.float64))
        hold_to_restatement(e, "random case %d: %dx%d %s" % (case, nx, ny, dtype))
        e.close()


# ---------------------------------------------------------------------------- a NaN is reported, not hidden
def test_a_nan_reaches_the_sums_whose_terms_hold_it(hip_api):
    e = engine(hip_api, 33, 17, "f64", "f32", ic=2)
    e.step(5)
    u = e.get("u")
    u[20, 9] = np.nan                           # an interior u face
    e.set("u", u)
    raw = e.energy()
    print(raw)
    res = restated(e)
    nan_sums = {k for k in enp.SUMS if np.isnan(enp.flat(res.terms[k])).any()}
    print("sums whose terms hold the NaN:", sorted(nan_sums))
    assert {"KE_U", "P_VISC", "P_ADV", "P_PRES"} <= nan_sums and not nan_sums & {"KE_V", "SUM_RHO", "SUM_RHO_I", "SUM_RHO_J", "SUM_GRADF"}
    assert all(math.isnan(raw[k]) == (k in nan_sums) for k in enp.SUMS)
    enp.check(raw, res, istep=5, ctx="a NaN in u", say=print, R=inp.diag_chunk_rows(33, 17))
    assert raw["MAX_ACC_SIGMA"] == res.amax < math.inf


# ---------------------------------------------------------------------------- the FMA build
WORKER = """
import sys
import numpy as np
sys.path[:0] = [%r, %r]
import _energy_np as enp
import _interface_np as inp
from vof2d._lib import hip_api
from vof2d.engine import Engine, make_desc
api = hip_api(fast=True)
for (nx, ny, dtype, ic) in ((96, 130, "f64", 3), (40, 129, "f32", 2)):
    e = Engine(api, make_desc(api, nx, ny, dtype, "f32"))
    e.set_init_F(ic)
    e.step(20)
    res = enp.restate(e.get("F"), e.get("u"), e.get("v"), e.get("p"), enp.params_of(e))
    enp.check(e.energy(), res, istep=20, ctx="fma build %%dx%%d %%s" %% (nx, ny, dtype), say=print, R=inp.diag_chunk_rows(nx, ny))
    assert any(t.any() for t in res.terms["P_SIGMA"])
print("fma ok")
"""


def test_the_fma_build_gives_the_same_bits(hip_api, tmp_path):
    """On the FMA-contracted library (a process loads one of the two: it runs in a child) the row equals, bit for bit, the restatement fed
    with that build's own read-back fields: nothing inside k_energy is contracted."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = WORKER % (os.path.join(root, "taichi-2d-vof_amd"), os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "fma ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------- behind a k_tm batch
def test_behind_a_k_tm_batch(hip_api):
    nx, ny, dtype, ic = TM_GRID
    e = engine(hip_api, nx, ny, dtype, "f32", ic=ic)
    e.step(40)
    assert e.get_counter("tm_steps") >= 2
    raw = e.energy()                            # first: the handle is ahead, its ghost cells virtual
    enp.check(raw, restated(e), istep=40, ctx="2048x2048 f32 ic 2 behind vof_step(40)", say=print, R=inp.diag_chunk_rows(nx, ny))


# ---------------------------------------------------------------------------- read-only and reproducible
@pytest.mark.parametrize("nx,ny,dtype,ic", [(256, 256, "f64", 1), TM_GRID])
def test_reads_only_and_interleaves_with_vof_step(hip_api, nx, ny, dtype, ic):
    a, b = (engine(hip_api, nx, ny, dtype, "f32", ic=ic) for _ in range(2))
    a.step(7); b.step(7)
    before = {n: a.get(n) for n in FIELDS}
    warn = a.get_counter("courant_violations")
    r1 = a.energy()
    r2 = a.energy()
    assert r1 == r2                             # identical bits (no NaN in this state)
    assert a.istep == 7 and a.get_counter("courant_violations") == warn
    assert all(np.array_equal(a.get(n), before[n]) for n in FIELDS)
    for _ in range(2):
        a.step(7); b.step(7)
        a.energy()
    if (nx, ny, dtype, ic) == TM_GRID:
        assert a.get_counter("tm_steps") >= 2
    assert_same_state(a, b, "%dx%d %s: vof_energy between vof_step(7) calls" % (nx, ny, dtype))


# ---------------------------------------------------------------------------- vof_step_energy held to its definition
def loop_on_a_twin(b, nsteps, every, K=0, crit="rel"):
    rows = []
    for _ in range(nsteps // every):
        b.step_mg(every, K, crit) if K else b.step(every)
        rows.append(vec(b.energy()))
    if nsteps % every:
        b.step_mg(nsteps % every, K, crit) if K else b.step(nsteps % every)
    return np.array(rows).reshape(len(rows), _abi.VOF_ENERGY_N)


@pytest.mark.parametrize("K", [0, 2])
@pytest.mark.parametrize("nsteps,every", [(10, 3), (8, 1), (5, 7)])
@pytest.mark.parametrize("nx,ny,dtype,ic", [(64, 64, "f64", 1), (200, 200, "f32", 3)])
def test_step_energy_is_the_loop_on_a_twin(hip_api, nx, ny, dtype, ic, nsteps, every, K):
    a, b, c = (engine(hip_api, nx, ny, dtype, "f32", ic=ic) for _ in range(3))
    ctx = "%dx%d %s ic %d: step_energy(%d, %d, K = %d)" % (nx, ny, dtype, ic, nsteps, every, K)
    rows = a.step_energy(nsteps, every, K, "rel")
    want = loop_on_a_twin(b, nsteps, every, K)
    print(ctx, "rows", rows.shape, "last", rows[-1] if len(rows) else None)
    assert rows.shape == (nsteps // every, _abi.VOF_ENERGY_N) and rows.dtype == np.float64
    assert np.array_equal(rows, want), ctx
    assert list(rows[:, energy.ISTEP]) == [float(every * (r + 1)) for r in range(nsteps // every)]
    assert not rows[:, len(energy.NAMES):].any()                                 # unused slots read 0
    assert_same_state(a, b, ctx)
    c.step_mg(nsteps, K, "rel") if K else c.step(nsteps)
    assert_same_state(a, c, ctx + " against one call of nsteps")


def test_step_energy_of_no_steps(hip_api):
    e = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    assert e.step_energy(0, 5).shape == (0, _abi.VOF_ENERGY_N) and e.istep == 0
    done = C.c_int64(-1)
    assert hip_api.step_energy(e.handle, 0, 1, 0, _abi.VOF_RESID_REL, None, 0, C.byref(done)) == 0 and done.value == 0


def test_refusals_leave_the_handle_alone(hip_api):
    e = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    e.step(2)
    before = {n: e.get(n) for n in FIELDS}
    out = (C.c_double * (4 * _abi.VOF_ENERGY_N))()
    done = C.c_int64(-1)
    REL = _abi.VOF_RESID_REL
    assert hip_api.energy(e.handle, None) == _abi.VOF_EINVAL
    for args in ((4, 0, 0, REL, out, 4), (4, -1, 0, REL, out, 4), (-1, 1, 0, REL, out, 4), (4, 1, 0, REL, None, 4), (4, 1, 0, REL, out, 3),
                 (4, 1, -1, REL, out, 4), (4, 1, 2, 7, out, 4)):
        assert hip_api.step_energy(e.handle, *args, C.byref(done)) == _abi.VOF_EINVAL, args
    assert e.istep == 2 and all(np.array_equal(e.get(n), before[n]) for n in FIELDS)
    twin = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    twin.step(2)
    assert_same_state(e, twin, "after the refusals")
    # a NULL out does not matter with no row due
    assert hip_api.step_energy(e.handle, 1, 2, 0, REL, None, 0, None) == 0 and e.istep == 3


def test_a_strip_and_a_phased_step_are_refused(hip_api):
    s = engine(hip_api, 128, 128, "f64", "f32", ic=3, rows=(0, 80), own=(1, 60))
    before = {n: s.get(n) for n in FIELDS}
    for call in (s.energy, lambda: s.step_energy(4, 2)):
        with pytest.raises(VofError, match="VOF_ESTATE") as err:
            call()
        assert "whole domain" in str(err.value)
    assert s.istep == 0 and all(np.array_equal(s.get(n), before[n]) for n in FIELDS)
    e = engine(hip_api, 64, 64, "f64", "f32", ic=3)
    e.step(1)
    e.step_phase(0)
    for call in (e.energy, lambda: e.step_energy(4, 2)):
        with pytest.raises(VofError, match="VOF_ESTATE"):
            call()
    e.step_phase(1); e.step_phase(2)
    assert e.energy()["ISTEP"] == 2 == e.istep


def test_vof_curvature_gives_the_bytes_it_gave_before_the_helper_moved(hip_api):
    """tests/golden/curvature/curv_96x130_f64.npz holds the rows and the summary of vof_curvature on the 96 x 130 bubble after 20 steps, recorded with
    the library as it was before KAPPA_CSF moved into kappa_csf (tests/golden/make_curv_golden.py)."""
    with np.load(os.path.join(GOLDEN, "curvature", "curv_96x130_f64.npz")) as z:
        rows0, summ0 = z["rows"], z["summary"]
    e = engine(hip_api, 96, 130, "f64", "f32", ic=3, Lx=0.1, Ly=0.13)
    e.step(20)
    rows, summ = e.curvature()
    from vof2d import curvature
    assert len(rows0) > 100 and rows.tobytes() == rows0.tobytes()
    assert np.array([summ[k] for k in curvature.SUMMARY], dtype=np.float64).tobytes() == summ0.tobytes()


# ---------------------------------------------------------------------------- the command line
def test_cli_writes_the_csv(hip_api, tmp_path, monkeypatch):
    from vof2d import cli
    monkeypatch.chdir(tmp_path)
    argv = ["-ic", "1", "--nx", "64", "--ny", "64", "--dtype", "f64", "--steps", "20", "--energy-every", "5"]
    assert cli.run(cli.parse_args(argv), api=hip_api, world=1, rank=0, out=lambda *a: None) == 0
    text = open(os.path.join(str(tmp_path), "data", "energy.csv")).read().strip().split("\n")
    assert text[0].split(",") == ["istep", "time"] + list(energy.DERIVED) and len(text) == 5
    e = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    consts = (e.get_param("dx"), e.get_param("dy"), e.get_param("gx"), e.get_param("gy"), e.get_param("sigma"))
    for k, line in enumerate(text[1:]):
        e.step(5)
        d = energy.derive(e.energy(), *consts)
        want = [str(5 * (k + 1)), repr(5 * (k + 1) * e.get_param("dt"))] + [repr(float(d[c])) for c in energy.DERIVED]
        assert line.split(",") == want
    assert d["ke"] > 0 and d["pe"] > 0 and d["p_grav"] != 0
    # strips: refused with a message that names the option
    with pytest.raises(SystemExit) as err:
        cli.run(cli.build_parser().parse_args(argv + ["--gpus", "2"]), api=object(), world=2, rank=0, out=lambda *a: None)
    assert "--energy-every" in str(err.value)
