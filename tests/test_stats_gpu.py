"""vof_stats_begin / _sample / _get / _summary and vof_step_stats on the GPU (include/vof2d.h).

One judge: tests/_stats_np.py, the NumPy restatement of a sample, fed with the fields of a twin handle that takes the same
steps and is read back with get_field where the first takes a sample.  Every plane and the summary must equal it byte for byte
(a NaN equals a NaN whatever its sign and payload: the host and the device generate different default NaNs for 0 x inf).

Shapes, from the geometry of k_stats (kernels/stats.h; V = 2 columns a lane for both precisions, vof2d_device.h): a wave's tile
is 64 V = 128 columns, a block's four tiles 512: ny = 127, 128, 129 and 511, 512, 513 -- one below, on and one past either, odd
and even (an odd ny leaves the last lane with one column of the grid and one of the planes' pad).  nx = 64: 32 chunks of 2 rows
by the rule of k_diag; nx = 33: the last chunk has one row, which the two-row loop hands to its one-row tail; knob
stats_chunk_rows = 5: two iterations of the two-row loop and the tail in every chunk, the last chunk shorter.  Square cells
(Ly = Lx ny / nx) and rectangular ones, f64 and f32, -ic 1, 2, 3 after 30 warm steps, 24 steps.  dt = 2e-4, fifty times the
default, so that the front crosses cells within the run.
"""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _stats_np as snp
from test_step_mg_gpu import FIELDS, assert_same_state
from util import engine
from vof2d import _abi, stats
from vof2d.engine import VofError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)
WARM, STEPS, LEVEL, DT = 30, 24, 0.5, 2e-4
EVERY, MASKS = (1, 3, 5), (1, 2, 3)


def consts(nx, ny, sq):
    kw = {"dt": DT}
    if sq:
        kw.update(Lx=0.1, Ly=0.1 * ny / nx)
    return kw


def flow(api, nx, ny, dtype, ic, sq=False, chunk=0, warm=WARM, **kw):
    e = engine(api, nx, ny, dtype, "f32", ic=ic, **consts(nx, ny, sq), **kw)
    if chunk:
        e.set_param("stats_chunk_rows", chunk)
    if warm:
        e.step(warm)
    return e


def fields_of(e):
    return e.get("F"), e.get("u"), e.get("v"), e.istep


def planes_of(e, mask):
    return {p: e.stats_plane(p) for p in stats.planes_of(mask)}


def hold(e, mask, samples, level, ctx):
    """Every plane of `e` and its summary against the restatement fed with `samples`."""
    want, wsum = snp.run(samples, mask, level) if samples else (snp.begin(e.nx, e.ny, mask), snp.summary(snp.begin(e.nx, e.ny, mask), [], mask, level, e.nx, e.ny))
    got = planes_of(e, mask)
    assert sorted(got) == sorted(want), ctx
    for p in got:
        nan = np.isnan(want[p])
        a, b = np.where(nan & np.isnan(got[p]), 0.0, got[p]), np.where(nan, 0.0, want[p])
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
            i, j = bad[0]
            raise AssertionError("%s %s: %d cells differ, first at [%d,%d]: %r vs %r; rows %d..%d cols %d..%d" % (
                ctx, p, len(bad), i, j, a[i, j], b[i, j], bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max()))
    assert e.stats_summary() == wsum, ctx
    return got, wsum


_TWINS = {}


def twin_samples(api, case):
    """(F, u, v, istep) behind every one of the 24 steps of a twin that steps one step at a time; once per case, never changed."""
    if case not in _TWINS:
        nx, ny, dtype, ic, sq, chunk = case
        t = flow(api, nx, ny, dtype, ic, sq)
        out = []
        for _ in range(STEPS):
            t.step(1)
            out.append(fields_of(t))
        t.close()
        _TWINS[case] = out
    return _TWINS[case]


# ---------------------------------------------------------------------------- byte for byte
#        nx  ny   dtype  ic sq     chunk
CASES = [(64, 127, "f64", 1, True, 0), (64, 128, "f32", 2, False, 0), (64, 129, "f64", 3, False, 5), (64, 511, "f32", 3, True, 0),
         (64, 512, "f64", 2, True, 5), (64, 513, "f64", 1, False, 0), (33, 129, "f32", 1, False, 0), (33, 513, "f64", 3, True, 5),
         (64, 513, "f32", 2, False, 5)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%s-ic%d-%s-chunk%d" % (c[0], c[1], c[2], c[3], "sq" if c[4] else "rect", c[5]))
def test_step_stats_equals_the_restatement_byte_for_byte(hip_api, case):
    nx, ny, dtype, ic, sq, chunk = case
    every_step = twin_samples(hip_api, case)
    for every in EVERY:
        samples = [every_step[k] for k in range(every - 1, STEPS - STEPS % every, every)]
        # the twin stepping `every` at a time ends in the same fields as one step at a time (the batches of vof_step give the same bits)
        t = flow(hip_api, nx, ny, dtype, ic, sq)
        t.step(every)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(fields_of(t)[:3], samples[0][:3])) and t.istep == samples[0][3]
        t.close()
        for mask in MASKS:
            ctx = "%dx%d %s ic %d %s chunk %d, every %d mask %d" % (nx, ny, dtype, ic, "square" if sq else "rect", chunk, every, mask)
            e = flow(hip_api, nx, ny, dtype, ic, sq, chunk)
            e.stats_begin(mask, LEVEL)
            assert e.step_stats(STEPS, every) == STEPS // every, ctx
            assert e.istep == WARM + STEPS, ctx
            got, summ = hold(e, mask, samples, LEVEL, ctx)
            assert summ["SAMPLES"] == STEPS // every and summ["ISTEP_FIRST"] == WARM + every and summ["ISTEP_LAST"] == WARM + STEPS - STEPS % every
            if mask & 2:   # properties
                arr = got["ARRIVAL"]
                assert np.array_equal(arr >= 0, got["MAX_F"] >= LEVEL) and (got["WET"] <= summ["SAMPLES"]).all(), ctx
                assert (((arr >= summ["ISTEP_FIRST"]) & (arr <= summ["ISTEP_LAST"])) | (arr == -1)).all(), ctx
                assert summ["EVER_WET"] == (arr >= 0).sum() > 0 and summ["MAX_SPEED2"] == got["MAX_SPEED2"].max() > 0, ctx
            if mask & 1:
                assert (got["SUM_U"] != 0).any() and (got["SUM_UV"] != 0).any() and (got["SUM_F"] > 0).any(), ctx
            e.close()


def test_multigrid_steps_equal_the_restatement(hip_api):
    a, b = (flow(hip_api, 64, 129, "f64", 1, warm=10) for _ in range(2))
    a.stats_begin(3, LEVEL)
    assert a.step_stats(11, 3, 2, "rel") == 3
    samples = []
    for _ in range(3):
        b.step_mg(3, 2, "rel")
        samples.append(fields_of(b))
    b.step_mg(2, 2, "rel")
    hold(a, 3, samples, LEVEL, "step_stats(11, 3, K = 2)")
    assert_same_state(a, b, "step_stats(11, 3, K = 2) against vof_step_mg in groups")
    c = flow(hip_api, 64, 129, "f64", 1, warm=10)
    c.step_mg(11, 2, "rel")
    assert_same_state(a, c, "step_stats(11, 3, K = 2) against vof_step_mg(11)")


def synthetic_F(e, k, rng):
    """A field that makes every branch of a sample live: values below 0, above 1, exactly the level, a front that moves with k."""
    T = e.np_dtype
    F = rng.uniform(-0.25, 1.25, (e.nx + 2, e.ny + 2)).astype(T)
    F[:, : 10 + 7 * k] = T(1.0)
    F[5:9, :] = T(0.5)
    F[20:24, 40:] = T(0.0)
    return F


@pytest.mark.parametrize("dtype,level", [("f64", 0.5), ("f32", 1.0), ("f64", 0.25)])
def test_samples_by_hand_between_the_other_verbs(hip_api, dtype, level):
    """vof_stats_sample only enqueues: between vof_step, vof_step_diag, vof_step_dye, after vof_set_field.  vof_set_field,
    vof_set_init_F and the dye leave the planes alone."""
    nx, ny = 64, 129
    a, b = (flow(hip_api, nx, ny, dtype, 3, warm=6) for _ in range(2))
    rng = np.random.default_rng(7)
    a.stats_begin(3, level)
    hold(a, 3, [], level, "cleared planes")
    samples = []

    def both(call):
        call(a); call(b)

    def sample():
        a.stats_sample()
        samples.append(fields_of(b))

    both(lambda e: e.step(3)); sample()
    both(lambda e: e.step_diag(4, 2)); sample()
    both(lambda e: e.dye_set(e.get("F")))
    both(lambda e: e.step_dye(3, 1)); sample()
    both(lambda e: e.dye_advance())
    hold(a, 3, samples, level, "%s level %g after step, step_diag, step_dye" % (dtype, level))
    for k in range(4):                              # a synthetic front that moves, written from outside; the flow goes on from its own F
        real, F = b.get("F"), synthetic_F(a, k, rng)
        both(lambda e: e.set("F", F)); sample()
        both(lambda e: e.set("F", real))
        both(lambda e: e.step(2)); sample()
    got, summ = hold(a, 3, samples, level, "%s level %g with fields set from outside" % (dtype, level))
    assert len(np.unique(got["ARRIVAL"])) >= 5 and ((got["WET"] > 0) & (got["WET"] < len(samples))).any() and summ["SAMPLES"] == len(samples) == 11
    assert got["MAX_F"].max() == 1.0 and got["MAX_F"].min() >= 0.0
    d = stats.derive(got, summ["SAMPLES"], DT)
    assert all((d[k] >= 0).all() for k in ("F_var", "u_var", "v_var")) and np.isnan(d["arrival_time"]).any() == bool((got["ARRIVAL"] < 0).any())
    # what leaves the statistics alone
    both(lambda e: e.set("u", e.get("u")))
    both(lambda e: e.set_init_F(2))
    both(lambda e: e.dye_set(None))
    hold(a, 3, samples, level, "after vof_set_field, vof_set_init_F and the dye's release")
    a.step(5); b.step(5)
    assert_same_state(a, b, "the steps behind the samples")


def test_every_chunk_length_gives_the_same_bytes(hip_api):
    """Rows a wave marches: the rule's 2, one row (the tail alone), 5, 16 (the length of large grids: eight iterations of the two-row
    loop), 40 (one chunk for the 33 rows)."""
    nx, ny, dtype, ic = 33, 513, "f32", 3
    ref = None
    for chunk in (0, 1, 5, 16, 40):
        e = flow(hip_api, nx, ny, dtype, ic, chunk=chunk, warm=5)
        e.stats_begin(3, LEVEL)
        e.step_stats(6, 2)
        got = planes_of(e, 3)
        if ref is None:
            ref = got
        assert all(got[p].tobytes() == ref[p].tobytes() for p in ref), chunk
        e.close()
    assert (ref["SUM_U"] != 0).any() and (ref["ARRIVAL"] >= 0).any()


# ---------------------------------------------------------------------------- the FMA build
WORKER = """
import sys
import numpy as np
sys.path[:0] = [%r, %r]
import _stats_np as snp
from vof2d import stats
from vof2d._lib import hip_api
from vof2d.engine import Engine, make_desc
api = hip_api(fast=True)
for (nx, ny, dtype, ic) in ((64, 129, "f64", 1), (33, 513, "f32", 3)):
    a, b = (Engine(api, make_desc(api, nx, ny, dtype, "f32", dt=2e-4)) for _ in range(2))
    for e in (a, b):
        e.set_init_F(ic)
        e.step(30)
    a.stats_begin(3, 0.5)
    assert a.step_stats(24, 3) == 8
    samples = []
    for _ in range(8):
        b.step(3)
        samples.append((b.get("F"), b.get("u"), b.get("v"), b.istep))
    want, wsum = snp.run(samples, 3, 0.5)
    for p in stats.PLANES:
        got = a.stats_plane(p)
        assert got.tobytes() == want[p].tobytes(), (nx, ny, dtype, p, int((got.view(np.uint64) != want[p].view(np.uint64)).sum()))
    assert a.stats_summary() == wsum
    assert (want["SUM_UV"] != 0).any()
print("fma ok")
"""


def test_the_fma_build_accumulates_the_same_bits(hip_api, tmp_path):
    """On the FMA-contracted library (a process loads one of the two: it runs in a child) the planes equal the restatement fed
    with that build's own read-back fields: nothing inside k_stats is contracted."""
    code = WORKER % (os.path.join(ROOT, "taichi-2d-vof_amd"), os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fma ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------- invariance
@pytest.mark.parametrize("dtype,ic", [("f64", 1), ("f32", 3)])
def test_the_statistics_leave_the_run_alone(hip_api, dtype, ic):
    a, b = (flow(hip_api, 64, 129, dtype, ic, warm=4) for _ in range(2))
    a.stats_begin(3, LEVEL)
    a.step_stats(23, 4); b.step(23)
    assert_same_state(a, b, "step_stats(23, 4) against vof_step(23)")
    a.step(17); b.step(17)                                  # (batch graphs on both)
    assert_same_state(a, b, "a vof_step behind the statistics")
    a.stats_summary(); a.stats_plane("SUM_F"); a.stats_sample()
    a.step(6); b.step(6)
    assert_same_state(a, b, "a vof_step behind summary, get and sample")
    # a second begin clears; another mask too; 0 releases
    assert a.stats_summary()["SAMPLES"] == 6
    a.stats_begin(3, 0.75)
    hold(a, 3, [], 0.75, "cleared by a second vof_stats_begin")
    a.stats_sample()
    a.stats_begin(2, LEVEL)
    hold(a, 2, [], LEVEL, "cleared by a vof_stats_begin with another mask")
    with pytest.raises(VofError, match="VOF_ESTATE"):
        a.stats_plane("SUM_F")
    a.stats_begin(0, 0.0)
    for call in (a.stats_sample, a.stats_summary, lambda: a.stats_plane("MAX_F"), lambda: a.step_stats(2, 1)):
        with pytest.raises(VofError, match="VOF_ESTATE"):
            call()
    a.stats_begin(0, 0.0)                                   # nothing to release: fine
    assert_same_state(a, b, "begin, clear, release")
    a.stats_begin(1, LEVEL)
    a.stats_sample()
    hold(a, 1, [fields_of(b)], LEVEL, "begun again after a release")


# ---------------------------------------------------------------------------- NaN and infinity
def test_nan_and_infinity_touch_their_own_cells_alone(hip_api):
    nx, ny = 64, 129
    a, b = (flow(hip_api, nx, ny, "f64", 1, warm=5) for _ in range(2))
    clean = fields_of(b)
    F, u, v = (x.copy() for x in clean[:3])
    F[5, 7] = np.nan; u[10, 20] = np.nan; v[15, 128] = np.inf
    for e in (a, b):
        e.set("F", F); e.set("u", u); e.set("v", v)
    a.stats_begin(3, LEVEL)
    a.stats_sample()
    got, summ = hold(a, 3, [fields_of(b)], LEVEL, "a NaN in F and in u, an infinity in v")
    ref, _ = snp.run([clean], 3, LEVEL)
    hit = np.zeros((nx, ny), bool)
    hit[4, 6] = hit[9, 19] = hit[8, 19] = hit[14, 127] = hit[14, 126] = True     # the cell of F; the two cells of the u face; of the v face
    for p in stats.PLANES:
        assert got[p][~hit].tobytes() == ref[p][~hit].tobytes(), p
    for c in ((9, 19), (8, 19)):
        assert all(math.isnan(got[p][c]) for p in ("SUM_U", "SUM_UU", "SUM_UV", "SUM_FU")) and got["MAX_SPEED2"][c] == math.inf
    for c in ((14, 127), (14, 126)):
        assert got["SUM_V"][c] == math.inf and got["SUM_VV"][c] == math.inf and got["MAX_SPEED2"][c] == math.inf
    # the plain clamp of vof_diagnostics takes a NaN F to Fc = 0: not wet, and the F sums of the cell stay finite
    assert got["WET"][4, 6] == 0.0 and got["ARRIVAL"][4, 6] == -1.0 and got["MAX_F"][4, 6] == 0.0 and got["SUM_F"][4, 6] == 0.0
    assert summ["MAX_SPEED2"] == math.inf


# ---------------------------------------------------------------------------- refusals
def test_refusals_leave_planes_counts_and_fields_alone(hip_api):
    e = flow(hip_api, 64, 129, "f64", 1, warm=2)
    api, h, EINVAL, ESTATE, REL = hip_api, e.handle, _abi.VOF_EINVAL, _abi.VOF_ESTATE, _abi.VOF_RESID_REL
    UNTOUCHED = -777.25
    buf = np.full(64 * 129 + 3, UNTOUCHED)
    bp = buf.ctypes.data_as(DP)
    summ = (C.c_double * _abi.VOF_STATS_SUM_N)(*([UNTOUCHED] * _abi.VOF_STATS_SUM_N))
    done = C.c_int64(-1)
    # no statistics yet
    assert api.stats_sample(h) == ESTATE and api.stats_get(h, 0, bp, buf.size) == ESTATE and api.stats_summary(h, summ) == ESTATE
    assert api.step_stats(h, 2, 1, 0, REL, C.byref(done)) == ESTATE and e.istep == 2 and done.value == -1
    assert api.stats_begin(h, 0, 0.5) == 0
    assert api.stats_begin(h, 3, 1.0) == 0 and api.stats_begin(h, 1, LEVEL) == 0          # (level 1 is allowed; a second begin is fine)
    t = flow(hip_api, 64, 129, "f64", 1, warm=2)                                          # the twin takes the steps alone
    e.step_stats(4, 2); t.step(4)
    kept, ksum = planes_of(e, 1), e.stats_summary()
    assert ksum["SAMPLES"] == 2 and (kept["SUM_F"] > 0).any()
    # a bad begin: the old statistics stay
    for mask, level in ((4, 0.5), (-1, 0.5), (7, 0.5), (3, 0.0), (3, -0.5), (3, 1.5), (3, math.nan), (3, math.inf)):
        assert api.stats_begin(h, mask, level) == EINVAL, (mask, level)
    # get: a short cap, an unknown slot, NULL; a slot of the group that is off
    assert api.stats_get(h, 0, bp, 64 * 129 - 1) == EINVAL and api.stats_get(h, 13, bp, buf.size) == EINVAL and api.stats_get(h, -1, bp, buf.size) == EINVAL
    assert api.stats_get(h, 0, None, buf.size) == EINVAL and api.stats_summary(h, None) == EINVAL
    assert api.stats_get(h, _abi.VOF_STATS_ARRIVAL, bp, buf.size) == ESTATE and api.stats_get(h, _abi.VOF_STATS_MAX_F, bp, buf.size) == ESTATE
    assert (buf == UNTOUCHED).all()
    assert api.stats_get(h, _abi.VOF_STATS_SUM_FV, bp, 64 * 129) == 0 and (buf[64 * 129:] == UNTOUCHED).all() and not (buf[:64 * 129] == UNTOUCHED).any()
    #            nsteps every K crit
    for args in ((4, 0, 0, REL), (4, -1, 0, REL), (-1, 1, 0, REL), (4, 1, -1, REL), (4, 1, 2, 7)):
        assert api.step_stats(h, *args, C.byref(done)) == EINVAL, args
    assert done.value == -1 and e.istep == 6
    # a bad criterion does not matter without multigrid steps; samples_taken may be NULL; a remainder alone takes no sample
    assert api.step_stats(h, 1, 2, 0, 7, None) == 0 and e.istep == 7 and api.step_stats(h, 0, 1, 0, REL, C.byref(done)) == 0 and done.value == 0
    t.step(1)
    # a phased step in progress
    e.step_phase(0); t.step_phase(0)
    for call in (e.stats_sample, e.stats_summary, lambda: e.stats_plane(0), lambda: e.step_stats(2, 1), lambda: e.stats_begin(3, LEVEL), lambda: e.stats_begin(0, LEVEL)):
        with pytest.raises(VofError, match="VOF_ESTATE"):
            call()
    for ph in (1, 2):
        e.step_phase(ph); t.step_phase(ph)
    assert e.istep == 8
    now = planes_of(e, 1)
    assert all(now[p].tobytes() == kept[p].tobytes() for p in kept) and e.stats_summary() == ksum
    assert_same_state(e, t, "refused calls")
    # a strip
    s = engine(hip_api, 128, 128, "f64", "f32", ic=1, rows=(0, 80), own=(1, 60))
    fields = {n: s.get(n) for n in FIELDS}
    for call in (lambda: s.stats_begin(3, LEVEL), s.stats_sample, s.stats_summary, lambda: s.stats_plane(0), lambda: s.step_stats(2, 1)):
        with pytest.raises(VofError, match="VOF_ESTATE") as err:
            call()
        assert "whole domain" in str(err.value)
    assert s.istep == 0 and all(np.array_equal(s.get(n), fields[n]) for n in FIELDS)


# ---------------------------------------------------------------------------- the command line
def test_cli_samples_saves_and_writes_the_summary(hip_api, tmp_path, monkeypatch):
    from vof2d import cli
    monkeypatch.chdir(tmp_path)
    argv = ["-ic", "3", "--nx", "64", "--ny", "129", "--dtype", "f64", "--dt", "2e-4", "--steps", "23", "--stats-every", "4", "--stats-from", "6",
            "--stats-save-every", "10", "--diag-every", "5", "--depths-every", "7"]
    lines = []
    assert cli.run(cli.parse_args(argv), api=hip_api, world=1, rank=0, out=lambda *a: lines.append(" ".join(str(x) for x in a))) == 0
    assert any("Statistics begun" in ln for ln in lines)
    b = engine(hip_api, 64, 129, "f64", "f32", ic=3, dt=DT)
    samples = []
    b.step(8); samples.append(fields_of(b))                 # the multiples of 4 from step 6 on: 8, 12, 16, 20
    for _ in range(3):
        b.step(4); samples.append(fields_of(b))
    want, wsum = snp.run(samples, 3, 0.5)
    z = np.load(os.path.join("data", "stats_000023.npz"))
    assert int(z["N"]) == 4 and int(z["istep"]) == 23 and int(z["mask"]) == 3
    for p in stats.PLANES:
        assert z[p].tobytes() == want[p].tobytes(), p
    d = stats.derive(want, 4, DT)
    for k in d:
        assert z[k].tobytes() == d[k].tobytes(), k
    z10 = np.load(os.path.join("data", "stats_000010.npz"))
    assert int(z10["N"]) == 1 and z10["SUM_F"].tobytes() == snp.run(samples[:1], 3, 0.5)[0]["SUM_F"].tobytes()
    assert int(np.load(os.path.join("data", "stats_000020.npz"))["N"]) == 4
    text = open(os.path.join("data", "stats.csv")).read().strip().split("\n")
    assert text[0] == ",".join(("istep", "time") + tuple(k.lower() for k in stats.SUMMARY)) and [ln.split(",")[0] for ln in text[1:]] == ["10", "20", "23"]
    assert text[-1] == ",".join(["23", repr(23 * DT)] + [repr(float(wsum[c])) for c in stats.SUMMARY])
    assert os.path.exists(os.path.join("data", "diagnostics.csv")) and os.path.exists(os.path.join("data", "depths_000021.npy"))
