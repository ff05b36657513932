"""vof_set_scene on the GPU (include/vof2d.h): F and its sweep twin against tests/_scene_np.py, the NumPy restatement, byte for
byte on every stored cell, ghost cells included (a NaN equals a NaN whatever its sign and payload: a cell that keeps some of its
samples of a NaN F_old is a NaN on both sides, and the host and the device need not agree on which).

Shapes, from the geometry of k_scene (kernels/scene.h): one lane per stored cell, blocks of 256 columns over j = 0 .. ny + 1, one
grid row per stored row.  37 x 300: 302 columns are two blocks, the second partial (46 lanes: its last wave is cut too), 39 rows;
5 x 3: one partial wave, the smallest grid the library makes; 64 x 48 with Ly = Lx / 2: square cells, one block.  S = 1 (no
shortcut, one bit), 8 (one group of 64 bits), 16 (four groups, the shortcuts per group).  The sample counts of the restatement are
computed once per (grid, spacing, S) and shared by the fields, flags and tests that need them.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _scene_np as snp
from test_step_mg_gpu import FIELDS, assert_same_state
from util import engine
from vof2d import _abi, scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scenes")
DP = C.POINTER(C.c_double)

#        nx  ny   Ly    coord_cast
GRIDS = [(37, 300, 0.1, "f32"), (5, 3, 0.1, "f32"), (64, 48, 0.05, "f32"), (37, 300, 0.1, "none"), (5, 3, 0.1, "none")]
SAMPLES = (1, 8, 16)


def the_scene(nx, ny, Lx, Ly, dx, dy):
    """One list with every kind; a rotated box and a rotated ellipse; overlapping shapes; two rects that abut mid-cell; LIQUID under
    GAS; a disc smaller than a sample spacing strictly inside a cell, centred on a sample of S = 8 (and on none of S = 16); a shape
    wholly outside the domain; an ellipse that reaches into all four ghost bands; a zero-extent box on a cell centre (a sample of
    S = 1 alone); a zero-area triangle; a half-plane through cell corners (samples of every even S lie on it)."""
    xm = (int(0.3 * nx) + 0.5) * dx
    tiny_x, tiny_y = (0.0 + (3 + 0.5) * 0.125) * dx, (0.0 + (5 + 0.5) * 0.125) * dy      # sample (3, 5) of cell (1, 1) at S = 8
    ci, cj = max(nx // 2, 1), max(ny - 1, 1)
    return scene.pack([
        scene.ellipse(0.5 * Lx, 0.5 * Ly, 0.5 * Lx + 0.6 * dx, 0.5 * Ly + 0.6 * dy, 0.0, "liquid"),
        scene.box(0.45 * Lx, 0.55 * Ly, 0.2 * Lx, 0.1 * Ly, 33.0, "gas"),
        scene.ellipse(0.55 * Lx, 0.5 * Ly, 0.15 * Lx, 0.07 * Ly, -20.0, "liquid"),
        scene.rect(0.2 * Lx, xm, 0.7 * Ly, 0.8 * Ly, "gas"),
        scene.rect(xm, 0.4 * Lx, 0.7 * Ly, 0.8 * Ly, "gas"),
        scene.disc(tiny_x, tiny_y, min(dx, dy) / 40.0, "liquid"),
        scene.disc(-3.0 * Lx, 0.5 * Ly, 0.2 * Lx, "liquid"),
        scene.disc(0.5 * Lx, 7.0 * Ly, 0.3 * Ly, "gas"),
        scene.box(((ci - 1) + 0.5) * dx, ((cj - 1) + 0.5) * dy, 0.0, 0.0, 0.0, "gas"),
        scene.triangle((0.1 * Lx, 0.1 * Ly), (0.2 * Lx, 0.2 * Ly), (0.3 * Lx, 0.3 * Ly), "gas"),
        scene.triangle((0.05 * Lx, 0.6 * Ly), (0.25 * Lx, 0.65 * Ly), (0.1 * Lx, 0.95 * Ly), "liquid"),
        scene.polygon([(0.7 * Lx, 0.1 * Ly), (0.9 * Lx, 0.12 * Ly), (0.85 * Lx, 0.3 * Ly), (0.72 * Lx, 0.25 * Ly)], "gas"),
        scene.halfplane((nx - 2) * dx, ny * dy, -dy, -dx, "liquid"),
    ])


def make(api, nx, ny, Ly, cast, dtype, **kw):
    return engine(api, nx, ny, dtype, cast, Lx=0.1, Ly=Ly, **kw)


def spacing(e):
    return e.get_param("dx"), e.get_param("dy")


_SAMPLED = {}


def sampled(recs, S, dx, dy, rows, ncols):
    key = (recs.tobytes(), S, dx, dy, int(rows[0]), len(rows), ncols)
    if key not in _SAMPLED:
        _SAMPLED[key] = snp.counts(recs, S, dx, dy, rows, ncols)
    return _SAMPLED[key]


def restated(e, base, recs, S, clear):
    dx, dy = spacing(e)
    rows = e.row_lo + np.arange(e.nrows)
    rep = (max(e.own_lo, 1, e.row_lo + 1), min(e.own_hi, e.nx, e.row_hi - 1))
    return snp.paint(base, recs, S, clear, dx, dy, e.row_lo, rep, sampled(recs, S, dx, dy, rows, e.ny + 2))


def same_bytes(got, want, ctx):
    nan = np.isnan(want)
    a, b = np.where(nan & np.isnan(got), 0, got), np.where(nan, 0, want)
    if a.tobytes() != b.tobytes():
        u = np.uint64 if got.dtype == np.float64 else np.uint32
        bad = np.argwhere(a.view(u) != b.view(u))
        i, j = bad[0]
        raise AssertionError("%s: %d cells differ, first at [%d,%d]: %r vs %r; rows %d..%d cols %d..%d" % (
            ctx, len(bad), i, j, got[i, j], want[i, j], bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max()))


def rough_field(e, seed):
    """Values inside and outside [0, 1] with NaN and -0.0 cells sprinkled over untouched, covered and cut cells alike."""
    rng = np.random.default_rng(seed)
    F = rng.uniform(-0.2, 1.2, (e.nrows, e.ny + 2))
    flat = F.reshape(-1)
    flat[::7] = np.nan
    flat[3::11] = -0.0
    return F.astype(e.np_dtype)


def hold(e, base, recs, S, clear, ctx):
    """Paint with the shortcuts on and off: both equal the restatement, F and twin, and so does the summary."""
    want, painted, mixed = restated(e, base, recs, S, clear)
    for shortcuts in (1, 0):
        e.set("F", base)
        e.set_param("scene_shortcuts", shortcuts)
        assert e.get_param("scene_shortcuts") == shortcuts
        summ = e.set_scene(recs, S, clear)
        c2 = "%s shortcuts %d" % (ctx, shortcuts)
        same_bytes(e.get("F"), want, c2 + " F")
        same_bytes(e.get("F2"), want, c2 + " twin")
        assert summ == {"SHAPES": float(len(recs)), "SAMPLES": float(S), "PAINTED": float(painted), "MIXED": float(mixed), "ISTEP": float(e.istep)}, c2
    return want, painted, mixed


# ---------------------------------------------------------------------------- byte for byte
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d-Ly%g-%s" % g)
def test_set_scene_equals_the_restatement_byte_for_byte(hip_api, grid, dtype):
    nx, ny, Ly, cast = grid
    e = make(hip_api, nx, ny, Ly, cast, dtype, ic=3)
    dx, dy = spacing(e)
    recs = the_scene(nx, ny, 0.1, Ly, dx, dy)
    assert {int(r[0]) for r in recs} == {0, 1, 2, 3} and len(recs) == 14
    ic3 = e.get("F")
    rough = rough_field(e, 5)
    for S in SAMPLES:
        for clear in (True, False):
            for name, base in (("ic3", ic3), ("rough", rough)):
                ctx = "%dx%d Ly %g %s %s S %d clear %d over %s" % (nx, ny, Ly, cast, dtype, S, clear, name)
                want, painted, mixed = hold(e, base, recs, S, clear, ctx)
                if clear:
                    assert painted == nx * ny and not np.isnan(want).any(), ctx
                else:
                    assert painted < nx * ny or nx < 8, ctx
                if S > 1 and nx > 8:
                    assert 0 < mixed < painted and (want == 1).any() and (want == 0).any(), ctx
    e.close()


def test_the_small_features_are_neither_dropped_nor_invented(hip_api):
    """The disc smaller than a sample spacing shows in its one sample at S = 8 and in none at S = 16; the zero-extent box takes the one
    sample of S = 1 that lies on it; the shape outside the domain paints nothing."""
    nx, ny = 37, 300
    e = make(hip_api, nx, ny, 0.1, "none", "f64")
    dx, dy = spacing(e)
    recs = the_scene(nx, ny, 0.1, 0.1, dx, dy)
    e.set_scene(recs, 8, True)
    assert e.get("F")[1, 1] == 1.0 / 64
    e.set_scene(recs, 16, True)
    assert e.get("F")[1, 1] == 0.0
    e.set_scene(recs, 1, True)
    F = e.get("F")
    assert F[nx // 2, ny - 1] == 0.0 and F[nx // 2 + 1, ny - 1] == 1.0 and F[nx // 2 - 1, ny - 1] == 1.0        # a hole of one cell in the liquid
    summ = e.set_scene([scene.disc(-0.3, 0.05, 0.02, "liquid"), scene.disc(0.05, 0.7, 0.03, "liquid")], 8, False)
    assert summ["PAINTED"] == 0 and summ["MIXED"] == 0 and e.get("F").tobytes() == F.tobytes()
    # an empty list: the identity without CLEAR, an empty domain with it
    assert e.set_scene([], 16, False) == {"SHAPES": 0.0, "SAMPLES": 16.0, "PAINTED": 0.0, "MIXED": 0.0, "ISTEP": 0.0}
    assert e.get("F").tobytes() == F.tobytes()
    assert e.set_scene([], 4, True)["PAINTED"] == nx * ny and not e.get("F").any() and not e.get("F2").any()
    e.close()


def test_the_longest_list_and_every_sample_count(hip_api):
    """1024 shapes (the list is read with a wave-uniform index to its end), S = 2 and 4 as well."""
    nx, ny = 21, 130
    e = make(hip_api, nx, ny, 0.1, "f32", "f64", ic=2)
    dx, dy = spacing(e)
    rng = np.random.default_rng(11)
    shapes = []
    for k in range(_abi.VOF_SCENE_MAX_SHAPES):
        x, y, r, ang = rng.uniform(0, 0.1), rng.uniform(0, 0.1), rng.uniform(0.001, 0.01), rng.uniform(-180, 180)
        phase = "liquid" if k % 3 else "gas"
        shapes.append((scene.disc(x, y, r, phase), scene.box(x, y, r, 2 * r, ang, phase), scene.halfplane(x, y, r - 0.005, 0.004, phase) if k % 64 == 0 else
                       scene.ellipse(x, y, 2 * r, r, ang, phase), scene.triangle((x, y), (x + 3 * r, y + r), (x - r, y + 2 * r), phase))[k % 4])
    recs = scene.pack(shapes)
    base = e.get("F")
    for S, n in ((2, 1024), (4, 1024), (8, 300)):
        hold(e, base, recs[:n], S, False, "%d shapes S %d" % (n, S))
    e.close()


# ---------------------------------------------------------------------------- refusals, and what a call leaves alone
def test_refusals_change_nothing_and_a_valid_call_leaves_u_v_p_alone(hip_api):
    nx, ny = 37, 300
    e = make(hip_api, nx, ny, 0.1, "f32", "f64", ic=3)
    rng = np.random.default_rng(2)
    for n in ("u", "v", "p"):
        e.set(n, rng.uniform(-1, 1, (nx + 2, ny + 2)))
    before = {n: e.get(n) for n in FIELDS + ("F2",)}
    api, h, EINVAL = hip_api, e.handle, _abi.VOF_EINVAL
    good = scene.pack([scene.box(0.05, 0.05, 0.02, 0.01, 30.0, "liquid"), scene.halfplane(0.0, 0.02, 0.0, 1.0, "liquid")])
    summ = (C.c_double * _abi.VOF_SCENE_SUM_N)(*([-7.0] * _abi.VOF_SCENE_SUM_N))

    def call(recs, n, S, flags):
        a = np.ascontiguousarray(recs, dtype=np.float64) if recs is not None else None
        return api.set_scene(h, a.ctypes.data_as(DP) if a is not None else None, n, S, flags, summ)

    def with_(k, c, x):
        r = good.copy()
        r[k, c] = x
        return r

    assert call(good, -1, 8, 0) == EINVAL and call(good, _abi.VOF_SCENE_MAX_SHAPES + 1, 8, 0) == EINVAL and call(None, 2, 8, 0) == EINVAL
    for S in (0, 3, 32, -8):
        assert call(good, 2, S, 1) == EINVAL, S
    for flags in (2, 3, -1):
        assert call(good, 2, 8, flags) == EINVAL, flags
    bad = [with_(1, 0, 4.0), with_(0, 0, -1.0), with_(0, 1, 2.0), with_(1, 1, 0.5), with_(0, 4, -0.01), with_(0, 5, -1.0), with_(0, 6, 0.9), with_(0, 7, 0.6),
           with_(1, 5, 0.0), with_(0, 2, np.nan), with_(1, 3, np.inf), with_(1, 7, -np.inf), with_(0, 0, np.nan)]
    for k, recs in enumerate(bad):
        assert call(recs, 2, 8, 1) == EINVAL, k
        assert api.last_error(h), k
    assert list(summ) == [-7.0] * _abi.VOF_SCENE_SUM_N
    for n in before:
        assert e.get(n).tobytes() == before[n].tobytes(), n
    assert call(good, 2, 8, 1) == 0 and summ[_abi.VOF_SCENE_SUM_PAINTED] == nx * ny and summ[5] == 0.0
    assert api.set_scene(h, good.ctypes.data_as(DP), 2, 8, 0, None) == 0                        # (no summary asked for)
    for n in ("u", "v", "p"):
        assert e.get(n).tobytes() == before[n].tobytes(), n
    assert e.get("F").tobytes() != before["F"].tobytes() and e.get("F").tobytes() == e.get("F2").tobytes()
    e.close()


# ---------------------------------------------------------------------------- strips
@pytest.mark.parametrize("cuts", [((1, 15, 0, 20), (16, 37, 11, 38)), ((1, 9, 0, 13), (10, 30, 6, 33), (31, 37, 27, 38))], ids=["two", "three"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_strips_hold_the_rows_of_the_whole_domain_and_their_counts_add_up(hip_api, cuts, dtype):
    nx, ny = 37, 300
    whole = make(hip_api, nx, ny, 0.1, "f32", dtype, ic=3)
    dx, dy = spacing(whole)
    recs = the_scene(nx, ny, 0.1, 0.1, dx, dy)
    for S, clear in ((8, False), (16, True)):
        whole.set_init_F(3)
        total = whole.set_scene(recs, S, clear)
        F = whole.get("F")
        painted = mixed = 0
        for (own_lo, own_hi, row_lo, row_hi) in cuts:
            s = make(hip_api, nx, ny, 0.1, "f32", dtype, ic=3, rows=(row_lo, row_hi), own=(own_lo, own_hi))
            assert spacing(s) == (dx, dy)
            summ = s.set_scene(recs, S, clear)
            same_bytes(s.get("F"), F[row_lo:row_hi + 1], "strip %d..%d S %d" % (row_lo, row_hi, S))
            same_bytes(s.get("F2"), F[row_lo:row_hi + 1], "strip %d..%d S %d twin" % (row_lo, row_hi, S))
            want = restated(s, whole_base(hip_api, nx, ny, dtype)[row_lo:row_hi + 1], recs, S, clear)
            assert (summ["PAINTED"], summ["MIXED"]) == want[1:]
            painted += summ["PAINTED"]; mixed += summ["MIXED"]
            s.close()
        assert (painted, mixed) == (total["PAINTED"], total["MIXED"]) and mixed > 0
    whole.close()


_BASE = {}


def whole_base(api, nx, ny, dtype):
    if (nx, ny, dtype) not in _BASE:
        e = make(api, nx, ny, 0.1, "f32", dtype, ic=3)
        _BASE[(nx, ny, dtype)] = e.get("F")
        e.close()
    return _BASE[(nx, ny, dtype)]


def test_strip_solver_paints_its_strip_and_is_fresh(hip_api, tmp_path):
    from vof2d.comms import EnvComm
    from vof2d.strips import StripSolver
    s = StripSolver(64, 48, "f64", ic=1, api=hip_api, comm=EnvComm(rank=0, world=1, rdzv_dir=str(tmp_path)), Lx=0.1, Ly=0.05)   # (the torch-free carrier)
    s._fresh = False
    recs, S = scene.load(os.path.join(GOLDEN, "two_drops.json"))
    summ = s.set_scene(recs, S, True)
    assert s._fresh and summ["PAINTED"] == 64 * 48
    dx, dy = spacing(s.eng)
    want, _, _ = snp.paint(np.zeros((66, 50)), recs, S, True, dx, dy)
    same_bytes(s.eng.get("F"), want, "StripSolver.set_scene")
    s.close()


def test_the_strip_driver_of_the_command_line_paints_and_adds_the_counts_up(hip_api, tmp_path):
    """What `2dvof.py --gpus N --scene FILE` runs on every rank (cli._Strips.paint_scene), here with one rank and the torch-free carrier."""
    from vof2d import cli
    from vof2d.comms import EnvComm
    path = os.path.join(GOLDEN, "column_step.json")
    args = cli.parse_args(["--scene", path, "--nx", "64", "--ny", "48", "--dtype", "f32", "-ic", "3"])
    drv = cli._Strips(args, hip_api, EnvComm(rank=0, world=1, rdzv_dir=str(tmp_path)), 0, 1)
    before = drv.eng.get("F")
    drv.s._fresh = False
    got = drv.paint_scene(args.scene_shapes, args.scene_samples, False)
    want, painted, mixed = snp.paint(before, args.scene_shapes, args.scene_samples, False, *spacing(drv.eng))
    assert got == (painted, mixed) and mixed > 0 and drv.s._fresh
    same_bytes(drv.eng.get("F"), want, "cli._Strips.paint_scene")
    drv.close()


# ---------------------------------------------------------------------------- the first step
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("clear", [True, False])
def test_the_first_steps_equal_those_of_the_same_state_uploaded(hip_api, dtype, clear):
    """Ghost cells and state as after vof_set_field: vof_step(3) gives the same F, u, v, p either way -- also on a handle that has
    stepped before (ghost cells virtual, batch graphs built)."""
    nx, ny, Ly = 64, 48, 0.05
    a, b, c = (make(hip_api, nx, ny, Ly, "f32", dtype, ic=3) for _ in range(3))
    dx, dy = spacing(a)
    recs = the_scene(nx, ny, 0.1, Ly, dx, dy)
    c.set_scene(recs, 8, clear)
    b.set("F", c.get("F"))
    a.set_scene(recs, 8, clear)
    a.step(3); b.step(3)
    assert_same_state(a, b, "set_scene + vof_step(3) against set_field + vof_step(3)")
    a.step(20); b.step(20)
    b.set_scene(recs[:5], 16, False)                       # painted over the moving state, no field read in front of it
    c.set("F", a.get("F"))
    c.set_scene(recs[:5], 16, False)
    a.set("F", c.get("F"))
    a.step(3); b.step(3)
    for n in ("F", "u", "v", "p"):
        assert a.get(n).tobytes() == b.get(n).tobytes(), n
    assert a.istep == b.istep == 26
    for e in (a, b, c):
        e.close()


def test_vof2d_set_scene(hip_api):
    from vof2d.solver import VOF2D
    sim = VOF2D(64, 48, dtype="f32", api=hip_api, Lx=0.1, Ly=0.05)
    recs, S = scene.load(os.path.join(GOLDEN, "tilted_pool.json"))
    summ = sim.set_scene(recs, S, clear=True)
    want, painted, mixed = snp.paint(np.zeros((66, 50), np.float32), recs, S, True, sim.dx, sim.dy)
    same_bytes(sim.eng.get("F"), want, "VOF2D.set_scene")
    assert (summ["PAINTED"], summ["MIXED"]) == (painted, mixed)


# ---------------------------------------------------------------------------- the FMA build
WORKER = """
import sys
import numpy as np
sys.path[:0] = [%r, %r]
import _scene_np as snp
import test_scene_gpu as t
from vof2d._lib import hip_api
api = hip_api(fast=True)
for (nx, ny, Ly, cast, dtype) in ((37, 300, 0.1, "none", "f64"), (64, 48, 0.05, "f32", "f32")):
    e = t.make(api, nx, ny, Ly, cast, dtype, ic=3)
    dx, dy = t.spacing(e)
    recs = t.the_scene(nx, ny, 0.1, Ly, dx, dy)
    base = t.rough_field(e, 9)
    for S in (8, 16):
        want, painted, mixed = t.hold(e, base, recs, S, False, "fma %%dx%%d %%s S %%d" %% (nx, ny, dtype, S))
        assert mixed > 0
print("fma ok")
"""


def test_the_fma_build_paints_the_same_bytes(hip_api):
    """On the FMA-contracted library (a process loads one of the two: it runs in a child) the bytes equal the restatement's: no
    product of k_scene is contracted."""
    code = WORKER % (os.path.join(ROOT, "taichi-2d-vof_amd"), os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fma ok" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------- the command line
def test_cli_paints_the_scene_and_runs(hip_api, tmp_path, monkeypatch):
    from vof2d import cli
    monkeypatch.chdir(tmp_path)
    at_step_0 = []
    paint = cli._Single.paint_scene

    def spy(self, *a):
        out = paint(self, *a)
        at_step_0.append((self.eng.get("F"), self.eng.istep))
        return out

    monkeypatch.setattr(cli._Single, "paint_scene", spy)
    path = os.path.join(GOLDEN, "column_step.json")
    lines = []
    argv = ["--scene", path, "--nx", "64", "--ny", "64", "--dtype", "f64", "--steps", "2", "--save-every", "2"]
    assert cli.run(cli.parse_args(argv), api=hip_api, world=1, rank=0, out=lambda *a: lines.append(" ".join(str(x) for x in a))) == 0
    recs, S = scene.load(path)
    b = engine(hip_api, 64, 64, "f64", "f32")
    want, painted, mixed = snp.paint(np.zeros((66, 66)), recs, S, True, *spacing(b))
    assert len(at_step_0) == 1 and at_step_0[0][1] == 0
    same_bytes(at_step_0[0][0], want, "F at step 0")
    said = [ln for ln in lines if "Scene" in ln]
    assert len(said) == 1 and "painted %d cells, %d of them mixed" % (painted, mixed) in said[0]
    b.set("F", want)
    b.step(2)
    z = np.load(os.path.join("data", "%08d.npz" % 2))
    assert z["F"].tobytes() == b.get("F").tobytes() and z["u"].tobytes() == b.get("u").tobytes()
    # over -ic 3 with the file's samples overridden
    at_step_0.clear()
    argv = ["--scene", path, "--scene-over-ic", "-ic", "3", "--scene-samples", "2", "--nx", "64", "--ny", "64", "--dtype", "f64", "--steps", "1"]
    assert cli.run(cli.parse_args(argv), api=hip_api, world=1, rank=0, out=lambda *a: None) == 0
    c = engine(hip_api, 64, 64, "f64", "f32", ic=3)
    same_bytes(at_step_0[0][0], snp.paint(c.get("F"), recs, 2, False, *spacing(c))[0], "F at step 0 over -ic 3")
