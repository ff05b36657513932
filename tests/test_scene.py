"""vof_set_scene on the CPU: the NumPy restatement (tests/_scene_np.py, the judge of the GPU tests) held to what the contract of
include/vof2d.h promises, and the host side, vof2d/scene.py.

The area bound.  A closed convex curve crosses at most 2 (W / hx + H / hy) + 4 cells of a grid of spacing hx x hy laid over its
W x H bounding box (each of the W / hx + 1 vertical and H / hy + 1 horizontal grid lines at most twice; a new cell per crossing);
every other sub-cell of size dx/S x dy/S is counted exactly or not at all, and a crossed one is off by at most its own area.  With
the rounding of the extents to whole grid lines: |sum F dx dy - A| <= (2 (W / (dx/S) + H / (dy/S)) + 8) dx dy / S^2.
"""
import json
import math
import os

import numpy as np
import pytest

import _scene_np as snp
from vof2d import _abi, scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes")
SCENES = {"two_drops": (4, 8), "tilted_pool": (2, 16), "column_step": (6, 8)}     # records, samples


def grid(nx, ny, Lx=0.1, Ly=0.1):
    return Lx / nx, Ly / ny


def zeros(nx, ny, dtype=np.float64):
    return np.zeros((nx + 2, ny + 2), dtype=dtype)


# ---------------------------------------------------------------------------- the area bound
@pytest.mark.parametrize("nx,ny,Lx,Ly", [(37, 300, 0.1, 0.1), (64, 48, 0.1, 0.05), (21, 19, 0.1, 0.1)])
@pytest.mark.parametrize("S", [1, 2, 8, 16])
def test_area_of_a_rotated_box_and_ellipse_within_the_bound(nx, ny, Lx, Ly, S):
    dx, dy = grid(nx, ny, Lx, Ly)
    m = min(Lx, Ly)
    hx, hy = 0.3 * m, 0.15 * m
    worst = 0.0
    for (ox, oy, ang) in ((0.0, 0.0, 30.0), (0.031 * m, -0.047 * m, 71.0), (-0.05 * m, 0.05 * m, -12.5)):
        cx, cy = 0.5 * Lx + ox, 0.5 * Ly + oy
        c, s = math.cos(math.radians(ang)), math.sin(math.radians(ang))
        for make, area, W, H in ((scene.box, 4 * hx * hy, 2 * (abs(c) * hx + abs(s) * hy), 2 * (abs(s) * hx + abs(c) * hy)),
                                 (scene.ellipse, math.pi * hx * hy, 2 * math.hypot(c * hx, s * hy), 2 * math.hypot(s * hx, c * hy))):
            assert cx - W / 2 > 0 and cx + W / 2 < Lx and cy - H / 2 > 0 and cy + H / 2 < Ly        # inside the domain
            F, painted, mixed = snp.paint(zeros(nx, ny), scene.pack([make(cx, cy, hx, hy, ang, "liquid")]), S, True, dx, dy)
            bound = (2 * (W / (dx / S) + H / (dy / S)) + 8) * dx * dy / (S * S)
            err = abs(float(F.sum()) * dx * dy - area)
            print("%dx%d S=%d %s at %+.4f %+.4f %g deg: |err| %.3e, bound %.3e (%.2f)" % (nx, ny, S, make.__name__, ox, oy, ang, err, bound, err / bound))
            assert err <= bound
            assert F[0].sum() == 0 and F[-1].sum() == 0 and F[:, 0].sum() == 0 and F[:, -1].sum() == 0 and F.min() >= 0 and F.max() <= 1
            if S > 1:
                assert 0 < mixed < painted == (nx * ny)
            worst = max(worst, err / bound)
    assert worst > 0.0                                  # (the sum is not the exact area: the test would see a bound of the wrong scale)


# ---------------------------------------------------------------------------- painting
DY = (1.0 / 32, 1.0 / 16)     # dyadic spacings: every coordinate below is exact, a sample on a shared edge is on it exactly


@pytest.mark.parametrize("S", [1, 2, 8])
def test_two_rects_that_abut_mid_cell_leave_no_seam(S):
    dx, dy = DY
    nx, ny = 32, 16
    xm, ym = 10.5 * dx, 6.5 * dy                         # through the middle of cells: at S = 1 the sample lies on the line
    whole = scene.pack([scene.rect(3.25 * dx, 20.75 * dx, 2.5 * dy, 11.25 * dy, "liquid")])
    in_x = scene.pack([scene.rect(3.25 * dx, xm, 2.5 * dy, 11.25 * dy, "liquid"), scene.rect(xm, 20.75 * dx, 2.5 * dy, 11.25 * dy, "liquid")])
    in_y = scene.pack([scene.rect(3.25 * dx, 20.75 * dx, 2.5 * dy, ym, "liquid"), scene.rect(3.25 * dx, 20.75 * dx, ym, 11.25 * dy, "liquid")])
    want = snp.paint(zeros(nx, ny), whole, S, True, dx, dy)
    assert want[0].sum() > 0
    for two in (in_x, in_y):
        got = snp.paint(zeros(nx, ny), two, S, True, dx, dy)
        assert got[0].tobytes() == want[0].tobytes() and got[1:] == want[1:]


def test_a_later_shape_overrides_an_earlier_one():
    dx, dy = grid(21, 19)
    liq, gas = scene.disc(0.05, 0.05, 0.03, "liquid"), scene.disc(0.05, 0.05, 0.03, "gas")
    ones = np.ones((23, 21))
    for clear in (True, False):
        F, painted, mixed = snp.paint(ones, scene.pack([liq, gas]), 8, clear, dx, dy)
        only_gas = snp.paint(ones, scene.pack([gas]), 8, clear, dx, dy)
        assert F.tobytes() == only_gas[0].tobytes() and (painted, mixed) == only_gas[1:]
        assert F[11, 10] == 0.0 and (F[1, 1] == 0.0 if clear else F[1, 1] == 1.0)
    F, _, _ = snp.paint(ones, scene.pack([gas, liq]), 8, True, dx, dy)
    assert F[11, 10] == 1.0


def test_a_polygon_is_the_fan_of_its_triangles():
    pts = [(0.02, 0.02), (0.07, 0.03), (0.08, 0.06), (0.05, 0.08), (0.025, 0.06)]
    fan = [scene.triangle(pts[0], pts[k], pts[k + 1], "liquid") for k in range(1, 4)]
    assert scene.polygon(pts, "liquid") == fan
    assert scene.pack([scene.polygon(pts, "liquid")]).tobytes() == scene.pack(fan).tobytes()
    dx, dy = grid(37, 30)
    F, _, _ = snp.paint(zeros(37, 30), scene.pack([scene.polygon(pts)]), 8, True, dx, dy)
    shoelace = 0.5 * abs(sum(pts[k][0] * pts[(k + 1) % 5][1] - pts[(k + 1) % 5][0] * pts[k][1] for k in range(5)))
    assert abs(F.sum() * dx * dy - shoelace) < 0.02 * shoelace and F.max() == 1.0       # (the shared edges of the fan: no seam, no double count)


def test_over_a_fresh_field_clear_changes_nothing_and_an_empty_list_is_the_identity():
    dx, dy = grid(21, 19)
    recs = scene.pack([scene.box(0.05, 0.04, 0.03, 0.01, 20.0), scene.halfplane(0.0, 0.012, 0.0, 1.0), scene.disc(0.08, 0.08, 0.01, "gas")])
    for dtype in (np.float64, np.float32):
        a, b = snp.paint(zeros(21, 19, dtype), recs, 8, False, dx, dy), snp.paint(zeros(21, 19, dtype), recs, 8, True, dx, dy)
        assert a[0].tobytes() == b[0].tobytes() and a[0].dtype == dtype and a[0].max() == 1.0
        assert a[1] < b[1] == 21 * 19                      # PAINTED: the touched cells; with CLEAR every cell
    rng = np.random.default_rng(3)
    F = rng.uniform(-1, 2, (23, 21))
    F[4, 5], F[6, 7] = np.nan, -0.0
    out, painted, mixed = snp.paint(F, scene.pack([]), 16, False, dx, dy)
    assert out.tobytes() == F.tobytes() and (painted, mixed) == (0, 0)
    out, painted, mixed = snp.paint(F, scene.pack([]), 16, True, dx, dy)
    assert out.tobytes() == np.zeros_like(F).tobytes() and (painted, mixed) == (21 * 19, 0)


def test_cells_no_shape_touches_keep_their_bits_and_a_covered_nan_is_gone():
    dx, dy = grid(21, 19)
    F = np.full((23, 21), 0.25)
    F[2, 3], F[3, 3], F[20, 18] = np.nan, -0.0, np.nan     # far from the shape
    F[11, 10] = np.nan                                      # fully covered
    F[11, 16] = 0.5                                         # cut by the edge
    recs = scene.pack([scene.rect(0.03, 0.07, 0.03, 15.5 * dy, "liquid")])
    out, painted, mixed = snp.paint(F, recs, 8, False, dx, dy)
    keep = np.ones_like(F, dtype=bool)
    keep[6:16, 5:17] = False
    assert out[keep].tobytes() == F[keep].tobytes() and np.signbit(out[3, 3]) and np.isnan(out[2, 3])
    assert out[11, 10] == 1.0 and not np.isnan(out[6:16, 5:17]).any()
    assert out[11, 16] == 0.5 * 1.0 + 0.5 * 0.5             # half its samples liquid, half keep the 0.5
    assert mixed > 0 and painted > mixed
    # float32: the value is rounded once
    out32, _, _ = snp.paint(np.full((23, 21), np.float32(0.1)), recs, 8, False, dx, dy)
    assert out32.dtype == np.float32 and out32[11, 16] == np.float32(0.5 + 0.5 * float(np.float32(0.1)))


# ---------------------------------------------------------------------------- the host side
def test_pack_refuses_what_the_library_refuses():
    good = [scene.box(0.05, 0.05, 0.01, 0.02, 30.0), scene.ellipse(0.05, 0.05, 0.0, 0.0), scene.halfplane(0, 0, 0, -1), scene.triangle((0, 0), (0, 0), (0, 0))]
    assert scene.pack(good).shape == (4, _abi.VOF_SHAPE_N) and scene.pack([]).shape == (0, _abi.VOF_SHAPE_N)
    K, P = _abi.VOF_SHAPE_BOX, _abi.VOF_SCENE_LIQUID
    bad = {
        "kind": (7.0, P, 0, 0, 1, 1, 1, 0), "fractional kind": (0.5, P, 0, 0, 1, 1, 1, 0), "phase": (K, 2.0, 0, 0, 1, 1, 1, 0),
        "nan": (K, P, math.nan, 0, 1, 1, 1, 0), "inf": (_abi.VOF_SHAPE_TRIANGLE, P, 0, 0, math.inf, 1, 1, 0),
        "negative hx": (K, P, 0, 0, -1e-9, 1, 1, 0), "negative hy": (_abi.VOF_SHAPE_ELLIPSE, P, 0, 0, 1, -1, 1, 0),
        "not a rotation": (K, P, 0, 0, 1, 1, 1, 1e-4), "zero c, s": (_abi.VOF_SHAPE_ELLIPSE, P, 0, 0, 1, 1, 0, 0),
        "zero normal": (_abi.VOF_SHAPE_HALFPLANE, P, 0.1, 0.1, 0.0, -0.0, 0, 0), "short": (K, P, 0, 0, 1, 1, 1),
    }
    for why, rec in bad.items():
        with pytest.raises(ValueError):
            scene.pack([good[0], rec])
    assert scene.pack([(K, P, 0, 0, 1, 1, math.cos(0.3), math.sin(0.3))]).shape == (1, 8)
    with pytest.raises(ValueError):
        scene.pack([good[0]] * (_abi.VOF_SCENE_MAX_SHAPES + 1))
    assert len(scene.pack([good[0]] * _abi.VOF_SCENE_MAX_SHAPES)) == _abi.VOF_SCENE_MAX_SHAPES
    for s in (0, 3, 32, -1, 2.5, True):
        with pytest.raises(ValueError):
            scene.check_samples(s)
    with pytest.raises(ValueError, match="plasma"):
        scene.box(0, 0, 1, 1, 0, "plasma")
    # rect is the axis-aligned box, the right angles are exact
    assert scene.rect(0.25, 0.75, 1.0, 2.0, "gas") == (0.0, 0.0, 0.5, 1.5, 0.25, 0.5, 1.0, 0.0)
    assert scene.box(0, 0, 1, 2, 90.0)[6:] == (0.0, 1.0) and scene.box(0, 0, 1, 2, -180.0)[6:] == (-1.0, 0.0)
    assert scene.disc(1, 2, 3, "gas") == (1.0, 0.0, 1.0, 2.0, 3.0, 3.0, 1.0, 0.0)


def test_loads_names_what_it_does_not_know():
    ok = '{"samples": 4, "shapes": [{"kind": "disc", "phase": "liquid", "cx": 0.05, "cy": 0.05, "r": 0.01}]}'
    recs, samples = scene.loads(ok)
    assert samples == 4 and recs.tobytes() == scene.pack([scene.disc(0.05, 0.05, 0.01, "liquid")]).tobytes()
    assert scene.loads('{"shapes": []}')[1] == 8
    for text, name in (('{"shapes": [{"kind": "blob", "phase": "gas"}]}', "blob"), ('{"shapes": [], "sample": 4}', "sample"),
                       ('{"shapes": [{"kind": "disc", "phase": "liquid", "cx": 0, "cy": 0, "r": 1, "radius": 2}]}', "radius"),
                       ('{"shapes": [{"kind": "disc", "phase": "solid", "cx": 0, "cy": 0, "r": 1}]}', "solid"),
                       ('{"shapes": [{"kind": "disc", "phase": "gas", "cx": 0, "cy": 0}]}', "'r'"),
                       ('{"samples": 3, "shapes": []}', "3"), ('{"samples": 8}', "shapes")):
        with pytest.raises(ValueError, match=name):
            scene.loads(text)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_example_scenes_load_and_round_trip(name):
    path = os.path.join(GOLDEN, name + ".json")
    recs, samples = scene.load(path)
    assert (len(recs), samples) == SCENES[name] and recs.dtype == np.float64
    doc = json.load(open(path))
    again, samples2 = scene.loads(json.dumps(doc))
    assert again.tobytes() == recs.tobytes() and samples2 == samples
    assert scene.pack(recs).tobytes() == recs.tobytes()                 # the packed array passes through, checked again
    by_hand = scene.pack([scene.shape_of(s) for s in doc["shapes"]])
    assert by_hand.tobytes() == recs.tobytes()
    # the scene holds both phases and paints a state with liquid, gas and an interface on the default domain
    dx, dy = grid(64, 64)
    F, painted, mixed = snp.paint(zeros(64, 64), recs, samples, True, dx, dy)
    assert {int(r[1]) for r in recs} == {0, 1} and painted == 64 * 64 and 0 < mixed < painted and F.max() == 1.0 and F.min() == 0.0
