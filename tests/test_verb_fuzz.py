"""The generators of the verb fuzz judged on the CPU (tests/_verb_fuzz.py; the device leg is tests/test_verb_fuzz_gpu.py).

The fixed-seed slice is replayed through the restatements alone -- the fields of a case are drawn (a flow state comes from the CPU
oracle, which vof_step equals bit for bit), the comparisons of the restatements are formed again and counted on either side of
equality -- and must reach every tie, kind, family, capacity class, strip and boundary grid it claims to.  The counts are printed
and stand in the assertion messages: this test fixes the size of the slice from below.

The restatements themselves are judged on the new inputs (lattice and edge fields, where ties are the rule) by the
definition-level judges of tests/test_*.py, taken to those fields: the PLIC line that cuts off the area F, the naive statistics,
a second labelling, the depth of a column counted cell by cell, the colour index by the header's words one pixel at a time.
"""
import collections
import math

import numpy as np
import pytest

import _blobs_np as bnp
import _depths_np as dpn
import _frames_np as fnp
import _interface_np as inp
import _scene_np as scn
import _stats_np as stn
import _tracers_np as tnp
import _verb_fuzz as vf

_CENSUS = {}


def census(api):
    """The counts of the whole committed slice, once per session."""
    if not _CENSUS:
        c = collections.Counter()
        consts = {}
        for leg in "ABC":
            for seed in vf.slice_seeds(leg):
                case = vf.DRAW[leg](seed)
                g = case["grid"]
                key = (g["nx"], g["ny"], g["dtype"], g["cast"], tuple(sorted(g["kw"].items())))
                if key not in consts:
                    e = vf.make(api, g)
                    consts[key] = vf.consts_of(e)
                    e.close()
                k = consts[key]
                if leg == "A":
                    vf.census_a(c, case, vf.fields_of(api, case), k, vf.positions_of(case, k)[0])
                elif leg == "B":
                    vf.census_b(c, case)
                else:
                    vf.census_c(c, case, k, vf.scene_of(case, k))
        _CENSUS["c"] = c
        for name in sorted(c):
            print("%-55s %d" % (name, c[name]))
    return _CENSUS["c"]


def need(c, names, what):
    missing = [n for n in names if c[n] == 0]
    assert not missing, "%s the slice does not reach: %s; the counts: %s" % (what, missing, {n: c[n] for n in names})


def test_the_generator_is_deterministic():
    for leg in "ABC":
        a, b = vf.DRAW[leg](vf.SEED0 + 3), vf.DRAW[leg](vf.SEED0 + 3)
        assert a == b and vf.describe(a) == vf.describe(b)
        assert vf.DRAW[leg](vf.SEED0 + 4) != a
    case = vf.draw_a(vf.SEED0 + 1)
    shape = (case["grid"]["nx"] + 2, case["grid"]["ny"] + 2)
    for kind in ("lattice", "edges"):
        f1, f2 = vf.drawn_fields(case, 7, shape, kind), vf.drawn_fields(case, 7, shape, kind)
        assert all(f1[n].tobytes() == f2[n].tobytes() and f1[n].shape == shape and np.isfinite(f1[n]).all() for n in f1)


def test_every_tie_of_the_interface_is_reached_on_both_sides(oracle_api):
    c = census(oracle_api)
    need(c, ["%s %s" % (t, s) for t in vf.IFACE_TIES for s in ("<", "==", ">")], "comparisons of vof_interface")
    need(c, ["segments", "degenerate"], "cells of vof_interface")


def test_every_other_tie_is_reached(oracle_api):
    c = census(oracle_api)
    need(c, ["blobs: F == threshold", "stats: Fc == level", "depths: the top cell holds F == 0.5", "depths: a row without a top",
             "depths: the front cell holds F == 0.5"], "threshold ties")
    need(c, ["frame: t == 0", "frame: t == 1", "frame: a mean on a bin edge", "frame: contour mean == 0.5", "frame: a NaN pixel", "frame: auto range",
             "frame: fixed range", "frame: inverted range (refused)"], "frame ties")
    need(c, ["sample: %s a whole number (%s)" % (a, w) for a in "st" for w in "uvF"] + ["sample: x == 0", "sample: x == Lx", "sample: y == 0", "sample: y == Ly",
                                                                                        "gauge: ig clamped"], "sample positions")
    need(c, ["scene: a sample on an edge (%s)" % k for k in ("box", "ellipse", "halfplane", "triangle")], "scene edges")
    need(c, ["scene: S = %d" % S for S in (1, 2, 4, 8, 16)] + ["scene: clear", "scene: over the field"], "scene calls")


def test_every_kind_family_capacity_strip_and_grid_is_reached(oracle_api):
    c = census(oracle_api)
    need(c, ["kind: " + k for k in vf.KINDS] + ["sprinkle: " + s for s in set(vf.SPRINKLES)], "field kinds")
    need(c, ["grid: f64", "grid: f32", "grid: cast f32", "grid: cast none", "cells: square", "cells: rectangular"], "precisions, casts, cells")
    need(c, ["family: " + f for f in vf.FAMILIES], "verb families")
    need(c, ["op: " + o for o in vf.OPS_B] + ["steps with multigrid cycles", "steps with sweeps", "eager", "graphs"], "operations of leg B")
    need(c, ["capacity: " + k for k in vf.CAPS], "capacity classes")
    need(c, ["strip: " + k for k in vf.STRIPS] + ["strip: owns nothing", "strip: without row 1 and row nx"], "strips")
    need(c, ["grid: ny %s %d columns" % (w, vf.TILE * k) for k in (1, 2, 3, 4) for w in ("one below", "on", "one past")], "tile widths")
    need(c, ["grid: ny on the 112-column stride", "grid: ny one past the 112-column stride"] + ["grid: ny + 2 %s 256 columns" % w for w in ("one below", "on", "one past")]
         + ["grid: fewer than 64 columns", "grid: the smallest nx", "grid: more entries than scan threads", "grid: more blocks than folding threads", "grid: nx odd",
            "grid: nx even", "grid: nx a multiple of 4", "grid: nx one past a multiple of 4", "grid: nx a multiple of 32", "grid: nx one past a multiple of 32"], "grids")


def test_strips_are_drawn_inside_what_they_store():
    rng = np.random.default_rng(5)
    for _ in range(2000):
        nx = int(rng.choice(vf.NX_SET + (1025,)))
        s = vf.draw_strip(rng, nx)
        (r0, r1), (o0, o1) = s["rows"], s["own"]
        assert 0 <= r0 and r1 <= nx + 1 and r1 - r0 >= 2
        assert r0 + 1 <= min(o0, o1 + 1) and max(o1, o0 - 1) <= r1 - 1 and 1 <= o0 and o1 <= nx, s


# ---------------------------------------------------------------------------------------------------- the yardsticks on ties
JUDGED = [(33, 17, "f64", "lattice", 0.25), (17, 129, "f32", "lattice", 0.0), (9, 63, "f64", "edges", 2.0 ** -20), (33, 40, "f32", "edges", 0.125),
          (16, 16, "f64", "lattice", float(np.float32(1e-6)))]


def judged_case(nx, ny, dtype, kind, eps, seed=11):
    case = dict(vf.draw_a(seed), kind=kind, eps=eps, sprinkle="none")
    case["grid"] = dict(case["grid"], nx=nx, ny=ny, dtype=dtype)
    return case, vf.drawn_fields(case, seed, (nx + 2, ny + 2))


@pytest.mark.parametrize("nx,ny,dtype,kind,eps", JUDGED)
@pytest.mark.parametrize("dx,dy", [(0.01, 0.01), (0.01, 0.013)])
def test_the_plic_line_cuts_off_the_area_F_on_ties(nx, ny, dtype, kind, eps, dx, dy):
    """The judge of tests/test_interface.py on lattice and edge fields: the unit square left of the segment has the area F (to 1e-13,
    that test's bound), both ends lie on the cell boundary, the liquid is on the left, the normal has unit length -- whichever branch a
    tie takes.  A cell whose F is within 1e-13 of 0 or 1 has a segment shorter than the bound can see: only its ends are judged."""
    case, f = judged_case(nx, ny, dtype, kind, eps)
    F = f["F"].astype(np.float64)
    rows, summary, unit = inp.restate(F, eps, dx, dy)
    c = collections.Counter()
    vf.census_interface(c, F, eps, dx, dy, 1, nx)
    assert summary["SEGMENTS"] == len(rows) == c["segments"] > 0 and summary["DEGENERATE"] == c["degenerate"]
    worst = 0.0
    for r, u in zip(rows, unit):
        i, j = int(r[0]), int(r[1])
        assert eps < F[i, j] < 1.0 - eps
        a, b = u[3] - u[1], -(u[2] - u[0])
        worst = max(worst, abs(inp.clipped_area(a, b, a * u[0] + b * u[1]) - F[i, j]))
        for xi, eta in ((u[0], u[1]), (u[2], u[3])):
            assert (xi in (0.0, 1.0) and -1e-15 <= eta <= 1 + 1e-15) or (eta in (0.0, 1.0) and -1e-15 <= xi <= 1 + 1e-15), (i, j, xi, eta)
        assert r[2] == (i - 1 + u[0]) * dx and r[3] == (j - 1 + u[1]) * dy and r[4] == (i - 1 + u[2]) * dx and r[5] == (j - 1 + u[3]) * dy
        assert (r[4] - r[2]) * r[7] - (r[5] - r[3]) * r[6] <= 0.0, (i, j)
        assert abs(math.hypot(r[6], r[7]) - 1.0) <= 1e-15
    ties = {t: c[t + " =="] for t in vf.IFACE_TIES}
    print(nx, ny, dtype, kind, eps, "segments", len(rows), "worst area error %.3e" % worst, "ties", ties)
    assert worst <= 1e-13
    if kind == "lattice":
        assert ties["a ? b"] > 0 and ties["F ? 0.5"] > 0 and ties["mxsum ? 0"] + ties["mysum ? 0"] > 0, ties


@pytest.mark.parametrize("nx,ny,dtype,kind,eps", JUDGED)
def test_the_statistics_equal_the_naive_judge_on_ties(nx, ny, dtype, kind, eps):
    """tests/test_stats.py's judge: the stacked samples, np.mean, argmax over the wet flags -- on fields full of Fc == level."""
    case, _ = judged_case(nx, ny, dtype, kind, eps)
    for level in (0.5, 0.25, 1.0):
        samples = []
        for n in range(4):
            f = vf.drawn_fields(dict(case, level=level), 100 + n, (nx + 2, ny + 2))
            samples.append((f["F"], f["u"], f["v"], 10 + 3 * n))
        pl, summ = stn.run(samples, 3, level)
        want = stn.naive(samples, level)
        Fc = np.stack([stn.cell_values(*s[:3])[0] for s in samples])
        print(nx, ny, dtype, kind, "level", level, "cells with Fc == level", int((Fc == level).sum()))
        assert (Fc == level).any()
        assert np.array_equal(pl["WET"], want["wet"]) and np.array_equal(pl["ARRIVAL"], want["arrival"]) and np.array_equal(pl["MAX_F"], want["F_max"])
        assert np.array_equal(pl["WET"], (Fc >= level).sum(axis=0)) and np.array_equal(pl["MAX_SPEED2"], want["speed2_max"])
        for plane, key in (("SUM_F", "F_mean"), ("SUM_UV", "uv_mean"), ("SUM_FU", "Fu_mean")):
            assert np.all(np.abs(pl[plane] / 4 - want[key]) <= 1e-12 * np.abs(want[key])), plane
        assert summ["EVER_WET"] == float((want["arrival"] >= 0).sum())


def second_labelling(mem):
    """4-connected components by union-find over the faces, numbered by their smallest cell in (i, j) order."""
    nr, nc = mem.shape
    parent = list(range(nr * nc))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i in range(nr):
        for j in range(nc):
            if mem[i, j]:
                for a, b in ((i + 1, j), (i, j + 1)):
                    if a < nr and b < nc and mem[a, b]:
                        x, y = find(i * nc + j), find(a * nc + b)
                        if x != y:
                            parent[max(x, y)] = min(x, y)
    lab, names = np.full((nr, nc), -1, dtype=np.int32), {}
    for i in range(nr):
        for j in range(nc):
            if mem[i, j]:
                lab[i, j] = names.setdefault(find(i * nc + j), len(names))
    return lab, len(names)


@pytest.mark.parametrize("nx,ny,dtype,kind,eps", JUDGED)
def test_blobs_and_depths_by_the_headers_words_on_ties(nx, ny, dtype, kind, eps):
    case, f = judged_case(nx, ny, dtype, kind, eps)
    F = f["F"].astype(np.float64)
    for thr in (0.5, 0.25, 0.75):
        at = int((F[1:-1, 1:-1] == thr).sum())
        for phase in (bnp.LIQUID, bnp.GAS):
            rows, summ, lab = bnp.restate(f["F"], f["u"], f["v"], phase, thr)
            mem = np.array([[(F[i, j] >= thr) if phase == bnp.LIQUID else (F[i, j] < thr) for j in range(1, ny + 1)] for i in range(1, nx + 1)])
            wlab, n = second_labelling(mem)
            assert summ["BLOBS"] == n and summ["MEMBER_CELLS"] == int(mem.sum()) and np.array_equal(lab, wlab), (thr, phase)
            w = np.clip(F[1:-1, 1:-1], 0.0, 1.0) if phase == bnp.LIQUID else 1.0 - np.clip(F[1:-1, 1:-1], 0.0, 1.0)
            for b in range(n):
                t = w[lab == b]
                assert rows[b, bnp.CELLS] == t.size and abs(rows[b, bnp.SUM_W] - math.fsum(t)) <= t.size * 2.0 ** -52 * math.fsum(np.abs(t))
        print(nx, ny, dtype, kind, "threshold", thr, "cells on it", at)
        assert at > 0 or thr != 0.5
    res = dpn.restate(f["F"])
    for i in range(1, nx + 1):
        top = 0
        for j in range(1, ny + 1):
            if F[i, j] >= 0.5:
                top = j
        assert res["top"][i - 1] == top
    wet = [i for i in range(1, nx + 1) if F[i, 1] >= 0.5]
    assert (res["front_lo"], res["front_hi"]) == ((wet[0], wet[-1]) if wet else (0, 0))
    di, dj, total = dpn.ordered(res["terms"], 2)
    assert all(dpn.within_bound(di[i - 1], F[i, 1:-1]) for i in range(1, nx + 1)) and dpn.within_bound(total, F[1:-1, 1:-1])


@pytest.mark.parametrize("nx,ny,dtype,kind,eps", JUDGED)
def test_the_colour_index_by_the_headers_words_on_ties(nx, ny, dtype, kind, eps):
    """One pixel at a time, in Python doubles, from the text of include/vof2d.h: t <= 0 or hi == lo or t NaN -> 0, t >= 1 -> 255, else
    (int)(t * 255.0 + 0.5); the contour where s = (mF >= 0.5) changes towards a + 1 or b + 1; a NaN mean takes lut[257]."""
    case, f = judged_case(nx, ny, dtype, kind, eps)
    f = vf.sprinkle(f, "nan", 3, names=("F",))
    lut = fnp.default_lut()
    for bx, by, lo, hi in ((1, 1, 0.0, 1.0), (1, 1, 0.25, 0.5), (2, 3, 0.125, 0.875), (1, 1, 0.0, 0.0)):
        rgb, m, summ = fnp.frame(fnp.F, f, bx, by, fnp.CONTOUR, lo, hi, lut)
        pw, ph = m.shape
        if lo == hi:
            ok = m[~np.isnan(m)]
            lo, hi = float(ok.min()), float(ok.max())
        assert (summ[3], summ[4]) == (lo, hi)
        ties = 0
        for a in range(pw):
            for b in range(ph):
                x = float(m[a, b])
                if x != x:
                    idx = 257
                else:
                    t = (x - lo) / (hi - lo) if hi != lo else 0.0
                    idx = 0 if (t <= 0.0 or hi == lo or t != t) else 255 if t >= 1.0 else int(t * 255.0 + 0.5)
                    ties += int(t in (0.0, 1.0)) + int(x == 0.5)
                    s = x >= 0.5
                    if (a + 1 < pw and s != (float(m[a + 1, b]) >= 0.5)) or (b + 1 < ph and s != (float(m[a, b + 1]) >= 0.5)):
                        idx = 256
                assert tuple(rgb[ph - 1 - b, a]) == tuple(lut[idx]), (bx, by, lo, hi, a, b, x)
        print(nx, ny, dtype, kind, (bx, by, lo, hi), "pixels on an end of the range or on the contour level", ties)
        assert ties > 0 or (bx, by) != (1, 1)


def test_samples_on_faces_and_scene_samples_on_edges_by_scalar_arithmetic():
    """A sample at a field point is the field value, on every face, corner and wall of the half-cell lattice; a scene sample on an
    edge is inside (closed tests), decided again in Python doubles one sample at a time."""
    case = dict(vf.draw_a(21), npos=60)
    g = case["grid"] = dict(case["grid"], nx=9, ny=17, dtype="f64")
    k = dict(dx=0.1 / 9, dy=0.1 / 17, dxi=1 / (0.1 / 9), dyi=1 / (0.1 / 17), Lx=0.1, Ly=0.1)
    xy, refused = vf.positions_of(case, k)
    G = tnp.Grid(9, 17, k["dxi"], k["dyi"], k["Lx"], k["Ly"])
    f = vf.drawn_fields(case, 5, (11, 19), "lattice")
    Ff, u, v = tnp.fields(f["F"], f["u"], f["v"], record=True)
    hits = 0
    for x, y in xy.tolist():
        for fld in (Ff, u, v):
            ib, jb, a, b = tnp.cell(fld.which, x, y, G)
            val = tnp.sample(fld, x, y, G)
            if a == 0.0 and b == 0.0:
                assert val == fld.v[ib][jb]
                hits += 1
            assert 0.0 <= a <= 1.0 + 1e-12 and 0.0 <= b <= 1.0 + 1e-12, (fld.which, x, y, a, b)
    assert hits > 10 and len(refused) == 6 and (xy.min() >= 0) and xy[:, 0].max() == k["Lx"] and xy[:, 1].max() == k["Ly"]
    cs = dict(vf.draw_c(22), S=4, nshapes=10)
    cs["grid"] = g
    recs = vf.scene_of(cs, k)
    n_liq, n_keep = scn.counts(recs, 4, k["dx"], k["dy"], np.arange(11), 19)
    c = collections.Counter()
    vf.census_scene(c, recs, 4, k["dx"], k["dy"], np.arange(11), 19)
    print("samples on an edge", dict(c))
    assert sum(c.values()) > 0
    for (i, j) in ((0, 0), (3, 5), (9, 17), (10, 18), (5, 1)):
        liq = keep = 0
        for a in range(4):
            for b in range(4):
                xs, ys = vf.sample_coord(i, a, 4, k["dx"]), vf.sample_coord(j, b, 4, k["dy"])
                state = scn.KEEP
                for rec in recs:
                    if bool(scn.inside(rec, np.array([[xs]]), np.array([[ys]]))[0, 0]):
                        state = int(rec[1])
                liq += state == scn.LIQUID
                keep += state == scn.KEEP
        assert (n_liq[i, j], n_keep[i, j]) == (liq, keep), (i, j)
