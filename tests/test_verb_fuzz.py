"""The generators of the verb fuzz judged on the CPU (tests/_verb_fuzz.py; the device leg is tests/test_verb_fuzz_gpu.py).

The fixed-seed slice is replayed through the restatements alone -- the fields of a case are drawn (a flow state comes from the CPU
oracle, which vof_step equals bit for bit), the comparisons of the restatements are formed again and counted on either side of
equality -- and must reach every tie, kind, family, capacity class, strip and boundary grid it claims to.  The counts are printed
and stand in the assertion messages: this test fixes the size of the slice from below.

The restatements themselves are judged on the new inputs (lattice and edge fields, where ties are the rule) by the
definition-level judges of tests/test_*.py, taken to those fields: the PLIC line that cuts off the area F, the naive statistics,
a second labelling, the depth of a column counted cell by cell, the colour index by the header's words one pixel at a time; for
vof_regrid the range, volume and order of a cell's children, the selects at k == 0 and the pair sums against math.fsum, for vof_curvature
every row again in Python doubles, for vof_energy the reference's predictor on lattice fields and SG one face at a time.
"""
import collections
import math

import numpy as np
import pytest

import _blobs_np as bnp
import _curvature_np as cnp
import _depths_np as dpn
import _energy_np as enp
import _frames_np as fnp
import _interface_np as inp
import _regrid_np as rnp
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
        for leg in "ABCD":
            for seed in vf.slice_seeds(leg):
                case = vf.DRAW[leg](seed)
                g = case["src" if leg == "D" else "grid"]
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
                elif leg == "D":
                    vf.census_d(c, case, vf.fields_d(api, case), k)
                else:
                    vf.census_c(c, case, k, vf.scene_of(case, k))
        _CENSUS["c"] = c
        for name in sorted(c):
            print("%-55s %d" % (name, c[name]))
    return _CENSUS["c"]


def need(c, names, what):
    missing = [n for n in names if c[n] == 0]
    assert not missing, "%s the slice does not reach: %s; the counts: %s" % (what, missing, {n: c[n] for n in names})


# draw_a, draw_b and draw_c of three committed seeds as they were before the second stream existed (recorded from the parent of the
# commit that added the stream): every key of that day keeps its value; the operations the second stream inserts into leg B stand at case["inserted"]
DRAWN_BEFORE = {
    ("A", 20261023): {'leg': 'A', 'seed': 20261023, 'grid': {'nx': 17, 'ny': 128, 'dtype': 'f64', 'cast': 'none', 'cells': 'default', 'kw': {}}, 'kind': 'edges', 'ic': 3, 'steps': 1, 'sprinkle': 'naninf', 'eps': 0.125, 'thr': 0.30000001192092896, 'level': 0.5, 'frame': {'q': 'U', 'bx': 3, 'by': 133, 'contour': False, 'symmetric': True, 'lo': 0.25, 'hi': 0.5, 'lut': False}, 'npos': 26, 'caps': {'interface': 'short', 'blobs': 'short', 'tracers': 'generous', 'gauges': 'generous', 'depths': 'generous', 'frame': 'generous'}, 'strip': {'kind': 'middle', 'rows': (5, 14), 'own': (6, 13)}},
    ("A", 20261077): {'leg': 'A', 'seed': 20261077, 'grid': {'nx': 31, 'ny': 511, 'dtype': 'f32', 'cast': 'none', 'cells': 'square', 'kw': {'Lx': 0.1, 'Ly': 1.6483870967741936}}, 'kind': 'edges', 'ic': 2, 'steps': 0, 'sprinkle': 'none', 'eps': 0.125, 'thr': 0.5, 'level': 0.5, 'frame': {'q': 'DYE', 'bx': 36, 'by': 3, 'contour': False, 'symmetric': False, 'lo': 0.0, 'hi': 1.0, 'lut': False}, 'npos': 36, 'caps': {'interface': 'generous', 'blobs': 'exact', 'tracers': 'exact', 'gauges': 'short', 'depths': 'exact', 'frame': 'short'}, 'strip': {'kind': 'random', 'rows': (16, 27), 'own': (19, 24)}},
    ("A", 20261140): {'leg': 'A', 'seed': 20261140, 'grid': {'nx': 15, 'ny': 255, 'dtype': 'f32', 'cast': 'f32', 'cells': 'free', 'kw': {'Lx': 0.13, 'Ly': 0.1}}, 'kind': 'edges', 'ic': 2, 'steps': 1, 'sprinkle': 'none', 'eps': 1e-06, 'thr': 0.5, 'level': 0.25, 'frame': {'q': 'SPEED', 'bx': 3, 'by': 1, 'contour': False, 'symmetric': False, 'lo': 0.0, 'hi': 0.0, 'lut': False}, 'npos': 13, 'caps': {'interface': 'zero', 'blobs': 'zero', 'tracers': 'short', 'gauges': 'exact', 'depths': 'zero', 'frame': 'zero'}, 'strip': {'kind': 'none', 'rows': (6, 9), 'own': (8, 7)}},
    ("B", 20261023): {'leg': 'B', 'seed': 20261023, 'grid': {'nx': 17, 'ny': 128, 'dtype': 'f64', 'cast': 'none', 'cells': 'default', 'kw': {}}, 'kind': 'lattice', 'ic': 3, 'warm': 2, 'eager': False, 'eps': 1e-06, 'thr': 0.5, 'level': 0.5, 'frame': {'q': 'U', 'bx': 1, 'by': 2, 'contour': True, 'symmetric': True, 'lo': 0.0, 'hi': 1.0, 'lut': True}, 'npos': 12, 'sprinkle': 'none', 'caps': {'interface': 'short', 'blobs': 'zero', 'tracers': 'generous', 'gauges': 'generous', 'depths': 'generous', 'frame': 'short'}, 'ops': [('refused_strip', 'gauges_get'), ('refused_strip', 'step_frames'), ('overwrite', 'F', 653185922), ('readonly', 'gauges_get'), ('refused_strip', 'step_dye'), ('knob', 'dye_fused', 0), ('step_stats', 5, 3, 1, 1, 0.25, False), ('knob', 'mg_graph', 0)]},
    ("B", 20261077): {'leg': 'B', 'seed': 20261077, 'grid': {'nx': 17, 'ny': 511, 'dtype': 'f32', 'cast': 'none', 'cells': 'square', 'kw': {'Lx': 0.1, 'Ly': 3.0058823529411764}}, 'kind': 'lattice', 'ic': 3, 'warm': 0, 'eager': True, 'eps': 9.999999974752427e-07, 'thr': 0.75, 'level': 0.5, 'frame': {'q': 'DYE', 'bx': 4, 'by': 516, 'contour': True, 'symmetric': False, 'lo': 0.0, 'hi': 0.0, 'lut': True}, 'npos': 8, 'sprinkle': 'none', 'caps': {'interface': 'exact', 'blobs': 'exact', 'tracers': 'generous', 'gauges': 'exact', 'depths': 'short', 'frame': 'zero'}, 'ops': [('set_scene', 1041839635, 2, False), ('stats_hand', 'edges', 975457223, 2, 0.5, 'nan'), ('overwrite', 'u', 572080256), ('step_gauges', 4, 3, 2)]},
    ("B", 20261140): {'leg': 'B', 'seed': 20261140, 'grid': {'nx': 15, 'ny': 255, 'dtype': 'f32', 'cast': 'f32', 'cells': 'free', 'kw': {'Lx': 0.13, 'Ly': 0.1}}, 'kind': 'lattice', 'ic': 1, 'warm': 2, 'eager': False, 'eps': 0.125, 'thr': 0.75, 'level': 0.5, 'frame': {'q': 'F', 'bx': 1, 'by': 1, 'contour': False, 'symmetric': False, 'lo': 0.375, 'hi': 0.375, 'lut': True}, 'npos': 14, 'sprinkle': 'none', 'caps': {'interface': 'generous', 'blobs': 'zero', 'tracers': 'zero', 'gauges': 'generous', 'depths': 'generous', 'frame': 'zero'}, 'ops': [('knob', 'dye_fused', 0), ('step_tracers', 3, 2, 0, 0), ('set_scene', 459458003, 8, True), ('step_diag', 4, 1, 0), ('stats_hand', 'edges', 199222999, 3, 0.30000001192092896, 'none'), ('refused_phase', 'stats_sample')]},
    ("C", 20261023): {'leg': 'C', 'seed': 20261023, 'grid': {'nx': 17, 'ny': 128, 'dtype': 'f64', 'cast': 'none', 'cells': 'default', 'kw': {}}, 'ic': 3, 'S': 16, 'clear': True, 'nshapes': 10, 'base': 'rough', 'shortcuts': 1, 'strip': {'kind': 'none', 'rows': (3, 6), 'own': (5, 4)}, 'steps': 2},
    ("C", 20261077): {'leg': 'C', 'seed': 20261077, 'grid': {'nx': 31, 'ny': 511, 'dtype': 'f32', 'cast': 'none', 'cells': 'square', 'kw': {'Lx': 0.1, 'Ly': 1.6483870967741936}}, 'ic': 1, 'S': 8, 'clear': True, 'nshapes': 1, 'base': 'rough', 'shortcuts': 0, 'strip': {'kind': 'single', 'rows': (0, 4), 'own': (1, 1)}, 'steps': 2},
    ("C", 20261140): {'leg': 'C', 'seed': 20261140, 'grid': {'nx': 15, 'ny': 255, 'dtype': 'f32', 'cast': 'f32', 'cells': 'free', 'kw': {'Lx': 0.13, 'Ly': 0.1}}, 'ic': 2, 'S': 16, 'clear': True, 'nshapes': 1, 'base': 'edges', 'shortcuts': 0, 'strip': {'kind': 'none', 'rows': (5, 10), 'own': (8, 7)}, 'steps': 2},
}


def test_the_committed_seeds_draw_what_they_drew_before_the_second_stream():
    for (leg, seed), before in DRAWN_BEFORE.items():
        case = vf.DRAW[leg](seed)
        if leg == "B":
            assert all(case["ops"][n][0] in vf.OPS_B2 or case["ops"][n][1] == vf.LATER for n in case["inserted"])
            case = dict(case, ops=[op for n, op in enumerate(case["ops"]) if n not in case["inserted"]])
        assert {k: case[k] for k in before} == before, (leg, seed)
    assert sum(len(vf.draw_b(seed)["inserted"]) for _, seed in DRAWN_BEFORE) > 0


def test_the_generator_is_deterministic():
    for leg in "ABCD":
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


def test_every_tie_of_curvature_energy_and_regrid_is_reached_on_all_three_sides(oracle_api):
    c = census(oracle_api)
    # m == 0 in a row cannot be: AXIS 0 means |mxsum| dx <= |mysum| dy, so m = mysum == 0 makes both sums 0 (or a product that underflowed from
    # below 1e-10), which is a degenerate cell, no row; AXIS 1 means |mxsum| dx > |mysum| dy >= 0; a NaN in the 3 x 3 cells reaches both sums
    NO_TIE = "curv: m ? 0 =="
    need(c, [n for n in ("%s %s" % (t, s) for t in vf.CURV_TIES + vf.ENERGY_TIES + vf.REGRID_TIES for s in ("<", "==", ">")) if n != NO_TIE], "comparisons of the three verbs")
    assert c[NO_TIE] == 0, "a row of vof_curvature with m == 0: the argument above is wrong, and the flip of m >= 0 is no longer neutral"
    need(c, ["curv: VALID rows", "curv: rows not VALID", "curv: a stencil clamped on both sides", "curv: more entries than scan threads with rows"]
         + ["curv capacity: " + k for k in vf.CAPS], "rows and capacities of vof_curvature")
    need(c, ["energy: a face with equal F", "energy: a face with unequal F", "energy: a face between +0 and -0", "energy: a face with a NaN F",
             "energy: a NaN that only a select keeps out of a sum"], "faces of vof_energy")
    need(c, ["regrid: si == 0", "regrid: sj == 0", "regrid: rx ry == 256", "regrid: a factor of 15", "regrid: a factor of 16", "regrid: terms no power of two",
             "regrid: along i only", "regrid: along j only", "regrid: copy", "regrid: unequal factors", "regrid: a chunk that starts inside a parent",
             "regrid: PLIC", "regrid: without PLIC", "regrid: eps = 0", "regrid: degenerate source cells", "regrid: a source with NaN", "regrid: a source with inf",
             "regrid: refine", "regrid: coarsen", "regrid: round trip", "regrid: steps behind it",
             "regrid: al == n1 where the two branches round apart"]
         + ["regrid: %s to %s" % (a, b) for a in ("f64", "f32") for b in ("f64", "f32")] + ["regrid: dst " + p for p in vf.PRE_D]
         + ["regrid: refused, " + r for r in vf.REFUSALS_D], "factors, dtypes, states and refusals of vof_regrid")
    need(c, ["regrid: dst ny %s %d columns" % (w, vf.TILE * k) for k in (1, 2, 3, 4) for w in ("one below", "on", "one past")]
         + ["regrid: dst ny fewer than 64 columns", "regrid: dst ny on the 112-column stride", "regrid: dst ny one past the 112-column stride"], "dst widths of vof_regrid")
    need(c, ["op: %s of the later verbs" % o for o in vf.REFUSED_B2] + ["regrid_in: with fuse_tm and f_zero_map"], "the new refusals and knobs of leg B")
    assert all(c["op: " + o] >= 10 for o in vf.OPS_B2), {o: c["op: " + o] for o in vf.OPS_B2}


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


# ---------------------------------------------------------------------------------------------------- vof_regrid, vof_curvature, vof_energy on ties
REGRID_FACTORS = [(2, 2), (3, 5), (16, 16), (7, 1)]


@pytest.mark.parametrize("nx,ny,dtype,kind,eps", JUDGED)
def test_regrid_children_keep_the_range_the_volume_and_the_order_on_ties(nx, ny, dtype, kind, eps):
    """The children of a cell with a line lie in [0, 1], their mean is the parent's F within 32 2^-52 (the bound of tests/test_regrid.py),
    and going along k' and m' -- away from the liquid corner, al falling -- a child's F never increases, whichever branch a tie takes."""
    case, f = judged_case(nx, ny, dtype, kind, eps)
    dx, dy = 0.1 / nx, 0.1 / ny
    kind_, a, b, alpha, fx, fy = rnp.line(f["F"], eps, dx, dy)
    row = kind_ == 2
    F0 = f["F"].astype(np.float64)[1:-1, 1:-1][row]
    assert row.sum() > 20
    no = np.zeros(int(row.sum()), dtype=bool)
    for rx, ry in REGRID_FACTORS:
        kids = np.array([[rnp.child_F(a[row], b[row], alpha[row], fx[row], fy[row], k, m, rx, ry) for m in range(ry)] for k in range(rx)])
        worst = float(np.abs(kids.astype(np.longdouble).mean(axis=(0, 1)) - F0).max()) / 2.0 ** -52
        print(nx, ny, dtype, kind, eps, (rx, ry), "cells with a line", int(row.sum()), "worst |mean - F| %.2f 2^-52" % worst, "children outside [0, 1]",
              int(((kids < 0) | (kids > 1)).sum()))
        assert kids.min() >= 0.0 and kids.max() <= 1.0 and worst <= 32.0
        along = np.array([[rnp.child_F(a[row], b[row], alpha[row], no, no, k, m, rx, ry) for m in range(ry)] for k in range(rx)])      # indexed [k', m']
        assert (along[1:] <= along[:-1]).all() and (along[:, 1:] <= along[:, :-1]).all(), (rx, ry)


def test_regrid_selects_and_sums_by_their_definitions():
    """u and v at k == 0 and m == 0 are the lerp with weight 0 on finite fields (==: the sign of a zero is the select's to keep); pair_sum is
    math.fsum within n 2^-52 fsum(|t|), and exact for 2^l equal terms."""
    case, f = judged_case(9, 12, "f64", "edges", 0.125)
    inner, _, _ = rnp.refine_interior(f, 3, 4, False, 0.0, 0.01, 0.01)
    u, v = f["u"].astype(np.float64), f["v"].astype(np.float64)
    for I in range(1, 10):
        for J in range(1, 13):
            for m in range(4):
                assert inner["u"][(I - 1) * 3, (J - 1) * 4 + m] == u[I, J] + (0.0 / 3.0) * (u[I + 1, J] - u[I, J])
            for k in range(3):
                assert inner["v"][(I - 1) * 3 + k, (J - 1) * 4] == v[I, J] + (0.0 / 4.0) * (v[I, J + 1] - v[I, J])
    rng = np.random.default_rng(3)
    for n in (1, 3, 35, 105, 240, 256):
        t = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, size=n)
        got, exact = float(rnp.pair_sum(np.float64(x) for x in t)), math.fsum(t)
        print("pair_sum of %d terms: |d| %.3e, bound %.3e" % (n, abs(got - exact), n * 2.0 ** -52 * math.fsum(np.abs(t))))
        assert abs(got - exact) <= n * 2.0 ** -52 * math.fsum(np.abs(t))
    for l in range(9):
        for x in (0.1, float(np.float32(1e-6)), -0.0, 5e-324, 1.0 / 3.0):
            s = rnp.pair_sum(np.float64(x) for _ in range(2 ** l))
            assert s == x * 2.0 ** l and math.copysign(1.0, s) == math.copysign(1.0, x) and (s / 2.0 ** l) == x


def test_curvature_by_the_headers_words_on_ties():
    """Every row of the JUDGED fields again in Python doubles, one cell at a time, from the words of include/vof2d.h and the head of
    kernels/curvature.h: AXIS, the liquid end, VALID, hp, hpp, KAPPA, compared with ==."""
    seen = collections.Counter()
    for nx, ny, dtype, kind, eps in JUDGED:
        case, fld = judged_case(nx, ny, dtype, kind, eps)
        dx, dy = 0.1 / nx, 0.13 / ny
        F = [[float(x) for x in r] for r in fld["F"].astype(np.float64)]
        f = lambda ii, jj: F[min(max(ii, 0), nx + 1)][min(max(jj, 0), ny + 1)]
        cx, cy = -1 / (2 * dx), -1 / (2 * dy)
        rows, summ = cnp.restate(fld["F"], eps, dx, dy)
        assert len(rows) > 0
        for r in rows:
            i, j = int(r[cnp.I]), int(r[cnp.J])
            g = lambda di, dj: f(i + di, j + dj)
            mx1 = cx * (((g(1, 1) + g(1, 0)) - g(0, 1)) - g(0, 0)); my1 = cy * (((g(1, 1) - g(1, 0)) + g(0, 1)) - g(0, 0))
            mx2 = cx * (((g(1, 0) + g(1, -1)) - g(0, 0)) - g(0, -1)); my2 = cy * (((g(1, 0) - g(1, -1)) + g(0, 0)) - g(0, -1))
            mx3 = cx * (((g(0, 0) + g(0, -1)) - g(-1, 0)) - g(-1, -1)); my3 = cy * (((g(0, 0) - g(0, -1)) + g(-1, 0)) - g(-1, -1))
            mx4 = cx * (((g(0, 1) + g(0, 0)) - g(-1, 1)) - g(-1, 0)); my4 = cy * (((g(0, 1) - g(0, 0)) + g(-1, 1)) - g(-1, 0))
            mxsum, mysum = (((mx1 + mx2) + mx3) + mx4) / 4, (((my1 + my2) + my3) + my4) / 4
            assert eps < g(0, 0) < 1 - eps and not (abs(mxsum) < 1e-10 and abs(mysum) < 1e-10)
            ax, by = abs(mxsum) * dx, abs(mysum) * dy
            axis = 1 if ax > by else 0
            m = mxsum if axis else mysum
            tl = -3 if m >= 0 else 3
            cell = (lambda d, t: g(t, d)) if axis else (lambda d, t: g(d, t))
            H, valid = {}, True
            for d in (-1, 0, 1):
                h = cell(d, -3)
                for t in (-2, -1, 0, 1, 2, 3):
                    h = h + cell(d, t)
                H[d] = h
                valid = valid and cell(d, tl) >= 1 - eps and cell(d, -tl) <= eps
                seen["an end cell on 1 - eps or on eps"] += int(cell(d, tl) == 1 - eps or cell(d, -tl) == eps)
            hs, ht = (dx, dy) if axis else (dy, dx)
            hp = ((H[1] - H[-1]) * hs) / (2 * ht)
            hpp = (((H[1] - 2 * H[0]) + H[-1]) * hs) / (ht * ht)
            q = 1 + hp * hp
            kappa = hpp / (q * math.sqrt(q))
            want = (float(valid), float(axis), kappa if valid else 0.0, hp if valid else 0.0, g(0, 0))
            assert (r[cnp.VALID], r[cnp.AXIS], r[cnp.KAPPA], r[cnp.HP], r[cnp.FVAL]) == want, (nx, ny, kind, i, j, r, want)
            seen["ax == by"] += int(ax == by)
            seen["m == 0"] += int(m == 0)
            seen["VALID"] += int(valid)
            seen["rows"] += 1
    print(dict(seen))
    # (m == 0 cannot be in a row: test_every_tie_of_curvature_energy_and_regrid_is_reached_on_all_three_sides says why)
    assert seen["ax == by"] > 0 and seen["an end cell on 1 - eps or on eps"] > 0 and seen["VALID"] > 0 and seen["m == 0"] == 0


@pytest.mark.parametrize("nx,ny", [(33, 17), (16, 40)])
def test_the_energy_pieces_are_the_predictor_on_lattice_fields(nx, ny):
    """test_the_pieces_are_the_predictor of tests/test_energy.py on a lattice field with tame velocities, where w == 0, here == 0 and equal F
    across a face are the rule: u + dt A is the oracle's u_star with ==."""
    import vof_oracle_np as onp
    case, _ = judged_case(nx, ny, "f64", "lattice", 1e-6)
    f = vf.drawn_fields(case, 12, (nx + 2, ny + 2), "lattice", tame=True)         # (a seed that draws the lattice of eighths: v = 0 is on it)
    t = onp.new_state(nx, ny, 1, np.float64, "f32")
    for n in ("F", "u", "v", "p"):
        getattr(t, n)[...] = f[n]
    r = enp.restate(t.F, t.u, t.v, t.p, enp.params_of_oracle(t.prm))
    onp.cal_nu_rho(t); onp.get_normal_young(t); onp.advect_upwind(t)
    dt = float(t.prm.dt)
    us = t.u[2:nx + 1, 1:ny + 1] + dt * r.uf["A"]
    vs = t.v[1:nx + 1, 2:ny + 1] + dt * r.vf["A"]
    c = collections.Counter()
    vf.census_energy(c, f)
    print({k: v for k, v in c.items() if "==" in k or "equal" in k})
    assert c["energy: u ? 0 =="] > 0 and c["energy: v ? 0 =="] > 0 and c["energy: here ? 0 =="] > 0 and c["energy: a face with equal F"] > 0
    assert np.array_equal(r.kappa, t.kappa[1:-1, 1:-1]) and np.array_equal(r.rho, t.rho) and np.array_equal(r.nu, t.nu)
    assert np.array_equal(us, t.u_star[2:nx + 1, 1:ny + 1]) and np.array_equal(vs, t.v_star[1:nx + 1, 2:ny + 1])


def test_the_surface_tension_term_one_face_at_a_time():
    """SG of every face in Python doubles: 0 where the raw F is equal across the face -- +0 beside -0 included, a NaN kappa beside it or
    not --, the written expression elsewhere; a NaN compared as a NaN."""
    case, f = judged_case(9, 63, "f64", "edges", 2.0 ** -20)
    f = vf.sprinkle(f, "nan", 4, names=("F",))
    F = f["F"].astype(np.float64)
    F[3, 5:9] = [0.0, -0.0, 0.0, -0.0]
    F[5:8, 20] = [-0.0, 0.0, -0.0]
    nx, ny = 9, 63
    prm = dict(dx=0.1 / nx, dy=0.1 / ny, dxi=nx / 0.1, dyi=ny / 0.1, dxi2=(nx / 0.1) ** 2, dyi2=(ny / 0.1) ** 2, rho_l=1000.0, rho_g=1.0, nu_l=1e-6, nu_g=1.5e-5, sigma=0.07,
               gx=0.0, gy=-9.8)
    r = enp.restate(F, f["u"], f["v"], f["p"], prm)
    kappa = np.zeros_like(F); kappa[1:-1, 1:-1] = r.kappa
    seen = collections.Counter()
    for faces, (di, dj), h, lo_i, lo_j in ((r.uf, (1, 0), prm["dx"], 2, 1), (r.vf, (0, 1), prm["dy"], 1, 2)):
        for i in range(lo_i, nx + 1):
            for j in range(lo_j, ny + 1):
                f0, fb = float(F[i, j]), float(F[i - di, j - dj])
                k0, kb, r0, rb = float(kappa[i, j]), float(kappa[i - di, j - dj]), float(r.rho[i, j]), float(r.rho[i - di, j - dj])
                want = 0.0 if f0 == fb else (((((-prm["sigma"]) * (f0 - fb)) * ((k0 + kb) / 2.0)) / h) * 2) / (r0 + rb)
                got = float(faces["SG"][i - lo_i, j - lo_j])
                assert got == want or (got != got and want != want), (i, j, got, want)
                seen["equal F"] += int(f0 == fb)
                seen["+0 beside -0"] += int(f0 == 0.0 and fb == 0.0 and math.copysign(1.0, f0) != math.copysign(1.0, fb))
                seen["equal F beside a NaN kappa"] += int(f0 == fb and (k0 != k0 or kb != kb))
                seen["a NaN F"] += int(f0 != f0 or fb != fb)
    print(dict(seen))
    assert all(seen[k] > 0 for k in ("equal F", "+0 beside -0", "equal F beside a NaN kappa", "a NaN F")), dict(seen)
