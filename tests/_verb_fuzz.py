"""Generators of the verb fuzz (tests/test_verb_fuzz.py judges them on the CPU, tests/test_verb_fuzz_gpu.py runs them on the
device): everything a case is made of comes from its seed, as in draw_case of tests/test_fuzz_gpu.py.  Importable without a GPU.

A case is drawn in two stages.  draw_a / draw_b / draw_c / draw_d(seed) give a dict of plain numbers: the grid, the kind of field, the
thresholds, the frame spec, the capacities, the strip, the seeds of the arrays.  fields_of / positions_of / scene_of turn those into
arrays once the constants of the handle are known (dx, dy, Lx, Ly of vof_get_param: the library decides them, so the positions on
cell faces and the shape edges through sample points are formed from its doubles, not from a guess of them).

Grids sit on and beside the boundaries of the extension kernels (csrc/vof2d_device.h, csrc/kernels/*.h, csrc/runtime/rows.h):
  ny   64 V = 128 columns a wave (cell_tile, V = 2 for both dtypes), four waves a block (k_stats and every pass of reduced_rows):
       128 k + {-1, 0, 1}, k = 1 .. 4; the 112-column stride of k_dye (TransportGeom): 112, 113; the 256-column blocks of k_scene over
       j = 0 .. ny + 1: ny + 2 = 255, 256, 257; fewer than 64 columns: one wave with idle lanes
  nx   the chunk lengths the cells-per-wave rule gives small grids -- 2 (diag_chunk, depths, frames, stats), 4 (cell_rows_chunk) -- and the
       32 rows of kBlobRows, on and beside them, odd and even; 3, the smallest vof_create takes; 1025 x 6 and 2051 x 3: more (row, tile)
       entries than k_cell_rows_scan has threads (1024), and 257 blocks of partials for the 256 folding threads of k_row_finish

Leg D (vof_regrid) draws a PAIR of grids.  kernels/regrid.h is destination-centred, so dst ny walks through NY_D -- the tile edges 128 k +
{-1, 0, 1}, the widths below 64 columns, 112 and 113 -- and src follows from the drawn direction and factors (1, 2, 3, 4, 5, 7, 8, 15, 16: every
odd factor has a middle child with si == 0, 16 x 16 is the 256 terms of PairSum's top level, 35, 105, 240 fold from several levels); dst nx comes
from NX_SET, so that refining by 3, 5 or 7 a row chunk begins inside a parent.  The larger grid holds at most 40 000 cells.

Everything drawn since a leg was first committed comes from a second generator, np.random.default_rng([seed, 1]) (second_stream): the
committed seeds of legs A, B and C keep their grids, kinds, fields, positions, strips and operations (tests/test_verb_fuzz.py holds three of
them to a literal).  In leg B the second stream inserts 0 to 2 operations -- step_energy, regrid_out, regrid_in, refusals of the later verbs --
at drawn positions of the sequence the first stream drew.

Field kinds: "flow" (an -ic state after a few steps), "lattice" (multiples of 1/4 or 1/8 in blocks of cells, so that neighbours are
equal: a == b, axis-aligned normals, F == 0.5), "edges" (every value drawn from the verbs' thresholds and their floating-point
neighbours in the field's dtype, +-0, a subnormal, values below 0 and above 1).  Any kind may be sprinkled with NaN, or NaN and +-inf.

What is NOT drawn, and why (nothing else is excluded):
  * a non-finite field, or a lattice / edges field, under a time step: include/vof2d.h defines vof_step for the reference's states;
    after the first inf / NaN the library and the reference may part (v_max / v_min against comparisons, tests/test_fuzz_gpu.py), and
    random F with O(1) velocities is past the Courant number at which the transport's contract ends.  Steps run on flow states and on
    the perturbations of them tests/test_fuzz_gpu.py draws; the drawn fields are sampled by hand (vof_stats_sample) and taken back
  * +-inf under vof_diagnostics, vof_dye_stats and vof_frame: the header defines the result (sums propagate), but inf - inf makes a NaN
    whose sign IEEE 754 leaves to the implementation, the frames are held byte for byte (tests/test_frames_gpu.py), and the judges of
    the two reductions form math.fsum of the terms, which refuses infinite terms of both signs.  Those three get NaN only
  * +-inf under vof_energy: for the reason of vof_diagnostics -- the header defines the result, but the judge forms math.fsum of the terms,
    which refuses infinities of both signs, and the sign of the NaN an inf - inf makes is the implementation's.  vof_energy gets NaN only, in
    F, u, v and p, with velocities and pressures as drawn (not tamed); vof_curvature takes +-inf (its helper compares NaN slots as NaN).
    Nothing else is excluded under vof_energy
  * the BITS of a NaN under vof_regrid: a source sprinkled with NaN or +-inf is given to it, and dst is compared entry by entry, every
    entry that is no NaN bit for bit and the NaNs in the same places; the sign and payload of the NaN an inf - inf, a 0 * inf or the
    narrowing of a NaN to float makes are the implementation's (IEEE 754), the host's and the device's differ.  Nothing else is excluded:
    finite sources are compared byte for byte, ghost rings and F2 included
  * steps behind a vof_regrid from anything but a flow source: the stepping rule of the first entry -- a lattice or edges state, or a
    sprinkled one, is no state vof_step is defined on.  Behind a flow source dst steps beside a twin fed the restated arrays.  Nothing else
    is excluded: the call itself, the second call, the round trip and the refusal run on every kind
  * a NaN under the VORT quantity of vof_frame: VORT subtracts, the device subtracts by adding the negated operand, which turns the sign
    of a NaN operand, the host keeps it; IEEE 754 allows both and tests/test_frames_gpu.py compares the means as bytes.  The other
    quantities add and multiply only and take the sprinkled NaN; a sprinkled case that drew VORT renders SPEED instead
  * a non-finite dye under vof_dye_advance ("the values are expected to be finite"), a non-finite position, time or spec field (refused
    by the header: drawn as refusals, not as inputs)
  * tracer and gauge positions outside the closed domain as inputs: the header refuses them; they are drawn as refusals
  * eps, thresholds and levels outside their open / half-open intervals: refused by the header; drawn inside, ends of (0, 1] included
  * mg_coarse_block = 1 on the twin alone: "other bits than the launches'" by the header; the knob is set on both handles or on none
"""
import math

import numpy as np

import _frames_np as fnp
import _interface_np as inp
import _scene_np as scn
import _tracers_np as tnp

V = 2                      # VecWidth<T>::V of csrc/vof2d_device.h
TILE = 64 * V              # cell_tile of csrc/kernels/cells.h
NY_TILE = tuple(TILE * k + d for k in (1, 2, 3, 4) for d in (-1, 0, 1))
NY_DYE = (112, 113)        # TransportGeom<2>::STRIDE
NY_SCENE = (253, 254, 255)  # ny + 2 on and beside the 256 columns of a block of k_scene
NY_IDLE = (3, 4, 6, 17, 40, 63)
NX_SET = (3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65)
TALL = ((1025, 6), (2051, 3))
ALL_NY = NY_TILE + NY_DYE + NY_SCENE + NY_IDLE          # (6 and 3 are the widths of the tall thin grids too)
MAX_CELLS = 17000
KINDS = ("flow", "lattice", "edges")
SPRINKLES = ("none", "none", "nan", "naninf")
EPS = (float(np.float32(1e-6)), 2.0 ** -20, 1e-6, 0.0, 0.25, 0.125)
THRESHOLDS = (0.5, 0.5, 0.25, 0.125, 0.75, float(np.float32(0.3)))
LEVELS = (0.5, 0.5, 0.25, 1.0, 0.125, float(np.float32(0.3)))
RANGES = ((0.0, 1.0), (0.25, 0.5), (-0.5, 0.5), (0.0, 0.0), (0.375, 0.375), (0.125, 0.875), (1.0, 0.0))   # fixed, auto (lo == hi), inverted (refused)
QUANTITIES = ("F", "U", "V", "SPEED", "P", "VORT", "DYE")
CAPS = ("zero", "short", "exact", "generous")
STRIPS = ("single", "none", "middle", "random")
NP = {"f64": np.float64, "f32": np.float32}
INF_OK = ("interface", "blobs", "depths", "tracers", "gauges", "curvature")     # the read-only verbs drawn on fields with +-inf (module docstring)
READ_ONLY = ("diagnostics", "interface", "blobs", "depths", "frame", "dye_stats", "gauges", "tracers", "curvature", "energy")
STRIP_VERBS = ("diagnostics", "interface", "blobs", "depths")      # the read-only verbs that take a strip (include/vof2d.h)
FAMILIES = ("diagnostics", "interface", "blobs", "tracers", "depths", "gauges", "dye", "frames", "stats", "scene", "solve_p_cg", "solve_p_mg", "step_mg",
            "curvature", "energy", "regrid")
FACTORS = (1, 2, 3, 4, 5, 7, 8, 15, 16)      # of vof_regrid: every odd factor has a middle child (si == 0), 15 and 16 the longest sums
NY_D = NY_TILE + NY_IDLE + NY_DYE          # dst ny of leg D: the kernels of kernels/regrid.h are destination-centred
MAX_CELLS_D = 40000                        # the larger grid of a vof_regrid pair
PRE_D = ("fresh", "stepped", "nan")        # dst before the call
REFUSALS_D = ("mixed directions", "no integer ratio", "a factor of 17", "another Lx", "PLIC with eps 0.5", "PLIC with a negative eps", "PLIC with a NaN eps",
              "a flag bit outside VOF_REGRID_PLIC", "dst == src")


# ------------------------------------------------------------------------------------------------------------ grids
def draw_grid(rng, seed):
    """nx, ny, dtype, coordinate cast, cell shape.  ny walks through every boundary value as the seed counts up (consecutive seeds
    reach them all: a slice of a few dozen cases cannot leave one out by chance); the rest is drawn."""
    ny = ALL_NY[seed % len(ALL_NY)]
    if ny in dict((t[1], t) for t in TALL) and rng.random() < 0.85:
        nx = dict((t[1], t[0]) for t in TALL)[ny]
    else:
        ok = [n for n in NX_SET if n * ny <= MAX_CELLS]
        nx = int(ok[int(rng.integers(0, len(ok)))])
    kw = {}
    cells = str(rng.choice(["default", "square", "free"]))
    if cells == "square" and nx != ny:
        kw = {"Lx": 0.1, "Ly": 0.1 * ny / nx}
    elif cells == "free":
        kw = {"Lx": float(rng.choice([0.1, 0.13, 0.07])), "Ly": float(rng.choice([0.1, 0.05, 0.2]))}
    return dict(nx=nx, ny=ny, dtype=str(rng.choice(["f64", "f32"])), cast=str(rng.choice(["f32", "none"])), cells=cells, kw=kw)


def make(api, g, ic=None, **more):
    """A handle of the drawn grid (util.engine)."""
    from util import engine
    return engine(api, g["nx"], g["ny"], g["dtype"], g["cast"], ic=ic, **dict(g["kw"], **more))


def consts_of(e):
    return {k: e.get_param(k) for k in ("dx", "dy", "dxi", "dyi", "Lx", "Ly", "dt")}


def draw_strip(rng, nx, kind=None):
    """(rows, own) of a strip whose owned rows lie inside the rows it can compute (row_lo + 1 .. row_hi - 1)."""
    kind = str(rng.choice(STRIPS)) if kind is None else kind
    if kind == "middle" and nx < 6:
        kind = "single"
    if kind == "single":
        o = int(rng.integers(1, nx + 1))
        own = (o, o)
    elif kind == "none":
        o = int(rng.integers(1, nx))
        own = (o + 1, o)
    elif kind == "middle":       # holds neither row 1 nor row nx
        a, b = sorted(int(x) for x in rng.integers(3, nx - 1, size=2))
        own = (a, b)
    else:
        a, b = sorted(int(x) for x in rng.integers(1, nx + 1, size=2))
        own = (a, b)
    lo, hi = min(own[0], own[1]), max(own[0], own[1])
    halo = int(rng.integers(1, 4))
    rows = (max(0, lo - halo), min(nx + 1, hi + halo))
    if kind == "middle":
        rows = (max(2, lo - halo), min(nx - 1, hi + halo))
    if rows[1] - rows[0] < 2:
        rows = (rows[0], rows[0] + 2) if rows[0] + 2 <= nx + 1 else (rows[1] - 2, rows[1])
    assert rows[0] + 1 <= lo and hi <= rows[1] - 1 and 0 <= rows[0] and rows[1] <= nx + 1, (kind, own, rows)
    return dict(kind=kind, rows=rows, own=own)


# ------------------------------------------------------------------------------------------------------------ fields
def neighbours(t, T):
    """t in the field's dtype and the numbers next to it on both sides, as doubles."""
    x = T(t)
    return [float(np.nextafter(x, T(-np.inf))), float(x), float(np.nextafter(x, T(np.inf)))]


def edge_pool(case, T):
    """The values of an "edges" field: the thresholds the case drew (a leg that draws none: eps 1e-6, 0.5, the range 0 .. 1) and
    their neighbours, the bin edges of the frame range, zeros, subnormals, values outside [0, 1]."""
    eps, thr, level = case.get("eps", 1e-6), case.get("thr", 0.5), case.get("level", 0.5)
    lo, hi = case.get("frame", {}).get("lo", 0.0), case.get("frame", {}).get("hi", 1.0)
    pool = []
    for t in (eps, 1.0 - eps, 0.5, thr, level, lo, hi, 0.0, 1.0):
        pool += neighbours(t, T)
    if hi > lo:                                          # means that land on the edge between two colour bins: (k + 0.5) / 255 of the range
        pool += [lo + (hi - lo) * (k + 0.5) / 255.0 for k in (0, 1, 127, 254)]
    pool += [0.0, -0.0, float(np.finfo(T).smallest_subnormal), -float(np.finfo(T).smallest_subnormal), -0.25, 1.25, 0.5, 0.5, 0.5]
    return np.array(pool, dtype=np.float64)


def blocky(rng, shape, values):
    """Values drawn per block of 1-3 x 1-3 cells: equal neighbours, so that gradients vanish along one axis or are equal along both."""
    bi, bj = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    coarse = rng.choice(values, size=(-(-shape[0] // bi), -(-shape[1] // bj)))
    return np.repeat(np.repeat(coarse, bi, axis=0), bj, axis=1)[:shape[0], :shape[1]]


def drawn_fields(case, seed, shape, kind=None, tame=False):
    """{F, u, v, p, C} of kind "lattice" or "edges", dense arrays of `shape` in the case's dtype, finite.  tame: velocities of
    the order 1e-3 (multiples of 2^-13)."""
    rng = np.random.default_rng(seed)
    T = NP[case["grid"]["dtype"]]
    kind = case["kind"] if kind is None else kind
    assert kind in ("lattice", "edges"), kind
    if kind == "lattice":
        q = int(rng.choice([4, 8]))
        lat = np.arange(q + 1) / q
        F, C, p = blocky(rng, shape, lat), blocky(rng, shape, lat), blocky(rng, shape, lat * 4.0 - 2.0)
        u, v = blocky(rng, shape, lat - 0.5), blocky(rng, shape, lat - 0.375)
    else:
        pool = edge_pool(case, T)
        F, C, p = (rng.choice(pool, size=shape) for _ in range(3))
        if rng.random() < 0.5:
            F = blocky(rng, shape, pool)
        vel = np.concatenate([pool - 0.5, pool, [0.0, -0.0, 0.25, -0.25]])
        u, v = rng.choice(vel, size=shape), rng.choice(vel, size=shape)
    if tame:
        u, v = u * 2.0 ** -10, v * 2.0 ** -10
    return {k: np.ascontiguousarray(a.astype(T)) for k, a in (("F", F), ("u", u), ("v", v), ("p", p), ("C", C))}


def sprinkle(fields, how, seed, names=("F", "u", "v", "p", "C")):
    """NaN (how = "nan") or NaN, +inf and -inf (how = "naninf") in a few cells of every named field, ghost cells included."""
    if how == "none":
        return fields
    rng = np.random.default_rng(seed)
    out = dict(fields)
    bad = [np.nan] if how == "nan" else [np.nan, np.inf, -np.inf]
    for n in names:
        a = out[n].copy()
        k = int(rng.integers(1, 4))
        a[rng.integers(0, a.shape[0], size=k), rng.integers(0, a.shape[1], size=k)] = rng.choice(bad, size=k)
        out[n] = a
    return out


def flow_fields(api, g, ic, steps, seed):
    """{F, u, v, p, C} behind `steps` steps of -ic `ic`; the dye a multiple of F that exceeds it in places."""
    e = make(api, g, ic=ic)
    e.step(steps)
    f = {n: e.get(n) for n in ("F", "u", "v", "p")}
    e.close()
    rng = np.random.default_rng(seed)
    f["C"] = (f["F"] * rng.choice([0.0, 0.5, 1.0, 1.25], size=f["F"].shape)).astype(f["F"].dtype)
    return f


def fields_of(api, case):
    """The whole-domain fields of a leg A case."""
    g = case["grid"]
    shape = (g["nx"] + 2, g["ny"] + 2)
    f = flow_fields(api, g, case["ic"], case["steps"], case["seed"]) if case["kind"] == "flow" else drawn_fields(case, case["seed"] + 1, shape)
    return sprinkle(f, case["sprinkle"], case["seed"] + 2)


# ------------------------------------------------------------------------------------------------------------ positions
def positions_of(case, c):
    """(inside (n, 2), refused (m, 2)): positions on the lattice of half cells -- faces, corners, centres --, 0, Lx and Ly themselves, a
    few anywhere; and positions the header refuses (outside the closed domain, not finite)."""
    g = case["grid"]
    rng = np.random.default_rng(case["seed"] + 3)
    nx, ny, Lx, Ly, dx, dy = g["nx"], g["ny"], c["Lx"], c["Ly"], c["dx"], c["dy"]
    p = [(0.0, 0.0), (Lx, 0.0), (0.0, Ly), (Lx, Ly)]
    for _ in range(case["npos"]):
        kx, ky = int(rng.integers(0, 2 * nx + 1)), int(rng.integers(0, 2 * ny + 1))
        p.append((min(0.5 * kx * dx, Lx), min(0.5 * ky * dy, Ly)))
    for _ in range(6):
        p += [(float(rng.choice([0.0, Lx])), min(0.5 * int(rng.integers(0, 2 * ny + 1)) * dy, Ly)),
              (min(0.5 * int(rng.integers(0, 2 * nx + 1)) * dx, Lx), float(rng.choice([0.0, Ly]))),
              (float(rng.uniform(0, Lx)), float(rng.uniform(0, Ly)))]
    inside = np.array(p, dtype=np.float64)
    refused = np.array([(-0.5 * dx, 0.5 * Ly), (float(np.nextafter(Lx, np.inf)), 0.0), (0.5 * Lx, Ly + dy), (0.5 * Lx, -1e-300), (np.nan, 0.0), (0.0, np.inf)])
    return inside, refused


# ------------------------------------------------------------------------------------------------------------ scenes
def sample_coord(cell, a, S, d):
    """The coordinate of sample a of cell `cell` (include/vof2d.h, vof_set_scene): one rounding."""
    return ((float(cell) - 1.0) + (float(a) + 0.5) * (1.0 / S)) * d


def scene_of(case, c):
    """The (n, 8) records: shapes whose edges pass through sample positions of the drawn S (closed tests: the sample is inside), and
    random ones of every kind."""
    from vof2d import scene
    g = case["grid"]
    rng = np.random.default_rng(case["seed"] + 4)
    nx, ny, S, dx, dy, Lx, Ly = g["nx"], g["ny"], case["S"], c["dx"], c["dy"], c["Lx"], c["Ly"]
    ph = lambda: str(rng.choice(["liquid", "gas"]))

    def sx():
        return sample_coord(int(rng.integers(0, nx + 2)), int(rng.integers(0, S)), S, dx)

    def sy():
        return sample_coord(int(rng.integers(0, ny + 2)), int(rng.integers(0, S)), S, dy)

    shapes = []
    for _ in range(case["nshapes"]):
        k = str(rng.choice(["halfplane_x", "halfplane_y", "box", "ellipse", "triangle", "random_box", "random_ellipse", "random_triangle", "random_halfplane"]))
        if k == "halfplane_x":          # (xs - px0) * 1 + (ys - py0) * 0 == 0 on a whole column of samples
            shapes.append(scene.halfplane(sx(), sy(), float(rng.choice([1.0, -1.0])), 0.0, ph()))
        elif k == "halfplane_y":
            shapes.append(scene.halfplane(sx(), sy(), 0.0, float(rng.choice([1.0, -1.0])), ph()))
        elif k == "box":                # |xs - cx| == hx at the sample the half extent was measured to
            cx, cy, ex, ey = sx(), sy(), sx(), sy()
            shapes.append(scene.box(cx, cy, abs(ex - cx), abs(ey - cy), 0.0, ph()))
        elif k == "ellipse":            # a disc through a sample on its horizontal axis: (r r)^2 + 0 <= (r r)^2
            cx, cy, ex = sx(), sy(), sx()
            shapes.append(scene.ellipse(cx, cy, abs(ex - cx), abs(ex - cx), 0.0, ph()))
        elif k == "triangle":           # an upright edge along a column of samples: e0 == 0 there
            x0, x2 = sx(), sx()
            shapes.append(scene.triangle((x0, sy()), (x0, sy()), (x2, sy()), ph()))
        elif k == "random_box":
            shapes.append(scene.box(rng.uniform(-0.1, 1.1) * Lx, rng.uniform(-0.1, 1.1) * Ly, rng.uniform(0, 0.4) * Lx, rng.uniform(0, 0.4) * Ly, float(rng.uniform(-90, 90)), ph()))
        elif k == "random_ellipse":
            shapes.append(scene.ellipse(rng.uniform(0, 1) * Lx, rng.uniform(0, 1) * Ly, rng.uniform(0, 0.5) * Lx, rng.uniform(0, 0.5) * Ly, float(rng.uniform(-90, 90)), ph()))
        elif k == "random_triangle":
            shapes.append(scene.triangle(*[(rng.uniform(-0.2, 1.2) * Lx, rng.uniform(-0.2, 1.2) * Ly) for _ in range(3)], ph()))
        else:
            shapes.append(scene.halfplane(rng.uniform(0, 1) * Lx, rng.uniform(0, 1) * Ly, float(rng.uniform(-1, 1)), float(rng.uniform(0.1, 1)), ph()))
    return scene.pack(shapes) if shapes else np.zeros((0, scn.N))


# ------------------------------------------------------------------------------------------------------------ the cases
def draw_frame(rng, nx, ny):
    lo, hi = RANGES[int(rng.integers(0, len(RANGES)))]
    return dict(q=str(rng.choice(QUANTITIES)), bx=int(rng.choice([1, 1, 2, 3, 4, 7, nx + 5])), by=int(rng.choice([1, 1, 2, 3, 5, ny + 5])),
                contour=bool(rng.random() < 0.5), symmetric=bool(rng.random() < 0.4), lo=lo, hi=hi, lut=bool(rng.random() < 0.5))


def second_stream(seed):
    """The generator of everything drawn for a case since its leg was first committed: the first stream, np.random.default_rng(seed),
    gives every committed seed the grid, kind, fields, positions, strip and operations it always had."""
    return np.random.default_rng([seed, 1])


def draw_a(seed):
    """Leg A: one state, every read-only verb on it, on the single domain and on a drawn strip."""
    rng = np.random.default_rng(seed)
    g = draw_grid(rng, seed)
    kind = str(rng.choice(KINDS, p=[0.2, 0.4, 0.4]))
    case = dict(leg="A", seed=seed, grid=g, kind=kind, ic=int(rng.integers(1, 4)), steps=int(rng.choice([0, 1, 3, 6])),
                sprinkle=str(rng.choice(SPRINKLES)), eps=float(rng.choice(EPS)), thr=float(rng.choice(THRESHOLDS)), level=float(rng.choice(LEVELS)),
                frame=draw_frame(rng, g["nx"], g["ny"]), npos=int(rng.integers(8, 40)),
                caps={v: str(rng.choice(CAPS)) for v in ("interface", "blobs", "tracers", "gauges", "depths", "frame")},
                strip=draw_strip(rng, g["nx"]))
    if case["sprinkle"] != "none" and case["frame"]["q"] == "VORT":      # (a difference of NaNs: module docstring)
        case["frame"]["q"] = "SPEED"
    case["cap_curv"] = str(second_stream(seed).choice(CAPS))             # (what came later is drawn from the second stream: the draws above stay)
    return case


def draw_c(seed):
    """Leg C: vof_set_scene on a drawn field, whole domain and strip, then two steps."""
    rng = np.random.default_rng(seed)
    g = draw_grid(rng, seed)
    case = dict(leg="C", seed=seed, grid=g, ic=int(rng.integers(1, 4)),
                S=int(rng.choice([1, 2, 4, 8, 16])), clear=bool(rng.random() < 0.5), nshapes=int(rng.choice([0, 1, 3, 6, 10])),
                base=str(rng.choice(["ic", "edges", "rough"])), shortcuts=int(rng.integers(0, 2)), strip=draw_strip(rng, g["nx"]))
    case["steps"] = 2 if case["clear"] or case["base"] == "ic" else 0     # (only a painted state inside [0, 1] is stepped: module docstring)
    return case


KNOBS_B = {"stats_chunk_rows": (0, 1, 3, 5, 8), "scene_shortcuts": (0, 1), "dye_fused": (0, 1), "fctx_corr_rows": (0, 1, 4, 9), "mg_nu": (1, 2, 3),
           "mg_levels": (-1, 1, 2), "mg_graph": (0, 1)}
OPS_B0 = ("step", "step_mg", "step_diag", "step_stats", "stats_hand", "step_dye", "dye_hand", "step_tracers", "tracers_hand", "step_gauges", "step_frames",
         "set_scene", "solve_p_cg", "solve_p_mg", "readonly", "knob", "overwrite", "refused_phase", "refused_strip")
OPS_B2 = ("step_energy", "regrid_out", "regrid_in")      # inserted by the second stream
OPS_B = OPS_B0 + OPS_B2
LATER = "the later verbs"                                # what a refusal of the second stream tries: every name of REFUSED_B2, one after the other
REFUSED_B2 = {"refused_phase": ("energy", "step_energy", "curvature", "regrid_src", "regrid_dst"), "refused_strip": ("energy", "step_energy", "curvature")}


def partner_grid(rng, nx, ny):
    """(nx, ny) of a grid vof_regrid pairs with nx x ny: a divisor grid (factors that leave three rows and columns), a multiple grid
    (at most MAX_CELLS_D cells) or the grid itself."""
    way = str(rng.choice(["divisor", "multiple", "multiple", "same"]))
    if way == "divisor":
        fx = [r for r in FACTORS if nx % r == 0 and nx // r >= 3]
        fy = [r for r in FACTORS if ny % r == 0 and ny // r >= 3]
        return nx // int(rng.choice(fx)), ny // int(rng.choice(fy))
    if way == "multiple":
        pairs = [(a, b) for a in (1, 2, 3, 4) for b in (1, 2, 3, 4) if a * nx * b * ny <= MAX_CELLS_D]
        a, b = pairs[int(rng.integers(0, len(pairs)))]
        return a * nx, b * ny
    return nx, ny


def insert_b(seed, g, ops):
    """0 to 2 of the operations that came later, at drawn positions of the sequence `ops`; (the new sequence, where they stand)."""
    rng = second_stream(seed)
    ops, at = list(ops), []
    for _ in range(int(rng.integers(0, 3))):
        k = str(rng.choice(OPS_B2 + ("refused_phase", "refused_strip"), p=[0.24, 0.24, 0.24, 0.14, 0.14]))
        if k == "step_energy":
            op = (k, int(rng.integers(0, 7)), int(rng.integers(1, 4)), int(rng.choice([0, 0, 1, 2])))
        elif k == "regrid_out":
            op = (k,) + partner_grid(rng, g["nx"], g["ny"]) + (str(rng.choice(["f64", "f32"])), bool(rng.random() < 0.5))
        elif k == "regrid_in":
            op = (k,) + partner_grid(rng, g["nx"], g["ny"]) + (str(rng.choice(["f64", "f32"])), int(rng.integers(1, 5)), bool(rng.random() < 0.5), bool(rng.random() < 0.3))
        else:
            op = (k, LATER)
        pos = int(rng.integers(0, len(ops) + 1))
        at = [p + (p >= pos) for p in at] + [pos]
        ops.insert(pos, op)
    return ops, sorted(at)


def draw_b(seed):
    """Leg B: a sequence of operations on one handle beside a twin that only steps."""
    rng = np.random.default_rng(seed)
    g = draw_grid(rng, seed)
    if g["nx"] * g["ny"] > 9000:                                        # (the NumPy transport of the dye twin runs beside every step)
        g["nx"] = int([n for n in NX_SET if n * g["ny"] <= 9000][-1])
        if g["cells"] == "square":
            g["kw"] = {"Lx": 0.1, "Ly": 0.1 * g["ny"] / g["nx"]}
    ops = []
    for _ in range(int(rng.integers(4, 9))):
        k = str(rng.choice(OPS_B0))
        K = int(rng.choice([0, 0, 1, 2]))
        n, every = int(rng.integers(0, 7)), int(rng.integers(1, 4))
        if k == "step":
            ops.append((k, int(rng.integers(1, 6))))
        elif k == "step_mg":
            ops.append((k, int(rng.integers(1, 4)), int(rng.integers(1, 3))))
        elif k in ("step_diag", "step_gauges"):
            ops.append((k, n, every, K))
        elif k == "step_stats":
            ops.append((k, n, every, K, int(rng.integers(1, 4)), float(rng.choice(LEVELS)), bool(rng.random() < 0.5)))
        elif k == "stats_hand":
            ops.append((k, str(rng.choice(["lattice", "edges"])), int(rng.integers(0, 1 << 30)), int(rng.integers(1, 4)), float(rng.choice(LEVELS)),
                        str(rng.choice(["none", "nan", "naninf"]))))
        elif k == "step_dye":
            ops.append((k, n, int(rng.integers(0, 3)), K, int(rng.integers(0, 1 << 30))))
        elif k == "dye_hand":
            ops.append((k, int(rng.integers(0, 1 << 30))))
        elif k == "step_tracers":
            ops.append((k, n, every, K, int(rng.integers(0, 3))))
        elif k == "tracers_hand":
            ops.append((k, float(rng.choice([0.0, 1.0, 7.0, 1e3, 1e6, -5.0]))))
        elif k == "step_frames":
            ops.append((k, n, every, K, draw_frame(rng, g["nx"], g["ny"])))
        elif k == "set_scene":
            ops.append((k, int(rng.integers(0, 1 << 30)), int(rng.choice([1, 2, 4, 8])), bool(rng.random() < 0.3)))
        elif k in ("solve_p_cg", "solve_p_mg"):
            ops.append((k, int(rng.choice([1, 2, 3, 10])), str(rng.choice(["abs", "rel"]))))
        elif k == "knob":
            name = str(rng.choice(list(KNOBS_B)))
            ops.append((k, name, int(rng.choice(KNOBS_B[name]))))
        elif k == "overwrite":
            ops.append((k, str(rng.choice(["F", "u", "v", "p"])), int(rng.integers(0, 1 << 30))))
        else:
            ops.append((k, str(rng.choice(["step_diag", "step_stats", "step_dye", "step_tracers", "step_gauges", "step_frames", "stats_sample", "dye_advance", "tracers_advance", "gauges_get"]))))
    case = dict(leg="B", seed=seed, grid=g, kind="lattice", ic=int(rng.integers(1, 4)), warm=int(rng.choice([0, 2, 5])), eager=bool(rng.random() < 0.3),
                eps=float(rng.choice(EPS)), thr=float(rng.choice(THRESHOLDS)), level=0.5, frame=draw_frame(rng, g["nx"], g["ny"]), npos=int(rng.integers(4, 16)),
                sprinkle="none", caps={v: str(rng.choice(CAPS)) for v in ("interface", "blobs", "tracers", "gauges", "depths", "frame")}, ops=ops)
    case["ops"], case["inserted"] = insert_b(seed, g, ops)
    case["cap_curv"] = str(second_stream(seed + 1).choice(CAPS))
    return case


def draw_d(seed):
    """Leg D: vof_regrid between a drawn pair of grids.  dst ny walks through NY_D as the seed counts up; everything else comes from the
    second stream (the leg has no other)."""
    rng = second_stream(seed)
    ny = NY_D[seed % len(NY_D)]
    direction = str(rng.choice(["refine", "coarsen", "copy"], p=[0.5, 0.38, 0.12]))
    rx = ry = 1
    if direction == "refine":
        fy = [r for r in FACTORS if ny % r == 0 and ny // r >= 3]              # (a prime width: along i only)
        ry = int(rng.choice(fy))
        rx = int(rng.choice(FACTORS if ry > 1 else FACTORS[1:]))
        ok = [n for n in NX_SET if n % rx == 0 and n // rx >= 3 and n * ny <= MAX_CELLS_D]
        if not ok:                                                            # (15 divides no nx of NX_SET three times: it refines along j, and coarsens)
            rx = int(rng.choice([r for r in FACTORS if (r > 1 or ry > 1) and any(n % r == 0 and n // r >= 3 for n in NX_SET)]))
            ok = [n for n in NX_SET if n % rx == 0 and n // rx >= 3 and n * ny <= MAX_CELLS_D]
        nx = int(rng.choice(ok))
        src = (nx // rx, ny // ry)
    else:
        small = [n for n in NX_SET if n * ny * 4 <= MAX_CELLS_D] or [3]
        nx = 3 if rng.random() < 0.35 else int(rng.choice(small[:6] if rng.random() < 0.6 else small))
        if direction == "coarsen":
            pairs = [(a, b) for a in FACTORS for b in FACTORS if a * b > 1 and a * nx * b * ny <= MAX_CELLS_D]
            big = max(a * b for a, b in pairs)
            if rng.random() < 0.5:                                            # the longest sums the pair of grids has room for
                pairs = [(a, b) for a, b in pairs if a * b == big]
            rx, ry = pairs[int(rng.integers(0, len(pairs)))]
        src = (rx * nx, ry * ny)
    cells = str(rng.choice(["default", "square", "free"]))
    kw = {"Lx": 0.1, "Ly": 0.1 * ny / nx} if cells == "square" and nx != ny else \
         {"Lx": float(rng.choice([0.1, 0.13, 0.07])), "Ly": float(rng.choice([0.1, 0.05, 0.2]))} if cells == "free" else {}
    cast = str(rng.choice(["f32", "none"]))
    refusal = str(rng.choice(REFUSALS_D))
    if refusal == "a factor of 17" and 17 * src[0] * src[1] > MAX_CELLS_D:
        refusal = "no integer ratio"
    if refusal == "mixed directions" and src[0] == 3 and src[1] == 3:
        refusal = "no integer ratio"
    return dict(leg="D", seed=seed, grid=dict(nx=nx, ny=ny, dtype=str(rng.choice(["f64", "f32"])), cast=cast, cells=cells, kw=kw),
                src=dict(nx=src[0], ny=src[1], dtype=str(rng.choice(["f64", "f32"])), cast=cast, cells=cells, kw=kw),
                direction=direction, rx=rx, ry=ry, plic=bool(rng.random() < 0.6), eps=float(rng.choice(EPS)), kind=str(rng.choice(KINDS, p=[0.3, 0.35, 0.35])),
                sprinkle=str(rng.choice(SPRINKLES)), ic=int(rng.integers(1, 4)), steps=int(rng.choice([1, 3, 6])), istep=int(rng.integers(0, 1000)),
                pre=str(rng.choice(PRE_D)), refusal=refusal)


def fields_d(api, case):
    """F, u, v, p of the source of a leg D case (whole-domain arrays of the source's dtype)."""
    g = case["src"]
    if case["kind"] == "flow":
        f = flow_fields(api, g, case["ic"], case["steps"], case["seed"])
    else:
        f = drawn_fields(dict(case, grid=g), [case["seed"], 2], (g["nx"] + 2, g["ny"] + 2))
    return sprinkle(f, case["sprinkle"], [case["seed"], 3], names=("F", "u", "v", "p"))


def steps_d(case):
    """Steps behind a vof_regrid: from flow sources only (module docstring)."""
    return 2 if case["kind"] == "flow" and case["sprinkle"] == "none" else 0


def round_trip_d(case):
    """The header's claim: coarsening what a refinement by powers of two made of u, v and (without PLIC) F gives the bits back."""
    wide = case["grid"]["dtype"] == "f64" or case["src"]["dtype"] == "f32"
    return (case["direction"] in ("refine", "copy") and not case["plic"] and wide and case["sprinkle"] == "none"
            and all(r & (r - 1) == 0 for r in (case["rx"], case["ry"])))


def describe(case):
    return "leg %s seed %d: %r" % (case["leg"], case["seed"], {k: v for k, v in case.items() if k not in ("leg", "seed")})


def cap_of(cls, need, rng_seed):
    """A capacity of the drawn class for a list of `need` rows; (cap, class it really is)."""
    rng = np.random.default_rng(rng_seed)
    if cls == "zero" or (cls == "short" and need <= 1):
        return 0, "zero"
    if cls == "short":
        return int(rng.integers(1, need)), "short"
    if cls == "exact":
        return need, "exact"
    return need + int(rng.integers(1, 60)), "generous"


# ------------------------------------------------------------------------------------------------------------ the census of ties
def _three(c, name, lhs, rhs, where):
    """Counts the cells of `where` on each side of the comparison lhs ? rhs and on it."""
    with np.errstate(invalid="ignore"):
        c[name + " <"] += int((where & (lhs < rhs)).sum())
        c[name + " =="] += int((where & (lhs == rhs)).sum())
        c[name + " >"] += int((where & (lhs > rhs)).sum())


IFACE_TIES = ("eps ? F", "F ? 1 - eps", "a ? b", "F ? 0.5", "(2 n2) Fm ? n1", "alpha ? b", "alpha ? a", "mxsum ? 0", "mysum ? 0")


def census_interface(c, F, eps, dx, dy, lo, hi, row0=0):
    """The comparisons of vof_interface (the intermediate values of tests/_interface_np.py, formed again term for term) on the cells
    i in [lo, hi]: how many land on either side of each, and on the tie."""
    if hi < lo:
        return
    F = np.asarray(F).astype(np.float64)
    ny = F.shape[1] - 2
    cx, cy = -1 / (2 * dx), -1 / (2 * dy)
    f = lambda di, dj: F[lo - row0 + di: hi + 1 - row0 + di, 1 + dj: ny + 1 + dj]
    with np.errstate(all="ignore"):
        F0 = f(0, 0)
        every = np.ones(F0.shape, dtype=bool)
        _three(c, "eps ? F", np.float64(eps), F0, every)
        _three(c, "F ? 1 - eps", F0, np.float64(1.0 - eps), every)
        mixed = (eps < F0) & (F0 < 1.0 - eps)
        mx1 = cx * (((f(1, 1) + f(1, 0)) - f(0, 1)) - f(0, 0)); my1 = cy * (((f(1, 1) - f(1, 0)) + f(0, 1)) - f(0, 0))
        mx2 = cx * (((f(1, 0) + f(1, -1)) - f(0, 0)) - f(0, -1)); my2 = cy * (((f(1, 0) - f(1, -1)) + f(0, 0)) - f(0, -1))
        mx3 = cx * (((f(0, 0) + f(0, -1)) - f(-1, 0)) - f(-1, -1)); my3 = cy * (((f(0, 0) - f(0, -1)) + f(-1, 0)) - f(-1, -1))
        mx4 = cx * (((f(0, 1) + f(0, 0)) - f(-1, 1)) - f(-1, 0)); my4 = cy * (((f(0, 1) - f(0, 0)) + f(-1, 1)) - f(-1, 0))
        mxsum, mysum = (((mx1 + mx2) + mx3) + mx4) / 4, (((my1 + my2) + my3) + my4) / 4
        seg = mixed & ~((np.abs(mxsum) < 1e-10) & (np.abs(mysum) < 1e-10))
        ax, by = np.abs(mxsum) * dx, np.abs(mysum) * dy
        a, b = ax / (ax + by), by / (ax + by)
        n1, n2 = np.where(a < b, a, b), np.where(a < b, b, a)
        Fm = np.where(F0 <= 0.5, F0, 1.0 - F0)
        alpha = np.where((2.0 * n2) * Fm < n1, np.sqrt(((2.0 * n1) * n2) * Fm), n2 * Fm + n1 * 0.5)
        alpha = np.where(F0 > 0.5, 1.0 - alpha, alpha)
        _three(c, "a ? b", a, b, seg)
        _three(c, "F ? 0.5", F0, 0.5, seg)
        _three(c, "(2 n2) Fm ? n1", (2.0 * n2) * Fm, n1, seg)
        _three(c, "alpha ? b", alpha, b, seg & (b > 0.0))
        _three(c, "alpha ? a", alpha, a, seg & (a > 0.0))
        _three(c, "mxsum ? 0", mxsum, 0.0, seg)
        _three(c, "mysum ? 0", mysum, 0.0, seg)
        c["segments"] += int(seg.sum())
        c["degenerate"] += int((mixed & ~seg).sum())


def young_line(F, eps, dx, dy):
    """Youngs' sums and the line of every interior cell of the dense F (kernels/interface.h, the expressions census_interface forms on
    its rows): a dict of (nx, ny) arrays."""
    F = np.asarray(F).astype(np.float64)
    nx, ny = F.shape[0] - 2, F.shape[1] - 2
    cx, cy = -1 / (2 * dx), -1 / (2 * dy)
    f = lambda di, dj: F[1 + di: nx + 1 + di, 1 + dj: ny + 1 + dj]
    with np.errstate(all="ignore"):
        F0 = f(0, 0)
        mixed = (eps < F0) & (F0 < 1.0 - eps)
        mx1 = cx * (((f(1, 1) + f(1, 0)) - f(0, 1)) - f(0, 0)); my1 = cy * (((f(1, 1) - f(1, 0)) + f(0, 1)) - f(0, 0))
        mx2 = cx * (((f(1, 0) + f(1, -1)) - f(0, 0)) - f(0, -1)); my2 = cy * (((f(1, 0) - f(1, -1)) + f(0, 0)) - f(0, -1))
        mx3 = cx * (((f(0, 0) + f(0, -1)) - f(-1, 0)) - f(-1, -1)); my3 = cy * (((f(0, 0) - f(0, -1)) + f(-1, 0)) - f(-1, -1))
        mx4 = cx * (((f(0, 1) + f(0, 0)) - f(-1, 1)) - f(-1, 0)); my4 = cy * (((f(0, 1) - f(0, 0)) + f(-1, 1)) - f(-1, 0))
        mxsum, mysum = (((mx1 + mx2) + mx3) + mx4) / 4, (((my1 + my2) + my3) + my4) / 4
        degen = mixed & (np.abs(mxsum) < 1e-10) & (np.abs(mysum) < 1e-10)
        ax, by = np.abs(mxsum) * dx, np.abs(mysum) * dy
        a, b = ax / (ax + by), by / (ax + by)
        n1, n2 = np.where(a < b, a, b), np.where(a < b, b, a)
        Fm = np.where(F0 <= 0.5, F0, 1.0 - F0)
        alpha = np.where((2.0 * n2) * Fm < n1, np.sqrt(((2.0 * n1) * n2) * Fm), n2 * Fm + n1 * 0.5)
        alpha = np.where(F0 > 0.5, 1.0 - alpha, alpha)
    return dict(F0=F0, row=mixed & ~degen, degen=degen, mxsum=mxsum, mysum=mysum, ax=ax, by=by, a=a, b=b, alpha=alpha)


CURV_TIES = ("curv: ax ? by", "curv: m ? 0", "curv: liquid end ? 1 - eps", "curv: gas end ? eps")


def census_curvature(c, F, eps, dx, dy):
    """The comparisons of vof_curvature (kernels/curvature.h) on the rows of the dense F, formed again term for term."""
    F = np.asarray(F).astype(np.float64)
    nx, ny = F.shape[0] - 2, F.shape[1] - 2
    y = young_line(F, eps, dx, dy)
    row = y["row"]
    Fp = np.pad(F, 3, mode="edge")                       # f(ii, jj) = F[clamp(ii), clamp(jj)]
    f = lambda di, dj: Fp[4 + di: 4 + di + nx, 4 + dj: 4 + dj + ny]
    with np.errstate(invalid="ignore"):
        _three(c, "curv: ax ? by", y["ax"], y["by"], row)
        along_i = y["ax"] > y["by"]
        m = np.where(along_i, y["mxsum"], y["mysum"])
        _three(c, "curv: m ? 0", m, 0.0, row)
        low = m >= 0                                     # tl = -3: the liquid end is the low one
        valid = row.copy()
        for d in (-1, 0, 1):
            lo_end, hi_end = np.where(along_i, f(-3, d), f(d, -3)), np.where(along_i, f(3, d), f(d, 3))
            liq, gas = np.where(low, lo_end, hi_end), np.where(low, hi_end, lo_end)
            _three(c, "curv: liquid end ? 1 - eps", liq, 1.0 - eps, row)
            _three(c, "curv: gas end ? eps", gas, np.float64(eps), row)
            valid &= (liq >= 1.0 - eps) & (gas <= eps)
    rows = int(row.sum())
    c["curv: VALID rows"] += int(valid.sum())
    c["curv: rows not VALID"] += rows - int(valid.sum())
    c["curv: a stencil clamped on both sides"] += int(rows > 0 and (ny <= 5 or nx <= 5))
    c["curv: more entries than scan threads with rows"] += int(rows > 0 and nx * (-(-ny // TILE)) > inp.SCAN_THREADS)
    return rows


ENERGY_TIES = ("energy: u ? 0", "energy: v ? 0", "energy: here ? 0")


def census_energy(c, f):
    """The selects of vof_energy (kernels/energy.h) on the faces of the dense F, u, v, formed again term for term."""
    F, u, v = (np.asarray(f[n]).astype(np.float64) for n in ("F", "u", "v"))
    nx, ny = F.shape[0] - 2, F.shape[1] - 2
    U, W = (slice(2, nx + 1), slice(1, ny + 1)), (slice(1, nx + 1), slice(2, ny + 1))      # the u faces, the v faces
    with np.errstate(invalid="ignore"):
        _three(c, "energy: u ? 0", u[U], 0.0, np.ones(u[U].shape, dtype=bool))
        _three(c, "energy: v ? 0", v[W], 0.0, np.ones(v[W].shape, dtype=bool))
        here_u = 0.25 * (((v[1:nx, 1:ny + 1] + v[1:nx, 2:ny + 2]) + v[2:nx + 1, 1:ny + 1]) + v[2:nx + 1, 2:ny + 2])
        here_v = 0.25 * (((u[1:nx + 1, 1:ny] + u[1:nx + 1, 2:ny + 1]) + u[2:nx + 2, 1:ny]) + u[2:nx + 2, 2:ny + 1])
        _three(c, "energy: here ? 0", here_u, 0.0, np.ones(here_u.shape, dtype=bool))
        _three(c, "energy: here ? 0", here_v, 0.0, np.ones(here_v.shape, dtype=bool))
        for F0, Fb in ((F[U], F[1:nx, 1:ny + 1]), (F[W], F[1:nx + 1, 1:ny])):
            nan = np.isnan(F0) | np.isnan(Fb)
            c["energy: a face with equal F"] += int((F0 == Fb).sum())
            c["energy: a face with unequal F"] += int(((F0 != Fb) & ~nan).sum())
            c["energy: a face between +0 and -0"] += int(((F0 == 0.0) & (Fb == 0.0) & (np.signbit(F0) != np.signbit(Fb))).sum())
            c["energy: a face with a NaN F"] += int(nan.sum())


def energy_planted(case, f):
    """The fields of a leg A case made finite, then two NaNs planted where ONE select of vof_energy alone keeps them out of a sum (a
    sprinkled NaN in F, u or v is a term of P_ADV and P_SIGMA itself: whatever a select does beside it, the sum is a NaN):
      u[i, 0], a ghost cell only the u face (i, 1) reads, as ym of VY and of ddy, with here == 0 at that face: `here > 0` takes
               (yp - w), AY = 0 * ddy is a zero and P_ADV stays finite; `here >= 0` would take (w - ym) and make it a NaN
      F[nx + 1, j], a ghost cell no density of a face reads, in a patch of equal F: kappa is a NaN in the cells around it, the skip at
               equal F makes SG a zero there, P_SIGMA and MAX_ACC_SIGMA stay finite; 0 * kappa would make them NaN and inf
    Drawn from the second stream."""
    rng = second_stream(case["seed"] + 2)
    g = {n: np.where(np.isfinite(f[n]), f[n], 0).astype(f[n].dtype) for n in ("F", "u", "v", "p")}
    nx, ny = g["F"].shape[0] - 2, g["F"].shape[1] - 2
    i = int(rng.integers(2, nx + 1))
    g["v"][i - 1:i + 1, 1:3] = 0.0                    # here of the u face (i, 1)
    g["u"][i, 0] = np.nan
    j = int(rng.integers(1, ny + 1))
    g["F"][max(nx - 2, 0):, max(j - 3, 0):j + 4] = 0.5   # equal F across every face of a cell whose kappa the NaN reaches
    g["F"][nx + 1, j] = np.nan
    return g


REGRID_TIES = ("regrid: al ? 0", "regrid: al ? s'", "regrid: al ? n1", "regrid: al ? n2", "regrid: a' ? b'")


def chunk_starts_inside(nx_dst, ny_dst, rx):
    """Whether a row chunk of k_regrid_refine begins inside a parent: k != 0 at ra."""
    R = inp.chunk_rows(nx_dst, ny_dst)
    return any(((ra - 1) % rx) != 0 for ra in range(1, nx_dst + 1, R))


def census_d(c, case, f, k):
    """What a leg D case reaches, from the fields f of its source (as uploaded, or as read back) and the source's constants k."""
    g, s, rx, ry = case["grid"], case["src"], case["rx"], case["ry"]
    nx, ny = g["nx"], g["ny"]
    for kk in (1, 2, 3, 4):
        for d, name in ((-1, "one below"), (0, "on"), (1, "one past")):
            c["regrid: dst ny %s %d columns" % (name, TILE * kk)] += int(ny == TILE * kk + d)
    c["regrid: dst ny fewer than 64 columns"] += int(ny < 64)
    c["regrid: dst ny on the 112-column stride"] += int(ny == 112)
    c["regrid: dst ny one past the 112-column stride"] += int(ny == 113)
    c["regrid: " + case["direction"]] += 1
    c["regrid: %s to %s" % (s["dtype"], g["dtype"])] += 1
    c["regrid: PLIC" if case["plic"] else "regrid: without PLIC"] += 1
    c["regrid: eps = 0"] += int(case["eps"] == 0.0)
    c["regrid: dst " + case["pre"]] += 1
    c["regrid: refused, " + case["refusal"]] += 1
    c["regrid: rx ry == 256"] += int(rx * ry == 256)
    c["regrid: a factor of 15"] += int(15 in (rx, ry))
    c["regrid: a factor of 16"] += int(16 in (rx, ry))
    c["regrid: terms no power of two"] += int(case["direction"] == "coarsen" and (rx * ry) & (rx * ry - 1) != 0)
    c["regrid: along i only"] += int(rx > 1 and ry == 1)
    c["regrid: along j only"] += int(rx == 1 and ry > 1)
    c["regrid: copy"] += int(rx == ry == 1)
    c["regrid: unequal factors"] += int(rx != ry)
    c["regrid: round trip"] += int(round_trip_d(case))
    c["regrid: steps behind it"] += int(steps_d(case) > 0)
    c["kind: " + case["kind"]] += 1
    for n in ("F", "u", "v", "p"):
        a = np.asarray(f[n])
        c["regrid: a source with NaN"] += int(np.isnan(a).any())
        c["regrid: a source with inf"] += int(np.isinf(a).any())
    if case["direction"] == "refine":
        c["regrid: a chunk that starts inside a parent"] += int(chunk_starts_inside(nx, ny, rx))
        c["regrid: si == 0"] += int(rx % 2 == 1 and rx > 1)
        c["regrid: sj == 0"] += int(ry % 2 == 1 and ry > 1)
        if case["plic"]:
            y = young_line(f["F"], case["eps"], k["dx"], k["dy"])
            c["regrid: degenerate source cells"] += int(y["degen"].sum())
            row = y["row"]
            a, b, alpha = y["a"][row], y["b"][row], y["alpha"][row]
            fx, fy = (y["mxsum"] < 0.0)[row], (y["mysum"] < 0.0)[row]
            drx, dry = float(rx), float(ry)
            every = np.ones(a.shape, dtype=bool)
            with np.errstate(all="ignore"):
                a1, b1 = a / drx, b / dry
                s1 = a1 + b1
                n1, n2 = np.where(a1 < b1, a1, b1), np.where(a1 < b1, b1, a1)
                _three(c, "regrid: a' ? b'", a1, b1, every)
                for kk in range(rx):
                    for m in range(ry):
                        k1 = np.where(fx, rx - 1 - kk, kk).astype(np.float64)
                        m1 = np.where(fy, ry - 1 - m, m).astype(np.float64)
                        al = (alpha - a * (k1 / drx)) - b * (m1 / dry)
                        _three(c, "regrid: al ? 0", al, 0.0, every)
                        _three(c, "regrid: al ? s'", al, s1, every)
                        inside = (al > 0.0) & (al < s1)
                        _three(c, "regrid: al ? n1", al, n1, inside)
                        apart = ((al - n1 * 0.5) / n2).astype(NP[g["dtype"]]) != ((al * al) / ((2.0 * n1) * n2)).astype(NP[g["dtype"]])
                        c["regrid: al == n1 where the two branches round apart"] += int((inside & (al == n1) & apart).sum())
                        _three(c, "regrid: al ? n2", al, n2, inside & ~(al < n1))
    c["cases D"] += 1


def census_fields(c, case, f, lo=1, hi=None, row0=0):
    """Ties of the blob threshold, the stats level and the top of the depths on the cells i in [lo, hi] of F."""
    F = np.asarray(f["F"]).astype(np.float64)
    ny = F.shape[1] - 2
    hi = F.shape[0] - 2 + row0 if hi is None else hi
    if hi < lo:
        return
    own = F[lo - row0: hi + 1 - row0, 1: ny + 1]
    with np.errstate(invalid="ignore"):
        c["blobs: F == threshold"] += int((own == case["thr"]).sum())
        member = own >= 0.5
        top = np.where(member, np.arange(1, ny + 1)[None, :], 0).max(axis=1)
        rows = np.nonzero(top > 0)[0]
        c["depths: the top cell holds F == 0.5"] += int((own[rows, top[rows] - 1] == 0.5).sum())
        c["depths: a row without a top"] += int((top == 0).sum())
        c["depths: the front cell holds F == 0.5"] += int((own[:, 0] == 0.5).sum())
        c["stats: Fc == level"] += int((np.fmin(np.fmax(own, 0.0), 1.0) == case["level"]).sum())


def census_frame(c, case, f, c_):
    """Ties of vof_frame: a mean on an end of the fixed range, a mean whose scaled value is a whole number + 0.5 (the edge between
    two colour bins), a mean of F equal to 0.5 under the contour."""
    s = case["frame"]
    if s["hi"] < s["lo"]:
        c["frame: inverted range (refused)"] += 1
        return
    q = fnp.__dict__[s["q"]]
    m = fnp.means_of(fnp.cells(q, f, 0.5 * c_["dxi"], 0.5 * c_["dyi"]), s["bx"], s["by"])
    lo, hi = (s["lo"], s["hi"]) if s["hi"] > s["lo"] else fnp.auto_range(m, s["symmetric"])
    c["frame: auto range" if s["lo"] == s["hi"] else "frame: fixed range"] += 1
    with np.errstate(all="ignore"):
        t = (m - lo) / (hi - lo)
        mid = t * 255.0 + 0.5
        c["frame: t == 0"] += int((t == 0.0).sum())
        c["frame: t == 1"] += int((t == 1.0).sum())
        c["frame: a mean on a bin edge"] += int(((t > 0.0) & (t < 1.0) & (mid == np.floor(mid))).sum())
        c["frame: a NaN pixel"] += int(np.isnan(m).sum())
        if s["contour"]:
            mF = m if s["q"] == "F" else fnp.means_of(fnp.cells(fnp.F, f), s["bx"], s["by"])
            c["frame: contour mean == 0.5"] += int((mF == 0.5).sum())


def census_positions(c, xy, c_, g):
    """Samples exactly on a face (floor of a whole number) and at each wall."""
    G = tnp.Grid(g["nx"], g["ny"], c_["dxi"], c_["dyi"], c_["Lx"], c_["Ly"])
    for x, y in xy.tolist():
        for which, (ox, oy) in tnp.OFFSETS.items():
            s, t = x * G.dxi + ox, y * G.dyi + oy
            c["sample: s a whole number (%s)" % which] += int(s == math.floor(s))
            c["sample: t a whole number (%s)" % which] += int(t == math.floor(t))
        c["sample: x == 0"] += int(x == 0.0)
        c["sample: x == Lx"] += int(x == G.Lx)
        c["sample: y == 0"] += int(y == 0.0)
        c["sample: y == Ly"] += int(y == G.Ly)
        ig = math.floor(x * G.dxi) + 1
        c["gauge: ig clamped"] += int(ig > G.nx or ig < 1)


def census_scene(c, recs, S, dx, dy, rows, ncols):
    """Samples that lie exactly on the edge of a shape (the closed tests decide them)."""
    xs = scn.coords(rows, S, dx).reshape(-1, 1)
    ys = scn.coords(np.arange(ncols), S, dy).reshape(1, -1)
    with np.errstate(all="ignore"):
        for rec in recs:
            kind, a = int(rec[0]), [np.float64(x) for x in rec[2:]]
            if kind in (scn.BOX, scn.ELLIPSE):
                lx, ly = scn._local(a, xs, ys)
                if kind == scn.BOX:
                    on = ((np.abs(lx) == a[2]) & (np.abs(ly) <= a[3])) | ((np.abs(ly) == a[3]) & (np.abs(lx) <= a[2]))
                else:
                    t1, t2, t3 = lx * a[3], ly * a[2], a[2] * a[3]
                    on = t1 * t1 + t2 * t2 == t3 * t3
            elif kind == scn.HALFPLANE:
                on = (xs - a[0]) * a[2] + (ys - a[1]) * a[3] == 0.0
            else:
                x0, y0, x1, y1, x2, y2 = a
                e0 = (x1 - x0) * (ys - y0) - (y1 - y0) * (xs - x0)
                e1 = (x2 - x1) * (ys - y1) - (y2 - y1) * (xs - x1)
                e2 = (x0 - x2) * (ys - y2) - (y0 - y2) * (xs - x2)
                on = scn.inside(rec, xs, ys) & ((e0 == 0.0) | (e1 == 0.0) | (e2 == 0.0))
            c["scene: a sample on an edge (%s)" % ("box", "ellipse", "halfplane", "triangle")[kind]] += int(on.sum())


def grid_classes(c, g):
    nx, ny = g["nx"], g["ny"]
    for k in (1, 2, 3, 4):
        for d, name in ((-1, "one below"), (0, "on"), (1, "one past")):
            c["grid: ny %s %d columns" % (name, TILE * k)] += int(ny == TILE * k + d)
    c["grid: ny on the 112-column stride"] += int(ny == 112)
    c["grid: ny one past the 112-column stride"] += int(ny == 113)
    for d, name in ((-1, "one below"), (0, "on"), (1, "one past")):
        c["grid: ny + 2 %s 256 columns" % name] += int(ny + 2 == 256 + d)
    c["grid: fewer than 64 columns"] += int(ny < 64)
    c["grid: the smallest nx"] += int(nx == 3)
    ntj = -(-ny // TILE)                                             # column tiles; a pass has one wave per (chunk, tile), four waves a block
    blocks = -(-(-(-nx // inp.diag_chunk_rows(nx, ny)) * ntj) // 4)  # of k_diag and its kin: one partial each, folded by the 256 threads of k_row_finish
    c["grid: more entries than scan threads"] += int(nx * ntj > inp.SCAN_THREADS)      # (row, tile) entries of k_cell_rows_scan
    c["grid: more blocks than folding threads"] += int(blocks > 256)
    c["grid: nx odd" if nx % 2 else "grid: nx even"] += 1
    for R in (4, 32):
        c["grid: nx a multiple of %d" % R] += int(nx % R == 0)
        c["grid: nx one past a multiple of %d" % R] += int(nx % R == 1 and nx > R)
    c["grid: %s" % g["dtype"]] += 1
    c["grid: cast %s" % g["cast"]] += 1


def own_rows(strip, nx):
    return max(strip["own"][0], 1), min(strip["own"][1], nx)


# ------------------------------------------------------------------------------------------------------------ the committed slice
# The fixed seeds the pytest tests of tests/test_verb_fuzz_gpu.py run and tests/test_verb_fuzz.py replays on the CPU.  The counts per
# test come from the time a case takes on the device (profiles/verb_fuzz.md); tests/test_verb_fuzz.py fixes them from below.
SEED0 = 20261020
PER_TEST = {"A": 50, "B": 16, "C": 100, "D": 20}  # cases of one pytest test (leg D: one pass over NY_D)
TESTS = {"A": 3, "B": 5, "C": 1, "D": 15}       # pytest tests of the leg: test k runs the seeds SEED0 + k * PER_TEST .. + PER_TEST - 1
FOUND = {"A": (), "B": (), "C": (), "D": (20261024,)}    # seeds the campaigns found a divergence at (profiles/verb_fuzz.md): the last test of the leg replays them
DRAW = {"A": draw_a, "B": draw_b, "C": draw_c, "D": draw_d}


def slice_seeds(leg, k=None):
    """The seeds of test k of a leg (the last one also runs the seeds the campaigns found); k = None: of all its tests."""
    if k is not None:
        return [SEED0 + k * PER_TEST[leg] + n for n in range(PER_TEST[leg])] + (list(FOUND[leg]) if k == TESTS[leg] - 1 else [])
    return [s for t in range(TESTS[leg]) for s in slice_seeds(leg, t)]


# ------------------------------------------------------------------------------------------------------------ what a case reaches
def verbs_of(case):
    """The read-only verbs of a leg A case: all of them, or those drawn on fields with +-inf (module docstring)."""
    return INF_OK if case["sprinkle"] == "naninf" else READ_ONLY


FAMILY_OF = {"diagnostics": "diagnostics", "interface": "interface", "blobs": "blobs", "depths": "depths", "frame": "frames", "dye_stats": "dye",
             "gauges": "gauges", "tracers": "tracers", "step_diag": "diagnostics", "step_stats": "stats", "stats_hand": "stats", "step_dye": "dye",
             "dye_hand": "dye", "step_tracers": "tracers", "tracers_hand": "tracers", "step_gauges": "gauges", "step_frames": "frames",
             "set_scene": "scene", "solve_p_cg": "solve_p_cg", "solve_p_mg": "solve_p_mg", "step_mg": "step_mg", "curvature": "curvature",
             "energy": "energy", "step_energy": "energy", "regrid_out": "regrid", "regrid_in": "regrid"}


def census_a(c, case, f, k, xy):
    """What a leg A case reaches, from its fields f (as uploaded, or as read back from the device), the constants k of its handle and
    its positions xy."""
    g = case["grid"]
    grid_classes(c, g)
    c["cells: square" if k["dx"] == k["dy"] else "cells: rectangular"] += 1
    c["kind: " + case["kind"]] += 1
    c["sprinkle: " + case["sprinkle"]] += 1
    verbs = verbs_of(case)
    for v in verbs:
        c["family: " + FAMILY_OF[v]] += 1
    before = c["segments"]
    census_interface(c, f["F"], case["eps"], k["dx"], k["dy"], 1, g["nx"])
    need = {"interface": c["segments"] - before, "tracers": len(xy), "gauges": len(xy)}
    for v, n in need.items():
        c["capacity: " + cap_of(case["caps"][v], n, case["seed"])[1]] += 1
    rows = census_curvature(c, f["F"], case["eps"], k["dx"], k["dy"])
    c["curv capacity: " + cap_of(case["cap_curv"], rows, case["seed"])[1]] += 1
    if "energy" in verbs:
        census_energy(c, f)
        c["energy: a NaN that only a select keeps out of a sum"] += 2      # (energy_planted: one beside here == 0, one beside equal F)
    census_fields(c, case, f)
    if "frame" in verbs:
        census_frame(c, case, f, k)
    census_positions(c, xy, k, g)
    s = case["strip"]
    c["strip: " + s["kind"]] += 1
    lo, hi = own_rows(s, g["nx"])
    c["strip: owns nothing"] += int(hi < lo)
    c["strip: without row 1 and row nx"] += int(s["rows"][0] >= 2 and s["rows"][1] <= g["nx"] - 1)
    census_interface(c, f["F"], case["eps"], k["dx"], k["dy"], lo, hi)
    c["cases A"] += 1


def census_b(c, case):
    g = case["grid"]
    grid_classes(c, g)
    shape = (g["nx"] + 2, g["ny"] + 2)
    for op in case["ops"]:
        c["op: " + op[0]] += 1
        if op[0] in FAMILY_OF:
            c["family: " + FAMILY_OF[op[0]]] += 1
        if op[0] == "stats_hand":
            f = drawn_fields(case, op[2], shape, kind=op[1])
            census_fields(c, dict(case, level=op[4]), f)
            c["kind: " + op[1]] += 1
        if op[0] in ("step_diag", "step_stats", "step_dye", "step_tracers", "step_gauges", "step_frames"):
            c["steps with multigrid cycles" if op[3] else "steps with sweeps"] += 1
        if op[0] == "regrid_in" and op[-1]:
            c["regrid_in: with fuse_tm and f_zero_map"] += 1
        if op[0] in ("refused_phase", "refused_strip") and op[1] == LATER:
            c["op: %s of the later verbs" % op[0]] += 1
    c["eager" if case["eager"] else "graphs"] += 1
    c["cases B"] += 1


def census_c(c, case, k, recs):
    g = case["grid"]
    grid_classes(c, g)
    c["family: scene"] += 1
    c["scene: S = %d" % case["S"]] += 1
    c["scene: clear" if case["clear"] else "scene: over the field"] += 1
    c["scene: shapes"] += len(recs)
    census_scene(c, recs, case["S"], k["dx"], k["dy"], np.arange(g["nx"] + 2), g["ny"] + 2)
    s = case["strip"]
    c["strip: " + s["kind"]] += 1
    c["cases C"] += 1
