"""The dye, the parts a CPU can check: vof2d/dye.py (slots, derive, box), the NumPy restatement of the statistics
(tests/_dye_np.py) against independent one-liners on committed fixtures, the twin oracle state -- a dye seeded equal to F
reproduces F at every step and ends at the golden reference run --, the command line refusals, and the new names in the
header, the binding list and the library."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _dye_np as ynp
import vof_oracle_np as onp
from test_diag import fixture
from util import load_golden
from vof2d import _abi, cli, dye

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERBS = ("dye_set", "dye_get", "dye_advance", "dye_stats", "step_dye")


# ---------------------------------------------------------------------------- the boundary
def test_header_and_bindings_name_the_verbs():
    txt = open(os.path.join(ROOT, "include", "vof2d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in VERBS:
        assert re.search(r"\bint\s+vof_%s\s*\(" % name, code), name
        assert name in _abi.SIGNATURES and name in _abi.GPU_ONLY
    for k, name in enumerate(dye.NAMES):
        assert re.search(r"#define\s+VOF_DYE_%s\s+%d\b" % (name, k), code), name
        assert getattr(_abi, "VOF_DYE_" + name) == k == getattr(dye, name)
    assert re.search(r"#define\s+VOF_DYE_N\s+16\b", code) and _abi.VOF_DYE_N == 16


def test_library_exports_the_verbs_and_checks_null(hip_api):
    for name in VERBS:
        assert hasattr(hip_api.lib, "vof_" + name), name
    buf = np.zeros((5, 5))
    row = (C.c_double * 16)()
    EINVAL = _abi.VOF_EINVAL
    assert hip_api.dye_set(None, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == EINVAL
    assert hip_api.dye_set(None, None, 0) == EINVAL
    assert hip_api.dye_get(None, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == EINVAL
    assert hip_api.dye_advance(None) == EINVAL
    assert hip_api.dye_stats(None, row) == EINVAL
    assert hip_api.step_dye(None, 1, 1, 0, 0, row, 1, None) == EINVAL


# ---------------------------------------------------------------------------- dye.py
def test_names_slots_and_derive():
    assert len(dye.NAMES) == 12 and list(dye.raw_of([float(k) for k in range(16)])) == list(dye.NAMES)
    with pytest.raises(ValueError):
        dye.raw_of([0.0] * 12)
    raw = dict(ISTEP=5.0, CELLS=8.0, SUM_C=4.0, SUM_CI=10.0, SUM_CJ=6.0, SUM_C2=3.0, SUM_CF=3.0, SUM_CU=2.0, SUM_CV=-1.0, MIN_C=0.0, MAX_C=1.0, MAX_EXCESS=0.25)
    d = dye.derive(raw, 0.5, 0.25)
    assert list(d) == list(dye.DERIVED)
    assert d == {"amount": 4.0 * 0.5 * 0.25, "xc": (2.5 - 0.5) * 0.5, "yc": (1.5 - 0.5) * 0.25, "mean": 0.5, "variance": 3.0 / 8.0 - 0.25,
                 "outside_liquid": 0.25, "u": 0.5, "v": -0.25, "C_min": 0.0, "C_max": 1.0, "excess_max": 0.25}
    e = dye.derive(dict(raw, SUM_C=0.0, SUM_C2=0.0), 0.5, 0.25)           # no dye: NaN where a share of it is asked for
    assert e["amount"] == 0.0 and e["mean"] == 0.0 and e["variance"] == 0.0 and all(math.isnan(e[k]) for k in ("xc", "yc", "outside_liquid", "u", "v"))


def test_box_is_decided_at_cell_centres():
    F = np.arange(6 * 7, dtype=np.float32).reshape(6, 7) / 64 + 0.25          # nx = 4, ny = 5
    dx, dy = 0.25, 0.2
    Cb = dye.box(F, dx, dy, 0.25, 0.75, 0.0, 0.5)                       # centres x: 0.125 (i = 1) .. 0.875; y: 0.1 (j = 1) .. 0.9
    want = np.zeros_like(F)
    want[2:4, 1:3] = F[2:4, 1:3]                                        # x in {0.375, 0.625}, y in {0.1, 0.3}: y = 0.5 is the centre of j = 3
    want[2:4, 3] = F[2:4, 3]
    assert Cb.dtype == F.dtype and np.array_equal(Cb, want)
    assert np.array_equal(dye.box(F, dx, dy, -1, 2, -1, 2), F)         # the whole field, ghost cells included
    assert not dye.box(F, dx, dy, 0.26, 0.37, 0, 1).any()               # no centre inside
    two = dye.boxes(F, dx, dy, [(0.0, 0.25, 0.0, 1.0), (0.5, 1.0, 0.0, 0.2)])
    assert np.array_equal(two, np.maximum(dye.box(F, dx, dy, 0.0, 0.25, 0.0, 1.0), dye.box(F, dx, dy, 0.5, 1.0, 0.0, 0.2)))


# ---------------------------------------------------------------------------- the restatement of the statistics
@pytest.mark.parametrize("name,step", [("ref_ic1_200_f64", 1000), ("ref_ic3_33x17_f64", 300)])
def test_restatement_against_one_liners(name, step):
    F, u, v, c = fixture(name, step)
    nx, ny = F.shape[0] - 2, F.shape[1] - 2
    rng = np.random.default_rng(3)
    Cd = F * rng.uniform(0.0, 1.25, F.shape)                             # a dye that exceeds F in places
    terms, ext, cells = ynp.restate(Cd, F, u, v)
    assert cells == nx * ny and all(t.shape == (nx, ny) and t.dtype == np.float64 for t in terms.values())
    Ci, Fi = Cd[1:-1, 1:-1], F[1:-1, 1:-1]
    ii, jj = np.meshgrid(np.arange(1, nx + 1), np.arange(1, ny + 1), indexing="ij")
    uc, vc = (u[1:-1, 1:-1] + u[2:, 1:-1]) / 2, (v[1:-1, 1:-1] + v[1:-1, 2:]) / 2
    ones = {"SUM_C": Ci.sum(), "SUM_CI": (Ci * ii).sum(), "SUM_CJ": (Ci * jj).sum(), "SUM_C2": (Ci ** 2).sum(), "SUM_CF": (Ci * np.clip(Fi, 0, 1)).sum(),
            "SUM_CU": (Ci * uc).sum(), "SUM_CV": (Ci * vc).sum()}
    for k in ynp.SUMS:                 # n 2^-52 fsum|t|: the bound of any order of summing the n terms (tests/_diag_np.py)
        print(name, k, math.fsum(terms[k].ravel()), ones[k], ynp.bound_of(terms[k]))
        assert abs(math.fsum(terms[k].ravel()) - ones[k]) <= ynp.bound_of(terms[k]), k
    assert ext == {"MIN_C": Ci.min(), "MAX_C": Ci.max(), "MAX_EXCESS": (Ci - Fi).max()} and ext["MAX_EXCESS"] > 0 and ones["SUM_CU"] != 0
    ynp.check(ynp.raw_from(terms, ext, cells, step), terms, ext, cells, istep=step, ctx=name)
    with pytest.raises(AssertionError):
        bad = ynp.raw_from(terms, ext, cells, step)
        bad["SUM_CF"] += 4 * ynp.bound_of(terms["SUM_CF"]) + 1e-300
        ynp.check(bad, terms, ext, cells)
    # the kernels' order is one of those orders, and the row it forms has its unused slots at 0
    row = ynp.row_in_kernel_order(Cd, F, u, v, 2, step)
    ynp.check(dye.raw_of(row), terms, ext, cells, istep=step, ctx=name, R=2)
    assert not row[12:].any() and row[dye.CELLS] == nx * ny
    # a NaN cell of the dye
    Cn = Cd.copy()
    Cn[3, 3] = np.nan
    terms, ext, _ = ynp.restate(Cn, F, u, v)
    assert ext == {"MIN_C": -math.inf, "MAX_C": math.inf, "MAX_EXCESS": math.inf} and all(np.isnan(t).sum() == 1 for t in terms.values())


# ---------------------------------------------------------------------------- the twin oracle state
def test_twin_state_seeded_with_F_reproduces_F_and_ends_at_the_golden_run():
    ref = load_golden("ref_ic3_33x17_f64")
    s = onp.new_state(33, 17, 3, dtype=np.float64, coord_cast="f32")
    assert np.array_equal(s.F, ref["F_0"])
    twin = ynp.Twin(s.F, np.float64, "f32")
    for k in range(1, 301):
        onp.step(s, 1)
        Cd = twin.advance(s.u, s.v, s.istep)
        assert np.array_equal(Cd, s.F), "step %d: the dye left F" % k
        if k in (2, 300):
            assert all(np.array_equal(getattr(s, f), ref["%s_%d" % (f, k)]) for f in ("F", "u", "v", "p")), k
            assert np.array_equal(Cd, ref["F_%d" % k]), k
    assert 0.0 < Cd[1:-1, 1:-1].sum() < 33 * 17


def test_twin_state_carries_the_drop_alone():
    """The dye of the drop (F inside a box around it) moves and stays in [0, 1]: every sweep ends in var(0, 1, .), post_process_f
    in var(., 0, 1).  (The FCT clipping conserves the sum only approximately; the drift is printed, not judged.)"""
    s = onp.new_state(33, 17, 3, dtype=np.float64, coord_cast="f32")
    prm = s.prm
    C0 = dye.box(s.F, prm.dx_d, prm.dy_d, 0.0, prm.Lx, 0.5 * prm.Ly, prm.Ly)
    assert 0 < C0[1:-1, 1:-1].sum() < s.F[1:-1, 1:-1].sum()
    twin = ynp.Twin(C0, np.float64, "f32")
    for _ in range(120):
        onp.step(s, 1)
        Cd = twin.advance(s.u, s.v, s.istep)
    assert Cd.min() >= 0.0 and Cd.max() <= 1.0 and not np.array_equal(Cd, C0)
    print("relative drift of the sum over 120 steps:", Cd[1:-1, 1:-1].sum() / C0[1:-1, 1:-1].sum() - 1.0, "max(C - F):", (Cd - s.F)[1:-1, 1:-1].max())

# ---------------------------------------------------------------------------- the command line
DYE = ["--dye-box", "0.0,0.05,0.0,0.1"]


@pytest.mark.parametrize("more,word", [(["--gpus", "2"], "--gpus"), (["--verbs"], "--verbs"), (["--jacobi-tol", "1e-6"], "--jacobi-tol"),
                                       (["--diag-every", "5"], "--diag-every"), (["--tracers", "100"], "--tracers"),
                                       (["--gauge", "0.01,0.01", "--gauges-every", "5"], "--gauges-every")])
def test_conflicting_options_are_refused_by_name(more, word, capsys):
    with pytest.raises(SystemExit):
        cli.parse_args(DYE + more)
    err = capsys.readouterr().err
    assert "dye" in err and word in err


@pytest.mark.parametrize("bad", [["--dye-every", "0"] + DYE, ["--dye-save-every", "-1"] + DYE, ["--dye-every", "5"], ["--dye-file", "c.npy"] + DYE])
def test_bad_dye_options_are_refused(bad, capsys):
    with pytest.raises(SystemExit):
        cli.parse_args(bad)
    assert "--dye-" in capsys.readouterr().err


@pytest.mark.parametrize("more", [["--interface-every", "10", "--blobs-every", "10", "--depths-every", "10"], ["--pressure-solver", "mg", "--mg-cycles", "2"],
                                  ["--dye-box", "0.05,0.1,0,0.02", "--dye-every", "4", "--dye-save-every", "8", "--save-every", "8"]])
def test_dye_options_are_accepted(more):
    a = cli.parse_args(DYE + more)
    assert a.dye_box[0] == DYE[1] and cli.parse_dye_boxes(a.dye_box)[0] == (0.0, 0.05, 0.0, 0.1)
    with pytest.raises(SystemExit, match="four numbers"):
        cli.parse_dye_boxes(["1,2,3"])


def test_the_oracle_backend_is_refused_with_a_message(oracle_api, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    args = cli.parse_args(["-ic", "3", "--nx", "33", "--ny", "17", "--dtype", "f64", "--steps", "2"] + DYE)
    with pytest.raises(SystemExit) as err:
        cli.run(args, api=oracle_api, world=1, rank=0, out=lambda *a: None)
    assert "dye verbs" in str(err.value) and "backend" in str(err.value)
