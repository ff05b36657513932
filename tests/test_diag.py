"""Diagnostics on the device, the parts a CPU can check: vof2d/diag.py (combine, derive), the NumPy restatement of the
kernel (tests/_diag_np.py) against independent one-liners on committed fixtures, strips that add up to the domain, the
command line option, and the two new names in the header and the binding list."""
import math
import os
import re

import numpy as np
import pytest

import _diag_np as dnp
from util import load_golden
from vof2d import _abi, cli, diag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def row(**kw):
    r = {k: 0.0 for k in diag.NAMES}
    r.update(MIN_F=math.inf, MAX_F=-math.inf)
    r.update(kw)
    return r


# ---------------------------------------------------------------------------- diag.py
def test_names_and_slots():
    assert len(diag.NAMES) == 12 and _abi.VOF_DIAG_N == 16
    assert (diag.ISTEP, diag.SUM_F, diag.SUM_DIV2, diag.MAX_DIV, diag.MIN_F, diag.MAX_F, diag.CELLS) == (0, 1, 5, 6, 9, 10, 11)
    vec = [float(k) for k in range(16)]
    raw = diag.raw_of(vec)
    assert raw["SUM_KE"] == 4.0 and raw["MAX_V"] == 8.0 and raw["CELLS"] == 11.0 and list(raw) == list(diag.NAMES)
    with pytest.raises(ValueError):
        diag.raw_of([0.0] * 12)


def test_combine():
    a = row(ISTEP=7.0, SUM_F=1.5, SUM_FI=3.0, SUM_FJ=4.0, SUM_KE=0.25, SUM_DIV2=1e-4, MAX_DIV=0.5, MAX_U=2.0, MAX_V=0.1, MIN_F=0.0, MAX_F=1.0, CELLS=6.0)
    b = row(ISTEP=7.0, SUM_F=2.5, SUM_FI=1.0, SUM_FJ=0.5, SUM_KE=0.5, SUM_DIV2=2e-4, MAX_DIV=0.25, MAX_U=3.0, MAX_V=0.05, MIN_F=-1e-9, MAX_F=0.75, CELLS=4.0)
    c = diag.combine([a, b])
    assert c == row(ISTEP=7.0, SUM_F=4.0, SUM_FI=4.0, SUM_FJ=4.5, SUM_KE=0.75, SUM_DIV2=1e-4 + 2e-4, MAX_DIV=0.5, MAX_U=3.0, MAX_V=0.1,
                    MIN_F=-1e-9, MAX_F=1.0, CELLS=10.0)
    assert diag.combine([a]) == a
    # vectors as the ABI returns them are accepted, and the sums are added in rank order
    va = [a[k] for k in diag.NAMES] + [0.0] * 4
    assert diag.combine([va, b]) == c
    x, y, z = row(SUM_F=1e16), row(SUM_F=1.0), row(SUM_F=-1e16)
    assert diag.combine([x, y, z])["SUM_F"] == (1e16 + 1.0) + -1e16 and diag.combine([x, z, y])["SUM_F"] == 1.0
    with pytest.raises(ValueError, match="istep"):
        diag.combine([a, row(ISTEP=8.0)])
    with pytest.raises(ValueError):
        diag.combine([])


def test_combine_reports_a_nan_partial_as_inf():
    a, b = row(MAX_U=1.0, MAX_DIV=2.0, MIN_F=0.0, MAX_F=1.0, SUM_KE=1.0), row(MAX_U=math.nan, MAX_DIV=1.0, MIN_F=math.nan, MAX_F=math.nan, SUM_KE=math.nan)
    for parts in ([a, b], [b, a], [b]):
        c = diag.combine(parts)
        assert c["MAX_U"] == math.inf and c["MAX_F"] == math.inf and c["MIN_F"] == -math.inf
        assert math.isnan(c["SUM_KE"])
    assert diag.combine([a, b])["MAX_DIV"] == 2.0
    assert diag.combine([row(MAX_U=math.inf), a])["MAX_U"] == math.inf


def test_derive():
    dx, dy, dt = 0.5, 0.25, 1e-3
    raw = row(ISTEP=3.0, SUM_F=4.0, SUM_FI=10.0, SUM_FJ=6.0, SUM_KE=8.0, SUM_DIV2=9.0, MAX_DIV=2.0, MAX_U=3.0, MAX_V=4.0, MIN_F=-0.5, MAX_F=1.5, CELLS=4.0)
    d = diag.derive(raw, dx, dy, dt, 2, 2)
    assert list(d) == list(diag.DERIVED)
    assert d == {"volume": 4.0 * dx * dy, "xc": (10.0 / 4.0 - 0.5) * dx, "yc": (6.0 / 4.0 - 0.5) * dy, "kinetic_energy": 8.0 * dx * dy,
                 "div_max": 2.0, "div_l2": 1.5, "u_max": 3.0, "v_max": 4.0, "cfl": dt * max(3.0 / dx, 4.0 / dy), "F_min": -0.5, "F_max": 1.5}
    # one full cell (2, 3) of a 4 x 4 grid: its centre
    one = row(SUM_F=1.0, SUM_FI=2.0, SUM_FJ=3.0, CELLS=16.0)
    d = diag.derive(one, 0.1, 0.2, dt, 4, 4)
    assert d["xc"] == 1.5 * 0.1 and d["yc"] == 2.5 * 0.2 and d["volume"] == 1.0 * 0.1 * 0.2
    # an empty liquid: NaN centroids, no exception; the rest is what it is
    d = diag.derive(row(CELLS=16.0), 0.1, 0.2, dt, 4, 4)
    assert math.isnan(d["xc"]) and math.isnan(d["yc"]) and d["volume"] == 0.0 and d["div_l2"] == 0.0 and d["cfl"] == 0.0
    # a row of the ABI as it comes
    vec = np.zeros(16)
    vec[diag.SUM_F], vec[diag.SUM_FI], vec[diag.SUM_FJ], vec[diag.CELLS] = 1.0, 2.0, 3.0, 16.0
    assert diag.derive(vec, 0.1, 0.2, dt, 4, 4)["xc"] == 1.5 * 0.1
    # a diverged field: +inf maxima give an infinite CFL number, a NaN sum a NaN energy
    d = diag.derive(row(SUM_F=1.0, MAX_U=math.inf, SUM_KE=math.nan, SUM_DIV2=math.nan, CELLS=4.0), dx, dy, dt, 2, 2)
    assert d["cfl"] == math.inf and math.isnan(d["kinetic_energy"]) and math.isnan(d["div_l2"])


# ---------------------------------------------------------------------------- the restatement
FIXTURES = [("ref_ic1_200_f64", 1000), ("ref_ic3_33x17_f64", 300)]


def fixture(name, step):
    z = load_golden(name)
    c = dict(zip((str(n) for n in z["const_names"]), (float(x) for x in z["const"])))
    return z["F_%d" % step], z["u_%d" % step], z["v_%d" % step], c


@pytest.mark.parametrize("name,step", FIXTURES)
def test_restatement_against_one_liners(name, step):
    F, u, v, c = fixture(name, step)
    nx, ny = F.shape[0] - 2, F.shape[1] - 2
    terms, ext, cells = dnp.restate(F, u, v, c["dxi"], c["dyi"], c["rho_g"], c["rho_l"])
    assert cells == nx * ny and all(t.shape == (nx, ny) and t.dtype == np.float64 for t in terms.values())
    Fi = F[1:-1, 1:-1]
    ii, jj = np.meshgrid(np.arange(1, nx + 1), np.arange(1, ny + 1), indexing="ij")
    div = (u[2:, 1:-1] - u[1:-1, 1:-1]) * c["dxi"] + (v[1:-1, 2:] - v[1:-1, 1:-1]) * c["dyi"]
    rho = c["rho_g"] * (1 - np.clip(Fi, 0, 1)) + c["rho_l"] * np.clip(Fi, 0, 1)
    ke = rho * 0.5 * (((u[1:-1, 1:-1] + u[2:, 1:-1]) * 0.5) ** 2 + ((v[1:-1, 1:-1] + v[1:-1, 2:]) * 0.5) ** 2)
    ones = {"SUM_F": Fi.sum(), "SUM_FI": (Fi * ii).sum(), "SUM_FJ": (Fi * jj).sum(), "SUM_KE": ke.sum(), "SUM_DIV2": (div ** 2).sum()}
    for k in dnp.SUMS:
        print(name, k, math.fsum(terms[k].ravel()), ones[k], dnp.bound_of(terms[k]))
        assert abs(math.fsum(terms[k].ravel()) - ones[k]) <= dnp.bound_of(terms[k]), k
    assert ext == {"MAX_DIV": np.abs(div).max(), "MAX_U": np.abs(u[1:, 1:-1]).max(), "MAX_V": np.abs(v[1:-1, 1:]).max(),
                   "MIN_F": Fi.min(), "MAX_F": Fi.max()}
    assert ones["SUM_F"] > 0 and ext["MAX_U"] > 0 and ext["MAX_DIV"] > 0          # a late step: the flow is moving
    # the check the GPU tests use accepts np.sum's order of the same terms
    dnp.check(dnp.raw_from(terms, ext, cells, step), terms, ext, cells, istep=step, ctx=name)
    with pytest.raises(AssertionError):
        bad = dnp.raw_from(terms, ext, cells, step)
        bad["SUM_KE"] += 4 * dnp.bound_of(terms["SUM_KE"]) + 1e-300
        dnp.check(bad, terms, ext, cells)


@pytest.mark.parametrize("name,step", FIXTURES)
@pytest.mark.parametrize("nstrips", [2, 3])
def test_uneven_strips_combine_to_the_domain(name, step, nstrips):
    F, u, v, c = fixture(name, step)
    nx = F.shape[0] - 2
    cuts = {2: [0, nx // 3, nx], 3: [0, nx // 5, nx // 5 + nx // 2, nx]}[nstrips]
    args = (c["dxi"], c["dyi"], c["rho_g"], c["rho_l"])
    parts = []
    for k in range(nstrips):
        lo, hi = cuts[k] + 1, cuts[k + 1]
        r0, r1 = max(0, lo - 2), min(nx + 1, hi + 2)                 # stored rows: a two-row halo, indexed from r0
        t, e, n = dnp.restate(F[r0:r1 + 1], u[r0:r1 + 1], v[r0:r1 + 1], *args, lo=lo, hi=hi, row0=r0)
        assert n == (hi - lo + 1) * (F.shape[1] - 2)
        parts.append(dnp.raw_from(t, e, n, step))
    whole = diag.combine(parts)
    terms, ext, cells = dnp.restate(F, u, v, *args)
    dnp.check(whole, terms, ext, cells, istep=step, ctx="%s in %d strips" % (name, nstrips), say=print)
    assert sum(p["CELLS"] for p in parts) == cells


def test_restatement_reports_a_nan():
    F, u, v, c = fixture("ref_ic3_33x17_f64", 300)
    u = u.copy()
    u[10, 5] = np.nan
    terms, ext, _ = dnp.restate(F, u, v, c["dxi"], c["dyi"], c["rho_g"], c["rho_l"])
    assert ext["MAX_U"] == math.inf and ext["MAX_DIV"] == math.inf and ext["MAX_V"] < math.inf
    assert np.isnan(terms["SUM_KE"]).sum() == 2 and np.isnan(terms["SUM_DIV2"]).sum() == 2 and not np.isnan(terms["SUM_F"]).any()
    Fn = F.copy()
    Fn[3, 3] = np.nan
    _, ext, _ = dnp.restate(Fn, u, v, c["dxi"], c["dyi"], c["rho_g"], c["rho_l"])
    assert ext["MIN_F"] == -math.inf and ext["MAX_F"] == math.inf


# ---------------------------------------------------------------------------- the command line
@pytest.mark.parametrize("bad", ["0", "-5"])
def test_diag_every_below_one_is_refused(bad, capsys):
    with pytest.raises(SystemExit):
        cli.parse_args(["--diag-every", bad])
    assert "--diag-every" in capsys.readouterr().err


@pytest.mark.parametrize("more", [["--pressure-solver", "mg", "--mg-cycles", "3"], ["--gpus", "2"], ["--jacobi-tol", "1e-6"], []])
def test_diag_every_is_accepted(more):
    a = cli.parse_args(["--diag-every", "10"] + more)
    assert a.diag_every == 10
    assert cli.parse_args(more).diag_every is None
    # the option decides nothing about how a run continues
    assert cli.numerics_of(a, 4e-6) == cli.numerics_of(cli.parse_args(more), 4e-6)


# ---------------------------------------------------------------------------- the boundary
def test_header_and_bindings_name_both_verbs():
    txt = open(os.path.join(ROOT, "include", "vof2d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("diagnostics", "step_diag"):
        assert re.search(r"\bint\s+vof_%s\s*\(" % name, code), name
        assert name in _abi.SIGNATURES and name in _abi.GPU_ONLY
    for k, name in enumerate(diag.NAMES):
        assert re.search(r"#define\s+VOF_DIAG_%s\s+%d\b" % (name, k), code), name
    assert re.search(r"#define\s+VOF_DIAG_N\s+16\b", code)


def test_library_exports_both_verbs_and_checks_null(hip_api):
    import ctypes as C
    assert hasattr(hip_api.lib, "vof_diagnostics") and hasattr(hip_api.lib, "vof_step_diag")
    out = (C.c_double * 16)()
    assert hip_api.diagnostics(None, out) == _abi.VOF_EINVAL
    assert hip_api.step_diag(None, 1, 1, 0, 0, out, 1, None) == _abi.VOF_EINVAL
