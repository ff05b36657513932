"""The statistics, the parts a CPU can check: the NumPy restatement of a sample (tests/_stats_np.py) against a naive judge
-- np.mean over the stacked samples, argmax over the stacked wet flags -- on runs of the NumPy oracle; vof2d/stats.py (slots,
groups, the derived quantities); and the new names in the header, the binding list and the library."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _stats_np as snp
import vof_oracle_np as onp
from vof2d import _abi, stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERBS = ("stats_begin", "stats_sample", "stats_get", "stats_summary", "step_stats")
LEVEL = 0.5
_RUNS = {}


def oracle_samples(nx, ny, ic, warm=10, every=20, count=12):
    """(F, u, v, istep) behind every `every` steps of the NumPy oracle after `warm` steps; computed once per case, never changed.
    dt = 2e-4, fifty times the default: the front crosses cells within the 250 steps, so cells get wet at different samples."""
    key = (nx, ny, ic)
    if key not in _RUNS:
        s = onp.new_state(nx, ny, ic, np.float64, "f32", dt=2e-4)
        onp.step(s, warm)
        out = []
        for _ in range(count):
            onp.step(s, every)
            out.append((s.F.copy(), s.u.copy(), s.v.copy(), int(s.istep)))
        for t in out:
            for a in t[:3]:
                a.setflags(write=False)
        _RUNS[key] = out
    return _RUNS[key]


# ---------------------------------------------------------------------------- the boundary
def test_header_and_bindings_name_the_verbs():
    txt = open(os.path.join(ROOT, "include", "vof2d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in VERBS:
        assert re.search(r"\bint\s+vof_%s\s*\(" % name, code), name
        assert name in _abi.SIGNATURES and name in _abi.GPU_ONLY
    for k, name in enumerate(stats.PLANES):
        assert re.search(r"#define\s+VOF_STATS_%s\s+%d\b" % (name, k), code), name
        assert getattr(_abi, "VOF_STATS_" + name) == k == stats.slot_of(name) and snp.PLANES[k] == name
    for k, name in enumerate(stats.SUMMARY):
        assert re.search(r"#define\s+VOF_STATS_SUM_%s\s+%d\b" % (name, k), code), name
        assert getattr(_abi, "VOF_STATS_SUM_" + name) == k and snp.SUMMARY[k] == name
    assert re.search(r"#define\s+VOF_STATS_SUM_N\s+16\b", code) and _abi.VOF_STATS_SUM_N == 16
    assert re.search(r"#define\s+VOF_STATS_PLANES\s+13\b", code) and _abi.VOF_STATS_PLANES == 13 == len(stats.PLANES)
    assert re.search(r"#define\s+VOF_STATS_MOMENTS\s+1\b", code) and re.search(r"#define\s+VOF_STATS_ENVELOPE\s+2\b", code)
    assert re.search(r"#define\s+VOF_ABI_VERSION\s+2\b", code)                         # additions only
    assert "Pressure is left out on purpose" in txt


def test_library_exports_the_verbs_and_checks_null(hip_api):
    for name in VERBS:
        assert hasattr(hip_api.lib, "vof_" + name), name
    buf = np.zeros(16)
    bp = buf.ctypes.data_as(C.POINTER(C.c_double))
    EINVAL = _abi.VOF_EINVAL
    assert hip_api.stats_begin(None, 3, 0.5) == EINVAL and hip_api.stats_sample(None) == EINVAL
    assert hip_api.stats_get(None, 0, bp, 16) == EINVAL and hip_api.stats_summary(None, bp) == EINVAL
    assert hip_api.step_stats(None, 1, 1, 0, 0, None) == EINVAL


# ---------------------------------------------------------------------------- the restatement against the naive judge
@pytest.mark.parametrize("ic", [1, 2, 3])
@pytest.mark.parametrize("nx,ny", [(32, 32), (24, 40)])
def test_the_restatement_equals_the_naive_judge(nx, ny, ic):
    samples = oracle_samples(nx, ny, ic)
    n = len(samples)
    pl, summ = snp.run(samples, 3, LEVEL)
    want = snp.naive(samples, LEVEL)
    # the means: the chain S / N against np.mean of the same terms -- only the order of summing differs.  Relative 1e-12
    for plane, key in (("SUM_F", "F_mean"), ("SUM_F2", "F2_mean"), ("SUM_U", "u_mean"), ("SUM_V", "v_mean"), ("SUM_UU", "uu_mean"), ("SUM_VV", "vv_mean"),
                       ("SUM_UV", "uv_mean"), ("SUM_FU", "Fu_mean"), ("SUM_FV", "Fv_mean")):
        got = pl[plane] / n
        scale = np.abs(want[key])
        err = np.abs(got - want[key])
        print("%dx%d ic %d %s: max |d| / scale %.3e" % (nx, ny, ic, plane, float(np.max(err / np.where(scale > 0, scale, 1.0)))))
        assert np.all(err <= 1e-12 * scale), plane
    assert np.array_equal(pl["MAX_F"], want["F_max"]) and np.array_equal(pl["MAX_SPEED2"], want["speed2_max"])
    assert np.array_equal(pl["WET"], want["wet"]) and np.array_equal(pl["ARRIVAL"], want["arrival"])
    # the flow moves: a cell was reached after the first sample, the wet time is not all or nothing
    assert (pl["ARRIVAL"] > samples[0][3]).any() and ((pl["WET"] > 0) & (pl["WET"] < n)).any()
    assert (pl["WET"] == n).any() and (pl["WET"] == 0).any() and (pl["SUM_U"] != 0).any()
    assert samples[0][3] == 30 and samples[-1][3] == 250
    assert summ == {"SAMPLES": float(n), "ISTEP_FIRST": 30.0, "ISTEP_LAST": 250.0, "MASK": 3.0, "LEVEL": LEVEL, "CELLS": float(nx * ny),
                    "EVER_WET": float((want["arrival"] >= 0).sum()), "MAX_SPEED2": float(want["speed2_max"].max())}
    # properties of the planes
    assert np.array_equal(pl["ARRIVAL"] >= 0, pl["MAX_F"] >= LEVEL) and (pl["WET"] <= n).all()
    assert (((pl["ARRIVAL"] >= 30) & (pl["ARRIVAL"] <= 250)) | (pl["ARRIVAL"] == -1)).all()
    # a group alone gives the same planes
    for mask in (1, 2):
        one, s1 = snp.run(samples, mask, LEVEL)
        assert sorted(one) == sorted(stats.planes_of(mask)) and all(np.array_equal(one[p], pl[p]) for p in one)
        assert s1["MASK"] == mask and (s1["EVER_WET"], s1["MAX_SPEED2"]) == ((summ["EVER_WET"], summ["MAX_SPEED2"]) if mask == 2 else (0.0, 0.0))


def test_nan_and_infinity_in_the_restatement():
    F, u, v, k = (a.copy() if isinstance(a, np.ndarray) else a for a in oracle_samples(24, 40, 1)[3])
    F[5, 7] = np.nan; u[10, 20] = np.nan; v[15, 30] = np.inf
    pl, summ = snp.run([(F, u, v, k)], 3, LEVEL)
    clean, _ = snp.run([oracle_samples(24, 40, 1)[3]], 3, LEVEL)
    hit = np.zeros((24, 40), bool)
    hit[4, 6] = hit[9, 19] = hit[8, 19] = hit[14, 29] = hit[14, 28] = True        # the cell of F; the two cells of a u face; of a v face
    for p in snp.PLANES:
        assert pl[p][~hit].tobytes() == clean[p][~hit].tobytes(), p
    for c in ((9, 19), (8, 19)):
        assert all(math.isnan(pl[p][c]) for p in ("SUM_U", "SUM_UU", "SUM_UV", "SUM_FU")) and pl["MAX_SPEED2"][c] == math.inf and not math.isnan(pl["SUM_V"][c])
    for c in ((14, 29), (14, 28)):
        assert pl["SUM_V"][c] == math.inf and pl["SUM_VV"][c] == math.inf and pl["MAX_SPEED2"][c] == math.inf
    # the plain clamp takes a NaN F to 0: dry, and its F sums stay finite
    assert pl["SUM_F"][4, 6] == 0.0 and pl["WET"][4, 6] == 0.0 and pl["ARRIVAL"][4, 6] == -1.0 and pl["MAX_F"][4, 6] == 0.0
    assert summ["MAX_SPEED2"] == math.inf


# ---------------------------------------------------------------------------- vof2d/stats.py
def test_groups_slots_and_names():
    assert stats.mask_of("MOMENTS,ENVELOPE") == 3 and stats.mask_of("envelope") == 2 and stats.mask_of(["moments"]) == 1 and stats.mask_of(2) == 2
    with pytest.raises(ValueError, match="unknown statistics group"):
        stats.mask_of("MOMENTS,PRESSURE")
    assert stats.planes_of(1) == stats.PLANES[:9] and stats.planes_of(2) == stats.PLANES[9:] and stats.planes_of(3) == stats.PLANES
    assert stats.slot_of("ARRIVAL") == 12 and stats.slot_of(4) == 4
    assert list(stats.summary_of([float(k) for k in range(16)])) == list(stats.SUMMARY)
    with pytest.raises(ValueError):
        stats.summary_of([0.0] * 8)


@pytest.mark.parametrize("ic", [1, 3])
def test_derived_quantities(ic):
    samples = oracle_samples(24, 40, ic)
    n = len(samples)
    pl, _ = snp.run(samples, 3, LEVEL)
    dt = 2e-4
    d = stats.derive(pl, n, dt)
    assert sorted(d) == sorted(stats.DERIVED[1] + stats.DERIVED[2])
    want = snp.naive(samples, LEVEL)
    assert np.allclose(d["F_mean"], want["F_mean"], rtol=1e-12, atol=0) and np.array_equal(d["F_mean"], pl["SUM_F"] / n)
    for k in ("F_var", "u_var", "v_var"):
        assert (d[k] >= 0).all() and not np.isnan(d[k]).any()
    assert np.array_equal(d["uv"], pl["SUM_UV"] / n - d["u_mean"] * d["v_mean"])
    dry = pl["SUM_F"] == 0
    assert dry.any() and np.isnan(d["u_liquid"][dry]).all() and np.isnan(d["v_liquid"][dry]).all()
    assert np.array_equal(d["u_liquid"][~dry], (pl["SUM_FU"] / np.where(dry, 1.0, pl["SUM_F"]))[~dry]) and not np.isnan(d["v_liquid"][~dry]).any()
    assert np.array_equal(d["wet_fraction"], pl["WET"] / n) and d["wet_fraction"].max() == 1.0 and d["wet_fraction"].min() == 0.0
    assert np.array_equal(d["max_speed"], np.sqrt(pl["MAX_SPEED2"])) and np.array_equal(d["F_max"], pl["MAX_F"])
    never = pl["ARRIVAL"] < 0
    assert never.any() and np.isnan(d["arrival_time"][never]).all() and np.array_equal(d["arrival_time"][~never], pl["ARRIVAL"][~never] * dt)
    # one group alone
    assert sorted(stats.derive({p: pl[p] for p in stats.planes_of(2)}, n, dt)) == sorted(stats.DERIVED[2])
    assert sorted(stats.derive({p: pl[p] for p in stats.planes_of(1)}, n)) == sorted(stats.DERIVED[1])
    # no sample yet: NaN where N divides
    z = stats.derive(snp.begin(24, 40, 3), 0)
    assert np.isnan(z["F_mean"]).all() and np.isnan(z["wet_fraction"]).all() and np.isnan(z["arrival_time"]).all() and (z["max_speed"] == 0).all()


def test_a_state_sampled_n_times_has_its_value_as_mean_and_no_variance():
    F, u, v, k = oracle_samples(32, 32, 3)[-1]
    n = 7
    pl, _ = snp.run([(F, u, v, k)] * n, 3, LEVEL)
    Fc, uc, vc = snp.cell_values(F, u, v)
    d = stats.derive(pl, n)
    # S = n x accumulated in a chain: each addition errs by at most half an ulp of the running sum <= n |x|, n - 1 of them; so does the
    # chain of the squares (on top of the rounding of x * x), and mean^2 doubles the relative error of the mean
    eps = 2.0 ** -53
    for mean, var, x in ((d["F_mean"], d["F_var"], Fc), (d["u_mean"], d["u_var"], uc), (d["v_mean"], d["v_var"], vc)):
        assert np.all(np.abs(mean - x) <= n * eps * np.abs(x))
        assert np.all(var >= 0) and np.all(var <= 4 * (n + 1) * eps * x * x)
    assert np.array_equal(d["F_mean"][Fc == 1.0], np.ones(int((Fc == 1.0).sum()))) and (d["F_var"][Fc == 1.0] == 0).all()      # small integers are exact
    assert np.array_equal(pl["WET"], np.where(Fc >= LEVEL, float(n), 0.0)) and set(np.unique(pl["ARRIVAL"])) <= {-1.0, float(k)}
