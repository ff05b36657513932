"""Differential fuzz of the extension verbs against their NumPy restatements (tests/_*_np.py): the grids, fields, positions, scenes,
frame specs, capacities, strips and call sequences nobody chose, drawn from a seed by tests/_verb_fuzz.py (whose module docstring
lists what is not drawn, and why).  tests/test_verb_fuzz.py judges the generators and the restatements on the CPU.

  leg A   the verbs that only read -- vof_diagnostics (with the reduction order), vof_interface, vof_blobs (both phases), vof_depths,
          vof_frame, vof_dye_stats, vof_gauges_get, vof_tracers_get, vof_curvature (with the cells of vof_interface and, on f64, the
          solver's own kappa beside it), vof_energy -- on uploaded fields, each held to its restatement by the helper
          of its own test module, then with a drawn capacity (the tail of the buffer untouched), every call twice (the same bytes),
          on the single domain and on a drawn strip where the verb takes one; where it takes none (vof_curvature, vof_energy,
          vof_step_energy, vof_regrid with the strip as src and as dst) the strip must refuse it with VOF_ESTATE
  leg B   the verbs that keep state, in a drawn sequence on ONE handle beside a twin that runs only vof_step / vof_step_mg (and the
          writes that change the state): every vof_step_* is held to its definition -- the loop on the twin with the restatement
          applied to the twin's fields at each record --, F, u, v, p and istep are compared byte for byte after every operation, a
          refused call leaves everything as it was.  vof_step_energy is held like vof_step_diag; regrid_out carries the handle's state
          onto another grid (the restatement of the twin's fields) and must leave the handle equal to its twin; regrid_in gives handle and
          twin the state of one drawn flow source on a divisor or multiple grid, in front of cached graphs, kept zero maps (fuse_tm and
          f_zero_map on both, fzmap_wrong stays 0), the dye, the statistics planes, tracers and gauges, which all go on being held
  leg C   vof_set_scene against _scene_np.paint byte for byte, ghost cells included, whole domain and strip, then two steps against
          the same state uploaded
  leg D   vof_regrid between a drawn pair of grids, dtypes and kinds of source, into a dst that is fresh, stepped or full of NaN: F, F2,
          u, v, p with their ghost rings and the summary against _regrid_np.restate, twice; src untouched; with power-of-two factors and
          no PLIC the way back gives the bits of u, v, F (the header's claim, no restatement in it); behind a flow source two steps
          beside a twin fed by vof_set_field; one drawn call the header refuses, both handles as they were

A fixed-seed slice runs as pytest tests; the same generators run as a campaign outside pytest (what it found: profiles/verb_fuzz.md):
    python tests/test_verb_fuzz_gpu.py --leg A|B|C|D --seed S --cases N [--seconds T] [--log FILE] [--lib PATH] [--slice]
        stops at the first divergence; --slice: the committed slice instead of N cases from S; --lib: another build of the library
"""
import collections
import os
import sys
import time

import numpy as np
import pytest

if __name__ == "__main__":   # (campaign mode: the paths conftest.py sets up for pytest)
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p_ in (os.path.join(ROOT, "taichi-2d-vof_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT):
        if p_ not in sys.path:
            sys.path.insert(0, p_)
    if "--lib" in sys.argv:      # (another build, before anything loads the default one: the mechanism of hip_api(fast=True))
        import vof2d._lib as _lib
        _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])

import ctypes as C

import _dye_np as ynp
import _energy_np as enp
import _frames_np as fnp
import _interface_np as inp
import _regrid_np as rnp
import _scene_np as scn
import _tracers_np as tnp
import _verb_fuzz as vf
import test_blobs_gpu as blobs_gpu
import test_curvature_gpu as curv_gpu
import test_depths_gpu as depths_gpu
import test_diag_gpu as diag_gpu
import test_energy_gpu as energy_gpu
import test_frames_gpu as frames_gpu
import test_gauges_gpu as gauges_gpu
import test_interface_gpu as iface_gpu
import test_scene_gpu as scene_gpu
import test_stats_gpu as stats_gpu
import test_tracers_gpu as tracers_gpu
from util import STATE
from vof2d import _abi, curvature, frames
from vof2d.engine import VofError

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)
UNTOUCHED = -777.25
TIMES = collections.defaultdict(list)      # seconds per case, by leg


def state_bytes(e):
    return tuple(e.get(n).tobytes() for n in STATE) + (e.istep,)


def upload(e, f):
    """F, u, v, p of the dict f (whole-domain arrays) into e, the rows it stores."""
    r = (e.row_lo, e.row_hi)
    for n in STATE:
        e.set(n, f[n][r[0]:r[1] + 1], rows=r)


def read_back(e, dye):
    f = {n: e.get(n) for n in STATE}
    if dye:
        f["C"] = e.dye_get()
    return f


# ---------------------------------------------------------------------------------------------------- the read-only verbs, one by one
def v_diagnostics(api, e, case, xy, ctx, seed):
    return diag_gpu.vec(diag_gpu.hold_to_restatement(e, ctx, bits=True)).tobytes()


def v_interface(api, e, case, xy, ctx, seed):
    nonfinite = not np.isfinite(e.get("F")).all()
    rows, summ = iface_gpu.hold_to_restatement(e, ctx, eps=case["eps"], nan=nonfinite)
    if nonfinite:                           # (the helper then compares values: here every entry that is no NaN bit for bit, the sign of a zero included)
        assert tnp.same_bits(rows, iface_gpu.restated(e, case["eps"])[0]), ctx + ": the rows that hold no NaN, bit for bit"
    n = int(summ["SEGMENTS"])
    cap, _ = vf.cap_of(case["caps"]["interface"], n, seed)
    buf = np.full((cap + 2, _abi.VOF_IFACE_N), UNTOUCHED)
    s = (C.c_double * _abi.VOF_IFACE_SUM_N)()
    assert api.interface(e.handle, case["eps"], buf.ctypes.data_as(DP) if cap else None, cap, s) == 0, ctx
    m = min(cap, n)
    assert tnp.same_bits(buf[:m], rows[:m]) and np.all(buf[m:] == UNTOUCHED), "%s: interface with room for %d of %d rows" % (ctx, cap, n)
    assert s[_abi.VOF_IFACE_SUM_SEGMENTS] == n and s[_abi.VOF_IFACE_SUM_DEGENERATE] == summ["DEGENERATE"], ctx
    assert tnp.same_bits(np.array([s[_abi.VOF_IFACE_SUM_LENGTH]]), np.array([summ["LENGTH"]])), ctx
    return buf.tobytes() + bytes(s)


def v_blobs(api, e, case, xy, ctx, seed):
    nonfinite = not all(np.isfinite(e.get(n)).all() for n in ("F", "u", "v"))
    out = b""
    for k, phase in enumerate(blobs_gpu.PHASES):
        rows, summ, lab = blobs_gpu.hold_to_restatement(e, ctx, phase, case["thr"], nan=nonfinite)
        assert tnp.same_bits(rows, blobs_gpu.restated(e, phase, case["thr"])[0]), ctx + ": every entry that is no NaN, bit for bit"
        n = int(summ["BLOBS"])
        cap, _ = vf.cap_of(case["caps"]["blobs"], n, seed + k)
        buf = np.full((cap + 2, _abi.VOF_BLOB_N), UNTOUCHED)
        s = (C.c_double * _abi.VOF_BLOB_SUM_N)()
        labels = np.full(lab.shape, -7, dtype=np.int32)
        with_labels = bool((seed + k) & 1)
        assert api.blobs(e.handle, k, case["thr"], buf.ctypes.data_as(DP) if cap else None, cap, labels.ctypes.data_as(IP) if with_labels else None,
                         labels.nbytes if with_labels else 0, s) == 0, ctx
        m = min(cap, n)
        assert tnp.same_bits(buf[:m], rows[:m]) and np.all(buf[m:] == UNTOUCHED), "%s: %s blobs with room for %d of %d rows" % (ctx, phase, cap, n)
        assert np.array_equal(labels, lab) if with_labels else np.all(labels == -7), ctx
        assert [s[i] for i in range(4)] == [summ["BLOBS"], summ["MEMBER_CELLS"], summ["MAX_CELLS"], summ["ISTEP"]], ctx
        out += buf.tobytes() + labels.tobytes()
    return out


def v_depths(api, e, case, xy, ctx, seed):
    di, dj, top, summ = depths_gpu.hold(e, ctx)
    rows, ny = len(di), e.ny
    extra = {"zero": 0, "short": -1, "exact": 0, "generous": 7}[case["caps"]["depths"]]
    if extra < 0 and rows == 0:
        extra = 0
    rc, a, b, c, s = depths_gpu.raw(api, e, rows + extra, ny + max(extra, 0), rows + max(extra, 0))
    if extra < 0:                           # a cap below the rows: refused, nothing written
        assert rc == _abi.VOF_EINVAL and (a == UNTOUCHED).all() and (b == UNTOUCHED).all() and (c == -7).all() and s == [UNTOUCHED] * 8, ctx
        return di.tobytes() + dj.tobytes() + top.tobytes()
    assert rc == 0 and tnp.same_bits(a[:rows], di) and tnp.same_bits(b[:ny], dj) and np.array_equal(c[:rows], top), ctx
    assert (a[rows:] == UNTOUCHED).all() and (b[ny:] == UNTOUCHED).all() and (c[rows:] == -7).all(), ctx + ": the tails of the depths' buffers"
    return a.tobytes() + b.tobytes() + c.tobytes() + np.array(s).tobytes()


def v_frame(api, e, case, xy, ctx, seed, spec=None):
    s = case["frame"] if spec is None else spec
    if s["q"] == "DYE" and not getattr(e, "_has_dye", False):
        s = dict(s, q="F")
    sp = frames.spec(s["q"], s["bx"], s["by"], s["lo"], s["hi"], s["contour"], s["symmetric"])
    pw, ph = fnp.shape(e.nx, e.ny, min(s["bx"], e.nx), min(s["by"], e.ny))
    if s["hi"] < s["lo"]:                   # an inverted range: refused, the outputs untouched
        rc, rgb, m, summ = frames_gpu.raw_frame(api, e.handle, sp, pw * ph * 3, pw * ph)
        assert rc == _abi.VOF_EINVAL and (rgb == 77).all() and (m == UNTOUCHED).all() and summ == [UNTOUCHED] * 8, ctx
        return b""
    lut = frames_gpu.custom_lut() if s.get("lut") else None
    e.set_frame_lut(lut)
    f = read_back(e, getattr(e, "_has_dye", False))
    rgb0, m0, summ0 = frames_gpu.hold(e, f, s["q"], s["bx"], s["by"], ctx, lut, lo=s["lo"], hi=s["hi"], contour=s["contour"], symmetric=s["symmetric"])
    extra = {"zero": 0, "short": -1, "exact": 0, "generous": 9}[case["caps"]["frame"]]
    rc, rgb, m, summ = frames_gpu.raw_frame(api, e.handle, sp, pw * ph * 3 + extra, pw * ph + max(extra, 0))
    if extra < 0:
        assert rc == _abi.VOF_EINVAL and (rgb == 77).all() and (m == UNTOUCHED).all() and summ == [UNTOUCHED] * 8, ctx
        return rgb0.tobytes() + m0.tobytes()
    assert rc == 0 and rgb[:pw * ph * 3].tobytes() == rgb0.tobytes() and (rgb[pw * ph * 3:] == 77).all(), ctx + ": the picture and its tail"
    assert m[:pw * ph].tobytes() == m0.tobytes() and (m[pw * ph:] == UNTOUCHED).all(), ctx + ": the means and their tail"
    assert summ[:7] == [summ0[k] for k in frames.SUMMARY], ctx
    return rgb.tobytes() + m.tobytes() + np.array(summ).tobytes()


def v_dye_stats(api, e, case, xy, ctx, seed):
    raw = e.dye_stats()
    Cn, F, u, v = e.dye_get(), e.get("F"), e.get("u"), e.get("v")
    terms, ext, cells = ynp.restate(Cn, F, u, v)
    ynp.check(raw, terms, ext, cells, istep=e.istep, ctx=ctx, R=inp.diag_chunk_rows(e.nx, e.ny))
    return np.array([raw[k] for k in sorted(raw)]).tobytes()


def rows_with_capacity(call, full, cls, seed, width, count_slot, ctx):
    """vof_tracers_get / vof_gauges_get with a drawn capacity: the first rows, the same summary, the tail untouched."""
    n = len(full)
    cap, _ = vf.cap_of(cls, n, seed)
    buf = np.full((cap + 2, width), UNTOUCHED)
    s = (C.c_double * 8)()
    assert call(buf.ctypes.data_as(DP) if cap else None, cap, s) == 0, ctx
    m = min(cap, n)
    assert tnp.same_bits(buf[:m], full[:m]) and np.all(buf[m:] == UNTOUCHED) and s[count_slot] == n, "%s: room for %d of %d rows" % (ctx, cap, n)
    return buf.tobytes() + bytes(s)


def refuse_positions(setter, refused, ctx):
    for bad in refused:
        a = np.ascontiguousarray(bad.reshape(1, 2))
        assert setter(a.ctypes.data_as(DP), 1) == _abi.VOF_EINVAL, "%s: the position %r was taken" % (ctx, bad.tolist())


def v_gauges(api, e, case, xy, ctx, seed, records=0, refused=()):
    finite = bool(np.isfinite(e.get("F")).all())
    if records == 0:
        e.gauges_set(xy)
    refuse_positions(lambda p, n: api.gauges_set(e.handle, p, n), refused, ctx)
    if finite:
        rows = gauges_gpu.hold(e, xy, records, ctx)
    else:                                   # (the helper's cross-check against vof_depths compares with ==, which no NaN passes)
        rows, summ = e.gauges_get()
        assert tnp.same_bits(rows, gauges_gpu.restated_rows(e, xy)) and summ == {"COUNT": len(xy), "ISTEP": e.istep, "RECORDS": records}, ctx
    return rows_with_capacity(lambda p, cap, s: api.gauges_get(e.handle, p, cap, s), rows, case["caps"]["gauges"], seed, _abi.VOF_GAUGE_N, _abi.VOF_GAUGE_SUM_COUNT, ctx)


def v_tracers(api, e, case, xy, ctx, seed, refused=()):
    e.tracers_set(xy)
    refuse_positions(lambda p, n: api.tracers_set(e.handle, p, n), refused, ctx)
    rows = tracers_gpu.hold(e, xy, 0.0, ctx)
    return rows_with_capacity(lambda p, cap, s: api.tracers_get(e.handle, p, cap, s), rows, case["caps"]["tracers"], seed, _abi.VOF_TRACER_N, _abi.VOF_TRACER_SUM_COUNT, ctx)


def same_or_both_nan(x, y):
    return x == y or (x != x and y != y)


def v_curvature(api, e, case, xy, ctx, seed):
    """vof_curvature held to its restatement at the drawn eps (every entry that is no NaN bit for bit), its cells and order to those
    of vof_interface, then the raw call with a drawn capacity; on an f64 handle with a finite F (leg A: no step follows) KAPPA_CSF
    against the solver's own kappa behind vof_get_normal_young, a yardstick the restatement has no part in."""
    eps = case["eps"]
    nonfinite = not np.isfinite(e.get("F")).all()
    rows, summ = curv_gpu.hold_to_restatement(e, ctx, eps=eps, nan=nonfinite)
    assert tnp.same_bits(rows, curv_gpu.restated(e, eps)[0]), ctx + ": the rows that hold no NaN, bit for bit"
    seg, _ = e.interface(eps)
    assert np.array_equal(rows[:, :2], seg[:, :2]), ctx + ": the cells and the order of vof_interface"
    n = int(summ["ROWS"])
    cap, _ = vf.cap_of(case["cap_curv"], n, seed)
    buf = np.full((cap + 2, _abi.VOF_CURV_N), UNTOUCHED)
    s = (C.c_double * _abi.VOF_CURV_SUM_N)()
    assert api.curvature(e.handle, eps, buf.ctypes.data_as(DP) if cap else None, cap, s) == 0, ctx
    m = min(cap, n)
    assert tnp.same_bits(buf[:m], rows[:m]) and np.all(buf[m:] == UNTOUCHED), "%s: curvature with room for %d of %d rows" % (ctx, cap, n)
    got = curvature.summary_of(list(s))
    assert set(got) == set(summ) and all(same_or_both_nan(got[k], summ[k]) for k in summ), "%s: the summary with room for %d rows: %r against %r" % (ctx, cap, got, summ)
    if case["leg"] == "A" and e.np_dtype == np.float64 and not nonfinite and e.row_lo == 0 and e.row_hi == e.nx + 1:
        e.get_normal_young()
        own = e.get("kappa")[rows[:, 0].astype(int), rows[:, 1].astype(int)]
        bad = np.flatnonzero(curv_gpu.bits(own) != curv_gpu.bits(rows[:, curvature.KAPPA_CSF]))
        assert len(bad) == 0, "%s: KAPPA_CSF differs from kappa in %d rows, first %r: %r vs %r" % (ctx, len(bad), rows[bad[0], :2], rows[bad[0], curvature.KAPPA_CSF], own[bad[0]])
    return buf.tobytes() + bytes(s)


def v_energy(api, e, case, xy, ctx, seed):
    return energy_gpu.vec(energy_gpu.hold_to_restatement(e, ctx, bits=True)).tobytes()


VERBS = {"diagnostics": v_diagnostics, "interface": v_interface, "blobs": v_blobs, "depths": v_depths, "frame": v_frame, "dye_stats": v_dye_stats,
         "gauges": v_gauges, "tracers": v_tracers, "curvature": v_curvature, "energy": v_energy}


def read_only(api, e, case, verbs, xy, ctx, refused=()):
    """Every verb of `verbs` on e, twice: held to its restatement, the same bytes both times, the state untouched."""
    before = state_bytes(e)
    for v in verbs:
        kw = {"refused": refused} if v in ("gauges", "tracers") else {}
        once = VERBS[v](api, e, case, xy, "%s %s" % (ctx, v), case["seed"], **kw)
        again = VERBS[v](api, e, case, xy, "%s %s again" % (ctx, v), case["seed"], **kw)
        assert once == again, "%s: %s gave other bytes the second time" % (ctx, v)
    assert state_bytes(e) == before, ctx + ": a read-only verb changed F, u, v, p or istep"


# ---------------------------------------------------------------------------------------------------- leg A
def run_a(api, case, c=None):
    g = case["grid"]
    e = vf.make(api, g)
    try:
        k = vf.consts_of(e)
        f = vf.fields_of(api, case)
        upload(e, f)
        e.dye_set(f["C"])
        e._has_dye = True
        xy, refused = vf.positions_of(case, k)
        ctx = "seed %d %dx%d %s %s %s" % (case["seed"], g["nx"], g["ny"], g["dtype"], case["kind"], case["sprinkle"])
        read_only(api, e, case, vf.verbs_of(case), xy, ctx, refused)
        if c is not None:
            vf.census_a(c, case, read_back(e, True), k, e.tracers()[0][:, :2])
        if "energy" in vf.verbs_of(case):    # two NaNs that only a select of vof_energy keeps out of P_ADV and P_SIGMA
            upload(e, vf.energy_planted(case, f))
            raw = energy_gpu.hold_to_restatement(e, ctx + " energy with planted NaNs", bits=True)
            assert np.isfinite([raw["P_ADV"], raw["P_SIGMA"], raw["MAX_ACC_SIGMA"]]).all() and raw["P_VISC"] != raw["P_VISC"], "%s: %r" % (ctx, raw)
        st = case["strip"]
        s = vf.make(api, g, rows=st["rows"], own=st["own"])
        try:
            upload(s, f)
            read_only(api, s, case, [v for v in vf.verbs_of(case) if v in vf.STRIP_VERBS], xy, "%s strip %r owning %r" % (ctx, st["rows"], st["own"]))
            kept = state_bytes(e), state_bytes(s)
            for v, call in (("tracers_set", lambda: s.tracers_set(xy)), ("gauges_set", lambda: s.gauges_set(xy)), ("frame", lambda: s.frame("F")),
                            ("stats_begin", lambda: s.stats_begin(3, 0.5)), ("curvature", lambda: s.curvature(case["eps"])), ("energy", s.energy),
                            ("step_energy", lambda: s.step_energy(2, 1)), ("regrid from the strip", lambda: e.regrid_from(s, eps=case["eps"])),
                            ("regrid into the strip", lambda: s.regrid_from(e, eps=case["eps"]))):
                if tuple(st["rows"]) != (0, g["nx"] + 1):       # (a handle that stores every row is a whole domain, whatever it owns)
                    refused_with(call, "VOF_ESTATE", ctx + ": %s on a strip" % v)
            assert (state_bytes(e), state_bytes(s)) == kept, ctx + ": a call refused on the strip changed a handle"
        finally:
            s.close()
    finally:
        e.close()


def refused_with(call, code, ctx):
    try:
        call()
    except VofError as err:
        assert code in str(err), "%s: refused with %s" % (ctx, err)
        return
    raise AssertionError("%s: the call was accepted" % ctx)


# ---------------------------------------------------------------------------------------------------- leg C
def run_c(api, case, c=None):
    g = case["grid"]
    e = vf.make(api, g, ic=case["ic"])
    st = case["strip"]
    s = vf.make(api, g, ic=case["ic"], rows=st["rows"], own=st["own"])
    try:
        k = vf.consts_of(e)
        recs = vf.scene_of(case, k)
        S, clear = case["S"], case["clear"]
        ctx = "seed %d %dx%d %s S %d clear %d over %s, %d shapes" % (case["seed"], g["nx"], g["ny"], g["dtype"], S, clear, case["base"], len(recs))
        if case["base"] == "ic":
            base = e.get("F")
        elif case["base"] == "rough":
            base = scene_gpu.rough_field(e, case["seed"])
        else:
            base = vf.drawn_fields(case, case["seed"] + 5, (g["nx"] + 2, g["ny"] + 2), kind="edges")["F"]
        for h, hctx in ((e, ctx), (s, ctx + " strip %r owning %r" % (st["rows"], st["own"]))):
            mine = np.ascontiguousarray(base[h.row_lo:h.row_hi + 1])
            h.set("F", mine, rows=(h.row_lo, h.row_hi))
            h.set_param("scene_shortcuts", case["shortcuts"])
            summ = h.set_scene(recs, S, clear)
            want, painted, mixed = scene_gpu.restated(h, mine, recs, S, clear)
            scene_gpu.same_bytes(h.get("F"), want, hctx + " F")
            scene_gpu.same_bytes(h.get("F2"), want, hctx + " twin")
            assert summ == {"SHAPES": float(len(recs)), "SAMPLES": float(S), "PAINTED": float(painted), "MIXED": float(mixed), "ISTEP": float(h.istep)}, hctx
        if c is not None:
            vf.census_c(c, case, k, recs)
        if case["steps"]:
            F = e.get("F")
            assert np.isfinite(F).all() and F.min() >= 0 and F.max() <= 1, ctx + ": the generator drew a painted state outside [0, 1]"
            t = vf.make(api, g)
            try:
                t.set("F", F)
                e.step(case["steps"]); t.step(case["steps"])
                assert state_bytes(e) == state_bytes(t), ctx + ": two steps behind vof_set_scene against the same F uploaded"
            finally:
                t.close()
    finally:
        e.close(); s.close()


# ---------------------------------------------------------------------------------------------------- leg B
def step_twin(b, n, K):
    if n:
        b.step_mg(n, K, "rel") if K else b.step(n)


def run_b(api, case, c=None):
    g = case["grid"]
    a = vf.make(api, g, ic=case["ic"], flags=_abi.VOF_FLAG_NO_GRAPH if case["eager"] else 0)
    b = vf.make(api, g, ic=case["ic"])
    NPT = vf.NP[g["dtype"]]
    try:
        k = vf.consts_of(a)
        G = tnp.Grid.of(a)
        shape = (g["nx"] + 2, g["ny"] + 2)
        xy, refused = vf.positions_of(case, k)
        if case["warm"]:
            a.step(case["warm"]); b.step(case["warm"])
        stats, dye, tr, ga = None, None, None, None          # what the handle keeps, restated: (mask, level, samples), Twin, [xy, time], [records]
        base = "seed %d %dx%d %s%s" % (case["seed"], g["nx"], g["ny"], g["dtype"], " eager" if case["eager"] else "")

        def need_stats(mask, level, again=False):
            nonlocal stats
            if stats is None or again:
                a.stats_begin(mask, level)
                stats = (mask, level, [])

        def need_dye(seed):
            nonlocal dye
            if dye is None:
                F = b.get("F")
                C0 = (F * np.random.default_rng(seed).choice([0.0, 0.5, 1.0], size=F.shape)).astype(NPT)
                a.dye_set(C0)
                a._has_dye = True
                dye = ynp.Twin(C0, NPT, g["cast"], **g["kw"])

        def hold_kept(ctx):
            if stats is not None:
                stats_gpu.hold(a, stats[0], stats[2], stats[1], ctx)
            if dye is not None:
                assert a.dye_get().tobytes() == dye.C.astype(NPT).tobytes(), ctx + ": the dye"
            if tr is not None:
                tracers_gpu.hold(a, tr[0], tr[1], ctx)
            if ga is not None:
                v_gauges(api, a, case, xy, ctx, case["seed"], records=ga[0]) if ga[0] else gauges_gpu.hold(a, xy, 0, ctx)

        for n, op in enumerate(case["ops"]):
            ctx = "%s op %d %r" % (base, n, op)
            kind = op[0]
            if kind == "step":
                a.step(op[1]); b.step(op[1])
            elif kind == "step_mg":
                ra, rb = a.step_mg(op[1], op[2]), b.step_mg(op[1], op[2])
                assert np.array(ra).tobytes() == np.array(rb).tobytes(), ctx
            elif kind == "step_diag":
                _, nsteps, every, K = op
                rows = a.step_diag(nsteps, every, K)
                assert len(rows) == nsteps // every, ctx
                for r in range(nsteps // every):
                    step_twin(b, every, K)
                    want = diag_gpu.vec(diag_gpu.hold_to_restatement(b, ctx + " row %d on the twin" % r, bits=True))
                    assert rows[r].tobytes() == want.tobytes(), "%s: row %d" % (ctx, r)
                step_twin(b, nsteps % every, K)
            elif kind == "step_stats":
                _, nsteps, every, K, mask, level, again = op
                need_stats(mask, level, again)
                assert a.step_stats(nsteps, every, K) == nsteps // every, ctx
                for r in range(nsteps // every):
                    step_twin(b, every, K)
                    stats[2].append(stats_gpu.fields_of(b))
                step_twin(b, nsteps % every, K)
            elif kind == "stats_hand":
                _, fkind, seed, mask, level, spr = op
                need_stats(mask, level)
                saved = {f: b.get(f) for f in ("F", "u", "v")}
                f = vf.sprinkle(vf.drawn_fields(dict(case, level=stats[1]), seed, shape, kind=fkind), spr, seed + 1, names=("F", "u", "v"))
                for h in (a, b):
                    for name in ("F", "u", "v"):
                        h.set(name, f[name])
                a.stats_sample()
                stats[2].append((f["F"], f["u"], f["v"], a.istep))
                if c is not None:
                    vf.census_fields(c, dict(case, level=stats[1]), {"F": a.get("F")})
                stats_gpu.hold(a, stats[0], stats[2], stats[1], ctx)
                for h in (a, b):
                    for name in ("F", "u", "v"):
                        h.set(name, saved[name])
            elif kind == "step_dye":
                _, nsteps, every, K, seed = op
                need_dye(seed)
                rows = a.step_dye(nsteps, every, K)
                want, R = [], inp.diag_chunk_rows(g["nx"], g["ny"])
                for s_ in range(nsteps):
                    step_twin(b, 1, K)
                    u, v = b.get("u"), b.get("v")
                    dye.advance(u, v, b.istep)
                    if every and (s_ + 1) % every == 0:
                        want.append(ynp.row_in_kernel_order(dye.C.astype(NPT), b.get("F"), u, v, R, b.istep))
                assert rows.tobytes() == np.array(want).reshape(-1, _abi.VOF_DYE_N).tobytes(), ctx + ": the rows"
            elif kind == "dye_hand":
                dye = None
                need_dye(op[1])
                a.dye_advance()
                dye.advance(b.get("u"), b.get("v"), b.istep)
                v_dye_stats(api, a, case, xy, ctx, 0)
            elif kind in ("step_tracers", "tracers_hand"):
                if tr is None:
                    a.tracers_set(xy)
                    tr = [xy.copy(), 0.0]
                if kind == "tracers_hand":
                    h_ = op[1] * k["dt"]
                    a.tracers_advance(h_)
                    _, u, v = tracers_gpu.restated_fields(b)
                    tr = [tnp.advance(u, v, tr[0], h_, G), tr[1] + h_]
                else:
                    _, nsteps, every, K, snap_every = op
                    snaps = a.step_tracers(nsteps, every, K, "rel", snap_every)
                    want = []
                    for r in range(nsteps // every):
                        step_twin(b, every, K)
                        Ff, u, v = tracers_gpu.restated_fields(b)
                        h_ = float(every) * k["dt"]
                        tr = [tnp.advance(u, v, tr[0], h_, G), tr[1] + h_]
                        if snap_every and (r + 1) % snap_every == 0:
                            want.append(tnp.rows(Ff, u, v, tr[0], G))
                    step_twin(b, nsteps % every, K)
                    assert len(snaps) == len(want) and all(tnp.same_bits(x, y) for x, y in zip(snaps, want)), ctx + ": the snapshots"
            elif kind == "step_gauges":
                _, nsteps, every, K = op
                if ga is None:
                    a.gauges_set(xy)
                    ga = [0]
                recs = a.step_gauges(nsteps, every, K)
                assert len(recs) == nsteps // every, ctx
                for r in range(nsteps // every):
                    step_twin(b, every, K)
                    assert tnp.same_bits(recs[r], gauges_gpu.restated_rows(b, xy)), "%s: record %d" % (ctx, r)
                step_twin(b, nsteps % every, K)
                ga[0] += nsteps // every
            elif kind == "step_frames":
                _, nsteps, every, K, s = op
                if s["q"] == "DYE":
                    need_dye(case["seed"])
                kw = dict(quantity=s["q"], bx=s["bx"], by=s["by"], lo=s["lo"], hi=s["hi"], contour=s["contour"], symmetric=s["symmetric"], mg_cycles=K)
                if s["hi"] < s["lo"]:
                    before = state_bytes(a)
                    refused_with(lambda: a.step_frames(nsteps, every, **kw), "VOF_EINVAL", ctx)
                    assert state_bytes(a) == before, ctx
                else:
                    lut = frames_gpu.custom_lut() if s["lut"] else None
                    a.set_frame_lut(lut)
                    pics, summs = a.step_frames(nsteps, every, **kw)
                    assert len(pics) == nsteps // every, ctx
                    flags = (fnp.CONTOUR if s["contour"] else 0) | (fnp.SYMMETRIC if s["symmetric"] else 0)
                    for r in range(nsteps // every):
                        step_twin(b, every, K)
                        f = read_back(b, False)
                        if dye is not None:
                            f["C"] = dye.C.astype(NPT)
                        wrgb, _, wsum = fnp.frame(frames.QUANTITIES[s["q"]], f, s["bx"], s["by"], flags, s["lo"], s["hi"], lut, b.istep, 0.5 * k["dxi"], 0.5 * k["dyi"])
                        assert pics[r].tobytes() == wrgb.tobytes(), "%s: frame %d" % (ctx, r)
                        assert np.array([summs[r][q] for q in frames.SUMMARY] + [0.0]).tobytes() == wsum.tobytes(), "%s: summary %d" % (ctx, r)
                    step_twin(b, nsteps % every, K)
            elif kind == "set_scene":
                _, seed, S, clear = op
                recs = vf.scene_of(dict(case, seed=seed, S=S, nshapes=int(seed % 7)), k)
                F0 = b.get("F")
                want, painted, mixed = scn.paint(F0, recs, S, clear, k["dx"], k["dy"])
                for h in (a, b):
                    summ = h.set_scene(recs, S, clear)
                    assert (summ["PAINTED"], summ["MIXED"]) == (painted, mixed), ctx
                scene_gpu.same_bytes(a.get("F"), want, ctx)
            elif kind in ("solve_p_cg", "solve_p_mg"):
                args = (1e-9, op[1], 2, op[2])
                ra, rb = getattr(a, kind)(*args), getattr(b, kind)(*args)
                assert np.array(ra).tobytes() == np.array(rb).tobytes(), "%s: %r against %r" % (ctx, ra, rb)
            elif kind == "step_energy":
                _, nsteps, every, K = op
                rows = a.step_energy(nsteps, every, K, "rel")
                assert rows.shape == (nsteps // every, _abi.VOF_ENERGY_N), ctx
                for r in range(nsteps // every):
                    step_twin(b, every, K)
                    want = energy_gpu.vec(energy_gpu.hold_to_restatement(b, ctx + " row %d on the twin" % r, bits=True))
                    assert rows[r].tobytes() == want.tobytes(), "%s: row %d" % (ctx, r)
                step_twin(b, nsteps % every, K)
            elif kind == "regrid_out":          # "src is otherwise unchanged": the comparison with the twin below
                _, pnx, pny, dtype, plic = op
                d = vf.make(api, dict(g, nx=pnx, ny=pny, dtype=dtype))
                try:
                    summ = d.regrid_from(a, plic=plic, eps=case["eps"])
                    want, wsum = rnp.restate(read_back(b, False), pnx, pny, d.np_dtype, plic=plic, eps=case["eps"], dx=k["dx"], dy=k["dy"], istep=b.istep)
                    held_to_regrid(d, want, summ, wsum, True, ctx)
                finally:
                    d.close()
            elif kind == "regrid_in":           # what dst keeps is "left alone": hold_kept below; the eager handle and the graph-caching twin go on alike
                _, pnx, pny, dtype, nsteps, plic, tm = op
                src = vf.make(api, dict(g, nx=pnx, ny=pny, dtype=dtype), ic=case["ic"])
                try:
                    src.step(nsteps)
                    if tm:
                        for h in (a, b):
                            h.set_param("fuse_tm", 1); h.set_param("f_zero_map", 1)
                    fs = read_back(src, False)
                    want, wsum = rnp.restate(fs, g["nx"], g["ny"], NPT, plic=plic, eps=case["eps"], dx=src.get_param("dx"), dy=src.get_param("dy"), istep=nsteps)
                    for h in (a, b):
                        held_to_regrid(h, want, h.regrid_from(src, plic=plic, eps=case["eps"]), wsum, True, ctx)
                    assert tuple(src.get(n).tobytes() for n in STATE) == tuple(fs[n].tobytes() for n in STATE) and src.istep == nsteps, ctx + ": src changed"
                finally:
                    src.close()
            elif kind == "readonly":
                read_only(api, a, case, ["diagnostics", "interface", "blobs", "depths", "frame", "curvature", "energy"] + (["dye_stats"] if dye is not None else []), xy, ctx)
            elif kind == "knob":
                for h in ((a, b) if op[1] in ("mg_nu", "mg_levels") else (a,)):
                    h.set_param(op[1], op[2])
            elif kind == "overwrite":        # the "set" of tests/test_fuzz_gpu.py: a perturbation the flow stays tame under
                rng = np.random.default_rng(op[2])
                x = b.get(op[1]).astype(np.float64)
                if op[1] == "F":
                    x = np.clip(x + 0.3 * rng.standard_normal(x.shape) * (rng.random(x.shape) < 0.1), 0, 1)
                elif op[1] == "p":
                    x = x + rng.standard_normal(x.shape) * 10.0 ** rng.integers(-3, 3)
                else:
                    x = x + 1e-3 * rng.standard_normal(x.shape)
                for h in (a, b):
                    h.set(op[1], x)
            elif kind == "refused_phase":
                a.step_phase(0)
                call = {"step_diag": lambda: a.step_diag(2, 1), "step_stats": lambda: a.step_stats(2, 1), "step_dye": lambda: a.step_dye(2, 1),
                        "step_tracers": lambda: a.step_tracers(2, 1), "step_gauges": lambda: a.step_gauges(2, 1), "step_frames": lambda: a.step_frames(2, 1),
                        "stats_sample": a.stats_sample, "dye_advance": a.dye_advance, "tracers_advance": lambda: a.tracers_advance(1e-5),
                        "gauges_get": a.gauges_get, "energy": a.energy, "step_energy": lambda: a.step_energy(2, 1), "curvature": lambda: a.curvature(case["eps"]),
                        "regrid_src": lambda: other.regrid_from(a, eps=case["eps"]), "regrid_dst": lambda: a.regrid_from(other, eps=case["eps"])}
                other = vf.make(api, g, ic=case["ic"]) if op[1] == vf.LATER else None
                try:
                    kept = state_bytes(other) if other else None
                    for name in (vf.REFUSED_B2[kind] if op[1] == vf.LATER else (op[1],)):
                        refused_with(call[name], "VOF_ESTATE", "%s: %s" % (ctx, name))      # (what it must not have changed: the comparison with the twin below)
                    assert other is None or state_bytes(other) == kept, ctx + ": the other handle of a refused vof_regrid changed"
                finally:
                    if other:
                        other.close()
                a.step_phase(1); a.step_phase(2)
                b.step(1)
            elif kind == "refused_strip":
                half = max(g["nx"] // 2, 1)
                s = vf.make(api, g, ic=case["ic"], rows=(0, min(half + 2, g["nx"] + 1)), own=(1, half))
                try:
                    before = state_bytes(s)
                    call = {"step_diag": lambda: s.step_diag(2, 1), "step_stats": lambda: s.step_stats(2, 1), "step_dye": lambda: s.step_dye(2, 1),
                            "step_tracers": lambda: s.step_tracers(2, 1), "step_gauges": lambda: s.step_gauges(2, 1), "step_frames": lambda: s.step_frames(2, 1),
                            "stats_sample": s.stats_sample, "dye_advance": s.dye_advance, "tracers_advance": lambda: s.tracers_advance(1e-5),
                            "gauges_get": s.gauges_get, "energy": s.energy, "step_energy": lambda: s.step_energy(2, 1), "curvature": lambda: s.curvature(case["eps"])}
                    for name in (vf.REFUSED_B2[kind] if op[1] == vf.LATER else (op[1],)):
                        refused_with(call[name], "VOF_ESTATE", "%s: %s" % (ctx, name))
                    assert state_bytes(s) == before, ctx + ": a refused call changed the strip"
                finally:
                    s.close()
            else:
                raise AssertionError("unknown operation %r" % (op,))
            sa, sb = state_bytes(a), state_bytes(b)
            if sa != sb:
                bad = [f for f, x, y in zip(STATE + ("istep",), sa, sb) if x != y]
                raise AssertionError("%s: %s differ between the handle and its twin" % (ctx, ", ".join(bad)))
            assert all(np.isfinite(b.get(f)).all() for f in STATE), ctx + ": the generator drew a sequence that leaves a non-finite state"
            assert a.get_counter("courant_violations") == b.get_counter("courant_violations"), ctx
            assert a.get_counter("fzmap_wrong") == 0 and b.get_counter("fzmap_wrong") == 0, ctx + ": a kept zero map stands over a cell that is no zero"
            hold_kept(ctx + ", what the handle keeps")
        if c is not None:
            vf.census_b(c, case)
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------------- leg D
def held_to_regrid(d, want, summ, wsum, finite, ctx):
    """F, u, v, p of d with their ghost rings, F2 and the summary against the restatement: byte for byte, or, behind a source that
    is not finite, every entry that is no NaN bit for bit and the NaNs in the same places (module docstring of tests/_verb_fuzz.py)."""
    for n in STATE + ("F2",):
        got, w = d.get(n), want["F" if n == "F2" else n]
        assert got.dtype == w.dtype, ctx
        same = got.tobytes() == w.tobytes() if finite else tnp.same_bits(got, w)
        assert same, "%s: %s of dst differs from the restatement in %d cells" % (ctx, n, int(((got != w) & ~(np.isnan(got) & np.isnan(w))).sum()))
    if summ is not None:
        assert set(summ) == set(wsum) and all(same_or_both_nan(summ[q], wsum[q]) for q in wsum), "%s: the summary %r against %r" % (ctx, summ, wsum)
    assert not d.get("u")[0].any() and not np.signbit(d.get("u")[0]).any() and not d.get("v")[:, 0].any() and not np.signbit(d.get("v")[:, 0]).any(), \
        ctx + ": row 0 of u and column 0 of v are +0"


def refusal_d(api, case, src, dst, ctx):
    """The drawn call vof_regrid must refuse with VOF_EINVAL, both handles byte for byte as they were."""
    why, gs, gd = case["refusal"], case["src"], case["grid"]
    summ = (C.c_double * _abi.VOF_REGRID_SUM_N)()
    PLIC = _abi.VOF_REGRID_PLIC
    other = None
    if why == "mixed directions":
        shape = (2 * gs["nx"], gs["ny"] - 1) if gs["ny"] > 3 else (gs["nx"] - 1, 2 * gs["ny"])
        other = vf.make(api, dict(gs, nx=shape[0], ny=shape[1]))
    elif why == "no integer ratio":
        other = vf.make(api, dict(gs, nx=2 * gs["nx"] + 1, ny=2 * gs["ny"]))
    elif why == "a factor of 17":
        other = vf.make(api, dict(gs, nx=17 * gs["nx"]))
    elif why == "another Lx":
        other = vf.make(api, dict(gd, kw=dict(gd["kw"], Lx=2.0 * dst.get_param("Lx"), Ly=dst.get_param("Ly"))))
    try:
        pairs = [(other, src), (src, other)] if other is not None else [(src, src)] if why == "dst == src" else [(dst, src)]
        flags = 2 | (PLIC if case["plic"] else 0) if why.startswith("a flag bit") else PLIC if why.startswith("PLIC") else (PLIC if case["plic"] else 0)
        eps = {"PLIC with eps 0.5": 0.5, "PLIC with a negative eps": -1e-9, "PLIC with a NaN eps": float("nan")}.get(why, case["eps"])
        for x, y in pairs:
            before = state_bytes(x), state_bytes(y)
            rc = api.regrid(x.handle, y.handle, flags, eps, summ)
            assert rc == _abi.VOF_EINVAL, "%s: %s answered %d" % (ctx, why, rc)
            assert (state_bytes(x), state_bytes(y)) == before, "%s: the refused call (%s) changed a handle" % (ctx, why)
    finally:
        if other is not None:
            other.close()


def run_d(api, case, c=None):
    gd, gs = case["grid"], case["src"]
    src = vf.make(api, gs)
    pre = case["pre"]
    dst = vf.make(api, gd, ic=case["ic"] if pre == "stepped" else None)
    extra = []
    try:
        f = vf.fields_d(api, case)
        upload(src, f)
        src.istep = case["istep"]
        fs = read_back(src, False)
        finite = all(np.isfinite(fs[n]).all() for n in STATE)
        ctx = "seed %d %dx%d %s -> %dx%d %s %s %s%s eps %r, dst %s" % (case["seed"], gs["nx"], gs["ny"], gs["dtype"], gd["nx"], gd["ny"], gd["dtype"], case["kind"],
                                                                   case["sprinkle"], " PLIC" if case["plic"] else "", case["eps"], pre)
        if pre == "stepped":                 # graphs cached, ghost cells virtual
            dst.step(3)
        elif pre == "nan":                   # every cell of dst must come out "a function of the source alone"
            for n in STATE:
                dst.set(n, np.full((gd["nx"] + 2, gd["ny"] + 2), np.nan))
        want, wsum = rnp.restate(fs, gd["nx"], gd["ny"], dst.np_dtype, plic=case["plic"], eps=case["eps"], dx=src.get_param("dx"), dy=src.get_param("dy"),
                                 istep=case["istep"])
        kept = state_bytes(src)
        for again in ("", " again"):
            summ = dst.regrid_from(src, plic=case["plic"], eps=case["eps"])
            held_to_regrid(dst, want, summ, wsum, finite, ctx + again)
            assert dst.istep == src.istep == case["istep"], ctx + again
        assert state_bytes(src) == kept, ctx + ": src changed"
        if c is not None:
            vf.census_d(c, case, fs, vf.consts_of(src))
        if vf.round_trip_d(case):            # u, v, F back on src's grid, on every cell and face set_BC does not overwrite
            back = vf.make(api, gs)
            extra.append(back)
            back.regrid_from(dst, plic=False, eps=case["eps"])
            nx, ny = gs["nx"], gs["ny"]
            for n, (i0, j0) in (("F", (1, 1)), ("u", (2, 1)), ("v", (1, 2))):
                got, w = back.get(n)[i0:nx + 1, j0:ny + 1], fs[n][i0:nx + 1, j0:ny + 1]
                assert got.tobytes() == w.tobytes(), "%s: %s does not return from the round trip in %d cells" % (ctx, n, int((got != w).sum()))
        if vf.steps_d(case):                 # (flow sources only: module docstring of tests/_verb_fuzz.py)
            twin = vf.make(api, gd)
            extra.append(twin)
            for n in STATE:
                twin.set(n, want[n])
            twin.set_BC()
            twin.istep = case["istep"]
            dst.step(vf.steps_d(case)); twin.step(vf.steps_d(case))
            assert state_bytes(dst) == state_bytes(twin), ctx + ": two steps behind vof_regrid against a twin fed by vof_set_field"
        refusal_d(api, case, src, dst, ctx)
    finally:
        for h in [src, dst] + extra:
            h.close()


RUN = {"A": run_a, "B": run_b, "C": run_c, "D": run_d}


def run_case(api, leg, seed, c=None):
    """None, or what diverged."""
    case = vf.DRAW[leg](seed)
    t0 = time.time()
    try:
        RUN[leg](api, case, c)
    except (AssertionError, VofError, IndexError, ValueError, KeyError, TypeError, OverflowError) as err:
        return "%s\n    -> %s: %s" % (vf.describe(case), type(err).__name__, str(err)[:3000])
    finally:
        TIMES[leg].append(time.time() - t0)
    return None


def run_slice(api, leg, k):
    bad = [why for why in (run_case(api, leg, seed) for seed in vf.slice_seeds(leg, k)) if why]
    n = len(vf.slice_seeds(leg, k))
    print("leg %s test %d: %d cases, %.2f s a case (%s)" % (leg, k, n, sum(TIMES[leg][-n:]) / n, " ".join("%.2f" % t for t in TIMES[leg][-n:])))
    assert not bad, "%d of %d cases diverge:\n%s" % (len(bad), n, "\n".join(bad))


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(vf.TESTS["A"]))
def test_read_only_verbs_equal_their_restatements(hip_api, k):
    run_slice(hip_api, "A", k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(vf.TESTS["B"]))
def test_call_sequences_on_one_handle_equal_the_twin_and_the_restatements(hip_api, k):
    run_slice(hip_api, "B", k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(vf.TESTS["C"]))
def test_set_scene_equals_the_restatement(hip_api, k):
    run_slice(hip_api, "C", k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(vf.TESTS["D"]))
def test_regrid_between_drawn_grids_equals_the_restatement(hip_api, k):
    run_slice(hip_api, "D", k)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["A", "B", "C", "D"], required=True)
    ap.add_argument("--seed", type=int, default=vf.SEED0 + 100000)
    ap.add_argument("--cases", type=int, default=100)
    ap.add_argument("--seconds", type=float, default=0.0, help="stop after this much wall time (0: run all cases)")
    ap.add_argument("--log", default=None)
    ap.add_argument("--lib", default=None, help="another build of the library (loaded instead of csrc/build/libvof2d_hip.so)")
    ap.add_argument("--slice", action="store_true", help="the committed slice of the leg instead of --cases cases from --seed")
    args = ap.parse_args()
    from vof2d._lib import hip_api as load
    hip = load()
    out = open(args.log, "w") if args.log else sys.stdout
    seeds = vf.slice_seeds(args.leg) if args.slice else [args.seed + n for n in range(args.cases)]
    t0, ran, why, counts = time.time(), 0, None, collections.Counter()
    import contextlib
    import io
    for seed in seeds:
        if args.seconds and time.time() - t0 > args.seconds:
            break
        with contextlib.redirect_stdout(io.StringIO()):      # (the helpers print every figure they assert)
            why = run_case(hip, args.leg, seed, counts)
        ran += 1
        if why:                             # a divergence is a finding: stop there
            print("DIVERGES " + why, file=out, flush=True)
            break
    ts = TIMES[args.leg]
    print("verb fuzz leg %s on %s: %d cases from seed %d, %s; %.0f s, %.2f s a case (max %.2f)" % (
        args.leg, hip.path, ran, seeds[0], "DIVERGED at seed %d" % seeds[ran - 1] if why else "none diverges", time.time() - t0,
        sum(ts) / max(len(ts), 1), max(ts) if ts else 0.0), file=out, flush=True)
    for name in sorted(counts):
        print("    %-55s %d" % (name, counts[name]), file=out)
    out.flush()
    sys.exit(1 if why else 0)
