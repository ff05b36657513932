"""vof_regrid on the GPU (include/vof2d.h): F, u, v, p of dst with their ghost rings, and the summary, against tests/_regrid_np.py,
the NumPy restatement, byte for byte; what the call reads of src and leaves of dst; the refusals; the command line.

Sizes, from the geometry of the kernels (kernels/regrid.h: a wave owns 128 columns of dst and marches along i; a lane's source
column is (j - 1) / ry + 1): 33 x 17 -> 66 x 34 odd extents, -> 66 x 51 unequal factors, -> 132 x 136 a second, ragged column
tile; 128^2 -> 256^2 a tile edge on a parent boundary, -> 384 x 128 refinement along i only; 128^2 -> 64^2 and 32 x 16, 33 x 17 ->
11 x 17 the coarsening sums of 4, 32 and 3 terms; 33 x 17 onto itself the copy.  Every case runs the four dtype pairs, with and
without PLIC; the restatement of a case is computed once per (source dtype, PLIC) and rounded to either destination dtype.
"""
import ctypes as C

import numpy as np
import pytest

import _regrid_np as rnp
from test_regrid import state
from test_step_mg_gpu import FIELDS, assert_same_state
from util import STATE, assert_fields_same, engine
from vof2d import _abi, cli
from vof2d.solver import VOF2D

pytestmark = pytest.mark.gpu

BUBBLE, DAM = ("bubble33x17_f64", 100), ("dam128_f64", 100)
#        source  dst nx, ny
CASES = [(BUBBLE, 66, 34), (BUBBLE, 66, 51), (BUBBLE, 132, 136), (DAM, 256, 256), (DAM, 384, 128), (DAM, 64, 64), (DAM, 32, 16),
         (BUBBLE, 11, 17), (BUBBLE, 33, 17)]
NP = {"f64": np.float64, "f32": np.float32}
EPS = 1e-6


def source(api, case, dtype, **kw):
    """A handle that holds the golden state, converted to its dtype, at the state's step."""
    s = state(*case)
    e = engine(api, s["F"].shape[0] - 2, s["F"].shape[1] - 2, dtype, **kw)
    for n in STATE:
        e.set(n, s[n].astype(NP[dtype]))
    e.istep = case[1]
    return e


def dense(e):
    return {n: e.get(n) for n in STATE}


def restated(src_fields, src, dst, plic, istep=None):
    return rnp.restate(src_fields, dst.nx, dst.ny, dst.np_dtype, plic=plic, eps=EPS, dx=src.get_param("dx"), dy=src.get_param("dy"),
                       istep=src.istep if istep is None else istep)


def assert_bits(dst, want, summ, want_summ, ctx):
    for n in STATE:
        got = dst.get(n)
        assert got.dtype == want[n].dtype and got.tobytes() == want[n].tobytes(), "%s: %s differs in %d cells" % (ctx, n, int((got != want[n]).sum()))
    assert summ == want_summ, "%s: %r != %r" % (ctx, summ, want_summ)


@pytest.mark.parametrize("case,nx,ny", CASES, ids=["%s-to-%dx%d" % (c[0].split("_")[0], nx, ny) for c, nx, ny in CASES])
def test_bits_of_every_dtype_pair_with_and_without_plic(hip_api, case, nx, ny):
    for sdt in ("f64", "f32"):
        src = source(hip_api, case, sdt)
        fields = dense(src)
        for ddt in ("f64", "f32"):
            dst = engine(hip_api, nx, ny, ddt)
            for plic in (True, False):
                summ = dst.regrid_from(src, plic=plic, eps=EPS)
                want, want_summ = restated(fields, src, dst, plic)
                assert_bits(dst, want, summ, want_summ, "%s -> %s plic=%s" % (sdt, ddt, plic))
                assert dst.istep == case[1]
                if plic and nx > src.nx:
                    assert summ["PLIC_CELLS"] > 0
            dst.close()
        assert_fields_same(src, source(hip_api, case, sdt), ctx="src after the calls")
        src.close()


@pytest.mark.parametrize("knobs", [(), (("fuse_tm", 1), ("tm_rows", 8))], ids=["default-form", "k_tm-form"])
def test_the_source_is_read_as_get_field_sees_it_and_left_as_it_was(hip_api, knobs):
    """src has just run a batched vof_step(40): its ghost cells are virtual (and, in the k_tm form, its predictor ahead).  The bits are
    those of the restatement on what a twin of src returns; src stepped on equals a control nobody ever read."""
    def make():
        e = engine(hip_api, 128, 128, "f64", ic=1)
        for k, v in knobs:
            e.set_param(k, v)
        e.step(40)
        return e
    src, read, control = make(), make(), make()
    if knobs:
        assert src.get_counter("tm_steps") > 0
    dst = engine(hip_api, 256, 256, "f64")
    summ = dst.regrid_from(src, plic=True, eps=EPS)
    want, want_summ = restated(dense(read), read, dst, True, istep=40)
    assert_bits(dst, want, summ, want_summ, "after step(40)")
    src.step(9); control.step(9)
    assert_same_state(src, control, "src stepped on")
    # ... and without a summary the call does not wait: the same bits all the same
    dst2 = engine(hip_api, 256, 256, "f64")
    dst2.regrid_from(control, plic=True, eps=EPS, summary=False)
    control.step(3)                                      # (enqueued at once: it follows the kernels that read control)
    want2, _ = restated(dense(src), src, dst2, True)     # (src is where control was when it was read)
    for n in STATE:
        assert dst2.get(n).tobytes() == want2[n].tobytes(), n
    src.step(3)
    assert_same_state(src, control, "the control read by vof_regrid, stepped on at once")


@pytest.mark.parametrize("flags,pre,knobs", [(0, 0, ()), (_abi.VOF_FLAG_NO_GRAPH, 6, ()), (0, 6, ()), (0, 40, (("fuse_tm", 1), ("tm_rows", 8), ("f_zero_map", 1)))],
                         ids=["fresh", "eager-stepped", "graphs-stepped", "k_tm-stepped"])
def test_the_destination_goes_on_like_a_twin_fed_by_set_field(hip_api, flags, pre, knobs):
    src = source(hip_api, DAM, "f64")

    def make():
        e = engine(hip_api, 256, 256, "f64", flags=flags, ic=2 if pre else None)
        for k, v in knobs:
            e.set_param(k, v)
        if pre:
            e.step(pre)          # (graphs captured and cached, ghost cells virtual; the k_tm form: the predictor ahead, zero maps kept)
        return e
    dst, twin = make(), make()
    dst.regrid_from(src, plic=True, eps=EPS, summary=False)
    want, _ = restated(dense(src), src, dst, True)
    for n in STATE:
        twin.set(n, want[n])
    twin.set_BC()
    twin.istep = src.istep
    assert_fields_same(dst, twin, STATE, ctx="after the call")
    for n in (3, 24):
        dst.step(n); twin.step(n)
        assert_same_state(dst, twin, "step(%d)" % n)
    dst.step_mg(2, 2); twin.step_mg(2, 2)
    assert_same_state(dst, twin, "step_mg(2, 2)")
    if knobs:
        assert dst.get_counter("tm_steps") == twin.get_counter("tm_steps") > 0 and dst.get_counter("fzmap_wrong") == 0


def test_refusals_leave_both_handles_as_they_were(hip_api):
    def call(dst, src, flags=_abi.VOF_REGRID_PLIC, eps=EPS):
        return hip_api.regrid(dst.handle, src.handle, flags, eps, (C.c_double * _abi.VOF_REGRID_SUM_N)())

    def snapshot(e):
        return [e.get(n).tobytes() for n in FIELDS] + [e.istep]

    src = engine(hip_api, 64, 64, "f64", ic=1)
    src.step(3)
    dst = engine(hip_api, 128, 128, "f32", ic=2)
    dst.step(2)
    strip = engine(hip_api, 64, 64, "f64", ic=1, rows=(0, 40), own=(1, 22))
    strip_fine = engine(hip_api, 128, 128, "f64", ic=1, rows=(60, 129), own=(78, 128))
    others = {"mixed directions": engine(hip_api, 128, 32, "f64", ic=2), "no integer ratio": engine(hip_api, 96, 64, "f64", ic=2),
              "a factor of 17": engine(hip_api, 1088, 64, "f64", ic=2), "another Lx": engine(hip_api, 128, 128, "f64", ic=2, Lx=0.2)}
    everyone = [src, dst, strip, strip_fine] + list(others.values())
    before = [snapshot(e) for e in everyone]
    assert call(dst, strip) == _abi.VOF_ESTATE and call(strip_fine, src) == _abi.VOF_ESTATE and b"strip" in hip_api.last_error(strip_fine.handle)
    assert call(src, src) == _abi.VOF_EINVAL
    for why, other in others.items():
        assert call(other, src) == _abi.VOF_EINVAL, why
        assert call(src, other) == _abi.VOF_EINVAL, why
    for eps in (0.5, -1e-9, float("nan")):
        assert call(dst, src, eps=eps) == _abi.VOF_EINVAL
    for flags in (2, 3, -1):
        assert call(dst, src, flags=flags) == _abi.VOF_EINVAL
    assert hip_api.regrid(None, src.handle, 0, 0.0, None) == _abi.VOF_EINVAL and hip_api.regrid(dst.handle, None, 0, 0.0, None) == _abi.VOF_EINVAL
    assert [snapshot(e) for e in everyone] == before
    # a phased step in progress, on either side: refused; the step ends as that of a control
    for who in ("src", "dst"):
        a, b = engine(hip_api, 64, 64, "f64", ic=1), engine(hip_api, 64, 64, "f64", ic=1)
        other = engine(hip_api, 128, 128, "f64", ic=2)
        kept = snapshot(other)
        for ph in (0, 1):
            a.step_phase(ph); b.step_phase(ph)
            assert (call(other, a) if who == "src" else call(a, other)) == _abi.VOF_ESTATE
        a.step_phase(2); b.step_phase(2)
        assert_same_state(a, b, "the phased step around the refused calls")
        assert snapshot(other) == kept
        assert call(other, a, eps=0.0) == _abi.VOF_OK        # (eps 0 is allowed; the step is over)


def test_the_python_interface_and_the_command_line_agree(hip_api, tmp_path, monkeypatch):
    """A 64^2 run saved at step 20, then --regrid-from into 128^2 up to step 25, gives the F of VOF2D.regrid and 5 steps."""
    monkeypatch.chdir(tmp_path)
    lines = []
    say = lambda *a: lines.append(" ".join(str(x) for x in a))
    assert cli.run(cli.parse_args(["--nx", "64", "--ny", "64", "--dtype", "f64", "--steps", "20", "--save-every", "20"]), api=hip_api, world=1, rank=0, out=say) == 0
    argv = ["--nx", "128", "--ny", "128", "--dtype", "f32", "--dt", "2e-6", "--steps", "25", "--save-every", "25", "--regrid-from", "data/00000020.npz"]
    assert cli.run(cli.parse_args(argv), api=hip_api, world=1, rank=0, out=say) == 0
    said = [l for l in lines if "Regridded from" in l]
    assert len(said) == 1 and "(64 x 64 f64) at step 20: refined by (2, 2)" in said[0] and "volume" in said[0]
    assert any("differ" in l and "dt 4e-06 -> 2e-06" in l for l in lines)
    coarse = VOF2D(64, 64, dtype="f64", api=hip_api)
    coarse.set_init_F(1)
    coarse.step(20)
    fine = coarse.regrid(128, 128, dtype="f32", dt=2e-6)
    assert (fine.nx, fine.ny, fine.istep, fine.dt) == (128, 128, 20, 2e-6) and fine.regrid_summary["DIR"] == 1.0 and fine.regrid_summary["PLIC_CELLS"] > 0
    fine.step(5)
    z = np.load("data/00000025.npz")
    assert int(z["istep"]) == 25 and (int(z["nx"]), int(z["ny"]), str(z["dtype"])) == (128, 128, "f32")
    for n in STATE:
        assert z[n].tobytes() == getattr(fine, n).to_numpy().tobytes(), n
    with pytest.raises(ValueError):
        coarse.regrid(96, 64)
    with pytest.raises(SystemExit) as e:
        cli.run(cli.parse_args(["--nx", "96", "--ny", "64", "--dtype", "f64", "--steps", "21", "--regrid-from", "data/00000020.npz"]), api=hip_api, world=1, rank=0, out=say)
    assert "holds a 64x64 run, this one is 96x64" in str(e.value.code)
