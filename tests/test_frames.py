"""The NumPy restatement of vof_frame (tests/_frames_np.py) judged on its own, and the host side of vof2d/frames.py: no GPU.

The restatement's means against an independent reshape-mean within the bound for reordering a sum; the index, contour and NaN
rules on hand-built 4 x 6 cases; the PNG writer read back; the sampled colour tables; the block rule."""
import numpy as np
import pytest

import _frames_np as fnp
from vof2d import _abi, frames


def fields(F, u=None, v=None, p=None):
    z = np.zeros_like(F)
    return {"F": F, "u": z if u is None else u, "v": z if v is None else v, "p": z if p is None else p}


def dense(inner, ghost=0.0):
    a = np.full((inner.shape[0] + 2, inner.shape[1] + 2), ghost, dtype=np.float64)
    a[1:-1, 1:-1] = inner
    return a


# ---------------------------------------------------------------------------- the means
@pytest.mark.parametrize("nx,ny,bx,by", [(12, 18, 1, 1), (12, 18, 3, 2), (12, 18, 4, 9), (12, 18, 12, 18), (64, 96, 8, 8)])
def test_means_against_a_reshape_mean(nx, ny, bx, by):
    rng = np.random.default_rng(nx * 1000 + bx)
    q = rng.standard_normal((nx, ny)) * 10.0 ** rng.integers(-3, 4, (nx, ny))
    m = fnp.means_of(q, bx, by)
    want = q.reshape(nx // bx, bx, ny // by, by).transpose(0, 2, 1, 3).reshape(nx // bx, ny // by, bx * by).mean(axis=2)
    bound = bx * by * 2.0 ** -52 * np.abs(q).max()
    print("max |d|", np.abs(m - want).max(), "bound", bound)
    assert m.shape == (nx // bx, ny // by) and np.abs(m - want).max() <= bound
    # the stated order, cell by cell, on one pixel
    a, b = m.shape[0] - 1, m.shape[1] // 2
    S = 0.0
    for j in range(b * by, (b + 1) * by):
        c = 0.0
        for i in range(a * bx, (a + 1) * bx):
            c += q[i, j]
        S += c
    assert m[a, b] == S / (bx * by)


def test_partial_pixels_blocks_beyond_the_grid_and_the_cell_expressions():
    nx, ny = 7, 5
    rng = np.random.default_rng(5)
    F, u, v, p = (dense(rng.random((nx, ny)), ghost=0.25) for _ in range(4))
    u[:, :], v[:, :] = rng.standard_normal(u.shape), rng.standard_normal(v.shape)
    f = fields(F, u, v, p)
    m = fnp.means_of(fnp.cells(fnp.F, f), 3, 2)
    assert m.shape == (3, 3) and m[2, 2] == F[7, 5] and m[2, 0] == (F[7, 1] + F[7, 2]) / 2.0
    assert m[0, 2] == ((F[1, 5] + F[2, 5]) + F[3, 5]) / 3.0
    for bx, by in ((nx + 5, 1), (1, ny + 5), (100, 100)):
        mm = fnp.means_of(fnp.cells(fnp.P, f), bx, by)
        assert mm.shape == fnp.shape(nx, ny, min(bx, nx), min(by, ny)) == (1 if bx > 1 else nx, 1 if by > 1 else ny)
    hx, hy = 0.5 * 70.0, 0.5 * 50.0
    i, j = 7, 1                                   # a corner: every neighbour a ghost cell or a wall face
    uc = lambda i, j: (u[i, j] + u[i + 1, j]) * 0.5
    vc = lambda i, j: (v[i, j] + v[i, j + 1]) * 0.5
    assert fnp.cells(fnp.U, f)[i - 1, j - 1] == uc(i, j) and fnp.cells(fnp.V, f)[i - 1, j - 1] == vc(i, j)
    assert fnp.cells(fnp.SPEED, f)[i - 1, j - 1] == np.sqrt(uc(i, j) * uc(i, j) + vc(i, j) * vc(i, j))
    assert fnp.cells(fnp.VORT, f, hx, hy)[i - 1, j - 1] == (vc(i + 1, j) - vc(i - 1, j)) * hx - (uc(i, j + 1) - uc(i, j - 1)) * hy
    f32 = {k: a.astype(np.float32) for k, a in f.items()}
    assert fnp.cells(fnp.U, f32).dtype == np.float64
    assert fnp.cells(fnp.U, f32)[2, 3] == (np.float64(f32["u"][3, 4]) + np.float64(f32["u"][4, 4])) * 0.5


# ---------------------------------------------------------------------------- hand-built 4 x 6 cases
def frame46(inner, **kw):
    return fnp.frame(fnp.F, fields(dense(np.asarray(inner, dtype=np.float64))), 1, 1, **kw)


def test_the_index_rule():
    q = np.zeros((4, 6))
    q[0, 0], q[1, 0], q[2, 0], q[3, 0] = 2.0, 6.0, 4.0, 1.0          # t = 0, 1, 0.5, below the range
    q[0, 1], q[1, 1], q[2, 1], q[3, 1] = 7.0, 2.0 + 4.0 / 256.0, 2.0 + 4.0 / 1024.0, 2.0 + 4.0 * 0.75   # above; t = 1/256, 1/1024, 3/4 exactly
    q[0, 2:] = 2.0
    rgb, m, s = frame46(q, lo=2.0, hi=6.0)
    assert rgb.shape == (6, 4, 3) and m.shape == (4, 6) and s.tolist() == [4, 6, 0, 2.0, 6.0, 0, 0, 0]
    grey = lambda a, b: int(rgb[6 - 1 - b, a, 0])
    assert (rgb[..., 0] == rgb[..., 1]).all() and (rgb[..., 1] == rgb[..., 2]).all()
    assert [grey(0, 0), grey(1, 0), grey(3, 0), grey(0, 1)] == [0, 255, 0, 255]
    assert grey(2, 0) == int(0.5 * 255.0 + 0.5) == 128                 # half way: 127.5 + 0.5, truncated
    assert [grey(1, 1), grey(2, 1), grey(3, 1)] == [1, 0, 191]           # 0.996 + 0.5, 0.249 + 0.5, 191.25 + 0.5, truncated
    # hi == lo: auto range of a constant picture, index 0 everywhere
    rgb, m, s = frame46(np.full((4, 6), 3.5))
    assert (rgb == 0).all() and s[3] == s[4] == 3.5
    # auto: the extrema take the ends of the table; symmetric: zero in the middle
    rgb, m, s = frame46(q)
    assert (s[3], s[4]) == (0.0, 7.0) and int(rgb[6 - 1 - 1, 0, 0]) == 255 and int(rgb[0, 3, 0]) == 0
    rgb, m, s = frame46(q - 1.0, flags=fnp.SYMMETRIC)
    assert (s[3], s[4]) == (-6.0, 6.0) and int(rgb[0, 3, 0]) == int((-1.0 + 6.0) / 12.0 * 255.0 + 0.5)
    # -0.0 lies below +0.0 under the key
    z = np.zeros((4, 6)); z[1, 1] = -0.0
    lo, hi = fnp.auto_range(z, False)
    assert np.signbit(lo) and not np.signbit(hi)


def test_the_contour_rule_on_the_last_row_and_column():
    q = np.zeros((4, 6))
    q[3, :] = 1.0                                  # liquid in the last pixel column of the array (a = 3)
    q[:, 5] = 1.0                                  # and in the last pixel row (b = 5)
    rgb, m, s = frame46(q, lo=0.0, hi=1.0, flags=fnp.CONTOUR, lut=None)
    black = lambda a, b: rgb[6 - 1 - b, a].tolist() == [0, 0, 0] and fnp.contour_mask(m)[a, b]
    # the interface is marked on the gas side of it: (2, b) sees (3, b), (a, 4) sees (a, 5); the last row and column look at no neighbour beyond
    assert all(black(2, b) for b in range(5)) and all(black(a, 4) for a in range(3))
    assert not any(fnp.contour_mask(m)[3, :]) and not any(fnp.contour_mask(m)[:, 5])
    assert s[6] == 5 + 3 - 1 and int(fnp.contour_mask(m).sum()) == 7
    assert rgb[0, 3].tolist() == [255, 255, 255] and rgb[5, 0].tolist() == [0, 0, 0]     # (a = 0, b = 0 is gas: index 0 of the grey ramp)
    # exactly 0.5 is liquid, the double below is not
    q = np.full((4, 6), 0.5); q[1, 2] = np.nextafter(0.5, 0)
    c = fnp.contour_mask(q)
    assert np.argwhere(c).tolist() == [[0, 2], [1, 1], [1, 2]]
    # for another quantity the contour is F's: p constant, F split
    F = np.zeros((4, 6)); F[2:, :] = 1.0
    rgb, m, s = fnp.frame(fnp.P, fields(dense(F), p=dense(np.full((4, 6), 2.0))), 1, 1, fnp.CONTOUR, 0.0, 4.0)
    assert s[6] == 6 and (rgb[:, 1] == 0).all() and (rgb[:, 0] == 128).all()


def test_nan_takes_precedence():
    lut = fnp.default_lut(); lut[256] = (9, 8, 7); lut[257] = (1, 2, 3)
    q = np.zeros((4, 6)); q[2:, :] = 1.0
    q[1, 3] = np.nan                               # on the contour line (a = 1 sees a = 2)
    rgb, m, s = frame46(q, flags=fnp.CONTOUR, lut=lut)
    assert rgb[6 - 1 - 3, 1].tolist() == [1, 2, 3] and s[5] == 1 and s[6] == 6 - 1       # six pixels of a = 1 see the liquid of a = 2; the NaN one of them is NaN-coloured and not counted; as a neighbour it is gas
    assert (s[3], s[4]) == (0.0, 1.0)
    assert rgb[6 - 1 - 2, 1].tolist() == [9, 8, 7]
    # a NaN in F under another quantity: no NaN pixel, the contour takes NaN as gas
    rgb, m, s = fnp.frame(fnp.P, fields(dense(q), p=dense(np.ones((4, 6)))), 1, 1, fnp.CONTOUR, 0.0, 2.0, lut)
    assert s[5] == 0 and not np.isnan(m).any() and rgb[6 - 1 - 3, 1].tolist() == [9, 8, 7]
    # nothing but NaN
    rgb, m, s = frame46(np.full((4, 6), np.nan), lut=lut)
    assert (rgb == np.array([1, 2, 3], dtype=np.uint8)).all() and s.tolist() == [4, 6, 0, 0.0, 0.0, 24, 0, 0]
    # a NaN cell makes exactly its own pixel NaN
    big = np.zeros((8, 12)); big[5, 7] = np.nan
    assert np.argwhere(np.isnan(fnp.means_of(big, 2, 3))).tolist() == [[2, 2]]


def test_the_orientation_is_that_of_colour_image():
    q = np.zeros((4, 6)); q[0, 5] = 1.0           # i = 1 (left), j = 6 (top)
    rgb, _, _ = frame46(q, lo=0.0, hi=1.0)
    assert rgb[0, 0, 0] == 255 and rgb[..., 0].sum() == 255


# ---------------------------------------------------------------------------- vof2d/frames.py
def test_write_png_reads_back(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(1)
    for shape in ((5, 7, 3), (1, 1, 3), (64, 33, 3)):
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        path = str(tmp_path / ("f%d.png" % shape[0]))
        frames.write_png(path, a)
        with Image.open(path) as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), a)
    with pytest.raises(ValueError):
        frames.write_png(str(tmp_path / "bad.png"), np.zeros((4, 4), dtype=np.uint8))


def test_lut_samples_matplotlib_maps():
    pytest.importorskip("matplotlib")
    t = frames.lut("Blues")
    assert t.shape == (258, 3) and t.dtype == np.uint8
    assert tuple(t[0]) == (247, 251, 255) and tuple(t[255]) == (8, 48, 107) and tuple(t[256]) == (0, 0, 0) and tuple(t[257]) == (255, 0, 255)
    t = frames.lut("coolwarm", contour=(1, 2, 3), nan=(4, 5, 6))
    assert tuple(t[256]) == (1, 2, 3) and tuple(t[257]) == (4, 5, 6)
    assert np.array_equal(frames.default_lut(), fnp.default_lut())


def test_default_block_names_and_slots():
    assert [frames.default_block(*a) for a in ((200, 200), (1024, 1024), (1025, 1024), (4096, 4096), (8192, 4096), (300, 5000, 512))] == [1, 1, 2, 4, 8, 10]
    assert frames.shape(7, 5, 3, 2) == (3, 3) == fnp.shape(7, 5, 3, 2)
    assert [frames.QUANTITIES[k] for k in ("F", "U", "V", "SPEED", "P", "VORT", "DYE")] == [fnp.F, fnp.U, fnp.V, fnp.SPEED, fnp.P, fnp.VORT, fnp.DYE] == list(range(7))
    assert (_abi.VOF_FRAME_CONTOUR, _abi.VOF_FRAME_SYMMETRIC, _abi.VOF_FRAME_LUT_ROWS, _abi.VOF_FRAME_SUM_N) == (fnp.CONTOUR, fnp.SYMMETRIC, fnp.LUT_ROWS, fnp.SUM_N)
    assert frames.summary_of([4, 6, 9, -1.5, 2.5, 1, 3, 0]) == {"PW": 4, "PH": 6, "ISTEP": 9, "LO": -1.5, "HI": 2.5, "NAN_PIXELS": 1, "CONTOUR_PIXELS": 3}
    s = frames.spec("vort", 3, contour=True, symmetric=True)
    assert (s.quantity, s.bx, s.by, s.flags, s.lo, s.hi) == (5, 3, 3, 3, 0.0, 0.0)
    import ctypes
    assert ctypes.sizeof(_abi.FrameSpec) == 32
