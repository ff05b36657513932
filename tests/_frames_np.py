"""vof_frame restated in NumPy from the text of include/vof2d.h: the cell expressions, the column-then-row sums, the division, the
range, the index, the contour, the NaN rule and the orientation -- every operation in the stated order, each rounded on its
own (NumPy float64 arithmetic is IEEE, one rounding per operation).  The fields are the dense (nx+2, ny+2) arrays
vof_get_field returns, ghost cells included.

The judge of the restatement itself is tests/test_frames.py (an independent reshape-mean, hand-built cases)."""
import numpy as np

F, U, V, SPEED, P, VORT, DYE = range(7)
CONTOUR, SYMMETRIC = 1, 2
LUT_ROWS, LUT_CONTOUR, LUT_NAN = 258, 256, 257
SUM_N = 8


def default_lut():
    t = np.empty((LUT_ROWS, 3), dtype=np.uint8)
    t[:256] = np.arange(256, dtype=np.uint8)[:, None]
    t[LUT_CONTOUR], t[LUT_NAN] = (0, 0, 0), (255, 0, 255)
    return t


def shape(nx, ny, bx, by):
    return -(-nx // bx), -(-ny // by)


def chunking(nx, ny, bx, tile=128):
    """(R, chunks, K) of k_frame_cols (frame_geom of runtime/rows.h): the cells-per-wave rule with 2 and 32 gives a length, K =
    max(1, length // bx) whole pixel rows make a chunk of R = K bx rows.  No result depends on it: a pixel row lies in one chunk."""
    ntj = -(-ny // tile)
    bx = min(bx, nx)
    R = min(max(nx * ntj // 4096, 2), 32)
    P = 1
    while P * 2 <= R:
        P *= 2
    K = max(1, P // bx)
    pw = -(-nx // bx)
    return K * bx, -(-pw // K), K


def cells(quantity, fields, hx=None, hy=None):
    """q[i,j] on the interior, an (nx, ny) float64 array.  fields: dict of dense arrays F, u, v, p and (for DYE) C; hx = 0.5 dxi,
    hy = 0.5 dyi for VORT."""
    d = {k: np.asarray(a).astype(np.float64) for k, a in fields.items()}
    nx, ny = d["F"].shape[0] - 2, d["F"].shape[1] - 2
    I, J = slice(1, nx + 1), slice(1, ny + 1)
    if quantity in (F, P, DYE):
        return d[{F: "F", P: "p", DYE: "C"}[quantity]][I, J].copy()
    u, v = d["u"], d["v"]
    with np.errstate(all="ignore"):
        # uc(i,j) for i in [1, nx], j in [0, ny+1]; vc(i,j) for i in [0, nx+1], j in [1, ny]: the interior and the neighbours VORT asks for
        uc = (u[1:nx + 1, :] + u[2:nx + 2, :]) * 0.5
        vc = (v[:, 1:ny + 1] + v[:, 2:ny + 2]) * 0.5
        if quantity == U:
            return uc[:, J].copy()
        if quantity == V:
            return vc[I, :].copy()
        if quantity == SPEED:
            a, b = uc[:, J], vc[I, :]
            return np.sqrt(a * a + b * b)
        if quantity == VORT:
            return (vc[2:nx + 2, :] - vc[0:nx, :]) * hx - (uc[:, 2:ny + 2] - uc[:, 0:ny]) * hy
    raise ValueError(quantity)


def means_of(q, bx, by):
    """The (pw, ph) means of the (nx, ny) cell values in the stated order: per column c = 0.0; c += q[i,j], i ascending over the
    pixel row; S = 0.0; S += c_j, j ascending; m = S / cnt."""
    nx, ny = q.shape
    bx, by = min(bx, nx), min(by, ny)
    pw, ph = shape(nx, ny, bx, by)
    with np.errstate(all="ignore"):
        col = np.zeros((pw, ny))
        for k in range(bx):                       # the k-th row of every pixel row, where it has one
            rows = np.arange(pw) * bx + k
            live = rows < nx
            col[live] = col[live] + q[rows[live]]
        S = np.zeros((pw, ph))
        for k in range(by):
            c = np.arange(ph) * by + k
            live = c < ny
            S[:, live] = S[:, live] + col[:, c[live]]
        ni = np.minimum((np.arange(pw) + 1) * bx, nx) - np.arange(pw) * bx
        nj = np.minimum((np.arange(ph) + 1) * by, ny) - np.arange(ph) * by
        cnt = (ni[:, None] * nj[None, :]).astype(np.float64)
        return S / cnt


def key(x):
    """The order-preserving integer key of doubles: the bits with the sign bit flipped if it is clear, all bits flipped if it is set."""
    b = np.asarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b ^ np.uint64(1 << 63))


def auto_range(m, symmetric):
    ok = ~np.isnan(m)
    if not ok.any():
        lo = hi = 0.0
    else:
        v = m[ok]
        k = key(v)
        lo, hi = float(v[np.argmin(k)]), float(v[np.argmax(k)])
    if symmetric:
        A = max(abs(lo), abs(hi))
        lo, hi = -A, A
    return lo, hi


def index(m, lo, hi):
    """idx of non-NaN means (a NaN mean's entry is not used)."""
    with np.errstate(all="ignore"):
        t = (m - np.float64(lo)) / (np.float64(hi) - np.float64(lo))
        mid = (t * 255.0 + 0.5)
        idx = np.where(np.isfinite(mid), mid, 0.0).astype(np.int64)
        idx = np.where(t >= 1.0, 255, idx)
        idx = np.where(~(t > 0.0) | (hi == lo), 0, idx)
    return idx


def contour_mask(mF):
    s = mF >= 0.5                                  # (a NaN compares false)
    c = np.zeros(mF.shape, dtype=bool)
    c[:-1, :] |= s[:-1, :] != s[1:, :]
    c[:, :-1] |= s[:, :-1] != s[:, 1:]
    return c


def frame(quantity, fields, bx, by, flags=0, lo=0.0, hi=0.0, lut=None, istep=0, hx=None, hy=None):
    """(rgb (ph, pw, 3) uint8, means (pw, ph) float64, summary (SUM_N,) float64) of vof_frame."""
    lut = default_lut() if lut is None else np.asarray(lut, dtype=np.uint8)
    m = means_of(cells(quantity, fields, hx, hy), bx, by)
    pw, ph = m.shape
    if lo == hi:
        lo, hi = auto_range(m, bool(flags & SYMMETRIC))
    idx = index(m, lo, hi)
    ncont = 0
    if flags & CONTOUR:
        mF = m if quantity == F else means_of(cells(F, fields), bx, by)
        c = contour_mask(mF) & ~np.isnan(m)
        idx = np.where(c, LUT_CONTOUR, idx)
        ncont = int(c.sum())
    nan = np.isnan(m)
    idx = np.where(nan, LUT_NAN, idx)
    rgb = np.ascontiguousarray(lut[idx].transpose(1, 0, 2)[::-1])      # image row r is pixel row ph - 1 - r, image column c is a
    summary = np.zeros(SUM_N)
    summary[:7] = (pw, ph, istep, lo, hi, int(nan.sum()), ncont)
    return rgb, m, summary
