"""Restatement of the tracer verbs (vof_tracers_advance, vof_tracers_get) for the tests, term for term in the expression
order stated in the comment block of include/vof2d.h (and repeated at the head of csrc/kernels/tracers.h).  Written from
that comment, not from the kernel.

Scalar Python doubles throughout: IEEE binary64, every product and sum rounded on its own (Python has no fused
multiply-add in these expressions), so on the parity build (-ffp-contract=off) the device's values are these bits.  The
fields are whatever vof_get_field returns, (nx + 2, ny + 2) arrays of either dtype, converted to double first.
"""
import math

import numpy as np

N, SUM_N = 8, 8                      # VOF_TRACER_N, VOF_TRACER_SUM_N
X, Y, U, V, F = range(5)
COUNT, LOST, IN_LIQUID, ISTEP, TIME = range(5)
OFFSETS = {"u": (0.0, 0.5), "v": (0.5, 0.0), "F": (0.5, 0.5)}
NAN = float("nan")


class Grid:
    """What a sample needs of the handle: nx, ny and the Python-double dxi, dyi, Lx, Ly of vof_get_param."""

    def __init__(self, nx, ny, dxi, dyi, Lx, Ly):
        self.nx, self.ny, self.dxi, self.dyi, self.Lx, self.Ly = int(nx), int(ny), float(dxi), float(dyi), float(Lx), float(Ly)

    @classmethod
    def of(cls, e):
        return cls(e.nx, e.ny, e.get_param("dxi"), e.get_param("dyi"), e.get_param("Lx"), e.get_param("Ly"))


class Field:
    """A field as doubles, with a record of the cells loaded from it (`loads`: a list of (i, j), or None)."""

    def __init__(self, which, arr, record=False):
        a = np.asarray(arr)
        self.which, self.shape = which, a.shape
        self.v = a.astype(np.float64).tolist()
        self.loads = [] if record else None

    def at(self, i, j):
        if not (0 <= i < self.shape[0] and 0 <= j < self.shape[1]):
            raise IndexError("%s[%d, %d] outside the stored %r array" % (self.which, i, j, self.shape))
        if self.loads is not None:
            self.loads.append((i, j))
        return self.v[i][j]


def cell(which, x, y, g):
    """(ib, jb, a, b) of the bilinear sample of field `which` at (x, y)."""
    ox, oy = OFFSETS[which]
    s = x * g.dxi + ox
    t = y * g.dyi + oy
    i0 = 1 if ox == 0 else 0
    j0 = 1 if oy == 0 else 0
    ib = math.floor(s) + i0
    jb = math.floor(t) + j0
    ib = i0 if ib < i0 else (g.nx if ib > g.nx else ib)      # [1, nx] for u, [0, nx] for v and F
    jb = j0 if jb < j0 else (g.ny if jb > g.ny else jb)      # [1, ny] for v, [0, ny] for u and F
    a = s - float(ib - i0)
    b = t - float(jb - j0)
    return ib, jb, a, b


def sample(f, x, y, g):
    ib, jb, a, b = cell(f.which, x, y, g)
    f00, f10, f01, f11 = f.at(ib, jb), f.at(ib + 1, jb), f.at(ib, jb + 1), f.at(ib + 1, jb + 1)
    lo = f00 + a * (f10 - f00)
    hi = f01 + a * (f11 - f01)
    return lo + b * (hi - lo)


def clamp(c, L):
    return 0.0 if c < 0 else (L if c > L else c)             # (keeps a NaN: both comparisons fail)


def advance_one(u, v, x, y, h, g, events=None):
    """One midpoint advance of one tracer by h; (nan, nan) if it is lost (or was).  `events`, a set, receives the names
    of the walls a clamp acted on: "x0", "xL", "y0", "yL"."""
    if x != x:
        return NAN, NAN
    k1u, k1v = sample(u, x, y, g), sample(v, x, y, g)
    xm = x + (0.5 * h) * k1u
    ym = y + (0.5 * h) * k1v
    if not (math.isfinite(xm) and math.isfinite(ym)):
        return NAN, NAN
    _note(events, xm, ym, g)
    xm, ym = clamp(xm, g.Lx), clamp(ym, g.Ly)
    k2u, k2v = sample(u, xm, ym, g), sample(v, xm, ym, g)
    xn = x + h * k2u
    yn = y + h * k2v
    if not (math.isfinite(xn) and math.isfinite(yn)):
        return NAN, NAN
    _note(events, xn, yn, g)
    return clamp(xn, g.Lx), clamp(yn, g.Ly)


def _note(events, x, y, g):
    if events is None:
        return
    for hit, name in ((x < 0, "x0"), (x > g.Lx, "xL"), (y < 0, "y0"), (y > g.Ly, "yL")):
        if hit:
            events.add(name)


def fields(Fa, ua, va, record=False):
    return Field("F", Fa, record), Field("u", ua, record), Field("v", va, record)


def advance(u, v, xy, h, g, events=None):
    """All tracers of the (n, 2) array xy advanced by h on the Fields u, v; a new array."""
    out = np.empty((len(xy), 2), dtype=np.float64)
    for k, (x, y) in enumerate(np.asarray(xy, dtype=np.float64).tolist()):
        out[k] = advance_one(u, v, x, y, float(h), g, events)
    return out


def rows(Ff, u, v, xy, g):
    """The (n, N) rows: X, Y and U, V, F sampled there; NaN for a lost tracer; the unused slots 0."""
    out = np.zeros((len(xy), N), dtype=np.float64)
    for k, (x, y) in enumerate(np.asarray(xy, dtype=np.float64).tolist()):
        if x != x:
            out[k, :5] = NAN
        else:
            out[k, :5] = (x, y, sample(u, x, y, g), sample(v, x, y, g), sample(Ff, x, y, g))
    return out


def summary(r, istep, time):
    """The SUM_N doubles of the summary of the rows r."""
    s = np.zeros(SUM_N, dtype=np.float64)
    s[COUNT] = len(r)
    s[LOST] = int(np.isnan(r[:, X]).sum()) if len(r) else 0
    s[IN_LIQUID] = int((r[:, F] >= 0.5).sum()) if len(r) else 0
    s[ISTEP] = istep
    s[TIME] = time
    return s


def same_bits(a, b):
    """Equal bit for bit, the sign of a zero included; a NaN equals a NaN in the same place (IEEE 754 leaves the sign and
    payload of a NaN an operation makes to the implementation: the host's and the device's differ)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and np.where(na, 0.0, a).tobytes() == np.where(nb, 0.0, b).tobytes()


def rotation_fields(nx, ny, dx, dy, w, xc, yc, dtype=np.float64):
    """(F, u, v) of the rigid rotation u = -w (y - yc), v = w (x - xc) laid on the staggered (nx + 2, ny + 2) arrays, ghost
    cells included: u[i,j] at ((i - 1) dx, (j - 0.5) dy), v[i,j] at ((i - 0.5) dx, (j - 1) dy); F = 0."""
    i = np.arange(nx + 2, dtype=np.float64)[:, None]
    j = np.arange(ny + 2, dtype=np.float64)[None, :]
    u = -w * ((j - 0.5) * dy - yc) + 0.0 * i
    v = w * ((i - 0.5) * dx - xc) + 0.0 * j
    return np.zeros((nx + 2, ny + 2), dtype=dtype), u.astype(dtype), v.astype(dtype)
