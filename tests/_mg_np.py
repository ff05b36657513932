"""NumPy restatement of the geometric-multigrid pressure solve (vof_solve_p_mg), for the tests.

Written from the stencil of the reference's solve_p_jacobi (2dvof.py:258-263), the description of the method in
DESIGN.md 3.8 and the textbook (Trottenberg, Oosterlee, Schueller, "Multigrid", cell-centred grids), not from the
kernels.  Same equation, drift constant and residual as tests/_cg_np.py, whose pieces are imported:

    L p = b - c ap,  c = sum(b) / sum(ap);   r = (b - c ap) - L p,  z = r / ap;   residual max|z| or max|z| / max|p|

Hierarchy: level l has nx / 2^l x ny / 2^l cells and the coefficients dxi2 / 4^l, dyi2 / 4^l (the operator discretised
again on the coarser grid, same wall rule).  A level is added while both extents are even and the coarser level keeps
at least 4 cells each way.  One V(nu, nu) cycle, from the finest level down:

    nu damped Jacobi sweeps          e <- e + w ((f - L e) / ap),  w = 0.8
    restriction                      f_coarse = 0.25 ((r00 + r01) + (r10 + r11)) of r = f - L e,  e_coarse = 0
    ... the coarser levels ...
    prolongation                     e <- e + bilinear(e_coarse): 0.75 / 0.25 along j, then 0.75 / 0.25 along i (the
                                     weights 9/16, 3/16, 3/16, 1/16), the coarse value repeated beyond a wall
    nu damped Jacobi sweeps

On the finest level e is p and f is b - c ap.  On the coarsest level L e = f - c' ap (c' = sum(f) / sum(ap) of that
level; on a one-level hierarchy the c of the solve) is solved by diagonally preconditioned conjugate gradients from
e = 0 (p on a one-level hierarchy) until the recurrence's max|z| is at most 1e-2 of the starting one, at most
4 max(nx_l, ny_l) iterations.  Driver as the library's: check first, then check_every cycles between checks.

Measured with this module on ORACLE right-hand sides (tests/test_mg_solve.py prints the same figures), relative
criterion, V(2,2): levels / coarsest / cycles / worst factor per cycle after the second cycle.
Warm p = after predictor_state(..., 3); cold = p = 0 (steps 0).  Tolerance 1e-8 relative (fp32: 1e-5, tests/_cg_np.py).
    grid                        levels  coarsest  cycles warm / cold   worst factor warm / cold
    64x64 ic 1                    5      4x4          7 / 7              0.15 / 0.15
    64x64 ic 2                    5      4x4          6 / 6              0.14 / 0.16
    64x64 ic 3                    5      4x4          6 / 6              0.14 / 0.15
    96x130 ic 1                   2      48x65        8 / 8              0.23 / 0.23
    96x130 ic 2                   2      48x65        6 / 7              0.19 / 0.23
    96x130 ic 3                   2      48x65        7 / 8              0.20 / 0.24
    256x256 ic 1                  7      4x4          7 / 8              0.15 / 0.16
    256x256 ic 2                  7      4x4          6 / 7              0.17 / 0.16
    256x256 ic 3                  7      4x4          6 / 7              0.16 / 0.15
    80x50 ic 3, Lx 0.1 Ly 0.13    2      40x25       14 / 18             0.51 / 0.50   (dx != dy, ratio^2 4.3: point Jacobi smooths
                                                                                       the short direction badly; the worst grid)
    128x128 ic 1 fp32             6      4x4          3 / 4              0.14 / 0.14
    200x200 ic 1                  4      25x25        7 / 7              0.15 / 0.15
    48x80 ic 2 (ratio^2 2.8)      4      6x10        10 / 10             0.36 / 0.36
    96x96 ic 1 (knob tests)       5      6x6          7                  0.15          nu 1 / 3: 11 / 5 cycles; depth 1 / 2: 3 / 6
    48x80 ic 2 (knob tests)                                                            nu 1 / 3: 18 / 7 cycles; depth 1 / 2: 3 / 9
    128x96 ic 3                   5      8x6          8                  0.25
    1024^2, 2048^2, 4096^2 ic 1, cold   9 / 10 / 11 levels, 4x4:  8 / 8 / 8 cycles, worst factor 0.16 each (4096^2: 48 s on the CPU)
No grid needs more than 20 cycles, so none leaves the tests' list; the cap there is 40.
Distance between two solves of one problem to 1e-8 and to 1e-10 (max over the interior, means removed; max|p| 556 ... 939):
    64x64 ic 1 7.2e-5, 96x130 ic 2 2.3e-5, 256x256 ic 1 5.0e-4, 80x50 ic 3 2.2e-5
"""
import math

import numpy as np

import _cg_np as cg

OMEGA = 0.8
COARSE_REDUCTION = 1e-2


def hierarchy(nx, ny, max_levels=-1):
    """[(nx_l, ny_l)] from the finest level down."""
    levels = [(nx, ny)]
    while max_levels < 0 or len(levels) < max_levels:
        a, b = levels[-1]
        if a % 2 or b % 2 or a // 2 < 4 or b // 2 < 4:
            break
        levels.append((a // 2, b // 2))
    return levels


def coarse_cap(nx, ny):
    return 4 * max(nx, ny)


def smooth(e, f, co, nu):
    t = e.dtype.type
    ap = co[4]
    for _ in range(nu):
        e[1:-1, 1:-1] = (e[1:-1, 1:-1] + t(OMEGA) * ((f - cg.apply_L_diff(e, co)) / ap)).astype(e.dtype)


def restrict(e, f, co):
    r = (f - cg.apply_L_diff(e, co)).astype(e.dtype)
    return (e.dtype.type(0.25) * ((r[0::2, 0::2] + r[0::2, 1::2]) + (r[1::2, 0::2] + r[1::2, 1::2]))).astype(e.dtype)


def prolong_add(e, ec):
    """e += bilinear(ec) over the interior."""
    t = e.dtype.type
    E = np.pad(ec[1:-1, 1:-1], 1, mode="edge")
    lo = t(0.75) * E[:, 1:-1] + t(0.25) * E[:, :-2]       # fine column 2 jc - 1
    hi = t(0.75) * E[:, 1:-1] + t(0.25) * E[:, 2:]        # fine column 2 jc
    X = np.empty((E.shape[0], 2 * (E.shape[1] - 2)), dtype=e.dtype)
    X[:, 0::2], X[:, 1::2] = lo, hi
    add = np.empty((2 * (E.shape[0] - 2), X.shape[1]), dtype=e.dtype)
    add[0::2] = t(0.75) * X[1:-1] + t(0.25) * X[:-2]      # fine row 2 ic - 1
    add[1::2] = t(0.75) * X[1:-1] + t(0.25) * X[2:]       # fine row 2 ic
    e[1:-1, 1:-1] = (e[1:-1, 1:-1] + add).astype(e.dtype)


def coarse_solve(e, f, co, c, cap):
    """CG on L e = f - c ap from the given e, to COARSE_REDUCTION of the starting max|z| (the recurrence's); returns
    the iterations done."""
    dt = e.dtype
    ap = co[4]
    fc = (f - dt.type(c) * ap).astype(dt)
    s = np.zeros_like(e)

    def dot(a, b):
        return float(np.sum(a.astype(np.float64) * b.astype(np.float64)))

    r = (fc - cg.apply_L_diff(e, co)).astype(dt)
    z = (r / ap).astype(dt)
    z0 = float(np.abs(z).max())
    rz, rz_old, it = dot(r, z), 0.0, 0
    if not z0 > 0.0:
        return 0
    while it < cap:
        beta = rz / rz_old if rz_old != 0.0 else 0.0
        s[1:-1, 1:-1] = (z + dt.type(beta) * s[1:-1, 1:-1]).astype(dt)
        q = cg.apply_L_diff(s, co).astype(dt)
        sq = dot(s[1:-1, 1:-1], q)
        if sq == 0.0 or not math.isfinite(sq) or not math.isfinite(rz):
            break
        alpha = dt.type(rz / sq)
        if alpha == 0.0:
            break
        e[1:-1, 1:-1] = (e[1:-1, 1:-1] + alpha * s[1:-1, 1:-1]).astype(dt)
        r = (r - alpha * q).astype(dt)
        z = (r / ap).astype(dt)
        rz_old, rz = rz, dot(r, z)
        it += 1
        if float(np.abs(z).max()) <= COARSE_REDUCTION * z0:
            break
    return it


class Hierarchy:
    def __init__(self, nx, ny, dxi2, dyi2, dtype, max_levels=-1):
        self.sizes = hierarchy(nx, ny, max_levels)
        self.co = [cg.coefficients(a, b, dxi2 / 4.0 ** l, dyi2 / 4.0 ** l, dtype) for l, (a, b) in enumerate(self.sizes)]
        self.e = [None] + [np.zeros((a + 2, b + 2), dtype=dtype) for (a, b) in self.sizes[1:]]
        self.f = [None] * len(self.sizes)
        self.coarse_iters = 0

    def vcycle(self, p, f0, c, nu):
        last = len(self.sizes) - 1
        self.e[0], self.f[0] = p, f0
        for l in range(last):
            smooth(self.e[l], self.f[l], self.co[l], nu)
            self.f[l + 1] = restrict(self.e[l], self.f[l], self.co[l])
            self.e[l + 1][1:-1, 1:-1] = 0
        if last == 0:       # a one-level hierarchy: the coarsest-level solver alone, on the equation itself
            self.coarse_iters = coarse_solve(p, self.b0, self.co[0], c, coarse_cap(*self.sizes[0]))
        else:
            cc = cg.drift_of(np.pad(self.f[last], 1), self.co[last])
            self.coarse_iters = coarse_solve(self.e[last], self.f[last], self.co[last], cc, coarse_cap(*self.sizes[last]))
        for l in range(last - 1, -1, -1):
            prolong_add(self.e[l], self.e[l + 1])
            smooth(self.e[l], self.f[l], self.co[l], nu)


def mg_solve(p0, rhs, dxi2, dyi2, tol, max_cycles, check_every=1, criterion="abs", nu=2, max_levels=-1, history=None):
    """(p, cycles, residual, c).  `history`, a list, receives the residual of every check."""
    dt = p0.dtype
    nx, ny = p0.shape[0] - 2, p0.shape[1] - 2
    H = Hierarchy(nx, ny, dxi2, dyi2, dt, max_levels)
    co = H.co[0]
    ap = co[4]
    c = cg.drift_of(rhs, co)
    H.b0 = rhs[1:-1, 1:-1]
    f0 = (rhs[1:-1, 1:-1] - dt.type(c) * ap).astype(dt)
    p = p0.copy()

    def check():
        z = ((f0 - cg.apply_L_diff(p, co)) / ap).astype(dt)
        res = cg.residual_value(float(np.abs(z).max()) if np.isfinite(z).all() else math.inf,
                                float(np.abs(p[1:-1, 1:-1]).max()), criterion)
        if history is not None:
            history.append(res)
        return res

    res, done = check(), 0
    while res > tol and res < math.inf and done < max_cycles:
        n = min(check_every, max_cycles - done)
        for _ in range(n):
            H.vcycle(p, f0, c, nu)
        done += n
        res = check()
    return p, done, res, c


def worst_factor(history):
    """Largest ratio of consecutive residuals after the second cycle (checks every cycle)."""
    r = [b / a for a, b in zip(history[2:-1], history[3:]) if a > 0.0]
    return max(r) if r else float("nan")
