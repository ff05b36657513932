"""NumPy restatement of the conjugate-gradient pressure solve (vof_solve_p_cg), for the tests.

Written from the stencil of the reference's solve_p_jacobi (2dvof.py:258-263) and the textbook method, not from
the kernels: fields are whole (nx+2, ny+2) arrays as Engine.get returns them, only the interior is touched.

    ae, aw, an, a_s = dxi2 / dyi2, or 0 at the walls;  ap = -(ae + aw + an + a_s)
    L p = ae pE + aw pW + an pN + a_s pS + ap p
    c   = sum(b) / sum(ap)                      (the constant every Jacobi sweep adds once the rest has decayed)
    solve  L p = b - c ap   by conjugate gradients on -L preconditioned with -ap, from the given p
    r = (b - c ap) - L p,  z = r / ap;   residual: max|z| ("abs") or max|z| / max(max|p|, tiny) ("rel")

Sums are taken in double whatever the field type (math.fsum for c).

Rounding allowance of the checks that compare a sweep's update, or a recomputed max|z|, with what a solve reported
(`allowance`): the stencil value divided by ap carries a few ulps of max|p|, and c depends on the summation order.
Measured as |max|z| reported by cg_solve (difference form of L, below) - max|z| recomputed by z_of (the literal form
with ap p)| at the end of a solve to 1e-8 relative (fp32: 1e-5), in units of eps * max|p|, on oracle right-hand sides:
    fp64, first solve:  48x40 ic1 0.09, 48x40 ic3 0.33, 64x64 ic1 0.09, 64x64 ic3 0.15, 256x256 ic1 0.35
    fp64, after 3 steps: 64x64 ic1 0.04 / ic2 0.92 / ic3 0.26, 96x130 ic1 0.06 / ic2 0.22 / ic3 0.18,
                         80x50 (Lx 0.1, Ly 0.13) ic3 0.47, 128x128 ic1 0.02, 256x256 ic1 0.21
    fp32 (fields float32, sums double), after 3 steps: 128x128 ic1 0.05 (0.64 at 1e-6, next to the format's floor)
The largest is 0.92; four times that, rounded up, is the 4 of `allowance`.

fp32: the restatement with float32 fields converges on the 128x128 dam-break to 1e-4, 1e-5 (290 iterations) and 1e-6
(350) relative; at 1e-6 the recomputed residual (5.8e-7) is already 15 % off the reported one (5.1e-7) -- eps is 1.2e-7
-- so the tests use 1e-5.
"""
import math

import numpy as np

TINY = 1e-300   # VOF_RESID_TINY


def coefficients(nx, ny, dxi2, dyi2, dtype=np.float64):
    """(ae, aw, an, a_s, ap) over the interior, 2dvof.py:258-262, in the field type."""
    t = np.dtype(dtype).type
    i = np.arange(1, nx + 1)[:, None] + np.zeros((1, ny), dtype=int)
    j = np.arange(1, ny + 1)[None, :] + np.zeros((nx, 1), dtype=int)
    ae = np.where(i != nx, t(dxi2), t(0.0)).astype(dtype)
    aw = np.where(i != 1, t(dxi2), t(0.0)).astype(dtype)
    an = np.where(j != ny, t(dyi2), t(0.0)).astype(dtype)
    a_s = np.where(j != 1, t(dyi2), t(0.0)).astype(dtype)
    ap = (t(-1.0) * (ae + aw + an + a_s)).astype(dtype)
    return ae, aw, an, a_s, ap


def apply_L(p, co):
    """L p over the interior, the literal form."""
    ae, aw, an, a_s, ap = co
    return ae * p[2:, 1:-1] + aw * p[:-2, 1:-1] + an * p[1:-1, 2:] + a_s * p[1:-1, :-2] + ap * p[1:-1, 1:-1]


def apply_L_diff(p, co):
    """The same operator as differences to the centre (ap = -(sum of the others)): no cancellation against ap p."""
    ae, aw, an, a_s, _ = co
    pc = p[1:-1, 1:-1]
    return ae * (p[2:, 1:-1] - pc) + aw * (p[:-2, 1:-1] - pc) + an * (p[1:-1, 2:] - pc) + a_s * (p[1:-1, :-2] - pc)


def jacobi_update(p, rhs, dxi2, dyi2):
    """One sweep of 2dvof.py:258-266: the new p (ghost cells as they were)."""
    nx, ny = p.shape[0] - 2, p.shape[1] - 2
    ae, aw, an, a_s, ap = coefficients(nx, ny, dxi2, dyi2, p.dtype)
    out = p.copy()
    out[1:-1, 1:-1] = (rhs[1:-1, 1:-1] - ae * p[2:, 1:-1] - aw * p[:-2, 1:-1] - an * p[1:-1, 2:] - a_s * p[1:-1, :-2]) / ap
    return out


def drift_of(rhs, co):
    """c = sum(b) / sum(ap), both sums exact in double."""
    return math.fsum(rhs[1:-1, 1:-1].astype(np.float64).ravel()) / math.fsum(co[4].astype(np.float64).ravel())


def z_of(p, rhs, dxi2, dyi2):
    """(max|z|, max|p|, c) recomputed with the literal form of L, in the field type."""
    nx, ny = p.shape[0] - 2, p.shape[1] - 2
    co = coefficients(nx, ny, dxi2, dyi2, p.dtype)
    c = drift_of(rhs, co)
    z = ((rhs[1:-1, 1:-1] - p.dtype.type(c) * co[4]) - apply_L(p, co)) / co[4]
    return float(np.abs(z).max()), float(np.abs(p[1:-1, 1:-1]).max()), c


def residual_value(maxz, maxp, criterion):
    if not maxz < math.inf:
        return math.inf
    return maxz if criterion == "abs" else maxz / max(maxp, TINY)


def allowance(p):
    """Rounding allowance (module docstring) for quantities of the size of an update of p."""
    return 4.0 * float(np.finfo(p.dtype).eps) * float(np.abs(p[1:-1, 1:-1]).max())


def sweep_change(p_new, p_old):
    """(max - min, mean) of what a sweep changed over the interior."""
    d = p_new[1:-1, 1:-1].astype(np.float64) - p_old[1:-1, 1:-1].astype(np.float64)
    return float(d.max() - d.min()), float(d.mean())


def cg_solve(p0, rhs, dxi2, dyi2, tol, max_iters, check_every=10, criterion="abs"):
    """(p, iterations, residual, c).  Same driver as the library's: the residual is recomputed from p at the start and
    after every check_every iterations (the direction is kept), and that recomputed value decides."""
    dt = p0.dtype
    nx, ny = p0.shape[0] - 2, p0.shape[1] - 2
    co = coefficients(nx, ny, dxi2, dyi2, dt)
    ap = co[4]
    c = drift_of(rhs, co)
    f = (rhs[1:-1, 1:-1] - dt.type(c) * ap).astype(dt)
    p = p0.copy()
    s = np.zeros_like(p)

    def dot(a, b):
        return float(np.sum(a.astype(np.float64) * b.astype(np.float64)))

    def true_residual():
        r = (f - apply_L_diff(p, co)).astype(dt)
        z = (r / ap).astype(dt)
        return r, z, residual_value(float(np.abs(z).max()), float(np.abs(p[1:-1, 1:-1]).max()), criterion)

    r, z, res = true_residual()
    rz, rz_old, done = dot(r, z), 0.0, 0
    while res > tol and res < math.inf and done < max_iters:
        stop = False
        for _ in range(min(check_every, max_iters - done)):
            beta = rz / rz_old if rz_old != 0.0 else 0.0
            s[1:-1, 1:-1] = (z + dt.type(beta) * s[1:-1, 1:-1]).astype(dt)
            q = apply_L_diff(s, co).astype(dt)
            sq = dot(s[1:-1, 1:-1], q)
            if sq == 0.0 or not math.isfinite(sq) or not math.isfinite(rz):
                stop = True
                break
            alpha = dt.type(rz / sq)
            p[1:-1, 1:-1] = (p[1:-1, 1:-1] + alpha * s[1:-1, 1:-1]).astype(dt)
            r = (r - alpha * q).astype(dt)
            z = (r / ap).astype(dt)
            rz_old, rz = rz, dot(r, z)
        done += min(check_every, max_iters - done)
        r, z, res = true_residual()
        rz = dot(r, z)
        if stop:
            break
    return p, done, res, c
