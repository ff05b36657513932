"""NumPy restatement of vof_diagnostics for the tests, term for term in the expression order stated at the head of
taichi-2d-vof_amd/csrc/kernels/diag.h.

From the arrays F, u, v (rows indexed [i - row0], ghost columns included: ny + 2 columns) and the constants it returns the
per-cell terms of every sum as float64 arrays, and the extrema.  Sums are judged against math.fsum of those terms, and --
where the caller names the chunk length R of the launch -- held bit for bit to the order of tests/_reduce_np.py.

The tolerance is derived, not measured: summing n doubles in any order errs by at most (n - 1) 2^-53 sum|t_i| to first
order; the tests allow n 2^-52 fsum(|t|), a factor of two for the higher-order terms (and the rounding of fsum's own
result).  On the parity build (-ffp-contract=off) the terms themselves are the restatement's bits.  Extrema, CELLS and
ISTEP are compared with ==.
"""
import math

import numpy as np

from _reduce_np import fixed_order

SUMS = ("SUM_F", "SUM_FI", "SUM_FJ", "SUM_KE", "SUM_DIV2")
EXTREMA = ("MAX_DIV", "MAX_U", "MAX_V", "MIN_F", "MAX_F")


def _max_nan_inf(a):
    """max in which a NaN counts as +inf; -inf over nothing."""
    a = np.asarray(a, dtype=np.float64).ravel()
    if a.size == 0:
        return -math.inf
    return math.inf if np.isnan(a).any() else float(a.max())


def restate(F, u, v, dxi, dyi, rho_g, rho_l, lo=1, hi=None, row0=0):
    """(terms, extrema, cells) over the cells i in [lo, hi], j in [1, ny].  Row hi + 1 of u must be stored."""
    ny = F.shape[1] - 2
    if hi is None:
        hi = F.shape[0] - 2 + row0
    F, u, v = (np.asarray(a).astype(np.float64) for a in (F, u, v))
    I = slice(lo - row0, hi + 1 - row0)
    J = slice(1, ny + 1)
    f = F[I, J]
    uw, ue = u[I, J], u[lo - row0 + 1: hi + 2 - row0, J]
    vs, vn = v[I, J], v[I, 2: ny + 2]
    i = np.arange(lo, hi + 1, dtype=np.float64)[:, None]
    j = np.arange(1, ny + 1, dtype=np.float64)[None, :]
    uc = (uw + ue) * 0.5
    vc = (vs + vn) * 0.5
    Fc = np.fmin(np.fmax(f, 0.0), 1.0)
    rho = rho_g * (1.0 - Fc) + rho_l * Fc
    div = (ue - uw) * dxi + (vn - vs) * dyi
    terms = {
        "SUM_F": f.copy(),
        "SUM_FI": f * i,
        "SUM_FJ": f * j,
        "SUM_KE": (rho * 0.5) * (uc * uc + vc * vc),
        "SUM_DIV2": div * div,
    }
    extrema = {
        "MAX_DIV": max(0.0, _max_nan_inf(np.abs(div))),
        "MAX_U": max(0.0, _max_nan_inf(np.abs(uw)), _max_nan_inf(np.abs(ue))),
        "MAX_V": max(0.0, _max_nan_inf(np.abs(vs)), _max_nan_inf(np.abs(vn))),
        "MIN_F": -_max_nan_inf(-f),
        "MAX_F": _max_nan_inf(f),
    }
    return terms, extrema, float(f.size)


def bound_of(t):
    """n 2^-52 fsum(|t|): what any order of summing the n terms t may differ from their exact sum by."""
    t = np.asarray(t, dtype=np.float64).ravel()
    return t.size * 2.0 ** -52 * math.fsum(np.abs(t))


def check(raw, terms, extrema, cells, istep=None, ctx="", say=None, R=None):
    """Hold a raw row (dict keyed by vof2d.diag.NAMES) to the restatement; every figure goes through `say` first.
    R: the rows per wave chunk of the k_diag launch (diag_chunk_rows of tests/_interface_np.py); with it every sum must also
    equal the fixed-order sum of its terms (k_row_finish folds with 256 threads)."""
    msgs = []
    for k in SUMS:
        t = terms[k].ravel()
        if np.isnan(t).any():
            ok = raw[k] != raw[k]
            line = "%s %s: %r, the terms hold a NaN" % (ctx, k, raw[k])
        else:
            exact, bound = math.fsum(t), bound_of(t)
            ok = abs(raw[k] - exact) <= bound
            line = "%s %s: %r, fsum %r, |d| %.3e, bound %.3e" % (ctx, k, raw[k], exact, abs(raw[k] - exact), bound)
            if R is not None:
                fixed = fixed_order(terms[k], R, 256, "add")
                ok = ok and raw[k] == fixed
                line += ", in the kernels' order %r" % fixed
        if say:
            say(line)
        if not ok:
            msgs.append(line)
    for k in EXTREMA:
        line = "%s %s: %r, restated %r" % (ctx, k, raw[k], extrema[k])
        if say:
            say(line)
        if not raw[k] == extrema[k]:
            msgs.append(line)
    if not raw["CELLS"] == cells:
        msgs.append("%s CELLS: %r, restated %r" % (ctx, raw["CELLS"], cells))
    if istep is not None and not raw["ISTEP"] == istep:
        msgs.append("%s ISTEP: %r, expected %r" % (ctx, raw["ISTEP"], istep))
    assert not msgs, " ; ".join(msgs)


def raw_from(terms, extrema, cells, istep=0):
    """A row as the device would report it, with the sums formed by np.sum (pairwise: one more order of summing)."""
    raw = {"ISTEP": float(istep), "CELLS": float(cells)}
    raw.update({k: float(np.sum(terms[k])) for k in SUMS})
    raw.update(extrema)
    return raw


def div_max_table(n, nsteps=50, ic=1, ks=(1, 2, 3)):
    """max |div u| (and its rms) after nsteps steps of the NumPy restatements of tests/_step_mg_np.py: the reference's ten
    sweeps and K V-cycles per step -- the physical column beside the residuals of that module's table."""
    import _step_mg_np as smg
    import vof_oracle_np as onp
    out = {}
    for key in ("ten",) + tuple(ks):
        s = onp.new_state(n, n, ic, np.float64, "f32")
        res = smg.step_ten(s, nsteps) if key == "ten" else smg.step_mg(s, nsteps, key)
        prm = s.prm
        terms, ext, cells = restate(s.F, s.u, s.v, prm.dxi, prm.dyi, prm.rho_g, prm.rho_l)
        out[key] = (ext["MAX_DIV"], math.sqrt(math.fsum(terms["SUM_DIV2"].ravel()) / cells), ext["MAX_U"], ext["MAX_V"], res[-1])
    return out


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.join(here, "..", "oracle")]
    for n in [int(a) for a in sys.argv[1:]] or [64, 128]:
        for key, (dmax, dl2, umax, vmax, res) in div_max_table(n).items():
            print("%dx%d %s: div_max %.3e div_l2 %.3e | u_max %.3e v_max %.3e | residual of step 50 %.3e" % (
                n, n, "K = %d" % key if key != "ten" else "ten sweeps", dmax, dl2, umax, vmax, res), flush=True)
