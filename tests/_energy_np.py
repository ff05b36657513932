"""NumPy restatement of vof_energy for the tests, term for term in the expression order stated at the head of
taichi-2d-vof_amd/csrc/kernels/energy.h; the order of the sums is that of tests/_reduce_np.py.  It is the yardstick for bits.

`restate(F, u, v, p, prm)` takes the whole-domain arrays as vof_get_field returns them ((nx + 2, ny + 2), ghost cells included) and the
constants as a dict of the doubles of vof_get_param (`params_of`), and returns a namespace of
  uf, vf    the per-face pieces of the u faces (i in [2, nx], j in [1, ny]) and of the v faces (i in [1, nx], j in [2, ny]): dicts of
            VX, VY, AX, AY, SG, A, r, m as float64 arrays over exactly those faces
  terms     per sum, what every cell adds: an (nx, ny) array for the cell sums and for KE_U, KE_V, and a pair (west, south) of (nx, ny)
            arrays for the sums over both face kinds -- a face belongs to the cell it is the west or south face of, a cell without
            that face holds 0
  count     per sum, the number of its terms (cells or faces)
  amax      MAX_ACC_SIGMA
  kappa     the restated KAPPA_CSF of every interior cell
Selects are np.where on exactly the kernel's comparison, so a NaN takes the same branch.  tests/test_energy.py judges this restatement
against the reference's predictor and against closed forms.

A lane adds, per cell, the west term and then the south term of a face sum.  `fixed_order` of tests/_reduce_np.py folds ONE term per cell
(row by row, the lane's two columns in turn), so `lane_order` lays the two terms of a lane's two cells out as two rows of two columns:
row 2r holds (west, south) of the lane's first column, row 2r + 1 those of its second; with chunks of 2R such rows the fold visits west,
south, west, south of row r in the kernel's order, and the waves, blocks and folding threads are the same.
"""
import math
import types

import numpy as np

from _reduce_np import fixed_order

CELL_SUMS = ("SUM_RHO", "SUM_RHO_I", "SUM_RHO_J", "SUM_GRADF")
FACE_SUMS = ("KE_U", "KE_V", "P_VISC", "P_ADV", "P_GRAV", "P_SIGMA", "P_PRES")
SUMS = ("KE_U", "KE_V", "P_VISC", "P_ADV", "P_GRAV", "P_SIGMA", "P_PRES", "SUM_RHO", "SUM_RHO_I", "SUM_RHO_J", "SUM_GRADF")
PARAMS = ("dx", "dy", "dxi", "dyi", "dxi2", "dyi2", "rho_l", "rho_g", "nu_l", "nu_g", "sigma", "gx", "gy")


def params_of(e):
    """The constants of an engine (vof_get_param)."""
    return {k: e.get_param(k) for k in PARAMS}


def params_of_oracle(prm):
    """The constants of a state of oracle/vof_oracle_np.py, as doubles."""
    return {k: float(getattr(prm, k)) for k in PARAMS}


def kappa_csf(F, dx, dy):
    """KAPPA_CSF of kernels/curvature.h at every interior cell, and the Youngs sums (mxsum, mysum) of those cells."""
    F = np.asarray(F).astype(np.float64)
    nx, ny = F.shape[0] - 2, F.shape[1] - 2
    cx, cy, kx, ky = -1 / (2 * dx), -1 / (2 * dy), 1 / dx / 2, 1 / dy / 2

    def f(di, dj):
        return F[1 + di: 1 + di + nx, 1 + dj: 1 + dj + ny]

    with np.errstate(all="ignore"):
        mx1 = cx * (((f(1, 1) + f(1, 0)) - f(0, 1)) - f(0, 0)); my1 = cy * (((f(1, 1) - f(1, 0)) + f(0, 1)) - f(0, 0))
        mx2 = cx * (((f(1, 0) + f(1, -1)) - f(0, 0)) - f(0, -1)); my2 = cy * (((f(1, 0) - f(1, -1)) + f(0, 0)) - f(0, -1))
        mx3 = cx * (((f(0, 0) + f(0, -1)) - f(-1, 0)) - f(-1, -1)); my3 = cy * (((f(0, 0) - f(0, -1)) + f(-1, 0)) - f(-1, -1))
        mx4 = cx * (((f(0, 1) + f(0, 0)) - f(-1, 1)) - f(-1, 0)); my4 = cy * (((f(0, 1) - f(0, 0)) + f(-1, 1)) - f(-1, 0))
        mxsum = (((mx1 + mx2) + mx3) + mx4) / 4
        mysum = (((my1 + my2) + my3) + my4) / 4
        tiny = (np.abs(mxsum) < 1e-10) & (np.abs(mysum) < 1e-10)
        mag = np.sqrt(mxsum * mxsum + mysum * mysum)
        Nx = np.pad(np.where(tiny, mxsum, mxsum / mag), 1)      # N(a, b) = 0 outside [1, nx] x [1, ny]
        Ny = np.pad(np.where(tiny, mysum, mysum / mag), 1)
        kappa = -(kx * (Nx[2:, 1:-1] - Nx[:-2, 1:-1]) + ky * (Ny[1:-1, 2:] - Ny[1:-1, :-2]))
    return kappa, mxsum, mysum


def restate(F, u, v, p, prm):
    F, u, v, p = (np.asarray(a).astype(np.float64) for a in (F, u, v, p))
    nx, ny = F.shape[0] - 2, F.shape[1] - 2
    c = types.SimpleNamespace(**prm)
    with np.errstate(all="ignore"):
        # ---- the cells (all stored ones: the faces read the density of a neighbour)
        Fc = np.fmin(np.fmax(F, 0.0), 1.0)
        rho = c.rho_g * (1.0 - Fc) + c.rho_l * Fc
        nu = c.nu_l * Fc + c.nu_g * (1.0 - Fc)
        kin, mxsum, mysum = kappa_csf(F, c.dx, c.dy)
        kappa = np.zeros_like(F)
        kappa[1:-1, 1:-1] = kin
        I = np.arange(1, nx + 1, dtype=np.float64)[:, None]
        J = np.arange(1, ny + 1, dtype=np.float64)[None, :]
        C = (slice(1, nx + 1), slice(1, ny + 1))
        terms = {"SUM_RHO": rho[C].copy(), "SUM_RHO_I": rho[C] * I, "SUM_RHO_J": rho[C] * J,
                 "SUM_GRADF": np.sqrt(mxsum * mxsum + mysum * mysum)}

        def face(vel, di, dj, g, h, lo_i, lo_j):
            """The faces i in [lo_i, nx], j in [lo_j, ny] of the component `vel`; (di, dj) the step to the cell the face looks back
            to, g the gravity along the component and h the cell's length along it."""
            S = (slice(lo_i, nx + 1), slice(lo_j, ny + 1))

            def a(arr, si, sj):
                return arr[lo_i + si: nx + 1 + si, lo_j + sj: ny + 1 + sj]

            w = a(vel, 0, 0)
            if di:      # a u face: v_here = 0.25 * (((v[i-1,j] + v[i-1,j+1]) + v[i,j]) + v[i,j+1])
                here = 0.25 * (((a(v, -1, 0) + a(v, -1, 1)) + a(v, 0, 0)) + a(v, 0, 1))
                ddx = np.where(w > 0, (w - a(vel, -1, 0)) * c.dxi, (a(vel, 1, 0) - w) * c.dxi)
                ddy = np.where(here > 0, (w - a(vel, 0, -1)) * c.dyi, (a(vel, 0, 1) - w) * c.dyi)
                AX, AY = w * ddx, here * ddy
            else:       # a v face: u_here = 0.25 * (((u[i,j-1] + u[i,j]) + u[i+1,j-1]) + u[i+1,j])
                here = 0.25 * (((a(u, 0, -1) + a(u, 0, 0)) + a(u, 1, -1)) + a(u, 1, 0))
                ddx = np.where(here > 0, (w - a(vel, -1, 0)) * c.dxi, (a(vel, 1, 0) - w) * c.dxi)
                ddy = np.where(w > 0, (w - a(vel, 0, -1)) * c.dyi, (a(vel, 0, 1) - w) * c.dyi)
                AX, AY = here * ddx, w * ddy
            VX = (nu[S] * ((a(vel, -1, 0) - 2 * w) + a(vel, 1, 0))) * c.dxi2
            VY = (nu[S] * ((a(vel, 0, -1) - 2 * w) + a(vel, 0, 1))) * c.dyi2
            Fm, km, rm = a(F, -di, -dj), a(kappa, -di, -dj), a(rho, -di, -dj)
            SG = np.where(F[S] == Fm, 0.0, ((((-c.sigma) * (F[S] - Fm)) * ((kappa[S] + km) / 2.0)) / h) * 2 / (rho[S] + rm))
            A = ((((VX + VY) - AX) - AY) + g) + SG
            r = (rho[S] + rm) * 0.5
            m = r * w
            dp = (a(p, 0, 0) - a(p, -di, -dj)) * (c.dxi if di else c.dyi)
            pieces = dict(VX=VX, VY=VY, AX=AX, AY=AY, SG=SG, A=A, r=r, m=m, vel=w)
            sums = {"KE": (m * w) * 0.5, "P_VISC": m * (VX + VY), "P_ADV": -(m * (AX + AY)), "P_GRAV": m * g, "P_SIGMA": m * SG, "P_PRES": -(w * dp)}
            return pieces, sums

        uf, us = face(u, 1, 0, c.gx, c.dx, 2, 1)
        vf, vs = face(v, 0, 1, c.gy, c.dy, 1, 2)

        def west(t):                                 # over the cells: row i = 1 has no west face
            out = np.zeros((nx, ny)); out[1:, :] = t
            return out

        def south(t):
            out = np.zeros((nx, ny)); out[:, 1:] = t
            return out

        terms["KE_U"] = west(us["KE"])              # (one face kind: one term per cell)
        terms["KE_V"] = south(vs["KE"])
        for k in ("P_VISC", "P_ADV", "P_GRAV", "P_SIGMA", "P_PRES"):
            terms[k] = (west(us[k]), south(vs[k]))
        sg = np.concatenate([np.abs(uf["SG"]).ravel(), np.abs(vf["SG"]).ravel()])
        amax = 0.0 if sg.size == 0 else math.inf if np.isnan(sg).any() else max(0.0, float(sg.max()))
    nu_faces, nv_faces = (nx - 1) * ny, nx * (ny - 1)
    count = {k: nx * ny for k in CELL_SUMS}
    count.update({k: nu_faces + nv_faces for k in FACE_SUMS})
    count.update(KE_U=nu_faces, KE_V=nv_faces)
    return types.SimpleNamespace(uf=uf, vf=vf, terms=terms, count=count, amax=amax, kappa=kin, rho=rho, nu=nu, nx=nx, ny=ny)


def flat(t):
    """All terms of a sum as one array (for fsum and the bound)."""
    return np.concatenate([x.ravel() for x in t]) if isinstance(t, tuple) else np.asarray(t).ravel()


def lane_order(t):
    """(terms, factor): the array to hand to fixed_order and what multiplies R (see the head of this file)."""
    if not isinstance(t, tuple):
        return t, 1
    w, s = t
    n, ny = w.shape
    nye = ny + (ny & 1)
    wp, sp = np.zeros((n, nye)), np.zeros((n, nye))
    wp[:, :ny], sp[:, :ny] = w, s
    out = np.zeros((2 * n, nye))
    out[0::2, 0::2], out[0::2, 1::2] = wp[:, 0::2], sp[:, 0::2]
    out[1::2, 0::2], out[1::2, 1::2] = wp[:, 1::2], sp[:, 1::2]
    return out, 2


def in_kernel_order(t, R):
    arr, k = lane_order(t)
    return fixed_order(arr, k * R, 256, "add")


def bound_of(t, n):
    """n 2^-52 fsum(|t|) (tests/_diag_np.py): what any order of summing the n terms may differ from their exact sum by.  n: the cells
    of a cell sum, the faces of a face sum (`count` of the restatement; the zeros of the cells without a face are not terms)."""
    return n * 2.0 ** -52 * math.fsum(np.abs(flat(t)))


def check(raw, res, istep=None, ctx="", say=None, R=None):
    """Hold a raw row (dict keyed by vof2d.energy.NAMES) to the restatement `res`; every figure goes through `say` first.
    R: the rows per wave chunk of the k_energy launch (diag_chunk_rows of tests/_interface_np.py); with it every sum must also equal
    the fixed-order sum of its terms (k_row_finish folds with 256 threads)."""
    msgs = []
    for k in SUMS:
        t = flat(res.terms[k])
        if np.isnan(t).any():
            ok = raw[k] != raw[k]
            line = "%s %s: %r, the terms hold a NaN" % (ctx, k, raw[k])
        else:
            exact, bound = math.fsum(t), bound_of(res.terms[k], res.count[k])
            ok = abs(raw[k] - exact) <= bound
            line = "%s %s: %r, fsum %r, |d| %.3e, bound %.3e" % (ctx, k, raw[k], exact, abs(raw[k] - exact), bound)
            if R is not None:
                fixed = in_kernel_order(res.terms[k], R)
                ok = ok and raw[k] == fixed
                line += ", in the kernels' order %r" % fixed
        if say:
            say(line)
        if not ok:
            msgs.append(line)
    line = "%s MAX_ACC_SIGMA: %r, restated %r" % (ctx, raw["MAX_ACC_SIGMA"], res.amax)
    if say:
        say(line)
    if not raw["MAX_ACC_SIGMA"] == res.amax:
        msgs.append(line)
    if not raw["CELLS"] == float(res.nx * res.ny):
        msgs.append("%s CELLS: %r, restated %r" % (ctx, raw["CELLS"], float(res.nx * res.ny)))
    if istep is not None and not raw["ISTEP"] == istep:
        msgs.append("%s ISTEP: %r, expected %r" % (ctx, raw["ISTEP"], istep))
    assert not msgs, " ; ".join(msgs)


def raw_from(res, istep=0):
    """A row as the device would report it, with the sums formed by math.fsum (one more order of summing)."""
    raw = {"ISTEP": float(istep), "CELLS": float(res.nx * res.ny), "MAX_ACC_SIGMA": res.amax}
    raw.update({k: math.fsum(flat(res.terms[k])) for k in SUMS})
    return raw
