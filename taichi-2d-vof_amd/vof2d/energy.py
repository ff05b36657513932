"""The energy budget of the flow reduced on the device (vof_energy, vof_step_energy; include/vof2d.h): the slots of a row, the
physical quantities a row stands for and the rates between consecutive rows.

A row is VOF_ENERGY_N doubles.  `Engine.energy()` returns it as a dict keyed by NAMES; `Engine.step_energy()` returns an
(rows, VOF_ENERGY_N) array whose rows `raw_of` turns into the same dict.

The powers are those of the momentum predictor's own terms (2dvof.py:206-233), each weighted with the face's momentum per volume
m = r w: sum m * T dx dy is the rate at which the term T of du/dt changes sum (1/2) r w^2 dx dy while r stands still.
"""
from ._abi import VOF_ENERGY_N

(ISTEP, CELLS, KE_U, KE_V, P_VISC, P_ADV, P_GRAV, P_SIGMA, P_PRES, SUM_RHO, SUM_RHO_I, SUM_RHO_J, SUM_GRADF, MAX_ACC_SIGMA) = range(14)
NAMES = ("ISTEP", "CELLS", "KE_U", "KE_V", "P_VISC", "P_ADV", "P_GRAV", "P_SIGMA", "P_PRES", "SUM_RHO", "SUM_RHO_I", "SUM_RHO_J", "SUM_GRADF",
         "MAX_ACC_SIGMA")
DERIVED = ("ke", "pe", "se", "e_mech", "p_visc", "p_adv", "p_grav", "p_sigma", "p_pres", "p_predictor", "max_acc_sigma")
RATES = ("istep", "time", "dke_dt", "dpe_dt", "dse_dt", "p_predictor", "p_pres", "residual")


def raw_of(row):
    """One row (a sequence of VOF_ENERGY_N doubles, or a dict already) as {name: value}."""
    if isinstance(row, dict):
        return row
    if len(row) != VOF_ENERGY_N:
        raise ValueError("a row of the energy budget has %d values, not %d" % (VOF_ENERGY_N, len(row)))
    return {name: float(row[k]) for k, name in enumerate(NAMES)}


def derive(raw, dx, dy, gx, gy, sigma):
    """What the sums stand for, per unit depth.  Cell (i, j) has its centre at ((i - 0.5) dx, (j - 0.5) dy), so the potential energy
    -sum rho (g . x) dx dy is measured from the origin of the domain; `se` is sigma times the interface length, as the integral of
    |grad F| (Youngs' gradient) measures it; the powers are in watts per metre of depth."""
    r = raw_of(raw)
    area = dx * dy
    ke = (r["KE_U"] + r["KE_V"]) * area
    pe = -(gx * ((r["SUM_RHO_I"] - 0.5 * r["SUM_RHO"]) * dx) + gy * ((r["SUM_RHO_J"] - 0.5 * r["SUM_RHO"]) * dy)) * area
    se = sigma * r["SUM_GRADF"] * area
    p = {k.lower(): r[k] * area for k in ("P_VISC", "P_ADV", "P_GRAV", "P_SIGMA", "P_PRES")}
    out = {"ke": ke, "pe": pe, "se": se, "e_mech": ke + pe + se}
    out.update(p)
    out["p_predictor"] = p["p_visc"] + p["p_adv"] + p["p_grav"] + p["p_sigma"]
    out["max_acc_sigma"] = r["MAX_ACC_SIGMA"]
    return out


def rates(rows, dt):
    """Between consecutive rows (dicts of `derive` with the row's ISTEP under "istep", in ascending step order): the finite-difference
    d ke / dt, d pe / dt and d se / dt, the powers of the later row, and residual = d ke / dt - (p_predictor + p_pres).

    The residual is NOT an error bound, and it does not vanish for an exact solver.  It holds everything the powers leave out: the
    change of the face densities r with F over the interval (the powers weigh du/dt with r as it stands in the later row), the time
    discretisation (a difference over the interval against powers sampled at its end, and the O(dt) term (1/2) r (dt A)^2 of an explicit
    step), and what the ten-sweep projection leaves undone: p is the iterate the corrector used, not the solution of the pressure
    equation, so -sum w . grad p is the work of that iterate."""
    out = []
    for a, b in zip(rows[:-1], rows[1:]):
        span = (b["istep"] - a["istep"]) * dt
        dke, dpe, dse = ((b[k] - a[k]) / span for k in ("ke", "pe", "se"))
        out.append({"istep": b["istep"], "time": b["istep"] * dt, "dke_dt": dke, "dpe_dt": dpe, "dse_dt": dse, "p_predictor": b["p_predictor"],
                    "p_pres": b["p_pres"], "residual": dke - (b["p_predictor"] + b["p_pres"])})
    return out
