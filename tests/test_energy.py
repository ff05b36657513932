"""The NumPy restatement of vof_energy (tests/_energy_np.py) judged on the CPU: it is the reference's momentum predictor face by
face (== against oracle/vof_oracle_np.py), its pressure power sums by parts to sum p * div, it gives the closed forms of a pool at rest
and of a uniform stream, and the host side (vof2d/energy.py, the option, the slots of the header) agrees with it.

Bounds are derived, not measured: a sum of n terms formed in any order lies within n 2^-52 fsum(|t|) of the exact sum (tests/_diag_np.py);
a closed form whose constants carry a few roundings of their own gets 16 more terms' worth.  Every figure is printed before it is asserted.
"""
import math
import os
import re

import numpy as np
import pytest

import _energy_np as enp
import _reduce_np as rnp
import vof_oracle_np as onp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(33, 17, 2, {}), (48, 80, 3, {"Lx": 0.06}), (64, 64, 1, {})]


def states(nx, ny, ic, kw, stops=(0, 1, 30)):
    """The f64 oracle state at every stop."""
    s = onp.new_state(nx, ny, ic, np.float64, "f32", **kw)
    done = 0
    for upto in stops:
        onp.step(s, upto - done)
        done = upto
        yield upto, s


@pytest.fixture(scope="module")
def restated():
    """(state copy, restatement) of every case and stop: computed once, read by the tests below."""
    out = {}
    for nx, ny, ic, kw in CASES:
        for upto, s in states(nx, ny, ic, kw):
            t = onp.new_state(nx, ny, ic, np.float64, "f32", **kw)
            for n in ("F", "u", "v", "p"):
                getattr(t, n)[...] = getattr(s, n)
            out[(nx, ny, ic, upto)] = (t, enp.restate(t.F, t.u, t.v, t.p, enp.params_of_oracle(t.prm)))
    return out


# ---------------------------------------------------------------------------- the restatement is the reference's predictor
@pytest.mark.parametrize("nx,ny,ic,kw", CASES)
def test_the_pieces_are_the_predictor(restated, nx, ny, ic, kw):
    for upto in (0, 1, 30):
        t, r = restated[(nx, ny, ic, upto)]
        onp.cal_nu_rho(t); onp.get_normal_young(t); onp.advect_upwind(t)
        dt = float(t.prm.dt)
        us = t.u[2:nx + 1, 1:ny + 1] + dt * r.uf["A"]
        vs = t.v[1:nx + 1, 2:ny + 1] + dt * r.vf["A"]
        ubad, vbad = int((us != t.u_star[2:nx + 1, 1:ny + 1]).sum()), int((vs != t.v_star[1:nx + 1, 2:ny + 1]).sum())
        crossed = int((t.F[2:nx + 1, 1:ny + 1] != t.F[1:nx, 1:ny + 1]).sum()), int((t.F[1:nx + 1, 2:ny + 1] != t.F[1:nx + 1, 1:ny]).sum())
        print("%dx%d ic %d step %d: u faces off %d, v faces off %d; faces the interface crosses %r; kappa off %d" % (
            nx, ny, ic, upto, ubad, vbad, crossed, int((r.kappa != t.kappa[1:-1, 1:-1]).sum())))
        assert np.array_equal(r.kappa, t.kappa[1:-1, 1:-1])
        assert np.array_equal(r.rho, t.rho) and np.array_equal(r.nu, t.nu)       # (the plain clamp gives the bits of var(0, 1, F) on these states)
        assert ubad == 0 and vbad == 0
        if upto:
            assert crossed[0] > 0 and crossed[1] > 0                             # the equal-F skip and the gather are both exercised
            assert (r.uf["SG"] != 0).any() and (r.vf["SG"] != 0).any()


# ---------------------------------------------------------------------------- summation by parts
@pytest.mark.parametrize("nx,ny,ic,kw", CASES)
def test_the_pressure_power_is_sum_p_div(restated, nx, ny, ic, kw):
    """sum over the faces of -(w * dp/dn) == sum over the cells of p * div, given that the wall faces are 0 (set_BC).  The right side's terms
    are the two products p * ((ue - uw) * dxi) and p * ((vn - vs) * dyi) of every cell: their sum is p * div, and each is rounded relative
    to itself, as the n 2^-52 fsum(|t|) rule assumes."""
    t, r = restated[(nx, ny, ic, 30)]
    prm = t.prm
    assert not t.u[1, :].any() and not t.u[nx + 1, :].any() and not t.v[:, 1].any() and not t.v[:, ny + 1].any()
    C = (slice(1, nx + 1), slice(1, ny + 1))
    px = t.p[C] * ((t.u[2:nx + 2, 1:ny + 1] - t.u[C]) * float(prm.dxi))
    py = t.p[C] * ((t.v[1:nx + 1, 2:ny + 2] - t.v[C]) * float(prm.dyi))
    left = enp.flat(r.terms["P_PRES"])
    right = np.concatenate([px.ravel(), py.ravel()])
    bound = enp.bound_of(r.terms["P_PRES"], r.count["P_PRES"]) + right.size * 2.0 ** -52 * math.fsum(np.abs(right))
    a, b = math.fsum(left), math.fsum(right)
    print("%dx%d ic %d: P_PRES %r, sum p div %r, |d| %.3e, bound %.3e" % (nx, ny, ic, a, b, abs(a - b), bound))
    assert a != 0.0 and abs(a - b) <= bound


# ---------------------------------------------------------------------------- closed forms
def test_a_pool_at_rest():
    from vof2d import energy
    nx, ny, Lx, Ly = 32, 24, 0.08, 0.03
    s = onp.new_state(nx, ny, 1, np.float64, "none", Lx=Lx, Ly=Ly)
    s.F[...] = 0.0
    s.F[:, 1:ny // 2 + 1] = 1.0
    onp.set_BC(s)
    prm = enp.params_of_oracle(s.prm)
    r = enp.restate(s.F, s.u, s.v, s.p, prm)
    d = energy.derive(enp.raw_from(r), prm["dx"], prm["dy"], prm["gx"], prm["gy"], prm["sigma"])
    n = nx * ny + 16
    cols = r.terms["SUM_GRADF"].sum(axis=1) * prm["dy"]
    print("pool: SUM_GRADF * dy per column in [%r, %r]; se %r, sigma Lx %r; pe %r" % (cols.min(), cols.max(), d["se"], prm["sigma"] * Lx, d["pe"]))
    assert np.all(np.abs(cols - 1.0) <= 8 * 2.0 ** -52)
    assert abs(d["se"] - prm["sigma"] * Lx) <= n * 2.0 ** -52 * prm["sigma"] * Lx
    H = Ly / 2
    pe = -prm["gy"] * Lx * (prm["rho_l"] * H * H / 2 + prm["rho_g"] * (Ly * Ly - H * H) / 2)      # the two layers, hydrostatic
    scale = abs(prm["gy"]) * math.fsum(enp.flat(r.terms["SUM_RHO_J"])) * prm["dy"] * prm["dx"] * prm["dy"]
    print("pool: pe %r, two layers %r, |d| %.3e, bound %.3e" % (d["pe"], pe, abs(d["pe"] - pe), n * 2.0 ** -52 * scale))
    assert pe > 0 and abs(d["pe"] - pe) <= n * 2.0 ** -52 * scale
    assert all(d[k] == 0.0 for k in ("ke", "p_visc", "p_adv", "p_grav", "p_sigma", "p_pres", "p_predictor"))
    assert d["e_mech"] == d["pe"] + d["se"]


def test_a_uniform_stream():
    nx, ny, U, gx = 20, 12, 0.25, 2.0
    s = onp.new_state(nx, ny, 1, np.float64, "f32", gx=gx, gy=0.0)
    s.F[...] = 1.0
    s.u[2:nx + 1, :] = U
    prm = enp.params_of_oracle(s.prm)
    raw = enp.raw_from(enp.restate(s.F, s.u, s.v, s.p, prm))
    print(raw)
    faces = (nx - 1) * ny
    assert raw["P_GRAV"] == 1000.0 * gx * U * faces and raw["KE_U"] == 1000.0 * U * U * 0.5 * faces     # (every factor is a dyadic fraction: exact)
    assert raw["KE_V"] == 0.0 and raw["P_SIGMA"] == 0.0 and raw["P_PRES"] == 0.0 and raw["MAX_ACC_SIGMA"] == 0.0
    assert raw["SUM_RHO"] == 1000.0 * nx * ny and raw["SUM_RHO_I"] == 1000.0 * ny * nx * (nx + 1) / 2 and raw["SUM_GRADF"] == 0.0
    # the first and the last column of u faces see the wall's zero: upwind advection and viscosity act there alone
    assert raw["P_ADV"] != 0.0 and raw["P_VISC"] != 0.0


# ---------------------------------------------------------------------------- the order of the sums
@pytest.mark.parametrize("n,ny,R", [(5, 3, 2), (7, 130, 4), (9, 257, 2)])
def test_two_terms_a_cell_fold_in_the_lane_order(n, ny, R):
    """lane_order: with one of the two terms 0 everywhere the fold is that of the other term alone, cell by cell (adding 0.0 changes no
    sum that started from +0.0); with both, the sum differs from either order of "all west, then all south" only by rounding."""
    rng = np.random.default_rng(n * 1000 + ny)
    w, s, z = rng.standard_normal((n, ny)), rng.standard_normal((n, ny)), np.zeros((n, ny))
    assert enp.in_kernel_order((w, z), R) == rnp.fixed_order(w, R, 256, "add")
    assert enp.in_kernel_order((z, s), R) == rnp.fixed_order(s, R, 256, "add")
    both = enp.in_kernel_order((w, s), R)
    assert abs(both - math.fsum(enp.flat((w, s)))) <= enp.bound_of((w, s), 2 * n * ny)
    # a lane's four terms of a row: west, south of its first column, then of its second
    one = np.zeros((1, 2)), np.zeros((1, 2))
    one[0][0, :], one[1][0, :] = (1.0, 2.0 ** -53), (-1.0, 2.0 ** -53)
    assert enp.in_kernel_order(one, 2) == (((0.0 + 1.0) + -1.0) + 2.0 ** -53) + 2.0 ** -53 == 2.0 ** -52       # ("all west, then all south": 2^-53)


# ---------------------------------------------------------------------------- the host side
def test_derive_and_rates():
    from vof2d import energy
    raw = dict(ISTEP=10, CELLS=12, KE_U=3.0, KE_V=1.0, P_VISC=-2.0, P_ADV=-1.0, P_GRAV=8.0, P_SIGMA=0.5, P_PRES=-4.0, SUM_RHO=100.0, SUM_RHO_I=300.0, SUM_RHO_J=250.0,
               SUM_GRADF=6.0, MAX_ACC_SIGMA=7.0)
    row = [0.0] * 16
    for k, name in enumerate(energy.NAMES):
        row[k] = float(raw[name])
    assert energy.raw_of(row) == {k: float(x) for k, x in raw.items()} and energy.raw_of(raw) is raw
    with pytest.raises(ValueError):
        energy.raw_of([0.0] * 5)
    d = energy.derive(row, 0.5, 0.25, 2.0, -4.0, 0.125)
    assert tuple(d) == energy.DERIVED
    assert d["ke"] == 0.5 and d["se"] == 0.125 * 6.0 * 0.125
    assert d["pe"] == -(2.0 * ((300.0 - 50.0) * 0.5) + -4.0 * ((250.0 - 50.0) * 0.25)) * 0.125 == -6.25
    assert d["e_mech"] == d["ke"] + d["pe"] + d["se"]
    assert (d["p_visc"], d["p_adv"], d["p_grav"], d["p_sigma"], d["p_pres"]) == (-0.25, -0.125, 1.0, 0.0625, -0.5)
    assert d["p_predictor"] == -0.25 - 0.125 + 1.0 + 0.0625 and d["max_acc_sigma"] == 7.0
    a = dict(d, istep=10)
    b = dict(d, istep=14, ke=d["ke"] + 0.5, pe=d["pe"] - 0.25, se=d["se"] + 0.125, p_predictor=0.75, p_pres=-0.5)
    (r,) = energy.rates([a, b], 0.125)
    assert tuple(r) == energy.RATES
    assert (r["istep"], r["time"], r["dke_dt"], r["dpe_dt"], r["dse_dt"]) == (14, 1.75, 1.0, -0.5, 0.25)
    assert r["residual"] == 1.0 - (0.75 - 0.5) and energy.rates([a], 0.125) == []


def test_the_slots_of_the_header():
    from vof2d import _abi, energy
    txt = open(os.path.join(ROOT, "include", "vof2d.h")).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define VOF_ENERGY_(\w+) (\d+)$", txt, flags=re.M)}
    assert header.pop("N") == _abi.VOF_ENERGY_N == 16
    assert header == {name: k for k, name in enumerate(energy.NAMES)} and len(header) == 14
    assert all(getattr(_abi, "VOF_ENERGY_" + name) == k == getattr(energy, name) for name, k in header.items())
    assert set(enp.SUMS) | {"ISTEP", "CELLS", "MAX_ACC_SIGMA"} == set(energy.NAMES)
    assert "energy" in _abi.SIGNATURES and _abi.SIGNATURES["step_energy"] == _abi.SIGNATURES["step_diag"]
    assert {"energy", "step_energy"} <= set(_abi.GPU_ONLY)


def test_the_option(capsys):
    from vof2d import cli, recorders
    assert cli.parse_args([]).energy_every is None                               # off by default
    args = cli.parse_args(["--energy-every", "5", "--diag-every", "10", "--interface-every", "5"])
    assert args.energy_every == 5
    for bad, msg in ((["--energy-every", "0"], "--energy-every needs N >= 1"), (["--energy-every", "5", "--gpus", "2"], "--energy-every runs on one GPU")):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
        assert msg in capsys.readouterr().err

    with pytest.raises(SystemExit) as err:                                       # (a parser that skipped the checks: the run itself refuses)
        cli.run(cli.build_parser().parse_args(["--energy-every", "5", "--gpus", "2"]), api=object(), rank=0, world=2)
    assert "--energy-every runs on one GPU" in str(err.value)

    class Drv:
        diag_every, diag_in_advance = 10, False
    kinds = lambda a, world: [type(r).__name__ for r in recorders.recorders_of(a, Drv(), world)]
    assert kinds(args, 1)[:3] == ["Diag", "Energy", "Interface"] and "Energy" not in kinds(cli.parse_args([]), 1)
    assert recorders.Energy.header.split(",") == ["istep", "time"] + list(__import__("vof2d.energy", fromlist=["DERIVED"]).DERIVED)


def test_the_kernel_header_stands_alone(tmp_path):
    import test_kernel_headers as tkh
    if tkh.HIPCC is None:
        pytest.skip("hipcc is not installed")
    tkh.test_header_compiles_alone(tmp_path, "energy.h")
    assert tkh.includes("energy.h") == ["curvature.h"]                          # young_sums, young_unit, kappa_csf; through it cells.h
