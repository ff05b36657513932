"""NumPy restatement of vof_step_mg for the tests: the verbs of oracle/vof_oracle_np.py around the V-cycle of
tests/_mg_np.py -- K cycles per step, warm-started from the previous step's p -- and, beside it, the reference's step
with its ten sweeps.  Both report per step the quantity vof_step_mg records:

    max|z| / max|p|,   z = ((b - c ap) - L p) / ap,   c = sum(b) / sum(ap)        (relative criterion, tests/_cg_np.py)

of the step's right-hand side b and the p the step's pressure solve leaves ("what one more sweep would still change,
beyond the drift, over the size of p").

Measured with this module (python tests/_step_mg_np.py 64 128 256), -ic 1, fp64, 50 steps from set_init_F, V(2,2), relative
criterion -- worst and last residual of the 50 steps, then the residual of steps 1 ... 5 and of steps 10, 20, 30, 40, 50:
    64x64 ten sweeps: worst 5.855e-02 (step 1), last 1.725e-03 | steps 1-5: 5.85e-02 4.30e-02 3.22e-02 2.51e-02 2.02e-02 | 10, 20, 30, 40, 50: 9.20e-03 2.93e-03 2.98e-03 5.81e-03 1.73e-03
    64x64 K = 1: worst 1.249e-03 (step 1), last 1.258e-06 | steps 1-5: 1.25e-03 1.16e-03 5.53e-04 2.49e-04 3.36e-04 | 10, 20, 30, 40, 50: 1.06e-05 9.87e-05 3.90e-05 8.69e-07 1.26e-06
    64x64 K = 2: worst 1.766e-04 (step 2), last 6.978e-08 | steps 1-5: 8.65e-05 1.77e-04 9.34e-05 6.05e-05 4.58e-05 | 10, 20, 30, 40, 50: 8.00e-07 6.35e-06 3.72e-07 1.17e-05 6.98e-08
    64x64 K = 3: worst 2.509e-05 (step 2), last 8.226e-09 | steps 1-5: 7.35e-06 2.51e-05 1.48e-05 1.01e-05 7.78e-06 | 10, 20, 30, 40, 50: 1.99e-07 9.81e-07 7.64e-08 1.47e-06 8.23e-09
    128x128 ten sweeps: worst 5.131e-02 (step 1), last 6.052e-04 | steps 1-5: 5.13e-02 4.35e-02 3.27e-02 2.55e-02 2.06e-02 | 10, 20, 30, 40, 50: 1.01e-02 4.77e-03 2.87e-03 1.98e-03 6.05e-04
    128x128 K = 1: worst 1.239e-03 (step 4), last 3.271e-04 | steps 1-5: 1.08e-03 8.66e-04 1.00e-03 1.24e-03 4.69e-04 | 10, 20, 30, 40, 50: 4.79e-04 3.33e-04 2.79e-04 1.10e-04 3.27e-04
    128x128 K = 2: worst 1.643e-04 (step 2), last 3.202e-05 | steps 1-5: 1.20e-04 1.64e-04 1.51e-04 1.54e-04 8.01e-05 | 10, 20, 30, 40, 50: 4.84e-05 6.57e-05 7.22e-05 5.22e-05 3.20e-05
    128x128 K = 3: worst 2.567e-05 (step 2), last 5.134e-06 | steps 1-5: 1.60e-05 2.57e-05 2.19e-05 2.15e-05 1.26e-05 | 10, 20, 30, 40, 50: 6.35e-06 8.99e-06 1.07e-05 7.50e-06 5.13e-06
    256x256 ten sweeps: worst 3.320e-02 (step 2), last 2.488e-03 | steps 1-5: 3.18e-02 3.32e-02 3.15e-02 2.92e-02 2.55e-02 | 10, 20, 30, 40, 50: 1.04e-02 4.99e-03 3.26e-03 2.40e-03 2.49e-03
    256x256 K = 1: worst 2.018e-03 (step 1), last 1.286e-03 | steps 1-5: 2.02e-03 5.51e-04 1.10e-03 1.28e-03 1.13e-03 | 10, 20, 30, 40, 50: 1.05e-03 1.31e-03 1.16e-03 9.02e-04 1.29e-03
    256x256 K = 2: worst 4.161e-04 (step 4), last 1.026e-04 | steps 1-5: 2.25e-04 8.29e-05 1.57e-04 4.16e-04 1.54e-04 | 10, 20, 30, 40, 50: 1.49e-04 1.55e-04 1.58e-04 1.09e-04 1.03e-04
    256x256 K = 3: worst 6.979e-05 (step 4), last 2.546e-05 | steps 1-5: 3.04e-05 1.33e-05 2.48e-05 6.98e-05 2.12e-05 | 10, 20, 30, 40, 50: 2.25e-05 1.63e-05 1.75e-05 2.45e-05 2.55e-05
The trend: one more cycle per step buys a factor 5 ... 8 in every step's residual at every size; a fixed K holds its level
as the grid grows from 128^2 to 256^2 within a factor 3; the ten sweeps leave a residual that falls only as the flow settles.
Choice of K for tests/test_step_mg_gpu.py (the smallest K whose worst residual over the 50 steps is at least 100 x below
the ten-sweep run's, at 256x256): K = 1 16 x, K = 2 80 x, K = 3 476 x -- K = 3, worst 6.979e-05; the GPU test gets 4 x
that, 2.8e-4 (the margin of the restatement tests of tests/test_mg_solve_gpu.py), which the ten-sweep run's residual
after step 50, 2.5e-3, exceeds 9-fold.
"""
import numpy as np

import _cg_np as cg
import _mg_np as mg
import vof_oracle_np as onp


def rhs_of(s):
    """The field rhs of 2dvof.py:239-241 with its ghost ring (zeros)."""
    prm = s.prm
    nx, ny = prm.nx, prm.ny
    C = (slice(1, nx + 1), slice(1, ny + 1))
    us, vs = s.u_star, s.v_star
    out = np.zeros_like(s.p)
    out[C] = s.rho[C] / prm.dt * ((us[2: nx + 2, 1: ny + 1] - us[C]) * prm.dxi + (vs[1: nx + 1, 2: ny + 2] - vs[C]) * prm.dyi)
    return out


def residual_of(s, rhs, criterion="rel"):
    maxz, maxp, _ = cg.z_of(s.p, rhs, s.prm.dxi2, s.prm.dyi2)
    return cg.residual_value(maxz, maxp, criterion)


def step_mg(s, nsteps, cycles, criterion="rel", nu=2):
    """nsteps steps of the definition in include/vof2d.h; returns the list of per-step residuals."""
    out = []
    for _ in range(nsteps):
        s.istep += 1
        onp.cal_nu_rho(s); onp.get_normal_young(s); onp.advect_upwind(s); onp.set_BC(s)
        rhs = rhs_of(s)
        hist = []
        # tol = -1 never satisfied: exactly `cycles` cycles, one check in front and one behind
        p, done, res, _ = mg.mg_solve(s.p, rhs, s.prm.dxi2, s.prm.dyi2, -1.0, cycles, cycles, criterion, nu=nu, history=hist)
        assert done == cycles
        s.p[...] = p
        out.append(res)
        onp.update_uv(s); onp.set_BC(s); onp.solve_VOF_rudman(s); onp.post_process_f(s); onp.set_BC(s)
    return out


def step_ten(s, nsteps, criterion="rel", sweeps=10):
    """The reference's step; the same residual of every step's p against that step's rhs."""
    out = []
    for _ in range(nsteps):
        s.istep += 1
        onp.cal_nu_rho(s); onp.get_normal_young(s); onp.advect_upwind(s); onp.set_BC(s)
        rhs = rhs_of(s)
        for _ in range(sweeps):
            onp.solve_p_jacobi(s)
        out.append(residual_of(s, rhs, criterion))
        onp.update_uv(s); onp.set_BC(s); onp.solve_VOF_rudman(s); onp.post_process_f(s); onp.set_BC(s)
    return out


def table(n, nsteps=50, ic=1, ks=(1, 2, 3)):
    rows = {"ten": step_ten(onp.new_state(n, n, ic, np.float64, "f32"), nsteps)}
    for k in ks:
        rows[k] = step_mg(onp.new_state(n, n, ic, np.float64, "f32"), nsteps, k)
    return rows


if __name__ == "__main__":
    import sys
    for n in [int(a) for a in sys.argv[1:]] or [64, 128]:
        rows = table(n)
        for key, r in rows.items():
            print("%dx%d %s: worst %.3e (step %d), last %.3e | steps 1-5: %s | 10, 20, 30, 40, 50: %s" % (
                n, n, "K = %d" % key if key != "ten" else "ten sweeps", max(r), 1 + int(np.argmax(r)), r[-1],
                " ".join("%.2e" % x for x in r[:5]), " ".join("%.2e" % r[i] for i in (9, 19, 29, 39, 49))), flush=True)
