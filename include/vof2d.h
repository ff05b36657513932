/*
 * vof2d.h -- C ABI of libvof2d_hip.so, the MI355X (gfx950) drop-in for the hot
 * path of houkensjtu/taichi-2d-vof's 2dvof.py.
 *
 * The reference has no FFI: its boundary is the set of zero-argument
 * @ti.kernel callables (2dvof.py:137,162,198,206,236,269,283,321,385,452),
 * the module-global ti.field objects (2dvof.py:53-93) with
 * .to_numpy()/.from_numpy() (2dvof.py:44,46,535,565) and the 0-D field
 * sigma[None] (2dvof.py:28-29).  Each entry point below names the reference
 * line range it replaces.  Plain pointers and sizes only; every function
 * returns 0 on success or a negative VOF_E* code (message via
 * vof_last_error).  No exceptions or aborts cross this boundary.
 *
 * Layout at the boundary (vof_get_field/vof_set_field): C-contiguous
 * (row_hi-row_lo+1, ny+2) arrays of the handle's dtype, index [i - row_lo][j],
 * ghosts included -- exactly what F.to_numpy() returns in the reference for
 * the full domain (row_lo = 0, row_hi = nx+1).  The internal device pitch and
 * padding are private (vof_field_view exposes them for zero-copy halo
 * exchange).
 *
 * Threading: one host thread per handle; verbs enqueue asynchronously on the
 * handle's HIP stream; vof_get_field, vof_get_counter, vof_sync and the
 * timer functions synchronise that stream.
 */
#ifndef VOF2D_H
#define VOF2D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: VOF_HALO_ROWS grew from jacobi_iters + 6 to jacobi_iters + 8 (overlap mode 5: the momentum march of k_tm reads F, u*, v* one
 * stencil further than the four-kernel step): strips and checkpoints laid out with the old macro are refused by vof_create instead of
 * failing later in vof_comm_init. */
#define VOF_ABI_VERSION 2

/* dtype of every field (2dvof.py:9 default_fp) */
#define VOF_F64 0
#define VOF_F32 1

/* error codes */
#define VOF_OK 0
#define VOF_EINVAL (-1)  /* bad argument / unknown name / size mismatch */
#define VOF_EHIP (-2)    /* a HIP runtime call failed (see vof_last_error) */
#define VOF_ENOMEM (-3)
#define VOF_ESTATE (-4)  /* call not valid in the handle's current state */

/* width (rows) of the per-step deep halo a strip needs on each interior side.
 * Dependency radius of one step in i: modes 0-4 (the four-kernel step) normals 1 +
 * curvature 1 + predictor 1 + n Jacobi sweeps + update_uv 1 + fct_x_sweep 2 (velocity) = n + 5 on the low side,
 * rhs 1 + n + fct_x_sweep 3 + ... = n + 5 on the high side; overlap mode 5 (the pair kernels: the momentum march of
 * k_tm reads F'', u*, v* one stencil further) n + 7; one spare row is allocated.  ABI version 1 had n + 6. */
#define VOF_HALO_ROWS(jacobi_iters) ((jacobi_iters) + 8)

typedef struct vof2d_desc {
  int32_t abi_version;    /* VOF_ABI_VERSION */
  int32_t nx, ny;         /* global interior cells (2dvof.py:19-20) */
  int32_t dtype;          /* VOF_F64 | VOF_F32 (2dvof.py:9) */
  int32_t coord_cast_f32; /* 1: keep .astype(np.float32) of 2dvof.py:43,45 */
  int32_t row_lo, row_hi; /* global rows stored by this handle, inclusive.
                             Full domain: 0 .. nx+1.  A strip stores its owned
                             rows plus halo rows. */
  int32_t own_lo, own_hi; /* rows this handle owns (counters, residuals) */
  int32_t jacobi_iters;   /* sweeps per step; 10 in 2dvof.py:521 */
  int32_t device;         /* HIP device ordinal, -1 = current */
  int32_t flags;          /* VOF_FLAG_* */
  double Lx, Ly;          /* 2dvof.py:22-23 */
  double rho_l, rho_g;    /* :24-25 */
  double nu_l, nu_g;      /* :26-27 */
  double sigma;           /* :28-29 (runtime, see vof_set_param) */
  double gx, gy;          /* :30-31 */
  double dt;              /* :33 */
} vof2d_desc;

#define VOF_FLAG_NO_GRAPH 1 /* vof_step launches kernels eagerly (no hipGraph) */

typedef struct vof2d_ctx* vof2d_handle;

/* Fill *d with the constants of 2dvof.py:19-33 for an nx x ny full domain. */
int vof_desc_default(vof2d_desc* d, int32_t nx, int32_t ny, int32_t dtype);

/* Allocate the fields of 2dvof.py:53-89 that are state or scratch of the hot
 * path, zero-initialised (Taichi zero-fills; the solver relies on it,
 * SURVEY 8c-S5).  stream: a hipStream_t to enqueue on, or NULL to create one. */
int vof_create(const vof2d_desc* d, void* stream, vof2d_handle* out);
int vof_destroy(vof2d_handle h);

/* ---- the reference verbs (zero-argument @ti.kernel callables) ---- */
int vof_set_init_F(vof2d_handle h, int32_t ic);     /* 2dvof.py:137-159 (+102-134) */
int vof_set_BC(vof2d_handle h);                     /* :162-189 */
int vof_cal_nu_rho(vof2d_handle h);                 /* :198-203 */
int vof_get_normal_young(vof2d_handle h);           /* :283-309 */
int vof_advect_upwind(vof2d_handle h);              /* :206-233 */
/* n calls of solve_p_jacobi() (:236-266): rhs once, n Jacobi sweeps
 * (ping-pong p/pt), result in p. */
int vof_solve_p_jacobi(vof2d_handle h, int32_t n);
int vof_update_uv(vof2d_handle h);                  /* :269-280 */
int vof_fct_x_sweep(vof2d_handle h);                /* :321-382 */
int vof_fct_y_sweep(vof2d_handle h);                /* :385-448 */
/* :312-318, sweep order from istep parity (even: y then x) */
int vof_solve_VOF_rudman(vof2d_handle h, int64_t istep);
int vof_post_process_f(vof2d_handle h);             /* :452-455 */

/* nsteps iterations of the solver part of the main loop, 2dvof.py:506-528
 * (istep += 1 first; 10 Jacobi sweeps; x/y sweep alternation), using the fused
 * kernel schedule: on a full domain four launches per step -- k_momentum, two
 * five-sweep k_jacobi_tb, k_transport -- replayed from a hipGraph (the first step after set_init_F /
 * set_field / a single verb runs eagerly with the intermediate boundary launches the reference's
 * :518 / :525 stand for; steady-state steps are replayed in batches of 16 / 8 / 2 per graph launch, as chains of
 * launches on row blocks); large grids (either precision: from 4 M cells on where at least half of the cells are
 * gas, from 16 M cells on whatever they hold, in fp32 also below 6 M -- a rule on the state, looked at once per handle and initial state) run two launches per step --
 * k_jacobi_pair (ten sweeps) and k_tm (the step's transport + the next step's momentum), DESIGN.md 3.5 / 3.6 -- in
 * batches of 32 / 8 / 2 that chain.  Whatever the form, F u v p u_star v_star rhs read back after n steps are the
 * reference's after n steps.  rho / nu / mx / my / kappa scratch is not materialised (the k_tm form uses mx, my,
 * kappa as its second set of u_star, v_star, rhs arrays). */
int vof_step(vof2d_handle h, int64_t nsteps);
/* The same step split at the points where a field becomes final, for drivers that overlap the
 * halo exchange with compute (vof2d/strips.py, vof_step_exchange):
 *   phase 0 = predictor + pressure solve + set_BC(p, F)                      -> p final
 *   phase 1 = update_uv folded into the first FCT sweep + set_BC(u, v)       -> u, v final
 *   phase 2 = second FCT sweep + post_process_f + set_BC(F) on the owned rows -> F final
 * Order 0, 1, 2; phase 0 increments istep.  Halo rows of F are not produced by the second sweep: they
 * are the neighbours' to send. */
int vof_step_phase(vof2d_handle h, int32_t phase);
int vof_get_istep(vof2d_handle h, int64_t* istep);
int vof_set_istep(vof2d_handle h, int64_t istep);

/* Extension (not in the reference, whose :521-522 runs a fixed 10 sweeps; SURVEY 8f-1, BASELINE
 * configs[1] "Jacobi Poisson to 1e-6 residual"): rhs once, then Jacobi sweeps (:258-266) until the
 * residual of the last sweep of a batch is <= tol, checked every check_every sweeps, at most
 * max_iters sweeps.  The sweeps of a batch run fused (five per launch; ten -- k_jacobi_pair -- on square cells from 4 M
 * cells on) and the last launch reduces the two norms itself.
 *   VOF_RESID_ABS:  residual = max|p_new - p|                                  over owned rows
 *   VOF_RESID_REL:  residual = max|p_new - p| / max(max|p_new|, VOF_RESID_TINY)   
 * A non-finite update (a diverged field) reads as residual = +inf and ends the solve; that is the only
 * way to +inf: a finite update over a tiny max|p_new| gives a relative residual clamped to DBL_MAX.
 * *residual is this handle's local value; a multi-GPU driver all-reduces the two norms of
 * vof_jacobi_sweeps_norms itself (vof2d/strips.py). */
#define VOF_RESID_ABS 0
#define VOF_RESID_REL 1
#define VOF_RESID_TINY 1e-300
int vof_solve_p(vof2d_handle h, double tol, int32_t max_iters, int32_t check_every, int32_t criterion,
                int32_t* iters_done, double* residual);
/* Extension: the same pressure equation solved by preconditioned conjugate gradients instead of sweeps.
 * The right-hand side b (the field "rhs") of the pure-Neumann problem does not sum to zero, so the sweeps have no fixed
 * point: they tend to the p for which one more sweep adds the same constant c = sum(b) / sum(ap) to every cell.  This
 * verb solves for that p -- L p = b - c ap, with L and ap the stencil of :258-263 -- by conjugate gradients on -L
 * preconditioned with its diagonal, warm-started from the p of the handle, whose additive constant it keeps.  With
 * r = (b - c ap) - L p and z = r / ap ("what one more sweep would still change, beyond the drift"):
 *   VOF_RESID_ABS:  residual = max|z|                                     over the interior
 *   VOF_RESID_REL:  residual = max|z| / max(max|p|, VOF_RESID_TINY)
 * through vof_residual_value; r is recomputed from p at the start and at every check (every check_every iterations, at
 * most max_iters).  A start that satisfies tol returns 0 iterations; a non-finite value reads as +inf and ends the
 * solve.  build_rhs as in vof_jacobi_sweeps_norms.  *drift receives c.  All sums are formed in double in a fixed
 * order: the same state and call give the same bits.  Whole-domain handles only (a strip returns VOF_ESTATE). */
int vof_solve_p_cg(vof2d_handle h, double tol, int32_t max_iters, int32_t check_every, int32_t criterion,
                   int32_t build_rhs, int32_t* iters_done, double* residual, double* drift);
/* Extension: the SAME equation, drift constant, residual, stopping rule and warm start as vof_solve_p_cg, by geometric
 * multigrid -- the coefficients of :258-262 are constants, so a fixed number of V-cycles does, whatever the grid size.
 * Level l has nx / 2^l x ny / 2^l cells and the stencil with dxi2 / 4^l, dyi2 / 4^l and the same wall rule; levels are
 * added while both extents are even and the coarser level keeps at least 4 cells each way.  A grid with an odd factor
 * therefore gets a shallow hierarchy and a large coarsest level (96 x 130 -> 48 x 65): correct, but slower -- nothing
 * is padded or re-gridded.  One cycle: mg_nu (knob, default 2) damped Jacobi sweeps (0.8), the 4-cell mean of the
 * residual down, ..., conjugate gradients on the coarsest level to 1e-2 of its starting max|z|, ..., bilinear
 * interpolation up, mg_nu sweeps.  Knob mg_levels caps the depth (-1: none; 1: the coarsest-level solver alone).
 * The check runs first and then every check_every cycles, at most max_cycles: a start that satisfies tol does 0 cycles
 * and changes nothing; a non-finite value reads as +inf at the first check.  *drift receives c.  No atomics, fixed
 * summation order: the same state and call give the same bits and the same count.  Whole-domain handles only (a strip
 * returns VOF_ESTATE and is left untouched). */
int vof_solve_p_mg(vof2d_handle h, double tol, int32_t max_cycles, int32_t check_every, int32_t criterion,
                   int32_t build_rhs, int32_t* cycles_done, double* residual, double* drift);
/* Extension: nsteps steps of the main loop (2dvof.py:506-528) in which the ten sweeps of :521-522 are replaced by
 * `cycles` V-cycles of vof_solve_p_mg's cycle on that verb's equation, warm-started from the handle's p.  After the call
 * every readable field, istep and the courant_violations counter hold, bit for bit, what this sequence leaves, n times:
 *   istep += 1; cal_nu_rho; get_normal_young; advect_upwind; set_BC;
 *   vof_solve_p_mg(tol = -1, max_cycles = cycles, check_every = cycles, criterion, build_rhs = 1);   (exactly `cycles` cycles)
 *   update_uv; set_BC; solve_VOF_rudman(istep); post_process_f; set_BC
 * with the same knobs (mg_nu, mg_levels, mg_graph, mg_coarse_block).  The residual of every step is recorded on the
 * device; nothing is read back before the end of the call.  *last_residual: the residual that verb returns in the last
 * step (same kernels, same order of sums: equal bits); *worst_residual: the largest of the nsteps residuals;
 * *worst_step: the istep it belongs to (the first one on a tie).  A non-finite field reads as +inf (vof_residual_value)
 * and the steps go on.  nsteps = 0 does nothing and reports 0, 0, 0.  Any of the three pointers may be NULL; if all are,
 * the call does not synchronise.  cycles >= 1 and a valid criterion, else VOF_EINVAL; whole-domain handles only (a
 * strip returns VOF_ESTATE and is left untouched).  Steady-state steps replay one captured graph per step (none with
 * VOF_FLAG_NO_GRAPH or knob mg_graph = 0: same bits); calls interleave with vof_step in any order.
 * Knob "mg_coarse_block" (vof_set_param; default 0): the coarsest-level solve of a cycle -- of this verb and of
 * vof_solve_p_mg -- as one launch of one workgroup with the level held in LDS, where that level has at most 1024 cells
 * counting its ghost ring; vof_get_param reads 1 only where it is in effect.  Same solver, another order of sums:
 * other bits than the launches'. */
int vof_step_mg(vof2d_handle h, int64_t nsteps, int32_t cycles, int32_t criterion,
                double* last_residual, double* worst_residual, int64_t* worst_step);
/* Extension: what a user of a volume-of-fluid code watches, reduced on the device in one pass over F, u, v instead of
 * copying the fields to the host.  A row is VOF_DIAG_N doubles (unused slots read 0), over the handle's owned interior
 * cells, i in [max(own_lo, 1), min(own_hi, nx)] and j in [1, ny]; every operand is converted to double first:
 *   ISTEP     the handle's istep                      CELLS   the number of cells summed
 *   SUM_F     sum F                                   SUM_FI, SUM_FJ   sum F * i, sum F * j  (global integer indices: the host
 *             forms the coordinates, xc = (SUM_FI / SUM_F - 0.5) dx)
 *   SUM_KE    sum rho * 0.5 * (uc * uc + vc * vc), uc = (u[i,j] + u[i+1,j]) * 0.5, vc = (v[i,j] + v[i,j+1]) * 0.5 (interp_velocity,
 *             :492), rho = rho_g * (1 - Fc) + rho_l * Fc (:202) with the plain clamp Fc = fmin(fmax(F, 0), 1)
 *   SUM_DIV2, MAX_DIV   sum div * div and max |div|, div = (u[i+1,j] - u[i,j]) * dxi + (v[i,j+1] - v[i,j]) * dyi, with the dxi, dyi of
 *             vof_get_param: what the projection leaves in u, v
 *   MAX_U, MAX_V   max(|u[i,j]|, |u[i+1,j]|) and max(|v[i,j]|, |v[i,j+1]|) over the cells (both faces of every owned cell)
 *   MIN_F, MAX_F
 * The expression order is stated in csrc/kernels/diag.h; the sums are formed in double in a fixed order (no atomics): the
 * same state gives the same bits.  A NaN operand of a maximum counts as +inf (a NaN F: MAX_F = +inf, MIN_F = -inf), the
 * sums propagate it; nothing is skipped.  The values are those of the arrays vof_get_field would return at that moment
 * (ghost cells a fused step left virtual are settled first); no field, istep, counter or cached graph changes, and a
 * vof_step that follows gives the bits it would have given without the call.  Works on strip handles: the value is the
 * handle's partial (row own_hi + 1 of u is a stored halo row), the driver combines the partials (vof2d/diag.py).
 * Synchronises and copies the row to out. */
#define VOF_DIAG_ISTEP 0
#define VOF_DIAG_SUM_F 1
#define VOF_DIAG_SUM_FI 2
#define VOF_DIAG_SUM_FJ 3
#define VOF_DIAG_SUM_KE 4
#define VOF_DIAG_SUM_DIV2 5
#define VOF_DIAG_MAX_DIV 6
#define VOF_DIAG_MAX_U 7
#define VOF_DIAG_MAX_V 8
#define VOF_DIAG_MIN_F 9
#define VOF_DIAG_MAX_F 10
#define VOF_DIAG_CELLS 11
#define VOF_DIAG_N 16
int vof_diagnostics(vof2d_handle h, double* out /* VOF_DIAG_N */);
/* Extension: nsteps steps that record a time series of those rows on the device.  For r = 0 .. nsteps / every - 1: `every`
 * steps -- exactly vof_step(h, every) if mg_cycles == 0, exactly vof_step_mg(h, every, mg_cycles, criterion, NULL, NULL,
 * NULL) if mg_cycles >= 1 -- then row r; a remainder of nsteps % every steps is stepped and gets no row.  Nothing waits
 * for the device before the end of the call; then one copy writes rows x VOF_DIAG_N doubles to out and *rows_written
 * (may be NULL) is set.  Row r equals, bit for bit, what the loop "step `every` steps; vof_diagnostics" yields on a twin
 * handle, and every readable field, istep and courant_violations end where that loop (and a single vof_step(nsteps))
 * leaves them.  every < 1, nsteps < 0, cap_rows < nsteps / every, out == NULL with a row due, mg_cycles < 0, a bad
 * criterion with mg_cycles >= 1: VOF_EINVAL; a strip handle: VOF_ESTATE; the handle is left untouched by either.
 * nsteps == 0 does nothing and reports 0 rows. */
int vof_step_diag(vof2d_handle h, int64_t nsteps, int64_t every, int32_t mg_cycles, int32_t criterion,
                  double* out, int64_t cap_rows, int64_t* rows_written);
/* Extension: the interface itself, as one PLIC (piecewise-linear) segment per mixed cell, reconstructed and compacted on the device
 * instead of copying F to the host and contouring it.  Cells: the handle's owned interior cells, i in [max(own_lo, 1), min(own_hi, nx)],
 * j in [1, ny]; every operand is converted to double first (one code path for both dtypes).
 *   mixed       eps < F && F < 1 - eps (a NaN F is not mixed); eps NaN, negative or >= 0.5: VOF_EINVAL
 *   mxsum, mysum  Youngs' gradient of 2dvof.py:287-297 in that order of operations, with the double dx, dy of vof_get_param, on the array
 *               vof_get_field would return at that moment (ghost cells a fused step left virtual are settled first)
 *   degenerate  |mxsum| < 1e-10 && |mysum| < 1e-10 (the reference's test, :300): counted in SUM_DEGENERATE, no row
 *   the line    in the unit cell, with a = |mxsum| dx and b = |mysum| dy scaled to a + b = 1, n1 = min, n2 = max, Fm = min(F, 1 - F):
 *               alpha = sqrt(2 n1 n2 Fm) if 2 n2 Fm < n1, else n2 Fm + n1 / 2; alpha -> 1 - alpha if F > 0.5; liquid is a xi + b eta < alpha.
 *               One end lies on xi = 0 if b > 0 and alpha <= b, else on eta = 1; the other on eta = 0 if a > 0 and alpha <= a, else on
 *               xi = 1; xi -> 1 - xi if mxsum < 0, eta -> 1 - eta if mysum < 0; x = (i - 1 + xi) dx, y = (j - 1 + eta) dy
 *   ties        every comparison above is the one written: eps < F and F < 1 - eps are strict (F == eps and F == 1 - eps, the double
 *               1.0 - eps, are not mixed), 2 n2 Fm < n1 is strict, alpha <= b and alpha <= a take the tie, mxsum < 0 and mysum < 0 leave a
 *               zero (of either sign) unmirrored, n1 = n2 where a == b and Fm = 0.5 where F == 0.5.  At a == b, F == 0.5 (Fm),
 *               alpha == a, alpha == b, mxsum == 0 and mysum == 0 both branches give the same row; at F == 0.5 (alpha -> 1 - alpha) and at
 *               2 n2 Fm == n1 they may differ in the last bits, and the written one holds
 *   a row       VOF_IFACE_N doubles: I, J (global cell indices), (X0, Y0) -> (X1, Y1) ordered so that the liquid lies to the LEFT,
 *               (NX, NY) = (mxsum, mysum) / its Euclidean norm: the unit normal in physical space, liquid -> gas
 * The expression order is stated in csrc/kernels/interface.h.  Rows come in ascending (i, j) order, i first.  At most cap_rows rows are
 * written and nothing behind min(SEGMENTS, cap_rows) rows is touched; `summary` always describes ALL segments, so rows = NULL with
 * cap_rows = 0 sizes a buffer or reads the length alone:
 *   SUM_SEGMENTS    rows that exist (may exceed cap_rows)          SUM_DEGENERATE  mixed cells without an orientation
 *   SUM_LENGTH      sum of sqrt(ddx * ddx + ddy * ddy) over all segments, in double, in the fixed order that file states
 *   SUM_ISTEP       the handle's istep
 * No atomics anywhere: the same state and call give the same bytes.  No field, istep, counter or cached graph changes, and a vof_step /
 * vof_step_mg / vof_step_diag that follows gives the bits it would have given without the call.  Works on strip handles: the value is
 * the strip's own rows (the neighbours i -+ 1 of an owned row are stored halo rows); the strips' rows in rank order are the domain's
 * list.  rows == NULL with cap_rows > 0, cap_rows < 0, summary == NULL, a bad eps, more than 2^31 - 1 cells: VOF_EINVAL, the handle
 * untouched.  Synchronises and copies out. */
#define VOF_IFACE_I 0   /* global cell indices, as doubles */
#define VOF_IFACE_J 1
#define VOF_IFACE_X0 2  /* end points in physical coordinates; liquid lies to the LEFT of (X0,Y0) -> (X1,Y1) */
#define VOF_IFACE_Y0 3
#define VOF_IFACE_X1 4
#define VOF_IFACE_Y1 5
#define VOF_IFACE_NX 6  /* unit normal in physical space, liquid -> gas (the direction of mxsum, mysum) */
#define VOF_IFACE_NY 7
#define VOF_IFACE_N 8
#define VOF_IFACE_SUM_SEGMENTS 0   /* slots of `summary`: rows that exist (may exceed cap_rows) */
#define VOF_IFACE_SUM_DEGENERATE 1 /* mixed cells with no orientation: counted, no row */
#define VOF_IFACE_SUM_LENGTH 2     /* sum of the segments' physical lengths, ALL segments, fixed order */
#define VOF_IFACE_SUM_ISTEP 3
#define VOF_IFACE_SUM_N 4
int vof_interface(vof2d_handle h, double eps, double* rows, int64_t cap_rows, double* summary /* VOF_IFACE_SUM_N */);
/* Extension: how curved the interface is, by height functions, and how far the solver's own curvature (the CSF kappa = -div of Youngs'
 * normals, 2dvof.py:283-309) is from that.  One row per mixed cell with an orientation, the cells and the order of vof_interface at the
 * same eps (the I, J columns are equal row for row).  Whole-domain handles only (the stencil reaches three rows: a strip returns
 * VOF_ESTATE, as does a phased step in progress).  Every operand is converted to double first; ghost cells a fused step left virtual
 * are settled first; f(ii, jj) = F[clamp(ii, 0, nx + 1), clamp(jj, 0, ny + 1)].
 *   mixed, degenerate, mxsum, mysum   as vof_interface
 *   AXIS        |mxsum| dx > |mysum| dy ? 1 : 0 -- 1: the heights are summed along i, 0 (and the tie): along j
 *   heights     H[d], d = -1, 0, 1: the sum over t = -3 .. 3 of the raw f(i + d, j + t) (AXIS 0) or f(i + t, j + d) (AXIS 1)
 *   VALID       1.0 if in all three columns the end cell on the liquid side (t = -3 if the normal component along the axis is >= 0,
 *               else t = 3) is >= 1 - eps and the end cell on the gas side is <= eps (a NaN fails); else 0.0
 *   KAPPA, HP   with (hs, ht) = (dy, dx) for AXIS 0, (dx, dy) for AXIS 1: hp = (H[1] - H[-1]) hs / (2 ht),
 *               hpp = (H[1] - 2 H[0] + H[-1]) hs / ht^2, KAPPA = hpp / (1 + hp^2)^(3/2), HP = hp; both 0 where VALID is 0.
 *               The solver's sign: -1/R for a drop, +1/R for a bubble
 *   KAPPA_CSF   the solver's own curvature at the cell, evaluated in double: on an f64 handle, bit for bit, kappa[i, j] directly after
 *               vof_get_normal_young on the same F (normals of cells outside [1, nx] x [1, ny] are 0, as the reference leaves them)
 *   a row       VOF_CURV_N doubles: I, J, KAPPA, VALID, AXIS, KAPPA_CSF, HP, F
 * The expression order is stated in csrc/kernels/curvature.h.  Rows come in ascending (i, j) order, i first.  At most cap_rows rows are
 * written and nothing behind min(ROWS, cap_rows) rows is touched; `summary` always describes ALL rows, so rows = NULL with cap_rows = 0
 * sizes a buffer.  The summary, VOF_CURV_SUM_N doubles (unused slots read 0), sums in double in the fixed order that file states:
 *   SUM_ROWS (may exceed cap_rows), SUM_DEGENERATE, SUM_VALID; SUM_K, SUM_K2, MIN_K, MAX_K of KAPPA over the VALID rows; SUM_CSF,
 *   SUM_CSF2, MIN_CSF, MAX_CSF of KAPPA_CSF over all rows; ISTEP.  A NaN operand makes a maximum +inf and a minimum -inf; with no
 *   operand a sum reads 0, a maximum -inf and a minimum +inf.
 * No atomics anywhere: the same state and call give the same bytes.  No field, istep, counter or cached graph changes, and a vof_step*
 * that follows gives the bits it would have given without the call.  rows == NULL with cap_rows > 0, cap_rows < 0, summary == NULL, a
 * bad eps (the rule of vof_interface), more than 2^31 - 1 cells: VOF_EINVAL, the handle untouched.  Synchronises and copies out. */
#define VOF_CURV_I 0          /* global cell indices, as doubles */
#define VOF_CURV_J 1
#define VOF_CURV_KAPPA 2      /* height-function curvature (0 where VALID is 0) */
#define VOF_CURV_VALID 3      /* 1.0: the three columns span the interface */
#define VOF_CURV_AXIS 4       /* 1.0: heights summed along i; 0.0: along j */
#define VOF_CURV_KAPPA_CSF 5  /* the solver's own curvature at the cell */
#define VOF_CURV_HP 6         /* the slope of the height function (0 where VALID is 0) */
#define VOF_CURV_F 7
#define VOF_CURV_N 8
#define VOF_CURV_SUM_ROWS 0       /* slots of `summary`: rows that exist (may exceed cap_rows) */
#define VOF_CURV_SUM_DEGENERATE 1 /* mixed cells with no orientation: counted, no row */
#define VOF_CURV_SUM_VALID 2      /* rows whose VALID is 1 */
#define VOF_CURV_SUM_K 3          /* KAPPA over the VALID rows: sum, sum of squares, minimum, maximum */
#define VOF_CURV_SUM_K2 4
#define VOF_CURV_SUM_MIN_K 5
#define VOF_CURV_SUM_MAX_K 6
#define VOF_CURV_SUM_CSF 7        /* KAPPA_CSF over all rows: sum, sum of squares, minimum, maximum */
#define VOF_CURV_SUM_CSF2 8
#define VOF_CURV_SUM_MIN_CSF 9
#define VOF_CURV_SUM_MAX_CSF 10
#define VOF_CURV_SUM_ISTEP 11
#define VOF_CURV_SUM_N 16
int vof_curvature(vof2d_handle h, double eps, double* rows, int64_t cap_rows, double* summary /* VOF_CURV_SUM_N */);
/* Extension: where the flow's energy is and which term of the scheme is moving it, reduced on the device in one pass over F, u, v, p
 * instead of copying four fields to the host.  A row is VOF_ENERGY_N doubles (unused slots read 0) over the cells i in [1, nx], j in
 * [1, ny] and the faces the momentum predictor updates: the u faces i in [2, nx], j in [1, ny] and the v faces i in [1, nx], j in [2, ny].
 * Whole-domain handles only (the stencil reaches three rows of F: a strip returns VOF_ESTATE, as does a phased step in progress).  Every
 * operand is converted to double first (one code path for both dtypes), the constants are the doubles of vof_get_param; ghost cells a
 * fused step left virtual are settled first.  With Fc = fmin(fmax(F, 0), 1), rho = rho_g * (1 - Fc) + rho_l * Fc, nu = nu_l * Fc +
 * nu_g * (1.0 - Fc) (:202-203) and kappa the KAPPA_CSF of vof_curvature, a u face has, in the order of operations of 2dvof.py:209-219,
 *   w = u[i,j]   v_here (:209)   dudx, dudy (:210-211, the upwind selects)
 *   VX = nu[i,j] (u[i-1,j] - 2 w + u[i+1,j]) dxi2   VY = nu[i,j] (u[i,j-1] - 2 w + u[i,j+1]) dyi2   AX = w dudx   AY = v_here dudy
 *   SG = F[i,j] == F[i-1,j] ? 0 : -sigma (F[i,j] - F[i-1,j]) (kappa[i,j] + kappa[i-1,j]) / 2 / dx * 2 / (rho[i,j] + rho[i-1,j])   (the raw F)
 *   A = VX + VY - AX - AY + gx + SG: on an f64 handle w + dt * A is, bit for bit, the predictor's u_star[i,j]
 *   r = (rho[i,j] + rho[i-1,j]) * 0.5 (:272)   m = r w
 * and a v face the mirror (:222-232, :277: u_here, dvdx selected on u_here > 0, dvdy on v[i,j] > 0, gy, dy, rho[i,j] + rho[i,j-1]).
 *   ISTEP, CELLS       the handle's istep; nx * ny
 *   KE_U, KE_V         sum over the faces of (m * w) * 0.5
 *   P_VISC, P_ADV, P_GRAV, P_SIGMA   sums over both face kinds of m * (VX + VY), -(m * (AX + AY)), m * g, m * SG: the rate at which each
 *                      term of the predictor feeds (or drains) the kinetic energy, per dx dy
 *   P_PRES             sum of -(w * ((p[i,j] - p[i-1,j]) * dxi)) and of the v mirror with dyi: summed by parts, sum p * div
 *   SUM_RHO, SUM_RHO_I, SUM_RHO_J   sum rho, rho * i, rho * j over the cells (global integer indices as doubles, as SUM_FI, SUM_FJ)
 *   SUM_GRADF          sum over the cells of sqrt(mxsum^2 + mysum^2), Youngs' gradient of vof_interface: the interface length per dx dy
 *   MAX_ACC_SIGMA      max |SG| over both face kinds; starts at 0, a NaN counts as +inf
 * The full expression order is stated in csrc/kernels/energy.h; a face belongs to the cell it is the west or south face of and the sums are
 * formed in double in the fixed order of vof_diagnostics (no atomics): the same state gives the same bits, in either build.  A NaN operand
 * reaches exactly the sums whose terms hold it.  vof2d/energy.py forms the physical quantities.  No field, istep, counter or cached graph
 * changes, and a vof_step* that follows gives the bits it would have given without the call.  Synchronises and copies the row to out. */
#define VOF_ENERGY_ISTEP 0
#define VOF_ENERGY_CELLS 1
#define VOF_ENERGY_KE_U 2
#define VOF_ENERGY_KE_V 3
#define VOF_ENERGY_P_VISC 4
#define VOF_ENERGY_P_ADV 5
#define VOF_ENERGY_P_GRAV 6
#define VOF_ENERGY_P_SIGMA 7
#define VOF_ENERGY_P_PRES 8
#define VOF_ENERGY_SUM_RHO 9
#define VOF_ENERGY_SUM_RHO_I 10
#define VOF_ENERGY_SUM_RHO_J 11
#define VOF_ENERGY_SUM_GRADF 12
#define VOF_ENERGY_MAX_ACC_SIGMA 13
#define VOF_ENERGY_N 16
int vof_energy(vof2d_handle h, double* out /* VOF_ENERGY_N */);
/* Extension: nsteps steps that record a time series of those rows on the device -- the contract of vof_step_diag with vof_energy in the
 * place of vof_diagnostics: groups of `every` steps (vof_step, or vof_step_mg with mg_cycles >= 1), row r behind group r, a remainder
 * stepped without a row, nothing waits before the end of the call, one copy of rows x VOF_ENERGY_N doubles out.  Row r equals, bit for
 * bit, what the loop "step `every` steps; vof_energy" yields on a twin handle, and the state ends where vof_step(nsteps) / vof_step_mg
 * leaves it.  The argument errors are those of vof_step_diag (VOF_EINVAL); a strip handle or a phased step in progress: VOF_ESTATE; the
 * handle is left untouched by either.  nsteps == 0 does nothing and reports 0 rows. */
int vof_step_energy(vof2d_handle h, int64_t nsteps, int64_t every, int32_t mg_cycles, int32_t criterion,
                    double* out, int64_t cap_rows, int64_t* rows_written);
/* Extension: how many pieces the liquid (or the gas) is in, and what each piece is doing: connected-component labelling and per-blob
 * sums on the device instead of copying F, u, v to the host.  Cells: the handle's owned interior cells, i in [max(own_lo, 1), min(own_hi, nx)],
 * j in [1, ny]; ghost cells are never members; every operand is converted to double first (one code path for both dtypes).
 *   member      VOF_BLOB_LIQUID: F >= threshold; VOF_BLOB_GAS: F < threshold; a NaN F is a member of neither
 *   a blob      a maximal set of members connected through shared faces (4-connectivity: diagonal neighbours are not connected).  Its
 *               FIRST CELL is its smallest cell in ascending (i, j) order, i first; blobs are listed in ascending order of their first cell
 *   a row       VOF_BLOB_N doubles (unused slots read 0): I0, J0 the first cell (global indices); CELLS; IMIN, IMAX, JMIN, JMAX the extent
 *               (all integers, exact as doubles); SUM_W, SUM_WI, SUM_WJ = sum of w, w i, w j with w = Fc (liquid) or 1 - Fc (gas),
 *               Fc = fmin(fmax(F, 0), 1), i and j the global integer indices -- the volume is SUM_W dx dy, the centroid
 *               xc = (SUM_WI / SUM_W - 0.5) dx, yc = (SUM_WJ / SUM_W - 0.5) dy; SUM_WU, SUM_WV = sum of w uc, w vc with the cell-centre
 *               velocities uc = (u[i,j] + u[i+1,j]) / 2, vc = (v[i,j] + v[i,j+1]) / 2 of interp_velocity (2dvof.py:492), the expressions of
 *               vof_diagnostics -- the blob's velocity is SUM_WU / SUM_W.  A NaN in u or v reaches the sums of the blob that holds it only
 *   summary     SUM_BLOBS the blobs that exist (may exceed cap_rows), SUM_MEMBER_CELLS, SUM_MAX_CELLS the size of the largest blob,
 *               SUM_ISTEP the handle's istep; it always describes ALL blobs, so rows = NULL with cap_rows = 0 sizes a buffer
 *   labels      optional (NULL skips them): a dense (owned interior rows, ny) array of int32, the 0-based index of the cell's blob in the
 *               full list (also of blobs beyond cap_rows), -1 for a non-member; labels_bytes must match exactly
 * At most cap_rows rows are written and nothing behind min(BLOBS, cap_rows) rows is touched.  The same state and call give the same bytes,
 * on any run and any handle: the integers come from 32-bit integer atomics (independent of arrival order), the five sums are formed in
 * double in the fixed order csrc/kernels/blobs.h states, which depends on the geometry and the blob's own extent alone; no floating-point
 * atomics.  No field, istep, counter or cached graph changes, and a vof_step / vof_step_mg / vof_step_diag that follows gives the bits it
 * would have given without the call.  Works on strip handles: the value is that of the strip's own rows as if the strip's edges were
 * walls (row own_hi + 1 of u is a stored halo row); a driver joins the strips' lists (vof2d/blobs.py, combine).  A phase other than the
 * two, a threshold NaN or outside (0, 1), cap_rows < 0, rows == NULL with cap_rows > 0, summary == NULL, a wrong labels_bytes, more than
 * 2^31 - 1 cells: VOF_EINVAL, the handle untouched.  Synchronises and copies out. */
#define VOF_BLOB_LIQUID 0
#define VOF_BLOB_GAS 1
#define VOF_BLOB_I0 0     /* the first cell, global indices as doubles */
#define VOF_BLOB_J0 1
#define VOF_BLOB_CELLS 2
#define VOF_BLOB_IMIN 3
#define VOF_BLOB_IMAX 4
#define VOF_BLOB_JMIN 5
#define VOF_BLOB_JMAX 6
#define VOF_BLOB_SUM_W 7
#define VOF_BLOB_SUM_WI 8
#define VOF_BLOB_SUM_WJ 9
#define VOF_BLOB_SUM_WU 10
#define VOF_BLOB_SUM_WV 11
#define VOF_BLOB_N 16
#define VOF_BLOB_SUM_BLOBS 0
#define VOF_BLOB_SUM_MEMBER_CELLS 1
#define VOF_BLOB_SUM_MAX_CELLS 2
#define VOF_BLOB_SUM_ISTEP 3
#define VOF_BLOB_SUM_N 4
int vof_blobs(vof2d_handle h, int32_t phase, double threshold, double* rows, int64_t cap_rows,
              int32_t* labels, size_t labels_bytes, double* summary /* VOF_BLOB_SUM_N */);
/* Extension: where a fluid element goes.  Passive tracer particles owned by the handle, moved with the flow on the device instead of
 * copying u, v to the host every step.  All tracer arithmetic is in double, whatever the handle's dtype: every field operand is
 * converted to double on load (one code path).  dx, dy, dxi, dyi, Lx, Ly, dt are the Python-double values vof_get_param returns.
 *   positions   physical, x in [0, Lx], y in [0, Ly]; cell i covers [(i - 1) dx, i dx] (the convention of vof_interface)
 *   the fields  u[i,j] sits at ((i - 1) dx, (j - 0.5) dy), v[i,j] at ((i - 0.5) dx, (j - 1) dy), F[i,j] at ((i - 0.5) dx, (j - 0.5) dy);
 *               ghost cells count, with the values vof_get_field would return at that moment (ghost cells a fused step left virtual
 *               are settled first)
 *   a sample    bilinear, of a field f at (x, y): s = x * dxi + ox, t = y * dyi + oy with (ox, oy) = (0, 0.5) for u, (0.5, 0) for v,
 *               (0.5, 0.5) for F; ib = floor(s) + (ox == 0 ? 1 : 0) clamped to [1, nx] for u and to [0, nx] for v and F,
 *               a = s - (ib - (ox == 0 ? 1 : 0)); likewise jb from t, clamped to [1, ny] for v and to [0, ny] for u and F, and b; then, in
 *               exactly this order, lo = f[ib,jb] + a * (f[ib+1,jb] - f[ib,jb]), hi = f[ib,jb+1] + a * (f[ib+1,jb+1] - f[ib,jb+1]),
 *               value = lo + b * (hi - lo).  With these clamps every load lies inside the stored (nx + 2, ny + 2) array for any position
 *               of the closed domain, walls and corners included
 *   an advance  by a time h, on the frozen velocity field, by the explicit midpoint rule: k1 = (u, v)(x, y); xm = x + (0.5 * h) * k1.u,
 *               ym likewise; if xm or ym is not finite the tracer is lost, otherwise both are clamped; k2 = (u, v)(xm, ym);
 *               x' = x + h * k2.u, y' likewise; if either is not finite the tracer is lost, otherwise both are clamped.  The clamp is
 *               c < 0 ? 0 : (c > L ? L : c) (it keeps a NaN)
 *   lost        a lost tracer gets x = y = NaN and is never moved or sampled again; its U, V, F read NaN.  Nothing is skipped
 *               silently: lost tracers are counted
 *   a row       VOF_TRACER_N doubles: X, Y and U, V, F sampled at the tracer's current position; unused slots read 0.  Rows come in
 *               the order the tracers were given: a tracer's index is its identity for the life of the set
 *   summary     VOF_TRACER_SUM_N doubles: COUNT, LOST, IN_LIQUID (the number with sampled F >= 0.5), ISTEP, TIME (the sum of all h
 *               advanced since the set was given, accumulated on the host in call order); unused slots read 0
 * The expression order is stated in csrc/kernels/tracers.h.  The counts come from 32-bit integer atomics, no floating-point atomics: the
 * same state and calls give the same bytes.
 *   vof_tracers_set      replaces the handle's set and zeroes TIME; n = 0 clears it.  The positions are checked on the host: one that is
 *                        not finite or lies outside the closed domain returns VOF_EINVAL and the old set stays; so do n < 0,
 *                        n > 2^31 - 1 and xy == NULL with n > 0
 *   vof_tracers_advance  one advance of every tracer by `time` on the current u, v.  Enqueues only.  A non-finite time: VOF_EINVAL;
 *                        an empty set: VOF_OK, nothing is launched
 *   vof_tracers_get      samples U, V, F, forms the summary, synchronises and copies out.  At most cap_rows rows are written and nothing
 *                        behind min(COUNT, cap_rows) rows is touched; the summary always describes ALL tracers, so rows = NULL with
 *                        cap_rows = 0 reads the counts alone
 *   vof_step_tracers     for r = 0 .. nsteps / every - 1: `every` steps -- exactly vof_step(h, every) if mg_cycles == 0, exactly
 *                        vof_step_mg(h, every, mg_cycles, criterion, NULL, NULL, NULL) if mg_cycles >= 1 --, then one advance by
 *                        (double)every * dt, then, if snap_every >= 1 and (r + 1) % snap_every == 0, a snapshot of all rows recorded on
 *                        the device (COUNT x VOF_TRACER_N doubles).  A remainder of nsteps % every steps is stepped without an advance
 *                        (TIME shows the lag).  Nothing waits for the device before the end of the call; then one copy writes the
 *                        snapshots to snaps and *snaps_written (may be NULL) is set.  snap_every = 0 records nothing and snaps may be
 *                        NULL.  every < 1, nsteps < 0, snap_every < 0, cap_snaps below the snapshots due, snaps == NULL with one due,
 *                        mg_cycles < 0, a bad criterion with mg_cycles >= 1: VOF_EINVAL, the handle and the tracers untouched
 * Whole-domain handles only (a strip returns VOF_ESTATE and is left untouched); VOF_ESTATE too while a phased step is in progress.  No
 * field, istep, counter or cached graph changes because of tracers: a vof_step / vof_step_mg / vof_step_diag that follows gives the bits it
 * would have given without them.  vof_set_init_F and vof_set_field leave the set alone; vof_destroy releases it. */
#define VOF_TRACER_X 0
#define VOF_TRACER_Y 1
#define VOF_TRACER_U 2
#define VOF_TRACER_V 3
#define VOF_TRACER_F 4
#define VOF_TRACER_N 8
#define VOF_TRACER_SUM_COUNT 0
#define VOF_TRACER_SUM_LOST 1
#define VOF_TRACER_SUM_IN_LIQUID 2
#define VOF_TRACER_SUM_ISTEP 3
#define VOF_TRACER_SUM_TIME 4
#define VOF_TRACER_SUM_N 8
int vof_tracers_set(vof2d_handle h, const double* xy /* n x 2 */, int64_t n);
int vof_tracers_advance(vof2d_handle h, double time);
int vof_tracers_get(vof2d_handle h, double* rows, int64_t cap_rows, double* summary /* VOF_TRACER_SUM_N */);
int vof_step_tracers(vof2d_handle h, int64_t nsteps, int64_t every, int32_t mg_cycles, int32_t criterion,
                     int64_t snap_every, double* snaps, int64_t cap_snaps, int64_t* snaps_written);
/* Extension: the free-surface profile.  Both marginals of F, the top of the liquid over every row and the front on the floor, from one
 * pass over F on the device instead of copying F to the host.  Cells: the handle's owned interior cells, i in [max(own_lo, 1),
 * min(own_hi, nx)] -- `rows` of them, r = i - the first --, j in [1, ny]; every F is converted to double on load (one code path for both
 * dtypes); the values are those vof_get_field would return at that moment.
 *   depth_i[r]    the sum over j = 1 .. ny of (double)F[i,j]: times dy the liquid depth over the floor at x_i = (i - 0.5) dx (gravity is along
 *                 j: gy = -5, gx = 0 in the reference).  The raw F, not a clamp of it: a NaN is not hidden, it reaches depth_i of its own
 *                 row, depth_j of its own column and SUM, and nothing else
 *   depth_j[j-1]  the sum over the owned i, ascending, of (double)F[i,j]: times dx the liquid width at height y_j = (j - 0.5) dy.  On a
 *                 strip it is the strip's partial
 *   top[r]        the largest j in [1, ny] with F[i,j] >= 0.5, or 0 if there is none (a NaN is not a member); int32, exact.  It includes
 *                 spray and overturning: that is what "run-up" means
 *   summary       VOF_DEPTH_SUM_N doubles (unused slots read 0): ROWS, ISTEP; FRONT_LO and FRONT_HI, the smallest and the largest owned i
 *                 with F[i,1] >= 0.5 (global indices; both 0 if there is none); TOP_J the maximum of top; SUM, depth_i added in ascending
 *                 i, one row after the other -- times dx dy the liquid volume
 * The order of every sum is stated in csrc/kernels/depths.h and depends on the geometry alone; the integers come from 32-bit integer
 * atomics; no floating-point atomics: the same state gives the same bytes.  Each output may be NULL (its cap only has to be >= 0 then) and
 * is skipped; the summary always describes everything.  A non-NULL output needs cap_i >= rows, cap_j >= ny, cap_top >= rows respectively,
 * and nothing behind rows, ny, rows elements is touched.  summary == NULL, a non-NULL output whose cap is too small, a negative cap,
 * more than 2^31 - 1 cells: VOF_EINVAL, the handle untouched.  Works on strip handles: a driver concatenates depth_i and top in rank
 * order, adds the depth_j partials in rank order and takes min / max of the fronts (vof2d/gauges.py, combine).  No field, istep, counter
 * or cached graph changes, and a vof_step / vof_step_mg / vof_step_diag / vof_step_tracers that follows gives the bits it would have
 * given without the call.  Synchronises and copies out. */
#define VOF_DEPTH_SUM_ROWS 0
#define VOF_DEPTH_SUM_ISTEP 1
#define VOF_DEPTH_SUM_FRONT_LO 2  /* global row indices as doubles; 0: no liquid on the floor */
#define VOF_DEPTH_SUM_FRONT_HI 3
#define VOF_DEPTH_SUM_TOP_J 4
#define VOF_DEPTH_SUM_SUM 5
#define VOF_DEPTH_SUM_N 8
int vof_depths(vof2d_handle h, double* depth_i, int64_t cap_i, double* depth_j, int64_t cap_j,
               int32_t* top, int64_t cap_top, double* summary /* VOF_DEPTH_SUM_N */);
/* Extension: fixed sensors and their time series.  A gauge is a fixed physical position in the closed domain [0, Lx] x [0, Ly], owned by
 * the handle; what it reads is recorded on the device instead of copying F, u, v, p to the host for every sample.
 *   a row       VOF_GAUGE_N doubles: X, Y; U, V, F the bilinear samples of the tracers (the sample of vof_tracers_*, the same offsets and
 *               clamps); P, p sampled with F's offsets (0.5, 0.5) and clamps; DEPTH = depth_i[ig] * dy with ig = floor(X * dxi) + 1 clamped
 *               to [1, nx], the depth_i bits those of vof_depths on the same state and dy the double of vof_get_param; TOP = (double)top[ig].
 *               Rows come in the order the gauges were given
 *   P           carries the arbitrary constant of the pure-Neumann pressure solve and the drift of the ten sweeps: take differences
 *               against a gauge placed in the gas
 *   summary     VOF_GAUGE_SUM_N doubles (unused slots read 0): COUNT, ISTEP, RECORDS (the records vof_step_gauges has taken since the set
 *               was given)
 *   vof_gauges_set   replaces the handle's set and zeroes RECORDS; n = 0 clears it.  The positions are checked on the host exactly as
 *                    vof_tracers_set checks them, with the same errors; the old set stays on an error
 *   vof_gauges_get   settles the ghost cells, runs the vof_depths pass if any gauge exists, samples, synchronises and copies out.  At most
 *                    cap_rows rows are written and nothing behind min(COUNT, cap_rows) rows is touched
 *   vof_step_gauges  for r = 0 .. nsteps / every - 1: `every` steps -- exactly vof_step(h, every) if mg_cycles == 0, exactly
 *                    vof_step_mg(h, every, mg_cycles, criterion, NULL, NULL, NULL) if mg_cycles >= 1 --, then record r of COUNT x
 *                    VOF_GAUGE_N doubles, written on the device into a buffer the handle owns (grown before anything is enqueued): bit
 *                    for bit what vof_gauges_get yields behind the same steps.  A remainder of nsteps % every steps is stepped and gets
 *                    no record.  Nothing waits for the device before the end of the call; then one copy writes `out` and
 *                    *records_written (may be NULL) is set.  The argument errors are those of vof_step_diag (every < 1, nsteps < 0,
 *                    cap_records < nsteps / every, out == NULL with a record due, mg_cycles < 0, a bad criterion with mg_cycles >= 1);
 *                    an empty set with a record due is VOF_EINVAL too; the handle is untouched
 * Whole-domain handles only (a strip returns VOF_ESTATE and is left untouched; vof_depths works on strips); VOF_ESTATE too while a phased
 * step is in progress.  No field, istep, counter or cached graph changes because of gauges: every readable field, istep and
 * courant_violations end where a single vof_step(nsteps) leaves them.  vof_set_init_F and vof_set_field leave the set alone; vof_destroy
 * releases it. */
#define VOF_GAUGE_X 0
#define VOF_GAUGE_Y 1
#define VOF_GAUGE_U 2
#define VOF_GAUGE_V 3
#define VOF_GAUGE_F 4
#define VOF_GAUGE_P 5
#define VOF_GAUGE_DEPTH 6
#define VOF_GAUGE_TOP 7
#define VOF_GAUGE_N 8
#define VOF_GAUGE_SUM_COUNT 0
#define VOF_GAUGE_SUM_ISTEP 1
#define VOF_GAUGE_SUM_RECORDS 2
#define VOF_GAUGE_SUM_N 8
int vof_gauges_set(vof2d_handle h, const double* xy /* n x 2 */, int64_t n);
int vof_gauges_get(vof2d_handle h, double* rows, int64_t cap_rows, double* summary /* VOF_GAUGE_SUM_N */);
int vof_step_gauges(vof2d_handle h, int64_t nsteps, int64_t every, int32_t mg_cycles, int32_t criterion,
                    double* out, int64_t cap_records, int64_t* records_written);
/* Extension: a dye.  A second colour function C in the layout of F, owned by the handle and carried by the same transport as F: where the
 * liquid of a drop ends up, how much of one body reaches a wall, how well two bodies have mixed.  A dye seeded equal to F stays equal to F
 * bit for bit.
 *   vof_dye_set      src: a dense (nx+2, ny+2) array of the handle's dtype, ghost cells included, stored as given (the vof_set_field
 *                    convention; no boundary pass runs).  Replaces the handle's dye; src == NULL with nbytes == 0 releases it.  A wrong
 *                    nbytes is VOF_EINVAL and the old dye stays.  The values are expected to be finite
 *   vof_dye_get      the same layout; synchronises
 *   vof_dye_advance  one transport of the dye on the u, v vof_get_field would return at that moment (ghost cells a fused step left
 *                    virtual are settled first), with the handle's istep: solve_VOF_rudman(istep) (2dvof.py:312-318) with C for F, then
 *                    post_process_f (:452-455), then the F lines of set_BC (:168, 174, 181, 187) on C.  Enqueues only
 *   vof_dye_stats    one row of VOF_DYE_N doubles (unused slots read 0) reduced over the interior cells, every operand converted to
 *                    double: ISTEP, CELLS; SUM_C; SUM_CI, SUM_CJ (sum C * i, sum C * j, global integer indices as in vof_diagnostics);
 *                    SUM_C2; SUM_CF = sum C * Fc with the plain clamp Fc of vof_diagnostics; SUM_CU, SUM_CV = sum C * uc, sum C * vc with
 *                    uc, vc of interp_velocity in the expressions of vof_diagnostics; MIN_C, MAX_C; MAX_EXCESS = max(C - F).  A NaN operand
 *                    of a maximum counts as +inf (MIN_C: -inf); the sums propagate it.  The order of the sums is fixed (kernels/dye.h,
 *                    kernels/reduce.h): the same state gives the same bits
 *   vof_step_dye     nsteps times: one step -- exactly vof_step(h, 1) if mg_cycles == 0, exactly vof_step_mg(h, 1, mg_cycles, criterion,
 *                    NULL, NULL, NULL) if mg_cycles >= 1 --, then one vof_dye_advance; behind every `every`-th step row r of VOF_DYE_N
 *                    doubles is recorded on the device, bit for bit what vof_dye_stats yields behind the same steps.  every == 0 records
 *                    nothing (out may be NULL).  Nothing waits for the device before the end of the call; then one copy writes `out` and
 *                    *rows_written (may be NULL) is set.  The steps replay the handle's captured step graphs (VOF_FLAG_NO_GRAPH: eager
 *                    launches, the same bits); the dye needs u, v of every step in memory, so the batch graphs of vof_step are not
 *                    used.  The argument errors are those of vof_step_diag (every < 0 here, nsteps < 0, cap_rows < nsteps / every, out ==
 *                    NULL with a row due, mg_cycles < 0, a bad criterion with mg_cycles >= 1); the handle is untouched
 * Without a dye, advance, get, stats and step_dye return VOF_ESTATE.  Whole-domain handles only (a strip returns VOF_ESTATE and is left
 * untouched); VOF_ESTATE too while a phased step is in progress.  The dye never changes F, u, v, p, istep, a counter or a cached graph;
 * its sweeps count no Courant violations; every readable field, istep and courant_violations end where a single vof_step(nsteps) /
 * vof_step_mg(nsteps, ...) leaves them, and a step verb that follows gives the bits it would have given without the dye and leaves the dye
 * where it was.  vof_set_init_F and vof_set_field leave the dye alone; vof_destroy releases it.  Knob "dye_fused" (vof_set_param; default
 * 1): 0 runs the advance as the two sweep kernels and the post kernel instead of the one-pass k_dye -- the same bits. */
#define VOF_DYE_ISTEP 0
#define VOF_DYE_CELLS 1
#define VOF_DYE_SUM_C 2
#define VOF_DYE_SUM_CI 3
#define VOF_DYE_SUM_CJ 4
#define VOF_DYE_SUM_C2 5
#define VOF_DYE_SUM_CF 6
#define VOF_DYE_SUM_CU 7
#define VOF_DYE_SUM_CV 8
#define VOF_DYE_MIN_C 9
#define VOF_DYE_MAX_C 10
#define VOF_DYE_MAX_EXCESS 11
#define VOF_DYE_N 16
int vof_dye_set(vof2d_handle h, const void* src, size_t nbytes);
int vof_dye_get(vof2d_handle h, void* dst, size_t nbytes);
int vof_dye_advance(vof2d_handle h);
int vof_dye_stats(vof2d_handle h, double* out /* VOF_DYE_N */);
int vof_step_dye(vof2d_handle h, int64_t nsteps, int64_t every, int32_t mg_cycles, int32_t criterion,
                 double* out, int64_t cap_rows, int64_t* rows_written);
/* Extension: pictures.  One quantity box-averaged over bx x by cells per pixel, mapped through a 256-entry colour table to 8-bit RGB, the
 * interface marked on top, all on the device: pw x ph x 3 bytes leave it instead of whole fields (0.8 MB for a 512^2 picture of any grid).
 * The values are those vof_get_field would return at that moment (the ghost cells are settled first); every operand is converted to double
 * on load (one code path for both dtypes) and every product, sum, difference, quotient and root below is rounded on its own, in the
 * FMA-contracted build too.
 *   geometry    pw = ceil(nx / bx), ph = ceil(ny / by).  Pixel (a, b) covers the cells i in [a bx + 1, min((a+1) bx, nx)], j in [b by + 1,
 *               min((b+1) by, ny)]: cnt cells, fewer in the last pixel row and column.  rgb is dense (ph, pw, 3): image row r is pixel row
 *               b = ph - 1 - r (the top of the domain is the top of the picture), image column c is a -- the orientation of
 *               vis.colour_image.  means is dense (pw, ph), indexed [a, b] like a field
 *   cell value  F: F[i,j], raw.  P: p[i,j].  DYE: C[i,j] (without a dye: VOF_ESTATE).  U: uc = (u[i,j] + u[i+1,j]) * 0.5.  V: vc = (v[i,j] +
 *               v[i,j+1]) * 0.5 (the expressions of vof_diagnostics).  SPEED: sqrt(uc * uc + vc * vc).  VORT: (vc(i+1,j) - vc(i-1,j)) * hx -
 *               (uc(i,j+1) - uc(i,j-1)) * hy with hx = 0.5 * dxi, hy = 0.5 * dyi of the doubles of vof_get_param and vc(.), uc(.) the
 *               expressions above at the neighbouring cell -- at the walls a ghost cell
 *   mean        for every column j of the pixel c_j = 0.0; c_j += q[i,j] for i ascending; then S = 0.0; S += c_j for j ascending; then
 *               m = S / (double)cnt.  The order depends on the geometry alone.  A NaN cell makes exactly its own pixel NaN
 *   range       hi > lo: the fixed range.  lo == hi: auto, lo the minimum and hi the maximum of the non-NaN means (by integer atomics on an
 *               order-preserving key of the double, under which -0.0 lies below +0.0: no order of arrival matters); with
 *               VOF_FRAME_SYMMETRIC the auto range becomes [-A, A], A = max(|lo|, |hi|) (on a fixed range the flag is ignored); no non-NaN
 *               pixel gives lo = hi = 0
 *   colour      t = (m - lo) / (hi - lo); idx = 0 if t <= 0 or hi == lo (or t is NaN: an infinite mean over an infinite range), 255 if
 *               t >= 1, (int)(t * 255.0 + 0.5) otherwise, truncating; the pixel is lut[idx]
 *   contour     with VOF_FRAME_CONTOUR the pass also forms the means mF of F (for quantity F the same array); s(a,b) = (mF(a,b) >= 0.5), a NaN
 *               gives false; pixel (a,b) takes lut[256] if s(a,b) != s(a+1,b) with a + 1 < pw or s(a,b) != s(a,b+1) with b + 1 < ph
 *   NaN         a pixel whose own mean m is NaN takes lut[257], whatever else holds
 *   table       VOF_FRAME_LUT_ROWS x 3 bytes owned by the handle: entries 0..255 the map, 256 the contour colour, 257 the NaN colour.
 *               vof_frame_set_lut copies it in (synchronises); NULL restores the default, the grey ramp (k,k,k), contour (0,0,0), NaN
 *               (255,0,255).  The table is data: the library knows no colour map (vof2d/frames.py samples matplotlib's into it)
 *   summary     VOF_FRAME_SUM_N doubles (unused slots read 0): PW, PH, ISTEP; LO, HI, the range used; NAN_PIXELS; CONTOUR_PIXELS, the
 *               pixels that took lut[256]
 *   vof_frame        rgb and means may each be NULL and are then skipped (the cap only has to be >= 0); the summary always describes the
 *                    whole frame.  A non-NULL rgb needs cap_bytes >= pw ph 3, a non-NULL means cap_means >= pw ph; nothing behind that
 *                    is touched.  The results go through one pinned host buffer: one copy, one wait
 *   vof_step_frames  for r = 0 .. nsteps / every - 1: `every` steps -- exactly vof_step(h, every) if mg_cycles == 0, exactly
 *                    vof_step_mg(h, every, mg_cycles, criterion, NULL, NULL, NULL) if mg_cycles >= 1 --, then frame r: pw ph 3 bytes and
 *                    VOF_FRAME_SUM_N doubles, written on the device into buffers the handle owns (grown before anything is enqueued),
 *                    byte for byte what vof_frame yields behind the same steps.  A remainder of nsteps % every steps is stepped and gets
 *                    no frame.  Nothing waits for the device before the end of the call; then one copy each writes out_rgb and
 *                    out_summaries, and *frames_written (may be NULL) is set.  The argument errors are those of vof_step_gauges (every < 1,
 *                    nsteps < 0, cap_frames < nsteps / every, out_rgb or out_summaries NULL with a frame due, mg_cycles < 0, a bad
 *                    criterion with mg_cycles >= 1)
 * VOF_EINVAL too, the handle and the outputs untouched: spec == NULL, a quantity or a flag outside the lists, bx < 1 or by < 1, hi < lo or a
 * NaN or infinite lo / hi, summary == NULL, a negative cap or one too small for a non-NULL output, pw ph 3 > 2^31 - 1.  Whole-domain handles
 * only (a strip returns VOF_ESTATE and is left untouched); VOF_ESTATE too while a phased step is in progress.  No field, istep, counter or
 * cached graph changes; every readable field, istep and courant_violations end where vof_step(nsteps) / vof_step_mg(nsteps, ...) alone
 * leaves them, and a step verb that follows gives the bits it would have given without the call.  The order of every sum is stated in
 * csrc/kernels/frames.h; no floating-point atomics: the same state gives the same bytes.  vof_destroy releases the table and the buffers. */
#define VOF_FRAME_F 0
#define VOF_FRAME_U 1
#define VOF_FRAME_V 2
#define VOF_FRAME_SPEED 3
#define VOF_FRAME_P 4
#define VOF_FRAME_VORT 5
#define VOF_FRAME_DYE 6
#define VOF_FRAME_CONTOUR 1
#define VOF_FRAME_SYMMETRIC 2
#define VOF_FRAME_LUT_ROWS 258
#define VOF_FRAME_SUM_PW 0
#define VOF_FRAME_SUM_PH 1
#define VOF_FRAME_SUM_ISTEP 2
#define VOF_FRAME_SUM_LO 3
#define VOF_FRAME_SUM_HI 4
#define VOF_FRAME_SUM_NAN_PIXELS 5
#define VOF_FRAME_SUM_CONTOUR_PIXELS 6
#define VOF_FRAME_SUM_N 8
typedef struct vof2d_frame_spec {
  int32_t quantity;   /* VOF_FRAME_F, _U, _V, _SPEED, _P, _VORT, _DYE */
  int32_t bx, by;     /* cells per pixel along i and along j, >= 1 */
  int32_t flags;      /* VOF_FRAME_CONTOUR | VOF_FRAME_SYMMETRIC */
  double  lo, hi;     /* hi > lo: the fixed range; lo == hi: the range is taken from the picture (auto) */
} vof2d_frame_spec;
int vof_frame_set_lut(vof2d_handle h, const uint8_t* lut /* VOF_FRAME_LUT_ROWS x 3, or NULL */);
int vof_frame(vof2d_handle h, const vof2d_frame_spec* spec, uint8_t* rgb, int64_t cap_bytes, double* means, int64_t cap_means,
              double* summary /* VOF_FRAME_SUM_N */);
int vof_step_frames(vof2d_handle h, int64_t nsteps, int64_t every, int32_t mg_cycles, int32_t criterion,
                    const vof2d_frame_spec* spec, uint8_t* out_rgb, double* out_summaries, int64_t cap_frames, int64_t* frames_written);
/* Extension: statistics over a run.  Per interior cell (i in [1, nx], j in [1, ny]) the handle keeps running sums of F, u, v and their
 * products, the envelopes of F and of the speed, the number of samples the cell was wet in and the step the front first arrived at: the
 * time-mean, the variance and the Reynolds stress of a sloshing flow, a flood or arrival map -- without a field leaving the device between
 * the samples.  The accumulators are planes of doubles for both dtypes, in two groups chosen by a mask:
 *   VOF_STATS_MOMENTS   SUM_F, SUM_F2, SUM_U, SUM_V, SUM_UU, SUM_VV, SUM_UV, SUM_FU, SUM_FV
 *   VOF_STATS_ENVELOPE  MAX_F, MAX_SPEED2, WET, ARRIVAL
 * One sample takes the fields vof_get_field would return at that moment (the ghost cells are settled first); every operand is converted to
 * double on load and every product and sum below is rounded on its own, in the FMA-contracted build too.  Per cell, in this order:
 *   f = F[i,j]   Fc = fmin(fmax(f, 0), 1)   uc = (u[i,j] + u[i+1,j]) * 0.5   vc = (v[i,j] + v[i,j+1]) * 0.5      (Fc, uc, vc of vof_diagnostics)
 *   SUM_F += Fc   SUM_F2 += Fc * Fc   SUM_U += uc   SUM_V += vc   SUM_UU += uc * uc   SUM_VV += vc * vc   SUM_UV += uc * vc
 *   SUM_FU += Fc * uc   SUM_FV += Fc * vc
 *   s2 = uc * uc + vc * vc   MAX_SPEED2 = max(MAX_SPEED2, s2)   MAX_F = max(MAX_F, Fc)     (a NaN operand counts as +inf, as in vof_diagnostics)
 *   wet = (Fc >= level)   WET += wet ? 1.0 : 0.0   if (wet && ARRIVAL < 0) ARRIVAL = (double)istep
 * The sums propagate a NaN of u or v; the plain clamp takes a NaN F to Fc = 0, a dry cell.  A cell's chain depends on the samples alone: the
 * same samples give the same bits.  Pressure is left out on purpose: p is defined up to a constant that the ten sweeps move from step to
 * step, so its time-mean means nothing (the gauges record it raw).
 *   vof_stats_begin    allocates the planes of `mask` (VOF_STATS_MOMENTS | VOF_STATS_ENVELOPE) and clears them: the sums, MAX_F, MAX_SPEED2
 *                      and WET to 0, ARRIVAL to -1, the sample count to 0.  A second call clears again.  mask == 0 releases the statistics
 *                      (level is not looked at).  A mask outside {0, 1, 2, 3}, a level that is NaN or outside (0, 1]: VOF_EINVAL, the old
 *                      statistics stay.  VOF_ENOMEM leaves the handle without statistics
 *   vof_stats_sample   one sample of the state as it is, with the handle's istep.  Enqueues only; the handle counts the samples and keeps
 *                      the istep of the first and of the last
 *   vof_stats_get      one plane, dense (nx, ny) doubles indexed [i-1, j-1]; synchronises.  cap_elems < nx ny, dst == NULL or a slot outside
 *                      [0, VOF_STATS_PLANES): VOF_EINVAL; a slot of a group that is off: VOF_ESTATE
 *   vof_stats_summary  VOF_STATS_SUM_N doubles (unused slots read 0): SAMPLES, ISTEP_FIRST, ISTEP_LAST (0 before the first sample), MASK, LEVEL,
 *                      CELLS = nx ny; EVER_WET, the cells with ARRIVAL >= 0, and MAX_SPEED2, the maximum of that plane, reduced on the device in
 *                      a fixed order without floating-point atomics -- both read 0 if the envelope is off.  Synchronises
 *   vof_step_stats     for r = 0 .. nsteps / every - 1: `every` steps -- exactly vof_step(h, every) if mg_cycles == 0, exactly
 *                      vof_step_mg(h, every, mg_cycles, criterion, NULL, NULL, NULL) if mg_cycles >= 1 --, then one vof_stats_sample.  A
 *                      remainder of nsteps % every steps is stepped and gets no sample.  Nothing waits for the device; *samples_taken (may
 *                      be NULL) is set.  The argument errors are those of vof_step_gauges (every < 1, nsteps < 0, mg_cycles < 0, a bad
 *                      criterion with mg_cycles >= 1)
 * Without statistics begun, sample, get, summary and step_stats return VOF_ESTATE.  Whole-domain handles only (a strip returns VOF_ESTATE and
 * is left untouched); VOF_ESTATE too while a phased step is in progress.  No field, istep, counter or cached graph changes; every readable
 * field, istep and courant_violations end where vof_step(nsteps) / vof_step_mg(nsteps, ...) alone leaves them, and a step verb that follows
 * gives the bits it would have given without the call.  Because vof_stats_sample only enqueues, it may be called between any other stepping
 * verbs (vof_step_diag, vof_step_dye, vof_step_frames, ...).  vof_set_init_F, vof_set_field and the dye leave the statistics alone;
 * vof_destroy releases them.  A refused call leaves the handle and the outputs untouched.  Knob "stats_chunk_rows"
 * (vof_set_param; default 0: the rule of vof_diagnostics) sets the rows a wave of the pass marches -- the same bits. */
#define VOF_STATS_MOMENTS 1
#define VOF_STATS_ENVELOPE 2
#define VOF_STATS_SUM_F 0
#define VOF_STATS_SUM_F2 1
#define VOF_STATS_SUM_U 2
#define VOF_STATS_SUM_V 3
#define VOF_STATS_SUM_UU 4
#define VOF_STATS_SUM_VV 5
#define VOF_STATS_SUM_UV 6
#define VOF_STATS_SUM_FU 7
#define VOF_STATS_SUM_FV 8
#define VOF_STATS_MAX_F 9
#define VOF_STATS_MAX_SPEED2 10
#define VOF_STATS_WET 11
#define VOF_STATS_ARRIVAL 12
#define VOF_STATS_PLANES 13
#define VOF_STATS_SUM_SAMPLES 0
#define VOF_STATS_SUM_ISTEP_FIRST 1
#define VOF_STATS_SUM_ISTEP_LAST 2
#define VOF_STATS_SUM_MASK 3
#define VOF_STATS_SUM_LEVEL 4
#define VOF_STATS_SUM_CELLS 5
#define VOF_STATS_SUM_EVER_WET 6
#define VOF_STATS_SUM_MAX_SPEED2 7
#define VOF_STATS_SUM_N 16
int vof_stats_begin(vof2d_handle h, int32_t mask, double level);
int vof_stats_sample(vof2d_handle h);
int vof_stats_get(vof2d_handle h, int32_t slot, double* dst, int64_t cap_elems);
int vof_stats_summary(vof2d_handle h, double* out /* VOF_STATS_SUM_N */);
int vof_step_stats(vof2d_handle h, int64_t nsteps, int64_t every, int32_t mg_cycles, int32_t criterion, int64_t* samples_taken);

/* ---- an initial state painted from shapes (extension; kernels/scene.h) ----
 * vof_set_scene rasterises an ordered list of shapes into F on the device, with samples x samples sample points a cell.  It is the
 * input side next to vof_set_init_F: any state that is a union and difference of boxes, ellipses, half-planes and triangles, on a
 * whole domain and on a strip alike (every handle paints the rows it stores from the same list), without an array on the host.
 *   geometry    in doubles whatever the field type.  Cell (i, j) covers [(i-1) dx, i dx] x [(j-1) dy, j dy], dx and dy the doubles
 *               vof_get_param reports; a ghost cell is a cell like any other, outside the domain
 *   samples     S in {1, 2, 4, 8, 16}; sample (a, b), a, b in [0, S), of cell (i, j) sits at
 *                 xs = ((double)(i-1) + ((double)a + 0.5) * (1.0/S)) * dx,   ys = ((double)(j-1) + ((double)b + 0.5) * (1.0/S)) * dy
 *               (the bracket is exact: one rounding per coordinate)
 *   a shape     VOF_SHAPE_N doubles: KIND, PHASE (VOF_SCENE_LIQUID or VOF_SCENE_GAS), A0 .. A5.  Every difference, product and sum
 *               below is rounded on its own, in the order written (no fused multiply-add in either build); all tests are closed, so
 *               two shapes that share an edge leave no seam; a comparison with a NaN (an overflow) is false
 *     VOF_SHAPE_BOX        cx, cy, hx, hy, c, s:  px = xs - cx, py = ys - cy, lx = px*c + py*s, ly = py*c - px*s;
 *                          inside if |lx| <= hx and |ly| <= hy.  c, s: the cosine and sine of the rotation, given by the caller
 *     VOF_SHAPE_ELLIPSE    the same fields and lx, ly; inside if (lx*hy)*(lx*hy) + (ly*hx)*(ly*hx) <= (hx*hy)*(hx*hy)
 *     VOF_SHAPE_HALFPLANE  px0, py0, nx, ny (A4, A5 are not used):  inside if (xs - px0)*nx + (ys - py0)*ny <= 0
 *     VOF_SHAPE_TRIANGLE   x0, y0, x1, y1, x2, y2:  e0 = (x1-x0)*(ys-y0) - (y1-y0)*(xs-x0), e1 = (x2-x1)*(ys-y1) - (y2-y1)*(xs-x1),
 *                          e2 = (x0-x2)*(ys-y2) - (y0-y2)*(xs-x2); inside if all three are >= 0 or all three are <= 0
 *   painting    every sample starts as KEEP; the shapes are applied in list order, a sample inside a shape takes its phase: a later
 *               shape overrides an earlier one
 *   the value   n_liq, n_keep: the cell's samples that ended LIQUID, KEEP.  n_keep == S*S: the cell is not written, its bits stay
 *               (a NaN, a -0.0).  Otherwise F = ((double)n_liq + (double)n_keep * (double)F_old) * (1.0/(S*S)), rounded once to the
 *               field type; where n_keep == 0 F_old is not read (a NaN there does not leak).  With VOF_SCENE_CLEAR a KEEP sample counts
 *               as GAS: F_old is never read and every stored cell is written, F = n_liq / (S*S)
 *   written     F and its sweep twin, on every stored row and every column 0 .. ny + 1; u, v, p are not touched
 *   summary     VOF_SCENE_SUM_N doubles (may be NULL; unused slots read 0): SHAPES = n, SAMPLES = S, PAINTED = the cells with
 *               n_keep < S*S, MIXED = the cells whose samples are not all in one state (with VOF_SCENE_CLEAR: after KEEP became GAS),
 *               ISTEP.  Both counts are over the interior cells of the rows the handle reports (vof_diagnostics): strips add up
 * VOF_EINVAL, with nothing changed: a null handle; n < 0 or n > VOF_SCENE_MAX_SHAPES; shapes == NULL with n > 0; samples outside
 * {1, 2, 4, 8, 16}; a flag bit outside VOF_SCENE_CLEAR; an unknown KIND or PHASE; a number in a record that is not finite; a
 * negative half extent; |c*c + s*s - 1| > 1e-9; a half-plane with nx == ny == 0.  n == 0 is valid: the identity without
 * VOF_SCENE_CLEAR (nothing at all happens), an empty domain with it.
 * The handle's state is treated as vof_set_init_F treats it: pending ghost cells are settled first; afterwards F counts as written
 * from outside (its ghost cells are whatever the shapes gave them: the first step applies the boundary conditions).  The call waits
 * for the device (the counts are read back).  Knob "scene_shortcuts" (vof_set_param; default 1): 0 samples every cell against
 * every shape, 1 skips the sampling where the corner samples prove all samples inside or all outside -- the same bytes. */
#define VOF_SHAPE_N 8
#define VOF_SHAPE_KIND 0
#define VOF_SHAPE_PHASE 1
#define VOF_SHAPE_A0 2
#define VOF_SHAPE_BOX 0
#define VOF_SHAPE_ELLIPSE 1
#define VOF_SHAPE_HALFPLANE 2
#define VOF_SHAPE_TRIANGLE 3
#define VOF_SCENE_GAS 0
#define VOF_SCENE_LIQUID 1
#define VOF_SCENE_CLEAR 1
#define VOF_SCENE_MAX_SHAPES 1024
#define VOF_SCENE_SUM_SHAPES 0
#define VOF_SCENE_SUM_SAMPLES 1
#define VOF_SCENE_SUM_PAINTED 2
#define VOF_SCENE_SUM_MIXED 3
#define VOF_SCENE_SUM_ISTEP 4
#define VOF_SCENE_SUM_N 8
int vof_set_scene(vof2d_handle h, const double* shapes /* n x VOF_SHAPE_N */, int64_t n, int32_t samples, int32_t flags,
                  double* summary /* VOF_SCENE_SUM_N, may be NULL */);
/* = vof_solve_p(..., VOF_RESID_ABS, ...) */
int vof_solve_p_residual(vof2d_handle h, double tol, int32_t max_iters, int32_t check_every,
                         int32_t* iters_done, double* residual);
/* rhs build (if build_rhs) + n sweeps; *max_update = max|p_new - p| and *max_p = max|p_new| of the
 * last sweep over this handle's owned rows (a NaN entry counts as +inf). */
int vof_jacobi_sweeps_norms(vof2d_handle h, int32_t n, int32_t build_rhs, double* max_update, double* max_p);
/* the max_update half of vof_jacobi_sweeps_norms */
int vof_jacobi_sweeps_residual(vof2d_handle h, int32_t n, int32_t build_rhs, double* residual);
/* the residual of a criterion from the two (possibly all-reduced) norms; +inf for a non-finite update */
double vof_residual_value(double max_update, double max_p, int32_t criterion);

/* ---- fields: F.to_numpy() / F.from_numpy() (2dvof.py:44,46,535,565) ----
 * names: F u v p u_star v_star mx my kappa rho nu rhs */
int vof_get_field(vof2d_handle h, const char* name, void* dst, size_t nbytes);
int vof_set_field(vof2d_handle h, const char* name, const void* src, size_t nbytes);
/* rows [g0, g1] (global indices, inclusive) of a field, dense (g1-g0+1, ny+2) */
int vof_get_rows(vof2d_handle h, const char* name, int32_t g0, int32_t g1, void* dst, size_t nbytes);
int vof_set_rows(vof2d_handle h, const char* name, int32_t g0, int32_t g1, const void* src,
                 size_t nbytes);
/* device view for zero-copy halo exchange: element (i, j) lives at
 * base + ((i - row_lo) * pitch + col0 + j) * elem_size.  A write through the pointer is not seen by
 * the handle: after a view of "F" or "F2" the handle keeps no zero maps for k_tm (knob
 * f_zero_map has no effect on it any more), so that such a write is honoured as before. */
int vof_field_view(vof2d_handle h, const char* name, void** base, int64_t* pitch, int64_t* col0,
                   int64_t* nrows);
/* device-to-device copy of rows [g0, g1] of `name` from src into dst (same
 * nx, ny, dtype; rows must be stored by both).  Used for single-GPU strip
 * emulation; across GPUs the exchange is RCCL send/recv on vof_field_view.
 * Asynchronous and ordered on both handles: the copy follows everything enqueued
 * on src so far, and everything enqueued on src or dst afterwards follows the copy. */
int vof_copy_rows(vof2d_handle dst, vof2d_handle src, const char* name, int32_t g0, int32_t g1);

/* ---- a state carried onto a finer or coarser grid (extension; kernels/regrid.h) ----
 * vof_regrid reads F, u, v, p of src and writes them into dst, a handle of another nx x ny (and, if it likes, another dtype, dt,
 * jacobi_iters and material constants) over the same Lx x Ly: a flow spun up on a cheap grid goes on on a fine one, a fine run is
 * coarsened to compare resolutions.  Both are whole-domain handles on one device; each keeps its dtype: every operand is converted
 * to double on load, all arithmetic is in double, a result is rounded once, on store.
 *   direction   refinement: dst.nx = rx src.nx and dst.ny = ry src.ny; coarsening: src.nx = rx dst.nx and src.ny = ry dst.ny; rx, ry
 *               integers in [1, VOF_REGRID_MAX_FACTOR]; rx = ry = 1 is a copy (a conversion between the dtypes)
 *   refining    source cell (I, J), child (k, m), is the cell i = (I-1) rx + 1 + k, j = (J-1) ry + 1 + m of dst.  u: linear along i
 *               between the faces I and I + 1 of row J, the same for every m (v likewise along j): every child has its parent's
 *               discrete divergence.  p: bilinear between the source cell centres, ghost cells included.  F: the parent's value --
 *               or, with VOF_REGRID_PLIC, in every cell vof_interface gives a segment for at this eps, the share of the child's
 *               rectangle under the cell's PLIC line, which keeps the interface one cell of dst wide and the parent's volume to
 *               a few ulp
 *   coarsening  F, p: the mean of the rx ry children; u: the mean of the ry fine faces on the coarse face, v of the rx: the coarse
 *               divergence is the mean of the fine ones
 *               (the expressions and their order: kernels/regrid.h; tests/_regrid_np.py restates them)
 *   src         is read as vof_get_field would return it now (pending ghost cells and a chained batch are settled first) and is
 *               otherwise unchanged: its next steps give the bits they would have given
 *   dst         the interior of F, its twin, u, v, p; then the launch of vof_set_BC; istep = src's.  From there dst is, in every
 *               readable field after any number of steps, what vof_set_field of the four arrays, vof_set_BC and vof_set_istep
 *               would have made it.  Row 0 of u and column 0 of v, which nothing reads, are stored as 0.  The Courant counter,
 *               tracers, gauges, the dye, the statistics planes and the colour table of dst are left alone
 *   order       asynchronous: the kernels run on dst's stream behind everything enqueued on src so far, and whatever src enqueues
 *               next follows them.  The call waits for the device only if summary != NULL
 *   summary     VOF_REGRID_SUM_N doubles (may be NULL): RX, RY, DIR (+1 refined, -1 coarsened, 0 the same grid), PLIC_CELLS = the
 *               source cells whose children came from a line, DEGENERATE = the mixed source cells without an orientation (both 0
 *               without the flag and when coarsening), F_SRC and F_DST = the sums of (double)F over the interior of src and of
 *               dst as stored, each in the fixed order of kernels/reduce.h on its own grid, ISTEP
 * VOF_EINVAL, with both handles untouched: a null handle; dst == src; different devices; Lx or Ly that differ as doubles; grids
 * refined along one axis and coarsened along the other; a ratio that is no integer or larger than VOF_REGRID_MAX_FACTOR; a flag
 * bit outside VOF_REGRID_PLIC; with VOF_REGRID_PLIC an eps outside [0, 0.5).  VOF_ESTATE: a strip on either side; a phased step
 * (vof_step_phase) in progress on either side. */
#define VOF_REGRID_PLIC 1
#define VOF_REGRID_MAX_FACTOR 16
#define VOF_REGRID_SUM_RX 0
#define VOF_REGRID_SUM_RY 1
#define VOF_REGRID_SUM_DIR 2
#define VOF_REGRID_SUM_PLIC_CELLS 3
#define VOF_REGRID_SUM_DEGENERATE 4
#define VOF_REGRID_SUM_F_SRC 5
#define VOF_REGRID_SUM_F_DST 6
#define VOF_REGRID_SUM_ISTEP 7
#define VOF_REGRID_SUM_N 8
int vof_regrid(vof2d_handle dst, vof2d_handle src, int32_t flags, double eps, double* summary /* VOF_REGRID_SUM_N, may be NULL */);

/* ---- display fields (2dvof.py:458-492; full-domain handles only) ----
 * which: "vof" get_vof_field :458-462, "u" get_u_field :465-470, "v" get_v_field :473-478,
 * "vnorm" get_vnorm_field :481-486.  dst: the rgb_buf image, dense (2*nx, 2*ny) of the field dtype. */
int vof_get_vis_field(vof2d_handle h, const char* which, void* dst, size_t nbytes);
/* interp_velocity :488-492: cell-centred velocity V, dense (nx+2, ny+2, 2) of the field dtype. */
int vof_interp_velocity(vof2d_handle h, void* dst, size_t nbytes);

/* ---- scalars ---- */
/* settable: sigma (sigma[None], :28-29).  readable: sigma dt dx dy dxi dyi
 * dxi2 dyi2 Lx Ly rho_l rho_g nu_l nu_g gx gy (Python-double values).
 * Schedule knobs (settable, results never change): jacobi_tb (sweeps fused per launch: 5, 2 or 1),
 * jacobi_tb_adapt (the equal-cost work plan of the fused Jacobi launches), jacobi_tb_general (the
 * general-stencil form on square cells too), chunk lengths jacobi_tb_rows, momentum_rows, fctx_rows,
 * fctx_corr_rows, band_rows, rows_per_wave (rows a wave marches; 0 = heuristic), fuse_transport
 * (update_uv + both sweeps as one kernel on full domains; readable: 1 if in effect), virtual_ghosts
 * (no set_BC launch in steady-state steps).  Environment: VOF2D_DEBUG (trace to stderr), VOF2D_RCCL
 * (path of the RCCL to bind), VOF2D_XCHG_GRAPH=0 (never capture the exchange). */
int vof_set_param(vof2d_handle h, const char* name, double value);
int vof_get_param(vof2d_handle h, const char* name, double* value);
/* "courant_violations": number of faces that tripped the prints at
 * 2dvof.py:274-275,279-280 since creation (owned rows only). */
int vof_get_counter(vof2d_handle h, const char* name, int64_t* value);

/* ---- sync / timing / errors ---- */
int vof_sync(vof2d_handle h);
/* hipEvent pair on the handle's stream */
int vof_timer_start(vof2d_handle h);
int vof_timer_stop(vof2d_handle h, float* ms); /* records, synchronises, returns elapsed */
/* Built-in in-situ profiler: nsteps steps of the fused schedule with a start/stop event pair on
 * every dispatch (hipExtLaunchKernelGGL); per-kernel sums accumulate until vof_reset_profile.
 * kernel names: k_momentum k_set_bc k_jacobi k_jacobi_tb k_correct k_fct_x k_fct_y (+ k_normals
 * k_kappa k_predictor k_rhs when the momentum fusion is off).  The state advances by nsteps. */
int vof_profile_steps(vof2d_handle h, int64_t nsteps);
int vof_get_profile(vof2d_handle h, const char* kernel, double* avg_us, int64_t* launches);
int vof_reset_profile(vof2d_handle h);
/* n (even) Jacobi sweeps of the current rhs, back to back, between one hipEvent pair on the
 * handle's stream; *ms_per_sweep = elapsed / n.  p advances by n sweeps.  Uses the kernels the
 * step uses (k_jacobi_tb launches of `jacobi_tb` sweeps, k_jacobi when that parameter is 1). */
int vof_time_jacobi(vof2d_handle h, int32_t n, float* ms_per_sweep);
/* ---- strips over RCCL (extension: the reference is single-device) ----
 * A handle that stores a row strip (row_lo..row_hi with VOF_HALO_ROWS halo rows on each interior
 * side of own_lo..own_hi) can run the per-step halo exchange itself: rank r of `world` owns the
 * r-th strip counted from the left wall and trades W = VOF_HALO_ROWS(jacobi_iters) rows of F, u,
 * v, p with ranks r-1 and r+1 by ncclSend / ncclRecv, straight from / to field memory, on a
 * communication stream of its own.  RCCL is bound at run time (librccl.so.1; a copy already in the
 * process, e.g. PyTorch's, is reused), so single-GPU users need no RCCL.
 *   vof_comm_get_unique_id  on one rank; ship the VOF_COMM_ID_BYTES to the others (any transport)
 *   vof_comm_init           collective over all ranks (ncclCommInitRank)
 *   vof_step_exchange       nsteps x [phase 0, send/recv p, phase 1, send/recv u v, phase 2,
 *                           send/recv F, join]: each field leaves as soon as it is final for the
 *                           step and travels under the remaining kernels (overlap = 1).
 *                           overlap = 0: one exchange of all four after the step; overlap = 3: p, u,
 *                           v in one group after phase 1, F after phase 2 (one fork less); overlap = 4
 *                           (what the drivers use): update_uv and both sweeps as ONE kernel
 *                           (k_transport), first on the edge bands, then
 *                           send/recv p, u, v, F in one group, and the same kernel on the remaining
 *                           rows while they travel.  After the first step (RCCL connects on
 *                           first use) a step and its exchanges are one hipGraph launch (mode 4: two
 *                           steps per launch once both single-step graphs exist); if the
 *                           RCCL at hand cannot be captured the launches stay eager.  The host
 *                           does not block
 *   vof_comm_exchange       one exchange of the fields in field_mask, then join (for verb-level
 *                           drivers, e.g. the residual-terminated pressure solve)
 * VOF_COMM_LOOPBACK (self-test on one GPU): both neighbours are the calling rank itself. */
#define VOF_COMM_ID_BYTES 128
#define VOF_COMM_LOOPBACK 1
#define VOF_XCHG_F 1u
#define VOF_XCHG_U 2u
#define VOF_XCHG_V 4u
#define VOF_XCHG_P 8u
#define VOF_XCHG_US 16u   /* u*, v*, rhs: the exchange state of overlap mode 5 (next to F and p) */
#define VOF_XCHG_VS 32u
#define VOF_XCHG_RHS 64u
int vof_comm_get_unique_id(void* id /* VOF_COMM_ID_BYTES */);
int vof_comm_init(vof2d_handle h, const void* id, int32_t rank, int32_t world, int32_t flags);
int vof_comm_exchange(vof2d_handle h, uint32_t field_mask);
int vof_step_exchange(vof2d_handle h, int64_t nsteps, int32_t overlap);
/* overlap = 5: the strips run the kernels the single GPU runs.  The step boundary moves behind the momentum predictor:
 *   one call of n steps = k_momentum (owned rows), send/recv u*, v*, rhs
 *                         + (n - 1) x [k_jacobi_pair (ten sweeps, all stored rows), k_tm (this step's transport + the next
 *                           step's momentum) on the two edge bands beside k_tm on the other owned rows, send/recv F, u*, v*,
 *                           rhs, p in one group under the latter]
 *                         + [two k_jacobi_tb launches, k_transport on the edge bands, send/recv F, u, v, p, k_transport on
 *                           the other rows]  (the last step is mode 4's: u and v reach memory only there),
 * the middle steps two per hipGraph launch.  Halo depth: ten sweeps + 7 rows of the fused transport / momentum
 * marches <= VOF_HALO_ROWS.  vof_step_tm_piece runs the kernels of one piece WITHOUT the exchange (0: the k_momentum of
 * the first step, 1: one middle step, 2: the last step), for drivers that move the halos themselves (vof_copy_rows between
 * strip handles on one device: tests, tools/predict_strips.py). */
int vof_step_tm_piece(vof2d_handle h, int32_t piece);
/* max over all ranks of *value (ncclAllReduce on the compute stream, then a stream sync): the
 * global residual of the residual-terminated pressure solve, and a barrier for timing loops. */
int vof_comm_allreduce_max(vof2d_handle h, double* value);
/* ncclGetVersion code of the RCCL in use (0: none) and whether vof_step_exchange replays captured
 * graphs with this handle (verified from RCCL 2.27.7 on; older copies launch eagerly). */
int vof_comm_info(vof2d_handle h, int32_t* rccl_version, int32_t* graph_capture);
int vof_comm_destroy(vof2d_handle h);

/* Self-test of the kernels' exact constant-denominator division (the Jacobi update p = num / ap,
 * 2dvof.py:262-264, and the / dx, / dy, / dt, / (dx*dy) of :207-232 and :327-449 are evaluated as
 * Markstein-corrected multiplications by the reciprocal): n generated (numerator, denominator)
 * pairs -- ordinary, tiny, huge, special, and subnormal quotients on and beside the midpoints of
 * the subnormal grid -- are divided by that routine on the current device.  a_out, b_out, q_out:
 * host arrays of n elements of `dtype`; the caller checks q == a / b with the host's IEEE division
 * (tests/test_parity_gpu.py). */
int vof_selftest_division(int32_t dtype, int64_t n, uint64_t seed, void* a_out, void* b_out, void* q_out);
const char* vof_last_error(vof2d_handle h);
/* "hip-gfx950" for the product library, "cpu-oracle" for oracle/ */
const char* vof_backend(void);

#ifdef __cplusplus
}
#endif
#endif /* VOF2D_H */
