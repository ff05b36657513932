// vof2d_api.hip -- C ABI (include/vof2d.h) over the gfx950 kernels.
//
// Host-side runtime of the drop-in: owns the device arena, the HIP stream, the
// per-step launch schedule (eager or hipGraph replay) and the pitched
// host<->device copies behind to_numpy()/from_numpy().  No CPU compute path
// exists here: every verb is a kernel launch.
//
// This file holds the extern "C" entry points only: null and argument checks, the error messages, settle_ghosts, one
// call into the runtime, what the call did to the handle's state (a call into runtime/state.h).  The runtime behind them:
// They are included once, in the order of the #include lines below (each names the one before it; the diagnostic build adds
// runtime/diag.h at the end):
//   runtime/context.h    the handle (with its field views and its graph store), constants, read_back
//   runtime/buffers.h    DevBuf, the owner of a device allocation, and the handle's list of them; with runtime/carve.h, plain C++: the arenas cut into ranges
//   runtime/state.h      plain C++: what the fields and ghost cells hold (FieldState), a field written from outside, the prologue and epilogue of a step, the phase order
//   runtime/views.h      plain C++: which buffer each field id names and the four swaps that change it; the graphs captured against a view, kept by {kind, views, variant}
//   runtime/launches.h   chunk-length heuristics, one launch wrapper per kernel (tile counts from the geometry in vof2d_device.h)
//   runtime/graphs.h     what each kind of graph puts into its key, the one capture helper
//   runtime/rows.h       plain C++: the owned rows of a strip, its edge bands, the rest; what a launch of one part gets; the cells a handle reports
//   runtime/schedule.h   the per-step schedule, ghost-cell bookkeeping, dropping graphs
//   runtime/multigrid.h  the work arrays of the CG and multigrid solves, the hierarchy, one V-cycle and its graph, the driver loop of both
//   runtime/step.h       which form of the batch graphs a handle runs; a step in a batch, from its graph, eagerly; the steps of vof_step_mg
//   runtime/diag_reduce.h  the buffers and launches of vof_diagnostics, the loop of vof_step_diag
//   runtime/cell_rows.h  the buffers, launches and copies of vof_interface and vof_curvature
//   runtime/energy.h     the launch of k_energy on the reduced-row path of vof_diagnostics, the loop of vof_step_energy
//   runtime/blobs.h      the buffers, launches and copies of vof_blobs
//   runtime/tracers.h    the buffers, launches and copies of vof_tracers_*, the loop of vof_step_tracers
//   runtime/depths.h     the buffers, launches and copies of vof_depths and vof_gauges_*, the loop of vof_step_gauges
//   runtime/dye.h        the dye arrays, launches and copies of vof_dye_*, the loop of vof_step_dye
//   runtime/frames.h     the colour table, the buffers, launches and copies of vof_frame, the loop of vof_step_frames
//   runtime/stats.h      the accumulator planes, launches and copies of vof_stats_*, the loop of vof_step_stats
//   runtime/scene.h      plain C++: what vof_set_scene refuses, the packed records; the upload, the launch of k_scene, the summary
//   runtime/regrid.h     vof_regrid: the work buffer, the order on the two handles' streams, the launches, dst's state, the summary; with runtime/regrid_check.h, plain C++: the factors and what is refused
//   runtime/comm.h       strips over RCCL (bound with dlopen), the steps with their exchanges
//   runtime/selftest.h   device side of the division self-test
//   runtime/diag.h       diagnostic build only: the vof_debug_* entry points
#include "runtime/context.h"
#include "runtime/launches.h"
#include "runtime/graphs.h"
#include "runtime/schedule.h"
#include "runtime/multigrid.h"
#include "runtime/step.h"
#include "runtime/diag_reduce.h"
#include "runtime/cell_rows.h"
#include "runtime/energy.h"
#include "runtime/blobs.h"
#include "runtime/tracers.h"
#include "runtime/depths.h"
#include "runtime/dye.h"
#include "runtime/frames.h"
#include "runtime/stats.h"
#include "runtime/scene.h"
#include "runtime/regrid.h"
#include "runtime/comm.h"
#include "runtime/selftest.h"
#ifdef VOF_WAVE_TIMES
#include "runtime/diag.h"
#endif

namespace {

// schedule knobs (results never change; tools/sweep_rows.py, tools/variant_ab.py and the tests that
// force a code path use them): sweeps fused per launch, chunk lengths (0 = heuristic), the
// equal-cost work plan, the general Jacobi form on square cells, the fused full-domain schedule.
// All of them can be set; vof_get_param reads back the `readable` ones as they are (and some of the others as what the
// handle makes of them: rows_per_wave, overlap_halves, fuse_transport).
struct Knob { const char* name; int* (*at)(vof2d_ctx*); bool readable; };
#define KNOB(name, member, readable) {name, [](vof2d_ctx* h) { return &h->member; }, readable}
const Knob kKnobs[] = {
  KNOB("jacobi_tb", tb, true), KNOB("jacobi_tb_adapt", tb_adapt, true), KNOB("jacobi_tb_rows", tb_rows, false),
  KNOB("jacobi_tb_general", tb_general, false), KNOB("momentum_rows", mom_rows, false), KNOB("fctx_rows", fctx_rows, false),
  KNOB("fctx_corr_rows", fctx_corr_rows, false), KNOB("band_rows", band_rows, false), KNOB("rows_per_wave", rows_override, false),
  KNOB("fuse_transport", fuse_transport, false), KNOB("virtual_ghosts", virtual_ghosts, false), KNOB("buffer_stores", buf_stores, false),
  KNOB("overlap_halves", halves, false), KNOB("batch_steps", step_batch[0], false), KNOB("fuse_tm", fuse_tm, false),
  KNOB("tm_rows", tm_rows, false), KNOB("tm_taper", tm_taper, true), KNOB("f_zero_map", f_zero_map, true),
  KNOB("tm_tail_at1", tm_tail_at[0], false), KNOB("tm_tail_at2", tm_tail_at[1], false), KNOB("tm_tail_at3", tm_tail_at[2], false),
  KNOB("tm_tail_rows1", tm_tail_rows[0], false), KNOB("tm_tail_rows2", tm_tail_rows[1], false), KNOB("tm_tail_rows3", tm_tail_rows[2], false),
  KNOB("jacobi_pair", jpair, false), KNOB("jacobi_pair_rows", jpair_rows, false),
  KNOB("pair_slow10", pair_slow10, false), KNOB("solve_pairs", solve_pairs, false),
  KNOB("tb_slow10", tb_slow10, false), KNOB("tune_period", tune.period, false),
  KNOB("mg_nu", mg_nu, true), KNOB("mg_levels", mg_levels, true), KNOB("mg_graph", mg_graph, true),
  KNOB("mg_coarse_block", mg_coarse_block, false), KNOB("dye_fused", dye_fused, true),
  KNOB("stats_chunk_rows", stats_chunk, false), KNOB("scene_shortcuts", scene_shortcuts, true),
};
#undef KNOB
const Knob* find_knob(const char* name) {
  for (const Knob& k : kKnobs)
    if (!strcmp(name, k.name)) return &k;
  return nullptr;
}

// ---- checks several entry points share (0: go on)
int check_criterion(vof2d_ctx* h, int criterion) {
  return criterion != VOF_RESID_ABS && criterion != VOF_RESID_REL ? fail(h, VOF_EINVAL, "criterion must be VOF_RESID_ABS or VOF_RESID_REL") : VOF_OK;
}
int check_whole_domain(vof2d_ctx* h, const char* why_not_a_strip) {   // (the message names the entry point and the reason)
  return h->d.row_lo != 0 || h->d.row_hi != h->d.nx + 1 ? fail(h, VOF_ESTATE, why_not_a_strip) : VOF_OK;
}
int check_no_phased_step(vof2d_ctx* h) {
  return phased_step_in_progress(h->state) ? fail(h, VOF_ESTATE, "a phased step (vof_step_phase) is in progress") : VOF_OK;
}
// ... of the verbs that need the whole domain in one handle and no phased step under way (the message names them and the reason);
// lacks: the message where the handle lacks what the verb works on (a dye, statistics), else NULL
int check_verb_allowed(vof2d_ctx* h, const char* why_not_a_strip, const char* lacks = nullptr) {
  if (const int rc = check_whole_domain(h, why_not_a_strip)) return rc;
  if (const int rc = check_no_phased_step(h)) return rc;
  return lacks ? fail(h, VOF_ESTATE, lacks) : VOF_OK;
}
// What every vof_step_<verb> checks first, in this order: the handle, every (the verb's minimum and its message), nsteps, `between`
// (the message of a failed check of the verb's own that stands here, else NULL), mg_cycles, the criterion where it is used
int check_step_args(vof2d_ctx* h, int64_t nsteps, int64_t every, int mg_cycles, int criterion, const char* between = nullptr, int64_t min_every = 1,
                    const char* every_msg = "every must be >= 1") {
  if (!h) return VOF_EINVAL;
  if (every < min_every) return fail(h, VOF_EINVAL, every_msg);
  if (nsteps < 0) return fail(h, VOF_EINVAL, "nsteps must be >= 0");
  if (between) return fail(h, VOF_EINVAL, between);
  if (mg_cycles < 0) return fail(h, VOF_EINVAL, "mg_cycles must be >= 0 (0: the steps of vof_step)");
  return mg_cycles >= 1 ? check_criterion(h, criterion) : VOF_OK;
}
// ... and last: a call of no steps does nothing but report that it recorded nothing
bool no_steps(int64_t nsteps, int64_t* written) {
  if (nsteps == 0 && written) *written = 0;
  return nsteps == 0;
}
bool full_domain(const vof2d_ctx* h) { return h->g.wall_lo && h->g.wall_hi; }

}  // namespace

// =============================================================== C ABI
extern "C" {

int vof_desc_default(vof2d_desc* d, int32_t nx, int32_t ny, int32_t dtype) {
  if (!d || nx < 3 || ny < 3 || (dtype != VOF_F64 && dtype != VOF_F32)) return VOF_EINVAL;
  memset(d, 0, sizeof(*d));
  d->abi_version = VOF_ABI_VERSION;
  d->nx = nx; d->ny = ny; d->dtype = dtype; d->coord_cast_f32 = 1;
  d->row_lo = 0; d->row_hi = nx + 1; d->own_lo = 1; d->own_hi = nx;
  d->jacobi_iters = 10; d->device = -1; d->flags = 0;
  // 2dvof.py:22-33
  d->Lx = 0.1; d->Ly = 0.1; d->rho_l = 1000.0; d->rho_g = 50.0; d->nu_l = 1.0e-6; d->nu_g = 1.5e-5;
  d->sigma = 0.007; d->gx = 0; d->gy = -5; d->dt = 4e-6;
  return VOF_OK;
}

int vof_create(const vof2d_desc* d, void* stream, vof2d_handle* out) {
  if (!d || !out || d->abi_version != VOF_ABI_VERSION) return VOF_EINVAL;
  if (d->nx < 3 || d->ny < 3 || d->row_lo < 0 || d->row_hi > d->nx + 1 || d->row_hi - d->row_lo < 2) return VOF_EINVAL;
  if (d->dtype != VOF_F64 && d->dtype != VOF_F32) return VOF_EINVAL;
  if (d->jacobi_iters < 0) return VOF_EINVAL;
  vof2d_ctx* h = new (std::nothrow) vof2d_ctx();
  if (!h) return VOF_ENOMEM;
  h->err[0] = 0;
  h->d = *d;
  compute_consts(*d, h->cd);
  if (!(d->dtype == VOF_F64 ? divisors_ok<double>(h->cd) : divisors_ok<float>(h->cd))) {
    delete h;
    return VOF_EINVAL;  // a grid/time-step constant with an all-ones significand (see divisors_ok)
  }
  h->esz = d->dtype == VOF_F64 ? 8 : 4;
  h->V = d->dtype == VOF_F64 ? VecWidth<double>::V : VecWidth<float>::V;
  const int W = 64 * h->V;
  Geom& g = h->g;
  g.nx = d->nx; g.ny = d->ny; g.row_lo = d->row_lo; g.row_hi = d->row_hi;
  g.ilo = d->row_lo + 1 > 1 ? d->row_lo + 1 : 1;
  g.ihi = d->row_hi - 1 < d->nx ? d->row_hi - 1 : d->nx;
  g.own_lo = d->own_lo; g.own_hi = d->own_hi;
  g.wall_lo = d->row_lo == 0; g.wall_hi = d->row_hi == d->nx + 1;
  g.ntj = (d->ny + W - 1) / W;
  h->nty = d->dtype == VOF_F64 ? TransportGeom<VecWidth<double>::V>::tiles(d->ny) : TransportGeom<VecWidth<float>::V>::tiles(d->ny);
  const int align = 128 / (int)h->esz;  // elements per 128 bytes
  g.col0 = align - 1;                   // j = 1 lands on a 128-byte boundary
  // furthest column any lane touches: the overlapped tiles of k_fct_y / k_jacobi_tb start at most
  // H <= 12 columns left of j = 1 and their last tile may run a full tile past ny.
  const long maxcol = (long)d->ny + W + 16;
  g.pitch = ((g.col0 + maxcol + 1 + align - 1) / align) * align;
  const size_t nrows = (size_t)(d->row_hi - d->row_lo + 1);
  h->field_elems = nrows * (size_t)g.pitch + (size_t)align;  // + one 128-byte tail pad
  int rc = VOF_OK;
  do {
    if (d->device >= 0) {
      if (hipSetDevice(d->device) != hipSuccess) { rc = VOF_EHIP; break; }
    }
    if (hipGetDevice(&h->device) != hipSuccess) { rc = VOF_EHIP; break; }
    if (stream) {
      h->stream = reinterpret_cast<hipStream_t>(stream);
    } else {
      if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { rc = VOF_EHIP; break; }
      h->own_stream = true;
    }
    if (const char* ev = getenv("VOF2D_OVERLAP_HALVES")) h->halves = atoi(ev);   // (profiling runs: per-kernel counters want one kernel at a time)
    if (const char* ev = getenv("VOF2D_FUSE_TM")) h->fuse_tm = atoi(ev);
    const size_t bytes = h->field_elems * h->esz * NFIELDS;
    if (hipMalloc(reinterpret_cast<void**>(&h->arena), bytes) != hipSuccess) { rc = VOF_ENOMEM; break; }
    if (hipMemsetAsync(h->arena, 0, bytes, h->stream) != hipSuccess) { rc = VOF_EHIP; break; }
    h->views = FieldViews(h->arena, h->field_elems * h->esz);
    if ((rc = h->buf.courant.reserve(h, 4 * sizeof(unsigned long long), "vof_create: no memory for the counters", true))) break;
    const size_t tbmask_bytes = (2 * TB_BANDS * (TB_COLS / 64) + 1 + kTbPlanWaves) * sizeof(unsigned long long);   // the mask words, then the plan
    if ((rc = h->buf.tbmask.reserve(h, tbmask_bytes, "vof_create: no memory for the work plan", true))) break;
    h->d_courant = h->buf.courant.as<unsigned long long>();
    h->d_tbmask = h->buf.tbmask.as<unsigned long long>();
    if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) { rc = VOF_EHIP; break; }
    if (hipStreamSynchronize(h->stream) != hipSuccess) { rc = VOF_EHIP; break; }
  } while (0);
  if (rc != VOF_OK) {
    (void)hipGetLastError();
    vof_destroy(h);
    return rc;
  }
  *out = h;
  return VOF_OK;
}

int vof_destroy(vof2d_handle h) {
  if (!h) return VOF_EINVAL;
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  destroy_graphs(h);
  for (int k = 0; k < 2 * vof2d_ctx::kMaxTimed; ++k)
    if (h->tev[k]) (void)hipEventDestroy(h->tev[k]);
  for (hipEvent_t e : h->hev) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->tune.ev) if (e) (void)hipEventDestroy(e);
  for (hipStream_t st : h->chain_streams) (void)hipStreamDestroy(st);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->ev_gas) (void)hipEventDestroy(h->ev_gas);
  if (h->h_gas) (void)hipHostFree(h->h_gas);
  if (h->h_depths) (void)hipHostFree(h->h_depths);
  if (h->h_frame) (void)hipHostFree(h->h_frame);
  comm_teardown(h);
#ifdef VOF_SHORTCUT_STATS
  {
    unsigned long long a[16] = {};
    if (hipMemcpyFromSymbol(a, HIP_SYMBOL(vof::vof_stats), sizeof(a)) == hipSuccess && a[0] + a[3])
      fprintf(stderr, "[vof2d] shortcut stats (wave-rows): momentum rows %llu flat-normals %llu no-force %llu | transport rows %llu gas %llu liquid %llu "
              "uniform-update_uv %llu x-pipe-zero-bypass %llu x-stageB-skipped %llu x-stageD-clamp %llu | y rows swept %llu zero-flux %llu\n",
              a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11]);
  }
#endif
  h->buf.release();   // every work buffer (runtime/buffers.h)
  if (h->arena) (void)hipFree(h->arena);
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return VOF_OK;
}

int vof_set_init_F(vof2d_handle h, int32_t ic) {
  if (!h) return VOF_EINVAL;
  if (ic < 1 || ic > 3) return fail(h, VOF_EINVAL, "ic must be 1, 2 or 3 (2dvof.py:13)");
  settle_ghosts(h);
  DISPATCH_T(h, L<double>::init_F(h, ic), L<float>::init_F(h, ic));
  if (field_written(h->state, fF, full_domain(h), false)) forget_batch_form(h);
  if (tm_by_rule(h)) (void)post_gas_count(h);   // (the batch-form rule looks at the new F: the count is taken now, asynchronously, and read by the first batched step)
  return ensure_ok(h);
}
// ---- an initial state painted from shapes (kernels/scene.h, runtime/scene.h)
int vof_set_scene(vof2d_handle h, const double* shapes, int64_t n, int32_t samples, int32_t flags, double* summary) {
  if (!h) return VOF_EINVAL;
  if (const char* const msg = scene_check(shapes, n, samples, flags)) return fail(h, VOF_EINVAL, msg);
  return scene_run(h, shapes, n, samples, flags, summary);
}
// ---- a state carried onto a finer or coarser grid (kernels/regrid.h, runtime/regrid.h)
int vof_regrid(vof2d_handle dst, vof2d_handle src, int32_t flags, double eps, double* summary) {
  if (!dst || !src) return VOF_EINVAL;
  if (dst == src) return fail(dst, VOF_EINVAL, "vof_regrid: dst and src are the same handle");
  if (dst->device != src->device) return fail(dst, VOF_EINVAL, "vof_regrid: the handles are on different devices");
  RegridFactors f;
  if (const char* const msg = regrid_check(src->d.nx, src->d.ny, src->d.Lx, src->d.Ly, dst->d.nx, dst->d.ny, dst->d.Lx, dst->d.Ly, flags, eps, &f)) return fail(dst, VOF_EINVAL, msg);
  for (vof2d_ctx* const h : {dst, src}) {
    const int rc = check_verb_allowed(h, "vof_regrid needs the whole domain in both handles (a strip holds part of a state)");
    if (rc) return h == dst ? rc : fail(dst, rc, src->err);
  }
  return regrid_run(dst, src, f, flags, eps, summary);
}
int vof_set_BC(vof2d_handle h) {
  if (!h) return VOF_EINVAL;
  DISPATCH_T(h, (L<double>::set_bc<BC_ALL | BC_RHO>(h)), (L<float>::set_bc<BC_ALL | BC_RHO>(h)));
  bc_applied(h->state);   // this launch is the one a fused step left out
  return ensure_ok(h);
}
int vof_cal_nu_rho(vof2d_handle h) {
  if (!h) return VOF_EINVAL;
  settle_ghosts(h);
  DISPATCH_T(h, L<double>::nu_rho(h), L<float>::nu_rho(h));
  return ensure_ok(h);
}
int vof_get_normal_young(vof2d_handle h) {
  if (!h) return VOF_EINVAL;
  settle_ghosts(h);
  DISPATCH_T(h, (L<double>::normals(h), L<double>::kappa(h)), (L<float>::normals(h), L<float>::kappa(h)));
  verb_wrote_alt(h->state);
  return ensure_ok(h);
}
int vof_advect_upwind(vof2d_handle h) {
  if (!h) return VOF_EINVAL;
  settle_ghosts(h);
  DISPATCH_T(h, L<double>::predictor<true>(h), L<float>::predictor<true>(h));
  verb_wrote_alt(h->state);
  return ensure_ok(h);
}
int vof_solve_p_jacobi(vof2d_handle h, int32_t n) {
  if (!h) return VOF_EINVAL;
  settle_ghosts(h);
  if (n < 0) return fail(h, VOF_EINVAL, "n must be >= 0");
  if (n == 0) return VOF_OK;
  DISPATCH_T(h, (L<double>::rhs<true>(h), jacobi_n<double>(h, n, false)),
             (L<float>::rhs<true>(h), jacobi_n<float>(h, n, false)));
  return ensure_ok(h);
}
int vof_update_uv(vof2d_handle h) {
  if (!h) return VOF_EINVAL;
  settle_ghosts(h);
  DISPATCH_T(h, L<double>::correct<true>(h), L<float>::correct<true>(h));
  verb_wrote_uv(h->state);
  return ensure_ok(h);
}
int vof_fct_x_sweep(vof2d_handle h) {
  if (!h) return VOF_EINVAL;
  settle_ghosts(h);
  DISPATCH_T(h, (sweep_x<double, false, false>(h)), (sweep_x<float, false, false>(h)));
  verb_wrote_F(h->state);
  sweep_swapped(h);
  return ensure_ok(h);
}
int vof_fct_y_sweep(vof2d_handle h) {
  if (!h) return VOF_EINVAL;
  settle_ghosts(h);
  DISPATCH_T(h, (sweep_y<double, false, false>(h)), (sweep_y<float, false, false>(h)));
  verb_wrote_F(h->state);
  sweep_swapped(h);
  return ensure_ok(h);
}
int vof_solve_VOF_rudman(vof2d_handle h, int64_t istep) {
  if (!h) return VOF_EINVAL;
  int rc;
  if (istep % 2 == 0) {
    if ((rc = vof_fct_y_sweep(h))) return rc;
    return vof_fct_x_sweep(h);
  }
  if ((rc = vof_fct_x_sweep(h))) return rc;
  return vof_fct_y_sweep(h);
}
int vof_post_process_f(vof2d_handle h) {
  if (!h) return VOF_EINVAL;
  settle_ghosts(h);
  DISPATCH_T(h, L<double>::post(h), L<float>::post(h));
  verb_wrote_F(h->state);
  return ensure_ok(h);
}

int vof_step(vof2d_handle h, int64_t nsteps) {
  if (!h) return VOF_EINVAL;
  if (nsteps < 0) return fail(h, VOF_EINVAL, "nsteps must be >= 0");
  if (const int rc = check_no_phased_step(h)) return rc;
  return step_n(h, nsteps);   // (runtime/step.h: each step inside a batch graph, from its own graph, or eagerly)
}
int vof_step_phase(vof2d_handle h, int32_t phase) {
  if (!h) return VOF_EINVAL;
  if (phase < 0 || phase > 2) return fail(h, VOF_EINVAL, "phase must be 0, 1 or 2");
  if (!phase_is_next(h->state, phase)) return fail(h, VOF_ESTATE, "vof_step_phase must be called in the order 0, 1, 2");
  if (phase == 0) {
    settle_ghosts(h);
    h->istep += 1;
  }
  phase_taken(h->state, phase);
  return step_phase(h, phase);
}
int vof_get_istep(vof2d_handle h, int64_t* istep) {
  if (!h || !istep) return VOF_EINVAL;
  *istep = h->istep;
  return VOF_OK;
}
int vof_set_istep(vof2d_handle h, int64_t istep) {
  if (!h) return VOF_EINVAL;
  (void)settle_ahead(h);   // (the plan the last k_tm left is of the parity that was to follow)
  h->istep = istep;
  return VOF_OK;
}

double vof_residual_value(double max_update, double max_p, int32_t criterion) {
  return residual_rule(max_update, max_p, criterion);   // (kernels/residual_rule.h: the device forms it by the same lines)
}
int vof_jacobi_sweeps_norms(vof2d_handle h, int32_t n, int32_t build_rhs, double* max_update, double* max_p) {
  if (!h || !max_update || !max_p) return VOF_EINVAL;
  if (n < 1) return fail(h, VOF_EINVAL, "n must be >= 1");
  settle_ghosts(h);
  HIPCHK(h, hipMemsetAsync(h->d_courant + 1, 0, 2 * sizeof(unsigned long long), h->stream));
  if (build_rhs) DISPATCH_T(h, L<double>::rhs<false>(h), L<float>::rhs<false>(h));
  DISPATCH_T(h, jacobi_n<double>(h, n, true), jacobi_n<float>(h, n, true));
  int rc = ensure_ok(h);
  if (rc) return rc;
  unsigned long long bits[2] = {0, 0};
  if ((rc = read_back(h, bits, h->d_courant + 1, sizeof(bits)))) return rc;
  memcpy(max_update, &bits[0], sizeof(double));
  memcpy(max_p, &bits[1], sizeof(double));
  return VOF_OK;
}
int vof_jacobi_sweeps_residual(vof2d_handle h, int32_t n, int32_t build_rhs, double* residual) {
  double pmax = 0.0;
  if (!residual) return VOF_EINVAL;
  return vof_jacobi_sweeps_norms(h, n, build_rhs, residual, &pmax);
}

int vof_solve_p(vof2d_handle h, double tol, int32_t max_iters, int32_t check_every, int32_t criterion,
                int32_t* iters_done, double* residual) {
  if (!h || !iters_done || !residual) return VOF_EINVAL;
  if (max_iters < 1 || check_every < 1) return fail(h, VOF_EINVAL, "max_iters and check_every must be >= 1");
  if (const int rc = check_criterion(h, criterion)) return rc;
  int done = 0;
  double r = 0.0;
  bool first = true;
  while (done < max_iters) {
    const int n = check_every < max_iters - done ? check_every : max_iters - done;
    double upd = 0.0, pmax = 0.0;
    int rc = vof_jacobi_sweeps_norms(h, n, first ? 1 : 0, &upd, &pmax);
    if (rc) return rc;
    first = false;
    done += n;
    r = vof_residual_value(upd, pmax, criterion);
    if (r <= tol || !(r < HUGE_VAL)) break;   // converged, or diverged (a non-finite update reads +inf)
  }
  *iters_done = done;
  *residual = r;
  return VOF_OK;
}
int vof_solve_p_residual(vof2d_handle h, double tol, int32_t max_iters, int32_t check_every, int32_t* iters_done,
                         double* residual) {
  return vof_solve_p(h, tol, max_iters, check_every, VOF_RESID_ABS, iters_done, residual);
}

// ---- conjugate-gradient pressure solve (kernels/cg.h, runtime/multigrid.h)
int vof_solve_p_cg(vof2d_handle h, double tol, int32_t max_iters, int32_t check_every, int32_t criterion,
                   int32_t build_rhs, int32_t* iters_done, double* residual, double* drift) {
  if (!h || !iters_done || !residual || !drift) return VOF_EINVAL;
  if (max_iters < 1 || check_every < 1) return fail(h, VOF_EINVAL, "max_iters and check_every must be >= 1");
  if (const int rc = check_criterion(h, criterion)) return rc;
  if (const int rc = check_whole_domain(h, "vof_solve_p_cg needs the whole domain in one handle (the dot products of a strip would need an all-reduce)")) return rc;
  settle_ghosts(h);
  return cg_solve(h, tol, max_iters, check_every, criterion, build_rhs, iters_done, residual, drift);
}

// ---- geometric multigrid on the same equation (kernels/mg.h, runtime/multigrid.h)
int vof_solve_p_mg(vof2d_handle h, double tol, int32_t max_cycles, int32_t check_every, int32_t criterion,
                   int32_t build_rhs, int32_t* cycles_done, double* residual, double* drift) {
  if (!h || !cycles_done || !residual || !drift) return VOF_EINVAL;
  if (max_cycles < 1 || check_every < 1) return fail(h, VOF_EINVAL, "max_cycles and check_every must be >= 1");
  if (const int rc = check_criterion(h, criterion)) return rc;
  if (const int rc = check_whole_domain(h, "vof_solve_p_mg needs the whole domain in one handle (a strip's coarse levels and sums would span its neighbours)")) return rc;
  settle_ghosts(h);
  return mg_solve(h, tol, max_cycles, check_every, criterion, build_rhs, cycles_done, residual, drift);
}

// ---- time steps whose pressure solve is a fixed number of those cycles (runtime/step.h)
int vof_step_mg(vof2d_handle h, int64_t nsteps, int32_t cycles, int32_t criterion, double* last_residual, double* worst_residual,
                int64_t* worst_step) {
  if (!h) return VOF_EINVAL;
  if (nsteps < 0) return fail(h, VOF_EINVAL, "nsteps must be >= 0");
  if (cycles < 1) return fail(h, VOF_EINVAL, "cycles must be >= 1");
  if (const int rc = check_criterion(h, criterion)) return rc;
  if (const int rc = check_whole_domain(h, "vof_step_mg needs the whole domain in one handle (a strip's coarse levels and sums would span its neighbours)")) return rc;
  if (const int rc = check_no_phased_step(h)) return rc;
  return step_mg_n(h, nsteps, cycles, criterion, last_residual, worst_residual, worst_step);
}

// ---- diagnostics on the device (kernels/diag.h, runtime/diag_reduce.h)
int vof_diagnostics(vof2d_handle h, double* out) {
  if (!h || !out) return VOF_EINVAL;
  int rc = reduced_prepare(h, kDiagVerb, 1);
  if (rc) return rc;
  if ((rc = diag_enqueue(h, 0))) return rc;
  return read_back(h, out, h->buf.diag.rows.p, VOF_DIAG_N * sizeof(double));
}
int vof_step_diag(vof2d_handle h, int64_t nsteps, int64_t every, int32_t mg_cycles, int32_t criterion, double* out, int64_t cap_rows,
                  int64_t* rows_written) {
  if (const int rc = check_step_args(h, nsteps, every, mg_cycles, criterion)) return rc;
  if (cap_rows < nsteps / every) return fail(h, VOF_EINVAL, "cap_rows is smaller than nsteps / every");
  if (!out && nsteps / every > 0) return fail(h, VOF_EINVAL, "out is NULL and at least one row is due");
  if (const int rc = check_whole_domain(h, "vof_step_diag needs the whole domain in one handle (a strip's steps need their exchanges: call vof_diagnostics between them)")) return rc;
  if (const int rc = check_no_phased_step(h)) return rc;
  if (no_steps(nsteps, rows_written)) return VOF_OK;
  return step_diag_n(h, nsteps, every, mg_cycles, criterion, out, rows_written);
}

// ---- a row per interface cell (kernels/cell_rows.h, runtime/cell_rows.h)
namespace {
// what both verbs refuse, in this order; too_many_cells names the verb
int check_cell_rows_args(vof2d_ctx* h, double eps, const double* rows, int64_t cap_rows, const double* summary, const char* too_many_cells) {
  if (!h || !summary) return VOF_EINVAL;
  if (!(eps >= 0.0 && eps < 0.5)) return fail(h, VOF_EINVAL, "eps must lie in [0, 0.5)");
  if (cap_rows < 0 || (!rows && cap_rows > 0)) return fail(h, VOF_EINVAL, "rows is NULL with cap_rows > 0, or cap_rows < 0");
  return (int64_t)h->d.nx * h->d.ny > (int64_t)INT32_MAX ? fail(h, VOF_EINVAL, too_many_cells) : VOF_OK;
}
}  // namespace
// the interface as PLIC segments (kernels/interface.h)
int vof_interface(vof2d_handle h, double eps, double* rows, int64_t cap_rows, double* summary) {
  if (const int rc = check_cell_rows_args(h, eps, rows, cap_rows, summary, "vof_interface keeps 32-bit offsets: at most 2^31 - 1 cells")) return rc;
  return cell_rows_run(h, kIfaceRows, eps, rows, cap_rows, summary);
}
// height-function curvature beside the solver's own (kernels/curvature.h)
int vof_curvature(vof2d_handle h, double eps, double* rows, int64_t cap_rows, double* summary) {
  if (const int rc = check_cell_rows_args(h, eps, rows, cap_rows, summary, "vof_curvature keeps 32-bit offsets: at most 2^31 - 1 cells")) return rc;
  if (const int rc = check_verb_allowed(h, "vof_curvature needs the whole domain in one handle (curvature over row strips is not built)")) return rc;
  return cell_rows_run(h, kCurvRows, eps, rows, cap_rows, summary);
}

// ---- the energy budget of the flow (kernels/energy.h, runtime/energy.h)
int vof_energy(vof2d_handle h, double* out) {
  if (!h || !out) return VOF_EINVAL;
  if (const int rc = check_verb_allowed(h, "vof_energy needs the whole domain in one handle (the energy budget over row strips is not built)")) return rc;
  int rc = reduced_prepare(h, kEnergyVerb, 1);
  if (rc) return rc;
  if ((rc = energy_enqueue(h, 0))) return rc;
  return read_back(h, out, h->buf.energy.rows.p, VOF_ENERGY_N * sizeof(double));
}
int vof_step_energy(vof2d_handle h, int64_t nsteps, int64_t every, int32_t mg_cycles, int32_t criterion, double* out, int64_t cap_rows,
                    int64_t* rows_written) {
  if (const int rc = check_step_args(h, nsteps, every, mg_cycles, criterion)) return rc;
  if (cap_rows < nsteps / every) return fail(h, VOF_EINVAL, "cap_rows is smaller than nsteps / every");
  if (!out && nsteps / every > 0) return fail(h, VOF_EINVAL, "out is NULL and at least one row is due");
  if (const int rc = check_verb_allowed(h, "vof_step_energy needs the whole domain in one handle (the energy budget over row strips is not built)")) return rc;
  if (no_steps(nsteps, rows_written)) return VOF_OK;
  return step_energy_n(h, nsteps, every, mg_cycles, criterion, out, rows_written);
}

// ---- droplets and bubbles, labelled and measured (kernels/blobs.h, runtime/blobs.h)
int vof_blobs(vof2d_handle h, int32_t phase, double threshold, double* rows, int64_t cap_rows, int32_t* labels, size_t labels_bytes, double* summary) {
  if (!h || !summary) return VOF_EINVAL;
  if (phase != VOF_BLOB_LIQUID && phase != VOF_BLOB_GAS) return fail(h, VOF_EINVAL, "phase must be VOF_BLOB_LIQUID or VOF_BLOB_GAS");
  if (!(threshold > 0.0 && threshold < 1.0)) return fail(h, VOF_EINVAL, "threshold must lie in (0, 1)");
  if (cap_rows < 0 || (!rows && cap_rows > 0)) return fail(h, VOF_EINVAL, "rows is NULL with cap_rows > 0, or cap_rows < 0");
  if ((int64_t)h->d.nx * h->d.ny > (int64_t)INT32_MAX) return fail(h, VOF_EINVAL, "vof_blobs keeps 32-bit keys: at most 2^31 - 1 cells");
  if (labels && labels_bytes != (size_t)reported(h).cells() * sizeof(int32_t)) return fail(h, VOF_EINVAL, "labels_bytes is not (owned interior rows) x ny x 4");
  return blobs_run(h, phase, threshold, rows, cap_rows, labels, summary);
}

// ---- passive tracers moved with the flow (kernels/tracers.h, runtime/tracers.h)
namespace {
int check_tracers_allowed(vof2d_ctx* h) { return check_verb_allowed(h, "the vof_tracers_* verbs and vof_step_tracers need the whole domain in one handle (a tracer would leave a strip's rows)"); }
}  // namespace
int vof_tracers_set(vof2d_handle h, const double* xy, int64_t n) {
  if (!h) return VOF_EINVAL;
  if (n < 0 || n > (int64_t)INT32_MAX) return fail(h, VOF_EINVAL, "n must lie in [0, 2^31 - 1]");
  if (!xy && n > 0) return fail(h, VOF_EINVAL, "xy is NULL with n > 0");
  if (const int rc = check_tracers_allowed(h)) return rc;
  if (!tracer_positions_ok(h, xy, n)) return fail(h, VOF_EINVAL, "a position is not finite or lies outside [0, Lx] x [0, Ly]");
  return tracers_set(h, xy, n);
}
int vof_tracers_advance(vof2d_handle h, double time) {
  if (!h) return VOF_EINVAL;
  if (!std::isfinite(time)) return fail(h, VOF_EINVAL, "time must be finite");
  if (const int rc = check_tracers_allowed(h)) return rc;
  return tracers_advance(h, time);
}
int vof_tracers_get(vof2d_handle h, double* rows, int64_t cap_rows, double* summary) {
  if (!h || !summary) return VOF_EINVAL;
  if (cap_rows < 0 || (!rows && cap_rows > 0)) return fail(h, VOF_EINVAL, "rows is NULL with cap_rows > 0, or cap_rows < 0");
  if (const int rc = check_tracers_allowed(h)) return rc;
  return tracers_get(h, rows, cap_rows, summary);
}
int vof_step_tracers(vof2d_handle h, int64_t nsteps, int64_t every, int32_t mg_cycles, int32_t criterion, int64_t snap_every, double* snaps,
                     int64_t cap_snaps, int64_t* snaps_written) {
  if (const int rc = check_step_args(h, nsteps, every, mg_cycles, criterion, snap_every < 0 ? "snap_every must be >= 0 (0: no snapshots)" : nullptr)) return rc;
  const int64_t due = tracer_snaps_due(nsteps, every, snap_every);
  if (cap_snaps < due) return fail(h, VOF_EINVAL, "cap_snaps is smaller than the snapshots due, (nsteps / every) / snap_every");
  if (!snaps && due > 0) return fail(h, VOF_EINVAL, "snaps is NULL and at least one snapshot is due");
  if (const int rc = check_tracers_allowed(h)) return rc;
  if (no_steps(nsteps, snaps_written)) return VOF_OK;
  return step_tracers_n(h, nsteps, every, mg_cycles, criterion, snap_every, snaps, snaps_written);
}

// ---- both marginals of F, the top of the liquid, the front; fixed sensors (kernels/depths.h, runtime/depths.h)
int vof_depths(vof2d_handle h, double* depth_i, int64_t cap_i, double* depth_j, int64_t cap_j, int32_t* top, int64_t cap_top, double* summary) {
  if (!h || !summary) return VOF_EINVAL;
  if (cap_i < 0 || cap_j < 0 || cap_top < 0) return fail(h, VOF_EINVAL, "a cap is negative");
  if ((int64_t)h->d.nx * h->d.ny > (int64_t)INT32_MAX) return fail(h, VOF_EINVAL, "vof_depths keeps 32-bit offsets: at most 2^31 - 1 cells");
  const int64_t rows = reported(h).rows();
  if ((depth_i && cap_i < rows) || (top && cap_top < rows)) return fail(h, VOF_EINVAL, "cap_i or cap_top is smaller than the owned interior rows");
  if (depth_j && cap_j < h->d.ny) return fail(h, VOF_EINVAL, "cap_j is smaller than ny");
  return depths_run(h, depth_i, depth_j, top, summary);
}
namespace {
int check_gauges_allowed(vof2d_ctx* h) { return check_verb_allowed(h, "the vof_gauges_* verbs and vof_step_gauges need the whole domain in one handle (a gauge may lie outside a strip's rows: call vof_depths on the strips)"); }
}  // namespace
int vof_gauges_set(vof2d_handle h, const double* xy, int64_t n) {
  if (!h) return VOF_EINVAL;
  if (n < 0 || n > (int64_t)INT32_MAX) return fail(h, VOF_EINVAL, "n must lie in [0, 2^31 - 1]");
  if (!xy && n > 0) return fail(h, VOF_EINVAL, "xy is NULL with n > 0");
  if (const int rc = check_gauges_allowed(h)) return rc;
  if (!tracer_positions_ok(h, xy, n)) return fail(h, VOF_EINVAL, "a position is not finite or lies outside [0, Lx] x [0, Ly]");
  return gauges_set(h, xy, n);
}
int vof_gauges_get(vof2d_handle h, double* rows, int64_t cap_rows, double* summary) {
  if (!h || !summary) return VOF_EINVAL;
  if (cap_rows < 0 || (!rows && cap_rows > 0)) return fail(h, VOF_EINVAL, "rows is NULL with cap_rows > 0, or cap_rows < 0");
  if (const int rc = check_gauges_allowed(h)) return rc;
  return gauges_get(h, rows, cap_rows, summary);
}
int vof_step_gauges(vof2d_handle h, int64_t nsteps, int64_t every, int32_t mg_cycles, int32_t criterion, double* out, int64_t cap_records,
                    int64_t* records_written) {
  if (const int rc = check_step_args(h, nsteps, every, mg_cycles, criterion)) return rc;
  if (cap_records < nsteps / every) return fail(h, VOF_EINVAL, "cap_records is smaller than nsteps / every");
  if (!out && nsteps / every > 0) return fail(h, VOF_EINVAL, "out is NULL and at least one record is due");
  if (const int rc = check_gauges_allowed(h)) return rc;
  if (h->gauge_n == 0 && nsteps / every > 0) return fail(h, VOF_EINVAL, "the handle has no gauges and at least one record is due");
  if (no_steps(nsteps, records_written)) return VOF_OK;
  return step_gauges_n(h, nsteps, every, mg_cycles, criterion, out, records_written);
}

// ---- a marker field carried by the FCT transport (kernels/dye.h, runtime/dye.h)
namespace {
int check_dye_allowed(vof2d_ctx* h, bool needs_dye) {
  return check_verb_allowed(h, "the vof_dye_* verbs and vof_step_dye need the whole domain in one handle (a strip's sweeps need their exchanges)", needs_dye && !h->dye_on ? "the handle has no dye (vof_dye_set)" : nullptr);
}
}  // namespace
int vof_dye_set(vof2d_handle h, const void* src, size_t nbytes) {
  if (!h) return VOF_EINVAL;
  if (src ? nbytes != dye_dense_bytes(h) : nbytes != 0) return fail(h, VOF_EINVAL, "nbytes is not (nx+2) x (ny+2) of the field dtype (or not 0 with src NULL)");
  if (const int rc = check_dye_allowed(h, false)) return rc;
  return dye_set(h, src);
}
int vof_dye_get(vof2d_handle h, void* dst, size_t nbytes) {
  if (!h || !dst) return VOF_EINVAL;
  if (nbytes != dye_dense_bytes(h)) return fail(h, VOF_EINVAL, "nbytes is not (nx+2) x (ny+2) of the field dtype");
  if (const int rc = check_dye_allowed(h, true)) return rc;
  return dye_copy_host(h, h->dye_cur, dst, true);
}
int vof_dye_advance(vof2d_handle h) {
  if (!h) return VOF_EINVAL;
  if (const int rc = check_dye_allowed(h, true)) return rc;
  return dye_advance(h);
}
int vof_dye_stats(vof2d_handle h, double* out) {
  if (!h || !out) return VOF_EINVAL;
  int rc = check_dye_allowed(h, true);
  if (rc) return rc;
  if ((rc = reduced_prepare(h, kDyeVerb, 1))) return rc;
  if ((rc = dye_stats_enqueue(h, 0))) return rc;
  return read_back(h, out, h->buf.dye_stats.rows.p, VOF_DYE_N * sizeof(double));
}
int vof_step_dye(vof2d_handle h, int64_t nsteps, int64_t every, int32_t mg_cycles, int32_t criterion, double* out, int64_t cap_rows,
                 int64_t* rows_written) {
  if (const int rc = check_step_args(h, nsteps, every, mg_cycles, criterion, nullptr, 0, "every must be >= 0 (0: no rows)")) return rc;
  const int64_t due = every > 0 ? nsteps / every : 0;
  if (cap_rows < due) return fail(h, VOF_EINVAL, "cap_rows is smaller than nsteps / every");
  if (!out && due > 0) return fail(h, VOF_EINVAL, "out is NULL and at least one row is due");
  if (const int rc = check_dye_allowed(h, true)) return rc;
  if (no_steps(nsteps, rows_written)) return VOF_OK;
  return step_dye_n(h, nsteps, every, mg_cycles, criterion, out, rows_written);
}

// ---- colour-mapped pictures rendered on the device (kernels/frames.h, runtime/frames.h)
namespace {
int check_frames_allowed(vof2d_ctx* h) { return check_verb_allowed(h, "vof_frame_set_lut, vof_frame and vof_step_frames need the whole domain in one handle (frames over row strips are not built)"); }
// 0, or VOF_EINVAL with the message set: the spec alone (pixels: pw * ph of it)
int check_frame_spec(vof2d_ctx* h, const vof2d_frame_spec* spec, int64_t* pixels) {
  if (!spec) return fail(h, VOF_EINVAL, "spec is NULL");
  if (spec->quantity < 0 || spec->quantity >= FQ_N) return fail(h, VOF_EINVAL, "spec.quantity is not one of VOF_FRAME_F .. VOF_FRAME_DYE");
  if (spec->flags & ~(FRF_CONTOUR | FRF_SYMMETRIC)) return fail(h, VOF_EINVAL, "spec.flags has a bit outside VOF_FRAME_CONTOUR | VOF_FRAME_SYMMETRIC");
  if (spec->bx < 1 || spec->by < 1) return fail(h, VOF_EINVAL, "spec.bx and spec.by must be >= 1");
  if (!std::isfinite(spec->lo) || !std::isfinite(spec->hi) || spec->hi < spec->lo) return fail(h, VOF_EINVAL, "spec.lo and spec.hi must be finite with hi >= lo (lo == hi: the range of the picture)");
  const FrameGeom fg = frame_geom(h->d.nx, h->d.ny, h->g.ntj, 64 * h->V, spec->bx, spec->by);
  if (fg.pixels * 3 > (int64_t)INT32_MAX) return fail(h, VOF_EINVAL, "the picture would have more than 2^31 - 1 bytes");
  *pixels = fg.pixels;
  return VOF_OK;
}
}  // namespace
int vof_frame_set_lut(vof2d_handle h, const uint8_t* lut) {
  if (!h) return VOF_EINVAL;
  if (const int rc = check_frames_allowed(h)) return rc;
  return frame_set_lut(h, lut);
}
int vof_frame(vof2d_handle h, const vof2d_frame_spec* spec, uint8_t* rgb, int64_t cap_bytes, double* means, int64_t cap_means, double* summary) {
  if (!h || !summary) return VOF_EINVAL;
  int64_t pixels = 0;
  if (const int rc = check_frame_spec(h, spec, &pixels)) return rc;
  if (cap_bytes < 0 || cap_means < 0) return fail(h, VOF_EINVAL, "a cap is negative");
  if ((rgb && cap_bytes < pixels * 3) || (means && cap_means < pixels)) return fail(h, VOF_EINVAL, "cap_bytes is smaller than pw * ph * 3 or cap_means smaller than pw * ph");
  if (const int rc = check_frames_allowed(h)) return rc;
  if (spec->quantity == FQ_DYE && !h->dye_on) return fail(h, VOF_ESTATE, "the handle has no dye (vof_dye_set)");
  return frame_run(h, *spec, rgb, means, summary);
}
int vof_step_frames(vof2d_handle h, int64_t nsteps, int64_t every, int32_t mg_cycles, int32_t criterion, const vof2d_frame_spec* spec, uint8_t* out_rgb,
                    double* out_summaries, int64_t cap_frames, int64_t* frames_written) {
  if (const int rc = check_step_args(h, nsteps, every, mg_cycles, criterion)) return rc;
  int64_t pixels = 0;
  if (const int rc = check_frame_spec(h, spec, &pixels)) return rc;
  if (cap_frames < nsteps / every) return fail(h, VOF_EINVAL, "cap_frames is smaller than nsteps / every");
  if ((!out_rgb || !out_summaries) && nsteps / every > 0) return fail(h, VOF_EINVAL, "out_rgb or out_summaries is NULL and at least one frame is due");
  if (const int rc = check_frames_allowed(h)) return rc;
  if (spec->quantity == FQ_DYE && !h->dye_on) return fail(h, VOF_ESTATE, "the handle has no dye (vof_dye_set)");
  if (no_steps(nsteps, frames_written)) return VOF_OK;
  return step_frames_n(h, nsteps, every, mg_cycles, criterion, *spec, out_rgb, out_summaries, frames_written);
}

// ---- per-cell statistics over a run (kernels/stats.h, runtime/stats.h)
namespace {
int check_stats_allowed(vof2d_ctx* h, bool needs_stats) {
  return check_verb_allowed(h, "the vof_stats_* verbs and vof_step_stats need the whole domain in one handle (statistics over row strips are not built)", needs_stats && !h->stats_mask ? "the handle has no statistics (vof_stats_begin)" : nullptr);
}
}  // namespace
int vof_stats_begin(vof2d_handle h, int32_t mask, double level) {
  if (!h) return VOF_EINVAL;
  if (mask < 0 || mask > (VOF_STATS_MOMENTS | VOF_STATS_ENVELOPE)) return fail(h, VOF_EINVAL, "mask must be 0 or VOF_STATS_MOMENTS | VOF_STATS_ENVELOPE");
  if (mask != 0 && !(level > 0.0 && level <= 1.0)) return fail(h, VOF_EINVAL, "level must lie in (0, 1]");
  if (const int rc = check_stats_allowed(h, false)) return rc;
  return stats_begin(h, mask, level);
}
int vof_stats_sample(vof2d_handle h) {
  if (!h) return VOF_EINVAL;
  if (const int rc = check_stats_allowed(h, true)) return rc;
  return stats_sample(h);
}
int vof_stats_get(vof2d_handle h, int32_t slot, double* dst, int64_t cap_elems) {
  if (!h || !dst) return VOF_EINVAL;
  if (slot < 0 || slot >= VOF_STATS_PLANES) return fail(h, VOF_EINVAL, "slot is not one of VOF_STATS_SUM_F .. VOF_STATS_ARRIVAL");
  if (cap_elems < (int64_t)h->d.nx * h->d.ny) return fail(h, VOF_EINVAL, "cap_elems is smaller than nx ny");
  if (const int rc = check_stats_allowed(h, true)) return rc;
  if (!(h->stats_mask & (slot < kStatsMoments ? VOF_STATS_MOMENTS : VOF_STATS_ENVELOPE))) return fail(h, VOF_ESTATE, "the group of this slot is off (vof_stats_begin)");
  return stats_get(h, slot, dst);
}
int vof_stats_summary(vof2d_handle h, double* out) {
  if (!h || !out) return VOF_EINVAL;
  if (const int rc = check_stats_allowed(h, true)) return rc;
  return stats_summary(h, out);
}
int vof_step_stats(vof2d_handle h, int64_t nsteps, int64_t every, int32_t mg_cycles, int32_t criterion, int64_t* samples_taken) {
  if (const int rc = check_step_args(h, nsteps, every, mg_cycles, criterion)) return rc;
  if (const int rc = check_stats_allowed(h, true)) return rc;
  if (no_steps(nsteps, samples_taken)) return VOF_OK;
  return step_stats_n(h, nsteps, every, mg_cycles, criterion, samples_taken);
}

int vof_get_rows(vof2d_handle h, const char* name, int32_t g0, int32_t g1, void* dst, size_t nbytes) {
  if (!h || !dst) return VOF_EINVAL;
  settle_ghosts(h);
  int id = field_id(name);
  if (id < 0) return fail(h, VOF_EINVAL, "unknown field name");
  return copy_rows_host(h, id, g0, g1, dst, nbytes, true);
}
int vof_set_rows(vof2d_handle h, const char* name, int32_t g0, int32_t g1, const void* src, size_t nbytes) {
  if (!h || !src) return VOF_EINVAL;
  settle_ghosts(h);
  int id = field_id(name);
  if (id < 0) return fail(h, VOF_EINVAL, "unknown field name");
  int rc = copy_rows_host(h, id, g0, g1, const_cast<void*>(src), nbytes, false);
  if (rc == VOF_OK && id == fF) rc = copy_rows_host(h, fF2, g0, g1, const_cast<void*>(src), nbytes, false);
  if (field_written(h->state, id, full_domain(h), false)) forget_batch_form(h);
  return rc;
}
int vof_get_field(vof2d_handle h, const char* name, void* dst, size_t nbytes) {
  if (!h) return VOF_EINVAL;
  return vof_get_rows(h, name, h->d.row_lo, h->d.row_hi, dst, nbytes);
}
int vof_set_field(vof2d_handle h, const char* name, const void* src, size_t nbytes) {
  if (!h) return VOF_EINVAL;
  return vof_set_rows(h, name, h->d.row_lo, h->d.row_hi, src, nbytes);
}
int vof_field_view(vof2d_handle h, const char* name, void** base, int64_t* pitch, int64_t* col0, int64_t* nrows) {
  if (!h) return VOF_EINVAL;
  settle_ghosts(h);
  int id = field_id(name);
  if (id < 0) return fail(h, VOF_EINVAL, "unknown field name");
  // the caller may write through the pointer at any time, unseen: a handle that gave out F or its twin keeps no zero maps from here on
  // (fzmap_allowed; the next batch captures its graphs without them)
  if (id == fF || id == fF2) { h->f_view_given = true; step_wrote_F(h->state); }
  if (base) *base = h->fld[id];
  if (pitch) *pitch = h->g.pitch;
  if (col0) *col0 = h->g.col0;
  if (nrows) *nrows = h->d.row_hi - h->d.row_lo + 1;
  return VOF_OK;
}
int vof_copy_rows(vof2d_handle dst, vof2d_handle src, const char* name, int32_t g0, int32_t g1) {
  if (!dst || !src) return VOF_EINVAL;
  settle_ghosts(dst);
  settle_ghosts(src);
  int id = field_id(name);
  if (id < 0) return fail(dst, VOF_EINVAL, "unknown field name");
  if (dst->d.ny != src->d.ny || dst->d.nx != src->d.nx || dst->d.dtype != src->d.dtype)
    return fail(dst, VOF_EINVAL, "handles differ in nx, ny or dtype");
  if (g1 < g0 || g0 < src->d.row_lo || g1 > src->d.row_hi || g0 < dst->d.row_lo || g1 > dst->d.row_hi)
    return fail(dst, VOF_EINVAL, "rows not stored by both handles");
  // both use the same pitch/col0 (functions of ny and dtype only): one contiguous block
  const size_t off_s = (size_t)(g0 - src->d.row_lo) * src->g.pitch * src->esz;
  const size_t off_d = (size_t)(g0 - dst->d.row_lo) * dst->g.pitch * dst->esz;
  const size_t bytes = (size_t)(g1 - g0 + 1) * src->g.pitch * src->esz;
  // order, both ways: the copy runs on dst's stream after src's pending work, and whatever src enqueues next runs after
  // the copy -- a strip's next launches overwrite rows in place (p: the second five-sweep launch or the copy-back of an
  // odd launch count; rhs: k_tm) that a neighbour's pending copy may still have to read.  (Until round 6 only the first
  // half held: the differential fuzz of tests/test_fuzz_gpu.py met the other one in 2 of 1700 emulated strip runs,
  // both with five sweeps per step -- the shortest way from a copy to the next in-place write of p.)
  HIPCHK(dst, hipEventRecord(src->ev1, src->stream));
  HIPCHK(dst, hipStreamWaitEvent(dst->stream, src->ev1, 0));
  HIPCHK(dst, hipMemcpyAsync(reinterpret_cast<char*>(dst->fld[id]) + off_d,
                             reinterpret_cast<char*>(src->fld[id]) + off_s, bytes, hipMemcpyDeviceToDevice,
                             dst->stream));
  if (id == fF)
    HIPCHK(dst, hipMemcpyAsync(reinterpret_cast<char*>(dst->fld[fF2]) + off_d,
                               reinterpret_cast<char*>(src->fld[fF]) + off_s, bytes, hipMemcpyDeviceToDevice,
                               dst->stream));
  if (src->stream != dst->stream) {
    HIPCHK(dst, hipEventRecord(dst->ev1, dst->stream));
    HIPCHK(dst, hipStreamWaitEvent(src->stream, dst->ev1, 0));
  }
  if (field_written(dst->state, id, full_domain(dst), /*rows_only_inside=*/true)) forget_batch_form(dst);
  return VOF_OK;
}

// 2dvof.py:458-492 -- display fields.  The image / vector field is produced on the device into a
// scratch buffer allocated on first use and copied to the caller's dense host array.
constexpr const char* kVisNoMem = "hipMalloc of the visualisation buffer failed";
int vof_get_vis_field(vof2d_handle h, const char* which, void* dst, size_t nbytes) {
  if (!h || !which || !dst) return VOF_EINVAL;
  settle_ghosts(h);
  if (!full_domain(h)) return fail(h, VOF_ESTATE, "display fields need a full-domain handle");
  int mode = !strcmp(which, "vof") ? 0 : !strcmp(which, "u") ? 1 : !strcmp(which, "v") ? 2 : !strcmp(which, "vnorm") ? 3 : -1;
  if (mode < 0) return fail(h, VOF_EINVAL, "display field must be vof, u, v or vnorm");
  const size_t bytes = (size_t)4 * h->g.nx * h->g.ny * h->esz;
  if (nbytes != bytes) return fail(h, VOF_EINVAL, "buffer must be (2*nx, 2*ny) of the field dtype");
  int rc = h->buf.vis.reserve(h, bytes, kVisNoMem);
  if (rc) return rc;
  dim3 grid((2 * h->g.ny + 255) / 256, 2 * h->g.nx);
  const double umax = h->d.Lx / 0.2, vmax = h->d.Ly / 0.2;  // :468, :476, :484
  if (h->d.dtype == VOF_F64)
    launch(h, kOther, k_vis_field<double>, grid, 0, h->g, (const double*)F_<double>(h, fF), (const double*)F_<double>(h, fU),
           (const double*)F_<double>(h, fV), h->buf.vis.as<double>(), mode, umax, vmax);
  else
    launch(h, kOther, k_vis_field<float>, grid, 0, h->g, (const float*)F_<float>(h, fF), (const float*)F_<float>(h, fU),
           (const float*)F_<float>(h, fV), h->buf.vis.as<float>(), mode, (float)umax, (float)vmax);
  if ((rc = read_back(h, dst, h->buf.vis.p, bytes))) return rc;
  return ensure_ok(h);
}
int vof_interp_velocity(vof2d_handle h, void* dst, size_t nbytes) {
  if (!h || !dst) return VOF_EINVAL;
  settle_ghosts(h);
  if (!full_domain(h)) return fail(h, VOF_ESTATE, "interp_velocity needs a full-domain handle");
  const size_t bytes = (size_t)2 * (h->g.nx + 2) * (h->g.ny + 2) * h->esz;
  if (nbytes != bytes) return fail(h, VOF_EINVAL, "buffer must be (nx+2, ny+2, 2) of the field dtype");
  int rc = h->buf.vis.reserve(h, bytes, kVisNoMem);
  if (rc) return rc;
  dim3 grid((h->g.ny + 2 + 255) / 256, h->g.nx + 2);
  if (h->d.dtype == VOF_F64)
    launch(h, kOther, k_interp_velocity<double>, grid, 0, h->g, (const double*)F_<double>(h, fU),
           (const double*)F_<double>(h, fV), h->buf.vis.as<double>());
  else
    launch(h, kOther, k_interp_velocity<float>, grid, 0, h->g, (const float*)F_<float>(h, fU),
           (const float*)F_<float>(h, fV), h->buf.vis.as<float>());
  if ((rc = read_back(h, dst, h->buf.vis.p, bytes))) return rc;
  return ensure_ok(h);
}

int vof_set_param(vof2d_handle h, const char* name, double value) {
  if (!h || !name) return VOF_EINVAL;
  if (!strcmp(name, "sigma")) {  // sigma[None] = value (2dvof.py:28-29); constants are baked into graphs
    (void)settle_ahead(h);   // (a predictor formed ahead of its step used the old value)
    h->d.sigma = value;
    h->cd.sigma = value;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    destroy_graphs(h);
    return VOF_OK;
  }
  settle_ghosts(h);
  if (const Knob* k = find_knob(name)) {
    int* knob = k->at(h);
    *knob = (int)value;
    if (knob == &h->band_rows && *knob < 1) *knob = 1;
    if (knob == &h->step_batch[0]) *knob = *knob < 4 ? 4 : (*knob & ~1);   // an even number of steps (see step.h)
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    destroy_graphs(h);
    step_wrote_F(h->state);   // (a knob may switch k_tm's zero maps off and on again: what they say is given up)
    return VOF_OK;
  }
  return fail(h, VOF_EINVAL, "unknown or read-only parameter");
}
int vof_get_param(vof2d_handle h, const char* name, double* value) {
  if (!h || !name || !value) return VOF_EINVAL;
#define P(n) if (!strcmp(name, #n)) { *value = h->cd.n; return VOF_OK; }
  P(sigma) P(dt) P(dx) P(dy) P(dxi) P(dyi) P(dxi2) P(dyi2) P(rho_l) P(rho_g) P(nu_l) P(nu_g) P(gx) P(gy)
  P(nrm_x) P(nrm_y) P(kap_x) P(kap_y) P(dxdy) P(dtdy) P(dtdx) P(cfl_x) P(cfl_y) P(half_dx) P(half_dy)
  P(sqrt2dx) P(tiny)
#undef P
  if (!strcmp(name, "Lx")) { *value = h->d.Lx; return VOF_OK; }
  if (!strcmp(name, "Ly")) { *value = h->d.Ly; return VOF_OK; }
  if (!strcmp(name, "pitch")) { *value = (double)h->g.pitch; return VOF_OK; }
  if (!strcmp(name, "rows_per_wave")) { *value = (double)pick_rows(h, h->g.ntj); return VOF_OK; }
  if (!strcmp(name, "overlap_halves")) { *value = halves_eligible(h, h->step_batch[vof2d_ctx::kTuneBatch]) ? 1.0 : 0.0; return VOF_OK; }   // effective
  if (!strcmp(name, "gas_share")) { *value = h->gas_share; return VOF_OK; }   // share of exact-zero cells of F the batch-form rule saw (-1: not looked yet)
  if (!strcmp(name, "fuse_transport")) {  // 1 if vof_step runs both FCT sweeps as one kernel on this handle
    *value = (h->g.wall_lo && h->g.wall_hi && h->fuse_transport) ? 1.0 : 0.0;
    return VOF_OK;
  }
  if (!strcmp(name, "mg_coarse_block")) { *value = mg_block_in_effect(h) ? 1.0 : 0.0; return VOF_OK; }   // 1 if a cycle of this handle ends in k_mg_coarse_block
  if (const Knob* k = find_knob(name))
    if (k->readable) { *value = (double)*k->at(h); return VOF_OK; }
  return fail(h, VOF_EINVAL, "unknown parameter");
}
int vof_get_counter(vof2d_handle h, const char* name, int64_t* value) {
  if (!h || !name || !value) return VOF_EINVAL;
  if (!strcmp(name, "courant_violations")) {
    unsigned long long v = 0;
    if (const int rc = read_back(h, &v, h->d_courant, sizeof(v))) return rc;
    *value = (int64_t)v;
    return VOF_OK;
  }
  if (!strcmp(name, "tb_plan_active")) {   // 1 if the last fused step's k_jacobi_tb launches ran the equal-cost work plan (tb_make_plan)
    unsigned long long v = 0;
    if (const int rc = read_back(h, &v, h->d_tbmask + 2 * TB_BANDS * (TB_COLS / 64), sizeof(v))) return rc;
    *value = v ? 1 : 0;   // (plan[0] of an active plan carries its geometry: plan_key)
    return VOF_OK;
  }
#ifdef VOF_WAVE_TIMES
  if (!strncmp(name, "dbg_plan_", 9)) {   // diagnostic build: the plan word in memory and the geometry a k_jacobi_pair launch would expect
    unsigned long long v = 0;
    if (const int rc = read_back(h, &v, h->d_tbmask + 2 * TB_BANDS * (TB_COLS / 64), sizeof(v))) return rc;
    const TbPlan tp = L<double>::tb_plan(h, (int)(h->istep & 1), PlanFor::kJacobiPair);
    *value = !strcmp(name, "dbg_plan_word") ? (int64_t)v : !strcmp(name, "dbg_plan_waves") ? tp.waves : !strcmp(name, "dbg_plan_R") ? tp.R : tp.ntt;
    return VOF_OK;
  }
#endif
  if (!strcmp(name, "pair_launches")) {   // k_jacobi_pair launches replayed from batch graphs
    *value = h->pair_launches;
    return VOF_OK;
  }
  if (!strcmp(name, "tm_segments")) {   // row segments of the last k_tm launch enqueued (1: no tail; kernels/row_segments.h)
    *value = h->tm_segments_last;
    return VOF_OK;
  }
  if (!strcmp(name, "fzmap_flagged") || !strcmp(name, "fzmap_wrong")) {
    // k_tm's zero map of the current F, counted on demand (k_fzmap_check, kernels/fused_tm.h): the segments flagged, and those of
    // them whose cells are not all +0 bit for bit -- 0 unless the bookkeeping of runtime/state.h has a hole.  0 / 0 without maps.
    *value = 0;
    if (!h->fzmap_active) return VOF_OK;
    settle_ghosts(h);
    if (h->state.fzmap_stale) return VOF_OK;   // (the maps are cleared before they are looked at again: nothing is flagged)
    if (const int rc = h->buf.fzmap_cnt.reserve(h, 2 * sizeof(unsigned long long), "no memory for the zero-map counters")) return rc;
    unsigned long long v[2] = {0, 0};
    HIPCHK(h, hipMemsetAsync(h->buf.fzmap_cnt.p, 0, sizeof(v), h->stream));
    const int cur = (h->views.bits() & FieldViews::kF) ? 1 : 0;
    DISPATCH_T(h, L<double>::fzmap_check(h, cur), L<float>::fzmap_check(h, cur));
    if (const int rc = read_back(h, v, h->buf.fzmap_cnt.p, sizeof(v))) return rc;
    *value = (int64_t)v[!strcmp(name, "fzmap_wrong") ? 1 : 0];
    return ensure_ok(h);
  }
  if (!strcmp(name, "tm_chained_batches")) {   // k_tm batches that found the predictor of their first step in place
    *value = h->tm_chained;
    return VOF_OK;
  }
  if (!strcmp(name, "tm_steps")) {   // steps replayed from batch graphs in the k_tm form
    *value = h->tm_steps;
    return VOF_OK;
  }
  if (!strcmp(name, "tm_choice")) {   // -1: not decided (yet, or the knob decides), 0 / 1: the form the rule (fuse_tm = -1) or the timing (-2) chose
    *value = ((tm_auto(h) || tm_by_rule(h)) && h->tune.decided) ? h->tune.choice : -1;
    return VOF_OK;
  }
  if (!strcmp(name, "halves_steps")) {   // steps replayed from batch graphs in the two-chain form (enqueue_steps_halves)
    *value = h->halves_steps;
    return VOF_OK;
  }
  if (!strcmp(name, "exchange_graph_steps")) {  // steps vof_step_exchange replayed from a captured graph
    *value = h->xchg_graph_steps;
    return VOF_OK;
  }
  return fail(h, VOF_EINVAL, "unknown counter");
}

int vof_sync(vof2d_handle h) {
  if (!h) return VOF_EINVAL;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return ensure_ok(h);
}
int vof_timer_start(vof2d_handle h) {
  if (!h) return VOF_EINVAL;
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  return VOF_OK;
}
int vof_timer_stop(vof2d_handle h, float* ms) {
  if (!h || !ms) return VOF_EINVAL;
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  HIPCHK(h, hipEventSynchronize(h->ev1));
  HIPCHK(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
  return VOF_OK;
}
int vof_profile_steps(vof2d_handle h, int64_t nsteps) {
  if (!h) return VOF_EINVAL;
  if (nsteps < 0) return fail(h, VOF_EINVAL, "nsteps must be >= 0");
  if (const int rc = check_no_phased_step(h)) return rc;
  return profile_steps(h, nsteps);
}
int vof_get_profile(vof2d_handle h, const char* kernel, double* avg_us, int64_t* launches) {
  if (!h || !kernel) return VOF_EINVAL;
  for (int k = 0; k < NKERNELS; ++k)
    if (!strcmp(kernel, kKernelNames[k])) {
      if (avg_us) *avg_us = h->prof_cnt[k] ? 1e3 * h->prof_sum_ms[k] / (double)h->prof_cnt[k] : 0.0;
      if (launches) *launches = h->prof_cnt[k];
      return VOF_OK;
    }
  return fail(h, VOF_EINVAL, "unknown kernel name");
}
int vof_reset_profile(vof2d_handle h) {
  if (!h) return VOF_EINVAL;
  for (int k = 0; k < NKERNELS; ++k) { h->prof_sum_ms[k] = 0.0; h->prof_cnt[k] = 0; }
  return VOF_OK;
}
int vof_time_jacobi(vof2d_handle h, int32_t n, float* ms_per_sweep) {
  if (!h || !ms_per_sweep) return VOF_EINVAL;
  if (n < 2 || (n & 1)) return fail(h, VOF_EINVAL, "n must be even and >= 2");
  if (const int rc = check_no_phased_step(h)) return rc;
  // one hipEvent pair on the handle's stream around n back-to-back sweeps of the current rhs
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  DISPATCH_T(h, jacobi_n<double>(h, n, false), jacobi_n<float>(h, n, false));
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  HIPCHK(h, hipEventSynchronize(h->ev1));
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  *ms_per_sweep = ms / (float)n;
  return ensure_ok(h);
}
// ---- strips over RCCL: the per-step halo exchange without leaving the library
int vof_comm_get_unique_id(void* id) {
  if (!id) return VOF_EINVAL;
  Rccl* r = rccl();
  if (!r) return VOF_ESTATE;
  return r->GetUniqueId(id) == 0 ? VOF_OK : VOF_EHIP;
}
int vof_comm_init(vof2d_handle h, const void* id, int32_t rank, int32_t world, int32_t flags) {
  if (!h || !id || world < 1 || rank < 0 || rank >= world) return VOF_EINVAL;
  if (h->comm) return fail(h, VOF_ESTATE, "vof_comm_init: the handle already has a communicator");
  settle_ghosts(h);
  Rccl* r = rccl();
  if (!r) return fail(h, VOF_ESTATE, "RCCL (librccl.so.1) could not be loaded");
  const int W = VOF_HALO_ROWS(h->d.jacobi_iters);
  const bool lo = !h->g.wall_lo, hi = !h->g.wall_hi;  // interior edges
  const bool loop = (flags & VOF_COMM_LOOPBACK) != 0;
  if (lo && h->d.own_lo - W < h->d.row_lo) return fail(h, VOF_EINVAL, "fewer than VOF_HALO_ROWS rows stored below own_lo");
  if (hi && h->d.own_hi + W > h->d.row_hi) return fail(h, VOF_EINVAL, "fewer than VOF_HALO_ROWS rows stored above own_hi");
  if (h->d.own_hi - h->d.own_lo + 1 < W) return fail(h, VOF_EINVAL, "strip thinner than VOF_HALO_ROWS");
  if (!loop && ((lo && rank == 0) || (hi && rank == world - 1) || (!lo && rank != 0) || (!hi && rank != world - 1)))
    return fail(h, VOF_EINVAL, "rank does not match the strip: rank r of n owns the r-th row range from the left wall");
  HIPCHK(h, hipSetDevice(h->device));
  RcclId uid;
  memcpy(&uid, id, sizeof(uid));
  NCCLCHK(h, r->CommInitRank(&h->comm, world, uid, rank));
  HIPCHK(h, hipStreamCreateWithFlags(&h->cstream, hipStreamNonBlocking));
  HIPCHK(h, hipEventCreateWithFlags(&h->ev_ready, hipEventDisableTiming));
  HIPCHK(h, hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming));
  for (int k = 0; k < 3; ++k) HIPCHK(h, hipEventCreateWithFlags(&h->ev_fork[k], hipEventDisableTiming));
  // Capturing the send/recv groups into the step graph is verified with RCCL 2.27.7 (ROCm 7.2);
  // 2.26.6 (the copy bundled with PyTorch 2.10 + ROCm 7.0) crashes where the capture ends.
  h->xchg_graph = r->version >= 22707 ? 1 : 0;
  const char* ev = getenv("VOF2D_XCHG_GRAPH");
  if (ev) h->xchg_graph = atoi(ev);
  h->xchg_steps = 0;
  h->comm_rank = rank;
  h->comm_world = world;
  // loopback (self-test on one GPU): both neighbours are this rank; RCCL pairs the k-th send to a
  // peer with the k-th receive from it, so each halo receives the W owned rows next to it
  h->peer_lo = lo ? (loop ? rank : rank - 1) : -1;
  h->peer_hi = hi ? (loop ? rank : rank + 1) : -1;
  return VOF_OK;
}
int vof_comm_allreduce_max(vof2d_handle h, double* value) {
  if (!h || !value) return VOF_EINVAL;
  if (!h->comm) return fail(h, VOF_ESTATE, "vof_comm_init has not been called");
  Rccl* r = rccl();
  HIPCHK(h, hipSetDevice(h->device));
  if (const int rc = h->buf.red.reserve(h, sizeof(double), "vof_comm_allreduce_max: no memory for the scalar")) return rc;
  double* const red = h->buf.red.as<double>();
  // on the compute stream: ordered after everything enqueued so far, so it doubles as a barrier
  HIPCHK(h, hipMemcpyAsync(red, value, sizeof(double), hipMemcpyHostToDevice, h->stream));
  NCCLCHK(h, r->AllReduce(red, red, 1, /*ncclFloat64*/ 8, /*ncclMax*/ 2, h->comm, h->stream));
  return read_back(h, value, red, sizeof(double));
}
int vof_comm_info(vof2d_handle h, int32_t* rccl_version, int32_t* graph_capture) {
  if (!h) return VOF_EINVAL;
  Rccl* r = rccl();
  if (rccl_version) *rccl_version = r ? r->version : 0;
  if (graph_capture) *graph_capture = (h->comm && h->xchg_graph && !(h->d.flags & VOF_FLAG_NO_GRAPH)) ? 1 : 0;
  return VOF_OK;
}
int vof_comm_destroy(vof2d_handle h) {
  if (!h) return VOF_EINVAL;
  comm_teardown(h);
  return VOF_OK;
}
static unsigned field_mask_ok(uint32_t mask) { return mask != 0 && (mask & ~127u) == 0; }
int vof_comm_exchange(vof2d_handle h, uint32_t field_mask) {
  if (!h) return VOF_EINVAL;
  if (!h->comm) return fail(h, VOF_ESTATE, "vof_comm_init has not been called");
  if (!field_mask_ok(field_mask)) return fail(h, VOF_EINVAL, "field_mask: VOF_XCHG_F | _U | _V | _P | _US | _VS | _RHS");
  HIPCHK(h, hipSetDevice(h->device));
  settle_ghosts(h);
  int rc = comm_post(h, field_mask);
  return rc ? rc : comm_join(h);
}

int vof_step_tm_piece(vof2d_handle h, int32_t piece) {
  if (!h || piece < 0 || piece > 2) return VOF_EINVAL;
  if (const int rc = check_no_phased_step(h)) return rc;
  if (!mode5_ok(h)) return fail(h, VOF_ESTATE, "the pair kernels need the fused transport and five-sweep Jacobi launches");
  if (!clean_ghosts(h->state)) return fail(h, VOF_ESTATE, "the first step after set_init_F / set_field runs through vof_step");
  (void)settle_ahead(h);   // (a full domain that ran chained k_tm batches: its u*, v*, rhs are the last step's from here on)
  if (piece != 0) step_wrote_F(h->state);
  if (piece == 0) {
    DISPATCH_T(h, tm5_head<double>(h), tm5_head<float>(h));
  } else if (piece == 1) {
    h->istep += 1;
    DISPATCH_T(h, (tm5_jacobi<double>(h, (int)(h->istep & 1)), tm5_tm<double>(h, h->istep, 0)), (tm5_jacobi<float>(h, (int)(h->istep & 1)), tm5_tm<float>(h, h->istep, 0)));
    h->views.swap_F();
    h->views.swap_S();
  } else {
    h->istep += 1;
    const bool y_first = (h->istep % 2 == 0);
    DISPATCH_T(h, (jacobi_n<double>(h, h->d.jacobi_iters, false, -1), transport_part<double>(h, y_first, kAllOwned)),
               (jacobi_n<float>(h, h->d.jacobi_iters, false, -1), transport_part<float>(h, y_first, kAllOwned)));
    h->views.swap_F();
    if (!h->virtual_ghosts) DISPATCH_T(h, L<double>::set_bc<BC_ALL>(h), L<float>::set_bc<BC_ALL>(h));
  }
  finish_step(h->state, strip_step_plan(h, true));   // (nothing was dirty: refused above)
  return ensure_ok(h);
}
int vof_step_exchange(vof2d_handle h, int64_t nsteps, int32_t overlap) {
  if (!h || nsteps < 0 || overlap < 0 || overlap > 5 || overlap == 2) return VOF_EINVAL;   // (2 was retired: never worth it)
  if (!h->comm) return fail(h, VOF_ESTATE, "vof_comm_init has not been called");
  if (const int rc = check_no_phased_step(h)) return rc;
  step_wrote_F(h->state);
  HIPCHK(h, hipSetDevice(h->device));
  (void)settle_ahead(h);   // (see vof_step_tm_piece)
  return overlap == 5 ? step_exchange_mode5(h, nsteps) : step_exchange(h, nsteps, overlap);
}

int vof_selftest_division(int32_t dtype, int64_t n, uint64_t seed, void* a_out, void* b_out, void* q_out) {
  if (!a_out || !b_out || !q_out || n < 1 || (dtype != VOF_F64 && dtype != VOF_F32)) return VOF_EINVAL;
  const size_t bytes = (size_t)n * (dtype == VOF_F64 ? 8 : 4);
  char* dev = nullptr;
  if (hipMalloc(&dev, 3 * bytes) != hipSuccess) { (void)hipGetLastError(); return VOF_ENOMEM; }
  const unsigned blocks = (unsigned)((n + 255) / 256);
  if (dtype == VOF_F64)
    hipLaunchKernelGGL(k_selftest_division<double>, dim3(blocks), dim3(256), 0, 0, seed, n, (double*)dev,
                       (double*)(dev + bytes), (double*)(dev + 2 * bytes));
  else
    hipLaunchKernelGGL(k_selftest_division<float>, dim3(blocks), dim3(256), 0, 0, seed, n, (float*)dev,
                       (float*)(dev + bytes), (float*)(dev + 2 * bytes));
  hipError_t e = hipMemcpy(a_out, dev, bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(b_out, dev + bytes, bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(q_out, dev + 2 * bytes, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(dev);
  return e == hipSuccess ? VOF_OK : VOF_EHIP;
}
const char* vof_last_error(vof2d_handle h) { return h ? h->err : "null handle"; }
const char* vof_backend(void) { return "hip-gfx950"; }

}  // extern "C"
