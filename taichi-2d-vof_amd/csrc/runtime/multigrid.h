// runtime/multigrid.h -- the work arrays of vof_solve_p_cg, the hierarchy of vof_solve_p_mg, one V-cycle (enqueued, or captured once and
// replayed), the driver loop of both solves
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
#pragma once
#include "schedule.h"

namespace {

// The work arrays, reduction buffer and device scalars of vof_solve_p_cg, allocated by the first call of either solver:
// the checks of vof_solve_p_mg run the same residual kernel into the same scalars.
int cg_prepare(vof2d_ctx* h) {
  if (h->buf.cg_part.p) return VOF_OK;
  const size_t nblocks = blocks_rows(interior_rows(h), h->g.ntj, 1);   // (the most blocks a launch can have: one-row chunks, knob "rows_per_wave")
  const CgCarve c = carve_cg(h->field_elems * h->esz, nblocks * kCgPart, CG_NSCAL);
  // zeroed: cells outside the interior are never written again, they stay 0 (kernels/cg.h, k_cg_apply)
  int rc = h->buf.cg_fields.reserve(h, c.fields_total, "vof_solve_p_cg: no memory for the work arrays", true);
  if (rc) return rc;
  if ((rc = h->buf.cg_part.reserve(h, c.part_total, "vof_solve_p_cg: no memory for the reduction buffer", true))) return rc;
  for (int k = 0; k < 4; ++k) h->cg_fld[k] = h->buf.cg_fields.as<char>(c.fld[k]);
  h->cg_part = h->buf.cg_part.as<double>();
  h->cg_sc = h->buf.cg_part.as<double>(c.sc);
  return VOF_OK;
}

constexpr double kMgCoarseReduction = 1e-2;   // the coarsest-level solve ends at this fraction of its starting max|z| ...
inline int mg_coarse_cap(const Geom& g) { return 4 * (g.nx > g.ny ? g.nx : g.ny); }   // ... or after this many iterations

// Level l >= 1: nx / 2^l x ny / 2^l cells in a pitched layout built like the fields' (vof_create): interior column 1 on a
// 128-byte boundary, the pitch a multiple of 128 bytes with room for a whole wave tile right of ny.
Geom mg_level_geom(const vof2d_ctx* h, int nx, int ny) {
  Geom g{};
  const int W = 64 * h->V, align = 128 / (int)h->esz;
  g.nx = nx; g.ny = ny; g.row_lo = 0; g.row_hi = nx + 1; g.ilo = 1; g.ihi = nx; g.own_lo = 1; g.own_hi = nx;
  g.wall_lo = g.wall_hi = 1;
  g.ntj = (ny + W - 1) / W;
  g.col0 = align - 1;
  g.pitch = ((g.col0 + (long)ny + W + 16 + 1 + align - 1) / align) * align;
  return g;
}

// Coarsen while both extents are even and the coarser level keeps at least 4 cells each way.  Allocated once, as deep as
// the rule allows; the work arrays of the coarsest-level solve are sized for level 1, the largest level a cycle of two or
// more levels can end on (a one-level cycle solves on the grid itself, with the arrays of vof_solve_p_cg).
int mg_prepare(vof2d_ctx* h) {
  if (!h->mg_lv.empty()) return VOF_OK;
  std::vector<MgLevel> lv;
  MgLevel l0{};
  l0.g = h->g; l0.scale = 1.0; l0.bytes = h->field_elems * h->esz;
  lv.push_back(l0);
  const size_t align = 128 / h->esz;
  std::vector<size_t> bytes{l0.bytes};
  for (;;) {
    const MgLevel& f = lv.back();
    if (f.g.nx % 2 || f.g.ny % 2 || f.g.nx / 2 < 4 || f.g.ny / 2 < 4) break;
    MgLevel c{};
    c.g = mg_level_geom(h, f.g.nx / 2, f.g.ny / 2);
    c.scale = f.scale * 0.25;
    c.bytes = ((size_t)(c.g.nx + 2) * (size_t)c.g.pitch + align) * h->esz;
    bytes.push_back(c.bytes);
    lv.push_back(c);
  }
  if (lv.size() > 1) {
    const MgCarve c = carve_mg(bytes, CG_NSCAL);
    DevBuf& arena = h->buf.mg_arena;
    // zeroed: cells outside a level's interior are never written, they stay 0
    if (const int rc = arena.reserve(h, c.total, "vof_solve_p_mg: no memory for the coarser levels", true)) return rc;
    for (size_t l = 1; l < lv.size(); ++l) {
      lv[l].e[0] = arena.as<char>(c.level[l][0]); lv[l].e[1] = arena.as<char>(c.level[l][1]); lv[l].f = arena.as<char>(c.level[l][2]);
    }
    for (int k = 0; k < 4; ++k) h->mg_cgw[k] = arena.as<char>(c.cgw[k]);
    h->mg_sc = arena.as<double>(c.sc);
  }
  h->mg_lv.swap(lv);
  return VOF_OK;
}

inline int mg_depth(const vof2d_ctx* h) {
  const int all = (int)h->mg_lv.size();
  return h->mg_levels >= 1 && h->mg_levels < all ? h->mg_levels : all;
}

// Knob "mg_coarse_block": the coarsest level a cycle of this handle ends on -- by the rule of mg_prepare and the cap of
// knob "mg_levels", from the extents alone: vof_get_param may ask before the hierarchy exists -- and whether its solve
// runs as one workgroup (k_mg_coarse_block: the level with its ghost ring fits kMgBlockCells)
inline void mg_coarsest_extents(const vof2d_ctx* h, int& nx, int& ny) {
  nx = h->g.nx; ny = h->g.ny;
  for (int l = 1; (h->mg_levels < 1 || l < h->mg_levels) && !(nx % 2 || ny % 2 || nx / 2 < 4 || ny / 2 < 4); ++l) { nx /= 2; ny /= 2; }
}
inline bool mg_block_in_effect(const vof2d_ctx* h) {
  if (!h->mg_coarse_block || !(h->g.wall_lo && h->g.wall_hi)) return false;
  int nx, ny;
  mg_coarsest_extents(h, nx, ny);
  return (nx + 2) * (ny + 2) <= kMgBlockCells;
}

// One V(nu, nu) cycle on h->stream, a straight line of launches.  Every level's sweeps ping-pong between two arrays (p and
// pt on level 0): nu sweeps down, the correction added in place, nu sweeps up -- 2 nu in all, so e is back where it was.
template <typename T>
void mg_enqueue_cycle(vof2d_ctx* h) {
  using K = L<T>;
  const int last = mg_depth(h) - 1, nu = h->mg_nu < 1 ? 1 : h->mg_nu;
  std::vector<MgLevel>& lv = h->mg_lv;
  lv[0].e[0] = h->fld[fP]; lv[0].e[1] = h->fld[fPT]; lv[0].f = h->fld[fRHS];
  auto E = [&](int l, int k) { return reinterpret_cast<T*>(lv[l].e[k]); };
  auto F = [&](int l) { return reinterpret_cast<const T*>(lv[l].f); };
  auto sc = [&](int l) { return l == 0 ? (const double*)h->cg_sc : (const double*)nullptr; };
  auto sweeps = [&](int l, int from) {
    for (int k = 0; k < nu; ++k) K::mg_smooth(h, lv[l], E(l, (from + k) & 1), F(l), E(l, (from + k + 1) & 1), sc(l));
  };
  for (int l = 0; l < last; ++l) {
    sweeps(l, 0);
    K::mg_restrict(h, lv[l], lv[l + 1], E(l, nu & 1), F(l), reinterpret_cast<T*>(lv[l + 1].f), E(l + 1, 0), sc(l));
  }
  if (mg_block_in_effect(h))
    K::mg_coarse_block(h, lv[last], E(last, 0), F(last), sc(last), mg_coarse_cap(lv[last].g), kMgCoarseReduction);
  else if (last == 0)
    K::mg_coarse_solve(h, lv[0], E(0, 0), F(0), h->cg_fld, h->cg_sc, false, mg_coarse_cap(lv[0].g), kMgCoarseReduction);
  else
    K::mg_coarse_solve(h, lv[last], E(last, 0), F(last), h->mg_cgw, h->mg_sc, true, mg_coarse_cap(lv[last].g), kMgCoarseReduction);
  for (int l = last - 1; l >= 0; --l) {
    K::mg_prolong(h, lv[l], lv[l + 1], E(l + 1, 0), E(l, nu & 1));
    sweeps(l, nu & 1);
  }
}

// The pressure solve of a vof_step_mg step, enqueued on h->stream (eagerly, or inside the capture of the step): what
// vof_solve_p_mg(tol = -1, max_cycles = check_every = cycles, build_rhs = 1) runs behind the rhs the step's k_momentum
// has formed -- the clean direction arrays (the part of them the coarsest level reads; the block kernel reads none), the
// drift constant, the cycles, the residual -- minus the residual in front (nobody would read it) and every host wait,
// plus the record.  The caller has run cg_prepare and mg_prepare and holds the record (buf.mg_rec).
template <typename T>
void mg_enqueue_step_solve(vof2d_ctx* h, int cycles, int criterion) {
  if (!mg_block_in_effect(h)) {
    if (mg_depth(h) == 1) (void)hipMemsetAsync(h->cg_fld[1], 0, 2 * h->field_elems * h->esz, h->stream);
    else
      for (int k = 1; k <= 2; ++k) (void)hipMemsetAsync(h->mg_cgw[k], 0, h->mg_lv[mg_depth(h) - 1].bytes, h->stream);
  }
  L<T>::cg_drift(h, L<T>::cg_sum_ap(h));
  for (int k = 0; k < cycles; ++k) mg_enqueue_cycle<T>(h);
  L<T>::cg_residual(h, 1);
  launch_block(h, kOther, k_mg_step_record, dim3(1), 64u, 0, (const double*)h->cg_sc, h->buf.mg_rec.as<double>(), criterion);
}

// n cycles: replays of the one captured cycle (a cycle at 1024^2 is some hundred small launches), or the launches themselves
int mg_cycles(vof2d_ctx* h, int n) {
  if (!h->mg_graph) {
    for (int k = 0; k < n; ++k) DISPATCH_T(h, mg_enqueue_cycle<double>(h), mg_enqueue_cycle<float>(h));
    return ensure_ok(h);
  }
  hipGraphExec_t& exec = h->graphs.slot(graph_key(h, gMg));   // (a graph bakes its pointers in, and the views move: the key)
  int rc;
  if (!exec && (rc = capture_or_fail(h, true, &exec, "the multigrid cycle", [&] { DISPATCH_T(h, mg_enqueue_cycle<double>(h), mg_enqueue_cycle<float>(h)); })))
    return rc;
  for (int k = 0; k < n; ++k) HIPCHK(h, hipGraphLaunch(exec, h->stream));
  return VOF_OK;
}

// The driver loop of vof_solve_p_cg and vof_solve_p_mg, behind their prologues (the first residual is enqueued): read the
// scalars; stop at the tolerance, at a non-finite field, at the cap (where `stop_ends`: at a direction with nothing to
// divide by, CG_STOP, too: reported as it is); advance(n) enqueues n more iterations or cycles; the residual again
// (restart: the argument of cg_residual).
template <typename Advance>
int solve_loop(vof2d_ctx* h, double tol, int max_iters, int check_every, int criterion, bool stop_ends, int restart, Advance advance,
               int32_t* iters_done, double* residual, double* drift) {
  int done = 0, rc;
  double r = 0.0, sc[CG_NSCAL];
  for (;;) {
    if ((rc = ensure_ok(h)) || (rc = read_back(h, sc, h->cg_sc, sizeof(sc)))) return rc;
    r = vof_residual_value(sc[CG_MAXZ], sc[CG_MAXP], criterion);
    if (r <= tol || !(r < HUGE_VAL)) break;   // converged, or a non-finite field
    if (done >= max_iters || (stop_ends && sc[CG_STOP] != 0.0)) break;
    const int n = check_every < max_iters - done ? check_every : max_iters - done;
    if ((rc = advance(n))) return rc;
    done += n;
    DISPATCH_T(h, L<double>::cg_residual(h, restart), L<float>::cg_residual(h, restart));
  }
  *iters_done = done;
  *residual = r;
  *drift = sc[CG_C];
  return VOF_OK;
}
// what both solves start with, behind their clean direction arrays: the drift constant and the first residual
void solve_prologue(vof2d_ctx* h) {
  const double sum_ap = DISPATCH_B(h, L<double>::cg_sum_ap(h), L<float>::cg_sum_ap(h));
  DISPATCH_T(h, (L<double>::cg_drift(h, sum_ap), L<double>::cg_residual(h, 1)), (L<float>::cg_drift(h, sum_ap), L<float>::cg_residual(h, 1)));
}

// The driver of vof_solve_p_cg (arguments checked by the entry point)
int cg_solve(vof2d_ctx* h, double tol, int max_iters, int check_every, int criterion, int build_rhs, int32_t* iters_done,
             double* residual, double* drift) {
  if (const int rc = cg_prepare(h)) return rc;
  if (build_rhs) DISPATCH_T(h, L<double>::rhs<false>(h), L<float>::rhs<false>(h));
  // a new solve starts from the steepest-descent direction: beta = 0 and a clean direction array
  HIPCHK(h, hipMemsetAsync(h->cg_fld[1], 0, 2 * h->field_elems * h->esz, h->stream));
  solve_prologue(h);
  auto advance = [h](int n) {
    for (int k = 0; k < n; ++k) DISPATCH_T(h, L<double>::cg_iteration(h), L<float>::cg_iteration(h));
    return (int)VOF_OK;
  };
  return solve_loop(h, tol, max_iters, check_every, criterion, true, 0, advance, iters_done, residual, drift);
}

// The driver of vof_solve_p_mg (arguments checked by the entry point): c, then check / cycles / check ... as vof_solve_p_cg
int mg_solve(vof2d_ctx* h, double tol, int max_cycles, int check_every, int criterion, int build_rhs, int32_t* cycles_done,
             double* residual, double* drift) {
  int rc = cg_prepare(h);      // (the residual of the checks, the reduction buffer and the scalars are the CG verb's)
  if (rc) return rc;
  if ((rc = mg_prepare(h))) return rc;
  if (build_rhs) DISPATCH_T(h, L<double>::rhs<false>(h), L<float>::rhs<false>(h));
  // the coarsest-level solve starts every time from beta = 0 times the old direction: that array must be finite
  if (mg_depth(h) == 1) HIPCHK(h, hipMemsetAsync(h->cg_fld[1], 0, 2 * h->field_elems * h->esz, h->stream));
  else HIPCHK(h, hipMemsetAsync(h->mg_cgw[1], 0, 2 * h->mg_lv[1].bytes, h->stream));
  solve_prologue(h);
  return solve_loop(h, tol, max_cycles, check_every, criterion, false, 1, [h](int n) { return mg_cycles(h, n); }, cycles_done, residual, drift);
}

}  // namespace
