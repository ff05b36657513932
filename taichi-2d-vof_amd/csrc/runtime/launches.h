// runtime/launches.h -- chunk-length heuristics and L<T>: one launch wrapper per kernel (grid shape, chunk length, arguments), through the single launch() helper
//
// Part of the host-side runtime of libvof2d_hip.so; included (once, in this order) by vof2d_api.hip:
// context.h (with state.h), launches.h, schedule.h, comm.h, selftest.h.  Everything here has internal linkage.
#pragma once
#include "context.h"

namespace {

// ------------------------------------------------------------------ chunk lengths (launch geometry)
// Rows per wave chunk.  Every marching kernel trades lead-in / halo rows per chunk (re-read from
// HBM by the vertical neighbour) against the number of waves.  Two effects decide:
//  * residency rounds: a launch whose waves exceed what the chip holds at once (occupancy x 1024
//    SIMDs) by a little runs a nearly empty extra round (measured on k_jacobi_tb at 4096^2: 3010
//    waves 116 us, 3080 waves 158 us), so the chunk length is chosen to make the launch k full
//    rounds, k as small as the maximum chunk length allows;
//  * with few cells the critical path of one wave dominates, so chunks never exceed what keeps
//    one round's worth of waves busy (short chunks on small grids).
// Occupancy comes from the runtime's query for the actual kernel (it depends on the compiled
// register count); a 5 % margin absorbs the over-reporting noted in MI355X_MICROARCH.md.
// Used for the two register-heavy, long-lived-wave kernels (k_jacobi_tb: -15 us per step at
// 4096^2, k_momentum: -3 us); the HBM-bound kernels with short-lived waves measured best with the
// plain cells-per-wave rule (chunk_rows) and keep it.
// What the chip holds of `kernel` at once, in the unit its launch is counted in (cached per handle; one host thread per
// handle): waves of the kernels with blocks of four waves (256 threads; 8 blocks, 32 waves, per CU at most), blocks of
// the pair kernels (128 threads).  Without an answer from the runtime: three waves per SIMD / six pairs per CU of 256 CUs.
template <typename K>
long resident(vof2d_ctx* h, K kernel, int threads) {
  std::map<const void*, long>& cache = h->occ_cache;
  const void* key = reinterpret_cast<const void*>(kernel);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  const bool pairs = threads == 128;
  int blocks_per_cu = 0;
  long cap = pairs ? 6L * 256 : 3L * 256 * 4;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, kernel, threads, 0) == hipSuccess && blocks_per_cu > 0) {
    int cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    if (!pairs && blocks_per_cu > 8) blocks_per_cu = 8;
    cap = (long)blocks_per_cu * cus * (pairs ? 1 : 4);
  } else {
    (void)hipGetLastError();
  }
  cache[key] = cap;
  return cap;
}
inline int interior_rows(const vof2d_ctx* h) { return h->g.ihi - h->g.ilo + 1; }
int chunk_rows_fit(const vof2d_ctx* h, int ntiles, long capacity, int rmin, int rmax) {
  const long rows = interior_rows(h);
  const long cap = capacity * 95 / 100;
  int R_out = rmin;
  for (int k = 1; k <= 64; ++k) {
    long chunks_max = k * cap / ntiles;
    if (chunks_max < 1) continue;
    long R = (rows + chunks_max - 1) / chunks_max;
    if (R <= rmax) { R_out = (int)(R < rmin ? rmin : R); break; }
  }
  if (getenv("VOF2D_DEBUG"))
    fprintf(stderr, "[vof2d] chunk_rows_fit: rows=%ld tiles=%d capacity=%ld -> R=%d (%ld waves)\n", rows, ntiles,
            capacity, R_out, ((rows + R_out - 1) / R_out) * ntiles);
  return R_out;
}
// cells-per-wave rule (~4096 waves, chunk length a power of two), used by the x sweep, whose 6
// lead-in rows per chunk want long chunks (16 rows at 4096^2: 143 us; 8 rows 157 us, 4 rows 200 us)
int chunk_rows(const vof2d_ctx* h, int ntiles, int rmin, int rmax) {
  const long rows = interior_rows(h);
  long R = rows * ntiles / 4096;
  if (R < rmin) R = rmin;
  if (R > rmax) R = rmax;
  long P = 1;
  while (P * 2 <= R) P *= 2;
  return (int)(P < rmin ? rmin : P);
}
// The streaming kernels with at most one halo row per side (single-sweep Jacobi, y sweep, the
// per-verb kernels): very short chunks.  With the nontemporal hints on their single-use streams the
// halo rows of vertically adjacent chunks -- consecutive blocks, resident at the same time -- are
// L2 hits, and many short-lived waves balance better than few long ones: k_jacobi at 4096^2 fp64
// 64 us with 2-row chunks (1 row 72 us, 4 rows 65 us, 8 rows 69 us, 32 rows 73.5 us); y sweep 112 us
// with 1 row, 116 us with 2, 136 us with 16.
int pick_rows(const vof2d_ctx* h, int ntiles) {
  (void)ntiles;
  if (h->rows_override > 0) return h->rows_override;
  return 2;
}
inline unsigned blocks_rows(int rows, int ntiles, int R) {
  const long waves = (long)((rows + R - 1) / R) * ntiles;
  return (unsigned)((waves + 3) / 4);
}
// Runtime flags as template arguments: f(std::bool_constant<flags>...).  A launch whose kernel comes in several
// instantiations (store form, sweep order, ...) is written once, in a generic lambda.
template <typename F>
void dispatch(F&& f) { f(); }
template <typename F, typename... Flags>
void dispatch(F&& f, bool flag, Flags... flags) {
  if (flag) dispatch([&](auto... rest) { f(std::true_type{}, rest...); }, flags...);
  else dispatch([&](auto... rest) { f(std::false_type{}, rest...); }, flags...);
}

// The BS form of k_momentum (range-checked buffer stores, see store_buf_nt): a lane's V columns must be stored or
// skipped together (tiles start on odd columns, so ny must be even) and a field must fit the 32-bit byte offsets of
// a buffer instruction.  Everything else takes the form with exec-masked global stores.  (k_transport -- which moves
// its L2-miss traffic at 5.6 TB/s either way -- gained nothing from the same change and keeps its global stores.)
inline bool buffer_stores_ok(const vof2d_ctx* h) {
  return h->buf_stores && (h->g.ny % 2 == 0) && (size_t)h->field_elems * h->esz < ((size_t)1 << 31) - (1u << 20);
}

// k_tm's zero maps (kernels/fused_tm.h): knob "f_zero_map" 1: wherever allowed -- a full domain without a communicator whose k_tm
// runs the buffer-store form --, 0: never, -1 (the default): where allowed AND it was measured to pay: the share of exact-zero cells
// the batch-form rule counted is at least kTmGasShare (4096^2 rising bubble, 2 % gas: every row pays for its flags and next to none
// is skipped, + 1.3 %) on a grid of kTmAlwaysCells or more (4096^2 dam-break - 4.3 %, 8192^2 - 8.4 %; 2048^2, whose F and twin stay
// in the last-level cache, + 0.8 %: profiles/f_zero_map_ab.txt).  What a handle's batch graphs were captured with is h->fzmap_active
// (fzmap_prepare, runtime/schedule.h).
constexpr double kTmGasShare = 0.5;   // k_tm from this share of exact-zero cells of F on (tm_choice_by_rule, runtime/schedule.h)
constexpr long kTmAlwaysCells = 16000000L;   // ... and whatever F holds from this many cells on (the measurements behind it: "launches" below)
// (a handle that gave out a pointer to F or its twin, vof_field_view, keeps none: a write through the pointer cannot be seen)
inline size_t fzmap_bytes(const vof2d_ctx* h) {   // of one map: (nx + 2) rows of tiles + 2 words -- the marches request the words of one row past the last they load
  const int ntf = h->d.dtype == VOF_F64 ? TmGeom<VecWidth<double>::V>::tiles(h->g.ny) : TmGeom<VecWidth<float>::V>::tiles(h->g.ny);
  return (size_t)(h->g.nx + 2) * (size_t)(ntf + 2) * sizeof(unsigned);
}
// the allocation: four rows of padding (the march's one load reaches four rows back from a destination word), the map of the F array, the map of its twin
inline size_t fzmap_pad(const vof2d_ctx* h) { return fzmap_bytes(h) / (size_t)(h->g.nx + 2) * 4; }
inline size_t fzmap_offset(const vof2d_ctx* h, int array) { return fzmap_pad(h) + (size_t)array * fzmap_bytes(h); }
inline size_t fzmap_alloc_bytes(const vof2d_ctx* h) { return fzmap_offset(h, 2); }
inline bool fzmap_allowed(const vof2d_ctx* h) {
  if (h->f_view_given || fzmap_alloc_bytes(h) >= ((size_t)1 << 30)) return false;
  if (h->f_zero_map == 0 || !(h->g.wall_lo && h->g.wall_hi) || h->comm || !buffer_stores_ok(h) || !(h->buf_stores & 4)) return false;
  return h->f_zero_map > 0 || (h->gas_share >= kTmGasShare && (long)(h->g.ihi - h->g.ilo + 1) * h->g.ny >= kTmAlwaysCells);
}

// ------------------------------------------------------------------ launches
// kTmAlwaysCells (above, beside the zero maps' rule): from this many cells on a full domain runs the pair kernels whatever it holds (the rule of vof_step, runtime/schedule.h).  Re-measured
// with the kernels of round 6 (profiles/r06_forms_sweep.txt, ms/step pairs / chains on the rising bubble, 2 % gas): fp64 2048^2 0.253 / 0.227,
// 2560^2 0.325 / 0.312, 3072^2 0.405 / 0.411, 4096^2 0.592 / 0.614; fp32 2560^2 0.199 / 0.190, 3072^2 0.246 / 0.243, 4096^2 0.352 / 0.365
// (round 5, before the branch-free division tier: ties at 4096^2, hence 20 M then); 5120^2 0.78-0.83 / 0.89-0.92, 8192^2 1.67-1.71 / 2.17-2.20
constexpr long kTbPlanWaves = 16384;   // waves of a k_jacobi_tb launch the work plan can describe
// which kernel a work plan is for: the step's Jacobi launches are k_jacobi_tb's, or (the k_tm forms where the handle allows:
// jacobi_pair_ok) k_jacobi_pair's -- the tile columns, chunk lengths and wave counts differ (L<T>::tb_plan)
enum class PlanFor { kJacobiTb, kJacobiPair };
enum KernelId { kMomentum = 0, kSetBC, kJacobi, kJacobiTB, kCorrect, kFctX, kFctY, kNormals, kKappa, kPredictor,
                kRhs, kOther, kTransport, kJacobiPair, kTM, kTMUV, kCgApply, kCgUpdate, kCgResidual, kCgFinish, kMgSmooth, kMgRestrict, kMgProlong, kMgCoarseBlock, NKERNELS };
static_assert(NKERNELS <= 24, "vof2d_ctx::prof_sum_ms / prof_cnt");
const char* const kKernelNames[NKERNELS] = {"k_momentum", "k_set_bc", "k_jacobi", "k_jacobi_tb", "k_correct",
                                            "k_fct_x", "k_fct_y", "k_normals", "k_kappa", "k_predictor", "k_rhs",
                                            "other", "k_transport", "k_jacobi_pair", "k_tm", "k_tm_uv",
                                            "k_cg_apply", "k_cg_update", "k_cg_residual", "k_cg_finish",
                                            "k_mg_smooth", "k_mg_restrict", "k_mg_prolong", "k_mg_coarse_block"};   // (k_tm_uv: the k_tm launch that also stores u, v -- the last of a batch)

// One place through which every kernel is launched.  In profiling mode the dispatch carries its
// own start/stop events (hipExtLaunchKernelGGL: the begin/end timestamps of the dispatch itself,
// no extra barrier packets), otherwise it is a plain launch.
template <typename... KArgs, typename... Args>
void launch_block(vof2d_ctx* h, int kid, void (*kernel)(KArgs...), dim3 grid, unsigned threads, size_t lds, Args... args) {
  if (h->timed >= 0 && h->timed < vof2d_ctx::kMaxTimed) {
    const int k = h->timed++;
    h->tkid[k] = kid;
    hipExtLaunchKernelGGL(kernel, grid, dim3(threads), lds, h->stream, h->tev[2 * k], h->tev[2 * k + 1], 0, args...);
  } else {
    hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, h->stream, args...);
  }
}
// (blocks of four waves -- four adjacent tiles -- for every kernel but k_tm, whose block is a pair of waves)
template <typename... KArgs, typename... Args>
void launch(vof2d_ctx* h, int kid, void (*kernel)(KArgs...), dim3 grid, size_t lds, Args... args) {
  launch_block(h, kid, kernel, grid, 256u, lds, args...);
}

template <typename T>
struct L {
  static constexpr int V = VecWidth<T>::V;
  static Consts<T> C(vof2d_ctx* h) { return round_consts<T>(h->cd); }

  static void init_F(vof2d_ctx* h, int ic) {
    dim3 grid((h->g.ny + 2 + 255) / 256, h->g.row_hi - h->g.row_lo + 1);
    launch(h, kOther, k_init_F<T>, grid, 0, h->g, C(h), F_<T>(h, fF), F_<T>(h, fF2), ic, h->d.Lx, h->d.Ly,
           (int)(h->d.coord_cast_f32 || h->d.dtype == VOF_F32));
  }
  // own_rows_only: the row loop skips the halo rows of a strip (wall ghost rows are never halo)
  template <int MASK>
  static void set_bc(vof2d_ctx* h, bool own_rows_only = false) {
    const int nr = h->g.row_hi - h->g.row_lo + 1;
    const int n = nr > h->g.ny + 2 ? nr : h->g.ny + 2;
    const int r0 = (own_rows_only && !h->g.wall_lo) ? h->d.own_lo : h->d.row_lo;
    const int r1 = (own_rows_only && !h->g.wall_hi) ? h->d.own_hi : h->d.row_hi;
    launch(h, kSetBC, k_set_bc<T, MASK>, dim3((n + 255) / 256), 0, h->g, F_<T>(h, fU), F_<T>(h, fV), F_<T>(h, fF),
           F_<T>(h, fF2), F_<T>(h, fP), F_<T>(h, fRHO), r0, r1);
  }
  static void bc_F_cols(vof2d_ctx* h, T* F, int r0, int r1) {
    if (r1 < r0) return;
    launch(h, kSetBC, k_bc_F_cols<T>, dim3((r1 - r0 + 256) / 256), 0, h->g, F, r0, r1);
  }
  static void nu_rho(vof2d_ctx* h) {
    dim3 grid((h->g.ny + 2 + 255) / 256, h->g.row_hi - h->g.row_lo + 1);
    launch(h, kOther, k_nu_rho<T>, grid, 0, h->g, C(h), (const T*)F_<T>(h, fF), F_<T>(h, fRHO), F_<T>(h, fNU));
  }
  // (a, a2: another pair in the fields' layout in the place of F and its twin -- the dye, runtime/dye.h)
  static void post(vof2d_ctx* h, T* a = nullptr, T* a2 = nullptr) {
    dim3 grid((h->g.ny + 2 + 255) / 256, h->g.row_hi - h->g.row_lo + 1);
    launch(h, kOther, k_post<T>, grid, 0, h->g, a ? a : F_<T>(h, fF), a ? a2 : F_<T>(h, fF2));
  }
  // the F lines of set_BC (2dvof.py:168, 174, 181, 187) on such a pair, all stored rows of a full domain
  static void bc_F_pair(vof2d_ctx* h, T* a, T* a2) {
    const int nr = h->g.row_hi - h->g.row_lo + 1;
    const int n = nr > h->g.ny + 2 ? nr : h->g.ny + 2;
    launch(h, kSetBC, k_set_bc<T, BC_F>, dim3((n + 255) / 256), 0, h->g, F_<T>(h, fU), F_<T>(h, fV), a, a2, F_<T>(h, fP), F_<T>(h, fRHO), h->d.row_lo, h->d.row_hi);
  }
  static void normals(vof2d_ctx* h) {
    const int R = pick_rows(h, h->g.ntj);
    launch(h, kNormals, k_normals<T, V>, dim3(blocks_rows(interior_rows(h), h->g.ntj, R)), 0, h->g, C(h), (const T*)F_<T>(h, fF),
           F_<T>(h, fMX), F_<T>(h, fMY), R);
  }
  static void kappa(vof2d_ctx* h) {
    const int R = pick_rows(h, h->g.ntj);
    launch(h, kKappa, k_kappa<T, V>, dim3(blocks_rows(interior_rows(h), h->g.ntj, R)), 0, h->g, C(h), (const T*)F_<T>(h, fMX),
           (const T*)F_<T>(h, fMY), F_<T>(h, fKAPPA), R);
  }
  template <bool STORED>
  static void predictor(vof2d_ctx* h) {
    const int R = pick_rows(h, h->g.ntj);
    launch(h, kPredictor, k_predictor<T, V, STORED>, dim3(blocks_rows(interior_rows(h), h->g.ntj, R)), 0, h->g, C(h),
           (const T*)F_<T>(h, fU), (const T*)F_<T>(h, fV), (const T*)F_<T>(h, fKAPPA), (const T*)F_<T>(h, fF),
           (const T*)F_<T>(h, fRHO), (const T*)F_<T>(h, fNU), F_<T>(h, fUS), F_<T>(h, fVS), R);
  }
  // fused normals + kappa + predictor + rhs (vof_step only)
  // rows [first, last] of the predictor and the rhs (last < first: all computable rows)
  // plan_for: the kernel the step's Jacobi launches are (the planner block plans its geometry)
  static void momentum(vof2d_ctx* h, bool virt, int adapt_par, PlanFor plan_for, int first = 1, int last = 0) {
    const int ntt = MomentumGeom<V>::tiles(h->g.ny);
    if (last < first) { first = h->g.ilo; last = h->g.ihi; }
    const TbPlan tp = tb_plan(h, adapt_par, plan_for);   // (one extra block: the planner wave)
    dispatch([&](auto BS) {
      // one residency round while that keeps the chunks short (strips, small grids); on large grids
      // several rounds of 14-row chunks beat one round of long ones (4096^2: 184 vs 195 us, 8192^2:
      // 665 vs 758 us) -- the halo rows of adjacent, simultaneously resident chunks are L2 hits
      int R = h->mom_rows > 0 ? h->mom_rows : chunk_rows_fit(h, ntt, resident(h, k_momentum<T, V, BS()>, 256), 4, 64);
      if (h->mom_rows <= 0 && R > 32) R = 14;
      launch(h, kMomentum, k_momentum<T, V, BS()>, dim3(blocks_rows(last - first + 1, ntt, R) + (tp.masks ? 1u : 0u)), 0, h->g, C(h),
             (const T*)F_<T>(h, fF), (const T*)F_<T>(h, fU), (const T*)F_<T>(h, fV), F_<T>(h, fUS), F_<T>(h, fVS), F_<T>(h, fRHS), R, ntt,
             virt ? 1 : 0, tp, first, last);
    }, buffer_stores_ok(h) && (h->buf_stores & 1));
  }
  template <bool STORED>
  static void rhs(vof2d_ctx* h) {
    const int R = pick_rows(h, h->g.ntj);
    launch(h, kRhs, k_rhs<T, V, STORED>, dim3(blocks_rows(interior_rows(h), h->g.ntj, R)), 0, h->g, C(h), (const T*)F_<T>(h, fUS),
           (const T*)F_<T>(h, fVS), (const T*)F_<T>(h, fF), (const T*)F_<T>(h, fRHO), F_<T>(h, fRHS), R);
  }
  // one sweep src -> dst
  template <bool RESID>
  static void jacobi(vof2d_ctx* h, int src, int dst) {
    const int R = pick_rows(h, h->g.ntj);
    launch(h, kJacobi, k_jacobi<T, V, 2, RESID>, dim3(blocks_rows(interior_rows(h), h->g.ntj, R)), 0, h->g, C(h),
           (const T*)F_<T>(h, src), (const T*)F_<T>(h, fRHS), F_<T>(h, dst), R, h->d_courant + 1);
  }
  // TS sweeps src -> dst in one launch: tile count and rows per chunk.  RESID: the instantiation that reduces the norms
  // of its last sweep needs a few registers more, so its own occupancy decides the chunk length.
  static bool square_cells(vof2d_ctx* h) {   // square cells: the product-carrying pipeline
    const Consts<T> cc = C(h);
    return cc.dxi2 == cc.dyi2 && !h->tb_general;
  }
  template <int TS, bool RESID = false>
  static int jacobi_tb_plan(vof2d_ctx* h, bool sq, int& ntt) {
    ntt = sq ? JacobiTbGeom<V, TS, true>::tiles(h->g.ny) : JacobiTbGeom<V, TS, false>::tiles(h->g.ny);
    if (h->tb_rows > 0) return h->tb_rows;
    int R = 0;
    dispatch([&](auto SQ) { R = chunk_rows_fit(h, ntt, resident(h, k_jacobi_tb<T, V, TS, SQ(), RESID>, 256), 4, 96); }, sq);
    return R;
  }
  // k_jacobi_pair (two five-sweep launches as one, kernels/jacobi_pair.h): square cells, ten sweeps per step at least
  static bool jacobi_pair_ok(vof2d_ctx* h) {
    // (both precisions since the chained batches: 4096^2 fp32 dam-break 0.268 ms/step in the k_tm form with the pairs, 0.343 in
    //  chains; knob values 1 and 2 are the same now)
    return h->jpair >= 1 && square_cells(h) && h->tb >= 5 && h->d.jacobi_iters % 10 == 0;
  }
  // the Jacobi kernel of the k_tm forms (the batches of a full domain, the middle steps of overlap mode 5): what their plans are for
  static PlanFor plan_for_tm(vof2d_ctx* h) { return jacobi_pair_ok(h) ? PlanFor::kJacobiPair : PlanFor::kJacobiTb; }
  static bool pair_buffer_stores(const vof2d_ctx* h) { return buffer_stores_ok(h) && (h->buf_stores & 2); }
  static int jacobi_pair_geom(vof2d_ctx* h, int& ntt) {
    ntt = JacobiPairGeom<V, 5>::tiles(h->g.ny);
    if (h->jpair_rows > 0) return h->jpair_rows;
    int R = 0;
    dispatch([&](auto BS) { R = chunk_rows_fit(h, ntt, resident(h, k_jacobi_pair<T, V, 5, BS()>, 128), 8, 160); }, pair_buffer_stores(h));
    return R;
  }
  // ten sweeps src -> dst
  static void jacobi_pair(vof2d_ctx* h, int src, int dst, int adapt_par = -1, int first = 1, int last = 0) {
    if (last < first) { first = h->g.ilo; last = h->g.ihi; }
    int ntt = 0;
    const int R = jacobi_pair_geom(h, ntt);
    const TbPlan tp = tb_plan(h, adapt_par, PlanFor::kJacobiPair);
    const unsigned pairs = tp.masks ? (unsigned)tp.waves : (unsigned)(((last - first + R) / R) * ntt);
    dispatch([&](auto BS) {
      launch_block(h, kJacobiPair, k_jacobi_pair<T, V, 5, BS()>, dim3(pairs), 128u, 0, h->g, C(h), (const T*)F_<T>(h, src),
                   (const T*)F_<T>(h, fRHS), F_<T>(h, dst), R, ntt, tp, first, last);
    }, pair_buffer_stores(h));
  }
  // the work plan of the step's five-sweep launches (see tb_make_plan): active on parity-keyed step
  // sequences (adapt_par = istep & 1), square or not, up to TB_COLS tile columns; planned for the kernel that will read it
  static TbPlan tb_plan(vof2d_ctx* h, int adapt_par, PlanFor plan_for) {
    TbPlan tp{nullptr, nullptr, 0, 0, 0, 0, 0};
    if (adapt_par < 0 || !h->tb_adapt || h->tb < 5 || h->tb_rows > 0) return tp;
    int ntt = 0;
    int R;
    long waves;
    if (plan_for == PlanFor::kJacobiPair) {   // the plan's "waves" are pairs on 108-column tiles (jacobi_pair_geom); a plan is only ever read by the kernel it was planned for -- enqueue_tm_head, tm5_head
      R = jacobi_pair_geom(h, ntt);
      waves = (long)((h->g.ihi - h->g.ilo + R) / R) * ntt;
    } else {
      R = jacobi_tb_plan<5>(h, square_cells(h), ntt);
      waves = (long)blocks_rows(interior_rows(h), ntt, R) * 4;
    }
    if (ntt > TB_COLS || waves > kTbPlanWaves) return tp;
    tp.masks = h->d_tbmask;
    tp.plan = h->d_tbmask + 2 * TB_BANDS * (TB_COLS / 64);
    tp.ntt = ntt; tp.R = R; tp.waves = (int)waves; tp.par = adapt_par;
    tp.slow10 = plan_for == PlanFor::kJacobiPair ? h->pair_slow10 : h->tb_slow10;   // (what a row of a reported band costs: per kernel)
    return tp;
  }
  // TS sweeps src -> dst on rows [first, last] (last < first: all computable rows).  RESID: the last sweep also reduces
  // max|p_new - p| and max|p_new| over the owned rows into d_courant[1..2] (the residual-terminated solve):
  // same values, uniform chunks, all rows.
  template <int TS, bool RESID = false>
  static void jacobi_tb(vof2d_ctx* h, int src, int dst, int adapt_par = -1, int first = 1, int last = 0) {
    if (last < first) { first = h->g.ilo; last = h->g.ihi; }
    const Consts<T> cc = C(h);
    const bool sq = square_cells(h);
    int ntt = 0;
    const int R = jacobi_tb_plan<TS, RESID>(h, sq, ntt);
    TbPlan tp{nullptr, nullptr, 0, 0, 0, 0, 0};
    if (TS == 5 && !RESID) tp = tb_plan(h, adapt_par, PlanFor::kJacobiTb);
    // (with a plan the launch holds the waves of the whole grid's plan, whatever part of the rows it is for: every
    // wave takes the part of its planned chunk inside [first, last], or nothing)
    const unsigned all_blocks = blocks_rows(interior_rows(h), ntt, R);
    const unsigned nblk = tp.masks ? all_blocks : blocks_rows(last - first + 1, ntt, R);
    unsigned long long* const norms = RESID ? h->d_courant + 1 : nullptr;
    auto go = [&](auto SQ, auto BS) {
      launch(h, kJacobiTB, k_jacobi_tb<T, V, TS, SQ(), RESID, BS()>, dim3(nblk), 0, h->g, cc,
             (const T*)F_<T>(h, src), (const T*)F_<T>(h, fRHS), F_<T>(h, dst), R, ntt, norms, tp, first, last);
    };
    // the buffer-store form where the launch is ONE residency round of the chunk plan (4096^2, the strips of a multi-GPU
    // run: 105 -> 103 us, 53.7 -> 49.0 us): it needs 126 VGPRs instead of 129, i.e. four waves per SIMD are resident
    // where the plan counted on three, which breaks the round structure of a multi-round launch (8192^2 on one GPU:
    // 397 -> 435 us)
    static_assert(sizeof(T) * V == 16 || sizeof(T) * V == 8, "store_buf_nt: one b128 / b64 store per lane");
    if constexpr (!RESID) {
      if (sq && (long)all_blocks * 4 <= resident(h, k_jacobi_tb<T, V, TS, true, false>, 256) && pair_buffer_stores(h))
        return go(std::true_type{}, std::true_type{});
    }
    if (sq) go(std::true_type{}, std::false_type{}); else go(std::false_type{}, std::false_type{});
  }
  template <bool STORED>
  static void correct(vof2d_ctx* h) {
    const int R = pick_rows(h, h->g.ntj);
    launch(h, kCorrect, k_correct<T, V, STORED>, dim3(blocks_rows(interior_rows(h), h->g.ntj, R)), 0, h->g, C(h),
           (const T*)F_<T>(h, fP), (const T*)F_<T>(h, fF), (const T*)F_<T>(h, fRHO), (const T*)F_<T>(h, fUS),
           (const T*)F_<T>(h, fVS), F_<T>(h, fU), F_<T>(h, fV), R, h->d_courant);
  }
  // sweeps read fld[fF], write fld[fF2]; the caller swaps the two afterwards.
  // CORR: the sweep also performs update_uv (reads u*, v*, p; writes u, v) -- see k_fct_x.
  // rows [first, last] of the sweep's output (0, 0: all computable rows)
  // src, dst: another pair in the fields' layout in the place of F and its twin (the dye, runtime/dye.h; not with CORR)
  template <bool POST, bool CORR>
  static void fct_x(vof2d_ctx* h, int first = 0, int last = 0, const T* src = nullptr, T* dst = nullptr) {
    if (first == 0 && last == 0) { first = h->g.ilo; last = h->g.ihi; }
    const int forced = CORR && h->fctx_corr_rows > 0 ? h->fctx_corr_rows : h->fctx_rows;
    const int R = forced > 0 ? forced : chunk_rows(h, h->g.ntj, 4, 16);
    launch(h, kFctX, k_fct_x<T, V, POST, CORR>, dim3(blocks_rows(last - first + 1, h->g.ntj, R)), 0, h->g, C(h),
           src ? src : (const T*)F_<T>(h, fF), (const T*)F_<T>(h, fU), src ? dst : F_<T>(h, fF2), R, (const T*)F_<T>(h, fUS),
           (const T*)F_<T>(h, fVS), (const T*)F_<T>(h, fP), F_<T>(h, fU), F_<T>(h, fV), h->d_courant, first, last);
  }
  template <bool POST, bool CORR>
  static void fct_y(vof2d_ctx* h, int first = 0, int last = 0, const T* src = nullptr, T* dst = nullptr) {
    if (first == 0 && last == 0) { first = h->g.ilo; last = h->g.ihi; }
    const int R = h->rows_override > 0 ? h->rows_override : 1;   // rows are independent in this sweep
    launch(h, kFctY, k_fct_y<T, V, POST, CORR>, dim3(blocks_rows(last - first + 1, h->nty, R)), 0, h->g, C(h),
           src ? src : (const T*)F_<T>(h, fF), (const T*)F_<T>(h, fV), src ? dst : F_<T>(h, fF2), R, h->nty, (const T*)F_<T>(h, fUS),
           (const T*)F_<T>(h, fVS), (const T*)F_<T>(h, fP), F_<T>(h, fU), F_<T>(h, fV), h->d_courant, first, last);
  }
  // k_transport of this step + k_momentum of the next in one launch (k_tm): reads fld[fF], fld[fUS], fld[fVS], fld[fP];
  // writes fld[fF2], rhs, u*' / v*' into fld[fMX] / fld[fMY] (the caller alternates the pairs and swaps F), u and v
  // only with STORE_UV; adapt_par: parity of the NEXT step (its planner block rides here as it does in k_momentum)
  static int tm_body_rows(const vof2d_ctx* h, long rows, int ntf, long cap) {
    if (h->tm_rows > 0) return h->tm_rows;
    long k = (rows * ntf + cap * 25) / (cap * 50);
    if (k < 2) k = 2;
    long chunks = k * cap * 97 / 100 / ntf;
    if (chunks < 1) chunks = 1;
    const long R = (rows + chunks - 1) / chunks;
    return (int)(R < 16 ? 16 : (R > 96 ? 96 : R));
  }
  // The rows [first, last] of one launch as segments (kernels/row_segments.h): the body in chunks of tm_body_rows and, behind it, up to
  // three tail segments of shorter chunks.  The hardware hands the pairs out in index order, so the chunks of the last rows are the
  // ones that start last, and a launch ended with whole 52-row gas chunks (87 us each) at falling occupancy: Sum durations / (span x
  // slots) = 0.735.  Shorter chunks there fill the slots the body's pairs leave (0.82-0.85) at the price of their 14 lead-in steps.
  // Knob tm_taper: 0 one segment (no tail); 1 the tail as the knobs tm_tail_at1..3 (first row of tail segment 1..3; 0: none) and
  // tm_tail_rows1..3 (its chunk length) say, on any launch that takes its chunk length from here -- a segment whose first row is the
  // next one's is empty --; -1 (the default) by the rule; -2 the rule's cut without its condition on the body's chunk length.
  // THE RULE (kTmTaper): on a full domain whose launch runs more than one residency round with the heuristic's chunk length R >= 28,
  // the last rows go in chunks of R / 2, R / 4 and R / 6 (at least 8) rows, as many chunk rows of each as make 30 %, 40 % and 20 % of
  // the resident pairs (4096^2: rows 3500-3811 in 26-row chunks, 3812-4032 in 13s, 4033-4096 in 8s; 2923 -> 3885 pairs).  Swept with
  // tools/probes/tm_taper_ab.py, every run a process of its own, the candidates alternating (profiles/tm_taper_sweep.txt), ms/step
  // over steps 61-460, medians, off -> rule: 4096^2 dam-break 0.431 -> 0.400 (shares 30/40/0 0.405, 30/60/0 0.402, 30/60/30 0.404,
  // 30/40/45 0.405, 20/40/0 0.409; a box earlier 15/30/0 0.396, 30/40/80 0.396, R / 4 alone 0.409 against 0.390-0.391), 4096^2 bubble
  // 0.597 -> 0.543 (30/60/30 0.535, 30/40/0 0.548); with shares 30/40/0 and 30/40/45, between which the rule lies: 3072^2 (R = 29)
  // 0.271 -> 0.258 / 0.263, 5120^2 0.607 -> 0.586 / 0.589, 6144^2 0.861 -> 0.844 / 0.844,
  // 8192^2 (7.8 rounds: the tail is a small part) 1.45 -> 1.45.  2048^2 (R = 16: every tail chunk would be 8 rows, and the lead-in
  // steps cost more than the tail gives) 0.1586 -> 0.1605: hence R >= 28, the shortest body measured to gain.  Strips, one-round
  // launches and forced chunk lengths (tm_rows) keep one segment.
  struct TmTaperRule { int div[3]; int share[3]; int floor_rows; int min_body_rows; };   // tail segment j: chunks of R / div[j] rows (>= floor_rows), share[j] % of the resident pairs
  static constexpr TmTaperRule kTmTaper{{2, 4, 6}, {30, 40, 20}, 8, 28};
  static RowSegments tm_chunk_rows(const vof2d_ctx* h, int first, int last, int ntf, long cap) {
    const int R = tm_body_rows(h, last - first + 1, ntf, cap);
    int at[3] = {last + 1, last + 1, last + 1}, len[3] = {1, 1, 1};
    if (h->tm_taper > 0) {
      int lo = first;
      bool more = true;
      for (int j = 0; j < 3; ++j) {
        more = more && h->tm_tail_at[j] > 0;
        if (more) at[j] = h->tm_tail_at[j] < lo ? lo : (h->tm_tail_at[j] > last + 1 ? last + 1 : h->tm_tail_at[j]);
        len[j] = h->tm_tail_rows[j] > 0 ? h->tm_tail_rows[j] : 1;
        lo = at[j];
      }
    } else if (h->tm_taper < 0 && h->tm_rows <= 0 && h->g.wall_lo && h->g.wall_hi && first == h->g.ilo && last == h->g.ihi &&
               (long)row_seg_chunks(first, last, R) * ntf > cap && (R >= kTmTaper.min_body_rows || h->tm_taper == -2)) {
      int lo = last + 1;
      for (int j = 2; j >= 0; --j) {
        len[j] = R / kTmTaper.div[j] > kTmTaper.floor_rows ? R / kTmTaper.div[j] : kTmTaper.floor_rows;
        lo -= (int)((kTmTaper.share[j] * cap + 50L * ntf) / (100L * ntf)) * len[j];   // (chunk rows of the segment) * (their length)
        at[j] = lo;
      }
      if (at[0] < first + R) return row_segments(row_seg(first, last, R));
    }
    return row_segments(row_seg(first, at[0] - 1, R), row_seg(at[0], at[1] - 1, len[0]), row_seg(at[1], at[2] - 1, len[1]), row_seg(at[2], last, len[2]));
  }
  // rows [first, last] and, in the same launch, [first2, last2] (a strip's two edge bands: two segments of rows_forced-row chunks);
  // store_uv: the last k_tm of a batch; rhs_id: the array the next step's rhs goes to (fRHS, or fKAPPA where the caller alternates
  // the two: enqueue_steps_tm)
  // zero_maps: the launch keeps and uses the zero maps of F and its twin where the handle runs with them (h->fzmap_active; the caller
  // has cleared them if they were stale: fzmap_clear_if_stale, runtime/schedule.h) -- the ZMAP instantiation; every other launch is today's kernel
  static void tm(vof2d_ctx* h, bool y_first, bool store_uv, int adapt_par, PlanFor plan_for, int rhs_id, int first = 1, int last = 0, int rows_forced = 0, int first2 = 1, int last2 = 0,
                 bool zero_maps = false) {
    if (last < first) { first = h->g.ilo; last = h->g.ihi; }
    const int ntf = TmGeom<V>::tiles(h->g.ny);
    const TbPlan tp = tb_plan(h, adapt_par, plan_for);
    if (zero_maps && h->fzmap_active) {
      // each map belongs to its array, not to the view: the bit that picks the F pointers picks the maps
      const int cur = (h->views.bits() & FieldViews::kF) ? 1 : 0;
      const ZeroMaps zm{h->buf.fzmap.as<unsigned>(), (int)fzmap_offset(h, cur), (int)fzmap_offset(h, cur ^ 1), ntf + 2};
      dispatch([&](auto YF, auto UV) {
        const RowSegments rows = tm_chunk_rows(h, first, last, ntf, resident(h, k_tm<T, V, YF(), UV(), true, 0, true>, 128));
        const unsigned pairs = (unsigned)(row_chunks(rows) * ntf) + (tp.masks ? 1u : 0u);
        h->tm_segments_last = row_used_segments(rows);
        launch_block(h, UV() ? kTMUV : kTM, k_tm<T, V, YF(), UV(), true, 0, true>, dim3(pairs), 128u, 0, h->g, C(h), (const T*)F_<T>(h, fF), F_<T>(h, fF2), ntf,
                     (const T*)F_<T>(h, fUS), (const T*)F_<T>(h, fVS), (const T*)F_<T>(h, fP), F_<T>(h, fU), F_<T>(h, fV),
                     F_<T>(h, fMX), F_<T>(h, fMY), F_<T>(h, rhs_id), h->d_courant, tp, rows, zm);
      }, y_first, store_uv);
      return;
    }
    // pair chunks: a whole number of residency rounds, just filled (6 pairs per CU: 24 KB of LDS each) -- a launch that needs a
    // little more than k rounds pays for k + 1 --, as many rounds as keep the chunks near 50 rows (one round of 100-row
    // chunks: every step of every pair takes 3.3 us instead of 1.9).  4096^2, 112-column tiles, us per launch: 40 rows
    // (2.5 rounds) 261 / 281 (inside / behind the front), 48 252 / 282, 52 253 / 280, 54 256 / 277, 56 257 / 284,
    // 100 376 / 381 (tools/probes/pair_bound.py --rows)
    dispatch([&](auto YF, auto UV, auto BS) {
      const RowSegments rows = rows_forced > 0 ? row_segments(row_seg(first, last, rows_forced), row_seg(first2, last2, rows_forced))
                                              : tm_chunk_rows(h, first, last, ntf, resident(h, k_tm<T, V, YF(), UV(), true>, 128));
      const unsigned pairs = (unsigned)(row_chunks(rows) * ntf) + (tp.masks ? 1u : 0u);
      h->tm_segments_last = row_used_segments(rows);
      launch_block(h, UV() ? kTMUV : kTM, k_tm<T, V, YF(), UV(), BS()>, dim3(pairs), 128u, 0, h->g, C(h), (const T*)F_<T>(h, fF), F_<T>(h, fF2), ntf,
                   (const T*)F_<T>(h, fUS), (const T*)F_<T>(h, fVS), (const T*)F_<T>(h, fP), F_<T>(h, fU), F_<T>(h, fV),
                   F_<T>(h, fMX), F_<T>(h, fMY), F_<T>(h, rhs_id), h->d_courant, tp, rows, ZeroMaps{nullptr, 0, 0, 0});
    }, y_first, store_uv, buffer_stores_ok(h) && (h->buf_stores & 4));
  }
  // the counters of the zero map of array `cur` (0: the F array of creation, 1: its twin) into buf.fzmap_cnt: one thread per word
  static void fzmap_check(vof2d_ctx* h, int cur) {
    const int ntf = TmGeom<V>::tiles(h->g.ny);
    const long words = (long)h->g.nx * ntf;
    launch(h, kOther, k_fzmap_check<T, V>, dim3((unsigned)((words + 255) / 256)), 0, h->g, (const T*)h->views.table()[fF], ntf,
           h->buf.fzmap.as<const unsigned>(fzmap_offset(h, cur)), h->buf.fzmap_cnt.as<unsigned long long>());
  }
  // ---- conjugate gradients (kernels/cg.h)
  // sum of ap over the interior, in double, of the values the kernels form in T: ap depends on the position through
  // "first / last row or not" and "first / last column or not" only (2dvof.py:258-262), four values with their counts
  static double cg_sum_ap(const vof2d_ctx* h) { return sum_ap_of(C(const_cast<vof2d_ctx*>(h)), h->g.nx, h->g.ny); }
  static double sum_ap_of(const Consts<T>& c, int nx, int ny) {
    const T zero = (T)0.0;
    const T ax[2] = {c.dxi2 + zero, c.dxi2 + c.dxi2};          // ae + aw: wall row, inner row
    const double nrow[2] = {2.0, (double)(nx - 2)}, ncol[2] = {2.0, (double)(ny - 2)};
    double sum = 0.0;
    for (int a = 0; a < 2; ++a) {
      const T wall = (T)-1.0 * (ax[a] + c.dyi2 + zero), inner = (T)-1.0 * (ax[a] + c.dyi2 + c.dyi2);
      sum += nrow[a] * (ncol[0] * (double)wall + ncol[1] * (double)inner);
    }
    return sum;
  }
  // Where a solve runs: the handle's own grid (p, rhs, h->cg_fld, h->cg_sc) or the coarsest level of a multigrid cycle.
  // w: r, two directions (ping-pong), q in the grid's layout; sc: the scalars of the solve.  Rows per wave chunk: the
  // pointwise kernels and the residual like every streaming kernel (pick_rows; R1, n1 blocks); k_cg_apply forms the
  // direction of one extra row above and below its chunk, so its chunks are twice as long (R2, n2 blocks).  Every
  // launch leaves one partial per block in h->cg_part, which the k_cg_finish behind it folds.
  struct CgGrid {
    Geom g; Consts<T> c; T* e; const T* f; void* const* w; double* sc;
    int R1, R2; unsigned n1, n2;
  };
  static CgGrid cg_grid(vof2d_ctx* h, const Geom& g, const Consts<T>& c, T* e, const T* f, void* const (&w)[4], double* sc) {
    const int R1 = pick_rows(h, g.ntj), rows = g.ihi - g.ilo + 1;   // (the rows cell_tile cuts into chunks)
    return {g, c, e, f, w, sc, R1, 2 * R1, blocks_rows(rows, g.ntj, R1), blocks_rows(rows, g.ntj, 2 * R1)};
  }
  static CgGrid cg_own(vof2d_ctx* h) { return cg_grid(h, h->g, C(h), F_<T>(h, fP), (const T*)F_<T>(h, fRHS), h->cg_fld, h->cg_sc); }
  static void cg_finish(vof2d_ctx* h, const CgGrid& a, unsigned nblocks, int mode, double sum_ap = 0.0, int restart = 0) {
    launch(h, kCgFinish, k_cg_finish, dim3(1), 0, (const double*)h->cg_part, (int)nblocks, a.sc, mode, sum_ap, restart);
  }
  // c = sum(f) / sum(ap) into the scalars
  static void cg_drift(vof2d_ctx* h, const CgGrid& a, double sum_ap) {
    launch(h, kCgResidual, k_cg_sum<T, V>, dim3(a.n1), 0, a.g, a.f, a.R1, h->cg_part);
    cg_finish(h, a, a.n1, CG_FIN_SUMB, sum_ap);
  }
  static void cg_residual(vof2d_ctx* h, const CgGrid& a, int restart) {
    launch(h, kCgResidual, k_cg_residual<T, V>, dim3(a.n1), 0, a.g, a.c, (const T*)a.e, a.f, reinterpret_cast<T*>(a.w[0]), a.R1,
           (const double*)a.sc, h->cg_part);
    cg_finish(h, a, a.n1, CG_FIN_RESID, 0.0, restart);
  }
  // one iteration: two field kernels, each followed by its one-block reduction; s: which of w[1..2] holds the current direction
  static void cg_iteration(vof2d_ctx* h, const CgGrid& a, int& s) {
    T* const r = reinterpret_cast<T*>(a.w[0]);
    T* const s_old = reinterpret_cast<T*>(a.w[s]);
    s = 3 - s;
    T* const s_new = reinterpret_cast<T*>(a.w[s]);
    T* const q = reinterpret_cast<T*>(a.w[3]);
    launch(h, kCgApply, k_cg_apply<T, V>, dim3(a.n2), 0, a.g, a.c, (const T*)r, (const T*)s_old, s_new, q, a.R2, (const double*)a.sc, h->cg_part);
    cg_finish(h, a, a.n2, CG_FIN_APPLY);
    launch(h, kCgUpdate, k_cg_update<T, V>, dim3(a.n1), 0, a.g, a.c, a.e, (const T*)s_new, r, (const T*)q, a.R1, (const double*)a.sc, h->cg_part);
    cg_finish(h, a, a.n1, CG_FIN_UPDATE);
  }
  // ... on the handle's grid (h->cg_s survives between the cg_iteration calls of one solve)
  static void cg_drift(vof2d_ctx* h, double sum_ap) { cg_drift(h, cg_own(h), sum_ap); }
  static void cg_residual(vof2d_ctx* h, int restart) { cg_residual(h, cg_own(h), restart); }
  static void cg_iteration(vof2d_ctx* h) { cg_iteration(h, cg_own(h), h->cg_s); }
  // ---- multigrid (kernels/mg.h): every wrapper takes the level(s) it works on; level 0 is the handle's own grid
  static Consts<T> mg_consts(vof2d_ctx* h, const MgLevel& lv) {
    Consts<T> c = C(h);
    c.dxi2 = (T)(c.dxi2 * (T)lv.scale);   // exact: a power of four
    c.dyi2 = (T)(c.dyi2 * (T)lv.scale);
    return c;
  }
  static unsigned mg_blocks(const vof2d_ctx* h, const Geom& g, int R) { (void)h; return blocks_rows(g.nx, g.ntj, R); }
  // one sweep e -> en; sc: the scalars holding c on level 0, nullptr below it (f is stored there)
  static void mg_smooth(vof2d_ctx* h, const MgLevel& lv, const T* e, const T* f, T* en, const double* sc) {
    const int R = pick_rows(h, lv.g.ntj);
    launch(h, kMgSmooth, k_mg_smooth<T, V>, dim3(mg_blocks(h, lv.g, R)), 0, lv.g, mg_consts(h, lv), e, f, en, R, sc);
  }
  static void mg_restrict(vof2d_ctx* h, const MgLevel& fine, const MgLevel& coarse, const T* e, const T* f, T* fc, T* ec, const double* sc) {
    const int R = pick_rows(h, coarse.g.ntj);
    launch(h, kMgRestrict, k_mg_restrict<T, V>, dim3(mg_blocks(h, coarse.g, R)), 0, fine.g, coarse.g, mg_consts(h, fine), e, f, fc, ec, R, sc);
  }
  static void mg_prolong(vof2d_ctx* h, const MgLevel& fine, const MgLevel& coarse, const T* ec, T* e) {
    const int R = pick_rows(h, coarse.g.ntj);
    launch(h, kMgProlong, k_mg_prolong<T, V>, dim3(mg_blocks(h, coarse.g, R)), 0, fine.g, coarse.g, ec, e, R);
  }
  // L e = f - c' ap on one level by the kernels of kernels/cg.h, from the e it finds, until max|z| is down to `reduction`
  // of its start or `cap` iterations are enqueued (k_mg_coarse_stop); w: r, two directions, q in the level's layout;
  // own_drift: c' = sum(f) / sum(ap) of this level is formed first (on level 0 the solve's own c is in sc already)
  static void mg_coarse_solve(vof2d_ctx* h, const MgLevel& lv, T* e, const T* f, void* const (&w)[4], double* sc, bool own_drift,
                              int cap, double reduction) {
    const Consts<T> cc = mg_consts(h, lv);
    const CgGrid a = cg_grid(h, lv.g, cc, e, f, w, sc);
    if (own_drift) cg_drift(h, a, sum_ap_of(cc, lv.g.nx, lv.g.ny));
    cg_residual(h, a, 1);
    launch_block(h, kOther, k_mg_coarse_stop, dim3(1), 64u, 0, sc, 1, reduction);
    int s = 1;
    for (int it = 0; it < cap; ++it) {
      cg_iteration(h, a, s);
      launch_block(h, kOther, k_mg_coarse_stop, dim3(1), 64u, 0, sc, 0, reduction);
    }
  }
  // ... the same solve as ONE launch of one workgroup (knob "mg_coarse_block"; the caller has checked that the level fits:
  // mg_block_in_effect, runtime/multigrid.h).  sc_c: the scalars holding c where the level is the grid itself, else nullptr.
  static void mg_coarse_block(vof2d_ctx* h, const MgLevel& lv, T* e, const T* f, const double* sc_c, int cap, double reduction) {
    const Consts<T> cc = mg_consts(h, lv);
    launch(h, kMgCoarseBlock, k_mg_coarse_block<T>, dim3(1), 0, lv.g, cc, e, f, sc_c, sum_ap_of(cc, lv.g.nx, lv.g.ny), cap, reduction);
  }
  // update_uv + both sweeps + post_process_f in one pass (k_transport); reads fld[fF], writes fld[fF2]
  static int transport_rows(const vof2d_ctx* h) {
    return h->fctx_corr_rows > 0 ? h->fctx_corr_rows : chunk_rows(h, h->nty, 4, 16);
  }
  // the rows of `segments` (kernels/row_segments.h; all computable rows by default)
  static void transport(vof2d_ctx* h, bool y_first, const RowSegments* segments = nullptr) {
    const RowSegments rr = segments ? *segments : row_segments(row_seg(h->g.ilo, h->g.ihi, transport_rows(h)));
    const unsigned tr_blocks = (unsigned)(((long)row_chunks(rr) * h->nty + 3) / 4);
    dispatch([&](auto YF) {
      launch(h, kTransport, k_transport<T, V, YF()>, dim3(tr_blocks), 0, h->g, C(h),
             (const T*)F_<T>(h, fF), F_<T>(h, fF2), h->nty, (const T*)F_<T>(h, fUS), (const T*)F_<T>(h, fVS),
             (const T*)F_<T>(h, fP), F_<T>(h, fU), F_<T>(h, fV), h->d_courant, rr);
    }, y_first);
  }
};

}  // namespace
