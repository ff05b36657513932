// vof2d_kernels.h -- hand-written gfx950 kernels for the 2-D VOF hot path.
//
// Every kernel cites the reference lines (/root/reference/2dvof.py) it
// replaces.  Arithmetic follows the reference's Python expression order,
// left to right, with FMA contraction disabled (-ffp-contract=off), so the
// results equal the CPU oracle's value for value.
//
// All stencil kernels share one decomposition (vof2d_device.h): a wave owns
// 64*V contiguous columns and marches along i with a register window.
//
// The kernels live in kernels/, one file per family:
//   common.h     tile rows, streaming loads / stores, DPP neighbours, exact division
//   march.h      wave_index, tile_c0, tile_columns, tile_decode, row_ptr, zero_fill, wave_all_zero, wave_sum, courant_count, courant_publish, store_uv_row, normals_cell, corrected_velocity   (what the marching kernels share around the arithmetic of a row)
//   row_segments.h  the rows of a k_tm or k_transport launch as up to four segments of chunks, for host and device
//   verbs.h      one kernel per reference verb (the literal main loop, 2dvof.py:513-528)
//   plan.h       the equal-cost work plan of the fused Jacobi launches
//   momentum.h   k_momentum      (cal_nu_rho + get_normal_young + advect_upwind + rhs)
//   jacobi.h     k_jacobi, k_jacobi_tb   (solve_p_jacobi, the north-star kernel)
//   jacobi_pair.h  k_jacobi_pair   (two k_jacobi_tb launches as one: pairs of waves, result and rhs rows through LDS)
//   transport.h  k_fct_x, k_fct_y, k_transport   (update_uv + solve_VOF_rudman + post_process_f)
//   fused_tm.h   k_tm   (k_transport of one step + k_momentum of the next, rows handed over through LDS)
//   reduce.h     block_publish, fold_partials   (the fixed-order reduction of the families below; no kernel of its own)
//   cells.h      cell_tile, mul_rounded, Cell, reduced_rows, k_row_finish   (what the extension kernels share: the tile of the reported cells, the product no contraction reaches, a cell's operands, the pass that ends in one partial per block and the one block that turns the partials into a row)
//   cg.h         k_cg_apply, k_cg_update, k_cg_residual   (extension: conjugate gradients on the pressure equation)
//   mg.h         k_mg_smooth, k_mg_restrict, k_mg_prolong, k_mg_coarse_block, k_mg_step_record  (extension: geometric multigrid on the same equation)
//   diag.h       k_diag   (extension: volume, centroid, kinetic energy, divergence, extrema in one fixed-order pass)
//   cell_rows.h  k_cell_rows, k_cell_rows_scan; scan_counts   (what the two families below share: a row per interface cell, counted, scanned and emitted in (i, j) order)
//   interface.h  IfaceVerb   (extension: the interface as PLIC segments)
//   curvature.h  CurvVerb   (extension: height-function curvature of every mixed cell beside the solver's own CSF curvature)
//   energy.h     k_energy   (extension: the energy budget -- face kinetic energy, density moments, the interface measure and the power of every term of the momentum predictor, evaluated face by face in double with kappa gathered at the interface, in one fixed-order pass over F, u, v, p)
//   blobs.h      k_blob_init, k_blob_merge, k_blob_flatten, k_blob_number, k_blob_label, k_blob_stats, k_blob_summary, k_blob_plan, k_blob_sums, k_blob_rows   (extension: droplets and bubbles labelled by union-find, numbered by first cell, measured in a fixed order)
//   tracers.h    k_tracer_advance, k_tracer_sample, k_tracer_finish   (extension: passive particles, one per lane: bilinear gather on the staggered grid, midpoint rule, walls)
//   depths.h     k_depths, k_depths_fold, k_depths_finish, k_gauge_sample   (extension: both marginals of F, the top of the liquid per row and the front in one pass over F; fixed sensors that sample u, v, F, p and read them)
//   dye.h        k_dye, k_dye_stats   (extension: a marker field moved by both FCT sweeps in one pass over C, u, v; its sums and extrema in one fixed-order pass)
//   frames.h     k_frame_cols, k_frame_fold, k_frame_paint   (extension: a colour-mapped picture of F, u, v, the speed, p, the vorticity or the dye: box averages in a fixed order, a 256-entry colour table, the interface marked on top)
//   stats.h      k_stats, k_stats_fill, k_stats_summary   (extension: per-cell running sums of F, u, v and their products, envelopes, wet time and arrival step over a run: one streaming pass per sample over the fields and planes of doubles)
//   scene.h      k_scene   (extension: an initial state painted from an ordered list of boxes, ellipses, half-planes and triangles, S x S samples a cell as bit masks in registers)
//   regrid.h     k_regrid_refine, k_regrid_coarsen, k_regrid_ring, k_regrid_sum, k_regrid_finish   (extension: a state carried onto a finer or coarser grid: F of a mixed cell's children from its PLIC line, u, v linear along the face normal, p bilinear; box means the other way)
//   residual_rule.h  the residual of a criterion from the two norms of a check, for host and device
#pragma once
#include "kernels/common.h"
#include "kernels/march.h"
#include "kernels/verbs.h"
#include "kernels/plan.h"
#include "kernels/momentum.h"
#include "kernels/jacobi.h"
#include "kernels/jacobi_pair.h"
#include "kernels/transport.h"
#include "kernels/fused_tm.h"
#include "kernels/reduce.h"
#include "kernels/cells.h"
#include "kernels/cg.h"
#include "kernels/mg.h"
#include "kernels/diag.h"
#include "kernels/cell_rows.h"
#include "kernels/interface.h"
#include "kernels/curvature.h"
#include "kernels/energy.h"
#include "kernels/blobs.h"
#include "kernels/tracers.h"
#include "kernels/depths.h"
#include "kernels/dye.h"
#include "kernels/frames.h"
#include "kernels/stats.h"
#include "kernels/scene.h"
#include "kernels/regrid.h"
