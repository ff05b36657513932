// runtime/buffers.h -- DevBuf, the one owner of a device allocation of the handle beside the field arena, and the
// handle's list of them
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip); context.h includes it in front of the handle.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/vof2d.h"
#include "carve.h"

struct vof2d_ctx;
namespace {   // what DevBuf needs of the handle; defined behind it (runtime/context.h)
int fail(vof2d_ctx* h, int code, const char* msg);
hipStream_t stream_of(const vof2d_ctx* h);

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;   // the capacity
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  template <typename T> T* as(size_t byte_offset = 0) const { return reinterpret_cast<T*>(static_cast<char*>(p) + byte_offset); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  // Room for `want` bytes.  Nothing to do if it is there; otherwise the old contents are given up -- behind a wait for the
  // handle's stream: launches that read them may still be queued (hipFree waits anyway) -- and `zero` clears the new ones on
  // that stream.  VOF_ENOMEM with the message `what` and an empty buffer if there is no memory.
  int reserve(vof2d_ctx* h, size_t want, const char* what, bool zero = false) {
    if (bytes >= want) return VOF_OK;
    hipStream_t const stream = stream_of(h);
    if (p) (void)hipStreamSynchronize(stream);
    release();
    if (hipMalloc(&p, want) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      return fail(h, VOF_ENOMEM, what);
    }
    bytes = want;
    if (zero && hipMemsetAsync(p, 0, want, stream) != hipSuccess) {
      release();
      return fail(h, VOF_EHIP, "hipMemsetAsync of a new work buffer failed");
    }
    return VOF_OK;
  }
};

struct CellRowBufs { DevBuf work, rows; };   // a verb that emits a row per interface cell (runtime/cell_rows.h): the row counts, turned into offsets in place, the partials, the summary (CellRowsCarve); the rows, grown on demand
struct RowBufs { DevBuf part, rows; };   // a verb that reduces the reported cells to rows (runtime/diag_reduce.h): one partial per block of its pass; the rows recorded on the device

// Every work buffer of a handle: allocated by the first call that needs it (the first two: vof_create), kept until
// vof_destroy.  Nothing but DevBufs (a RowBufs or a CellRowBufs is two), so that they are released as one flat range: one added here is released too.
struct WorkBufs {
  DevBuf courant;      // device counters: [0] courant, [1] max|p_new - p| bits, [2] max|p_new| bits (residual solve), [3] exact-zero cells of F
  DevBuf tbmask;       // work plan of k_jacobi_tb (TbPlan): 2 x TB_BANDS mask words, then the plan (1 + waves entries)
  DevBuf cg_fields;    // vof_solve_p_cg (runtime/multigrid.h, CgCarve): r, two direction arrays (ping-pong), q
  DevBuf cg_part;      // ... one partial per block (kCgPart doubles), then the CG_NSCAL device scalars
  DevBuf mg_arena;     // vof_solve_p_mg (MgCarve): the levels below the grid, the work arrays and scalars of the coarsest-level solve
  DevBuf mg_rec;       // vof_step_mg: the residual record (kernels/mg.h, MGR_*)
  RowBufs diag;        // vof_diagnostics / vof_step_diag (runtime/diag_reduce.h): the partials of k_diag, rows of VOF_DIAG_N doubles
  CellRowBufs iface;   // vof_interface (runtime/cell_rows.h): segments of VOF_IFACE_N doubles
  CellRowBufs curv;    // vof_curvature (runtime/cell_rows.h): rows of VOF_CURV_N doubles
  RowBufs energy;      // vof_energy / vof_step_energy (runtime/energy.h): the partials of k_energy, rows of VOF_ENERGY_N doubles
  DevBuf blob_work;    // vof_blobs (runtime/blobs.h, BlobCarve): what the geometry fixes
  DevBuf blob_rec;     // ... grown on demand: the integer records of the blobs (kBlobRec ints each),
  DevBuf blob_off;     // the wave offsets and
  DevBuf blob_rows;    // the rows (VOF_BLOB_N doubles each) of the blobs asked for,
  DevBuf blob_part;    // the partials of their sums (kBlobSums doubles each)
  DevBuf tracer_pos;   // vof_tracers_* (runtime/tracers.h): the positions, n x 2 doubles -- state, not scratch: replaced by vof_tracers_set alone, whatever the three below do
  DevBuf tracer_rows;  // ... the rows of vof_tracers_get (VOF_TRACER_N doubles each), grown on demand
  DevBuf tracer_snaps; // ... the snapshots vof_step_tracers records, grown on demand
  DevBuf tracer_cnt;   // ... the integer counters (TRC_N words), then the summary (VOF_TRACER_SUM_N doubles)
  DevBuf depths_work;  // vof_depths (runtime/depths.h, DepthsCarve): the partials, depth_i, depth_j, the summary, top and the fronts' words
  DevBuf gauge_pos;    // vof_gauges_* (runtime/depths.h): the positions, n x 2 doubles -- state, not scratch: replaced by vof_gauges_set alone
  DevBuf gauge_rows;   // ... the rows of vof_gauges_get (VOF_GAUGE_N doubles each), grown on demand
  DevBuf gauge_recs;   // ... the records vof_step_gauges takes, grown on demand
  DevBuf dye;          // vof_dye_* (runtime/dye.h): the dye and its twin, two arrays in the fields' layout -- state, not scratch: replaced by vof_dye_set alone
  RowBufs dye_stats;   // ... the partials of k_dye_stats, rows of VOF_DYE_N doubles
  DevBuf frame_work;   // vof_frame (runtime/frames.h, FrameCarve): the column partials, the means of F, the words; the means, the summary, the picture
  DevBuf frame_lut;    // ... the colour table, 258 x 3 bytes -- state, not scratch: replaced by vof_frame_set_lut alone
  DevBuf frame_recs;   // ... the pictures vof_step_frames records, their summaries behind them, grown on demand
  DevBuf stats;        // vof_stats_* (runtime/stats.h, StatsCarve): the accumulator planes -- state, not scratch: cleared by vof_stats_begin alone --, the partials and results of the summary
  DevBuf scene;        // vof_set_scene (runtime/scene.h): the shape list as k_scene reads it (room for VOF_SCENE_MAX_SHAPES records), the slots of the two counters behind it
  DevBuf regrid;       // vof_regrid into this handle (runtime/regrid.h, RegridCarve): the counts of the refining pass, the partials of the two sums of F, the four results
  DevBuf vis;          // scratch for the display fields (vof_get_vis_field / vof_interp_velocity), grown on demand
  DevBuf red;          // device scalar of vof_comm_allreduce_max
  DevBuf fzmap;        // k_tm's zero maps (kernels/fused_tm.h): one word per (interior row, k_tm tile column) of the F array and, behind it, of its twin -- one allocation: one buffer descriptor in the march --, reserved zeroed
  DevBuf fzmap_cnt;    // ... the two words of the counters "fzmap_flagged", "fzmap_wrong"

  DevBuf* begin() { return &courant; }
  DevBuf* end() { return begin() + sizeof(WorkBufs) / sizeof(DevBuf); }
  void release() { for (DevBuf* b = begin(); b != end(); ++b) b->release(); }
};
static_assert(sizeof(RowBufs) == 2 * sizeof(DevBuf) && sizeof(CellRowBufs) == 2 * sizeof(DevBuf) && sizeof(WorkBufs) % sizeof(DevBuf) == 0, "WorkBufs is walked as one array");

}  // namespace
