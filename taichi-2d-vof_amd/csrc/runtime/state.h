// runtime/state.h -- what a handle's fields and ghost cells hold, and what the next step may assume: the flags, the
// one place a field write from outside or a verb changes them, the prologue and epilogue of a step, the phase order
//
// Plain C++ (no HIP): the host runtime includes it through context.h, the CPU tests compile it on its own
// (tests/host/state_check.cpp).
#pragma once

namespace vof {

enum FieldId { fF = 0, fF2, fU, fV, fP, fPT, fUS, fVS, fMX, fMY, fKAPPA, fRHO, fNU, fRHS, NFIELDS };

struct FieldState {
  bool f_ghosts_dirty = true;    // F's ghost cells may not satisfy set_BC (after set_init_F / from_numpy / a single verb)
  bool uv_ghosts_dirty = false;  // u / v were written without a set_BC since (update_uv verb, from_numpy): their ghost cells are not mirror images
  bool ghosts_virtual = false;   // the last fused step skipped its set_BC launch: the ghost cells in memory are stale
                                 // (k_momentum forms the ones it reads; everything else goes through settle_ghosts)
  bool alt_dirty = false;        // a verb or a field write left something in mx / my (the second u*, v* pair of the k_tm forms): cleared at the head of a strip call (tm5_head)
  bool ahead = false;            // u*, v*, rhs hold the predictor of step istep + 1 (the chained k_tm batches; settle_ahead)
  int next_phase = 0;            // the phase vof_step_phase takes next; not 0: a phased step is in progress
  bool fzmap_stale = true;       // F or its twin was written by something that keeps no zero map (anything but a k_tm launch of a batch that
                                 // does): a flag may stand over cells that are no longer zeros -- both maps are cleared before the next such batch
};

// ---- fields written other than by a step.  Field `id` was written from outside: by the host (vof_set_rows, vof_set_init_F)
// or, rows_only_inside, with rows of another handle (vof_copy_rows: the rows come with their ghost columns -- on a strip that
// is the halo exchange and says nothing; on a full domain the rows' neighbours' ghost cells may no longer mirror them -- and
// the twin of F is never named alone).  True if F changed: the caller forgets the batch form the rule chose (forget_batch_form).
inline bool field_written(FieldState& s, int id, bool full_domain, bool rows_only_inside) {
  if (id == fF || id == fF2) s.fzmap_stale = true;   // (either array, named alone or not: a map belongs to its array)
  if (rows_only_inside && !full_domain) return false;
  const bool f = id == fF || (id == fF2 && !rows_only_inside);
  if (f) s.f_ghosts_dirty = true;
  if (id == fMX || id == fMY) s.alt_dirty = true;
  if (id == fU || id == fV) s.uv_ghosts_dirty = true;
  return f;
}
// ... and by a verb, per class of verb
inline void bc_applied(FieldState& s) { s.f_ghosts_dirty = s.uv_ghosts_dirty = s.ghosts_virtual = false; }   // vof_set_BC: the launch a fused step left out
inline void verb_wrote_F(FieldState& s) { s.f_ghosts_dirty = s.fzmap_stale = true; }     // the FCT sweeps, vof_post_process_f (F is advanced, not replaced: the batch form stays)
inline void verb_wrote_uv(FieldState& s) { s.uv_ghosts_dirty = true; }   // vof_update_uv
inline void verb_wrote_alt(FieldState& s) { s.alt_dirty = true; }        // vof_get_normal_young, vof_advect_upwind: mx, my

// ---- a step.  What the handle can do ...
struct StepCaps {
  bool full_domain;      // both walls in one handle
  bool fuse_transport;   // knob: update_uv and both FCT sweeps in one kernel
  bool virtual_ghosts;   // knob (a strip: always asked as it is): the step's set_BC launch left out
  bool graphs;           // captured steps allowed (no VOF_FLAG_NO_GRAPH, and whatever else the entry point asks)
};
// ... and what the step about to run is
struct StepPlan {
  bool lean;       // F's ghost cells are consistent: the schedule without the reference's intermediate set_BC calls
  bool virt;       // the fused full-domain schedule that leaves the ghost cells virtual (not virt: settle_ghosts first)
  bool captured;   // the handle's regular schedule: what the graphs hold
};
inline bool clean_ghosts(const FieldState& s) { return !s.f_ghosts_dirty && !s.uv_ghosts_dirty; }
inline StepPlan plan_step(const FieldState& s, StepCaps c) {
  return {!s.f_ghosts_dirty, c.full_domain && c.fuse_transport && c.virtual_ghosts && clean_ghosts(s), c.graphs && clean_ghosts(s)};
}
inline void finish_step(FieldState& s, StepPlan p) {
  s.f_ghosts_dirty = s.uv_ghosts_dirty = false;
  s.ghosts_virtual = p.virt;
}

// ---- k_tm's zero maps (kernels/fused_tm.h).  The invariant: a flag is 1 only if the last write to that segment of that array was a
// k_tm store (or skipped store) of zeros.  Every other writer of F or its twin -- a field write, a verb (above), a step in any form
// but the k_tm batches that keep the maps -- leaves the bit set; the one place that enqueues such a batch asks fzmap_take_stale first
// and clears both maps where it says so.
inline void step_wrote_F(FieldState& s) { s.fzmap_stale = true; }   // k_transport, the sweeps of a phased or eager step, k_tm without maps
inline bool fzmap_take_stale(FieldState& s) {
  const bool stale = s.fzmap_stale;
  s.fzmap_stale = false;
  return stale;
}

// ---- the phases of a step (vof_step_phase): 0, 1, 2 in this order; every other kind of step waits for phase 2
inline bool phased_step_in_progress(const FieldState& s) { return s.next_phase != 0; }
inline bool phase_is_next(const FieldState& s, int phase) { return phase == s.next_phase; }
inline void phase_taken(FieldState& s, int phase) {
  s.next_phase = phase == 2 ? 0 : phase + 1;
  if (phase == 2) s.f_ghosts_dirty = s.uv_ghosts_dirty = false;   // the phases carry every set_BC of the step
}

}  // namespace vof
