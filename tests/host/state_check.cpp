// Stand-alone check (host compiler, no HIP) of runtime/state.h: every combination of the flags x what the handle can do x every
// field, written as a whole or in rows, against the expressions the runtime held before state.h existed, restated literally
// (line numbers: commit c4c5476); and the order of the phases.  Exit status 0 and "ok" on success; the first failing checks are
// printed otherwise.
#include <cstdio>

#include "runtime/state.h"

using namespace vof;

static int failures = 0;
#define CHECK(cond, ...)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      if (failures++ < 20) { std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                               \
  } while (0)

// The handle as it was: the six loose members of vof2d_ctx (runtime/context.h:269-297) and what the expressions looked at
struct Before {
  bool f_ghosts_dirty, uv_ghosts_dirty, ghosts_virtual, alt_dirty, ahead;
  int next_phase;
  bool wall_lo, wall_hi;          // h->g.wall_lo, h->g.wall_hi
  int fuse_transport, virtual_ghosts;
  bool forgot;                    // forget_batch_form was called
};
// runtime/schedule.h:408-411
static bool step_leaves_ghosts_virtual(const Before* h) {
  return h->wall_lo && h->wall_hi && h->fuse_transport &&
         h->virtual_ghosts && !h->f_ghosts_dirty && !h->uv_ghosts_dirty;
}
// runtime/step.h:213-216 (step_n's prologue; the same lines at :287-290 and :360-361) and :229-231 (the epilogue)
struct PlanBefore { bool lean, virt, captured; };
static PlanBefore prologue_before(const Before* h, bool use_graph) {
  const bool lean = !h->f_ghosts_dirty;
  const bool virt = step_leaves_ghosts_virtual(h);
  const bool captured = use_graph && lean && !h->uv_ghosts_dirty;
  return {lean, virt, captured};
}
static void epilogue_before(Before* h, bool virt) {
  h->f_ghosts_dirty = false;
  h->uv_ghosts_dirty = false;
  h->ghosts_virtual = virt;
}
// vof2d_api.hip:475-477 (vof_set_rows)
static void set_rows_before(Before* h, int id) {
  if (id == fF || id == fF2) { h->f_ghosts_dirty = true; h->forgot = true; }
  if (id == fMX || id == fMY) h->alt_dirty = true;
  if (id == fU || id == fV) h->uv_ghosts_dirty = true;
}
// vof2d_api.hip:531-535 (vof_copy_rows)
static void copy_rows_before(Before* dst, int id) {
  if (dst->wall_lo && dst->wall_hi) {
    if (id == fF) { dst->f_ghosts_dirty = true; dst->forgot = true; }
    if (id == fMX || id == fMY) dst->alt_dirty = true;
    if (id == fU || id == fV) dst->uv_ghosts_dirty = true;
  }
}

static FieldState state_of(const Before& b) {
  FieldState s;
  s.f_ghosts_dirty = b.f_ghosts_dirty; s.uv_ghosts_dirty = b.uv_ghosts_dirty; s.ghosts_virtual = b.ghosts_virtual;
  s.alt_dirty = b.alt_dirty; s.ahead = b.ahead; s.next_phase = b.next_phase;
  return s;
}
static bool same(const FieldState& s, const Before& b) {
  return s.f_ghosts_dirty == b.f_ghosts_dirty && s.uv_ghosts_dirty == b.uv_ghosts_dirty && s.ghosts_virtual == b.ghosts_virtual &&
         s.alt_dirty == b.alt_dirty && s.ahead == b.ahead && s.next_phase == b.next_phase;
}

int main() {
  {   // runtime/context.h:269-297: what a new handle holds
    const FieldState s;
    CHECK(s.f_ghosts_dirty && !s.uv_ghosts_dirty && !s.ghosts_virtual && !s.alt_dirty && !s.ahead && s.next_phase == 0, "initial values");
  }
  long combos = 0;
  for (int flags = 0; flags < 32; ++flags)
    for (int phase = 0; phase < 3; ++phase)
      for (int caps = 0; caps < 32; ++caps) {
        Before b{(flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0, (flags & 16) != 0, phase,
                 (caps & 1) != 0, (caps & 2) != 0, (caps >> 2) & 1, (caps >> 3) & 1, false};
        const bool use_graph = (caps & 16) != 0;
        const StepCaps c{b.wall_lo && b.wall_hi, b.fuse_transport != 0, b.virtual_ghosts != 0, use_graph};
        // ---- the prologue and the epilogue of a step
        const FieldState s0 = state_of(b);
        const StepPlan p = plan_step(s0, c);
        const PlanBefore q = prologue_before(&b, use_graph);
        CHECK(p.lean == q.lean && p.virt == q.virt && p.captured == q.captured, "plan_step: flags %d caps %d", flags, caps);
        CHECK(clean_ghosts(s0) == !(b.f_ghosts_dirty || b.uv_ghosts_dirty), "clean_ghosts: flags %d", flags);   // vof2d_api.hip:829, runtime/comm.h:306
        {
          FieldState s = s0;
          Before a = b;
          finish_step(s, p);
          epilogue_before(&a, q.virt);
          CHECK(same(s, a), "finish_step: flags %d caps %d", flags, caps);
          if (q.captured && q.virt) {   // runtime/step.h:220-224: behind a batch only `h->ghosts_virtual = true`
            Before a2 = b;
            a2.ghosts_virtual = true;
            CHECK(same(s, a2), "finish_step behind a batch: flags %d caps %d", flags, caps);
          }
        }
        // ---- a field written from outside, as a whole or in rows (the flags do not know which), and rows copied from another handle
        for (int id = 0; id < NFIELDS; ++id) {
          FieldState s = s0;
          Before a = b;
          const bool forget = field_written(s, id, c.full_domain, false);
          set_rows_before(&a, id);
          CHECK(same(s, a) && forget == a.forgot, "field_written(%d): flags %d caps %d", id, flags, caps);
          s = s0;
          a = b;
          const bool forget2 = field_written(s, id, c.full_domain, true);
          copy_rows_before(&a, id);
          CHECK(same(s, a) && forget2 == a.forgot, "field_written(%d, rows of another handle): flags %d caps %d", id, flags, caps);
        }
        // ---- the verbs: vof2d_api.hip:203-205, :248 / :256 / :274, :241, :218 / :225
        {
          FieldState s = s0; Before a = b;
          bc_applied(s);
          a.f_ghosts_dirty = false; a.uv_ghosts_dirty = false; a.ghosts_virtual = false;
          CHECK(same(s, a), "set_BC: flags %d", flags);
          s = s0; a = b;
          verb_wrote_F(s);
          a.f_ghosts_dirty = true;
          CHECK(same(s, a), "a verb that wrote F: flags %d", flags);
          s = s0; a = b;
          verb_wrote_uv(s);
          a.uv_ghosts_dirty = true;
          CHECK(same(s, a), "update_uv: flags %d", flags);
          s = s0; a = b;
          verb_wrote_alt(s);
          a.alt_dirty = true;
          CHECK(same(s, a), "a verb that wrote mx, my: flags %d", flags);
        }
        // ---- the phases: vof2d_api.hip:281 (and five more), :287, :294-295
        CHECK(phased_step_in_progress(s0) == (b.next_phase != 0), "phased_step_in_progress: phase %d", phase);
        for (int ph = 0; ph < 3; ++ph) {
          CHECK(phase_is_next(s0, ph) == !(ph != b.next_phase), "phase_is_next(%d): next %d", ph, phase);
          FieldState s = s0; Before a = b;
          phase_taken(s, ph);
          a.next_phase = ph == 2 ? 0 : ph + 1;
          if (ph == 2) a.f_ghosts_dirty = a.uv_ghosts_dirty = false;
          CHECK(same(s, a), "phase_taken(%d): flags %d", ph, flags);
        }
        ++combos;
      }
  {   // the order 0, 1, 2, twice, and every call out of order refused on the way
    FieldState s;
    for (int round = 0; round < 2; ++round)
      for (int ph = 0; ph < 3; ++ph) {
        CHECK(phased_step_in_progress(s) == (ph != 0), "round %d phase %d", round, ph);
        for (int other = -1; other < 4; ++other) CHECK(phase_is_next(s, other) == (other == ph), "phase %d asked while %d is next", other, ph);
        phase_taken(s, ph);
      }
    CHECK(!phased_step_in_progress(s) && !s.f_ghosts_dirty && !s.uv_ghosts_dirty, "behind phase 2");
  }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("%ld combinations ok\n", combos);
  return 0;
}
