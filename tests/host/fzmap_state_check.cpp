// Stand-alone check (host compiler, no HIP) of the zero-map bit of runtime/state.h (FieldState::fzmap_stale), the companion of
// state_check.cpp: the invariant "a flag is 1 only if the last write to that segment of that array was a k_tm store of zeros" holds
// on the host if every writer of F or its twin other than a map-keeping k_tm batch leaves the bit set, and only the batch's
// prologue (fzmap_take_stale) takes it away.  Every transition, from both values of the bit and over every other flag, against
// that statement.  Exit status 0 and "ok" on success; the first failing checks are printed otherwise.
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

static FieldState state_of(int bits, bool stale) {
  FieldState s;
  s.f_ghosts_dirty = bits & 1; s.uv_ghosts_dirty = bits & 2; s.ghosts_virtual = bits & 4; s.alt_dirty = bits & 8; s.ahead = bits & 16;
  s.fzmap_stale = stale;
  return s;
}
static bool others_same(const FieldState& a, const FieldState& b) {
  return a.f_ghosts_dirty == b.f_ghosts_dirty && a.uv_ghosts_dirty == b.uv_ghosts_dirty && a.ghosts_virtual == b.ghosts_virtual &&
         a.alt_dirty == b.alt_dirty && a.ahead == b.ahead && a.next_phase == b.next_phase;
}

int main() {
  {   // a new handle: nothing is known about its F
    const FieldState s;
    CHECK(s.fzmap_stale, "a new handle starts stale");
  }
  for (int bits = 0; bits < 32; ++bits)
    for (int stale = 0; stale < 2; ++stale) {
      const FieldState s0 = state_of(bits, stale != 0);
      // a field written from outside: F or its twin, whole or in rows, full domain or strip -- stale; any other field: as it was
      for (int id = 0; id < NFIELDS; ++id)
        for (int full = 0; full < 2; ++full)
          for (int rows = 0; rows < 2; ++rows) {
            FieldState s = s0;
            (void)field_written(s, id, full != 0, rows != 0);
            const bool f = id == fF || id == fF2;
            CHECK(s.fzmap_stale == (f || s0.fzmap_stale), "field_written id %d full %d rows %d from %d", id, full, rows, stale);
          }
      {   // the verbs that write F (the FCT sweeps, post_process_f)
        FieldState s = s0;
        verb_wrote_F(s);
        CHECK(s.fzmap_stale && s.f_ghosts_dirty, "verb_wrote_F");
      }
      {   // a step in any form that keeps no map
        FieldState s = s0;
        step_wrote_F(s);
        CHECK(s.fzmap_stale && others_same(s, s0), "step_wrote_F changes the one bit");
      }
      {   // the verbs and calls that do not write F leave the bit alone
        FieldState s = s0;
        verb_wrote_uv(s); verb_wrote_alt(s); bc_applied(s);
        CHECK(s.fzmap_stale == s0.fzmap_stale, "verbs that leave F alone");
        for (int lean = 0; lean < 2; ++lean) {
          FieldState t = s0;
          finish_step(t, StepPlan{lean != 0, lean != 0, lean != 0});
          CHECK(t.fzmap_stale == s0.fzmap_stale, "finish_step says nothing about who wrote F");
        }
        for (int ph = 0; ph < 3; ++ph) {
          FieldState t = s0;
          phase_taken(t, ph);
          CHECK(t.fzmap_stale == s0.fzmap_stale, "phase_taken");
        }
      }
      {   // the prologue of a map-keeping batch: reports the bit once, leaves it clear, touches nothing else
        FieldState s = s0;
        const bool first = fzmap_take_stale(s);
        CHECK(first == s0.fzmap_stale && !s.fzmap_stale && others_same(s, s0), "fzmap_take_stale");
        CHECK(!fzmap_take_stale(s) && !s.fzmap_stale, "a second batch in a row clears nothing");
        // ... and any writer in between makes the next batch clear again
        step_wrote_F(s);
        CHECK(fzmap_take_stale(s), "batch, other step, batch");
        (void)field_written(s, fF2, true, true);
        CHECK(fzmap_take_stale(s), "batch, rows copied into the twin alone, batch");
        verb_wrote_F(s);
        CHECK(fzmap_take_stale(s), "batch, sweep, batch");
      }
    }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
