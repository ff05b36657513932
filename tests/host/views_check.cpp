// Stand-alone check (host compiler, no HIP) of runtime/views.h.
// (a) The views, over every sequence of up to 6 swaps drawn from the four: the table stays a permutation of the creation
//     pointers; the bits equal what the runtime compared before views.h existed -- each pair's first pointer against its value
//     at creation (ori_F and xchg5_key of runtime/graphs.h at commit 32a67b2, restated literally, and the same for rhs); a copy
//     taken before further swaps and put back restores table and bits (capture_graph).
// (b) The store, with a destroy functor that counts: equal keys share a slot, keys that differ in the kind, in any one view bit
//     or in the variant do not; clearing a kind destroys exactly that kind's graphs, once each, behind one quiesce(); the 17th
//     key of a kind destroys the 16 before it and nothing of another kind; clearing all leaves none alive.
// Exit status 0 and "ok" on success; the first failing checks are printed otherwise.
#include <algorithm>
#include <cstdio>
#include <set>
#include <vector>

#include "runtime/views.h"

using namespace vof;

static int failures = 0;
#define CHECK(cond, ...)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      if (failures++ < 20) { std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                               \
  } while (0)

// ---- (a)
static char arena[NFIELDS * 64];
struct Homes { void *f_home, *us_home, *p_home, *rhs_home; };
// runtime/graphs.h:11 and :14 at 32a67b2
static int ori_F_before(const FieldViews& v, const Homes& h) { return v.table()[fF] == h.f_home ? 0 : 1; }
static unsigned bits_before(const FieldViews& v, const Homes& h) {
  return (unsigned)ori_F_before(v, h) * FieldViews::kF | (v.table()[fUS] == h.us_home ? 0 : 1) * FieldViews::kS |
         (v.table()[fP] == h.p_home ? 0 : 1) * FieldViews::kP | (v.table()[fRHS] == h.rhs_home ? 0 : 1) * FieldViews::kR;
}
static void apply(FieldViews& v, int s) {
  if (s == 0) v.swap_F(); else if (s == 1) v.swap_P(); else if (s == 2) v.swap_S(); else v.swap_SR();
}
static bool same_views(const FieldViews& a, const FieldViews& b) {
  return a.bits() == b.bits() && std::equal(a.table(), a.table() + NFIELDS, b.table());
}
static long check_views() {
  const FieldViews fresh(arena, 64);
  const Homes homes{fresh.table()[fF], fresh.table()[fUS], fresh.table()[fP], fresh.table()[fRHS]};
  for (int k = 0; k < NFIELDS; ++k) CHECK(fresh.table()[k] == arena + 64 * k, "creation, field %d", k);
  CHECK(fresh.bits() == 0, "creation bits");
  long seqs = 0;
  for (int len = 0; len <= 6; ++len)
    for (int code = 0; code < (1 << (2 * len)); ++code) {
      FieldViews v = fresh;
      int n[4] = {0, 0, 0, 0};
      for (int k = 0; k < len; ++k) {
        const int s = (code >> (2 * k)) & 3;
        apply(v, s);
        n[s] += 1;
        if (k == len / 2) {   // what a capture does: the views move under the enqueueing, then are put back
          const FieldViews keep = v;
          FieldViews w = v;
          for (int j = k; j < len; ++j) apply(w, (code >> (2 * j)) & 3);
          w = keep;
          CHECK(same_views(w, v), "copy and restore: len %d code %d at %d", len, code, k);
        }
      }
      std::vector<void*> got(v.table(), v.table() + NFIELDS), want(fresh.table(), fresh.table() + NFIELDS);
      std::sort(got.begin(), got.end());
      std::sort(want.begin(), want.end());
      CHECK(got == want, "permutation: len %d code %d", len, code);
      CHECK(v.bits() == bits_before(v, homes), "bits %u, pointers say %u: len %d code %d", v.bits(), bits_before(v, homes), len, code);
      // ... and what the counts of swaps say (swap_SR is S and R together); the arrays no swap names stay put
      const unsigned by_count = (n[0] & 1) * FieldViews::kF | (n[1] & 1) * FieldViews::kP | ((n[2] + n[3]) & 1) * FieldViews::kS | (n[3] & 1) * FieldViews::kR;
      CHECK(v.bits() == by_count, "bits %u, counts say %u: len %d code %d", v.bits(), by_count, len, code);
      CHECK((v.table()[fVS] == fresh.table()[fVS]) == (v.table()[fUS] == fresh.table()[fUS]), "u* and v* move together: len %d code %d", len, code);
      for (int id : {fU, fV, fRHO, fNU}) CHECK(v.table()[id] == fresh.table()[id], "field %d moved: len %d code %d", id, len, code);
      ++seqs;
    }
  return seqs;
}

// ---- (b)
struct Graph { int id; };
struct Log {
  std::vector<int> destroyed;
  int quiesced = 0;
  int quiet_for = 0;   // destroys the last quiesce() still covers: a destroy without one in front of it in the same clear is a failure
};
struct CountingDestroy {
  Log* log;
  void quiesce() { log->quiesced += 1; log->quiet_for = 1 << 30; }
  void operator()(Graph* g) {
    CHECK(log->quiet_for > 0, "graph %d destroyed with no quiesce() in front", g->id);
    log->destroyed.push_back(g->id);
  }
};
using Store = GraphStore<Graph*, CountingDestroy>;

static std::vector<Graph> pool(256);
static Graph* capture_into(Store& s, const GraphKey& k, int id) {
  Graph*& slot = s.slot(k);
  if (!slot) { pool[id].id = id; slot = &pool[id]; }
  return slot;
}
static void check_store() {
  Log log;
  {
    Store s{CountingDestroy{&log}};
    CHECK(!s.any() && s.find({gStep, 0, 0}) == nullptr, "an empty store");
    const GraphKey base{gStepMg, 5u, 9};
    Graph* const g0 = capture_into(s, base, 0);
    CHECK(s.any() && s.find(base) == g0 && capture_into(s, base, 1) == g0 && &s.slot(base) == &s.slot(GraphKey{gStepMg, 5u, 9}), "equal keys, one slot");
    // one field of the key changed at a time: the kind, each of the four view bits, the variant
    std::vector<GraphKey> others = {{gStep, 5u, 9}, {gStepMg, 5u, 8}};
    for (unsigned bit : {FieldViews::kF, FieldViews::kP, FieldViews::kS, FieldViews::kR}) others.push_back({gStepMg, 5u ^ bit, 9});
    std::set<Graph**> slots = {&s.slot(base)};
    int id = 1;
    for (const GraphKey& k : others) {
      CHECK(s.find(k) == nullptr, "key (%d, %u, %d) found before its capture", k.kind, k.views, k.variant);
      Graph* const g = capture_into(s, k, id);
      CHECK(g == &pool[id] && s.find(k) == g && s.find(base) == g0, "key (%d, %u, %d)", k.kind, k.views, k.variant);
      slots.insert(&s.slot(k));
      ++id;
    }
    CHECK(slots.size() == 1 + others.size(), "%zu slots for %zu keys", slots.size(), 1 + others.size());
    CHECK(log.destroyed.empty() && log.quiesced == 0, "nothing destroyed so far");
    // a slot that was asked for and never filled (a failed capture) is not a graph
    s.slot({gPhase, 0u, 3});
    CHECK(s.find({gPhase, 0u, 3}) == nullptr, "an empty slot");
    // clear one kind: gStepMg holds ids 0 and 2 .. 6, gStep holds id 1
    log.quiet_for = 0;
    s.clear_kind(gStepMg);
    std::vector<int> d = log.destroyed;
    std::sort(d.begin(), d.end());
    CHECK((d == std::vector<int>{0, 2, 3, 4, 5, 6}) && log.quiesced == 1, "clear_kind: %zu destroyed, %d quiesce", d.size(), log.quiesced);
    CHECK(s.find(base) == nullptr && s.find({gStep, 5u, 9}) == &pool[1] && s.any(), "clear_kind leaves the other kinds");
    s.clear_kind(gStepMg);
    s.clear_kind(gPhase);   // (only the empty slot: nothing to wait for)
    CHECK(log.destroyed.size() == 6 && log.quiesced == 1, "clearing nothing destroys nothing and waits for nothing");
    // the cap: 16 keys of a kind stay, the slot of the 17th clears the kind -- and only it
    log.destroyed.clear();
    for (int c = 0; c < Store::kCap; ++c) capture_into(s, {gStepMg, 1u, c}, 100 + c);
    capture_into(s, {gMg, 1u, 0}, 99);
    CHECK(log.destroyed.empty(), "16 keys of a kind: none destroyed");
    for (int c = 0; c < Store::kCap; ++c) CHECK(s.find({gStepMg, 1u, c}) == &pool[100 + c], "key %d of 16", c);
    log.quiet_for = 0;
    Graph* const g17 = capture_into(s, {gStepMg, 1u, Store::kCap}, 100 + Store::kCap);
    d = log.destroyed;
    std::sort(d.begin(), d.end());
    std::vector<int> first16;
    for (int c = 0; c < Store::kCap; ++c) first16.push_back(100 + c);
    CHECK(d == first16 && log.quiesced == 2, "the 17th key: %zu destroyed, %d quiesce", d.size(), log.quiesced);
    CHECK(s.find({gStepMg, 1u, Store::kCap}) == g17 && s.find({gStepMg, 1u, 0}) == nullptr, "the 17th key has its slot, the first is gone");
    CHECK(s.find({gMg, 1u, 0}) == &pool[99] && s.find({gStep, 5u, 9}) == &pool[1], "the other kinds stay");
    // by predicate (one form's batches, the kinds that hold the communicator)
    capture_into(s, {gXchg, 0u, 8}, 50); capture_into(s, {gXchg2, 0u, 0}, 51); capture_into(s, {gXchg5, 2u, 1}, 52);
    log.destroyed.clear();
    log.quiet_for = 0;
    s.clear_if([](const GraphKey& k) { return k.kind >= gXchg; });
    d = log.destroyed;
    std::sort(d.begin(), d.end());
    CHECK((d == std::vector<int>{50, 51, 52}) && log.quiesced == 3, "clear_if: %zu destroyed", d.size());
    // clear all: the three that are left, once each
    log.destroyed.clear();
    log.quiet_for = 0;
    s.clear();
    d = log.destroyed;
    std::sort(d.begin(), d.end());
    CHECK((d == std::vector<int>{1, 99, 100 + Store::kCap}) && !s.any(), "clear: %zu destroyed", d.size());
    s.clear();
    CHECK(log.destroyed.size() == 3 && log.quiesced == 4, "a second clear destroys nothing");
  }
  CHECK(log.destroyed.size() == 3, "the store's destructor destroys nothing: the handle clears it first");
}

int main() {
  const long seqs = check_views();
  check_store();
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("%ld swap sequences and the store ok\n", seqs);
  return 0;
}
