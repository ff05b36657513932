// runtime/views.h -- the handle's view of its field arrays (which buffer of a pair the host calls the first), and the keyed
// store of the graphs captured against a view
//
// A captured graph holds raw pointers, and four pairs of arrays trade places under it: F / its twin, p / pt, (u*, v*) / (mx, my),
// rhs / kappa.  The four swaps below are the only places an entry of the table changes after creation; each flips one bit, and
// every graph is kept under {kind, all four bits, what else the kind bakes in}: a graph is found only while the views are what
// they were at its capture.
//
// Plain C++ (no HIP): the host runtime includes it through context.h, the CPU tests compile it on its own
// (tests/host/views_check.cpp).
#pragma once
#include <cstddef>
#include <map>
#include <tuple>

#include "state.h"

namespace vof {

// ---- the views: a value (capture_graph keeps a copy and puts it back)
class FieldViews {
 public:
  enum : unsigned { kF = 1, kP = 2, kS = 4, kR = 8 };   // the pair is the other way round from creation
  using Table = void*[NFIELDS];
  FieldViews() = default;
  FieldViews(char* arena, size_t field_bytes) {
    for (int k = 0; k < NFIELDS; ++k) fld_[k] = arena + (size_t)k * field_bytes;
  }
  const Table& table() const { return fld_; }
  unsigned bits() const { return bits_; }
  void swap_F() { swap(fF, fF2, kF); }
  void swap_P() { swap(fP, fPT, kP); }
  void swap_S() { swap(fUS, fMX, kS); swap(fVS, fMY, 0); }
  // ... and rhs with the (otherwise verb-only) kappa array: the chained k_tm batches, whose every launch leaves the
  // previous step's u*, v*, rhs intact beside the next step's (enqueue_steps_tm)
  void swap_SR() { swap_S(); swap(fRHS, fKAPPA, kR); }

 private:
  void swap(int a, int b, unsigned bit) {
    void* t = fld_[a]; fld_[a] = fld_[b]; fld_[b] = t;
    bits_ ^= bit;
  }
  Table fld_ = {};
  unsigned bits_ = 0;
};

// ---- the graphs.  The kinds that captured send / recv nodes (they hold the communicator) come last: gXchg and up.
enum GraphKind { gStep = 0, gBatch, gPhase, gMg, gStepMg, gXchg, gXchg2, gXchg5 };
// variant: what the kind bakes in besides the views, packed by the call site (runtime/graphs.h)
struct GraphKey {
  int kind;
  unsigned views;
  int variant;
  bool operator<(const GraphKey& o) const { return std::tie(kind, views, variant) < std::tie(o.kind, o.views, o.variant); }
};

// Exec: a pointer-like graph handle (null: none).  Destroy: quiesce() waits for everything that may still be replaying a
// graph, operator()(Exec) destroys one.  Graphs leave through clear_if alone, which calls quiesce() once in front of the
// first it destroys.  A kind holds at most kCap graphs -- a bound on memory (a caller sweeping the cycle count of
// vof_step_mg would otherwise grow the store without limit): the slot of one more clears the kind first.
template <typename Exec, typename Destroy>
class GraphStore {
 public:
  static constexpr int kCap = 16;
  explicit GraphStore(Destroy d = Destroy()) : destroy_(d) {}
  GraphStore(const GraphStore&) = delete;
  GraphStore& operator=(const GraphStore&) = delete;

  Exec find(const GraphKey& k) const {
    const auto it = m_.find(k);
    return it == m_.end() ? Exec() : it->second;
  }
  // where the graph of k is, or is to be captured into (null then, and after a failed capture); stays valid until the entry leaves
  Exec& slot(const GraphKey& k) {
    const auto it = m_.find(k);
    if (it != m_.end()) return it->second;
    int n = 0;
    for (const auto& e : m_) n += e.first.kind == k.kind;
    if (n >= kCap) clear_kind(k.kind);
    return m_[k];
  }
  bool any() const {
    for (const auto& e : m_)
      if (e.second) return true;
    return false;
  }
  template <typename Pred>
  void clear_if(Pred&& pred) {
    bool quiet = false;
    for (auto it = m_.begin(); it != m_.end();) {
      if (!pred(it->first)) { ++it; continue; }
      if (it->second) {
        if (!quiet) destroy_.quiesce();
        quiet = true;
        destroy_(it->second);
      }
      it = m_.erase(it);
    }
  }
  void clear_kind(int kind) { clear_if([kind](const GraphKey& k) { return k.kind == kind; }); }
  void clear() { clear_if([](const GraphKey&) { return true; }); }

 private:
  std::map<GraphKey, Exec> m_;
  Destroy destroy_;
};

}  // namespace vof
