// runtime/comm.h -- strips over RCCL: run-time binding (dlopen), the halo send/recv groups, the step with its exchanges
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
#pragma once
#include "step.h"

namespace {

// ---- RCCL, bound at run time (dlopen): the library has no link-time dependency on it, and a
// process that already carries an RCCL (PyTorch's) shares that copy instead of loading a second.
struct Rccl {
  void* dl = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, RcclId, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*GetVersion)(int*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  int version = 0;
  char why[256] = "";
};
Rccl* rccl_bind(Rccl& r);
Rccl* rccl() {
  // C++11 magic static: the binding happens once, also when two handles are created on two threads
  static Rccl r;
  static Rccl* const bound = rccl_bind(r);
  return bound;
}
Rccl* rccl_bind(Rccl& r) {
  const char* cands[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  const char* forced = getenv("VOF2D_RCCL");
  void* dl = (forced && *forced) ? dlopen(forced, RTLD_NOW | RTLD_LOCAL)
                                 : dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);  // a copy the process already mapped
  for (size_t k = 0; !dl && k < sizeof(cands) / sizeof(cands[0]); ++k) dl = dlopen(cands[k], RTLD_NOW | RTLD_LOCAL);
  if (!dl) { snprintf(r.why, sizeof(r.why), "librccl.so.1 not found: %s", dlerror()); return nullptr; }
#define SYM(field, name)                                                              \
  do {                                                                                \
    *reinterpret_cast<void**>(&r.field) = dlsym(dl, name);                            \
    if (!r.field) { snprintf(r.why, sizeof(r.why), "RCCL lacks %s", name); dlclose(dl); return nullptr; } \
  } while (0)
  SYM(GetUniqueId, "ncclGetUniqueId"); SYM(CommInitRank, "ncclCommInitRank"); SYM(CommDestroy, "ncclCommDestroy");
  SYM(Send, "ncclSend"); SYM(Recv, "ncclRecv"); SYM(GroupStart, "ncclGroupStart"); SYM(GroupEnd, "ncclGroupEnd");
  SYM(GetErrorString, "ncclGetErrorString"); SYM(AllReduce, "ncclAllReduce"); SYM(GetVersion, "ncclGetVersion");
#undef SYM
  (void)r.GetVersion(&r.version);
  r.dl = dl;
  return &r;
}

#define NCCLCHK(h, call)                                                                         \
  do {                                                                                           \
    int r_ = (call);                                                                             \
    if (r_ != 0) {                                                                               \
      snprintf((h)->err, sizeof((h)->err), "%s:%d %s -> %s", __FILE__, __LINE__, #call,          \
               rccl()->GetErrorString(r_));                                                      \
      return VOF_EHIP;                                                                           \
    }                                                                                            \
  } while (0)

void comm_teardown(vof2d_ctx* h) {
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->cstream) (void)hipStreamSynchronize(h->cstream);
  h->graphs.clear_if([](const GraphKey& k) { return k.kind >= gXchg; });  // captured send/recv nodes hold the communicator: they go first
  if (h->comm && rccl()) (void)rccl()->CommDestroy(h->comm);
  h->comm = nullptr;
  if (h->ev_ready) (void)hipEventDestroy(h->ev_ready);
  if (h->ev_done) (void)hipEventDestroy(h->ev_done);
  for (int k = 0; k < 3; ++k) {
    if (h->ev_fork[k]) (void)hipEventDestroy(h->ev_fork[k]);
    h->ev_fork[k] = nullptr;
  }
  if (h->cstream) (void)hipStreamDestroy(h->cstream);
  h->ev_ready = h->ev_done = nullptr;
  h->cstream = nullptr;
  h->peer_lo = h->peer_hi = -1;
}

// Halo exchange of the fields in `mask` with both neighbours: W = VOF_HALO_ROWS owned rows out, W
// halo rows in, per side -- a row is `pitch` contiguous elements, so each message is one contiguous
// block of field memory (no packing).  One RCCL group on the communication stream, ordered after
// everything enqueued on the compute stream so far; the compute stream does not wait (comm_join).
// (s_in_alt: between the launches of k_tm and the host's swap the new u*, v* still live in the mx / my arrays;
// on_cstream: whatever the messages wait for was enqueued on the communication stream itself)
constexpr int kTmBandRows = 6;    // rows per pair chunk of k_tm's edge-band launch
constexpr int kTmReachRows = 8;   // halo rows of F, u*, v* the marches of k_tm read beyond the owned rows (3 + 3 + 1: x pipeline, momentum window, faces)
// shallow: F, u*, v* travel kTmReachRows deep only (mode 5's middle steps: all k_tm reads of them; p and rhs serve the ten
// sweeps in front of it and travel W deep)
int comm_post(vof2d_ctx* h, unsigned mask, bool f_in_twin = false, int fork = -1, bool s_in_alt = false, bool on_cstream = false, bool shallow = false) {
  Rccl* r = rccl();
  const int W = VOF_HALO_ROWS(h->d.jacobi_iters);
  const size_t row_bytes = (size_t)h->g.pitch * h->esz;
  if (!on_cstream) {
    hipEvent_t ready = fork >= 0 ? h->ev_fork[fork] : h->ev_ready;
    HIPCHK(h, hipEventRecord(ready, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->cstream, ready, 0));
  }
  static const int ids[7] = {fF, fU, fV, fP, fUS, fVS, fRHS};
  NCCLCHK(h, r->GroupStart());
  // Inside the group no early return: a failing send / recv must still be followed by GroupEnd, or
  // the next (eager) exchange would nest inside the group left open and never be issued.
  int first_err = 0;
  const char* what = "";
  auto note = [&](int rc, const char* call) { if (rc != 0 && first_err == 0) { first_err = rc; what = call; } };
  for (int k = 0; k < 7; ++k) {
    if (!(mask & (1u << k))) continue;
    // between the two transport phases the new F still lives in the twin buffer
    const int id = (k == 0 && f_in_twin) ? fF2 : (k == 4 && s_in_alt) ? fMX : (k == 5 && s_in_alt) ? fMY : ids[k];
    char* base = reinterpret_cast<char*>(h->fld[id]);
    auto row = [&](int g) { return base + (size_t)(g - h->d.row_lo) * row_bytes; };
    const int D = (shallow && (k == 0 || k == 4 || k == 5) && kTmReachRows < W) ? kTmReachRows : W;   // rows of this field
    const size_t bytes = (size_t)D * row_bytes;
    if (h->peer_lo >= 0) {
      note(r->Send(row(h->d.own_lo), bytes, /*ncclInt8*/ 0, h->peer_lo, h->comm, h->cstream), "ncclSend(lo)");
      note(r->Recv(row(h->d.own_lo - D), bytes, 0, h->peer_lo, h->comm, h->cstream), "ncclRecv(lo)");
    }
    if (h->peer_hi >= 0) {
      note(r->Send(row(h->d.own_hi - D + 1), bytes, 0, h->peer_hi, h->comm, h->cstream), "ncclSend(hi)");
      note(r->Recv(row(h->d.own_hi + 1), bytes, 0, h->peer_hi, h->comm, h->cstream), "ncclRecv(hi)");
    }
  }
  note(r->GroupEnd(), "ncclGroupEnd");
  if (first_err != 0) {
    snprintf(h->err, sizeof(h->err), "halo exchange: %s -> %s", what, r->GetErrorString(first_err));
    return VOF_EHIP;
  }
  return VOF_OK;
}
// the compute stream waits for every exchange posted so far
int comm_join(vof2d_ctx* h) {
  HIPCHK(h, hipEventRecord(h->ev_done, h->cstream));
  HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_done, 0));
  return VOF_OK;
}


// The end of a step whose p is final, by the fused transport (update_uv + both sweeps in one pass), edge bands first:
// p, u, v and F (from the twin buffer) leave as soon as the bands exist and travel under the transport of the
// remaining rows.  One group for all four fields: p has been final since the pressure solve, but a separate fork for
// it costs more (a 6-12 us gap on the compute queue) than its 1/4 of the bytes.
template <typename T>
int enqueue_transport_exchange(vof2d_ctx* h) {
  int rc;
  const bool y_first = (h->istep % 2 == 0);
  transport_part<T>(h, y_first, kEdgeBands);
  if ((rc = comm_post(h, VOF_XCHG_P | VOF_XCHG_F | VOF_XCHG_U | VOF_XCHG_V, /*f_in_twin=*/true, 1))) return rc;
  transport_part<T>(h, y_first, kRest);
  h->views.swap_F();
  if ((rc = comm_join(h))) return rc;
  if (!h->virtual_ghosts) L<T>::template set_bc<BC_ALL>(h);
  return VOF_OK;
}

// One step with its exchanges on (compute stream, communication stream).  mode 0: one exchange of
// all four fields after the step; 1: each field leaves as soon as it is final (p after phase 0,
// u, v after phase 1, F after phase 2); 3: p, u, v together after phase 1, F after phase 2 (one fork
// less); 4: the fused transport, edge bands first, one group for all four fields (the default of the
// drivers).  Enqueued eagerly or under stream capture.
template <typename T>
int enqueue_step_exchange(vof2d_ctx* h, int mode) {
  int rc;
  // lean phases (no boundary launch inside): the rows travel with whatever ghost columns they
  // have, and one set_bc<u,v,F,p> over all stored rows -- owned and received alike -- follows the
  // join.  Only reached on steps that start with consistent F ghosts (vof_step_exchange).
  // With virtual ghosts (see enqueue_step) even that launch goes: the rows travel with stale ghost
  // columns and the next step's k_momentum forms the ones it reads, for owned and received rows alike.
  const bool lean = true;
  const bool virt = h->virtual_ghosts != 0;
  enqueue_phase<T>(h, 0, h->istep, false, lean, virt, (int)(h->istep & 1));
  if (mode == 4) return enqueue_transport_exchange<T>(h);
  if (mode == 1 && (rc = comm_post(h, VOF_XCHG_P, false, 0))) return rc;   // p is final
  enqueue_phase<T>(h, 1, h->istep, false, lean);
  if (mode && (rc = comm_post(h, mode == 3 ? (VOF_XCHG_P | VOF_XCHG_U | VOF_XCHG_V) : (VOF_XCHG_U | VOF_XCHG_V), false, 1))) return rc;  // u, v are final
  enqueue_phase<T>(h, 2, h->istep, false, lean);
  if ((rc = comm_post(h, mode ? VOF_XCHG_F : (VOF_XCHG_F | VOF_XCHG_U | VOF_XCHG_V | VOF_XCHG_P), false, 2))) return rc;
  if ((rc = comm_join(h))) return rc;           // halos complete before the next step
  if (lean && !virt) L<T>::template set_bc<BC_ALL>(h);
  return VOF_OK;
}

// ---- overlap mode 5: the strips run the pair kernels (include/vof2d.h, vof_step_exchange) ----
// the first step's k_momentum: u*, v*, rhs of the owned rows (their halo rows arrive by exchange: mode 5's state)
template <typename T>
void tm5_head(vof2d_ctx* h) {
  // The middle steps alternate u*, v* between their own arrays and mx, my, and a call may end with the host's view on
  // the second pair: the cells the predictor never writes (u* on i = 1, v* on j = 1, ny + 1, the ghost cells) must hold
  // the zeros the reference's never-written entries hold (S5), not what a verb (get_normal_young) left there.
  if (h->state.alt_dirty) {
    (void)hipMemsetAsync(h->fld[fMX], 0, h->field_elems * h->esz, h->stream);
    (void)hipMemsetAsync(h->fld[fMY], 0, h->field_elems * h->esz, h->stream);
    h->state.alt_dirty = false;
  }
  const RowRange o = strip_rows(h).owned;
  L<T>::momentum(h, true, (int)((h->istep + 1) & 1), L<T>::plan_for_tm(h), o.first, o.last);    // (the planner block plans the geometry of the kernel that will run)
}
// the sweeps of a middle step on all stored rows: batch_jacobi (runtime/schedule.h), in uniform chunks where the pair kernel does not apply
template <typename T>
void tm5_jacobi(vof2d_ctx* h, int par) { batch_jacobi<T>(h, par, -1); }
// k_tm on one part of the owned rows (runtime/rows.h); the launch of the body carries the planner block
template <typename T>
void tm5_tm(vof2d_ctx* h, int64_t istep, int part) {
  const PartRows pr = part_rows(strip_rows(h), part);
  const bool y_first = (istep % 2 == 0);
  const PlanFor plan_for = L<T>::plan_for_tm(h);
  if (!pr.body.empty()) L<T>::tm(h, y_first, false, (int)((istep + 1) & 1), plan_for, fRHS, pr.body.first, pr.body.last);
  // both bands in ONE launch, in short chunks (a pair's march is its rows + 14 steps whatever its rows: the bands are
  // what the send / recv group waits for -- 8192-wide interior strip of 8: two launches of 18-row chunks 56 + 69 us)
  const RowRange b1 = pr.band_lo.empty() ? pr.band_hi : pr.band_lo, b2 = pr.band_lo.empty() ? kNoRows : pr.band_hi;
  if (!b1.empty()) L<T>::tm(h, y_first, false, -1, plan_for, fRHS, b1.first, b1.last, kTmBandRows, b2.first, b2.last);
}
// one middle step with its exchange: the edge bands on the communication stream in front of the send / recv group,
// the other rows on the compute stream beside them (launches of k_tm on disjoint rows read the old arrays and write
// the new ones: they do not depend on each other)
template <typename T>
int enqueue_mid_step5(vof2d_ctx* h) {
  int rc;
  tm5_jacobi<T>(h, (int)(h->istep & 1));
  HIPCHK(h, hipEventRecord(h->ev_fork[1], h->stream));
  HIPCHK(h, hipStreamWaitEvent(h->cstream, h->ev_fork[1], 0));
  { StreamScope on(h, h->cstream); tm5_tm<T>(h, h->istep, 1); }
  if ((rc = comm_post(h, VOF_XCHG_F | VOF_XCHG_US | VOF_XCHG_VS | VOF_XCHG_RHS | VOF_XCHG_P, /*f_in_twin=*/true, 1, /*s_in_alt=*/true, /*on_cstream=*/true, /*shallow=*/true))) return rc;
  tm5_tm<T>(h, h->istep, 2);
  h->views.swap_F();
  h->views.swap_S();
  return comm_join(h);
}
// the last step of a call: mode 4's step without its k_momentum (u, v reach memory here)
template <typename T>
int enqueue_tail_step5(vof2d_ctx* h) {
  jacobi_n<T>(h, h->d.jacobi_iters, false, -1);     // (uniform chunks: the plan in memory is of the pairs' geometry)
  return enqueue_transport_exchange<T>(h);
}

// ---- the steps of a strip with their exchanges (vof_step_exchange)
// a capture that failed after the fork may leave a communication stream inside the invalidated capture: the eager launches
// that follow need working ones
bool comm_streams_usable_after_failed_capture(vof2d_ctx* h) {
  for (hipStream_t* st : {&h->cstream}) {
    if (!*st) continue;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(*st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
      (void)hipGetLastError();
      (void)hipStreamDestroy(*st);
      *st = nullptr;
      if (hipStreamCreateWithFlags(st, hipStreamNonBlocking) != hipSuccess) return false;
    }
  }
  return true;
}
// Captures the steps `enqueue` launches, exchanges included, into *slot -- or, if this RCCL / runtime cannot capture them,
// switches the form off (*form_on = 0) and leaves the caller to carry on with `fallback`.  An error only where not even
// that is possible.
template <typename Enqueue>
int capture_exchange_or_switch_off(vof2d_ctx* h, hipGraphExec_t* slot, int* form_on, const char* what, const char* fallback, Enqueue&& enqueue) {
  const bool dbg = getenv("VOF2D_DEBUG") != nullptr;
  if (dbg) fprintf(stderr, "[vof2d] capturing %s (parity %d)\n", what, (int)(h->istep & 1));
  const hipError_t e = capture_graph(h, hipStreamCaptureModeRelaxed, /*upload=*/false, slot, [&] {
    const int rc = enqueue();
    if (dbg) fprintf(stderr, "[vof2d]   enqueued (rc %d), ending capture\n", rc);
    return rc == VOF_OK;
  });
  if (e == hipSuccess) return VOF_OK;
  (void)hipGetLastError();
  *form_on = 0;
  if (!comm_streams_usable_after_failed_capture(h)) return fail(h, VOF_EHIP, "cannot recreate the communication stream after a failed capture");
  if (dbg) fprintf(stderr, "[vof2d] capture of %s failed (%s / %s): %s\n", what, hipGetErrorString(e), h->err, fallback);
  return VOF_OK;
}

// the kernels of mode 5 need: two-column tiles whose lanes are stored or skipped together, square cells or not (k_jacobi_pair
// falls back to two k_jacobi_tb launches), the fused transport and its virtual ghosts
// plan_step for the steps of a strip with their exchanges.  The difference: a captured step runs lean with the boundary launch
// left out wherever the knob says so, whatever the transport (enqueue_step_exchange) -- virt does not ask for a full domain
// or the fused transport as plan_step's does.  The steps of mode 5 and of vof_step_tm_piece are of this kind too, captured or
// not (graphs = true): both entry points have seen to it that nothing is dirty.
StepPlan strip_step_plan(const vof2d_ctx* h, bool graphs) {
  StepPlan p = plan_step(h->state, step_caps(h, graphs));
  p.virt = p.captured && h->virtual_ghosts;
  return p;
}
bool mode5_ok(const vof2d_ctx* h) {
  return h->fuse_transport && h->tb >= 5 && h->d.jacobi_iters % 5 == 0 && h->d.jacobi_iters >= 5 && h->g.nx >= 16;
}
// n steps of mode 5: see include/vof2d.h.  The middle steps are replayed two per hipGraph launch (all three pairs of
// arrays -- F / twin, u* v* / mx my, p / pt -- are back where they were after two steps); the head and the tail of a
// call, and an odd middle step, are launched eagerly.
int step_exchange_mode5(vof2d_ctx* h, int64_t nsteps) {
  int rc;
  if (!mode5_ok(h)) return fail(h, VOF_ESTATE, "overlap mode 5 needs the fused transport and five-sweep Jacobi launches");
  if (nsteps == 0) return VOF_OK;
  if (!clean_ghosts(h->state) || h->xchg_steps == 0) {
    // the first step after set_init_F / set_field (the reference's intermediate set_BC calls), and the first of a
    // communicator (RCCL connects on first use): a step of mode 1
    if ((rc = vof_step_exchange(h, 1, 1))) return rc;
    if (--nsteps == 0) return VOF_OK;
  }
  const bool want_graph = !(h->d.flags & VOF_FLAG_NO_GRAPH) && h->xchg_graph;
  // head
  DISPATCH_T(h, tm5_head<double>(h), tm5_head<float>(h));
  if ((rc = comm_post(h, VOF_XCHG_US | VOF_XCHG_VS | VOF_XCHG_RHS))) return rc;
  if ((rc = comm_join(h))) return rc;
  int64_t mid = nsteps - 1;
  auto mid_step = [&]() -> int {
    h->istep += 1;
    int r2 = VOF_OK;
    DISPATCH_T(h, r2 = enqueue_mid_step5<double>(h), r2 = enqueue_mid_step5<float>(h));
    return r2;
  };
  auto eager_mid = [&] { h->xchg_steps += 1; return mid_step(); };
  if (mid & 1) { if ((rc = eager_mid())) return rc; mid -= 1; }
  while (mid > 0) {
    hipGraphExec_t& exec = h->graphs.slot(graph_key(h, gXchg5, (int)((h->istep + 1) & 1)));
    if (want_graph && h->xchg5_graph && !exec &&
        (rc = capture_exchange_or_switch_off(h, &exec, &h->xchg5_graph, "two middle steps of mode 5", "eager", [&] { const int r2 = mid_step(); return r2 ? r2 : mid_step(); })))
      return rc;
    if (want_graph && h->xchg5_graph && exec) {
      HIPCHK(h, hipGraphLaunch(exec, h->stream));
      h->istep += 2;
      h->xchg_steps += 2;
      h->xchg_graph_steps += 2;
    } else {
      if ((rc = eager_mid()) || (rc = eager_mid())) return rc;
    }
    mid -= 2;
  }
  // tail
  h->istep += 1;
  DISPATCH_T(h, rc = enqueue_tail_step5<double>(h), rc = enqueue_tail_step5<float>(h));
  if (rc) return rc;
  h->xchg_steps += 1;
  finish_step(h->state, strip_step_plan(h, true));   // (nothing was dirty: the first step of the call saw to that)
  return ensure_ok(h);
}

// nsteps steps of overlap mode 0, 1, 3 or 4, each with its exchanges
int step_exchange(vof2d_ctx* h, int64_t nsteps, int overlap) {
  const bool want_graph = !(h->d.flags & VOF_FLAG_NO_GRAPH);
  auto& G = h->graphs;
  auto one_step = [&]() -> int {
    int r2 = VOF_OK;
    DISPATCH_T(h, r2 = enqueue_step_exchange<double>(h, overlap), r2 = enqueue_step_exchange<float>(h, overlap));
    return r2;
  };
  for (int64_t s = 0; s < nsteps; ++s) {
    // the captured step leaves the ghost cells virtual (if the handle does that at all); every other
    // way through this loop wants them settled first
    const StepPlan p = strip_step_plan(h, want_graph && h->xchg_graph && h->xchg_steps > 0);
    if (!p.virt) settle_ghosts(h);
    h->istep += 1;   // (behind settle_ghosts here, in front of it in step_loop: settle_ghosts does not look at istep)
    const int par = (int)(h->istep & 1);
    const GraphKey one = graph_key(h, gXchg, overlap * 2 + par), next = {gXchg, one.views ^ FieldViews::kF, one.variant ^ 1};   // this step's graph, and (mode 4) the next step's
    int rc;
    // The first step of a communicator runs eagerly: RCCL sets its peer connections up on first
    // use, which must not happen inside a capture.  After that the whole step -- kernels on the
    // compute stream, the send/recv groups forked onto the communication stream, the join -- is
    // one hipGraph per (sweep order, mode): one launch per step instead of four graph launches
    // and three RCCL group launches (~100 us of host time each).
    // Two mode-4 steps per graph launch (a graph launch leaves ~9 us of idle queue behind it, see step.h):
    // only once both single-step graphs of this handle exist, i.e. this RCCL has shown that it can be
    // captured; two steps return the F / twin pair and the parity to where they were.
    if (p.captured && overlap == 4 && h->xchg_pair && p.virt && nsteps - s >= 2 && G.find(one) && G.find(next)) {
      hipGraphExec_t& two = G.slot(graph_key(h, gXchg2, par));
      if (!two &&
          (rc = capture_exchange_or_switch_off(h, &two, &h->xchg_pair, "two steps + exchanges", "one step per launch (those graphs are known to work)", [&] {
             const int r2 = one_step();
             h->istep += 1;
             return r2 ? r2 : one_step();
           })))
        return rc;
      if (two) {
        HIPCHK(h, hipGraphLaunch(two, h->stream));
        h->istep += 1;
        s += 1;
        h->xchg_steps += 2;
        h->xchg_graph_steps += 2;
        finish_step(h->state, p);
        continue;
      }
    }
    if (p.captured) {
      hipGraphExec_t& exec = G.slot(one);
      if (!exec && (rc = capture_exchange_or_switch_off(h, &exec, &h->xchg_graph, "step + exchanges", "eager", one_step))) return rc;
      if (exec) {
        HIPCHK(h, hipGraphLaunch(exec, h->stream));
        if (overlap == 4) h->views.swap_F();   // the fused transport swaps the F / twin pair once per step
        h->xchg_steps += 1;
        h->xchg_graph_steps += 1;
        finish_step(h->state, p);
        continue;
      }
    }
    h->istep -= 1;  // vof_step_phase(0) advances it
    const int eo = overlap == 4 ? 1 : overlap;   // eager steps (the first of a communicator, ...) of mode 4 run as mode 1
    if ((rc = vof_step_phase(h, 0))) return rc;
    if (eo == 1 && (rc = comm_post(h, VOF_XCHG_P))) return rc;
    if ((rc = vof_step_phase(h, 1))) return rc;
    if (eo && (rc = comm_post(h, eo == 3 ? (VOF_XCHG_P | VOF_XCHG_U | VOF_XCHG_V) : (VOF_XCHG_U | VOF_XCHG_V)))) return rc;
    if ((rc = vof_step_phase(h, 2))) return rc;
    if ((rc = comm_post(h, eo ? VOF_XCHG_F : (VOF_XCHG_F | VOF_XCHG_U | VOF_XCHG_V | VOF_XCHG_P)))) return rc;
    if ((rc = comm_join(h))) return rc;
    h->xchg_steps += 1;
  }
  return VOF_OK;
}

}  // namespace
