// runtime/step.h -- the scheduler behind vof_step, vof_step_phase and vof_profile_steps: which form of the batch graphs a
// handle runs, the batches, and the three ways a step is run (inside a batch, from its own graph, eagerly)
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
#pragma once
#include "groups.h"
#include "schedule.h"
#include "multigrid.h"

namespace {

// Which form of the batch graphs a large fp64 full domain runs (knob fuse_tm = -1, the default): a RULE on the state, so
// that two handles on the same data always run the same schedule.  k_tm + k_jacobi_pair win where most rows are cheap for
// the transport pipeline (gas: the x pipeline bypasses itself, the y stage is skipped) and lose where they are not -- 4096^2
// dam-break (5/6 gas) 0.49 against 0.56 ms/step for the chains, 4096^2 rising bubble (2 % gas) 0.81 against 0.61 -- so the
// rule is the share of exact-zero cells of F when the handle first batches steps (and again after F was replaced from
// outside): one small kernel and one 8-byte read-back, where the graphs are being captured anyway.
// The count is POSTED (kernel + 8-byte copy into pinned host memory + event, all asynchronous) where F is replaced as a
// whole -- vof_set_init_F -- or, failing that, by the first step that needs it; vof_step only waits for the event, which
// after set_init_F has long fired: no device sync inside a timed vof_step.  Anything that fails on the way (a caller's
// stream under capture, no pinned memory) leaves the handle undecided and on the other form: never an error of vof_step.
bool post_gas_count(vof2d_ctx* h) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(h->stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return false; }
  if (!h->h_gas && hipHostMalloc(reinterpret_cast<void**>(&h->h_gas), sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); h->h_gas = nullptr; return false; }
  if (!h->ev_gas && hipEventCreateWithFlags(&h->ev_gas, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); h->ev_gas = nullptr; return false; }
  unsigned long long* cnt = h->d_courant + 3;
  bool ok = hipMemsetAsync(cnt, 0, sizeof(*cnt), h->stream) == hipSuccess;
  const unsigned blocks = (unsigned)(h->g.ihi - h->g.ilo + 1 < 2048 ? h->g.ihi - h->g.ilo + 1 : 2048);
  if (h->d.dtype == VOF_F64) hipLaunchKernelGGL(k_gas_cells<double>, dim3(blocks), dim3(256), 0, h->stream, h->g, (const double*)F_<double>(h, fF), cnt);
  else hipLaunchKernelGGL(k_gas_cells<float>, dim3(blocks), dim3(256), 0, h->stream, h->g, (const float*)F_<float>(h, fF), cnt);
  ok = ok && hipMemcpyAsync(h->h_gas, cnt, sizeof(*cnt), hipMemcpyDeviceToHost, h->stream) == hipSuccess;
  ok = ok && hipEventRecord(h->ev_gas, h->stream) == hipSuccess;
  if (!ok) (void)hipGetLastError();
  h->gas_pending = ok;
  return ok;
}
void decide_batch_form_by_rule(vof2d_ctx* h) {
  if (!h->gas_pending && !post_gas_count(h)) return;
  h->gas_pending = false;
  if (hipEventSynchronize(h->ev_gas) != hipSuccess) { (void)hipGetLastError(); return; }
  const unsigned long long n = *h->h_gas;
  h->gas_share = (double)n / ((double)(h->g.ihi - h->g.ilo + 1) * (double)h->g.ny);
  h->tune.choice = tm_choice_by_rule(h, h->gas_share);
  h->tune.decided = true;
  if (getenv("VOF2D_DEBUG")) fprintf(stderr, "[vof2d] batch form by rule: %.3f of the cells are gas -> %s\n", h->gas_share, h->tune.choice ? "k_tm" : "chains / plain");
}

// fuse_tm = -2: the handle times both forms on its own data -- four batches of step_batch[kTuneBatch] steps, alternating
// -- keeps the faster, and times them again every `period` batches.  True if the batch about to run is a timed one (of
// form tune.n & 1; run_step_batch records the events and counts it); `remaining`: steps left in the call.
bool tune_next_is_timed(vof2d_ctx* h, int64_t remaining) {
  TuneState& t = h->tune;
  if (t.n == 4) {
    bool done = hipEventSynchronize(t.ev[7]) == hipSuccess;
    for (int k = 0; k < 4 && done; ++k) {
      float ms = 0.f;
      done = hipEventElapsedTime(&ms, t.ev[2 * k], t.ev[2 * k + 1]) == hipSuccess;
      t.ms[k & 1] += ms;
    }
    t.choice = (done && t.ms[1] < 0.99f * t.ms[0]) ? 1 : 0;
    t.n = 5;
    t.decided = true;
    if (!done) (void)hipGetLastError();
    if (getenv("VOF2D_DEBUG")) fprintf(stderr, "[vof2d] batch forms timed: %.3f ms (chains / plain) vs %.3f ms (k_tm) per 16 steps -> %s\n", t.ms[0], t.ms[1], t.choice ? "k_tm" : "chains / plain");
  }
  if (t.n == 5 && t.period > 0 && t.age >= t.period) {   // time the forms again (the choice made stands meanwhile)
    t.n = 0; t.age = 0; t.ms[0] = t.ms[1] = 0.f;
  }
  if (t.n < 4) return remaining >= h->step_batch[vof2d_ctx::kTuneBatch];
  t.age += 1;
  return false;
}

// THE form of the batch graphs of a handle, 0: the chains or the plain sequence, 1: k_tm.  In this order: the knob where it
// says so; on "by rule" the rule's decision; on "auto" the timed exploration's; and never the form that could not be captured.
// decide = false only looks (vof_profile_steps): an open decision reads as form 0.  decide = true (a steady-state step of
// vof_step with `remaining` steps to go) takes the rule's decision if it is open and moves the exploration on; *timed is
// set where the batch about to run is one the exploration times.
int batch_form(vof2d_ctx* h, bool decide, int64_t remaining = 0, bool* timed = nullptr) {
  int variant = 0;
  if (h->fuse_tm > 0) variant = tm_eligible(h) ? 1 : 0;
  else if (tm_by_rule(h) || tm_auto(h)) {
    if (decide && tm_by_rule(h) && !h->tune.decided) decide_batch_form_by_rule(h);   // (the count could not be taken: form 0, and another try next call)
    if (decide && tm_auto(h)) *timed = tune_next_is_timed(h, remaining);
    variant = (timed && *timed) ? (h->tune.n & 1) : (h->tune.decided ? h->tune.choice : 0);
  }
  return h->tm_broken ? 0 : variant;
}

// steps per graph launch of batch size b: the chained k_tm batches pay one u, v store per batch and nothing else, so
// their largest is twice the other form's (whose chains drift kHalvesDrift rows per launch: halves_prepare)
int batch_steps(const vof2d_ctx* h, int variant, int b) {
  return (variant && b == 0) ? 2 * h->step_batch[0] : h->step_batch[b];
}
// The batch graphs (batch_steps steady-state steps per launch) of the (parity, orientation) pair the current step
// finds and of the pair the next step will find -- the two pairs a run alternates between; a handle whose parity
// was moved alone (vof_set_istep) gets the other two on its next steady-state step.  Captures enqueue nothing.  Any
// failure on the way switches the form off for the handle and leaves the other form, the single-step graphs (or eager
// launches) to carry on: never an error of vof_step.
void build_step_batches(vof2d_ctx* h, int variant) {
  bool ok = true;
  for (int c = 0; c < 2 && ok; ++c) {
    if (c) h->views.swap_F();                                   // the pair as the NEXT step will find it
    const int64_t first = h->istep + c;
    for (int b = 0; b < vof2d_ctx::kStepBatches && ok; ++b) {
      hipGraphExec_t& slot = h->graphs.slot(graph_key(h, gBatch, batch_variant(variant, b, first)));
      if (slot) continue;
      const int K = batch_steps(h, variant, b);
      const bool chains = !variant && halves_eligible(h, K) && halves_prepare(h, K);
      ok = capture_graph(h, hipStreamCaptureModeThreadLocal, /*upload=*/true, &slot, [&] {
        bool enq = true;
        if (chains) {
          h->halves_captured[b] = true;
          DISPATCH_T(h, enq = enqueue_steps_halves<double>(h, first, K), enq = enqueue_steps_halves<float>(h, first, K));
        } else if (variant) DISPATCH_T(h, enqueue_steps_tm<double>(h, first, K), enqueue_steps_tm<float>(h, first, K));
        else
          for (int k = 0; k < K; ++k)
            DISPATCH_T(h, enqueue_step<double>(h, first + k, true, true), enqueue_step<float>(h, first + k, true, true));
        return enq;
      }) == hipSuccess;
    }
    if (c) h->views.swap_F();
  }
  if (!ok) {
    (void)hipGetLastError();
    h->graphs.clear_if([variant](const GraphKey& k) { return k.kind == gBatch && batch_form_of(k) == variant; });
    // the k_tm form failing leaves the other form's batch graphs in use; only when those fail is it one graph launch per step
    if (variant) h->tm_broken = true; else h->batching = false;
    if (getenv("VOF2D_DEBUG")) fprintf(stderr, "[vof2d] step batches (%s) could not be captured: %s\n", variant ? "k_tm form" : "chains / plain",
                                       variant ? "the other form stays" : "one graph launch per step");
  }
}

// ---- the three ways vof_step runs a step (step_loop and step_n pick)
// 1. Inside a batch: as many of the `remaining` steps as the largest batch graph that fits holds, one graph launch.  An
// even number of steps leaves the F / twin pair and the host's view of it where they were.  Parity and orientation flip
// together from step to step, so two (parity, orientation) pairs are reachable; the batch graphs of both are captured the
// first time a steady-state step comes by, so that no later call pays for an instantiation in the middle of a run.
// *ran: the steps the launch ran, 0 if no batch fits (or batching is off): the step is then run on its own.
int run_step_batch(vof2d_ctx* h, int64_t remaining, int* ran) {
  *ran = 0;
  const int par = (int)(h->istep & 1);
  bool timed = false;
  int variant = batch_form(h, true, remaining, &timed);
  if (variant) fzmap_prepare(h);   // (in front of the captures too: a graph bakes in whether the handle has its zero maps)
  auto batch = [&](int form, int b) { return h->graphs.find(graph_key(h, gBatch, batch_variant(form, b, h->istep))); };
  if (h->batching && !batch(variant, 0)) {
    build_step_batches(h, variant);
    if (variant && h->tm_broken) {
      variant = 0; timed = false;
      if (h->batching && !batch(0, 0)) build_step_batches(h, 0);
    }
  }
  TuneState& t = h->tune;
  for (int b = timed ? vof2d_ctx::kTuneBatch : 0; b < vof2d_ctx::kStepBatches; ++b) {   // (while the forms are being timed: batches of the timed size)
    const int K = batch_steps(h, variant, b);
    hipGraphExec_t const exec = batch(variant, b);
    if (remaining < K || !exec) continue;
    const bool time_it = timed && b == vof2d_ctx::kTuneBatch && h->batching;
    if (time_it) {
      for (int k = 0; k < 2; ++k)
        if (!t.ev[2 * t.n + k] && hipEventCreate(&t.ev[2 * t.n + k]) != hipSuccess) return fail(h, VOF_EHIP, "hipEventCreate");
      if (hipEventRecord(t.ev[2 * t.n], h->stream) != hipSuccess) return fail(h, VOF_EHIP, "hipEventRecord");
    }
    if (variant) {
      // the k_tm batches chain: each ends with the next step's predictor in place (enqueue_steps_tm); only the first
      // after anything else needs its k_momentum launched in front
      if (h->state.ahead) h->tm_chained += 1;
      else DISPATCH_T(h, enqueue_tm_head<double>(h, par), enqueue_tm_head<float>(h, par));
      h->state.ahead = true;
    } else { h->state.ahead = false; step_wrote_F(h->state); }
    if (variant)
      if (const int rc = fzmap_clear_if_stale(h)) return rc;
    if (hipGraphLaunch(exec, h->stream) != hipSuccess) return fail(h, VOF_EHIP, "hipGraphLaunch of a step batch");
    if (time_it) {
      if (hipEventRecord(t.ev[2 * t.n + 1], h->stream) == hipSuccess) t.n += 1;
      else (void)hipGetLastError();   // (the batch ran: this timing is lost, the steps are not)
    }
    // (what jacobi_pair_ok looks at changes through vof_set_param only, which drops the graphs: it says what they were captured with)
    if (variant) { h->tm_steps += K; if (DISPATCH_B(h, L<double>::jacobi_pair_ok(h), L<float>::jacobi_pair_ok(h))) h->pair_launches += (int64_t)K * (h->d.jacobi_iters / 10); }
    else if (h->halves_captured[b]) h->halves_steps += K;
    *ran = K;
    return VOF_OK;
  }
  return VOF_OK;
}
// 2. From the step's own graph, captured on first use.  Graphs bake the field pointers in: one per (parity, field
// views: graph_key).  The two-kernel transport swaps the pair twice per step, the fused one once.
int run_step_graph(vof2d_ctx* h, bool virt) {
  h->state.ahead = false;   // (this step forms its own predictor, into the host's view of u*, v*, rhs)
  step_wrote_F(h->state);
  hipGraphExec_t& exec = h->graphs.slot(graph_key(h, gStep, (int)(h->istep & 1)));
  int rc;
  if (!exec && (rc = capture_or_fail(h, /*upload=*/true, &exec, "the step graph", [&] {
        DISPATCH_T(h, enqueue_step<double>(h, h->istep, true, virt), enqueue_step<float>(h, h->istep, true, virt));
      })))
    return rc;
  HIPCHK(h, hipGraphLaunch(exec, h->stream));
  if (h->g.wall_lo && h->g.wall_hi && h->fuse_transport) h->views.swap_F();     // keep the host's view in step with what the replayed kernels did
  return VOF_OK;
}
// 3. Eagerly, launch by launch: the first step after set_init_F / from_numpy / a single verb (lean = false: the schedule with
// the reference's intermediate set_BC calls), the one step after u / v were written without a set_BC (stored ghost cells
// must be read as they are, a captured step holds the kernels of the regular schedule), and every step of a handle
// created with VOF_FLAG_NO_GRAPH.  mg: the steps of vof_step_mg.
int run_step_eager(vof2d_ctx* h, bool lean, bool virt, const StepMg* mg) {
  h->state.ahead = false;   // (see run_step_graph)
  step_wrote_F(h->state);
  DISPATCH_T(h, enqueue_step<double>(h, h->istep, lean, virt, mg), enqueue_step<float>(h, h->istep, lean, virt, mg));
  return ensure_ok(h);
}

// nsteps steps of vof_step (mg == nullptr) or vof_step_mg: prologue and epilogue of a step from runtime/state.h.  A step that
// starts with consistent F ghosts runs the lean schedule (full domains: k_momentum, 2 x k_jacobi_tb, k_transport and no boundary
// launch -- virtual ghosts; strips: the two-kernel transport and one boundary launch at the end).  run_captured(plan, steps
// left, &ran) is how a step of the handle's regular schedule runs: inside a batch graph that runs *ran steps, or (*ran left
// 0) from the step's own graph.
template <typename RunCaptured>
int step_loop(vof2d_ctx* h, int64_t nsteps, bool use_graph, const StepMg* mg, RunCaptured&& run_captured) {
  for (int64_t s = 0; s < nsteps; ++s) {
    h->istep += 1;
    const StepPlan p = plan_step(h->state, step_caps(h, use_graph));
    if (!p.virt) settle_ghosts(h);
    int rc, ran = 0;
    if ((rc = p.captured ? run_captured(p, nsteps - s, &ran) : run_step_eager(h, p.lean, p.virt, mg))) return rc;
    if (ran) { h->istep += ran - 1; s += ran - 1; }
    finish_step(h->state, p);   // (behind a batch: nothing was dirty, the ghost cells are virtual)
  }
  return VOF_OK;
}
int step_n(vof2d_ctx* h, int64_t nsteps) {
  return step_loop(h, nsteps, !(h->d.flags & VOF_FLAG_NO_GRAPH), nullptr, [h](const StepPlan& p, int64_t remaining, int* ran) {
    if (p.virt) {   // steady state of a full domain
      if (const int rc = run_step_batch(h, remaining, ran)) { h->istep -= 1; return rc; }
      if (*ran) return (int)VOF_OK;
    }
    return run_step_graph(h, p.virt);
  });
}

// ---- vof_step_mg: the same three ways minus the batches, the step's sweeps replaced by `cycles` V-cycles (enqueue_step
// with a StepMg).  The step graphs bake in the cycle count and the criterion of the record beside the views: both are in
// the key (at most GraphStore::kCap of them stay), and the graphs go with every other when a knob changes (destroy_graphs).
int run_step_mg_graph(vof2d_ctx* h, bool virt, const StepMg& mg) {
  h->state.ahead = false;   // (see run_step_graph; settled in front of the loop: step_mg_n)
  step_wrote_F(h->state);
  hipGraphExec_t& exec = h->graphs.slot(graph_key(h, gStepMg, (mg.cycles * 2 + mg.criterion) * 2 + (int)(h->istep & 1)));
  int rc;
  if (!exec && (rc = capture_or_fail(h, /*upload=*/true, &exec, "the multigrid step graph", [&] {
        DISPATCH_T(h, enqueue_step<double>(h, h->istep, true, virt, &mg), enqueue_step<float>(h, h->istep, true, virt, &mg));
      })))
    return rc;
  HIPCHK(h, hipGraphLaunch(exec, h->stream));
  if (h->fuse_transport) h->views.swap_F();     // (a full domain: see run_step_graph)
  return VOF_OK;
}
// nsteps steps; the record of the call into whichever of the three pointers are given (one 32-byte read-back at the end;
// none, and no wait, if all are null).  The entry point has checked the arguments and that the handle is a full domain.
int step_mg_n(vof2d_ctx* h, int64_t nsteps, int cycles, int criterion, double* last_residual, double* worst_residual, int64_t* worst_step) {
  double rec[MGR_N] = {};
  const int64_t istep0 = h->istep;
  if (nsteps > 0) {
    int rc = cg_prepare(h);
    if (rc) return rc;
    if ((rc = mg_prepare(h))) return rc;
    if ((rc = h->buf.mg_rec.reserve(h, sizeof(rec), "vof_step_mg: no memory for the residual record"))) return rc;
    HIPCHK(h, hipMemsetAsync(h->buf.mg_rec.p, 0, sizeof(rec), h->stream));
    // A k_tm batch of vof_step may have left the next step's predictor formed ahead: it is formed again (k_momentum is the
    // first launch of every step here, and writes the same bits from the same u, v, F), so all that is to do is to hand
    // the handle back in the state every other entry point expects.
    (void)settle_ahead(h);
    const StepMg mg{cycles, criterion};
    if ((rc = step_loop(h, nsteps, !(h->d.flags & VOF_FLAG_NO_GRAPH) && h->mg_graph, &mg,
                        [h, &mg](const StepPlan& p, int64_t, int*) { return run_step_mg_graph(h, p.virt, mg); })))
      return rc;
    if ((last_residual || worst_residual || worst_step) && (rc = read_back(h, rec, h->buf.mg_rec.p, sizeof(rec)))) return rc;
  }
  if (last_residual) *last_residual = rec[MGR_LAST];
  if (worst_residual) *worst_residual = rec[MGR_WORST];
  if (worst_step) *worst_step = rec[MGR_COUNT] > 0.0 ? istep0 + (int64_t)rec[MGR_WORST_AT] : 0;
  return VOF_OK;
}

// The steps of every vof_step_<verb> (their loop: step_groups, runtime/groups.h): those of vof_step_mg with `cycles` V-cycles and no
// record read back where cycles > 0, else those of vof_step
int step_n_or_mg(vof2d_ctx* h, int64_t nsteps, int cycles, int criterion) {
  return cycles > 0 ? step_mg_n(h, nsteps, cycles, criterion, nullptr, nullptr, nullptr) : step_n(h, nsteps);
}
// ... nsteps of them in groups of `every` with after(r) behind group r, then the remainder: the loop of the six step_<verb>_n.
// Reserving buffers before anything is enqueued, the read-backs at the end and the counters are each verb's own; its entry point
// has checked the arguments, that the handle is a whole domain with what the verb works on and that no phased step is in progress.
template <class After>
int step_groups_n(vof2d_ctx* h, int64_t nsteps, int64_t every, int cycles, int criterion, After&& after) {
  return step_groups(nsteps, every, [&](int64_t n) { return step_n_or_mg(h, n, cycles, criterion); }, after);
}

// One phase of a step (vof_step_phase: the caller has checked the order of the phases)
int step_phase(vof2d_ctx* h, int phase) {
  if (phase != 0) step_wrote_F(h->state);
  if (h->d.flags & VOF_FLAG_NO_GRAPH) {
    DISPATCH_T(h, enqueue_phase<double>(h, phase, h->istep), enqueue_phase<float>(h, phase, h->istep));
    return ensure_ok(h);
  }
  hipGraphExec_t& exec = h->graphs.slot(graph_key(h, gPhase, phase == 0 ? 0 : 2 * phase - 1 + (int)(h->istep & 1)));
  int rc;
  if (!exec && (rc = capture_or_fail(h, /*upload=*/false, &exec, "a phase graph", [&] {
        DISPATCH_T(h, enqueue_phase<double>(h, phase, h->istep), enqueue_phase<float>(h, phase, h->istep));
      })))
    return rc;
  HIPCHK(h, hipGraphLaunch(exec, h->stream));
  if (phase == 1 || phase == 2) h->views.swap_F();   // keep the host's view of the F / twin buffers in step with what the replayed kernels did
  return VOF_OK;
}

// nsteps steps of the fused schedule launched eagerly with a start/stop event pair on every
// dispatch; durations accumulate per kernel (vof_get_profile).  Steps are enqueued in batches
// without host synchronisation in between (an idle GPU drops its clocks).
int profile_steps(vof2d_ctx* h, int64_t nsteps) {
  for (int k = 0; k < 2 * vof2d_ctx::kMaxTimed; ++k)
    if (!h->tev[k]) HIPCHK(h, hipEventCreate(&h->tev[k]));
  const int per_step = 16 + h->d.jacobi_iters;  // upper bound of launches in one step
  int64_t done = 0;
  while (done < nsteps) {
    h->timed = 0;
    int batch = 0;
    // A handle whose batch graphs run the k_tm form is profiled in that form: the same launch sequence, eagerly, every
    // launch between its own event pair (k_momentum, K x k_jacobi_pair / 2 K x k_jacobi_tb, K - 1 x k_tm, k_transport).
    const bool tm_form = batch_form(h, false) == 1 && plan_step(h->state, step_caps(h, false)).virt && nsteps - done >= 2;
    if (tm_form) {
      // (1 + K x (Jacobi launches + 1) launches, each with its own event pair out of the pool)
      const int per_tm_step = 1 + (DISPATCH_B(h, L<double>::jacobi_pair_ok(h), L<float>::jacobi_pair_ok(h)) ? h->d.jacobi_iters / 10 : h->d.jacobi_iters / 5);
      int K = 2;   // the handle's own batch sizes (an even number of steps each), as far as the event pool allows
      for (int b = vof2d_ctx::kStepBatches - 1; b >= 0; --b)
        if (nsteps - done >= batch_steps(h, 1, b) && 1 + batch_steps(h, 1, b) * per_tm_step <= vof2d_ctx::kMaxTimed && batch_steps(h, 1, b) > K) K = batch_steps(h, 1, b);
      if (1 + K * per_tm_step > vof2d_ctx::kMaxTimed) { h->timed = -1; return fail(h, VOF_ESTATE, "a k_tm batch of two steps has more launches than the profiling event pool"); }
      fzmap_prepare(h);
      if (const int rc = fzmap_clear_if_stale(h)) { h->timed = -1; return rc; }
      if (!h->state.ahead) DISPATCH_T(h, enqueue_tm_head<double>(h, (int)((h->istep + 1) & 1)), enqueue_tm_head<float>(h, (int)((h->istep + 1) & 1)));
      h->state.ahead = true;
      DISPATCH_T(h, enqueue_steps_tm<double>(h, h->istep + 1, K), enqueue_steps_tm<float>(h, h->istep + 1, K));
      h->istep += K;
      h->state.ghosts_virtual = true;
      batch = K;
    }
    while (!tm_form && done + batch < nsteps && h->timed + per_step <= vof2d_ctx::kMaxTimed) {
      h->istep += 1;
      h->state.ahead = false;   // (cleared in front of settle_ghosts, unlike step_loop: no copy of a predictor formed ahead, no ensure_ok per step)
      const StepPlan p = plan_step(h->state, step_caps(h, false));
      if (!p.virt) settle_ghosts(h);
      step_wrote_F(h->state);
      DISPATCH_T(h, enqueue_step<double>(h, h->istep, p.lean, p.virt), enqueue_step<float>(h, h->istep, p.lean, p.virt));
      finish_step(h->state, p);
      ++batch;
    }
    const int launches = h->timed;
    h->timed = -1;
    if (batch == 0) return fail(h, VOF_ESTATE, "a step has more launches than the profiling event pool");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // Dispatch start -> stop.  A dispatch's start stamp is taken when the command processor picks
    // the packet up, while the predecessor's last waves are still draining, so for kernels that
    // follow a long-tailed kernel the figure includes that overlap (the per-step sum can exceed the
    // wall time by ~5 %); it is a diagnostic breakdown, rocprofv3 gives exclusive times.
    for (int k = 0; k < launches; ++k) {
      float ms = 0.f;
      HIPCHK(h, hipEventElapsedTime(&ms, h->tev[2 * k], h->tev[2 * k + 1]));
      h->prof_sum_ms[h->tkid[k]] += ms;
      h->prof_cnt[h->tkid[k]] += 1;
    }
    done += batch;
  }
  return ensure_ok(h);
}

}  // namespace
