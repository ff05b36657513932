// runtime/graphs.h -- the keys of the handle's graph store (GraphStore, views.h) and the one way a graph is captured
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
#pragma once
#include "launches.h"

namespace {

// Graphs bake the field pointers in: every key carries the handle's current views (runtime/views.h).  variant is what the
// kind bakes in besides them, and nothing else:
//   gStep    parity of the step                gPhase   0 for phase 0, else 2 * phase - 1 + parity
//   gBatch   batch_variant (below)             gMg      0
//   gStepMg  (cycles * 2 + criterion) * 2 + parity
//   gXchg    overlap mode * 2 + parity         gXchg2, gXchg5   parity of the first step
inline GraphKey graph_key(const vof2d_ctx* h, int kind, int variant = 0) { return {kind, h->views.bits(), variant}; }
// form: 0 chains or the plain sequence, 1 k_tm; b: the batch size step_batch[b]; first: the batch's first step
inline int batch_variant(int form, int b, int64_t first) { return (form * vof2d_ctx::kStepBatches + b) * 2 + (int)(first & 1); }
inline int batch_form_of(const GraphKey& k) { return k.variant / (2 * vof2d_ctx::kStepBatches); }

// Captures what `enqueue` launches on h->stream (it returns false if something could not be enqueued) and instantiates
// it into *exec.  A capture enqueues nothing, but enqueueing runs the host-side swaps of the field views and may move
// istep: both are put back, so the caller redoes them after a LAUNCH, as it does after every replay.  The stream always
// leaves capture mode.  On failure *exec is null and the sticky error is the caller's to clear: what a failed capture means
// (an error, or a form switched off) is the caller's policy.
// mode: ThreadLocal for graphs of the handle's own stream; Relaxed for the exchange graphs (RCCL's calls inside).
// upload: pay for the upload now, not in the first replay -- possibly inside a timed region.
template <typename Enqueue>
hipError_t capture_graph(vof2d_ctx* h, hipStreamCaptureMode mode, bool upload, hipGraphExec_t* exec, Enqueue&& enqueue) {
  *exec = nullptr;
  const FieldViews views = h->views;
  const int64_t istep = h->istep;
  hipStream_t const stream = h->stream;
  hipError_t e = hipStreamBeginCapture(stream, mode);
  if (e != hipSuccess) return e;
  const bool enqueued = enqueue();
  hipGraph_t graph = nullptr;
  e = hipStreamEndCapture(stream, &graph);
  h->views = views;
  h->istep = istep;
  if (e == hipSuccess && !(enqueued && graph)) e = hipErrorUnknown;
  if (e == hipSuccess) e = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
  if (graph) (void)hipGraphDestroy(graph);
  if (e != hipSuccess) *exec = nullptr;
  else if (upload) (void)hipGraphUpload(*exec, stream);
  return e;
}
// ... for the graphs of the handle's own stream, whose failed capture is an error of the call (the exchange graphs fall
// back instead: capture_exchange_or_switch_off, comm.h)
template <typename Enqueue>
int capture_or_fail(vof2d_ctx* h, bool upload, hipGraphExec_t* exec, const char* what, Enqueue&& enqueue) {
  const hipError_t e = capture_graph(h, hipStreamCaptureModeThreadLocal, upload, exec, [&] { enqueue(); return true; });
  if (e != hipSuccess) snprintf(h->err, sizeof(h->err), "capture of %s: %s", what, hipGetErrorString(e));
  return e == hipSuccess ? VOF_OK : VOF_EHIP;
}

}  // namespace
