// runtime/graphs.h -- the keys of the graph cache (GraphCache, context.h) and the one way a graph is captured
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
#pragma once
#include "launches.h"

namespace {

// Graphs bake the field pointers in, so they are keyed by which buffer of a pair the host's view calls the first:
// 0 where F is in the buffer it had at creation, 1 where it is in its twin
inline int ori_F(const vof2d_ctx* h) { return h->fld[fF] == h->f_home ? 0 : 1; }
// the middle steps of mode 5 move all three pairs: parity of the first step | F / twin << 1 | (u*, v*) / (mx, my) << 2 | p / pt << 3
inline int xchg5_key(const vof2d_ctx* h) {
  return (int)((h->istep + 1) & 1) | (ori_F(h) << 1) | ((h->fld[fUS] == h->us_home ? 0 : 1) << 2) | ((h->fld[fP] == h->p_home ? 0 : 1) << 3);
}

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
  void* keep[NFIELDS];
  memcpy(keep, h->fld, sizeof(keep));
  const int64_t istep = h->istep;
  hipStream_t const stream = h->stream;
  hipError_t e = hipStreamBeginCapture(stream, mode);
  if (e != hipSuccess) return e;
  const bool enqueued = enqueue();
  hipGraph_t graph = nullptr;
  e = hipStreamEndCapture(stream, &graph);
  memcpy(h->fld, keep, sizeof(keep));
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
