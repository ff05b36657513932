// runtime/regrid.h -- vof_regrid: the work buffer, the order on the two handles' streams, the launches of kernels/regrid.h, what
// the call does to dst's state, the summary
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
#pragma once
#include "regrid_check.h"
#include "scene.h"

namespace {

static_assert(RGS_RX == VOF_REGRID_SUM_RX && RGS_DIR == VOF_REGRID_SUM_DIR && RGS_PLIC_CELLS == VOF_REGRID_SUM_PLIC_CELLS && RGS_F_DST == VOF_REGRID_SUM_F_DST &&
              RGS_ISTEP == VOF_REGRID_SUM_ISTEP && RGS_N == VOF_REGRID_SUM_N && RGF_PLIC == VOF_REGRID_PLIC && kRegridMaxFactor == VOF_REGRID_MAX_FACTOR,
              "kernels/regrid.h and include/vof2d.h name the same things");

// rows of dst per wave chunk of the refining and coarsening kernels (refining, a chunk re-reads three rows of the source: the
// cells-per-wave rule of vof_interface); the sums of F take the chunks of vof_diagnostics on their own handle (diag_chunk), which
// fix their order
inline int regrid_chunk(const vof2d_ctx* h) { return chunk_rows(h, h->g.ntj, 4, 32); }

// dst's work buffer: the counts of k_regrid_refine, the partials of the two sums, the four doubles of k_regrid_finish
struct RegridCarve { unsigned nb, nb_src, nb_dst; size_t cnt, sum_src, sum_dst, out, total; };   // blocks; offsets in doubles; bytes
inline RegridCarve regrid_carve(const vof2d_ctx* dst, const vof2d_ctx* src) {
  RegridCarve c;
  c.nb = reported(dst).blocks(regrid_chunk(dst));
  c.nb_src = reported(src).blocks(diag_chunk(src));
  c.nb_dst = reported(dst).blocks(diag_chunk(dst));
  c.cnt = 0;
  c.sum_src = c.cnt + (size_t)c.nb * kRegridPart;
  c.sum_dst = c.sum_src + c.nb_src;
  c.out = c.sum_dst + c.nb_dst;
  c.total = (c.out + kRegridOut) * sizeof(double);
  return c;
}

// the pass over dst's interior, on dst's stream (every launch of the call goes through dst)
template <typename Ts, typename Td>
void regrid_launch(vof2d_ctx* dst, vof2d_ctx* src, const RegridFactors& f, bool plic, double eps, const RegridCarve& cv) {
  constexpr int V = VecWidth<Td>::V;
  const Reported rep = reported(dst);
  const int R = regrid_chunk(dst);
  double* const cnt = dst->buf.regrid.as<double>() + cv.cnt;
  const Ts* const Fs = F_<Ts>(src, fF); const Ts* const us = F_<Ts>(src, fU); const Ts* const vs = F_<Ts>(src, fV); const Ts* const ps = F_<Ts>(src, fP);
  Td* const Fd = F_<Td>(dst, fF); Td* const Fd2 = F_<Td>(dst, fF2); Td* const ud = F_<Td>(dst, fU); Td* const vd = F_<Td>(dst, fV); Td* const pd = F_<Td>(dst, fP);
  if (f.dir > 0) {
    const IfaceConsts c = {eps, 1.0 - eps, src->cd.nrm_x, src->cd.nrm_y, src->cd.dx, src->cd.dy};
    if (plic) launch(dst, kOther, k_regrid_refine<Ts, Td, V, true>, dim3(cv.nb), 0, rep.g, src->g, Fs, us, vs, ps, Fd, Fd2, ud, vd, pd, f.rx, f.ry, R, c, cnt);
    else launch(dst, kOther, k_regrid_refine<Ts, Td, V, false>, dim3(cv.nb), 0, rep.g, src->g, Fs, us, vs, ps, Fd, Fd2, ud, vd, pd, f.rx, f.ry, R, c, cnt);
  } else {
    launch(dst, kOther, k_regrid_coarsen<Ts, Td, V>, dim3(cv.nb), 0, rep.g, src->g, Fs, us, vs, ps, Fd, Fd2, ud, vd, pd, f.rx, f.ry, R);
  }
  const int n = dst->g.nx > dst->g.ny ? dst->g.nx + 2 : dst->g.ny + 2;
  launch(dst, kOther, k_regrid_ring<Td>, dim3((n + 255) / 256), 0, dst->g, ud, vd);
}
template <typename T>
void regrid_sum_launch(vof2d_ctx* dst, vof2d_ctx* of, unsigned nb, double* part) {
  if (nb) launch(dst, kOther, k_regrid_sum<T, VecWidth<T>::V>, dim3(nb), 0, reported(of).g, (const T*)F_<T>(of, fF), diag_chunk(of), part);
}

// vof_regrid behind its checks.  The fields of src as vof_get_field would return them (settle_ghosts), the kernels on dst's stream
// behind everything pending on src and in front of whatever src enqueues next (the event pair of vof_copy_rows); then dst is what
// vof_set_field of the four arrays, vof_set_BC and vof_set_istep would have left: the fields written from outside, the boundary
// launch of vof_set_BC, the batch form forgotten and the gas count posted again (scene_run), src's istep.  Waits only for a summary.
int regrid_run(vof2d_ctx* dst, vof2d_ctx* src, const RegridFactors& f, int flags, double eps, double* summary) {
  const RegridCarve cv = regrid_carve(dst, src);
  if (const int rc = dst->buf.regrid.reserve(dst, cv.total, "vof_regrid: no memory for the partials")) return rc;
  settle_ghosts(src);
  settle_ghosts(dst);
  HIPCHK(dst, hipEventRecord(src->ev1, src->stream));
  HIPCHK(dst, hipStreamWaitEvent(dst->stream, src->ev1, 0));
  const bool plic = (flags & RGF_PLIC) != 0;
  const bool s64 = src->d.dtype == VOF_F64, d64 = dst->d.dtype == VOF_F64;
  if (s64 && d64) regrid_launch<double, double>(dst, src, f, plic, eps, cv);
  else if (s64) regrid_launch<double, float>(dst, src, f, plic, eps, cv);
  else if (d64) regrid_launch<float, double>(dst, src, f, plic, eps, cv);
  else regrid_launch<float, float>(dst, src, f, plic, eps, cv);
  bool f_written = false;
  for (const int id : {(int)fF, (int)fU, (int)fV, (int)fP}) f_written = field_written(dst->state, id, true, false) || f_written;
  if (f_written) forget_batch_form(dst);
  DISPATCH_T(dst, (L<double>::set_bc<BC_ALL | BC_RHO>(dst)), (L<float>::set_bc<BC_ALL | BC_RHO>(dst)));
  bc_applied(dst->state);
  dst->istep = src->istep;
  double* const buf = dst->buf.regrid.as<double>();
  if (summary) {
    if (s64) regrid_sum_launch<double>(dst, src, cv.nb_src, buf + cv.sum_src); else regrid_sum_launch<float>(dst, src, cv.nb_src, buf + cv.sum_src);
    if (d64) regrid_sum_launch<double>(dst, dst, cv.nb_dst, buf + cv.sum_dst); else regrid_sum_launch<float>(dst, dst, cv.nb_dst, buf + cv.sum_dst);
    launch(dst, kOther, k_regrid_finish, dim3(1), 0, (const double*)(buf + cv.cnt), f.dir > 0 ? (int)cv.nb : 0, (const double*)(buf + cv.sum_src), (int)cv.nb_src,
           (const double*)(buf + cv.sum_dst), (int)cv.nb_dst, buf + cv.out);
  }
  if (src->stream != dst->stream) {
    HIPCHK(dst, hipEventRecord(dst->ev1, dst->stream));
    HIPCHK(dst, hipStreamWaitEvent(src->stream, dst->ev1, 0));
  }
  if (tm_by_rule(dst)) (void)post_gas_count(dst);   // (see vof_set_init_F)
  if (const int rc = ensure_ok(dst)) return rc;
  if (summary) {
    double out[kRegridOut];
    if (const int rc = read_back(dst, out, buf + cv.out, sizeof(out))) return rc;
    for (int k = 0; k < VOF_REGRID_SUM_N; ++k) summary[k] = 0.0;
    summary[VOF_REGRID_SUM_RX] = (double)f.rx;
    summary[VOF_REGRID_SUM_RY] = (double)f.ry;
    summary[VOF_REGRID_SUM_DIR] = (double)f.dir;
    summary[VOF_REGRID_SUM_PLIC_CELLS] = out[0];
    summary[VOF_REGRID_SUM_DEGENERATE] = out[1];
    summary[VOF_REGRID_SUM_F_SRC] = out[2];
    summary[VOF_REGRID_SUM_F_DST] = out[3];
    summary[VOF_REGRID_SUM_ISTEP] = (double)dst->istep;
  }
  return VOF_OK;
}

}  // namespace
