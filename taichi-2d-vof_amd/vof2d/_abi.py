"""ctypes prototypes of the C ABI declared in include/vof2d.h.

`bind(lib, prefix)` attaches argtypes/restype to every entry point of a loaded
shared library.  The product always binds ``libvof2d_hip.so`` with prefix
``vof_`` (see `_lib.py`); the parity tests additionally bind the CPU oracle,
which exports the same signatures with prefix ``ovof_``.
"""
import ctypes as C

VOF_ABI_VERSION = 2
VOF_F64, VOF_F32 = 0, 1
VOF_OK, VOF_EINVAL, VOF_EHIP, VOF_ENOMEM, VOF_ESTATE = 0, -1, -2, -3, -4
VOF_FLAG_NO_GRAPH = 1
VOF_COMM_ID_BYTES, VOF_COMM_LOOPBACK = 128, 1
VOF_XCHG_F, VOF_XCHG_U, VOF_XCHG_V, VOF_XCHG_P = 1, 2, 4, 8
VOF_XCHG_US, VOF_XCHG_VS, VOF_XCHG_RHS = 16, 32, 64
VOF_RESID_ABS, VOF_RESID_REL, VOF_RESID_TINY = 0, 1, 1e-300
VOF_DIAG_N = 16   # doubles in a row of vof_diagnostics (the slots: vof2d/diag.py)
# vof_interface: the slots of a segment row and of the summary (vof2d/interface.py)
VOF_IFACE_I, VOF_IFACE_J, VOF_IFACE_X0, VOF_IFACE_Y0, VOF_IFACE_X1, VOF_IFACE_Y1, VOF_IFACE_NX, VOF_IFACE_NY, VOF_IFACE_N = range(9)
VOF_IFACE_SUM_SEGMENTS, VOF_IFACE_SUM_DEGENERATE, VOF_IFACE_SUM_LENGTH, VOF_IFACE_SUM_ISTEP, VOF_IFACE_SUM_N = range(5)
# vof_curvature: the slots of a row and of the summary (vof2d/curvature.py)
VOF_CURV_I, VOF_CURV_J, VOF_CURV_KAPPA, VOF_CURV_VALID, VOF_CURV_AXIS, VOF_CURV_KAPPA_CSF, VOF_CURV_HP, VOF_CURV_F, VOF_CURV_N = range(9)
(VOF_CURV_SUM_ROWS, VOF_CURV_SUM_DEGENERATE, VOF_CURV_SUM_VALID, VOF_CURV_SUM_K, VOF_CURV_SUM_K2, VOF_CURV_SUM_MIN_K, VOF_CURV_SUM_MAX_K,
 VOF_CURV_SUM_CSF, VOF_CURV_SUM_CSF2, VOF_CURV_SUM_MIN_CSF, VOF_CURV_SUM_MAX_CSF, VOF_CURV_SUM_ISTEP) = range(12)
VOF_CURV_SUM_N = 16
# vof_energy: the slots of a row (vof2d/energy.py)
(VOF_ENERGY_ISTEP, VOF_ENERGY_CELLS, VOF_ENERGY_KE_U, VOF_ENERGY_KE_V, VOF_ENERGY_P_VISC, VOF_ENERGY_P_ADV, VOF_ENERGY_P_GRAV, VOF_ENERGY_P_SIGMA,
 VOF_ENERGY_P_PRES, VOF_ENERGY_SUM_RHO, VOF_ENERGY_SUM_RHO_I, VOF_ENERGY_SUM_RHO_J, VOF_ENERGY_SUM_GRADF, VOF_ENERGY_MAX_ACC_SIGMA) = range(14)
VOF_ENERGY_N = 16
# vof_blobs: the phases, the slots of a blob's row and of the summary (vof2d/blobs.py)
VOF_BLOB_LIQUID, VOF_BLOB_GAS = 0, 1
(VOF_BLOB_I0, VOF_BLOB_J0, VOF_BLOB_CELLS, VOF_BLOB_IMIN, VOF_BLOB_IMAX, VOF_BLOB_JMIN, VOF_BLOB_JMAX, VOF_BLOB_SUM_W, VOF_BLOB_SUM_WI,
 VOF_BLOB_SUM_WJ, VOF_BLOB_SUM_WU, VOF_BLOB_SUM_WV) = range(12)
VOF_BLOB_N = 16
VOF_BLOB_SUM_BLOBS, VOF_BLOB_SUM_MEMBER_CELLS, VOF_BLOB_SUM_MAX_CELLS, VOF_BLOB_SUM_ISTEP, VOF_BLOB_SUM_N = range(5)
# vof_tracers_*: the slots of a tracer's row and of the summary (vof2d/tracers.py)
VOF_TRACER_X, VOF_TRACER_Y, VOF_TRACER_U, VOF_TRACER_V, VOF_TRACER_F = range(5)
VOF_TRACER_N = 8
VOF_TRACER_SUM_COUNT, VOF_TRACER_SUM_LOST, VOF_TRACER_SUM_IN_LIQUID, VOF_TRACER_SUM_ISTEP, VOF_TRACER_SUM_TIME = range(5)
VOF_TRACER_SUM_N = 8
# vof_depths and vof_gauges_*: the slots of the summaries and of a gauge's row (vof2d/gauges.py)
VOF_DEPTH_SUM_ROWS, VOF_DEPTH_SUM_ISTEP, VOF_DEPTH_SUM_FRONT_LO, VOF_DEPTH_SUM_FRONT_HI, VOF_DEPTH_SUM_TOP_J, VOF_DEPTH_SUM_SUM = range(6)
VOF_DEPTH_SUM_N = 8
VOF_GAUGE_X, VOF_GAUGE_Y, VOF_GAUGE_U, VOF_GAUGE_V, VOF_GAUGE_F, VOF_GAUGE_P, VOF_GAUGE_DEPTH, VOF_GAUGE_TOP, VOF_GAUGE_N = range(9)
VOF_GAUGE_SUM_COUNT, VOF_GAUGE_SUM_ISTEP, VOF_GAUGE_SUM_RECORDS = range(3)
VOF_GAUGE_SUM_N = 8
# vof_dye_*: the slots of a row of vof_dye_stats (vof2d/dye.py)
(VOF_DYE_ISTEP, VOF_DYE_CELLS, VOF_DYE_SUM_C, VOF_DYE_SUM_CI, VOF_DYE_SUM_CJ, VOF_DYE_SUM_C2, VOF_DYE_SUM_CF, VOF_DYE_SUM_CU, VOF_DYE_SUM_CV,
 VOF_DYE_MIN_C, VOF_DYE_MAX_C, VOF_DYE_MAX_EXCESS) = range(12)
VOF_DYE_N = 16
# vof_frame, vof_step_frames: the quantities, the flags, the rows of the colour table and the slots of the summary (vof2d/frames.py)
VOF_FRAME_F, VOF_FRAME_U, VOF_FRAME_V, VOF_FRAME_SPEED, VOF_FRAME_P, VOF_FRAME_VORT, VOF_FRAME_DYE = range(7)
VOF_FRAME_CONTOUR, VOF_FRAME_SYMMETRIC = 1, 2
VOF_FRAME_LUT_ROWS = 258
(VOF_FRAME_SUM_PW, VOF_FRAME_SUM_PH, VOF_FRAME_SUM_ISTEP, VOF_FRAME_SUM_LO, VOF_FRAME_SUM_HI, VOF_FRAME_SUM_NAN_PIXELS,
 VOF_FRAME_SUM_CONTOUR_PIXELS) = range(7)
VOF_FRAME_SUM_N = 8
# vof_stats_*: the groups, the planes in slot order and the slots of the summary (vof2d/stats.py)
VOF_STATS_MOMENTS, VOF_STATS_ENVELOPE = 1, 2
(VOF_STATS_SUM_F, VOF_STATS_SUM_F2, VOF_STATS_SUM_U, VOF_STATS_SUM_V, VOF_STATS_SUM_UU, VOF_STATS_SUM_VV, VOF_STATS_SUM_UV, VOF_STATS_SUM_FU,
 VOF_STATS_SUM_FV, VOF_STATS_MAX_F, VOF_STATS_MAX_SPEED2, VOF_STATS_WET, VOF_STATS_ARRIVAL, VOF_STATS_PLANES) = range(14)
(VOF_STATS_SUM_SAMPLES, VOF_STATS_SUM_ISTEP_FIRST, VOF_STATS_SUM_ISTEP_LAST, VOF_STATS_SUM_MASK, VOF_STATS_SUM_LEVEL, VOF_STATS_SUM_CELLS,
 VOF_STATS_SUM_EVER_WET, VOF_STATS_SUM_MAX_SPEED2) = range(8)
VOF_STATS_SUM_N = 16
# vof_set_scene: the fields of a shape record, the kinds, the phases, the flag, the limit and the slots of the summary (vof2d/scene.py)
VOF_SHAPE_N, VOF_SHAPE_KIND, VOF_SHAPE_PHASE, VOF_SHAPE_A0 = 8, 0, 1, 2
VOF_SHAPE_BOX, VOF_SHAPE_ELLIPSE, VOF_SHAPE_HALFPLANE, VOF_SHAPE_TRIANGLE = range(4)
VOF_SCENE_GAS, VOF_SCENE_LIQUID = 0, 1
VOF_SCENE_CLEAR = 1
VOF_SCENE_MAX_SHAPES = 1024
VOF_SCENE_SUM_SHAPES, VOF_SCENE_SUM_SAMPLES, VOF_SCENE_SUM_PAINTED, VOF_SCENE_SUM_MIXED, VOF_SCENE_SUM_ISTEP = range(5)
VOF_SCENE_SUM_N = 8
# vof_regrid: the flag, the limit and the slots of the summary (vof2d/regrid.py)
VOF_REGRID_PLIC = 1
VOF_REGRID_MAX_FACTOR = 16
(VOF_REGRID_SUM_RX, VOF_REGRID_SUM_RY, VOF_REGRID_SUM_DIR, VOF_REGRID_SUM_PLIC_CELLS, VOF_REGRID_SUM_DEGENERATE, VOF_REGRID_SUM_F_SRC,
 VOF_REGRID_SUM_F_DST, VOF_REGRID_SUM_ISTEP, VOF_REGRID_SUM_N) = range(9)

ERRNAMES = {VOF_EINVAL: "VOF_EINVAL", VOF_EHIP: "VOF_EHIP", VOF_ENOMEM: "VOF_ENOMEM",
            VOF_ESTATE: "VOF_ESTATE"}


def halo_rows(jacobi_iters):
    """VOF_HALO_ROWS of include/vof2d.h."""
    return int(jacobi_iters) + 8


class Desc(C.Structure):
    """struct vof2d_desc"""
    _fields_ = [
        ("abi_version", C.c_int32),
        ("nx", C.c_int32), ("ny", C.c_int32),
        ("dtype", C.c_int32),
        ("coord_cast_f32", C.c_int32),
        ("row_lo", C.c_int32), ("row_hi", C.c_int32),
        ("own_lo", C.c_int32), ("own_hi", C.c_int32),
        ("jacobi_iters", C.c_int32),
        ("device", C.c_int32),
        ("flags", C.c_int32),
        ("Lx", C.c_double), ("Ly", C.c_double),
        ("rho_l", C.c_double), ("rho_g", C.c_double),
        ("nu_l", C.c_double), ("nu_g", C.c_double),
        ("sigma", C.c_double),
        ("gx", C.c_double), ("gy", C.c_double),
        ("dt", C.c_double),
    ]


class FrameSpec(C.Structure):
    """struct vof2d_frame_spec"""
    _fields_ = [
        ("quantity", C.c_int32),
        ("bx", C.c_int32), ("by", C.c_int32),
        ("flags", C.c_int32),
        ("lo", C.c_double), ("hi", C.c_double),
    ]


H = C.c_void_p
_i32, _i64, _dbl, _str = C.c_int32, C.c_int64, C.c_double, C.c_char_p
_u8p = C.POINTER(C.c_uint8)

# name -> (restype, argtypes); the complete symbol list of include/vof2d.h
SIGNATURES = {
    "desc_default": (C.c_int, [C.POINTER(Desc), _i32, _i32, _i32]),
    "create": (C.c_int, [C.POINTER(Desc), C.c_void_p, C.POINTER(H)]),
    "destroy": (C.c_int, [H]),
    "set_init_F": (C.c_int, [H, _i32]),
    "set_scene": (C.c_int, [H, C.POINTER(_dbl), _i64, _i32, _i32, C.POINTER(_dbl)]),
    "set_BC": (C.c_int, [H]),
    "cal_nu_rho": (C.c_int, [H]),
    "get_normal_young": (C.c_int, [H]),
    "advect_upwind": (C.c_int, [H]),
    "solve_p_jacobi": (C.c_int, [H, _i32]),
    "update_uv": (C.c_int, [H]),
    "fct_x_sweep": (C.c_int, [H]),
    "fct_y_sweep": (C.c_int, [H]),
    "solve_VOF_rudman": (C.c_int, [H, _i64]),
    "post_process_f": (C.c_int, [H]),
    "step": (C.c_int, [H, _i64]),
    "step_phase": (C.c_int, [H, _i32]),
    "get_istep": (C.c_int, [H, C.POINTER(_i64)]),
    "set_istep": (C.c_int, [H, _i64]),
    "solve_p_residual": (C.c_int, [H, _dbl, _i32, _i32, C.POINTER(_i32), C.POINTER(_dbl)]),
    "jacobi_sweeps_residual": (C.c_int, [H, _i32, _i32, C.POINTER(_dbl)]),
    "jacobi_sweeps_norms": (C.c_int, [H, _i32, _i32, C.POINTER(_dbl), C.POINTER(_dbl)]),
    "residual_value": (_dbl, [_dbl, _dbl, _i32]),
    "solve_p": (C.c_int, [H, _dbl, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_dbl)]),
    "solve_p_cg": (C.c_int, [H, _dbl, _i32, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_dbl), C.POINTER(_dbl)]),
    "solve_p_mg": (C.c_int, [H, _dbl, _i32, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_dbl), C.POINTER(_dbl)]),
    "step_mg": (C.c_int, [H, _i64, _i32, _i32, C.POINTER(_dbl), C.POINTER(_dbl), C.POINTER(_i64)]),
    "diagnostics": (C.c_int, [H, C.POINTER(_dbl)]),
    "step_diag": (C.c_int, [H, _i64, _i64, _i32, _i32, C.POINTER(_dbl), _i64, C.POINTER(_i64)]),
    "interface": (C.c_int, [H, _dbl, C.POINTER(_dbl), _i64, C.POINTER(_dbl)]),
    "curvature": (C.c_int, [H, _dbl, C.POINTER(_dbl), _i64, C.POINTER(_dbl)]),
    "energy": (C.c_int, [H, C.POINTER(_dbl)]),
    "step_energy": (C.c_int, [H, _i64, _i64, _i32, _i32, C.POINTER(_dbl), _i64, C.POINTER(_i64)]),
    "blobs": (C.c_int, [H, _i32, _dbl, C.POINTER(_dbl), _i64, C.POINTER(_i32), C.c_size_t, C.POINTER(_dbl)]),
    "tracers_set": (C.c_int, [H, C.POINTER(_dbl), _i64]),
    "tracers_advance": (C.c_int, [H, _dbl]),
    "tracers_get": (C.c_int, [H, C.POINTER(_dbl), _i64, C.POINTER(_dbl)]),
    "step_tracers": (C.c_int, [H, _i64, _i64, _i32, _i32, _i64, C.POINTER(_dbl), _i64, C.POINTER(_i64)]),
    "depths": (C.c_int, [H, C.POINTER(_dbl), _i64, C.POINTER(_dbl), _i64, C.POINTER(_i32), _i64, C.POINTER(_dbl)]),
    "gauges_set": (C.c_int, [H, C.POINTER(_dbl), _i64]),
    "gauges_get": (C.c_int, [H, C.POINTER(_dbl), _i64, C.POINTER(_dbl)]),
    "step_gauges": (C.c_int, [H, _i64, _i64, _i32, _i32, C.POINTER(_dbl), _i64, C.POINTER(_i64)]),
    "dye_set": (C.c_int, [H, C.c_void_p, C.c_size_t]),
    "dye_get": (C.c_int, [H, C.c_void_p, C.c_size_t]),
    "dye_advance": (C.c_int, [H]),
    "dye_stats": (C.c_int, [H, C.POINTER(_dbl)]),
    "step_dye": (C.c_int, [H, _i64, _i64, _i32, _i32, C.POINTER(_dbl), _i64, C.POINTER(_i64)]),
    "frame_set_lut": (C.c_int, [H, _u8p]),
    "frame": (C.c_int, [H, C.POINTER(FrameSpec), _u8p, _i64, C.POINTER(_dbl), _i64, C.POINTER(_dbl)]),
    "step_frames": (C.c_int, [H, _i64, _i64, _i32, _i32, C.POINTER(FrameSpec), _u8p, C.POINTER(_dbl), _i64, C.POINTER(_i64)]),
    "stats_begin": (C.c_int, [H, _i32, _dbl]),
    "stats_sample": (C.c_int, [H]),
    "stats_get": (C.c_int, [H, _i32, C.POINTER(_dbl), _i64]),
    "stats_summary": (C.c_int, [H, C.POINTER(_dbl)]),
    "step_stats": (C.c_int, [H, _i64, _i64, _i32, _i32, C.POINTER(_i64)]),
    "get_field": (C.c_int, [H, _str, C.c_void_p, C.c_size_t]),
    "set_field": (C.c_int, [H, _str, C.c_void_p, C.c_size_t]),
    "get_rows": (C.c_int, [H, _str, _i32, _i32, C.c_void_p, C.c_size_t]),
    "set_rows": (C.c_int, [H, _str, _i32, _i32, C.c_void_p, C.c_size_t]),
    "field_view": (C.c_int, [H, _str, C.POINTER(C.c_void_p), C.POINTER(_i64), C.POINTER(_i64),
                             C.POINTER(_i64)]),
    "copy_rows": (C.c_int, [H, H, _str, _i32, _i32]),
    "regrid": (C.c_int, [H, H, _i32, _dbl, C.POINTER(_dbl)]),
    "get_vis_field": (C.c_int, [H, _str, C.c_void_p, C.c_size_t]),
    "interp_velocity": (C.c_int, [H, C.c_void_p, C.c_size_t]),
    "set_param": (C.c_int, [H, _str, _dbl]),
    "get_param": (C.c_int, [H, _str, C.POINTER(_dbl)]),
    "get_counter": (C.c_int, [H, _str, C.POINTER(_i64)]),
    "sync": (C.c_int, [H]),
    "timer_start": (C.c_int, [H]),
    "timer_stop": (C.c_int, [H, C.POINTER(C.c_float)]),
    "time_jacobi": (C.c_int, [H, _i32, C.POINTER(C.c_float)]),
    "profile_steps": (C.c_int, [H, _i64]),
    "get_profile": (C.c_int, [H, _str, C.POINTER(_dbl), C.POINTER(_i64)]),
    "reset_profile": (C.c_int, [H]),
    "comm_get_unique_id": (C.c_int, [C.c_void_p]),
    "comm_init": (C.c_int, [H, C.c_void_p, _i32, _i32, _i32]),
    "comm_exchange": (C.c_int, [H, C.c_uint32]),
    "step_exchange": (C.c_int, [H, _i64, _i32]),
    "step_tm_piece": (C.c_int, [H, _i32]),
    "comm_allreduce_max": (C.c_int, [H, C.POINTER(_dbl)]),
    "comm_info": (C.c_int, [H, C.POINTER(_i32), C.POINTER(_i32)]),
    "comm_destroy": (C.c_int, [H]),
    "selftest_division": (C.c_int, [_i32, _i64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "last_error": (C.c_char_p, [H]),
    "backend": (C.c_char_p, []),
}


# entry points that only the GPU library implements (timing / profiling on a HIP stream)
GPU_ONLY = ("timer_start", "timer_stop", "time_jacobi", "profile_steps", "get_profile", "reset_profile",
            "selftest_division", "comm_get_unique_id", "comm_init", "comm_exchange", "step_exchange", "step_tm_piece", "comm_destroy",
            "comm_allreduce_max", "comm_info", "solve_p_cg", "solve_p_mg", "step_mg", "diagnostics", "step_diag", "interface", "curvature", "energy", "step_energy", "blobs",
            "tracers_set", "tracers_advance", "tracers_get", "step_tracers", "depths", "gauges_set", "gauges_get", "step_gauges",
            "dye_set", "dye_get", "dye_advance", "dye_stats", "step_dye", "frame_set_lut", "frame", "step_frames",
            "stats_begin", "stats_sample", "stats_get", "stats_summary", "step_stats", "set_scene", "regrid")


class Api:
    """Bound entry points of one library: api.step(h, n) -> int."""

    def __init__(self, lib, prefix, optional=()):
        self.lib, self.prefix = lib, prefix
        missing = []
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, prefix + name)
            except AttributeError:
                if name not in optional:
                    missing.append(prefix + name)
                continue
            fn.restype, fn.argtypes = res, args
            setattr(self, name, fn)
        if missing:
            raise ImportError("library %r lacks symbols: %s" % (getattr(lib, "_name", lib), ", ".join(missing)))


def bind(lib, prefix="vof_", optional=()):
    return Api(lib, prefix, optional)
