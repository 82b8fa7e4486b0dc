"""MI355X-native MPF hot path: Python host mirror of the C ABI in include/mpf_c.h.

The product is lib/libmpf_amd.so (hand-written HIP kernels for gfx950 + C++ host driver); this
module only binds it with ctypes and uses torch for device memory and streams.  There is no CPU
fallback: importing works anywhere (so the build can be checked without a GPU), but every compute
entry point raises if the library is missing or no GPU is present.

The directory name contains '-', so import it with
    importlib.import_module("mixed-precision_lu_factorization_amd")
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPF_LIB") or os.path.join(_HERE, "lib", "libmpf_amd.so")   # (MPF_LIB: another build of the product library, for A/B runs of tools/)
# the same sources built with -DMPF_PROBE: + microbenchmarks and measured-slower kernel variants; tools/ and bench.py's
# on-box peak measurements load it, a product run never does (include/mpf_probe.h)
PROBE_LIB_PATH = os.environ.get("MPF_PROBE_LIB") or os.path.join(_HERE, "lib", "libmpf_probe.so")   # (tools: another build of the probe library for A/B runs)

TRAIL_FP64 = 0
TRAIL_FP16 = 1
TRAIL_FP16X3 = 2

# every symbol include/mpf_c.h declares (tests check the library exports all of them)
C_ABI_SYMBOLS = [
    "mpf_create", "mpf_destroy", "mpf_set_stream", "mpf_synchronize", "mpf_last_error", "mpf_get_stats",
    "mpf_device_report", "mpf_factor_host", "mpf_factor_dev", "mpf_double_to_fp16", "mpf_hdiv",
    "mpf_hgetf2_pivots", "mpf_hgetf2", "mpf_laswp", "mpf_dgetf2_npv", "mpf_dtrsm_llnu", "mpf_dgemm_minus",
    "mpf_solve_ir", "mpf_hgetf2_capacity_rows", "mpf_set_option", "mpf_get_option", "mpf_option_name", "mpf_hgemm_minus", "mpf_hgemm_minus_f32", "mpf_w32_from_f64", "mpf_w32_to_f64", "mpf_w32_laswp", "mpf_gesv", "mpf_matgen_dev", "mpf_matgen_cols_dev",
    "mpf_matgen_state", "mpf_rccl_unique_id", "mpf_rccl_init", "mpf_rccl_destroy", "mpf_rccl_version", "mpf_rccl_info", "mpf_rccl_bcast_probe", "mpf_factor_dist",
    "mpf_solve_ir_dist", "mpf_rccl_selftest", "mpf_check_plu_dev", "mpf_check_plu_host", "mpf_solve_ir_nrhs",
    "mpf_solve_gmres_ir", "mpf_trim", "mpf_dist_set_p2p",
    "mpf_solve_ir_trans", "mpf_lange", "mpf_geequ", "mpf_gecon", "mpf_gesvx",
    "mpf_getrs", "mpf_solve_ir_block", "mpf_gerfs", "mpf_gesvx_block",
    "mpf_dgetf2_piv", "mpf_solve_gmres_ir_block", "mpf_dgetf2_tp",
    "mpf_residual_x", "mpf_gerfsx",
    "mpf_gerpvgrw", "mpf_gerfsx_scaled", "mpf_gesvxx_block",
    "mpf_getri", "mpf_getdet",
    "mpf_getrf_batched", "mpf_getrs_batched",
    "mpf_getri_batched", "mpf_getdet_batched",
    "mpf_lange_batched", "mpf_gecon_batched", "mpf_residual_batched", "mpf_gerfs_batched",
    "mpf_getrf_batched_blocked", "mpf_getrs_batched_blocked",
    "mpf_getri_batched_blocked", "mpf_getdet_batched_blocked",
    "mpf_lange_batched_blocked", "mpf_gecon_batched_blocked", "mpf_residual_batched_blocked", "mpf_gerfs_batched_blocked",
    "mpf_vbatch_create", "mpf_vbatch_create_blocked", "mpf_vbatch_destroy", "mpf_vbatch_info", "mpf_vbatch_offsets",
    "mpf_getrf_vbatched", "mpf_getrs_vbatched", "mpf_getri_vbatched", "mpf_getdet_vbatched",
    "mpf_lange_vbatched", "mpf_gecon_vbatched", "mpf_residual_vbatched", "mpf_gerfs_vbatched",
    "mpf_geequ_batched", "mpf_laqge_batched", "mpf_lascl2_batched",
    "mpf_geequ_batched_blocked", "mpf_laqge_batched_blocked", "mpf_lascl2_batched_blocked",
    "mpf_geequ_vbatched", "mpf_laqge_vbatched", "mpf_lascl2_vbatched",
]
PROBE_ONLY_SYMBOLS = ["mpf_microbench", "mpf_debug_mfma4", "mpf_debug_gate", "mpf_debug_hgemm_again"]   # include/mpf_probe.h
CXX_SYMBOL_MPF = "_Z3MPFPdiiPi"  # void MPF(double*, int, int, int*)  (reference MPF.h:3)


class MpfOpts(C.Structure):
    _fields_ = [("trailing", C.c_int32), ("verbose", C.c_int32), ("fused_panel", C.c_int32),
                ("sync_timing", C.c_int32), ("no_lookahead", C.c_int32), ("superpanel", C.c_int32), ("pivot_path", C.c_int32), ("pivot_search", C.c_int32)]


class MpfStats(C.Structure):
    _fields_ = [("ms_total", C.c_double), ("ms_h2d", C.c_double), ("ms_d2h", C.c_double),
                ("ms_hpanel", C.c_double), ("ms_laswp", C.c_double), ("ms_dpanel", C.c_double),
                ("ms_trsm", C.c_double), ("ms_gemm", C.c_double), ("n", C.c_int64), ("nb", C.c_int32),
                ("panels", C.c_int32), ("hpanel_timeouts", C.c_int32), ("info", C.c_int32),
                ("gemm_launches", C.c_int32), ("lookahead", C.c_int32), ("superpanel", C.c_int32),
                ("pivot_path", C.c_int32), ("gemm_flops", C.c_double), ("gemm_bytes", C.c_double),
                ("ms_gemm_big", C.c_double), ("gemm_big_flops", C.c_double), ("gemm_big_bytes", C.c_double),
                ("ms_cvt", C.c_double), ("ms_blockrow", C.c_double), ("gemm_big_launches", C.c_int32), ("host_rows_streamed", C.c_int32),
                ("host_late_segments", C.c_int32), ("pivot_search", C.c_int32), ("fp16_fused", C.c_int32),
                ("lazy_onepass_blocks", C.c_int32)]


class MpfIrStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("rel_residual", C.c_double),
                ("history", C.c_double * 32), ("ms_total", C.c_double), ("stalled", C.c_int32), ("reserved", C.c_int32)]


class MpfGmresStats(C.Structure):
    _fields_ = [("outer_iterations", C.c_int32), ("inner_iterations", C.c_int32), ("converged", C.c_int32), ("budget_expired", C.c_int32),
                ("rel_residual", C.c_double), ("history", C.c_double * 32), ("ms_total", C.c_double)]


class MpfRcclInfo(C.Structure):
    _fields_ = [("version", C.c_int32), ("has_comm", C.c_int32), ("comm_count", C.c_int32), ("comm_rank", C.c_int32), ("has_p2p", C.c_int32),
                ("device", C.c_int32), ("visible_devices", C.c_int32), ("reserved", C.c_int32),
                ("bcast_calls", C.c_int64), ("bcast_bytes", C.c_int64), ("allreduce_calls", C.c_int64), ("p2p_calls", C.c_int64), ("p2p_bytes", C.c_int64),
                ("link_type", C.c_int32 * 16), ("link_hops", C.c_int32 * 16), ("peer_access", C.c_int32 * 16)]


class MpfGesvStats(C.Structure):
    _fields_ = [("path", C.c_int32), ("info", C.c_int32), ("ms_factor_fp16", C.c_double), ("ms_ir_fp16", C.c_double),
                ("ms_factor_fp64", C.c_double), ("ms_ir_fp64", C.c_double), ("ms_total", C.c_double),
                ("ir_fp16", MpfIrStats), ("ir_final", MpfIrStats), ("gmres_budget_ms", C.c_double), ("gmres_budget_expired", C.c_int32),
                ("reserved", C.c_int32)]


class MpfGeconStats(C.Structure):
    _fields_ = [("solves", C.c_int32), ("solves_t", C.c_int32), ("iterations", C.c_int32), ("reserved", C.c_int32),
                ("ainvnm", C.c_double), ("ms_total", C.c_double)]


class MpfGesvxStats(C.Structure):
    _fields_ = [("path", C.c_int32), ("info", C.c_int32), ("equed", C.c_int32), ("skipped_by_rcond", C.c_int32),
                ("rowcnd", C.c_double), ("colcnd", C.c_double), ("amax", C.c_double), ("anorm", C.c_double), ("kappa_max", C.c_double),
                ("rcond_lowp", C.c_double), ("rcond", C.c_double), ("ms_equilibrate", C.c_double), ("ms_factor", C.c_double),
                ("ms_gecon", C.c_double), ("ms_ir", C.c_double), ("ms_total", C.c_double), ("ir_lowp", MpfIrStats), ("ir_final", MpfIrStats)]


class MpfGerfsStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("lacn2_iterations", C.c_int32), ("solves", C.c_int32), ("reserved", C.c_int32),
                ("ms_total", C.c_double)]


class MpfGerfsxStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("x_state", C.c_int32), ("z_state", C.c_int32), ("solves", C.c_int32),
                ("final_dx_x", C.c_double), ("final_dz_z", C.c_double), ("dxratmax", C.c_double), ("dzratmax", C.c_double),
                ("ms_total", C.c_double)]


BCAST_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
P2P_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p)


class MpfDist(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("bcast", BCAST_FN), ("allreduce", ALLREDUCE_FN), ("user", C.c_void_p)]


class MPFError(RuntimeError):
    pass


def build(force=False):
    """Compile lib/libmpf_amd.so (product) and lib/libmpf_probe.so (tools) for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))]
    srcs += [os.path.join(_HERE, "..", "include", h) for h in ("mpf_c.h", "MPF.h", "mpf_probe.h")] + [os.path.join(_HERE, "Makefile")]
    stale = force or any(not os.path.exists(lp) or any(os.path.getmtime(s) > os.path.getmtime(lp) for s in srcs)
                         for lp in (LIB_PATH, PROBE_LIB_PATH))
    if stale:
        subprocess.run(["make", "-C", _HERE, "-s", "-j8", "all", "probe"], check=True)
    return LIB_PATH


_libs = {}


def load_library(probe=False):
    """dlopen the product library (probe=True: the probe build, tools only); raises MPFError (never falls back) when absent."""
    if probe in _libs:
        return _libs[probe]
    # torch first: libmpf_amd.so must bind to the HIP runtime torch already loaded (one runtime per process;
    # loading the system libamdhip64 before torch's bundled one leaves the process without devices)
    import torch  # noqa: F401
    path = PROBE_LIB_PATH if probe else LIB_PATH
    if not os.path.exists(path):
        raise MPFError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback)")
    L = C.CDLL(path)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    L.mpf_create.argtypes = [C.POINTER(vp), C.c_int]
    L.mpf_destroy.argtypes = [vp]
    L.mpf_set_stream.argtypes = [vp, vp]
    L.mpf_synchronize.argtypes = [vp]
    L.mpf_last_error.argtypes = [vp]
    L.mpf_last_error.restype = C.c_char_p
    L.mpf_get_stats.argtypes = [vp, C.POINTER(MpfStats)]
    L.mpf_set_option.argtypes = [vp, C.c_char_p, i64]
    L.mpf_get_option.argtypes = [vp, C.c_char_p, C.POINTER(i64)]
    L.mpf_option_name.argtypes = [i32, C.c_char_p, i64]
    L.mpf_device_report.argtypes = [C.c_char_p, i64]
    L.mpf_factor_host.argtypes = [vp, vp, i64, i32, vp, C.POINTER(MpfOpts)]
    L.mpf_trim.argtypes = [vp]
    L.mpf_dist_set_p2p.argtypes = [vp, P2P_FN, vp]
    L.mpf_factor_dev.argtypes = [vp, vp, i64, i64, i32, vp, C.POINTER(MpfOpts)]
    L.mpf_double_to_fp16.argtypes = [vp, vp, vp, i64]
    L.mpf_hdiv.argtypes = [vp, vp, vp, vp, i64]
    L.mpf_hgetf2_pivots.argtypes = [vp, vp, i64, i32, i32, i32, vp, vp]
    L.mpf_hgetf2.argtypes = [vp, vp, i64, i32, i32, vp]
    L.mpf_laswp.argtypes = [vp, vp, i64, i64, i32, i32, vp]
    L.mpf_dgetf2_npv.argtypes = [vp, vp, i64, i32, i32, i32]
    L.mpf_dgetf2_piv.argtypes = [vp, vp, i64, i32, i32, i32, i32, vp, C.POINTER(i32)]
    L.mpf_dgetf2_tp.argtypes = [vp, vp, i64, i32, i32, i32, i32, vp, C.POINTER(i32)]
    L.mpf_dtrsm_llnu.argtypes = [vp, i32, i64, vp, i64, vp, i64]
    L.mpf_dgemm_minus.argtypes = [vp, i64, i64, i32, vp, i64, vp, i64, vp, i64]
    L.mpf_hgemm_minus.argtypes = [vp, i64, i64, i32, vp, i64, vp, i64, vp, i64, i32]
    L.mpf_hgemm_minus_f32.argtypes = [vp, i64, i64, i32, vp, i64, vp, i64, vp, i64, i32]
    L.mpf_w32_from_f64.argtypes = [vp, vp, i64, vp, i64, i64, i64]
    L.mpf_w32_to_f64.argtypes = [vp, vp, i64, vp, i64, i64, i64]
    L.mpf_w32_laswp.argtypes = [vp, vp, i64, i64, i32, i32, vp]
    L.mpf_solve_ir.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, vp, i32, dbl, C.POINTER(MpfIrStats)]
    L.mpf_solve_ir_nrhs.argtypes = [vp, vp, i64, vp, i64, vp, i64, i32, vp, i64, vp, i64, i32, dbl, C.POINTER(MpfIrStats)]
    L.mpf_solve_gmres_ir.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, vp, i32, i32, dbl, C.POINTER(MpfGmresStats)]
    L.mpf_gesv.argtypes = [vp, vp, i64, i64, i32, vp, vp, vp, vp, i32, dbl, i32, C.POINTER(MpfGesvStats)]
    L.mpf_solve_ir_trans.argtypes = [vp, vp, i64, vp, i64, vp, i64, i32, vp, i64, vp, i64, i32, dbl, C.POINTER(MpfIrStats)]
    L.mpf_lange.argtypes = [vp, vp, i64, i64, i64, C.c_char, C.POINTER(dbl)]
    L.mpf_geequ.argtypes = [vp, vp, i64, i64, vp, vp, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl)]
    L.mpf_gecon.argtypes = [vp, vp, i64, i64, C.c_char, dbl, C.POINTER(dbl), C.POINTER(MpfGeconStats)]
    L.mpf_gesvx.argtypes = [vp, vp, i64, i64, i32, vp, vp, vp, vp, i32, i32, i32, dbl, i32, dbl, vp, vp, C.POINTER(MpfGesvxStats)]
    L.mpf_getrs.argtypes = [vp, i32, vp, i64, vp, i64, i32, vp, i64]
    L.mpf_solve_ir_block.argtypes = [vp, i32, vp, i64, vp, i64, vp, i64, i32, vp, i64, vp, i64, i32, dbl, C.POINTER(MpfIrStats)]
    L.mpf_solve_gmres_ir_block.argtypes = [vp, i32, vp, i64, vp, i64, vp, i64, i32, vp, i64, vp, i64, i32, i32, dbl, C.POINTER(MpfGmresStats)]
    L.mpf_gerfs.argtypes = [vp, i32, vp, i64, vp, i64, vp, i64, i32, vp, i64, vp, i64, i32, C.POINTER(dbl), C.POINTER(dbl),
                            C.POINTER(MpfGerfsStats)]
    L.mpf_residual_x.argtypes = [vp, i32, vp, i64, i64, i32, vp, i64, vp, i64, vp, i64]
    L.mpf_gerfsx.argtypes = [vp, i32, vp, i64, vp, i64, vp, i64, i32, vp, i64, vp, i64, i32, C.POINTER(dbl), C.POINTER(dbl),
                             C.POINTER(MpfGerfsxStats)]
    L.mpf_gesvx_block.argtypes = [vp, vp, i64, i64, i32, vp, vp, i32, vp, i64, vp, i64, i32, i32, i32, dbl, i32, dbl, i32, vp, vp,
                                  C.POINTER(dbl), C.POINTER(dbl), C.POINTER(MpfGesvxStats), C.POINTER(MpfIrStats), C.POINTER(MpfGerfsStats)]
    L.mpf_gerpvgrw.argtypes = [vp, vp, i64, vp, i64, i64, vp, vp, C.POINTER(dbl)]
    L.mpf_gerfsx_scaled.argtypes = [vp, i32, vp, i64, vp, i64, vp, i64, i32, vp, i64, vp, i64, i32, vp, vp, C.POINTER(dbl), C.POINTER(dbl),
                                    C.POINTER(dbl), C.POINTER(MpfGerfsxStats)]
    L.mpf_gesvxx_block.argtypes = [vp, vp, i64, i64, i32, vp, vp, i32, vp, i64, vp, i64, i32, i32, i32, dbl, i32, dbl, i32, vp, vp,
                                   C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl), C.POINTER(MpfGesvxStats),
                                   C.POINTER(MpfIrStats), C.POINTER(MpfGerfsxStats)]
    L.mpf_getri.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, i64]
    L.mpf_getdet.argtypes = [vp, vp, i64, vp, i64, vp, vp, C.POINTER(dbl), C.POINTER(i64)]
    L.mpf_getrf_batched.argtypes = [vp, vp, i64, i64, i32, i64, vp, i64, vp, i32]
    L.mpf_getrs_batched.argtypes = [vp, i32, vp, i64, i64, i32, i64, vp, i64, i32, vp, i64, i64]
    L.mpf_getri_batched.argtypes = [vp, vp, i64, i64, i32, i64, vp, i64, vp, i64, i64, vp]
    L.mpf_getrf_batched_blocked.argtypes = L.mpf_getrf_batched.argtypes
    L.mpf_getrs_batched_blocked.argtypes = L.mpf_getrs_batched.argtypes
    L.mpf_getdet_batched.argtypes = [vp, vp, i64, i64, i32, i64, vp, i64, vp, vp]
    L.mpf_getri_batched_blocked.argtypes = L.mpf_getri_batched.argtypes
    L.mpf_lange_batched.argtypes = [vp, C.c_char, vp, i64, i64, i32, i64, vp]
    L.mpf_gecon_batched.argtypes = [vp, C.c_char, vp, i64, i64, i32, i64, vp, vp, vp]
    L.mpf_residual_batched.argtypes = [vp, i32, vp, i64, i64, i32, i64, i32, vp, i64, i64, vp, i64, i64, vp, i64, i64, vp]
    L.mpf_gerfs_batched.argtypes = [vp, i32, vp, i64, i64, vp, i64, i64, i32, i64, vp, i64, i32, vp, i64, i64, vp, i64, i64, i32, vp, vp, vp]
    L.mpf_getdet_batched_blocked.argtypes = L.mpf_getdet_batched.argtypes
    L.mpf_lange_batched_blocked.argtypes = L.mpf_lange_batched.argtypes
    L.mpf_gecon_batched_blocked.argtypes = L.mpf_gecon_batched.argtypes
    L.mpf_residual_batched_blocked.argtypes = L.mpf_residual_batched.argtypes
    L.mpf_gerfs_batched_blocked.argtypes = L.mpf_gerfs_batched.argtypes
    L.mpf_vbatch_create.argtypes = [vp, i64, vp, vp, vp, C.POINTER(vp)]
    L.mpf_vbatch_create_blocked.argtypes = L.mpf_vbatch_create.argtypes
    L.mpf_vbatch_destroy.argtypes = [vp]
    L.mpf_vbatch_destroy.restype = None
    L.mpf_vbatch_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.mpf_vbatch_offsets.argtypes = [vp, vp, vp]
    L.mpf_getrf_vbatched.argtypes = [vp, vp, vp, vp, vp, i32]
    L.mpf_getrs_vbatched.argtypes = [vp, vp, i32, vp, vp, i32, vp, i64]
    L.mpf_getri_vbatched.argtypes = [vp, vp, vp, vp, vp, vp]
    L.mpf_getdet_vbatched.argtypes = [vp, vp, vp, vp, vp, vp]
    L.mpf_lange_vbatched.argtypes = [vp, vp, C.c_char, vp, vp]
    L.mpf_gecon_vbatched.argtypes = [vp, vp, C.c_char, vp, vp, vp, vp]
    L.mpf_residual_vbatched.argtypes = [vp, vp, i32, vp, i32, vp, i64, vp, i64, vp, i64, vp]
    L.mpf_gerfs_vbatched.argtypes = [vp, vp, i32, vp, vp, vp, i32, vp, i64, vp, i64, i32, vp, vp, vp]
    L.mpf_geequ_batched.argtypes = [vp, vp, i64, i64, i32, i64, vp, vp, vp, vp, vp, vp]
    L.mpf_laqge_batched.argtypes = [vp, i32, vp, i64, i64, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mpf_lascl2_batched.argtypes = [vp, vp, i32, i64, i32, vp, i64, i64, vp, i32]
    L.mpf_geequ_batched_blocked.argtypes = L.mpf_geequ_batched.argtypes
    L.mpf_laqge_batched_blocked.argtypes = L.mpf_laqge_batched.argtypes
    L.mpf_lascl2_batched_blocked.argtypes = L.mpf_lascl2_batched.argtypes
    L.mpf_geequ_vbatched.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mpf_laqge_vbatched.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mpf_lascl2_vbatched.argtypes = [vp, vp, vp, i32, vp, i64, vp, i32]
    L.mpf_matgen_dev.argtypes = [vp, vp, i64, i64, i64]
    L.mpf_matgen_cols_dev.argtypes = [vp, vp, i64, i64, i64, i64, i64]
    L.mpf_matgen_state.argtypes = [i64, C.POINTER(C.c_uint32)]
    L.mpf_rccl_unique_id.argtypes = [vp]
    L.mpf_rccl_init.argtypes = [vp, vp, i32, i32]
    L.mpf_rccl_destroy.argtypes = [vp]
    L.mpf_rccl_version.argtypes = []
    L.mpf_rccl_selftest.argtypes = [vp]
    L.mpf_check_plu_dev.argtypes = [vp, vp, i64, vp, i64, vp, i64, C.POINTER(dbl), C.POINTER(dbl)]
    L.mpf_check_plu_host.argtypes = [vp, vp, vp, i64, C.POINTER(dbl), C.POINTER(dbl)]
    L.mpf_factor_dist.argtypes = [vp, vp, i64, i64, i32, vp, C.POINTER(MpfDist), C.POINTER(MpfOpts)]
    L.mpf_solve_ir_dist.argtypes = [vp, vp, i64, vp, i64, vp, i64, i32, vp, vp, i32, dbl, C.POINTER(MpfDist), C.POINTER(MpfIrStats)]
    for name in C_ABI_SYMBOLS:
        if name != "mpf_last_error":
            getattr(L, name).restype = C.c_int
    if probe:
        L.mpf_microbench.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
        L.mpf_microbench.restype = C.c_int
    _libs[probe] = L
    return L


def option_names():
    L = load_library()
    buf = C.create_string_buffer(64)
    n = L.mpf_option_name(-1, buf, 64)
    out = []
    for i in range(n):
        L.mpf_option_name(i, buf, 64)
        out.append(buf.value.decode())
    return out


def device_report():
    """HIP analogue of the reference's check_cooperative_groups.cu probe."""
    L = load_library()
    buf = C.create_string_buffer(4096)
    n = L.mpf_device_report(buf, 4096)
    return n, buf.value.decode()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _colmajor_ld(t):
    """Leading dimension of a 2-D torch tensor that is a column-major view (stride(0) == 1)."""
    assert t.dim() == 2 and t.stride(0) == 1, "need a column-major matrix (e.g. X.t() of a contiguous tensor)"
    return t.stride(1) if t.shape[1] > 1 else max(t.shape[0], 1)


class MPFContext:
    """Owns a mpf_ctx.  Matrices are torch float64 CUDA tensors in COLUMN-MAJOR layout, i.e. a
    tensor `A` with A.stride() == (1, lda) -- create one with `colmajor(n, m)` or `from_numpy_f`."""

    def __init__(self, device=0, use_torch_stream=True, stream=None, probe=False, options=None):
        import torch
        if not torch.cuda.is_available():
            raise MPFError("no GPU visible: the MPF hot path is HIP-only (no CPU fallback)")
        self.torch = torch
        self.probe = probe
        self.L = load_library(probe)
        self.h = C.c_void_p()
        rc = self.L.mpf_create(C.byref(self.h), device)
        if rc != 0:
            raise MPFError("mpf_create failed: " + self.L.mpf_last_error(None).decode())
        self.device = torch.device("cuda", device)
        self.stream = stream  # a torch.cuda.Stream this context always launches on; None: torch's CURRENT stream,
        self._follow = stream is None and use_torch_stream  # re-read at every call (so `with torch.cuda.stream(s):` works)
        self._bound = None
        if stream is not None:
            self.L.mpf_set_stream(self.h, C.c_void_p(stream.cuda_stream))
        self._bind()
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, name, value):
        """Per-context behaviour switch (include/mpf_c.h mpf_set_option); defaults came from MPF_* at construction."""
        self._check(self.L.mpf_set_option(self.h, name.encode(), int(value)), "mpf_set_option")

    def rccl_info(self):
        """mpf_rccl_info as a dict (the multi-GPU bench line's `rccl` object is built from it)."""
        inf = MpfRcclInfo()
        self.L.mpf_rccl_info.argtypes = [C.c_void_p, C.POINTER(MpfRcclInfo)]
        self._check(self.L.mpf_rccl_info(self.h, C.byref(inf)), "mpf_rccl_info")
        nd = min(int(inf.visible_devices), 16)
        return {"version": int(inf.version), "has_comm": bool(inf.has_comm), "comm_count": int(inf.comm_count), "comm_rank": int(inf.comm_rank),
                "has_p2p": bool(inf.has_p2p), "device": int(inf.device), "visible_devices": int(inf.visible_devices),
                "bcast_calls": int(inf.bcast_calls), "bcast_bytes": int(inf.bcast_bytes), "allreduce_calls": int(inf.allreduce_calls),
                "p2p_calls": int(inf.p2p_calls), "p2p_bytes": int(inf.p2p_bytes),
                "link_type_to_device": [int(inf.link_type[d]) for d in range(nd)], "link_hops_to_device": [int(inf.link_hops[d]) for d in range(nd)],
                "peer_access_to_device": [int(inf.peer_access[d]) for d in range(nd)]}

    def rccl_bcast_probe(self, nbytes, root=0, reps=5):
        """ms per ncclBroadcast of nbytes on the context's communicator (every rank calls it)."""
        self._bind()
        ms = C.c_double(0)
        self.L.mpf_rccl_bcast_probe.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
        self._check(self.L.mpf_rccl_bcast_probe(self.h, int(nbytes), int(root), int(reps), C.byref(ms)), "mpf_rccl_bcast_probe")
        return ms.value

    def hgetf2_capacity_rows(self, waiters=0, form=0):
        """Tallest panel (rows) the LDS pivot kernel takes beside `waiters` waiting workgroups (-w: beside the pipelined chain on a
        w-column panel); form 0 = either form, 1 = full slab, 2 = column window."""
        self.L.mpf_hgetf2_capacity_rows.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        self.L.mpf_hgetf2_capacity_rows.restype = C.c_int64
        return int(self.L.mpf_hgetf2_capacity_rows(self.h, waiters, form))

    def get_option(self, name):
        v = C.c_int64(0)
        self._check(self.L.mpf_get_option(self.h, name.encode(), C.byref(v)), "mpf_get_option")
        return v.value

    def _bind(self):
        """Launch on the stream the caller's torch operations are ordered on: torch's current stream, looked up at every
        call unless an explicit stream was given at construction."""
        if self._follow:
            cur = self.torch.cuda.current_stream(self.device).cuda_stream
            if cur != self._bound:
                self.L.mpf_set_stream(self.h, C.c_void_p(cur))
                self._bound = cur

    def close(self):
        if self.h:
            for vb in list(getattr(self, "_vbatches", ())):      # a descriptor is destroyed before its context
                vb.close()
            self.L.mpf_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise MPFError(f"{what} failed ({rc}): " + self.L.mpf_last_error(self.h).decode())
        return rc

    # ---- helpers ---------------------------------------------------------------------------
    def colmajor(self, rows, cols, dtype=None):
        t = self.torch
        return t.empty((cols, rows), dtype=dtype or t.float64, device=self.device).t()

    def colmajor_batch(self, batch, rows, cols, dtype=None):
        """A tensor of logical shape (batch, rows, cols) whose matrices are column-major and packed: strides (rows * cols, 1, rows)."""
        t = self.torch
        return t.empty((batch, cols, rows), dtype=dtype or t.float64, device=self.device).transpose(1, 2)

    def from_numpy_f(self, a):
        """numpy (rows, cols) array -> column-major device tensor of the same logical shape."""
        import numpy as np
        t = self.torch
        af = np.asfortranarray(a)
        return t.from_numpy(np.ascontiguousarray(af.T)).to(self.device).t()

    def to_numpy_f(self, x):
        import numpy as np
        return np.asfortranarray(x.t().contiguous().cpu().numpy().T)

    def synchronize(self):
        self._bind()
        self._check(self.L.mpf_synchronize(self.h), "synchronize")

    def stats(self):
        s = MpfStats()
        self.L.mpf_get_stats(self.h, C.byref(s))
        return s

    def microbench(self, which):
        """0: f64 MFMA TFLOP/s, 1: f16 MFMA TFLOP/s, 2: HBM copy TB/s (measured on this box).  Probe library only:
        construct the context with probe=True."""
        if not self.probe:
            raise MPFError("microbench lives in libmpf_probe.so: MPFContext(device, probe=True)")
        self._bind()
        r = C.c_double(0)
        self._check(self.L.mpf_microbench(self.h, which, C.byref(r)), "microbench")
        return r.value

    def matgen(self, n, skip=4, out=None, col0=0, ncols=None):
        """The reference generator's matrix (matrix_generator.cpp:55-80 as benchmark.cpp reads it: `matgen f n (n-2) lin`
        for skip = 4), produced on the device; columns [col0, col0 + ncols) of it when given.  Column-major tensor."""
        self._bind()
        ncols = n - col0 if ncols is None else ncols
        if out is None:
            out = self.colmajor(n, ncols)
        assert out.shape == (n, ncols) and out.dtype == self.torch.float64
        rc = self.L.mpf_matgen_cols_dev(self.h, _ptr(out), _colmajor_ld(out), n, skip, col0, ncols)
        self._check(rc, "mpf_matgen_cols_dev")
        return out

    # ---- whole path ------------------------------------------------------------------------
    def factor(self, A, nb, ipiv=None, trailing=TRAIL_FP64, fused_panel=False, sync_timing=False, verbose=False,
               no_lookahead=False, superpanel=0, pivot_path=0, pivot_search=0, fp16_fused=None):
        """mpf_factor_dev: in-place MPF of the column-major device matrix A (N x N).
        fp16_fused: None = the context's option fp16_fused as it stands; 0 / 1 = that option for this call only (put back afterwards):
        1 = the fp16 pivot panel eliminates with one fused multiply-add per element (contract C2f: other pivots and factors).
        pivot_search: 0 = the reference's fp16 pre-pivoting, 1 = LAPACK's partial pivoting, searched in fp64, 2 = tournament pivoting
        in fp64 (mpf_dgetf2_tp's rule); also context option pivot_fp64 = 1 or 2, which gesv, gesvx, gesvx_block, gesvxx_block and factor_host follow.
        Returns (ipiv int32 device tensor, info)."""
        self._bind()
        t = self.torch
        n = A.shape[0]
        assert A.shape[1] == n and A.dtype == t.float64
        if ipiv is None:
            ipiv = t.arange(1, n + 1, dtype=t.int32, device=self.device)  # benchmark.cpp:215-217
        o = MpfOpts(trailing=trailing, verbose=int(verbose), fused_panel=int(fused_panel), sync_timing=int(sync_timing),
                    no_lookahead=int(no_lookahead), superpanel=int(superpanel), pivot_path=int(pivot_path),
                    pivot_search=int(pivot_search))
        if fp16_fused is None:
            rc = self.L.mpf_factor_dev(self.h, _ptr(A), _colmajor_ld(A), n, nb, _ptr(ipiv), C.byref(o))
        else:
            before = self.get_option("fp16_fused")
            self.set_option("fp16_fused", int(fp16_fused))
            try:
                rc = self.L.mpf_factor_dev(self.h, _ptr(A), _colmajor_ld(A), n, nb, _ptr(ipiv), C.byref(o))
            finally:
                self.set_option("fp16_fused", before)
        return ipiv, self._check(rc, "mpf_factor_dev")

    def trim(self):
        """mpf_trim: give the context's large cached buffers (host-path copies, working copies) back to the device."""
        self._bind()
        self._check(self.L.mpf_trim(self.h), "mpf_trim")

    def factor_host(self, A_np, nb, ipiv_np=None, **kw):
        """mpf_factor_host: numpy column-major matrix in host memory, factored in place."""
        import numpy as np
        assert A_np.dtype == np.float64 and A_np.flags.f_contiguous
        n = A_np.shape[0]
        if ipiv_np is None:
            ipiv_np = np.arange(1, n + 1, dtype=np.int32)
        o = MpfOpts(trailing=kw.get("trailing", TRAIL_FP64), fused_panel=int(kw.get("fused_panel", False)),
                    pivot_search=int(kw.get("pivot_search", 0)))
        rc = self.L.mpf_factor_host(self.h, C.c_void_p(A_np.ctypes.data), n, nb, C.c_void_p(ipiv_np.ctypes.data),
                                    C.byref(o))
        return ipiv_np, self._check(rc, "mpf_factor_host")

    def solve_ir(self, A, LU, ipiv, b, max_iter=10, tol=1e-12):
        self._bind()
        t = self.torch
        n = A.shape[0]
        x = t.empty(n, dtype=t.float64, device=self.device)
        st = MpfIrStats()
        rc = self.L.mpf_solve_ir(self.h, _ptr(A), _colmajor_ld(A), _ptr(LU), _colmajor_ld(LU), _ptr(ipiv), n,
                                 _ptr(b), _ptr(x), max_iter, tol, C.byref(st))
        self._check(rc, "mpf_solve_ir")
        return x, st

    def solve_ir_nrhs(self, A, LU, ipiv, B, max_iter=10, tol=1e-12):
        """mpf_solve_ir_nrhs: B is N x nrhs column-major; returns (X, list of per-column stats)."""
        self._bind()
        n, nrhs = B.shape
        X = self.colmajor(n, nrhs)
        st = (MpfIrStats * nrhs)()
        rc = self.L.mpf_solve_ir_nrhs(self.h, _ptr(A), _colmajor_ld(A), _ptr(LU), _colmajor_ld(LU), _ptr(ipiv), n, nrhs,
                                      _ptr(B), _colmajor_ld(B), _ptr(X), _colmajor_ld(X), max_iter, tol, st)
        self._check(rc, "mpf_solve_ir_nrhs")
        return X, list(st)

    def solve_gmres_ir(self, A, LU, ipiv, b, max_outer=10, restart=30, tol=1e-12):
        """mpf_solve_gmres_ir: refinement with GMRES (preconditioned by the factors) on the correction equation."""
        self._bind()
        t = self.torch
        n = A.shape[0]
        x = t.empty(n, dtype=t.float64, device=self.device)
        st = MpfGmresStats()
        rc = self.L.mpf_solve_gmres_ir(self.h, _ptr(A), _colmajor_ld(A), _ptr(LU), _colmajor_ld(LU), _ptr(ipiv), n, _ptr(b), _ptr(x),
                                       max_outer, restart, tol, C.byref(st))
        self._check(rc, "mpf_solve_gmres_ir")
        return x, st

    def check_plu(self, A, LU, ipiv):
        """The reference's acceptance test on the device (benchmark.cpp:106-144): returns (max|A - P L U|, ||.||_F / ||A||_F)."""
        self._bind()
        mx, fro = C.c_double(0), C.c_double(0)
        rc = self.L.mpf_check_plu_dev(self.h, _ptr(A), _colmajor_ld(A), _ptr(LU), _colmajor_ld(LU), _ptr(ipiv), A.shape[0],
                                      C.byref(mx), C.byref(fro))
        self._check(rc, "mpf_check_plu_dev")
        return mx.value, fro.value

    # ---- multi-GPU (one process per GPU, 1-D block-cyclic columns) ---------------------------
    def rccl_init(self, rank, world, group=None):
        """Create this context's RCCL communicator; the 128-byte unique id travels through torch.distributed."""
        import torch.distributed as tdist
        ident = [None]
        if world == 1:
            buf = C.create_string_buffer(128)
            self._check(self.L.mpf_rccl_unique_id(buf), "mpf_rccl_unique_id")
            self._check(self.L.mpf_rccl_init(self.h, buf, 0, 1), "mpf_rccl_init")
            return
        # every rank must be able to load librccl BEFORE any rank enters ncclCommInitRank (a rank that cannot would return
        # without entering the collective and leave its peers waiting there): agree on that over torch.distributed first
        loaded = [int(self.L.mpf_rccl_version() > 0)]
        everyone = [None] * world
        tdist.all_gather_object(everyone, loaded[0], group=group)
        if not all(everyone):
            raise RuntimeError(f"librccl not loadable on ranks {[r for r, ok in enumerate(everyone) if not ok]}")
        if rank == 0:   # a failure here must still reach the other ranks, or they would wait in the broadcast for ever
            buf = C.create_string_buffer(128)
            if self.L.mpf_rccl_unique_id(buf) == 0:
                ident[0] = bytes(buf.raw)
        tdist.broadcast_object_list(ident, src=0, group=group)
        if ident[0] is None:
            raise RuntimeError("mpf_rccl_unique_id failed on rank 0 (librccl not loadable?)")
        self._check(self.L.mpf_rccl_init(self.h, C.c_char_p(ident[0]), rank, world), "mpf_rccl_init")

    def dist_set_p2p(self, fn):
        """mpf_dist_set_p2p: point-to-point callback (a P2P_FN the caller keeps alive, or None) for the distributed solves' chain."""
        self._bind()
        self._check(self.L.mpf_dist_set_p2p(self.h, fn if fn is not None else C.cast(None, P2P_FN), None), "mpf_dist_set_p2p")

    def factor_dist(self, Aloc, n, nb, dist, ipiv=None, trailing=TRAIL_FP64, no_lookahead=False, pivot_path=0, verbose=False, superpanel=0,
                    pivot_search=0):
        """mpf_factor_dist: Aloc = this rank's column blocks (n x local columns, column-major); returns (ipiv, info).
        superpanel: panels per super-panel in the fp16 modes (0 = the context's default, 1 = one-level schedule)."""
        self._bind()
        t = self.torch
        if ipiv is None:
            ipiv = t.arange(1, n + 1, dtype=t.int32, device=self.device)
        o = MpfOpts(trailing=trailing, no_lookahead=int(no_lookahead), pivot_path=int(pivot_path), verbose=int(verbose), superpanel=int(superpanel),
                    pivot_search=int(pivot_search))
        ld = _colmajor_ld(Aloc) if Aloc.shape[1] > 0 else n
        rc = self.L.mpf_factor_dist(self.h, _ptr(Aloc) if Aloc.shape[1] > 0 else C.c_void_p(0), max(ld, n), n, nb, _ptr(ipiv),
                                    C.byref(dist), C.byref(o))
        return ipiv, self._check(rc, "mpf_factor_dist")

    def solve_ir_dist(self, Aloc, LUloc, ipiv, b, n, nb, dist, max_iter=10, tol=1e-12):
        self._bind()
        t = self.torch
        x = t.empty(n, dtype=t.float64, device=self.device)
        st = MpfIrStats()
        has = Aloc.shape[1] > 0
        rc = self.L.mpf_solve_ir_dist(self.h, _ptr(Aloc) if has else C.c_void_p(0), max(_colmajor_ld(Aloc), n) if has else n,
                                      _ptr(LUloc) if has else C.c_void_p(0), max(_colmajor_ld(LUloc), n) if has else n, _ptr(ipiv),
                                      n, nb, _ptr(b), _ptr(x), max_iter, tol, C.byref(dist), C.byref(st))
        self._check(rc, "mpf_solve_ir_dist")
        return x, st

    # ---- step operators --------------------------------------------------------------------
    def double_to_fp16(self, x):
        self._bind()
        t = self.torch
        out = t.empty(x.numel(), dtype=t.int16, device=self.device)
        self._check(self.L.mpf_double_to_fp16(self.h, _ptr(x), _ptr(out), x.numel()), "double_to_fp16")
        return out

    def hdiv(self, a_bits, b_bits):
        self._bind()
        t = self.torch
        q = t.empty_like(a_bits)
        self._check(self.L.mpf_hdiv(self.h, _ptr(a_bits), _ptr(b_bits), _ptr(q), a_bits.numel()), "hdiv")
        return q

    def hgetf2_pivots(self, P, ipiv_offset=0, want_panel=False):
        """P: column-major fp64 view rows x cols.  Returns (ipiv int32[cols], fp16 panel bits or None)."""
        self._bind()
        t = self.torch
        rows, cols = P.shape
        ipiv = t.zeros(cols, dtype=t.int32, device=self.device)
        out = self.colmajor(rows, cols, dtype=t.int16) if want_panel else None
        rc = self.L.mpf_hgetf2_pivots(self.h, _ptr(P), _colmajor_ld(P), rows, cols, ipiv_offset, _ptr(ipiv), _ptr(out))
        self._check(rc, "hgetf2_pivots")
        return ipiv, out

    def hgetf2(self, P16):
        self._bind()
        t = self.torch
        rows, cols = P16.shape
        ipiv = t.zeros(cols, dtype=t.int32, device=self.device)
        self._check(self.L.mpf_hgetf2(self.h, _ptr(P16), _colmajor_ld(P16), rows, cols, _ptr(ipiv)), "hgetf2")
        return ipiv

    def laswp(self, A, k, cols, ipiv_global):
        self._bind()
        self._check(self.L.mpf_laswp(self.h, _ptr(A), _colmajor_ld(A), A.shape[1], k, cols, _ptr(ipiv_global)), "laswp")

    def dgetf2_npv(self, P, fused=False):
        self._bind()
        rows, cols = P.shape
        self._check(self.L.mpf_dgetf2_npv(self.h, _ptr(P), _colmajor_ld(P), rows, cols, int(fused)), "dgetf2_npv")

    def dgetf2_piv(self, P, fused=False, ipiv_offset=0):
        """mpf_dgetf2_piv: LAPACK dgetf2 (fp64 partial pivoting) in place on the column-major panel P (rows x cols).
        Returns (ipiv int32[min(rows, cols)] = pivot row + 1 + ipiv_offset, info = first zero pivot or 0)."""
        self._bind()
        t = self.torch
        rows, cols = P.shape
        ipiv = t.zeros(min(rows, cols), dtype=t.int32, device=self.device)
        info = C.c_int32(0)
        self._check(self.L.mpf_dgetf2_piv(self.h, _ptr(P), _colmajor_ld(P), rows, cols, int(fused), int(ipiv_offset), _ptr(ipiv),
                                          C.byref(info)), "dgetf2_piv")
        return ipiv, info.value

    def dgetf2_tp(self, P, fused=False, ipiv_offset=0):
        """mpf_dgetf2_tp: the same panel with tournament pivoting (the rule in include/mpf_c.h), in place on the column-major panel P.
        Returns (ipiv int32[min(rows, cols)] = pivot row + 1 + ipiv_offset, info = first zero diagonal entry or 0)."""
        self._bind()
        t = self.torch
        rows, cols = P.shape
        ipiv = t.zeros(min(rows, cols), dtype=t.int32, device=self.device)
        info = C.c_int32(0)
        self._check(self.L.mpf_dgetf2_tp(self.h, _ptr(P), _colmajor_ld(P), rows, cols, int(fused), int(ipiv_offset), _ptr(ipiv),
                                         C.byref(info)), "dgetf2_tp")
        return ipiv, info.value

    def dtrsm_llnu(self, Lm, B):
        self._bind()
        m, n = B.shape
        assert Lm.shape[0] >= m and Lm.shape[1] >= m, "dtrsm_llnu: L smaller than m x m"
        self._check(self.L.mpf_dtrsm_llnu(self.h, m, n, _ptr(Lm), _colmajor_ld(Lm), _ptr(B), _colmajor_ld(B)), "dtrsm")

    def dgemm_minus(self, Cm, A, B):
        self._bind()
        m, n = Cm.shape
        k = A.shape[1]
        assert A.shape == (m, k) and B.shape == (k, n), "dgemm_minus: operand shapes do not match C"
        self._check(self.L.mpf_dgemm_minus(self.h, m, n, k, _ptr(A), _colmajor_ld(A), _ptr(B), _colmajor_ld(B),
                                           _ptr(Cm), _colmajor_ld(Cm)), "dgemm")

    def hgemm_minus(self, Cm, A, B, split=False):
        """fp16-in / fp32-accumulate variant of dgemm_minus (speed mode of the trailing update); split=True uses
        hi + 2^-11 lo operands (three MFMA products, fp32-class accuracy)."""
        self._bind()
        m, n = Cm.shape
        k = A.shape[1]
        assert A.shape == (m, k) and B.shape == (k, n), "hgemm_minus: operand shapes do not match C"
        self._check(self.L.mpf_hgemm_minus(self.h, m, n, k, _ptr(A), _colmajor_ld(A), _ptr(B), _colmajor_ld(B),
                                           _ptr(Cm), _colmajor_ld(Cm), int(split)), "hgemm")

    def hgemm_minus_f32(self, Cm, A, B, split=False):
        """mpf_hgemm_minus_f32: the fp16 update on an fp32 column-major matrix (the fp16 modes' working copy)."""
        self._bind()
        assert Cm.dtype == self.torch.float32
        m, n = Cm.shape
        k = A.shape[1]
        assert A.shape == (m, k) and B.shape == (k, n), "hgemm_minus_f32: operand shapes do not match C"
        self._check(self.L.mpf_hgemm_minus_f32(self.h, m, n, k, _ptr(A), _colmajor_ld(A), _ptr(B), _colmajor_ld(B),
                                               _ptr(Cm), _colmajor_ld(Cm), int(split)), "hgemm_f32")

    # the fp32 working copy of the fp16 modes (row-major torch float32 tensors: W[i, j] contiguous in j)
    def w32_from_f64(self, A, W):
        self._bind()
        rows, cols = A.shape
        assert W.shape == (rows, cols) and W.dtype == self.torch.float32 and W.stride(1) == 1
        self._check(self.L.mpf_w32_from_f64(self.h, _ptr(A), _colmajor_ld(A), _ptr(W), W.stride(0), rows, cols), "w32_from_f64")

    def w32_to_f64(self, W, A):
        self._bind()
        rows, cols = A.shape
        assert W.shape == (rows, cols) and W.dtype == self.torch.float32 and W.stride(1) == 1
        self._check(self.L.mpf_w32_to_f64(self.h, _ptr(W), W.stride(0), _ptr(A), _colmajor_ld(A), rows, cols), "w32_to_f64")

    def w32_laswp(self, W, k, cols, ipiv_global):
        self._bind()
        assert W.dtype == self.torch.float32 and W.stride(1) == 1
        self._check(self.L.mpf_w32_laswp(self.h, _ptr(W), W.stride(0), W.shape[1], k, cols, _ptr(ipiv_global)), "w32_laswp")

    def gesv(self, A, b, nb=256, max_iter=10, tol=1e-12, try_fp16=True, work=None):
        """mpf_gesv: x with ||b - A x|| / ||b|| <= tol by the fastest path (fp16 trailing + refinement, else fp64)."""
        self._bind()
        t = self.torch
        n = A.shape[0]
        if work is None:
            work = self.colmajor(n, n)
        ipiv = t.empty(n, dtype=t.int32, device=self.device)
        x = t.empty(n, dtype=t.float64, device=self.device)
        st = MpfGesvStats()
        rc = self.L.mpf_gesv(self.h, _ptr(A), _colmajor_ld(A), n, nb, _ptr(work), _ptr(ipiv), _ptr(b), _ptr(x), max_iter, tol,
                             int(try_fp16), C.byref(st))  # try_fp16: 0 fp64 only, 1/True fp16, 2 fp16x3
        self._check(rc, "mpf_gesv")
        return x, st, work, ipiv

    # ---- expert driver (include/mpf_c.h: transposed solve, norms, equilibration, condition estimate) ------------------------
    def solve_ir_trans(self, A, LU, ipiv, B, max_iter=10, tol=1e-12):
        """mpf_solve_ir_trans: A^T X = B with the factors of A.  B: vector (N) or N x nrhs column-major; returns (X, stats) --
        stats a list per column when B is a matrix."""
        self._bind()
        n = A.shape[0]
        vec = B.dim() == 1
        nrhs = 1 if vec else B.shape[1]
        X = self.torch.empty(n, dtype=self.torch.float64, device=self.device) if vec else self.colmajor(n, nrhs)
        st = (MpfIrStats * max(nrhs, 1))()
        ldb = n if vec else _colmajor_ld(B)
        ldx = n if vec else _colmajor_ld(X)
        rc = self.L.mpf_solve_ir_trans(self.h, _ptr(A), _colmajor_ld(A), _ptr(LU), _colmajor_ld(LU), _ptr(ipiv), n, nrhs,
                                       _ptr(B), ldb, _ptr(X), ldx, max_iter, tol, st)
        self._check(rc, "mpf_solve_ir_trans")
        return X, (st[0] if vec else list(st)[:nrhs])

    def lange(self, A, norm="1"):
        """mpf_lange: '1'/'O', 'I', 'M' or 'F' norm of the column-major matrix A (M x N)."""
        self._bind()
        m, n = A.shape
        out = C.c_double(0)
        ld = _colmajor_ld(A) if m > 0 and n > 0 else max(m, 1)
        self._check(self.L.mpf_lange(self.h, _ptr(A), ld, m, n, norm.encode()[:1], C.byref(out)), "mpf_lange")
        return out.value

    def geequ(self, A):
        """mpf_geequ: power-of-two row / column scale factors.  Returns (r, c, rowcnd, colcnd, amax, info)."""
        self._bind()
        t = self.torch
        n = A.shape[0]
        r = t.zeros(n, dtype=t.float64, device=self.device)
        c = t.zeros(n, dtype=t.float64, device=self.device)
        rc_, cc_, am = C.c_double(0), C.c_double(0), C.c_double(0)
        info = self._check(self.L.mpf_geequ(self.h, _ptr(A), _colmajor_ld(A), n, _ptr(r), _ptr(c), C.byref(rc_), C.byref(cc_), C.byref(am)),
                           "mpf_geequ")
        return r, c, rc_.value, cc_.value, am.value, info

    def gecon(self, LU, anorm, norm="1"):
        """mpf_gecon: reciprocal condition number of the factored matrix (LAPACK dgecon).  Returns (rcond, stats)."""
        self._bind()
        rcond = C.c_double(0)
        st = MpfGeconStats()
        self._check(self.L.mpf_gecon(self.h, _ptr(LU), _colmajor_ld(LU), LU.shape[0], norm.encode()[:1], float(anorm), C.byref(rcond),
                                     C.byref(st)), "mpf_gecon")
        return rcond.value, st

    def cond(self, A, LU, ipiv=None, norm="1"):
        """Estimated condition number of A from its factors: anorm * ||(L U)^-1|| = 1 / rcond (norm '1' or 'I'; ipiv is accepted
        for symmetry with the solves -- the pivots change neither norm).  inf where rcond is 0."""
        anorm = self.lange(A, norm)
        rcond, _ = self.gecon(LU, anorm, norm)
        return float("inf") if rcond == 0 else 1.0 / rcond

    def gesvx(self, A, b, nb=256, trans=False, equilibrate=1, try_fp16=1, kappa_max=0.0, max_iter=10, tol=1e-12, work=None,
              want_scales=False):
        """mpf_gesvx: equilibrate, factor (try_fp16: 0 fp64, 1 fp16, 2 fp16x3), estimate rcond, refine against A, fall back to
        fp64.  Returns (x, stats, work, ipiv) and, with want_scales, (r, c) as well."""
        self._bind()
        t = self.torch
        n = A.shape[0]
        if work is None:
            work = self.colmajor(n, n)
        ipiv = t.empty(n, dtype=t.int32, device=self.device)
        x = t.empty(n, dtype=t.float64, device=self.device)
        r = t.empty(n, dtype=t.float64, device=self.device) if want_scales else None
        c = t.empty(n, dtype=t.float64, device=self.device) if want_scales else None
        st = MpfGesvxStats()
        rc = self.L.mpf_gesvx(self.h, _ptr(A), _colmajor_ld(A), n, nb, _ptr(work), _ptr(ipiv), _ptr(b), _ptr(x), int(bool(trans)),
                              int(equilibrate), int(try_fp16), float(kappa_max), max_iter, tol, _ptr(r), _ptr(c), C.byref(st))
        self._check(rc, "mpf_gesvx")
        out = (x, st, work, ipiv)
        return out + (r, c) if want_scales else out

    # ---- blocked multi-right-hand-side solve (include/mpf_c.h: mpf_getrs, mpf_solve_ir_block) -----------------------------------
    def _rhs(self, B):
        """(matrix view, nrhs, ld) of a vector (N) or N x nrhs column-major right-hand side."""
        if B.dim() == 1:
            return B.view(-1, 1), 1, max(B.shape[0], 1)
        return B, B.shape[1], _colmajor_ld(B)

    def _out_like(self, n, B):
        """(new output, ld) shaped like the right-hand side B: a vector when B is, else n x nrhs column-major."""
        if B.dim() == 1:
            return self.torch.empty(n, dtype=self.torch.float64, device=self.device), n
        X = self.colmajor(n, B.shape[1])
        return X, _colmajor_ld(X)

    def _inout(self, n, X, overwrite):
        """X itself (overwrite), or a copy of it: a vector's clone, a matrix's column-major copy."""
        if overwrite:
            return X
        if X.dim() == 1:
            return X.clone()
        Xc = self.colmajor(n, X.shape[1])
        Xc.copy_(X)
        return Xc

    def getrs(self, LU, ipiv, B, trans=False, overwrite=False):
        """mpf_getrs: X = A^-1 B (or A^-T B) with the factors of A.  Returns a new column-major X and leaves B untouched, unless
        overwrite=True: then B itself is solved in place and returned."""
        self._bind()
        n = LU.shape[0]
        X = self._inout(n, B, overwrite)
        _, nrhs, ldx = self._rhs(X)
        rc = self.L.mpf_getrs(self.h, int(bool(trans)), _ptr(LU), _colmajor_ld(LU), _ptr(ipiv), n, nrhs, _ptr(X), ldx)
        self._check(rc, "mpf_getrs")
        return X

    def solve_ir_block(self, A, LU, ipiv, B, trans=False, max_iter=10, tol=1e-12):
        """mpf_solve_ir_block: refinement of all columns of B together (per-column rules of solve_ir_nrhs / solve_ir_trans).
        Returns (X, list of per-column stats); X is a vector when B is."""
        self._bind()
        n = A.shape[0]
        _, nrhs, ldb = self._rhs(B)
        X, ldx = self._out_like(n, B)
        st = (MpfIrStats * max(nrhs, 1))()
        rc = self.L.mpf_solve_ir_block(self.h, int(bool(trans)), _ptr(A), _colmajor_ld(A), _ptr(LU), _colmajor_ld(LU), _ptr(ipiv), n,
                                       nrhs, _ptr(B), ldb, _ptr(X), ldx, max_iter, tol, st)
        self._check(rc, "mpf_solve_ir_block")
        return X, list(st)[:nrhs]

    def solve_gmres_ir_block(self, A, LU, ipiv, B, trans=False, max_outer=10, restart=30, tol=1e-12):
        """mpf_solve_gmres_ir_block: GMRES-IR on all columns of B together, op(A) = A or A^T (trans).  Returns (X, list of per-column
        MpfGmresStats); X is a vector when B is.  A column that did not converge does not raise: its stats say so."""
        self._bind()
        n = A.shape[0]
        _, nrhs, ldb = self._rhs(B)
        X, ldx = self._out_like(n, B)
        st = (MpfGmresStats * max(nrhs, 1))()
        rc = self.L.mpf_solve_gmres_ir_block(self.h, int(bool(trans)), _ptr(A), _colmajor_ld(A), _ptr(LU), _colmajor_ld(LU), _ptr(ipiv), n,
                                             nrhs, _ptr(B), ldb, _ptr(X), ldx, max_outer, restart, tol, st)
        self._check(rc, "mpf_solve_gmres_ir_block")
        return X, list(st)[:nrhs]

    # ---- error bounds for solves (include/mpf_c.h: mpf_gerfs) -------------------------------------------------------------------
    def gerfs(self, A, LU, ipiv, B, X, trans=False, itmax=0, overwrite=False):
        """mpf_gerfs (LAPACK dgerfs): refines the solution X of op(A) X = B and returns (X, ferr, berr, stats) -- ferr and berr numpy
        arrays with one entry per column, stats a list per column.  X is copied first and B, X stay untouched, unless
        overwrite=True: then X itself is refined in place and returned.  itmax = 0: LAPACK's 5 corrections at most."""
        import numpy as np
        self._bind()
        n = A.shape[0]
        Xr = self._inout(n, X, overwrite)
        _, nrhs, ldb = self._rhs(B)
        _, nx, ldx = self._rhs(Xr)
        assert nx == nrhs, "gerfs: B and X need the same number of columns"
        ferr, berr = np.zeros(max(nrhs, 1)), np.zeros(max(nrhs, 1))
        st = (MpfGerfsStats * max(nrhs, 1))()
        dp = C.POINTER(C.c_double)
        rc = self.L.mpf_gerfs(self.h, int(bool(trans)), _ptr(A), _colmajor_ld(A), _ptr(LU), _colmajor_ld(LU), _ptr(ipiv), n, nrhs,
                              _ptr(B), ldb, _ptr(Xr), ldx, int(itmax), ferr.ctypes.data_as(dp), berr.ctypes.data_as(dp), st)
        self._check(rc, "mpf_gerfs")
        return Xr, ferr[:nrhs], berr[:nrhs], list(st)[:nrhs]

    # ---- extra-precise refinement (include/mpf_c.h: mpf_residual_x, mpf_gerfsx) -------------------------------------------------------
    def residual_x(self, A, X, B, trans=False):
        """mpf_residual_x: R = B - op(A) X with every element accumulated in twice the working precision and rounded once.  Returns
        a new R (a vector when B is); A, X, B stay untouched."""
        self._bind()
        n = A.shape[0]
        _, nrhs, ldb = self._rhs(B)
        _, nx, ldx = self._rhs(X)
        assert nx == nrhs, "residual_x: B and X need the same number of columns"
        R, ldr = self._out_like(n, B)
        rc = self.L.mpf_residual_x(self.h, int(bool(trans)), _ptr(A), _colmajor_ld(A), n, nrhs, _ptr(X), ldx, _ptr(B), ldb, _ptr(R), ldr)
        self._check(rc, "mpf_residual_x")
        return R

    def gerfsx(self, A, LU, ipiv, B, X, trans=False, ithresh=0, overwrite=False):
        """mpf_gerfsx (LAPACK dgerfsx with the extra-precise residual): refines the solution X of op(A) X = B and returns
        (X, err_norm, err_comp, stats) -- the normwise and componentwise forward error bounds as numpy arrays with one entry per column,
        stats a list per column (x_state 2 = converged).  X is copied first and B, X stay untouched, unless overwrite=True: then X itself
        is refined in place and returned.  ithresh = 0: LAPACK's 10 iterations at most.  A column that did not converge does not raise:
        its stats say so."""
        import numpy as np
        self._bind()
        n = A.shape[0]
        Xr = self._inout(n, X, overwrite)
        _, nrhs, ldb = self._rhs(B)
        _, nx, ldx = self._rhs(Xr)
        assert nx == nrhs, "gerfsx: B and X need the same number of columns"
        en, ec = np.zeros(max(nrhs, 1)), np.zeros(max(nrhs, 1))
        st = (MpfGerfsxStats * max(nrhs, 1))()
        dp = C.POINTER(C.c_double)
        rc = self.L.mpf_gerfsx(self.h, int(bool(trans)), _ptr(A), _colmajor_ld(A), _ptr(LU), _colmajor_ld(LU), _ptr(ipiv), n, nrhs,
                               _ptr(B), ldb, _ptr(Xr), ldx, int(ithresh), en.ctypes.data_as(dp), ec.ctypes.data_as(dp), st)
        self._check(rc, "mpf_gerfsx")
        return Xr, en[:nrhs], ec[:nrhs], list(st)[:nrhs]

    # ---- expert driver for many right-hand sides (include/mpf_c.h: mpf_gesvx_block) ---------------------------------------------
    def gesvx_block(self, A, B, nb=256, trans=False, equilibrate=1, try_fp16=1, kappa_max=0.0, max_iter=10, tol=1e-12, itmax=0,
                    bounds=True, work=None, want_scales=False):
        """mpf_gesvx_block: mpf_gesvx's steps with one factorization for all columns of B (a vector or N x nrhs column-major):
        blocked refinement against A and, with bounds, dgerfs's berr and ferr of the original system.  Returns
        (X, ferr, berr, stats, ir_stats, gerfs_stats, work, ipiv) and, with want_scales, (r, c) as well; ferr, berr (numpy arrays)
        and gerfs_stats (a list per column, like ir_stats) are None with bounds=False.  X is a vector when B is."""
        import numpy as np
        self._bind()
        t = self.torch
        n = A.shape[0]
        _, nrhs, ldb = self._rhs(B)
        if work is None:
            work = self.colmajor(n, n)
        ipiv = t.empty(n, dtype=t.int32, device=self.device)
        X, ldx = self._out_like(n, B)
        r = t.empty(n, dtype=t.float64, device=self.device) if want_scales else None
        c = t.empty(n, dtype=t.float64, device=self.device) if want_scales else None
        st = MpfGesvxStats()
        ist = (MpfIrStats * max(nrhs, 1))()
        rst = (MpfGerfsStats * max(nrhs, 1))()
        dp = C.POINTER(C.c_double)
        ferr = np.zeros(max(nrhs, 1)) if bounds else None
        berr = np.zeros(max(nrhs, 1)) if bounds else None
        rc = self.L.mpf_gesvx_block(self.h, _ptr(A), _colmajor_ld(A), n, nb, _ptr(work), _ptr(ipiv), nrhs, _ptr(B), ldb, _ptr(X), ldx,
                                    int(bool(trans)), int(equilibrate), int(try_fp16), float(kappa_max), max_iter, tol, int(itmax),
                                    _ptr(r), _ptr(c), ferr.ctypes.data_as(dp) if bounds else None,
                                    berr.ctypes.data_as(dp) if bounds else None, C.byref(st), ist, rst)
        self._check(rc, "mpf_gesvx_block")
        out = (X, ferr[:nrhs] if bounds else None, berr[:nrhs] if bounds else None, st, list(ist)[:nrhs],
               list(rst)[:nrhs] if bounds else None, work, ipiv)
        return out + (r, c) if want_scales else out

    # ---- extra-precise expert solve (include/mpf_c.h: mpf_gerpvgrw, mpf_gerfsx_scaled, mpf_gesvxx_block) --------------------------------
    def gerpvgrw(self, A, LU, r=None, c=None):
        """mpf_gerpvgrw (LAPACK dla_gerpvgrw): the reciprocal pivot growth min(1, min_j max_i |a_ij r_i c_j| / max_{i <= j} |u_ij|) of
        the factors LU of Dr A Dc; r, c: the scale vectors as device tensors, or None for the identity.  Returns a float."""
        self._bind()
        out = C.c_double(0)
        rc = self.L.mpf_gerpvgrw(self.h, _ptr(A), _colmajor_ld(A), _ptr(LU), _colmajor_ld(LU), A.shape[0], _ptr(r), _ptr(c), C.byref(out))
        self._check(rc, "mpf_gerpvgrw")
        return out.value

    def gerfsx_scaled(self, A, LU, ipiv, B, X, trans=False, ithresh=0, r=None, c=None, want_berr=True, overwrite=False):
        """mpf_gerfsx_scaled: gerfsx with LU the factors of Dr A Dc (r, c: device tensors or None) and, with want_berr, the componentwise
        backward error of the returned X.  Returns (X, err_norm, err_comp, berr, stats); berr is None without want_berr.  X, B and
        overwrite as gerfsx."""
        import numpy as np
        self._bind()
        n = A.shape[0]
        Xr = self._inout(n, X, overwrite)
        _, nrhs, ldb = self._rhs(B)
        _, nx, ldx = self._rhs(Xr)
        assert nx == nrhs, "gerfsx_scaled: B and X need the same number of columns"
        en, ec, be = np.zeros(max(nrhs, 1)), np.zeros(max(nrhs, 1)), np.zeros(max(nrhs, 1))
        st = (MpfGerfsxStats * max(nrhs, 1))()
        dp = C.POINTER(C.c_double)
        rc = self.L.mpf_gerfsx_scaled(self.h, int(bool(trans)), _ptr(A), _colmajor_ld(A), _ptr(LU), _colmajor_ld(LU), _ptr(ipiv), n, nrhs,
                                      _ptr(B), ldb, _ptr(Xr), ldx, int(ithresh), _ptr(r), _ptr(c), en.ctypes.data_as(dp),
                                      ec.ctypes.data_as(dp), be.ctypes.data_as(dp) if want_berr else None, st)
        self._check(rc, "mpf_gerfsx_scaled")
        return Xr, en[:nrhs], ec[:nrhs], be[:nrhs] if want_berr else None, list(st)[:nrhs]

    def gesvxx_block(self, A, B, nb=256, trans=False, equilibrate=1, try_fp16=1, kappa_max=0.0, max_iter=10, tol=1e-12, ithresh=0,
                     want_berr=True, want_rpvgrw=True, work=None, want_scales=False):
        """mpf_gesvxx_block: gesvx_block's steps with the extra-precise refinement after the plain one, gerfsx's two forward error
        bounds of the original system, berr and the reciprocal pivot growth.  Returns (X, err_norm, err_comp, berr, rpvgrw, stats,
        ir_stats, gerfsx_stats, work, ipiv) and, with want_scales, (r, c) as well; berr / rpvgrw are None when not asked for.  X is a
        vector when B is.  A column that did not converge does not raise: gerfsx_stats say so (x_state 2 = converged)."""
        import numpy as np
        self._bind()
        t = self.torch
        n = A.shape[0]
        _, nrhs, ldb = self._rhs(B)
        if work is None:
            work = self.colmajor(n, n)
        ipiv = t.empty(n, dtype=t.int32, device=self.device)
        X, ldx = self._out_like(n, B)
        r = t.empty(n, dtype=t.float64, device=self.device) if want_scales else None
        c = t.empty(n, dtype=t.float64, device=self.device) if want_scales else None
        st = MpfGesvxStats()
        ist = (MpfIrStats * max(nrhs, 1))()
        xst = (MpfGerfsxStats * max(nrhs, 1))()
        dp = C.POINTER(C.c_double)
        en, ec, be = np.zeros(max(nrhs, 1)), np.zeros(max(nrhs, 1)), np.zeros(max(nrhs, 1))
        pg = C.c_double(0)
        rc = self.L.mpf_gesvxx_block(self.h, _ptr(A), _colmajor_ld(A), n, nb, _ptr(work), _ptr(ipiv), nrhs, _ptr(B), ldb, _ptr(X), ldx,
                                     int(bool(trans)), int(equilibrate), int(try_fp16), float(kappa_max), max_iter, tol, int(ithresh),
                                     _ptr(r), _ptr(c), en.ctypes.data_as(dp), ec.ctypes.data_as(dp),
                                     be.ctypes.data_as(dp) if want_berr else None, C.byref(pg) if want_rpvgrw else None, C.byref(st), ist, xst)
        self._check(rc, "mpf_gesvxx_block")
        out = (X, en[:nrhs], ec[:nrhs], be[:nrhs] if want_berr else None, pg.value if want_rpvgrw else None, st, list(ist)[:nrhs],
               list(xst)[:nrhs], work, ipiv)
        return out + (r, c) if want_scales else out

    # ---- inverse and determinant from the factors (include/mpf_c.h: mpf_getri, mpf_getdet) ---------------------------------------------
    def _factor_args(self, LU, ipiv, r, c):
        """The argument checks getri and getdet share: a square float64 LU, int32 pivots and float64 scales of its size, all on the device."""
        t = self.torch
        n = LU.shape[0]
        assert LU.dim() == 2 and LU.shape[1] == n and LU.dtype == t.float64 and LU.is_cuda
        assert ipiv.dtype == t.int32 and ipiv.is_cuda and ipiv.dim() == 1 and ipiv.numel() == n and ipiv.is_contiguous(), \
            "ipiv: a contiguous int32 device tensor of N entries"
        for s in (r, c):
            assert s is None or (s.dtype == t.float64 and s.is_cuda and s.dim() == 1 and s.numel() == n and s.is_contiguous()), \
                "r, c: contiguous float64 device tensors of N entries, or None"
        return n

    def getri(self, LU, ipiv, r=None, c=None, out=None):
        """mpf_getri (LAPACK dgetri): inv(A) from the factors LU, ipiv of Dr A Dc (r, c: the scale vectors as device tensors, or None
        for the identity), out of place.  out: a column-major N x N tensor to receive it (a new one when None).  Returns (inv, info):
        info = i + 1 when u_ii is the first zero on U's diagonal -- `out` is then untouched -- else 0."""
        self._bind()
        n = self._factor_args(LU, ipiv, r, c)
        if out is None:
            out = self.colmajor(n, n)
        assert out.shape == (n, n) and out.dtype == self.torch.float64 and out.is_cuda
        rc = self.L.mpf_getri(self.h, _ptr(LU), _colmajor_ld(LU), _ptr(ipiv), n, _ptr(r), _ptr(c), _ptr(out), _colmajor_ld(out))
        return out, self._check(rc, "mpf_getri")

    def getdet(self, LU, ipiv, r=None, c=None):
        """mpf_getdet: det(A) = mant * 2**expo from the factors of Dr A Dc, |mant| in [0.5, 1) or 0 (no overflow at any N).  Returns
        (mant, expo) as a float and an int; (0.0, 0) for a singular U, (nan, 0) for a non-finite one."""
        self._bind()
        n = self._factor_args(LU, ipiv, r, c)
        mant, expo = C.c_double(0), C.c_int64(0)
        rc = self.L.mpf_getdet(self.h, _ptr(LU), _colmajor_ld(LU), _ptr(ipiv), n, _ptr(r), _ptr(c), C.byref(mant), C.byref(expo))
        self._check(rc, "mpf_getdet")
        return mant.value, expo.value

    def slogdet(self, LU, ipiv, r=None, c=None):
        """(sign, log|det A|) as numpy.linalg.slogdet returns them, from getdet: log|mant| + expo ln 2 on the host -- one rounded
        logarithm, not N.  (0.0, -inf) for a singular U."""
        import math
        mant, expo = self.getdet(LU, ipiv, r, c)
        if mant == 0.0:
            return 0.0, -math.inf
        if math.isnan(mant):
            return math.nan, math.nan
        return math.copysign(1.0, mant), math.log(abs(mant)) + expo * math.log(2.0)

    def inv(self, A, nb=256, **factor_kw):
        """inv(A): factors a copy of A (factor's keyword arguments apply), then getri.  Raises MPFError when U has a zero pivot."""
        W = self.colmajor(A.shape[0], A.shape[0])
        W.copy_(A)
        ipiv, info = self.factor(W, nb, **factor_kw)
        X, info2 = self.getri(W, ipiv)
        if info or info2:
            raise MPFError(f"inv: the matrix is singular (zero pivot {info or info2})")
        return X

    # ---- LU of many small matrices (include/mpf_c.h: mpf_getrf_batched, mpf_getrs_batched) ----------------------------------------------
    @staticmethod
    def _batch_layout(M):
        """(ld, stride) of a (batch, rows, cols) tensor whose matrices are column-major as they stand (stride 1 along the rows,
        ld >= rows, matrices that do not overlap), or None: such a tensor has to be copied."""
        b, r, c = M.shape
        s0, s1, s2 = M.stride()
        if r > 1 and s1 != 1:
            return None
        ld = s2 if c > 1 else max(r, 1)
        if ld < max(r, 1) or (b > 1 and s0 < ld * c):
            return None
        return ld, (s0 if b > 1 else ld * c)

    def _batch_arg(self, M, what, overwrite, copy=True):
        """(tensor, ld, stride) the library takes: M itself when overwrite (an error unless its matrices are column-major), else a
        packed column-major copy; copy=False: M itself when its layout allows (read-only arguments)."""
        t = self.torch
        assert M.dim() == 3 and M.dtype == t.float64 and M.is_cuda, f"{what}: a (batch, rows, cols) float64 device tensor"
        lay = self._batch_layout(M)
        if overwrite and lay is None:
            raise MPFError(f"{what}: overwrite=True needs column-major matrices (MPFContext.colmajor_batch); this tensor would be copied")
        if not overwrite and (copy or lay is None):
            W = self.colmajor_batch(*M.shape)
            W.copy_(M)
            M, lay = W, self._batch_layout(W)
        return (M,) + lay

    def getrf_batched(self, A, fused=False, overwrite=False, ipiv=None, info=None):
        """mpf_getrf_batched: LAPACK dgetrf (fp64 partial pivoting, mpf_dgetf2_piv's pivots and bits) of every matrix of the
        (batch, n, n) tensor A, n <= 128.  Returns (LU, ipiv, info): LU a column-major batch (A itself with overwrite=True, which
        needs A's matrices column-major -- any other layout, torch's row-major default included, is copied), ipiv int32 (batch, n),
        1-based, info int32 (batch,) on the device: the first zero pivot of each matrix or 0.  ipiv / info: tensors to receive them
        (ipiv rows may be padded: stride(1) == 1, stride(0) >= n)."""
        return self._getrf_batched(A, fused, overwrite, ipiv, info, "getrf_batched")

    def _getrf_batched(self, A, fused, overwrite, ipiv, info, entry):
        self._bind()
        t = self.torch
        assert A.dim() == 3 and A.shape[1] == A.shape[2], "A: (batch, n, n)"
        batch, n = A.shape[0], A.shape[1]
        LU, lda, stride = self._batch_arg(A, entry, overwrite)
        if ipiv is None:
            ipiv = t.zeros((batch, n), dtype=t.int32, device=self.device)
        if info is None:
            info = t.zeros(batch, dtype=t.int32, device=self.device)
        assert ipiv.dtype == t.int32 and ipiv.is_cuda and ipiv.shape == (batch, n) and (n <= 1 or ipiv.stride(1) == 1)
        assert info.dtype == t.int32 and info.is_cuda and info.shape == (batch,) and info.is_contiguous()
        sp = ipiv.stride(0) if batch > 1 else max(n, 1)
        rc = getattr(self.L, "mpf_" + entry)(self.h, _ptr(LU), lda, stride, n, batch, _ptr(ipiv), sp, _ptr(info), int(bool(fused)))
        self._check(rc, "mpf_" + entry)
        return LU, ipiv, info

    def getrs_batched(self, LU, ipiv, B, trans=False, overwrite=False):
        """mpf_getrs_batched: X[b] = A[b]^-1 B[b] (or A[b]^-T B[b]) with the factors of getrf_batched; B is (batch, n, nrhs), or
        (batch, n) for one right-hand side each.  Returns a new column-major X and leaves B untouched, unless overwrite=True: then B
        itself (column-major matrices) is solved in place and returned."""
        return self._getrs_batched(LU, ipiv, B, trans, overwrite, "getrs_batched")

    def _getrs_batched(self, LU, ipiv, B, trans, overwrite, entry):
        self._bind()
        t = self.torch
        if B.dim() == 2:
            return self._getrs_batched(LU, ipiv, B.unsqueeze(2), trans, overwrite, entry).squeeze(2)
        assert LU.dim() == 3 and LU.shape[1] == LU.shape[2] and B.dim() == 3 and B.shape[:2] == LU.shape[:2], "LU: (batch, n, n), B: (batch, n, nrhs)"
        batch, n, nrhs = B.shape
        LUm, ldlu, slu = self._batch_arg(LU, entry, False, copy=False)
        assert ipiv.dtype == t.int32 and ipiv.is_cuda and ipiv.shape == (batch, n)
        if n > 1 and ipiv.stride(1) != 1:
            ipiv = ipiv.contiguous()
        sp = ipiv.stride(0) if batch > 1 else max(n, 1)
        X, ldb, sb = self._batch_arg(B, entry, overwrite)
        rc = getattr(self.L, "mpf_" + entry)(self.h, int(bool(trans)), _ptr(LUm), ldlu, slu, n, batch, _ptr(ipiv), sp, nrhs, _ptr(X), ldb, sb)
        self._check(rc, "mpf_" + entry)
        return X

    def solve_batched(self, A, B, trans=False):
        """X[b] = A[b]^-1 B[b] (or A[b]^-T B[b]) for a (batch, n, n) tensor A, n <= 128: getrf_batched on a copy, then getrs_batched.
        Raises MPFError naming the first singular matrix."""
        LU, ipiv, info = self.getrf_batched(A)
        bad = self.torch.nonzero(info)
        if bad.numel():
            b = int(bad[0])
            raise MPFError(f"solve_batched: matrix {b} of the batch is singular (zero pivot {int(info[b])})")
        return self.getrs_batched(LU, ipiv, B, trans=trans)

    # ---- the expert layer for those batches (include/mpf_c.h: mpf_lange_batched, mpf_gecon_batched, mpf_residual_batched, mpf_gerfs_batched) --
    def lange_batched(self, A, norm="1"):
        """mpf_lange_batched: the '1' / 'O', 'I' or 'M' norm of every matrix of the (batch, n, n) tensor A, n <= 128, as a float64
        (batch,) device tensor; sums are the header's halving tree, a NaN in a matrix gives NaN for it."""
        return self._lange_batched(A, norm, "lange_batched")

    def _lange_batched(self, A, norm, entry):
        self._bind()
        t = self.torch
        assert A.dim() == 3 and A.shape[1] == A.shape[2], "A: (batch, n, n)"
        batch, n = A.shape[0], A.shape[1]
        Am, lda, sa = self._batch_arg(A, entry, False, copy=False)
        out = t.zeros(batch, dtype=t.float64, device=self.device)
        self._check(getattr(self.L, "mpf_" + entry)(self.h, norm.encode()[:1], _ptr(Am), lda, sa, n, batch, _ptr(out)), "mpf_" + entry)
        return out

    def gecon_batched(self, LU, anorm, norm="1", want_ainvnm=False):
        """mpf_gecon_batched: rcond[b] = (1 / ||(L U)^-1||) / anorm[b] from getrf_batched's factors, the norm of the inverse computed
        exactly (not dgecon's estimate).  anorm: a float64 (batch,) device tensor (lange_batched of the matrices, same norm).
        Returns rcond, or (rcond, ainvnm) with want_ainvnm; rcond is 0 for anorm 0, a zero on U's diagonal or a non-finite inverse."""
        return self._gecon_batched(LU, anorm, norm, want_ainvnm, "gecon_batched")

    def _gecon_batched(self, LU, anorm, norm, want_ainvnm, entry):
        self._bind()
        t = self.torch
        assert LU.dim() == 3 and LU.shape[1] == LU.shape[2], "LU: (batch, n, n)"
        batch, n = LU.shape[0], LU.shape[1]
        LUm, ldlu, slu = self._batch_arg(LU, entry, False, copy=False)
        assert anorm.dtype == t.float64 and anorm.is_cuda and anorm.shape == (batch,)
        anorm = anorm.contiguous()
        rcond = t.zeros(batch, dtype=t.float64, device=self.device)
        ainv = t.zeros(batch, dtype=t.float64, device=self.device) if want_ainvnm else None
        rc = getattr(self.L, "mpf_" + entry)(self.h, norm.encode()[:1], _ptr(LUm), ldlu, slu, n, batch, _ptr(anorm), _ptr(rcond),
                                             _ptr(ainv) if want_ainvnm else None)
        self._check(rc, "mpf_" + entry)
        return (rcond, ainv) if want_ainvnm else rcond

    def residual_batched(self, A, X, B, trans=False, want_w=True):
        """mpf_residual_batched: (R, W) with R[b] = B[b] - op(A[b]) X[b] and W[b] = |B[b]| + |op(A[b])| |X[b]| (W None without
        want_w), new column-major tensors; X and B are (batch, n, nrhs), or (batch, n) for one column each."""
        return self._residual_batched(A, X, B, trans, want_w, "residual_batched")

    def _residual_batched(self, A, X, B, trans, want_w, entry):
        self._bind()
        if B.dim() == 2:
            R, W = self._residual_batched(A, X.unsqueeze(2), B.unsqueeze(2), trans, want_w, entry)
            return R.squeeze(2), (W.squeeze(2) if want_w else None)
        assert A.dim() == 3 and A.shape[1] == A.shape[2] and B.dim() == 3 and B.shape[:2] == A.shape[:2] and X.shape == B.shape, \
            "A: (batch, n, n), X and B: (batch, n, nrhs)"
        batch, n, nrhs = B.shape
        Am, lda, sa = self._batch_arg(A, entry, False, copy=False)
        Xm, ldx, sx = self._batch_arg(X, entry, False, copy=False)
        Bm, ldb, sb = self._batch_arg(B, entry, False, copy=False)
        R = self.colmajor_batch(batch, n, nrhs)
        W = self.colmajor_batch(batch, n, nrhs) if want_w else None
        ldr, sr = self._batch_layout(R)
        rc = getattr(self.L, "mpf_" + entry)(self.h, int(bool(trans)), _ptr(Am), lda, sa, n, batch, nrhs, _ptr(Xm), ldx, sx, _ptr(Bm), ldb,
                                             sb, _ptr(R), ldr, sr, _ptr(W) if want_w else None)
        self._check(rc, "mpf_" + entry)
        return R, W

    def gerfs_batched(self, A, LU, ipiv, B, X, trans=False, itmax=0, overwrite=False, want_ferr=True):
        """mpf_gerfs_batched: dgerfs per matrix and column with getrf_batched's factors.  X holds a solution (getrs_batched's) and
        is refined: a new column-major tensor, or X itself with overwrite=True (column-major matrices).  Returns (X, ferr, berr,
        iters): float64 / int32 (batch, nrhs) device tensors (ferr None without want_ferr).  ferr bounds max_i |x_i - xtrue_i| /
        max_i |x_i| with the exact norm where dgerfs estimates it."""
        return self._gerfs_batched(A, LU, ipiv, B, X, trans, itmax, overwrite, want_ferr, "gerfs_batched")

    def _gerfs_batched(self, A, LU, ipiv, B, X, trans, itmax, overwrite, want_ferr, entry):
        self._bind()
        t = self.torch
        if B.dim() == 2:
            Xr, ferr, berr, its = self._gerfs_batched(A, LU, ipiv, B.unsqueeze(2), X.unsqueeze(2), trans, itmax, overwrite, want_ferr, entry)
            return Xr.squeeze(2), ferr, berr, its
        assert A.dim() == 3 and A.shape[1] == A.shape[2] and B.dim() == 3 and B.shape[:2] == A.shape[:2] and X.shape == B.shape, \
            "A: (batch, n, n), B and X: (batch, n, nrhs)"
        assert LU.shape == A.shape
        nrhs = B.shape[2]
        Am, lda, sa = self._batch_arg(A, entry, False, copy=False)
        LUm, ldlu, slu, ipiv, sp, batch, n = self._batch_factors(LU, ipiv, entry)
        Bm, ldb, sb = self._batch_arg(B, entry, False, copy=False)
        Xm, ldx, sx = self._batch_arg(X, entry, overwrite)
        ferr = t.zeros((batch, nrhs), dtype=t.float64, device=self.device) if want_ferr else None
        berr = t.zeros((batch, nrhs), dtype=t.float64, device=self.device)
        its = t.zeros((batch, nrhs), dtype=t.int32, device=self.device)
        rc = getattr(self.L, "mpf_" + entry)(self.h, int(bool(trans)), _ptr(Am), lda, sa, _ptr(LUm), ldlu, slu, n, batch, _ptr(ipiv), sp,
                                             nrhs, _ptr(Bm), ldb, sb, _ptr(Xm), ldx, sx, int(itmax), _ptr(ferr) if want_ferr else None,
                                             _ptr(berr), _ptr(its))
        self._check(rc, "mpf_" + entry)
        return Xm, ferr, berr, its

    def cond_batched(self, A, norm="1"):
        """rcond of every matrix of the (batch, n, n) tensor A, n <= 128: getrf_batched on a copy, lange_batched, gecon_batched.  0
        for a singular matrix; nothing is read back."""
        return self._cond_batched(A, norm, "")

    def _cond_batched(self, A, norm, suffix):
        LU, _, _ = getattr(self, "getrf_batched" + suffix)(A)
        return getattr(self, "gecon_batched" + suffix)(LU, getattr(self, "lange_batched" + suffix)(A, norm), norm)

    def solvex_batched(self, A, B, trans=False, itmax=0):
        """dgesvx's shape without equilibration (gesvx_batched adds it) for a batch, n <= 128: getrf_batched on a copy, lange_batched / gecon_batched (the
        '1' norm, or 'I' with trans), getrs_batched, gerfs_batched.  Returns (X, rcond, ferr, berr, info), all on the device; never
        raises on a singular matrix: info[b] is its first zero pivot and rcond[b] is 0 (its X, ferr and berr are not meaningful)."""
        return self._solvex_batched(A, B, trans, itmax, "")

    def _solvex_batched(self, A, B, trans, itmax, suffix):
        norm = "I" if trans else "1"
        LU, ipiv, info = getattr(self, "getrf_batched" + suffix)(A)
        rcond = getattr(self, "gecon_batched" + suffix)(LU, getattr(self, "lange_batched" + suffix)(A, norm), norm)
        X = getattr(self, "getrs_batched" + suffix)(LU, ipiv, B, trans=trans)
        X, ferr, berr, _ = getattr(self, "gerfs_batched" + suffix)(A, LU, ipiv, B, X, trans=trans, itmax=itmax, overwrite=True)
        return X, rcond, ferr, berr, info

    # ---- the same for one order up to 1024 (include/mpf_c.h: mpf_getrf_batched_blocked, mpf_getrs_batched_blocked) ------------------------
    def getrf_batched_blocked(self, A, fused=False, overwrite=False, ipiv=None, info=None):
        """mpf_getrf_batched_blocked: getrf_batched for n <= 1024 -- the same arguments, layout handling, results and bits (a
        right-looking blocked LU, three launches per panel step for the whole batch).  Options batched_blocked_min_n (smaller n go to
        getrf_batched's kernels) and batched_blocked_nb (panel width) change no bit."""
        return self._getrf_batched(A, fused, overwrite, ipiv, info, "getrf_batched_blocked")

    def getrs_batched_blocked(self, LU, ipiv, B, trans=False, overwrite=False):
        """mpf_getrs_batched_blocked: getrs_batched for n <= 1024 with the factors of getrf_batched_blocked."""
        return self._getrs_batched(LU, ipiv, B, trans, overwrite, "getrs_batched_blocked")

    def solve_batched_blocked(self, A, B, trans=False):
        """X[b] = A[b]^-1 B[b] (or A[b]^-T B[b]) for a (batch, n, n) tensor A, n <= 1024: getrf_batched_blocked on a copy, then
        getrs_batched_blocked.  Raises MPFError naming the first singular matrix."""
        LU, ipiv, info = self.getrf_batched_blocked(A)
        bad = self.torch.nonzero(info)
        if bad.numel():
            b = int(bad[0])
            raise MPFError(f"solve_batched_blocked: matrix {b} of the batch is singular (zero pivot {int(info[b])})")
        return self.getrs_batched_blocked(LU, ipiv, B, trans=trans)

    def _batch_factors(self, LU, ipiv, what):
        """(LU, ldlu, strideLU, ipiv, strideP, batch, n) of a batch of factors as the library reads them (LU is copied only when its
        matrices are not column-major as they stand)."""
        t = self.torch
        assert LU.dim() == 3 and LU.shape[1] == LU.shape[2], "LU: (batch, n, n)"
        batch, n = LU.shape[0], LU.shape[1]
        LUm, ldlu, slu = self._batch_arg(LU, what, False, copy=False)
        assert ipiv.dtype == t.int32 and ipiv.is_cuda and ipiv.shape == (batch, n)
        if n > 1 and ipiv.stride(1) != 1:
            ipiv = ipiv.contiguous()
        return LUm, ldlu, slu, ipiv, (ipiv.stride(0) if batch > 1 else max(n, 1)), batch, n

    def getri_batched(self, LU, ipiv, out=None, info=None):
        """mpf_getri_batched: inv(A[b]) from the factors of getrf_batched, out of place, bit for bit getrs_batched on an identity.
        out: a (batch, n, n) tensor of column-major matrices to receive the inverses (colmajor_batch; a new one when None); info:
        an int32 (batch,) device tensor.  Returns (inv, info): info[b] = i + 1 when u_ii is the first zero on U[b]'s diagonal --
        out[b] is then untouched -- else 0."""
        return self._getri_batched(LU, ipiv, out, info, "getri_batched")

    def _getri_batched(self, LU, ipiv, out, info, entry):
        self._bind()
        t = self.torch
        LUm, ldlu, slu, ipiv, sp, batch, n = self._batch_factors(LU, ipiv, entry)
        if out is None:
            out = self.colmajor_batch(batch, n, n)
        assert out.dim() == 3 and out.shape == (batch, n, n) and out.dtype == t.float64 and out.is_cuda
        lay = self._batch_layout(out)
        if lay is None:
            raise MPFError(f"{entry}: out needs column-major matrices (MPFContext.colmajor_batch)")
        if info is None:
            info = t.zeros(batch, dtype=t.int32, device=self.device)
        assert info.dtype == t.int32 and info.is_cuda and info.shape == (batch,) and info.is_contiguous()
        rc = getattr(self.L, "mpf_" + entry)(self.h, _ptr(LUm), ldlu, slu, n, batch, _ptr(ipiv), sp, _ptr(out), lay[0], lay[1], _ptr(info))
        self._check(rc, "mpf_" + entry)
        return out, info

    def getdet_batched(self, LU, ipiv):
        """mpf_getdet_batched: det(A[b]) = mant[b] * 2**expo[b] from the factors of getrf_batched, |mant| in [0.5, 1) or 0.  Returns
        (mant float64 (batch,), expo int32 (batch,)) on the device; (0, 0) for a singular U[b], (nan, 0) for a non-finite one."""
        return self._getdet_batched(LU, ipiv, "getdet_batched")

    def _getdet_batched(self, LU, ipiv, entry):
        self._bind()
        t = self.torch
        LUm, ldlu, slu, ipiv, sp, batch, n = self._batch_factors(LU, ipiv, entry)
        mant = t.full((batch,), 0.5, dtype=t.float64, device=self.device)     # n == 0: the empty product, mpf_getdet's (0.5, 1)
        expo = t.ones(batch, dtype=t.int32, device=self.device)
        rc = getattr(self.L, "mpf_" + entry)(self.h, _ptr(LUm), ldlu, slu, n, batch, _ptr(ipiv), sp, _ptr(mant), _ptr(expo))
        self._check(rc, "mpf_" + entry)
        return mant, expo

    def inv_batched(self, A):
        """inv(A[b]) for a (batch, n, n) tensor A, n <= 128: getrf_batched on a copy, then getri_batched.  Raises MPFError naming the
        first singular matrix."""
        return self._inv_batched(A, "")

    def _inv_batched(self, A, suffix):
        LU, ipiv, info = getattr(self, "getrf_batched" + suffix)(A)
        X, info2 = getattr(self, "getri_batched" + suffix)(LU, ipiv)
        for inf in (info, info2):
            bad = self.torch.nonzero(inf)
            if bad.numel():
                b = int(bad[0])
                raise MPFError(f"inv_batched{suffix}: matrix {b} of the batch is singular (zero pivot {int(inf[b])})")
        return X

    def slogdet_batched(self, A_or_LU, ipiv=None):
        """(sign, log|det A[b]|) as torch.linalg.slogdet returns them, device tensors of (batch,): from getdet_batched,
        log|mant| + expo ln 2 -- one rounded logarithm per matrix.  (0, -inf) for a zero determinant, (nan, nan) for a non-finite one.
        ipiv=None: A_or_LU holds the matrices, and a copy is factored first; otherwise it holds getrf_batched's factors."""
        return self._slogdet_batched(A_or_LU, ipiv, "")

    def _slogdet_batched(self, A_or_LU, ipiv, suffix):
        import math
        t = self.torch
        if ipiv is None:
            A_or_LU, ipiv, _ = getattr(self, "getrf_batched" + suffix)(A_or_LU)
        mant, expo = getattr(self, "getdet_batched" + suffix)(A_or_LU, ipiv)
        sign = t.where(t.isnan(mant), mant, t.sign(mant))         # (sign(0) is 0; sign(nan) is not nan on every backend)
        return sign, t.log(t.abs(mant)) + expo.to(t.float64) * math.log(2.0)  # (expo is 0 beside log(0) = -inf and log(nan) = nan)

    # ---- the same for one order up to 1024 (include/mpf_c.h: mpf_getri_batched_blocked, mpf_getdet_batched_blocked) -----------------------
    def getri_batched_blocked(self, LU, ipiv, out=None, info=None):
        """mpf_getri_batched_blocked: getri_batched for n <= 1024 with the factors of getrf_batched_blocked -- the same arguments,
        results and bits (bit for bit getrs_batched_blocked on an identity that is never formed).  Options batched_blocked_min_n
        (smaller n go to getri_batched's kernels) and batched_blocked_inv_ct (columns per workgroup) change no bit."""
        return self._getri_batched(LU, ipiv, out, info, "getri_batched_blocked")

    def getdet_batched_blocked(self, LU, ipiv):
        """mpf_getdet_batched_blocked: getdet_batched for n <= 1024 (mpf_getdet's chunks of 256 per matrix)."""
        return self._getdet_batched(LU, ipiv, "getdet_batched_blocked")

    def inv_batched_blocked(self, A):
        """inv(A[b]) for a (batch, n, n) tensor A, n <= 1024: getrf_batched_blocked on a copy, then getri_batched_blocked.  Raises
        MPFError naming the first singular matrix."""
        return self._inv_batched(A, "_blocked")

    def slogdet_batched_blocked(self, A_or_LU, ipiv=None):
        """slogdet_batched for n <= 1024: from getdet_batched_blocked (and getrf_batched_blocked when ipiv is None)."""
        return self._slogdet_batched(A_or_LU, ipiv, "_blocked")

    # ---- the expert layer for one order up to 1024 (include/mpf_c.h: mpf_lange_batched_blocked, mpf_gecon_batched_blocked, ...) ---------
    def lange_batched_blocked(self, A, norm="1"):
        """mpf_lange_batched_blocked: lange_batched for n <= 1024 -- the same arguments, results and bits (the tree padded to 1024)."""
        return self._lange_batched(A, norm, "lange_batched_blocked")

    def gecon_batched_blocked(self, LU, anorm, norm="1", want_ainvnm=False):
        """mpf_gecon_batched_blocked: gecon_batched for n <= 1024 with the factors of getrf_batched_blocked; the norm of the inverse is
        exact, its chains are reduced on the fly and never stored (no n x n workspace)."""
        return self._gecon_batched(LU, anorm, norm, want_ainvnm, "gecon_batched_blocked")

    def residual_batched_blocked(self, A, X, B, trans=False, want_w=True):
        """mpf_residual_batched_blocked: residual_batched for n <= 1024."""
        return self._residual_batched(A, X, B, trans, want_w, "residual_batched_blocked")

    def gerfs_batched_blocked(self, A, LU, ipiv, B, X, trans=False, itmax=0, overwrite=False, want_ferr=True):
        """mpf_gerfs_batched_blocked: gerfs_batched for n <= 1024 with the factors of getrf_batched_blocked and a solution from
        getrs_batched_blocked; the same rule, outputs and, for n <= 128, bits."""
        return self._gerfs_batched(A, LU, ipiv, B, X, trans, itmax, overwrite, want_ferr, "gerfs_batched_blocked")

    def cond_batched_blocked(self, A, norm="1"):
        """rcond of every matrix of the (batch, n, n) tensor A, n <= 1024: getrf_batched_blocked on a copy, lange_batched_blocked,
        gecon_batched_blocked.  0 for a singular matrix; nothing is read back."""
        return self._cond_batched(A, norm, "_blocked")

    def solvex_batched_blocked(self, A, B, trans=False, itmax=0):
        """solvex_batched for n <= 1024 from the blocked entries (gesvx_batched_blocked adds equilibration).  Returns (X, rcond, ferr, berr, info), all on the device; never
        raises on a singular matrix: info[b] is its first zero pivot and rcond[b] is 0."""
        return self._solvex_batched(A, B, trans, itmax, "_blocked")


    # ---- equilibration of those batches (include/mpf_c.h: mpf_geequ_batched, mpf_laqge_batched, mpf_lascl2_batched) --------------------------
    def geequ_batched(self, A):
        """mpf_geequ_batched: mpf_geequ's power-of-two row and column factors of every matrix of the (batch, n, n) tensor A, n <= 128.
        Returns (r, c, rowcnd, colcnd, amax, info): float64 (batch, n) and (batch,) device tensors and int32 info -- 0, i + 1 for the
        first zero row, n + j + 1 for the first zero scaled column, 2 n + 1 for a NaN or Inf in the matrix (what the contract leaves
        unset stays zero here)."""
        return self._geequ_batched(A, "geequ_batched")

    def _geequ_batched(self, A, entry):
        self._bind()
        t = self.torch
        assert A.dim() == 3 and A.shape[1] == A.shape[2], "A: (batch, n, n)"
        batch, n = A.shape[0], A.shape[1]
        Am, lda, sa = self._batch_arg(A, entry, False, copy=False)
        r, c = (t.zeros((batch, n), dtype=t.float64, device=self.device) for _ in range(2))
        rowcnd, colcnd, amax = (t.zeros(batch, dtype=t.float64, device=self.device) for _ in range(3))
        info = t.zeros(batch, dtype=t.int32, device=self.device)
        rc = getattr(self.L, "mpf_" + entry)(self.h, _ptr(Am), lda, sa, n, batch, _ptr(r), _ptr(c), _ptr(rowcnd), _ptr(colcnd), _ptr(amax),
                                             _ptr(info))
        self._check(rc, "mpf_" + entry)
        return r, c, rowcnd, colcnd, amax, info

    def laqge_batched(self, A, r, c, rowcnd, colcnd, amax, info, rule=1, overwrite=False):
        """mpf_laqge_batched: As[b] = Dr A[b] Dc with geequ_batched's results, by rule 0 (never), 1 (dlaqge's rule as mpf_gesvx
        states it) or 2 (always both), decided per matrix on the device; a matrix with info != 0 is never scaled.  Returns (As,
        equed, spread): a column-major batch (A itself with overwrite=True), int32 (batch,) with 0 none / 1 rows / 2 columns / 3
        both, and float64 (batch, 2) with max r / min r and max c / min c of the sides that were scaled (1 otherwise).  Without
        overwrite As is a new tensor of A's column-major layout (a packed one when A's had to be copied), formed out of place."""
        return self._laqge_batched(A, r, c, rowcnd, colcnd, amax, info, rule, overwrite, "laqge_batched")

    def _laqge_batched(self, A, r, c, rowcnd, colcnd, amax, info, rule, overwrite, entry):
        self._bind()
        t = self.torch
        assert A.dim() == 3 and A.shape[1] == A.shape[2], "A: (batch, n, n)"
        batch, n = A.shape[0], A.shape[1]
        Am, lda, sa = self._batch_arg(A, entry, overwrite, copy=False)
        As = Am if overwrite else t.empty_strided(Am.shape, Am.stride(), dtype=t.float64, device=self.device)
        for v, shape in ((r, (batch, n)), (c, (batch, n)), (rowcnd, (batch,)), (colcnd, (batch,)), (amax, (batch,))):
            assert v.dtype == t.float64 and v.is_cuda and v.shape == shape and v.is_contiguous()
        assert info.dtype == t.int32 and info.is_cuda and info.shape == (batch,) and info.is_contiguous()
        equed = t.zeros(batch, dtype=t.int32, device=self.device)
        spread = t.ones((batch, 2), dtype=t.float64, device=self.device)
        rc = getattr(self.L, "mpf_" + entry)(self.h, int(rule), _ptr(Am), lda, sa, n, batch, _ptr(r), _ptr(c), _ptr(rowcnd), _ptr(colcnd),
                                             _ptr(amax), _ptr(info), _ptr(As), _ptr(equed), _ptr(spread))
        self._check(rc, "mpf_" + entry)
        return As, equed, spread

    def lascl2_batched(self, s, V, equed=None, bit=0, overwrite=False):
        """mpf_lascl2_batched: V[b] = diag(s[b]) V[b] for the matrices with equed[b] & bit (all of them when equed is None); V is
        (batch, n, nrhs) or (batch, n), s float64 (batch, n).  Returns a new column-major tensor, or V itself with overwrite=True."""
        return self._lascl2_batched(s, V, equed, bit, overwrite, "lascl2_batched")

    def _lascl2_batched(self, s, V, equed, bit, overwrite, entry):
        self._bind()
        t = self.torch
        if V.dim() == 2:
            return self._lascl2_batched(s, V.unsqueeze(2), equed, bit, overwrite, entry).squeeze(2)
        assert V.dim() == 3 and s.dtype == t.float64 and s.is_cuda and s.shape == V.shape[:2] and s.is_contiguous(), "s: (batch, n), V: (batch, n, nrhs)"
        batch, n, nrhs = V.shape
        Vm, ldv, sv = self._batch_arg(V, entry, overwrite)
        if equed is not None:
            assert equed.dtype == t.int32 and equed.is_cuda and equed.shape == (batch,) and equed.is_contiguous()
        rc = getattr(self.L, "mpf_" + entry)(self.h, _ptr(s), n, batch, nrhs, _ptr(Vm), ldv, sv, _ptr(equed) if equed is not None else None,
                                             int(bit))
        self._check(rc, "mpf_" + entry)
        return Vm

    def gesvx_batched(self, A, B, trans=False, itmax=0, equilibrate=1):
        """dgesvx for a batch, n <= 128, composed of the batched entries in dgesvx's order: geequ_batched, laqge_batched into a copy
        (equilibrate: its rule -- 0 never, 1 dlaqge's, 2 always), getrf_batched, lange_batched / gecon_batched of the equilibrated
        matrix, lascl2_batched on a copy of B, getrs_batched, gerfs_batched on the equilibrated system, lascl2_batched on X, and ferr
        times the spread of the scaling on X's side.  Returns (X, rcond, ferr, berr, info, equed, r, c), all on the device; rcond and
        info are the equilibrated matrix's; never raises on a singular or flagged matrix.  equilibrate=0: solvex_batched's bits."""
        return self._gesvx_batched(A, B, trans, itmax, equilibrate, "")

    def _gesvx_batched(self, A, B, trans, itmax, equilibrate, suffix):
        f = lambda name: getattr(self, name + "_batched" + suffix)   # noqa: E731
        norm = "I" if trans else "1"
        r, c, rowcnd, colcnd, amax, einfo = f("geequ")(A)
        As, equed, spread = f("laqge")(A, r, c, rowcnd, colcnd, amax, einfo, rule=equilibrate)
        LU, ipiv, info = f("getrf")(As)
        rcond = f("gecon")(LU, f("lange")(As, norm), norm)
        Bs = f("lascl2")(c if trans else r, B, equed, 2 if trans else 1)
        X = f("getrs")(LU, ipiv, Bs, trans=trans)
        X, ferr, berr, _ = f("gerfs")(As, LU, ipiv, Bs, X, trans=trans, itmax=itmax, overwrite=True)
        X = f("lascl2")(r if trans else c, X, equed, 1 if trans else 2, overwrite=True)
        ferr = ferr * spread[:, 0 if trans else 1].unsqueeze(1)
        return X, rcond, ferr, berr, info, equed, r, c

    def geequ_batched_blocked(self, A):
        """mpf_geequ_batched_blocked: geequ_batched for n <= 1024 -- the same arguments, results and bits (a matrix spread over
        several workgroups, four launches)."""
        return self._geequ_batched(A, "geequ_batched_blocked")

    def laqge_batched_blocked(self, A, r, c, rowcnd, colcnd, amax, info, rule=1, overwrite=False):
        """mpf_laqge_batched_blocked: laqge_batched for n <= 1024."""
        return self._laqge_batched(A, r, c, rowcnd, colcnd, amax, info, rule, overwrite, "laqge_batched_blocked")

    def lascl2_batched_blocked(self, s, V, equed=None, bit=0, overwrite=False):
        """mpf_lascl2_batched_blocked: lascl2_batched for n <= 1024."""
        return self._lascl2_batched(s, V, equed, bit, overwrite, "lascl2_batched_blocked")

    def gesvx_batched_blocked(self, A, B, trans=False, itmax=0, equilibrate=1):
        """gesvx_batched for n <= 1024 from the blocked entries; equilibrate=0: solvex_batched_blocked's bits."""
        return self._gesvx_batched(A, B, trans, itmax, equilibrate, "_blocked")

    # ---- the same for matrices of different orders (include/mpf_c.h: mpf_vbatch_create, mpf_getrf_vbatched, ...) --------------------------
    def vbatch(self, n, ld=None, off=None):
        """mpf_vbatch_create: the descriptor of a batch of matrices of orders n[b] <= 128 inside one allocation -- matrix b column-major
        at element offset off[b] with leading dimension ld[b] (ld=None: n[b]; off=None: packed).  Returns a VBatch."""
        return VBatch(self, n, ld, off)

    def vbatch_blocked(self, n, ld=None, off=None):
        """mpf_vbatch_create_blocked: vbatch for orders n[b] <= 1024 -- the same arguments and the same VBatch.  Every matrix's results
        are bit for bit those of the *_batched_blocked methods on that matrix alone.  Option batched_blocked_min_n (which matrices of
        order <= 128 take the small kernels) is read here, once."""
        return VBatch(self, n, ld, off, blocked=True)


class VBatch:
    """A variable-size batch (mpf_vbatch): `batch` matrices of orders n[b] in one flat float64 device tensor of `extent` elements; the
    pivots of all matrices in one int32 tensor of total_n, matrix b's at offv[b]; right-hand sides as one tall (total_n, nrhs)
    column-major matrix.  Attributes: batch, total_n, extent, n, ld, off, offv (numpy).  Every method is asynchronous on the context's
    stream except solve / inv, which read info back."""

    def __init__(self, ctx, n, ld=None, off=None, blocked=False):
        import weakref
        import numpy as np
        ctx._bind()
        self.ctx, self.h = ctx, C.c_void_p()
        self.n = np.ascontiguousarray(n, dtype=np.int32).reshape(-1)
        batch = self.n.size
        args = []
        for name, a in (("ld", ld), ("off", off)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
                assert a.size == batch, f"{name}: one entry per matrix"
            args.append(a)
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None and a.size else None   # noqa: E731
        create = "mpf_vbatch_create_blocked" if blocked else "mpf_vbatch_create"
        rc = getattr(ctx.L, create)(ctx.h, batch, ptr(self.n), ptr(args[0]), ptr(args[1]), C.byref(self.h))
        ctx._check(rc, create)
        b, tn, ext = C.c_int64(), C.c_int64(), C.c_int64()
        ctx.L.mpf_vbatch_info(self.h, C.byref(b), C.byref(tn), C.byref(ext))
        self.batch, self.total_n, self.extent = b.value, tn.value, ext.value
        self.off, self.offv = np.zeros(batch, dtype=np.int64), np.zeros(batch, dtype=np.int64)
        ctx.L.mpf_vbatch_offsets(self.h, ptr(self.off), ptr(self.offv))
        self.ld = args[0] if args[0] is not None else self.n.astype(np.int64)
        if not hasattr(ctx, "_vbatches"):
            ctx._vbatches = weakref.WeakSet()
        ctx._vbatches.add(self)

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.L.mpf_vbatch_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- layout helpers -------------------------------------------------------------------------------------------------------------
    def pack(self, mats, fill=0.0):
        """A flat float64 device tensor of `extent` elements holding the matrices (numpy arrays or tensors, n[b] x n[b]) in this layout;
        the elements between them are `fill`."""
        import numpy as np
        assert len(mats) == self.batch
        flat = np.full(self.extent, fill, dtype=np.float64)
        for b, M in enumerate(mats):
            nb, l, o = int(self.n[b]), int(self.ld[b]), int(self.off[b])
            if nb == 0:
                continue
            M = M.cpu().numpy() if hasattr(M, "cpu") else np.asarray(M, dtype=np.float64)
            assert M.shape == (nb, nb), f"matrix {b}: ({nb}, {nb})"
            np.lib.stride_tricks.as_strided(flat[o:], (nb, nb), (8, 8 * l))[...] = M
        return self.ctx.torch.from_numpy(flat).to(self.ctx.device)

    def unpack(self, flat):
        """The matrices of a flat tensor in this layout: a list of n[b] x n[b] column-major views of `flat`."""
        assert flat.dim() == 1 and flat.numel() >= self.extent
        return [flat.as_strided((int(nb), int(nb)), (1, int(l)), int(o)) if nb else flat.new_zeros((0, 0))
                for nb, l, o in zip(self.n, self.ld, self.off)]

    def _flat(self, x, what):
        t = self.ctx.torch
        assert x.dim() == 1 and x.dtype == t.float64 and x.is_cuda and x.is_contiguous() and x.numel() >= self.extent, \
            f"{what}: a flat float64 device tensor of at least extent = {self.extent} elements"
        return x

    def _pivots(self, ipiv):
        t = self.ctx.torch
        assert ipiv.dim() == 1 and ipiv.dtype == t.int32 and ipiv.is_cuda and ipiv.is_contiguous() and ipiv.numel() >= self.total_n
        return ipiv

    def _info(self, info):
        t = self.ctx.torch
        if info is None:
            info = t.zeros(self.batch, dtype=t.int32, device=self.ctx.device)
        assert info.dtype == t.int32 and info.is_cuda and info.shape == (self.batch,) and info.is_contiguous()
        return info

    # ---- the four operations ----------------------------------------------------------------------------------------------------------
    def getrf(self, A, fused=False, overwrite=False, ipiv=None, info=None):
        """mpf_getrf_vbatched: (LU, ipiv, info) -- LU flat in this layout (A itself with overwrite=True, else a copy), ipiv int32
        (total_n,), 1-based, matrix b's at offv[b]; info int32 (batch,): the first zero pivot of each matrix or 0."""
        ctx, t = self.ctx, self.ctx.torch
        ctx._bind()
        LU = self._flat(A, "getrf") if overwrite else self._flat(A, "getrf").clone()
        if ipiv is None:
            ipiv = t.zeros(self.total_n, dtype=t.int32, device=ctx.device)
        info = self._info(info)
        rc = ctx.L.mpf_getrf_vbatched(ctx.h, self.h, _ptr(LU), _ptr(self._pivots(ipiv)), _ptr(info), int(bool(fused)))
        ctx._check(rc, "mpf_getrf_vbatched")
        return LU, ipiv, info

    def getrs(self, LU, ipiv, B, trans=False, overwrite=False):
        """mpf_getrs_vbatched: the block-diagonal solve X = D^-1 B (or D^-T B); B is (total_n,) or a column-major (total_n, nrhs)
        tensor (MPFContext.colmajor).  Returns a new X unless overwrite=True (B itself, solved in place)."""
        ctx = self.ctx
        ctx._bind()
        if B.dim() == 1:
            assert B.is_contiguous()
            return self.getrs(LU, ipiv, B.unsqueeze(1), trans, overwrite).squeeze(1)
        assert B.dim() == 2 and B.shape[0] == self.total_n and B.dtype == ctx.torch.float64 and B.is_cuda, "B: (total_n, nrhs) float64"
        nrhs = B.shape[1]
        colmajor = (B.shape[0] <= 1 or B.stride(0) == 1) and (nrhs <= 1 or B.stride(1) >= max(self.total_n, 1))
        if overwrite:
            if not colmajor:
                raise MPFError("getrs: overwrite=True needs a column-major B (MPFContext.colmajor); this tensor would be copied")
            X = B
        else:
            X = ctx.colmajor(self.total_n, nrhs)
            X.copy_(B)
        ldb = X.stride(1) if nrhs > 1 else max(self.total_n, 1)
        rc = ctx.L.mpf_getrs_vbatched(ctx.h, self.h, int(bool(trans)), _ptr(self._flat(LU, "getrs")), _ptr(self._pivots(ipiv)), nrhs,
                                      _ptr(X), ldb)
        ctx._check(rc, "mpf_getrs_vbatched")
        return X

    def getri(self, LU, ipiv, out=None, info=None):
        """mpf_getri_vbatched: (inv, info) -- the inverses flat in this layout, out of place (out: a flat tensor to receive them; a
        zero-filled one when None); info[b] = i + 1 when u_ii is the first zero on U[b]'s diagonal -- inv[b] is then untouched."""
        ctx, t = self.ctx, self.ctx.torch
        ctx._bind()
        if out is None:
            out = t.zeros(max(self.extent, 1), dtype=t.float64, device=ctx.device)
        info = self._info(info)
        rc = ctx.L.mpf_getri_vbatched(ctx.h, self.h, _ptr(self._flat(LU, "getri")), _ptr(self._pivots(ipiv)), _ptr(self._flat(out, "getri out")),
                                      _ptr(info))
        ctx._check(rc, "mpf_getri_vbatched")
        return out, info

    def getdet(self, LU, ipiv):
        """mpf_getdet_vbatched: (mant float64 (batch,), expo int32 (batch,)) on the device, det(A[b]) = mant[b] * 2**expo[b]."""
        ctx, t = self.ctx, self.ctx.torch
        ctx._bind()
        mant = t.zeros(self.batch, dtype=t.float64, device=ctx.device)
        expo = t.zeros(self.batch, dtype=t.int32, device=ctx.device)
        rc = ctx.L.mpf_getdet_vbatched(ctx.h, self.h, _ptr(self._flat(LU, "getdet")), _ptr(self._pivots(ipiv)), _ptr(mant), _ptr(expo))
        ctx._check(rc, "mpf_getdet_vbatched")
        return mant, expo

    def _raise_singular(self, what, infos):
        for inf in infos:
            bad = self.ctx.torch.nonzero(inf)
            if bad.numel():
                b = int(bad[0])
                raise MPFError(f"{what}: matrix {b} of the batch is singular (zero pivot {int(inf[b])})")

    def solve(self, A, B, trans=False):
        """X = D^-1 B (or D^-T B) for the matrices in the flat tensor A: getrf on a copy, then getrs.  Raises MPFError naming the first
        singular matrix."""
        LU, ipiv, info = self.getrf(A)
        self._raise_singular("solve_batched", (info,))
        return self.getrs(LU, ipiv, B, trans=trans)

    def inv(self, A):
        """The inverses of the matrices in the flat tensor A, flat in this layout: getrf on a copy, then getri.  Raises MPFError naming
        the first singular matrix."""
        LU, ipiv, info = self.getrf(A)
        X, info2 = self.getri(LU, ipiv)
        self._raise_singular("inv_batched", (info, info2))
        return X

    def slogdet(self, A_or_LU, ipiv=None):
        """(sign, log|det A[b]|) as MPFContext.slogdet_batched returns them, device tensors of (batch,).  ipiv=None: A_or_LU holds the
        matrices, and a copy is factored first; otherwise it holds getrf's factors."""
        import math
        t = self.ctx.torch
        if ipiv is None:
            A_or_LU, ipiv, _ = self.getrf(A_or_LU)
        mant, expo = self.getdet(A_or_LU, ipiv)
        sign = t.where(t.isnan(mant), mant, t.sign(mant))
        return sign, t.log(t.abs(mant)) + expo.to(t.float64) * math.log(2.0)

    # ---- the expert layer (include/mpf_c.h: mpf_lange_vbatched, mpf_gecon_vbatched, mpf_residual_vbatched, mpf_gerfs_vbatched) --------------
    # Every result of matrix b is bit for bit what the *_batched_blocked method returns for that matrix alone (for n[b] <= 128 also what
    # the small *_batched method returns), on a descriptor of either kind.
    def _tall(self, M, what, overwrite, copy=True):
        """(tensor, ld) of a tall (total_n, nrhs) column-major operand: M itself when it is column-major, else a column-major copy
        (refused with overwrite=True)."""
        ctx = self.ctx
        assert M.dim() == 2 and M.shape[0] == self.total_n and M.dtype == ctx.torch.float64 and M.is_cuda, f"{what}: (total_n, nrhs) float64"
        nrhs = M.shape[1]
        colmajor = (M.shape[0] <= 1 or M.stride(0) == 1) and (nrhs <= 1 or M.stride(1) >= max(self.total_n, 1))
        if overwrite and not colmajor:
            raise MPFError(f"{what}: overwrite=True needs a column-major tensor (MPFContext.colmajor); this one would be copied")
        if not colmajor or (copy and not overwrite):
            T = ctx.colmajor(self.total_n, nrhs)
            T.copy_(M)
            M = T
        return M, (M.stride(1) if nrhs > 1 else max(self.total_n, 1))

    def lange(self, A, norm="1"):
        """mpf_lange_vbatched: the '1' / 'O', 'I' or 'M' norm of every matrix of the flat tensor A, a float64 (batch,) device tensor
        (0 for a matrix of order 0)."""
        ctx, t = self.ctx, self.ctx.torch
        ctx._bind()
        out = t.zeros(self.batch, dtype=t.float64, device=ctx.device)
        ctx._check(ctx.L.mpf_lange_vbatched(ctx.h, self.h, norm.encode()[:1], _ptr(self._flat(A, "lange")), _ptr(out)), "mpf_lange_vbatched")
        return out

    def gecon(self, LU, anorm, norm="1", want_ainvnm=False):
        """mpf_gecon_vbatched: rcond[b] = (1 / ||(L U)^-1||) / anorm[b] from getrf's factors, the norm of the inverse exact.  anorm: a
        float64 (batch,) device tensor (lange of the matrices, same norm).  Returns rcond, or (rcond, ainvnm) with want_ainvnm; rcond
        is 0 for anorm 0, a zero on U's diagonal or a non-finite inverse, 1 for a matrix of order 0."""
        ctx, t = self.ctx, self.ctx.torch
        ctx._bind()
        assert anorm.dtype == t.float64 and anorm.is_cuda and anorm.shape == (self.batch,)
        anorm = anorm.contiguous()
        rcond = t.zeros(self.batch, dtype=t.float64, device=ctx.device)
        ainv = t.zeros(self.batch, dtype=t.float64, device=ctx.device) if want_ainvnm else None
        rc = ctx.L.mpf_gecon_vbatched(ctx.h, self.h, norm.encode()[:1], _ptr(self._flat(LU, "gecon")), _ptr(anorm), _ptr(rcond),
                                      _ptr(ainv) if want_ainvnm else None)
        ctx._check(rc, "mpf_gecon_vbatched")
        return (rcond, ainv) if want_ainvnm else rcond

    def residual(self, A, X, B, trans=False, want_w=True):
        """mpf_residual_vbatched: (R, W) with R = B - op(D) X and W = |B| + |op(D)| |X| for the block-diagonal D of the matrices in
        the flat tensor A (W None without want_w), new column-major tensors; X and B are (total_n, nrhs), or (total_n,)."""
        ctx = self.ctx
        ctx._bind()
        if B.dim() == 1:
            R, W = self.residual(A, X.unsqueeze(1), B.unsqueeze(1), trans, want_w)
            return R.squeeze(1), (W.squeeze(1) if want_w else None)
        assert X.shape == B.shape
        nrhs = B.shape[1]
        Xm, ldx = self._tall(X, "residual X", False, copy=False)
        Bm, ldb = self._tall(B, "residual B", False, copy=False)
        R = ctx.colmajor(self.total_n, nrhs)
        W = ctx.colmajor(self.total_n, nrhs) if want_w else None
        ldr = R.stride(1) if nrhs > 1 else max(self.total_n, 1)
        rc = ctx.L.mpf_residual_vbatched(ctx.h, self.h, int(bool(trans)), _ptr(self._flat(A, "residual")), nrhs, _ptr(Xm), ldx, _ptr(Bm), ldb,
                                         _ptr(R), ldr, _ptr(W) if want_w else None)
        ctx._check(rc, "mpf_residual_vbatched")
        return R, W

    def gerfs(self, A, LU, ipiv, B, X, trans=False, itmax=0, overwrite=False, want_ferr=True):
        """mpf_gerfs_vbatched: dgerfs per matrix and column with getrf's factors.  X holds a solution (getrs's) and is refined: a new
        column-major tensor, or X itself with overwrite=True.  Returns (X, ferr, berr, iters): float64 / int32 (batch, nrhs) device
        tensors (ferr None without want_ferr); the columns of a matrix of order 0 give 0."""
        ctx, t = self.ctx, self.ctx.torch
        ctx._bind()
        if B.dim() == 1:
            Xr, ferr, berr, its = self.gerfs(A, LU, ipiv, B.unsqueeze(1), X.unsqueeze(1), trans, itmax, overwrite, want_ferr)
            return Xr.squeeze(1), ferr, berr, its
        assert X.shape == B.shape
        nrhs = B.shape[1]
        Bm, ldb = self._tall(B, "gerfs B", False, copy=False)
        Xm, ldx = self._tall(X, "gerfs X", overwrite)
        ferr = t.zeros((self.batch, nrhs), dtype=t.float64, device=ctx.device) if want_ferr else None
        berr = t.zeros((self.batch, nrhs), dtype=t.float64, device=ctx.device)
        its = t.zeros((self.batch, nrhs), dtype=t.int32, device=ctx.device)
        rc = ctx.L.mpf_gerfs_vbatched(ctx.h, self.h, int(bool(trans)), _ptr(self._flat(A, "gerfs")), _ptr(self._flat(LU, "gerfs LU")),
                                      _ptr(self._pivots(ipiv)), nrhs, _ptr(Bm), ldb, _ptr(Xm), ldx, int(itmax),
                                      _ptr(ferr) if want_ferr else None, _ptr(berr), _ptr(its))
        ctx._check(rc, "mpf_gerfs_vbatched")
        return Xm, ferr, berr, its

    def cond(self, A, norm="1"):
        """rcond of every matrix in the flat tensor A: getrf on a copy, lange, gecon.  0 for a singular matrix; nothing is read back."""
        LU, _, _ = self.getrf(A)
        return self.gecon(LU, self.lange(A, norm), norm)

    def solvex(self, A, B, trans=False, itmax=0):
        """dgesvx's shape without equilibration (VBatch.gesvx adds it) for the whole descriptor: getrf on a copy, lange / gecon (the '1' norm, or 'I' with
        trans), getrs, gerfs.  Returns (X, rcond, ferr, berr, info), all on the device; never raises on a singular matrix: info[b] is
        its first zero pivot and rcond[b] is 0 (its X, ferr and berr are not meaningful)."""
        norm = "I" if trans else "1"
        LU, ipiv, info = self.getrf(A)
        rcond = self.gecon(LU, self.lange(A, norm), norm)
        X = self.getrs(LU, ipiv, B, trans=trans)
        X, ferr, berr, _ = self.gerfs(A, LU, ipiv, B, X, trans=trans, itmax=itmax, overwrite=True)
        return X, rcond, ferr, berr, info

    # ---- equilibration (include/mpf_c.h: mpf_geequ_vbatched, mpf_laqge_vbatched, mpf_lascl2_vbatched) ------------------------------------------
    def _vec(self, s, what):
        t = self.ctx.torch
        assert s.dim() == 1 and s.dtype == t.float64 and s.is_cuda and s.is_contiguous() and s.numel() >= self.total_n, \
            f"{what}: a float64 device tensor of total_n = {self.total_n} elements"
        return s

    def geequ(self, A):
        """mpf_geequ_vbatched: (r, c, rowcnd, colcnd, amax, info) of every matrix of the flat tensor A -- r and c float64 (total_n,),
        matrix b's at offv[b]; the others (batch,).  A matrix of order 0 gives rowcnd = colcnd = 1, amax = 0, info = 0."""
        ctx, t = self.ctx, self.ctx.torch
        ctx._bind()
        r, c = (t.zeros(max(self.total_n, 1), dtype=t.float64, device=ctx.device) for _ in range(2))
        rowcnd, colcnd, amax = (t.zeros(self.batch, dtype=t.float64, device=ctx.device) for _ in range(3))
        info = self._info(None)
        rc = ctx.L.mpf_geequ_vbatched(ctx.h, self.h, _ptr(self._flat(A, "geequ")), _ptr(r), _ptr(c), _ptr(rowcnd), _ptr(colcnd), _ptr(amax),
                                      _ptr(info))
        ctx._check(rc, "mpf_geequ_vbatched")
        return r[:self.total_n], c[:self.total_n], rowcnd, colcnd, amax, info

    def laqge(self, A, r, c, rowcnd, colcnd, amax, info, rule=1, overwrite=False):
        """mpf_laqge_vbatched: (As, equed, spread) as MPFContext.laqge_batched returns them, As flat in this layout (A itself with
        overwrite=True, else a new tensor formed out of place, zero between the matrices)."""
        ctx, t = self.ctx, self.ctx.torch
        ctx._bind()
        Am = self._flat(A, "laqge")
        As = Am if overwrite else t.zeros_like(Am)
        equed = t.zeros(self.batch, dtype=t.int32, device=ctx.device)
        spread = t.ones((self.batch, 2), dtype=t.float64, device=ctx.device)
        for v in (rowcnd, colcnd, amax):
            assert v.dtype == t.float64 and v.is_cuda and v.shape == (self.batch,) and v.is_contiguous()
        rc = ctx.L.mpf_laqge_vbatched(ctx.h, self.h, int(rule), _ptr(Am), _ptr(self._vec(r, "laqge r")), _ptr(self._vec(c, "laqge c")),
                                      _ptr(rowcnd), _ptr(colcnd), _ptr(amax), _ptr(self._info(info)), _ptr(As), _ptr(equed), _ptr(spread))
        ctx._check(rc, "mpf_laqge_vbatched")
        return As, equed, spread

    def lascl2(self, s, V, equed=None, bit=0, overwrite=False):
        """mpf_lascl2_vbatched: V = diag(s) V on the rows of the matrices with equed[b] & bit (all when equed is None); V is
        (total_n,) or a (total_n, nrhs) tensor, s float64 (total_n,).  Returns a new column-major tensor, or V itself with overwrite."""
        ctx, t = self.ctx, self.ctx.torch
        ctx._bind()
        if V.dim() == 1:
            assert V.is_contiguous()
            return self.lascl2(s, V.unsqueeze(1), equed, bit, overwrite).squeeze(1)
        Vm, ldv = self._tall(V, "lascl2 V", overwrite)
        if equed is not None:
            assert equed.dtype == t.int32 and equed.is_cuda and equed.shape == (self.batch,) and equed.is_contiguous()
        rc = ctx.L.mpf_lascl2_vbatched(ctx.h, self.h, _ptr(self._vec(s, "lascl2 s")), Vm.shape[1], _ptr(Vm), ldv,
                                       _ptr(equed) if equed is not None else None, int(bit))
        ctx._check(rc, "mpf_lascl2_vbatched")
        return Vm

    def gesvx(self, A, B, trans=False, itmax=0, equilibrate=1):
        """MPFContext.gesvx_batched for the whole descriptor: (X, rcond, ferr, berr, info, equed, r, c), all on the device;
        equilibrate=0: solvex's bits."""
        norm = "I" if trans else "1"
        r, c, rowcnd, colcnd, amax, einfo = self.geequ(A)
        As, equed, spread = self.laqge(A, r, c, rowcnd, colcnd, amax, einfo, rule=equilibrate)
        LU, ipiv, info = self.getrf(As)
        rcond = self.gecon(LU, self.lange(As, norm), norm)
        Bs = self.lascl2(c if trans else r, B, equed, 2 if trans else 1)
        X = self.getrs(LU, ipiv, Bs, trans=trans)
        X, ferr, berr, _ = self.gerfs(As, LU, ipiv, Bs, X, trans=trans, itmax=itmax, overwrite=True)
        X = self.lascl2(r if trans else c, X, equed, 1 if trans else 2, overwrite=True)
        ferr = ferr * spread[:, 0 if trans else 1].unsqueeze(1)
        return X, rcond, ferr, berr, info, equed, r, c
