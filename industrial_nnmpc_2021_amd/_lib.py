"""ctypes binding of libnnmpc_hip.so (C ABI: include/nnmpc.h).  Fails loudly."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnnmpc_hip.so")

HOST, DEVICE = 0, 1
ST_OPTIMAL, ST_MAXITER, ST_NUMERIC = 0, 1, 2
OUT_SEQUENCE, OUT_FIRST_MOVE = 0, 1
EINVAL, EHIP, ENOMEM, ENOTIMPL = -1, -2, -3, -4


class QpOpts(C.Structure):
    _fields_ = [("max_batch", C.c_int32), ("nb", C.c_int32), ("max_ipm_iters", C.c_int32),
                ("max_polish_rounds", C.c_int32), ("max_refine", C.c_int32),
                ("max_rounds", C.c_int32), ("sub_steps", C.c_int32), ("stale_max_changes", C.c_int32),
                ("stale_cg_limit", C.c_int32), ("method", C.c_int32), ("asm_max_active", C.c_int32),
                ("asm_max_rounds", C.c_int32), ("asm_f32_rounds", C.c_int32), ("seg_max", C.c_int32), ("asm_tail_batch", C.c_int32), ("asm_predict_iters", C.c_int32), ("asm_overlap", C.c_int32), ("ipm_tol", C.c_float), ("refine_tol", C.c_double),
                ("bound_tol", C.c_double)]


class QpStats(C.Structure):
    _fields_ = [("problems", C.c_int64), ("rounds", C.c_int64), ("factorizations", C.c_int64),
                ("ipm_iterations", C.c_int64), ("panel_launches", C.c_int64),
                ("panel_ms", C.c_double), ("diag_ms", C.c_double), ("trsv_ms", C.c_double),
                ("total_ms", C.c_double), ("panel_flops", C.c_double), ("trsv_solves", C.c_int64), ("asm_solved", C.c_int64),
                ("asm_rounds", C.c_int64), ("asm_gemm_launches", C.c_int64), ("asm_gemm_ms", C.c_double),
                ("asm_gemm_flops", C.c_double), ("asm_lambda_ms", C.c_double), ("asm_update_ms", C.c_double), ("asm_lambda_flops", C.c_double),
                ("asm_lambda_bytes", C.c_double), ("asm_e1max", C.c_double),
                ("asm_e2max", C.c_double), ("asm_full_checks", C.c_int64), ("asm_lambda32_ms", C.c_double),
                ("asm_lambda64_ms", C.c_double), ("asm_lambda32_flops", C.c_double),
                ("asm_lambda32_launches", C.c_int64), ("asm_lambda64_launches", C.c_int64), ("asm_far_passes", C.c_int64), ("asm_side_ms", C.c_double),
                ("asm_small_passes", C.c_int64), ("asm_predict_launches", C.c_int64), ("asm_predict_ms", C.c_double),
                ("asm_predict_flops", C.c_double), ("asm_overlapped_passes", C.c_int64),
                ("mult_ms", C.c_double), ("mult_launches", C.c_int64),
                ("sens_ms", C.c_double), ("sens_launches", C.c_int64), ("sens_lds_problems", C.c_int64),
                ("sens_slab_problems", C.c_int64), ("sens_total_ms", C.c_double),
                ("adj_ms", C.c_double), ("adj_launches", C.c_int64), ("adj_lds_problems", C.c_int64),
                ("adj_slab_problems", C.c_int64), ("adj_total_ms", C.c_double),
                ("asm_carried", C.c_int64), ("asm_shared_passes", C.c_int64)]


CL_MPC, CL_NN, CL_SATDLQR, CL_US, CL_NN_UNSTD = 0, 1, 2, 3, 4
NN_STRUCTURED, NN_UNSTD, NN_UNSTD_RELU = 0, 1, 2
CL_PLANT_LINEAR, CL_PLANT_CSTRS_FLASH, CSTRS_NPAR = 0, 1, 51


class ClModel(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("nx", "nu", "ny", "nd", "nz")] + \
               [(k, C.c_void_p) for k in ("A", "B", "C", "Bp", "Aaug", "Baug", "Caug", "L", "tb", "Qb", "Qy", "q0", "Cd",
                                          "Eb", "Xb", "Xu", "Qaug", "Raug", "Maug", "ulb", "uub", "x0", "xhat0", "uprev0")]


class ClSlot(C.Structure):
    _fields_ = [("kind", C.c_int32), ("qp", C.c_void_p), ("nlayers", C.c_int32), ("dims", C.c_void_p), ("W", C.c_void_p),
                ("b", C.c_void_p), ("with_uprev", C.c_int32), ("xscale", C.c_void_p), ("Kaug", C.c_void_p)]


EXPORTS = ["nnmpc_last_error", "nnmpc_qp_create", "nnmpc_qp_destroy", "nnmpc_qp_solve_batch",
           "nnmpc_qp_solve_batch_warm", "nnmpc_qp_solve_batch_ex", "nnmpc_qp_solve_batch_dual", "nnmpc_qp_multipliers",
           "nnmpc_qp_sensitivity", "nnmpc_qp_adjoint",
           "nnmpc_qp_set_inverse", "nnmpc_qp_dims",
           "nnmpc_qp_first_moves", "nnmpc_qp_set_farfield", "nnmpc_qp_farfield_missing",
           "nnmpc_qp_set_profiling", "nnmpc_qp_get_stats", "nnmpc_qp_debug_factor_solve", "nnmpc_qp_debug_factor_fail",
           "nnmpc_qp_debug_predict", "nnmpc_qp_debug_gemm",
           "nnmpc_nn_create", "nnmpc_nn_create_ex", "nnmpc_nn_destroy", "nnmpc_nn_forward", "nnmpc_nn_last_ms", "nnmpc_nn_last_hidden_ms",
           "nnmpc_train_create", "nnmpc_train_create_ex", "nnmpc_train_destroy", "nnmpc_train_set_data", "nnmpc_train_grad", "nnmpc_train_step",
           "nnmpc_train_epoch", "nnmpc_train_eval", "nnmpc_train_get_weights", "nnmpc_train_set_weights",
           "nnmpc_train_snapshot", "nnmpc_train_restore", "nnmpc_train_last_ms", "nnmpc_train_dw_slices",
           "nnmpc_train_padding_max",
           "nnmpc_train_create_tan", "nnmpc_train_set_tangents", "nnmpc_train_set_tan_weight", "nnmpc_train_last_losses",
           "nnmpc_train_create_tan_ex", "nnmpc_train_set_tangents_ex",
           "nnmpc_train_group_create", "nnmpc_train_group_destroy", "nnmpc_train_group_set_data",
           "nnmpc_train_group_epoch", "nnmpc_train_group_eval", "nnmpc_train_group_get_weights",
           "nnmpc_train_group_set_weights", "nnmpc_train_group_snapshot", "nnmpc_train_group_restore",
           "nnmpc_train_group_padding_max", "nnmpc_train_group_last_ms", "nnmpc_train_group_last_launches",
           "nnmpc_train_create_group_ex",
           "nnmpc_train_create_group_tan", "nnmpc_train_set_group_tangents", "nnmpc_train_set_group_tan_weights",
           "nnmpc_train_last_group_losses",
           "nnmpc_chain_create", "nnmpc_chain_destroy", "nnmpc_chain_run", "nnmpc_chain_reset", "nnmpc_chain_last_ms",
           "nnmpc_ts_create", "nnmpc_ts_destroy", "nnmpc_ts_solve_batch",
           "nnmpc_cl_create", "nnmpc_cl_destroy", "nnmpc_cl_run", "nnmpc_cl_reset", "nnmpc_cl_last_ms",
           "nnmpc_cl_set_plant", "nnmpc_cl_last_plant_ms", "nnmpc_cstrs_flow",
           "nnmpc_device_count", "nnmpc_set_device", "nnmpc_device_synchronize", "nnmpc_dev_mem_info",
           "nnmpc_dev_malloc", "nnmpc_dev_free", "nnmpc_dev_memset", "nnmpc_memcpy_h2d", "nnmpc_memcpy_d2h",
           "nnmpc_memcpy_d2d", "nnmpc_host_alloc_pinned", "nnmpc_host_free_pinned",
           "nnmpc_comm_unique_id", "nnmpc_comm_init", "nnmpc_comm_destroy", "nnmpc_comm_rank", "nnmpc_comm_world",
           "nnmpc_comm_gather_rows", "nnmpc_comm_allreduce_max", "nnmpc_comm_barrier"]

_lib = None


class NnmpcError(RuntimeError):
    pass


def load():
    """Load the HIP library; raise (never fall back) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NnmpcError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, dp = C.c_void_p, C.c_int32, C.c_void_p
    lib.nnmpc_last_error.restype = C.c_char_p
    lib.nnmpc_last_error.argtypes = []
    lib.nnmpc_qp_create.restype = i32
    lib.nnmpc_qp_create.argtypes = [C.POINTER(vp), i32, i32, i32, dp, dp, dp, C.POINTER(QpOpts)]
    lib.nnmpc_qp_destroy.restype = i32
    lib.nnmpc_qp_destroy.argtypes = [vp]
    lib.nnmpc_qp_solve_batch.restype = i32
    lib.nnmpc_qp_solve_batch.argtypes = [vp, i32, dp, dp, dp, dp, dp, dp, dp, i32]
    lib.nnmpc_qp_solve_batch_warm.restype = i32
    lib.nnmpc_qp_solve_batch_warm.argtypes = [vp, i32, dp, dp, dp, dp, dp, dp, dp, dp, i32]
    lib.nnmpc_qp_set_inverse.restype = i32
    lib.nnmpc_qp_set_inverse.argtypes = [vp, dp, dp]
    lib.nnmpc_qp_set_farfield.restype = i32
    lib.nnmpc_qp_set_farfield.argtypes = [vp, i32, i32, dp, dp, dp]
    lib.nnmpc_qp_farfield_missing.restype = i32
    lib.nnmpc_qp_farfield_missing.argtypes = [vp, C.POINTER(i32)]
    lib.nnmpc_qp_set_profiling.restype = i32
    lib.nnmpc_qp_set_profiling.argtypes = [vp, i32]
    lib.nnmpc_qp_get_stats.restype = i32
    lib.nnmpc_qp_get_stats.argtypes = [vp, C.POINTER(QpStats), i32]
    lib.nnmpc_qp_debug_factor_solve.restype = i32
    lib.nnmpc_qp_debug_factor_solve.argtypes = [vp, i32, dp, dp, dp, dp]
    lib.nnmpc_qp_debug_factor_fail.restype = i32
    lib.nnmpc_qp_debug_factor_fail.argtypes = [vp, i32, dp]
    lib.nnmpc_qp_debug_predict.restype = i32
    lib.nnmpc_qp_debug_predict.argtypes = [vp, i32, dp, dp, dp, i32, i32, dp, dp, C.POINTER(C.c_double)]
    lib.nnmpc_qp_debug_gemm.restype = i32
    lib.nnmpc_qp_debug_gemm.argtypes = [vp, i32, i32, i32, i32, dp, C.c_int64, C.c_int64, dp, C.c_int64, dp, C.c_int64, C.c_int64,
                                        dp, i32, dp, i32, dp, dp, dp]
    lib.nnmpc_nn_create.restype = i32
    lib.nnmpc_nn_create.argtypes = [C.POINTER(vp), i32, C.POINTER(i32), C.POINTER(dp), C.POINTER(dp),
                                    i32, i32, i32, dp, dp, dp, i32, i32]
    lib.nnmpc_nn_create_ex.restype = i32
    lib.nnmpc_nn_create_ex.argtypes = lib.nnmpc_nn_create.argtypes + [i32]
    lib.nnmpc_nn_destroy.restype = i32
    lib.nnmpc_nn_destroy.argtypes = [vp]
    lib.nnmpc_nn_forward.restype = i32
    lib.nnmpc_nn_forward.argtypes = [vp, i32, dp, dp, dp, dp, dp, i32]
    lib.nnmpc_nn_last_ms.restype = i32
    lib.nnmpc_nn_last_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.nnmpc_nn_last_hidden_ms.restype = i32
    lib.nnmpc_nn_last_hidden_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    f64, pf64, pi32, pdp = C.c_double, C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(dp)
    lib.nnmpc_train_create.restype = i32
    lib.nnmpc_train_create.argtypes = [C.POINTER(vp), i32, pi32, pdp, pdp, i32, i32, i32, i32, f64, f64, f64, f64]
    lib.nnmpc_train_create_ex.restype = i32                       # the same with the form (NN_STRUCTURED, NN_UNSTD, NN_UNSTD_RELU)
    lib.nnmpc_train_create_ex.argtypes = lib.nnmpc_train_create.argtypes + [i32]
    lib.nnmpc_train_destroy.restype = i32
    lib.nnmpc_train_destroy.argtypes = [vp]
    lib.nnmpc_train_set_data.restype = i32
    lib.nnmpc_train_set_data.argtypes = [vp, i32, dp, dp, dp, dp, dp, i32]
    lib.nnmpc_train_grad.restype = i32
    lib.nnmpc_train_grad.argtypes = [vp, i32, dp, pf64, pdp, pdp]
    lib.nnmpc_train_step.restype = i32
    lib.nnmpc_train_step.argtypes = [vp, i32, dp, pf64]
    lib.nnmpc_train_epoch.restype = i32
    lib.nnmpc_train_epoch.argtypes = [vp, i32, dp, i32, pf64]
    lib.nnmpc_train_eval.restype = i32
    lib.nnmpc_train_eval.argtypes = [vp, i32, i32, pf64]
    lib.nnmpc_train_get_weights.restype = i32
    lib.nnmpc_train_get_weights.argtypes = [vp, pdp, pdp]
    lib.nnmpc_train_set_weights.restype = i32
    lib.nnmpc_train_set_weights.argtypes = [vp, pdp, pdp]
    lib.nnmpc_train_snapshot.restype = i32
    lib.nnmpc_train_snapshot.argtypes = [vp]
    lib.nnmpc_train_restore.restype = i32
    lib.nnmpc_train_restore.argtypes = [vp]
    lib.nnmpc_train_last_ms.restype = i32
    lib.nnmpc_train_last_ms.argtypes = [vp, pf64, pf64]
    lib.nnmpc_train_dw_slices.restype = i32
    lib.nnmpc_train_dw_slices.argtypes = [vp, pi32]
    lib.nnmpc_train_padding_max.restype = i32
    lib.nnmpc_train_padding_max.argtypes = [vp, pf64]
    lib.nnmpc_train_create_tan.restype = i32                      # nnmpc_train_create_ex for the tangent loss (NN_STRUCTURED only)
    lib.nnmpc_train_create_tan.argtypes = lib.nnmpc_train_create_ex.argtypes
    lib.nnmpc_train_set_tangents.restype = i32                    # (h, n, dx, duprev, t, ptr_kind)
    lib.nnmpc_train_set_tangents.argtypes = [vp, i32, dp, dp, dp, i32]
    lib.nnmpc_train_set_tan_weight.restype = i32
    lib.nnmpc_train_set_tan_weight.argtypes = [vp, f64]
    lib.nnmpc_train_last_losses.restype = i32
    lib.nnmpc_train_last_losses.argtypes = [vp, pf64, pf64]
    lib.nnmpc_train_create_tan_ex.restype = i32                   # nnmpc_train_create_tan + (dirs, whole_input)
    lib.nnmpc_train_create_tan_ex.argtypes = lib.nnmpc_train_create_ex.argtypes + [i32, i32]
    lib.nnmpc_train_set_tangents_ex.restype = i32                 # (h, n, dirs, dx, duprev, dxs, dus, t, ptr_kind)
    lib.nnmpc_train_set_tangents_ex.argtypes = [vp, i32, i32, dp, dp, dp, dp, dp, i32]
    # the sweep in one handle: each entry replaces G calls of the nnmpc_train_* function named beside it
    lib.nnmpc_train_group_create.restype = i32                    # nnmpc_train_create
    lib.nnmpc_train_group_create.argtypes = [C.POINTER(vp), i32, i32, pi32, pdp, pdp, i32, i32, i32, i32, f64, f64, f64, f64]
    lib.nnmpc_train_create_group_ex.restype = i32                 # nnmpc_train_create_ex: the same with the group's form
    lib.nnmpc_train_create_group_ex.argtypes = lib.nnmpc_train_group_create.argtypes + [i32]
    lib.nnmpc_train_group_destroy.restype = i32                   # nnmpc_train_destroy
    lib.nnmpc_train_group_destroy.argtypes = [vp]
    lib.nnmpc_train_group_set_data.restype = i32                  # nnmpc_train_set_data (one shared dataset)
    lib.nnmpc_train_group_set_data.argtypes = [vp, i32, dp, dp, dp, dp, dp, i32]
    lib.nnmpc_train_group_epoch.restype = i32                     # nnmpc_train_epoch
    lib.nnmpc_train_group_epoch.argtypes = [vp, dp, dp, i32, dp]
    lib.nnmpc_train_group_eval.restype = i32                      # nnmpc_train_eval
    lib.nnmpc_train_group_eval.argtypes = [vp, dp, dp, dp]
    lib.nnmpc_train_group_get_weights.restype = i32               # nnmpc_train_get_weights
    lib.nnmpc_train_group_get_weights.argtypes = [vp, i32, pdp, pdp]
    lib.nnmpc_train_group_set_weights.restype = i32               # nnmpc_train_set_weights
    lib.nnmpc_train_group_set_weights.argtypes = [vp, i32, pdp, pdp]
    lib.nnmpc_train_group_snapshot.restype = i32                  # nnmpc_train_snapshot, by mask
    lib.nnmpc_train_group_snapshot.argtypes = [vp, dp]
    lib.nnmpc_train_group_restore.restype = i32                   # nnmpc_train_restore, by mask
    lib.nnmpc_train_group_restore.argtypes = [vp, dp]
    lib.nnmpc_train_group_padding_max.restype = i32               # nnmpc_train_padding_max
    lib.nnmpc_train_group_padding_max.argtypes = [vp, pf64]
    lib.nnmpc_train_group_last_ms.restype = i32                   # nnmpc_train_last_ms
    lib.nnmpc_train_group_last_ms.argtypes = [vp, pf64, pf64]
    lib.nnmpc_train_group_last_launches.restype = i32             # (new: launches of the last epoch / eval)
    lib.nnmpc_train_group_last_launches.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.nnmpc_train_create_group_tan.restype = i32                # nnmpc_train_create_tan: a group with one tangent weight per member
    lib.nnmpc_train_create_group_tan.argtypes = lib.nnmpc_train_create_group_ex.argtypes
    lib.nnmpc_train_set_group_tangents.restype = i32              # nnmpc_train_set_tangents (one shared set)
    lib.nnmpc_train_set_group_tangents.argtypes = [vp, i32, dp, dp, dp, i32]
    lib.nnmpc_train_set_group_tan_weights.restype = i32           # (h, w[G])
    lib.nnmpc_train_set_group_tan_weights.argtypes = [vp, dp]
    lib.nnmpc_train_last_group_losses.restype = i32               # nnmpc_train_last_losses, (h, mse[G], tan_mse[G])
    lib.nnmpc_train_last_group_losses.argtypes = [vp, dp, dp]
    u64 = C.c_uint64
    lib.nnmpc_qp_solve_batch_ex.restype = i32
    lib.nnmpc_qp_solve_batch_ex.argtypes = [vp, i32, dp, dp, dp, dp, dp, dp, dp, dp, i32, i32]
    lib.nnmpc_qp_solve_batch_dual.restype = i32                   # _ex plus the bound multipliers (mult before ptr_kind)
    lib.nnmpc_qp_solve_batch_dual.argtypes = [vp, i32, dp, dp, dp, dp, dp, dp, dp, dp, dp, i32, i32]
    lib.nnmpc_qp_multipliers.restype = i32
    lib.nnmpc_qp_multipliers.argtypes = [vp, i32, dp, dp, dp, dp, dp, i32]
    lib.nnmpc_qp_sensitivity.restype = i32                        # (h, B, D, active, status, dx0, dlb, dub, du, dmult, flag, ptr_kind, out_kind)
    lib.nnmpc_qp_sensitivity.argtypes = [vp, i32, i32, dp, dp, dp, dp, dp, dp, dp, dp, i32, i32]
    lib.nnmpc_qp_adjoint.restype = i32                            # (h, B, D, active, status, v, gx0, glb, gub, gbound, flag, ptr_kind, in_kind)
    lib.nnmpc_qp_adjoint.argtypes = [vp, i32, i32, dp, dp, dp, dp, dp, dp, dp, dp, i32, i32]
    lib.nnmpc_qp_first_moves.restype = i32
    lib.nnmpc_qp_first_moves.argtypes = [dp, C.c_int64, dp, i32, i32, dp]
    lib.nnmpc_qp_dims.restype = i32
    lib.nnmpc_qp_dims.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.nnmpc_chain_create.restype = i32
    lib.nnmpc_chain_create.argtypes = [C.POINTER(vp), vp, i32, i32, i32, i32, dp, dp, dp, dp, dp, dp, dp]
    lib.nnmpc_chain_destroy.restype = i32
    lib.nnmpc_chain_destroy.argtypes = [vp]
    lib.nnmpc_chain_run.restype = i32
    lib.nnmpc_chain_run.argtypes = [vp, i32, dp, dp, dp, dp, dp, dp, dp, i32, i32]
    lib.nnmpc_chain_reset.restype = i32
    lib.nnmpc_chain_reset.argtypes = [vp]
    lib.nnmpc_chain_last_ms.restype = i32
    lib.nnmpc_chain_last_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.nnmpc_ts_create.restype = i32
    lib.nnmpc_ts_create.argtypes = [C.POINTER(vp), i32, i32, dp, dp, dp, dp]
    lib.nnmpc_ts_destroy.restype = i32
    lib.nnmpc_ts_destroy.argtypes = [vp]
    lib.nnmpc_ts_solve_batch.restype = i32
    lib.nnmpc_ts_solve_batch.argtypes = [vp, i32, dp, dp, dp, dp, dp, dp, i32]
    lib.nnmpc_cl_create.restype = i32
    lib.nnmpc_cl_create.argtypes = [C.POINTER(vp), C.POINTER(ClModel), vp, i32, C.POINTER(ClSlot), i32, C.POINTER(i32)]
    lib.nnmpc_cl_destroy.restype = i32
    lib.nnmpc_cl_destroy.argtypes = [vp]
    lib.nnmpc_cl_run.restype = i32
    lib.nnmpc_cl_run.argtypes = [vp, i32, i32, dp, dp, dp, dp, dp, dp] + [dp] * 9 + [i32]
    lib.nnmpc_cl_reset.restype = i32
    lib.nnmpc_cl_reset.argtypes = [vp]
    lib.nnmpc_cl_last_ms.restype = i32
    lib.nnmpc_cl_last_ms.argtypes = [vp, C.POINTER(C.c_double), dp, dp]
    lib.nnmpc_cl_set_plant.restype = i32
    lib.nnmpc_cl_set_plant.argtypes = [vp, i32, dp, i32, C.c_double, i32]
    lib.nnmpc_cl_last_plant_ms.restype = i32
    lib.nnmpc_cl_last_plant_ms.argtypes = [vp, C.POINTER(C.c_double)]
    lib.nnmpc_cstrs_flow.restype = i32
    lib.nnmpc_cstrs_flow.argtypes = [i32, dp, i32, C.c_double, i32, dp, dp, dp, dp, i32]
    lib.nnmpc_device_count.restype = i32
    lib.nnmpc_device_count.argtypes = []
    lib.nnmpc_set_device.restype = i32
    lib.nnmpc_set_device.argtypes = [i32]
    lib.nnmpc_device_synchronize.restype = i32
    lib.nnmpc_device_synchronize.argtypes = []
    lib.nnmpc_dev_mem_info.restype = i32
    lib.nnmpc_dev_mem_info.argtypes = [C.POINTER(u64), C.POINTER(u64)]
    lib.nnmpc_dev_malloc.restype = i32
    lib.nnmpc_dev_malloc.argtypes = [C.POINTER(vp), u64]
    lib.nnmpc_dev_free.restype = i32
    lib.nnmpc_dev_free.argtypes = [vp]
    lib.nnmpc_dev_memset.restype = i32
    lib.nnmpc_dev_memset.argtypes = [vp, i32, u64]
    for name in ("nnmpc_memcpy_h2d", "nnmpc_memcpy_d2h", "nnmpc_memcpy_d2d"):
        getattr(lib, name).restype = i32
        getattr(lib, name).argtypes = [vp, vp, u64]
    lib.nnmpc_host_alloc_pinned.restype = i32
    lib.nnmpc_host_alloc_pinned.argtypes = [C.POINTER(vp), u64]
    lib.nnmpc_host_free_pinned.restype = i32
    lib.nnmpc_host_free_pinned.argtypes = [vp]
    lib.nnmpc_comm_unique_id.restype = i32
    lib.nnmpc_comm_unique_id.argtypes = [vp]
    lib.nnmpc_comm_init.restype = i32
    lib.nnmpc_comm_init.argtypes = [C.POINTER(vp), vp, i32, i32]
    lib.nnmpc_comm_destroy.restype = i32
    lib.nnmpc_comm_destroy.argtypes = [vp]
    lib.nnmpc_comm_rank.restype = i32
    lib.nnmpc_comm_rank.argtypes = [vp]
    lib.nnmpc_comm_world.restype = i32
    lib.nnmpc_comm_world.argtypes = [vp]
    lib.nnmpc_comm_gather_rows.restype = i32
    lib.nnmpc_comm_gather_rows.argtypes = [vp, dp, C.POINTER(C.c_int64), i32, dp, i32]
    lib.nnmpc_comm_allreduce_max.restype = i32
    lib.nnmpc_comm_allreduce_max.argtypes = [vp, C.POINTER(C.c_double)]
    lib.nnmpc_comm_barrier.restype = i32
    lib.nnmpc_comm_barrier.argtypes = [vp]
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().nnmpc_last_error().decode(errors="replace")
        raise NnmpcError(f"{what} failed (code {rc}): {msg}")


class DeviceArray:
    """HBM-resident array owned through the library (nnmpc_dev_malloc): shape, numpy dtype, data_ptr().

    What a torch CUDA tensor is used for elsewhere -- device memory that outlives a call -- without binding
    anything but libnnmpc_hip.so.  ``DeviceArray.from_host(a)`` uploads, ``.to_host()`` downloads.
    """

    def __init__(self, shape, dtype):
        import numpy as np
        self.shape = tuple(int(v) for v in (shape if hasattr(shape, "__len__") else (shape,)))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self._p = C.c_void_p()
        check(load().nnmpc_dev_malloc(C.byref(self._p), self.nbytes), "nnmpc_dev_malloc")

    @classmethod
    def from_host(cls, a):
        import numpy as np
        a = np.ascontiguousarray(a)
        d = cls(a.shape, a.dtype)
        d.upload(a)
        return d

    def data_ptr(self):
        return self._p.value or 0

    def upload(self, a):
        import numpy as np
        a = np.ascontiguousarray(a, dtype=self.dtype)
        if a.nbytes != self.nbytes:
            raise ValueError("upload: size mismatch")
        check(load().nnmpc_memcpy_h2d(self._p, a.ctypes.data_as(C.c_void_p), self.nbytes), "nnmpc_memcpy_h2d")

    def to_host(self, rows=None):
        """The whole array, or its first ``rows`` rows."""
        import numpy as np
        shape = self.shape if rows is None else (int(rows),) + self.shape[1:]
        out = np.empty(shape, self.dtype)
        check(load().nnmpc_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self._p, out.nbytes), "nnmpc_memcpy_d2h")
        return out

    def row_ptr(self, row):
        """Device address of row ``row`` (leading dimension)."""
        import numpy as np
        stride = int(np.prod(self.shape[1:], dtype=np.int64)) * self.dtype.itemsize
        return C.c_void_p((self._p.value or 0) + int(row) * stride)

    def free(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            load().nnmpc_dev_free(self._p)
            self._p = C.c_void_p()

    __del__ = free


def set_device(dev):
    check(load().nnmpc_set_device(int(dev)), "nnmpc_set_device")


def synchronize():
    check(load().nnmpc_device_synchronize(), "nnmpc_device_synchronize")


def device_count():
    return int(load().nnmpc_device_count())
