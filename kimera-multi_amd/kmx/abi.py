"""ctypes binding of include/kmx_abi.h (the drop-in C ABI).

The product path has exactly one backend: the in-tree HIP library
``kmx/libkmx.so`` built for gfx950 by ``csrc/Makefile``. There is no CPU
fallback: if the library is missing or no HIP device is visible, the handles
raise ``KmxError`` (the CPU restatement in ``oracle/`` is test infrastructure
and is never reached from here).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_LIB_PATH = Path(__file__).resolve().parent / "libkmx.so"

KMX_OK = 0
KMX_ETIMEOUT = -6
ABI_VERSION = 10  # include/kmx_abi.h KMX_ABI_VERSION this binding is written for
KMX_COST_L2 = 0
KMX_COMM_ID_BYTES = 128  # include/kmx_abi.h (ncclUniqueId)
KMX_COST_GNC_TLS = 1
KMX_SCHEDULE_SEQUENTIAL = 0
KMX_SCHEDULE_CONCURRENT = 1
KMX_EVAL_COST_EGRAD = 0
KMX_EVAL_EHESS = 1
KMX_EVAL_RGRAD = 2
KMX_EVAL_RHESS = 3
KMX_EVAL_PRECON = 4
KMX_EVAL_RETRACT = 5
KMX_EVAL_PROJECT = 6
KMX_NORM_L1 = 0
KMX_NORM_HAMMING = 1
KMX_RNG_GCC9 = 0
KMX_RNG_GCC11 = 1
KMX_LCD_STAGE_2D2D = 1
KMX_LCD_STAGE_RECOVER = 2
KMX_EINVAL = -1
KMX_ESTATE = -3
KMX_EUNSUP = -5
KMX_VOC_TF_IDF = 0
KMX_VOC_TF = 1
KMX_VOC_IDF = 2
KMX_VOC_BINARY = 3

TCG_STOP_NAMES = {0: "none", 1: "negative_curvature", 2: "exceeded_trust_region",
                  3: "linear", 4: "superlinear", 5: "max_iterations", 6: "skipped"}


class KmxError(RuntimeError):
    pass


class PgoParams(C.Structure):
    _fields_ = [
        ("d", C.c_int), ("r", C.c_int), ("rtr_iterations", C.c_int),
        ("tcg_max_iterations", C.c_int), ("tcg_kappa", C.c_double),
        ("tcg_theta", C.c_double), ("rtr_initial_radius", C.c_double),
        ("rtr_max_radius", C.c_double), ("rtr_accept_rho", C.c_double),
        ("gradnorm_tol", C.c_double), ("use_preconditioner", C.c_int),
        ("precond_shift", C.c_double), ("robust_cost", C.c_int),
        ("gnc_barc", C.c_double), ("gnc_mu_init", C.c_double),
        ("gnc_mu_step", C.c_double), ("acceleration", C.c_int), ("restart_interval", C.c_int),
        ("method", C.c_int), ("tcg_form", C.c_int), ("rgd_stepsize", C.c_double), ("tile_incidences", C.c_int),
        ("reserved", C.c_int),
    ]


class IterStats(C.Structure):
    _fields_ = [
        ("updated", C.c_int), ("tcg_iterations", C.c_int), ("tcg_stop", C.c_int),
        ("accepted", C.c_int), ("f_init", C.c_double), ("gradnorm_init", C.c_double),
        ("f_final", C.c_double), ("rho", C.c_double), ("radius", C.c_double),
        ("rel_change", C.c_double), ("edges", C.c_int64), ("hessvecs", C.c_int64),
    ]

    def as_dict(self) -> dict:
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["tcg_stop"] = TCG_STOP_NAMES.get(self.tcg_stop, str(self.tcg_stop))
        return d


class PgoCounters(C.Structure):
    _fields_ = [
        ("hessvec_ms_total", C.c_double), ("hessvec_launches", C.c_int64),
        ("hessvec_alg_bytes", C.c_double), ("edges_iters", C.c_int64),
        ("block_updates", C.c_int64), ("hessvecs", C.c_int64), ("gnc_updates", C.c_int64),
    ]


class GncState(C.Structure):
    _fields_ = [
        ("inner_iter", C.c_int32), ("updates", C.c_int32), ("last_fired", C.c_int32),
        ("rounds", C.c_int32), ("mu", C.c_double), ("reserved", C.c_double * 3),
    ]

    def as_dict(self) -> dict:
        return {"inner_iter": self.inner_iter, "updates": self.updates, "last_fired": bool(self.last_fired),
                "rounds": self.rounds, "mu": self.mu}


class LcdParams(C.Structure):
    _fields_ = [
        ("norm", C.c_int), ("lowe_ratio", C.c_double), ("min_2d2d_inliers", C.c_int),
        ("min_3d3d_inliers", C.c_int), ("ransac_threshold_2d2d", C.c_double),
        ("ransac_threshold_3d3d", C.c_double), ("ransac_max_iterations", C.c_int),
        ("ransac_probability", C.c_double), ("ransac_randomize", C.c_int),
        ("ransac_seed", C.c_uint32), ("rng_variant", C.c_int),
        ("use_1point_3d3d", C.c_int), ("pose_recovery_type", C.c_int), ("min_2d3d_inliers", C.c_int),
        ("ransac_threshold_2d3d", C.c_double), ("algorithm_2d2d", C.c_int), ("refine_pose", C.c_int),
        ("rng_stream", C.c_int), ("reserved", C.c_int * 1),
    ]


class LcdResult(C.Structure):
    _fields_ = [
        ("n_matches", C.c_int32), ("mono_inliers", C.c_int32),
        ("stereo_inliers", C.c_int32), ("accepted", C.c_int32),
        ("iterations_2d2d", C.c_int32), ("pnp_inliers", C.c_int32),
        ("T_query_match", C.c_double * 12),
    ]


class ChordalParams(C.Structure):
    """kmx_chordal_params (0 in a field: the library's default)."""
    _fields_ = [("rtol", C.c_double), ("max_iterations", C.c_int32), ("check_every", C.c_int32)]


class ChordalRobustParams(C.Structure):
    """kmx_chordal_robust_params (0 in a field: the library's default)."""
    _fields_ = [("barc", C.c_double), ("mu_init", C.c_double), ("mu_step", C.c_double),
                ("max_updates", C.c_int32), ("reserved", C.c_int32)]


class ChordalRobustInfo(C.Structure):
    """kmx_chordal_robust_info: one per block of a kmx_chordal_solve_robust."""
    _fields_ = [("updates", C.c_int32), ("converged", C.c_int32), ("n_kept", C.c_int32), ("n_rejected", C.c_int32),
                ("n_fractional", C.c_int32), ("reserved", C.c_int32), ("mu", C.c_double)]


class ChordalBlockInfo(C.Structure):
    """kmx_chordal_block_info: one per block of a kmx_chordal_solve."""
    _fields_ = [("iterations_rot", C.c_int32), ("iterations_trans", C.c_int32), ("converged", C.c_int32),
                ("relres_rot", C.c_double * 3), ("relres_trans", C.c_double * 3)]


class CertParams(C.Structure):
    """kmx_cert_params (0 in max_steps / test_every / check_every: the library's default)."""
    _fields_ = [("eta", C.c_double), ("max_steps", C.c_int32), ("test_every", C.c_int32),
                ("check_every", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64)]


class CertResult(C.Structure):
    """kmx_cert_result."""
    _fields_ = [("decision", C.c_int32), ("steps", C.c_int32), ("theta_min", C.c_double),
                ("theta_max", C.c_double), ("residual", C.c_double)]


class CertPointInfo(C.Structure):
    """kmx_cert_point_info."""
    _fields_ = [("cost", C.c_double), ("trace_lambda", C.c_double), ("stationarity", C.c_double)]


KMX_CERT_UNDECIDED, KMX_CERT_CERTIFIED, KMX_CERT_NEGATIVE = 0, 1, 2
CERT_DECISION = ("UNDECIDED", "CERTIFIED", "NEGATIVE")  # kmx_abi.h KMX_CERT_* in their order


class BowDetectParams(C.Structure):
    """kmx_bow_detect_params (LcdParams.yaml:3-12)."""
    _fields_ = [("use_nss", C.c_int32), ("alpha", C.c_double), ("min_nss_factor", C.c_double),
                ("max_db_results", C.c_int32), ("recent_frames_window", C.c_int32),
                ("max_intraisland_gap", C.c_int32), ("min_matches_per_island", C.c_int32),
                ("max_nrFrames_between_queries", C.c_int32), ("max_nrFrames_between_islands", C.c_int32),
                ("min_temporal_matches", C.c_int32)]


class BowDetectRecord(C.Structure):
    """kmx_bow_detect_record: one per query of a device-side detection (48 bytes)."""
    _fields_ = [("query_id", C.c_int32), ("status", C.c_int32), ("match_id", C.c_int32), ("n_kept", C.c_int32),
                ("island_start", C.c_int32), ("island_end", C.c_int32), ("score", C.c_double), ("nss", C.c_double),
                ("island_score", C.c_double)]


# the same layout for numpy: np.zeros(nq, BOW_RECORD_DTYPE) is a kmx_bow_detect_record[nq]
BOW_RECORD_DTYPE = np.dtype([(n, np.int32 if t is C.c_int32 else np.float64) for n, t in BowDetectRecord._fields_])
assert BOW_RECORD_DTYPE.itemsize == C.sizeof(BowDetectRecord) == 48

# kmx_abi.h: the status enum in its order, and the two modes
BOW_STATUS = ("NO_MATCHES", "LOW_NSS_FACTOR", "LOW_SCORE", "NO_GROUPS", "FAILED_TEMPORAL_CONSTRAINT", "LOOP_DETECTED")
BOW_MODE_INTRA, BOW_MODE_INTER = 0, 1



class MeshParams(C.Structure):
    """kmx_mesh_params."""
    _fields_ = [("k", C.c_int32), ("n_robots", C.c_int32), ("window_ns", C.c_int64)]


class MeshInfo(C.Structure):
    """kmx_mesh_info_t."""
    _fields_ = [("n_nodes", C.c_int64), ("n_vertices", C.c_int64), ("node_capacity", C.c_int64),
                ("vertex_capacity", C.c_int64), ("device_bytes", C.c_int64), ("k", C.c_int32),
                ("lds_nodes", C.c_int32), ("last_bind_blocks", C.c_int32), ("last_bind_global_blocks", C.c_int32)]


class MeshStats(C.Structure):
    """kmx_mesh_stats."""
    _fields_ = [("n_vertices", C.c_int64), ("n_unbound", C.c_int64), ("n_partial", C.c_int64),
                ("max_displacement", C.c_double), ("sum_sq_displacement", C.c_double)]


class SimplifyParams(C.Structure):
    """kmx_simplify_params."""
    _fields_ = [("resolution", C.c_double), ("horizon_ns", C.c_int64), ("n_robots", C.c_int32),
                ("initial_slots", C.c_int32)]


class SimplifyInfo(C.Structure):
    """kmx_simplify_info_t."""
    _fields_ = [("n_vertices", C.c_int64), ("n_faces_in", C.c_int64), ("n_control", C.c_int64),
                ("n_faces_kept", C.c_int64), ("vertex_slots", C.c_int64), ("face_slots", C.c_int64),
                ("device_bytes", C.c_int64), ("vertex_rehashes", C.c_int32), ("face_rehashes", C.c_int32),
                ("scan_span", C.c_int32), ("scan_span2", C.c_int32)]


class DgraphParams(C.Structure):
    """kmx_dgraph_params (0 in a field: the library's default; rel_tol < 0: its default)."""
    _fields_ = [("lambda_init", C.c_double), ("lambda_factor", C.c_double), ("lambda_min", C.c_double),
                ("lambda_max", C.c_double), ("rel_tol", C.c_double), ("abs_tol", C.c_double), ("cg_rtol", C.c_double),
                ("max_iterations", C.c_int32), ("cg_max_iterations", C.c_int32), ("check_every", C.c_int32),
                ("reserved", C.c_int32)]


class DgraphResult(C.Structure):
    """kmx_dgraph_result."""
    _fields_ = [("cost_initial", C.c_double), ("cost_final", C.c_double), ("lambda_final", C.c_double),
                ("gradnorm_initial", C.c_double), ("iterations", C.c_int32), ("accepted", C.c_int32),
                ("stop_reason", C.c_int32), ("cg_iterations", C.c_int32)]


class DgraphLogEntry(C.Structure):
    """kmx_dgraph_log_entry: one per outer iteration."""
    _fields_ = [("cost", C.c_double), ("trial_cost", C.c_double), ("lam", C.c_double),
                ("cg_iterations", C.c_int32), ("accepted", C.c_int32)]


KMX_DGRAPH_EVAL_COST, KMX_DGRAPH_EVAL_GRAD, KMX_DGRAPH_EVAL_JTJ, KMX_DGRAPH_EVAL_BLOCKS = 0, 1, 2, 3
DGRAPH_STOP = {1: "rel_tol", 2: "abs_tol", 3: "max_iterations", 4: "lambda_max", 5: "zero_gradient"}

_lib = None


def lib() -> C.CDLL:
    """Load libkmx.so (once). Raises KmxError when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = Path(os.environ.get("KMX_LIB", _LIB_PATH))
    if not path.exists():
        raise KmxError(
            f"HIP library {path} not found: build it with `make -C kimera-multi_amd/csrc` "
            "(or __graft_entry__.build()). There is no CPU fallback.")
    L = C.CDLL(str(path))
    P, i32, i64, f64, u8 = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_uint8
    pi32, pf64, pu8, pi64 = C.POINTER(i32), C.POINTER(f64), C.POINTER(u8), C.POINTER(i64)
    sig = {
        "kmx_last_error": ([], C.c_char_p),
        "kmx_abi_version": ([], C.c_int),
        "kmx_device_count": ([C.POINTER(C.c_int)], C.c_int),
        "kmx_pgo_create": ([C.POINTER(PgoParams), C.c_int, C.POINTER(P)], C.c_int),
        "kmx_pgo_destroy": ([P], C.c_int),
        "kmx_pgo_set_stream": ([P, P], C.c_int),
        "kmx_pgo_set_tcg_poll": ([P, C.c_int], C.c_int),
        "kmx_pgo_get_tcg_groups": ([P, C.POINTER(C.c_int), pi32], C.c_int),
        "kmx_pgo_get_group_reduction": ([P, C.POINTER(C.c_int)], C.c_int),
        "kmx_comm_unique_id": ([P, i64], C.c_int),
        "kmx_runtime_info": ([C.c_char_p, i64], C.c_int),
        "kmx_pgo_comm_init": ([P, P, C.c_int, C.c_int, f64], C.c_int),
        "kmx_pgo_comm_destroy": ([P], C.c_int),
        "kmx_pgo_get_public": ([P, pf64, pf64], C.c_int),
        "kmx_pgo_set_exchange": ([P, pi32, pi64, pi32, pi64], C.c_int),
        "kmx_pgo_exchange": ([P], C.c_int),
        "kmx_pgo_set_graph": ([P, C.c_int, pi32, pu8, i64, pi32, pi32, pi32, pi32,
                               pf64, pf64, pf64, pf64, pf64, pu8], C.c_int),
        "kmx_pgo_set_iterate": ([P, C.c_int, pf64], C.c_int),
        "kmx_pgo_get_iterate": ([P, C.c_int, pf64], C.c_int),
        "kmx_pgo_public_count": ([P, pi64, pi64, pi64], C.c_int),
        "kmx_pgo_pack_public": ([P, P], C.c_int),
        "kmx_pgo_unpack_public": ([P, P], C.c_int),
        "kmx_pgo_refresh_local": ([P], C.c_int),
        "kmx_pgo_gather_public_rows": ([P, P, i64, P], C.c_int),
        "kmx_pgo_scatter_public_rows": ([P, P, i64, P], C.c_int),
        "kmx_pgo_exchange_pack": ([P, P, i64, P, C.c_int, P], C.c_int),
        "kmx_pgo_exchange_unpack": ([P, P, i64, P, C.c_int, P], C.c_int),
        "kmx_pgo_set_neighbor_poses": ([P, i64, pi32, pi32, pf64], C.c_int),
        "kmx_pgo_iterate": ([P, pu8, C.POINTER(IterStats)], C.c_int),
        "kmx_pgo_iterate_async": ([P, C.c_int, C.c_int], C.c_int),
        "kmx_pgo_sync": ([P], C.c_int),
        "kmx_pgo_sync_timeout": ([P, f64], C.c_int),
        "kmx_pgo_debug_step_stamps": ([P, i64], C.c_int),
        "kmx_pgo_update_weights": ([P, pf64], C.c_int),
        "kmx_pgo_get_mu": ([P, pf64], C.c_int),
        "kmx_pgo_set_mu": ([P, f64], C.c_int),
        "kmx_pgo_set_gnc_schedule": ([P, C.c_int, C.c_int, C.c_int, f64], C.c_int),
        "kmx_pgo_get_gnc_state": ([P, C.POINTER(GncState)], C.c_int),
        "kmx_pgo_set_gnc_state": ([P, C.POINTER(GncState)], C.c_int),
        "kmx_pgo_get_status": ([P, pf64], C.c_int),
        "kmx_pgo_set_status": ([P, pf64], C.c_int),
        "kmx_pgo_memory": ([P, pi64, C.POINTER(C.c_int)], C.c_int),
        "kmx_pgo_get_weights": ([P, pf64], C.c_int),
        "kmx_pgo_set_weights": ([P, pf64], C.c_int),
        "kmx_pgo_shared_count": ([P, pi64], C.c_int),
        "kmx_pgo_pack_shared_weights": ([P, P], C.c_int),
        "kmx_pgo_unpack_shared_weights": ([P, P], C.c_int),
        "kmx_pgo_get_trajectory": ([P, C.c_int, pf64, pf64], C.c_int),
        "kmx_pgo_eval": ([P, C.c_int, C.c_int, pf64, pf64, pf64], C.c_int),
        "kmx_pgo_local_edges": ([P, C.c_int, pi64], C.c_int),
        "kmx_pgo_enable_timing": ([P, C.c_int], C.c_int),
        "kmx_pgo_read_counters": ([P, C.POINTER(PgoCounters)], C.c_int),
    }
    pu32 = C.POINTER(C.c_uint32)
    sig.update({
        "kmx_lcd_knn2": ([C.c_int, C.c_double, pu8, i32, pu8, i32, pi32, pi32], C.c_int),
        "kmx_lcd_create": ([C.POINTER(LcdParams), C.c_int, C.POINTER(P)], C.c_int),
        "kmx_lcd_destroy": ([P], C.c_int),
        "kmx_lcd_set_stream": ([P, P], C.c_int),
        "kmx_lcd_set_frames": ([P, P], C.c_int),
        "kmx_lcd_add_frames": ([P, i32, i32, pi32, pu8, pf64, pf64, pi32], C.c_int),
        "kmx_lcd_pool_info": ([P, pi32, pi32, pi32], C.c_int),
        "kmx_lcd_match": ([P, i32, pi32, pi32, pi32, pi32], C.c_int),
        "kmx_lcd_verify": ([P, i32, pi32, pi32, C.POINTER(LcdResult), pu8], C.c_int),
        "kmx_lcd_verify_async": ([P, i32, pi32, pi32], C.c_int),
        "kmx_lcd_verify_matches": ([P, i32, pi32, pi32, pi64, pi32, pi32, C.c_int, pf64,
                                    C.POINTER(LcdResult), pu8], C.c_int),
        "kmx_lcd_sync": ([P], C.c_int),
        "kmx_lcd_enable_timing": ([P, C.c_int], C.c_int),
        "kmx_lcd_read_timing": ([P, pf64, pf64], C.c_int),
        "kmx_bow_create": ([C.c_int, C.POINTER(P)], C.c_int),
        "kmx_bow_destroy": ([P], C.c_int),
        "kmx_bow_set_stream": ([P, P], C.c_int),
        "kmx_bow_set_database": ([P, i32, i32, pi64, pu32, pf64], C.c_int),
        "kmx_bow_query": ([P, i32, pi64, pu32, pf64, pi32, i32, pi32, pi32, pf64], C.c_int),
        "kmx_bow_query_async": ([P, i32, pi64, pu32, pf64, pi32, i32], C.c_int),
        "kmx_bow_sync": ([P], C.c_int),
        "kmx_bow_score_pairs": ([P, i32, pi64, pu32, pf64, pi64, pu32, pf64, pf64], C.c_int),
        "kmx_bow_reset": ([P, i32], C.c_int),
        "kmx_bow_add_entries": ([P, i32, pi64, pu32, pf64, pi32], C.c_int),
        "kmx_bow_add_from_voc": ([P, P, pi32, pi32], C.c_int),
        "kmx_bow_seal": ([P], C.c_int),
        "kmx_bow_set_tail_cap": ([P, i32], C.c_int),
        "kmx_bow_info": ([P, pi32, pi32, pi32, pi32, pi64, pi64], C.c_int),
        "kmx_bow_get_entries": ([P, i32, i32, pi64, pu32, pf64, i64], C.c_int),
        "kmx_bow_query_entries": ([P, P, i32, pi32, pi32, i32, pi32, pi32, pf64], C.c_int),
        "kmx_bow_query_entries_async": ([P, P, i32, pi32, pi32, i32], C.c_int),
        "kmx_bow_fetch": ([P, i32, i32, pi32, pi32, pf64], C.c_int),
        "kmx_bow_score_entries": ([P, i32, pi32, pi32, pf64], C.c_int),
        "kmx_bow_detect_entries": ([P, P, i32, pi32, i32, C.POINTER(BowDetectParams), C.POINTER(BowDetectRecord),
                                    pi32, pi32], C.c_int),
        "kmx_bow_detect_entries_async": ([P, P, i32, pi32, i32, C.POINTER(BowDetectParams)], C.c_int),
        "kmx_bow_detect_fetch": ([P, i32, C.POINTER(BowDetectRecord), pi32, pi32], C.c_int),
        "kmx_bow_decide_results": ([P, i32, i32, pi32, pi32, pi32, pf64, pf64, pi32, i32,
                                    C.POINTER(BowDetectParams), i32, C.POINTER(BowDetectRecord)], C.c_int),
        "kmx_bow_get_temporal_state": ([P, pi32], C.c_int),
        "kmx_bow_set_temporal_state": ([P, pi32], C.c_int),
        "kmx_bow_enable_timing": ([P, C.c_int], C.c_int),
        "kmx_bow_read_detect_timing": ([P, pf64], C.c_int),
        "kmx_voc_create": ([C.c_int, i32, pi32, pu8, pf64, i32, pi32, C.c_int, C.POINTER(P)], C.c_int),
        "kmx_voc_destroy": ([P], C.c_int),
        "kmx_voc_set_stream": ([P, P], C.c_int),
        "kmx_voc_info": ([P, pi32, pi32, pi32, pi32, pi32, pi32], C.c_int),
        "kmx_voc_transform": ([P, i32, i32, pi32, pu8, pi32, pu32, pf64], C.c_int),
        "kmx_voc_transform_pool": ([P, P, i32, pi32, pi32, pu32, pf64], C.c_int),
        "kmx_voc_transform_async": ([P, i32, i32, pi32, pu8], C.c_int),
        "kmx_voc_transform_pool_async": ([P, P, i32, pi32], C.c_int),
        "kmx_voc_sync": ([P], C.c_int),
        "kmx_voc_enable_timing": ([P, C.c_int], C.c_int),
        "kmx_voc_read_timing": ([P, pf64, pf64], C.c_int),
        "kmx_chordal_create": ([C.c_int, C.POINTER(P)], C.c_int),
        "kmx_chordal_destroy": ([P], C.c_int),
        "kmx_chordal_set_stream": ([P, P], C.c_int),
        "kmx_chordal_set_graph": ([P, i32, i32, pi32, i64, pi32, pi32, pf64, pf64, pf64, pf64, pf64, i32, pi32],
                                  C.c_int),
        "kmx_chordal_set_weights": ([P, pf64], C.c_int),
        "kmx_chordal_solve": ([P, C.POINTER(ChordalParams), pf64, pf64, pf64, pf64, C.POINTER(ChordalBlockInfo)],
                              C.c_int),
        "kmx_chordal_get_timing": ([P, pf64], C.c_int),
        "kmx_chordal_residuals": ([P, pf64, pf64, pf64, C.c_double, C.POINTER(C.c_uint8), pf64, pf64], C.c_int),
        "kmx_chordal_solve_robust": ([P, C.POINTER(ChordalParams), C.POINTER(ChordalRobustParams),
                                      C.POINTER(C.c_uint8), pf64, pf64, pf64, pf64, pf64,
                                      C.POINTER(ChordalBlockInfo), C.POINTER(ChordalRobustInfo)], C.c_int),
        "kmx_chordal_get_robust_stats": ([P, pf64], C.c_int),
        "kmx_cert_create": ([C.c_int, C.POINTER(P)], C.c_int),
        "kmx_cert_destroy": ([P], C.c_int),
        "kmx_cert_set_stream": ([P, P], C.c_int),
        "kmx_cert_set_graph": ([P, i32, i64, pi32, pi32, pf64, pf64, pf64, pf64, pf64], C.c_int),
        "kmx_cert_set_weights": ([P, pf64], C.c_int),
        "kmx_cert_set_point": ([P, i32, pf64, C.POINTER(CertPointInfo)], C.c_int),
        "kmx_cert_get_lambda": ([P, pf64], C.c_int),
        "kmx_cert_apply": ([P, pf64, pf64], C.c_int),
        "kmx_cert_min_eig": ([P, C.POINTER(CertParams), C.POINTER(CertResult), pf64], C.c_int),
        "kmx_cert_get_coefficients": ([P, i32, pf64, pf64, pi32], C.c_int),
        "kmx_cert_ritz": ([i32, pf64, pf64, f64, C.POINTER(CertResult)], C.c_int),
        "kmx_cert_start_vector": ([C.c_uint64, i64, pf64], C.c_int),
        "kmx_cert_get_timing": ([P, pf64], C.c_int),
        "kmx_cert_get_host_timing": ([P, pf64], C.c_int),
        "kmx_cert_escape": ([P, pf64, i32, pf64, pf64, pi32], C.c_int),
        "kmx_cert_escape_commit": ([P, i32, pf64, C.POINTER(CertPointInfo)], C.c_int),
        "kmx_cert_get_escape_timing": ([P, pf64], C.c_int),
        "kmx_mesh_create": ([C.POINTER(MeshParams), C.c_int, C.POINTER(P)], C.c_int),
        "kmx_mesh_destroy": ([P], C.c_int),
        "kmx_mesh_set_stream": ([P, P], C.c_int),
        "kmx_mesh_info": ([P, C.POINTER(MeshInfo), pi64, pi64], C.c_int),
        "kmx_mesh_add_nodes": ([P, i64, pi32, pi64, pf64, pf64], C.c_int),
        "kmx_mesh_set_node_poses": ([P, i64, i64, pf64, pf64], C.c_int),
        "kmx_mesh_add_vertices": ([P, i64, pi32, pi64, C.POINTER(C.c_float), pi64], C.c_int),
        "kmx_mesh_bind": ([P, i64, i64], C.c_int),
        "kmx_mesh_get_bindings": ([P, i64, i64, pi32, pf64, pi32], C.c_int),
        "kmx_mesh_deform": ([P, i64, i64, C.POINTER(C.c_float), C.POINTER(MeshStats)], C.c_int),
        "kmx_mesh_deform_device": ([P, i64, i64, P], C.c_int),
        "kmx_mesh_sync": ([P], C.c_int),
        "kmx_mesh_enable_timing": ([P, C.c_int], C.c_int),
        "kmx_mesh_read_timing": ([P, pf64, pf64], C.c_int),
        "kmx_dgraph_create": ([C.c_int, C.POINTER(P)], C.c_int),
        "kmx_dgraph_destroy": ([P], C.c_int),
        "kmx_dgraph_set_stream": ([P, P], C.c_int),
        "kmx_dgraph_set_graph": ([P, i32, pf64, pf64, i64, pi32, pi32, pf64], C.c_int),
        "kmx_dgraph_set_weights": ([P, pf64], C.c_int),
        "kmx_dgraph_set_priors": ([P, pu8, pf64, pf64, pf64, pf64], C.c_int),
        "kmx_dgraph_set_poses": ([P, pf64, pf64], C.c_int),
        "kmx_dgraph_get_poses": ([P, pf64, pf64], C.c_int),
        "kmx_dgraph_eval": ([P, i32, pf64, pf64], C.c_int),
        "kmx_dgraph_solve": ([P, C.POINTER(DgraphParams), C.POINTER(DgraphResult)], C.c_int),
        "kmx_dgraph_get_log": ([P, i32, C.POINTER(DgraphLogEntry), pi32], C.c_int),
        "kmx_dgraph_get_timing": ([P, pf64], C.c_int),
        "kmx_simplify_create": ([C.POINTER(SimplifyParams), C.c_int, C.POINTER(P)], C.c_int),
        "kmx_simplify_destroy": ([P], C.c_int),
        "kmx_simplify_set_stream": ([P, P], C.c_int),
        "kmx_simplify_sync": ([P], C.c_int),
        "kmx_simplify_info": ([P, C.POINTER(SimplifyInfo)], C.c_int),
        "kmx_simplify_add": ([P, i64, pi32, pi64, C.POINTER(C.c_float), i64, pi32, pi64, pi64], C.c_int),
        "kmx_simplify_get_control": ([P, i64, i64, pf64, pi64, pi32, pi32], C.c_int),
        "kmx_simplify_get_vertex_map": ([P, i64, i64, pi32], C.c_int),
        "kmx_simplify_get_faces": ([P, i64, i64, pi32], C.c_int),
        "kmx_simplify_edges": ([P, pi64], C.c_int),
        "kmx_simplify_get_edges": ([P, pi32], C.c_int),
        "kmx_simplify_graph": ([P, i32, pi64, pi64, f64, f64, pi32, pi32, pf64, pi64, pi64], C.c_int),
        "kmx_simplify_enable_timing": ([P, C.c_int], C.c_int),
        "kmx_simplify_read_timing": ([P, pf64, pf64, pf64], C.c_int),
    })
    for name, (argt, rest) in sig.items():
        if not hasattr(L, name):
            raise KmxError(f"{path} lacks the entry point {name}: rebuild it")
        fn = getattr(L, name)
        fn.argtypes = argt
        fn.restype = rest
    if L.kmx_abi_version() != ABI_VERSION:
        raise KmxError(f"{path} implements ABI {L.kmx_abi_version()}, this binding needs {ABI_VERSION}: rebuild it")
    _lib = L
    return L


def check(rc: int, what: str = "") -> None:
    if rc != KMX_OK:
        msg = lib().kmx_last_error().decode(errors="replace")
        raise KmxError(f"{what} failed ({rc}): {msg}")


def device_count() -> int:
    n = C.c_int(0)
    check(lib().kmx_device_count(C.byref(n)), "kmx_device_count")
    return n.value


def fptr(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags.c_contiguous, (a.dtype, a.flags)
    return a.ctypes.data_as(C.POINTER(C.c_double))


def iptr(a: np.ndarray):
    assert a.dtype == np.int32 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def i64ptr(a: np.ndarray):
    assert a.dtype == np.int64 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def f32ptr(a: np.ndarray):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_float))


def u32ptr(a: np.ndarray):
    assert a.dtype == np.uint32 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def u8ptr(a: np.ndarray):
    assert a.dtype == np.uint8 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def runtime_info() -> dict:
    """Where libkmx's RCCL / HIP calls resolve in this process, with versions
    (kmx_runtime_info), plus every librccl / libamdhip64 mapped into the
    process (/proc/self/maps): torch ships a librccl.so.1 of the same SONAME,
    so which copy serves kmx depends on load order."""
    import json
    buf = C.create_string_buffer(4096)
    check(lib().kmx_runtime_info(buf, 4096), "kmx_runtime_info")
    info = json.loads(buf.value.decode())
    import re
    mapped = {"librccl": set(), "libamdhip64": set()}
    # the core libraries only, by basename (librccl.so, librccl.so.1, ...): an
    # RCCL plugin such as librccl-net.so is not a second copy of RCCL
    core = {k: re.compile(rf"^{k}\.so(\.\d+)*$") for k in mapped}
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                parts = line.split()
                if len(parts) >= 6:
                    path = parts[-1]
                    for k in mapped:
                        if core[k].match(os.path.basename(path)):
                            mapped[k].add(os.path.realpath(path))
    except OSError:
        pass
    info["mapped_rccl"] = sorted(mapped["librccl"])
    info["mapped_hip"] = sorted(mapped["libamdhip64"])
    info["rccl_path_real"] = os.path.realpath(info["rccl_path"]) if info["rccl_path"] != "?" else "?"
    info["single_rccl"] = len(info["mapped_rccl"]) <= 1 and (
        not info["mapped_rccl"] or info["rccl_path_real"] in info["mapped_rccl"])
    return info
