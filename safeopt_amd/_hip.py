"""ctypes binding of libsafeopt_hip.so (include/safeopt_hip.h).

There is NO CPU fallback: every numerical entry point of the package goes
through this module, and a missing library or a missing GPU raises.
"""
from __future__ import annotations

import ctypes as C
import itertools
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SAFEOPT_HIP_LIB: another build of the same library, for same-box A/B runs)
LIB_PATH = os.environ.get("SAFEOPT_HIP_LIB") or os.path.join(_HERE, "libsafeopt_hip.so")

c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)
c_i32_p = C.POINTER(C.c_int32)
c_u32_p = C.POINTER(C.c_uint32)
c_i64_p = C.POINTER(C.c_int64)
c_u8_p = C.POINTER(C.c_uint8)
vp = C.c_void_p
vpp = C.POINTER(C.c_void_p)
# host-side collectives a caller may plug in (sgp_comm_init_host)
HOST_ALLREDUCE_F64 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int)
HOST_ALLREDUCE_I32 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.c_int)
HOST_ALLGATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)

RBF, MATERN32, MATERN52 = 0, 1, 2
Q, S, M, G, MEAN, VAR, CAND, WIDTH, VAR_H = 0, 1, 2, 3, 4, 5, 6, 7, 8
ARGMAX_MG_WIDTH, ARGMAX_UCB, ARGMAX_LCB = 0, 1, 2
SWARM_TYPES = {"greedy": 0, "maximizers": 1, "expanders": 2, "safe_set": 3}
MAX_D, MAX_PARTS, MAX_GPS, TOPK = 8, 4, 8, 16
MAX_JOINT = 8192          # SGP_MAX_JOINT: rows of one joint prediction
MAX_PATHS = 64            # SGP_MAX_PATHS: sample paths of one call
MAX_FEATURES = 16384      # SGP_MAX_FEATURES: random Fourier features of a sample path
MAX_BATCH = 64            # SGP_MAX_BATCH: query points of one hallucinated batch
MAX_BLOCK = 16            # SGP_MAX_BLOCK: observations of one block append
MAX_MES = 64              # SGP_MAX_MES: maxima of one max-value entropy search
MES_ALL, MES_S, MES_MG = 0, 1, 2                        # candidate rows of sgp_grid_mes
MES_FLOOR_NONE, MES_FLOOR_MEAN, MES_FLOOR_VALUE = 0, 1, 2
EI_EI, EI_PI = 0, 1                                     # kind of sgp_ei_eval / sgp_grid_ei
EI_TAU_MEAN, EI_TAU_VALUE = 1, 2                        # the incumbent of sgp_grid_ei
MAX_ISE = 4096            # SGP_MAX_ISE: candidates of one information-theoretic safe exploration
ISE_UNSAFE, ISE_ALL = 0, 1                              # the rows z of sgp_grid_ise

# name -> (restype, argtypes); mirrors include/safeopt_hip.h one to one
PROTOTYPES = {
    "sgp_device_count": (C.c_int, [c_int_p]),
    "sgp_create": (C.c_int, [C.c_int, vpp]),
    "sgp_destroy": (None, [vp]),
    "sgp_last_error": (C.c_char_p, [vp]),
    "sgp_sync": (C.c_int, [vp]),
    "sgp_gp_create": (C.c_int, [vp, C.c_int, C.c_int, c_int_p, c_double_p,
                                c_double_p, C.c_double, vpp]),
    "sgp_gp_destroy": (None, [vp]),
    "sgp_gp_set_data": (C.c_int, [vp, c_double_p, c_double_p, C.c_int64,
                                  c_int_p, c_double_p]),
    "sgp_gp_set_hyper": (C.c_int, [vp, c_double_p, c_double_p, C.c_double,
                                   c_int_p, c_double_p]),
    "sgp_gp_lml": (C.c_int, [vp, c_double_p, c_double_p, C.c_double, c_double_p,
                             c_int_p]),
    "sgp_gp_loo": (C.c_int, [vp, c_double_p, c_double_p, c_double_p, c_int_p]),
    "sgp_gp_loo_lml": (C.c_int, [vp, c_double_p, c_double_p, C.c_double, c_double_p,
                                 c_int_p]),
    "sgp_gp_append": (C.c_int, [vp, c_double_p, C.c_double, c_int_p]),
    "sgp_gp_append_block": (C.c_int, [vp, c_double_p, c_double_p, C.c_int, c_int_p]),
    "sgp_gp_pop": (C.c_int, [vp]),
    "sgp_gp_remove": (C.c_int, [vp, C.c_int64, c_int_p]),
    "sgp_gp_set_data_w": (C.c_int, [vp, c_double_p, c_double_p, c_double_p, C.c_int64,
                                    c_int_p, c_double_p]),
    "sgp_gp_append_w": (C.c_int, [vp, c_double_p, C.c_double, c_double_p, c_int_p]),
    "sgp_gp_append_block_w": (C.c_int, [vp, c_double_p, c_double_p, c_double_p, C.c_int,
                                        c_int_p]),
    "sgp_gp_reweigh": (C.c_int, [vp, C.c_int64, C.c_double, C.c_double, c_int_p]),
    "sgp_gp_get_noise_scale": (C.c_int, [vp, c_double_p]),
    "sgp_gp_predict": (C.c_int, [vp, c_double_p, C.c_int64, C.c_int64,
                                 C.c_int64, c_double_p, c_double_p]),
    "sgp_gp_predict_cov": (C.c_int, [vp, c_double_p, C.c_int64, C.c_int64,
                                     C.c_int64, c_double_p, c_double_p]),
    "sgp_gp_posterior_draw": (C.c_int, [vp, c_double_p, C.c_int64, C.c_int64,
                                        C.c_int64, c_double_p, C.c_int, c_double_p,
                                        c_double_p, c_int_p, c_double_p]),
    "sgp_gp_path_weights": (C.c_int, [vp, c_double_p, c_double_p, C.c_int, c_double_p,
                                      c_double_p, C.c_int, c_double_p]),
    "sgp_gp_paths_eval": (C.c_int, [vp, c_double_p, c_double_p, C.c_int, c_double_p,
                                    c_double_p, C.c_int, c_double_p, C.c_int64, C.c_int64,
                                    C.c_int64, c_double_p]),
    "sgp_grid_paths": (C.c_int, [vp, vp, c_double_p, c_double_p, C.c_int, c_double_p,
                                 c_double_p, C.c_int, C.c_int, c_double_p, c_double_p,
                                 c_i64_p]),
    "sgp_grid_paths_comm": (C.c_int, [vp, vp, c_double_p, c_double_p, C.c_int, c_double_p,
                                      c_double_p, C.c_int, C.c_int, c_double_p, c_double_p,
                                      c_i64_p]),
    "sgp_mes_eval": (C.c_int, [vp, c_double_p, c_double_p, C.c_int64, c_double_p, C.c_int,
                               C.c_double, c_double_p]),
    "sgp_grid_mes": (C.c_int, [vp, c_double_p, C.c_int, C.c_int, C.c_int, C.c_double,
                               c_double_p, c_double_p, c_i64_p, c_double_p]),
    "sgp_grid_mes_comm": (C.c_int, [vp, c_double_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                    c_double_p, c_double_p, c_i64_p, c_double_p]),
    "sgp_ei_eval": (C.c_int, [vp, c_double_p, c_double_p, C.c_int64, C.c_int, c_double_p,
                              C.c_int, C.c_double, C.c_double, c_double_p]),
    "sgp_grid_ei": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                              c_double_p, c_double_p, c_double_p, c_i64_p, c_double_p]),
    "sgp_grid_ei_comm": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                   c_double_p, c_double_p, c_double_p, c_i64_p, c_double_p]),
    "sgp_ise_eval": (C.c_int, [vp, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int64,
                               C.c_double, c_double_p]),
    "sgp_grid_ise": (C.c_int, [vp, vpp, C.c_int, c_double_p, c_i64_p, C.c_int, C.c_int,
                               c_double_p, c_i64_p, c_double_p, c_i64_p, c_double_p,
                               c_double_p]),
    "sgp_grid_ise_at": (C.c_int, [vp, vpp, C.c_int, c_double_p, c_i64_p, c_double_p, c_double_p,
                                  C.c_int, C.c_int, c_double_p, c_i64_p, c_double_p, c_i64_p]),
    "sgp_grid_ise_comm": (C.c_int, [vp, vpp, C.c_int, c_double_p, c_i64_p, c_double_p,
                                    c_double_p, C.c_int, C.c_int, c_double_p, c_i64_p,
                                    c_double_p, c_i64_p]),
    "sgp_grid_ise_keys": (C.c_int, [vp, vpp, C.c_int, c_double_p, c_i64_p, c_double_p,
                                    c_double_p]),
    "sgp_grid_ise_hist": (C.c_int, [vp, vpp, C.c_int, c_double_p, C.c_double, C.c_double,
                                    c_u32_p]),
    "sgp_grid_ise_list": (C.c_int, [vp, vpp, C.c_int, c_double_p, C.c_double, C.c_int, c_i64_p,
                                    c_i64_p, c_double_p, c_double_p, c_double_p]),
    "sgp_gp_get_factor": (C.c_int, [vp, c_double_p, c_double_p]),
    "sgp_gp_clone": (C.c_int, [vp, vpp]),
    "sgp_grid_batch_next": (C.c_int, [vp, vpp, C.c_int, C.c_int, C.c_int, C.c_double,
                                      c_double_p, c_i64_p, C.c_int, c_double_p, c_i64_p]),
    "sgp_grid_batch_next_comm": (C.c_int, [vp, vpp, C.c_int, C.c_int, C.c_int, C.c_double,
                                           c_double_p, c_i64_p, C.c_int, C.c_int, c_double_p,
                                           c_i64_p, c_int_p]),
    "sgp_kern_K": (C.c_int, [vp, C.c_int, C.c_int, c_int_p, c_double_p,
                             c_double_p, c_double_p, C.c_int64, c_double_p,
                             C.c_int64, c_double_p]),
    "sgp_grid_create": (C.c_int, [vp, c_double_p, C.c_int64, C.c_int,
                                  C.c_int64, C.c_int64, C.c_int, C.c_int64,
                                  vpp]),
    "sgp_grid_destroy": (None, [vp]),
    "sgp_grid_set_context": (C.c_int, [vp, c_double_p, C.c_int]),
    "sgp_grid_set_axes": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                    c_double_p, c_int_p]),
    "sgp_grid_confidence": (C.c_int, [vp, vpp, C.c_int, C.c_double,
                                      c_double_p, c_double_p]),
    "sgp_grid_posterior": (C.c_int, [vp, vpp, C.c_int]),
    "sgp_grid_rank1_update": (C.c_int, [vp, vpp, C.c_int, c_int_p, C.c_double,
                                        c_double_p, c_double_p]),
    "sgp_grid_rank1_remove": (C.c_int, [vp, vpp, C.c_int, c_int_p, C.c_double,
                                        c_double_p, c_double_p]),
    "sgp_grid_rank1_reweigh": (C.c_int, [vp, vpp, C.c_int, c_int_p, C.c_double,
                                         c_double_p, c_double_p]),
    "sgp_grid_rankb_update": (C.c_int, [vp, vpp, C.c_int, c_int_p, C.c_double,
                                        c_double_p, c_double_p]),
    "sgp_grid_upload_Q": (C.c_int, [vp, c_double_p, c_double_p, c_double_p]),
    "sgp_grid_maximizers": (C.c_int, [vp, C.c_double, c_double_p]),
    "sgp_grid_candidates": (C.c_int, [vp, C.c_double, c_double_p, c_double_p,
                                      C.c_int, c_i64_p]),
    "sgp_grid_topk": (C.c_int, [vp, C.c_int, C.c_double, C.c_int64, C.c_int,
                                c_double_p, c_i64_p, c_int_p]),
    "sgp_grid_gather_rows": (C.c_int, [vp, c_i64_p, C.c_int, c_double_p,
                                       c_double_p, c_double_p, c_double_p]),
    "sgp_grid_expander_check": (C.c_int, [vp, vpp, C.c_int, C.c_double,
                                          c_double_p, C.c_int, c_double_p,
                                          c_double_p, c_double_p, C.c_double,
                                          c_i32_p]),
    "sgp_grid_lipschitz_check": (C.c_int, [vp, C.c_int, c_double_p,
                                           c_double_p, C.c_int, c_double_p,
                                           c_double_p, c_i32_p]),
    "sgp_grid_sets_front": (C.c_int, [vp, C.c_double, C.c_int, C.c_double,
                                      c_double_p, c_double_p, c_double_p,
                                      c_double_p, c_double_p, c_double_p]),
    "sgp_grid_sets_front_comm": (C.c_int, [vp, c_double_p, c_double_p,
                                           c_double_p, c_double_p, c_double_p,
                                           c_double_p, c_double_p]),
    "sgp_grid_sets_fused": (C.c_int, [vp, vpp, C.c_int, C.c_double, c_double_p,
                                      C.c_double, c_double_p, c_double_p,
                                      C.c_double, c_double_p, c_double_p,
                                      c_double_p, c_double_p, c_i32_p,
                                      c_double_p, c_i64_p, c_double_p]),
    "sgp_grid_expander_batch": (C.c_int, [vp, vpp, C.c_int, C.c_double, c_double_p, C.c_int,
                                          C.c_double, C.c_int64, C.c_int, c_double_p, c_i64_p,
                                          c_int_p, c_i32_p]),
    "sgp_grid_expander_pass": (C.c_int, [vp, vpp, C.c_int, C.c_double, c_double_p, C.c_int,
                                         C.c_double, C.c_int64, C.c_double, C.c_double, C.c_int,
                                         c_double_p, c_double_p]),
    "sgp_grid_lipschitz_pass": (C.c_int, [vp, C.c_int, c_double_p, c_double_p, C.c_int, C.c_double,
                                          C.c_int64, C.c_double, C.c_double, C.c_int, c_double_p,
                                          c_double_p]),
    "sgp_grid_pass_lipschitz_test": (C.c_int, [vp, C.c_int, c_double_p, c_double_p, C.c_int,
                                               c_double_p, c_double_p, c_i32_p]),
    "sgp_grid_expanders_small_all": (C.c_int, [vp, vpp, C.c_int, C.c_double, c_double_p, C.c_int,
                                               C.POINTER(C.c_int), c_i64_p, c_double_p, c_i32_p]),
    "sgp_grid_pass_hist": (C.c_int, [vp, C.c_int, C.c_double, C.c_int64, C.c_double, C.c_double,
                                     c_u32_p]),
    "sgp_grid_pass_list": (C.c_int, [vp, C.c_int, C.c_double, C.c_int64, C.c_double, C.c_int,
                                     c_int_p, c_i64_p, c_double_p, c_double_p, c_double_p]),
    "sgp_grid_pass_test": (C.c_int, [vp, vpp, C.c_int, C.c_double, c_double_p, C.c_int,
                                     c_double_p, c_double_p, c_i32_p]),
    "sgp_grid_step_small": (C.c_int, [vp, vpp, C.c_int, C.c_double, c_double_p, c_double_p,
                                      c_double_p, c_double_p, c_double_p, c_double_p,
                                      c_double_p, c_i32_p, c_double_p, c_i64_p, c_double_p]),
    "sgp_grid_step_small_ok": (C.c_int, [vp, vpp, C.c_int]),
    "sgp_grid_step_small_many": (C.c_int, [vpp, vpp, c_int_p, C.c_int, c_double_p, c_double_p,
                                           c_double_p, c_double_p, c_double_p, c_double_p,
                                           c_double_p, c_double_p, c_i32_p, c_double_p,
                                           c_i64_p, c_double_p]),
    "sgp_grid_expanders_small": (C.c_int, [vp, vpp, C.c_int, C.c_double, c_double_p, c_i64_p,
                                           C.c_int, c_i32_p]),
    "sgp_grid_sets_fused_comm": (C.c_int, [vp, vpp, C.c_int, C.c_double, c_double_p,
                                           c_double_p, c_double_p, C.c_double,
                                           c_double_p, c_double_p, c_double_p,
                                           c_double_p, c_i32_p, c_double_p, c_i64_p,
                                           c_double_p]),
    "sgp_grid_sets_back": (C.c_int, [vp, vpp, C.c_int, C.c_double, c_double_p,
                                     c_double_p, c_double_p, c_double_p,
                                     C.c_double, C.c_int64, C.c_int,
                                     c_double_p, c_i32_p, c_double_p,
                                     c_i64_p]),
    "sgp_grid_mark_expanders": (C.c_int, [vp, c_i64_p, C.c_int]),
    "sgp_grid_unmark_expanders": (C.c_int, [vp, c_i64_p, C.c_int]),
    "sgp_grid_argmax": (C.c_int, [vp, C.c_int, c_double_p, c_double_p,
                                  c_i64_p]),
    "sgp_grid_download": (C.c_int, [vp, C.c_int, vp]),
    "sgp_grid_upload_mask": (C.c_int, [vp, C.c_int, c_u8_p]),
    "sgp_swarm_fitness": (C.c_int, [vp, vpp, C.c_int, C.c_int, c_double_p,
                                    C.c_int64, C.c_double, c_double_p,
                                    c_double_p, C.c_double, c_double_p,
                                    c_u8_p]),
    "sgp_swarm_fitness_path": (C.c_int, [vp, vpp, C.c_int, c_double_p, C.c_int64,
                                         C.c_double, c_double_p, c_double_p,
                                         c_double_p, c_double_p, C.c_int, c_double_p,
                                         c_double_p, c_double_p, c_u8_p]),
    "sgp_swarm_fitness_hall": (C.c_int, [vp, vpp, vpp, C.c_int, C.c_int, c_double_p,
                                         C.c_int64, C.c_double, c_double_p,
                                         c_double_p, C.c_double, c_double_p,
                                         c_u8_p, c_double_p]),
    "sgp_swarm_fitness_mes": (C.c_int, [vp, vpp, C.c_int, c_double_p, C.c_int64,
                                        C.c_double, c_double_p, c_double_p,
                                        c_double_p, C.c_int, C.c_double, c_double_p,
                                        c_u8_p, c_double_p]),
    "sgp_swarm_fitness_ise": (C.c_int, [vp, vpp, C.c_int, c_double_p, C.c_int64,
                                        C.c_double, c_double_p, c_double_p,
                                        c_double_p, c_double_p, c_double_p, C.c_int,
                                        c_double_p, c_u8_p, c_double_p, c_i64_p, c_double_p,
                                        c_double_p, c_double_p]),
    "sgp_swarm_fitness_ei": (C.c_int, [vp, vpp, C.c_int, c_double_p, C.c_int64,
                                       C.c_double, c_double_p, c_double_p,
                                       C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                                       c_double_p, c_u8_p, c_double_p, c_double_p]),
    "sgp_swarm_grow": (C.c_int, [vp, vp, c_double_p, C.c_int64, c_double_p,
                                 C.c_int64, C.c_double, C.c_double, c_u8_p]),
    "sgp_swarm_run": (C.c_int, [vp, vpp, C.c_int, C.c_int, C.c_double,
                                c_double_p, c_double_p, C.c_double, C.c_int64,
                                c_double_p, c_double_p, c_double_p, c_double_p,
                                c_double_p, c_double_p, c_double_p, C.c_int,
                                C.c_int, C.c_double, C.c_double, c_double_p,
                                C.c_uint64]),
    "sgp_swarm_run_hall": (C.c_int, [vp, vpp, vpp, C.c_int, C.c_int, C.c_double,
                                     c_double_p, c_double_p, C.c_double, C.c_int64,
                                     c_double_p, c_double_p, c_double_p, c_double_p,
                                     c_double_p, c_double_p, c_double_p, C.c_int,
                                     C.c_int, C.c_double, C.c_double, c_double_p,
                                     C.c_uint64]),
    "sgp_swarm_run_hall_shard": (C.c_int, [vp, vpp, vpp, C.c_int, C.c_int, C.c_double,
                                           c_double_p, c_double_p, C.c_double, C.c_int64,
                                           c_double_p, c_double_p, c_double_p, c_double_p,
                                           c_double_p, c_double_p, c_double_p, C.c_int,
                                           C.c_int, C.c_double, C.c_double, c_double_p,
                                           C.c_uint64, C.c_int64, C.c_int64]),
    "sgp_swarm_run_mes": (C.c_int, [vp, vpp, C.c_int, C.c_double,
                                    c_double_p, c_double_p, C.c_int64,
                                    c_double_p, c_double_p, c_double_p, c_double_p,
                                    c_double_p, c_double_p, c_double_p, C.c_int,
                                    C.c_int, C.c_double, C.c_double, c_double_p,
                                    C.c_uint64, c_double_p, C.c_int, C.c_double]),
    "sgp_swarm_run_mes_shard": (C.c_int, [vp, vpp, C.c_int, C.c_double,
                                          c_double_p, c_double_p, C.c_int64,
                                          c_double_p, c_double_p, c_double_p, c_double_p,
                                          c_double_p, c_double_p, c_double_p, C.c_int,
                                          C.c_int, C.c_double, C.c_double, c_double_p,
                                          C.c_uint64, c_double_p, C.c_int, C.c_double,
                                          C.c_int64, C.c_int64]),
    "sgp_swarm_run_ise": (C.c_int, [vp, vpp, C.c_int, C.c_double,
                                    c_double_p, c_double_p, C.c_int64,
                                    c_double_p, c_double_p, c_double_p, c_double_p,
                                    c_double_p, c_double_p, c_double_p, C.c_int,
                                    C.c_int, C.c_double, C.c_double, c_double_p,
                                    C.c_uint64, c_double_p, c_double_p, c_double_p, C.c_int]),
    "sgp_swarm_run_ise_shard": (C.c_int, [vp, vpp, C.c_int, C.c_double,
                                          c_double_p, c_double_p, C.c_int64,
                                          c_double_p, c_double_p, c_double_p, c_double_p,
                                          c_double_p, c_double_p, c_double_p, C.c_int,
                                          C.c_int, C.c_double, C.c_double, c_double_p,
                                          C.c_uint64, c_double_p, c_double_p, c_double_p,
                                          C.c_int, C.c_int64, C.c_int64]),
    "sgp_swarm_run_ei": (C.c_int, [vp, vpp, C.c_int, C.c_double,
                                   c_double_p, c_double_p, C.c_int64,
                                   c_double_p, c_double_p, c_double_p, c_double_p,
                                   c_double_p, c_double_p, c_double_p, C.c_int,
                                   C.c_int, C.c_double, C.c_double, c_double_p,
                                   C.c_uint64, C.c_int, C.c_double, C.c_double, C.c_int,
                                   C.c_int]),
    "sgp_swarm_run_ei_shard": (C.c_int, [vp, vpp, C.c_int, C.c_double,
                                         c_double_p, c_double_p, C.c_int64,
                                         c_double_p, c_double_p, c_double_p, c_double_p,
                                         c_double_p, c_double_p, c_double_p, C.c_int,
                                         C.c_int, C.c_double, C.c_double, c_double_p,
                                         C.c_uint64, C.c_int, C.c_double, C.c_double, C.c_int,
                                         C.c_int, C.c_int64, C.c_int64]),
    "sgp_swarm_run_path": (C.c_int, [vp, vpp, C.c_int, C.c_double,
                                     c_double_p, c_double_p, C.c_int64,
                                     c_double_p, c_double_p, c_double_p, c_double_p,
                                     c_double_p, c_double_p, c_double_p, C.c_int,
                                     C.c_int, C.c_double, C.c_double, c_double_p,
                                     C.c_uint64, c_double_p, c_double_p, C.c_int,
                                     c_double_p, c_double_p]),
    "sgp_swarm_run_path_shard": (C.c_int, [vp, vpp, C.c_int, C.c_double,
                                           c_double_p, c_double_p, C.c_int64,
                                           c_double_p, c_double_p, c_double_p, c_double_p,
                                           c_double_p, c_double_p, c_double_p, C.c_int,
                                           C.c_int, C.c_double, C.c_double, c_double_p,
                                           C.c_uint64, c_double_p, c_double_p, C.c_int,
                                           c_double_p, c_double_p, C.c_int64, C.c_int64]),
    "sgp_swarm_run_shard": (C.c_int, [vp, vpp, C.c_int, C.c_int, C.c_double,
                                      c_double_p, c_double_p, C.c_double, C.c_int64,
                                      c_double_p, c_double_p, c_double_p, c_double_p,
                                      c_double_p, c_double_p, c_double_p, C.c_int,
                                      C.c_int, C.c_double, C.c_double, c_double_p,
                                      C.c_uint64, C.c_int64, C.c_int64]),
    "sgp_comm_unique_id": (C.c_int, [vp]),
    "sgp_comm_init": (C.c_int, [vp, vp, C.c_int, C.c_int]),
    "sgp_comm_init_host": (C.c_int, [vp, C.c_int, C.c_int, HOST_ALLREDUCE_F64,
                                     HOST_ALLREDUCE_I32, HOST_ALLGATHER, vp]),
    "sgp_comm_allreduce_max": (C.c_int, [vp, c_double_p, C.c_int]),
    "sgp_comm_allgather": (C.c_int, [vp, vp, vp, C.c_int64]),
    "sgp_comm_barrier": (C.c_int, [vp]),
    "sgp_timer_start": (C.c_int, [vp]),
    "sgp_timer_stop": (C.c_int, [vp, C.POINTER(C.c_float)]),
    "sgp_profile_enable": (C.c_int, [vp, C.c_int]),
    "sgp_profile_read": (C.c_int, [vp, c_double_p, c_i64_p, c_double_p]),
    "sgp_profile_read_last": (C.c_int, [vp, c_double_p]),
    "sgp_ctx_alloc_count": (C.c_int64, [vp]),
    "sgp_comm_count": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "sgp_ctx_set_sweep": (C.c_int, [vp, C.c_int]),
    "sgp_ctx_last_sweep": (C.c_int, [vp]),
    "sgp_ctx_set_share": (C.c_int, [vp, C.c_int]),

}

_lib = None


class _stdout_to_stderr(object):
    """RCCL prints a version banner on stdout when a communicator is created;
    keep stdout clean (bench.py promises exactly one JSON line there)."""

    def __enter__(self):
        import sys
        try:
            sys.stdout.flush()
            self.saved = os.dup(1)
            os.dup2(2, 1)
        except OSError:
            self.saved = None
        return self

    def __exit__(self, *exc):
        if self.saved is not None:
            try:                      # RCCL uses buffered C stdio: flush it
                C.CDLL(None).fflush(None)   # while fd 1 still is stderr
            except Exception:
                pass
            os.dup2(self.saved, 1)
            os.close(self.saved)
        return False


class HipError(RuntimeError):
    """A call into libsafeopt_hip.so failed (HIP / RCCL / argument error)."""


def lib():
    """Load the shared library once; fail loudly if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipError(
                "libsafeopt_hip.so is not built (%s). Run "
                "`python -m safeopt_amd.build`; there is no CPU fallback."
                % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def device_count():
    n = C.c_int(0)
    lib().sgp_device_count(C.byref(n))
    return n.value


def dptr(a):
    return a.ctypes.data_as(c_double_p)


def f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


class Context(object):
    """One device context (stream, scratch, optional RCCL communicator)."""

    _default = {}

    def __init__(self, device=0):
        L = lib()
        if device_count() <= device:
            raise HipError("no HIP device %d visible: %s -- the HIP path is "
                           "the only path" % (device, L.sgp_last_error(None).decode()))
        h = vp()
        rc = L.sgp_create(device, C.byref(h))
        if rc != 0:
            raise HipError(L.sgp_last_error(None).decode())
        self.h = h
        self.device = device
        self.rank, self.world = 0, 1
        self.sweep_forced = any(os.environ.get(k) for k in
                                ("SGP_SWEEP", "SGP_NO_TINY", "SGP_NO_STEP_SMALL"))

    @classmethod
    def default(cls, device=None):
        if device is None:
            device = int(os.environ.get("SAFEOPT_HIP_DEVICE",
                                        os.environ.get("LOCAL_RANK", "0")))
            n = device_count()
            world = int(os.environ.get("LOCAL_WORLD_SIZE",
                                       os.environ.get("WORLD_SIZE", "1")))
            if n > 0 and device >= n:
                shared = os.environ.get("SAFEOPT_COMM", "rccl") == "socket"
                if world > 1 and "SAFEOPT_HIP_DEVICE" not in os.environ and not shared:
                    # two ranks on one GPU: RCCL would fail or hang in
                    # ncclCommInitRank -- say what is wrong instead
                    raise HipError(
                        "LOCAL_RANK %d but only %d visible GPU(s): one process per "
                        "GPU (launch with --nproc-per-node <= %d, or set "
                        "SAFEOPT_HIP_DEVICE explicitly)" % (device, n, n))
                device %= n
        if device not in cls._default:
            cls._default[device] = Context(device)
        return cls._default[device]

    def check(self, rc):
        if rc != 0:
            raise HipError("libsafeopt_hip (rc=%d): %s"
                           % (rc, lib().sgp_last_error(self.h).decode()))

    def sync(self):
        self.check(lib().sgp_sync(self.h))

    # -- measurement
    def timer_start(self):
        self.check(lib().sgp_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float(0)
        self.check(lib().sgp_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def profile_enable(self, on=True):
        self.check(lib().sgp_profile_enable(self.h, int(bool(on))))

    def profile_read(self):
        ms, n, fl = C.c_double(0), C.c_int64(0), C.c_double(0)
        self.check(lib().sgp_profile_read(self.h, C.byref(ms), C.byref(n),
                                          C.byref(fl)))
        return ms.value, n.value, fl.value

    def profile_read_last(self):
        """Milliseconds of the last timed launch alone (``sgp_profile_read_last``)."""
        ms = C.c_double(0)
        self.check(lib().sgp_profile_read_last(self.h, C.byref(ms)))
        return ms.value

    def alloc_count(self):
        """Device allocations made so far (a warm loop must not add any)."""
        return int(lib().sgp_ctx_alloc_count(self.h))

    def comm_count(self):
        """Ranks of the RCCL communicator (ncclCommCount); 1 without one."""
        n = C.c_int(0)
        self.check(lib().sgp_comm_count(self.h, C.byref(n)))
        return n.value

    def set_share(self, on):
        """GPs with identical inputs / kernel / noise share the variance contraction
        of the sweep (default on); returns the previous setting."""
        return bool(lib().sgp_ctx_set_share(self.h, int(bool(on))))

    def set_sweep(self, which):
        """Posterior-sweep kernel: 'auto' | 'classic' (4 waves) | 'pair' (paired
        waves) | 'mid' (= auto: the resident-factor kernel where it applies, which
        'classic' and 'pair' switch off), '-nosplit' appended: remainder tiles are not cut into runs of
        chunks, '-notables': no factor tables on tensor grids (set_axes), '-streamed':
        small factors go through the 4-wave kernel's double buffer instead of staying
        in LDS for the launch, '-unmerged': the paired kernel runs one j-block per stage
        (the schedule until round 5; merged stages: csrc/sweep_pair.hip), '-nohand': GPs
        with the inputs and kernel of the GP in front evaluate their own covariances
        instead of receiving the leader's (csrc/sweep_pair.hip, "hand-down"); or the integer
        of sgp_ctx_set_sweep.  Returns the
        previous setting (a name)."""
        names = ("auto", "classic", "pair", "mid", "auto-nosplit", "classic-nosplit",
                 "pair-nosplit", None)
        names = names + tuple(n + "-notables" if n else None for n in names)
        names = names + tuple(n + "-streamed" if n else None for n in names)
        names = names + tuple(n + "-unmerged" if n else None for n in names)
        names = names + tuple(n + "-nohand" if n else None for n in names)

        def code(w):          # a name, or the integer of sgp_ctx_set_sweep
            return int(w) if isinstance(w, (int, np.integer)) else names.index(w)

        old = names[int(lib().sgp_ctx_set_sweep(self.h, code(which)))]
        #: a sweep kernel is forced (A/B runs, tests): no one-launch step of small grids
        # (3 = 'mid' counts too: step_small_eligible in csrc/step_small.hip refuses every
        # non-zero choice, the driver must not pick the one-launch step then)
        self.sweep_forced = (code(which) & 3) != 0
        return old

    def last_sweep(self):
        """Kernel of the last posterior sweep: 'classic' | 'pair' | 'tiny' | 'few-points' |
        'step-small' | 'mid'."""
        return (None, "classic", "pair", "tiny", "few-points",
                "step-small", "mid")[int(lib().sgp_ctx_last_sweep(self.h)) & 255]

    def step_small_many(self, plan):
        """One ``sgp_grid_step_small_many`` call on the members of ``plan`` (a
        :class:`FleetPlan` of this context, its inputs filled in): the B one-launch steps
        side by side.  The results are in the plan's arrays."""
        rc = plan.fn(*plan.args)
        if rc != 0:
            self.check(rc)

    def last_sweep_handed(self):
        """Did the last posterior sweep hand covariances from a GP to GPs with the same
        inputs and kernel (the paired kernel's hand-down, csrc/sweep_pair.hip)?"""
        return bool(int(lib().sgp_ctx_last_sweep(self.h)) & 256)

    # -- RCCL
    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(128)
        with _stdout_to_stderr():
            rc = lib().sgp_comm_unique_id(buf)
        if rc != 0:
            raise HipError(lib().sgp_last_error(None).decode())
        return buf.raw

    def comm_init(self, uid, rank, world):
        buf = C.create_string_buffer(uid, 128)
        with _stdout_to_stderr():
            rc = lib().sgp_comm_init(self.h, buf, rank, world)
        self.check(rc)
        self.rank, self.world = rank, world

    def comm_init_host(self, comm):
        """The caller's collectives as this context's transport (``sgp_comm_init_host``):
        ``comm`` has ``rank``, ``world``, ``allreduce_max(array)`` and ``allgather(array)``
        on host arrays (``dist.SocketComm``).  The N-rank entry points then stage their
        device operands through the host around these calls."""
        def _guard(fn):
            def run(*a):
                try:
                    fn(*a)
                    return 0
                except Exception:           # noqa -- nothing may unwind through the C frames
                    import traceback
                    traceback.print_exc()
                    return 1
            return run

        def ar_f64(_user, buf, n):
            a = np.ctypeslib.as_array(buf, shape=(n,))
            a[:] = comm.allreduce_max(a.copy())

        def ar_i32(_user, buf, n):
            a = np.ctypeslib.as_array(buf, shape=(n,))
            # (flags / small counts: exact in float64)
            a[:] = comm.allreduce_max(a.astype(np.float64)).astype(np.int32)

        def ag(_user, send, recv, nbytes):
            raw = C.string_at(send, nbytes)
            parts = comm.allgather(np.frombuffer(raw, dtype=np.uint8))
            C.memmove(recv, np.ascontiguousarray(parts).ctypes.data, nbytes * comm.world)

        # (the ctypes thunks must outlive the context's use of them)
        self._host_cbs = (HOST_ALLREDUCE_F64(_guard(ar_f64)), HOST_ALLREDUCE_I32(_guard(ar_i32)),
                          HOST_ALLGATHER(_guard(ag)))
        self.check(lib().sgp_comm_init_host(self.h, int(comm.rank), int(comm.world),
                                            *self._host_cbs, None))
        self.rank, self.world = int(comm.rank), int(comm.world)

    def allreduce_max(self, a):
        a = f64(a).copy()
        self.check(lib().sgp_comm_allreduce_max(self.h, dptr(a), a.size))
        return a

    def allgather_bytes(self, b):
        out = C.create_string_buffer(len(b) * self.world)
        src = C.create_string_buffer(bytes(b), len(b))
        self.check(lib().sgp_comm_allgather(self.h, src, out, len(b)))
        return out.raw

    def barrier(self):
        self.check(lib().sgp_comm_barrier(self.h))

    def mes_eval(self, mean, var, ystar, floor=-np.inf):
        """Max-value entropy search acquisition at arbitrary points (``sgp_mes_eval``): the
        posterior ``mean`` / ``var`` of the objective there, the maxima ``ystar`` (K) and a
        ``floor`` under them (-inf: none) -> alpha, in the shape of ``mean``."""
        mean, var, ystar = f64(mean), f64(var), f64(ystar).reshape(-1)
        if mean.shape != var.shape:
            raise ValueError("mean %r and var %r differ in shape" % (mean.shape, var.shape))
        out = np.empty(mean.shape)
        self.check(lib().sgp_mes_eval(self.h, dptr(mean), dptr(var), mean.size, dptr(ystar),
                                      int(ystar.size), float(floor), dptr(out)))
        return out

    def ei_eval(self, mean, var, tau, xi=0.0, kind=EI_EI, fmin=None):
        """Log expected improvement (``kind=EI_EI``) or log probability of improvement
        (``EI_PI``) at arbitrary points (``sgp_ei_eval``): the posterior ``mean`` / ``var`` there,
        ``(G, N)`` with the objective in row 0 (or ``(N,)`` for the objective alone), the
        incumbent ``tau`` and the margin ``xi`` -> alpha ``(N,)``, a natural logarithm.
        ``fmin`` (G): every GP with a finite entry adds the log probability that it lies above
        it; ``None``: no weights."""
        mean, var = f64(mean), f64(var)
        if mean.shape != var.shape:
            raise ValueError("mean %r and var %r differ in shape" % (mean.shape, var.shape))
        if mean.ndim > 2:
            raise ValueError("mean must be (G, N) or (N,), got %r" % (mean.shape,))
        G, N = (int(mean.shape[0]), int(mean.shape[1])) if mean.ndim == 2 else (1, int(mean.size))
        if fmin is not None:
            fmin = f64(fmin).reshape(-1)
            if fmin.size != G:
                raise ValueError("%d fmin for %d GPs" % (fmin.size, G))
        out = np.empty(N)
        self.check(lib().sgp_ei_eval(self.h, dptr(mean), dptr(var), N, G,
                                     None if fmin is None else dptr(fmin), int(kind), float(tau),
                                     float(xi), dptr(out)))
        return out

    def ise_eval(self, mu, vz, vx, c, s):
        """The term of information-theoretic safe exploration at arbitrary points
        (``sgp_ise_eval``): ``mu = mean(z) - fmin``, the variances ``vz`` at ``z`` and ``vx``
        at the measured point, their posterior covariance ``c`` -- arrays of one shape -- and
        the noise variance ``s`` of a measurement -> the approximate mutual information in
        nats, in that shape."""
        mu, vz, vx, c = f64(mu), f64(vz), f64(vx), f64(c)
        if not (mu.shape == vz.shape == vx.shape == c.shape):
            raise ValueError("mu %r, vz %r, vx %r and c %r differ in shape"
                             % (mu.shape, vz.shape, vx.shape, c.shape))
        out = np.empty(mu.shape)
        self.check(lib().sgp_ise_eval(self.h, dptr(mu), dptr(vz), dptr(vx), dptr(c), mu.size,
                                      float(s), dptr(out)))
        return out

    def kern_K(self, kdesc, X1, X2):
        d, kinds, variances, inv_ls = kdesc
        X1 = f64(X1).reshape(-1, d)
        X2 = f64(X2).reshape(-1, d)
        out = np.empty((X1.shape[0], X2.shape[0]))
        if out.size:
            self.check(lib().sgp_kern_K(
                self.h, d, len(kinds), kinds.ctypes.data_as(c_int_p),
                dptr(variances), dptr(inv_ls), dptr(X1), X1.shape[0],
                dptr(X2), X2.shape[0], dptr(out)))
        return out


def _gp_array(gps):
    arr = (vp * len(gps))(*[g.h for g in gps])
    return C.cast(arr, vpp)


class FleetPlan(object):
    """The arguments of ``sgp_grid_step_small_many`` for a fixed list of grids, built once:
    handle arrays, packed inputs and outputs, and their pointers.  Per step the caller
    writes ``beta[b]`` and the rows ``fmin[b]`` / ``scaling[b]`` / ``thr_beta[b]``, calls
    ``set_gps(b, gps)`` (a no-op while the handles stay) and ``Context.step_small_many``;
    ``result(b, value, gidx, max_l)`` is then what ``DeviceGrid.step_small`` returns for
    member ``b``, as views of the packed arrays."""

    def __init__(self, ctx, grids):
        B = len(grids)
        self.ctx, self.grids, self.B = ctx, list(grids), B
        self.grid_arr = (vp * B)(*[g.h for g in grids])
        self.gp_arr = (vp * (B * MAX_GPS))()
        self.G = (C.c_int * B)(*[g.G for g in grids])
        self.beta = np.zeros(B)
        self.fmin = np.full((B, MAX_GPS), -np.inf)
        self.scaling = np.ones((B, MAX_GPS))
        self.thr_beta = np.zeros((B, MAX_GPS))
        self.out5 = np.zeros((B, 6))
        self.x = np.zeros((B, MAX_D))
        self.mean = np.zeros((B, MAX_GPS))
        self.q = np.zeros((B, 2 * MAX_GPS))
        self.flags = np.zeros((B, MAX_GPS), dtype=np.int32)
        self.value = np.zeros(B)
        self.gidx = np.zeros(B, dtype=np.int64)
        self.max_l = np.zeros(B)
        self._keys = [None] * B
        self.rows = [(self.fmin[b, :g.G], self.scaling[b, :g.G], self.thr_beta[b, :g.G])
                     for b, g in enumerate(grids)]
        self._views = [(self.out5[b], self.x[b, :g.d], self.mean[b, :g.G], self.q[b, :2 * g.G],
                        self.flags[b, :g.G]) for b, g in enumerate(grids)]
        self.fn = lib().sgp_grid_step_small_many
        self.args = (C.cast(self.grid_arr, vpp), C.cast(self.gp_arr, vpp), self.G, B,
                     dptr(self.beta), dptr(self.fmin), dptr(self.scaling), dptr(self.thr_beta),
                     dptr(self.out5), dptr(self.x), dptr(self.mean), dptr(self.q),
                     self.flags.ctypes.data_as(c_i32_p), dptr(self.value),
                     self.gidx.ctypes.data_as(c_i64_p), dptr(self.max_l))

    def set_gps(self, b, gps):
        key = tuple(g.h.value for g in gps)
        if self._keys[b] != key:
            self._keys[b] = key
            for i in range(MAX_GPS):
                self.gp_arr[b * MAX_GPS + i] = gps[i].h if i < len(gps) else None

    def result(self, b, value, gidx, max_l):
        return self._views[b] + (value, gidx, max_l)


class DeviceGP(object):
    """Device-resident GP state (training data, packed L^-1, alpha)."""

    _serials = itertools.count(1)      # process-wide, never reused

    def __init__(self, ctx, kdesc, noise_var):
        d, kinds, variances, inv_ls = kdesc
        self.ctx = ctx
        self.d = d
        h = vp()
        ctx.check(lib().sgp_gp_create(
            ctx.h, d, len(kinds), kinds.ctypes.data_as(c_int_p),
            dptr(variances), dptr(inv_ls), float(noise_var), C.byref(h)))
        self.h = h
        self.n_parts = len(kinds)
        self.n = 0
        self.jitter = 0.0
        # data version: bumped by every change; `appended` = the last change
        # was a one-row append whose rank-1 record is on the device, `removed` =
        # it was the removal of one row (`remove`), likewise
        self.version = 0
        self.appended = False
        self.removed = False
        # ... `reweighed` = it re-weighted one observation in place (`reweigh`), likewise
        self.reweighed = False
        # ... `block` = b > 0: it was a block append of b rows (`append_block`) whose block
        # record is on the device
        self.block = 0
        self.serial = next(DeviceGP._serials)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().sgp_gp_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _scales(self, noise_scale, rows):
        """``noise_scale`` as ``rows`` float64 values, or None (all ones, the code without
        scales).  Refused here, before anything is written: a scale that is not finite or
        not positive."""
        if noise_scale is None:
            return None
        r = np.ascontiguousarray(np.broadcast_to(f64(noise_scale).reshape(-1), (rows,)))
        if not (np.all(np.isfinite(r)) and np.all(r > 0)):
            raise ValueError("noise scales must be finite and positive, got %r" % (r,))
        return r

    def set_data(self, X, Y, noise_scale=None):
        """Fit to ``(X, Y)``; ``noise_scale``: one scale ``r_i > 0`` per observation, its
        noise variance is ``(noise_var + 1e-8) r_i`` (None: all ones)."""
        X = f64(X).reshape(-1, self.d)
        Y = f64(Y).reshape(-1)
        r = self._scales(noise_scale, X.shape[0])
        info, jit = C.c_int(0), C.c_double(0)
        if r is None:
            rc = lib().sgp_gp_set_data(self.h, dptr(X), dptr(Y), X.shape[0],
                                       C.byref(info), C.byref(jit))
        else:
            rc = lib().sgp_gp_set_data_w(self.h, dptr(X), dptr(Y), dptr(r), X.shape[0],
                                         C.byref(info), C.byref(jit))
        if rc > 0 or info.value != 0:
            raise np.linalg.LinAlgError(
                lib().sgp_last_error(self.ctx.h).decode())
        self.ctx.check(rc)
        self.n = X.shape[0]
        self.jitter = jit.value
        self.version += 1
        self.appended = self.removed = self.reweighed = False
        self.block = 0

    def _hyper(self, variances, inv_ls):
        variances = f64(variances).reshape(-1)
        inv_ls = f64(inv_ls).reshape(-1)
        if variances.size != self.n_parts or inv_ls.size != self.n_parts * self.d:
            raise ValueError("hyper-parameters of %d parts on %d columns expected"
                             % (self.n_parts, self.d))
        return variances, inv_ls

    def set_hyper(self, variances, inv_ls, noise_var):
        """New hyper-parameters for the resident data: the descriptor is rewritten in
        place and the data are factorised again (no allocation, no upload); jitter and
        ``LinAlgError`` as ``set_data``."""
        variances, inv_ls = self._hyper(variances, inv_ls)
        info, jit = C.c_int(0), C.c_double(0)
        rc = lib().sgp_gp_set_hyper(self.h, dptr(variances), dptr(inv_ls),
                                    float(noise_var), C.byref(info), C.byref(jit))
        self.version += 1
        self.appended = self.removed = self.reweighed = False
        self.block = 0
        if rc > 0 or info.value != 0:
            self.n = 0
            raise np.linalg.LinAlgError(
                lib().sgp_last_error(self.ctx.h).decode())
        self.ctx.check(rc)
        self.jitter = jit.value

    def lml(self, variances, inv_ls, noise_var):
        """``(log p(y | X, theta), d/d noise_var, d/d variance[P], d/d inv_ls[P, d],
        info)`` in one round trip; the GP is left fitted at theta when ``info == 0``
        (no jitter), unfitted -- data resident -- otherwise."""
        variances, inv_ls = self._hyper(variances, inv_ls)
        P, d = self.n_parts, self.d
        out = np.empty(2 + P + P * d)
        info = C.c_int(0)
        self.version += 1
        self.appended = self.removed = self.reweighed = False
        self.block = 0
        self.ctx.check(lib().sgp_gp_lml(self.h, dptr(variances), dptr(inv_ls),
                                        float(noise_var), dptr(out), C.byref(info)))
        self.jitter = 0.0
        return (float(out[0]), float(out[1]), out[2:2 + P].copy(),
                out[2 + P:].reshape(P, d).copy(), int(info.value))

    def loo_lml(self, variances, inv_ls, noise_var):
        """``(L_LOO, d/d noise_var, d/d variance[P], d/d inv_ls[P, d], info)``: the
        leave-one-out log pseudo-likelihood and its gradient at theta, the 5-tuple and the
        contract of ``lml`` (``sgp_gp_loo_lml``)."""
        variances, inv_ls = self._hyper(variances, inv_ls)
        P, d = self.n_parts, self.d
        out = np.empty(2 + P + P * d)
        info = C.c_int(0)
        self.version += 1
        self.appended = self.removed = self.reweighed = False
        self.block = 0
        self.ctx.check(lib().sgp_gp_loo_lml(self.h, dptr(variances), dptr(inv_ls),
                                            float(noise_var), dptr(out), C.byref(info)))
        self.jitter = 0.0
        return (float(out[0]), float(out[1]), out[2:2 + P].copy(),
                out[2 + P:].reshape(P, d).copy(), int(info.value))

    def loo(self):
        """``(mean, var, sum_log_pred)``: every observation predicted from all the others
        (``(n,)`` each; ``var`` is that of the noisy observation) and the sum of their log
        predictive densities, from the factor as it stands (``sgp_gp_loo``).
        ``LinAlgError`` when a ``(Ky^-1)_ii`` is not positive and finite."""
        mean, var = np.empty(self.n), np.empty(self.n)
        total, info = C.c_double(0), C.c_int(0)
        self.ctx.check(lib().sgp_gp_loo(self.h, dptr(mean), dptr(var), C.byref(total),
                                        C.byref(info)))
        if info.value != 0:
            raise np.linalg.LinAlgError("(Ky^-1)_ii of observation %d is not positive"
                                        % (info.value - 1))
        return mean, var, float(total.value)

    def append(self, x, y, noise_scale=None):
        """One more observation by a bordered update; False = not possible
        (no capacity / pivot not positive): the caller refits with set_data.
        ``noise_scale``: the scale of the new observation (None: 1)."""
        x = f64(x).reshape(self.d)
        r = self._scales(noise_scale, 1)
        info = C.c_int(0)
        if r is None:
            self.ctx.check(lib().sgp_gp_append(self.h, dptr(x), float(y),
                                               C.byref(info)))
        else:
            self.ctx.check(lib().sgp_gp_append_w(self.h, dptr(x), float(y), dptr(r),
                                                 C.byref(info)))
        if info.value != 0:
            return False
        self.n += 1
        self.version += 1
        self.appended, self.removed, self.reweighed = True, False, False
        self.block = 0
        return True

    def append_block(self, X, y, noise_scale=None):
        """``b`` more observations (``1 <= b <= MAX_BLOCK``) by ONE bordered update with a
        ``b x b`` corner (``sgp_gp_append_block``): one read-back and one re-pack instead of
        ``b``.  False = not possible (no capacity / a pivot not positive), the GP is then
        exactly as it was: the caller refits with set_data."""
        X = f64(X).reshape(-1, self.d)
        y = f64(y).reshape(-1)
        b = X.shape[0]
        if y.size != b or not 1 <= b <= MAX_BLOCK:
            raise ValueError("a block of 1..%d rows with one value each, got X %r, y %r"
                             % (MAX_BLOCK, X.shape, y.shape))
        r = self._scales(noise_scale, b)
        info = C.c_int(0)
        if r is None:
            self.ctx.check(lib().sgp_gp_append_block(self.h, dptr(X), dptr(y), b,
                                                     C.byref(info)))
        else:
            self.ctx.check(lib().sgp_gp_append_block_w(self.h, dptr(X), dptr(y), dptr(r), b,
                                                       C.byref(info)))
        if info.value != 0:
            return False
        self.n += b
        self.version += 1
        self.appended = self.removed = self.reweighed = False
        self.block = b
        return True

    def pop(self):
        """Drop the last observation (O(n^2))."""
        self.ctx.check(lib().sgp_gp_pop(self.h))
        self.n -= 1
        self.version += 1
        self.appended = self.removed = self.reweighed = False
        self.block = 0

    def remove(self, index):
        """Forget observation ``index`` (0 .. n-1), whichever it is, by an O(n^2) downdate
        of the factor (``sgp_gp_remove``); False = a pivot of the downdate is not positive:
        the GP is untouched and the caller refits with set_data."""
        info = C.c_int(0)
        self.ctx.check(lib().sgp_gp_remove(self.h, int(index), C.byref(info)))
        if info.value != 0:
            return False
        self.n -= 1
        self.version += 1
        self.appended, self.removed, self.reweighed = False, True, False
        self.block = 0
        return True

    def reweigh(self, index, y, r):
        """Observation ``index`` (0 .. n-1) becomes ``(y, r)`` in place: value ``y``, noise
        scale ``r``, by an O(n^2) update of the factor (``sgp_gp_reweigh``); ``n`` and the
        inputs stay.  False = a pivot of the update is not positive: the GP is untouched
        and the caller refits with set_data.  Refused with nothing written: an index
        outside 0 .. n-1, a value that is not finite, a scale that is not finite or not
        positive."""
        index = int(index)
        if not 0 <= index < self.n:
            raise IndexError("row %d of %d observations" % (index, self.n))
        y = float(y)
        if not np.isfinite(y):
            raise ValueError("the value of an observation must be finite, got %r" % (y,))
        r = float(self._scales(r, 1)[0])
        info = C.c_int(0)
        self.ctx.check(lib().sgp_gp_reweigh(self.h, index, y, r, C.byref(info)))
        if info.value != 0:
            return False
        self.version += 1
        self.appended, self.removed, self.reweighed = False, False, True
        self.block = 0
        return True

    def noise_scale(self):
        """The ``n`` noise scales as the device holds them (ones without scales)."""
        r = np.empty(self.n)
        self.ctx.check(lib().sgp_gp_get_noise_scale(self.h, dptr(r)))
        return r

    def predict(self, Xnew):
        Xnew = np.asarray(Xnew, dtype=np.float64)
        if Xnew.ndim != 2 or Xnew.shape[1] != self.d:
            Xnew = np.atleast_2d(Xnew).reshape(-1, self.d)
        N = Xnew.shape[0]
        it = Xnew.itemsize
        if Xnew.strides[0] % it or Xnew.strides[1] % it or \
                min(Xnew.strides) < 0:
            Xnew = np.ascontiguousarray(Xnew)
        mean = np.empty((N, 1))
        var = np.empty((N, 1))
        if N:
            self.ctx.check(lib().sgp_gp_predict(
                self.h, dptr(Xnew), N, Xnew.strides[0] // it,
                Xnew.strides[1] // it, dptr(mean), dptr(var)))
        return mean, var

    def _joint_rows(self, Xnew):
        Xnew = np.asarray(Xnew, dtype=np.float64)
        if Xnew.ndim != 2 or Xnew.shape[1] != self.d:
            Xnew = np.atleast_2d(Xnew).reshape(-1, self.d)
        it = Xnew.itemsize
        if Xnew.strides[0] % it or Xnew.strides[1] % it or \
                min(Xnew.strides) < 0:
            Xnew = np.ascontiguousarray(Xnew)
        if Xnew.shape[0] > MAX_JOINT:
            raise ValueError("%d rows in one joint prediction: at most SGP_MAX_JOINT = %d"
                             % (Xnew.shape[0], MAX_JOINT))
        return Xnew, Xnew.strides[0] // it, Xnew.strides[1] // it

    def predict_cov(self, Xnew):
        """Joint posterior of the rows of ``Xnew``: mean ``(N, 1)`` and covariance
        ``(N, N)``, exactly symmetric, not clipped."""
        Xnew, sr, sc = self._joint_rows(Xnew)
        N = Xnew.shape[0]
        mean = np.empty((N, 1))
        cov = np.empty((N, N))
        self.ctx.check(lib().sgp_gp_predict_cov(self.h, dptr(Xnew), N, sr, sc,
                                                dptr(mean), dptr(cov)))
        return mean, cov

    def draw(self, Xnew, Z):
        """``(out, mean, jitter_used)``: ``out = mean + C Z`` (N, S) for the caller's
        normals ``Z`` (N, S), ``C`` the Cholesky factor of the joint covariance (+ GPy's
        jitter when it is needed).  ``LinAlgError`` when no jitter makes it positive."""
        Xnew, sr, sc = self._joint_rows(Xnew)
        N = Xnew.shape[0]
        Z = f64(Z)
        if Z.ndim != 2 or Z.shape[0] != N or Z.shape[1] < 1 or N < 1:
            raise ValueError("Z must be (N, S) with N = %d rows and S >= 1, got %r"
                             % (N, Z.shape))
        S = Z.shape[1]
        out = np.empty((N, S))
        mean = np.empty((N, 1))
        info, jit = C.c_int(0), C.c_double(0)
        rc = lib().sgp_gp_posterior_draw(self.h, dptr(Xnew), N, sr, sc, dptr(Z), S, dptr(out),
                                         dptr(mean), C.byref(info), C.byref(jit))
        if rc > 0 or info.value != 0:
            raise np.linalg.LinAlgError(lib().sgp_last_error(self.ctx.h).decode())
        self.ctx.check(rc)
        return out, mean, jit.value

    def _path_args(self, Omega, phase, W):
        Omega = f64(Omega).reshape(-1, self.d)
        m = Omega.shape[0]
        phase = f64(phase).reshape(m)
        W = f64(W)
        if W.ndim != 2 or W.shape[0] != m:
            raise ValueError("W must be (m, S) with m = %d features, got %r" % (m, W.shape))
        return Omega, phase, W, m, W.shape[1]

    def path_weights(self, Omega, phase, W, E):
        """Data weights ``V = alpha - Ky^-1 (Phi(X) W + E)`` (n, S) of sample paths
        (``sgp_gp_path_weights``; safeopt_amd/paths.py has the formulas)."""
        Omega, phase, W, m, S = self._path_args(Omega, phase, W)
        E = f64(E)
        if E.shape != (self.n, S):
            raise ValueError("E must be (n, S) = (%d, %d), got %r" % (self.n, S, E.shape))
        V = np.empty((self.n, S))
        self.ctx.check(lib().sgp_gp_path_weights(self.h, dptr(Omega), dptr(phase), m, dptr(W),
                                                 dptr(E), S, dptr(V)))
        return V

    def paths_eval(self, Omega, phase, W, V, Xnew):
        """The sample paths at the rows of ``Xnew``: ``(N, S)`` (``sgp_gp_paths_eval``)."""
        Omega, phase, W, m, S = self._path_args(Omega, phase, W)
        V = f64(V)
        if V.shape != (self.n, S):
            raise ValueError("V must be (n, S) = (%d, %d), got %r" % (self.n, S, V.shape))
        Xnew = np.asarray(Xnew, dtype=np.float64)
        if Xnew.ndim != 2 or Xnew.shape[1] != self.d:
            Xnew = np.atleast_2d(Xnew).reshape(-1, self.d)
        it = Xnew.itemsize
        if Xnew.strides[0] % it or Xnew.strides[1] % it or min(Xnew.strides) < 0:
            Xnew = np.ascontiguousarray(Xnew)
        N = Xnew.shape[0]
        out = np.empty((N, S))
        self.ctx.check(lib().sgp_gp_paths_eval(
            self.h, dptr(Omega), dptr(phase), m, dptr(W), dptr(V), S, dptr(Xnew), N,
            Xnew.strides[0] // it, Xnew.strides[1] // it, dptr(out)))
        return out

    def clone(self):
        """A second device GP with this one's state (``sgp_gp_clone``): the same bits in the
        data, ``L^-1``, ``alpha`` and the packed operands, and room for ``MAX_BATCH`` more
        appends.  Appending to it, refitting or destroying it leaves this GP alone, and it
        outlives this GP."""
        h = vp()
        self.ctx.check(lib().sgp_gp_clone(self.h, C.byref(h)))
        twin = object.__new__(DeviceGP)
        twin.ctx, twin.d, twin.h = self.ctx, self.d, h
        twin.n_parts, twin.n, twin.jitter = self.n_parts, self.n, self.jitter
        twin.version, twin.appended = self.version, self.appended
        twin.removed = self.removed
        twin.reweighed = self.reweighed
        twin.block = 0            # (a clone carries no block record)
        twin.serial = next(DeviceGP._serials)
        return twin

    def destroy(self):
        """Release the device GP now (a private copy whose owner is done with it)."""
        if getattr(self, "h", None):
            lib().sgp_gp_destroy(self.h)
            self.h = None

    def factor(self):
        Linv = np.empty((self.n, self.n))
        alpha = np.empty(self.n)
        self.ctx.check(lib().sgp_gp_get_factor(self.h, dptr(Linv), dptr(alpha)))
        return Linv, alpha


def tensor_grid_axes(points):
    """``(counts, strides, axis values)`` of an (N, d) array whose rows are a tensor
    grid -- row ``i`` has column ``k`` equal to ``values[k][(i // strides[k]) % counts[k]]``,
    as ``linearly_spaced_combinations`` builds it (safeopt/utilities.py:21-54), constant
    columns (contexts) having one point -- or None.  Necessary conditions only (run
    lengths, periods, the chain of the strides): the device compares every row
    (``DeviceGrid.set_axes``)."""
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[0] < 1:
        return None
    N, d = points.shape
    counts, strides, values = [], [], []
    for k in range(d):
        col = points[:, k]
        change = np.flatnonzero(col[1:] != col[:-1])
        if change.size == 0:
            counts.append(1); strides.append(1); values.append(col[:1].copy())
            continue
        run = int(change[0]) + 1
        firsts = col[::run]
        again = np.flatnonzero(firsts[1:] == firsts[0])
        cnt = int(again[0]) + 1 if again.size else int(firsts.size)
        counts.append(cnt); strides.append(run); values.append(firsts[:cnt].copy())
    total, expect = 1, 1
    for k in sorted((k for k in range(d) if counts[k] > 1), key=lambda k: strides[k]):
        if strides[k] != expect:
            return None
        expect *= counts[k]
        total *= counts[k]
    if total != N or N >= 2 ** 31:
        return None
    return counts, strides, values


class DeviceGrid(object):
    """This rank's shard of SafeOpt.inputs resident in HBM, with Q/S/M/G."""

    def __init__(self, ctx, inputs, G, global_offset=0):
        inputs = np.asarray(inputs, dtype=np.float64)
        assert inputs.ndim == 2
        if min(inputs.strides) < 0:
            inputs = np.ascontiguousarray(inputs)
        self.ctx = ctx
        self.N, self.d = inputs.shape
        self.G = G
        self.goff = int(global_offset)
        h = vp()
        ctx.check(lib().sgp_grid_create(
            ctx.h, dptr(inputs), self.N, self.d, inputs.strides[0],
            inputs.strides[1], G, self.goff, C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().sgp_grid_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_context(self, c):
        c = f64(c).reshape(-1)
        self.ctx.check(lib().sgp_grid_set_context(self.h, dptr(c), c.size))

    def set_axes(self, axes):
        """Declare the rows a tensor grid (``axes`` from ``tensor_grid_axes`` of the
        WHOLE grid, this shard's rows being its rows ``goff .. goff + N``); the device
        checks the declaration against the resident rows.  True when it holds: RBF
        kernels are then swept through per-axis factor tables."""
        if axes is None:
            return False
        counts, strides, values = axes
        cnt = np.ascontiguousarray(counts, dtype=np.int64)
        stv = np.ascontiguousarray(strides, dtype=np.int64)
        vals = f64(np.concatenate([np.asarray(v, dtype=np.float64) for v in values]))
        ok = C.c_int(0)
        self.ctx.check(lib().sgp_grid_set_axes(
            self.h, int(cnt.size), cnt.ctypes.data_as(C.POINTER(C.c_int64)),
            stv.ctypes.data_as(C.POINTER(C.c_int64)), dptr(vals), C.byref(ok)))
        return bool(ok.value)

    def upload_mask(self, what, mask):
        """``S`` / ``M`` / ``G`` of this shard from the host (user code wrote into the mirror)."""
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        assert m.shape == (self.N,)
        self.ctx.check(lib().sgp_grid_upload_mask(self.h, int(what), m.ctypes.data_as(c_u8_p)))

    def clear_axes(self):
        """Forget the tensor-grid declaration (the sweeps evaluate covariances again)."""
        one = np.ones(self.d, dtype=np.int64)
        ok = C.c_int(0)
        self.ctx.check(lib().sgp_grid_set_axes(
            self.h, self.d, one.ctypes.data_as(C.POINTER(C.c_int64)),
            one.ctypes.data_as(C.POINTER(C.c_int64)), dptr(np.zeros(self.d)), C.byref(ok)))
        assert not ok.value

    def confidence(self, gps, beta, fmin, defer=False):
        """``defer``: enqueue only; ``max l0[S]`` stays on the device and comes
        back with the next ``sets_fused`` call (returns ``(None, None)``)."""
        fmin = f64(fmin)
        out = np.empty(2)
        self.ctx.check(lib().sgp_grid_confidence(
            self.h, _gp_array(gps), len(gps), float(beta), dptr(fmin),
            None if defer else dptr(out)))
        return (None, None) if defer else (out[0], bool(out[1]))

    def posterior(self, gps):
        """Resident mean / var of every GP from a full sweep; Q, S untouched."""
        self.ctx.check(lib().sgp_grid_posterior(self.h, _gp_array(gps), len(gps)))

    def rank1_update(self, gps, which, beta, fmin, defer=False):
        fmin = f64(fmin)
        w = np.ascontiguousarray(which, dtype=np.int32)
        out = np.empty(2)
        self.ctx.check(lib().sgp_grid_rank1_update(
            self.h, _gp_array(gps), len(gps), w.ctypes.data_as(c_int_p),
            float(beta), dptr(fmin), None if defer else dptr(out)))
        return (None, None) if defer else (out[0], bool(out[1]))

    def rankb_update(self, gps, which, beta, fmin, defer=False):
        """``rank1_update`` after one ``DeviceGP.append_block`` on the GPs of ``which``
        (``b`` from each GP's block record; it may differ per GP)."""
        fmin = f64(fmin)
        w = np.ascontiguousarray(which, dtype=np.int32)
        out = np.empty(2)
        self.ctx.check(lib().sgp_grid_rankb_update(
            self.h, _gp_array(gps), len(gps), w.ctypes.data_as(c_int_p),
            float(beta), dptr(fmin), None if defer else dptr(out)))
        return (None, None) if defer else (out[0], bool(out[1]))

    def rank1_remove(self, gps, which, beta, fmin, defer=False):
        """``rank1_update`` after one ``DeviceGP.remove`` on the GPs of ``which``."""
        fmin = f64(fmin)
        w = np.ascontiguousarray(which, dtype=np.int32)
        out = np.empty(2)
        self.ctx.check(lib().sgp_grid_rank1_remove(
            self.h, _gp_array(gps), len(gps), w.ctypes.data_as(c_int_p),
            float(beta), dptr(fmin), None if defer else dptr(out)))
        return (None, None) if defer else (out[0], bool(out[1]))

    def rank1_reweigh(self, gps, which, beta, fmin, defer=False):
        """``rank1_update`` after one ``DeviceGP.reweigh`` on the GPs of ``which``."""
        fmin = f64(fmin)
        w = np.ascontiguousarray(which, dtype=np.int32)
        out = np.empty(2)
        self.ctx.check(lib().sgp_grid_rank1_reweigh(
            self.h, _gp_array(gps), len(gps), w.ctypes.data_as(c_int_p),
            float(beta), dptr(fmin), None if defer else dptr(out)))
        return (None, None) if defer else (out[0], bool(out[1]))

    def upload_Q(self, Qh, fmin):
        Qh = f64(Qh).reshape(self.N, 2 * self.G)
        fmin = f64(fmin)
        out = np.empty(2)
        self.ctx.check(lib().sgp_grid_upload_Q(self.h, dptr(Qh), dptr(fmin),
                                               dptr(out)))
        return out[0], bool(out[1])

    def maximizers(self, max_l):
        out = C.c_double(0)
        self.ctx.check(lib().sgp_grid_maximizers(self.h, float(max_l),
                                                 C.byref(out)))
        return out.value

    def candidates(self, max_var, scaling, thr_beta, full_sets=False):
        scaling = f64(scaling)
        thr_beta = f64(thr_beta)
        counts = np.zeros(2, dtype=np.int64)
        self.ctx.check(lib().sgp_grid_candidates(
            self.h, float(max_var), dptr(scaling), dptr(thr_beta),
            int(bool(full_sets)), counts.ctypes.data_as(c_i64_p)))
        return int(counts[0]), int(counts[1])

    def topk(self, mode, cut_w, cut_idx, k=TOPK):
        w = np.empty(k)
        idx = np.empty(k, dtype=np.int64)
        n = C.c_int(0)
        self.ctx.check(lib().sgp_grid_topk(
            self.h, int(mode), float(cut_w), int(cut_idx), k, dptr(w),
            idx.ctypes.data_as(c_i64_p), C.byref(n)))
        return w[:n.value], idx[:n.value]

    def gather_rows(self, gidx):
        gidx = np.ascontiguousarray(gidx, dtype=np.int64)
        m = gidx.size
        x = np.empty((m, self.d))
        mean = np.empty((m, self.G))
        var = np.empty((m, self.G))
        Qr = np.empty((m, 2 * self.G))
        if m:
            self.ctx.check(lib().sgp_grid_gather_rows(
                self.h, gidx.ctypes.data_as(c_i64_p), m, dptr(x), dptr(mean),
                dptr(var), dptr(Qr)))
        return x, mean, var, Qr

    def expander_check(self, gps, beta, fmin, xc, mu_c, u_c, near_frac=0.0):
        fmin = f64(fmin)
        xc = f64(xc).reshape(-1, self.d)
        m = xc.shape[0]
        mu_c = f64(mu_c).reshape(m, self.G)
        u_c = f64(u_c).reshape(m, self.G)
        flags = np.zeros((m, self.G), dtype=np.int32)
        self.ctx.check(lib().sgp_grid_expander_check(
            self.h, _gp_array(gps), len(gps), float(beta), dptr(fmin), m,
            dptr(xc), dptr(mu_c), dptr(u_c), float(near_frac),
            flags.ctypes.data_as(c_i32_p)))
        return flags

    def expander_batch(self, gps, beta, fmin, mode, cut_w, cut_idx, k):
        """The next ``k`` candidates behind the cut and whether they are expanders (exact
        scan), one device round trip: ``(widths, global indices, flags (m, G))``."""
        fmin = f64(fmin)
        w = np.empty(k)
        idx = np.empty(k, dtype=np.int64)
        n = C.c_int(0)
        flags = np.zeros((k, self.G), dtype=np.int32)
        self.ctx.check(lib().sgp_grid_expander_batch(
            self.h, _gp_array(gps), len(gps), float(beta), dptr(fmin), int(mode),
            float(cut_w), int(cut_idx), int(k), dptr(w), idx.ctypes.data_as(c_i64_p),
            C.byref(n), flags.ctypes.data_as(c_i32_p)))
        return w[:n.value], idx[:n.value], flags[:n.value]

    def expanders_small_all(self, gps, beta, fmin, cap=4096):
        """Every candidate of a small grid tested in one round trip
        (``sgp_grid_expanders_small_all``): ``(global rows in row order, widths, flags (m, G))``,
        or None when there are more than ``cap`` candidates."""
        fmin = f64(fmin)
        cap = int(min(cap, self.N))
        gidx = np.empty(cap, dtype=np.int64)
        width = np.empty(cap)
        flags = np.empty((cap, len(gps)), dtype=np.int32)
        n = C.c_int(0)
        self.ctx.check(lib().sgp_grid_expanders_small_all(
            self.h, _gp_array(gps), len(gps), float(beta), dptr(fmin), cap, C.byref(n),
            gidx.ctypes.data_as(c_i64_p), dptr(width), flags.ctypes.data_as(c_i32_p)))
        if n.value > cap:
            return None
        return gidx[:n.value], width[:n.value], flags[:n.value]

    def expander_pass(self, gps, beta, fmin, mode, cut_w, cut_idx, key_lo, key_hi, want,
                      scaling=None):
        """About ``want`` candidates behind the cut, all tested in one scan of the unsafe rows
        (``sgp_grid_expander_pass``): ``(tested, hits, key, row of the first expander in
        visiting order, key below which candidates are left or -inf, row of the arg-max of the
        step taken behind the test or -1 -- with ``scaling``, ``mode`` 0)``."""
        fmin = f64(fmin)
        sc = None if scaling is None else f64(scaling)
        out = np.zeros(6)
        self.ctx.check(lib().sgp_grid_expander_pass(
            self.h, _gp_array(gps), len(gps), float(beta), dptr(fmin), int(mode), float(cut_w),
            int(cut_idx), float(key_lo), float(key_hi), int(want),
            None if sc is None else dptr(sc), dptr(out)))
        return (int(out[0]), int(out[1]), float(out[2]), int(out[3]), float(out[4]), int(out[5]))

    def lipschitz_pass(self, fmin, lipschitz, mode, cut_w, cut_idx, key_lo, key_hi, want,
                       scaling=None):
        """The same pass with Lipschitz certificates (``sgp_grid_lipschitz_pass``); result as
        ``expander_pass``."""
        fmin, lipschitz = f64(fmin), f64(lipschitz)
        sc = None if scaling is None else f64(scaling)
        out = np.zeros(6)
        self.ctx.check(lib().sgp_grid_lipschitz_pass(
            self.h, len(fmin), dptr(fmin), dptr(lipschitz), int(mode), float(cut_w), int(cut_idx),
            float(key_lo), float(key_hi), int(want), None if sc is None else dptr(sc), dptr(out)))
        return (int(out[0]), int(out[1]), float(out[2]), int(out[3]), float(out[4]), int(out[5]))

    def pass_hist(self, mode, cut_w, cut_idx, key_lo, key_hi):
        """This shard's histogram (4096 bins over [key_lo, key_hi]) of the keys of its
        candidates behind the cut (``sgp_grid_pass_hist``)."""
        hist = np.zeros(4096, dtype=np.uint32)
        self.ctx.check(lib().sgp_grid_pass_hist(
            self.h, int(mode), float(cut_w), int(cut_idx), float(key_lo), float(key_hi),
            hist.ctypes.data_as(c_u32_p)))
        return hist

    def pass_list(self, mode, cut_w, cut_idx, thr, cap):
        """This shard's candidates behind the cut with key >= thr: ``(global rows, keys, rows
        (m, d), u - mu (m, G))`` (``sgp_grid_pass_list``)."""
        cap = max(int(cap), 1)
        gidx = np.empty(cap, dtype=np.int64)
        key = np.empty(cap)
        x = np.empty((cap, self.d))
        resid = np.empty((cap, self.G))
        n = C.c_int(0)
        self.ctx.check(lib().sgp_grid_pass_list(
            self.h, int(mode), float(cut_w), int(cut_idx), float(thr), cap, C.byref(n),
            gidx.ctypes.data_as(c_i64_p), dptr(key), dptr(x), dptr(resid)))
        m = n.value
        return gidx[:m], key[:m], x[:m], resid[:m]

    def pass_test(self, gps, beta, fmin, xc, resid):
        """Flags (K, G): candidate c lifts one of this shard's unsafe rows above fmin_i
        (``sgp_grid_pass_test``)."""
        fmin = f64(fmin)
        xc = f64(xc).reshape(-1, self.d)
        K = xc.shape[0]
        resid = f64(resid).reshape(K, self.G)
        flags = np.zeros((K, self.G), dtype=np.int32)
        if K:
            self.ctx.check(lib().sgp_grid_pass_test(
                self.h, _gp_array(gps), len(gps), float(beta), dptr(fmin), K, dptr(xc),
                dptr(resid), flags.ctypes.data_as(c_i32_p)))
        return flags

    def pass_lipschitz_test(self, fmin, lipschitz, xc, u_c):
        """Flags (K, G) of the Lipschitz test of K gathered candidates against this shard's
        unsafe rows (``sgp_grid_pass_lipschitz_test``)."""
        fmin, lipschitz = f64(fmin), f64(lipschitz)
        xc = f64(xc).reshape(-1, self.d)
        K = xc.shape[0]
        u_c = f64(u_c).reshape(K, self.G)
        flags = np.zeros((K, self.G), dtype=np.int32)
        if K:
            self.ctx.check(lib().sgp_grid_pass_lipschitz_test(
                self.h, self.G, dptr(fmin), dptr(lipschitz), K, dptr(xc), dptr(u_c),
                flags.ctypes.data_as(c_i32_p)))
        return flags

    def lipschitz_check(self, fmin, lipschitz, xc, u_c):
        fmin = f64(fmin)
        lipschitz = f64(lipschitz)
        xc = f64(xc).reshape(-1, self.d)
        m = xc.shape[0]
        u_c = f64(u_c).reshape(m, self.G)
        flags = np.zeros((m, self.G), dtype=np.int32)
        self.ctx.check(lib().sgp_grid_lipschitz_check(
            self.h, self.G, dptr(fmin), dptr(lipschitz), m, dptr(xc),
            dptr(u_c), flags.ctypes.data_as(c_i32_p)))
        return flags

    def sets_front(self, max_l, max_var, scaling, thr_beta):
        scaling = f64(scaling)
        thr_beta = f64(thr_beta)
        out5 = np.empty(6)           # [5] = candidates tied with the first one
        x = np.empty(self.d)
        mean = np.empty(self.G)
        q = np.empty(2 * self.G)
        self.ctx.check(lib().sgp_grid_sets_front(
            self.h, float(max_l), int(max_var is not None),
            0.0 if max_var is None else float(max_var), dptr(scaling),
            dptr(thr_beta), dptr(out5), dptr(x), dptr(mean), dptr(q)))
        return out5, x, mean, q

    def sets_front_comm(self, scaling, thr_beta):
        scaling, thr_beta = f64(scaling), f64(thr_beta)
        out5 = np.empty(6)
        x = np.empty(self.d)
        mean = np.empty(self.G)
        q = np.empty(2 * self.G)
        ml = C.c_double(0)
        self.ctx.check(lib().sgp_grid_sets_front_comm(
            self.h, dptr(scaling), dptr(thr_beta), dptr(out5), dptr(x),
            dptr(mean), dptr(q), C.byref(ml)))
        return out5, x, mean, q, ml.value

    def sets_back(self, gps, beta, fmin, xc, mu_c, u_c, near_frac, gidx_c,
                  scaling, mark=True):
        fmin = f64(fmin)
        scaling = f64(scaling)
        xc, mu_c, u_c = f64(xc), f64(mu_c), f64(u_c)
        flags = np.zeros(self.G, dtype=np.int32)
        v = C.c_double(0)
        i = C.c_int64(0)
        self.ctx.check(lib().sgp_grid_sets_back(
            self.h, _gp_array(gps), len(gps), float(beta), dptr(fmin),
            dptr(xc), dptr(mu_c), dptr(u_c), float(near_frac), int(gidx_c),
            int(bool(mark)), dptr(scaling), flags.ctypes.data_as(c_i32_p),
            C.byref(v), C.byref(i)))
        return flags, v.value, i.value

    def sets_fused(self, gps, beta, fmin, max_l, scaling, thr_beta, near_frac):
        fmin, scaling, thr_beta = f64(fmin), f64(scaling), f64(thr_beta)
        out5 = np.empty(6)           # [5] = candidates tied with the first one
        x = np.empty(self.d)
        mean = np.empty(self.G)
        q = np.empty(2 * self.G)
        flags = np.zeros(self.G, dtype=np.int32)
        v = C.c_double(0)
        i = C.c_int64(0)
        ml = C.c_double(0)
        self.ctx.check(lib().sgp_grid_sets_fused(
            self.h, _gp_array(gps), len(gps), float(beta), dptr(fmin),
            float('nan') if max_l is None else float(max_l), dptr(scaling),
            dptr(thr_beta), float(near_frac), dptr(out5), dptr(x), dptr(mean),
            dptr(q), flags.ctypes.data_as(c_i32_p), C.byref(v), C.byref(i),
            C.byref(ml)))
        return out5, x, mean, q, flags, v.value, i.value, ml.value

    def expanders_small(self, gps, beta, fmin, gidx):
        """Which of the candidate rows ``gidx`` are expanders, per GP: ``(m, G)`` flags in
        one round trip (small grids: ``sgp_grid_expanders_small``)."""
        gidx = np.ascontiguousarray(gidx, dtype=np.int64)
        flags = np.zeros((gidx.size, self.G), dtype=np.int32)
        if gidx.size:
            self.ctx.check(lib().sgp_grid_expanders_small(
                self.h, _gp_array(gps), len(gps), float(beta), dptr(f64(fmin)),
                gidx.ctypes.data_as(c_i64_p), int(gidx.size), flags.ctypes.data_as(c_i32_p)))
        return flags

    def step_small_ok(self, gps):
        """Does ``step_small`` serve this grid with these (fitted) GPs?"""
        return bool(lib().sgp_grid_step_small_ok(self.h, _gp_array(gps), len(gps)))

    def step_small(self, gps, beta, fmin, scaling, thr_beta):
        """A whole ``SafeOpt.optimize()`` of a small grid in one launch and one read-back
        (``sgp_grid_step_small``); returns what ``sets_fused`` returns.  The output
        buffers and their pointers are built once (this is the 30-microsecond path)."""
        ss = self.__dict__.get("_ss")
        if ss is None:
            out5, x, mean, q = np.empty(6), np.empty(self.d), np.empty(self.G), np.empty(2 * self.G)
            flags = np.zeros(self.G, dtype=np.int32)
            v, i, ml = C.c_double(0), C.c_int64(0), C.c_double(0)
            ss = self._ss = dict(
                out=(out5, x, mean, q, flags, v, i, ml),
                ptr=(dptr(out5), dptr(x), dptr(mean), dptr(q), flags.ctypes.data_as(c_i32_p),
                     C.byref(v), C.byref(i), C.byref(ml)),
                fn=lib().sgp_grid_step_small, gps=None, gp_arr=None)
        key = tuple(g.h.value for g in gps)
        if ss["gps"] != key:
            ss["gps"], ss["gp_arr"] = key, _gp_array(gps)
        # (the three input arrays are the optimiser's own attributes: their pointers are
        # looked up once per array object -- the cache holds the arrays, so an id is not reused)
        ins = ss.get("ins")
        if ins is None or ins[0] is not fmin or ins[1] is not scaling or ins[2] is not thr_beta:
            # (f64: the same object back when it already is a contiguous float64 array)
            conv = (f64(fmin), f64(scaling), f64(thr_beta))
            ins = ss["ins"] = (fmin, scaling, thr_beta) + conv + tuple(dptr(a) for a in conv)
        elif ins[3] is not fmin or ins[4] is not scaling:
            # converted copies (an integer fmin, say): their VALUES may have been edited
            ins[3][...], ins[4][...], ins[5][...] = fmin, scaling, thr_beta
        rc = ss["fn"](self.h, ss["gp_arr"], len(gps), float(beta), ins[6], ins[7], ins[8],
                      *ss["ptr"])
        if rc != 0:
            self.ctx.check(rc)
        out5, x, mean, q, flags, v, i, ml = ss["out"]
        return out5, x, mean, q, flags, v.value, i.value, ml.value

    def sets_fused_comm(self, gps, beta, fmin, scaling, thr_beta, near_frac):
        """N-rank certified step in one round trip (merges behind in-stream collectives)."""
        fmin, scaling, thr_beta = f64(fmin), f64(scaling), f64(thr_beta)
        out5 = np.empty(6)
        x = np.empty(self.d)
        mean = np.empty(self.G)
        q = np.empty(2 * self.G)
        flags = np.zeros(self.G, dtype=np.int32)
        v = C.c_double(0)
        i = C.c_int64(0)
        ml = C.c_double(0)
        self.ctx.check(lib().sgp_grid_sets_fused_comm(
            self.h, _gp_array(gps), len(gps), float(beta), dptr(fmin), dptr(scaling),
            dptr(thr_beta), float(near_frac), dptr(out5), dptr(x), dptr(mean),
            dptr(q), flags.ctypes.data_as(c_i32_p), C.byref(v), C.byref(i),
            C.byref(ml)))
        return out5, x, mean, q, flags, v.value, i.value, ml.value

    def mark_expanders(self, gidx):
        gidx = np.ascontiguousarray(gidx, dtype=np.int64)
        if gidx.size:
            self.ctx.check(lib().sgp_grid_mark_expanders(
                self.h, gidx.ctypes.data_as(c_i64_p), gidx.size))

    def unmark_expanders(self, gidx):
        gidx = np.ascontiguousarray(gidx, dtype=np.int64)
        if gidx.size:
            self.ctx.check(lib().sgp_grid_unmark_expanders(
                self.h, gidx.ctypes.data_as(c_i64_p), gidx.size))

    def argmax(self, mode, scaling):
        scaling = f64(scaling)
        v = C.c_double(0)
        i = C.c_int64(0)
        self.ctx.check(lib().sgp_grid_argmax(self.h, int(mode), dptr(scaling),
                                             C.byref(v), C.byref(i)))
        return v.value, i.value

    def batch_next(self, gps, first, mode, beta, scaling, picked):
        """One pick of a hallucinated batch (``sgp_grid_batch_next``): ``gps`` are clones with
        the pending pick appended; ``(value, global row)`` of the best row of the mask that is
        not in ``picked``, ``(-inf, -1)`` when none is left.  ``first``: the downdate starts
        from the resident variances instead of the hallucinated ones (``download(VAR_H)``)."""
        scaling = f64(scaling)
        picked = np.ascontiguousarray(picked, dtype=np.int64).reshape(-1)
        v = C.c_double(0)
        i = C.c_int64(0)
        self.ctx.check(lib().sgp_grid_batch_next(
            self.h, _gp_array(gps), len(gps), int(bool(first)), int(mode), float(beta),
            dptr(scaling), picked.ctypes.data_as(c_i64_p), int(picked.size), C.byref(v),
            C.byref(i)))
        return v.value, i.value

    def batch_next_comm(self, gps, first, mode, beta, scaling, picked, stop=False):
        """``batch_next`` over the shards of all ranks of the context's communicator
        (``sgp_grid_batch_next_comm``): ``(value, global row, stop_any)``, the same on every
        rank -- a collective, every rank calls it.  ``stop``: this rank takes no part in the
        pick (its append failed) and only reports that; ``stop_any``: some rank did."""
        scaling = f64(scaling)
        picked = np.ascontiguousarray(picked, dtype=np.int64).reshape(-1)
        v = C.c_double(0)
        i = C.c_int64(0)
        any_stop = C.c_int(0)
        self.ctx.check(lib().sgp_grid_batch_next_comm(
            self.h, _gp_array(gps), len(gps), int(bool(first)), int(mode), float(beta),
            dptr(scaling), picked.ctypes.data_as(c_i64_p), int(picked.size), int(bool(stop)),
            C.byref(v), C.byref(i), C.byref(any_stop)))
        return v.value, i.value, bool(any_stop.value)

    def paths(self, gp, Omega, phase, W, V, mask=False, values=False, best=True, comm=False):
        """Sample paths of ``gp`` over the resident rows (``sgp_grid_paths``): ``(values (N, S)
        or None, best value (S), its global row (S))`` -- the arg-max over all rows, or over
        the rows of the safe set with ``mask``; -inf / -1 when no row qualifies.  ``comm``:
        ``sgp_grid_paths_comm`` -- the arg-max over the rows of ALL ranks of the context's
        communicator, the same on every rank (``values`` stays this rank's block)."""
        Omega, phase, W, m, S = gp._path_args(Omega, phase, W)
        V = f64(V)
        if V.shape != (gp.n, S):
            raise ValueError("V must be (n, S) = (%d, %d), got %r" % (gp.n, S, V.shape))
        vals = np.empty((self.N, S)) if values else None
        bv = np.empty(S) if best else None
        bi = np.empty(S, dtype=np.int64) if best else None
        call = lib().sgp_grid_paths_comm if comm else lib().sgp_grid_paths
        self.ctx.check(call(
            self.h, gp.h, dptr(Omega), dptr(phase), m, dptr(W), dptr(V), S, int(bool(mask)),
            None if vals is None else dptr(vals), None if bv is None else dptr(bv),
            None if bi is None else bi.ctypes.data_as(c_i64_p)))
        return vals, bv, bi

    def mes(self, ystar, rows=MES_S, floor='mean', alpha=False, comm=False):
        """Max-value entropy search over the resident posterior of GP 0 (``sgp_grid_mes``):
        ``(alpha (N,) or None, value, global row, floor used)`` -- the arg-max of alpha over
        the candidate ``rows`` (``MES_ALL`` / ``MES_S`` / ``MES_MG``), -inf / -1 when no row
        qualifies.  ``floor``: ``'mean'`` (the largest mean of GP 0 over ``S``), ``None``, or
        a float.  ``comm``: ``sgp_grid_mes_comm`` -- floor and arg-max
        over the rows of ALL ranks of the context's communicator, the same on every rank
        (``alpha`` stays this rank's block); a collective."""
        ystar = f64(ystar).reshape(-1)
        if floor is None:
            mode, fv = MES_FLOOR_NONE, 0.0
        elif isinstance(floor, str):
            if floor != 'mean':
                raise ValueError("floor must be 'mean', None or a float, got %r" % (floor,))
            mode, fv = MES_FLOOR_MEAN, 0.0
        else:
            mode, fv = MES_FLOOR_VALUE, float(floor)
        al = np.empty(self.N) if alpha else None
        v, i, fu = C.c_double(0), C.c_int64(0), C.c_double(0)
        call = lib().sgp_grid_mes_comm if comm else lib().sgp_grid_mes
        self.ctx.check(call(self.h, dptr(ystar), int(ystar.size), int(rows), mode, fv,
                            None if al is None else dptr(al), C.byref(v), C.byref(i),
                            C.byref(fu)))
        return al, v.value, i.value, fu.value

    def ei(self, kind=EI_EI, rows=MES_S, tau='mean', xi=0.0, fmin=None, alpha=False,
           comm=False):
        """Log expected improvement / log probability of improvement over the resident posterior
        (``sgp_grid_ei``): ``(alpha (N,) or None, value, global row, tau used)`` -- the arg-max
        of alpha over the candidate ``rows`` (``MES_ALL`` / ``MES_S`` / ``MES_MG``), -inf / -1
        when no row qualifies.  ``tau``: ``'mean'`` (the largest mean of GP 0 over ``S``) or a
        finite float.  ``fmin`` (G) or ``None``: the feasibility weights.  ``comm``:
        ``sgp_grid_ei_comm`` -- incumbent and arg-max over the rows of ALL ranks of the
        context's communicator, the same on every rank (``alpha`` stays this rank's block); a
        collective."""
        if isinstance(tau, str):
            if tau != 'mean':
                raise ValueError("tau must be 'mean' or a float, got %r" % (tau,))
            mode, tv = EI_TAU_MEAN, 0.0
        else:
            mode, tv = EI_TAU_VALUE, float(tau)
        if fmin is not None:
            fmin = f64(fmin).reshape(-1)
            if fmin.size != self.G:
                raise ValueError("%d fmin for %d GPs" % (fmin.size, self.G))
        al = np.empty(self.N) if alpha else None
        v, i, tu = C.c_double(0), C.c_int64(0), C.c_double(0)
        call = lib().sgp_grid_ei_comm if comm else lib().sgp_grid_ei
        self.ctx.check(call(self.h, int(kind), int(rows), mode, tv, float(xi),
                            None if fmin is None else dptr(fmin),
                            None if al is None else dptr(al), C.byref(v), C.byref(i),
                            C.byref(tu)))
        return al, v.value, i.value, tu.value

    def ise(self, gps, fmin, cand, about=ISE_UNSAFE, pairs=False, cov=False):
        """Information-theoretic safe exploration over the resident posterior
        (``sgp_grid_ise``): the candidates ``cand`` (global rows of this shard) against the
        rows outside ``S`` (``ISE_UNSAFE``) or every row (``ISE_ALL``) ->
        ``(alpha (K,), target (K,), value, global row, pairs (K, N) or None, cov (G, K, N) or
        None)``; -inf / -1 where no row qualifies.  ``pairs`` / ``cov``: test outputs."""
        fmin = f64(fmin).reshape(-1)
        cand = np.ascontiguousarray(cand, dtype=np.int64).reshape(-1)
        K, G = int(cand.size), len(gps)
        if fmin.size != G:
            raise ValueError("%d fmin for %d GPs" % (fmin.size, G))
        alpha = np.empty(K)
        target = np.empty(K, dtype=np.int64)
        pr = np.empty((K, self.N)) if pairs else None
        cv = np.empty((G, K, self.N)) if cov else None
        v, i = C.c_double(0), C.c_int64(0)
        self.ctx.check(lib().sgp_grid_ise(
            self.h, _gp_array(gps), G, dptr(fmin), cand.ctypes.data_as(c_i64_p), K, int(about),
            dptr(alpha), target.ctypes.data_as(c_i64_p), C.byref(v), C.byref(i),
            None if pr is None else dptr(pr), None if cv is None else dptr(cv)))
        return alpha, target, v.value, i.value, pr, cv

    def ise_at(self, gps, fmin, cand, xc, vx, about=ISE_UNSAFE, comm=False):
        """``ise`` with the candidates by value (``sgp_grid_ise_at``): ``cand`` global rows of
        the WHOLE grid, ``xc (K, d)`` their coordinates, ``vx (G, K)`` their variances ->
        ``(alpha (K,), target (K,), value, global row)`` over this shard's rows.  ``comm``:
        ``sgp_grid_ise_comm`` -- merged over the shards of all ranks of the context's
        communicator, the same on every rank; a collective."""
        fmin = f64(fmin).reshape(-1)
        cand = np.ascontiguousarray(cand, dtype=np.int64).reshape(-1)
        K, G = int(cand.size), len(gps)
        if fmin.size != G:
            raise ValueError("%d fmin for %d GPs" % (fmin.size, G))
        xc = f64(xc).reshape(K, self.d)
        vx = f64(vx).reshape(G, K)
        alpha = np.empty(K)
        target = np.empty(K, dtype=np.int64)
        v, i = C.c_double(0), C.c_int64(0)
        call = lib().sgp_grid_ise_comm if comm else lib().sgp_grid_ise_at
        self.ctx.check(call(
            self.h, _gp_array(gps), G, dptr(fmin), cand.ctypes.data_as(c_i64_p), dptr(xc),
            dptr(vx), K, int(about), dptr(alpha), target.ctypes.data_as(c_i64_p), C.byref(v),
            C.byref(i)))
        return alpha, target, v.value, i.value

    def ise_keys(self, gps, fmin):
        """``(count, min, max)`` of the keys ``sum_{g active} log1p(var_g / s_g) / 2`` of this
        shard's safe rows (``sgp_grid_ise_keys``); ``(0, inf, -inf)`` without one."""
        fmin = f64(fmin).reshape(-1)
        n, lo, hi = C.c_int64(0), C.c_double(0), C.c_double(0)
        self.ctx.check(lib().sgp_grid_ise_keys(self.h, _gp_array(gps), len(gps), dptr(fmin),
                                               C.byref(n), C.byref(lo), C.byref(hi)))
        return n.value, lo.value, hi.value

    def ise_hist(self, gps, fmin, key_lo, key_hi):
        """This shard's histogram (4096 bins over [key_lo, key_hi]) of the keys of its safe
        rows (``sgp_grid_ise_hist``)."""
        fmin = f64(fmin).reshape(-1)
        hist = np.zeros(4096, dtype=np.uint32)
        self.ctx.check(lib().sgp_grid_ise_hist(
            self.h, _gp_array(gps), len(gps), dptr(fmin), float(key_lo), float(key_hi),
            hist.ctypes.data_as(c_u32_p)))
        return hist

    def ise_list(self, gps, fmin, thr, cap):
        """This shard's safe rows with key >= thr in ascending row (``sgp_grid_ise_list``):
        ``(count, global rows, device keys, x (m, d), var (m, G))``, ``m = min(count, cap)``:
        a count above ``cap`` is the caller's to notice."""
        fmin = f64(fmin).reshape(-1)
        cap = max(int(cap), 0)
        room = max(cap, 1)
        gidx = np.empty(room, dtype=np.int64)
        key = np.empty(room)
        x = np.empty((room, self.d))
        var = np.empty((room, self.G))
        n = C.c_int64(0)
        self.ctx.check(lib().sgp_grid_ise_list(
            self.h, _gp_array(gps), len(gps), dptr(fmin), float(thr), cap, C.byref(n),
            gidx.ctypes.data_as(c_i64_p), dptr(key), dptr(x), dptr(var)))
        m = min(n.value, cap)
        return n.value, gidx[:m], key[:m], x[:m], var[:m]

    def download(self, what, out=None):
        if what == Q:
            shape, dt = (self.N, 2 * self.G), np.float64
        elif what in (S, M, G, CAND):
            shape, dt = (self.N,), np.uint8
        elif what == WIDTH:
            shape, dt = (self.N,), np.float64
        else:
            shape, dt = (self.G, self.N), np.float64
        buf = np.empty(shape, dtype=dt)
        self.ctx.check(lib().sgp_grid_download(self.h, what,
                                               buf.ctypes.data_as(vp)))
        if dt == np.uint8:
            buf = buf.view(np.bool_)
        if out is not None:
            np.copyto(out, buf)
            return out
        return buf


def grid_paths_comm(grid, gp, Omega, phase, W, V, mask=False, values=False, best=True):
    """``DeviceGrid.paths`` merged over the ranks of the grid's communicator
    (``sgp_grid_paths_comm``): every rank gets the arg-max over the rows of all ranks; a
    collective -- every rank calls it, with the same paths."""
    return grid.paths(gp, Omega, phase, W, V, mask=mask, values=values, best=best, comm=True)


def swarm_grow(ctx, gp, S, B, scale2, thr=0.95):
    """Rows of ``B`` to append to the safe set ``S`` (bool mask, in order)."""
    d = gp.d
    S = f64(S).reshape(-1, d)
    B = f64(B).reshape(-1, d)
    accept = np.zeros(B.shape[0], dtype=np.uint8)
    if B.shape[0]:
        ctx.check(lib().sgp_swarm_grow(
            ctx.h, gp.h, dptr(S), S.shape[0], dptr(B), B.shape[0],
            float(scale2), float(thr), accept.ctypes.data_as(c_u8_p)))
    return accept.view(np.bool_)


def _swarm_path_args(gp, path):
    """``(Omega, phase, m, w, v)`` of ONE sample path, checked against its GP."""
    Omega, phase, w, v = path
    Omega = f64(Omega).reshape(-1, gp.d)
    m = Omega.shape[0]
    phase, w, v = f64(phase), f64(w), f64(v)
    if phase.shape != (m,) or w.shape != (m,):
        raise ValueError("phase and w must be (m,) with m = %d features, got %r and %r"
                         % (m, phase.shape, w.shape))
    if v.shape != (gp.n,):
        raise ValueError("v must be (n,) = (%d,), got %r" % (gp.n, v.shape))
    return Omega, phase, m, w, v


def _swarm_ise_args(gps, ise):
    """``(targets, zmean, zvar, T)`` of an 'ise' swarm as contiguous float64 arrays: targets
    ``(T, d)``, the targets' posterior ``(G, T)`` each."""
    targets, zmean, zvar = ise
    targets = f64(targets).reshape(-1, gps[0].d)
    T = targets.shape[0]
    zmean, zvar = f64(zmean), f64(zvar)
    if zmean.shape != (len(gps), T) or zvar.shape != (len(gps), T):
        raise ValueError("zmean and zvar must be (G, T) = (%d, %d), got %r and %r"
                         % (len(gps), T, zmean.shape, zvar.shape))
    return targets, zmean, zvar, T


def _swarm_ei_args(ei):
    """``ei = (kind, tau, xi, weigh, free)`` of an 'ei' swarm as the C side takes it: ``kind``
    ``'ei'`` / ``'pi'`` or its code, ``weigh`` and ``free`` as 0 / 1 (an int is passed on as it
    is, for the library to refuse)."""
    kind, tau, xi, weigh, free = ei
    kind = {"ei": EI_EI, "pi": EI_PI}.get(kind, kind) if isinstance(kind, str) else kind
    return (int(kind), float(tau), float(xi), int(weigh), int(free))


def _swarm_call(ctx, name, gps, swarm_type, path, clones, mes=None, ise=None, ei=None):
    """The C symbol ``sgp_swarm_<name>[_path|_hall|_mes|_ise|_ei]`` of a swarm variant, the head of its
    argument list -- ``ctx, gps[, clones], G[, swarm type]`` -- and the staged-on-the-host
    path arguments that close it (``path = (Omega, phase, w, v)``, one sample path of
    ``gps[0]``; ``clones[g]``: ``gps[g].clone()`` with the pending picks appended; ``mes =
    (ystar, floor)``: the maxima of a max-value entropy search and the floor under them;
    ``ise = (targets, zmean, zvar)``: the targets of an information-theoretic safe exploration
    and their posterior; ``ei = (kind, tau, xi, weigh, free)``: the incumbent and the switches
    of an expected-improvement swarm)."""
    if ei is not None and (path is not None or clones is not None or mes is not None
                           or ise is not None):
        raise NotImplementedError("an 'ei' swarm takes neither a path, clones, maxima nor "
                                  "targets")
    if ise is not None and (path is not None or clones is not None or mes is not None):
        raise NotImplementedError("an 'ise' swarm takes neither a path, clones nor maxima")
    if mes is not None and (path is not None or clones is not None):
        raise NotImplementedError("a 'mes' swarm takes neither a path nor clones")
    head, tail = (ctx.h, _gp_array(gps)), ()
    if clones is not None:
        if len(clones) != len(gps):
            raise ValueError("%d clones for %d GPs" % (len(clones), len(gps)))
        name, head = name + "_hall", head + (_gp_array(clones),)
    head += (len(gps),)
    if path is not None:
        Omega, phase, m, w, v = _swarm_path_args(gps[0], path)
        name, tail = name + "_path", (dptr(Omega), dptr(phase), m, dptr(w), dptr(v))
    elif mes is not None:
        ystar = f64(mes[0]).reshape(-1)
        name, tail = name + "_mes", (dptr(ystar), int(ystar.size), float(mes[1]))
    elif ise is not None:
        targets, zmean, zvar, T = _swarm_ise_args(gps, ise)
        name, tail = name + "_ise", (dptr(targets), dptr(zmean), dptr(zvar), T)
    elif ei is not None:
        name, tail = name + "_ei", _swarm_ei_args(ei)
    else:
        head += (SWARM_TYPES[swarm_type],)
    return name, head, tail


def _swarm_run(ctx, gps, swarm_type, fit, state, schedule, path=None, clones=None,
               shard=None, mes=None, ise=None, ei=None):
    """Every whole PSO run on the device: ``fit = (beta, fmin, scaling, best_lower_bound)``,
    ``state = (positions, velocities, best_positions, best_values, global_best,
    velocity_scale, bounds)`` -- the first five updated in place -- and ``schedule = (init,
    iters, inertia0, step, rand, seed)``, the structs of the C side.  ``path`` (a Thompson
    swarm; ``swarm_type`` and the best lower bound are not used), ``clones`` (a hallucinated
    swarm), ``mes = (ystar, floor)`` (a max-value entropy search swarm; ``swarm_type`` and the
    best lower bound are not used), ``ise = (targets, zmean, zvar)`` (an information-theoretic
    safe exploration swarm, likewise), ``ei = (kind, tau, xi, weigh, free)`` (an expected-
    improvement swarm, likewise) and ``shard = (p0, P_total)`` pick the entry point
    (``sgp_swarm_run[_hall|_path|_mes|_ise|_ei][_shard]``)."""
    beta, fmin, scaling, best_lower_bound = fit
    init, iters, inertia0, step, rand, seed = schedule
    P = state[0].shape[0]
    if clones is not None and path is not None:
        raise NotImplementedError("a hallucinated swarm is a maximizers or an expanders "
                                  "swarm, not a Thompson swarm")
    name, head, tail = _swarm_call(ctx, "sgp_swarm_run", gps, swarm_type, path, clones, mes,
                                   ise, ei)
    for a in state[:5]:
        assert a.dtype == np.float64 and a.flags.c_contiguous
    vscale = f64(state[5])
    bnd = None if state[6] is None else f64(state[6])
    rnd = None if rand is None else f64(rand).ravel()
    args = head + (float(beta), dptr(f64(fmin)), dptr(f64(scaling)))
    if path is None and mes is None and ise is None and ei is None:
        args += (float(best_lower_bound),)
    args += (P,) + tuple(dptr(a) for a in state[:5]) + (
        dptr(vscale), None if bnd is None else dptr(bnd), int(bool(init)), int(iters),
        float(inertia0), float(step), None if rnd is None else dptr(rnd), int(seed)) + tail
    if shard is not None:
        name, args = name + "_shard", args + (int(shard[0]), int(shard[1]))
    ctx.check(getattr(lib(), name)(*args))


def _swarm_fitness(ctx, gps, swarm_type, particles, fit, path=None, clones=None,
                   want_var=False, mes=None, want_post=False, ise=None, want=(), ei=None):
    """Every swarm fitness call: ``(values, safe)`` of ``particles``, with ``want_var`` (a
    hallucinated swarm's) also the hallucinated variances ``(G, P)``, with ``want_post`` (a
    'mes' swarm's) also the posterior ``(2, P)`` of GP 0 the term was formed from; ``fit``,
    ``path``, ``clones``, ``mes`` and ``ise`` as for :func:`_swarm_run`.  An 'ise' swarm
    returns ``(values, safe, out)``, ``out`` a dict of the arrays named in ``want``: 'alpha'
    (P), 'target' (P, int64), 'post' (G, 2, P), 'pairs' (P, T), 'cov' (G, P, T).  An 'ei'
    swarm returns ``(values, safe)``, or with a non-empty ``want`` ``(values, safe, out)``:
    'alpha' (P), 'post' (G, 2, P)."""
    beta, fmin, scaling, best_lower_bound = fit
    name, head, tail = _swarm_call(ctx, "sgp_swarm_fitness", gps, swarm_type, path, clones, mes,
                                   ise, ei)
    particles = f64(particles).reshape(-1, gps[0].d)
    P = particles.shape[0]
    values = np.empty(P)
    safe = np.empty(P, dtype=np.uint8)
    var_h = np.empty((len(gps), P)) if want_var else None
    args = head + (dptr(particles), P, float(beta), dptr(f64(fmin)), dptr(f64(scaling)))
    if path is None and mes is None and ise is None and ei is None:
        args += (float(best_lower_bound),)
    args += tail + (dptr(values), safe.ctypes.data_as(c_u8_p))
    if clones is not None:
        args += (None if var_h is None else dptr(var_h),)
    post = np.empty((2, P)) if want_post else None
    if mes is not None:
        args += (None if post is None else dptr(post),)
    out = {}
    if ise is not None:
        unknown = set(want) - {"alpha", "target", "post", "pairs", "cov"}
        if unknown:
            raise ValueError("unknown outputs %r of an 'ise' swarm" % sorted(unknown))
        G, T = len(gps), tail[3]
        shapes = {"alpha": (P,), "target": (P,), "post": (G, 2, P), "pairs": (P, T),
                  "cov": (G, P, T)}
        for k in ("alpha", "target", "post", "pairs", "cov"):
            if k in want:
                out[k] = np.empty(shapes[k], dtype=np.int64 if k == "target" else np.float64)
        args += tuple((out[k].ctypes.data_as(c_i64_p) if k == "target" else dptr(out[k]))
                      if k in out else None for k in ("alpha", "target", "post", "pairs", "cov"))
    if ei is not None:
        unknown = set(want) - {"alpha", "post"}
        if unknown:
            raise ValueError("unknown outputs %r of an 'ei' swarm" % sorted(unknown))
        shapes = {"alpha": (P,), "post": (len(gps), 2, P)}
        for k in ("alpha", "post"):
            if k in want:
                out[k] = np.empty(shapes[k])
        args += tuple(dptr(out[k]) if k in out else None for k in ("alpha", "post"))
    # (an empty hallucinated call still checks its clones, an empty 'mes' call its maxima, an
    # empty 'ise' call its targets, an empty 'ei' call its incumbent)
    if P or clones is not None or mes is not None or ise is not None or ei is not None:
        ctx.check(getattr(lib(), name)(*args))
    if ise is not None or (ei is not None and want):
        return values, safe.view(np.bool_), out
    if want_post:
        return values, safe.view(np.bool_), post
    if want_var:
        return values, safe.view(np.bool_), var_h
    return values, safe.view(np.bool_)


def swarm_run(ctx, gps, swarm_type, beta, fmin, scaling, best_lower_bound,
              positions, velocities, best_positions, best_values, global_best,
              velocity_scale, bounds, init, iters, inertia0, step, rand, seed=0,
              shard=None):
    """Whole PSO run on the device; the state arrays are updated in place.

    ``shard=(p0, P_total)``: the arrays hold the rows ``[p0, p0 + P)`` of a swarm of
    ``P_total`` sharded over the ranks of ``ctx``'s communicator
    (``sgp_swarm_run_shard``); ``global_best`` comes back as the whole swarm's."""
    _swarm_run(ctx, gps, swarm_type, (beta, fmin, scaling, best_lower_bound),
               (positions, velocities, best_positions, best_values, global_best,
                velocity_scale, bounds), (init, iters, inertia0, step, rand, seed), shard=shard)


def swarm_fitness(ctx, gps, swarm_type, particles, beta, fmin, scaling,
                  best_lower_bound):
    return _swarm_fitness(ctx, gps, swarm_type, particles,
                          (beta, fmin, scaling, best_lower_bound))


def swarm_fitness_path(ctx, gps, particles, beta, fmin, scaling, path):
    """Fitness and safety of ``particles`` for a Thompson swarm (``sgp_swarm_fitness_path``):
    ``path = (Omega, phase, w, v)``, one sample path of ``gps[0]`` with contiguous 1-D ``w``
    and ``v`` (a column of a ``PosteriorPaths``)."""
    return _swarm_fitness(ctx, gps, None, particles, (beta, fmin, scaling, 0.0), path=path)


def swarm_run_path(ctx, gps, beta, fmin, scaling, positions, velocities, best_positions,
                   best_values, global_best, velocity_scale, bounds, init, iters, inertia0,
                   step, rand, path, seed=0, shard=None):
    """Whole PSO run of a Thompson swarm on the device (``sgp_swarm_run_path``); the state
    arrays are updated in place, ``path`` as for :func:`swarm_fitness_path`.

    ``shard=(p0, P_total)``: the arrays hold the rows ``[p0, p0 + P)`` of a swarm of
    ``P_total`` sharded over the ranks of ``ctx``'s communicator
    (``sgp_swarm_run_path_shard``), as for :func:`swarm_run`."""
    _swarm_run(ctx, gps, None, (beta, fmin, scaling, 0.0),
               (positions, velocities, best_positions, best_values, global_best,
                velocity_scale, bounds), (init, iters, inertia0, step, rand, seed),
               path=path, shard=shard)


def swarm_fitness_hall(ctx, gps, clones, swarm_type, particles, beta, fmin, scaling,
                       best_lower_bound, want_var=False):
    """Fitness and safety of ``particles`` for a hallucinated swarm
    (``sgp_swarm_fitness_hall``): ``clones[g]`` is ``gps[g].clone()`` with the pending picks
    of the batch appended.  The width term comes from the clones' variance, everything else
    from ``gps``.  ``want_var``: also the hallucinated variances, ``(G, P)``."""
    return _swarm_fitness(ctx, gps, swarm_type, particles,
                          (beta, fmin, scaling, best_lower_bound), clones=clones,
                          want_var=want_var)


def swarm_run_hall(ctx, gps, clones, swarm_type, beta, fmin, scaling, best_lower_bound,
                   positions, velocities, best_positions, best_values, global_best,
                   velocity_scale, bounds, init, iters, inertia0, step, rand, seed=0,
                   shard=None):
    """Whole PSO run of a hallucinated swarm on the device (``sgp_swarm_run_hall``); the state
    arrays are updated in place, ``clones`` as for :func:`swarm_fitness_hall`.

    ``shard=(p0, P_total)``: the arrays hold the rows ``[p0, p0 + P)`` of a swarm of
    ``P_total`` sharded over the ranks of ``ctx``'s communicator
    (``sgp_swarm_run_hall_shard``), as for :func:`swarm_run`."""
    _swarm_run(ctx, gps, swarm_type, (beta, fmin, scaling, best_lower_bound),
               (positions, velocities, best_positions, best_values, global_best,
                velocity_scale, bounds), (init, iters, inertia0, step, rand, seed),
               clones=clones, shard=shard)


def swarm_fitness_mes(ctx, gps, particles, beta, fmin, scaling, ystar, floor=-np.inf,
                      want_post=False):
    """Fitness and safety of ``particles`` for a max-value entropy search swarm
    (``sgp_swarm_fitness_mes``): ``values = alpha + total_pen`` with ``alpha`` the acquisition
    of :meth:`Context.mes_eval` on the posterior of ``gps[0]``, ``ystar`` (K) the maxima and
    ``floor`` the value under them (-inf: none), the penalty and ``safe`` those of the
    maximizers swarm.  ``want_post``: also that posterior, ``(2, P)`` mean | var."""
    return _swarm_fitness(ctx, gps, None, particles, (beta, fmin, scaling, 0.0),
                          mes=(ystar, floor), want_post=want_post)


def swarm_run_mes(ctx, gps, beta, fmin, scaling, positions, velocities, best_positions,
                  best_values, global_best, velocity_scale, bounds, init, iters, inertia0,
                  step, rand, ystar, floor=-np.inf, seed=0, shard=None):
    """Whole PSO run of a max-value entropy search swarm on the device
    (``sgp_swarm_run_mes``); the state arrays are updated in place, ``ystar`` and ``floor`` as
    for :func:`swarm_fitness_mes`.

    ``shard=(p0, P_total)``: the arrays hold the rows ``[p0, p0 + P)`` of a swarm of
    ``P_total`` sharded over the ranks of ``ctx``'s communicator
    (``sgp_swarm_run_mes_shard``), as for :func:`swarm_run`."""
    _swarm_run(ctx, gps, None, (beta, fmin, scaling, 0.0),
               (positions, velocities, best_positions, best_values, global_best,
                velocity_scale, bounds), (init, iters, inertia0, step, rand, seed),
               mes=(ystar, floor), shard=shard)


def swarm_fitness_ise(ctx, gps, particles, beta, fmin, scaling, targets, zmean, zvar, want=()):
    """Fitness and safety of ``particles`` for an information-theoretic safe exploration swarm
    (``sgp_swarm_fitness_ise``): ``values = alpha + total_pen`` with ``alpha[p] = max_t pair(p,
    t)`` over the ``targets`` (T, d), whose noiseless posterior is ``zmean`` / ``zvar`` (G, T);
    the penalty and ``safe`` are those of the maximizers swarm.  Returns ``(values, safe,
    out)``; ``want`` names the further arrays of ``out``: 'alpha' (P), 'target' (P), 'post'
    (G, 2, P), and the test outputs 'pairs' (P, T) and 'cov' (G, P, T)."""
    return _swarm_fitness(ctx, gps, None, particles, (beta, fmin, scaling, 0.0),
                          ise=(targets, zmean, zvar), want=want)


def swarm_run_ise(ctx, gps, beta, fmin, scaling, positions, velocities, best_positions,
                  best_values, global_best, velocity_scale, bounds, init, iters, inertia0,
                  step, rand, targets, zmean, zvar, seed=0, shard=None):
    """Whole PSO run of an information-theoretic safe exploration swarm on the device
    (``sgp_swarm_run_ise``); the state arrays are updated in place, ``targets``, ``zmean`` and
    ``zvar`` as for :func:`swarm_fitness_ise`.

    ``shard=(p0, P_total)``: the arrays hold the rows ``[p0, p0 + P)`` of a swarm of
    ``P_total`` sharded over the ranks of ``ctx``'s communicator
    (``sgp_swarm_run_ise_shard``), as for :func:`swarm_run`."""
    _swarm_run(ctx, gps, None, (beta, fmin, scaling, 0.0),
               (positions, velocities, best_positions, best_values, global_best,
                velocity_scale, bounds), (init, iters, inertia0, step, rand, seed),
               ise=(targets, zmean, zvar), shard=shard)


def swarm_fitness_ei(ctx, gps, particles, beta, fmin, scaling, kind, tau, xi, weigh, free,
                     want_alpha=False, want_post=False):
    """Fitness and safety of ``particles`` for an expected-improvement swarm
    (``sgp_swarm_fitness_ei``): ``values = alpha + total_pen`` with ``alpha`` the logarithm of
    :meth:`Context.ei_eval` on the posterior of ``gps`` -- ``kind`` ``'ei'`` / ``'pi'`` (or
    ``EI_EI`` / ``EI_PI``), the incumbent ``tau``, the margin ``xi``, with ``weigh`` the log
    probability of feasibility of every GP with a finite ``fmin`` -- the penalty and ``safe``
    those of the maximizers swarm; ``free``: ``values = alpha`` and ``safe`` all true, penalty
    and safety rule switched off.  Returns ``(values, safe)``, followed by ``alpha`` (P) with
    ``want_alpha`` and by the posterior ``(G, 2, P)`` mean | var with ``want_post``."""
    want = (("alpha",) if want_alpha else ()) + (("post",) if want_post else ())
    res = _swarm_fitness(ctx, gps, None, particles, (beta, fmin, scaling, 0.0),
                         ei=(kind, tau, xi, weigh, free), want=want)
    if not want:
        return res
    return res[:2] + tuple(res[2][k] for k in want)


def swarm_run_ei(ctx, gps, beta, fmin, scaling, positions, velocities, best_positions,
                 best_values, global_best, velocity_scale, bounds, init, iters, inertia0,
                 step, rand, kind, tau, xi, weigh, free, seed=0, shard=None):
    """Whole PSO run of an expected-improvement swarm on the device (``sgp_swarm_run_ei``); the
    state arrays are updated in place, ``kind`` .. ``free`` as for :func:`swarm_fitness_ei`.

    ``shard=(p0, P_total)``: the arrays hold the rows ``[p0, p0 + P)`` of a swarm of
    ``P_total`` sharded over the ranks of ``ctx``'s communicator
    (``sgp_swarm_run_ei_shard``), as for :func:`swarm_run`."""
    _swarm_run(ctx, gps, None, (beta, fmin, scaling, 0.0),
               (positions, velocities, best_positions, best_values, global_best,
                velocity_scale, bounds), (init, iters, inertia0, step, rand, seed),
               ei=(kind, tau, xi, weigh, free), shard=shard)
