"""ctypes binding of liblincheck.so (include/lincheck.h, include/lincheck_synth.h).

This is the build's own library, loaded in-process.  It exposes the GPU
checker (lc_*) and the seeded synthetic-history generator (lc_synth_*).
Loading fails loudly when the HIP library is missing, and when it was built
from other sources than the tree it is loaded from (lc_build_id() against
csrc/build_id.py): there is no fallback and no stale binary.
"""
import ctypes
import importlib.util
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# LINCHECK_LIB: dev-only override (A/B builds of the same ABI in tools/)
LIB_PATH = os.environ.get("LINCHECK_LIB") or os.path.join(_HERE, "liblincheck.so")

LC_F_READ, LC_F_WRITE, LC_F_CAS = 0, 1, 2
LC_NIL = -1
LC_INF = (1 << 63) - 1
LC_VALID, LC_INVALID, LC_UNKNOWN = 1, 0, -1

REASONS = {
    0: "none",
    1: "nonlinearizable",
    2: "config-budget",
    3: "window-overflow",
    4: "malformed",
    5: "unknown-f",
    7: "time-budget",
    6: "frontier-lds",
}
LC_REASON_NONLINEARIZABLE = 1
LC_REASON_CONFIG_BUDGET = 2
LC_REASON_WINDOW_OVERFLOW = 3
LC_REASON_MALFORMED = 4
LC_REASON_UNKNOWN_F = 5
LC_FLAG_NO_HBM_RETRY = 1
LC_FLAG_NO_FAST_PATH = 2
LC_FLAG_NO_GAP_TIER = 4
LC_FLAG_WHOLE_GPU = 8
LC_FLAG_NO_TIMING = 16
LC_FLAG_COUNTED_CLASSES = 32
LC_FLAG_SEARCH_WITNESS = 64
LC_FLAG_COUNTED_WITNESS = 128  # only with LC_FLAG_SEARCH_WITNESS
LC_COUNTED_MAX_CLASSES = 16
LC_WITNESS_NONE, LC_WITNESS_FULL, LC_WITNESS_PREFIX = 0, 1, 2
LC_WITNESS_ORDER_FULL, LC_WITNESS_ORDER_PREFIX = 3, 4  # LC_FLAG_SEARCH_WITNESS (witness.py)
LC_CERT_NONE, LC_CERT_DUP, LC_CERT_UNREACH, LC_CERT_CLAIMS, LC_CERT_PAIR, LC_CERT_ORDER, \
    LC_CERT_HALL, LC_CERT_PROOF = range(8)

# lc_op: 6 x int64 (f, value, expected, version, call, ret); arrays are (n, 6).
# lc_op32 (ABI 4): the same fields as 6 x 32 bits, arrays (n, 6) int32 with
# call / ret holding the uint32 bit patterns (LC_INF32 = 0xFFFFFFFF reads -1).
LC_INF32 = 0xFFFFFFFF
OP_FIELDS = ("f", "value", "expected", "version", "call", "ret")
RESULT_DTYPE = np.dtype([
    ("verdict", "<i4"), ("reason", "<i4"), ("fail_op", "<i8"),
    ("fail_prefix_end", "<i8"), ("configs_explored", "<i8"),
    ("max_frontier", "<i8"),
])
assert RESULT_DTYPE.itemsize == 40


class LcOpts(ctypes.Structure):
    _fields_ = [("init_version", ctypes.c_int64), ("init_value", ctypes.c_int64),
                ("max_configs_per_key", ctypes.c_int64),
                ("time_budget_ms", ctypes.c_int64), ("flags", ctypes.c_int64)]


class LcStats(ctypes.Structure):
    _fields_ = [("kernel_ms", ctypes.c_double), ("hbm_kernel_ms", ctypes.c_double),
                ("total_ms", ctypes.c_double), ("n_keys", ctypes.c_int64),
                ("n_ops", ctypes.c_int64), ("n_hbm_keys", ctypes.c_int64),
                ("n_devices", ctypes.c_int64), ("fast_kernel_ms", ctypes.c_double),
                ("jit_kernel_ms", ctypes.c_double), ("n_jit_keys", ctypes.c_int64),
                ("gap_kernel_ms", ctypes.c_double), ("n_gap_keys", ctypes.c_int64),
                ("n_malformed", ctypes.c_int64)]


class LcDeviceStats(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("pinned", ctypes.c_int32),
                ("key_begin", ctypes.c_int64), ("key_end", ctypes.c_int64),
                ("h2d_bytes", ctypes.c_int64), ("h2d_ms", ctypes.c_double),
                ("kernel_ms", ctypes.c_double), ("total_ms", ctypes.c_double)]


class LcCallProfile(ctypes.Structure):
    _fields_ = [("total_ms", ctypes.c_double), ("checked_ms", ctypes.c_double),
                ("planned_ms", ctypes.c_double), ("first_start_ms", ctypes.c_double),
                ("last_start_ms", ctypes.c_double), ("first_end_ms", ctypes.c_double),
                ("last_end_ms", ctypes.c_double), ("joined_ms", ctypes.c_double),
                ("whole_gpu_ms", ctypes.c_double), ("n_devices", ctypes.c_int64),
                ("n_chunks", ctypes.c_int64)]


class LcTotals(ctypes.Structure):
    _fields_ = [("calls", ctypes.c_int64), ("timed_calls", ctypes.c_int64),
                ("fast_kernel_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double)]


class LcCountedLayout(ctypes.Structure):
    _fields_ = [("n_classes", ctypes.c_int32), ("field_bits", ctypes.c_int32),
                ("slots", ctypes.c_int32), ("fits", ctypes.c_int32)] + \
               [(f, ctypes.c_int64 * LC_COUNTED_MAX_CLASSES)
                for f in ("f", "value", "expected", "version", "members")] + \
               [(f, ctypes.c_int32 * LC_COUNTED_MAX_CLASSES) for f in ("shift", "width")]


class LcCountedStats(ctypes.Structure):
    _fields_ = [("n_keys", ctypes.c_int64), ("n_decided", ctypes.c_int64),
                ("n_unfit", ctypes.c_int64), ("kernel_ms", ctypes.c_double)]


class LcWitnessStats(ctypes.Structure):
    _fields_ = [("n_keys", ctypes.c_int64), ("n_found", ctypes.c_int64),
                ("n_budget", ctypes.c_int64), ("n_window", ctypes.c_int64),
                ("nodes", ctypes.c_int64), ("cache_hits", ctypes.c_int64),
                ("kernel_ms", ctypes.c_double)]


class LcCountedWitnessStats(ctypes.Structure):
    _fields_ = [("n_keys", ctypes.c_int64), ("n_found", ctypes.c_int64),
                ("n_budget", ctypes.c_int64), ("n_unfit", ctypes.c_int64),
                ("nodes", ctypes.c_int64), ("cache_hits", ctypes.c_int64),
                ("kernel_ms", ctypes.c_double)]


# lc_counted_config (include/lincheck_counted.h)
COUNTED_CONFIG_DTYPE = np.dtype([("version", "<i8"), ("value", "<i8"), ("n_pending", "<i8"),
                                 ("pending_at", "<i8")])
assert COUNTED_CONFIG_DTYPE.itemsize == 32


class LcAux(ctypes.Structure):
    _fields_ = [("witness", ctypes.c_void_p), ("witness_kind", ctypes.c_void_p),
                ("certificate", ctypes.c_void_p), ("certificate_set", ctypes.c_void_p)]


# lc_event / lc_events_out / lc_events_stats (include/lincheck_events.h): events
# are (n, 6) int32 arrays — key, process, tf, value, expected, version
LC_EV_SKIP = -1
LC_EV_INVOKE, LC_EV_OK, LC_EV_FAIL, LC_EV_INFO = 0, 1, 2, 3


class LcEvent(ctypes.Structure):
    _fields_ = [("key", ctypes.c_int32), ("process", ctypes.c_int32), ("tf", ctypes.c_uint32),
                ("value", ctypes.c_int32), ("expected", ctypes.c_int32),
                ("version", ctypes.c_int32)]


class LcEventsOut(ctypes.Structure):
    _fields_ = [("ops32", ctypes.c_void_p), ("completion", ctypes.c_void_p),
                ("key_off", ctypes.c_void_p), ("key_base", ctypes.c_void_p),
                ("cap", ctypes.c_int64), ("n_ops", ctypes.c_int64)]


class LcEventsStats(ctypes.Structure):
    _fields_ = [("h2d_ms", ctypes.c_double), ("split_ms", ctypes.c_double),
                ("check_ms", ctypes.c_double), ("total_ms", ctypes.c_double),
                ("n_events", ctypes.c_int64), ("n_client", ctypes.c_int64),
                ("n_ops", ctypes.c_int64), ("n_fail_pairs", ctypes.c_int64),
                ("n_ignored_completions", ctypes.c_int64), ("n_big_keys", ctypes.c_int64)]


class LcEventsLimits(ctypes.Structure):
    _fields_ = [("max_lds_events", ctypes.c_int64), ("lds_process_capacity", ctypes.c_int64)]


# lc_set_full (include/lincheck_setfull.h): adds, reads and elements are numpy
# structured arrays of the C structs' layout
LC_SF_NEVER_READ, LC_SF_STABLE, LC_SF_LOST = 0, 1, 2
LC_SF_STALE, LC_SF_DUPLICATED = 1, 2
SF_ADD_DTYPE = np.dtype([("value", "<i8"), ("ok_time", "<i8"), ("inv_pos", "<i4"), ("ok_pos", "<i4")])
SF_READ_DTYPE = np.dtype([("inv_time", "<i8"), ("ok_time", "<i8"), ("off", "<i8"), ("inv_pos", "<i4"),
                          ("ok_pos", "<i4"), ("len", "<i4"), ("pad", "<i4")])
SF_ELEMENT_DTYPE = np.dtype([("outcome", "<i4"), ("flags", "<i4"), ("known_pos", "<i4"),
                             ("last_present", "<i4"), ("last_absent", "<i4"), ("dup_max", "<i4"),
                             ("stable_latency_ms", "<i8"), ("lost_latency_ms", "<i8")])
assert (SF_ADD_DTYPE.itemsize, SF_READ_DTYPE.itemsize, SF_ELEMENT_DTYPE.itemsize) == (24, 40, 40)


class LcSfSummary(ctypes.Structure):
    _fields_ = [("valid", ctypes.c_int32), ("linearizable", ctypes.c_int32),
                ("n_elements", ctypes.c_int64), ("n_stable", ctypes.c_int64),
                ("n_lost", ctypes.c_int64), ("n_never_read", ctypes.c_int64),
                ("n_stale", ctypes.c_int64), ("n_duplicated", ctypes.c_int64),
                ("n_phantom", ctypes.c_int64), ("n_tiles", ctypes.c_int64),
                ("h2d_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("total_ms", ctypes.c_double)]


class LcSfLimits(ctypes.Structure):
    _fields_ = [("tile_bytes", ctypes.c_int64), ("default_tile_bytes", ctypes.c_int64),
                ("max_position", ctypes.c_int64), ("value_bytes", ctypes.c_int64)]


# lc_append_check (include/lincheck_append.h): txns, mops, edges, keys and
# witness steps are numpy structured arrays of the C structs' layout
LC_AP_OK, LC_AP_INFO, LC_AP_FAIL = 0, 1, 2
LC_AP_APPEND, LC_AP_READ = 0, 1
LC_AP_WW, LC_AP_WR, LC_AP_RW, LC_AP_RT = 0, 1, 2, 3
LC_AP_MAX_CYCLES = 16
LC_AP_R_NONPREFIX, LC_AP_R_DUPLICATE, LC_AP_R_G1A, LC_AP_R_PHANTOM, LC_AP_R_G1B, LC_AP_R_INTERNAL, \
    LC_AP_R_EXTERNAL = 1, 2, 4, 8, 16, 32, 64
LC_AP_R_ANOMALY = 63
LC_AP_K_INCOMPATIBLE, LC_AP_K_NO_ORDER = 1, 2
LC_AP_CLASSES = ("G0", "G1c", "G-single", "G2-item", "G0-realtime", "G1c-realtime", "G-single-realtime",
                 "G2-item-realtime")
AP_TXN_DTYPE = np.dtype([("mop_off", "<i8"), ("inv_pos", "<i4"), ("comp_pos", "<i4"), ("type", "<i4"),
                         ("mop_len", "<i4")])
AP_MOP_DTYPE = np.dtype([("key", "<i8"), ("value", "<i8"), ("f", "<i4"), ("len", "<i4")])
AP_EDGE_DTYPE = np.dtype([("from", "<i4"), ("to", "<i4"), ("type", "<i4"), ("pad", "<i4"), ("key", "<i8")])
AP_KEY_DTYPE = np.dtype([("key", "<i8"), ("longest", "<i8"), ("len", "<i4"), ("flags", "<i4"),
                         ("first_dup", "<i4"), ("first_failed", "<i4"), ("first_phantom", "<i4"),
                         ("pad", "<i4")])
AP_STEP_DTYPE = np.dtype([("txn", "<i4"), ("type", "<i4"), ("key", "<i8")])
assert (AP_TXN_DTYPE.itemsize, AP_MOP_DTYPE.itemsize, AP_EDGE_DTYPE.itemsize, AP_KEY_DTYPE.itemsize,
        AP_STEP_DTYPE.itemsize) == (24, 24, 24, 40, 16)


class LcApOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in
                ("mop_flags", "txn_flags", "keys", "edges", "byc", "rt_lo", "rt_hi", "scc", "scc_class",
                 "steps", "cycle_off", "cycle_scc")]


class LcApSummary(ctypes.Structure):
    _fields_ = [("valid", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("n_incompatible_order", ctypes.c_int64), ("n_nonprefix", ctypes.c_int64),
                ("n_duplicate", ctypes.c_int64), ("n_g1a", ctypes.c_int64), ("n_phantom", ctypes.c_int64),
                ("n_g1b", ctypes.c_int64), ("n_internal", ctypes.c_int64), ("n_class", ctypes.c_int64 * 8),
                ("n_keys", ctypes.c_int64), ("n_ok", ctypes.c_int64), ("n_nodes", ctypes.c_int64),
                ("n_edges", ctypes.c_int64), ("n_scc", ctypes.c_int64),
                ("n_cycles_returned", ctypes.c_int64), ("n_slow_reads", ctypes.c_int64),
                ("h2d_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("host_graph_ms", ctypes.c_double), ("total_ms", ctypes.c_double)]


class LcApLimits(ctypes.Structure):
    _fields_ = [("max_payload", ctypes.c_int64), ("default_max_payload", ctypes.c_int64),
                ("max_position", ctypes.c_int64), ("max_mops", ctypes.c_int64)]


# lc_wr_check (include/lincheck_wr.h): the txn, edge and step records are
# list-append's
LC_WR_OK, LC_WR_INFO, LC_WR_FAIL = 0, 1, 2
LC_WR_WRITE, LC_WR_READ = 0, 1
LC_WR_NIL = -2 ** 63
LC_WR_WFR_KEYS = 1
LC_WR_R_INTERNAL, LC_WR_R_PHANTOM, LC_WR_R_G1A, LC_WR_R_G1B, LC_WR_R_EXTERNAL = 1, 2, 4, 8, 16
LC_WR_R_ANOMALY = 15
LC_WR_K_CYCLIC, LC_WR_K_LOST_UPDATE = 1, 2
WR_TXN_DTYPE, WR_EDGE_DTYPE, WR_STEP_DTYPE = AP_TXN_DTYPE, AP_EDGE_DTYPE, AP_STEP_DTYPE
WR_MOP_DTYPE = np.dtype([("key", "<i8"), ("value", "<i8"), ("f", "<i4"), ("known", "<i4")])
WR_KEY_DTYPE = np.dtype([("key", "<i8"), ("cyc_value", "<i8"), ("flags", "<i4"), ("n_writes", "<i4"),
                         ("n_versions", "<i4"), ("n_ext_reads", "<i4")])
assert (WR_MOP_DTYPE.itemsize, WR_KEY_DTYPE.itemsize) == (24, 32)


class LcWrOut(ctypes.Structure):
    _fields_ = [("mop_flags", ctypes.c_void_p), ("txn_flags", ctypes.c_void_p), ("keys", ctypes.c_void_p),
                ("edges", ctypes.c_void_p), ("edge_cap", ctypes.c_int64)] + \
               [(f, ctypes.c_void_p) for f in ("byc", "rt_lo", "rt_hi", "scc", "scc_class", "steps", "cycle_off",
                                               "cycle_scc")]


class LcWrSummary(ctypes.Structure):
    _fields_ = [("valid", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("n_internal", ctypes.c_int64), ("n_phantom", ctypes.c_int64), ("n_g1a", ctypes.c_int64),
                ("n_g1b", ctypes.c_int64), ("n_cyclic_keys", ctypes.c_int64), ("n_lost_update", ctypes.c_int64),
                ("n_class", ctypes.c_int64 * 8),
                ("n_keys", ctypes.c_int64), ("n_versions", ctypes.c_int64), ("n_ok", ctypes.c_int64),
                ("n_nodes", ctypes.c_int64), ("n_edges", ctypes.c_int64), ("n_edges_raw", ctypes.c_int64),
                ("n_scc", ctypes.c_int64), ("n_cycles_returned", ctypes.c_int64),
                ("h2d_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("host_graph_ms", ctypes.c_double), ("total_ms", ctypes.c_double)]


class LcWrLimits(ctypes.Structure):
    _fields_ = [("max_edges", ctypes.c_int64), ("default_max_edges", ctypes.c_int64),
                ("max_position", ctypes.c_int64), ("max_mops", ctypes.c_int64)]


# lc_wr_check_lin (include/lincheck_wrlin.h)
LC_WR_LINEARIZABLE_KEYS = 2
WR_LIN_KEY_DTYPE = np.dtype([("n_pairs", "<i8"), ("n_touches", "<i4"), ("n_vedges", "<i4")])
assert WR_LIN_KEY_DTYPE.itemsize == 16


class LcWrLinSummary(ctypes.Structure):
    _fields_ = [("n_touches", ctypes.c_int64), ("n_pairs", ctypes.c_int64), ("n_vedges", ctypes.c_int64),
                ("max_key_versions", ctypes.c_int64), ("lin_kernel_ms", ctypes.c_double)]


class LcWrLinLimits(ctypes.Structure):
    _fields_ = [("max_key_versions", ctypes.c_int64), ("wave_key_versions", ctypes.c_int64)]


# lc_cycle_screen (include/lincheck_screen.h): the txn and edge records are
# list-append's
LC_SCREEN_RT, LC_SCREEN_TRIM = 1, 2


class LcScreenOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in ("reach_lo", "reach_hi", "mark")]


class LcScreenSummary(ctypes.Structure):
    _fields_ = [("clean", ctypes.c_int32), ("label_rounds", ctypes.c_int32), ("trim_rounds", ctypes.c_int32),
                ("max_rounds", ctypes.c_int32), ("n_rt_members", ctypes.c_int64),
                ("n_trim_survivors", ctypes.c_int64), ("h2d_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("total_ms", ctypes.c_double)]


class LcScreenLimits(ctypes.Structure):
    _fields_ = [("max_rounds", ctypes.c_int32), ("default_max_rounds", ctypes.c_int32)]


# lc_cycle_reach and the restricted checker calls (include/lincheck_cycles.h)
LC_REACH_ALL = 1


class LcReachSummary(ctypes.Structure):
    _fields_ = [("first_hit", ctypes.c_int64), ("n_queries_run", ctypes.c_int64), ("nodes_visited", ctypes.c_int64),
                ("h2d_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double), ("total_ms", ctypes.c_double)]


class LcReachLimits(ctypes.Structure):
    _fields_ = [("max_nodes", ctypes.c_int64), ("min_work", ctypes.c_int64), ("default_min_work", ctypes.c_int64),
                ("max_workgroups", ctypes.c_int32), ("pad", ctypes.c_int32)]


class LcCycleSearchSummary(ctypes.Structure):
    _fields_ = [("restricted", ctypes.c_int32), ("pad", ctypes.c_int32), ("n_marked", ctypes.c_int64),
                ("n_device_searches", ctypes.c_int64), ("n_device_queries", ctypes.c_int64),
                ("n_host_fallbacks", ctypes.c_int64), ("search_ms", ctypes.c_double)]


# lc_cycles_host's hook: (user, n_nodes, pred_off, pred, n_queries, q_node, q_head_off, q_heads, first_hit) -> int
LC_REACH_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
                               ctypes.POINTER(ctypes.c_int32), ctypes.c_int64, ctypes.POINTER(ctypes.c_int32),
                               ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32),
                               ctypes.POINTER(ctypes.c_int64))


# lc_watch_check (include/lincheck_watch.h)
LC_WT_DELETE, LC_WT_INSERT = 0, 1
LC_WT_NO_SCRIPT = 1
LC_WT_MAX_D_LIMIT = 4096
WT_THREAD_DTYPE = np.dtype([("off", "<i8"), ("len", "<i8"), ("revision", "<i8"), ("thread", "<i8")])
WT_DELTA_DTYPE = np.dtype([("thread", "<i4"), ("flags", "<u4"), ("edit_distance", "<i8"), ("prefix", "<i8"),
                           ("suffix", "<i8"), ("script_off", "<i8"), ("script_len", "<i8")])
WT_EDIT_DTYPE = np.dtype([("at", "<i8"), ("value", "<i8"), ("op", "<i4"), ("pad", "<i4")])
assert (WT_THREAD_DTYPE.itemsize, WT_DELTA_DTYPE.itemsize, WT_EDIT_DTYPE.itemsize) == (32, 48, 24)


class LcWtOut(ctypes.Structure):
    _fields_ = [("cls", ctypes.c_void_p), ("distance", ctypes.c_void_p), ("deltas", ctypes.c_void_p),
                ("edits", ctypes.c_void_p), ("edit_cap", ctypes.c_int64)]


class LcWtSummary(ctypes.Structure):
    _fields_ = [("valid", ctypes.c_int32), ("canonical", ctypes.c_int32), ("canonical_size", ctypes.c_int64),
                ("n_threads", ctypes.c_int64), ("n_classes", ctypes.c_int64), ("n_deltas", ctypes.c_int64),
                ("n_edits", ctypes.c_int64), ("n_no_script", ctypes.c_int64), ("n_by_host", ctypes.c_int64),
                ("n_collisions", ctypes.c_int64), ("revisions_equal", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("h2d_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double), ("total_ms", ctypes.c_double)]


class LcWtLimits(ctypes.Structure):
    _fields_ = [("max_d", ctypes.c_int64), ("default_max_d", ctypes.c_int64), ("trace_bytes", ctypes.c_int64),
                ("default_trace_bytes", ctypes.c_int64), ("max_len", ctypes.c_int64),
                ("max_device_len", ctypes.c_int64), ("hash_mask", ctypes.c_uint64)]


# lc_perf_stats (include/lincheck_perf.h)
LC_PS_MAX_Q = 8
LC_PS_NONE = -2 ** 63
PS_EVENT_DTYPE = np.dtype([("time", "<i8"), ("process", "<i4"), ("f", "<u2"), ("type", "u1"), ("pad", "u1")])
assert PS_EVENT_DTYPE.itemsize == 16
PS_DEFAULT_QS = (0.5, 0.95, 0.99, 1.0)
PS_DEFAULT_RATE_DT_NS = 10 * 10 ** 9
PS_DEFAULT_QUANT_DT_NS = 30 * 10 ** 9


class LcPsParams(ctypes.Structure):
    _fields_ = [("n_f", ctypes.c_int32), ("n_q", ctypes.c_int32), ("q", ctypes.c_double * LC_PS_MAX_Q),
                ("rate_dt_ns", ctypes.c_int64), ("quant_dt_ns", ctypes.c_int64)]


class LcPsOut(ctypes.Structure):
    _fields_ = [("by_f", ctypes.c_void_p), ("comp_pos", ctypes.c_void_p), ("latency_ns", ctypes.c_void_p),
                ("rate", ctypes.c_void_p), ("rate_cap", ctypes.c_int64), ("quant", ctypes.c_void_p),
                ("quant_n", ctypes.c_void_p), ("quant_cap", ctypes.c_int64)]


class LcPsSummary(ctypes.Structure):
    _fields_ = [("valid", ctypes.c_int32), ("pad", ctypes.c_int32), ("n_events", ctypes.c_int64),
                ("n_client", ctypes.c_int64), ("n_pairs", ctypes.c_int64), ("n_pending", ctypes.c_int64),
                ("n_ignored_completions", ctypes.c_int64), ("n_mismatched_f", ctypes.c_int64),
                ("count", ctypes.c_int64), ("ok", ctypes.c_int64), ("fail", ctypes.c_int64),
                ("info", ctypes.c_int64), ("t_max", ctypes.c_int64), ("n_rate_buckets", ctypes.c_int64),
                ("n_quant_buckets", ctypes.c_int64), ("h2d_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("total_ms", ctypes.c_double)]


class LcPsLimits(ctypes.Structure):
    _fields_ = [("max_f", ctypes.c_int64), ("max_table_entries", ctypes.c_int64), ("lds_entries", ctypes.c_int64),
                ("default_lds_entries", ctypes.c_int64), ("wave", ctypes.c_int32), ("block", ctypes.c_int32),
                ("chunk", ctypes.c_int32), ("max_grid", ctypes.c_int32)]


class LcSynthParams(ctypes.Structure):
    _fields_ = [("n_keys", ctypes.c_int64), ("ops_per_key", ctypes.c_int64),
                ("concurrency", ctypes.c_int32), ("n_values", ctypes.c_int32),
                ("p_info", ctypes.c_double), ("p_anomaly", ctypes.c_double),
                ("seed", ctypes.c_uint64), ("info_frac", ctypes.c_double)]


_lib = None


def source_build_id():
    """Hash of the csrc/ + include/ sources in this tree (csrc/build_id.py)."""
    spec = importlib.util.spec_from_file_location(
        "lincheck_build_id", os.path.join(_HERE, "csrc", "build_id.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.build_id()


def lib():
    """Load liblincheck.so once; raise if it has not been built, or was built
    from sources other than this tree's."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "liblincheck.so not built (%s); run `python -c 'import "
                "__graft_entry__ as g; g.build()'` — there is no CPU fallback" % LIB_PATH)
        # torch ships its own HIP runtime (torch/lib/libamdhip64.so) next to
        # the system one this library links; torch only initialises its GPU
        # if it is loaded first, so load it first whenever it is installed
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        L.lc_build_id.argtypes = []
        L.lc_build_id.restype = ctypes.c_char_p
        built = L.lc_build_id().decode()
        if not os.environ.get("LINCHECK_LIB"):  # dev A/B builds are other sources on purpose
            want = source_build_id()
            if built != want:
                raise RuntimeError(
                    "stale liblincheck.so: built from sources %s, this tree is %s; rebuild "
                    "(make -C jepsen/etcd_amd/csrc)" % (built, want))
        p, i64, i32, u32, vp = (ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                ctypes.c_uint32, ctypes.c_void_p)
        L.lc_open.argtypes = [u32, ctypes.POINTER(vp)]
        L.lc_open.restype = ctypes.c_int
        L.lc_check.argtypes = [vp, p, p, i64, ctypes.POINTER(LcOpts), p]
        L.lc_check.restype = ctypes.c_int
        L.lc_check_device.argtypes = [vp, vp, vp, i64, ctypes.POINTER(LcOpts), vp, vp]
        L.lc_check_device.restype = ctypes.c_int
        L.lc_check_ex.argtypes = [vp, p, p, i64, ctypes.POINTER(LcOpts), p, ctypes.POINTER(LcAux)]
        L.lc_check_ex.restype = ctypes.c_int
        L.lc_check_device_ex.argtypes = [vp, vp, vp, i64, ctypes.POINTER(LcOpts), vp, vp,
                                         ctypes.POINTER(LcAux)]
        L.lc_check_device_ex.restype = ctypes.c_int
        L.lc_check32.argtypes = [vp, p, p, p, i64, ctypes.POINTER(LcOpts), p,
                                 ctypes.POINTER(LcAux)]
        L.lc_check32.restype = ctypes.c_int
        L.lc_check_device32.argtypes = [vp, vp, vp, vp, i64, ctypes.POINTER(LcOpts), vp, vp,
                                        ctypes.POINTER(LcAux)]
        L.lc_check_device32.restype = ctypes.c_int
        L.lc_pack32.argtypes = [p, p, i64, p, p]
        L.lc_pack32.restype = ctypes.c_int
        L.lc_pack16.argtypes = [p, p, i64, p, p]
        L.lc_pack16.restype = ctypes.c_int
        L.lc_check16.argtypes = [vp, p, p, p, i64, ctypes.POINTER(LcOpts), p,
                                 ctypes.POINTER(LcAux)]
        L.lc_check16.restype = ctypes.c_int
        L.lc_check_frontiers.argtypes = [vp, p, p, i64, p, ctypes.POINTER(LcOpts), vp, i32, p]
        L.lc_check_frontiers.restype = ctypes.c_int
        L.lc_last_totals.argtypes = [vp, ctypes.POINTER(LcTotals), i32]
        L.lc_last_totals.restype = ctypes.c_int
        L.lc_quiesce.argtypes = [vp]
        L.lc_quiesce.restype = ctypes.c_int
        L.lc_last_call_profile.argtypes = [vp, ctypes.POINTER(LcCallProfile)]
        L.lc_last_call_profile.restype = ctypes.c_int
        L.lc_key_cost.argtypes = [p, p, i64, p]
        L.lc_key_cost.restype = ctypes.c_int
        L.lc_last_stats.argtypes = [vp, ctypes.POINTER(LcStats)]
        L.lc_last_stats.restype = ctypes.c_int
        L.lc_last_device_stats.argtypes = [vp, i32, ctypes.POINTER(LcDeviceStats)]
        L.lc_last_device_stats.restype = ctypes.c_int
        L.lc_host_register.argtypes = [vp, vp, ctypes.c_uint64]
        L.lc_host_register.restype = ctypes.c_int
        L.lc_host_unregister.argtypes = [vp, vp]
        L.lc_host_unregister.restype = ctypes.c_int
        L.lc_last_error.argtypes = [vp]
        L.lc_last_error.restype = ctypes.c_char_p
        L.lc_close.argtypes = [vp]
        L.lc_close.restype = None
        L.lc_default_opts.argtypes = [ctypes.POINTER(LcOpts)]
        L.lc_default_opts.restype = None
        L.lc_plan_partition.argtypes = [p, p, i64, i32, p]
        L.lc_plan_partition.restype = ctypes.c_int
        L.lc_counted_plan.argtypes = [p, i64, ctypes.POINTER(LcCountedLayout)]
        L.lc_counted_plan.restype = ctypes.c_int
        L.lc_last_counted_stats.argtypes = [vp, ctypes.POINTER(LcCountedStats)]
        L.lc_last_counted_stats.restype = ctypes.c_int
        if hasattr(L, "lc_last_witness_stats"):  # (additive to ABI 5: a LINCHECK_LIB may lack it)
            L.lc_last_witness_stats.argtypes = [vp, ctypes.POINTER(LcWitnessStats)]
            L.lc_last_witness_stats.restype = ctypes.c_int
        if hasattr(L, "lc_last_counted_witness_stats"):  # (the same)
            L.lc_last_counted_witness_stats.argtypes = [vp, ctypes.POINTER(LcCountedWitnessStats)]
            L.lc_last_counted_witness_stats.restype = ctypes.c_int
        if hasattr(L, "lc_check_frontiers_counted"):  # (additive to ABI 5: a LINCHECK_LIB may lack it)
            L.lc_check_frontiers_counted.argtypes = [vp, p, p, i64, p, ctypes.POINTER(LcOpts), p, i32,
                                                     p, p, p, i64]
            L.lc_check_frontiers_counted.restype = ctypes.c_int
        if hasattr(L, "lc_check_events"):  # (additive to ABI 5: a LINCHECK_LIB may lack it)
            L.lc_events_pack_host.argtypes = [p, i64, i64, ctypes.POINTER(LcEventsOut)]
            L.lc_events_pack_host.restype = ctypes.c_int
            L.lc_events_pack.argtypes = [vp, p, i64, i64, ctypes.POINTER(LcEventsOut)]
            L.lc_events_pack.restype = ctypes.c_int
            L.lc_check_events.argtypes = [vp, p, i64, i64, ctypes.POINTER(LcOpts), p,
                                          ctypes.POINTER(LcAux), ctypes.POINTER(LcEventsOut)]
            L.lc_check_events.restype = ctypes.c_int
            L.lc_last_events_stats.argtypes = [vp, ctypes.POINTER(LcEventsStats)]
            L.lc_last_events_stats.restype = ctypes.c_int
            L.lc_events_limits.argtypes = [ctypes.POINTER(LcEventsLimits)]
            L.lc_events_limits.restype = ctypes.c_int
        if hasattr(L, "lc_set_full"):  # (additive to ABI 5: a LINCHECK_LIB may lack it)
            L.lc_set_full_host.argtypes = [p, i64, p, i64, p, i64, i32, p, ctypes.POINTER(LcSfSummary)]
            L.lc_set_full_host.restype = ctypes.c_int
            L.lc_set_full.argtypes = [vp, p, i64, p, i64, p, i64, i32, p, ctypes.POINTER(LcSfSummary)]
            L.lc_set_full.restype = ctypes.c_int
            L.lc_set_full_limits.argtypes = [ctypes.POINTER(LcSfLimits)]
            L.lc_set_full_limits.restype = ctypes.c_int
        if hasattr(L, "lc_append_check"):  # (additive to ABI 5: a LINCHECK_LIB may lack it)
            ap = [p, i64, p, i64, p, i64, ctypes.POINTER(LcApOut), ctypes.POINTER(LcApSummary)]
            L.lc_append_check_host.argtypes = ap
            L.lc_append_check_host.restype = ctypes.c_int
            L.lc_append_check.argtypes = [vp] + ap
            L.lc_append_check.restype = ctypes.c_int
            L.lc_append_limits.argtypes = [ctypes.POINTER(LcApLimits)]
            L.lc_append_limits.restype = ctypes.c_int
        if hasattr(L, "lc_wr_check"):  # (additive to ABI 5: a LINCHECK_LIB may lack it)
            wr = [p, i64, p, i64, ctypes.c_uint32, ctypes.POINTER(LcWrOut), ctypes.POINTER(LcWrSummary)]
            L.lc_wr_check_host.argtypes = wr
            L.lc_wr_check_host.restype = ctypes.c_int
            L.lc_wr_check.argtypes = [vp] + wr
            L.lc_wr_check.restype = ctypes.c_int
            L.lc_wr_limits.argtypes = [ctypes.POINTER(LcWrLimits)]
            L.lc_wr_limits.restype = ctypes.c_int
        if hasattr(L, "lc_wr_check_lin"):  # (additive to ABI 5: a LINCHECK_LIB may lack it)
            wl = [p, i64, p, i64, ctypes.c_uint32, ctypes.POINTER(LcWrOut), ctypes.POINTER(LcWrSummary), p,
                  ctypes.POINTER(LcWrLinSummary)]
            L.lc_wr_check_lin_host.argtypes = wl
            L.lc_wr_check_lin_host.restype = ctypes.c_int
            L.lc_wr_check_lin.argtypes = [vp] + wl
            L.lc_wr_check_lin.restype = ctypes.c_int
            L.lc_wr_lin_limits.argtypes = [ctypes.POINTER(LcWrLinLimits)]
            L.lc_wr_lin_limits.restype = ctypes.c_int
        if hasattr(L, "lc_watch_check"):  # (additive to ABI 5: a LINCHECK_LIB may lack it)
            wt = [p, i64, p, i64, i64, ctypes.c_uint32, ctypes.POINTER(LcWtOut), ctypes.POINTER(LcWtSummary)]
            L.lc_watch_check_host.argtypes = wt
            L.lc_watch_check_host.restype = ctypes.c_int
            L.lc_watch_check.argtypes = [vp] + wt
            L.lc_watch_check.restype = ctypes.c_int
            L.lc_watch_limits.argtypes = [ctypes.POINTER(LcWtLimits)]
            L.lc_watch_limits.restype = ctypes.c_int
        if hasattr(L, "lc_perf_stats"):  # (additive to ABI 5: a LINCHECK_LIB may lack it)
            ps = [p, i64, ctypes.POINTER(LcPsParams), ctypes.POINTER(LcPsOut), ctypes.POINTER(LcPsSummary)]
            L.lc_perf_stats_host.argtypes = ps
            L.lc_perf_stats_host.restype = ctypes.c_int
            L.lc_perf_stats.argtypes = [vp] + ps
            L.lc_perf_stats.restype = ctypes.c_int
            L.lc_perf_stats_limits.argtypes = [ctypes.POINTER(LcPsLimits)]
            L.lc_perf_stats_limits.restype = ctypes.c_int
        if hasattr(L, "lc_cycle_screen"):  # (additive to ABI 5: a LINCHECK_LIB may lack it)
            sc = [p, i64, p, i64, ctypes.POINTER(LcScreenOut), ctypes.POINTER(LcScreenSummary)]
            L.lc_cycle_screen_host.argtypes = sc
            L.lc_cycle_screen_host.restype = ctypes.c_int
            L.lc_cycle_screen.argtypes = [vp] + sc
            L.lc_cycle_screen.restype = ctypes.c_int
            L.lc_screen_limits.argtypes = [ctypes.POINTER(LcScreenLimits)]
            L.lc_screen_limits.restype = ctypes.c_int
        if hasattr(L, "lc_append_check_screened"):  # (additive to ABI 5: a LINCHECK_LIB may lack it)
            scr = ctypes.POINTER(LcScreenSummary)
            L.lc_append_check_screened.argtypes = [vp, p, i64, p, i64, p, i64, ctypes.POINTER(LcApOut),
                                                   ctypes.POINTER(LcApSummary), scr]
            L.lc_append_check_screened.restype = ctypes.c_int
            L.lc_wr_check_screened.argtypes = [vp, p, i64, p, i64, ctypes.c_uint32, ctypes.POINTER(LcWrOut),
                                               ctypes.POINTER(LcWrSummary), scr]
            L.lc_wr_check_screened.restype = ctypes.c_int
        if hasattr(L, "lc_cycle_reach"):  # (additive to ABI 5: a LINCHECK_LIB may lack it)
            rs = [i64, p, p, i64, i64, p, p, p, i64, ctypes.c_uint32, p, ctypes.POINTER(LcReachSummary)]
            L.lc_cycle_reach_host.argtypes = rs
            L.lc_cycle_reach_host.restype = ctypes.c_int
            L.lc_cycle_reach.argtypes = [vp] + rs
            L.lc_cycle_reach.restype = ctypes.c_int
            L.lc_cycle_reach_limits.argtypes = [ctypes.POINTER(LcReachLimits)]
            L.lc_cycle_reach_limits.restype = ctypes.c_int
            L.lc_cycles_host.argtypes = [p, i64, p, i64, p, LC_REACH_FN, p, i64, i64, p, p, p, p, p, p, p,
                                         ctypes.POINTER(LcCycleSearchSummary)]
            L.lc_cycles_host.restype = ctypes.c_int
        if hasattr(L, "lc_append_check_restricted"):  # (additive to ABI 5: a LINCHECK_LIB may lack it)
            scr, srch = ctypes.POINTER(LcScreenSummary), ctypes.POINTER(LcCycleSearchSummary)
            L.lc_append_check_restricted.argtypes = [vp, p, i64, p, i64, p, i64, ctypes.POINTER(LcApOut),
                                                     ctypes.POINTER(LcApSummary), scr, srch]
            L.lc_append_check_restricted.restype = ctypes.c_int
            L.lc_wr_check_restricted.argtypes = [vp, p, i64, p, i64, ctypes.c_uint32, ctypes.POINTER(LcWrOut),
                                                 ctypes.POINTER(LcWrSummary), scr, srch]
            L.lc_wr_check_restricted.restype = ctypes.c_int
        L.lc_abi_version.argtypes = []
        L.lc_abi_version.restype = ctypes.c_int
        L.lc_synth_register.argtypes = [ctypes.POINTER(LcSynthParams), p, p, p,
                                        ctypes.POINTER(i64), ctypes.c_int]
        L.lc_synth_register.restype = ctypes.c_int
        L.lc_synth_key.argtypes = [ctypes.POINTER(LcSynthParams), i64, p, p, p, i64,
                                   ctypes.POINTER(i64), ctypes.POINTER(i32)]
        L.lc_synth_key.restype = ctypes.c_int
        _lib = L
    return _lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def default_opts(max_configs_per_key=0, init_version=0, init_value=LC_NIL, flags=0,
                 time_budget_ms=0):
    o = LcOpts()
    lib().lc_default_opts(ctypes.byref(o))
    o.max_configs_per_key = max_configs_per_key
    o.time_budget_ms = time_budget_ms
    o.init_version = init_version
    o.init_value = init_value
    o.flags = flags
    return o


def as_ops(ops):
    a = np.ascontiguousarray(ops, dtype=np.int64)
    if a.ndim != 2 or a.shape[1] != 6:
        a = a.reshape(-1, 6)
    return a


def as_ops32(ops32):
    a = np.ascontiguousarray(ops32, dtype=np.int32)
    if a.ndim != 2 or a.shape[1] != 6:
        a = a.reshape(-1, 6)
    return a


def pack32(ops, key_off):
    """lc_pack32 (ABI 4): (ops32 (n, 6) int32, key_base int64 per key), the
    records narrowed by the device's own rules (include/lincheck.h)."""
    ops = as_ops(ops)
    key_off = np.ascontiguousarray(key_off, dtype=np.int64)
    out = np.zeros((len(ops), 6), dtype=np.int32)
    base = np.zeros(max(len(key_off) - 1, 0), dtype=np.int64)
    rc = lib().lc_pack32(_ptr(ops), _ptr(key_off), len(key_off) - 1, _ptr(out), _ptr(base))
    if rc != 0:
        raise LcError(rc, "lc_pack32")
    return out, base


def as_ops16(ops16):
    a = np.ascontiguousarray(ops16, dtype=np.uint32)
    if a.ndim != 2 or a.shape[1] != 4:
        a = a.reshape(-1, 4)
    return a


LC_ID15_MAX = 0x7FFD
ERANGE = 34


def pack16(ops, key_off):
    """lc_pack16 (include/lincheck.h, round 6): (ops16 (n, 4) uint32 — fve,
    version, call, ret — key_base int64 per key), or None when some record
    that is not malformed holds a value or expected id above LC_ID15_MAX
    (the batch then goes as lc_op32: pack32)."""
    ops = as_ops(ops)
    key_off = np.ascontiguousarray(key_off, dtype=np.int64)
    out = np.zeros((len(ops), 4), dtype=np.uint32)
    base = np.zeros(max(len(key_off) - 1, 0), dtype=np.int64)
    rc = lib().lc_pack16(_ptr(ops), _ptr(key_off), len(key_off) - 1, _ptr(out), _ptr(base))
    if rc == -ERANGE:
        return None
    if rc != 0:
        raise LcError(rc, "lc_pack16")
    return out, base


class LcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("lincheck error %d: %s" % (code, msg))
        self.code = code


def as_events(events):
    a = np.ascontiguousarray(events, dtype=np.int32)
    if a.ndim != 2 or a.shape[1] != 6:
        a = a.reshape(-1, 6)
    return a


class _EventsOut:
    """Caller-side arrays of an lc_events_out for `events` over n_keys keys."""

    def __init__(self, events, n_keys):
        # cap: the invokes among the client events (at least what the library counts)
        cap = int(((events[:, 0] >= 0) & ((events[:, 2] & 0xFF) == LC_EV_INVOKE)).sum())
        self.ops32 = np.zeros((cap, 6), dtype=np.int32)
        self.completion = np.full(cap, -3, dtype=np.int32)
        self.key_off = np.zeros(max(n_keys, 0) + 1, dtype=np.int64)
        self.key_base = np.zeros(max(n_keys, 0), dtype=np.int64)
        self.cap = cap
        self.c = LcEventsOut(self.ops32.ctypes.data, self.completion.ctypes.data,
                             self.key_off.ctypes.data, self.key_base.ctypes.data, cap, -1)

    def result(self):
        n = int(self.c.n_ops)
        return self.ops32[:n], self.key_off, self.key_base, self.completion[:n]


def pack_events_host(events, n_keys):
    """lc_events_pack_host: the per-key split and history completion of an
    event array on the host -> (ops32 (n_ops, 6) int32, key_off, key_base,
    completion: per record the position of its completion event or -1)."""
    events = as_events(events)
    out = _EventsOut(events, n_keys)
    rc = lib().lc_events_pack_host(_ptr(events), len(events), n_keys, ctypes.byref(out.c))
    if rc != 0:
        raise LcError(rc, "lc_events_pack_host")
    return out.result()


def events_limits():
    """lc_events_limits: {"max_lds_events", "lds_process_capacity"}."""
    s = LcEventsLimits()
    rc = lib().lc_events_limits(ctypes.byref(s))
    if rc != 0:
        raise LcError(rc, "lc_events_limits")
    return {f: getattr(s, f) for f, _ in LcEventsLimits._fields_}


def _set_full_args(adds, reads, read_values):
    adds = np.ascontiguousarray(adds, dtype=SF_ADD_DTYPE)
    reads = np.ascontiguousarray(reads, dtype=SF_READ_DTYPE)
    read_values = np.ascontiguousarray(read_values, dtype=np.int64)
    return adds, reads, read_values, np.zeros(len(adds), dtype=SF_ELEMENT_DTYPE), LcSfSummary()


def _set_full_summary(s):
    return {f: getattr(s, f) for f, _ in LcSfSummary._fields_}


def set_full_host(adds, reads, read_values, linearizable=True):
    """lc_set_full_host: set-full's rules on the host -> (elements
    (SF_ELEMENT_DTYPE, one per add), the summary as a dict)."""
    adds, reads, read_values, out, s = _set_full_args(adds, reads, read_values)
    rc = lib().lc_set_full_host(_ptr(adds), len(adds), _ptr(reads), len(reads), _ptr(read_values),
                                len(read_values), int(bool(linearizable)), _ptr(out), ctypes.byref(s))
    if rc != 0:
        raise LcError(rc, "lc_set_full_host")
    return out, _set_full_summary(s)


def set_full_limits():
    """lc_set_full_limits: {"tile_bytes", "default_tile_bytes", "max_position", "value_bytes"}."""
    s = LcSfLimits()
    rc = lib().lc_set_full_limits(ctypes.byref(s))
    if rc != 0:
        raise LcError(rc, "lc_set_full_limits")
    return {f: getattr(s, f) for f, _ in LcSfLimits._fields_}


class _TxnGraphCall:
    """What one lc_append_check / lc_wr_check call (device or host) has beside
    its inputs: the output arrays both lc_ap_out and lc_wr_out name, allocated
    as the headers size them, and the summary."""

    def _outputs(self, key_dtype, edge_room):
        """-> the arrays' pointers by name, for the call's out struct."""
        nt, nm = max(len(self.txns), 1), max(len(self.mops), 1)
        i4 = lambda n: np.zeros(n, dtype=np.int32)  # noqa: E731
        self.arrays = {
            "mop_flags": i4(nm), "txn_flags": i4(nt), "keys": np.zeros(nm, dtype=key_dtype),
            "edges": np.zeros(max(edge_room, 1), dtype=AP_EDGE_DTYPE),
            "byc": i4(nt), "rt_lo": i4(nt), "rt_hi": i4(nt), "scc": i4(nt), "scc_class": i4(nt),
            "steps": np.zeros(nt, dtype=AP_STEP_DTYPE),
            "cycle_off": np.zeros(LC_AP_MAX_CYCLES + 1, dtype=np.int64), "cycle_scc": i4(LC_AP_MAX_CYCLES),
        }
        return {k: _ptr(v) for k, v in self.arrays.items()}

    def result(self):
        """-> (a dict of the output arrays cut to their counts, the summary as a dict)."""
        s = {}
        for f, _ in self.summary._fields_:
            v = getattr(self.summary, f)
            s[f] = list(v) if f == "n_class" else v
        a, nt, nm = self.arrays, len(self.txns), len(self.mops)
        n_steps = int(a["cycle_off"][s["n_cycles_returned"]])
        out = {"mop_flags": a["mop_flags"][:nm], "txn_flags": a["txn_flags"][:nt], "keys": a["keys"][:s["n_keys"]],
               "edges": a["edges"][:s["n_edges"]], "byc": a["byc"][:s["n_ok"]], "rt_lo": a["rt_lo"][:nt],
               "rt_hi": a["rt_hi"][:nt], "scc": a["scc"][:nt], "scc_class": a["scc_class"][:nt],
               "steps": a["steps"][:n_steps], "cycle_off": a["cycle_off"][:s["n_cycles_returned"] + 1],
               "cycle_scc": a["cycle_scc"][:s["n_cycles_returned"]]}
        return out, s


class _AppendCall(_TxnGraphCall):
    """One lc_append_check(_host) call's arrays: the inputs made contiguous,
    the outputs allocated as the header sizes them."""

    def __init__(self, txns, mops, values):
        self.txns = np.ascontiguousarray(txns, dtype=AP_TXN_DTYPE)
        self.mops = np.ascontiguousarray(mops, dtype=AP_MOP_DTYPE)
        self.values = np.ascontiguousarray(values, dtype=np.int64)
        n_reads = int((self.mops["f"] == LC_AP_READ).sum())
        self.out = LcApOut(**self._outputs(AP_KEY_DTYPE, n_reads + len(self.mops)))  # 2 reads + appends
        self.summary = LcApSummary()

    def args(self):
        return (_ptr(self.txns), len(self.txns), _ptr(self.mops), len(self.mops), _ptr(self.values),
                len(self.values), ctypes.byref(self.out), ctypes.byref(self.summary))


def append_check_host(txns, mops, values):
    """lc_append_check_host: list-append's rules on the host -> (a dict of the
    output arrays of include/lincheck_append.h's lc_ap_out, the summary as a dict)."""
    call = _AppendCall(txns, mops, values)
    rc = lib().lc_append_check_host(*call.args())
    if rc != 0:
        raise LcError(rc, "lc_append_check_host")
    return call.result()


def append_limits():
    """lc_append_limits: {"max_payload", "default_max_payload", "max_position", "max_mops"}."""
    s = LcApLimits()
    rc = lib().lc_append_limits(ctypes.byref(s))
    if rc != 0:
        raise LcError(rc, "lc_append_limits")
    return {f: getattr(s, f) for f, _ in LcApLimits._fields_}


class _WrCall(_TxnGraphCall):
    """One lc_wr_check(_host) call's arrays: the inputs made contiguous, the
    outputs allocated as the header sizes them, the edges with room for
    edge_cap (None: two per mop and 16, which a history without large reader
    x writer products stays within)."""

    def __init__(self, txns, mops, wfr_keys=True, edge_cap=None):
        self.txns = np.ascontiguousarray(txns, dtype=WR_TXN_DTYPE)
        self.mops = np.ascontiguousarray(mops, dtype=WR_MOP_DTYPE)
        self.flags = LC_WR_WFR_KEYS if wfr_keys else 0
        self.edge_cap = 2 * len(self.mops) + 16 if edge_cap is None else int(edge_cap)
        self.out = LcWrOut(edge_cap=self.edge_cap, **self._outputs(WR_KEY_DTYPE, self.edge_cap))
        self.summary = LcWrSummary()

    def args(self):
        return (_ptr(self.txns), len(self.txns), _ptr(self.mops), len(self.mops), self.flags,
                ctypes.byref(self.out), ctypes.byref(self.summary))


def _wr_run(fn, who, error_text, txns, mops, wfr_keys, edge_cap):
    """The call, made again with room where the edges did not fit a default
    edge_cap (-ENOSPC leaves n_edges in the summary for that)."""
    call = _WrCall(txns, mops, wfr_keys, edge_cap)
    rc = fn(call)
    if rc == -28 and edge_cap is None:
        call = _WrCall(call.txns, call.mops, wfr_keys, int(call.summary.n_edges))
        rc = fn(call)
    if rc != 0:
        raise LcError(rc, error_text() if rc in (-22, -7, -28) else who)
    return call.result()


def wr_check_host(txns, mops, wfr_keys=True, edge_cap=None):
    """lc_wr_check_host: rw-register's rules on the host -> (a dict of the
    output arrays of include/lincheck_wr.h's lc_wr_out, the summary as a dict)."""
    return _wr_run(lambda call: lib().lc_wr_check_host(*call.args()), "lc_wr_check_host",
                   lambda: "lc_wr_check_host", txns, mops, wfr_keys, edge_cap)


def wr_limits():
    """lc_wr_limits: {"max_edges", "default_max_edges", "max_position", "max_mops"}."""
    s = LcWrLimits()
    rc = lib().lc_wr_limits(ctypes.byref(s))
    if rc != 0:
        raise LcError(rc, "lc_wr_limits")
    return {f: getattr(s, f) for f, _ in LcWrLimits._fields_}


class _WrLinCall(_WrCall):
    """One lc_wr_check_lin(_host) call's arrays: _WrCall's, the flags with the
    lin bit, and the lc_wr_lin_key records and the lin summary beside them."""

    def __init__(self, txns, mops, wfr_keys=True, linearizable_keys=True, edge_cap=None):
        super().__init__(txns, mops, wfr_keys, edge_cap)
        if linearizable_keys:
            self.flags |= LC_WR_LINEARIZABLE_KEYS
        self.lin_keys = np.zeros(max(len(self.mops), 1), dtype=WR_LIN_KEY_DTYPE)
        self.lin_summary = LcWrLinSummary()

    def args(self):
        return super().args() + (_ptr(self.lin_keys), ctypes.byref(self.lin_summary))

    def result(self):
        """-> (the output arrays with "lin_keys" among them, the summary, the lin summary)."""
        out, s = super().result()
        out["lin_keys"] = self.lin_keys[:s["n_keys"]]
        return out, s, _struct_dict(self.lin_summary)


def _wr_lin_run(fn, who, error_text, txns, mops, wfr_keys, linearizable_keys, edge_cap):
    """_wr_run for the lin calls: made again with room after -ENOSPC."""
    call = _WrLinCall(txns, mops, wfr_keys, linearizable_keys, edge_cap)
    rc = fn(call)
    if rc == -28 and edge_cap is None:
        call = _WrLinCall(call.txns, call.mops, wfr_keys, linearizable_keys, int(call.summary.n_edges))
        rc = fn(call)
    if rc != 0:
        raise LcError(rc, error_text() if rc in (-22, -7, -28) else who)
    return call.result()


def has_wr_lin():
    """Whether the loaded library has lc_wr_check_lin (a LINCHECK_LIB may lack it)."""
    return hasattr(lib(), "lc_wr_check_lin")


def wr_check_lin_host(txns, mops, wfr_keys=True, linearizable_keys=True, edge_cap=None):
    """lc_wr_check_lin_host (include/lincheck_wrlin.h) -> (wr_check_host's
    output arrays and "lin_keys", the summary, the lin summary)."""
    return _wr_lin_run(lambda call: lib().lc_wr_check_lin_host(*call.args()), "lc_wr_check_lin_host",
                       lambda: "lc_wr_check_lin_host", txns, mops, wfr_keys, linearizable_keys, edge_cap)


def wr_lin_limits():
    """lc_wr_lin_limits: {"max_key_versions", "wave_key_versions"}."""
    s = LcWrLinLimits()
    rc = lib().lc_wr_lin_limits(ctypes.byref(s))
    if rc != 0:
        raise LcError(rc, "lc_wr_lin_limits")
    return _struct_dict(s)


def has_screened():
    """Whether the loaded library has the screened checker calls (a LINCHECK_LIB may lack them)."""
    return hasattr(lib(), "lc_append_check_screened")


def _screen_dict(s):
    return {f: getattr(s, f) for f, _ in LcScreenSummary._fields_}


class _ScreenCall:
    """One lc_cycle_screen(_host) call's arrays: the inputs made contiguous,
    the three output arrays, one entry per txn."""

    def __init__(self, txns, edges):
        self.txns = np.ascontiguousarray(txns, dtype=AP_TXN_DTYPE)
        self.edges = np.ascontiguousarray(edges, dtype=AP_EDGE_DTYPE)
        nt = max(len(self.txns), 1)
        self.arrays = {f: np.zeros(nt, dtype=np.int32) for f in ("reach_lo", "reach_hi", "mark")}
        self.out = LcScreenOut(**{k: _ptr(v) for k, v in self.arrays.items()})
        self.summary = LcScreenSummary()

    def args(self):
        return (_ptr(self.txns), len(self.txns), _ptr(self.edges), len(self.edges), ctypes.byref(self.out),
                ctypes.byref(self.summary))

    def result(self):
        """-> (a dict of the output arrays, the summary as a dict)."""
        nt = len(self.txns)
        return ({k: v[:nt] for k, v in self.arrays.items()},
                {f: getattr(self.summary, f) for f, _ in LcScreenSummary._fields_})


def cycle_screen_host(txns, edges):
    """lc_cycle_screen_host: the screen of include/lincheck_screen.h on the host
    -> ({"reach_lo", "reach_hi", "mark"}, the summary as a dict)."""
    call = _ScreenCall(txns, edges)
    rc = lib().lc_cycle_screen_host(*call.args())
    if rc != 0:
        raise LcError(rc, "lc_cycle_screen_host")
    return call.result()


def screen_limits():
    """lc_screen_limits: {"max_rounds", "default_max_rounds"}."""
    s = LcScreenLimits()
    rc = lib().lc_screen_limits(ctypes.byref(s))
    if rc != 0:
        raise LcError(rc, "lc_screen_limits")
    return {f: getattr(s, f) for f, _ in LcScreenLimits._fields_}


def has_restricted():
    """Whether the loaded library has the restricted checker calls (a LINCHECK_LIB may lack them)."""
    return hasattr(lib(), "lc_append_check_restricted")


def _struct_dict(s):
    return {f: getattr(s, f) for f, _ in s._fields_ if f != "pad"}


class _ReachCall:
    """One lc_cycle_reach(_host) call's arrays: the inputs made contiguous, hit
    with one entry per query."""

    def __init__(self, n_nodes, pred_off, pred, q_node, q_head_off, q_heads, all_queries):
        self.n_nodes = int(n_nodes)
        self.pred_off = np.ascontiguousarray(pred_off, dtype=np.int64)
        self.pred = np.ascontiguousarray(pred, dtype=np.int32)
        self.q_node = np.ascontiguousarray(q_node, dtype=np.int32)
        self.q_head_off = np.ascontiguousarray(q_head_off, dtype=np.int64)
        self.q_heads = np.ascontiguousarray(q_heads, dtype=np.int32)
        self.flags = LC_REACH_ALL if all_queries else 0
        # (-7: what no call writes, so a test can see that nothing was written)
        self.hit = np.full(max(len(self.q_node), 1), -7, dtype=np.int32)
        self.summary = LcReachSummary()

    def args(self):
        return (self.n_nodes, _ptr(self.pred_off), _ptr(self.pred), len(self.pred), len(self.q_node),
                _ptr(self.q_node), _ptr(self.q_head_off), _ptr(self.q_heads), len(self.q_heads), self.flags,
                _ptr(self.hit), ctypes.byref(self.summary))

    def result(self):
        """-> (hit, one entry per query, or None without all_queries; the summary as a dict)."""
        return (self.hit[:len(self.q_node)] if self.flags else None), _struct_dict(self.summary)


def cycle_reach_host(n_nodes, pred_off, pred, q_node, q_head_off, q_heads, all_queries=False):
    """lc_cycle_reach_host: batched backward reachability, first hit
    (include/lincheck_cycles.h), on the host -> (hit or None, the summary as a dict)."""
    call = _ReachCall(n_nodes, pred_off, pred, q_node, q_head_off, q_heads, all_queries)
    rc = lib().lc_cycle_reach_host(*call.args())
    if rc != 0:
        err = LcError(rc, "lc_cycle_reach_host")
        err.call = call
        raise err
    return call.result()


def cycle_reach_limits():
    """lc_cycle_reach_limits: {"max_nodes", "min_work", "default_min_work", "max_workgroups"}."""
    s = LcReachLimits()
    rc = lib().lc_cycle_reach_limits(ctypes.byref(s))
    if rc != 0:
        raise LcError(rc, "lc_cycle_reach_limits")
    return _struct_dict(s)


def cycles_host(txns, edges, mark=None, reach=None, min_work=0, max_nodes=0):
    """lc_cycles_host: rule 7 alone on the host, over the whole graph (mark
    None) or over the marked txns; reach(n_nodes, pred_off, pred, q_node,
    q_head_off, q_heads) -> first_hit answers the class loop's searches in
    place of the host loop (None: it refuses, and the host loop runs, as it
    does for a search over more than max_nodes > 0 nodes) -> (a dict of scc, scc_class, steps, cycle_off,
    cycle_scc, n_class, n_scc; the search summary as a dict)."""
    txns = np.ascontiguousarray(txns, dtype=AP_TXN_DTYPE)
    edges = np.ascontiguousarray(edges, dtype=AP_EDGE_DTYPE)
    nt = max(len(txns), 1)
    out = {"scc": np.zeros(nt, np.int32), "scc_class": np.zeros(nt, np.int32),
           "steps": np.zeros(nt, dtype=AP_STEP_DTYPE), "cycle_off": np.zeros(LC_AP_MAX_CYCLES + 1, np.int64),
           "cycle_scc": np.zeros(LC_AP_MAX_CYCLES, np.int32), "n_class": np.zeros(8, np.int64)}
    n_scc, srch = ctypes.c_int64(0), LcCycleSearchSummary()
    if mark is not None:
        mark = np.ascontiguousarray(mark, dtype=np.int32)

    def hook(_user, n_nodes, pred_off, pred, n_queries, q_node, q_head_off, q_heads, first_hit):
        po = np.ctypeslib.as_array(pred_off, (n_nodes + 1,))
        qo = np.ctypeslib.as_array(q_head_off, (n_queries + 1,))
        pr = np.ctypeslib.as_array(pred, (int(po[-1]),)) if po[-1] else np.zeros(0, np.int32)
        qh = np.ctypeslib.as_array(q_heads, (int(qo[-1]),)) if qo[-1] else np.zeros(0, np.int32)
        first = reach(n_nodes, po, pr, np.ctypeslib.as_array(q_node, (n_queries,)), qo, qh)
        if first is None:
            return 1
        first_hit[0] = int(first)
        return 0

    fn = LC_REACH_FN(hook) if reach is not None else LC_REACH_FN()
    rc = lib().lc_cycles_host(_ptr(txns), len(txns), _ptr(edges), len(edges), _ptr(mark) if mark is not None else None,
                              fn, None, int(min_work), int(max_nodes), _ptr(out["scc"]), _ptr(out["scc_class"]),
                              _ptr(out["steps"]),
                              _ptr(out["cycle_off"]), _ptr(out["cycle_scc"]), _ptr(out["n_class"]),
                              ctypes.byref(n_scc), ctypes.byref(srch))
    if rc != 0:
        raise LcError(rc, "lc_cycles_host")
    out["scc"], out["scc_class"] = out["scc"][:len(txns)], out["scc_class"][:len(txns)]
    out["steps"] = out["steps"][:int(out["cycle_off"][-1])]
    out["n_scc"] = n_scc.value
    return out, _struct_dict(srch)


class _WatchCall:
    """One lc_watch_check(_host) call's arrays: the inputs made contiguous,
    the outputs allocated as the header sizes them, the edits with room for
    edit_cap (None: 4,096, and as many as the call then asks for)."""

    def __init__(self, threads, values, n_nonmonotonic=0, flags=0, edit_cap=None):
        self.threads = np.ascontiguousarray(threads, dtype=WT_THREAD_DTYPE)
        self.values = np.ascontiguousarray(values, dtype=np.int64)
        self.n_nonmonotonic, self.flags = int(n_nonmonotonic), int(flags)
        nt = max(len(self.threads), 1)
        self.edit_cap = 4096 if edit_cap is None else int(edit_cap)
        self.arrays = {"cls": np.zeros(nt, dtype=np.int32), "distance": np.zeros(nt, dtype=np.int64),
                       "deltas": np.zeros(nt, dtype=WT_DELTA_DTYPE),
                       "edits": np.zeros(max(self.edit_cap, 1), dtype=WT_EDIT_DTYPE)}
        self.out = LcWtOut(edit_cap=self.edit_cap, **{k: _ptr(v) for k, v in self.arrays.items()})
        self.summary = LcWtSummary()

    def args(self):
        return (_ptr(self.threads), len(self.threads), _ptr(self.values), len(self.values), self.n_nonmonotonic,
                self.flags, ctypes.byref(self.out), ctypes.byref(self.summary))

    def result(self):
        """-> (a dict of the output arrays cut to their counts, the summary as a dict)."""
        s = {f: getattr(self.summary, f) for f, _ in LcWtSummary._fields_}
        a, nt = self.arrays, len(self.threads)
        return {"cls": a["cls"][:nt], "distance": a["distance"][:nt], "deltas": a["deltas"][:s["n_deltas"]],
                "edits": a["edits"][:s["n_edits"]]}, s


def _watch_run(fn, who, error_text, threads, values, n_nonmonotonic, flags, edit_cap):
    """The call, made again with room where the scripts did not fit a default
    edit_cap (-ENOSPC leaves n_edits in the summary for that)."""
    call = _WatchCall(threads, values, n_nonmonotonic, flags, edit_cap)
    rc = fn(call)
    if rc == -28 and edit_cap is None:
        call = _WatchCall(call.threads, call.values, n_nonmonotonic, flags, int(call.summary.n_edits))
        rc = fn(call)
    if rc != 0:
        err = LcError(rc, error_text() if rc in (-22, -7, -28) else who)
        err.n_edits = int(call.summary.n_edits) if rc == -28 else None
        raise err
    return call.result()


def watch_check_host(threads, values, n_nonmonotonic=0, flags=0, edit_cap=None):
    """lc_watch_check_host: the watch checker's rules on the host -> (a dict of
    the output arrays of include/lincheck_watch.h's lc_wt_out, the summary as a
    dict).  -ENOSPC with a given edit_cap raises LcError with n_edits set."""
    return _watch_run(lambda call: lib().lc_watch_check_host(*call.args()), "lc_watch_check_host",
                      lambda: "lc_watch_check_host", threads, values, n_nonmonotonic, flags, edit_cap)


def watch_limits():
    """lc_watch_limits: {"max_d", "default_max_d", "trace_bytes", "default_trace_bytes", "max_len",
    "max_device_len", "hash_mask"}."""
    s = LcWtLimits()
    rc = lib().lc_watch_limits(ctypes.byref(s))
    if rc != 0:
        raise LcError(rc, "lc_watch_limits")
    return {f: getattr(s, f) for f, _ in LcWtLimits._fields_}


class _PerfStatsCall:
    """One lc_perf_stats(_host) call's arrays: the events made contiguous, the
    tables allocated with rate_cap / quant_cap buckets per row (None: rule 7's
    counts, from the client events' largest time), the point arrays on
    request."""

    def __init__(self, events, n_f, qs, rate_dt_ns, quant_dt_ns, points, rate_cap, quant_cap):
        self.events = np.ascontiguousarray(events, dtype=PS_EVENT_DTYPE)
        qs = [float(q) for q in qs]
        self.params = LcPsParams(n_f=int(n_f), n_q=len(qs), rate_dt_ns=int(rate_dt_ns), quant_dt_ns=int(quant_dt_ns))
        for i, q in enumerate(qs[:LC_PS_MAX_Q]):
            self.params.q[i] = q
        n, nf, nq = len(self.events), max(int(n_f), 1), min(len(qs), LC_PS_MAX_Q)
        client = self.events["time"][self.events["process"] >= 0]
        t_max = max(int(client.max()), 0) if len(client) else 0
        if rate_cap is None:
            rate_cap = t_max // int(rate_dt_ns) + 1 if rate_dt_ns > 0 else 1
        if quant_cap is None:
            quant_cap = t_max // int(quant_dt_ns) + 1 if quant_dt_ns > 0 else 1
        self.rate_cap, self.quant_cap = int(rate_cap), int(quant_cap)
        if max(nf * 3 * self.rate_cap, nf * self.quant_cap * max(nq, 1)) > 1 << 28:  # (the library answers -E2BIG)
            self.rate_cap = self.quant_cap = 1
        self.arrays = {"by_f": np.zeros((nf, 4), dtype=np.int64),
                       "rate": np.zeros((nf, 3, max(self.rate_cap, 0)), dtype=np.int64),
                       "quant": np.zeros((nf, max(self.quant_cap, 0), nq), dtype=np.int64),
                       "quant_n": np.zeros((nf, max(self.quant_cap, 0)), dtype=np.int64),
                       "comp_pos": np.zeros(n, dtype=np.int32) if points else None,
                       "latency_ns": np.zeros(n, dtype=np.int64) if points else None}
        # (a pointer that is never NULL for the tables: an empty array's may be)
        self._room = {k: (v if v is None or v.size else np.zeros(1, dtype=v.dtype)) for k, v in self.arrays.items()}
        self.out = LcPsOut(rate_cap=self.rate_cap, quant_cap=self.quant_cap,
                           **{k: _ptr(v) for k, v in self._room.items()})
        self.summary = LcPsSummary()

    def args(self):
        return (_ptr(self.events) if len(self.events) else None, len(self.events), ctypes.byref(self.params),
                ctypes.byref(self.out), ctypes.byref(self.summary))

    def result(self):
        return self.arrays, {f: getattr(self.summary, f) for f, _ in LcPsSummary._fields_ if f != "pad"}


def _perf_stats_run(fn, error_text, events, n_f, qs, rate_dt_ns, quant_dt_ns, points, rate_cap, quant_cap):
    call = _PerfStatsCall(events, n_f, qs, rate_dt_ns, quant_dt_ns, points, rate_cap, quant_cap)
    rc = fn(call)
    if rc != 0:
        err = LcError(rc, error_text())
        # -ENOSPC: rule 7's counts, for a call with room
        err.needed = (int(call.summary.n_rate_buckets), int(call.summary.n_quant_buckets)) if rc == -28 else None
        raise err
    return call.result()


def perf_stats_host(events, n_f, qs=PS_DEFAULT_QS, rate_dt_ns=PS_DEFAULT_RATE_DT_NS,
                    quant_dt_ns=PS_DEFAULT_QUANT_DT_NS, points=True, rate_cap=None, quant_cap=None):
    """lc_perf_stats_host: the rules of include/lincheck_perf.h on the host ->
    (a dict of lc_ps_out's arrays: by_f (n_f, 4), rate (n_f, 3, buckets), quant
    (n_f, buckets, n_q), quant_n (n_f, buckets), comp_pos and latency_ns (None
    without points); the summary as a dict).  The tables have rule 7's bucket
    counts unless rate_cap / quant_cap say otherwise; -ENOSPC raises LcError
    with .needed = (n_rate_buckets, n_quant_buckets)."""
    return _perf_stats_run(lambda call: lib().lc_perf_stats_host(*call.args()), lambda: "lc_perf_stats_host",
                           events, n_f, qs, rate_dt_ns, quant_dt_ns, points, rate_cap, quant_cap)


def perf_stats_limits():
    """lc_perf_stats_limits: {"max_f", "max_table_entries", "lds_entries", "default_lds_entries", "wave",
    "block", "chunk", "max_grid"}."""
    s = LcPsLimits()
    rc = lib().lc_perf_stats_limits(ctypes.byref(s))
    if rc != 0:
        raise LcError(rc, "lc_perf_stats_limits")
    return {f: getattr(s, f) for f, _ in LcPsLimits._fields_}


class Context:
    """An lc_ctx on the GPUs of device_mask (0 = all)."""

    def __init__(self, device_mask=0):
        h = ctypes.c_void_p()
        rc = lib().lc_open(device_mask, ctypes.byref(h))
        if rc != 0:
            raise LcError(rc, "lc_open failed (no usable GPU; there is no CPU fallback)")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().lc_close(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def last_error(self):
        return lib().lc_last_error(self._h).decode()

    def stats(self):
        s = self.stats_raw()
        return {f: getattr(s, f) for f, _ in LcStats._fields_}

    def stats_raw(self, into=None):
        """lc_last_stats into an LcStats struct (reused when given)."""
        s = into if into is not None else LcStats()
        lib().lc_last_stats(self._h, ctypes.byref(s))
        return s

    def counted_stats(self):
        """lc_last_counted_stats: the counted tier's share of the last call
        (LC_FLAG_COUNTED_CLASSES), summed over its devices."""
        s = LcCountedStats()
        rc = lib().lc_last_counted_stats(self._h, ctypes.byref(s))
        if rc != 0:
            raise LcError(rc, "lc_last_counted_stats")
        return {f: getattr(s, f) for f, _ in LcCountedStats._fields_}

    def last_witness_stats(self):
        """lc_last_witness_stats: the witness search's share of the last call
        (LC_FLAG_SEARCH_WITNESS), summed over its devices."""
        s = LcWitnessStats()
        rc = lib().lc_last_witness_stats(self._h, ctypes.byref(s))
        if rc != 0:
            raise LcError(rc, "lc_last_witness_stats")
        return {f: getattr(s, f) for f, _ in LcWitnessStats._fields_}

    def last_counted_witness_stats(self):
        """lc_last_counted_witness_stats: the share of the counted witness
        stage (LC_FLAG_SEARCH_WITNESS | LC_FLAG_COUNTED_WITNESS) of the last
        call, summed over its devices."""
        s = LcCountedWitnessStats()
        rc = lib().lc_last_counted_witness_stats(self._h, ctypes.byref(s))
        if rc != 0:
            raise LcError(rc, "lc_last_counted_witness_stats")
        return {f: getattr(s, f) for f, _ in LcCountedWitnessStats._fields_}

    def device_stats(self):
        """lc_last_device_stats for every device of the last lc_check: one
        dict per device (its key range, copies, kernels, wall time)."""
        out = []
        for i in range(int(self.stats_raw().n_devices)):
            d = LcDeviceStats()
            if lib().lc_last_device_stats(self._h, i, ctypes.byref(d)) != 0:
                break
            out.append({f: getattr(d, f) for f, _ in LcDeviceStats._fields_})
        return out

    def host_register(self, arr):
        """lc_host_register: page-lock a numpy array's buffer for repeated
        lc_check calls (unregister with host_unregister before freeing it)."""
        rc = lib().lc_host_register(self._h, ctypes.c_void_p(arr.ctypes.data), arr.nbytes)
        if rc != 0:
            raise LcError(rc, self.last_error())

    def host_unregister(self, arr):
        rc = lib().lc_host_unregister(self._h, ctypes.c_void_p(arr.ctypes.data))
        if rc != 0:
            raise LcError(rc, self.last_error())

    def _check_host(self, fn, ops, key_off, extra, opts, raise_on_error, witness, certificate):
        key_off = np.ascontiguousarray(key_off, dtype=np.int64)
        n_keys = len(key_off) - 1
        out = np.zeros(max(n_keys, 0), dtype=RESULT_DTYPE)
        o = opts if opts is not None else default_opts()
        wit = kind = cert = cset = None
        aux = None
        if witness or certificate:
            wit = np.full(len(ops), -3, dtype=np.int32)
            kind = np.full(max(n_keys, 0), -3, dtype=np.int32)
            if certificate:
                cert = np.full((max(n_keys, 0), 4), -3, dtype=np.int32)
                cset = np.zeros(len(ops), dtype=np.int32)
            aux = ctypes.byref(LcAux(wit.ctypes.data, kind.ctypes.data,
                                     cert.ctypes.data if certificate else None,
                                     cset.ctypes.data if certificate else None))
        rc = fn(self._h, _ptr(ops), _ptr(key_off), *extra, n_keys, ctypes.byref(o), _ptr(out), aux)
        if rc != 0 and raise_on_error:
            raise LcError(rc, self.last_error())
        if certificate:
            return rc, out, wit, kind, cert, cset
        return (rc, out, wit, kind) if witness else (rc, out)

    def check(self, ops, key_off, opts=None, raise_on_error=True, witness=False,
              certificate=False):
        """Host-buffer check. Returns (rc, results structured array), or with
        witness=True (rc, results, witness per record, witness kind per key)
        from lc_check_ex (include/lincheck.h, lc_aux); certificate=True adds
        the infeasibility certificates (int32[n_keys, 4]) and their position
        sets (int32 per record): (rc, results, witness, kind, cert, cert_set)."""
        return self._check_host(lib().lc_check_ex, as_ops(ops), key_off, (), opts,
                                raise_on_error, witness, certificate)

    def check32(self, ops32, key_off, key_base=None, opts=None, raise_on_error=True,
                witness=False, certificate=False):
        """lc_check32 (ABI 4): 24-byte records from host memory ((n, 6) int32,
        as pack32 makes them) and their key bases; returns as check()."""
        ops32 = as_ops32(ops32)
        base = None if key_base is None else np.ascontiguousarray(key_base, dtype=np.int64)
        if base is not None and len(base) != len(key_off) - 1:
            # lc_check32 reads n_keys bases: a short array would be read past its end
            raise ValueError(f"key_base has {len(base)} entries for {len(key_off) - 1} keys")
        return self._check_host(lib().lc_check32, ops32, key_off, (_ptr(base),), opts,
                                raise_on_error, witness, certificate)

    def check16(self, ops16, key_off, key_base=None, opts=None, raise_on_error=True,
                witness=False, certificate=False):
        """lc_check16 (round 6): 16-byte records from host memory ((n, 4)
        uint32, as pack16 makes them) and their key bases; returns as check()."""
        ops16 = as_ops16(ops16)
        base = None if key_base is None else np.ascontiguousarray(key_base, dtype=np.int64)
        if base is not None and len(base) != len(key_off) - 1:
            raise ValueError(f"key_base has {len(base)} entries for {len(key_off) - 1} keys")
        return self._check_host(lib().lc_check16, ops16, key_off, (_ptr(base),), opts,
                                raise_on_error, witness, certificate)

    def events_pack(self, events, n_keys):
        """lc_events_pack: pack_events_host's result, computed on the device."""
        events = as_events(events)
        out = _EventsOut(events, n_keys)
        rc = lib().lc_events_pack(self._h, _ptr(events), len(events), n_keys, ctypes.byref(out.c))
        if rc != 0:
            raise LcError(rc, self.last_error())
        return out.result()

    def check_events(self, events, n_keys, opts=None, raise_on_error=True, witness=False,
                     certificate=False, packed=False):
        """lc_check_events: split, completion and check of an event array on
        the device.  Returns as check() — the per-record outputs indexed like
        the packed records — and with packed=True one more element, the
        records as pack_events_host returns them."""
        events = as_events(events)
        out = np.zeros(max(n_keys, 0), dtype=RESULT_DTYPE)
        o = opts if opts is not None else default_opts()
        pk = _EventsOut(events, n_keys) if packed or witness or certificate else None
        wit = kind = cert = cset = None
        aux = None
        if witness or certificate:
            wit = np.full(pk.cap, -3, dtype=np.int32)
            kind = np.full(max(n_keys, 0), -3, dtype=np.int32)
            if certificate:
                cert = np.full((max(n_keys, 0), 4), -3, dtype=np.int32)
                cset = np.zeros(pk.cap, dtype=np.int32)
            aux = ctypes.byref(LcAux(wit.ctypes.data, kind.ctypes.data,
                                     cert.ctypes.data if certificate else None,
                                     cset.ctypes.data if certificate else None))
        rc = lib().lc_check_events(self._h, _ptr(events), len(events), n_keys, ctypes.byref(o),
                                   _ptr(out), aux, ctypes.byref(pk.c) if pk else None)
        if rc != 0 and raise_on_error:
            raise LcError(rc, self.last_error())
        n_ops = max(int(pk.c.n_ops), 0) if pk else 0
        ret = (rc, out)
        if certificate:
            ret = (rc, out, wit[:n_ops], kind, cert, cset[:n_ops])
        elif witness:
            ret = (rc, out, wit[:n_ops], kind)
        return ret + (pk.result(),) if packed else ret

    def append_check(self, txns, mops, values):
        """lc_append_check: append_check_host's result, with rules 1-6 on the device."""
        call = _AppendCall(txns, mops, values)
        rc = lib().lc_append_check(self._h, *call.args())
        if rc != 0:
            raise LcError(rc, self.last_error() if rc in (-22, -7) else "lc_append_check")
        return call.result()

    def append_check_screened(self, txns, mops, values):
        """lc_append_check_screened: append_check's result, and the screen's
        summary as a third value; rule 7 runs on the host only where the
        screen did not prove the graph clean."""
        call, scr = _AppendCall(txns, mops, values), LcScreenSummary()
        rc = lib().lc_append_check_screened(self._h, *call.args(), ctypes.byref(scr))
        if rc != 0:
            raise LcError(rc, self.last_error() if rc in (-22, -7) else "lc_append_check_screened")
        return call.result() + (_screen_dict(scr),)

    def wr_check_screened(self, txns, mops, wfr_keys=True, edge_cap=None):
        """lc_wr_check_screened: wr_check's result, and the screen's summary as
        a third value; rule 9 runs on the host only where the screen did not
        prove the graph clean."""
        scr = LcScreenSummary()
        out, s = _wr_run(lambda call: lib().lc_wr_check_screened(self._h, *call.args(), ctypes.byref(scr)),
                         "lc_wr_check_screened", self.last_error, txns, mops, wfr_keys, edge_cap)
        return out, s, _screen_dict(scr)

    def append_check_restricted(self, txns, mops, values):
        """lc_append_check_restricted: append_check_screened's result, and the
        cycle search's summary as a fourth value; where the screen did not
        prove the graph clean, rule 7 runs over the marked txns only."""
        call, scr, srch = _AppendCall(txns, mops, values), LcScreenSummary(), LcCycleSearchSummary()
        rc = lib().lc_append_check_restricted(self._h, *call.args(), ctypes.byref(scr), ctypes.byref(srch))
        if rc != 0:
            raise LcError(rc, self.last_error() if rc in (-22, -7) else "lc_append_check_restricted")
        return call.result() + (_screen_dict(scr), _struct_dict(srch))

    def wr_check_restricted(self, txns, mops, wfr_keys=True, edge_cap=None):
        """lc_wr_check_restricted: wr_check_screened's result, and the cycle
        search's summary as a fourth value."""
        scr, srch = LcScreenSummary(), LcCycleSearchSummary()
        out, s = _wr_run(lambda call: lib().lc_wr_check_restricted(self._h, *call.args(), ctypes.byref(scr),
                                                                   ctypes.byref(srch)),
                         "lc_wr_check_restricted", self.last_error, txns, mops, wfr_keys, edge_cap)
        return out, s, _screen_dict(scr), _struct_dict(srch)

    def cycle_reach(self, n_nodes, pred_off, pred, q_node, q_head_off, q_heads, all_queries=False):
        """lc_cycle_reach: cycle_reach_host's result, computed on the device."""
        call = _ReachCall(n_nodes, pred_off, pred, q_node, q_head_off, q_heads, all_queries)
        rc = lib().lc_cycle_reach(self._h, *call.args())
        if rc != 0:
            err = LcError(rc, self.last_error() if rc in (-22, -7) else "lc_cycle_reach")
            err.call = call
            raise err
        return call.result()

    def watch_check(self, threads, values, n_nonmonotonic=0, flags=0, edit_cap=None):
        """lc_watch_check: watch_check_host's result, with the hashes, the
        compares, the forward passes and the backtracks on the device."""
        return _watch_run(lambda call: lib().lc_watch_check(self._h, *call.args()), "lc_watch_check",
                          self.last_error, threads, values, n_nonmonotonic, flags, edit_cap)

    def perf_stats(self, events, n_f, qs=PS_DEFAULT_QS, rate_dt_ns=PS_DEFAULT_RATE_DT_NS,
                   quant_dt_ns=PS_DEFAULT_QUANT_DT_NS, points=True, rate_cap=None, quant_cap=None):
        """lc_perf_stats: perf_stats_host's result, with the sorts, the pair
        pass and the quantile selection on the device."""
        return _perf_stats_run(lambda call: lib().lc_perf_stats(self._h, *call.args()), self.last_error,
                               events, n_f, qs, rate_dt_ns, quant_dt_ns, points, rate_cap, quant_cap)

    def wr_check(self, txns, mops, wfr_keys=True, edge_cap=None):
        """lc_wr_check: wr_check_host's result, with rules 1-8 on the device."""
        return _wr_run(lambda call: lib().lc_wr_check(self._h, *call.args()), "lc_wr_check", self.last_error,
                       txns, mops, wfr_keys, edge_cap)

    def wr_check_lin(self, txns, mops, wfr_keys=True, linearizable_keys=True, edge_cap=None):
        """lc_wr_check_lin: wr_check_lin_host's result, with rules 1-8 on the device."""
        return _wr_lin_run(lambda call: lib().lc_wr_check_lin(self._h, *call.args()), "lc_wr_check_lin",
                           self.last_error, txns, mops, wfr_keys, linearizable_keys, edge_cap)

    def cycle_screen(self, txns, edges):
        """lc_cycle_screen: cycle_screen_host's result, computed on the device."""
        call = _ScreenCall(txns, edges)
        rc = lib().lc_cycle_screen(self._h, *call.args())
        if rc != 0:
            raise LcError(rc, self.last_error() if rc == -22 else "lc_cycle_screen")
        return call.result()

    def set_full(self, adds, reads, read_values, linearizable=True):
        """lc_set_full: set_full_host's result, computed on the device."""
        adds, reads, read_values, out, s = _set_full_args(adds, reads, read_values)
        rc = lib().lc_set_full(self._h, _ptr(adds), len(adds), _ptr(reads), len(reads),
                               _ptr(read_values), len(read_values), int(bool(linearizable)),
                               _ptr(out), ctypes.byref(s))
        if rc != 0:
            raise LcError(rc, self.last_error() if rc == -22 else "lc_set_full")
        return out, _set_full_summary(s)

    def last_events_stats(self):
        """lc_last_events_stats: the last events_pack / check_events call."""
        s = LcEventsStats()
        rc = lib().lc_last_events_stats(self._h, ctypes.byref(s))
        if rc != 0:
            raise LcError(rc, "lc_last_events_stats")
        return {f: getattr(s, f) for f, _ in LcEventsStats._fields_}

    def check_frontiers(self, ops, key_off, stop_ops, max_per_key=10, opts=None):
        """lc_check_frontiers (include/lincheck_fx.h, ABI 4): for every key,
        up to max_per_key configurations of its JIT frontier just before the
        :ok return of record stop_ops[k], as (version, value id, pending
        record indices) tuples — or None where the device search could not
        get there (the caller's fallback: FrontierExchange.frontier)."""
        from .fx import LcFxConfig
        ops = as_ops(ops)
        key_off = np.ascontiguousarray(key_off, dtype=np.int64)
        n_keys = len(key_off) - 1
        stop = np.ascontiguousarray(stop_ops, dtype=np.int64)
        if len(stop) != n_keys:
            raise ValueError(f"stop_ops has {len(stop)} entries for {n_keys} keys")
        buf = (LcFxConfig * max(1, n_keys * max_per_key))()
        n_out = np.zeros(max(n_keys, 1), dtype=np.int32)
        o = opts if opts is not None else default_opts()
        rc = lib().lc_check_frontiers(self._h, _ptr(ops), _ptr(key_off), n_keys, _ptr(stop),
                                      ctypes.byref(o), ctypes.cast(buf, ctypes.c_void_p),
                                      max_per_key, _ptr(n_out))
        if rc != 0:
            raise LcError(rc, self.last_error())
        out = []
        for k in range(n_keys):
            n = int(n_out[k])
            if n < 0:
                out.append(None)
                continue
            out.append([(int(c.version), int(c.value), tuple(int(c.pending[j]) for j in range(c.n_pending)))
                        for c in buf[k * max_per_key:k * max_per_key + n]])
        return out

    def check_frontiers_counted(self, ops, key_off, stop_ops, max_per_key=10, opts=None):
        """lc_check_frontiers_counted (include/lincheck_counted.h): as
        check_frontiers, from the counted search — keys with more than 64 ops
        open, every pending list whole.  Returns (configs, totals):
        configs[k] is None where the search could not get there, else up to
        max_per_key (version, value id, pending record indices) tuples;
        totals[k] (int64) is the frontier's size, -1 with None."""
        ops = as_ops(ops)
        key_off = np.ascontiguousarray(key_off, dtype=np.int64)
        n_keys = len(key_off) - 1
        stop = np.ascontiguousarray(stop_ops, dtype=np.int64)
        if len(stop) != n_keys:
            raise ValueError(f"stop_ops has {len(stop)} entries for {n_keys} keys")
        if n_keys <= 0:
            return [], np.zeros(0, dtype=np.int64)
        cap = int(max_per_key) * int(key_off[-1] - key_off[0])
        cfg = np.zeros(n_keys * max(int(max_per_key), 0), dtype=COUNTED_CONFIG_DTYPE)
        pending = np.empty(max(cap, 1), dtype=np.int64)
        n_out = np.zeros(n_keys, dtype=np.int32)
        totals = np.zeros(n_keys, dtype=np.int64)
        o = opts if opts is not None else default_opts()
        rc = lib().lc_check_frontiers_counted(self._h, _ptr(ops), _ptr(key_off), n_keys, _ptr(stop),
                                              ctypes.byref(o), _ptr(cfg), max_per_key, _ptr(n_out),
                                              _ptr(totals), _ptr(pending), cap)
        if rc != 0:
            raise LcError(rc, self.last_error())
        out = []
        for k in range(n_keys):
            n = int(n_out[k])
            if n <= 0:
                out.append(None if n < 0 else [])
                continue
            c = cfg[k * max_per_key:k * max_per_key + n]
            # one slice of `pending` per configuration, one tolist() per key
            at, npend = c["pending_at"], c["n_pending"]
            idx = np.repeat(at - np.concatenate(([0], np.cumsum(npend)[:-1])), npend) + \
                np.arange(int(npend.sum()))
            flat = pending[idx].tolist()
            ends = np.cumsum(npend).tolist()
            out.append([(v, x, tuple(flat[e - m:e])) for v, x, m, e in
                        zip(c["version"].tolist(), c["value"].tolist(), npend.tolist(), ends)])
        return out, totals

    def quiesce(self):
        """lc_quiesce (ABI 5): stop the resident version-order grid now (it
        otherwise leaves after LC_RESIDENT_IDLE_US without a call)."""
        rc = lib().lc_quiesce(self._h)
        if rc != 0:
            raise LcError(rc, self.last_error())

    def totals(self, reset=False):
        """lc_last_totals (ABI 4): calls and device time summed since the last
        reset, every pending event read first."""
        t = LcTotals()
        lib().lc_last_totals(self._h, ctypes.byref(t), 1 if reset else 0)
        return {f: getattr(t, f) for f, _ in LcTotals._fields_}

    def call_profile(self):
        """lc_last_call_profile: where the last host call's wall time went."""
        pr = LcCallProfile()
        lib().lc_last_call_profile(self._h, ctypes.byref(pr))
        return {f: getattr(pr, f) for f, _ in LcCallProfile._fields_}

    def check_device(self, d_ops, d_key_off, n_keys, d_out, stream=None, opts=None,
                     d_witness=None, d_witness_kind=None):
        """Device-pointer check (ints), e.g. from torch tensors' data_ptr();
        with d_witness / d_witness_kind (device pointers) lc_check_device_ex."""
        o = opts if opts is not None else default_opts()
        args = (self._h, ctypes.c_void_p(d_ops), ctypes.c_void_p(d_key_off), n_keys,
                ctypes.byref(o), ctypes.c_void_p(d_out),
                ctypes.c_void_p(stream) if stream else None)
        if d_witness is not None:
            aux = LcAux(d_witness, d_witness_kind, None, None)
            rc = lib().lc_check_device_ex(*args, ctypes.byref(aux))
        else:
            rc = lib().lc_check_device(*args)
        if rc != 0:
            raise LcError(rc, self.last_error())
        return rc


    def check_device32(self, d_ops32, d_key_off, d_key_base, n_keys, d_out, stream=None,
                       opts=None):
        """lc_check_device32 (ABI 4): 24-byte records resident on the GPU."""
        o = opts if opts is not None else default_opts()
        rc = lib().lc_check_device32(self._h, ctypes.c_void_p(d_ops32), ctypes.c_void_p(d_key_off),
                                     ctypes.c_void_p(d_key_base) if d_key_base else None, n_keys,
                                     ctypes.byref(o), ctypes.c_void_p(d_out),
                                     ctypes.c_void_p(stream) if stream else None, None)
        if rc != 0:
            raise LcError(rc, self.last_error())
        return rc

    def bind_check_device32(self, d_ops32, d_key_off, d_key_base, n_keys, d_out, stream=None,
                            opts=None):
        """lc_check_device32 (ABI 4) with its arguments converted once, as
        bind_check_device: 24-byte records resident on the device."""
        L = lib()
        o = opts if opts is not None else default_opts()
        args = (self._h, ctypes.c_void_p(d_ops32), ctypes.c_void_p(d_key_off),
                ctypes.c_void_p(d_key_base) if d_key_base else None, ctypes.c_int64(n_keys),
                ctypes.byref(o), ctypes.c_void_p(d_out),
                ctypes.c_void_p(stream) if stream else None, None)
        fn = L.lc_check_device32

        def call():
            rc = fn(*args)
            if rc != 0:
                raise LcError(rc, self.last_error())

        call._keep = (o,)
        return call

    def bind_check_device(self, d_ops, d_key_off, n_keys, d_out, stream=None, opts=None,
                          stats=None):
        """check_device with its arguments converted once: returns a
        zero-argument callable that runs the check (and fills `stats`, an
        LcStats, when given) and raises LcError on failure.  For loops that
        time the same call over and over (bench.py)."""
        L = lib()
        o = opts if opts is not None else default_opts()
        args = (self._h, ctypes.c_void_p(d_ops), ctypes.c_void_p(d_key_off),
                ctypes.c_int64(n_keys), ctypes.byref(o), ctypes.c_void_p(d_out),
                ctypes.c_void_p(stream) if stream else None)
        fn, st_fn = L.lc_check_device, L.lc_last_stats
        st_args = (self._h, ctypes.byref(stats)) if stats is not None else None

        def call():
            rc = fn(*args)
            if rc != 0:
                raise LcError(rc, self.last_error())
            if st_args is not None:
                st_fn(*st_args)
            return stats

        call._keep = (o, stats)  # the byref targets must outlive the closure
        return call


def plan_partition(key_off, n_parts, ops=None):
    """lc_plan_partition: n_parts+1 key bounds at equal estimated cost (by
    lc_key_cost with ops; by record count without)."""
    key_off = np.ascontiguousarray(key_off, dtype=np.int64)
    if ops is not None:
        ops = as_ops(ops)
    bounds = np.zeros(n_parts + 1, dtype=np.int64)
    rc = lib().lc_plan_partition(_ptr(ops), _ptr(key_off), len(key_off) - 1, n_parts,
                                 _ptr(bounds))
    if rc != 0:
        raise LcError(rc, "lc_plan_partition")
    return bounds


def counted_plan(records):
    """lc_counted_plan: the class table the counted tier
    (LC_FLAG_COUNTED_CLASSES) uses for one key's records, as a dict —
    n_classes, field_bits, slots, fits, and `classes`: per class (the first
    LC_COUNTED_MAX_CLASSES) f, value, expected, version, members, shift,
    width.  Host-only."""
    ops = as_ops(records)
    lay = LcCountedLayout()
    rc = lib().lc_counted_plan(_ptr(ops), len(ops), ctypes.byref(lay))
    if rc != 0:
        raise LcError(rc, "lc_counted_plan")
    per = ("f", "value", "expected", "version", "members", "shift", "width")
    n = min(int(lay.n_classes), LC_COUNTED_MAX_CLASSES)
    return {"n_classes": int(lay.n_classes), "field_bits": int(lay.field_bits),
            "slots": int(lay.slots), "fits": int(lay.fits),
            "classes": [{f: int(getattr(lay, f)[c]) for f in per} for c in range(n)]}


def key_cost(ops, key_off):
    """lc_key_cost: estimated device cost per key (record-scan units)."""
    ops = as_ops(ops)
    key_off = np.ascontiguousarray(key_off, dtype=np.int64)
    out = np.zeros(len(key_off) - 1, dtype=np.float64)
    rc = lib().lc_key_cost(_ptr(ops), _ptr(key_off), len(out), _ptr(out))
    if rc != 0:
        raise LcError(rc, "lc_key_cost")
    return out


def synth_params(n_keys, ops_per_key, concurrency=10, n_values=5, p_info=0.0,
                 p_anomaly=0.0, seed=0x5EED0000, info_frac=0.0):
    return LcSynthParams(n_keys, ops_per_key, concurrency, n_values, p_info,
                         p_anomaly, seed, info_frac)


def synth(n_keys, ops_per_key, concurrency=10, n_values=5, p_info=0.0,
          p_anomaly=0.0, seed=0x5EED0000, n_threads=None, info_frac=0.0):
    """Packed synthetic histories: (ops (n,6) int64, key_off, labels, n_invocations).
    info_frac > 0 makes exactly round(info_frac * ops_per_key) records of
    every key crashed writes/CAS (include/lincheck_synth.h)."""
    prm = synth_params(n_keys, ops_per_key, concurrency, n_values, p_info,
                       p_anomaly, seed, info_frac)
    ops = np.zeros((n_keys * ops_per_key, 6), dtype=np.int64)
    key_off = np.zeros(n_keys + 1, dtype=np.int64)
    labels = np.zeros(n_keys, dtype=np.int32)
    ninv = ctypes.c_int64(0)
    if n_threads is None:
        n_threads = min(16, os.cpu_count() or 1)
    rc = lib().lc_synth_register(ctypes.byref(prm), _ptr(ops), _ptr(key_off),
                                 _ptr(labels), ctypes.byref(ninv), n_threads)
    if rc != 0:
        raise LcError(rc, "lc_synth_register")
    return ops, key_off, labels, ninv.value


def synth_key(key, ops_per_key, concurrency=10, n_values=5, p_info=0.0,
              p_anomaly=0.0, seed=0x5EED0000, info_frac=0.0):
    """One key's full op stream incl. :fail: (ops, proc, status, label)."""
    prm = synth_params(1, ops_per_key, concurrency, n_values, p_info, p_anomaly, seed,
                       info_frac)
    n = ctypes.c_int64(0)
    lab = ctypes.c_int32(0)
    cap = 4 * ops_per_key + 64
    while True:
        ops = np.zeros((cap, 6), dtype=np.int64)
        proc = np.zeros(cap, dtype=np.int32)
        st = np.zeros(cap, dtype=np.int32)
        rc = lib().lc_synth_key(ctypes.byref(prm), key, _ptr(ops), _ptr(proc), _ptr(st),
                                cap, ctypes.byref(n), ctypes.byref(lab))
        if rc == 0:
            k = n.value
            return ops[:k], proc[:k], st[:k], lab.value
        cap = n.value
