"""ctypes binding of syzgydb_amd/libsyzgy_scan.so (include/syzgy_scan.h).

The library is the product; this module only loads it and declares the
prototypes.  There is no Python or CPU fallback: if the shared object is
missing, loading fails loudly with the build command to run.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SZG_LIB_PATH selects an alternative build of the same library (kernel tuning experiments)
LIB_PATH = os.environ.get("SZG_LIB_PATH") or os.path.join(_HERE, "libsyzgy_scan.so")

SZG_EUCLIDEAN = 0
SZG_COSINE = 1

SZG_OK = 0
SZG_E_INVALID = -1
SZG_E_NOMEM = -2
SZG_E_DEVICE = -3
SZG_E_TRUNCATED = -4
SZG_E_NODEVICE = -5
SZG_E_RANGE = -6
SZG_E_UNSUPPORTED = -7

# every symbol include/syzgy_scan.h declares (tests check the .so exports them all)
EXPORTS = [
    "szg_index_create", "szg_index_destroy", "szg_row_bytes", "szg_index_load",
    "szg_index_append", "szg_index_overwrite", "szg_index_tombstone", "szg_index_rows",
    "szg_index_live_rows", "szg_index_read_rows", "szg_search_topk", "szg_search_radius",
    "szg_strerror", "szg_last_error", "szg_abi_version", "szg_set_timing", "szg_get_stats",
    "szg_reset_stats", "szg_set_option", "szg_index_synth", "szg_index_set_row_base",
    "szg_merge_topk", "szg_merge_topk_records", "szg_index_append_f64", "szg_distances", "szg_pair_distances", "szg_index_overwrite_f64",
    "szg_search_radius_batch", "szg_comm_unique_id", "szg_comm_create", "szg_comm_create_host", "szg_comm_destroy",
    "szg_comm_reserve", "szg_index_attach_comm", "szg_search_topk_sharded", "szg_search_radius_sharded",
    "szg_comm_merge_topk", "szg_comm_merge_radius", "szg_comm_get_stats", "szg_comm_reset_stats",
    "szg_comm_last_radius", "szg_comm_chain_topk", "szg_comm_debug_inject",
    # device-resident filter masks (added under ABI 4)
    "szg_mask_create", "szg_mask_create_rows", "szg_mask_combine", "szg_mask_count", "szg_mask_read",
    "szg_mask_destroy", "szg_search_topk_masked", "szg_search_radius_masked", "szg_index_mask_stats",
    # compaction / reorder on the device (added under ABI 4)
    "szg_index_reorder", "szg_index_compact",
    # resident metadata columns (added under ABI 4)
    "szg_column_create", "szg_column_append", "szg_column_set", "szg_column_rows", "szg_column_read",
    "szg_column_destroy", "szg_mask_where_f64", "szg_mask_where_in_f64", "szg_mask_where_u32", "szg_mask_where_present",
    # text columns (added under ABI 4)
    "szg_column_create_str", "szg_column_append_str", "szg_column_set_str", "szg_column_read_str", "szg_mask_where_str",
    # byte automata over text columns (added under ABI 4)
    "szg_mask_where_dfa",
    # columns carried across compaction / reorder (added under ABI 4)
    "szg_index_reorder_carry", "szg_index_compact_carry", "szg_column_get_info",
    # bulk mutations: many rows per call (added under ABI 4)
    "szg_index_overwrite_rows", "szg_index_overwrite_rows_f64", "szg_index_tombstone_rows", "szg_index_tombstone_mask",
    "szg_column_set_rows", "szg_debug_bulk_plan",
    # ingest from device memory (added under ABI 4)
    "szg_index_append_dev", "szg_index_overwrite_rows_dev",
    # vectors out to device memory, queries from it (added under ABI 4)
    "szg_index_fetch_rows_dev", "szg_search_topk_dev", "szg_search_radius_dev",
    # host-only test hook
    "szg_debug_scan_plan", "szg_debug_scan_group", "szg_debug_reorder_plan", "szg_debug_option_check",
    "szg_debug_option_get",   # (not host-only: reads an option back from a handle or its sketch index)
    "szg_debug_scan_group_ring", "szg_debug_merge_short_plan", "szg_debug_scan_matrix",
    "szg_debug_scan_select", "szg_debug_scan_wide", "szg_debug_scan_collect", "szg_debug_scan_share",
    # who owns device memory: the counters and the refusal countdown (added under ABI 4)
    "szg_debug_device_memory", "szg_debug_refuse_device_alloc",
    # the certificate trace: what each pass handed to certification (added under ABI 4)
    "szg_debug_trace_certificates", "szg_debug_certificates",
    # the sketch index's state, read only (added under ABI 4)
    "szg_debug_sketch_info", "szg_debug_sketch_rows",
    # the matrix sweep's masked forms (option sketch_masked): the plan hook and the counters
    "szg_debug_scan_masked", "szg_debug_sketch_masked",
    # the certification bound of a key as a pure function (csrc/key_bound.h), host only
    "szg_debug_key_eps",
    # top-k of large k through the sketch (option sketch_topk_collect): the counters and the sample plan hook
    "szg_index_sketch_topk_stats", "szg_debug_sample_plan",
    # a sketch batch's queries prepared on the card (option query_prep): the counters, the two-sided hook, the batch rule
    "szg_index_query_prep_stats", "szg_debug_query_prep", "szg_debug_query_prep_serves",
]
# szg_cert_record.pass / .keys, szg_cert_entry.flags
SZG_CERT_TOPK, SZG_CERT_SKETCH, SZG_CERT_ESCALATION, SZG_CERT_RADIUS_SINGLE, SZG_CERT_RADIUS_SHARED = range(5)
SZG_CERT_SKETCH_RADIUS = 5   # radius collect on the sketch (option sketch_radius), recorded on the float32 handle
SZG_CERT_SKETCH_TOPK_COLLECT = 6   # top-k of large k through the sketch (option sketch_topk_collect): sample bound + collect
(SZG_CERT_KEYS_SINGLE, SZG_CERT_KEYS_SHARED_INT8, SZG_CERT_KEYS_SHARED_BF16, SZG_CERT_KEYS_BF16_BAND,
 SZG_CERT_KEYS_BF16_RESCORED) = range(5)
SZG_CERT_ENTRY_NO_KEY = 1
SZG_MASK_AND, SZG_MASK_OR, SZG_MASK_ANDNOT, SZG_MASK_NOT = 0, 1, 2, 3
SZG_COL_F64, SZG_COL_U32, SZG_COL_STR = 0, 1, 2
SZG_CMP_EQ, SZG_CMP_NE, SZG_CMP_LT, SZG_CMP_LE, SZG_CMP_GT, SZG_CMP_GE = range(6)
SZG_STR_STARTS_WITH, SZG_STR_ENDS_WITH, SZG_STR_CONTAINS = 6, 7, 8   # szg_mask_where_str only
SZG_SRC_F64, SZG_SRC_F32, SZG_SRC_F16, SZG_SRC_BF16 = range(4)   # szg_dev_vectors.dtype
SZG_STR_PATTERN_MAX = 256
SZG_DFA_STATES_MAX = 32768     # szg_mask_where_dfa: states of an automaton
SZG_DFA_TABLE_MAX = 1 << 20    # ... and n_states * n_classes entries of its table
SZG_COMM_ID_BYTES = 128
# int (*szg_allgather_fn)(void *user, const void *send, void *recv, uint64_t bytes_per_rank)
ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64)
# int (*szg_replay_fn)(void *user, int j, int k, uint64_t *heap_rows, double *heap_dist, int32_t *heap_n)
REPLAY_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
                             ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32))


class SzgCommStats(ctypes.Structure):
    _fields_ = [("exchanges", ctypes.c_uint64), ("exchange_us", ctypes.c_double), ("host_us", ctypes.c_double),
                ("rccl_ranks", ctypes.c_int), ("zero_copy", ctypes.c_int), ("chained_replays", ctypes.c_uint64),
                ("status_rounds", ctypes.c_uint64), ("chain_rounds", ctypes.c_uint64)]

# include/syzgy_pager.h
PAGER_EXPORTS = [
    "szg_pager_open", "szg_pager_close", "szg_pager_options", "szg_pager_count", "szg_pager_skipped",
    "szg_pager_ids", "szg_pager_vectors", "szg_pager_metadata", "szg_pager_load",
]
SZG_E_IO = -8
SZG_E_FORMAT = -9


class SzgStats(ctypes.Structure):
    _fields_ = [
        ("queries", ctypes.c_uint64),
        ("scan_launches", ctypes.c_uint64),
        ("escalations", ctypes.c_uint64),
        ("scan_bytes", ctypes.c_uint64),
        ("scan_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
        ("timed_launches", ctypes.c_uint64),
        ("full_replays", ctypes.c_uint64),
        ("mq_launches", ctypes.c_uint64),
        ("mq_queries", ctypes.c_uint64),
        ("mq_fallbacks", ctypes.c_uint64),
        ("host_prep_us", ctypes.c_double),
        ("host_finish_us", ctypes.c_double),
        ("host_enqueue_us", ctypes.c_double),
        ("sketch_queries", ctypes.c_uint64),
        ("sketch_fallbacks", ctypes.c_uint64),
        ("mq_bf16_sweeps", ctypes.c_uint64),
        ("sketch_radius_queries", ctypes.c_uint64),
        ("sketch_radius_fallbacks", ctypes.c_uint64),
    ]


class SzgSketchTopkStats(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in ("queries", "fallbacks", "sample_rows", "candidates", "overflows")]


class SzgQueryPrepStats(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in ("queries_dev", "queries_host", "launches")]


class SzgSamplePlan(ctypes.Structure):
    _fields_ = ([(name, ctypes.c_int32) for name in ("serves", "stride", "blocks", "reserved")] +
                [(name, ctypes.c_uint64) for name in ("tiles", "sample_rows", "slots", "key_bytes", "cap", "lds_bytes")])


class SzgScanPlan(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int32) for name in (
        "r16", "L", "P", "gpw", "pow2", "dense", "tiled", "grid", "block", "ring_depth", "shaped", "nontemporal",
        "rows_per_block")]


class SzgCertRecord(ctypes.Structure):
    _fields_ = ([(name, ctypes.c_int32) for name in ("query", "pass_", "keys", "sweep", "certified", "k")] +
                [("row_lo", ctypes.c_uint64), ("row_hi", ctypes.c_uint64)] +
                [(name, ctypes.c_double) for name in ("thr_min", "kmax", "thr", "eps", "D", "slack")] +
                [("first_entry", ctypes.c_uint64), ("n_entries", ctypes.c_uint64)])


class SzgCertEntry(ctypes.Structure):
    _fields_ = [("row", ctypes.c_uint64), ("dist", ctypes.c_double), ("ub", ctypes.c_double), ("key", ctypes.c_float),
                ("flags", ctypes.c_uint32)]


class SzgSketchInfo(ctypes.Structure):
    _fields_ = ([(name, ctypes.c_int32) for name in ("exists", "in_sync", "disabled", "n_shards")] +
                [("rows", ctypes.c_uint64), ("max_ang", ctypes.c_double), ("gscale", ctypes.c_double),
                 ("n_exc", ctypes.c_uint64)])


class SzgScanMaskedPlan(ctypes.Structure):
    _fields_ = [(name, ctypes.c_int32) for name in ("serves", "wide", "share", "tile_skip", "steps_form", "launches", "passes")]


class SzgSketchMaskedInfo(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in ("launches", "skip_launches", "queries")]


class SzgColumnInfo(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("rows", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64),
                ("heap_used", ctypes.c_uint64), ("heap_capacity", ctypes.c_uint64)]


class SzgDfa(ctypes.Structure):
    _fields_ = [("n_states", ctypes.c_uint32), ("n_classes", ctypes.c_uint32), ("start", ctypes.c_uint32),
                ("class_of", ctypes.POINTER(ctypes.c_uint8)), ("next", ctypes.POINTER(ctypes.c_uint16)),
                ("accept_bits", ctypes.POINTER(ctypes.c_uint64))]


class SzgDevVectors(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("dtype", ctypes.c_int), ("device", ctypes.c_int), ("n_rows", ctypes.c_uint64),
                ("row_stride", ctypes.c_uint64)]


class SzgMaskStats(ctypes.Structure):
    _fields_ = [("live_masks", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64), ("h2d_bytes", ctypes.c_uint64),
                ("d2d_bytes", ctypes.c_uint64), ("shared_batches", ctypes.c_uint64)]


class SzgError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        msg = "%s failed: %d" % (where, code)
        if detail:
            msg += " (%s)" % detail
        super().__init__(msg)


_lib = None


def load():
    """Load the HIP library; raise if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "syzgydb_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C syzgydb_amd/csrc`.  There is no CPU fallback." % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp = ctypes.c_void_p
    u8p = ctypes.POINTER(ctypes.c_uint8)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    f64p = ctypes.POINTER(ctypes.c_double)
    i32p = ctypes.POINTER(ctypes.c_int32)
    intp = ctypes.POINTER(ctypes.c_int)

    L.szg_abi_version.restype = ctypes.c_int
    L.szg_abi_version.argtypes = []
    L.szg_strerror.restype = ctypes.c_char_p
    L.szg_strerror.argtypes = [ctypes.c_int]
    L.szg_last_error.restype = ctypes.c_char_p
    L.szg_last_error.argtypes = []
    L.szg_row_bytes.restype = ctypes.c_int64
    L.szg_row_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    L.szg_index_create.restype = ctypes.c_int
    L.szg_index_create.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   intp, ctypes.c_int]
    L.szg_index_destroy.restype = None
    L.szg_index_destroy.argtypes = [vp]
    L.szg_index_load.restype = ctypes.c_int
    L.szg_index_load.argtypes = [vp, u8p, ctypes.c_uint64]
    L.szg_index_append.restype = ctypes.c_int
    L.szg_index_append.argtypes = [vp, u8p, ctypes.c_uint64]
    L.szg_index_overwrite.restype = ctypes.c_int
    L.szg_index_overwrite.argtypes = [vp, ctypes.c_uint64, u8p]
    L.szg_index_tombstone.restype = ctypes.c_int
    L.szg_index_tombstone.argtypes = [vp, ctypes.c_uint64]
    L.szg_index_rows.restype = ctypes.c_uint64
    L.szg_index_rows.argtypes = [vp]
    L.szg_index_live_rows.restype = ctypes.c_uint64
    L.szg_index_live_rows.argtypes = [vp]
    L.szg_index_read_rows.restype = ctypes.c_int
    L.szg_index_read_rows.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, u8p]
    L.szg_search_topk.restype = ctypes.c_int
    L.szg_search_topk.argtypes = [vp, f64p, ctypes.c_int, ctypes.c_int, u64p, u64p, f64p, i32p]
    L.szg_search_radius.restype = ctypes.c_int
    L.szg_search_radius.argtypes = [vp, f64p, ctypes.c_double, u64p, u64p, f64p, ctypes.c_uint64,
                                    u64p]
    L.szg_set_timing.restype = ctypes.c_int
    L.szg_set_timing.argtypes = [vp, ctypes.c_int]
    L.szg_get_stats.restype = ctypes.c_int
    L.szg_get_stats.argtypes = [vp, ctypes.POINTER(SzgStats)]
    L.szg_reset_stats.restype = ctypes.c_int
    L.szg_reset_stats.argtypes = [vp]
    L.szg_set_option.restype = ctypes.c_int
    L.szg_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_int64]
    L.szg_index_synth.restype = ctypes.c_int
    L.szg_index_synth.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
    L.szg_index_set_row_base.restype = ctypes.c_int
    L.szg_index_set_row_base.argtypes = [vp, ctypes.c_uint64]
    L.szg_merge_topk.restype = ctypes.c_int
    L.szg_merge_topk.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, u64p, f64p,
                                 i32p, u64p, f64p, i32p, u8p]
    L.szg_merge_topk_records.restype = ctypes.c_int
    L.szg_merge_topk_records.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_int64), u64p, f64p, i32p, u8p]
    L.szg_index_append_f64.restype = ctypes.c_int
    L.szg_index_append_f64.argtypes = [vp, f64p, ctypes.c_uint64]
    L.szg_index_overwrite_f64.restype = ctypes.c_int
    L.szg_index_overwrite_f64.argtypes = [vp, ctypes.c_uint64, f64p]
    L.szg_distances.restype = ctypes.c_int
    L.szg_distances.argtypes = [vp, f64p, u64p, ctypes.c_uint64, f64p]
    L.szg_pair_distances.restype = ctypes.c_int
    L.szg_pair_distances.argtypes = [vp, u64p, u64p, ctypes.c_uint64, f64p]
    L.szg_search_radius_batch.restype = ctypes.c_int
    L.szg_search_radius_batch.argtypes = [vp, f64p, ctypes.c_int, f64p, u64p, u64p, f64p, ctypes.c_uint64, u64p]
    # (an older build selected through SZG_LIB_PATH for an A/B run has no masks: masks= then fails at the call)
    if hasattr(L, "szg_mask_create"):
        L.szg_mask_create.restype = ctypes.c_int
        L.szg_mask_create.argtypes = [vp, u64p, ctypes.POINTER(vp)]
        L.szg_mask_create_rows.restype = ctypes.c_int
        L.szg_mask_create_rows.argtypes = [vp, u64p, ctypes.c_uint64, ctypes.POINTER(vp)]
        L.szg_mask_combine.restype = ctypes.c_int
        L.szg_mask_combine.argtypes = [ctypes.c_int, vp, vp, ctypes.POINTER(vp)]
        L.szg_mask_count.restype = ctypes.c_uint64
        L.szg_mask_count.argtypes = [vp]
        L.szg_mask_read.restype = ctypes.c_int
        L.szg_mask_read.argtypes = [vp, u64p]
        L.szg_mask_destroy.restype = None
        L.szg_mask_destroy.argtypes = [vp]
        L.szg_search_topk_masked.restype = ctypes.c_int
        L.szg_search_topk_masked.argtypes = [vp, f64p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp), ctypes.c_int, u64p,
                                             f64p, i32p]
        L.szg_search_radius_masked.restype = ctypes.c_int
        L.szg_search_radius_masked.argtypes = [vp, f64p, ctypes.c_int, f64p, ctypes.POINTER(vp), ctypes.c_int, u64p, f64p,
                                               ctypes.c_uint64, u64p]
        L.szg_index_mask_stats.restype = ctypes.c_int
        L.szg_index_mask_stats.argtypes = [vp, ctypes.POINTER(SzgMaskStats)]
    if hasattr(L, "szg_index_reorder"):   # (as the masks: an older build for an A/B run cannot compact)
        L.szg_index_reorder.restype = ctypes.c_int
        L.szg_index_reorder.argtypes = [vp, u64p, ctypes.c_uint64, ctypes.POINTER(vp), ctypes.c_int]
        L.szg_index_compact.restype = ctypes.c_int
        L.szg_index_compact.argtypes = [vp, u64p, u64p, ctypes.POINTER(vp), ctypes.c_int]
        L.szg_debug_reorder_plan.restype = ctypes.c_int
        L.szg_debug_reorder_plan.argtypes = [ctypes.c_uint64, u64p, u64p, ctypes.c_uint64, ctypes.c_int, u64p]
    if hasattr(L, "szg_column_create"):   # (as the masks: an older build for an A/B run has no columns)
        L.szg_column_create.restype = ctypes.c_int
        L.szg_column_create.argtypes = [vp, ctypes.c_int, vp, u64p, ctypes.c_uint64, ctypes.POINTER(vp)]
        L.szg_column_append.restype = ctypes.c_int
        L.szg_column_append.argtypes = [vp, vp, u64p, ctypes.c_uint64]
        L.szg_column_set.restype = ctypes.c_int
        L.szg_column_set.argtypes = [vp, ctypes.c_uint64, vp]
        L.szg_column_rows.restype = ctypes.c_uint64
        L.szg_column_rows.argtypes = [vp]
        L.szg_column_read.restype = ctypes.c_int
        L.szg_column_read.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, vp, u64p]
        L.szg_column_destroy.restype = None
        L.szg_column_destroy.argtypes = [vp]
        L.szg_mask_where_f64.restype = ctypes.c_int
        L.szg_mask_where_f64.argtypes = [vp, ctypes.c_int, ctypes.c_double, vp, ctypes.POINTER(vp)]
        L.szg_mask_where_in_f64.restype = ctypes.c_int
        L.szg_mask_where_in_f64.argtypes = [vp, f64p, ctypes.c_uint32, vp, ctypes.POINTER(vp)]
        L.szg_mask_where_u32.restype = ctypes.c_int
        L.szg_mask_where_u32.argtypes = [vp, u64p, ctypes.c_uint32, vp, ctypes.POINTER(vp)]
        L.szg_mask_where_present.restype = ctypes.c_int
        L.szg_mask_where_present.argtypes = [vp, vp, ctypes.POINTER(vp)]
    if hasattr(L, "szg_column_create_str"):   # (an older build for an A/B run has no text columns)
        L.szg_column_create_str.restype = ctypes.c_int
        L.szg_column_create_str.argtypes = [vp, u8p, u64p, u64p, ctypes.c_uint64, ctypes.POINTER(vp)]
        L.szg_column_append_str.restype = ctypes.c_int
        L.szg_column_append_str.argtypes = [vp, u8p, u64p, u64p, ctypes.c_uint64]
        L.szg_column_set_str.restype = ctypes.c_int
        L.szg_column_set_str.argtypes = [vp, ctypes.c_uint64, u8p, ctypes.c_uint64]
        L.szg_column_read_str.restype = ctypes.c_int
        L.szg_column_read_str.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, u64p, u8p, ctypes.c_uint64, u64p]
        L.szg_mask_where_str.restype = ctypes.c_int
        L.szg_mask_where_str.argtypes = [vp, ctypes.c_int, u8p, ctypes.c_uint32, vp, ctypes.POINTER(vp)]
    if hasattr(L, "szg_mask_where_dfa"):   # (an older build for an A/B run walks no automata)
        L.szg_mask_where_dfa.restype = ctypes.c_int
        L.szg_mask_where_dfa.argtypes = [vp, ctypes.POINTER(SzgDfa), vp, ctypes.POINTER(vp)]
    if hasattr(L, "szg_index_reorder_carry"):   # (an older build for an A/B run carries no columns)
        L.szg_index_reorder_carry.restype = ctypes.c_int
        L.szg_index_reorder_carry.argtypes = [vp, u64p, ctypes.c_uint64, ctypes.POINTER(vp), ctypes.c_int,
                                              ctypes.POINTER(vp), ctypes.c_int]
        L.szg_index_compact_carry.restype = ctypes.c_int
        L.szg_index_compact_carry.argtypes = [vp, u64p, u64p, ctypes.POINTER(vp), ctypes.c_int, ctypes.POINTER(vp),
                                              ctypes.c_int]
        L.szg_column_get_info.restype = ctypes.c_int
        L.szg_column_get_info.argtypes = [vp, ctypes.POINTER(SzgColumnInfo)]
    if hasattr(L, "szg_index_overwrite_rows"):   # (an older build for an A/B run mutates one row per call)
        L.szg_index_overwrite_rows.restype = ctypes.c_int
        L.szg_index_overwrite_rows.argtypes = [vp, u64p, u8p, ctypes.c_uint64]
        L.szg_index_overwrite_rows_f64.restype = ctypes.c_int
        L.szg_index_overwrite_rows_f64.argtypes = [vp, u64p, f64p, ctypes.c_uint64]
        L.szg_index_tombstone_rows.restype = ctypes.c_int
        L.szg_index_tombstone_rows.argtypes = [vp, u64p, ctypes.c_uint64, u64p]
        L.szg_index_tombstone_mask.restype = ctypes.c_int
        L.szg_index_tombstone_mask.argtypes = [vp, vp, u64p]
        L.szg_column_set_rows.restype = ctypes.c_int
        L.szg_column_set_rows.argtypes = [vp, u64p, vp, u64p, ctypes.c_uint64]
        L.szg_debug_bulk_plan.restype = ctypes.c_int
        L.szg_debug_bulk_plan.argtypes = [ctypes.c_uint64, ctypes.c_uint64, u64p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                          u64p, u64p, u64p, u64p, u64p]
    if hasattr(L, "szg_index_append_dev"):   # (an older build for an A/B run takes vectors from the host only)
        L.szg_index_append_dev.restype = ctypes.c_int
        L.szg_index_append_dev.argtypes = [vp, ctypes.POINTER(SzgDevVectors), u64p, ctypes.c_uint64]
        L.szg_index_overwrite_rows_dev.restype = ctypes.c_int
        L.szg_index_overwrite_rows_dev.argtypes = [vp, u64p, ctypes.POINTER(SzgDevVectors), u64p, ctypes.c_uint64]
    if hasattr(L, "szg_index_fetch_rows_dev"):   # (an older build for an A/B run serves vectors and queries on the host only)
        i32p = ctypes.POINTER(ctypes.c_int32)
        L.szg_index_fetch_rows_dev.restype = ctypes.c_int
        L.szg_index_fetch_rows_dev.argtypes = [vp, u64p, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(SzgDevVectors)]
        L.szg_search_topk_dev.restype = ctypes.c_int
        L.szg_search_topk_dev.argtypes = [vp, ctypes.POINTER(SzgDevVectors), u64p, ctypes.c_int, ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, u64p, f64p, i32p]
        L.szg_search_radius_dev.restype = ctypes.c_int
        L.szg_search_radius_dev.argtypes = [vp, ctypes.POINTER(SzgDevVectors), u64p, ctypes.c_int, f64p,
                                            ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, u64p, f64p, ctypes.c_uint64, u64p]
    L.szg_comm_unique_id.restype = ctypes.c_int
    L.szg_comm_unique_id.argtypes = [u8p]
    L.szg_comm_create.restype = ctypes.c_int
    L.szg_comm_create.argtypes = [ctypes.POINTER(vp), u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.szg_comm_create_host.restype = ctypes.c_int
    L.szg_comm_create_host.argtypes = [ctypes.POINTER(vp), ALLGATHER_FN, vp, ctypes.c_int, ctypes.c_int]
    L.szg_comm_destroy.restype = None
    L.szg_comm_destroy.argtypes = [vp]
    L.szg_comm_reserve.restype = ctypes.c_int
    L.szg_comm_reserve.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    L.szg_index_attach_comm.restype = ctypes.c_int
    L.szg_index_attach_comm.argtypes = [vp, vp]
    L.szg_search_topk_sharded.restype = ctypes.c_int
    L.szg_search_topk_sharded.argtypes = [vp, f64p, ctypes.c_int, ctypes.c_int, u64p, u64p, f64p, i32p, u8p]
    L.szg_search_radius_sharded.restype = ctypes.c_int
    L.szg_search_radius_sharded.argtypes = [vp, f64p, ctypes.c_int, f64p, u64p, u64p, f64p, ctypes.c_uint64, u64p]
    L.szg_comm_merge_topk.restype = ctypes.c_int
    L.szg_comm_merge_topk.argtypes = [vp, ctypes.c_int, ctypes.c_int, u64p, f64p, i32p, u64p, f64p, i32p, u8p]
    L.szg_comm_merge_radius.restype = ctypes.c_int
    L.szg_comm_merge_radius.argtypes = [vp, ctypes.c_int, u64p, u64p, f64p, u64p, f64p, ctypes.c_uint64, u64p]
    L.szg_comm_get_stats.restype = ctypes.c_int
    L.szg_comm_get_stats.argtypes = [vp, ctypes.POINTER(SzgCommStats)]
    L.szg_comm_reset_stats.restype = ctypes.c_int
    L.szg_comm_reset_stats.argtypes = [vp]
    L.szg_comm_last_radius.restype = ctypes.c_int
    L.szg_comm_last_radius.argtypes = [vp, ctypes.c_int, u64p, f64p, ctypes.c_uint64, u64p]
    L.szg_comm_chain_topk.restype = ctypes.c_int
    L.szg_comm_chain_topk.argtypes = [vp, ctypes.c_int, ctypes.c_int, REPLAY_FN, vp, u64p, f64p, i32p]
    L.szg_comm_debug_inject.restype = ctypes.c_int
    L.szg_comm_debug_inject.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    L.szg_pager_open.restype = ctypes.c_int
    L.szg_pager_open.argtypes = [ctypes.POINTER(vp), ctypes.c_char_p, ctypes.c_int]
    L.szg_pager_close.restype = None
    L.szg_pager_close.argtypes = [vp]
    L.szg_pager_options.restype = ctypes.c_int
    L.szg_pager_options.argtypes = [vp, intp, intp, intp]
    L.szg_pager_count.restype = ctypes.c_uint64
    L.szg_pager_count.argtypes = [vp]
    L.szg_pager_skipped.restype = ctypes.c_uint64
    L.szg_pager_skipped.argtypes = [vp]
    L.szg_pager_ids.restype = ctypes.c_int
    L.szg_pager_ids.argtypes = [vp, u64p]
    L.szg_pager_vectors.restype = ctypes.c_int
    L.szg_pager_vectors.argtypes = [vp, u8p, ctypes.c_uint64]
    L.szg_pager_metadata.restype = ctypes.c_int
    L.szg_pager_metadata.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(u8p), u64p]
    L.szg_pager_load.restype = ctypes.c_int
    L.szg_pager_load.argtypes = [vp, vp]
    if hasattr(L, "szg_debug_scan_plan"):   # (as the masks: an older build for an A/B run has no plan hook)
        L.szg_debug_scan_plan.restype = ctypes.c_int
        L.szg_debug_scan_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.POINTER(SzgScanPlan)]
    if hasattr(L, "szg_debug_scan_group"):
        L.szg_debug_scan_group.restype = ctypes.c_int
        L.szg_debug_scan_group.argtypes = [ctypes.c_int] * 8 + [ctypes.POINTER(ctypes.c_int32), u64p,
                                                                ctypes.POINTER(ctypes.c_int32)]
    if hasattr(L, "szg_debug_scan_matrix"):
        L.szg_debug_scan_matrix.restype = ctypes.c_int
        L.szg_debug_scan_matrix.argtypes = [ctypes.c_int] * 10 + [ctypes.POINTER(ctypes.c_int32)] * 2 + [u64p,
                                                                                                    ctypes.POINTER(ctypes.c_int32)]
    if hasattr(L, "szg_debug_scan_wide"):
        L.szg_debug_scan_wide.restype = ctypes.c_int
        L.szg_debug_scan_wide.argtypes = ([ctypes.c_int] * 12 + [ctypes.POINTER(ctypes.c_int32)] * 2 +
                                          [ctypes.POINTER(ctypes.c_uint64)])
    if hasattr(L, "szg_debug_scan_share"):
        L.szg_debug_scan_share.restype = ctypes.c_int
        L.szg_debug_scan_share.argtypes = ([ctypes.c_int] * 13 + [ctypes.POINTER(ctypes.c_int32)] * 4 +
                                           [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32,
                                            ctypes.POINTER(ctypes.c_int32)])
    if hasattr(L, "szg_debug_scan_masked"):
        L.szg_debug_scan_masked.restype = ctypes.c_int
        L.szg_debug_scan_masked.argtypes = [ctypes.c_int] * 15 + [ctypes.POINTER(SzgScanMaskedPlan)]
        L.szg_debug_sketch_masked.restype = ctypes.c_int
        L.szg_debug_sketch_masked.argtypes = [vp, ctypes.POINTER(SzgSketchMaskedInfo)]
    if hasattr(L, "szg_index_sketch_topk_stats"):
        L.szg_index_sketch_topk_stats.restype = ctypes.c_int
        L.szg_index_sketch_topk_stats.argtypes = [vp, ctypes.POINTER(SzgSketchTopkStats)]
        L.szg_debug_sample_plan.restype = ctypes.c_int
        L.szg_debug_sample_plan.argtypes = [ctypes.c_uint64] + [ctypes.c_int] * 5 + [ctypes.POINTER(SzgSamplePlan)]
    if hasattr(L, "szg_index_query_prep_stats"):   # (an older build for an A/B run has no such option)
        L.szg_index_query_prep_stats.restype = ctypes.c_int
        L.szg_index_query_prep_stats.argtypes = [vp, ctypes.POINTER(SzgQueryPrepStats)]
        L.szg_debug_query_prep.restype = ctypes.c_int
        L.szg_debug_query_prep.argtypes = [vp, f64p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint8), f64p]
        L.szg_debug_query_prep_serves.restype = ctypes.c_int
        L.szg_debug_query_prep_serves.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    if hasattr(L, "szg_debug_scan_collect"):
        L.szg_debug_scan_collect.restype = ctypes.c_int
        L.szg_debug_scan_collect.argtypes = ([ctypes.c_int] * 10 + [ctypes.POINTER(ctypes.c_int32)] * 3 +
                                             [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int32)])
    if hasattr(L, "szg_debug_scan_select"):
        L.szg_debug_scan_select.restype = ctypes.c_int
        L.szg_debug_scan_select.argtypes = [ctypes.c_int] * 11 + [ctypes.POINTER(ctypes.c_int32)] * 2
    if hasattr(L, "szg_debug_scan_group_ring"):
        L.szg_debug_scan_group_ring.restype = ctypes.c_int
        L.szg_debug_scan_group_ring.argtypes = [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_int32)] * 3
    if hasattr(L, "szg_debug_merge_short_plan"):
        L.szg_debug_merge_short_plan.restype = ctypes.c_int
        L.szg_debug_merge_short_plan.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int32)] * 2
    if hasattr(L, "szg_debug_option_check"):
        L.szg_debug_option_check.restype = ctypes.c_int
        L.szg_debug_option_check.argtypes = [ctypes.c_char_p, ctypes.c_int64]
    if hasattr(L, "szg_debug_option_get"):   # (an older build for an A/B run has no such hook)
        L.szg_debug_option_get.restype = ctypes.c_int
        L.szg_debug_option_get.argtypes = [vp, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
    if hasattr(L, "szg_debug_key_eps"):   # (an older build for an A/B run has no such hook)
        L.szg_debug_key_eps.restype = ctypes.c_int
        L.szg_debug_key_eps.argtypes = [ctypes.c_int] * 6 + [ctypes.c_double] * 5 + [f64p]
    if hasattr(L, "szg_debug_device_memory"):   # (as the masks: an older build for an A/B run does not count)
        L.szg_debug_device_memory.restype = ctypes.c_int
        L.szg_debug_device_memory.argtypes = [u64p, u64p]
        L.szg_debug_refuse_device_alloc.restype = ctypes.c_int
        L.szg_debug_refuse_device_alloc.argtypes = [ctypes.c_int64]
    if hasattr(L, "szg_debug_trace_certificates"):   # (as the masks: an older build for an A/B run keeps no trace)
        L.szg_debug_trace_certificates.restype = ctypes.c_int
        L.szg_debug_trace_certificates.argtypes = [vp, ctypes.c_int]
        L.szg_debug_certificates.restype = ctypes.c_int
        L.szg_debug_certificates.argtypes = [vp, ctypes.POINTER(SzgCertRecord), ctypes.c_uint64,
                                             ctypes.POINTER(SzgCertEntry), ctypes.c_uint64, u64p, u64p, u64p]
    if hasattr(L, "szg_debug_sketch_info"):   # (as the masks: an older build for an A/B run shows no sketch state)
        L.szg_debug_sketch_info.restype = ctypes.c_int
        L.szg_debug_sketch_info.argtypes = [vp, ctypes.POINTER(SzgSketchInfo), u64p, ctypes.c_uint64]
        L.szg_debug_sketch_rows.restype = ctypes.c_int
        L.szg_debug_sketch_rows.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, u8p, u64p, ctypes.c_uint64]
    L.szg_debug_f64_probe.restype = ctypes.c_int
    L.szg_debug_f64_probe.argtypes = [ctypes.c_int, f64p, f64p, f64p, ctypes.c_uint64]
    _lib = L
    return L


def check(code, where):
    if code != SZG_OK:
        L = load()
        detail = L.szg_last_error().decode("utf-8", "replace")
        if not detail:
            detail = L.szg_strerror(code).decode()
        raise SzgError(code, where, detail)
