"""ctypes loader for libimpg_gpu.so (the C ABI of include/impg_gpu.h).

The library is built in-tree by `make -C impg_amd/csrc` (hipcc, gfx950); there
is no CPU fallback: a missing library is an ImportError-like RuntimeError, and
every query on a machine without a GPU fails with IMPG_E_HIP.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IMPG_GPU_LIB") or os.path.join(_HERE, "libimpg_gpu.so")  # override: kernel experiments
CSRC = os.path.join(_HERE, "csrc")

IMPG_OK = 0
IMPG_E_INVALID, IMPG_E_HIP, IMPG_E_OOM, IMPG_E_IO, IMPG_E_UNSUPPORTED, IMPG_E_CANCELLED = -1, -2, -3, -4, -5, -6
STREAM_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
ORDER_COITREES, ORDER_SORTED = 0, 1
HIT_NONE = 0xFFFFFFFF

RECORD_DTYPE = np.dtype([("query_id", "<u4"), ("target_id", "<u4"), ("query_start", "<i4"), ("query_end", "<i4"),
                         ("target_start", "<i4"), ("target_end", "<i4"), ("cigar_off", "<u8"), ("cigar_len", "<u4"),
                         ("strand", "<u4")], align=True)
RANGE_DTYPE = np.dtype([("target_id", "<u4"), ("start", "<i4"), ("end", "<i4")])
INTERVAL_DTYPE = np.dtype([("query_id", "<u4"), ("q_first", "<i4"), ("q_last", "<i4"),
                           ("target_id", "<u4"), ("t_first", "<i4"), ("t_last", "<i4")])
assert RECORD_DTYPE.itemsize == 40 and RANGE_DTYPE.itemsize == 12
TP_RECORD_DTYPE = np.dtype([("query_id", "<u4"), ("target_id", "<u4"), ("query_start", "<i4"), ("query_end", "<i4"),
                            ("target_start", "<i4"), ("target_end", "<i4"), ("seg_off", "<u8"), ("n_segs", "<u4"),
                            ("strand", "<u4"), ("query_contig_start", "<i8")], align=True)  # impg_gpu_tp_record_t
assert TP_RECORD_DTYPE.itemsize == 48
COMM_ID_BYTES = 128


class TpMode(C.Structure):  # impg_gpu_tp_mode_t
    _fields_ = [("fastga", C.c_int32), ("trace_spacing", C.c_int32), ("max_complexity", C.c_int32)]


ALLGATHER_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_uint64))
ALLTOALLV_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p,
                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))


class HostTransport(C.Structure):  # impg_gpu_host_transport_t
    _fields_ = [("ctx", C.c_void_p), ("allgather_u64", ALLGATHER_CB), ("alltoallv", ALLTOALLV_CB)]


class Params(C.Structure):
    _fields_ = [("transitive", C.c_int32), ("dfs", C.c_int32), ("max_depth", C.c_uint32),
                ("min_transitive_len", C.c_int32), ("min_distance_between_ranges", C.c_int32),
                ("min_output_length", C.c_int32), ("min_identity", C.c_double),
                ("store_cigar", C.c_int32), ("multi_impg", C.c_int32), ("original_sequence_coordinates", C.c_int32),
                ("consider_strandness", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("projected", C.c_uint64), ("pairs", C.c_uint64), ("frontier_ranges", C.c_uint64),
                ("levels", C.c_uint32), ("ms_total", C.c_float), ("ms_lookup", C.c_float),
                ("ms_project", C.c_float), ("ms_update", C.c_float), ("project_launches", C.c_uint64),
                ("ms_exchange", C.c_float)]


class DevicePart(C.Structure):  # impg_gpu_device_part_t
    _fields_ = [("first_range", C.c_size_t), ("n_ranges", C.c_size_t), ("level", C.c_uint32), ("n_frontier", C.c_uint32),
                ("slot_stride", C.c_uint32), ("n_slots", C.c_uint64), ("query_id", C.c_void_p), ("coords", C.c_void_p), ("source", C.c_void_p),
                ("frontier", C.c_void_p), ("rows", C.c_void_p), ("offsets", C.c_void_p)]


ROWS_ATTRIBUTED, ROWS_ORDERED, ROWS_ORDERED_SLOTS = 0, 1, 2
REGIONS_MASKED, REGIONS_MISSING = 0, 1
SELECT_LONGEST, SELECT_TOTAL, SELECT_SAMPLE, SELECT_HAPLOTYPE = 0, 1, 2, 3
BED_ROW_DTYPE = np.dtype([("range", "<u4"), ("query_id", "<u4"), ("start", "<i4"), ("end", "<i4"), ("strand", "<u4")])  # impg_gpu_bed_row_t
PARTITION_ROW_DTYPE = np.dtype([("seq_id", "<u4"), ("start", "<i4"), ("end", "<i4")])  # impg_gpu_partition_row_t


class PartitionOpts(C.Structure):  # impg_gpu_partition_opts_t
    _fields_ = [("window_size", C.c_int64), ("merge_distance", C.c_int32), ("min_missing_size", C.c_int32),
                ("min_boundary_distance", C.c_int32), ("selection", C.c_int32), ("separator", C.c_char_p),
                ("rehome_singletons", C.c_int32), ("state_on_host", C.c_int32)]


class SupportOpts(C.Structure):  # impg_gpu_support_opts_t
    _fields_ = [("span_bp", C.c_int32), ("merge_distance", C.c_int32)]


class RefineOpts(C.Structure):  # impg_gpu_refine_opts_t
    _fields_ = [("span_bp", C.c_int32), ("max_extension", C.c_double), ("extension_step", C.c_int32), ("merge_distance", C.c_int32),
                ("use_max_entities", C.c_int32), ("support_on_host", C.c_int32)]


class SortPass(C.Structure):  # impg_gpu_sort_pass_t
    _fields_ = [("keys", C.c_void_p), ("wide", C.c_int), ("bits", C.c_uint)]


RESOLVE_FIELDS = ("records", "resolved", "absent", "inconsistent", "ops_in", "ops_out", "m_ops", "m_bases", "m_eq_bases", "m_x_bases",
                  "bad_eq_bases", "bad_x_bases")


class ResolveReport(C.Structure):  # impg_gpu_resolve_report_t
    _fields_ = [(k, C.c_uint64) for k in RESOLVE_FIELDS]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in RESOLVE_FIELDS}


REFINE_RECORD_DTYPE =np.dtype([("target_id", "<u4"), ("refined_start", "<i4"), ("refined_end", "<i4"), ("original_start", "<i4"),
                                ("original_end", "<i4"), ("left_extension", "<i4"), ("right_extension", "<i4"), ("support_count", "<u4"),
                                ("original_support_count", "<u4")])  # impg_gpu_refine_record_t
ROWS_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p))
SURVIVOR_DTYPE = np.dtype([("seq_id", "<u4"), ("q_lo", "<i4"), ("q_hi", "<i4")])  # impg_gpu_survivor_t
NO_ENTITY = 0xFFFFFFFF
FRONTIER_DTYPE = np.dtype([("target_id", "<u4"), ("start", "<i4"), ("end", "<i4"), ("range_idx", "<u4")])


class ImpgGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("impg_gpu error %d: %s" % (code, msg))
        self.code = code


def build(force=False):
    """Compile libimpg_gpu.so for gfx950 (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "-s", "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    return LIB_PATH


class Mask(C.Structure):  # impg_gpu_mask_t
    _fields_ = [("n_seqs", C.c_uint32), ("seq_id", C.c_void_p), ("sequence_length", C.c_void_p),
                ("range_off", C.c_void_p), ("ranges", C.c_void_p)]


# every symbol include/impg_gpu.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("impg_gpu_last_error", C.c_char_p, []),
    ("impg_gpu_device_count", C.c_int, []),
    ("impg_gpu_index_create", C.c_int, [_P, C.c_size_t, _P, C.c_size_t, _P, C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    ("impg_gpu_index_create_files", C.c_int, [_P, C.c_size_t, _P, C.c_size_t, _P, C.c_uint32, _P, C.c_uint32, C.c_int, C.c_int,
                                              C.c_int, C.POINTER(_P)]),
    ("impg_gpu_index_create_tracepoints", C.c_int, [_P, C.c_size_t, _P, _P, _P, C.c_size_t, _P, _P, C.c_uint32, C.c_int, C.c_int, C.c_int,
                                                    C.POINTER(_P)]),
    ("impg_gpu_index_create_tracepoints_multi", C.c_int, [_P, C.c_size_t, _P, _P, _P, C.c_size_t, _P, _P, C.c_uint32, C.c_int, C.c_int, _P, C.c_int, C.c_int,
                                                    C.POINTER(_P)]),
    ("impg_gpu_index_create_from_paf", C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    ("impg_gpu_index_create_from_paf_streamed", C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.POINTER(_P)]),
    ("impg_gpu_selftest_paf_ingest", C.c_int, [C.POINTER(C.c_char_p), C.c_size_t, C.c_uint64, C.c_int, C.c_int, C.c_uint, C.c_uint64, C.POINTER(_P),
                                               C.POINTER(C.c_size_t), C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(_P), C.POINTER(C.c_size_t),
                                               C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(_P), _P]),
    ("impg_gpu_cigar_resolve", C.c_int, [_P, C.c_size_t, _P, C.c_size_t, _P, _P, C.c_uint32, _P, C.c_int, C.c_int, C.POINTER(_P), C.POINTER(_P),
                                         C.POINTER(C.c_size_t), C.POINTER(_P), C.POINTER(ResolveReport)]),
    ("impg_gpu_selftest_cigar_resolve", C.c_int, [_P, C.c_size_t, _P, C.c_size_t, _P, _P, C.c_uint32, _P, C.c_int, C.c_int, C.c_uint32, C.POINTER(_P),
                                                  C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(_P), C.POINTER(ResolveReport)]),
    ("impg_gpu_index_create_from_paf_resolved", C.c_int, [C.POINTER(C.c_char_p), C.c_int, _P, C.c_int, C.c_int, C.c_int, C.POINTER(ResolveReport),
                                                          C.POINTER(_P), C.POINTER(_P)]),
    ("impg_gpu_index_save", C.c_int, [_P, C.c_char_p]),
    ("impg_gpu_index_load", C.c_int, [C.c_char_p, C.c_int, C.POINTER(_P)]),
    ("impg_gpu_query_batch_stream", C.c_int, [_P, _P, C.c_size_t, _P, _P, _P, C.c_size_t, C.c_size_t, _P, _P, C.POINTER(C.c_uint64)]),
    ("impg_gpu_index_load_rank", C.c_int, [C.c_char_p, C.c_int, _P, C.POINTER(_P)]),
    ("impg_gpu_index_load_multi", C.c_int, [C.c_char_p, _P, C.c_int, C.c_int, C.POINTER(_P)]),
    ("impg_gpu_index_load_impg", C.c_int, [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    ("impg_gpu_index_destroy", None, [_P]),
    ("impg_gpu_num_seqs", C.c_uint32, [_P]),
    ("impg_gpu_seq_name", C.c_char_p, [_P, C.c_uint32]),
    ("impg_gpu_seq_len", C.c_int64, [_P, C.c_uint32]),
    ("impg_gpu_seq_id", C.c_int64, [_P, C.c_char_p]),
    ("impg_gpu_num_targets", C.c_size_t, [_P]),
    ("impg_gpu_target_ids", C.c_size_t, [_P, _P, C.c_size_t]),
    ("impg_gpu_num_entries", C.c_size_t, [_P]),
    ("impg_gpu_num_records", C.c_size_t, [_P]),
    ("impg_gpu_device_bytes", C.c_size_t, [_P]),
    ("impg_gpu_index_approximate", C.c_int, [_P]),
    ("impg_gpu_set_option", C.c_int, [_P, C.c_char_p, C.c_int64]),
    ("impg_gpu_get_counter", C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int64)]),
    ("impg_gpu_option_key", C.c_char_p, [C.c_size_t]),
    ("impg_gpu_counter_key", C.c_char_p, [C.c_size_t]),
    ("impg_gpu_host_pool_trim", C.c_uint64, [C.c_uint64]),
    ("impg_gpu_visit_rank", C.c_int, [C.c_uint32, C.c_int, _P]),
    ("impg_gpu_query_batch", C.c_int, [_P, _P, C.c_size_t, C.POINTER(Params), C.POINTER(_P)]),
    ("impg_gpu_query_batch_masked", C.c_int, [_P, _P, C.c_size_t, C.POINTER(Params), _P, C.POINTER(_P)]),
    ("impg_gpu_query_batch_filtered", C.c_int, [_P, _P, C.c_size_t, C.POINTER(Params), _P, _P, C.POINTER(_P)]),
    ("impg_gpu_parse_subsequence", C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32)]),
    ("impg_gpu_subset_keep", C.c_int, [C.c_char_p, C.c_size_t, _P, C.c_size_t, _P, C.POINTER(C.c_size_t)]),
    ("impg_gpu_query", C.c_int, [_P, C.c_uint32, C.c_int32, C.c_int32, C.POINTER(Params), C.POINTER(_P)]),
    ("impg_gpu_results_num_ranges", C.c_size_t, [_P]),
    ("impg_gpu_results_total", C.c_size_t, [_P]),
    ("impg_gpu_results_offsets", _P, [_P]),
    ("impg_gpu_results_intervals", _P, [_P]),
    ("impg_gpu_results_projected", C.c_uint64, [_P]),
    ("impg_gpu_results_cigar_offsets", _P, [_P]),
    ("impg_gpu_results_cigar_ops", _P, [_P]),
    ("impg_gpu_results_timing", None, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("impg_gpu_results_free", None, [_P]),
    ("impg_gpu_query_batch_stats", C.c_int, [_P, _P, C.c_size_t, C.POINTER(Params), _P, _P, C.POINTER(Stats)]),
    ("impg_gpu_query_batch_stats_dev", C.c_int, [_P, _P, C.c_size_t, C.POINTER(Params), _P, _P, C.POINTER(Stats)]),
    ("impg_gpu_query_batch_device", C.c_int, [_P, _P, C.c_size_t, C.c_int, C.POINTER(Params), C.c_int, C.POINTER(_P)]),
    ("impg_gpu_device_rows_num_parts", C.c_size_t, [_P]),
    ("impg_gpu_device_rows_part", C.c_int, [_P, C.c_size_t, C.POINTER(DevicePart)]),
    ("impg_gpu_device_rows_stats", None, [_P, C.POINTER(Stats)]),
    ("impg_gpu_device_rows_place_ms", C.c_float, [_P]),
    ("impg_gpu_device_rows_part_device", C.c_int, [_P, C.c_size_t, C.POINTER(C.c_int)]),
    ("impg_gpu_device_rows_batch_offset", C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("impg_gpu_device_rows_check", C.c_int, [_P, _P, _P]),
    ("impg_gpu_device_rows_free", None, [_P]),
    ("impg_gpu_bed_merge", C.c_long, [_P, C.c_size_t, C.c_int32, C.c_int]),
    ("impg_gpu_results_bed", C.c_int, [_P, _P, _P, C.POINTER(Params), C.c_int32, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    ("impg_gpu_query_batch_bed", C.c_int, [_P, _P, C.c_size_t, C.POINTER(Params), _P, C.c_int32, _P, C.POINTER(_P), C.POINTER(C.c_size_t),
                                           _P]),
    ("impg_gpu_query_batch_bed_fd", C.c_int, [_P, _P, C.c_size_t, C.POINTER(Params), _P, C.c_int32, _P, C.c_int, C.POINTER(C.c_uint64), _P]),
    ("impg_gpu_query_batch_bedpe", C.c_int, [_P, _P, C.c_size_t, C.POINTER(Params), _P, C.c_int32, _P, C.POINTER(_P), C.POINTER(C.c_size_t),
                                             _P]),
    ("impg_gpu_query_batch_bedpe_fd", C.c_int, [_P, _P, C.c_size_t, C.POINTER(Params), _P, C.c_int32, _P, C.c_int, C.POINTER(C.c_uint64), _P]),
    ("impg_gpu_query_batch_paf", C.c_int, [_P, _P, C.c_size_t, C.POINTER(Params), _P, C.c_int32, _P, C.POINTER(_P), C.POINTER(C.c_size_t),
                                           _P]),
    ("impg_gpu_query_batch_paf_fd", C.c_int, [_P, _P, C.c_size_t, C.POINTER(Params), _P, C.c_int32, _P, C.c_int, C.POINTER(C.c_uint64), _P]),
    ("impg_gpu_results_paf", C.c_int, [_P, _P, _P, C.POINTER(Params), C.c_int32, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    ("impg_gpu_parse_cigar", C.c_long, [C.c_char_p, C.c_size_t, _P, C.c_size_t]),
    ("impg_gpu_parse_target_range", C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("impg_gpu_comm_unique_id", C.c_int, [_P, C.c_int]),
    ("impg_gpu_comm_create_rccl", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    ("impg_gpu_comm_create_host", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    ("impg_gpu_comm_destroy", None, [_P]),
    ("impg_gpu_comm_info", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_char_p)]),
    ("impg_gpu_comm_check", C.c_int, [_P, C.c_int]),
    ("impg_gpu_index_create_rank", C.c_int, [_P, C.c_size_t, _P, C.c_size_t, _P, C.c_uint32, _P, C.c_uint32, C.c_int, C.c_int,
                                             C.c_int, _P, C.POINTER(_P)]),
    ("impg_gpu_index_create_from_paf_rank", C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    ("impg_gpu_index_create_multi", C.c_int, [_P, C.c_size_t, _P, C.c_size_t, _P, C.c_uint32, _P, C.c_uint32, C.c_int, C.c_int,
                                              _P, C.c_int, C.c_int, C.POINTER(_P)]),
    ("impg_gpu_index_create_from_paf_multi", C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int,
                                                       C.POINTER(_P)]),
    ("impg_gpu_shard_assign", C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    ("impg_gpu_index_shard_info", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _P, C.c_size_t]),
    ("impg_gpu_index_hop_profile", C.c_int, [_P, _P, C.c_size_t, C.c_int, C.POINTER(C.c_size_t)]),
    ("impg_gpu_regions_create", C.c_int, [_P, C.c_uint32, C.c_int, C.c_int, C.POINTER(_P)]),
    ("impg_gpu_regions_apply", C.c_int, [_P, _P, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("impg_gpu_regions_apply_device", C.c_int, [_P, _P, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, _P, C.c_size_t,
                                                C.POINTER(C.c_size_t)]),
    ("impg_gpu_regions_last_rows", C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("impg_gpu_regions_get", C.c_int, [_P, C.c_int, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("impg_gpu_regions_select", C.c_int, [_P, C.c_int, C.c_char_p, _P, C.c_int64, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("impg_gpu_regions_free", None, [_P]),
    ("impg_gpu_partition_starting_windows", C.c_int, [_P, C.c_size_t, _P, C.c_uint32, C.c_int64, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("impg_gpu_partition_rehome", C.c_int, [_P, _P, C.c_size_t]),
    ("impg_gpu_partition_bed_text", C.c_int, [_P, _P, C.c_size_t, _P, C.c_uint32, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    ("impg_gpu_partition_create", C.c_int, [_P, C.POINTER(Params), C.POINTER(PartitionOpts), _P, C.c_size_t, C.POINTER(_P)]),
    ("impg_gpu_partition_next_windows", C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("impg_gpu_partition_window", C.c_int, [_P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("impg_gpu_partition_run", C.c_int, [_P, C.c_char_p, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
    ("impg_gpu_partition_run_fasta", C.c_int, [_P, C.c_char_p, C.POINTER(C.c_uint64)]),
    ("impg_gpu_partition_window_fasta", C.c_int, [_P, _P, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    ("impg_gpu_partition_rows_fasta", C.c_int, [_P, _P, C.c_size_t, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    ("impg_gpu_partition_fasta_text", C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    ("impg_gpu_partition_regions", _P, [_P]),
    ("impg_gpu_partition_counter", C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int64)]),
    ("impg_gpu_partition_destroy", None, [_P]),
    ("impg_gpu_support_rows", C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, _P, _P, C.POINTER(SupportOpts), C.c_int, C.c_int, _P, _P,
                                        C.POINTER(_P), C.POINTER(C.c_uint64)]),
    ("impg_gpu_refine", C.c_int, [_P, _P, C.c_size_t, C.POINTER(Params), C.POINTER(RefineOpts), _P, _P, _P, _P, C.POINTER(_P)]),
    ("impg_gpu_refine_rows", C.c_int, [ROWS_CB, _P, _P, C.c_uint32, _P, C.c_size_t, C.POINTER(RefineOpts), _P, _P, _P, _P, C.c_int, C.POINTER(_P)]),
    ("impg_gpu_refine_num_records", C.c_size_t, [_P]),
    ("impg_gpu_refine_records", _P, [_P]),
    ("impg_gpu_refine_survivor_offsets", _P, [_P]),
    ("impg_gpu_refine_survivors", _P, [_P]),
    ("impg_gpu_refine_stats", None, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("impg_gpu_refine_batch_times", C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("impg_gpu_refine_text", C.c_int, [_P, _P, C.c_uint32, _P, C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(_P), C.POINTER(C.c_size_t)]),
    ("impg_gpu_refine_free", None, [_P]),
    ("impg_gpu_entity_ids", C.c_int, [_P, C.c_size_t, C.c_int, C.c_char_p, _P, C.POINTER(C.c_uint32)]),
    ("impg_synth_paf", C.c_int, [C.c_uint64, C.c_size_t, C.c_uint32, C.c_int32, C.c_int32, C.c_uint32, _P, _P, C.c_size_t,
                                 C.POINTER(C.c_size_t)]),
    ("impg_synth_paf_text", C.c_int, [C.c_uint64, C.c_size_t, C.c_uint32, C.c_int32, C.c_int32, C.c_uint32, C.c_char_p]),
    ("impg_synth_skewed_paf_text", C.c_int, [C.c_uint64, C.c_size_t, C.c_uint32, C.c_int32, C.c_char_p, C.POINTER(C.c_uint64)]),
    ("impg_gpu_selftest_order_sort", C.c_int, [C.c_int, C.c_uint32, C.c_uint, C.c_uint64]),
    ("impg_gpu_selftest_scan", C.c_int, [C.c_int, C.c_int, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.POINTER(C.c_uint64), _P]),
    ("impg_gpu_selftest_offsets", C.c_int, [C.c_int, _P, C.c_uint32, C.c_int, _P, C.POINTER(C.c_uint64)]),
    ("impg_gpu_selftest_key_sort", C.c_int, [C.c_int, C.c_uint32, _P, C.c_uint32, C.c_int, _P, C.c_uint32, _P, _P]),
    ("impg_gpu_selftest_bed_rows", C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint32, C.c_uint64, C.c_int32, C.c_int, C.c_int, _P, C.POINTER(_P),
                                             C.POINTER(C.c_size_t), C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(_P), C.POINTER(_P),
                                             C.POINTER(C.c_size_t)]),
    ("impg_gpu_selftest_bedpe_rows", C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, C.c_int32, C.c_int, _P, C.POINTER(_P),
                                               C.POINTER(C.c_size_t)]),
    ("impg_gpu_selftest_paf_rows", C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint32, _P, _P, C.c_int32, C.c_int, _P, C.POINTER(_P),
                                             C.POINTER(C.c_size_t)]),
    ("impg_gpu_sequences_from_fasta", C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    ("impg_gpu_sequences_from_memory", C.c_int, [_P, _P, _P, C.c_size_t, C.POINTER(_P)]),
    ("impg_gpu_sequences_num", C.c_size_t, [_P]),
    ("impg_gpu_sequences_name", C.c_char_p, [_P, C.c_size_t]),
    ("impg_gpu_sequences_bases", _P, [_P, C.c_size_t, C.POINTER(C.c_uint64)]),
    ("impg_gpu_sequences_exceptions", C.c_int, [_P, C.c_size_t, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("impg_gpu_sequences_free", None, [_P]),
    ("impg_gpu_index_set_sequences", C.c_int, [_P, _P]),
    ("impg_gpu_index_load_sequences", C.c_int, [_P, _P, C.c_size_t]),
    ("impg_gpu_selftest_sequence_reader", C.c_int, [C.c_char_p, C.c_uint64, C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64),
                                                    C.POINTER(C.c_uint64)]),
    ("impg_gpu_selftest_sequence_ingest_host", C.c_int, [_P, C.c_size_t, _P, _P, C.c_size_t, C.c_uint64, C.c_int, _P, C.POINTER(_P),
                                                         C.POINTER(C.c_size_t), _P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), _P]),
    ("impg_gpu_query_batch_fasta", C.c_int, [_P, _P, C.c_size_t, C.POINTER(Params), _P, C.c_int32, _P, C.c_int, C.POINTER(_P),
                                             C.POINTER(C.c_size_t), _P]),
    ("impg_gpu_query_batch_fasta_fd", C.c_int, [_P, _P, C.c_size_t, C.POINTER(Params), _P, C.c_int32, _P, C.c_int, C.c_int,
                                                C.POINTER(C.c_uint64), _P]),
    ("impg_gpu_results_fasta", C.c_int, [_P, _P, C.POINTER(Params), C.c_int32, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    ("impg_gpu_fasta_text", C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, C.c_int32, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    ("impg_gpu_selftest_fasta_rows", C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint32, C.c_int32, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    ("impg_synth_seq_name", C.c_int, [C.c_uint32, C.c_char_p, C.c_size_t]),
    ("impg_synth_bed", C.c_int, [C.c_uint64, C.c_size_t, C.c_uint32, C.c_int32, C.c_int32, _P]),
]

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libimpg_gpu.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "or `make -C impg_amd/csrc` (there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _LIB = L
    return _LIB


def check(rc):
    if rc != IMPG_OK:
        raise ImpgGpuError(rc, lib().impg_gpu_last_error().decode(errors="replace"))


def free(ptr):
    C.CDLL(None).free(ptr)
