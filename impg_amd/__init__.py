"""impg_amd: MI355X-native batch interval-query + CIGAR-projection engine that
drops in behind impg's ImpgIndex::query / query_transitive_* (C ABI in
include/impg_gpu.h, HIP kernels in impg_amd/csrc)."""
from ._lib import (IMPG_E_HIP, IMPG_E_INVALID, IMPG_E_UNSUPPORTED, ORDER_COITREES, ORDER_SORTED, ImpgGpuError,
                   INTERVAL_DTYPE, RANGE_DTYPE, RECORD_DTYPE, build, lib)
from .index import Comm, DeviceRows, GpuImpg, PartitionSession, Regions, partitions_bed_text, rehome_singleton_slivers, starting_windows, support_rows, entity_ids, refine_rows, RefineResult, PreparedMask, QueryResults, Sequences, fasta_text, partition_fasta_text, prepare_mask, shard_assign, make_params, option_keys, counter_keys, resolve_cigars, parse_subsequence, subset_keep, synth_bed, synth_paf, synth_paf_text, synth_seq_name, synth_skewed_paf_text, selftest_sequence_reader, selftest_sequence_ingest_host

__all__ = ["GpuImpg", "DeviceRows", "Regions", "PartitionSession", "partitions_bed_text", "rehome_singleton_slivers", "starting_windows", "support_rows", "entity_ids", "refine_rows", "RefineResult", "PreparedMask", "prepare_mask", "Comm", "shard_assign", "QueryResults", "Sequences", "fasta_text", "partition_fasta_text", "make_params", "option_keys", "counter_keys", "resolve_cigars", "synth_paf", "synth_paf_text", "synth_skewed_paf_text", "synth_bed", "synth_seq_name", "selftest_sequence_reader", "selftest_sequence_ingest_host",
           "build", "lib", "ImpgGpuError", "ORDER_COITREES", "ORDER_SORTED", "IMPG_E_HIP", "IMPG_E_INVALID",
           "IMPG_E_UNSUPPORTED", "INTERVAL_DTYPE", "RANGE_DTYPE", "RECORD_DTYPE"]
