// Run-time settings of an index handle: the values impg_gpu_set_option stores, the table it checks them against, what a
// multi-GPU handle hands to its ranks, and the index builders' environment switches.  Host-only: no HIP in here, so a
// plain C++ program can include it and walk the table.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace impg {

// Every stored option, under its key's name, with its default.  An engine takes a copy when it is leased (Engine::opt).
// "results identical": the option moves work between kernels or changes a layout nobody reads by position, for A/B runs
// and tests; what a query returns does not depend on it.
struct Options {
  int64_t pair_budget = 1ll << 28;    // candidate pairs per level kept in HBM at once; a level beyond it splits the batch by ranges
  int64_t chunk_ranges = 0;           // ranges per chunk (0 = try the whole batch; on a sharded index: one chunk per lane, at most 50 000)
  int64_t locality_min = 4096;        // frontier size from which the projection runs in window order (0 = never; results identical)
  int64_t device_rows_pool_bytes = 160ll << 30;  // HBM kept between impg_gpu_query_batch_device calls: freed slot arrays, reused by the next call
  int64_t fuse_final_level = 1;       // a counting run's final level enumerates its pairs from the count pass's windows: no emit pass (results identical)
  int64_t regroup_entries = 1;        // a projection block sorts its 256 pairs by entry before reading the index (results identical)
  int64_t walk_kernel = 1;            // the per-query walk (walk_device.inc): 0 never, 1 DFS batches of any size and depth-limited BFS batches of <= 64 ranges, 2 every BFS batch of <= 64 ranges
  int64_t segment_groups = 1;         // the update's hits grouped query by query (1) or by the library's radix sort (0); results identical
  int64_t segment_parts = 0;          // slices a query's hits are grouped in: 0 = from the level's size, n = that many on every level that groups by segments (testing; results identical)
  int64_t walk_members = 0;           // workgroups per query of the walk's grid form (depth-limited BFS, <= 64 ranges): 0 = as many as fit (<= 32), 1 = no grid form
  int64_t filter_covered = 0;         // visited update: hits covered by their group's old list dropped before the replay (0 off: it bought nothing where hits are covered by the list as it GROWS; 1 always; 2 long groups; results identical)
  int64_t update_stats = 0;           // visited update: every level's groups per tier and rare path counted into the update_* counters (1: one small copy per level)
  int64_t lookup_stats = 0;           // lookup: every level's wide windows counted by the path that emitted them into the lookup_wide_* counters (1: one small copy per level)
  int64_t wide_emit_cap = 4096;       // hits lookup_emit_wide_kernel sorts in one LDS pass (testing; results identical)
  int64_t wide_emit_bins = 1024;      // rank bins it groups a window's hits by beyond that (testing; results identical)
  int64_t lookup_coop = 1;            // lookup: a level with a lookup order is counted by lookup_count_coop_kernel (1) or by the lane kernel (0); results identical
  int64_t lookup_coop_span = 256;     // entries a wave of that kernel stages at most; a wider span takes the lane body (testing; results identical)
  int64_t place_offsets_blocks = 1;   // a fused final level takes its place offsets in two levels, a scan over the sums of the count pass's waves (1), or from the scan over every range's count (0); results identical
  // store_cigar on a tracepoint index: 0 refused; 1 every row carries the approximate mode's CIGAR, [matches '='] [mismatches 'X']
  // with a zero count left out (impg.rs:1479-1486) -- statistics, not an alignment: the lengths do not add up to the row's
  // coordinates.  No effect on a CIGAR index; not saved with the index.
  int64_t approximate_cigar = 0;
  int64_t free_slot_order = 1;        // counting runs lay their slots out in projection order (1) or keep the reference order (0); results identical
  // failure injection for the tests of the multi-rank failure agreement (0 = off): (rank + 1) << 16 | hop of the batch
  // (1-based, counted per lane) at which that rank throws on the owner side / on the home side of the hop
  int64_t debug_fail_owner = 0, debug_fail_home = 0;
  int64_t bed_text_piece_bytes = 256ll << 20;  // device BED text: bytes of whole rows per piece crossing PCIe (bed_device.hip; results identical)
  int64_t bedpe_group_log2 = 2;       // device BEDPE: log2 of the lanes that sum one row's CIGAR (bedpe_device.hip; 2 .. 6; results identical)
  int64_t paf_group_log2 = 2;         // device PAF: log2 of the lanes that fuse and print one row's CIGAR (paf_device.inc; 2 .. 6; results identical)
  int64_t sequence_store_packed = 0;  // the form impg_gpu_index_set_sequences uploads: 0 a byte per base, 1 two bits per base + runs of the other bytes, 2 the smaller (fasta_device.hip; read at attach; text identical)
  int64_t sequence_ingest_piece_bytes = 64ll << 20;  // impg_gpu_index_load_sequences: bytes of a file's text per piece crossing PCIe (sequence_ingest.cpp; a multiple of 16; results identical)
  int64_t lane_schedule = 0;        // tests: forced lane start / hand-over order of a sharded batch (run_lanes, sharded.cpp; 0 = off, then IMPG_LANE_SCHEDULE)
};

// One row per key of impg_gpu_set_option: lo <= value <= hi or the call is refused with `refusal` (IMPG_E_INVALID).
struct OptionRow {
  const char *key;
  int64_t lo, hi;
  int64_t Options::*member;  // null: the key acts instead of storing (impg_gpu_set_option runs it)
  bool flag;                 // stored as value != 0
  bool to_ranks;             // a multi-GPU handle copies it to its ranks before every batch (options_to_ranks)
  const char *refusal;
};
constexpr OptionRow OPTION_TABLE[] = {
    {"pair_budget", 1024, 0xFFFFFFEFll, &Options::pair_budget, false, true, "pair_budget out of range"},
    {"chunk_ranges", 0, (1ll << 31) - 1, &Options::chunk_ranges, false, true, "chunk_ranges out of range"},
    {"locality_min", 0, (1ll << 31) - 1, &Options::locality_min, false, true, "locality_min out of range"},
    {"device_rows_pool_bytes", 0, INT64_MAX, &Options::device_rows_pool_bytes, false, true, "device_rows_pool_bytes must not be negative"},
    {"fuse_final_level", INT64_MIN, INT64_MAX, &Options::fuse_final_level, true, true, ""},
    {"regroup_entries", INT64_MIN, INT64_MAX, &Options::regroup_entries, true, false, ""},
    {"walk_kernel", 0, 2, &Options::walk_kernel, false, false, "walk_kernel is 0, 1 or 2"},
    {"segment_groups", INT64_MIN, INT64_MAX, &Options::segment_groups, true, false, ""},
    {"segment_parts", 0, 4096, &Options::segment_parts, false, false, "segment_parts is 0 .. 4096"},
    {"walk_members", 0, 64, &Options::walk_members, false, false, "walk_members is 0 .. 64"},
    {"filter_covered", 0, 2, &Options::filter_covered, false, false, "filter_covered is 0, 1 or 2"},
    {"update_stats", INT64_MIN, INT64_MAX, &Options::update_stats, true, false, ""},
    {"lookup_stats", INT64_MIN, INT64_MAX, &Options::lookup_stats, true, false, ""},
    {"wide_emit_cap", 64, 4096, &Options::wide_emit_cap, false, false, "wide_emit_cap is 64 .. 4096"},
    {"wide_emit_bins", 2, 1024, &Options::wide_emit_bins, false, false, "wide_emit_bins is 2 .. 1024"},
    {"lookup_coop", INT64_MIN, INT64_MAX, &Options::lookup_coop, true, false, ""},
    {"lookup_coop_span", 4, 256, &Options::lookup_coop_span, false, false, "lookup_coop_span is 4 .. 256"},
    {"place_offsets_blocks", INT64_MIN, INT64_MAX, &Options::place_offsets_blocks, true, false, ""},
    {"approximate_cigar", 0, 1, &Options::approximate_cigar, false, true, "approximate_cigar is 0 or 1"},
    {"free_slot_order", INT64_MIN, INT64_MAX, &Options::free_slot_order, true, false, ""},
    {"debug_fail_owner", 0, 0xFFFFFFFFll, &Options::debug_fail_owner, false, true, "debug_fail_* out of range"},
    {"debug_fail_home", 0, 0xFFFFFFFFll, &Options::debug_fail_home, false, true, "debug_fail_* out of range"},
    {"lane_schedule", 0, INT64_MAX, &Options::lane_schedule, false, true, "lane_schedule out of range"},
    {"bed_text_piece_bytes", 64, 1ll << 40, &Options::bed_text_piece_bytes, false, false, "bed_text_piece_bytes is 64 .. 2^40"},
    {"bedpe_group_log2", 2, 6, &Options::bedpe_group_log2, false, false, "bedpe_group_log2 is 2 .. 6"},
    {"paf_group_log2", 2, 6, &Options::paf_group_log2, false, false, "paf_group_log2 is 2 .. 6"},
    {"sequence_store_packed", 0, 2, &Options::sequence_store_packed, false, false, "sequence_store_packed is 0, 1 or 2"},
    {"sequence_ingest_piece_bytes", 16, 1ll << 32, &Options::sequence_ingest_piece_bytes, false, false, "sequence_ingest_piece_bytes is 16 .. 2^32, a multiple of 16"},
    // Actions, so that a process's FIRST call costs what its later ones do.
    // A pinned host block of this size goes into the library's pool now (host_mem.cpp): the first result-returning call
    // copies into a recycled block like every later one (pinning 5 GB costs ~0.3-1 s, inside the call otherwise).  Blocks
    // beyond IMPG_PINNED_POOL_BYTES (6 GiB) are not kept: ask for what the calls return.
    {"prewarm_result_bytes", 0, INT64_MAX, nullptr, false, false, "prewarm_result_bytes is a size"},
    // The per-query walk's slabs (walk_device.inc) exist before the first call that needs them: 1 = the 64 slabs of the
    // per-call / small-batch BFS shape, 2 = also the DFS batch's slabs (~15 GB: one per resident wave).
    {"prewarm_walk", 0, 2, nullptr, false, false, "prewarm_walk is 0, 1 or 2"},
};
constexpr size_t N_OPTIONS = sizeof(OPTION_TABLE) / sizeof(OPTION_TABLE[0]);

constexpr const OptionRow *option_row(const char *key) {  // null: no such key
  for (const OptionRow &r : OPTION_TABLE)
    if (__builtin_strcmp(r.key, key) == 0) return &r;  // (the builtin: usable in a constant expression)
  return nullptr;
}
// range check, then store (an action's row stores nothing); false: refused, r.refusal says why
inline bool option_store(Options &o, const OptionRow &r, int64_t value) {
  if (value < r.lo || value > r.hi) return false;
  if (r.member) o.*r.member = r.flag ? (int64_t)(value != 0) : value;
  return true;
}
// What a multi-GPU handle hands to a rank before every batch, of whichever form.  The other options have no effect on
// a multi handle: its ranks keep their defaults.
inline void options_to_ranks(const Options &from, Options &rank) {
  for (const OptionRow &r : OPTION_TABLE)
    if (r.to_ranks) rank.*r.member = from.*r.member;
}

// The index builders' environment switches, read on every call (tests toggle them inside one process).  The host and
// the device builder must read them alike: they are each other's checkers.
struct BuildSwitches {
  bool prefix_lines;    // IMPG_PREFIX_LINES=0 builds without prefix lines
  bool identity_lines;  // IMPG_IDENTITY_LINES=1 builds the identity lines with the index, not on first use
  bool host_build;      // IMPG_BUILD_HOST: host threads build (and tokenise) instead of the device
  bool timing;          // IMPG_BUILD_TIMING: the builders' phases on stderr
  uint64_t batch_ops;   // IMPG_BUILD_BATCH_OPS: ops per upload of the device builder's batches (tests; the host builder has no batches)
  uint64_t paf_pool_ops;  // IMPG_PAF_INGEST_POOL_OPS: the first size of the streamed PAF ingest's op pool (tests; 0: from the files' sizes)
};
constexpr uint64_t BUILD_BATCH_OPS = 64ull << 20;  // 256 MB of ops per upload
inline BuildSwitches build_switches() {
  const char *pfx = getenv("IMPG_PREFIX_LINES"), *idl = getenv("IMPG_IDENTITY_LINES"), *bat = getenv("IMPG_BUILD_BATCH_OPS"),
             *ppo = getenv("IMPG_PAF_INGEST_POOL_OPS");
  const unsigned long long b = bat ? strtoull(bat, nullptr, 10) : 0ull;
  return BuildSwitches{!(pfx && atoi(pfx) == 0), idl && atoi(idl) == 1, getenv("IMPG_BUILD_HOST") != nullptr, getenv("IMPG_BUILD_TIMING") != nullptr,
                       b ? (uint64_t)b : BUILD_BATCH_OPS, ppo ? (uint64_t)strtoull(ppo, nullptr, 10) : 0ull};
}

}  // namespace impg
