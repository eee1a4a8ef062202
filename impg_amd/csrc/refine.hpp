// The boundary support of `impg refine` (reference src/commands/refine.rs:665-850): for a batch of candidate regions, each
// with its query's rows in emission order, the sequences whose merged alignments cover both boundaries, and the number of
// distinct entities (PanSN keys, handed over as ids) among them.  refine.cpp holds the host twin, written the reference's
// sequential way, and the C entry points; refine_device.hip holds the same computation as kernels over rows that lie in HBM.
#pragma once
#include <cstdint>
#include <vector>

#include "engine.hpp"

namespace impg {

constexpr uint32_t NO_ENTITY = 0xFFFFFFFFu;

// What a call needs besides the rows: all host arrays, checked by the entry point.
struct SupportInput {
  const impg_gpu_range_t *cand = nullptr;  // [n_cand]: target and the clamped start / end
  size_t n_cand = 0;
  uint32_t n_seq = 0;
  const uint32_t *entity_of = nullptr;     // [n_seq] or null: identity
  const uint32_t *max_entities = nullptr;  // [n_cand] or null
  // the blacklist, normalised: per sequence sorted by start, overlapping ranges joined (both ends inclusive)
  std::vector<uint32_t> bl_off;            // [n_seq + 1], or empty: no blacklist
  std::vector<int32_t> bl_rng;             // (start, end) pairs
  int32_t span_bp = 0, merge_distance = 0;
};
struct SupportOutput {
  std::vector<uint32_t> count;                  // [n_cand]
  bool want_survivors = false;
  std::vector<uint64_t> surv_off;               // [n_cand + 1]
  std::vector<impg_gpu_survivor_t> survivors;   // ascending sequence id inside a candidate
  uint64_t longest_group = 0;                   // rows of the longest (candidate, sequence) group folded
};

// sorts every sequence's ranges and joins those that overlap; IMPG_E_INVALID for a table that is not one
void normalise_blacklist(const uint32_t *off, const int32_t *ranges, uint32_t n_seq, std::vector<uint32_t> &off_out, std::vector<int32_t> &rng_out);
// the host twin: rows and offsets in host memory
void support_host(const impg_gpu_interval_t *rows, const uint64_t *offsets, const SupportInput &in, SupportOutput &out);

// The kernels' scratch and the tables of one run of calls (one refine pass after the other reuses them).
struct SupportDevice {
  int device;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  DevBuf key_a, key_b, val_a, val_b, flag, pos, hull, s_cand, s_seq, s_rng, s_off, d_cand, d_ent, d_max, d_bloff, d_blrng, d_count, d_nrow, ctr, tmp,
      up_rows, up_off;
  uint32_t *h_hdr = nullptr;  // pinned
  SupportDevice(int device, hipStream_t s);
  ~SupportDevice();
  // rows[offsets[c] .. offsets[c + 1]) of candidate c, both in this device's memory (offsets: u32, as an ordered part's)
  void run(const impg_gpu_interval_t *d_rows, uint32_t n_rows, const uint32_t *d_offsets, const SupportInput &in, SupportOutput &out);
  void run_host_rows(const impg_gpu_interval_t *rows, const uint64_t *offsets, const SupportInput &in, SupportOutput &out);
};

enum RefineStat { REFINE_PASSES = 0, REFINE_CANDIDATES, REFINE_PARTS, REFINE_ROWS_TO_HOST, REFINE_LONGEST_GROUP };

// build_flanks (refine.rs:852-876) and the reading of --max-extension (:177-185)
std::vector<int32_t> build_flanks(int32_t max_extension, int32_t step);
int32_t max_extension_bp(double max_extension, int32_t locus_len);

// capi.cpp: impg_gpu_query_batch_device with the subset filter of impg_gpu_query_batch_filtered (one GPU only)
int query_batch_device_filtered(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, int ranges_on_device,
                                const impg_gpu_params_t *params, int layout, const uint8_t *subset_keep, impg_gpu_device_rows_t **out);

}  // namespace impg
