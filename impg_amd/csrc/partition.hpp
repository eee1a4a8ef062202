// `impg partition` (reference src/commands/partition.rs:158-1408): the state between two windows' queries --
// masked_regions and missing_regions -- and the interval algebra that updates it.  partition.cpp holds the host twin
// and everything that is host work in the reference too (windows, name grouping, rehoming, text); partition_device.hip
// holds the same state as two CSR tables in HBM and the same algebra as kernels.
#pragma once
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "engine.hpp"

namespace impg {

struct PIv {  // the query-side interval of a row: all that reaches BED output
  uint32_t seq;
  int32_t lo, hi;
};

// What select_and_window_sequences (partition.rs:715-937) needs to know about the missing map.
struct SelSummary {
  bool any = false;  // the longest missing range: max by (length, sequence id, start)
  uint32_t seq = 0;
  int32_t lo = 0, hi = 0;
  std::vector<int64_t> total;  // missing bases per sequence; 0 = the sequence has left the map
};

struct HostRegions {
  std::vector<int32_t> len;
  std::vector<std::vector<std::pair<int32_t, int32_t>>> masked, missing;
  HostRegions(const int64_t *seq_len, uint32_t n_seq);
  // merge_overlaps(d), extend_to_close_boundaries, mask_and_update_regions, merge_overlaps(0)
  void apply(const impg_gpu_interval_t *rows, size_t n, int32_t d, int32_t min_missing, int32_t min_boundary, std::vector<PIv> &out);
  void summary(SelSummary &s) const;
};

struct DeviceRegions {
  int device;
  uint32_t n_seq;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  DevBuf len;                                // int32[n_seq]
  DevBuf m_off[2], m_rng[2], x_off[2], x_rng[2];  // masked / missing: u32 off[n_seq + 1], int2 ranges; two buffers each
  int m_cur = 0, x_cur = 0;
  uint32_t n_mask = 0, n_missing = 0;
  bool mask_has_empty = false;
  SelSummary longest;                        // of the current missing table (the totals are read on demand)
  DevBuf totals[2];                          // u64[n_seq] each: missing bases per sequence; a window writes the other one
  int t_cur = 0;                             // ... and it becomes current together with the tables, or not at all
  uint64_t launches = 0;                     // kernel launches + rocPRIM calls issued (a library sort or scan is several kernels and counts once)
  // scratch
  DevBuf key_a, key_b, val_a, val_b, mk, pm, head, pos, a_key, a_hi, b_lo, b_hi, c_key, c_hi, e_key, e_hi, s_a, s_first, s_cnt,
      s_off, o_key, o_hi, t_key, t_hi, n_key, n_hi, ctr, out_rows, tmp, up_rows;
  uint32_t *h_hdr = nullptr;  // pinned
  DeviceRegions(int device, const int64_t *seq_len, uint32_t n_seq, hipStream_t s);
  ~DeviceRegions();
  // one window's steps 2-8 on rows that lie in HBM; the window's output rows come back
  void apply(const impg_gpu_interval_t *d_rows, uint32_t n, int32_t d, int32_t min_missing, int32_t min_boundary, std::vector<PIv> &out);
  void apply_host_rows(const impg_gpu_interval_t *rows, uint32_t n, int32_t d, int32_t min_missing, int32_t min_boundary, std::vector<PIv> &out);
  void get(int which, uint32_t *off_out, std::vector<int32_t> &ranges);
  void summary(SelSummary &s, bool want_totals);
  const uint32_t *mask_off() const { return m_off[m_cur].as<uint32_t>(); }
  const int32_t *mask_ranges() const { return m_rng[m_cur].as<int32_t>(); }
};

// select_and_window_sequences from a summary; names may be null for longest / total
void select_windows(const SelSummary &s, const std::vector<int32_t> &len, int selection, const std::string &sep,
                    const std::vector<std::string> *names, int64_t window_size, std::vector<impg_gpu_range_t> &out);
// the name prefix sequences are grouped by: the first field, or the first two with the separator between them (:812-823)
std::string pansn_prefix(const std::string &name, const std::string &sep, bool haplotype);
// the windows of a starting-sequences list (partition.rs:220-246)
void starting_windows(const uint32_t *ids, size_t n, const std::vector<int32_t> &len, int64_t window_size, std::vector<impg_gpu_range_t> &out);
using Partition = std::pair<uint64_t, std::vector<PIv>>;
void rehome_singleton_slivers(std::vector<Partition> &parts);

// the rows of one transitive query left in HBM (capi.cpp): the per-query walk where it applies, the batch engine otherwise
uint32_t query_rows_device(impg_gpu_index &ix, Engine &E, const impg_gpu_range_t &range, const impg_gpu_params_t &p, DevBuf &rows,
                           const impg_gpu_interval_t *&d_rows, bool &walked);
Engine *try_lease_engine(impg_gpu_index &ix);  // null when every engine is out
void return_engine(impg_gpu_index &ix, Engine *e);

}  // namespace impg
