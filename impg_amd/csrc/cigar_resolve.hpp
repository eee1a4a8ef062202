// M ops resolved against the sequences into '=' / 'X' ops, before the index is built: what the
// driver (cigar_resolve.cpp), its host twin and the kernels (cigar_resolve_device.hip) agree on.  tests/eqx_ref.py states
// the same rules in plain Python.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "impg_internal.hpp"

namespace impg {
namespace cigar_resolve {

constexpr uint32_t TILE_BASES = 1024;      // bases of an '=', 'X' or 'M' op one wave compares (a multiple of 64)
constexpr uint32_t TILE_BASES_MAX = 4096;  // a tile's 64-base masks live one per lane
enum Flag : uint8_t { FLAG_OK = 0, FLAG_ABSENT = 1, FLAG_INCONSISTENT = 2 };

// the FASTA writer's complement: A <-> T, C <-> G, every other byte itself (the store is upper case)
IMPG_HD inline uint8_t comp(uint8_t c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }

// What the host knows of a record before anybody reads an op: which store sequences it names (SEQ_ABSENT: none) and
// whether its intervals lie inside them.  pre[i] is FLAG_OK, FLAG_ABSENT or FLAG_INCONSISTENT; records without ops are FLAG_OK.
struct Plan {
  std::vector<uint32_t> store_of_id;  // [n_seq]
  std::vector<uint8_t> pre;           // [n_records]
  std::vector<uint64_t> first;        // [n_records + 1] ops of the records before record i (the pool in record order)
};
// IMPG_E_INVALID: a sequence id >= n_seq, a CIGAR outside the pool
Plan make_plan(const impg_gpu_record_t *records, size_t n_records, size_t n_ops, const char *const *names_of_ids, const int64_t *seq_len,
               uint32_t n_seq, const SeqStore &st);

struct Result {
  std::vector<uint64_t> off;   // [n_records] new cigar_off
  std::vector<uint32_t> len;   // [n_records] new cigar_len
  std::vector<uint8_t> flags;  // [n_records]
  uint64_t n_out = 0;
  impg_gpu_resolve_report_t report{};
};
// the records' flags counted into the report, and the build's limit on a record's ops (its own error)
void finish(const impg_gpu_record_t *records, size_t n_records, Result &r);

// The host twin: single-threaded and plain.  ops: the pool the records address; out: the new pool in record order.
void resolve_host(const impg_gpu_record_t *records, size_t n_records, const uint32_t *ops, const Plan &plan, const SeqStore &st, Result &r,
                  std::vector<uint32_t> &out);
// The kernels.  d_ops: the pool in HBM (the records address it in any order); d_out: the new pool, allocated at its size.
// tile_bases: 0 = TILE_BASES, else a multiple of 64 up to TILE_BASES_MAX.  IMPG_E_OOM names the bytes it wanted.
void resolve_device(const impg_gpu_record_t *records, size_t n_records, const uint32_t *d_ops, size_t n_ops, const Plan &plan, const SeqStore &st,
                    uint32_t tile_bases, int device, Result &r, DevBuf &d_out);

}  // namespace cigar_resolve
}  // namespace impg
