// PAF files streamed into HBM (impg_gpu_index_create_from_paf_streamed): what the driver and the host twin
// (paf_ingest.cpp) share with the kernels (paf_ingest_device.hip).  DESIGN.md section 5.5.
//
// A file's text is cut into pieces of whole lines: the bytes behind a piece's last '\n' open the next piece, the text's end
// closes a file's last line.  A piece goes through six phases, all of them on the device:
//   scan     a lane owns 16 bytes and counts its '\n'; an exclusive sum numbers the lines and places line_start[]
//   heads    a thread per line walks to the line's 11th tab (the end of field 10) or its end: six numbers, the strand, two
//            name spans, the line's first failing check (parse_line's order, host_ingest.cpp)
//   tag      every field start tests its next five bytes against "cg:Z:" (atomicMin into cg_at[line]); every tab behind
//            cg_at[line] does atomicMin into cg_end[line]
//   names    both spans hashed and looked up in a read-only table of the names known so far (equal hash AND equal bytes);
//            the unknown ones are listed in occurrence order with their bytes and come home, the host gives them ids,
//            patches those records and uploads the rebuilt table
//   cigars   cigar_count_kernel -> exclusive sum -> cigar_tokens_kernel (index_build_device.hip) at the pool's running offset
//   records  appended to the record array in HBM
// The functions below are the per-line and per-name steps as both the kernels and the twin run them.  Every loop in them
// is bounded by the line's end or by the table's capacity, both arguments.
#pragma once
#include <string>
#include <vector>

#include "impg_internal.hpp"
#include "sequence_ingest.hpp"

namespace impg {
namespace paf_ingest {

// the counters of the route, in the order impg_gpu_selftest_paf_ingest reports them
enum Stat { DEVICE, PIECES, TEXT_BYTES, LINES, CARRIED_BYTES, BUFFER_GROWS, POOL_REGROWS, UNKNOWN_NAMES, INFLATED_BLOCKS, N_STATS };
// a line's first failing check (0: none), in parse_line's order
enum LineErr { LINE_OK, LINE_FIELDS, LINE_NUMBER, LINE_NO_STRAND, LINE_STRAND, LINE_CIGAR };
inline const char *line_err_text(uint32_t e) {
  return e == LINE_FIELDS ? "Not enough fields in PAF record" : e == LINE_NUMBER ? "Invalid field" : e == LINE_NO_STRAND ? "Expected '+' or '-' for strand"
         : e == LINE_STRAND ? "Invalid strand" : "Invalid CIGAR operation";
}
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr size_t MAX_BUFFER = (1ull << 32) - 16;  // offsets in a piece are 32 bits
constexpr size_t DEFAULT_PIECE = 64u << 20;

struct Head {  // what the heads phase leaves of a line
  uint64_t len[2];        // the two length fields (query, target)
  uint32_t c[4];          // query start, end, target start, end: the low 32 bits
  uint32_t name_at[2], name_len[2];
  uint32_t strand, err;
  uint32_t end, pad;      // the line's end less its '\r'
};
struct Unknown {  // an occurrence of a name the table did not hold
  uint32_t occ;   // 2 * line + {0: query, 1: target}
  uint32_t len;
  uint64_t at;    // its bytes in the list's byte array
  int64_t seq_len;
};
// The names known so far, as the host builds them and the device reads them: open addressing, a slot holds id + 1
struct Table {
  uint32_t cap = 16;                 // slots, a power of two, more than twice the names
  std::vector<uint32_t> slot;        // [cap]
  std::vector<uint64_t> hash, off;   // [n], [n + 1]: name id's hash, its bytes in pool
  std::string pool;
};
struct TableView { uint32_t cap; const uint32_t *slot; const uint64_t *hash, *off; const char *pool; };

// usize::from_str as to_u64 (host_ingest.cpp) has it: an optional '+', then digits only, at least one; 64-bit wrap
IMPG_HD inline bool number_field(const char *t, uint32_t a, uint32_t b, uint64_t &v) {
  uint32_t i = (a < b && t[a] == '+') ? a + 1u : a;
  if (i >= b) return false;
  uint64_t x = 0;
  for (; i < b; i++) {
    const unsigned d = (unsigned)(unsigned char)t[i] - (unsigned)'0';
    if (d > 9u) return false;
    x = x * 10u + d;
  }
  v = x;
  return true;
}
// the heads phase of the line t[start, raw_end): raw_end is its '\n' (or the text's end)
IMPG_HD inline Head line_head(const char *t, uint32_t start, uint32_t raw_end) {
  Head h{};
  uint32_t end = raw_end;
  if (end > start && t[end - 1u] == '\r') end--;
  h.end = end;
  uint32_t fa[11], fb[11];  // fields 0 .. 10
  uint32_t nf = 0, st = start;
  for (uint32_t i = start; i < end && nf < 11u; i++)
    if (t[i] == '\t') {
      fa[nf] = st;
      fb[nf] = i;
      nf++;
      st = i + 1u;
    }
  if (nf < 11u) { h.err = LINE_FIELDS; return h; }  // fewer than 11 tabs: fewer than 12 fields
  uint64_t v[6];
  const int which[6] = {1, 2, 3, 6, 7, 8};
  bool ok = true;
  for (int k = 0; k < 6; k++) ok = number_field(t, fa[which[k]], fb[which[k]], v[k]) && ok;
  if (!ok) { h.err = LINE_NUMBER; return h; }
  if (fa[4] == fb[4]) { h.err = LINE_NO_STRAND; return h; }
  const char sc = t[fa[4]];
  if (sc != '+' && sc != '-') { h.err = LINE_STRAND; return h; }
  h.len[0] = v[0]; h.len[1] = v[3];
  h.c[0] = (uint32_t)v[1]; h.c[1] = (uint32_t)v[2]; h.c[2] = (uint32_t)v[4]; h.c[3] = (uint32_t)v[5];
  h.name_at[0] = fa[0]; h.name_len[0] = fb[0] - fa[0];
  h.name_at[1] = fa[5]; h.name_len[1] = fb[5] - fa[5];
  h.strand = sc == '-';
  return h;
}
// FNV-1a, cut to hash_bits (a test's way to make names collide)
IMPG_HD inline uint64_t name_hash(const char *p, uint32_t n, unsigned hash_bits) {
  uint64_t h = 0xCBF29CE484222325ull;
  for (uint32_t i = 0; i < n; i++) h = (h ^ (unsigned char)p[i]) * 0x100000001B3ull;
  h ^= h >> 32;
  return hash_bits >= 64u ? h : h & ((1ull << hash_bits) - 1ull);
}
// the id of the name p[0, n), NONE where the table does not hold it
IMPG_HD inline uint32_t table_find(const TableView &T, const char *p, uint32_t n, uint64_t h) {
  for (uint32_t k = 0; k < T.cap; k++) {
    const uint32_t s = T.slot[(uint32_t)(h + k) & (T.cap - 1u)];
    if (!s) return NONE;
    const uint32_t id = s - 1u;
    if (T.hash[id] != h || T.off[id + 1u] - T.off[id] != n) continue;
    const char *q = T.pool + T.off[id];
    bool same = true;
    for (uint32_t i = 0; i < n && same; i++) same = p[i] == q[i];
    if (same) return id;
  }
  return NONE;
}

struct Backend {
  virtual ~Backend() {}
  virtual void begin(size_t buffer_bytes, uint64_t pool_ops, unsigned hash_bits) = 0;
  virtual char *buffer(int which) = 0;
  // both blocks and the device text now hold buffer_bytes; block `which` keeps its first `keep` bytes
  virtual void grow(size_t buffer_bytes, int which, size_t keep) = 0;
  virtual void table(const Table &t) = 0;  // (the rebuilt table replaces the one before)
  // phases scan .. names of the n bytes in block `which`, queued: the driver reads the next piece meanwhile
  virtual void piece_begin(int which, size_t n) = 0;
  virtual void piece_unknowns(uint32_t &n_lines, std::vector<Unknown> &list, std::string &bytes) = 0;
  // the ids of the listed occurrences, then phases cigars and records; returns the piece's first LineErr, its ops in n_ops
  virtual uint32_t piece_end(const std::vector<uint32_t> &occ, const std::vector<uint32_t> &id, uint64_t &n_ops, uint64_t &pool_regrows) = 0;
  virtual void end() = 0;
};

struct Loaded {
  HostSeqIndex seq;
  std::vector<uint64_t> file_first;
  uint64_t n_records = 0, n_ops = 0;
  uint64_t stats[N_STATS] = {};
  double read_seconds = 0, resolve_seconds = 0;
};
// ops to reserve for files of these sizes (plain: text bytes / 3; compressed: 4 x that)
uint64_t initial_pool_ops(const std::vector<std::string> &paths);
// The driver: every file through B, piece by piece.  Throws Error.
void load_files(Backend &B, const std::vector<std::string> &paths, size_t piece_bytes, unsigned hash_bits, uint64_t pool_ops, Loaded &out);

// The host twin of the kernels (CPU tests, the sanitizer program; never a fallback)
struct HostBackend : Backend {
  std::vector<char> buf[2];
  std::vector<impg_gpu_record_t> records;
  std::vector<uint32_t> ops;
  size_t pool_cap = 0;
  unsigned hash_bits = 64;
  Table T;
  const char *cur = nullptr;
  int cur_which = 0;
  size_t cur_n = 0;
  std::vector<uint32_t> line_start, cg_at, cg_end, ids;
  std::vector<Head> heads;
  void begin(size_t buffer_bytes, uint64_t pool_ops, unsigned hb) override;
  char *buffer(int which) override { return buf[which].data(); }
  void grow(size_t buffer_bytes, int which, size_t keep) override;
  void table(const Table &t) override { T = t; }
  void piece_begin(int which, size_t n) override;
  void piece_unknowns(uint32_t &n_lines, std::vector<Unknown> &list, std::string &bytes) override;
  uint32_t piece_end(const std::vector<uint32_t> &occ, const std::vector<uint32_t> &id, uint64_t &n_ops, uint64_t &pool_regrows) override;
  void end() override {}
};

}  // namespace paf_ingest

// index_build_device.hip: the tokenizer's two kernels, launched on s (one wave a span; spans of text + boff[i], blen[i] bytes)
void cigar_count_launch(const char *text, const unsigned long long *boff, const uint32_t *blen, uint32_t n, uint32_t *cnt, uint32_t *bad, hipStream_t s);
void cigar_tokens_launch(const char *text, const unsigned long long *boff, const uint32_t *blen, uint32_t n, const unsigned long long *op_off, uint32_t *ops,
                         hipStream_t s);
// paf_ingest_device.hip: the device leg of impg_gpu_selftest_paf_ingest
void paf_ingest_selftest_device(const std::vector<std::string> &paths, size_t piece_bytes, int device, unsigned hash_bits, uint64_t pool_ops,
                                paf_ingest::Loaded &L, std::vector<impg_gpu_record_t> &records, std::vector<uint32_t> &ops);
// ... and the ingest of impg_gpu_index_create_from_paf_streamed: records home, the op pool left in d_ops
void paf_ingest_device(const std::vector<std::string> &paths, size_t piece_bytes, int device, paf_ingest::Loaded &L,
                       std::vector<impg_gpu_record_t> &records, DevBuf &d_ops);

}  // namespace impg
