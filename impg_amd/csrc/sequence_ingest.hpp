// Sequence files straight into HBM (impg_gpu_index_load_sequences): what the reader, the per-piece state machine and the
// store's layout share between the host side (sequence_ingest.cpp: the reader, the driver, the host twin) and the device
// side (sequence_ingest_device.hip: the kernels and the call itself).  DESIGN.md section 5.5.
//
// A file's text is cut into pieces of option "sequence_ingest_piece_bytes".  A piece goes through two phases:
//   scan    which bytes lie on header lines, how many bases and record heads the piece holds, the header lines' bytes
//           (compacted, '\n' included) and, per head, how many of the piece's bases lie before it.  The driver cuts the
//           names from the header bytes, resolves them and builds the piece's record table;
//   place   every base goes to its place in the store (upper-cased; in the packed form as 2 bits, and the runs of the
//           bytes that are not A/C/G/T come back).
// The carry between two pieces is what only the text tells: whether the next byte starts a line, whether it lies on a
// header line, whether a record is open.  Where the open record's bases go, and how many it has had, the driver knows --
// it assigned the place -- and hands over as entry 0 of the next piece's record table.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "impg_internal.hpp"

namespace impg {

constexpr size_t RUN_BYTES = sizeof(uint2) + 1;  // a run in HBM
// What the packed form of a store holds beside its stream: the places, the runs and the block tables, all on the host
// (fasta_device.hip, PackedStore, says how the kernels read them)
struct PackedPlan {
  typedef unsigned long long u64;
  std::vector<u64> off, run_off, blk_off;  // [n_ids], [n_ids + 1], [n_ids]
  std::vector<uint2> runs;
  std::vector<unsigned char> run_byte;
  std::vector<uint32_t> blk;
  u64 end = 64;  // the stream's bases, the alignment of every sequence included
  explicit PackedPlan(size_t n_ids)
      : off(std::max<size_t>(n_ids, 1), SEQ_NOT_IN_HBM), run_off(n_ids + 1, 0), blk_off(std::max<size_t>(n_ids, 1), 0) {}
  size_t stream_bytes() const { return (size_t)(end / 4u) + 64; }
  size_t bytes() const { return stream_bytes() + runs.size() * RUN_BYTES + blk.size() * 4; }
  // the run tables of sequence `id`, `len` bases long: once per id, in id order (no runs: a sequence without any, or absent)
  void add_runs(size_t id, u64 len, const std::vector<SeqRun> &r) {
    run_off[id + 1] = run_off[id];
    if (r.empty()) return;
    run_off[id + 1] += r.size();
    blk_off[id] = blk.size();
    size_t k = 0;  // first[b] = the runs that end at or before base 1024 * b
    for (u64 b = 0; b <= (len + 1023u) >> 10; b++) {
      while (k < r.size() && (u64)r[k].end <= b << 10) k++;
      blk.push_back((uint32_t)k);
    }
    for (const SeqRun &x : r) {
      runs.push_back(make_uint2(x.start, x.end));
      run_byte.push_back(x.byte);
    }
  }
};

namespace ingest {

constexpr uint64_t NO_PLACE = ~0ull;

struct Carry {  // a file's first piece starts from Carry{0, 1, 0, 0}
  uint32_t in_header;      // the piece's first byte continues a header line
  uint32_t at_line_start;  // ... starts a line
  uint32_t open;           // a record is open
  uint32_t pad;
};
// One record of a piece's table: entry 0 is the record open when the piece starts (dest NO_PLACE where none is), entry j
// the j-th head of the piece.  Base number r of the piece (counted from 0) that lies in the record is base
// r - first_rank + before of its sequence, and is stored only where that is below len.
struct Rec {
  uint64_t dest;        // the sequence's first base in the store (a byte, or a base of the packed stream); NO_PLACE: not stored
  uint64_t before;      // bases the record has had in earlier pieces
  uint32_t first_rank;  // bases of the piece in front of the record
  uint32_t len;         // the index's length of the sequence
};
struct PieceRun { uint32_t rec, start, end; uint8_t byte; };  // a maximal stretch of one byte that is not A/C/G/T within the piece
struct PieceScan {
  uint64_t n_bases = 0, n_heads = 0;
  bool text_before_head = false;  // a base while no record is open
  std::vector<char> header;       // the header lines' bytes
  std::vector<uint32_t> head_rank;  // [n_heads]
};

struct Backend {
  virtual ~Backend() {}
  virtual void begin(size_t piece_bytes, size_t store_bytes, bool packed) = 0;  // the store reserved, all zero
  virtual char *buffer(int which) = 0;                                          // where piece `which` (0 / 1) is read into
  virtual void file_start() = 0;
  virtual void scan_begin(int which, size_t n) = 0;  // (queued: the driver reads the next piece meanwhile)
  virtual void scan_end(PieceScan &out) = 0;
  virtual void place(const Rec *recs, uint32_t n_recs, std::vector<PieceRun> &runs) = 0;  // runs: the packed form's
  virtual void end() = 0;                                                                // everything placed
};

enum Stat { PIECES, TEXT_BYTES, BASES, INFLATED_BLOCKS, DROPPED_SEQUENCES, N_STATS };
struct Loaded {
  bool packed = false;
  std::vector<std::string> names;   // every sequence met, in file order
  std::vector<uint64_t> counts;     // ... and its bases
  std::vector<uint32_t> store_of_id;  // [n_ids] which of them an index id is, SEQ_ABSENT
  std::vector<uint64_t> off;        // [max(n_ids, 1)] byte form: the places
  PackedPlan plan{0};               // packed form: the places and the run tables
  size_t store_bytes = 0;           // of the reservation in use (what fasta_store_bytes reports)
  uint64_t stats[N_STATS] = {};
  double read_seconds = 0;          // spent in the reader (copying, inflating), all files
};
// bytes to reserve for the store of an index with these lengths, whichever of its sequences the files hold
size_t reserve_bytes(const std::vector<int64_t> &lens, bool packed);
// The driver: every file through B, piece by piece.  name_of_id[id] as the index prints it.  Throws Error.
void load_files(Backend &B, const std::vector<std::string> &paths, const std::vector<std::string> &name_of_id, const std::vector<int64_t> &lens,
                size_t piece_bytes, bool packed, Loaded &out);

// A sequence file's text, piece by piece: plain, one gzip stream (or members), or BGZF inflated block by block on a few threads
class FileText {
 public:
  FileText(const std::string &path, uint64_t *inflated_blocks);
  ~FileText();
  FileText(const FileText &) = delete;
  FileText &operator=(const FileText &) = delete;
  size_t next(char *dst, size_t cap);  // the next `cap` bytes of text (fewer: the text ends there; 0: it has ended)
 private:
  struct Z;
  std::string path_;
  const unsigned char *m_ = nullptr;
  size_t sz_ = 0, at_ = 0;
  int kind_ = 0;
  Z *z_ = nullptr;
  std::vector<unsigned char> bounce_;
  size_t b_at_ = 0, b_n_ = 0;
  uint64_t *blocks_;
  size_t next_gzip(char *dst, size_t cap);
  size_t next_bgzf(char *dst, size_t cap);
};

}  // namespace ingest
}  // namespace impg
