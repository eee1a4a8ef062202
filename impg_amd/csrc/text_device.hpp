// What the device text writers share (bed_device.hip: BED rows; bedpe_device.hip: BEDPE lines; each keeps only its line's
// field layout, a length kernel and a write kernel): the name / shift / range-name tables and the printers of a sequence,
// a range name and a decimal (here); the tables' upload and the piece loop that moves finished text across PCIe
// (TextTableBufs, device_text_pieces: text_device.hip); and device_rows_text, which runs a format's two kernels around them.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "device_prims.hpp"
#include "engine.hpp"

namespace impg {

struct TextTables {
  const char *names;            // printed sequence names back to back ("base" under --original-sequence-coordinates)
  const uint32_t *name_off;     // [n_seq + 1]
  const uint32_t *shift;        // [n_seq] offset added to the coordinates (main.rs:11876-11883)
  uint32_t n_names;             // 0: sequences print as their ids
  const char *rnames;           // the chunk's range names back to back
  const uint32_t *rname_off;    // [n_ranges + 1]
  const uint32_t *seq_len;      // [n_lens] the sequence lengths PAF prints (all 0 under --original-sequence-coordinates); null unless asked for
  uint32_t n_lens;              // an id from here on prints the length 0
};
__device__ __forceinline__ uint32_t dec_digits(uint32_t v) {
  uint32_t d = 1;
  while (v >= 10u) { v /= 10u; d++; }
  return d;
}
__device__ __forceinline__ char *put_dec(char *p, uint32_t v, uint32_t digits) {
  for (uint32_t k = digits; k > 0; k--) { p[k - 1] = (char)('0' + v % 10u); v /= 10u; }
  return p + digits;
}
// a sequence as it prints: its name, or its id where the index has no names
__device__ __forceinline__ uint32_t seq_text_len(const TextTables &t, uint32_t id) {
  return id < t.n_names ? t.name_off[id + 1] - t.name_off[id] : dec_digits(id);
}
__device__ __forceinline__ char *put_seq(char *p, const TextTables &t, uint32_t id) {
  if (id >= t.n_names) return put_dec(p, id, dec_digits(id));
  const char *nm = t.names + t.name_off[id];
  const uint32_t nl = t.name_off[id + 1] - t.name_off[id];
  for (uint32_t k = 0; k < nl; k++) p[k] = nm[k];
  return p + nl;
}
__device__ __forceinline__ uint32_t seq_shift(const TextTables &t, uint32_t id) { return id < t.n_names ? t.shift[id] : 0u; }
__device__ __forceinline__ uint32_t seq_len_of(const TextTables &t, uint32_t id) { return id < t.n_lens ? t.seq_len[id] : 0u; }
__device__ __forceinline__ char *put_range_name(char *p, const TextTables &t, uint32_t q) {
  const char *rn = t.rnames + t.rname_off[q];
  const uint32_t rl = t.rname_off[q + 1] - t.rname_off[q];
  for (uint32_t k = 0; k < rl; k++) p[k] = rn[k];
  return p + rl;
}

// A merged row as the query-axis sweep of bed_device.hip leaves it (BED prints it as a line, FASTA as a record), 16 bytes
struct BedRow {
  uint32_t q_strand;  // range index | reverse strand << 31
  uint32_t query_id;
  int32_t start, end;  // (printed as u32, like the reference: an inconsistent CIGAR can project below zero)
};

// The tables of one chunk on the device (uploaded on E.stream; they live as long as this object)
struct TextTableBufs {
  DevBuf d_nb, d_noff, d_shift, d_rb, d_roff, d_len;
  TextTables t{};
  TextTableBufs(Engine &E, const impg_gpu_index &ix, uint32_t n_ranges, const std::vector<std::string> &rnames, bool original_coords,
                bool with_lengths = false);  // with_lengths: PAF's two length columns

 private:
  std::string nb, rb;  // (the sources of the asynchronous uploads)
  std::vector<uint32_t> noff, nshift, roff, lens;
};

// n_rows rows of d_len[r] bytes each as text, streamed to `sink(ptr, bytes)` in pieces of whole rows of at most PIECE
// bytes (option bed_text_piece_bytes) through two pinned buffers: while the host consumes one piece the device formats
// and copies the next.  write(r0, r1, d_off + r0, base, out) enqueues the kernel that writes rows [r0, r1), row r at
// out + (d_off[r] - base).  what: the row's kind, for the refusal of a single row longer than the buffer.
void device_text_pieces(Engine &E, const uint32_t *d_len, uint32_t n_rows, const char *what,
                        const std::function<void(uint32_t, uint32_t, const unsigned long long *, unsigned long long, char *)> &write,
                        const std::function<void(const char *, size_t)> &sink, std::atomic<uint64_t> &pieces, std::atomic<uint64_t> &bytes);

// What device_text_pieces allocates per call, kept by an owner that makes many calls (a partition session: one text per
// window): the tables of the index's names, the two piece buffers with their pinned twins and events, and the per-text
// scratch.  Everything is made at the first text and freed with the owner; `allocs` counts how often the piece buffers
// were allocated or grown, `uploads` how often the tables were uploaded.  The device is current when it dies.
struct TextStream {
  std::unique_ptr<TextTableBufs> tables;
  DevBuf piece[2];
  char *pin[2] = {nullptr, nullptr};
  size_t cap = 0;  // of each of the four buffers
  hipEvent_t done[2] = {nullptr, nullptr};
  DevBuf rows, len, off, bad, stmp;  // a text's records, their lengths and offsets ([n + 1] each), the refusal marks
  uint64_t allocs = 0, uploads = 0;
  TextStream() = default;
  TextStream(const TextStream &) = delete;
  TextStream &operator=(const TextStream &) = delete;
  ~TextStream() { drop(); }
  void reserve(size_t bytes, hipStream_t s);  // room for pieces of `bytes` bytes; grows, never shrinks
  void drop();
};

// A text of `total` bytes whose record r starts at byte h_off[r] (h_off[n_rec] = total; the same offsets lie on the
// device), streamed to `sink` in pieces of exactly PIECE bytes (option bed_text_piece_bytes; the last one shorter),
// cut wherever that falls -- inside a header, on a line break, inside a record that spans many pieces -- through
// the stream's two pinned buffers.  write(r0, r1, base, n_bytes, out) enqueues the kernel that writes bytes
// [base, base + n_bytes) of the text to `out`; records [r0, r1) are the ones that hold them.  No record is refused for
// its length.  S.reserve() has been called with min(PIECE, total) or more.
void device_text_windows(Engine &E, TextStream &S, const unsigned long long *h_off, uint32_t n_rec,
                         const std::function<void(uint32_t, uint32_t, unsigned long long, unsigned long long, char *)> &write,
                         const std::function<void(const char *, size_t)> &sink, std::atomic<uint64_t> &pieces, std::atomic<uint64_t> &bytes);

// n_rows records of type Row (in `rows`, on the device) as text: the chunk's tables, len_kernel for every line's length,
// then write_kernel piece by piece.  pieces / bytes: the format's two text counters.
template <class Row, void (*len_kernel)(const Row *, uint32_t, TextTables, uint32_t *),
          void (*write_kernel)(const Row *, uint32_t, TextTables, const unsigned long long *, unsigned long long, char *)>
void device_rows_text(Engine &E, const impg_gpu_index &ix, const DevBuf &rows, uint32_t n_rows, uint32_t n_ranges,
                      const std::vector<std::string> &rnames, bool original_coords, const std::function<void(const char *, size_t)> &sink,
                      const char *what, std::atomic<uint64_t> &pieces, std::atomic<uint64_t> &bytes) {
  if (!n_rows) return;
  hipStream_t s = E.stream;
  TextTableBufs tb(E, ix, n_ranges, rnames, original_coords);
  const TextTables t = tb.t;
  DevBuf len;
  len.reserve((size_t)n_rows * 4);
  len_kernel<<<prims::cdiv(n_rows, 256), 256, 0, s>>>(rows.as<Row>(), n_rows, t, len.as<uint32_t>());
  device_text_pieces(E, len.as<uint32_t>(), n_rows, what,
                     [&](uint32_t r0, uint32_t r1, const unsigned long long *off, unsigned long long base, char *out) {
                       write_kernel<<<prims::cdiv(r1 - r0, 256), 256, 0, s>>>(rows.as<Row>() + r0, r1 - r0, t, off, base, out);
                     },
                     sink, pieces, bytes);
}

}  // namespace impg
