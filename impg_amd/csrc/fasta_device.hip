// FASTA records on the device (output_results_fasta, main.rs:12351-12415): the merged rows of the query-axis sweep
// (bed_device.hip, strands apart, no gap_2d) printed as ">{name}:{start}-{end}[/rc]\n" and their bases in lines of 80, from a
// sequence store that lives in HBM (one byte per base, or two bits per base).  sequences.cpp holds the host side of the
// same text.
//
//   store     SEQ_PAD zero bytes, the present sequences back to back in id order, padding behind them; off[id] = the place
//             of the sequence's first base, SEQ_NOT_IN_HBM where the store lacks it.  The padding lets the writer's aligned
//             16-byte loads read past either end of a sequence.
//   packed    the same store at a quarter of the size (option "sequence_store_packed", read at attach; PackedStore below):
//             2 bits a base, the bytes that are not A/C/G/T kept as runs beside them, packed on the device chunk by chunk
//             (fasta_pack_kernel, upload_packed).  The kernels below are the same ones: the write kernel is a template on
//             the store's form and differs in where a lane's 16 source bases come from -- 32 bits of the stream turned into
//             letters in registers, the runs' bytes laid over them -- and nowhere else; the text is the same byte for byte.
//   lengths   one thread per record: header + body, body = L + ceil(L / 80) bytes (a single '\n' for L = 0 -- nothing at all
//             under the partition body rule, below); the same thread marks the first record whose sequence the store lacks,
//             or whose row leaves its sequence -- refused before any text is written.
//   text      a record is megabytes of bases, not forty bytes of fields: the write kernel's grid covers the piece's BYTES,
//             each lane 16 consecutive ones, aligned in the piece buffer.  A lane finds its record in the piece's offsets
//             (one search for the wave's first byte and one for its last; a search of its own only when those differ).  A
//             lane whose 16 bytes lie inside one body, short of its last byte, holds at most one line break: the bases
//             before and behind it are one contiguous run of the source, read with two aligned 16-byte loads and shifted
//             into place (read backwards and complemented for "/rc"), the '\n' spliced in, one 16-byte store.  Every other
//             lane -- headers, a record's last bytes, records a few bytes long -- computes its bytes one at a time.
//   partition `impg partition -o fasta` (write_partition_fasta, partition.rs:1630-1680; device_partition_fasta below) prints
//             a window's final intervals from where DeviceRegions::apply leaves them: one kernel makes them the writer's
//             records, the length kernel takes the partition body rule -- a record of no bases is its header alone -- and
//             the write kernel its byte-window form: the piece is bytes [base, base + n_bytes) of the text wherever that
//             falls, its first record may begin before it and its last may end behind it, and every record's length is
//             its own (off[r + 1] - off[r], the last record's included), never the piece's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <functional>
#include <string>

#include "device_prims.hpp"
#include "engine.hpp"
#include "partition.hpp"
#include "sequence_ingest.hpp"
#include "text_device.hpp"

namespace impg {

namespace {

using prims::cdiv;
typedef unsigned long long u64;
typedef unsigned __int128 u128;

struct FastaStore {
  const unsigned char *bases;  // 16-byte aligned
  const u64 *off;              // [n_ids]
  const uint32_t *len;         // [n_ids] the index's sequence lengths
  uint32_t n_ids;
  static constexpr bool packed = false;
};
// The packed form (option "sequence_store_packed"): 2 bits a base, A C G T = 0 1 2 3, base i of the stream in bits
// 2 * (i & 15) and up of word i >> 4 (bits 2 * (i & 3) of byte i >> 2).  64 zero bases in front, every present sequence
// from a multiple of 64 bases on, 64 zero bytes or more behind the last; off[id] counts BASES.  A byte that is not A/C/G/T
// packs as 0 and is kept in a run: a maximal stretch of one such byte, (start, end) in its sequence, the runs sorted, a CSR
// offset per id.  A sequence that has runs also has a table over its blocks of 1 024 bases, first[b] = its runs that end at
// or before base 1 024 * b: the runs that can touch bases [a, b) are first[a / 1024] .. first[(b - 1) / 1024 + 1] inclusive,
// one candidate where no run lies near, none to look at where the sequence has no runs.
struct PackedStore {
  const uint32_t *words;  // 16-byte aligned
  const u64 *off;         // [n_ids] the sequence's first base in the stream
  const uint32_t *len;
  uint32_t n_ids;
  const u64 *run_off;             // [n_ids + 1]
  const uint2 *runs;              // (start, end) in the sequence
  const unsigned char *run_byte;  // what the run's bases print as
  const u64 *blk_off;             // [n_ids] where the block table of a sequence with runs starts in blk
  const uint32_t *blk;            // first[0 .. ceil(len / 1024)] per such sequence
  static constexpr bool packed = true;
};
constexpr uint32_t ACGT = 0x54474341u;      // code c prints as byte c of it
constexpr uint32_t FASTA_OK = 0xFFFFFFFFu;  // no record to refuse

__device__ __forceinline__ uint32_t fasta_header_len(const TextTables &t, const BedRow &x, bool flip) {
  return 1u + seq_text_len(t, x.query_id) + 1u + dec_digits((uint32_t)x.start) + 1u + dec_digits((uint32_t)x.end) + (flip ? 3u : 0u) + 1u;
}
// PART: the partition body rule (chunks(80) of nothing prints nothing); else output_results_fasta's empty line
template <bool PART> __device__ __forceinline__ uint32_t fasta_body_len(uint32_t L) { return L ? L + (L + 79u) / 80u : PART ? 0u : 1u; }

// bad[0] / bad[1]: the first record on a sequence the store lacks / that leaves its sequence
template <bool PART>
__global__ __launch_bounds__(256) void fasta_len_kernel(const BedRow *__restrict__ rows, uint32_t n, TextTables t, FastaStore st, int reverse_complement,
                                                        uint32_t *__restrict__ len, uint32_t *__restrict__ bad) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const BedRow x = rows[r];
  const bool present = x.query_id < st.n_ids && st.off[x.query_id] != SEQ_NOT_IN_HBM;
  if (!present) atomicMin(&bad[0], r);
  else if (x.start < 0 || x.end < x.start || (uint32_t)x.end > st.len[x.query_id]) atomicMin(&bad[1], r);
  const bool flip = reverse_complement && (x.q_strand >> 31);
  const uint32_t L = x.end >= x.start ? (uint32_t)(x.end - x.start) : 0u;
  len[r] = fasta_header_len(t, x, flip) + fasta_body_len<PART>(L);
}
// a window's final intervals (DeviceRegions::out_rows) as the writer's records: forward, no range
__global__ __launch_bounds__(256) void fasta_piv_rows_kernel(const PIv *__restrict__ in, uint32_t n, BedRow *__restrict__ rows) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const PIv x = in[r];
  rows[r] = BedRow{0u, x.seq, x.lo, x.hi};
}

// digit `pos` (0 = the leading one) of v, which prints with `digits` digits
__device__ __forceinline__ char dec_char(uint32_t v, uint32_t digits, uint32_t pos) {
  for (uint32_t k = digits - 1u - pos; k > 0; k--) v /= 10u;
  return (char)('0' + v % 10u);
}
__device__ __forceinline__ unsigned char base_complement(unsigned char c) {  // graph.rs:814-828
  return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}
// ---- the packed store's readers
// The runs of sequence `id` that can touch its bases [a, b), 0 <= a < b <= its length: [lo, hi) of st.runs, every run
// before lo ends at or before a.  Two words for a sequence without runs; two more and the table's two where it has some,
// and a search only where more than one run remains.
__device__ __forceinline__ void runs_near(const PackedStore &st, uint32_t id, uint32_t a, uint32_t b, u64 &lo, u64 &hi) {
  const u64 r0 = st.run_off[id], r1 = st.run_off[id + 1];
  lo = hi = r0;
  if (r0 == r1) return;
  const uint32_t *first = st.blk + st.blk_off[id];
  lo = r0 + first[a >> 10];
  hi = min(r0 + first[((b - 1u) >> 10) + 1u] + 1u, r1);  // (the run behind that one starts in a later block)
  u64 top = hi;
  while (top - lo > 1u) {  // the first run that ends behind a; `hi - 1` if none does
    const u64 mid = lo + (top - lo) / 2u;
    if (st.runs[mid - 1u].y > a) top = mid; else lo = mid;
  }
}
// the 16 bases from place P of the stream on: 32 bits from two aligned words (the padding covers a read beyond a sequence)
__device__ __forceinline__ uint32_t load_codes16(const uint32_t *__restrict__ words, u64 P) {
  const u64 w = P >> 4;
  const u64 v = ((u64)words[w + 1u] << 32) | words[w];
  return (uint32_t)(v >> ((unsigned)(P & 15ull) * 2u));
}
__device__ __forceinline__ u64 expand8(uint32_t c) {  // eight codes in the low 16 bits -> their letters
  u64 r = 0;
#pragma unroll
  for (unsigned i = 0; i < 8u; i++) r |= (u64)((ACGT >> (8u * ((c >> (2u * i)) & 3u))) & 0xFFu) << (8u * i);
  return r;
}
// S holds 16 bases of sequence `id`, byte i base wa + i of it (forward) or base wb - 1 - i (turned round), wb = wa + 16; a
// byte outside the sequence is one the caller drops.  The bytes under a run become the run's byte -- the same on either
// strand: the complement leaves every byte that is not A/C/G/T as it is.
__device__ __forceinline__ u128 overlay_runs(const PackedStore &st, uint32_t id, u128 S, long long wa, bool turned) {
  const long long wb = wa + 16;
  const uint32_t ca = (uint32_t)max(wa, 0ll), cb = (uint32_t)min(wb, (long long)st.len[id]);
  u64 k, hi;
  runs_near(st, id, ca, cb, k, hi);
  for (; k < hi; k++) {
    const uint2 run = st.runs[k];
    if (run.x >= cb) break;
    const uint32_t s = max(run.x, ca), e = min(run.y, cb);
    if (s >= e) continue;
    const unsigned i0 = (unsigned)(turned ? wb - (long long)e : (long long)s - wa), n = e - s;
    const u64 fill = 0x0101010101010101ull * st.run_byte[k];
    const u128 m = (n < 16u ? ((u128)1 << (8u * n)) - 1u : ~(u128)0) << (8u * i0);
    S = (S & ~m) | ((((u128)fill << 64) | fill) & m);
  }
  return S;
}
// base `pos` of sequence `id`, one at a time (the slow path)
__device__ __forceinline__ unsigned char store_base(const PackedStore &st, uint32_t id, uint32_t pos) {
  const u64 P = st.off[id] + pos;
  u64 k, hi;
  runs_near(st, id, pos, pos + 1u, k, hi);
  if (k < hi) {
    const uint2 run = st.runs[k];
    if (run.x <= pos && pos < run.y) return st.run_byte[k];
  }
  return (unsigned char)(ACGT >> (8u * ((st.words[P >> 4] >> ((unsigned)(P & 15ull) * 2u)) & 3u)));
}

// byte x of a record rec_len bytes long: its header, then its body (a record without a body -- no bases under the partition
// body rule -- has rec_len == hl and is never asked for one)
template <class Store>
__device__ unsigned char fasta_byte(const TextTables &t, const Store &st, const BedRow &row, bool flip, uint32_t hl, u64 rec_len, u64 x) {
  if (x >= hl) {
    const u64 j = x - hl;
    if (j + 1 == rec_len - hl || j % 81u == 80u) return '\n';
    const u64 idx = j - j / 81u;
    if constexpr (Store::packed) {
      const unsigned char c = store_base(st, row.query_id, (uint32_t)(flip ? (u64)row.end - 1u - idx : (u64)row.start + idx));
      return flip ? base_complement(c) : c;
    } else {
      const u64 so = st.off[row.query_id];
      const unsigned char c = st.bases[flip ? so + (u64)row.end - 1u - idx : so + (u64)row.start + idx];
      return flip ? base_complement(c) : c;
    }
  }
  uint32_t h = (uint32_t)x;
  if (h == 0) return '>';
  h -= 1u;
  const uint32_t nl = seq_text_len(t, row.query_id);
  if (h < nl) return row.query_id < t.n_names ? (unsigned char)t.names[t.name_off[row.query_id] + h] : (unsigned char)dec_char(row.query_id, nl, h);
  h -= nl;
  if (h == 0) return ':';
  h -= 1u;
  const uint32_t d1 = dec_digits((uint32_t)row.start), d2 = dec_digits((uint32_t)row.end);
  if (h < d1) return (unsigned char)dec_char((uint32_t)row.start, d1, h);
  h -= d1;
  if (h == 0) return '-';
  h -= 1u;
  if (h < d2) return (unsigned char)dec_char((uint32_t)row.end, d2, h);
  h -= d2;
  if (flip && h < 3u) return h == 0 ? '/' : h == 1 ? 'r' : 'c';
  return '\n';
}
// the record that holds byte g (absolute): the last r in [lo, hi) with off[r] <= g; off[lo] <= g
__device__ __forceinline__ uint32_t fasta_find(const u64 *__restrict__ off, uint32_t lo, uint32_t hi, u64 g) {
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ u128 load16(const unsigned char *p) {  // p 16-byte aligned
  const uint4 v = *reinterpret_cast<const uint4 *>(p);
  return ((u128)(((u64)v.w << 32) | v.z) << 64) | (((u64)v.y << 32) | v.x);
}
// the 16 bytes at p, of any alignment: two aligned loads (the store's padding covers what they read beyond a sequence)
__device__ __forceinline__ u128 load16_any(const unsigned char *base, u64 at) {
  const u64 a0 = at & ~15ull;
  const unsigned sh = (unsigned)(at & 15ull) * 8u;
  const u128 lo = load16(base + a0), hi = load16(base + a0 + 16u);
  return sh ? (lo >> sh) | (hi << (128u - sh)) : lo;
}

// records [0, n_rec) of a piece: record r at out + (off[r] - base), the piece n_bytes long.  One lane per 16 bytes.
// Store: FastaStore or PackedStore -- the two differ in where a lane's 16 source bases come from, and in fasta_byte's.
// WINDOW: the byte-window form.  The piece is bytes [base, base + n_bytes) of a longer text: off[0] <= base (record 0 may
// begin before the piece, off[r] - base wraps round and every use of it below is modular), off[n_rec] >= base + n_bytes is
// there to be read, and a record's length is off[r + 1] - off[r] even where it runs on behind the piece.
template <class Store, bool WINDOW>
__global__ __launch_bounds__(256) void fasta_write_kernel(const BedRow *__restrict__ rows, uint32_t n_rec, TextTables t, Store st,
                                                          int reverse_complement, const u64 *__restrict__ off, u64 base, u64 n_bytes,
                                                          char *__restrict__ out) {
  const u64 lane = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 p = lane * 16u;
  // the wave's first and last byte: if one record holds both, it holds every lane's
  const u64 w0 = (lane & ~63ull) * 16u;
  if (w0 >= n_bytes) return;
  const u64 w1 = min(w0 + 64u * 16u, n_bytes) - 1u;
  const uint32_t rf = fasta_find(off, 0u, n_rec, base + w0);
  const uint32_t rl = fasta_find(off, rf, n_rec, base + w1);
  if (p >= n_bytes) return;
  uint32_t r = rf == rl ? rf : fasta_find(off, rf, rl + 1u, base + p);
  BedRow row = rows[r];
  bool flip = reverse_complement && (row.q_strand >> 31);
  uint32_t hl = fasta_header_len(t, row, flip);
  u64 rec_at = off[r] - base;                                              // the record's first byte in the piece
  u64 rec_len = (WINDOW || r + 1u < n_rec ? off[r + 1u] - base : n_bytes) - rec_at;
  const u64 x0 = p - rec_at;
  // (WINDOW: the record may go on behind the piece, the buffer does not)
  if (x0 >= hl && x0 + 16u < rec_len && (!WINDOW || p + 16u <= n_bytes)) {
    // 16 bytes of one body, its last byte not among them: at most one line break, at k (16: none)
    const u64 j0 = x0 - hl;
    const u64 line0 = j0 / 81u;
    const unsigned col0 = (unsigned)(j0 - line0 * 81u);
    const unsigned k = 80u - col0 < 16u ? 80u - col0 : 16u;
    const u64 s0 = j0 - line0;  // the base index of byte 0 (of byte 1 where byte 0 is the break)
    const u64 so = st.off[row.query_id];
    u128 S;
    if constexpr (Store::packed) {
      // 32 bits of the stream: the 16 bases from `start + s0` on, or the 16 that end at `end - 1 - s0` with their fields
      // turned round and every code ^ 3; their letters; then the runs' bytes over them, before the break goes in
      uint32_t c;
      long long wa;
      if (!flip) {
        wa = (long long)row.start + (long long)s0;
        c = load_codes16(st.words, so + (u64)wa);
      } else {
        wa = (long long)row.end - 1 - (long long)s0 - 15;
        c = __builtin_bitreverse32(load_codes16(st.words, so + (u64)row.end - 1u - s0 - 15u));
        c = ~(((c >> 1) & 0x55555555u) | ((c & 0x55555555u) << 1));
      }
      S = overlay_runs(st, row.query_id, ((u128)expand8(c >> 16) << 64) | expand8(c), wa, flip);
    } else if (!flip) S = load16_any(st.bases, so + (u64)row.start + s0);
    else {
      // bytes hi, hi - 1, ...: read the 16 bytes that end at hi, turn them round, complement each
      const u128 F = load16_any(st.bases, so + (u64)row.end - 1u - s0 - 15u);
      const u64 f_lo = (u64)F, f_hi = (u64)(F >> 64);
      u64 r_lo = __builtin_bswap64(f_hi), r_hi = __builtin_bswap64(f_lo);
      u64 c_lo = 0, c_hi = 0;
#pragma unroll
      for (unsigned i = 0; i < 8u; i++) {
        c_lo |= (u64)base_complement((unsigned char)(r_lo >> (8u * i))) << (8u * i);
        c_hi |= (u64)base_complement((unsigned char)(r_hi >> (8u * i))) << (8u * i);
      }
      S = ((u128)c_hi << 64) | c_lo;
    }
    if (k < 16u) {
      const unsigned kb = k * 8u;
      const u128 below = kb ? S & (((u128)1 << kb) - 1u) : (u128)0;
      const u128 above = k < 15u ? (S >> kb) << (kb + 8u) : (u128)0;
      S = below | ((u128)'\n' << kb) | above;
    }
    const u64 s_lo = (u64)S, s_hi = (u64)(S >> 64);
    *reinterpret_cast<uint4 *>(out + p) = make_uint4((uint32_t)s_lo, (uint32_t)(s_lo >> 32), (uint32_t)s_hi, (uint32_t)(s_hi >> 32));
    return;
  }
  // headers, a record's last bytes, several records in one lane: byte by byte
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  const unsigned n_own = (unsigned)min((u64)16u, n_bytes - p);
#pragma unroll
  for (unsigned i = 0; i < 16u; i++) {
    if (i < n_own) {
      const u64 g = p + i;
      while (g >= rec_at + rec_len) {  // (a record is never empty: its header alone is 6 bytes)
        r++;
        row = rows[r];
        flip = reverse_complement && (row.q_strand >> 31);
        hl = fasta_header_len(t, row, flip);
        rec_at += rec_len;
        rec_len = (WINDOW || r + 1u < n_rec ? off[r + 1u] - base : n_bytes) - rec_at;
      }
      w[i >> 2] |= (uint32_t)fasta_byte(t, st, row, flip, hl, rec_len, g - rec_at) << (8u * (i & 3u));
    }
  }
  if (n_own == 16u) *reinterpret_cast<uint4 *>(out + p) = make_uint4(w[0], w[1], w[2], w[3]);
  else {
    // the piece's last lane: the buffer is not promised to reach 16 bytes beyond the text
#pragma unroll
    for (unsigned i = 0; i < 16u; i++)
      if (i < n_own) out[p + i] = (char)(w[i >> 2] >> (8u * (i & 3u)));
  }
}

// A staged chunk of the byte stream into the packed one: a lane reads 16 bytes and writes their 32 bits, word `lane` of out.
// Every byte that is not A/C/G/T (a run's, the zero bytes between two sequences) packs as 0.
__global__ __launch_bounds__(256) void fasta_pack_kernel(const uint4 *__restrict__ stage, u64 n_words, uint32_t *__restrict__ out) {
  const u64 lane = (u64)blockIdx.x * 256u + threadIdx.x;
  if (lane >= n_words) return;
  const uint4 v = stage[lane];
  const uint32_t in[4] = {v.x, v.y, v.z, v.w};
  uint32_t w = 0;
#pragma unroll
  for (unsigned i = 0; i < 16u; i++) {
    const uint32_t c = (in[i >> 2] >> (8u * (i & 3u))) & 0xFFu;
    w |= (c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 0u) << (2u * i);
  }
  out[lane] = w;
}

// IMPG_FASTA_PIECE_TIMING=<file> (a probe's switch, read on every call): every piece's write kernel between two events, and
// a second copy of the same piece into a pinned buffer of the probe's own between two more, so that the kernel can be held
// against the copy it is meant to hide behind.  "bytes kernel_ms copy_ms" per piece is appended to the file.
struct PieceTiming {
  const char *path = getenv("IMPG_FASTA_PIECE_TIMING");
  std::vector<hipEvent_t> ev;  // four per piece
  std::vector<u64> bytes;
  char *pin = nullptr;
  size_t pin_cap = 0;
  bool on() const { return path && *path; }
  hipEvent_t mark(hipStream_t s) {
    hipEvent_t e;
    IMPG_HIP(hipEventCreate(&e));
    ev.push_back(e);
    IMPG_HIP(hipEventRecord(e, s));
    return e;
  }
  void copy(const char *src, u64 n, hipStream_t s) {
    if (n > pin_cap) {
      if (pin) { IMPG_HIP(hipStreamSynchronize(s)); (void)hipHostFree(pin); pin = nullptr; }
      IMPG_HIP(hipHostMalloc((void **)&pin, (size_t)n, hipHostMallocDefault));
      pin_cap = (size_t)n;
    }
    mark(s);
    IMPG_HIP(hipMemcpyAsync(pin, src, (size_t)n, hipMemcpyDeviceToHost, s));
    mark(s);
    bytes.push_back(n);
  }
  void report() {  // (the stream is idle)
    FILE *f = fopen(path, "a");
    for (size_t k = 0; f && k < bytes.size(); k++) {
      float kernel_ms = 0, copy_ms = 0;
      if (hipEventElapsedTime(&kernel_ms, ev[4 * k], ev[4 * k + 1]) != hipSuccess || hipEventElapsedTime(&copy_ms, ev[4 * k + 2], ev[4 * k + 3]) != hipSuccess) break;
      fprintf(f, "%llu %.6f %.6f\n", bytes[k], (double)kernel_ms, (double)copy_ms);
    }
    if (f) fclose(f);
  }
  ~PieceTiming() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    if (pin) (void)hipHostFree(pin);
  }
};

}  // namespace

namespace {

constexpr u64 PACK_CHUNK_BASES = 64ull << 20;  // IMPG_SEQ_PACK_CHUNK=<bases> sets another (tests: a chunk's end inside a sequence)
// What the packed form of the attached store would hold (PackedPlan, sequence_ingest.hpp: the places, the runs and the block
// tables, all on the host; impg_gpu_index_load_sequences builds the same tables from the runs its kernels extract)
PackedPlan plan_packed(const impg_gpu_index &ix) {
  const SeqStore &st = *ix.seq_store;
  const size_t n_ids = ix.store_of_id.size();
  PackedPlan p(n_ids);
  std::vector<SeqRun> runs;
  for (size_t id = 0; id < n_ids; id++) {
    runs.clear();
    const uint32_t s = ix.store_of_id[id];
    if (s == SEQ_ABSENT) { p.add_runs(id, 0, runs); continue; }
    const u64 len = st.off[s + 1] - st.off[s];  // (the index's length: below 2^31)
    p.off[id] = p.end;
    p.end += (len + 63u) & ~63ull;
    seq_exception_runs(st.bases.data() + st.off[s], (size_t)len, runs);
    p.add_runs(id, len, runs);
  }
  return p;
}

void upload(DevBuf &d, const void *src, size_t bytes) {  // (never an empty buffer: a kernel argument points into it)
  d.reserve(std::max<size_t>(bytes, 16));
  if (bytes) IMPG_HIP(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
}

// The packed stream is made on the device chunk by chunk: the host lays a window of the stream out one byte per base in a
// pinned block -- the sequences at their places, zero bytes between them --, the block goes to a staging buffer in HBM and
// fasta_pack_kernel packs it into place.  A window starts and ends at a multiple of 64 bases of the stream, and so of every
// sequence.  Peak HBM during attach: the packed stream, the run tables and this ONE staging chunk -- never the store at a
// byte per base.
void upload_packed(impg_gpu_index &ix, const PackedPlan &p) {
  const SeqStore &st = *ix.seq_store;
  const size_t n_ids = ix.store_of_id.size();
  const char *env = getenv("IMPG_SEQ_PACK_CHUNK");
  const u64 asked = env ? strtoull(env, nullptr, 10) : 0ull;
  const u64 chunk = std::max<u64>(((asked ? asked : PACK_CHUNK_BASES) + 63u) & ~63ull, 64);
  ix.d_seq_bases.reserve(p.stream_bytes());
  IMPG_HIP(hipMemset(ix.d_seq_bases.p, 0, p.stream_bytes()));
  upload(ix.d_seq_off, p.off.data(), p.off.size() * 8);
  upload(ix.d_seq_run_off, p.run_off.data(), p.run_off.size() * 8);
  upload(ix.d_seq_blk_off, p.blk_off.data(), p.blk_off.size() * 8);
  upload(ix.d_seq_runs, p.runs.data(), p.runs.size() * sizeof(uint2));
  upload(ix.d_seq_run_byte, p.run_byte.data(), p.run_byte.size());
  upload(ix.d_seq_blk, p.blk.data(), p.blk.size() * 4);
  const u64 stage_bytes = std::min<u64>(chunk, p.end - 64u);
  if (stage_bytes) {
    DevBuf d_stage;
    d_stage.reserve((size_t)stage_bytes);
    size_t pin_cap = 0;
    char *pin = (char *)pinned_take((size_t)stage_bytes, pin_cap);
    try {
      size_t id = 0;  // the first sequence that reaches into the window
      for (u64 b0 = 64; b0 < p.end; b0 += chunk) {
        const u64 b1 = std::min<u64>(b0 + chunk, p.end);
        u64 cur = b0;
        for (size_t j = id; j < n_ids; j++) {
          const uint32_t s = ix.store_of_id[j];
          if (s == SEQ_ABSENT) continue;
          if (p.off[j] >= b1) break;
          const u64 a = std::max<u64>(p.off[j], b0), b = std::min<u64>(p.off[j] + (st.off[s + 1] - st.off[s]), b1);
          if (a < b) {
            memset(pin + (cur - b0), 0, (size_t)(a - cur));
            memcpy(pin + (a - b0), st.bases.data() + st.off[s] + (a - p.off[j]), (size_t)(b - a));
            cur = b;
          }
          if (p.off[j] + (st.off[s + 1] - st.off[s]) <= b1) id = j + 1;
        }
        memset(pin + (cur - b0), 0, (size_t)(b1 - cur));
        IMPG_HIP(hipMemcpy(d_stage.p, pin, (size_t)(b1 - b0), hipMemcpyHostToDevice));
        const u64 n_words = (b1 - b0) / 16u;
        fasta_pack_kernel<<<cdiv(n_words, 256), 256>>>(d_stage.as<uint4>(), n_words, ix.d_seq_bases.as<uint32_t>() + b0 / 16u);
        IMPG_HIP(hipGetLastError());
        IMPG_HIP(hipDeviceSynchronize());  // (the next window overwrites the pinned block and the staging buffer)
      }
    } catch (...) {
      pinned_give(pin, pin_cap);
      throw;
    }
    pinned_give(pin, pin_cap);
  }
  ix.seq_packed = true;
  ix.fasta_stats[FASTA_STORE_BYTES] = p.bytes();
  ix.fasta_stats[FASTA_STORE_PACKED] = 1;
  ix.fasta_stats[FASTA_STORE_EXCEPTION_RUNS] = p.runs.size();
}

}  // namespace

// The store's bases in HBM, in the handle's id order (impg_gpu_index_set_sequences; the device is current), in the form
// option "sequence_store_packed" asks for: 0 a byte per base, 1 packed, 2 whichever takes fewer bytes -- decided on the
// host, from the runs, before anything is uploaded
void upload_sequences(impg_gpu_index &ix) {
  const SeqStore &st = *ix.seq_store;
  ix.seq_packed = false;
  ix.fasta_stats[FASTA_STORE_PACKED] = 0;
  ix.fasta_stats[FASTA_STORE_EXCEPTION_RUNS] = 0;
  if (ix.opt.sequence_store_packed) {
    const PackedPlan p = plan_packed(ix);
    u64 as_bytes = SEQ_PAD;
    for (const uint32_t s : ix.store_of_id)
      if (s != SEQ_ABSENT) as_bytes += st.off[s + 1] - st.off[s];
    if (ix.opt.sequence_store_packed == 1 || p.bytes() < (size_t)((as_bytes + 15u) & ~15ull) + 64) return upload_packed(ix, p);
  }
  for (DevBuf *d : {&ix.d_seq_run_off, &ix.d_seq_runs, &ix.d_seq_run_byte, &ix.d_seq_blk_off, &ix.d_seq_blk}) d->release();
  const size_t n_ids = ix.store_of_id.size();
  std::vector<u64> off(std::max<size_t>(n_ids, 1), SEQ_NOT_IN_HBM);
  u64 at = SEQ_PAD;
  for (size_t id = 0; id < n_ids; id++) {
    const uint32_t s = ix.store_of_id[id];
    if (s == SEQ_ABSENT) continue;
    off[id] = at;
    at += st.off[s + 1] - st.off[s];
  }
  const size_t bytes = (size_t)((at + 15u) & ~15ull) + 64;  // (an aligned load that starts at the last base reads 32 bytes from there)
  ix.d_seq_bases.reserve(bytes);
  ix.d_seq_off.reserve(off.size() * 8);
  IMPG_HIP(hipMemset(ix.d_seq_bases.p, 0, bytes));
  for (size_t id = 0; id < n_ids; id++) {
    const uint32_t s = ix.store_of_id[id];
    if (s == SEQ_ABSENT || st.off[s + 1] == st.off[s]) continue;
    IMPG_HIP(hipMemcpy(ix.d_seq_bases.as<char>() + off[id], st.bases.data() + st.off[s], (size_t)(st.off[s + 1] - st.off[s]), hipMemcpyHostToDevice));
  }
  IMPG_HIP(hipMemcpy(ix.d_seq_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice));
  ix.fasta_stats[FASTA_STORE_BYTES] = bytes;
}

namespace {

// the store as the kernels take it, in both forms (the length kernel asks for presence and bounds only: one for both)
struct StoreViews {
  FastaStore st;
  PackedStore pst;
  StoreViews(const impg_gpu_index &ix, const TextTables &t)
      : st{ix.d_seq_bases.as<unsigned char>(), ix.d_seq_off.as<u64>(), t.seq_len, std::min<uint32_t>((uint32_t)ix.store_of_id.size(), t.n_lens)},
        pst{ix.d_seq_bases.as<uint32_t>(), st.off, st.len, st.n_ids, ix.d_seq_run_off.as<u64>(), ix.d_seq_runs.as<uint2>(),
            ix.d_seq_run_byte.as<unsigned char>(), ix.d_seq_blk_off.as<u64>(), ix.d_seq_blk.as<uint32_t>()} {}
};
// what fasta_len_kernel marked: the first record on a sequence the store lacks, else the first that leaves its sequence
void refuse_marked(const impg_gpu_index &ix, const BedRow *rows, const uint32_t *h_bad) {
  if (h_bad[0] == FASTA_OK && h_bad[1] == FASTA_OK) return;
  const bool lacks = h_bad[0] != FASTA_OK;
  BedRow x;
  IMPG_HIP(hipMemcpy(&x, rows + h_bad[lacks ? 0 : 1], sizeof x, hipMemcpyDeviceToHost));
  const std::string name = x.query_id < ix.seq.names.size() ? ix.seq.names[x.query_id] : std::to_string(x.query_id);
  if (lacks) throw Error{IMPG_E_INVALID, "Sequence '" + name + "' not found in the sequence store"};
  throw Error{IMPG_E_INVALID, "row " + name + ":" + std::to_string(x.start) + "-" + std::to_string(x.end) + " leaves its sequence of " +
                                  std::to_string(x.query_id < ix.seq.lens.size() ? ix.seq.lens[x.query_id] : 0) + " bases"};
}
// one piece's write kernel, of the form the attached store has; under the probe's switch between two events, with the
// second copy behind it
template <bool WINDOW>
void write_piece(const impg_gpu_index &ix, const StoreViews &v, const TextTables &t, PieceTiming &timing, const BedRow *rows, uint32_t n_rec, int rc,
                 const u64 *off, u64 base, u64 n_bytes, char *out, hipStream_t s) {
  if (timing.on()) timing.mark(s);
  if (ix.seq_packed) fasta_write_kernel<PackedStore, WINDOW><<<cdiv(n_bytes, 16u * 256u), 256, 0, s>>>(rows, n_rec, t, v.pst, rc, off, base, n_bytes, out);
  else fasta_write_kernel<FastaStore, WINDOW><<<cdiv(n_bytes, 16u * 256u), 256, 0, s>>>(rows, n_rec, t, v.st, rc, off, base, n_bytes, out);
  IMPG_HIP(hipGetLastError());
  if (timing.on()) {
    timing.mark(s);
    timing.copy(out, n_bytes, s);
  }
}

}  // namespace

void device_fasta_text(Engine &E, const impg_gpu_index &ix, const DevBuf &rows, uint32_t n_rows, bool reverse_complement,
                       const std::function<void(const char *, size_t)> &sink) {
  if (!ix.seq_store) throw Error{IMPG_E_INVALID, "FASTA output needs a sequence store (impg_gpu_index_set_sequences)"};
  if (!n_rows) return;
  hipStream_t s = E.stream;
  // (no range names, and the names as the index has them: --original-sequence-coordinates does not touch FASTA)
  TextTableBufs tb(E, ix, 0, std::vector<std::string>(), false, /*with_lengths=*/true);
  const TextTables t = tb.t;
  const StoreViews v(ix, t);
  const int rc = reverse_complement ? 1 : 0;
  DevBuf len, bad;
  len.reserve((size_t)n_rows * 4);
  bad.reserve(256);
  IMPG_HIP(hipMemsetAsync(bad.p, 0xFF, 8, s));
  fasta_len_kernel<false><<<cdiv(n_rows, 256), 256, 0, s>>>(rows.as<BedRow>(), n_rows, t, v.st, rc, len.as<uint32_t>(), bad.as<uint32_t>());
  uint32_t h_bad[2];
  std::vector<uint32_t> h_len(n_rows);
  IMPG_HIP(hipMemcpyAsync(h_bad, bad.p, 8, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipMemcpyAsync(h_len.data(), len.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipStreamSynchronize(s));
  refuse_marked(ix, rows.as<BedRow>(), h_bad);
  // the pieces' sizes, which the byte-centric grid needs: the records' offsets on the host
  std::vector<u64> h_off((size_t)n_rows + 1, 0);
  for (uint32_t r = 0; r < n_rows; r++) h_off[r + 1] = h_off[r] + h_len[r];
  PieceTiming timing;
  device_text_pieces(E, len.as<uint32_t>(), n_rows, "FASTA",
                     [&](uint32_t r0, uint32_t r1, const unsigned long long *off, unsigned long long base, char *out) {
                       write_piece<false>(ix, v, t, timing, rows.as<BedRow>() + r0, r1 - r0, rc, off, base, h_off[r1] - h_off[r0], out, s);
                     },
                     sink, ix.fasta_stats[FASTA_TEXT_PIECES], ix.fasta_stats[FASTA_TEXT_BYTES]);
  if (timing.on()) timing.report();
}

// `impg partition -o fasta`: the records of one window's final intervals, n of them at d_rows in HBM (forward, printed in
// the order they lie in), under the partition body rule, cut into byte-window pieces.  S outlives the call: its tables
// are uploaded and its buffers made at the first text, `hint` bytes large (and at most a piece) so that a later, longer
// text finds them large enough.  Refusals as device_fasta_text's, raised before the sink sees a byte.
void device_partition_fasta(Engine &E, const impg_gpu_index &ix, TextStream &S, const PIv *d_rows, uint32_t n, unsigned long long hint,
                            const std::function<void(const char *, size_t)> &sink) {
  if (!ix.seq_store) throw Error{IMPG_E_INVALID, "FASTA output needs a sequence store (impg_gpu_index_set_sequences)"};
  if (!n) return;
  hipStream_t s = E.stream;
  if (!S.tables) {
    S.tables = std::make_unique<TextTableBufs>(E, ix, 0, std::vector<std::string>(), false, /*with_lengths=*/true);
    S.uploads++;
  }
  const TextTables t = S.tables->t;
  const StoreViews v(ix, t);
  prims::grow(S.rows, (size_t)n * sizeof(BedRow));
  prims::grow(S.len, ((size_t)n + 1) * 4);
  prims::grow(S.off, ((size_t)n + 1) * 8);
  prims::grow(S.bad, 256);
  BedRow *rows = S.rows.as<BedRow>();
  IMPG_HIP(hipMemsetAsync(S.bad.p, 0xFF, 8, s));
  IMPG_HIP(hipMemsetAsync(S.len.as<uint32_t>() + n, 0, 4, s));  // (the scan of n + 1 lengths leaves the total in off[n])
  fasta_piv_rows_kernel<<<cdiv(n, 256), 256, 0, s>>>(d_rows, n, rows);
  fasta_len_kernel<true><<<cdiv(n, 256), 256, 0, s>>>(rows, n, t, v.st, 0, S.len.as<uint32_t>(), S.bad.as<uint32_t>());
  IMPG_HIP(hipGetLastError());
  prims::exclusive_sum(S.stmp, S.len.as<uint32_t>(), S.off.as<u64>(), (size_t)n + 1, s);
  uint32_t h_bad[2];
  std::vector<u64> h_off((size_t)n + 1);
  IMPG_HIP(hipMemcpyAsync(h_bad, S.bad.p, 8, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipMemcpyAsync(h_off.data(), S.off.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipStreamSynchronize(s));
  refuse_marked(ix, rows, h_bad);
  const u64 PIECE = std::max<u64>((u64)E.opt.bed_text_piece_bytes, 1);
  S.reserve((size_t)std::min<u64>(PIECE, std::max<u64>(h_off[n], hint)), s);
  PieceTiming timing;
  device_text_windows(E, S, h_off.data(), n,
                      [&](uint32_t r0, uint32_t r1, unsigned long long base, unsigned long long n_bytes, char *out) {
                        write_piece<true>(ix, v, t, timing, rows + r0, r1 - r0, 0, S.off.as<u64>() + r0, base, n_bytes, out, s);
                      },
                      sink, ix.fasta_stats[FASTA_TEXT_PIECES], ix.fasta_stats[FASTA_TEXT_BYTES]);
  ix.fasta_stats[FASTA_RECORDS] += n;
  if (timing.on()) timing.report();
}

}  // namespace impg
