// Sequence files straight into HBM, the device side (impg_gpu_index_load_sequences; sequence_ingest.hpp has the two phases
// of a piece and the carry, sequence_ingest.cpp the reader and the driver).  A lane owns 16
// consecutive bytes of the piece's text, read with one 16-byte load; what it knows of them is a few 16-bit masks, counted
// with popcounts, and everything that needs the bytes before it comes from scans over ONE value per lane:
//
//   line state  a byte lies on a header line if its line's first byte is '>'.  Lines are of any length, so this is a scan:
//               each lane folds its 16 bytes into a map of the state (keep it / header / body), the maps are composed by
//               inclusive_scan, and the state a lane starts from is the scanned map of the lane before (the carry's for
//               lane 0).  One byte per lane in, one out.
//   classes     bases (not on a header line, not '\n', not '\r'), record heads ('>' at a line start) and header bytes, counted
//               per lane; three exclusive sums give a lane the piece's bases, heads and header bytes in front of it.
//   headers     the header lines' bytes compacted ('\n' included), and per head the bases in front of it: what the host
//               needs to cut the names and to count every record's bases.  A base while no record is open raises the flag.
//   place       byte form: every base upper-cased to dest + position, a 16-byte store where a lane's 16 bases are one
//               aligned stretch of one sequence, byte stores elsewhere.  Packed form: the piece's bases are first compacted
//               (upper-cased) so that base r's neighbours are r - 1 and r + 1 whatever line ends lay between them; a lane
//               of 16 compacted bases finds its record in the table, packs with fasta_pack_kernel's code -- a word it fills
//               alone is stored, a partial one completed with atomicOr into the zeroed stream -- and counts the heads and
//               ends of the runs of one byte that is not A/C/G/T; two more sums place them, a second pass writes them.
//   Every store is bounded by the sequence's own place: position < len, or the base is counted and never written.
//
// HBM temporaries per text byte: the text itself, 26 bytes per lane of 16 (two map bytes, three counts and
// their three sums), and in the packed form the compacted bases (one byte per base) and 16 bytes per lane of 16 bases.
// No kernel loops on data: every loop is over a lane's 16 bytes or bounded by n_recs, a launch argument.
#include <hip/hip_runtime.h>

#include "device_prims.hpp"
#include "engine.hpp"
#include "sequence_ingest.hpp"

namespace impg {

namespace {

using prims::cdiv;
using namespace ingest;
typedef unsigned long long u64;

struct Summary { u64 n_bases, n_heads, n_hdr, n_runs; uint32_t err, pad; };

struct MapCompose {  // maps of the line state: bit 1 set = "the state is bit 0 from here on", 0 = keep it
  __host__ __device__ uint8_t operator()(uint8_t a, uint8_t b) const { return (b & 2u) ? b : a; }
};

struct LaneText {
  uint32_t w[4];
  unsigned n;  // valid bytes
  __device__ __forceinline__ unsigned char at(unsigned i) const { return (unsigned char)(w[i >> 2] >> (8u * (i & 3u))); }
};
__device__ __forceinline__ LaneText lane_text(const uint4 *__restrict__ text, u64 lane, u64 n_bytes) {
  const uint4 v = text[lane];
  return LaneText{{v.x, v.y, v.z, v.w}, (unsigned)min((u64)16u, n_bytes - lane * 16u)};
}
// does the lane's first byte start a line?
__device__ __forceinline__ bool lane_starts_line(const uint4 *__restrict__ text, u64 lane, const Carry &c) {
  return lane ? reinterpret_cast<const unsigned char *>(text)[lane * 16u - 1u] == '\n' : c.at_line_start != 0;
}
__device__ __forceinline__ uint32_t upper4(uint32_t x) {  // a-z -> A-Z in four bytes at once
  const uint32_t y = x & 0x7F7F7F7Fu;
  const uint32_t m = (y + 0x1F1F1F1Fu) & ~(y + 0x05050505u) & ~x & 0x80808080u;  // bit 7: 0x61 <= byte <= 0x7A
  return x - (m >> 2);
}
__device__ __forceinline__ unsigned char upper1(unsigned char c) { return c >= 'a' && c <= 'z' ? (unsigned char)(c - 32) : c; }

// the lane's bytes by class, from the state it starts in
struct LaneMasks { uint32_t hdr, base, head; };
__device__ __forceinline__ LaneMasks lane_masks(const LaneText &t, bool start, bool hdr) {
  LaneMasks m{0u, 0u, 0u};
#pragma unroll
  for (unsigned i = 0; i < 16u; i++) {
    if (i < t.n) {
      const unsigned char ch = t.at(i);
      if (start) {
        hdr = ch == '>';
        if (hdr) m.head |= 1u << i;
      }
      if (hdr) m.hdr |= 1u << i;
      else if (ch != '\n' && ch != '\r') m.base |= 1u << i;
      start = ch == '\n';
    }
  }
  return m;
}
__device__ __forceinline__ bool lane_hdr_in(const uint8_t *__restrict__ st, u64 lane, const Carry &c) {
  return lane ? (st[lane - 1u] & 1u) != 0 : c.in_header != 0;
}

__global__ __launch_bounds__(256) void ingest_map_kernel(const uint4 *__restrict__ text, u64 n_bytes, u64 n_lanes, const Carry *__restrict__ carry,
                                                         uint8_t *__restrict__ map) {
  const u64 lane = (u64)blockIdx.x * 256u + threadIdx.x;
  if (lane >= n_lanes) return;
  const Carry c = *carry;
  const LaneText t = lane_text(text, lane, n_bytes);
  bool start = lane_starts_line(text, lane, c);
  uint8_t m = lane == 0 && !start ? (uint8_t)(2u | (c.in_header ? 1u : 0u)) : (uint8_t)0;
#pragma unroll
  for (unsigned i = 0; i < 16u; i++) {
    if (i < t.n) {
      const unsigned char ch = t.at(i);
      if (start) m = (uint8_t)(2u | (ch == '>' ? 1u : 0u));
      start = ch == '\n';
    }
  }
  map[lane] = m;
}

__global__ __launch_bounds__(256) void ingest_class_kernel(const uint4 *__restrict__ text, u64 n_bytes, u64 n_lanes, const Carry *__restrict__ carry,
                                                           const uint8_t *__restrict__ st, uint32_t *__restrict__ base_cnt,
                                                           uint32_t *__restrict__ head_cnt, uint32_t *__restrict__ hdr_cnt) {
  const u64 lane = (u64)blockIdx.x * 256u + threadIdx.x;
  if (lane >= n_lanes) return;
  const Carry c = *carry;
  const LaneMasks m = lane_masks(lane_text(text, lane, n_bytes), lane_starts_line(text, lane, c), lane_hdr_in(st, lane, c));
  base_cnt[lane] = __popc(m.base);
  head_cnt[lane] = __popc(m.head);
  hdr_cnt[lane] = __popc(m.hdr);
}

// the piece's totals and the state behind its last byte (one thread)
__global__ void ingest_scan_finish_kernel(const uint4 *__restrict__ text, u64 n_bytes, u64 n_lanes, const Carry *__restrict__ carry,
                                          const uint8_t *__restrict__ st, const uint32_t *__restrict__ base_cnt, const uint32_t *__restrict__ base_rank,
                                          const uint32_t *__restrict__ head_cnt, const uint32_t *__restrict__ head_ord,
                                          const uint32_t *__restrict__ hdr_cnt, const uint32_t *__restrict__ hdr_rank, Summary *__restrict__ sum,
                                          Carry *__restrict__ next) {
  const u64 last = n_lanes - 1u;
  sum->n_bases = (u64)base_rank[last] + base_cnt[last];
  sum->n_heads = (u64)head_ord[last] + head_cnt[last];
  sum->n_hdr = (u64)hdr_rank[last] + hdr_cnt[last];
  sum->n_runs = 0;
  sum->err = 0;
  const bool nl = reinterpret_cast<const unsigned char *>(text)[n_bytes - 1u] == '\n';
  *next = Carry{(uint32_t)(!nl && (st[last] & 1u)), (uint32_t)nl, (uint32_t)(carry->open || sum->n_heads), 0u};
}

__global__ __launch_bounds__(256) void ingest_header_kernel(const uint4 *__restrict__ text, u64 n_bytes, u64 n_lanes, const Carry *__restrict__ carry,
                                                            const uint8_t *__restrict__ st, const uint32_t *__restrict__ base_rank,
                                                            const uint32_t *__restrict__ head_ord, const uint32_t *__restrict__ hdr_rank, u64 n_hdr,
                                                            u64 n_heads, char *__restrict__ names, uint32_t *__restrict__ head_rank,
                                                            Summary *__restrict__ sum) {
  const u64 lane = (u64)blockIdx.x * 256u + threadIdx.x;
  if (lane >= n_lanes) return;
  const Carry c = *carry;
  const LaneText t = lane_text(text, lane, n_bytes);
  const LaneMasks m = lane_masks(t, lane_starts_line(text, lane, c), lane_hdr_in(st, lane, c));
  u64 hp = hdr_rank[lane], ho = head_ord[lane];
  uint32_t br = base_rank[lane];
  if (!c.open && ho == 0u) {  // no head before the lane: a base before the lane's first head is text before the first '>'
    const uint32_t before_head = m.head ? (m.head & (0u - m.head)) - 1u : 0xFFFFu;
    if (m.base & before_head) sum->err = 1u;  // (every lane that sees one writes the same value)
  }
#pragma unroll
  for (unsigned i = 0; i < 16u; i++) {
    if ((m.head >> i) & 1u) {
      if (ho < n_heads) head_rank[ho] = br;
      ho++;
    }
    if ((m.hdr >> i) & 1u) {
      if (hp < n_hdr) names[hp] = (char)t.at(i);
      hp++;
    }
    br += (m.base >> i) & 1u;
  }
}

// byte form: text -> store
__global__ __launch_bounds__(256) void ingest_place_bytes_kernel(const uint4 *__restrict__ text, u64 n_bytes, u64 n_lanes, const Carry *__restrict__ carry,
                                                                 const uint8_t *__restrict__ st, const uint32_t *__restrict__ base_rank,
                                                                 const uint32_t *__restrict__ head_ord, const Rec *__restrict__ recs, uint32_t n_recs,
                                                                 unsigned char *__restrict__ out, u64 out_bytes) {
  const u64 lane = (u64)blockIdx.x * 256u + threadIdx.x;
  if (lane >= n_lanes) return;
  const Carry c = *carry;
  const LaneText t = lane_text(text, lane, n_bytes);
  const LaneMasks m = lane_masks(t, lane_starts_line(text, lane, c), lane_hdr_in(st, lane, c));
  if (!m.base) return;
  uint32_t rec = head_ord[lane], r = base_rank[lane];
  if (rec >= n_recs) return;
  Rec R = recs[rec];
  if (m.base == 0xFFFFu) {  // 16 bases of one record (a head is a header byte: there is none)
    const u64 pos = (u64)(r - R.first_rank) + R.before;
    if (R.dest == NO_PLACE || pos >= R.len) return;
    const u64 P = R.dest + pos;
    if (pos + 16u <= R.len && (P & 15u) == 0u && P + 16u <= out_bytes) {
      *reinterpret_cast<uint4 *>(out + P) = make_uint4(upper4(t.w[0]), upper4(t.w[1]), upper4(t.w[2]), upper4(t.w[3]));
      return;
    }
  }
#pragma unroll
  for (unsigned i = 0; i < 16u; i++) {
    if ((m.head >> i) & 1u) {
      rec++;
      if (rec < n_recs) R = recs[rec];
    }
    if ((m.base >> i) & 1u) {
      const u64 pos = (u64)(r - R.first_rank) + R.before;
      if (rec < n_recs && R.dest != NO_PLACE && pos < R.len && R.dest + pos < out_bytes) out[R.dest + pos] = upper1(t.at(i));
      r++;
    }
  }
}

// packed form, first step: text -> the piece's bases, compacted and upper-cased
__global__ __launch_bounds__(256) void ingest_compact_kernel(const uint4 *__restrict__ text, u64 n_bytes, u64 n_lanes, const Carry *__restrict__ carry,
                                                             const uint8_t *__restrict__ st, const uint32_t *__restrict__ base_rank, u64 n_bases,
                                                             unsigned char *__restrict__ stage) {
  const u64 lane = (u64)blockIdx.x * 256u + threadIdx.x;
  if (lane >= n_lanes) return;
  const Carry c = *carry;
  const LaneText t = lane_text(text, lane, n_bytes);
  const LaneMasks m = lane_masks(t, lane_starts_line(text, lane, c), lane_hdr_in(st, lane, c));
  u64 r = base_rank[lane];
#pragma unroll
  for (unsigned i = 0; i < 16u; i++) {
    if ((m.base >> i) & 1u) {
      if (r < n_bases) stage[r] = upper1(t.at(i));
      r++;
    }
  }
}

__device__ __forceinline__ bool is_acgt(unsigned char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
// the record that holds base r of the piece: the last j with first_rank[j] <= r (first_rank[0] = 0)
__device__ __forceinline__ uint32_t rec_of(const Rec *__restrict__ recs, uint32_t n_recs, uint32_t r) {
  uint32_t lo = 0, hi = n_recs;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (recs[mid].first_rank <= r) lo = mid; else hi = mid;
  }
  return lo;
}
// packed form, second step: a lane of 16 compacted bases.  WRITE_RUNS = false: pack them into the stream and count the
// heads and ends of runs; true: write the runs, the k-th head and the k-th end of the piece being one run.
template <bool WRITE_RUNS>
__global__ __launch_bounds__(256) void ingest_pack_kernel(const unsigned char *__restrict__ stage, u64 n_bases, const Rec *__restrict__ recs, uint32_t n_recs,
                                                          uint32_t *__restrict__ words, u64 n_words, uint32_t *__restrict__ head_cnt,
                                                          uint32_t *__restrict__ end_cnt, const uint32_t *__restrict__ head_at,
                                                          const uint32_t *__restrict__ end_at, u64 n_runs, uint32_t *__restrict__ run_rec,
                                                          uint32_t *__restrict__ run_start, uint32_t *__restrict__ run_end,
                                                          unsigned char *__restrict__ run_byte) {
  const u64 lane = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 r0 = lane * 16u;
  if (r0 >= n_bases) return;
  const unsigned cnt = (unsigned)min((u64)16u, n_bases - r0);
  const uint4 v = *reinterpret_cast<const uint4 *>(stage + r0);
  const LaneText t{{v.x, v.y, v.z, v.w}, cnt};
  const unsigned char before = r0 ? stage[r0 - 1u] : (unsigned char)0, behind = r0 + 16u < n_bases ? stage[r0 + 16u] : (unsigned char)0;
  uint32_t rec = rec_of(recs, n_recs, (uint32_t)r0);
  Rec R = recs[rec];
  u64 cur_w = ~0ull;
  uint32_t bits = 0, filled = 0, heads = 0, ends = 0;
  u64 hk = 0, ek = 0;
  if (WRITE_RUNS) { hk = head_at[lane]; ek = end_at[lane]; }
  auto flush = [&]() {
    if (cur_w < n_words) {
      if (filled == 16u) words[cur_w] = bits;
      else if (bits) atomicOr(&words[cur_w], bits);
    }
  };
#pragma unroll
  for (unsigned i = 0; i < 16u; i++) {
    if (i < cnt) {
      const uint32_t r = (uint32_t)r0 + i;
      while (rec + 1u < n_recs && recs[rec + 1u].first_rank <= r) R = recs[++rec];
      const u64 pos = (u64)(r - R.first_rank) + R.before;
      if (R.dest != NO_PLACE && pos < R.len) {
        const unsigned char ch = t.at(i);
        if (!WRITE_RUNS) {
          const u64 P = R.dest + pos;
          if ((P >> 4) != cur_w) { flush(); cur_w = P >> 4; bits = 0; filled = 0; }
          bits |= (ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 0u) << (2u * (unsigned)(P & 15u));
          filled++;
        }
        if (!is_acgt(ch)) {
          // the base before / behind it in the same sequence, where the piece holds it
          const bool first = r == R.first_rank, last = r + 1u == n_bases || pos + 1u >= R.len || (rec + 1u < n_recs && recs[rec + 1u].first_rank == r + 1u);
          const unsigned char prev = i ? t.at(i - 1u) : before, next = i + 1u < 16u ? t.at(i + 1u) : behind;
          if (first || prev != ch) {
            if (WRITE_RUNS && hk < n_runs) { run_rec[hk] = rec; run_start[hk] = (uint32_t)pos; run_byte[hk] = ch; }
            hk++;
            heads++;
          }
          if (last || next != ch) {
            if (WRITE_RUNS && ek < n_runs) run_end[ek] = (uint32_t)pos + 1u;
            ek++;
            ends++;
          }
        }
      }
    }
  }
  if (!WRITE_RUNS) {
    flush();
    head_cnt[lane] = heads;
    end_cnt[lane] = ends;
  }
}
__global__ void ingest_runs_total_kernel(const uint32_t *__restrict__ head_cnt, const uint32_t *__restrict__ head_at, u64 n_lanes, Summary *__restrict__ sum) {
  sum->n_runs = (u64)head_at[n_lanes - 1u] + head_cnt[n_lanes - 1u];
}

// IMPG_SEQ_INGEST_TIMING=<file> (a probe's switch): per piece "bytes h2d_ms device_ms" appended to the file -- the copy of
// the piece's text between two events, and the sum over the piece's groups of kernels (each group queued without a host
// round trip inside it, between two events of its own), then every group's own time: scan, headers, place, runs --, then "reader <seconds>": what the reader took to copy or
// inflate every piece
struct IngestTiming {
  const char *path = getenv("IMPG_SEQ_INGEST_TIMING");
  struct Piece { u64 bytes; hipEvent_t e[2]; std::vector<hipEvent_t> spans; };  // spans: begin, end, begin, end, ...
  std::vector<Piece> pieces;
  bool on() const { return path && *path; }
  ~IngestTiming() {
    FILE *f = on() ? fopen(path, "a") : nullptr;
    for (Piece &p : pieces) {
      float ms = 0, k = 0;
      double kernels_ms = 0;
      std::string groups;  // scan, headers, place (packed: compact + pack + sums, then the runs' pass where there are runs)
      for (size_t i = 0; i + 1 < p.spans.size(); i += 2)
        if (hipEventElapsedTime(&k, p.spans[i], p.spans[i + 1]) == hipSuccess) { kernels_ms += k; groups += " " + std::to_string(k); }
      if (f && hipEventElapsedTime(&ms, p.e[0], p.e[1]) == hipSuccess) fprintf(f, "%llu %.6f %.6f%s\n", p.bytes, (double)ms, kernels_ms, groups.c_str());
      (void)hipEventDestroy(p.e[0]);
      (void)hipEventDestroy(p.e[1]);
      for (hipEvent_t e : p.spans) (void)hipEventDestroy(e);
    }
    if (f) fclose(f);
  }
};

struct DeviceBackend : Backend {
  impg_gpu_index &ix;
  hipStream_t s = nullptr;
  char *pin[2] = {nullptr, nullptr};
  size_t pin_cap[2] = {0, 0};
  bool packed = false;
  size_t store_bytes = 0;
  u64 n = 0, n_lanes = 0;  // the piece in flight
  int cur = 0;             // d_carry[cur] goes in, d_carry[cur ^ 1] comes out
  Summary *h_sum = nullptr;  // pinned
  size_t h_sum_cap = 0;
  Summary sum{};
  DevBuf d_text, d_map, d_st, d_cnt[3], d_rank[3], d_names, d_head_rank, d_recs, d_stage, d_rcnt[2], d_rat[2], d_run[4], d_sum, d_carry, d_tmp;
  IngestTiming timing;

  explicit DeviceBackend(impg_gpu_index &x) : ix(x) {}
  ~DeviceBackend() override {
    if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    for (int k = 0; k < 2; k++) if (pin[k]) pinned_give(pin[k], pin_cap[k]);
    if (h_sum) pinned_give(h_sum, h_sum_cap);
  }
  Carry *carry(int k) const { return d_carry.as<Carry>() + k; }
  void span_mark() {  // the begin or the end of a group of kernels of the piece in flight
    if (!timing.on()) return;
    hipEvent_t e;
    IMPG_HIP(hipEventCreate(&e));
    timing.pieces.back().spans.push_back(e);
    IMPG_HIP(hipEventRecord(e, s));
  }

  void begin(size_t piece_bytes, size_t bytes, bool p) override {
    packed = p;
    store_bytes = bytes;
    IMPG_HIP(hipStreamCreate(&s));
    for (int k = 0; k < 2; k++) pin[k] = (char *)pinned_take(piece_bytes, pin_cap[k]);
    h_sum = (Summary *)pinned_take(sizeof(Summary), h_sum_cap);
    const size_t lanes = piece_bytes / 16;
    d_text.reserve(piece_bytes + 16);
    d_map.reserve(lanes);
    d_st.reserve(lanes);
    for (int k = 0; k < 3; k++) { d_cnt[k].reserve(lanes * 4); d_rank[k].reserve(lanes * 4); }
    d_sum.reserve(256);
    d_carry.reserve(256);
    if (packed) {
      d_stage.reserve(piece_bytes + 16);
      for (int k = 0; k < 2; k++) { d_rcnt[k].reserve(lanes * 4); d_rat[k].reserve(lanes * 4); }
    }
    ix.d_seq_bases.reserve(store_bytes);
    IMPG_HIP(hipMemsetAsync(ix.d_seq_bases.p, 0, store_bytes, s));
  }
  char *buffer(int which) override { return pin[which]; }
  void file_start() override {
    const Carry c{0u, 1u, 0u, 0u};
    cur = 0;
    IMPG_HIP(hipStreamSynchronize(s));  // (the copy below reads a local)
    IMPG_HIP(hipMemcpy(carry(0), &c, sizeof c, hipMemcpyHostToDevice));
  }
  void scan_begin(int which, size_t bytes) override {
    n = bytes;
    n_lanes = (n + 15u) / 16u;
    const uint32_t grid = cdiv(n_lanes, 256);
    if (timing.on()) {
      IngestTiming::Piece p{n, {nullptr, nullptr}, {}};
      IMPG_HIP(hipEventCreate(&p.e[0]));
      IMPG_HIP(hipEventCreate(&p.e[1]));
      timing.pieces.push_back(p);
      IMPG_HIP(hipEventRecord(p.e[0], s));
    }
    IMPG_HIP(hipMemcpyAsync(d_text.p, pin[which], n, hipMemcpyHostToDevice, s));
    if (timing.on()) IMPG_HIP(hipEventRecord(timing.pieces.back().e[1], s));
    span_mark();
    const uint4 *text = d_text.as<uint4>();
    ingest_map_kernel<<<grid, 256, 0, s>>>(text, n, n_lanes, carry(cur), d_map.as<uint8_t>());
    prims::inclusive_scan(d_tmp, d_map.as<uint8_t>(), d_st.as<uint8_t>(), (size_t)n_lanes, MapCompose(), s);
    ingest_class_kernel<<<grid, 256, 0, s>>>(text, n, n_lanes, carry(cur), d_st.as<uint8_t>(), d_cnt[0].as<uint32_t>(), d_cnt[1].as<uint32_t>(),
                                             d_cnt[2].as<uint32_t>());
    for (int k = 0; k < 3; k++) prims::exclusive_sum(d_tmp, d_cnt[k].as<uint32_t>(), d_rank[k].as<uint32_t>(), (size_t)n_lanes, s);
    ingest_scan_finish_kernel<<<1, 1, 0, s>>>(text, n, n_lanes, carry(cur), d_st.as<uint8_t>(), d_cnt[0].as<uint32_t>(), d_rank[0].as<uint32_t>(),
                                              d_cnt[1].as<uint32_t>(), d_rank[1].as<uint32_t>(), d_cnt[2].as<uint32_t>(), d_rank[2].as<uint32_t>(),
                                              d_sum.as<Summary>(), carry(cur ^ 1));
    IMPG_HIP(hipGetLastError());
    span_mark();
    IMPG_HIP(hipMemcpyAsync(h_sum, d_sum.p, sizeof(Summary), hipMemcpyDeviceToHost, s));
  }
  void scan_end(PieceScan &out) override {
    IMPG_HIP(hipStreamSynchronize(s));
    sum = *h_sum;
    if (sum.n_bases > n || sum.n_heads > n || sum.n_hdr > n) throw Error{IMPG_E_HIP, "internal: sequence ingest counted more than the piece holds"};
    prims::grow(d_names, (size_t)sum.n_hdr);
    prims::grow(d_head_rank, (size_t)sum.n_heads * 4);
    span_mark();
    ingest_header_kernel<<<cdiv(n_lanes, 256), 256, 0, s>>>(d_text.as<uint4>(), n, n_lanes, carry(cur), d_st.as<uint8_t>(), d_rank[0].as<uint32_t>(),
                                                            d_rank[1].as<uint32_t>(), d_rank[2].as<uint32_t>(), sum.n_hdr, sum.n_heads,
                                                            d_names.as<char>(), d_head_rank.as<uint32_t>(), d_sum.as<Summary>());
    IMPG_HIP(hipGetLastError());
    span_mark();
    out.n_bases = sum.n_bases;
    out.n_heads = sum.n_heads;
    out.header.resize((size_t)sum.n_hdr);
    out.head_rank.resize((size_t)sum.n_heads);
    if (sum.n_hdr) IMPG_HIP(hipMemcpyAsync(out.header.data(), d_names.p, (size_t)sum.n_hdr, hipMemcpyDeviceToHost, s));
    if (sum.n_heads) IMPG_HIP(hipMemcpyAsync(out.head_rank.data(), d_head_rank.p, (size_t)sum.n_heads * 4, hipMemcpyDeviceToHost, s));
    IMPG_HIP(hipMemcpyAsync(h_sum, d_sum.p, sizeof(Summary), hipMemcpyDeviceToHost, s));
    IMPG_HIP(hipStreamSynchronize(s));
    out.text_before_head = h_sum->err != 0;
    cur ^= 1;  // (place() reads the carry the piece was scanned with: carry(cur ^ 1) from here on)
  }
  void place(const Rec *recs, uint32_t n_recs, std::vector<PieceRun> &runs) override {
    const Carry *c_in = carry(cur ^ 1);
    prims::grow(d_recs, (size_t)n_recs * sizeof(Rec));
    IMPG_HIP(hipMemcpyAsync(d_recs.p, recs, (size_t)n_recs * sizeof(Rec), hipMemcpyHostToDevice, s));
    IMPG_HIP(hipStreamSynchronize(s));  // (recs is the caller's, and pageable)
    span_mark();
    const uint32_t grid = cdiv(n_lanes, 256);
    if (!packed) {
      ingest_place_bytes_kernel<<<grid, 256, 0, s>>>(d_text.as<uint4>(), n, n_lanes, c_in, d_st.as<uint8_t>(), d_rank[0].as<uint32_t>(),
                                                     d_rank[1].as<uint32_t>(), d_recs.as<Rec>(), n_recs, ix.d_seq_bases.as<unsigned char>(), store_bytes);
      IMPG_HIP(hipGetLastError());
      span_mark();
      return;
    }
    const u64 nb = sum.n_bases, b_lanes = (nb + 15u) / 16u, n_words = store_bytes / 4u;
    const uint32_t bgrid = cdiv(b_lanes, 256);
    ingest_compact_kernel<<<grid, 256, 0, s>>>(d_text.as<uint4>(), n, n_lanes, c_in, d_st.as<uint8_t>(), d_rank[0].as<uint32_t>(), nb,
                                               d_stage.as<unsigned char>());
    ingest_pack_kernel<false><<<bgrid, 256, 0, s>>>(d_stage.as<unsigned char>(), nb, d_recs.as<Rec>(), n_recs, ix.d_seq_bases.as<uint32_t>(), n_words,
                                                    d_rcnt[0].as<uint32_t>(), d_rcnt[1].as<uint32_t>(), nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                                                    nullptr);
    IMPG_HIP(hipGetLastError());
    for (int k = 0; k < 2; k++) prims::exclusive_sum(d_tmp, d_rcnt[k].as<uint32_t>(), d_rat[k].as<uint32_t>(), (size_t)b_lanes, s);
    ingest_runs_total_kernel<<<1, 1, 0, s>>>(d_rcnt[0].as<uint32_t>(), d_rat[0].as<uint32_t>(), b_lanes, d_sum.as<Summary>());
    span_mark();
    IMPG_HIP(hipMemcpyAsync(h_sum, d_sum.p, sizeof(Summary), hipMemcpyDeviceToHost, s));
    IMPG_HIP(hipStreamSynchronize(s));
    const u64 n_runs = h_sum->n_runs;
    if (n_runs > nb) throw Error{IMPG_E_HIP, "internal: sequence ingest counted more runs than bases"};
    if (n_runs) {
      for (int k = 0; k < 3; k++) prims::grow(d_run[k], (size_t)n_runs * 4);
      prims::grow(d_run[3], (size_t)n_runs);
      span_mark();
      ingest_pack_kernel<true><<<bgrid, 256, 0, s>>>(d_stage.as<unsigned char>(), nb, d_recs.as<Rec>(), n_recs, nullptr, 0, nullptr, nullptr,
                                                     d_rat[0].as<uint32_t>(), d_rat[1].as<uint32_t>(), n_runs, d_run[0].as<uint32_t>(),
                                                     d_run[1].as<uint32_t>(), d_run[2].as<uint32_t>(), d_run[3].as<unsigned char>());
      IMPG_HIP(hipGetLastError());
      span_mark();
    }
    std::vector<uint32_t> h[3];
    std::vector<unsigned char> hb((size_t)n_runs);
    for (int k = 0; k < 3 && n_runs; k++) {
      h[k].resize((size_t)n_runs);
      IMPG_HIP(hipMemcpyAsync(h[k].data(), d_run[k].p, (size_t)n_runs * 4, hipMemcpyDeviceToHost, s));
    }
    if (n_runs) IMPG_HIP(hipMemcpyAsync(hb.data(), d_run[3].p, (size_t)n_runs, hipMemcpyDeviceToHost, s));
    IMPG_HIP(hipStreamSynchronize(s));
    for (u64 k = 0; k < n_runs; k++) runs.push_back(PieceRun{h[0][k], h[1][k], h[2][k], hb[k]});
  }
  void end() override { IMPG_HIP(hipStreamSynchronize(s)); }
};

void upload(DevBuf &d, const void *src, size_t bytes) {  // (never an empty buffer: a kernel argument points into it)
  d.reserve(std::max<size_t>(bytes, 16));
  if (bytes) IMPG_HIP(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
}

}  // namespace
}  // namespace impg

using namespace impg;

extern "C" int impg_gpu_index_load_sequences(impg_gpu_index_t *ix, const char *const *paths, size_t n_paths) {
  IMPG_TRY
  if (!ix || (n_paths && !paths)) throw Error{IMPG_E_INVALID, "null argument"};
  if (ix->shard || ix->cluster) throw Error{IMPG_E_UNSUPPORTED, "a sequence store on a sharded index"};
  if (ix->tp_mode) throw Error{IMPG_E_UNSUPPORTED, "a sequence store on a tracepoint index (it has no sequence names)"};
  std::vector<std::string> p;
  for (size_t i = 0; i < n_paths; i++) {
    if (!paths[i]) throw Error{IMPG_E_INVALID, "null argument"};
    p.push_back(paths[i]);
  }
  IMPG_HIP(hipSetDevice(ix->device));
  ix->seq_store.reset();  // the call replaces any attached store; after a failure the handle has none
  ix->store_of_id.clear();
  ix->drop_device_sequences();
  for (auto &c : ix->ingest_stats) c = 0;
  if (ix->opt.sequence_store_packed == 2)
    throw Error{IMPG_E_INVALID, "sequence_store_packed = 2 (the smaller form) needs every run counted before a base is placed: "
                                "impg_gpu_index_load_sequences takes 0 or 1 (impg_gpu_index_set_sequences keeps the choice)"};
  const bool packed = ix->opt.sequence_store_packed == 1;
  std::vector<std::string> names(ix->seq.lens.size());
  for (size_t id = 0; id < names.size(); id++) names[id] = id < ix->seq.names.size() ? ix->seq.names[id] : std::to_string(id);
  try {
    ingest::Loaded L;
    {
      DeviceBackend B(*ix);
      ingest::load_files(B, p, names, ix->seq.lens, (size_t)ix->opt.sequence_ingest_piece_bytes, packed, L);
    }
    if (const char *tp = getenv("IMPG_SEQ_INGEST_TIMING")) {
      if (FILE *f = *tp ? fopen(tp, "a") : nullptr) {  // (behind the pieces' lines, which the backend wrote when it went)
        fprintf(f, "reader %.6f\n", L.read_seconds);
        fclose(f);
      }
    }
    auto st = std::make_shared<SeqStore>();
    st->device_only = true;
    st->names = L.names;
    st->off.assign(1, 0);
    for (size_t i = 0; i < L.names.size(); i++) {
      st->off.push_back(st->off.back() + L.counts[i]);
      st->by_name.emplace(L.names[i], (uint32_t)i);
    }
    if (packed) {
      const PackedPlan &pl = L.plan;
      upload(ix->d_seq_off, pl.off.data(), pl.off.size() * 8);
      upload(ix->d_seq_run_off, pl.run_off.data(), pl.run_off.size() * 8);
      upload(ix->d_seq_blk_off, pl.blk_off.data(), pl.blk_off.size() * 8);
      upload(ix->d_seq_runs, pl.runs.data(), pl.runs.size() * sizeof(uint2));
      upload(ix->d_seq_run_byte, pl.run_byte.data(), pl.run_byte.size());
      upload(ix->d_seq_blk, pl.blk.data(), pl.blk.size() * 4);
      ix->fasta_stats[FASTA_STORE_EXCEPTION_RUNS] = pl.runs.size();
    } else upload(ix->d_seq_off, L.off.data(), L.off.size() * 8);
    ix->seq_packed = packed;
    ix->fasta_stats[FASTA_STORE_BYTES] = L.store_bytes;
    ix->fasta_stats[FASTA_STORE_PACKED] = packed ? 1 : 0;
    for (int k = 0; k < ingest::N_STATS; k++) ix->ingest_stats[k] = L.stats[k];
    ix->store_of_id = L.store_of_id;
    ix->seq_store = st;
  } catch (...) {
    ix->seq_store.reset();
    ix->store_of_id.clear();
    ix->drop_device_sequences();
    throw;
  }
  return IMPG_OK;
  IMPG_CATCH
}
