// PAF files streamed into HBM, the device side (impg_gpu_index_create_from_paf_streamed; paf_ingest.hpp has the phases of a
// piece and the steps the twin shares, paf_ingest.cpp the driver).  In the byte-wise kernels a lane
// owns 16 consecutive bytes of the piece, read with one 16-byte load, and knows them as 16-bit masks of '\n' and '\t'; the
// line of a byte is the exclusive sum of the lanes' '\n' counts plus a popcount.  The per-line kernels are a thread a line
// (heads, spans, records) or a thread a name (lookup), and the CIGARs go through the tokenizer's own two kernels.
// No kernel loops on data alone: every loop is over a lane's 16 bytes, or bounded by the line's end, the name's length
// (part of a line) or the table's capacity.  Every store is bounded by the count its array was sized with.
#include <hip/hip_runtime.h>

#include "device_prims.hpp"
#include "engine.hpp"
#include "paf_ingest.hpp"

namespace impg {

namespace {

using prims::cdiv;
using namespace paf_ingest;
typedef unsigned long long u64;

struct Summary { uint32_t n_nl, last_is_nl, n_unknown, first_bad; u64 unknown_bytes, n_ops; uint32_t cigar_bad, internal; };

struct LaneText {
  uint32_t w[4];
  unsigned n;  // valid bytes
  __device__ __forceinline__ unsigned char at(unsigned i) const { return (unsigned char)(w[i >> 2] >> (8u * (i & 3u))); }
};
__device__ __forceinline__ LaneText lane_text(const uint4 *__restrict__ text, u64 lane, u64 n_bytes) {
  const uint4 v = text[lane];
  return LaneText{{v.x, v.y, v.z, v.w}, (unsigned)min((u64)16u, n_bytes - lane * 16u)};
}
__device__ __forceinline__ uint32_t mask_of(const LaneText &t, unsigned char c) {
  uint32_t m = 0;
#pragma unroll
  for (unsigned i = 0; i < 16u; i++)
    if (i < t.n && t.at(i) == c) m |= 1u << i;
  return m;
}

// ---- scan ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void paf_nl_count_kernel(const uint4 *__restrict__ text, u64 n_bytes, u64 n_lanes, uint32_t *__restrict__ cnt) {
  const u64 lane = (u64)blockIdx.x * 256u + threadIdx.x;
  if (lane >= n_lanes) return;
  cnt[lane] = __popc(mask_of(lane_text(text, lane, n_bytes), '\n'));
}
__global__ void paf_scan_finish_kernel(const uint4 *__restrict__ text, u64 n_bytes, u64 n_lanes, const uint32_t *__restrict__ cnt,
                                       const uint32_t *__restrict__ rank, Summary *__restrict__ sum) {
  sum->n_nl = rank[n_lanes - 1u] + cnt[n_lanes - 1u];
  sum->last_is_nl = reinterpret_cast<const unsigned char *>(text)[n_bytes - 1u] == '\n';
  sum->first_bad = NONE;
  sum->cigar_bad = 0;
  sum->internal = 0;
}
// line_start[l + 1] = the byte behind line l's '\n'; the text's end closes a last line without one as a '\n' at n would
__global__ __launch_bounds__(256) void paf_line_start_kernel(const uint4 *__restrict__ text, u64 n_bytes, u64 n_lanes, const uint32_t *__restrict__ rank,
                                                             uint32_t n_lines, uint32_t *__restrict__ line_start) {
  const u64 lane = (u64)blockIdx.x * 256u + threadIdx.x;
  if (lane >= n_lanes) return;
  if (lane == 0) line_start[0] = 0u;  // (line_start[n_lines] is paf_last_line_kernel's)
  const uint32_t nl = mask_of(lane_text(text, lane, n_bytes), '\n');
  uint32_t r = rank[lane];
#pragma unroll
  for (unsigned i = 0; i < 16u; i++)
    if ((nl >> i) & 1u) {
      r++;
      if (r < n_lines) line_start[r] = (uint32_t)(lane * 16u + i) + 1u;
    }
}
__global__ void paf_last_line_kernel(u64 n_bytes, uint32_t n_lines, const Summary *__restrict__ sum, uint32_t *__restrict__ line_start) {
  line_start[n_lines] = (uint32_t)n_bytes + (sum->last_is_nl ? 0u : 1u);
}

// ---- heads --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void paf_heads_kernel(const char *__restrict__ text, u64 n_bytes, const uint32_t *__restrict__ line_start, uint32_t n_lines,
                                                        Head *__restrict__ heads, uint32_t *__restrict__ cg_at, uint32_t *__restrict__ cg_end,
                                                        Summary *__restrict__ sum) {
  const uint32_t l = blockIdx.x * 256u + threadIdx.x;
  if (l >= n_lines) return;
  const uint32_t a = min(line_start[l], (uint32_t)n_bytes), b = min(max(line_start[l + 1u], a + 1u) - 1u, (uint32_t)n_bytes);
  const Head h = line_head(text, a, b);
  heads[l] = h;
  cg_at[l] = NONE;
  cg_end[l] = h.end;
  if (h.err) atomicMin(&sum->first_bad, l);
}

// ---- the tag --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void paf_tag_kernel(const uint4 *__restrict__ text, u64 n_bytes, u64 n_lanes, const uint32_t *__restrict__ rank,
                                                      const Head *__restrict__ heads, uint32_t n_lines, uint32_t *__restrict__ cg_at) {
  const u64 lane = (u64)blockIdx.x * 256u + threadIdx.x;
  if (lane >= n_lanes) return;
  const LaneText t = lane_text(text, lane, n_bytes);
  const uint32_t c = mask_of(t, 'c');
  if (!c) return;
  const unsigned char *bytes = reinterpret_cast<const unsigned char *>(text);
  const uint32_t nl = mask_of(t, '\n'), tab = mask_of(t, '\t');
  const unsigned char before = lane ? bytes[lane * 16u - 1u] : (unsigned char)'\n';
  const uint32_t starts = (((nl | tab) << 1) | (before == '\n' || before == '\t' ? 1u : 0u)) & c;  // field starts that hold a 'c'
  const uint32_t r = rank[lane];
#pragma unroll
  for (unsigned i = 0; i < 16u; i++)
    if ((starts >> i) & 1u) {
      const uint32_t line = r + __popc(nl & ((1u << i) - 1u));
      const u64 p = lane * 16u + i;
      if (line < n_lines && p + 5u <= heads[line].end && bytes[p + 1u] == 'g' && bytes[p + 2u] == ':' && bytes[p + 3u] == 'Z' && bytes[p + 4u] == ':')
        atomicMin(&cg_at[line], (uint32_t)p);
    }
}
__global__ __launch_bounds__(256) void paf_tag_end_kernel(const uint4 *__restrict__ text, u64 n_bytes, u64 n_lanes, const uint32_t *__restrict__ rank,
                                                          uint32_t n_lines, const uint32_t *__restrict__ cg_at, uint32_t *__restrict__ cg_end) {
  const u64 lane = (u64)blockIdx.x * 256u + threadIdx.x;
  if (lane >= n_lanes) return;
  const LaneText t = lane_text(text, lane, n_bytes);
  const uint32_t tab = mask_of(t, '\t');
  if (!tab) return;
  const uint32_t nl = mask_of(t, '\n'), r = rank[lane];
#pragma unroll
  for (unsigned i = 0; i < 16u; i++)
    if ((tab >> i) & 1u) {
      const uint32_t line = r + __popc(nl & ((1u << i) - 1u)), p = (uint32_t)(lane * 16u + i);
      if (line >= n_lines) continue;
      const uint32_t at = cg_at[line];
      if (at != NONE && p > at) atomicMin(&cg_end[line], p);
    }
}

// ---- names ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void paf_names_kernel(const char *__restrict__ text, const Head *__restrict__ heads, uint32_t n_occ, TableView T,
                                                        unsigned hash_bits, uint32_t *__restrict__ ids, uint32_t *__restrict__ flag,
                                                        uint32_t *__restrict__ ulen) {
  const uint32_t o = blockIdx.x * 256u + threadIdx.x;
  if (o >= n_occ) return;
  const Head &h = heads[o >> 1];
  uint32_t id = NONE, unknown = 0, len = 0;
  if (!h.err) {
    const char *nm = text + h.name_at[o & 1u];
    len = h.name_len[o & 1u];
    id = table_find(T, nm, len, name_hash(nm, len, hash_bits));
    unknown = id == NONE;
  }
  ids[o] = id;
  flag[o] = unknown;
  ulen[o] = unknown ? len : 0u;
}
__global__ void paf_unknown_total_kernel(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ upos, const uint32_t *__restrict__ ulen,
                                         const u64 *__restrict__ uat, uint32_t n_occ, Summary *__restrict__ sum) {
  sum->n_unknown = upos[n_occ - 1u] + flag[n_occ - 1u];
  sum->unknown_bytes = uat[n_occ - 1u] + ulen[n_occ - 1u];
}
__global__ __launch_bounds__(256) void paf_unknown_write_kernel(const char *__restrict__ text, const Head *__restrict__ heads, uint32_t n_occ,
                                                                const uint32_t *__restrict__ flag, const uint32_t *__restrict__ upos,
                                                                const u64 *__restrict__ uat, uint32_t n_unknown, u64 n_bytes_out,
                                                                Unknown *__restrict__ list, char *__restrict__ out) {
  const uint32_t o = blockIdx.x * 256u + threadIdx.x;
  if (o >= n_occ || !flag[o]) return;
  const Head &h = heads[o >> 1];
  const uint32_t k = upos[o], len = h.name_len[o & 1u];
  const u64 at = uat[o];
  if (k >= n_unknown || at + len > n_bytes_out) return;
  list[k] = Unknown{o, len, at, (int64_t)h.len[o & 1u]};
  const char *nm = text + h.name_at[o & 1u];
  for (uint32_t i = 0; i < len; i++) out[at + i] = nm[i];
}
__global__ __launch_bounds__(256) void paf_patch_kernel(const uint32_t *__restrict__ occ, const uint32_t *__restrict__ id, uint32_t n, uint32_t n_occ,
                                                        uint32_t *__restrict__ ids) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k < n && occ[k] < n_occ) ids[occ[k]] = id[k];
}

// ---- cigars, records --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void paf_spans_kernel(const uint32_t *__restrict__ cg_at, const uint32_t *__restrict__ cg_end, uint32_t n_lines,
                                                        u64 *__restrict__ boff, uint32_t *__restrict__ blen) {
  const uint32_t l = blockIdx.x * 256u + threadIdx.x;
  if (l >= n_lines) return;
  const uint32_t at = cg_at[l], end = cg_end[l];
  const bool on = at != NONE && end >= at + 5u;
  boff[l] = on ? (u64)at + 5u : 0ull;
  blen[l] = on ? end - (at + 5u) : 0u;
}
__global__ void paf_ops_total_kernel(const uint32_t *__restrict__ cnt, const u64 *__restrict__ off, uint32_t n_lines, const uint32_t *__restrict__ bad,
                                     Summary *__restrict__ sum) {
  sum->n_ops = off[n_lines - 1u] + cnt[n_lines - 1u];
  sum->cigar_bad = *bad;
}
__global__ __launch_bounds__(256) void paf_records_kernel(const Head *__restrict__ heads, const uint32_t *__restrict__ ids, const uint32_t *__restrict__ cnt,
                                                          const u64 *__restrict__ off, uint32_t n_lines, u64 pool_at, impg_gpu_record_t *__restrict__ out,
                                                          Summary *__restrict__ sum) {
  const uint32_t l = blockIdx.x * 256u + threadIdx.x;
  if (l >= n_lines) return;
  const Head &h = heads[l];
  const uint32_t q = ids[2u * l], t = ids[2u * l + 1u];
  if (q == NONE || t == NONE) sum->internal = 1u;
  out[l] = impg_gpu_record_t{q, t, (int32_t)h.c[0], (int32_t)h.c[1], (int32_t)h.c[2], (int32_t)h.c[3], pool_at + off[l], cnt[l], h.strand};
}

// IMPG_PAF_INGEST_TIMING=<file> (a probe's switch): one line "pieces .. h2d_ms .. scan_ms .. names_ms .. cigars_ms .. wait_s ..
// free_start .. free_low .." appended when the ingest ends: the copies of the pieces' text, the three groups of kernels (scan, heads, tag
// and lookup; the unknown names' list; patch, cigars and records), the host's waits for the device, and the low-water mark of
// free HBM sampled once a piece
struct Timing {
  const char *path = getenv("IMPG_PAF_INGEST_TIMING");
  bool on() const { return path && *path; }
  hipEvent_t e[6] = {};
  double ms[3 + 1] = {0, 0, 0, 0}, wait_s = 0;
  size_t free_low = ~(size_t)0;
  uint64_t pieces = 0;
  size_t free_start = 0;  // free HBM before the ingest's first block
  void start() {
    if (!on()) return;
    for (auto &x : e) IMPG_HIP(hipEventCreate(&x));
    size_t tot = 0;
    (void)hipMemGetInfo(&free_start, &tot);
  }
  void mark(int k, hipStream_t s) { if (on()) IMPG_HIP(hipEventRecord(e[k], s)); }
  void add(int group, int a, int b) {
    float f = 0;
    if (on() && hipEventElapsedTime(&f, e[a], e[b]) == hipSuccess) ms[group] += f;
  }
  void sample() {
    if (!on()) return;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) free_low = std::min(free_low, fr);
    pieces++;
  }
  ~Timing() {
    if (!on()) return;
    if (FILE *f = fopen(path, "a")) {
      fprintf(f, "pieces %llu h2d_ms %.3f scan_ms %.3f names_ms %.3f cigars_ms %.3f wait_s %.6f free_start %zu free_low %zu\n", (unsigned long long)pieces,
              ms[0], ms[1], ms[2], ms[3], wait_s, free_start, free_low);
      fclose(f);
    }
    for (auto &x : e) if (x) (void)hipEventDestroy(x);
  }
};

struct DeviceBackend : Backend {
  int device;
  hipStream_t s = nullptr;
  char *pin[2] = {nullptr, nullptr};
  size_t pin_cap[2] = {0, 0}, buf_bytes = 0;
  Summary *h_sum = nullptr;  // pinned
  size_t h_sum_cap = 0;
  unsigned hash_bits = 64;
  u64 n = 0, n_lanes = 0;  // the piece in flight
  uint32_t n_lines = 0;
  u64 pool_cap = 0, pool_used = 0, rec_cap = 0, rec_used = 0;  // ops, records
  DevBuf d_text, d_cnt, d_rank, d_sum, d_ls, d_heads, d_cg_at, d_cg_end, d_ids, d_flag, d_ulen, d_upos, d_uat, d_list, d_bytes, d_occ, d_pid, d_boff, d_blen,
      d_ccnt, d_coff, d_bad, d_tmp, d_slot, d_hash, d_off, d_npool, d_pool, d_rec;
  TableView tv{16, nullptr, nullptr, nullptr, nullptr};
  Timing timing;

  explicit DeviceBackend(int dev) : device(dev) {}
  ~DeviceBackend() override {
    if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    for (int k = 0; k < 2; k++) if (pin[k]) pinned_give(pin[k], pin_cap[k]);
    if (h_sum) pinned_give(h_sum, h_sum_cap);
  }
  void wait() {
    const auto t0 = std::chrono::steady_clock::now();
    IMPG_HIP(hipStreamSynchronize(s));
    timing.wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  const Summary &summary() {  // the device's summary as it stands when the queue has drained
    IMPG_HIP(hipMemcpyAsync(h_sum, d_sum.p, sizeof(Summary), hipMemcpyDeviceToHost, s));
    wait();
    return *h_sum;
  }
  void begin(size_t buffer_bytes, uint64_t pool_ops, unsigned hb) override {
    IMPG_HIP(hipSetDevice(device));
    IMPG_HIP(hipStreamCreate(&s));
    timing.start();
    hash_bits = hb;
    buf_bytes = buffer_bytes;
    for (int k = 0; k < 2; k++) pin[k] = (char *)pinned_take(buffer_bytes, pin_cap[k]);
    h_sum = (Summary *)pinned_take(sizeof(Summary), h_sum_cap);
    d_sum.reserve(256);
    d_bad.reserve(256);
    pool_cap = std::max<u64>(pool_ops, 1);
    try {
      d_pool.reserve((size_t)pool_cap * 4 + 64);
    } catch (const Error &e) {
      if (e.code != IMPG_E_OOM) throw;
      throw Error{IMPG_E_OOM, "not enough device memory for the op pool of the streamed PAF ingest (" + std::to_string(pool_cap * 4 >> 20) +
                                  " MiB): impg_gpu_index_create_from_paf builds such an input with the host's help"};
    }
    rec_cap = 1024;
    d_rec.reserve((size_t)rec_cap * sizeof(impg_gpu_record_t));
  }
  char *buffer(int which) override { return pin[which]; }
  void grow(size_t buffer_bytes, int which, size_t keep) override {
    wait();  // (the piece in flight has left its block; the device text grows when the next piece arrives)
    for (int k = 0; k < 2; k++) {
      size_t cap = 0;
      char *p = (char *)pinned_take(buffer_bytes, cap);
      if (k == which && keep) memcpy(p, pin[k], keep);
      pinned_give(pin[k], pin_cap[k]);
      pin[k] = p;
      pin_cap[k] = cap;
    }
    buf_bytes = buffer_bytes;
  }
  void up(DevBuf &d, const void *src, size_t bytes) {
    d.reserve(std::max<size_t>(bytes, 256));
    if (bytes) IMPG_HIP(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
  }
  void table(const Table &t) override {
    wait();
    up(d_slot, t.slot.data(), t.slot.size() * 4);
    up(d_hash, t.hash.data(), t.hash.size() * 8);
    up(d_off, t.off.data(), t.off.size() * 8);
    up(d_npool, t.pool.data(), t.pool.size());
    tv = TableView{t.cap, d_slot.as<uint32_t>(), d_hash.as<uint64_t>(), d_off.as<uint64_t>(), d_npool.as<char>()};
  }
  void piece_begin(int which, size_t bytes) override {
    n = bytes;
    n_lanes = (n + 15u) / 16u;
    const uint32_t grid = cdiv(n_lanes, 256);
    if (d_text.cap < n + 16) d_text.reserve(buf_bytes + 16);
    prims::grow(d_cnt, n_lanes * 4);
    prims::grow(d_rank, n_lanes * 4);
    timing.sample();
    timing.mark(0, s);
    IMPG_HIP(hipMemcpyAsync(d_text.p, pin[which], n, hipMemcpyHostToDevice, s));
    timing.mark(1, s);
    const uint4 *text = d_text.as<uint4>();
    paf_nl_count_kernel<<<grid, 256, 0, s>>>(text, n, n_lanes, d_cnt.as<uint32_t>());
    prims::exclusive_sum(d_tmp, d_cnt.as<uint32_t>(), d_rank.as<uint32_t>(), (size_t)n_lanes, s);
    paf_scan_finish_kernel<<<1, 1, 0, s>>>(text, n, n_lanes, d_cnt.as<uint32_t>(), d_rank.as<uint32_t>(), d_sum.as<Summary>());
    IMPG_HIP(hipGetLastError());
    const Summary &sm = summary();
    if ((u64)sm.n_nl > n) throw Error{IMPG_E_HIP, "internal: PAF ingest counted more lines than the piece has bytes"};
    if (sm.n_nl >= (1u << 31) - 1u) throw Error{IMPG_E_UNSUPPORTED, "2^31 lines or more in one piece of a PAF file: choose smaller pieces"};
    n_lines = sm.n_nl + (sm.last_is_nl ? 0u : 1u);
    const uint32_t L = n_lines, lgrid = cdiv(L, 256), n_occ = 2u * L, ogrid = cdiv(n_occ, 256);
    prims::grow(d_ls, ((size_t)L + 1) * 4);
    prims::grow(d_heads, (size_t)L * sizeof(Head));
    prims::grow(d_cg_at, (size_t)L * 4);
    prims::grow(d_cg_end, (size_t)L * 4);
    for (DevBuf *b : {&d_ids, &d_flag, &d_ulen, &d_upos}) prims::grow(*b, (size_t)n_occ * 4);
    prims::grow(d_uat, (size_t)n_occ * 8);
    paf_line_start_kernel<<<grid, 256, 0, s>>>(text, n, n_lanes, d_rank.as<uint32_t>(), L, d_ls.as<uint32_t>());
    paf_last_line_kernel<<<1, 1, 0, s>>>(n, L, d_sum.as<Summary>(), d_ls.as<uint32_t>());
    paf_heads_kernel<<<lgrid, 256, 0, s>>>(d_text.as<char>(), n, d_ls.as<uint32_t>(), L, d_heads.as<Head>(), d_cg_at.as<uint32_t>(),
                                           d_cg_end.as<uint32_t>(), d_sum.as<Summary>());
    paf_tag_kernel<<<grid, 256, 0, s>>>(text, n, n_lanes, d_rank.as<uint32_t>(), d_heads.as<Head>(), L, d_cg_at.as<uint32_t>());
    paf_tag_end_kernel<<<grid, 256, 0, s>>>(text, n, n_lanes, d_rank.as<uint32_t>(), L, d_cg_at.as<uint32_t>(), d_cg_end.as<uint32_t>());
    paf_names_kernel<<<ogrid, 256, 0, s>>>(d_text.as<char>(), d_heads.as<Head>(), n_occ, tv, hash_bits, d_ids.as<uint32_t>(), d_flag.as<uint32_t>(),
                                           d_ulen.as<uint32_t>());
    IMPG_HIP(hipGetLastError());
    prims::exclusive_sum(d_tmp, d_flag.as<uint32_t>(), d_upos.as<uint32_t>(), (size_t)n_occ, s);
    prims::exclusive_sum(d_tmp, d_ulen.as<uint32_t>(), d_uat.as<u64>(), (size_t)n_occ, s);
    paf_unknown_total_kernel<<<1, 1, 0, s>>>(d_flag.as<uint32_t>(), d_upos.as<uint32_t>(), d_ulen.as<uint32_t>(), d_uat.as<u64>(), n_occ, d_sum.as<Summary>());
    IMPG_HIP(hipGetLastError());
    timing.mark(2, s);
  }
  uint32_t first_bad = NONE;
  void piece_unknowns(uint32_t &lines, std::vector<Unknown> &list, std::string &bytes) override {
    const Summary sm = summary();
    timing.add(0, 0, 1);
    timing.add(1, 1, 2);
    const uint32_t n_occ = 2u * n_lines;
    if (sm.n_unknown > n_occ || sm.unknown_bytes > 2u * n) throw Error{IMPG_E_HIP, "internal: PAF ingest listed more names than the piece holds"};
    first_bad = sm.first_bad;
    lines = n_lines;
    list.resize(sm.n_unknown);
    bytes.resize((size_t)sm.unknown_bytes);
    if (!sm.n_unknown) return;
    prims::grow(d_list, (size_t)sm.n_unknown * sizeof(Unknown));
    prims::grow(d_bytes, (size_t)sm.unknown_bytes);
    timing.mark(3, s);
    paf_unknown_write_kernel<<<cdiv(n_occ, 256), 256, 0, s>>>(d_text.as<char>(), d_heads.as<Head>(), n_occ, d_flag.as<uint32_t>(), d_upos.as<uint32_t>(),
                                                             d_uat.as<u64>(), sm.n_unknown, sm.unknown_bytes, d_list.as<Unknown>(), d_bytes.as<char>());
    IMPG_HIP(hipGetLastError());
    timing.mark(4, s);
    IMPG_HIP(hipMemcpyAsync(list.data(), d_list.p, (size_t)sm.n_unknown * sizeof(Unknown), hipMemcpyDeviceToHost, s));
    if (sm.unknown_bytes) IMPG_HIP(hipMemcpyAsync(&bytes[0], d_bytes.p, (size_t)sm.unknown_bytes, hipMemcpyDeviceToHost, s));
    wait();
    timing.add(2, 3, 4);
  }
  // room for `need` more elements of `elem` bytes behind the `used` ones: a larger block and a device-to-device copy
  bool make_room(DevBuf &d, u64 &cap, u64 used, u64 need, size_t elem, bool by_half) {
    if (used + need <= cap) return false;
    u64 nc = cap;
    while (used + need > nc) nc = std::max<u64>(by_half ? nc + nc / 2 : nc * 2, 64);
    DevBuf bigger;
    try {
      bigger.reserve((size_t)nc * elem + 64);
    } catch (const Error &e) {
      if (e.code != IMPG_E_OOM) throw;
      throw Error{IMPG_E_OOM, "not enough device memory to grow the streamed PAF ingest's arrays (" + std::to_string(nc * elem >> 20) +
                                  " MiB beside the " + std::to_string(cap * elem >> 20) + " in use): impg_gpu_index_create_from_paf builds such an input with the host's help"};
    }
    if (used) IMPG_HIP(hipMemcpyAsync(bigger.p, d.p, (size_t)used * elem, hipMemcpyDeviceToDevice, s));
    wait();
    d.swap(bigger);
    cap = nc;
    return true;
  }
  uint32_t piece_end(const std::vector<uint32_t> &occ, const std::vector<uint32_t> &id, uint64_t &n_ops, uint64_t &pool_regrows) override {
    const uint32_t L = n_lines, n_occ = 2u * L;
    const uint32_t Lc = first_bad == NONE ? L : std::min(first_bad, L);  // the lines whose CIGAR check comes before any bad head
    if (!occ.empty()) {
      up(d_occ, occ.data(), occ.size() * 4);
      up(d_pid, id.data(), id.size() * 4);
    }
    timing.mark(3, s);
    if (!occ.empty()) paf_patch_kernel<<<cdiv(occ.size(), 256), 256, 0, s>>>(d_occ.as<uint32_t>(), d_pid.as<uint32_t>(), (uint32_t)occ.size(), n_occ, d_ids.as<uint32_t>());
    n_ops = 0;
    if (Lc) {
      prims::grow(d_boff, (size_t)L * 8);
      prims::grow(d_blen, (size_t)L * 4);
      prims::grow(d_ccnt, (size_t)L * 4);
      prims::grow(d_coff, (size_t)L * 8);
      IMPG_HIP(hipMemsetAsync(d_bad.p, 0, 4, s));
      paf_spans_kernel<<<cdiv(Lc, 256), 256, 0, s>>>(d_cg_at.as<uint32_t>(), d_cg_end.as<uint32_t>(), Lc, d_boff.as<u64>(), d_blen.as<uint32_t>());
      cigar_count_launch(d_text.as<char>(), d_boff.as<u64>(), d_blen.as<uint32_t>(), Lc, d_ccnt.as<uint32_t>(), d_bad.as<uint32_t>(), s);
      prims::exclusive_sum(d_tmp, d_ccnt.as<uint32_t>(), d_coff.as<u64>(), (size_t)Lc, s);
      paf_ops_total_kernel<<<1, 1, 0, s>>>(d_ccnt.as<uint32_t>(), d_coff.as<u64>(), Lc, d_bad.as<uint32_t>(), d_sum.as<Summary>());
      IMPG_HIP(hipGetLastError());
      const Summary sm = summary();
      if (sm.cigar_bad) return LINE_CIGAR;
      n_ops = sm.n_ops;
    }
    if (first_bad != NONE) {
      Head h;
      IMPG_HIP(hipMemcpy(&h, d_heads.as<Head>() + Lc, sizeof h, hipMemcpyDeviceToHost));
      return h.err ? h.err : (uint32_t)LINE_FIELDS;
    }
    if (n_ops > 2u * n) throw Error{IMPG_E_HIP, "internal: PAF ingest counted more ops than the piece has bytes"};
    if (make_room(d_pool, pool_cap, pool_used, n_ops, 4, true)) pool_regrows++;
    make_room(d_rec, rec_cap, rec_used, L, sizeof(impg_gpu_record_t), false);
    cigar_tokens_launch(d_text.as<char>(), d_boff.as<u64>(), d_blen.as<uint32_t>(), L, d_coff.as<u64>(), d_pool.as<uint32_t>() + pool_used, s);
    paf_records_kernel<<<cdiv(L, 256), 256, 0, s>>>(d_heads.as<Head>(), d_ids.as<uint32_t>(), d_ccnt.as<uint32_t>(), d_coff.as<u64>(), L, pool_used,
                                                   d_rec.as<impg_gpu_record_t>() + rec_used, d_sum.as<Summary>());
    IMPG_HIP(hipGetLastError());
    timing.mark(4, s);
    const Summary sm = summary();  // (the text is dead from here on: the next piece may overwrite it)
    timing.add(3, 3, 4);
    if (sm.internal) throw Error{IMPG_E_HIP, "internal: PAF ingest left a name without an id"};
    pool_used += n_ops;
    rec_used += L;
    return LINE_OK;
  }
  void end() override { wait(); }
  void records_home(std::vector<impg_gpu_record_t> &out) {
    out.resize((size_t)rec_used);
    if (rec_used) IMPG_HIP(hipMemcpy(out.data(), d_rec.p, (size_t)rec_used * sizeof(impg_gpu_record_t), hipMemcpyDeviceToHost));
  }
};

void require(int device) {
  int k = 0;
  if (hipGetDeviceCount(&k) != hipSuccess || k <= 0) throw Error{IMPG_E_HIP, "no HIP device available (libimpg_gpu has no CPU fallback)"};
  if (device < 0 || device >= k) throw Error{IMPG_E_INVALID, "device ordinal out of range"};
}

}  // namespace

void paf_ingest_selftest_device(const std::vector<std::string> &paths, size_t piece_bytes, int device, unsigned hash_bits, uint64_t pool_ops,
                                paf_ingest::Loaded &L, std::vector<impg_gpu_record_t> &records, std::vector<uint32_t> &ops) {
  require(device);
  DeviceBackend B(device);
  paf_ingest::load_files(B, paths, piece_bytes, hash_bits, pool_ops, L);
  B.records_home(records);
  ops.resize((size_t)B.pool_used);
  if (B.pool_used) IMPG_HIP(hipMemcpy(ops.data(), B.d_pool.p, (size_t)B.pool_used * 4, hipMemcpyDeviceToHost));
}

void paf_ingest_device(const std::vector<std::string> &paths, size_t piece_bytes, int device, paf_ingest::Loaded &L,
                       std::vector<impg_gpu_record_t> &records, DevBuf &d_ops) {
  require(device);
  DeviceBackend B(device);
  paf_ingest::load_files(B, paths, piece_bytes, 64, build_switches().paf_pool_ops, L);
  B.records_home(records);
  d_ops.adopt(B.d_pool);
}

}  // namespace impg
