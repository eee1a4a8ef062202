// M ops resolved against the sequences, in HBM (cigar_resolve.hpp).  Two passes over the same items,
// count then write, so that the new pool is allocated at its size.  No lane's and no wave's work grows with an op's length:
//   ops     gather_kernel   a lane per op: its record (a search in the records' first ops), its word, its deltas; one scan
//                           of the deltas gives every op its place in its record and every record its sums (flags_kernel)
//   items   items_kernel    an '=', 'X' or 'M' op of a resolvable record is cut into tiles of `tile` bases, every other op
//                           is one item; a scan of the counts numbers the items
//   count   tile_kernel<0>  a wave per item.  A tile's positions are compared 64 at a time, coalesced on both spans (the
//                           '-' strand descending and complemented in registers), and balloted: lane c keeps the mask of
//                           chunk c.  A run belongs to the tile it STARTS in -- position 0 of the op, or a class unlike
//                           the position before, which for a tile's first position the wave reads itself -- so the
//                           number of runs a tile writes depends on no other tile
//   scans                   the runs before every item, and for every tile (lead, through): the positions in front of
//                           its first start and whether it has none.  F[i] = lead[i] + (through[i] ? F[i + 1] : 0) is
//                           what tile i - 1's last run gains behind its tile: the associative summary of paf_device.inc's
//                           merged elements, scanned from the back (the summaries are stored back to front).  An op's
//                           first tile starts a run at 0 and every other item has (0, no): no chain crosses an op border
//   write   tile_kernel<1>  the same masks again; every start writes its op, its length ending at the next start of the
//                           tile or, for the tile's last, at the tile's end + F[i + 1]
// '=' and 'X' ops are tiled alike for the check (bad_eq_bases / bad_x_bases); their first tile copies the op.
#include "cigar_resolve.hpp"
#include "device_prims.hpp"

namespace impg {
namespace cigar_resolve {
using prims::cdiv;

namespace {
typedef unsigned long long u64;
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t THROUGH = 1u << 31;
enum Stat { S_M_OPS, S_M_BASES, S_M_EQ, S_M_X, S_BAD_EQ, S_BAD_X, S_TOO_LONG, N_STATS };

struct Sum3 { u64 t, q, bad; };
struct Sum3Plus {
  __host__ __device__ Sum3 operator()(const Sum3 &a, const Sum3 &b) const { return Sum3{a.t + b.t, a.q + b.q, a.bad + b.bad}; }
};
// a = the summary of the items behind b's (the scan runs back to front)
struct LeadJoin {
  __host__ __device__ uint32_t operator()(uint32_t a, uint32_t b) const {
    return (b & THROUGH) ? ((b & ~THROUGH) + (a & ~THROUGH)) | (a & THROUGH) : b;
  }
};

struct View {  // by value to every kernel
  const impg_gpu_record_t *rec;
  const u64 *first;        // [n_rec + 1]
  uint32_t n_rec;
  u64 n_in;                // ops of all records
  uint32_t *opw, *orec;    // [n_in] an op's word and record, in record order
  uint32_t *ot, *oq;       // [n_in] target / query positions of its record in front of it (resolvable records)
  Sum3 *sum;               // [n_in] inclusive sums of the deltas over all ops
  uint8_t *flags;          // [n_rec]
  u64 *item_off;           // [n_in + 1]
  uint32_t n_items, tile;
  const uint8_t *bases;
  const u64 *seq_off;      // [n_seq] first base of a sequence in `bases`
  u64 *stats;
};

__device__ __forceinline__ u64 wave_sum(u64 v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
  for (int o = 32; o; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}

__global__ __launch_bounds__(256) void gather_kernel(View v, const uint32_t *__restrict__ pool) {
  const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
  if (j >= v.n_in) return;
  uint32_t lo = 0, hi = v.n_rec;  // the first record whose ops start behind op j
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (v.first[mid] <= j) lo = mid + 1;
    else hi = mid;
  }
  const uint32_t r = lo - 1;
  const uint32_t w = pool[v.rec[r].cigar_off + (j - v.first[r])];
  const uint32_t code = w >> 29, len = w & OP_LEN_MASK;
  v.opw[j] = w;
  v.orec[j] = r;
  v.sum[j] = Sum3{code != 2 ? len : 0u, code != 3 ? len : 0u, code > 4 ? 1u : 0u};
}

__global__ __launch_bounds__(256) void flags_kernel(View v) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= v.n_rec) return;
  const impg_gpu_record_t rc = v.rec[r];
  if (!rc.cigar_len || v.flags[r] != FLAG_OK) return;
  const u64 a = v.first[r];
  const Sum3 lo = a ? v.sum[a - 1] : Sum3{0, 0, 0}, hi = v.sum[a + rc.cigar_len - 1];
  if (hi.bad != lo.bad || hi.t - lo.t != (u64)(rc.target_end - rc.target_start) || hi.q - lo.q != (u64)(rc.query_end - rc.query_start))
    v.flags[r] = FLAG_INCONSISTENT;
}

// items of op j (the scan's sentinel at n_in: none), and its place in its record
__global__ __launch_bounds__(256) void items_kernel(View v, uint32_t *__restrict__ n_items) {
  const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
  u64 m_ops = 0, m_bases = 0;
  if (j <= v.n_in) {
    uint32_t n = 0;
    if (j < v.n_in) {
      const uint32_t w = v.opw[j], code = w >> 29, len = w & OP_LEN_MASK, r = v.orec[j];
      n = 1;
      if (v.flags[r] == FLAG_OK) {
        const u64 a = v.first[r];
        const Sum3 lo = a ? v.sum[a - 1] : Sum3{0, 0, 0}, me = v.sum[j];
        v.ot[j] = (uint32_t)(me.t - lo.t) - (code != 2 ? len : 0u);
        v.oq[j] = (uint32_t)(me.q - lo.q) - (code != 3 ? len : 0u);
        if (code <= 1 || code == 4) n = max(1u, (len + v.tile - 1) / v.tile);
        if (code == 4) { m_ops = 1; m_bases = len; }
      }
    }
    n_items[j] = n;
  }
  m_ops = wave_sum(m_ops);
  m_bases = wave_sum(m_bases);
  if ((threadIdx.x & 63) == 0 && m_ops) {
    atomicAdd(&v.stats[S_M_OPS], m_ops);
    atomicAdd(&v.stats[S_M_BASES], m_bases);
  }
}

// A wave per item.  WRITE = false: out_cnt[item] = the ops it will write, summ_rev = its (lead, through), back to front.
// WRITE = true: the ops, at out_off[item]; lead_rev = the scanned summaries.
template <bool WRITE>
__global__ __launch_bounds__(256) void tile_kernel(View v, uint32_t *__restrict__ out_cnt, uint32_t *__restrict__ summ_rev,
                                                   const u64 *__restrict__ out_off, const uint32_t *__restrict__ lead_rev,
                                                   uint32_t *__restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  const u64 item = (u64)blockIdx.x * 4u + (threadIdx.x >> 6);
  if (item >= v.n_items) return;  // (the whole wave)
  u64 lo = 0, hi = v.n_in;        // the first op whose items start behind this one
  while (lo < hi) {
    const u64 mid = lo + (hi - lo) / 2;
    if (v.item_off[mid] <= item) lo = mid + 1;
    else hi = mid;
  }
  const u64 j = lo - 1;
  const uint32_t w = v.opw[j], code = w >> 29, len = w & OP_LEN_MASK, r = v.orec[j];
  const uint32_t k = (uint32_t)(item - v.item_off[j]);
  const bool tiled = v.flags[r] == FLAG_OK && (code <= 1 || code == 4);
  if (!tiled || code <= 1 || len == 0) {  // ops that stay as they are; 0M -> 0=
    const bool writes = k == 0;
    if (WRITE) {
      if (writes && lane == 0) out[out_off[item]] = code == 4 && tiled ? 0u : w;
    } else if (lane == 0) {
      out_cnt[item] = writes ? 1u : 0u;
      summ_rev[v.n_items - 1 - item] = 0;
    }
    if (WRITE || !tiled || len == 0) return;
  }
  // ---- the tile's positions, 64 at a time: lane c keeps chunk c's mask of differing positions
  const impg_gpu_record_t rc = v.rec[r];
  const uint32_t p0 = k * v.tile, tl = min(v.tile, len - p0), nch = (tl + 63) / 64;
  const uint8_t *T = v.bases + v.seq_off[rc.target_id] + (u64)rc.target_start + v.ot[j] + p0;
  const uint8_t *Q = v.bases + v.seq_off[rc.query_id];
  const bool rev = rc.strand != 0;
  Q += rev ? (u64)rc.query_end - 1 - v.oq[j] - p0 : (u64)rc.query_start + v.oq[j] + p0;
  auto differs = [&](int64_t i) { return T[i] != (rev ? comp(Q[-i]) : Q[i]); };
  u64 xm = 0;
  for (uint32_t c0 = 0; c0 < nch; c0 += 4) {  // (four chunks' loads in flight)
    bool d[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
      const uint32_t i = (c0 + u) * 64 + lane;
      d[u] = i < tl && differs(i);
    }
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
      const u64 b = __ballot(d[u]);
      if (lane == c0 + u) xm = b;
    }
  }
  const uint32_t rest = tl & 63;
  const u64 vm = lane >= nch ? 0ull : (lane == nch - 1 && rest) ? (1ull << rest) - 1 : ~0ull;
  if (code <= 1) {  // (count pass) the check of an '=' / 'X' op
    const u64 nd = wave_sum(__popcll(xm & vm));
    if (lane == 0) {
      if (code == 0 && nd) atomicAdd(&v.stats[S_BAD_EQ], nd);
      if (code == 1 && tl - nd) atomicAdd(&v.stats[S_BAD_X], tl - nd);
    }
    return;
  }
  // ---- starts: a class unlike the position before; position 0 of the op always
  const u64 before = __shfl_up(xm, 1);
  u64 carry = lane ? before >> 63 : 0;
  if (k && lane == 0) carry = differs(-1) ? 1 : 0;
  u64 sm = (xm ^ ((xm << 1) | carry)) & vm;
  if (k == 0 && lane == 0) sm |= 1;
  const uint32_t first = wave_min(sm ? lane * 64 + (uint32_t)__builtin_ctzll(sm) : NONE);
  if (!WRITE) {
    const u64 n = wave_sum(__popcll(sm)), nx = wave_sum(__popcll(xm & vm));
    if (lane == 0) {
      out_cnt[item] = (uint32_t)n;
      summ_rev[v.n_items - 1 - item] = first == NONE ? tl | THROUGH : first;
      if (nx) atomicAdd(&v.stats[S_M_X], nx);
      if (tl - nx) atomicAdd(&v.stats[S_M_EQ], tl - nx);
    }
    return;
  }
  uint32_t pre = __popcll(sm);  // starts in the chunks in front of this lane's
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(pre, o);
    if ((int)lane >= o) pre += t;
  }
  pre -= __popcll(sm);
  uint32_t nxt = sm ? lane * 64 + (uint32_t)__builtin_ctzll(sm) : NONE;  // the first start in the chunks behind it
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_down(nxt, o);
    if ((int)lane + o < 64) nxt = min(nxt, t);
  }
  nxt = __shfl_down(nxt, 1);
  if (lane == 63) nxt = NONE;
  const uint32_t gain = item + 1 < v.n_items ? lead_rev[v.n_items - 2 - item] & ~THROUGH : 0u;
  const uint32_t tile_end = tl + gain;
  const u64 base = out_off[item];
  for (uint32_t c = 0; c < nch; c++) {
    const u64 S = __shfl(sm, c), X = __shfl(xm, c);
    const uint32_t behind = __shfl(nxt, c), at = __shfl(pre, c);
    if (!((S >> lane) & 1)) continue;
    const uint32_t p = c * 64 + lane;
    const u64 higher = (S >> lane) >> 1;
    const uint32_t next = higher ? p + 1 + (uint32_t)__builtin_ctzll(higher) : behind == NONE ? tile_end : behind;
    out[base + at + __popcll(S & ((1ull << lane) - 1))] = ((uint32_t)((X >> lane) & 1) << 29) | (next - p);
  }
}

__global__ __launch_bounds__(256) void records_kernel(View v, const u64 *__restrict__ out_off, u64 *__restrict__ new_off, uint32_t *__restrict__ new_len) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= v.n_rec) return;
  const u64 a = out_off[v.item_off[v.first[r]]], b = out_off[v.item_off[v.first[r] + v.rec[r].cigar_len]];
  new_off[r] = a;
  new_len[r] = (uint32_t)min(b - a, (u64)NONE);
  if (b - a > OP_LEN_MASK) atomicAdd(&v.stats[S_TOO_LONG], 1ull);
}

}  // namespace

void resolve_device(const impg_gpu_record_t *records, size_t n_records, const uint32_t *d_ops, size_t n_ops, const Plan &plan, const SeqStore &st,
                    uint32_t tile_bases, int device, Result &r, DevBuf &d_out) {
  const uint32_t tile = tile_bases ? tile_bases : TILE_BASES;
  if (tile % 64 || tile > TILE_BASES_MAX) throw Error{IMPG_E_INVALID, "tile_bases is 0 or a multiple of 64 up to 4096"};
  if (n_records >= (1ull << 31)) throw Error{IMPG_E_UNSUPPORTED, "more than 2^31 records in one index"};
  r = Result{};
  r.off.assign(n_records, 0);
  r.len.assign(n_records, 0);
  r.flags = plan.pre;
  const u64 n_in = plan.first[n_records];
  d_out.reserve(256);
  if (!n_in) { finish(records, n_records, r); return; }
  IMPG_HIP(hipSetDevice(device));
  hipStream_t s = nullptr;
  size_t free_b = 0, total_b = 0;
  IMPG_HIP(hipMemGetInfo(&free_b, &total_b));
  const auto t_begin = std::chrono::steady_clock::now();
  // the store's sequences that the table names, back to back behind SEQ_PAD bytes
  const size_t n_store = st.names.size();
  std::vector<uint8_t> used(n_store, 0);
  for (uint32_t s_of : plan.store_of_id) if (s_of != SEQ_ABSENT) used[s_of] = 1;
  std::vector<u64> dev_off(n_store, 0);
  u64 store_bytes = SEQ_PAD;
  for (size_t i = 0; i < n_store; i++)
    if (used[i]) { dev_off[i] = store_bytes; store_bytes += st.off[i + 1] - st.off[i]; }
  store_bytes += SEQ_PAD;
  u64 wanted = (u64)n_ops * 4;  // (the pool the caller brought)
  auto take = [&](DevBuf &b, u64 bytes, const char *what) {
    wanted += bytes;
    if (bytes > free_b || wanted - (u64)n_ops * 4 > free_b)
      throw Error{IMPG_E_OOM, std::string("cigar resolve: the sequences, both op pools and the pass's arrays want ") + std::to_string(wanted) +
                                  " bytes of HBM (at " + what + "); " + std::to_string(free_b + (u64)n_ops * 4) + " are there"};
    b.reserve(std::max<size_t>((size_t)bytes, 256));
  };
  DevBuf d_bases, d_seq_off, d_rec, d_first, d_flags, d_opw, d_orec, d_ot, d_oq, d_sum, d_nitems, d_item_off, d_stats, tmp;
  take(d_bases, store_bytes, "the sequences");
  IMPG_HIP(hipMemsetAsync(d_bases.p, 0, SEQ_PAD, s));
  IMPG_HIP(hipMemsetAsync(d_bases.as<uint8_t>() + store_bytes - SEQ_PAD, 0, SEQ_PAD, s));
  for (size_t i = 0; i < n_store;) {
    if (!used[i]) { i++; continue; }
    size_t e = i;
    while (e < n_store && used[e]) e++;
    if (st.off[e] > st.off[i])
      IMPG_HIP(hipMemcpyAsync(d_bases.as<uint8_t>() + dev_off[i], st.bases.data() + st.off[i], st.off[e] - st.off[i], hipMemcpyHostToDevice, s));
    i = e;
  }
  std::vector<u64> seq_off(plan.store_of_id.size());
  for (size_t id = 0; id < seq_off.size(); id++) seq_off[id] = plan.store_of_id[id] == SEQ_ABSENT ? SEQ_NOT_IN_HBM : dev_off[plan.store_of_id[id]];
  take(d_seq_off, seq_off.size() * 8, "the sequence table");
  take(d_rec, n_records * sizeof(impg_gpu_record_t), "the records");
  take(d_first, (n_records + 1) * 8, "the records");
  take(d_flags, n_records, "the records");
  take(d_stats, N_STATS * 8, "the report");
  if (!seq_off.empty()) IMPG_HIP(hipMemcpyAsync(d_seq_off.p, seq_off.data(), seq_off.size() * 8, hipMemcpyHostToDevice, s));
  IMPG_HIP(hipMemcpyAsync(d_rec.p, records, n_records * sizeof(impg_gpu_record_t), hipMemcpyHostToDevice, s));
  IMPG_HIP(hipMemcpyAsync(d_first.p, plan.first.data(), (n_records + 1) * 8, hipMemcpyHostToDevice, s));
  IMPG_HIP(hipMemcpyAsync(d_flags.p, plan.pre.data(), n_records, hipMemcpyHostToDevice, s));
  IMPG_HIP(hipMemsetAsync(d_stats.p, 0, N_STATS * 8, s));
  take(d_opw, n_in * 4, "the ops");
  take(d_orec, n_in * 4, "the ops");
  take(d_ot, n_in * 4, "the ops");
  take(d_oq, n_in * 4, "the ops");
  take(d_sum, n_in * sizeof(Sum3), "the ops");
  take(d_nitems, (n_in + 1) * 4, "the ops");
  take(d_item_off, (n_in + 1) * 8, "the ops");
  View v{};
  v.rec = d_rec.as<impg_gpu_record_t>();
  v.first = d_first.as<u64>();
  v.n_rec = (uint32_t)n_records;
  v.n_in = n_in;
  v.opw = d_opw.as<uint32_t>();
  v.orec = d_orec.as<uint32_t>();
  v.ot = d_ot.as<uint32_t>();
  v.oq = d_oq.as<uint32_t>();
  v.sum = d_sum.as<Sum3>();
  v.flags = d_flags.as<uint8_t>();
  v.item_off = d_item_off.as<u64>();
  v.tile = tile;
  v.bases = d_bases.as<uint8_t>();
  v.seq_off = d_seq_off.as<u64>();
  v.stats = d_stats.as<u64>();
  // ---- ops: record, word, place; the records' sums and flags; items
  const char *timing = getenv("IMPG_RESOLVE_TIMING");  // a file: one line per call (scripts/resolve_probe.py)
  if (timing) IMPG_HIP(hipStreamSynchronize(s));
  const auto t_kernels = std::chrono::steady_clock::now();
  gather_kernel<<<cdiv(n_in, 256), 256, 0, s>>>(v, d_ops);
  IMPG_HIP(hipGetLastError());
  prims::inclusive_scan(tmp, v.sum, v.sum, (size_t)n_in, Sum3Plus(), s);
  flags_kernel<<<cdiv(n_records, 256), 256, 0, s>>>(v);
  items_kernel<<<cdiv(n_in + 1, 256), 256, 0, s>>>(v, d_nitems.as<uint32_t>());
  IMPG_HIP(hipGetLastError());
  prims::exclusive_sum(tmp, d_nitems.as<uint32_t>(), v.item_off, (size_t)n_in + 1, s);
  u64 n_items = 0;
  IMPG_HIP(hipMemcpyAsync(&n_items, v.item_off + n_in, 8, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipMemcpyAsync(r.flags.data(), d_flags.p, n_records, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipStreamSynchronize(s));
  if (n_items >= NONE - 1) throw Error{IMPG_E_UNSUPPORTED, "cigar resolve: 2^32 op tiles in one pool"};
  v.n_items = (uint32_t)n_items;
  d_sum.release();
  d_nitems.release();
  // ---- count, the scans, the records' new ops
  DevBuf d_cnt, d_out_off, d_summ, d_lead, d_new_off, d_new_len;
  take(d_cnt, (n_items + 1) * 4, "the tiles");
  take(d_out_off, (n_items + 1) * 8, "the tiles");
  take(d_summ, n_items * 4, "the tiles");
  take(d_lead, n_items * 4, "the tiles");
  take(d_new_off, n_records * 8, "the records");
  take(d_new_len, n_records * 4, "the records");
  IMPG_HIP(hipMemsetAsync(d_cnt.as<uint32_t>() + n_items, 0, 4, s));
  tile_kernel<false><<<cdiv(n_items, 4), 256, 0, s>>>(v, d_cnt.as<uint32_t>(), d_summ.as<uint32_t>(), nullptr, nullptr, nullptr);
  IMPG_HIP(hipGetLastError());
  prims::exclusive_sum(tmp, d_cnt.as<uint32_t>(), d_out_off.as<u64>(), (size_t)n_items + 1, s);
  prims::inclusive_scan(tmp, d_summ.as<uint32_t>(), d_lead.as<uint32_t>(), (size_t)n_items, LeadJoin(), s);
  records_kernel<<<cdiv(n_records, 256), 256, 0, s>>>(v, d_out_off.as<u64>(), d_new_off.as<u64>(), d_new_len.as<uint32_t>());
  IMPG_HIP(hipGetLastError());
  u64 n_out = 0, stats[N_STATS];
  IMPG_HIP(hipMemcpyAsync(&n_out, d_out_off.as<u64>() + n_items, 8, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipMemcpyAsync(stats, d_stats.p, sizeof stats, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipMemcpyAsync(r.off.data(), d_new_off.p, n_records * 8, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipMemcpyAsync(r.len.data(), d_new_len.p, n_records * 4, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipStreamSynchronize(s));
  if (stats[S_TOO_LONG]) throw Error{IMPG_E_UNSUPPORTED, "CIGAR longer than 2^29 ops"};
  // ---- write
  d_cnt.release();
  d_summ.release();
  take(d_out, n_out * 4, "the new op pool");
  tile_kernel<true><<<cdiv(n_items, 4), 256, 0, s>>>(v, nullptr, nullptr, d_out_off.as<u64>(), d_lead.as<uint32_t>(), d_out.as<uint32_t>());
  IMPG_HIP(hipGetLastError());
  IMPG_HIP(hipStreamSynchronize(s));
  if (FILE *f = timing && *timing ? fopen(timing, "a") : nullptr) {
    const auto t_end = std::chrono::steady_clock::now();
    fprintf(f, "upload_s %.6f kernels_s %.6f items %llu ops_in %llu ops_out %llu store_bytes %llu wanted_bytes %llu\n",
            std::chrono::duration<double>(t_kernels - t_begin).count(), std::chrono::duration<double>(t_end - t_kernels).count(), n_items, n_in, n_out,
            store_bytes, wanted);
    fclose(f);
  }
  r.n_out = n_out;
  r.report.m_ops = stats[S_M_OPS];
  r.report.m_bases = stats[S_M_BASES];
  r.report.m_eq_bases = stats[S_M_EQ];
  r.report.m_x_bases = stats[S_M_X];
  r.report.bad_eq_bases = stats[S_BAD_EQ];
  r.report.bad_x_bases = stats[S_BAD_X];
  finish(records, n_records, r);
}

}  // namespace cigar_resolve
}  // namespace impg
