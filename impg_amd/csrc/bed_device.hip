// BED post-processing on the device: merge_adjusted_intervals_gap_2d (src/main.rs:12858-13011) followed by
// merge_query_adjusted_intervals (src/main.rs:12474-12560), as output_results_bed (src/main.rs:11849-11892) runs
// them for every query range -- but for all ranges of a chunk at once and on the hit slots where they lie, so that
// only merged rows cross PCIe.  bed.cpp holds the host-side implementation of the same two merges (one range at a
// time, for impg_gpu_results_bed / impg_gpu_bed_merge); the parity tests compare both with the CPU restatement of the reference.
//
//   rows      every emitted result of the chunk (self intervals, then level by level in slot order), numbered in
//             that order: within one range this is the reference's emission order, which all tie rules refer to
//   gap_2d    rows sorted by (range, query seq, target seq, strand | q.first ascending on '+', descending on '-' |
//             emission order): two stable radix sorts.  One thread per row replays the reference's inner loop over
//             the rows behind it in its group (skip strictly-backward starts, stop at the first query gap > d,
//             link when the target also moves forward by a gap <= d) and links with a lock-free union-find whose
//             root is always the smallest member, i.e. the chain's first row in emission order -- the slot the
//             reference writes the merged row to.  Boxes by atomic min / max into the root.
//   query axis rows sorted by (range, query seq | start | forward first | current order); the reference's sweep
//             merges a row into the running one while start <= running end + d.  Sorted by start, "running end" is
//             the prefix maximum of the ends inside the (range, sequence) segment: a run breaks exactly where
//             start > prefix max + d.  The merged strand is the strand of the last row whose own length exceeds the
//             span merged before it (else the run's first row's): main.rs:12535-12547 unrolled.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <string>

#include "device_prims.hpp"
#include "engine.hpp"
#include "text_device.hpp"

namespace impg {

namespace {

using prims::bits_for;
using prims::cdiv;
using prims::ord_u32;

// ---- gap_2d --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gap_keys_kernel(ConstRows R, uint32_t n, unsigned seq_bits, uint32_t *__restrict__ k32,
                                                       unsigned long long *__restrict__ k64, uint32_t *__restrict__ idx) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int4 c = R.c[i];
  const bool f = c.x <= c.y;
  k32[i] = ord_u32(f ? c.x : -c.x);  // q.first ascending on '+', descending on '-' (main.rs:12893-12901)
  k64[i] = ((((unsigned long long)R.q[i] << seq_bits | R.qid[i]) << seq_bits | R.tid[i]) << 1) | (f ? 1ull : 0ull);
  idx[i] = i;
}
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x) {
  uint32_t p = parent[x];
  while (p != x) {
    const uint32_t gp = parent[p];
    if (gp != p) parent[x] = gp;  // path halving (benign race: only ever points further up)
    x = p;
    p = parent[x];
  }
  return x;
}
__device__ __forceinline__ void uf_unite(uint32_t *parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a > b) { const uint32_t t = a; a = b; b = t; }  // the smaller index stays the root: the chain's first row in emission order
    if (atomicCAS(&parent[b], b, a) == b) return;
  }
}
// one thread per sorted position a: the reference's loop over b > a inside a's group (main.rs:12925-12960)
__global__ __launch_bounds__(256) void gap_link_kernel(ConstRows R, const uint32_t *__restrict__ perm, const unsigned long long *__restrict__ skey,
                                                       uint32_t n, int32_t merge_distance, uint32_t *__restrict__ parent) {
  const uint32_t a = blockIdx.x * 256u + threadIdx.x;
  if (a >= n) return;
  const unsigned long long ka = skey[a];
  const bool f = (ka & 1ull) != 0;
  const uint32_t ia = perm[a];
  const int4 A = R.c[ia];
  const long long d = merge_distance;
  const long long qa_start = f ? A.x : A.y, qa_end = f ? A.y : A.x;
  for (uint32_t b = a + 1; b < n && skey[b] == ka; b++) {
    const uint32_t ib = perm[b];
    const int4 B = R.c[ib];
    const long long qb_start = f ? B.x : B.y;
    if (qb_start < qa_start) continue;  // strictly-backward start
    if (qb_start - qa_end > d) break;   // query gap too large: later rows of the group are not tried
    const long long t_gap = f ? (long long)B.z - A.w : (long long)A.z - B.w;
    const bool t_forward = f ? B.z > A.z : B.w < A.w;
    if (t_forward && t_gap <= d) uf_unite(parent, ia, ib);
  }
}
// the chain's bounding box, gathered at its root (the box itself is order-independent)
__global__ __launch_bounds__(256) void gap_box_kernel(ConstRows R, uint32_t n, uint32_t *__restrict__ parent, int4 *__restrict__ box,
                                                      uint32_t *__restrict__ is_root) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = uf_find(parent, i);
  is_root[i] = r == i ? 1u : 0u;
  if (r == i) return;
  const int4 c = R.c[i];
  const bool f = c.x <= c.y;  // (a chain never mixes strands)
  int *b = reinterpret_cast<int *>(box + r);
  if (f) { atomicMin(b + 0, c.x); atomicMax(b + 1, c.y); } else { atomicMax(b + 0, c.x); atomicMin(b + 1, c.y); }
  atomicMin(b + 2, c.z);
  atomicMax(b + 3, c.w);
}
__global__ __launch_bounds__(256) void compact_rows_kernel(ConstRows in, const int4 *__restrict__ box, uint32_t n, const uint32_t *__restrict__ flag,
                                                           const uint32_t *__restrict__ pos, Rows out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const uint32_t d = pos[i];
  out.q[d] = in.q[i]; out.qid[d] = in.qid[i]; out.tid[d] = in.tid[i];
  out.c[d] = box[i];
}

// ---- query axis ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void axis_keys_kernel(ConstRows R, uint32_t n, unsigned seq_bits, unsigned long long *__restrict__ k_lo,
                                                        unsigned long long *__restrict__ k_hi, uint32_t *__restrict__ idx) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int4 c = R.c[i];
  const bool f = c.x <= c.y;
  k_lo[i] = ((unsigned long long)ord_u32(min(c.x, c.y)) << 1) | (f ? 0ull : 1ull);  // start, forward first (main.rs:12486-12499)
  k_hi[i] = ((unsigned long long)R.q[i] << seq_bits) | R.qid[i];
  idx[i] = i;
}
// per sorted row: (segment id << 32 | end) for the prefix maximum; a segment = one (range, query sequence) [+ strand
// run when the strands stay apart]
__global__ __launch_bounds__(256) void axis_seg_kernel(ConstRows R, const uint32_t *__restrict__ perm, const unsigned long long *__restrict__ skey,
                                                       uint32_t n, int merge_strands, uint32_t *__restrict__ seg_head) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  bool head = k == 0 || skey[k] != skey[k - 1];
  if (!head && !merge_strands) {
    const int4 a = R.c[perm[k - 1]], b = R.c[perm[k]];
    head = (a.x <= a.y) != (b.x <= b.y);
  }
  seg_head[k] = head ? 1u : 0u;
}
__global__ __launch_bounds__(256) void axis_val_kernel(ConstRows R, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ seg_head,
                                                       const uint32_t *__restrict__ seg_id, uint32_t n, unsigned long long *__restrict__ val) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const int4 c = R.c[perm[k]];
  val[k] = ((unsigned long long)(seg_id[k] + seg_head[k]) << 32) | ord_u32(max(c.x, c.y));  // (exclusive scan + own flag = 1-based id)
}
__global__ __launch_bounds__(256) void axis_run_heads_kernel(ConstRows R, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ seg_head,
                                                             const unsigned long long *__restrict__ pmax, uint32_t n, int32_t merge_distance,
                                                             uint32_t *__restrict__ run_head) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  bool head = seg_head[k] != 0 || merge_distance < 0;  // main.rs:12515: a negative distance keeps everything apart
  if (!head) {
    const int4 c = R.c[perm[k]];
    const int32_t ns = min(c.x, c.y);
    const uint32_t ce = (uint32_t)(pmax[k - 1] & 0xFFFFFFFFull) ^ 0x80000000u;
    // main.rs:12523 adds in i32 and the reference's release build wraps: the sum is taken unsigned and read back signed
    head = ns > (int32_t)(ce + (uint32_t)merge_distance);
  }
  run_head[k] = head ? 1u : 0u;
}
// one thread per sorted row; run r = run_id[k] (exclusive scan of the heads + own flag - 1)
__global__ __launch_bounds__(256) void axis_emit_kernel(ConstRows R, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ run_head,
                                                        const uint32_t *__restrict__ run_pos, const unsigned long long *__restrict__ pmax,
                                                        const uint32_t *__restrict__ head_of, uint32_t n, int merge_strands,
                                                        BedRow *__restrict__ out, uint32_t *__restrict__ strand_key) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint32_t run = run_pos[k] + run_head[k] - 1u;
  const uint32_t i = perm[k];
  const int4 c = R.c[i];
  const bool f = c.x <= c.y;
  const int32_t ns = min(c.x, c.y), ne = max(c.x, c.y);
  const bool tail = k + 1 == n || run_head[k + 1] != 0;
  if (run_head[k]) {
    out[run].q_strand = R.q[i];
    out[run].query_id = R.qid[i];
    out[run].start = ns;
    atomicMax(&strand_key[run], (1u << 1) | (f ? 0u : 1u));  // position 0 of the run: the fallback strand
  } else if (merge_strands) {
    // the merged strand follows the last row whose own length exceeds the span merged before it (main.rs:12535-12547)
    const long long ce_prev = (long long)(int32_t)((uint32_t)(pmax[k - 1] & 0xFFFFFFFFull) ^ 0x80000000u);
    // the span merged so far starts at the run's head (rows of a run are sorted by start): head_of[k] = its position,
    // a prefix maximum over the head positions
    const uint32_t h = head_of[k];
    const int4 hc = R.c[perm[h]];
    const long long cs = min(hc.x, hc.y);
    if ((long long)ne - ns > ce_prev - cs) atomicMax(&strand_key[run], ((k - h + 1u) << 1) | (f ? 0u : 1u));
  }
  if (tail) {
    // (a run that is a single row ends where the row ends: with a negative distance every row is its own run and the
    // prefix maximum, which runs over the whole segment, is not the row's end)
    const int32_t ce = run_head[k] ? ne : (int32_t)((uint32_t)(pmax[k] & 0xFFFFFFFFull) ^ 0x80000000u);
    out[run].end = ce;  // (the strand is filled in by axis_strand_kernel)
  }
}
__global__ __launch_bounds__(256) void head_pos_kernel(const uint32_t *__restrict__ run_head, uint32_t n, uint32_t *__restrict__ v) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k < n) v[k] = run_head[k] ? k : 0u;
}
__global__ __launch_bounds__(256) void axis_strand_kernel(BedRow *__restrict__ out, const uint32_t *__restrict__ strand_key, uint32_t n_runs) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r < n_runs) out[r].q_strand |= (strand_key[r] & 1u) << 31;
}

}  // namespace

// ---- text ---------------------------------------------------------------------------------------------------------------
// "{name}\t{start}\t{end}\t{range name}\t.\t{strand}\n" per merged row (output_results_bed, main.rs:11868-11890), written
// by the device: a transitive batch prints gigabytes, which the host's cores format slower than PCIe moves them.
__global__ __launch_bounds__(256) void text_len_kernel(const BedRow *__restrict__ rows, uint32_t n, TextTables t, uint32_t *__restrict__ len) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const BedRow x = rows[r];
  const uint32_t sh = seq_shift(t, x.query_id);
  const uint32_t q = x.q_strand & 0x7FFFFFFFu;
  len[r] = seq_text_len(t, x.query_id) + dec_digits((uint32_t)x.start + sh) + dec_digits((uint32_t)x.end + sh) + (t.rname_off[q + 1] - t.rname_off[q]) + 8u;
}
__global__ __launch_bounds__(256) void text_write_kernel(const BedRow *__restrict__ rows, uint32_t n, TextTables t,
                                                         const unsigned long long *__restrict__ off, unsigned long long base, char *__restrict__ out) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const BedRow x = rows[r];
  char *p = out + (off[r] - base);
  const uint32_t sh = seq_shift(t, x.query_id);
  const uint32_t a = (uint32_t)x.start + sh, b = (uint32_t)x.end + sh;
  p = put_seq(p, t, x.query_id); *p++ = '\t';
  p = put_dec(p, a, dec_digits(a)); *p++ = '\t';
  p = put_dec(p, b, dec_digits(b)); *p++ = '\t';
  p = put_range_name(p, t, x.q_strand & 0x7FFFFFFFu);
  *p++ = '\t'; *p++ = '.'; *p++ = '\t';
  *p++ = (x.q_strand >> 31) ? '-' : '+';
  *p++ = '\n';
}

typedef unsigned long long u64;

// The rows' chains (gap_2d): n > 1 rows -> one row per chain in `to`, the chain's box where its first row stood; returns
// their number.  ks.perm, k32, k64: n words each.
static uint32_t gap_2d(Engine &E, ConstRows R, uint32_t n, unsigned seq_bits, unsigned q_bits, int32_t merge_distance, prims::KeySort &ks,
                       DevBuf &k32, DevBuf &k64, DevRows &to) {
  hipStream_t s = E.stream;
  gap_keys_kernel<<<cdiv(n, 256), 256, 0, s>>>(R, n, seq_bits, k32.as<uint32_t>(), k64.as<u64>(), ks.perm.as<uint32_t>());
  ks.run({{k32.p, false, 32}, {k64.p, true, q_bits + 2 * seq_bits + 1}}, /*first_in_order=*/true, n, s);
  DevBuf parent, box, root_flag, root_pos;
  parent.reserve((size_t)n * 4); box.reserve((size_t)n * 16); root_flag.reserve((size_t)n * 4); root_pos.reserve((size_t)n * 4);
  prims::iota_kernel<<<cdiv(n, 256), 256, 0, s>>>(parent.as<uint32_t>(), n);
  gap_link_kernel<<<cdiv(n, 256), 256, 0, s>>>(R, ks.order, (const u64 *)ks.sorted_keys, n, merge_distance, parent.as<uint32_t>());
  IMPG_HIP(hipMemcpyAsync(box.p, R.c, (size_t)n * 16, hipMemcpyDeviceToDevice, s));
  gap_box_kernel<<<cdiv(n, 256), 256, 0, s>>>(R, n, parent.as<uint32_t>(), box.as<int4>(), root_flag.as<uint32_t>());
  const uint32_t m = (uint32_t)E.scan(root_flag.as<uint32_t>(), root_pos.as<uint32_t>(), n);
  to.reserve(m, 256);
  compact_rows_kernel<<<cdiv(n, 256), 256, 0, s>>>(R, box.as<int4>(), n, root_flag.as<uint32_t>(), root_pos.as<uint32_t>(), to.view());
  return m;
}

// The sweep along the query axis: m rows -> their runs as BedRows in `out`, grouped by range; returns their number.
// ks.perm, k_lo, k_hi: m words each.  The stream is synchronised when this returns.
static uint32_t query_axis(Engine &E, ConstRows R, uint32_t m, unsigned seq_bits, unsigned q_bits, int32_t merge_distance, bool merge_strands,
                           prims::KeySort &ks, DevBuf &k_lo, DevBuf &k_hi, DevBuf &out) {
  hipStream_t s = E.stream;
  DevBuf kq, seg_head, seg_id, val, pmax, run_head, run_pos, head_of, strand_key, stmp;  // (stmp: the two prefix maxima's temp storage)
  const size_t mb4 = (size_t)m * 4, mb8 = (size_t)m * 8;
  seg_head.reserve(mb4); seg_id.reserve(mb4); pmax.reserve(mb8); run_head.reserve(mb4); run_pos.reserve(mb4);
  out.reserve((size_t)m * sizeof(BedRow) + 256);
  // (besides the sweep's keys this lists the rows in ks.perm, which is all the branch without a sweep takes from it)
  axis_keys_kernel<<<cdiv(m, 256), 256, 0, s>>>(R, m, seq_bits, k_lo.as<u64>(), k_hi.as<u64>(), ks.perm.as<uint32_t>());
  // (main.rs:12479: the sweep runs when a range has more than one row and (d >= 0 or strands merge); a range with one
  // row is its own run either way, so running it for every range changes nothing)
  if (merge_distance >= 0 || merge_strands) {
    ks.run({{k_lo.p, true, 33}, {k_hi.p, true, q_bits + seq_bits}}, /*first_in_order=*/true, m, s);
    val.reserve(mb8);
    axis_seg_kernel<<<cdiv(m, 256), 256, 0, s>>>(R, ks.order, (const u64 *)ks.sorted_keys, m, merge_strands ? 1 : 0, seg_head.as<uint32_t>());
    (void)E.scan(seg_head.as<uint32_t>(), seg_id.as<uint32_t>(), m);
    axis_val_kernel<<<cdiv(m, 256), 256, 0, s>>>(R, ks.order, seg_head.as<uint32_t>(), seg_id.as<uint32_t>(), m, val.as<u64>());
    prims::inclusive_max(stmp, val.as<u64>(), pmax.as<u64>(), m, s);
    axis_run_heads_kernel<<<cdiv(m, 256), 256, 0, s>>>(R, ks.order, seg_head.as<uint32_t>(), pmax.as<u64>(), m, merge_distance, run_head.as<uint32_t>());
  } else {
    // no merging at all: the rows as they are, sorted by range only (stable: emission order within a range), each its own
    // run -- one segment, and a negative distance keeps everything apart
    kq.reserve(mb4);
    IMPG_HIP(hipMemcpyAsync(kq.p, R.q, mb4, hipMemcpyDeviceToDevice, s));
    ks.run({{kq.p, false, q_bits}}, /*first_in_order=*/true, m, s);
    IMPG_HIP(hipMemsetAsync(seg_head.p, 0, mb4, s));
    IMPG_HIP(hipMemsetAsync(seg_id.p, 0, mb4, s));
    axis_val_kernel<<<cdiv(m, 256), 256, 0, s>>>(R, ks.order, seg_head.as<uint32_t>(), seg_id.as<uint32_t>(), m, pmax.as<u64>());
    axis_run_heads_kernel<<<cdiv(m, 256), 256, 0, s>>>(R, ks.order, seg_head.as<uint32_t>(), pmax.as<u64>(), m, -1, run_head.as<uint32_t>());
  }
  const uint32_t n_runs = (uint32_t)E.scan(run_head.as<uint32_t>(), run_pos.as<uint32_t>(), m);
  strand_key.reserve((size_t)n_runs * 4 + 256);
  IMPG_HIP(hipMemsetAsync(strand_key.p, 0, (size_t)n_runs * 4, s));
  if (merge_strands) {
    head_of.reserve(mb4);
    head_pos_kernel<<<cdiv(m, 256), 256, 0, s>>>(run_head.as<uint32_t>(), m, seg_id.as<uint32_t>());
    prims::inclusive_max(stmp, seg_id.as<uint32_t>(), head_of.as<uint32_t>(), m, s);
  }
  axis_emit_kernel<<<cdiv(m, 256), 256, 0, s>>>(R, ks.order, run_head.as<uint32_t>(), run_pos.as<uint32_t>(), pmax.as<u64>(), head_of.as<uint32_t>(), m,
                                                 merge_strands ? 1 : 0, out.as<BedRow>(), strand_key.as<uint32_t>());
  axis_strand_kernel<<<cdiv(n_runs, 256), 256, 0, s>>>(out.as<BedRow>(), strand_key.as<uint32_t>(), n_runs);
  IMPG_HIP(hipStreamSynchronize(s));  // (the scratch buffers of this function die here)
  return n_runs;
}

// Scattered rows -> merged BED rows, left on the device in `out` (grouped by range, in output order); returns their
// number.  R: n rows numbered in emission order (within a range: the reference's; rows of different ranges may
// interleave), ids < n_seq, range indices < n_ranges.  Counts into the handle's bed_* counters.  gap (diagnostics):
// the rows between the two merges, copied to the host in their order -- a chain stands where its first row stood.
// bed = false (FASTA, output_results_fasta: main.rs:12362): the sweep along the query axis alone, no gap_2d before it,
// and the bed_* counters stay as they are.
static uint32_t merge_rows(Engine &E, const impg_gpu_index &ix, Rows R, uint32_t n, uint64_t n_seq, uint32_t n_ranges, int32_t merge_distance,
                           bool merge_strands, DevBuf &out, BedGapRows *gap = nullptr, bool bed = true) {
  hipStream_t s = E.stream;
  const unsigned seq_bits = bits_for(n_seq), q_bits = bits_for(n_ranges);
  // (with no merge at all the rows are only grouped by range: no key holds a sequence id)
  if ((merge_distance >= 0 || merge_strands) && q_bits + 2 * seq_bits + 1 > 64) throw Error{IMPG_E_UNSUPPORTED, "too many sequences for the device-side BED merge (use impg_gpu_results_bed)"};
  prims::KeySort ks;
  DevBuf k32, k64a, k64b;  // the sorts' keys, at the rows' own indices
  ks.perm.reserve((size_t)n * 4); k32.reserve((size_t)n * 4); k64a.reserve((size_t)n * 8); k64b.reserve((size_t)n * 8);
  DevRows chains;
  Rows cur = R;
  uint32_t m = n;
  if (bed && merge_distance >= 0 && n > 1) {
    m = gap_2d(E, R, n, seq_bits, q_bits, merge_distance, ks, k32, k64a, chains);
    cur = chains.view();
  }
  if (gap) {
    std::vector<uint32_t> hq(m), hqid(m), htid(m);
    std::vector<int4> hc(m);
    IMPG_HIP(hipMemcpyAsync(hq.data(), cur.q, (size_t)m * 4, hipMemcpyDeviceToHost, s));
    IMPG_HIP(hipMemcpyAsync(hqid.data(), cur.qid, (size_t)m * 4, hipMemcpyDeviceToHost, s));
    IMPG_HIP(hipMemcpyAsync(htid.data(), cur.tid, (size_t)m * 4, hipMemcpyDeviceToHost, s));
    IMPG_HIP(hipMemcpyAsync(hc.data(), cur.c, (size_t)m * 16, hipMemcpyDeviceToHost, s));
    IMPG_HIP(hipStreamSynchronize(s));
    gap->range = hq;
    gap->rows.resize(m);
    for (uint32_t i = 0; i < m; i++) gap->rows[i] = impg_gpu_interval_t{hqid[i], hc[i].x, hc[i].y, htid[i], hc[i].z, hc[i].w};
  }
  const uint32_t n_runs = query_axis(E, cur, m, seq_bits, q_bits, merge_distance, merge_strands, ks, k64a, k64b, out);
  if (!bed) return n_runs;
  ix.bed_stats[BED_ROWS] += n;
  ix.bed_stats[BED_GAP_ROOTS] += m;
  ix.bed_stats[BED_RUNS] += n_runs;
  return n_runs;
}

// Rows of one chunk -> merged BED rows (merge_rows).  levels / self_dev: what Engine::run kept for the chunk.
// fasta_rows_in (FASTA): the rows go through the sweep alone, strands apart (merge_rows with bed = false); their number
// before it is left there.
static uint32_t chunk_rows_merged(Engine &E, const impg_gpu_index &ix, uint32_t n_ranges, const impg_gpu_params_t &p, int32_t merge_distance,
                                  std::vector<std::unique_ptr<LevelBufs>> &levels, DevBuf &self_dev, DevBuf &out, uint32_t *fasta_rows_in) {
  // ---- rows: range-major, the reference's emission order within a range (rows_device.hip) ---------------------------
  uint32_t n = 0;
  DevRows rows;
  {
    RowPlan pl;  // (its tables go back to the pool at the end of this block, before the sorts take their memory)
    plan_rows(E, n_ranges, p, levels, self_dev, /*plain_retain=*/true, pl);
    n = pl.n_rows;
    if (!n) return 0;
    rows.reserve(n);
    scatter_rows(E, levels, pl, rows.sinks());
    IMPG_HIP(hipStreamSynchronize(E.stream));
  }
  // the levels' slots are not needed any more: give their memory back before the sorts take theirs
  levels.clear();
  if (fasta_rows_in) {
    *fasta_rows_in = n;
    return merge_rows(E, ix, rows.view(), n, ix.view.n_seq, n_ranges, merge_distance, /*merge_strands=*/false, out, nullptr, /*bed=*/false);
  }
  return merge_rows(E, ix, rows.view(), n, ix.view.n_seq, n_ranges, merge_distance, p.consider_strandness == 0, out);
}

uint32_t device_bed_rows(Engine &E, const impg_gpu_index &ix, uint32_t n_ranges, const impg_gpu_params_t &p, int32_t merge_distance,
                         std::vector<std::unique_ptr<LevelBufs>> &levels, DevBuf &self_dev, DevBuf &out) {
  return chunk_rows_merged(E, ix, n_ranges, p, merge_distance, levels, self_dev, out, nullptr);
}
uint32_t device_fasta_rows(Engine &E, const impg_gpu_index &ix, uint32_t n_ranges, const impg_gpu_params_t &p, int32_t merge_distance,
                           std::vector<std::unique_ptr<LevelBufs>> &levels, DevBuf &self_dev, DevBuf &out, uint32_t &rows_in) {
  rows_in = 0;
  return chunk_rows_merged(E, ix, n_ranges, p, merge_distance, levels, self_dev, out, &rows_in);
}

// The FASTA sweep on rows the caller brings (impg_gpu_selftest_fasta_rows): uploaded as they are, then merge_rows as a
// chunk of impg_gpu_query_batch_fasta runs it; returns the merged rows' number, the rows in `out`.
uint32_t device_fasta_selftest_rows(Engine &E, const impg_gpu_index &ix, const impg_gpu_interval_t *rows, const uint32_t *row_range, uint32_t n,
                                    uint32_t n_ranges, int32_t merge_distance, DevBuf &out) {
  if (!n) return 0;
  DevRows dev;
  dev.upload(E, rows, row_range, n);
  return merge_rows(E, ix, dev.view(), n, ix.view.n_seq, n_ranges, merge_distance, /*merge_strands=*/false, out, nullptr, /*bed=*/false);
}

// The merge and the text on rows the caller brings (impg_gpu_selftest_bed_rows): uploaded as they are, then merge_rows
// and device_bed_text as a chunk of a query runs them.  merged: the rows as the device left them; text: appended to.
void device_bed_selftest(Engine &E, const impg_gpu_index &ix, const impg_gpu_interval_t *rows, const uint32_t *row_range, uint32_t n,
                         uint32_t n_ranges, uint64_t n_seq, int32_t merge_distance, bool merge_strands, bool original_coords,
                         const std::vector<std::string> &rnames, std::vector<impg_gpu_bed_row_t> &merged, std::string &text, BedGapRows *gap) {
  merged.clear();
  if (!n) return;
  DevRows dev;
  DevBuf out;
  dev.upload(E, rows, row_range, n);
  const uint32_t n_runs = merge_rows(E, ix, dev.view(), n, n_seq, n_ranges, merge_distance, merge_strands, out, gap);
  std::vector<BedRow> h(n_runs);
  if (n_runs) IMPG_HIP(hipMemcpy(h.data(), out.p, (size_t)n_runs * sizeof(BedRow), hipMemcpyDeviceToHost));
  merged.resize(n_runs);
  for (uint32_t r = 0; r < n_runs; r++) merged[r] = impg_gpu_bed_row_t{h[r].q_strand & 0x7FFFFFFFu, h[r].query_id, h[r].start, h[r].end, h[r].q_strand >> 31};
  device_bed_text(E, ix, out, n_runs, n_ranges, rnames, original_coords, [&](const char *p, size_t k) { text.append(p, k); });
}

// The merged rows of a chunk as text (text_device.hpp)
void device_bed_text(Engine &E, const impg_gpu_index &ix, const DevBuf &rows, uint32_t n_rows, uint32_t n_ranges,
                     const std::vector<std::string> &rnames, bool original_coords,
                     const std::function<void(const char *, size_t)> &sink) {
  device_rows_text<BedRow, text_len_kernel, text_write_kernel>(E, ix, rows, n_rows, n_ranges, rnames, original_coords, sink, "BED",
                                                               ix.bed_stats[BED_TEXT_PIECES], ix.bed_stats[BED_TEXT_BYTES]);
}

}  // namespace impg
