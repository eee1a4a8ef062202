// The support count of `impg refine` (reference src/commands/refine.rs:665-850) over rows that lie in HBM; refine.cpp is
// the host twin, written the reference's sequential way.
//
// A call holds the rows of n_cand candidates, rows[offsets[c] .. offsets[c + 1]) in emission order.
//
//   1 keys: a thread per row finds its candidate (binary search in offsets[]), drops holes (query_id = 0xFFFFFFFF) and
//     rows of the candidate's own target (:687-689), refuses a foreign sequence id (the row is dropped: nothing indexes
//     with it) and counts the candidate's rows up to 2 (:680-682: a candidate of at most one row supports nothing)
//   2 two stable radix sorts with the row index as payload: by (q_start, q_end) -- signed, so with the sign bits
//     flipped --, then by (candidate, query_id): a group's rows in the order of the reference's stable sort (:808-812),
//     ties in emission order; dropped rows carry the candidate n_cand and sort behind the others
//   3 ONE LANE PER GROUP (the thread at the group's first row) runs the left fold merge_intervals / should_merge
//     (:799-850) over the group's stretch -- overlapping intervals are not adjacent under its measure, so the fold is
//     order-dependent and no scan --, tests every merged interval's cover (:785-797), builds the hull of the covering
//     ones and searches the blacklist: the first range with end >= q_lo, then start <= q_hi (both ends inclusive,
//     :736-748).  merge_distance < 0 leaves every row its own interval; cover and hull do not depend on their order
//   4 surviving groups are compacted (a scan of the flags): (candidate, sequence, q_lo, q_hi) in ascending (candidate,
//     sequence); a candidate's stretch by binary search
//   5 distinct entities: identity = the survivors themselves; else (candidate, entity) keys sorted, heads counted; a
//     survivor without a key (0xFFFFFFFF) sorts behind the others and counts nothing (:756); then the clamp at
//     max_entities (:758-763)
// The host learns the number of survivors (to size stage 5), then count[], a three-word header and, on request, the survivors.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_prims.hpp"
#include "refine.hpp"

namespace impg {

namespace {

typedef unsigned long long u64;
constexpr u64 LOW32 = 0xFFFFFFFFull;
enum { C_ERR = 0, C_LONGEST, C_NSURV, C_WORDS = 4 };

__device__ __forceinline__ uint32_t flip(int32_t v) { return (uint32_t)v ^ 0x80000000u; }  // signed order as unsigned order
__device__ __forceinline__ uint32_t upper_u32(const uint32_t *__restrict__ a, uint32_t n, uint32_t x) {  // entries <= x
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ uint32_t lower_u32(const uint32_t *__restrict__ a, uint32_t n, uint32_t x) {  // entries < x
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ long long adiff(int32_t a, int32_t b) { return a > b ? (long long)a - b : (long long)b - a; }

// ---- stage 1 --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void key_kernel(const impg_gpu_interval_t *__restrict__ rows, uint32_t n, const uint32_t *__restrict__ offsets,
                                                  uint32_t n_cand, const impg_gpu_range_t *__restrict__ cand, uint32_t n_seq,
                                                  u64 *__restrict__ key1, u64 *__restrict__ key2, uint32_t *__restrict__ idx,
                                                  uint32_t *__restrict__ nrow, uint32_t *__restrict__ ctr) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const impg_gpu_interval_t r = rows[i];
  const uint32_t u = upper_u32(offsets, n_cand + 1, i);  // 1 .. n_cand for offsets that start at 0 and end at n
  bool ok = false;
  uint32_t c = n_cand;
  if (u >= 1 && u <= n_cand && r.query_id != HIT_NONE) {
    c = u - 1;
    if (r.query_id >= n_seq) ctr[C_ERR] = 1;  // (never indexes a table with a foreign id)
    else {
      if (nrow[c] < 2) atomicAdd(&nrow[c], 1u);
      ok = r.query_id != cand[c].target_id;
    }
  }
  key1[i] = ((u64)flip(min(r.q_first, r.q_last)) << 32) | flip(max(r.q_first, r.q_last));
  key2[i] = ok ? (((u64)c << 32) | r.query_id) : ((u64)n_cand << 32);
  idx[i] = i;
}

// ---- stage 3 --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fold_kernel(const impg_gpu_interval_t *__restrict__ rows, const u64 *__restrict__ key, const uint32_t *__restrict__ idx,
                                                   uint32_t n, uint32_t n_cand, const impg_gpu_range_t *__restrict__ cand,
                                                   const uint32_t *__restrict__ nrow, const uint32_t *__restrict__ bl_off,
                                                   const int2 *__restrict__ bl_rng, int32_t span_bp, int32_t d, uint32_t *__restrict__ flag,
                                                   int2 *__restrict__ hull, uint32_t *__restrict__ ctr) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j > n) return;
  uint32_t f = 0;
  if (j < n) {
    const u64 k = key[j];
    const uint32_t c = (uint32_t)(k >> 32);
    if (c < n_cand && (j == 0 || key[j - 1] != k) && nrow[c] >= 2) {
      const uint32_t seq = (uint32_t)(k & LOW32);
      const long long rs = cand[c].start, re = cand[c].end;
      const long long span = min(max(re - rs, 0ll), (long long)max(span_bp, 0));
      const long long left_thr = rs + span, right_thr = re - span;
      bool any = false, open = false;
      int32_t lo = 0, hi = 0, qs = 0, qe = 0, ts = 0, te = 0;
      uint32_t m = j;
      for (; m < n && key[m] == k; m++) {
        const impg_gpu_interval_t r = rows[idx[m]];
        const int32_t nqs = min(r.q_first, r.q_last), nqe = max(r.q_first, r.q_last);
        const int32_t nts = min(r.t_first, r.t_last), nte = max(r.t_first, r.t_last);
        if (open && d >= 0 && (min(adiff(qe, nqs), adiff(qs, nqe)) <= (long long)d || min(adiff(te, nts), adiff(ts, nte)) <= (long long)d)) {
          qs = min(qs, nqs); qe = max(qe, nqe);
          ts = min(ts, nts); te = max(te, nte);
          continue;
        }
        if (open && ts <= rs && te >= re && te >= left_thr && ts <= right_thr) {
          lo = any ? min(lo, qs) : qs;
          hi = any ? max(hi, qe) : qe;
          any = true;
        }
        qs = nqs; qe = nqe; ts = nts; te = nte;
        open = true;
      }
      if (open && ts <= rs && te >= re && te >= left_thr && ts <= right_thr) {
        lo = any ? min(lo, qs) : qs;
        hi = any ? max(hi, qe) : qe;
        any = true;
      }
      if (m - j > ctr[C_LONGEST]) atomicMax(&ctr[C_LONGEST], m - j);
      if (any && bl_off) {
        const uint32_t b0 = bl_off[seq], bn = bl_off[seq + 1] - b0;
        const int2 *r = bl_rng + b0;
        uint32_t a = 0, b = bn;
        while (a < b) {  // the first range with end >= lo
          const uint32_t mid = (a + b) >> 1;
          if (r[mid].y < lo) a = mid + 1; else b = mid;
        }
        if (a < bn && r[a].x <= hi) any = false;
      }
      if (any) { f = 1; hull[j] = make_int2(lo, hi); }
    }
  }
  flag[j] = f;
}

// ---- stage 4 --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void compact_kernel(const u64 *__restrict__ key, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                                      const int2 *__restrict__ hull, uint32_t n, uint32_t n_cand, const uint32_t *__restrict__ entity_of,
                                                      uint32_t *__restrict__ s_cand, uint32_t *__restrict__ s_seq, int2 *__restrict__ s_rng,
                                                      u64 *__restrict__ ekey, uint32_t *__restrict__ ctr) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j == 0) ctr[C_NSURV] = pos[n];
  if (j >= n || !flag[j]) return;
  const uint32_t p = pos[j];  // < the number of flags set <= n
  const uint32_t c = (uint32_t)(key[j] >> 32), seq = (uint32_t)(key[j] & LOW32);
  s_cand[p] = c;
  s_seq[p] = seq;
  s_rng[p] = hull[j];
  if (entity_of) {
    const uint32_t e = entity_of[seq];  // seq < n_seq: stage 1 dropped every other row
    ekey[p] = e == NO_ENTITY ? ((u64)n_cand << 32) : (((u64)c << 32) | e);
  }
}
__global__ __launch_bounds__(256) void offsets_kernel(const uint32_t *__restrict__ s_cand, uint32_t n_surv, uint32_t n_cand, uint32_t *__restrict__ s_off) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c <= n_cand) s_off[c] = lower_u32(s_cand, n_surv, c);
}

// ---- stage 5 --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void entity_heads_kernel(const u64 *__restrict__ ekey, uint32_t n_surv, uint32_t n_cand, uint32_t *__restrict__ count) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n_surv) return;
  const u64 k = ekey[p];
  const uint32_t c = (uint32_t)(k >> 32);
  if (c < n_cand && (p == 0 || ekey[p - 1] != k)) atomicAdd(&count[c], 1u);
}
__global__ __launch_bounds__(256) void count_finish_kernel(const uint32_t *__restrict__ s_off, const uint32_t *__restrict__ max_entities, uint32_t n_cand,
                                                           int identity, uint32_t *__restrict__ count) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= n_cand) return;
  uint32_t v = identity ? s_off[c + 1] - s_off[c] : count[c];
  if (max_entities) v = min(v, max_entities[c]);
  count[c] = v;
}

using prims::bits_upto;
using prims::cdiv1;

}  // namespace

SupportDevice::SupportDevice(int device_, hipStream_t s) : device(device_), stream(s) {
  if (!stream) { IMPG_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)); own_stream = true; }
  IMPG_HIP(hipHostMalloc((void **)&h_hdr, 256, hipHostMallocDefault));
}

SupportDevice::~SupportDevice() {
  if (h_hdr) (void)hipHostFree(h_hdr);
  if (own_stream && stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
}

void SupportDevice::run(const impg_gpu_interval_t *d_rows, uint32_t n, const uint32_t *d_offsets, const SupportInput &in, SupportOutput &out) {
  const uint32_t n_cand = (uint32_t)in.n_cand;
  out.count.assign(n_cand, 0);
  out.surv_off.clear();
  out.survivors.clear();
  out.longest_group = 0;
  if (out.want_survivors) out.surv_off.assign((size_t)n_cand + 1, 0);
  if (n_cand == 0 || n == 0) return;
  if (n >= (1u << 30)) throw Error{IMPG_E_UNSUPPORTED, "more than 2^30 rows in one call"};
  hipStream_t s = stream;
  using prims::grow;
  const bool identity = in.entity_of == nullptr, bl = !in.bl_off.empty();
  // the call's tables
  grow(d_cand, (size_t)n_cand * sizeof(impg_gpu_range_t));
  IMPG_HIP(hipMemcpyAsync(d_cand.p, in.cand, (size_t)n_cand * sizeof(impg_gpu_range_t), hipMemcpyHostToDevice, s));
  if (!identity && in.n_seq) {
    grow(d_ent, (size_t)in.n_seq * 4);
    IMPG_HIP(hipMemcpyAsync(d_ent.p, in.entity_of, (size_t)in.n_seq * 4, hipMemcpyHostToDevice, s));
  }
  if (in.max_entities) {
    grow(d_max, (size_t)n_cand * 4);
    IMPG_HIP(hipMemcpyAsync(d_max.p, in.max_entities, (size_t)n_cand * 4, hipMemcpyHostToDevice, s));
  }
  if (bl) {
    if (in.bl_off.size() != (size_t)in.n_seq + 1 || in.bl_rng.size() != 2 * (size_t)in.bl_off.back())
      throw Error{IMPG_E_INVALID, "internal: blacklist table of another size"};
    grow(d_bloff, in.bl_off.size() * 4);
    grow(d_blrng, in.bl_rng.size() * 4);
    IMPG_HIP(hipMemcpyAsync(d_bloff.p, in.bl_off.data(), in.bl_off.size() * 4, hipMemcpyHostToDevice, s));
    if (!in.bl_rng.empty()) IMPG_HIP(hipMemcpyAsync(d_blrng.p, in.bl_rng.data(), in.bl_rng.size() * 4, hipMemcpyHostToDevice, s));
  }
  grow(ctr, C_WORDS * 4);
  grow(d_nrow, (size_t)n_cand * 4);
  grow(d_count, (size_t)n_cand * 4);
  IMPG_HIP(hipMemsetAsync(ctr.p, 0, C_WORDS * 4, s));
  IMPG_HIP(hipMemsetAsync(d_nrow.p, 0, (size_t)n_cand * 4, s));
  IMPG_HIP(hipMemsetAsync(d_count.p, 0, (size_t)n_cand * 4, s));
  // 1
  grow(key_a, (size_t)n * 8); grow(key_b, (size_t)n * 8); grow(s_rng, (size_t)n * 8);
  grow(val_a, (size_t)n * 4); grow(val_b, (size_t)n * 4);
  u64 *k2 = s_rng.as<u64>();  // (the survivors' ranges are written after the second sort has read this)
  key_kernel<<<cdiv1(n, 256), 256, 0, s>>>(d_rows, n, d_offsets, n_cand, d_cand.as<impg_gpu_range_t>(), in.n_seq, key_a.as<u64>(), k2,
                                          val_a.as<uint32_t>(), d_nrow.as<uint32_t>(), ctr.as<uint32_t>());
  // 2
  prims::radix_sort_pairs(tmp, key_a.as<u64>(), key_b.as<u64>(), val_a.as<uint32_t>(), val_b.as<uint32_t>(), n, 0u, 64u, s);
  prims::gather_kernel<u64><<<cdiv1(n, 256), 256, 0, s>>>(k2, val_b.as<uint32_t>(), n, key_a.as<u64>());
  prims::radix_sort_pairs(tmp, key_a.as<u64>(), key_b.as<u64>(), val_b.as<uint32_t>(), val_a.as<uint32_t>(), n, 0u, 32u + bits_upto(n_cand), s);
  const u64 *skey = key_b.as<u64>();
  const uint32_t *sidx = val_a.as<uint32_t>();
  // 3
  grow(flag, ((size_t)n + 1) * 4); grow(pos, ((size_t)n + 1) * 4); grow(hull, (size_t)n * 8);
  fold_kernel<<<cdiv1((size_t)n + 1, 256), 256, 0, s>>>(d_rows, skey, sidx, n, n_cand, d_cand.as<impg_gpu_range_t>(), d_nrow.as<uint32_t>(),
                                                       bl ? d_bloff.as<uint32_t>() : nullptr, d_blrng.as<int2>(), in.span_bp, in.merge_distance,
                                                       flag.as<uint32_t>(), hull.as<int2>(), ctr.as<uint32_t>());
  // 4
  prims::exclusive_sum(tmp, flag.as<uint32_t>(), pos.as<uint32_t>(), (size_t)n + 1, s);
  grow(s_cand, (size_t)n * 4); grow(s_seq, (size_t)n * 4); grow(s_off, ((size_t)n_cand + 1) * 4);
  compact_kernel<<<cdiv1(n, 256), 256, 0, s>>>(skey, flag.as<uint32_t>(), pos.as<uint32_t>(), hull.as<int2>(), n, n_cand,
                                              identity ? nullptr : d_ent.as<uint32_t>(), s_cand.as<uint32_t>(), s_seq.as<uint32_t>(),
                                              s_rng.as<int2>(), key_a.as<u64>(), ctr.as<uint32_t>());
  IMPG_HIP(hipMemcpyAsync(h_hdr, ctr.p, C_WORDS * 4, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipStreamSynchronize(s));
  const uint32_t n_surv = h_hdr[C_NSURV];
  if (n_surv > n) throw Error{IMPG_E_HIP, "internal: more survivors than rows"};
  offsets_kernel<<<cdiv1((size_t)n_cand + 1, 256), 256, 0, s>>>(s_cand.as<uint32_t>(), n_surv, n_cand, s_off.as<uint32_t>());
  // 5
  if (!identity && n_surv) {
    prims::radix_sort_pairs(tmp, key_a.as<u64>(), key_b.as<u64>(), val_a.as<uint32_t>(), val_b.as<uint32_t>(), n_surv, 0u, 32u + bits_upto(n_cand), s);
    entity_heads_kernel<<<cdiv1(n_surv, 256), 256, 0, s>>>(key_b.as<u64>(), n_surv, n_cand, d_count.as<uint32_t>());
  }
  count_finish_kernel<<<cdiv1(n_cand, 256), 256, 0, s>>>(s_off.as<uint32_t>(), in.max_entities ? d_max.as<uint32_t>() : nullptr, n_cand, identity ? 1 : 0,
                                                        d_count.as<uint32_t>());
  IMPG_HIP(hipMemcpyAsync(out.count.data(), d_count.p, (size_t)n_cand * 4, hipMemcpyDeviceToHost, s));
  std::vector<uint32_t> off32, seqs;
  std::vector<int32_t> rng;
  if (out.want_survivors) {
    off32.resize((size_t)n_cand + 1);
    seqs.resize(n_surv);
    rng.resize((size_t)n_surv * 2);
    IMPG_HIP(hipMemcpyAsync(off32.data(), s_off.p, off32.size() * 4, hipMemcpyDeviceToHost, s));
    if (n_surv) {
      IMPG_HIP(hipMemcpyAsync(seqs.data(), s_seq.p, (size_t)n_surv * 4, hipMemcpyDeviceToHost, s));
      IMPG_HIP(hipMemcpyAsync(rng.data(), s_rng.p, (size_t)n_surv * 8, hipMemcpyDeviceToHost, s));
    }
  }
  IMPG_HIP(hipStreamSynchronize(s));
  out.longest_group = h_hdr[C_LONGEST];
  // (a refused row: the kernels have run, nothing indexed with it, and nothing of the call is handed out)
  if (h_hdr[C_ERR]) {
    out.count.assign(n_cand, 0);
    throw Error{IMPG_E_INVALID, "a row names an unknown sequence"};
  }
  if (out.want_survivors) {
    out.survivors.resize(n_surv);
    for (uint32_t p = 0; p < n_surv; p++) out.survivors[p] = impg_gpu_survivor_t{seqs[p], rng[2 * (size_t)p], rng[2 * (size_t)p + 1]};
    for (size_t c = 0; c <= n_cand; c++) out.surv_off[c] = off32[c];
  }
}

}  // namespace impg
