// masked_regions and missing_regions of `impg partition` resident in HBM, and one window's update of them as kernels
// (reference src/commands/partition.rs:939-1408; partition.cpp is the host twin, written the reference's sequential way).
//
// Layout: each map is a CSR table over the sequence ids -- u32 off[n_seq + 1], int2 ranges -- the layout the engines'
// masked queries read (Engine::mask_off / mask_ranges): the session hands the masked table to its engine by pointer.
// Every window rebuilds a table into the other of its two buffers.
//
// All interval lists are (key = seq << 32 | start, end) pairs sorted by key.  "Merge" everywhere is the same pass: the
// running end of the reference's sweeps is the prefix maximum of the ends inside the sequence (a max-scan of
// seq << 32 | end: the sequence id in the high word restarts it), and a run starts where start > prefix max + d.
//
//   1 rows -> (key, end), stable radix sort                         merge_overlaps' par_sort_by_key (:945-950)
//   2 merge at d                                                     :952-974
//   3 boundary extension, per interval                               :1369-1408
//   4 fragment candidates: the missing range that holds the start strictly inside, and the one that holds the end: two
//     binary searches an interval (only those can pass the tests of :1040-1055); sorted, merged at 0 with touching runs
//     joined (:1062-1075).  The loop of :1089-1099 mutates start / end while it walks the merged list; the list is
//     disjoint and non-touching, so at most one extension holds the original start and at most one the original end, an
//     extension applied for the start cannot move the end unless it holds the end too, and after start = ext_start no
//     later extension reaches it: start' = ext_start of the one holding start, end' = ext_end of the one holding end --
//     two more binary searches.  The starts stay non-decreasing inside a sequence.
//   5 minus the mask as it was: per interval the overlapping mask ranges [a, b) by binary search, the number of gaps, a
//     scan, a thread per surviving segment                            :1142-1243
//   6 sort, merge at 0: the window's output rows                      merge_overlaps(0)
//   7 mask insert: the old table and the extended intervals, both sorted, are merged by rank (a binary search each) and
//     run through the merge at 0, which joins overlapping and touching ranges as SortedRanges::insert does (impg.rs:
//     330-353); untouched sequences pass through unchanged
//   8 missing minus the new mask: stage 5's kernels on the missing table, then the merge at 0 (what missing.insert does
//     with touching pieces, :1300, :1309); a sequence whose set empties simply has no ranges (:1313-1316)
//   9 selection: atomic max of (length << 32 | range index) -- the table is ordered by (sequence, start), so the index
//     breaks ties as max_by does (:739-744) -- and the missing bases per sequence, summed into the one of two buffers
//     that is not current
// Nothing a window writes is current before its header is read: a refused row (norm_kernel) drops tables and sums alike.
// The host learns two things per window besides the output rows: the number of segments of stage 5 (to size stage 6) and
// a nine-word header (counts, flags, the longest missing range).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_prims.hpp"
#include "partition.hpp"

namespace impg {

namespace {

typedef unsigned long long u64;
constexpr u64 LOW32 = 0xFFFFFFFFull;
enum { H_NOUT = 0, H_NMASK, H_NMISS, H_EMPTY, H_ERR, H_SELANY, H_SELSEQ, H_SELLO, H_SELHI, H_SEGS, H_WORDS };
// device counters (ctr[]): valid items of the lists in flight
enum { C_N = 0, C_M, C_CAND, C_EXT, C_SEG, C_OUT, C_COMB, C_NMASK, C_XSEG, C_NMISS, C_HDR = 16, C_BEST = 32 /* u64, 8-byte aligned */, C_WORDS = 40 };

__device__ __forceinline__ uint32_t key_seq(u64 k) { return (uint32_t)(k >> 32); }
__device__ __forceinline__ int32_t key_lo(u64 k) { return (int32_t)(k & LOW32); }
__device__ __forceinline__ u64 make_key(uint32_t seq, int32_t lo) { return ((u64)seq << 32) | (uint32_t)lo; }

// number of ranges of r[0..n) with start < p
__device__ __forceinline__ uint32_t lower_start(const int2 *__restrict__ r, uint32_t n, int32_t p) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (r[mid].x < p) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// number of ranges of r[0..n) with start <= p (p may be INT32_MAX: no p + 1)
__device__ __forceinline__ uint32_t upper_start(const int2 *__restrict__ r, uint32_t n, int32_t p) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (r[mid].x <= p) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// number of ranges of r[0..n) with end <= p (ends ascend with the starts in a disjoint list)
__device__ __forceinline__ uint32_t upper_end(const int2 *__restrict__ r, uint32_t n, int32_t p) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (r[mid].y <= p) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ uint32_t lower_key(const u64 *__restrict__ k, uint32_t n, u64 x) {  // keys < x
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (k[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ uint32_t upper_u32(const uint32_t *__restrict__ a, uint32_t n, uint32_t x) {  // entries <= x
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- stage 1 --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void norm_kernel(const impg_gpu_interval_t *__restrict__ rows, uint32_t n, uint32_t n_seq,
                                                   u64 *__restrict__ key, int32_t *__restrict__ hi, uint32_t *__restrict__ ctr) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i == 0) ctr[C_N] = n;
  if (i >= n) return;
  const impg_gpu_interval_t r = rows[i];
  int32_t a = min(r.q_first, r.q_last), b = max(r.q_first, r.q_last);
  uint32_t s = r.query_id;
  if (s >= n_seq || a < 0) { ctr[C_HDR + H_ERR] = 1; s = 0; a = b = 0; }  // (never indexes a table with a foreign id)
  key[i] = make_key(s, a);
  hi[i] = b;
}

// ---- the merge: runs of a sorted list -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxkey_kernel(const u64 *__restrict__ key, const int32_t *__restrict__ hi, uint32_t n_ub,
                                                     const uint32_t *__restrict__ d_n, u64 *__restrict__ mk) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_ub) return;
  mk[i] = i < *d_n ? ((key[i] & ~LOW32) | (uint32_t)hi[i]) : 0ull;
}
__global__ __launch_bounds__(256) void head_kernel(const u64 *__restrict__ key, const u64 *__restrict__ pm, uint32_t n_ub,
                                                   const uint32_t *__restrict__ d_n, int32_t d, uint32_t *__restrict__ head) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > n_ub) return;
  uint32_t h = 0;
  if (i < n_ub && i < *d_n) {
    if (i == 0) h = 1;
    else {
      const u64 k = key[i], p = pm[i - 1];
      h = key_seq(k) != key_seq(key[i - 1]) || (long long)key_lo(k) > (long long)(int32_t)(p & LOW32) + d;
    }
  }
  head[i] = h;
}
__global__ __launch_bounds__(256) void run_write_kernel(const u64 *__restrict__ key, const u64 *__restrict__ pm, const uint32_t *__restrict__ head,
                                                        const uint32_t *__restrict__ pos, uint32_t n_ub, const uint32_t *__restrict__ d_n,
                                                        u64 *__restrict__ out_key, int32_t *__restrict__ out_hi, uint32_t *__restrict__ d_n_out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i == 0) *d_n_out = pos[n_ub];
  const uint32_t n = *d_n;
  if (i >= n_ub || i >= n) return;
  const uint32_t g = pos[i] + head[i] - 1u;
  if (head[i]) out_key[g] = key[i];
  if (i + 1 == n || head[i + 1]) out_hi[g] = (int32_t)(pm[i] & LOW32);
}

// ---- stages 3 + 4a: boundary extension, fragment candidates -------------------------------------------------------------
__global__ __launch_bounds__(256) void extend_cand_kernel(const u64 *__restrict__ a_key, const int32_t *__restrict__ a_hi, uint32_t n_ub,
                                                          const uint32_t *__restrict__ d_m, const int32_t *__restrict__ len,
                                                          const uint32_t *__restrict__ x_off, const int2 *__restrict__ x_rng, int32_t min_boundary,
                                                          int32_t min_missing, uint32_t n_seq, int32_t *__restrict__ b_lo, int32_t *__restrict__ b_hi,
                                                          u64 *__restrict__ c_key, int32_t *__restrict__ c_hi, uint32_t *__restrict__ ctr) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g == 0) ctr[C_CAND] = 2u * n_ub;  // (invalid candidates carry the sequence id n_seq and sort behind the others)
  if (g >= n_ub) return;
  const u64 inv = make_key(n_seq, 0);
  u64 k0 = inv, k1 = inv;
  int32_t h0 = 0, h1 = 0;
  if (g < *d_m) {
    const uint32_t s = key_seq(a_key[g]);
    int32_t lo = key_lo(a_key[g]), hi = a_hi[g];
    if (min_boundary > 0) {
      const int32_t L = len[s];
      if (lo < min_boundary) lo = 0;
      if (L - hi < min_boundary) hi = L;
    }
    b_lo[g] = lo;
    b_hi[g] = hi;
    const uint32_t xa = x_off[s], xn = x_off[s + 1] - xa;
    const int2 *r = x_rng + xa;
    if (xn) {
      uint32_t j = lower_start(r, xn, lo);  // ranges starting before lo: the last of them may hold lo
      if (j) {
        const int2 m = r[j - 1];
        if (lo < m.y && lo - m.x < min_missing) { k0 = make_key(s, m.x); h0 = lo; }
      }
      j = lower_start(r, xn, hi);
      if (j) {
        const int2 m = r[j - 1];
        if (hi < m.y && m.y - hi < min_missing) { k1 = make_key(s, hi); h1 = m.y; }
      }
    }
  }
  c_key[2 * g] = k0; c_hi[2 * g] = h0;
  c_key[2 * g + 1] = k1; c_hi[2 * g + 1] = h1;
}
// candidates sorted: the invalid ones are at the end; their number follows from the first invalid key
__global__ __launch_bounds__(256) void count_valid_kernel(const u64 *__restrict__ key, uint32_t n, uint32_t n_seq, uint32_t *__restrict__ d_n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const bool v = key_seq(key[i]) < n_seq;
  const bool pv = i == 0 ? true : key_seq(key[i - 1]) < n_seq;
  if (!v && pv) *d_n = i;
  if (v && i + 1 == n) *d_n = n;
}

// ---- stages 4b + 5a: apply the extensions, count the pieces the old mask leaves -----------------------------------------
__global__ __launch_bounds__(256) void apply_count_kernel(const u64 *__restrict__ a_key, uint32_t n_ub, const uint32_t *__restrict__ d_m,
                                                          int32_t *__restrict__ b_lo, int32_t *__restrict__ b_hi, const u64 *__restrict__ e_key,
                                                          const int32_t *__restrict__ e_hi, const uint32_t *__restrict__ d_ne,
                                                          const uint32_t *__restrict__ m_off, const int2 *__restrict__ m_rng,
                                                          uint32_t *__restrict__ s_a, uint32_t *__restrict__ s_first, uint32_t *__restrict__ s_cnt) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g > n_ub) return;
  uint32_t cnt = 0;
  if (g < n_ub && g < *d_m) {
    const uint32_t s = key_seq(a_key[g]);
    int32_t lo = b_lo[g], hi = b_hi[g];
    const uint32_t ne = *d_ne;
    if (ne) {
      uint32_t j = lower_key(e_key, ne, make_key(s, lo) + 1);  // extensions starting at or before lo
      int32_t nlo = lo, nhi = hi;
      if (j && key_seq(e_key[j - 1]) == s && e_hi[j - 1] >= lo) nlo = key_lo(e_key[j - 1]);
      j = lower_key(e_key, ne, make_key(s, hi) + 1);
      if (j && key_seq(e_key[j - 1]) == s && e_hi[j - 1] >= hi) nhi = max(hi, e_hi[j - 1]);
      lo = min(lo, nlo);
      hi = nhi;
      b_lo[g] = lo;
      b_hi[g] = hi;
    }
    const uint32_t ma = m_off[s], mn = m_off[s + 1] - ma;
    const int2 *r = m_rng + ma;
    const uint32_t a = upper_end(r, mn, lo);    // first mask range that ends behind lo
    const uint32_t b = lower_start(r, mn, hi);  // first that starts at or behind hi
    uint32_t first = 0;
    if (lo < hi) {
      if (b > a) {
        first = r[a].x <= lo;
        cnt = (b - a) + 1u - first - (r[b - 1].y >= hi ? 1u : 0u);
      } else cnt = 1;
    }
    s_a[g] = ma + a;
    s_first[g] = first | ((b > a ? b - a : 0u) << 1);
  }
  s_cnt[g] = cnt;
}
// a thread per surviving piece: piece j of item g lies between mask ranges a + t - 1 and a + t, t = j + first
__global__ __launch_bounds__(256) void piece_write_kernel(const u64 *__restrict__ item_key, const int32_t *__restrict__ item_lo,
                                                          const int32_t *__restrict__ item_hi, uint32_t n_items_ub,
                                                          const uint32_t *__restrict__ s_a, const uint32_t *__restrict__ s_first,
                                                          const uint32_t *__restrict__ s_off, const int2 *__restrict__ m_rng, uint32_t n_ub,
                                                          u64 *__restrict__ out_key, int32_t *__restrict__ out_hi, uint32_t *__restrict__ d_n_out) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  const uint32_t total = s_off[n_items_ub];
  if (t == 0) *d_n_out = total;
  if (t >= n_ub || t >= total) return;
  const uint32_t g = upper_u32(s_off, n_items_ub + 1, t) - 1u;
  const uint32_t j = t - s_off[g];
  const uint32_t first = s_first[g] & 1u, k = s_first[g] >> 1, a = s_a[g];
  const uint32_t u = j + first;
  const int32_t left = u == 0 ? item_lo[g] : m_rng[a + u - 1].y;
  const int32_t right = u < k ? m_rng[a + u].x : item_hi[g];
  out_key[t] = make_key(key_seq(item_key[g]), left);
  out_hi[t] = right;
}

// ---- stage 7: old mask ranges and new intervals, both sorted, into one sorted list ------------------------------------
__global__ __launch_bounds__(256) void mask_merge_kernel(const uint32_t *__restrict__ m_off, const int2 *__restrict__ m_rng, uint32_t n_old,
                                                         uint32_t n_seq, const u64 *__restrict__ a_key, const int32_t *__restrict__ b_lo,
                                                         const int32_t *__restrict__ b_hi, uint32_t n_ub, const uint32_t *__restrict__ d_m,
                                                         u64 *__restrict__ out_key, int32_t *__restrict__ out_hi, uint32_t *__restrict__ d_n_out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t m = min(*d_m, n_ub);
  if (i == 0) *d_n_out = n_old + m;
  if (i < n_old) {  // an old range goes in front of the new intervals with the same key
    const uint32_t s = upper_u32(m_off, n_seq + 1, i) - 1u;
    const int2 r = m_rng[i];
    // new intervals of s with start < r.x: their keys are (s, b_lo), non-decreasing
    uint32_t lo = 0, hi = m;
    const u64 x = make_key(s, r.x);
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (make_key(key_seq(a_key[mid]), b_lo[mid]) < x) lo = mid + 1; else hi = mid;
    }
    out_key[i + lo] = x;
    out_hi[i + lo] = r.y;
  } else if (i - n_old < m) {
    const uint32_t g = i - n_old;
    const uint32_t s = key_seq(a_key[g]);
    const uint32_t ma = m_off[s], mn = m_off[s + 1] - ma;
    const uint32_t rank = ma + upper_start(m_rng + ma, mn, b_lo[g]);  // old ranges of lower sequences, and of s with start <= lo
    out_key[g + rank] = make_key(s, b_lo[g]);
    out_hi[g + rank] = b_hi[g];
  }
}
// a merged (key, end) list -> a table
__global__ __launch_bounds__(256) void table_kernel(const u64 *__restrict__ key, const int32_t *__restrict__ hi, uint32_t n_ub,
                                                    const uint32_t *__restrict__ d_n, uint32_t n_seq, uint32_t *__restrict__ off,
                                                    int2 *__restrict__ rng, uint32_t *__restrict__ hdr, int count_word, int empty_word) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t n = min(*d_n, n_ub);
  if (i == 0) hdr[count_word] = n;
  if (i <= n_seq) off[i] = lower_key(key, n, make_key(i, 0));
  if (i < n) {
    const int32_t a = key_lo(key[i]), b = hi[i];
    rng[i] = make_int2(a, b);
    if (a == b && empty_word >= 0) hdr[empty_word] = 1;
  }
}

// ---- stage 8a: the missing ranges as items, counted against the new mask -----------------------------------------------
__global__ __launch_bounds__(256) void missing_count_kernel(const uint32_t *__restrict__ x_off, const int2 *__restrict__ x_rng, uint32_t n_x,
                                                            uint32_t n_seq, const uint32_t *__restrict__ m_off, const int2 *__restrict__ m_rng,
                                                            u64 *__restrict__ item_key, int32_t *__restrict__ item_lo, int32_t *__restrict__ item_hi,
                                                            uint32_t *__restrict__ s_a, uint32_t *__restrict__ s_first, uint32_t *__restrict__ s_cnt) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g > n_x) return;
  uint32_t cnt = 0;
  if (g < n_x) {
    const uint32_t s = upper_u32(x_off, n_seq + 1, g) - 1u;
    const int2 x = x_rng[g];
    const uint32_t ma = m_off[s], mn = m_off[s + 1] - ma;
    const int2 *r = m_rng + ma;
    const uint32_t a = upper_end(r, mn, x.x), b = lower_start(r, mn, x.y);
    uint32_t first = 0;
    if (b > a) {
      first = r[a].x <= x.x;
      cnt = (b - a) + 1u - first - (r[b - 1].y >= x.y ? 1u : 0u);
    } else cnt = 1;
    item_key[g] = make_key(s, x.x);
    item_lo[g] = x.x;
    item_hi[g] = x.y;
    s_a[g] = ma + a;
    s_first[g] = first | ((b > a ? b - a : 0u) << 1);
  }
  s_cnt[g] = cnt;
}

// ---- stage 9 ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void select_kernel(const u64 *__restrict__ key, const int32_t *__restrict__ hi, uint32_t n_ub,
                                                     const uint32_t *__restrict__ d_n, u64 *__restrict__ best, u64 *__restrict__ totals) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_ub || i >= *d_n) return;
  const u64 l = (u64)(uint32_t)(hi[i] - key_lo(key[i]));
  atomicMax(best, (l << 32) | i);
  atomicAdd(&totals[key_seq(key[i])], l);
}
__global__ void finish_kernel(const u64 *__restrict__ key, const int32_t *__restrict__ hi, const u64 *__restrict__ best, uint32_t *__restrict__ ctr,
                              const u64 *__restrict__ o_key, const int32_t *__restrict__ o_hi, uint32_t n_out_ub, PIv *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t *hdr = ctr + C_HDR;
  const uint32_t n_out = min(ctr[C_OUT], n_out_ub);
  if (i == 0) {
    hdr[H_NOUT] = n_out;
    const uint32_t n = hdr[H_NMISS];
    if (n) {
      const uint32_t k = (uint32_t)(*best & LOW32);
      hdr[H_SELANY] = 1;
      hdr[H_SELSEQ] = key_seq(key[k]);
      hdr[H_SELLO] = (uint32_t)key_lo(key[k]);
      hdr[H_SELHI] = (uint32_t)hi[k];
    }
  }
  if (i < n_out) out[i] = PIv{key_seq(o_key[i]), key_lo(o_key[i]), o_hi[i]};
}

using prims::bits_upto;
using prims::cdiv1;

struct Ops {
  DeviceRegions &R;
  hipStream_t s;
  void excl_scan(const uint32_t *in, uint32_t *out, size_t n) { prims::exclusive_sum(R.tmp, in, out, n, s); R.launches++; }
  void max_scan(const u64 *in, u64 *out, size_t n) { prims::inclusive_max(R.tmp, in, out, n, s); R.launches++; }
  // stable; keys of [0, 32 + seq bits)
  void sort(const u64 *kin, u64 *kout, const int32_t *vin, int32_t *vout, size_t n, unsigned end_bit) {
    prims::radix_sort_pairs(R.tmp, kin, kout, vin, vout, n, 0u, end_bit, s);
    R.launches++;
  }
  // runs of a sorted list of *d_n (<= n_ub) items: out[*d_n_out]
  void merge(const u64 *key, const int32_t *hi, uint32_t n_ub, const uint32_t *d_n, int32_t d, u64 *out_key, int32_t *out_hi, uint32_t *d_n_out) {
    prims::grow(R.mk, (size_t)n_ub * 8); prims::grow(R.pm, (size_t)n_ub * 8);
    prims::grow(R.head, ((size_t)n_ub + 1) * 4); prims::grow(R.pos, ((size_t)n_ub + 1) * 4);
    maxkey_kernel<<<cdiv1(n_ub, 256), 256, 0, s>>>(key, hi, n_ub, d_n, R.mk.as<u64>());
    max_scan(R.mk.as<u64>(), R.pm.as<u64>(), n_ub);
    head_kernel<<<cdiv1((size_t)n_ub + 1, 256), 256, 0, s>>>(key, R.pm.as<u64>(), n_ub, d_n, d, R.head.as<uint32_t>());
    excl_scan(R.head.as<uint32_t>(), R.pos.as<uint32_t>(), (size_t)n_ub + 1);
    run_write_kernel<<<cdiv1(n_ub, 256), 256, 0, s>>>(key, R.pm.as<u64>(), R.head.as<uint32_t>(), R.pos.as<uint32_t>(), n_ub, d_n, out_key, out_hi, d_n_out);
    R.launches += 3;
  }
};

}  // namespace

DeviceRegions::DeviceRegions(int device_, const int64_t *seq_len, uint32_t n_seq_, hipStream_t s) : device(device_), n_seq(n_seq_), stream(s) {
  if (n_seq >= 0x7FFFFFFFu) throw Error{IMPG_E_UNSUPPORTED, "too many sequences"};
  if (!stream) { IMPG_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)); own_stream = true; }
  IMPG_HIP(hipHostMalloc((void **)&h_hdr, 256, hipHostMallocDefault));
  std::vector<int32_t> L(n_seq);
  std::vector<uint32_t> xo(n_seq + 1, 0), mo(n_seq + 1, 0);
  std::vector<int32_t> xr;
  std::vector<u64> tot(n_seq, 0);
  int64_t best = -1;
  for (uint32_t q = 0; q < n_seq; q++) {
    L[q] = (int32_t)std::min<int64_t>(std::max<int64_t>(seq_len[q], 0), INT32_MAX);
    if (L[q] > 0) {
      tot[q] = (u64)L[q];
      xr.push_back(0); xr.push_back(L[q]);
      if (L[q] >= best) { best = L[q]; longest.any = true; longest.seq = q; longest.lo = 0; longest.hi = L[q]; }
    }
    xo[q + 1] = (uint32_t)(xr.size() / 2);
  }
  n_missing = (uint32_t)(xr.size() / 2);
  using prims::grow;
  grow(len, (size_t)n_seq * 4);
  for (int k = 0; k < 2; k++) grow(totals[k], (size_t)n_seq * 8);
  grow(ctr, C_WORDS * 4);
  for (int k = 0; k < 2; k++) { grow(m_off[k], ((size_t)n_seq + 1) * 4); grow(x_off[k], ((size_t)n_seq + 1) * 4); }
  grow(m_rng[0], 256); grow(x_rng[0], xr.size() * 4);
  // the state is built once on the host -- lengths, an empty mask, missing = every sequence -- and lives in HBM from here on
  if (n_seq) IMPG_HIP(hipMemcpyAsync(len.p, L.data(), (size_t)n_seq * 4, hipMemcpyHostToDevice, stream));
  if (n_seq) IMPG_HIP(hipMemcpyAsync(totals[0].p, tot.data(), (size_t)n_seq * 8, hipMemcpyHostToDevice, stream));
  IMPG_HIP(hipMemcpyAsync(m_off[0].p, mo.data(), ((size_t)n_seq + 1) * 4, hipMemcpyHostToDevice, stream));
  IMPG_HIP(hipMemcpyAsync(x_off[0].p, xo.data(), ((size_t)n_seq + 1) * 4, hipMemcpyHostToDevice, stream));
  if (!xr.empty()) IMPG_HIP(hipMemcpyAsync(x_rng[0].p, xr.data(), xr.size() * 4, hipMemcpyHostToDevice, stream));
  IMPG_HIP(hipMemsetAsync(ctr.p, 0, C_WORDS * 4, stream));
  IMPG_HIP(hipStreamSynchronize(stream));
}

DeviceRegions::~DeviceRegions() {
  if (h_hdr) (void)hipHostFree(h_hdr);
  if (own_stream && stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
}

void DeviceRegions::apply_host_rows(const impg_gpu_interval_t *rows, uint32_t n, int32_t d, int32_t min_missing, int32_t min_boundary, std::vector<PIv> &out) {
  up_rows.reserve(std::max<size_t>((size_t)n * sizeof(impg_gpu_interval_t), 256));
  if (n) IMPG_HIP(hipMemcpyAsync(up_rows.p, rows, (size_t)n * sizeof(impg_gpu_interval_t), hipMemcpyHostToDevice, stream));
  apply(up_rows.as<impg_gpu_interval_t>(), n, d, min_missing, min_boundary, out);
}

void DeviceRegions::apply(const impg_gpu_interval_t *d_rows, uint32_t n, int32_t d, int32_t min_missing, int32_t min_boundary, std::vector<PIv> &out) {
  out.clear();
  if (n == 0) return;  // mask_and_update_regions returns at once (:1321-1323): nothing changes
  if (d < 0) throw Error{IMPG_E_INVALID, "merge_distance < 0 is not supported"};
  if (n_seq == 0) throw Error{IMPG_E_INVALID, "rows for a state without sequences"};
  hipStream_t s = stream;
  Ops op{*this, s};
  const unsigned end_bit = 32 + bits_upto(n_seq);
  uint32_t *c = ctr.as<uint32_t>();
  const uint32_t n_old = n_mask, n_x = n_missing;
  const int mo = m_cur, xo = x_cur, mn = m_cur ^ 1, xn = x_cur ^ 1, tn = t_cur ^ 1;
  // 1
  prims::grow(key_a, (size_t)2 * n * 8); prims::grow(key_b, (size_t)2 * n * 8); prims::grow(val_a, (size_t)2 * n * 4); prims::grow(val_b, (size_t)2 * n * 4);
  IMPG_HIP(hipMemsetAsync(c + C_HDR, 0, H_WORDS * 4, s));
  norm_kernel<<<cdiv1(n, 256), 256, 0, s>>>(d_rows, n, n_seq, key_a.as<u64>(), val_a.as<int32_t>(), c);
  op.sort(key_a.as<u64>(), key_b.as<u64>(), val_a.as<int32_t>(), val_b.as<int32_t>(), n, end_bit);
  // 2
  prims::grow(a_key, (size_t)n * 8); prims::grow(a_hi, (size_t)n * 4);
  op.merge(key_b.as<u64>(), val_b.as<int32_t>(), n, c + C_N, d, a_key.as<u64>(), a_hi.as<int32_t>(), c + C_M);
  // 3 + 4
  prims::grow(b_lo, (size_t)n * 4); prims::grow(b_hi, (size_t)n * 4);
  extend_cand_kernel<<<cdiv1(n, 256), 256, 0, s>>>(a_key.as<u64>(), a_hi.as<int32_t>(), n, c + C_M, len.as<int32_t>(), x_off[xo].as<uint32_t>(),
                                                  x_rng[xo].as<int2>(), min_boundary, min_missing, n_seq, b_lo.as<int32_t>(), b_hi.as<int32_t>(),
                                                  key_a.as<u64>(), val_a.as<int32_t>(), c);
  op.sort(key_a.as<u64>(), key_b.as<u64>(), val_a.as<int32_t>(), val_b.as<int32_t>(), (size_t)2 * n, end_bit);
  count_valid_kernel<<<cdiv1((size_t)2 * n, 256), 256, 0, s>>>(key_b.as<u64>(), 2 * n, n_seq, c + C_CAND);
  prims::grow(e_key, (size_t)2 * n * 8); prims::grow(e_hi, (size_t)2 * n * 4);
  op.merge(key_b.as<u64>(), val_b.as<int32_t>(), 2 * n, c + C_CAND, 0, e_key.as<u64>(), e_hi.as<int32_t>(), c + C_EXT);
  // 5
  prims::grow(s_a, ((size_t)n + 1) * 4); prims::grow(s_first, ((size_t)n + 1) * 4); prims::grow(s_cnt, ((size_t)n + 1) * 4); prims::grow(s_off, ((size_t)n + 1) * 4);
  apply_count_kernel<<<cdiv1((size_t)n + 1, 256), 256, 0, s>>>(a_key.as<u64>(), n, c + C_M, b_lo.as<int32_t>(), b_hi.as<int32_t>(), e_key.as<u64>(),
                                                               e_hi.as<int32_t>(), c + C_EXT, m_off[mo].as<uint32_t>(), m_rng[mo].as<int2>(),
                                                               s_a.as<uint32_t>(), s_first.as<uint32_t>(), s_cnt.as<uint32_t>());
  op.excl_scan(s_cnt.as<uint32_t>(), s_off.as<uint32_t>(), (size_t)n + 1);
  launches += 4;
  IMPG_HIP(hipMemcpyAsync(h_hdr + 32, s_off.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipStreamSynchronize(s));
  const uint32_t n_seg = h_hdr[32];
  if (n_seg >= (1u << 30)) throw Error{IMPG_E_UNSUPPORTED, "a window leaves more than 2^30 pieces"};
  // 6
  const uint32_t sg = std::max(n_seg, 1u);
  prims::grow(t_key, (size_t)sg * 8); prims::grow(t_hi, (size_t)sg * 4); prims::grow(n_key, (size_t)sg * 8); prims::grow(n_hi, (size_t)sg * 4);
  prims::grow(o_key, (size_t)sg * 8); prims::grow(o_hi, (size_t)sg * 4);
  piece_write_kernel<<<cdiv1(sg, 256), 256, 0, s>>>(a_key.as<u64>(), b_lo.as<int32_t>(), b_hi.as<int32_t>(), n, s_a.as<uint32_t>(),
                                                    s_first.as<uint32_t>(), s_off.as<uint32_t>(), m_rng[mo].as<int2>(), sg, t_key.as<u64>(),
                                                    t_hi.as<int32_t>(), c + C_SEG);
  launches++;
  if (n_seg > 1) op.sort(t_key.as<u64>(), n_key.as<u64>(), t_hi.as<int32_t>(), n_hi.as<int32_t>(), n_seg, end_bit);
  const u64 *sk = n_seg > 1 ? n_key.as<u64>() : t_key.as<u64>();
  const int32_t *sh = n_seg > 1 ? n_hi.as<int32_t>() : t_hi.as<int32_t>();
  op.merge(sk, sh, sg, c + C_SEG, 0, o_key.as<u64>(), o_hi.as<int32_t>(), c + C_OUT);
  // 7
  const uint32_t comb = n_old + n;
  prims::grow(c_key, (size_t)comb * 8); prims::grow(c_hi, (size_t)comb * 4);
  prims::grow(key_a, (size_t)comb * 8); prims::grow(val_a, (size_t)comb * 4);
  mask_merge_kernel<<<cdiv1(comb, 256), 256, 0, s>>>(m_off[mo].as<uint32_t>(), m_rng[mo].as<int2>(), n_old, n_seq, a_key.as<u64>(), b_lo.as<int32_t>(),
                                                    b_hi.as<int32_t>(), n, c + C_M, c_key.as<u64>(), c_hi.as<int32_t>(), c + C_COMB);
  op.merge(c_key.as<u64>(), c_hi.as<int32_t>(), comb, c + C_COMB, 0, key_a.as<u64>(), val_a.as<int32_t>(), c + C_NMASK);
  prims::grow(m_rng[mn], (size_t)comb * 8);
  table_kernel<<<cdiv1(std::max<size_t>(comb, (size_t)n_seq + 1), 256), 256, 0, s>>>(key_a.as<u64>(), val_a.as<int32_t>(), comb, c + C_NMASK, n_seq,
                                                                                   m_off[mn].as<uint32_t>(), m_rng[mn].as<int2>(), c + C_HDR, H_NMASK, H_EMPTY);
  launches += 2;
  // 8
  const uint32_t xs_ub = std::max<uint32_t>(2 * n_x + comb, 1);
  const uint32_t nx1 = std::max(n_x, 1u);
  prims::grow(key_b, (size_t)nx1 * 8); prims::grow(b_lo, (size_t)nx1 * 4); prims::grow(b_hi, (size_t)nx1 * 4);
  prims::grow(s_a, ((size_t)n_x + 1) * 4); prims::grow(s_first, ((size_t)n_x + 1) * 4); prims::grow(s_cnt, ((size_t)n_x + 1) * 4); prims::grow(s_off, ((size_t)n_x + 1) * 4);
  missing_count_kernel<<<cdiv1((size_t)n_x + 1, 256), 256, 0, s>>>(x_off[xo].as<uint32_t>(), x_rng[xo].as<int2>(), n_x, n_seq, m_off[mn].as<uint32_t>(),
                                                                  m_rng[mn].as<int2>(), key_b.as<u64>(), b_lo.as<int32_t>(), b_hi.as<int32_t>(),
                                                                  s_a.as<uint32_t>(), s_first.as<uint32_t>(), s_cnt.as<uint32_t>());
  op.excl_scan(s_cnt.as<uint32_t>(), s_off.as<uint32_t>(), (size_t)n_x + 1);
  prims::grow(c_key, (size_t)xs_ub * 8); prims::grow(c_hi, (size_t)xs_ub * 4);
  prims::grow(key_a, (size_t)xs_ub * 8); prims::grow(val_a, (size_t)xs_ub * 4);
  piece_write_kernel<<<cdiv1(xs_ub, 256), 256, 0, s>>>(key_b.as<u64>(), b_lo.as<int32_t>(), b_hi.as<int32_t>(), n_x, s_a.as<uint32_t>(),
                                                       s_first.as<uint32_t>(), s_off.as<uint32_t>(), m_rng[mn].as<int2>(), xs_ub, c_key.as<u64>(),
                                                       c_hi.as<int32_t>(), c + C_XSEG);
  op.merge(c_key.as<u64>(), c_hi.as<int32_t>(), xs_ub, c + C_XSEG, 0, key_a.as<u64>(), val_a.as<int32_t>(), c + C_NMISS);
  prims::grow(x_rng[xn], (size_t)xs_ub * 8);
  table_kernel<<<cdiv1(std::max<size_t>(xs_ub, (size_t)n_seq + 1), 256), 256, 0, s>>>(key_a.as<u64>(), val_a.as<int32_t>(), xs_ub, c + C_NMISS, n_seq,
                                                                                    x_off[xn].as<uint32_t>(), x_rng[xn].as<int2>(), c + C_HDR, H_NMISS, -1);
  launches += 3;
  // 9
  IMPG_HIP(hipMemsetAsync(totals[tn].p, 0, std::max<size_t>((size_t)n_seq * 8, 8), s));
  IMPG_HIP(hipMemsetAsync(c + C_BEST, 0, 8, s));
  select_kernel<<<cdiv1(xs_ub, 256), 256, 0, s>>>(key_a.as<u64>(), val_a.as<int32_t>(), xs_ub, c + C_NMISS, (u64 *)(c + C_BEST), totals[tn].as<u64>());
  prims::grow(out_rows, (size_t)sg * sizeof(PIv));
  finish_kernel<<<cdiv1(sg, 256), 256, 0, s>>>(key_a.as<u64>(), val_a.as<int32_t>(), (const u64 *)(c + C_BEST), c, o_key.as<u64>(), o_hi.as<int32_t>(),
                                              sg, out_rows.as<PIv>());
  launches += 4;
  IMPG_HIP(hipMemcpyAsync(h_hdr, c + C_HDR, H_WORDS * 4, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipStreamSynchronize(s));
  // (a refused row leaves the state as it was: the tables and the sums just built are dropped, all of them in the
  // buffers that are not current)
  if (h_hdr[H_ERR]) throw Error{IMPG_E_INVALID, "a row names an unknown sequence or has a negative coordinate"};
  m_cur = mn;
  x_cur = xn;
  t_cur = tn;
  n_mask = h_hdr[H_NMASK];
  n_missing = h_hdr[H_NMISS];
  mask_has_empty = h_hdr[H_EMPTY] != 0;
  longest = SelSummary();
  longest.any = h_hdr[H_SELANY] != 0;
  longest.seq = h_hdr[H_SELSEQ];
  longest.lo = (int32_t)h_hdr[H_SELLO];
  longest.hi = (int32_t)h_hdr[H_SELHI];
  const uint32_t n_out = h_hdr[H_NOUT];
  out.resize(n_out);
  if (n_out) {
    IMPG_HIP(hipMemcpyAsync(out.data(), out_rows.p, (size_t)n_out * sizeof(PIv), hipMemcpyDeviceToHost, s));
    IMPG_HIP(hipStreamSynchronize(s));
  }
}

void DeviceRegions::get(int which, uint32_t *off_out, std::vector<int32_t> &ranges) {
  const DevBuf &o = which == IMPG_REGIONS_MASKED ? m_off[m_cur] : x_off[x_cur];
  const DevBuf &r = which == IMPG_REGIONS_MASKED ? m_rng[m_cur] : x_rng[x_cur];
  const uint32_t n = which == IMPG_REGIONS_MASKED ? n_mask : n_missing;
  IMPG_HIP(hipMemcpyAsync(off_out, o.p, ((size_t)n_seq + 1) * 4, hipMemcpyDeviceToHost, stream));
  ranges.resize((size_t)n * 2);
  if (n) IMPG_HIP(hipMemcpyAsync(ranges.data(), r.p, (size_t)n * 8, hipMemcpyDeviceToHost, stream));
  IMPG_HIP(hipStreamSynchronize(stream));
}

void DeviceRegions::summary(SelSummary &s, bool want_totals) {
  s = longest;
  if (!want_totals) return;
  s.total.assign(n_seq, 0);
  if (!n_seq) return;
  IMPG_HIP(hipMemcpyAsync(s.total.data(), totals[t_cur].p, (size_t)n_seq * 8, hipMemcpyDeviceToHost, stream));
  IMPG_HIP(hipStreamSynchronize(stream));
}

}  // namespace impg
