// BEDPE post-processing on the device: what output_results_bedpe (src/main.rs:11894-11987) prints for every query range
// after merge_adjusted_intervals (main.rs:12563-12845) -- for all ranges of a chunk at once, on the rows and the CIGAR
// pool where rows_device.hip left them, so that only text crosses PCIe.  paf_out.cpp holds the host-side restatement
// (one range at a time, CIGARs carried along); DESIGN 5.5 shows why the three steps below compute the same lines.
//
//   summary   BEDPE prints no CIGAR, only gi:f / bi:f, which are ratios of six sums over a merged row's ops.  One
//             32-byte record per row {m, x, ibp, dbp, ni, nd, ii, dd, first, last}: matched and mismatched bases,
//             inserted / deleted bases and ops, adjacent I-I / D-D op pairs inside the row, first and last op code.
//             The first row of every range is the input range itself and is dropped (main.rs:7474, :7486).
//   order     the remaining rows sorted by (range, query seq, forward?, q start, target seq, t_first), stable in
//             emission order (main.rs:12566-12582): three stable radix passes, least significant key first
//   link      the reference's fold only ever compares the next row with the row before it in that order (its overlap
//             arm cannot fire), so row k continues the run of row k-1 iff the pair is contiguous or a gap of at most d
//             on both axes: one thread per sorted row, run ids from a scan of the heads, sums by wrapping u32 atomics
//             (integer adds commute: the result does not depend on their order).  A join adds its gap to ibp / dbp
//             and one I / D op each, and merge_consecutive_cigar_ops (main.rs:13014-13035) removes one op for every
//             adjacent I-I / D-D pair: those inside the joined rows, and those of `A.last [I] [D] B.first` at the join.
//   text      one line per run, written by the device; gi / bi divided in f32 and printed as format!("{:.6}") does
// PAF (paf_device.inc, included at the end) runs the same summary, order and link stages and prints the merged CIGARs too.
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
struct RowSum {         // 32 bytes: two 16-byte stores
  uint32_t m, x, ibp, dbp;
  uint32_t ni_first;    // I ops | first op code << 29 (a row has fewer than 2^29 ops)
  uint32_t nd_last;     // D ops | last op code << 29
  uint32_t ii, dd;      // adjacent I-I / D-D op pairs
};
static_assert(sizeof(RowSum) == 32, "row summary is 32 bytes");
struct Run {  // a printed line, 64 bytes
  uint32_t range, qid, tid;
  int32_t q_first, q_last, t_first, t_last;
  uint32_t m, x, ibp, dbp, ni, nd;
  uint32_t pad[3];
};
static_assert(sizeof(Run) == 64, "run record is 64 bytes");
// the chunk's control block: flags[4] (u32) then counters[4] (u64)
enum { FLAG_NO_CIGAR = 0, FLAG_TARGET_REVERSE = 1 };
enum { CTR_SUMMARY_OPS = 0, CTR_JOINS_CONTIGUOUS = 1, CTR_JOINS_GAP = 2, CTR_FUSED_OPS = 3 };
struct Control {
  uint32_t flags[4];
  unsigned long long ctr[4];
};

// ---- summary ---------------------------------------------------------------------------------------------------------
// G lanes per row stride over the row's ops (one contiguous stretch of the pool: coalesced); the lane holding op k gets
// op k-1's code from its neighbour (the group's last lane of the step before for lane 0); sums by a butterfly over the
// group.  Rows of one wave have different lengths: a group whose row is done idles until the wave's longest is.
template <unsigned G>
__global__ __launch_bounds__(256) void summary_kernel(const uint32_t *__restrict__ row_range, const uint32_t *__restrict__ offsets,
                                                      const unsigned long long *__restrict__ coff, const uint32_t *__restrict__ pool, uint32_t n,
                                                      RowSum *__restrict__ sum, Control *__restrict__ ctl) {
  __shared__ unsigned long long block_ops;
  if (threadIdx.x == 0) block_ops = 0;
  __syncthreads();
  const unsigned long long row = (unsigned long long)blockIdx.x * (256u / G) + threadIdx.x / G;
  const uint32_t lane = threadIdx.x % G;
  const uint32_t r = (uint32_t)row;
  const bool live = row < n && r != offsets[row_range[r]];  // (the first row of a range is the range itself)
  if (live) {
    const unsigned long long a = coff[r];
    const uint32_t len = (uint32_t)(coff[r + 1] - a);
    const uint32_t *ops = pool + a;
    uint32_t m = 0, x = 0, ibp = 0, dbp = 0, ni = 0, nd = 0, ii = 0, dd = 0, ends = 0;  // ends: first code | last code << 3
    uint32_t carry = 7u;  // the code before the step's first op (7: none)
    for (uint32_t base = 0; base < len; base += G) {
      const uint32_t k = base + lane;
      const uint32_t op = k < len ? ops[k] : OP_PAD;  // (code 7, length 0: counts as nothing)
      const uint32_t code = op >> 29, l = op & OP_LEN_MASK;
      uint32_t before = __shfl_up(code, 1, G);
      if (lane == 0) before = carry;
      carry = __shfl(code, G - 1, G);
      m += (code == 0u || code == 4u) ? l : 0u;  // 'M' counts as matches (main.rs:12047)
      x += code == 1u ? l : 0u;
      ibp += code == 2u ? l : 0u;
      dbp += code == 3u ? l : 0u;
      ni += code == 2u;
      nd += code == 3u;
      ii += code == 2u && before == 2u;
      dd += code == 3u && before == 3u;
      if (k == 0) ends |= code;
      if (k + 1 == len) ends |= code << 3;
    }
    for (unsigned o = G / 2; o; o >>= 1) {
      m += __shfl_xor(m, o, G); x += __shfl_xor(x, o, G); ibp += __shfl_xor(ibp, o, G); dbp += __shfl_xor(dbp, o, G);
      ni += __shfl_xor(ni, o, G); nd += __shfl_xor(nd, o, G); ii += __shfl_xor(ii, o, G); dd += __shfl_xor(dd, o, G);
      ends |= __shfl_xor(ends, o, G);
    }
    if (lane == 0) {
      uint4 *out = reinterpret_cast<uint4 *>(sum + r);
      out[0] = make_uint4(m, x, ibp, dbp);
      out[1] = make_uint4(ni | (ends & 7u) << 29, nd | (ends >> 3) << 29, ii, dd);
      if (len == 0) ctl->flags[FLAG_NO_CIGAR] = 1u;
      else atomicAdd(&block_ops, (unsigned long long)len);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && block_ops) atomicAdd(&ctl->ctr[CTR_SUMMARY_OPS], block_ops);
}

// ---- order -----------------------------------------------------------------------------------------------------------
// one thread per row: the three sort keys at the row's own index, and the row listed among the kept ones (every range
// before it dropped one row, and so did its own: kept row r of range q is number r - (q + 1))
__global__ __launch_bounds__(256) void keys_kernel(ConstRows R, const uint32_t *__restrict__ offsets, uint32_t n, unsigned seq_bits, int sorted,
                                                   uint32_t *__restrict__ k_t, unsigned long long *__restrict__ k_mid,
                                                   unsigned long long *__restrict__ k_hi, uint32_t *__restrict__ kept, Control *__restrict__ ctl) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const uint32_t q = R.q[r];
  const uint32_t o0 = offsets[q], o1 = offsets[q + 1];
  if (r == o0) return;
  kept[r - (q + 1u)] = r;
  if (!sorted) return;
  const int4 c = R.c[r];
  // "Target intervals should always be in forward!" (main.rs:12604): the fold looks at every row of a range that has two
  // or more of them, and is not entered otherwise
  if (o1 - o0 >= 3u && c.z > c.w) ctl->flags[FLAG_TARGET_REVERSE] = 1u;
  const bool af = c.x < c.y;  // strict (main.rs:12566-12582): a row with q_first == q_last sorts with the reverse ones
  k_t[r] = ord_u32(c.z);
  k_mid[r] = ((((unsigned long long)(af ? 1u : 0u) << 32) | ord_u32(af ? c.x : c.y)) << seq_bits) | R.tid[r];
  k_hi[r] = ((unsigned long long)q << seq_bits) | R.qid[r];
}

// ---- link ------------------------------------------------------------------------------------------------------------
// Does row b continue the run of row a, the row before it in sorted order?  0: no, 1: contiguous, 2: gap.  qd / td: the
// gap on either axis.  (paf_out.cpp merge_rows with its overlap arm, which cannot fire, left out; the differences wrap
// like the reference's release build.)
__device__ __forceinline__ int join_kind(const ConstRows &R, uint32_t a, uint32_t b, int32_t d, bool &f, int32_t &qd, int32_t &td) {
  const int4 A = R.c[a], B = R.c[b];
  f = A.x <= A.y;
  if (R.q[a] != R.q[b] || R.qid[a] != R.qid[b] || R.tid[a] != R.tid[b] || f != (B.x <= B.y)) return 0;
  qd = (int32_t)(f ? (uint32_t)B.x - (uint32_t)A.y : (uint32_t)A.x - (uint32_t)B.y);
  td = (int32_t)(f ? (uint32_t)B.z - (uint32_t)A.w : (uint32_t)A.z - (uint32_t)B.w);
  if (qd == 0 && td == 0) return 1;
  // on the reverse strand the reference's query "overlap" test is really the gap test: a gap join there has qd == 0
  const bool q_over = f ? qd < 0 : qd > 0;
  if (!q_over && td >= 0 && qd >= 0 && (qd > 0 || td > 0) && qd <= d && td <= d) return 2;
  return 0;
}
__global__ __launch_bounds__(256) void heads_kernel(ConstRows R, const uint32_t *__restrict__ perm, uint32_t m, int32_t d, uint32_t *__restrict__ head) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= m) return;
  bool is_head = k == 0 || d < 0;
  if (!is_head) {
    bool f;
    int32_t qd, td;
    is_head = join_kind(R, perm[k - 1], perm[k], d, f, qd, td) == 0;
  }
  head[k] = is_head ? 1u : 0u;
}
// one thread per sorted row; run = run_pos[k] + head[k] - 1 (exclusive scan of the heads + own flag).  runs: zeroed.
__global__ __launch_bounds__(256) void reduce_kernel(ConstRows R, const RowSum *__restrict__ sum, const uint32_t *__restrict__ perm,
                                                     const uint32_t *__restrict__ head, const uint32_t *__restrict__ run_pos, uint32_t m, int32_t d,
                                                     Run *__restrict__ runs, Control *__restrict__ ctl) {
  __shared__ uint32_t block_ctr[3];  // contiguous joins, gap joins, fused ops
  if (threadIdx.x < 3) block_ctr[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k < m) {
    const uint32_t r = perm[k];
    const bool is_head = head[k] != 0, is_tail = k + 1 == m || head[k + 1] != 0;
    const bool joined = !(is_head && is_tail);  // no fusing happens without a join
    const uint4 s0 = reinterpret_cast<const uint4 *>(sum + r)[0], s1 = reinterpret_cast<const uint4 *>(sum + r)[1];
    uint32_t v_m = s0.x, v_x = s0.y, v_ibp = s0.z, v_dbp = s0.w, v_ni = s1.x & OP_LEN_MASK, v_nd = s1.y & OP_LEN_MASK;
    uint32_t fused = 0;
    if (joined) { v_ni -= s1.z; v_nd -= s1.w; fused = s1.z + s1.w; }
    const int4 c = R.c[r];
    const bool f = c.x <= c.y;
    if (!is_head) {
      const uint32_t rp = perm[k - 1];
      bool jf;
      int32_t qd = 0, td = 0;
      const int kind = join_kind(R, rp, r, d, jf, qd, td);
      // the join's ops: A.last, [I if qd > 0], [D if td > 0], B.first -- the reference prepends on the reverse strand
      const uint32_t p1x = sum[rp].ni_first, p1y = sum[rp].nd_last;
      const uint32_t a_last = f ? p1y >> 29 : s1.y >> 29, b_first = f ? s1.x >> 29 : p1x >> 29;
      uint32_t before = a_last, fi = 0, fd = 0;
      if (qd > 0) { fi += before == 2u; before = 2u; }
      if (td > 0) { fd += before == 3u; before = 3u; }
      fi += b_first == 2u && before == 2u;
      fd += b_first == 3u && before == 3u;
      v_ibp += (uint32_t)qd; v_dbp += (uint32_t)td;
      v_ni += (qd > 0) - fi; v_nd += (td > 0) - fd;
      fused += fi + fd;
      atomicAdd(&block_ctr[kind == 1 ? 0 : 1], 1u);
    }
    if (fused) atomicAdd(&block_ctr[2], fused);
    Run *run = runs + (run_pos[k] + (is_head ? 1u : 0u) - 1u);
    if (!joined) {
      run->m = v_m; run->x = v_x; run->ibp = v_ibp; run->dbp = v_dbp; run->ni = v_ni; run->nd = v_nd;
    } else {
      if (v_m) atomicAdd(&run->m, v_m);
      if (v_x) atomicAdd(&run->x, v_x);
      if (v_ibp) atomicAdd(&run->ibp, v_ibp);
      if (v_dbp) atomicAdd(&run->dbp, v_dbp);
      if (v_ni) atomicAdd(&run->ni, v_ni);
      if (v_nd) atomicAdd(&run->nd, v_nd);
    }
    // the run's box: {head.q_first, tail.q_last, head.t_first, tail.t_last} forward, {tail.q_first, head.q_last,
    // tail.t_first, head.t_last} reverse (main.rs:12663-12673)
    if (is_head) {
      run->range = R.q[r]; run->qid = R.qid[r]; run->tid = R.tid[r];
      if (f) { run->q_first = c.x; run->t_first = c.z; } else { run->q_last = c.y; run->t_last = c.w; }
    }
    if (is_tail) {
      if (f) { run->q_last = c.y; run->t_last = c.w; } else { run->q_first = c.x; run->t_first = c.z; }
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 && block_ctr[threadIdx.x])
    atomicAdd(&ctl->ctr[CTR_JOINS_CONTIGUOUS + threadIdx.x], (unsigned long long)block_ctr[threadIdx.x]);
}
static_assert(CTR_JOINS_GAP == CTR_JOINS_CONTIGUOUS + 1 && CTR_FUSED_OPS == CTR_JOINS_CONTIGUOUS + 2, "reduce_kernel's block counters");

// ---- text ------------------------------------------------------------------------------------------------------------
// A gi / bi value as format!("{:.6}") prints it with trailing zeros and a trailing '.' trimmed (put_f32, paf_out.cpp).
// f32 times 10^6 is exact in f64 (24 x 14 significant bits), so rounding the product to an integer, ties to even, is the
// correctly rounded six-decimal value.
struct F32Text {
  int special;             // 0: a number, 1: NaN, 2: inf
  bool neg;
  unsigned long long ip;   // integer part
  uint32_t frac, frac_digits;  // the fraction without its trailing zeros, and how many digits it prints with
};
__device__ __forceinline__ F32Text f32_text(float v) {
  F32Text t{0, false, 0ull, 0u, 0u};
  if (isnan(v)) { t.special = 1; return t; }
  t.neg = signbit(v);
  if (isinf(v)) { t.special = 2; return t; }
  const unsigned long long scaled = (unsigned long long)rint((double)fabsf(v) * 1e6);
  t.ip = scaled / 1000000ull;
  uint32_t fr = (uint32_t)(scaled % 1000000ull), digits = fr ? 6u : 0u;
  while (fr && fr % 10u == 0u) { fr /= 10u; digits--; }
  t.frac = fr; t.frac_digits = digits;
  return t;
}
__device__ __forceinline__ uint32_t dec_digits64(unsigned long long v) {
  uint32_t d = 1;
  while (v >= 10ull) { v /= 10ull; d++; }
  return d;
}
__device__ __forceinline__ uint32_t f32_len(const F32Text &t) {
  if (t.special == 1) return 3u;
  if (t.special == 2) return t.neg ? 4u : 3u;
  return (t.neg ? 1u : 0u) + dec_digits64(t.ip) + (t.frac_digits ? 1u + t.frac_digits : 0u);
}
__device__ __forceinline__ char *put_f32(char *p, const F32Text &t) {
  if (t.special == 1) { *p++ = 'N'; *p++ = 'a'; *p++ = 'N'; return p; }
  if (t.neg) *p++ = '-';
  if (t.special == 2) { *p++ = 'i'; *p++ = 'n'; *p++ = 'f'; return p; }
  const uint32_t id = dec_digits64(t.ip);
  unsigned long long v = t.ip;
  for (uint32_t k = id; k > 0; k--) { p[k - 1] = (char)('0' + (uint32_t)(v % 10ull)); v /= 10ull; }
  p += id;
  if (t.frac_digits) { *p++ = '.'; p = put_dec(p, t.frac, t.frac_digits); }
  return p;
}
// gi = m / (m + x + ni + nd), bi = m / (m + (x + ibp + dbp)): i32 sums (wrapping), divided in f32 (paf_out.cpp:262-274)
__device__ __forceinline__ void identities(const Run &x, F32Text &gi, F32Text &bi) {
  const float mf = __int2float_rn((int32_t)x.m);
  gi = f32_text(__fdiv_rn(mf, __int2float_rn((int32_t)(x.m + x.x + x.ni + x.nd))));
  bi = f32_text(__fdiv_rn(mf, __int2float_rn((int32_t)(x.m + (x.x + x.ibp + x.dbp)))));
}
// "{qname}\t{first}\t{last}\t{tname}\t{t_first}\t{t_last}\t{range name}\t0\t{+|-}\t+\tgi:f:{}\tbi:f:{}\n" (main.rs:11894-11987)
__global__ __launch_bounds__(256) void text_len_kernel(const Run *__restrict__ runs, uint32_t n, TextTables t, uint32_t *__restrict__ len) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const Run x = runs[r];
  const uint32_t qs = seq_shift(t, x.qid), ts = seq_shift(t, x.tid);
  const bool f = x.q_first <= x.q_last;
  const uint32_t first = (uint32_t)(f ? x.q_first : x.q_last) + qs, last = (uint32_t)(f ? x.q_last : x.q_first) + qs;
  F32Text gi, bi;
  identities(x, gi, bi);
  len[r] = seq_text_len(t, x.qid) + dec_digits(first) + dec_digits(last) + seq_text_len(t, x.tid) + dec_digits((uint32_t)x.t_first + ts) +
           dec_digits((uint32_t)x.t_last + ts) + (t.rname_off[x.range + 1] - t.rname_off[x.range]) + f32_len(gi) + f32_len(bi) +
           12u /* tabs and the newline */ + 3u /* 0, strand, + */ + 10u /* gi:f: bi:f: */;
}
__global__ __launch_bounds__(256) void text_write_kernel(const Run *__restrict__ runs, uint32_t n, TextTables t,
                                                         const unsigned long long *__restrict__ off, unsigned long long base, char *__restrict__ out) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const Run x = runs[r];
  char *p = out + (off[r] - base);
  const uint32_t qs = seq_shift(t, x.qid), ts = seq_shift(t, x.tid);
  const bool f = x.q_first <= x.q_last;
  const uint32_t first = (uint32_t)(f ? x.q_first : x.q_last) + qs, last = (uint32_t)(f ? x.q_last : x.q_first) + qs;
  const uint32_t tf = (uint32_t)x.t_first + ts, tl = (uint32_t)x.t_last + ts;
  F32Text gi, bi;
  identities(x, gi, bi);
  p = put_seq(p, t, x.qid); *p++ = '\t';
  p = put_dec(p, first, dec_digits(first)); *p++ = '\t';
  p = put_dec(p, last, dec_digits(last)); *p++ = '\t';
  p = put_seq(p, t, x.tid); *p++ = '\t';
  p = put_dec(p, tf, dec_digits(tf)); *p++ = '\t';
  p = put_dec(p, tl, dec_digits(tl)); *p++ = '\t';
  p = put_range_name(p, t, x.range);
  *p++ = '\t'; *p++ = '0'; *p++ = '\t'; *p++ = f ? '+' : '-'; *p++ = '\t'; *p++ = '+'; *p++ = '\t';
  *p++ = 'g'; *p++ = 'i'; *p++ = ':'; *p++ = 'f'; *p++ = ':';
  p = put_f32(p, gi);
  *p++ = '\t'; *p++ = 'b'; *p++ = 'i'; *p++ = ':'; *p++ = 'f'; *p++ = ':';
  p = put_f32(p, bi);
  *p++ = '\n';
}

// (the lanes per row come from option "bedpe_group_log2"; DESIGN 5.5 has the measurement behind its default)
template <unsigned G> void launch_summary(const uint32_t *row_range, const uint32_t *offsets, const unsigned long long *coff, const uint32_t *pool,
                                          uint32_t n, RowSum *sum, Control *ctl, hipStream_t s) {
  summary_kernel<G><<<cdiv(n, 256u / G), 256, 0, s>>>(row_range, offsets, coff, pool, n, sum, ctl);
}

// every range has its own first row, the one that is dropped (h_off: the ranges' first rows, n_ranges + 1)
void require_rows(const std::vector<uint32_t> &h_off) {
  for (size_t q = 0; q + 1 < h_off.size(); q++)
    if (h_off[q + 1] == h_off[q]) throw Error{IMPG_E_INVALID, "no result row to drop (the reference panics in Vec::remove(0))"};
}
// What the summary, order and link stages leave on the device.  BEDPE needs only the run records and drops the rest when
// merge_rows returns; PAF reads the summaries, the order and the heads again for its CIGARs (PafChunk, below).
struct Merged {
  DevBuf sum, ctl, head, run_pos;
  prims::KeySort ks;
  const uint32_t *perm = nullptr;  // the kept rows in sorted order (emission order when nothing is sorted)
  uint32_t m = 0, n_runs = 0;      // rows after the drop, lines
  Control counts{};                // the stages' counters, home
  explicit Merged(BufPool *pool) : ks(pool) { for (DevBuf *b : {&sum, &ctl, &head, &run_pos}) b->pool = pool; }
};
// R: n rows grouped by range in emission order, range q's at [d_offsets[q], d_offsets[q + 1]), none of the ranges empty;
// row r's ops at d_pool[d_coff[r] .. d_coff[r + 1]).  The run records go to `out`; M.m, M.n_runs and M.counts say what ran.
void merge_rows(Engine &E, const impg_gpu_index &ix, ConstRows R, uint32_t n, uint32_t n_ranges, const uint32_t *d_offsets,
                const unsigned long long *d_coff, const uint32_t *d_pool, int32_t merge_distance, DevBuf &out, Merged &M) {
  hipStream_t s = E.stream;
  const bool sorted = merge_distance >= 0;  // (a negative distance: neither a sort nor a merge, emission order)
  const unsigned seq_bits = bits_for(ix.view.n_seq), q_bits = bits_for(n_ranges);
  if (sorted && (33 + seq_bits > 64 || q_bits + seq_bits > 64))
    throw Error{IMPG_E_UNSUPPORTED, "too many sequences for the device-side BEDPE merge (use impg_gpu_results_paf)"};
  DevBuf &sum = M.sum, &ctl = M.ctl;
  const uint32_t m = M.m = n - n_ranges;  // rows after the drop
  if (!m) return;
  ctl.reserve(256);
  IMPG_HIP(hipMemsetAsync(ctl.p, 0, sizeof(Control), s));
  Control *d_ctl = ctl.as<Control>();
  // ---- summaries -----------------------------------------------------------------------------------------------------
  sum.reserve((size_t)n * sizeof(RowSum));
  RowSum *d_sum = sum.as<RowSum>();
  switch (E.opt.bedpe_group_log2) {
    case 3: launch_summary<8>(R.q, d_offsets, d_coff, d_pool, n, d_sum, d_ctl, s); break;
    case 4: launch_summary<16>(R.q, d_offsets, d_coff, d_pool, n, d_sum, d_ctl, s); break;
    case 5: launch_summary<32>(R.q, d_offsets, d_coff, d_pool, n, d_sum, d_ctl, s); break;
    case 6: launch_summary<64>(R.q, d_offsets, d_coff, d_pool, n, d_sum, d_ctl, s); break;
    default: launch_summary<4>(R.q, d_offsets, d_coff, d_pool, n, d_sum, d_ctl, s); break;
  }
  // ---- order -----------------------------------------------------------------------------------------------------------
  prims::KeySort &ks = M.ks;
  DevBuf k_t, k_mid, k_hi;
  DevBuf &head = M.head, &run_pos = M.run_pos;
  for (DevBuf *b : {&k_t, &k_mid, &k_hi}) b->pool = &E.level_pool;
  const size_t mb4 = (size_t)m * 4;
  ks.perm.reserve(mb4);
  if (sorted) { k_t.reserve((size_t)n * 4); k_mid.reserve((size_t)n * 8); k_hi.reserve((size_t)n * 8); }
  keys_kernel<<<cdiv(n, 256), 256, 0, s>>>(R, d_offsets, n, seq_bits, sorted ? 1 : 0, k_t.as<uint32_t>(), k_mid.as<unsigned long long>(),
                                           k_hi.as<unsigned long long>(), ks.perm.as<uint32_t>(), d_ctl);
  const uint32_t *perm = ks.perm.as<uint32_t>();
  if (sorted && m > 1) {
    // least significant key first: t_first | (forward?, q start, target seq) | (range, query seq); the keys stand at the
    // rows' indices and ks.perm lists the kept rows, so every pass gathers
    ks.run({{k_t.p, false, 32}, {k_mid.p, true, 33 + seq_bits}, {k_hi.p, true, q_bits + seq_bits}}, /*first_in_order=*/false, m, s);
    perm = ks.order;
  }
  M.perm = perm;
  // ---- link and reduce -------------------------------------------------------------------------------------------------
  head.reserve(mb4); run_pos.reserve(mb4);
  heads_kernel<<<cdiv(m, 256), 256, 0, s>>>(R, perm, m, merge_distance, head.as<uint32_t>());
  const uint32_t n_runs = (uint32_t)E.scan(head.as<uint32_t>(), run_pos.as<uint32_t>(), m);
  // the flags are home with the scan's synchronisation behind them: refuse before a run record exists
  Control &h_ctl = M.counts;
  IMPG_HIP(hipMemcpyAsync(&h_ctl, ctl.p, sizeof(Control), hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipStreamSynchronize(s));
  if (h_ctl.flags[FLAG_NO_CIGAR]) throw Error{IMPG_E_UNSUPPORTED, "a result row without CIGAR"};
  if (h_ctl.flags[FLAG_TARGET_REVERSE]) throw Error{IMPG_E_INVALID, "Target intervals should always be in forward!"};
  out.reserve((size_t)n_runs * sizeof(Run) + 256);
  IMPG_HIP(hipMemsetAsync(out.p, 0, (size_t)n_runs * sizeof(Run), s));
  reduce_kernel<<<cdiv(m, 256), 256, 0, s>>>(R, sum.as<RowSum>(), perm, head.as<uint32_t>(), run_pos.as<uint32_t>(), m, merge_distance,
                                             out.as<Run>(), d_ctl);
  IMPG_HIP(hipMemcpyAsync(&h_ctl, ctl.p, sizeof(Control), hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipStreamSynchronize(s));  // (the key buffers of this function go back to the pool here)
  M.n_runs = n_runs;
}
// BEDPE's use of it: the stages' buffers go back to the pool on return, the counters into the handle's bedpe_* ones
uint32_t merge_rows_bedpe(Engine &E, const impg_gpu_index &ix, ConstRows R, uint32_t n, uint32_t n_ranges, const uint32_t *d_offsets,
                          const unsigned long long *d_coff, const uint32_t *d_pool, int32_t merge_distance, DevBuf &out) {
  Merged M(&E.level_pool);
  ix.bedpe_stats[BEDPE_ROWS] += n - n_ranges;
  merge_rows(E, ix, R, n, n_ranges, d_offsets, d_coff, d_pool, merge_distance, out, M);
  ix.bedpe_stats[BEDPE_RUNS] += M.n_runs;
  ix.bedpe_stats[BEDPE_SUMMARY_OPS] += M.counts.ctr[CTR_SUMMARY_OPS];
  ix.bedpe_stats[BEDPE_JOINS_CONTIGUOUS] += M.counts.ctr[CTR_JOINS_CONTIGUOUS];
  ix.bedpe_stats[BEDPE_JOINS_GAP] += M.counts.ctr[CTR_JOINS_GAP];
  ix.bedpe_stats[BEDPE_FUSED_OPS] += M.counts.ctr[CTR_FUSED_OPS];
  return M.n_runs;
}

// The rows of a chunk and their CIGARs where the stages above take them: range-major, the reference's emission order
// within a range (rows_device.hip).  Returns the number of rows; the levels' memory goes back to the pool.
uint32_t place_rows(Engine &E, uint32_t n_ranges, const impg_gpu_params_t &p, std::vector<std::unique_ptr<LevelBufs>> &levels, DevBuf &self_dev,
                    DevRows &rows, DevBuf &coff, DevBuf &pool, DevBuf &offsets) {
  hipStream_t s = E.stream;
  DevBuf clen;
  clen.pool = &E.level_pool;
  uint32_t n = 0;
  {
    RowPlan pl;  // (its tables go back to the pool at the end of this block, before the sorts take their memory)
    plan_rows(E, n_ranges, p, levels, self_dev, /*plain_retain=*/true, pl);
    n = pl.n_rows;
    std::vector<uint32_t> h_off((size_t)n_ranges + 1);
    IMPG_HIP(hipMemcpyAsync(h_off.data(), pl.offsets.p, ((size_t)n_ranges + 1) * 4, hipMemcpyDeviceToHost, s));
    IMPG_HIP(hipStreamSynchronize(s));
    require_rows(h_off);
    rows.reserve(n); clen.reserve((size_t)n * 4);
    scatter_rows(E, levels, pl, rows.sinks(clen.as<uint32_t>()));
    (void)build_row_cigars(E, levels, pl, clen, coff, pool);
    offsets.reserve(((size_t)n_ranges + 1) * 4);
    IMPG_HIP(hipMemcpyAsync(offsets.p, pl.offsets.p, ((size_t)n_ranges + 1) * 4, hipMemcpyDeviceToDevice, s));
    IMPG_HIP(hipStreamSynchronize(s));
  }
  // the levels' slots and slices are not needed any more: give their memory back before the sorts take theirs
  levels.clear();
  return n;
}
// rows and CIGARs the caller brings (the self-tests), uploaded as they are; row_range does not decrease
uint32_t upload_rows(Engine &E, const impg_gpu_interval_t *rows, const uint32_t *row_range, uint32_t n, uint32_t n_ranges, const uint64_t *cigar_off,
                     const uint32_t *cigar_ops, DevRows &dev, DevBuf &coff, DevBuf &pool, DevBuf &offsets) {
  hipStream_t s = E.stream;
  std::vector<uint32_t> h_off((size_t)n_ranges + 1, 0);
  for (uint32_t i = 0; i < n; i++) h_off[row_range[i] + 1]++;
  for (uint32_t q = 0; q < n_ranges; q++) h_off[q + 1] += h_off[q];
  require_rows(h_off);
  const uint64_t n_ops = cigar_off[n];
  coff.reserve(((size_t)n + 1) * 8); pool.reserve(std::max<size_t>(n_ops * 4, 256)); offsets.reserve(((size_t)n_ranges + 1) * 4);
  IMPG_HIP(hipMemcpyAsync(coff.p, cigar_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
  if (n_ops) IMPG_HIP(hipMemcpyAsync(pool.p, cigar_ops, n_ops * 4, hipMemcpyHostToDevice, s));
  IMPG_HIP(hipMemcpyAsync(offsets.p, h_off.data(), ((size_t)n_ranges + 1) * 4, hipMemcpyHostToDevice, s));
  dev.upload(E, rows, row_range, n);  // (waits for the three copies above too)
  return n;
}
}  // namespace

// Rows of one chunk -> the runs BEDPE prints, left on the device in `out` (grouped by range, in output order); returns
// their number.  levels / self_dev: what Engine::run kept for the chunk, with store_cigar.  Every refusal is raised here,
// before any of the chunk's text exists.  Counts into the handle's bedpe_* counters.
uint32_t device_bedpe_rows(Engine &E, const impg_gpu_index &ix, uint32_t n_ranges, const impg_gpu_params_t &p, int32_t merge_distance,
                           std::vector<std::unique_ptr<LevelBufs>> &levels, DevBuf &self_dev, DevBuf &out) {
  DevRows rows(&E.level_pool);
  DevBuf coff, pool, offsets;
  for (DevBuf *b : {&coff, &pool, &offsets}) b->pool = &E.level_pool;
  const uint32_t n = place_rows(E, n_ranges, p, levels, self_dev, rows, coff, pool, offsets);
  return merge_rows_bedpe(E, ix, rows.view(), n, n_ranges, offsets.as<uint32_t>(), coff.as<unsigned long long>(), pool.as<uint32_t>(), merge_distance, out);
}

// The merge and the text on rows and CIGARs the caller brings (impg_gpu_selftest_bedpe_rows): uploaded as they are, then
// merge_rows and device_bedpe_text as a chunk of a query runs them.  row_range does not decrease; text: appended to.
void device_bedpe_selftest(Engine &E, const impg_gpu_index &ix, const impg_gpu_interval_t *rows, const uint32_t *row_range, uint32_t n,
                           uint32_t n_ranges, const uint64_t *cigar_off, const uint32_t *cigar_ops, int32_t merge_distance, bool original_coords,
                           const std::vector<std::string> &rnames, std::string &text) {
  DevRows dev;
  DevBuf coff, pool, offsets, out;
  upload_rows(E, rows, row_range, n, n_ranges, cigar_off, cigar_ops, dev, coff, pool, offsets);
  const uint32_t n_runs = merge_rows_bedpe(E, ix, dev.view(), n, n_ranges, offsets.as<uint32_t>(), coff.as<unsigned long long>(), pool.as<uint32_t>(),
                                           merge_distance, out);
  device_bedpe_text(E, ix, out, n_runs, n_ranges, rnames, original_coords, [&](const char *p, size_t k) { text.append(p, k); });
}

// The runs of a chunk as text (text_device.hpp)
void device_bedpe_text(Engine &E, const impg_gpu_index &ix, const DevBuf &runs, uint32_t n_runs, uint32_t n_ranges,
                       const std::vector<std::string> &rnames, bool original_coords, const std::function<void(const char *, size_t)> &sink) {
  device_rows_text<Run, text_len_kernel, text_write_kernel>(E, ix, runs, n_runs, n_ranges, rnames, original_coords, sink, "BEDPE",
                                                            ix.bedpe_stats[BEDPE_TEXT_PIECES], ix.bedpe_stats[BEDPE_TEXT_BYTES]);
}

// PAF: the same rows, summaries, order, link and run records, then the merged CIGARs themselves as cg:Z
#include "paf_device.inc"

}  // namespace impg
