// PAF post-processing on the device (part of bedpe_device.hip, inside namespace impg): what output_results_paf
// (src/main.rs:11989-12103) prints after merge_adjusted_intervals.  The summary, order and link stages and the run records
// are BEDPE's (merge_rows); what PAF adds is the merged CIGAR itself -- the concatenation across a run with
// merge_consecutive_cigar_ops (main.rs:13014-13035) over it -- printed as cg:Z without a sequential fold (DESIGN 5.5):
//
//   text order  a run's rows print in sorted order when it is forward and in reverse sorted order when it is reverse (the
//               reference prepends there).  Runs keep the sorted order of their heads.
//   elements    element t of a run = the gap ops of the join between text rows t-1 and t ([qd I] [td D], in that order on
//               both strands) followed by row t's own ops.  A run of one row prints its ops raw.  In a longer run every
//               maximal group of adjacent ops with one code prints as one op -- across element borders and through whole
//               elements.  A group belongs to the element it starts in.
//   scan        element t's last group goes on into the elements behind it for ext[t] bases: the leading group of the
//               concatenation of elements t+1 .., if its code is t's last code.  (lead_code, lead_len, all_same) of a
//               concatenation is an associative function of its parts, so all suffixes come from one segmented scan.
//   cg          G lanes stride over an element's ops; a segmented running sum is carried across steps; the lane holding a
//               group's last op knows the group's length and counts (first pass) or writes (second pass) its text.
// No lane's work grows with a run's length in rows.  One lane walks a row's LEADING group (elements_kernel), and a row
// with very many ops keeps its G lanes for ops / G steps, as in BEDPE's summary.
namespace {

struct PafControl {
  uint32_t flags[2];            // [0]: a line of 2^32 bytes or more
  unsigned long long ctr[2];    // ops printed, elements that print nothing
};
enum { ELEM_FIRST = 1u, ELEM_RAW = 2u, ELEM_STARTS = 4u, ELEM_LAST = 8u, ELEM_LAST_CODE_SHIFT = 4 };

// What the scan carries about a string of ops: bit 63 = a segment starts here, bit 35 = all_same (the string is one group),
// bits 34..32 = the leading group's code, bits 31..0 = its summed length.
constexpr unsigned long long SV_HEAD = 1ull << 63, SV_SAME = 1ull << 35;
__host__ __device__ inline uint32_t sv_code(unsigned long long v) { return (uint32_t)(v >> 32) & 7u; }
// The elements stand in REVERSE text order, so that the suffixes are an inclusive scan from the left: `right` is the
// element in front (a), `left` the summary of everything behind it (b).  (a . b).lead_len = a.lead_len + (a.all_same &&
// b.lead_code == a.lead_code ? b.lead_len : 0); a segment's start (the LAST element of a run) takes nothing from the left.
struct LeadCompose {
  __host__ __device__ unsigned long long operator()(unsigned long long left, unsigned long long right) const {
    if (right & SV_HEAD) return right;
    const bool through = (right & SV_SAME) && sv_code(right) == sv_code(left);
    const uint32_t len = (uint32_t)right + (through ? (uint32_t)left : 0u);
    return (left & SV_HEAD) | ((through && (left & SV_SAME)) ? SV_SAME : 0ull) | ((unsigned long long)sv_code(right) << 32) | len;
  }
};

// run_start[r] = the sorted position of run r's head; run_start[n_runs] = m
__global__ __launch_bounds__(256) void run_start_kernel(const uint32_t *__restrict__ head, const uint32_t *__restrict__ run_pos, uint32_t m,
                                                        uint32_t n_runs, uint32_t *__restrict__ run_start) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= m) return;
  if (head[k]) run_start[run_pos[k]] = k;
  if (k == 0) run_start[n_runs] = m;
}

// One thread per sorted row: its text position t (a reverse run is flipped inside [run_start[r], run_start[r + 1])), the gap
// of the join in front of it, and the element's summary at sv[m - 1 - t].  elem[t] = {row, qd, td, ELEM_* | last code << 4}.
__global__ __launch_bounds__(256) void elements_kernel(ConstRows R, const RowSum *__restrict__ sum, const unsigned long long *__restrict__ coff,
                                                       const uint32_t *__restrict__ pool, const uint32_t *__restrict__ perm,
                                                       const uint32_t *__restrict__ head, const uint32_t *__restrict__ run_pos,
                                                       const uint32_t *__restrict__ run_start, uint32_t m, int32_t d, uint4 *__restrict__ elem,
                                                       uint32_t *__restrict__ erun, unsigned long long *__restrict__ sv) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= m) return;
  const uint32_t run = run_pos[k] + head[k] - 1u;
  const uint32_t s0 = run_start[run], s1 = run_start[run + 1];
  const uint32_t r = perm[k];
  const int4 c = R.c[r];
  const bool f = c.x <= c.y;
  const uint32_t t = f ? k : s0 + (s1 - 1u - k);
  const bool first = t == s0, last = t + 1u == s1;
  uint32_t qd = 0, td = 0, before = 7u;
  if (!first) {
    // the row in front of it in the text: its predecessor in sorted order when forward, its successor when reverse; the
    // join is the one heads_kernel tested between the two sorted neighbours
    const uint32_t a = f ? perm[k - 1] : r, b = f ? r : perm[k + 1];
    bool jf;
    int32_t jq = 0, jt = 0;
    (void)join_kind(R, a, b, d, jf, jq, jt);
    qd = (uint32_t)jq; td = (uint32_t)jt;
    before = sum[f ? a : b].nd_last >> 29;
  }
  // the row's leading group (one lane: it ends at the first op of another code)
  const unsigned long long a0 = coff[r];
  const uint32_t len = (uint32_t)(coff[r + 1] - a0);
  const uint32_t *ops = pool + a0;
  uint32_t c0 = 7u, l0 = 0, j = 0;
  if (len) { c0 = ops[0] >> 29; l0 = ops[0] & OP_LEN_MASK; j = 1; }
  while (j < len && (ops[j] >> 29) == c0) { l0 += ops[j] & OP_LEN_MASK; j++; }
  const bool same0 = j == len;
  uint32_t lead_code = c0, lead_len = l0;
  bool all_same = same0;
  if (qd > 0) {
    lead_code = 2u; lead_len = qd; all_same = false;
    if (td == 0 && c0 == 2u) { lead_len += l0; all_same = same0; }
  } else if (td > 0) {
    lead_code = 3u; lead_len = td; all_same = false;
    if (c0 == 3u) { lead_len += l0; all_same = same0; }
  }
  const bool starts = first || before != lead_code;
  elem[t] = make_uint4(r, qd, td, (first ? ELEM_FIRST : 0u) | (s1 - s0 == 1u ? ELEM_RAW : 0u) | (starts ? ELEM_STARTS : 0u) | (last ? ELEM_LAST : 0u) |
                                      (sum[r].nd_last >> 29) << ELEM_LAST_CODE_SHIFT);
  erun[t] = run;
  sv[m - 1u - t] = (last ? SV_HEAD : 0ull) | (all_same ? SV_SAME : 0ull) | ((unsigned long long)lead_code << 32) | lead_len;
}

__device__ __forceinline__ char op_char(uint32_t code) { return code < 5u ? "=XIDM"[code] : '?'; }

// ---- cg --------------------------------------------------------------------------------------------------------------
// G lanes per element over its ops: the join's gap ops, then the row's stretch of the pool (coalesced).  The lane holding
// op k gets op k-1's code from its neighbour (the group's last lane of the step before for lane 0) and op k+1's from the
// other neighbour (lane G-1 reads it).  A segmented inclusive sum over the lanes, carried across steps, gives the lane of
// a group's last op the group's length; the element's last group takes ext on top.  The element's first group is
// skipped unless it starts here.  WRITE = false: ebytes[t] = the element's bytes, the counters.  WRITE = true: the text,
// element t at its line's start + pre[run] + (eoff[t] - eoff[the run's first element]).
template <unsigned G, bool WRITE>
__global__ __launch_bounds__(256) void cg_kernel(const uint4 *__restrict__ elem, const uint32_t *__restrict__ erun, const unsigned long long *__restrict__ coff,
                                                 const uint32_t *__restrict__ pool, const unsigned long long *__restrict__ sv, uint32_t m, uint32_t e0,
                                                 uint32_t e1, uint32_t *__restrict__ ebytes, PafControl *__restrict__ ctl,
                                                 const unsigned long long *__restrict__ eoff, const uint32_t *__restrict__ run_start,
                                                 const uint32_t *__restrict__ pre, const unsigned long long *__restrict__ off, uint32_t r0,
                                                 unsigned long long base, char *__restrict__ out) {
  __shared__ unsigned long long block_ctr[2];  // ops printed, elements that print nothing
  if (!WRITE) {
    if (threadIdx.x < 2) block_ctr[threadIdx.x] = 0;
    __syncthreads();
  }
  const unsigned long long et = (unsigned long long)e0 + (unsigned long long)blockIdx.x * (256u / G) + threadIdx.x / G;
  const uint32_t lane = threadIdx.x % G;
  if (et < e1) {
    const uint32_t t = (uint32_t)et;
    const uint4 e = elem[t];
    const uint32_t qd = e.y, td = e.z;
    const bool raw = e.w & ELEM_RAW, starts = e.w & ELEM_STARTS;
    const unsigned long long a0 = coff[e.x];
    const uint32_t len = (uint32_t)(coff[e.x + 1] - a0);
    const uint32_t *ops = pool + a0;
    const uint32_t n_gap = (qd > 0) + (td > 0), nv = n_gap + len;
    const uint32_t g0 = qd > 0 ? (2u << 29 | qd) : (3u << 29 | td), g1 = 3u << 29 | td;
    uint32_t ext = 0;
    if (!raw && !(e.w & ELEM_LAST)) {
      const unsigned long long behind = sv[m - 2u - t];  // the summary of elements t+1 .. of the run
      if (sv_code(behind) == ((e.w >> ELEM_LAST_CODE_SHIFT) & 7u)) ext = (uint32_t)behind;
    }
    auto vop = [&](uint32_t k) -> uint32_t { return k < n_gap ? (k == 0 ? g0 : g1) : k < nv ? ops[k - n_gap] : OP_PAD; };
    char *dst = nullptr;
    if (WRITE) {
      const uint32_t run = erun[t];
      dst = out + (off[run - r0] - base) + pre[run] + (eoff[t] - eoff[run_start[run]]);
    }
    uint32_t carry_code = 7u, carry_sum = 0, carry_bytes = 0, n_print = 0;
    bool carry_nf = false;
    for (uint32_t step = 0; step < nv; step += G) {
      const uint32_t k = step + lane;
      const uint32_t op = vop(k);
      const uint32_t code = op >> 29, l = op & OP_LEN_MASK;
      uint32_t prev = __shfl_up(code, 1, G), next = __shfl_down(code, 1, G);
      if (lane == 0) prev = carry_code;
      if (lane == G - 1) next = vop(k + 1) >> 29;
      const bool start = raw || code != prev;            // (k == 0: prev is 7)
      const bool end = k < nv && (raw || code != next);  // (k == nv - 1: next is 7)
      // segmented inclusive sum of the lengths, and "a group started at an op behind the element's first" (nf)
      uint32_t s = l;
      bool fl = start, nf = start && k > 0;
      for (unsigned o = 1; o < G; o <<= 1) {
        const uint32_t ps = __shfl_up(s, o, G);
        const int pf = __shfl_up((int)fl, o, G), pn = __shfl_up((int)nf, o, G);
        if (lane >= o) {
          if (!fl) s += ps;
          fl = fl || pf;
          nf = nf || pn;
        }
      }
      if (!fl) s += carry_sum;
      nf = nf || carry_nf;
      carry_sum = __shfl(s, G - 1, G);
      carry_nf = __shfl((int)nf, G - 1, G) != 0;
      carry_code = __shfl(code, G - 1, G);
      const bool emit = end && (raw || nf || starts);
      const uint32_t glen = s + (k + 1u == nv ? ext : 0u);
      const uint32_t digits = dec_digits(glen);
      const uint32_t nb = emit ? digits + 1u : 0u;
      uint32_t inc = nb;
      for (unsigned o = 1; o < G; o <<= 1) {
        const uint32_t pi = __shfl_up(inc, o, G);
        if (lane >= o) inc += pi;
      }
      if (WRITE && emit) {
        char *p = put_dec(dst + carry_bytes + (inc - nb), glen, digits);
        *p = op_char(code);
      }
      carry_bytes += __shfl(inc, G - 1, G);
      n_print += emit;
    }
    if (!WRITE) {
      for (unsigned o = G / 2; o; o >>= 1) n_print += __shfl_xor(n_print, o, G);
      if (lane == 0) {
        ebytes[t] = carry_bytes;
        if (n_print) atomicAdd(&block_ctr[0], (unsigned long long)n_print);
        else atomicAdd(&block_ctr[1], 1ull);
      }
    }
  }
  if (!WRITE) {
    __syncthreads();
    if (threadIdx.x < 2 && block_ctr[threadIdx.x]) atomicAdd(&ctl->ctr[threadIdx.x], block_ctr[threadIdx.x]);
  }
}

// ---- the line's fixed fields -------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t i32_len(int32_t v) { return v < 0 ? 1u + dec_digits(0u - (uint32_t)v) : dec_digits((uint32_t)v); }
__device__ __forceinline__ char *put_i32(char *p, int32_t v) {
  uint32_t u = (uint32_t)v;
  if (v < 0) { *p++ = '-'; u = 0u - u; }
  return put_dec(p, u, dec_digits(u));
}
// "{qname}\t{qlen}\t{first}\t{last}\t{+|-}\t{tname}\t{tlen}\t{t_first}\t{t_last}\t{matches}\t{block len}\t255\tgi:f:{}\tbi:f:{}\t
//  cg:Z:{ops}\tan:Z:{range name}\n" (main.rs:11989-12103); matches and block length print as i32
constexpr uint32_t PAF_PRE_FIXED = 14u /* tabs */ + 1u /* strand */ + 3u /* 255 */ + 15u /* gi:f: bi:f: cg:Z: */, PAF_POST_FIXED = 7u /* \tan:Z: \n */;
__global__ __launch_bounds__(256) void paf_len_kernel(const Run *__restrict__ runs, uint32_t n, TextTables t, const unsigned long long *__restrict__ eoff,
                                                      const uint32_t *__restrict__ run_start, uint32_t *__restrict__ len, uint32_t *__restrict__ pre,
                                                      PafControl *__restrict__ ctl) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const Run x = runs[r];
  const uint32_t qs = seq_shift(t, x.qid), ts = seq_shift(t, x.tid);
  const bool f = x.q_first <= x.q_last;
  const uint32_t first = (uint32_t)(f ? x.q_first : x.q_last) + qs, last = (uint32_t)(f ? x.q_last : x.q_first) + qs;
  F32Text gi, bi;
  identities(x, gi, bi);
  const uint32_t head = seq_text_len(t, x.qid) + dec_digits(seq_len_of(t, x.qid)) + dec_digits(first) + dec_digits(last) + seq_text_len(t, x.tid) +
                        dec_digits(seq_len_of(t, x.tid)) + dec_digits((uint32_t)x.t_first + ts) + dec_digits((uint32_t)x.t_last + ts) +
                        i32_len((int32_t)x.m) + i32_len((int32_t)(x.m + x.x + x.ibp + x.dbp)) + f32_len(gi) + f32_len(bi) + PAF_PRE_FIXED;
  const unsigned long long total = (unsigned long long)head + (eoff[run_start[r + 1]] - eoff[run_start[r]]) + PAF_POST_FIXED +
                                   (t.rname_off[x.range + 1] - t.rname_off[x.range]);
  if (total > 0xFFFFFFFFull) ctl->flags[0] = 1u;
  pre[r] = head;
  len[r] = (uint32_t)total;
}
// runs / pre / run_start: at the piece's first run; off[r]: the line's start in the whole text
__global__ __launch_bounds__(256) void paf_fields_kernel(const Run *__restrict__ runs, uint32_t n, TextTables t, const unsigned long long *__restrict__ off,
                                                         unsigned long long base, char *__restrict__ out, const uint32_t *__restrict__ pre,
                                                         const unsigned long long *__restrict__ eoff, const uint32_t *__restrict__ run_start) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const Run x = runs[r];
  char *line = out + (off[r] - base), *p = line;
  const uint32_t qs = seq_shift(t, x.qid), ts = seq_shift(t, x.tid);
  const bool f = x.q_first <= x.q_last;
  const uint32_t first = (uint32_t)(f ? x.q_first : x.q_last) + qs, last = (uint32_t)(f ? x.q_last : x.q_first) + qs;
  const uint32_t tf = (uint32_t)x.t_first + ts, tl = (uint32_t)x.t_last + ts, ql = seq_len_of(t, x.qid), tlen = seq_len_of(t, x.tid);
  F32Text gi, bi;
  identities(x, gi, bi);
  p = put_seq(p, t, x.qid); *p++ = '\t';
  p = put_dec(p, ql, dec_digits(ql)); *p++ = '\t';
  p = put_dec(p, first, dec_digits(first)); *p++ = '\t';
  p = put_dec(p, last, dec_digits(last)); *p++ = '\t';
  *p++ = f ? '+' : '-'; *p++ = '\t';
  p = put_seq(p, t, x.tid); *p++ = '\t';
  p = put_dec(p, tlen, dec_digits(tlen)); *p++ = '\t';
  p = put_dec(p, tf, dec_digits(tf)); *p++ = '\t';
  p = put_dec(p, tl, dec_digits(tl)); *p++ = '\t';
  p = put_i32(p, (int32_t)x.m); *p++ = '\t';
  p = put_i32(p, (int32_t)(x.m + x.x + x.ibp + x.dbp)); *p++ = '\t';
  *p++ = '2'; *p++ = '5'; *p++ = '5'; *p++ = '\t';
  *p++ = 'g'; *p++ = 'i'; *p++ = ':'; *p++ = 'f'; *p++ = ':';
  p = put_f32(p, gi);
  *p++ = '\t'; *p++ = 'b'; *p++ = 'i'; *p++ = ':'; *p++ = 'f'; *p++ = ':';
  p = put_f32(p, bi);
  *p++ = '\t'; *p++ = 'c'; *p++ = 'g'; *p++ = ':'; *p++ = 'Z'; *p++ = ':';
  // (the cg text between the two parts is cg_kernel's)
  p = line + pre[r] + (eoff[run_start[r + 1]] - eoff[run_start[r]]);
  *p++ = '\t'; *p++ = 'a'; *p++ = 'n'; *p++ = ':'; *p++ = 'Z'; *p++ = ':';
  p = put_range_name(p, t, x.range);
  *p++ = '\n';
}

// (the lanes per element come from option "paf_group_log2"; every value prints the same text)
template <bool WRITE, class... A> void launch_cg(int64_t group_log2, uint32_t n_elem, hipStream_t s, A... a) {
  switch (group_log2) {
    case 3: cg_kernel<8, WRITE><<<cdiv(n_elem, 256u / 8), 256, 0, s>>>(a...); break;
    case 4: cg_kernel<16, WRITE><<<cdiv(n_elem, 256u / 16), 256, 0, s>>>(a...); break;
    case 5: cg_kernel<32, WRITE><<<cdiv(n_elem, 256u / 32), 256, 0, s>>>(a...); break;
    case 6: cg_kernel<64, WRITE><<<cdiv(n_elem, 256u / 64), 256, 0, s>>>(a...); break;
    default: cg_kernel<4, WRITE><<<cdiv(n_elem, 256u / 4), 256, 0, s>>>(a...); break;
  }
}

}  // namespace

// A chunk between its rows call and its text call: the rows, their CIGARs, the run records and the elements
struct PafChunk {
  DevRows rows;
  DevBuf coff, pool, offsets, runs;
  Merged M;
  DevBuf run_start, elem, erun, sv, svs, ebytes, eoff, ctl, tmp;
  std::vector<uint32_t> h_run_start;
  uint32_t n = 0;
  explicit PafChunk(BufPool *bp) : rows(bp), M(bp) {
    for (DevBuf *b : {&coff, &pool, &offsets, &runs, &run_start, &elem, &erun, &sv, &svs, &ebytes, &eoff, &ctl, &tmp}) b->pool = bp;
  }
};
void PafChunkFree::operator()(PafChunk *c) const { delete c; }

namespace {
// C.rows / coff / pool / offsets placed, C.n rows: the merge, then the elements, their suffix summaries and their bytes.
// Every refusal of the chunk but the text buffer's is raised here.  Counts into the handle's paf_* counters.
void paf_elements(Engine &E, const impg_gpu_index &ix, PafChunk &C, uint32_t n_ranges, int32_t merge_distance) {
  typedef unsigned long long u64;
  hipStream_t s = E.stream;
  const ConstRows R = C.rows.view();
  Merged &M = C.M;
  merge_rows(E, ix, R, C.n, n_ranges, C.offsets.as<uint32_t>(), C.coff.as<u64>(), C.pool.as<uint32_t>(), merge_distance, C.runs, M);
  ix.paf_stats[PAF_ROWS] += M.m;
  const uint32_t m = M.m, n_runs = M.n_runs;
  if (!m) return;
  ix.paf_stats[PAF_RUNS] += n_runs;
  ix.paf_stats[PAF_JOINS_CONTIGUOUS] += M.counts.ctr[CTR_JOINS_CONTIGUOUS];
  ix.paf_stats[PAF_JOINS_GAP] += M.counts.ctr[CTR_JOINS_GAP];
  ix.paf_stats[PAF_OPS_READ] += M.counts.ctr[CTR_SUMMARY_OPS];
  C.run_start.reserve(((size_t)n_runs + 1) * 4);
  C.elem.reserve((size_t)m * 16); C.erun.reserve((size_t)m * 4); C.sv.reserve((size_t)m * 8); C.svs.reserve((size_t)m * 8);
  C.ebytes.reserve(((size_t)m + 1) * 4); C.eoff.reserve(((size_t)m + 1) * 8); C.ctl.reserve(256);
  IMPG_HIP(hipMemsetAsync(C.ctl.p, 0, sizeof(PafControl), s));
  IMPG_HIP(hipMemsetAsync(C.ebytes.as<uint32_t>() + m, 0, 4, s));
  run_start_kernel<<<cdiv(m, 256), 256, 0, s>>>(M.head.as<uint32_t>(), M.run_pos.as<uint32_t>(), m, n_runs, C.run_start.as<uint32_t>());
  elements_kernel<<<cdiv(m, 256), 256, 0, s>>>(R, M.sum.as<RowSum>(), C.coff.as<u64>(), C.pool.as<uint32_t>(), M.perm, M.head.as<uint32_t>(),
                                               M.run_pos.as<uint32_t>(), C.run_start.as<uint32_t>(), m, merge_distance, C.elem.as<uint4>(),
                                               C.erun.as<uint32_t>(), C.sv.as<u64>());
  prims::inclusive_scan(C.tmp, (const u64 *)C.sv.as<u64>(), C.svs.as<u64>(), (size_t)m, LeadCompose(), s);
  launch_cg<false>(E.opt.paf_group_log2, m, s, (const uint4 *)C.elem.as<uint4>(), (const uint32_t *)C.erun.as<uint32_t>(), (const u64 *)C.coff.as<u64>(),
                   (const uint32_t *)C.pool.as<uint32_t>(), (const u64 *)C.svs.as<u64>(), m, 0u, m, C.ebytes.as<uint32_t>(), C.ctl.as<PafControl>(),
                   (const u64 *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr, (const u64 *)nullptr, 0u, (u64)0, (char *)nullptr);
  prims::exclusive_sum(C.tmp, (const uint32_t *)C.ebytes.as<uint32_t>(), C.eoff.as<u64>(), (size_t)m + 1, s);
  C.h_run_start.resize((size_t)n_runs + 1);
  PafControl h_ctl;
  IMPG_HIP(hipMemcpyAsync(C.h_run_start.data(), C.run_start.p, ((size_t)n_runs + 1) * 4, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipMemcpyAsync(&h_ctl, C.ctl.p, sizeof(PafControl), hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipStreamSynchronize(s));
  ix.paf_stats[PAF_OPS_PRINTED] += h_ctl.ctr[0];
  ix.paf_stats[PAF_THROUGH_ROWS] += h_ctl.ctr[1];
  // the text needs the rows' ops, the elements and the run records; the merge's own buffers go back to the pool
  for (DevBuf *b : {&M.sum, &M.head, &M.run_pos, &M.ks.perm, &M.ks.spare, &M.ks.stage, &M.ks.tmp, &C.sv, &C.ebytes, &C.tmp}) b->release();
  M.perm = nullptr;
}
}  // namespace

PafChunkPtr device_paf_rows(Engine &E, const impg_gpu_index &ix, uint32_t n_ranges, const impg_gpu_params_t &p, int32_t merge_distance,
                            std::vector<std::unique_ptr<LevelBufs>> &levels, DevBuf &self_dev) {
  PafChunkPtr C(new PafChunk(&E.level_pool));
  C->n = place_rows(E, n_ranges, p, levels, self_dev, C->rows, C->coff, C->pool, C->offsets);
  paf_elements(E, ix, *C, n_ranges, merge_distance);
  return C;
}

// The chunk's lines as text (text_device.hpp): the line lengths from the fixed fields and the elements' bytes, then piece
// by piece the fixed fields of runs [r0, r1) and the cg text of their elements
void device_paf_text(Engine &E, const impg_gpu_index &ix, PafChunk &C, uint32_t n_ranges, const std::vector<std::string> &rnames, bool original_coords,
                     const std::function<void(const char *, size_t)> &sink) {
  typedef unsigned long long u64;
  const uint32_t n_runs = C.M.n_runs, m = C.M.m;
  if (!n_runs) return;
  hipStream_t s = E.stream;
  TextTableBufs tb(E, ix, n_ranges, rnames, original_coords, /*with_lengths=*/true);
  const TextTables t = tb.t;
  DevBuf len, pre;
  len.reserve((size_t)n_runs * 4); pre.reserve((size_t)n_runs * 4);
  paf_len_kernel<<<cdiv(n_runs, 256), 256, 0, s>>>(C.runs.as<Run>(), n_runs, t, C.eoff.as<u64>(), C.run_start.as<uint32_t>(), len.as<uint32_t>(),
                                                   pre.as<uint32_t>(), C.ctl.as<PafControl>());
  PafControl h_ctl;
  IMPG_HIP(hipMemcpyAsync(&h_ctl, C.ctl.p, sizeof(PafControl), hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipStreamSynchronize(s));
  if (h_ctl.flags[0]) throw Error{IMPG_E_UNSUPPORTED, "a single PAF row longer than the text buffer"};
  const int64_t group_log2 = E.opt.paf_group_log2;
  device_text_pieces(E, len.as<uint32_t>(), n_runs, "PAF",
                     [&](uint32_t r0, uint32_t r1, const u64 *off, u64 base, char *out) {
                       paf_fields_kernel<<<cdiv(r1 - r0, 256), 256, 0, s>>>(C.runs.as<Run>() + r0, r1 - r0, t, off, base, out, pre.as<uint32_t>() + r0,
                                                                            C.eoff.as<u64>(), C.run_start.as<uint32_t>() + r0);
                       const uint32_t e0 = C.h_run_start[r0], e1 = C.h_run_start[r1];
                       launch_cg<true>(group_log2, e1 - e0, s, (const uint4 *)C.elem.as<uint4>(), (const uint32_t *)C.erun.as<uint32_t>(),
                                       (const u64 *)C.coff.as<u64>(), (const uint32_t *)C.pool.as<uint32_t>(), (const u64 *)C.svs.as<u64>(), m, e0, e1,
                                       (uint32_t *)nullptr, (PafControl *)nullptr, (const u64 *)C.eoff.as<u64>(),
                                       (const uint32_t *)C.run_start.as<uint32_t>(), (const uint32_t *)pre.as<uint32_t>(), off, r0, base, out);
                     },
                     sink, ix.paf_stats[PAF_TEXT_PIECES], ix.paf_stats[PAF_TEXT_BYTES]);
}

// The merge, the elements and the text on rows and CIGARs the caller brings (impg_gpu_selftest_paf_rows), as a chunk of a
// query runs them.  row_range does not decrease; text: appended to.
void device_paf_selftest(Engine &E, const impg_gpu_index &ix, const impg_gpu_interval_t *rows, const uint32_t *row_range, uint32_t n,
                         uint32_t n_ranges, const uint64_t *cigar_off, const uint32_t *cigar_ops, int32_t merge_distance, bool original_coords,
                         const std::vector<std::string> &rnames, std::string &text) {
  PafChunk C(&E.level_pool);
  C.n = upload_rows(E, rows, row_range, n, n_ranges, cigar_off, cigar_ops, C.rows, C.coff, C.pool, C.offsets);
  paf_elements(E, ix, C, n_ranges, merge_distance);
  device_paf_text(E, ix, C, n_ranges, rnames, original_coords, [&](const char *p, size_t k) { text.append(p, k); });
}
