// The per-query walk: query_transitive_bfs / query_transitive_dfs (impg.rs:2311-2597, :2057-2309) for ONE query by ONE
// workgroup, all levels / all pops in a single launch.  (Included at the end of kernels.hip: it reuses the lookup
// searches, project_pair and replay_hits.)
//
// The batch engine (engine.cpp) advances every query of a batch level by level, a dozen launches and host round
// trips per level: right for 100 000 ranges of a BFS, wrong for the two shapes the reference's callers use most --
//   * one range per call (ImpgIndex::query_transitive_* from partition.rs:359-391, multi_impg.rs:518-530): a BFS
//     `-m 3` paid ~30 launches + ~20 synchronisations = 1.0 ms for 0.05 ms of work;
//   * DFS (and any walk whose steps are single pops): one pop per query per ROUND, every round a launch sequence
//     over all live queries -- a 100 000-range DFS batch took tens of minutes.
// Here a workgroup owns a query from its first lookup to its last row: frontier / stack, visited lists and the
// step's pairs live in the workgroup's slab of HBM (L2-resident), nothing returns to the host in between.
// Workgroups take queries from a shared counter, so a batch of any size runs in one launch.
//
//   step      a set of ranges processed together: a whole BFS level (cut into sub-steps of at most one range per
//             thread and HCAP pairs -- visited updates between sub-steps of a level are exact, the reference applies
//             a level's hits one by one in the same order), or the one range a DFS pop took off the stack
//   lookup    a thread per range: the two lower-bound searches of lookup_count_lane_kernel, window count;
//             a wave per range: hits in visit order (cross-lane bitonic sort of the ranks, as lookup_emit_kernel)
//   project   a thread per pair: project_pair (the same code as project_kernel)
//   update    hits keyed seq << 15 | slot, block bitonic sort (in LDS up to LCAP keys), a thread per sequence
//             replays its hits in slot order on the sequence's list (replay_hits) -- the order dependence of
//             impg.rs:2471-2560 binds per (query, sequence) only; pieces sorted by (sequence, start) and merged
//   DFS       pieces get depth + 1, merge into the sorted stack (existing records first on ties, like the stable
//             sort of impg.rs:2289), neighbours of one sequence merged keeping the first one's depth (:2291-2304)
//
//   masks     masked_regions (impg.rs:2077-2112, :2331-2373; what partition.rs:359-391 passes on every call): the range
//             goes through SortedRanges::insert on a copy of its target's mask list (several self intervals, or
//             none), a sequence's list opens as a copy of the map's
//   grid      a BFS with a depth limit, a handful of queries (the per-call shape): `members` workgroups per query.  The
//             first takes the query up to its last level -- the big one, whose update is dead (impg.rs:2376) -- and
//             publishes that frontier; all members share its ranges out (walk_final_level), two grid-wide hand-offs
//
//   multi     a MultiImpg worklist (multi_impg.rs:796-991): the DFS arm popped at either end, its steps Impg::query calls, a
//             pop's hits in five-key order (walk_body's MULTI); one wave per query, a budget of explored pops
//
// Not taken here (the caller falls back to the batch engine): store_cigar, MultiImpg under a mask, tracepoint
// indexes, more than 2^16 sequences, and any query that outgrows its slab or its pop budget (`overflow`).
struct WRec {
  uint32_t seq;
  int32_t start, end;
  uint32_t depth;
};
constexpr uint32_t WALK_SLOT_BITS = 15;  // pairs per step < 2^15

__host__ __device__ inline size_t walk_align(size_t x) { return (x + 255) & ~(size_t)255; }
struct WalkSlab {  // the carve-up of one workgroup's slab
  uint32_t *tab_off, *tab_len, *tab_cap;
  int2 *vpool;
  WRec *wa, *wb, *wc;
  uint2 *win;
  uint32_t *cnt, *pair_range, *pair_entry, *hqid, *skey, *gflag;
  int4 *hc;
  unsigned long long *sval, *pkey;
  int2 *gp;
  uint32_t *st_off, *st_len, *st_cap;  // DFS: the stack, one start-sorted list per sequence (the top = the last record of the highest sequence)
  int4 *spool;                        // {start, end, depth, -}
};
// (always inlined: as a call, the kernel's slab descriptor -- 23 wave-uniform pointers -- lived in scratch memory and every
// use of one was a load from it, in a kernel that is nothing but dependent loads)
__host__ __device__ __attribute__((always_inline)) inline size_t walk_slab_layout(char *base, uint32_t n_seq, uint32_t T, uint32_t wcap, uint32_t hcap, uint32_t vcap, uint32_t gcap,
                                                   uint32_t scap, WalkSlab *s) {
  size_t o = 0;
  auto take = [&](size_t bytes) { char *p = base ? base + o : nullptr; o += walk_align(bytes); return p; };
  char *p;
  p = take((size_t)n_seq * 4); if (s) s->tab_off = (uint32_t *)p;
  p = take((size_t)n_seq * 4); if (s) s->tab_len = (uint32_t *)p;
  p = take((size_t)n_seq * 4); if (s) s->tab_cap = (uint32_t *)p;
  p = take((size_t)vcap * 8); if (s) s->vpool = (int2 *)p;
  p = take((size_t)wcap * 16); if (s) s->wa = (WRec *)p;
  p = take((size_t)wcap * 16); if (s) s->wb = (WRec *)p;
  p = take((size_t)wcap * 16); if (s) s->wc = (WRec *)p;
  p = take((size_t)T * 8); if (s) s->win = (uint2 *)p;
  p = take((size_t)(T + 1) * 4); if (s) s->cnt = (uint32_t *)p;
  p = take((size_t)hcap * 4); if (s) s->pair_range = (uint32_t *)p;
  p = take((size_t)hcap * 4); if (s) s->pair_entry = (uint32_t *)p;
  p = take((size_t)hcap * 4); if (s) s->hqid = (uint32_t *)p;
  p = take((size_t)hcap * 4); if (s) s->skey = (uint32_t *)p;
  p = take((size_t)(hcap > wcap ? hcap : wcap) * 4); if (s) s->gflag = (uint32_t *)p;  // (heads of hit groups, of piece runs, of stack runs)
  p = take((size_t)hcap * 16); if (s) s->hc = (int4 *)p;
  p = take((size_t)hcap * 8); if (s) s->sval = (unsigned long long *)p;
  p = take((size_t)wcap * 8); if (s) s->pkey = (unsigned long long *)p;
  p = take((size_t)gcap * 8); if (s) s->gp = (int2 *)p;
  p = take((size_t)n_seq * 4); if (s) s->st_off = (uint32_t *)p;
  p = take((size_t)n_seq * 4); if (s) s->st_len = (uint32_t *)p;
  p = take((size_t)n_seq * 4); if (s) s->st_cap = (uint32_t *)p;
  p = take((size_t)scap * 16); if (s) s->spool = (int4 *)p;
  return o;
}

template <uint32_t NW> struct WalkLds {
  uint32_t wsum[NW];
  uint32_t nw, npc, vused, gpused, P, nact, ng, rows_run, flag, tmp, spused;
  int top_seq;  // DFS: highest sequence with a non-empty stack list (-1: the stack is empty)
  WRec top;
  unsigned long long acc_count, acc_cksum;
};

// What the MultiImpg arm keeps beside WalkLds (a struct of its own: the other instantiations' LDS stays as it was)
struct WalkMultiLds {
  int bot_seq;  // lowest sequence with a non-empty stack list, for the pop at the front (0x7FFFFFFF: the stack is empty)
};
// The arm's pop budget.  The reference's worklist always ends (visited lists only grow); a wrong kernel's may not, and a wave
// must not spin on a device that others use.  The headline index's lone `-m 3` call explores 834 pops (of 20 147): the cap is
// three orders above that.  Past it the query gives up with cause bit 256 and the batch engine answers, as for a slab limit.
constexpr uint32_t WALK_POP_BUDGET = 1u << 20;

template <uint32_t NW> __device__ __forceinline__ uint32_t wk_scan(uint32_t x, uint32_t *wsum, uint32_t &total) {
  const uint32_t inc = wave_incl_scan(x);
  const unsigned w = threadIdx.x >> 6;
  if (lane_id() == 63) wsum[w] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (unsigned k = 0; k < NW; k++) { base += k < w ? wsum[k] : 0u; tot += wsum[k]; }
  __syncthreads();
  total = tot;
  return base + inc - x;
}
// exclusive scan of a[0, n) in place; returns the total
template <uint32_t NW> __device__ __forceinline__ uint32_t wk_scan_array(uint32_t *a, uint32_t n, uint32_t *wsum) {
  uint32_t carry = 0;
  for (uint32_t b = 0; b < n; b += NW * 64u) {
    const uint32_t i = b + threadIdx.x;
    const uint32_t x = i < n ? a[i] : 0u;
    uint32_t tot;
    const uint32_t e = wk_scan<NW>(x, wsum, tot);
    if (i < n) a[i] = carry + e;
    carry += tot;
  }
  return carry;
}
// ascending bitonic sort of k[0, np2), np2 a power of two (pad with the type's maximum); k in LDS or global
template <uint32_t NW, class K> __device__ __forceinline__ void wk_sort(K *k, uint32_t np2) {
  for (uint32_t size = 2; size <= np2; size <<= 1)
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t i = threadIdx.x; i < (np2 >> 1); i += NW * 64u) {
        const uint32_t a = 2u * i - (i & (stride - 1u)), b = a + stride;
        const bool asc = (a & size) == 0u;
        const K ka = k[a], kb = k[b];
        if ((ka > kb) == asc) { k[a] = kb; k[b] = ka; }
      }
      __syncthreads();
    }
}
__device__ __forceinline__ uint32_t wk_pow2(uint32_t n) {
  uint32_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

// first index in [l, h) whose value passes (values ascending, the test monotone), h if none: one WAVE, 64 probes a round
// -- a DFS pop's two lower bounds were 14 dependent round trips of one lane, a third of the pop; this is two rounds each
// for anything up to 4 096 entries.  GE: value >= key, else value > key.
template <bool GE>
__device__ __forceinline__ uint32_t wk_wave_first(const int32_t *__restrict__ col, uint32_t l, uint32_t h, int32_t key) {
  const uint32_t lane = lane_id();
  while (h - l > 64u) {
    const uint32_t step = (h - l + 63u) / 64u;
    const uint32_t idx = min(l + (lane + 1u) * step - 1u, h - 1u);
    const int32_t x = col[idx];
    const unsigned long long m = __ballot(GE ? x >= key : x > key);
    if (!m) return h;  // (the last probe is h - 1)
    const uint32_t k = (uint32_t)__ffsll((long long)m) - 1u;
    h = min(l + (k + 1u) * step - 1u, h - 1u);  // passes: the first one is at or before it
    l = l + k * step;                           // (the probe before it, if any, did not pass)
  }
  const bool in = lane < h - l;
  const int32_t x = in ? col[l + lane] : 0;
  const unsigned long long m = __ballot(in && (GE ? x >= key : x > key));
  return m ? l + (uint32_t)__ffsll((long long)m) - 1u : h;
}

// hits of range r (window [lo, ub) of the entry columns) in visit order at pair_*[off ..): one wave (lookup_emit_kernel)
// TR: the transitive lookup's open test on ends_t, else Impg::query's closed one on ends (a MultiImpg step)
template <bool TR = true>
__device__ __forceinline__ void wk_emit_range(const DeviceIndexView &v, uint32_t lo, uint32_t ub, int32_t qs, uint32_t off, uint32_t r,
                                              uint32_t *__restrict__ pair_range, uint32_t *__restrict__ pair_entry) {
  const int32_t *ecol = end_col<TR>(v);
  const unsigned lane = lane_id();
  if (lo >= ub) return;
  if (ub - lo <= 64u) {
    const uint32_t i = lo + lane;
    const bool hit = i < ub && window_hit<TR>(ecol[i], qs);
    const unsigned long long m0 = __ballot(hit);
    uint32_t rk = hit ? (v.sorted_order ? lane : v.rank[i]) : 0xFFFFFFFFu;
    uint32_t who = lane;
#pragma unroll
    for (unsigned k = 2; k <= 64; k <<= 1) {
#pragma unroll
      for (unsigned j = k >> 1; j > 0; j >>= 1) {
        const uint32_t prk = (uint32_t)__shfl_xor((int)rk, (int)j);
        const uint32_t pwho = (uint32_t)__shfl_xor((int)who, (int)j);
        const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
        const bool take = keep_min ? prk < rk : prk > rk;
        rk = take ? prk : rk;
        who = take ? pwho : who;
      }
    }
    if (lane < (unsigned)__popcll(m0)) {
      pair_range[off + lane] = r;
      pair_entry[off + lane] = lo + who;
    }
    return;
  }
  // windows wider than one wave (dense targets): every hit counts the hits with a smaller rank
  for (uint32_t base = lo; base < ub; base += 64u) {
    const uint32_t i = base + lane;
    const bool hit = i < ub && window_hit<TR>(ecol[i], qs);
    const uint32_t rk = hit ? (v.sorted_order ? i - lo : v.rank[i]) : 0xFFFFFFFFu;
    uint32_t pos = 0;
    for (uint32_t b2 = lo; b2 < ub; b2 += 64u) {
      const uint32_t i2 = b2 + lane;
      const bool hit2 = i2 < ub && window_hit<TR>(ecol[i2], qs);
      const uint32_t rk2 = hit2 ? (v.sorted_order ? i2 - lo : v.rank[i2]) : 0xFFFFFFFFu;
      unsigned long long m = __ballot(hit2);
      while (m) {
        const int j = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
        m &= m - 1;
        const uint32_t rj = (uint32_t)__builtin_amdgcn_readlane((int)rk2, j);
        pos += rj < rk;
      }
    }
    if (hit) {
      pair_range[off + pos] = r;
      pair_entry[off + pos] = i;
    }
  }
}

// ---- hand-offs between the workgroups of a query (grid form).  Per-XCD L2s are not coherent and a CU's L1 is never
// refreshed by another CU's stores: the producer drains its stores, one lane releases at agent scope and stores the
// flag with an agent-scope atomic; a consumer polls that one word relaxed, acquires once at agent scope, and the
// workgroup's barrier follows.  Spins are bounded (a member that gives up flags the batch for the batch engine).
typedef __attribute__((address_space(1))) uint32_t wk_gu32;
constexpr unsigned long long WALK_SPIN_TICKS = 400000000ull;  // 4 s of the 100 MHz wall clock
__device__ __forceinline__ uint32_t wk_load(const uint32_t *p) {
  return __hip_atomic_load((wk_gu32 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// every storing wave calls this (block-uniformly); `word` gets `value` (store) or is incremented (add)
__device__ __forceinline__ void wk_publish(uint32_t *word, uint32_t value, bool add) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (add) (void)__hip_atomic_fetch_add((wk_gu32 *)word, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else __hip_atomic_store((wk_gu32 *)word, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
// the whole workgroup waits until *word >= want (one lane polls); false: gave up
__device__ __forceinline__ bool wk_wait(const uint32_t *word, uint32_t want, uint32_t *lds_word) {
  if (threadIdx.x == 0) {
    const unsigned long long t0 = wall_clock64();
    uint32_t x;
    for (;;) {
      x = wk_load(word);
      if (x >= want) break;
      __builtin_amdgcn_s_sleep(8);
      if (wall_clock64() - t0 > WALK_SPIN_TICKS) { x = 0xFFFFFFFFu; break; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    *lds_word = x;
  }
  __syncthreads();
  const uint32_t got = *lds_word;
  __syncthreads();
  return got != 0xFFFFFFFFu;
}

// The last level of a depth-limited BFS, shared out: member m of M takes ranges [nw m / M, nw (m + 1) / M) of the
// frontier R (the leader's, published): windows, pairs in visit order, projections -- into its OWN slab -- then its
// row count goes to the group's control block; once every member has arrived a member knows where its rows start
// (rows are in frontier order x visit order, like every other path's) and writes them.  No update: the level's hits
// feed no further level (impg.rs:2376).  Returns false if a hand-off timed out or the share outgrew the slab.
struct WalkFinalLds {
  uint32_t word, n_ok;
  unsigned long long ck;
};
template <uint32_t NW, int MODE>
__device__ __forceinline__ bool walk_final_level(const WalkArgs &A, const uint32_t q, const uint32_t m, const uint32_t M, WalkGroupCtl *ctl, const WRec *R,
                                                 const uint32_t nw, const uint32_t rows_before, const WalkSlab &B, uint32_t *wsum, WalkFinalLds &F,
                                                 unsigned long long &count_out, unsigned long long &cksum_out, uint32_t &rows_out) {
  constexpr uint32_t T = NW * 64u;
  const uint32_t tid = threadIdx.x;
  const DeviceIndexView &v = A.v;
  const bool ident = A.min_identity == A.min_identity;
  const SliceArrays no_sl{nullptr, nullptr, nullptr, nullptr};
  const uint32_t own_target = A.ranges[q].target_id;
  const uint32_t r0 = (uint32_t)((unsigned long long)nw * m / M), r1 = (uint32_t)((unsigned long long)nw * (m + 1u) / M);
  bool fine = true;
  if (tid == 0) { F.n_ok = 0; F.ck = 0; }
  // 1. the share's pairs
  uint32_t P = 0;
  for (uint32_t c0 = r0; c0 < r1 && fine; c0 += T) {
    const uint32_t s_n = min(T, r1 - c0);
    if (tid < s_n) {
      const WRec f = R[c0 + tid];
      uint32_t a = 0, sn = 0, off0 = 0, cnt0 = 0;
      if (f.seq < v.n_seq) {
        const uint4 *dp = reinterpret_cast<const uint4 *>(v.seg + f.seq);
        const uint4 d0 = dp[0], d1 = dp[1];
        a = d0.x; sn = d0.y;
        if (d0.z) { off0 = d0.w; cnt0 = d1.w; }
      }
      uint32_t l1 = 0, h1 = sn, l2 = 0, h2 = sn;
      if (cnt0) {
        uint32_t b1 = 0, e1 = cnt0, b2 = 0, e2 = cnt0;
        dual_search4<true>(v.starts_lvl + off0, b1, e1, v.pmax_lvl + off0, b2, e2, f.start, f.end);
        l1 = b1 < cnt0 ? 64u * b1 : sn; h1 = b1 < cnt0 ? min(l1 + 63u, sn) : sn;
        l2 = b2 < cnt0 ? 64u * b2 : sn; h2 = b2 < cnt0 ? min(l2 + 63u, sn) : sn;
      }
      dual_search4<true>(v.starts + a, l1, h1, v.pmax + a, l2, h2, f.start, f.end);
      B.win[tid] = make_uint2(a + min(l2, l1), a + l1);
    }
    __syncthreads();
    for (uint32_t r = tid >> 6; r < s_n; r += NW) {
      const uint2 w = B.win[r];
      const int32_t qs = R[c0 + r].start;
      uint32_t k = 0;
      for (uint32_t b = w.x; b < w.y; b += 64u) {
        const uint32_t i = b + lane_id();
        k += (uint32_t)__popcll(__ballot(i < w.y && window_hit<true>(v.ends_t[i], qs)));
      }
      if (lane_id() == 0) B.cnt[r] = k;
    }
    __syncthreads();
    const uint32_t c = tid < s_n ? B.cnt[tid] : 0u;
    __syncthreads();
    uint32_t tot;
    const uint32_t off = wk_scan<NW>(c, wsum, tot);
    if (P + tot > A.hcap) { fine = false; break; }  // (the share outgrew the slab: the batch engine runs the batch)
    if (tid < s_n) B.cnt[tid] = P + off;
    __syncthreads();
    for (uint32_t r = tid >> 6; r < s_n; r += NW) {
      const uint2 w = B.win[r];
      wk_emit_range(v, w.x, w.y, R[c0 + r].start, B.cnt[r], c0 + r, B.pair_range, B.pair_entry);
    }
    __syncthreads();
    P += tot;
  }
  if (!fine) P = 0;
  // 2. projections; a hit that is no row is marked so
  uint32_t my_emit = 0, my_ok = 0;
  unsigned long long my_ck = 0;
  for (uint32_t p = tid; p < P; p += T) {
    const WRec f = R[B.pair_range[p]];
    bool ok = false;
    uint32_t qid = HIT_NONE;
    TileScan res;
    res.found = res.any = false;
    res.pqs = res.pts = res.pqe = res.pte = -1;
#ifdef IMPG_PHASE_CLOCKS
    unsigned long long phase_t[10];
#endif
    project_pair<true, MODE>(v, B.pair_entry[p], f.start, f.end, p, ident ? A.min_identity : 0.0, A.err_flag, no_sl, A.accepted, ok, qid, res PHASE_PASS);
    int4 hc = make_int4(0, 0, 0, 0);
    if (ok) {
      my_ok += 1;
      hc = make_int4(res.pqs, res.pqe, res.pts, res.pte);
      if (A.subset_keep && qid != own_target && !A.subset_keep[qid]) qid = HIT_NONE;  // impg.rs:2430-2439
    }
    const bool emit = qid != HIT_NONE && !(A.min_output_length >= 0 && abs(hc.y - hc.x) < A.min_output_length);  // impg.rs:2482-2504
    if (emit) {
      unsigned long long ck = mix64(((unsigned long long)qid << 32) | (uint32_t)hc.x);
      ck = mix64(ck ^ (((unsigned long long)(uint32_t)hc.y << 32) | f.seq));
      ck = mix64(ck ^ (((unsigned long long)(uint32_t)hc.z << 32) | (uint32_t)hc.w));
      my_ck += ck;
      my_emit += 1;
    }
    B.hqid[p] = emit ? qid : HIT_NONE;
    B.hc[p] = hc;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    my_ck += (unsigned long long)__shfl_xor((long long)my_ck, o);
    my_ok += (uint32_t)__shfl_xor((int)my_ok, o);
  }
  __syncthreads();  // (F was zeroed by thread 0 above)
  if (lane_id() == 0) { atomicAdd(&F.ck, my_ck); atomicAdd(&F.n_ok, my_ok); }
  uint32_t n_emit;
  (void)wk_scan<NW>(my_emit, wsum, n_emit);
  if (tid == 0) {
    if (F.n_ok) atomicAdd(&A.accepted[(blockIdx.x % COUNT_SLOTS) * COUNT_STRIDE], (unsigned long long)F.n_ok);
    if (F.ck) atomicAdd(&ctl->cksum, F.ck);
    if (n_emit) atomicAdd(&ctl->count, (unsigned long long)n_emit);
    __hip_atomic_store((wk_gu32 *)&ctl->emit[m], n_emit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!fine) atomicOr(A.overflow, 2u);
  }
  wk_publish(&ctl->arrived, 1u, true);
  // 3. everyone has arrived: where this share's rows start
  if (m != 0 && !A.rows) return fine;  // (nobody waits for a helper without rows)
  if (!wk_wait(&ctl->arrived, M, &F.word)) { if (tid == 0) atomicOr(A.overflow, 128u); return false; }
  if (tid == 0) {
    uint32_t before = 0, all = 0;
    for (uint32_t k = 0; k < M; k++) { const uint32_t e = wk_load(&ctl->emit[k]); before += k < m ? e : 0u; all += e; }
    F.word = before; F.n_ok = all;
  }
  __syncthreads();
  uint32_t run = rows_before + F.word;
  rows_out = rows_before + F.n_ok;
  if (m == 0) {
    count_out = __hip_atomic_load(&ctl->count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    cksum_out = __hip_atomic_load(&ctl->cksum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  // 4. rows
  if (A.rows) {
    const unsigned long long row_base = A.row_base[q];
    const uint32_t row_cap = A.row_cap[q];
    for (uint32_t pb = 0; pb < P; pb += T) {
      const uint32_t p = pb + tid;
      const uint32_t qid = p < P ? B.hqid[p] : HIT_NONE;
      uint32_t tot;
      const uint32_t e = wk_scan<NW>(qid != HIT_NONE ? 1u : 0u, wsum, tot);
      if (qid != HIT_NONE && run + e < row_cap) {
        const int4 hc = B.hc[p];
        impg_gpu_interval_t iv{qid, hc.x, hc.y, R[B.pair_range[p]].seq, hc.z, hc.w};
        A.rows[row_base + run + e] = iv;
      }
      run += tot;
    }
  }
  return fine;
}

// MULTI: a MultiImpg worklist (MultiImpg::transitive_query_impl, multi_impg.rs:796-991) -- the DFS arm's one pop at a time with
//   pop      A.dfs: at the back, as the DFS arm; else at the front -- the first record of the lowest non-empty list
//   step     an Impg::query: the closed overlap test, the unclipped range (what Engine::expand selects for MultiImpg)
//   hits     in (query_id, q_first, q_last, t_first, t_last) order, ties by the entry's mrank, then the slot (key5_less): the
//            row order and the replay order; a hit on the popped sequence itself is no hit at all (multi_impg.rs:883-885)
//   budget   WALK_POP_BUDGET explored pops a query
// (written out at every use, not held in a variable: the other instantiations then read A.dfs where they always did)
#define WK_STACK (MULTI || A.dfs)   /* a stack / worklist of single pops (else: BFS levels) */
#define WK_BACK (!MULTI || A.dfs)   /* which end is popped */
template <uint32_t NW, uint32_t LCAP, int MODE, bool GRID, bool MULTI = false>
__device__ __forceinline__ void walk_body(const WalkArgs &A) {
  static_assert(!MULTI || (NW == 1 && !GRID), "the MultiImpg arm is the one-wave form's");
  constexpr uint32_t T = NW * 64u;
  constexpr bool TR = !MULTI;  // the lookups' and projections' TRANSITIVE
  __shared__ WalkLds<NW> S;
  __shared__ WalkMultiLds SM;
  __shared__ __attribute__((aligned(8))) uint32_t lkeys[LCAP];
  const uint32_t tid = threadIdx.x;
  const DeviceIndexView &v = A.v;
  // The slab descriptor -- 23 pointers, the same for every thread -- lives in LDS: as a local it did not fit the scalar
  // registers beside the index view and went to scratch memory, so every use of one was a load from memory in a kernel
  // that is nothing but dependent loads.
  __shared__ WalkSlab Bs;
  if (tid == 0) walk_slab_layout(A.slabs + (size_t)blockIdx.x * A.slab_bytes, v.n_seq, T, A.wcap, A.hcap, A.vcap, A.gcap, A.scap, &Bs);
  __syncthreads();
  const WalkSlab &B = Bs;
  const bool ident = A.min_identity == A.min_identity;
  const SliceArrays no_sl{nullptr, nullptr, nullptr, nullptr};
  unsigned long long tmark = 0;
  auto lap = [&](int k) {  // debug: clocks since the last mark go to phase k
    if (A.dbg && tid == 0) { const unsigned long long t = clock64(); atomicAdd(&A.dbg[k], t - tmark); tmark = t; }
  };
  auto bump = [&](int k, unsigned long long x) { if (A.dbg && tid == 0) atomicAdd(&A.dbg[k], x); };
  auto peak = [&](int k, unsigned long long x) { if (A.dbg && tid == 0) atomicMax(&A.dbg[k], x); };
  __shared__ WalkFinalLds FL;
  for (bool first_turn = true;; first_turn = false) {
    // ---- next query (grid form: the workgroup's own, once) -----------------------------------------------------------
    if (GRID && !first_turn) return;
    if (tid == 0) S.tmp = GRID ? blockIdx.x / A.members : atomicAdd(A.next_query, 1u);
    __syncthreads();
    const uint32_t q = S.tmp;
    __syncthreads();
    if (q >= A.n_queries) return;
    WalkGroupCtl *ctl = GRID ? A.ctl + q : nullptr;
    bool published = false;
    const impg_gpu_range_t rq = A.ranges[q];
    for (uint32_t i = tid; i < v.n_seq; i += T) { B.tab_len[i] = 0; B.tab_cap[i] = 0; B.st_len[i] = 0; B.st_cap[i] = 0; }
    if (tid == 0) { S.spused = 0; S.top_seq = -1; S.nw = 0; S.npc = 0; S.vused = 0; S.rows_run = 0; S.flag = 0; S.acc_count = 0; S.acc_cksum = 0; }
    __syncthreads();
    // level -1: the input range, clamped, opens the target's visited list, is the self interval and (if long enough)
    // the first frontier (impg.rs:2331-2373)
    const unsigned long long row_base = A.rows ? A.row_base[q] : 0ull;
    const uint32_t row_cap = A.rows ? A.row_cap[q] : 0u;
    if (A.mask_off) {
      // masked_regions: SortedRanges::insert (min_distance 0) on a copy of the target's mask list (impg.rs:2077-2112,
      // :2331-2373; visited_init_masked_kernel is the batch engine's form): every piece the list did not cover is a self
      // interval, the pieces of at least min_transitive_len open the frontier / the stack
      if (rq.target_id >= v.n_seq) { if (tid == 0) S.flag = 1; }
      else {
        const uint32_t ma = A.mask_off[rq.target_id], mlen = A.mask_off[rq.target_id + 1] - ma;
        const uint32_t cap0 = max(8u, 2u * (mlen + 1u));
        if (cap0 > A.vcap || mlen + 1u > A.gcap || mlen + 1u > A.wcap || (WK_STACK && mlen + 1u > A.scap)) { if (tid == 0) S.flag = 4; }
        else {
          int2 *Rl = B.vpool;
          for (uint32_t i = tid; i < mlen; i += T) Rl[i] = A.mask_ranges[ma + i];
          __syncthreads();
          if (tid == 0) {
            int32_t start = min(rq.start, rq.end), end = max(rq.start, rq.end);
            const int32_t sequence_length = A.mask_init_len[rq.target_id];
            if (start < 0) start = 0;                          // impg.rs:287-289
            if (end > sequence_length) end = sequence_length;  // impg.rs:294-296
            uint32_t len = mlen, np = 0;
            int2 *Pp = B.gp;
            int32_t current = start;
            uint32_t i = lower_bound_start(Rl, len, start);
            if (i > 0 && Rl[i - 1].y > start) i -= 1;
            while (i < len && current < end) {  // impg.rs:314-324
              const int2 rg = Rl[i];
              if (rg.x > end) break;
              if (current < rg.x) Pp[np++] = make_int2(current, rg.x);
              current = max(current, rg.y);
              i += 1;
            }
            if (current < end) Pp[np++] = make_int2(current, end);
            const uint32_t pos = lower_bound_start(Rl, len, start);  // impg.rs:330-343
            bool merge = true;
            uint32_t mfrom = 0;
            if (pos > 0 && Rl[pos - 1].y >= start) { Rl[pos - 1].y = max(Rl[pos - 1].y, end); mfrom = pos - 1; }
            else if (pos < len && end >= Rl[pos].x) { Rl[pos].x = min(start, Rl[pos].x); Rl[pos].y = max(end, Rl[pos].y); mfrom = pos; }
            else {
              for (uint32_t k = len; k > pos; k--) Rl[k] = Rl[k - 1];
              Rl[pos] = make_int2(start, end);
              len += 1;
              merge = false;
            }
            if (merge) {  // merge_forward_from, impg.rs:355-368
              uint32_t write = mfrom, read = mfrom + 1;
              while (read < len) {
                if (Rl[write].y >= Rl[read].x) Rl[write].y = max(Rl[write].y, Rl[read].y);
                else { write += 1; const int2 t2 = Rl[write]; Rl[write] = Rl[read]; Rl[read] = t2; }
                read += 1;
              }
              len = write + 1;
            }
            B.tab_off[rq.target_id] = 0; B.tab_len[rq.target_id] = len; B.tab_cap[rq.target_id] = cap0;
            S.vused = cap0;
            uint32_t nf = 0;
            for (uint32_t k = 0; k < np; k++) {
              const int2 pc = Pp[k];
              if (A.rows && k < row_cap) {
                impg_gpu_interval_t iv{rq.target_id, pc.x, pc.y, rq.target_id, pc.x, pc.y};
                A.rows[row_base + k] = iv;
              }
              if (abs(pc.x - pc.y) >= A.min_transitive_len) {
                B.wa[nf] = WRec{rq.target_id, pc.x, pc.y, 0u};
                if (WK_STACK) B.spool[nf] = make_int4(pc.x, pc.y, 0, 0);
                nf += 1;
              }
            }
            S.rows_run = np;
            S.nw = nf;
            if (WK_STACK && nf) {
              B.st_off[rq.target_id] = 0; B.st_len[rq.target_id] = nf; B.st_cap[rq.target_id] = max(8u, nf);
              S.spused = max(8u, nf);
              S.top_seq = (int)rq.target_id;
            }
          }
        }
      }
    } else if (tid == 0) {
      int32_t start = min(rq.start, rq.end), end = max(rq.start, rq.end);
      if (rq.target_id >= v.n_seq) S.flag = 1;  // cause 1  // (the batch engine answers queries on sequences the index does not know)
      else {
        const int32_t sl = v.seq_len[rq.target_id];
        if (start < 0) start = 0;
        if (end > sl) end = sl;
        B.tab_off[rq.target_id] = 0; B.tab_len[rq.target_id] = 1; B.tab_cap[rq.target_id] = 8;
        B.vpool[0] = make_int2(start, end);
        S.vused = 8;
        if (start < end) {
          if (A.rows && row_cap > 0) {
            impg_gpu_interval_t iv{rq.target_id, start, end, rq.target_id, start, end};
            A.rows[row_base] = iv;
          }
          S.rows_run = 1;
          if (abs(start - end) >= A.min_transitive_len) {
            B.wa[0] = WRec{rq.target_id, start, end, 0u};
            S.nw = 1;
            if (WK_STACK) {  // the stack's first record
              B.st_off[rq.target_id] = 0; B.st_len[rq.target_id] = 1; B.st_cap[rq.target_id] = 8;
              B.spool[0] = make_int4(start, end, 0, 0);
              S.spused = 8;
              S.top_seq = (int)rq.target_id;
            }
          }
        }
      }
    }
    if (MULTI && tid == 0) { SM.bot_seq = S.top_seq >= 0 ? S.top_seq : 0x7FFFFFFF; }  // (thread 0 set top_seq itself)
    __syncthreads();
    uint32_t level = 0;
    uint32_t pops = 0;  // MULTI: explored pops of this query
    bool failed = S.flag != 0;
    bool named = false;  // the failure's cause bit is in A.overflow already
    if (A.dbg && tid == 0) tmark = clock64();
    // ---- the walk -----------------------------------------------------------------------------------------------------
    while (!failed) {
      uint32_t nw = S.nw;
      if (!WK_STACK && nw == 0) break;
      uint32_t first, count, cur_depth;
      bool do_update;
      if (WK_STACK) {
        // Pop (impg.rs:2120-2127): the stack's top is the last record of the highest non-empty sequence list.  Records
        // too deep to be explored are popped and dropped: the list's tail of such records goes in one step (wave 0).
        if (S.top_seq < 0) break;
        if (WK_BACK && tid < 64) {
          int sq_i = S.top_seq;
          bool got_one = false;
          while (sq_i >= 0 && !got_one) {  // (wave 0 alone, no barrier: lists of records too deep to explore go one after the other)
            const uint32_t sq = (uint32_t)sq_i;
            const uint32_t len = B.st_len[sq];
            const int4 *L = B.spool + B.st_off[sq];
            uint32_t found = 0xFFFFFFFFu;  // index of the last explorable record
            for (uint32_t hi = len; hi > 0 && found == 0xFFFFFFFFu; hi = hi > 64u ? hi - 64u : 0u) {
              const bool in = lane_id() < hi;
              const uint32_t idx = hi - 1u - lane_id();
              const bool ok = in && !(A.max_depth > 0 && (uint32_t)L[in ? idx : 0].z >= A.max_depth);
              const unsigned long long m = __ballot(ok);
              if (m) found = hi - 1u - (uint32_t)(__ffsll((long long)m) - 1);
            }
            if (found != 0xFFFFFFFFu) {
              if (lane_id() == 0) {
                const int4 t = L[found];
                S.top = WRec{sq, t.x, t.y, (uint32_t)t.z};
                B.st_len[sq] = found;
                if (A.dbg) atomicAdd(&A.dbg[17], (unsigned long long)(len - 1u - found));
              }
              got_one = true;
            } else if (lane_id() == 0) {
              B.st_len[sq] = 0;
              if (A.dbg) atomicAdd(&A.dbg[17], (unsigned long long)len);
            }
            // the list may be empty now: the next non-empty sequence below (64 sequences per look)
            if (found == 0xFFFFFFFFu || found == 0u) {
              int nt = -1;
              for (int base = sq_i - 1; base >= 0 && nt < 0; base -= 64) {
                const int i = base - (int)lane_id();
                const unsigned long long m = __ballot(i >= 0 && B.st_len[i >= 0 ? i : 0] != 0u);
                if (m) nt = base - (__ffsll((long long)m) - 1);
              }
              sq_i = nt;
            }
          }
          if (lane_id() == 0) { S.top_seq = sq_i; S.tmp = got_one ? 1u : 0u; }
        } else if (MULTI && tid < 64) {
          // The front (multi_impg.rs:849-854): the first record of the lowest non-empty list.  The mirror image of the above:
          // a list's head of records too deep to explore goes in one step, the list then starts behind them (its offset
          // moves up, its capacity shrinks by as much); an emptied list sends the cursor up, 64 sequences per look.
          // (top_seq is only ever raised while the front is popped: it bounds the looks from above)
          int sq_i = SM.bot_seq;
          const int hi_seq = S.top_seq;
          bool got_one = false;
          while (sq_i <= hi_seq && !got_one) {
            const uint32_t sq = (uint32_t)sq_i;
            const uint32_t len = B.st_len[sq], off = B.st_off[sq];
            const int4 *L = B.spool + off;
            uint32_t found = 0xFFFFFFFFu;  // index of the first explorable record
            for (uint32_t lo = 0; lo < len && found == 0xFFFFFFFFu; lo += 64u) {
              const uint32_t idx = lo + lane_id();
              const bool in = idx < len;
              const bool ok = in && !(A.max_depth > 0 && (uint32_t)L[in ? idx : 0].z >= A.max_depth);
              const unsigned long long m = __ballot(ok);
              if (m) found = lo + (uint32_t)(__ffsll((long long)m) - 1);
            }
            const uint32_t gone = found != 0xFFFFFFFFu ? found + 1u : len;  // records that leave the list's head
            if (found != 0xFFFFFFFFu) {
              if (lane_id() == 0) {
                const int4 t = L[found];
                S.top = WRec{sq, t.x, t.y, (uint32_t)t.z};
                B.st_off[sq] = off + gone; B.st_len[sq] = len - gone; B.st_cap[sq] = B.st_cap[sq] - gone;  // (cap >= len >= gone)
                if (A.dbg) atomicAdd(&A.dbg[17], (unsigned long long)found);
              }
              got_one = true;
            } else if (lane_id() == 0) {
              B.st_len[sq] = 0;
              if (A.dbg) atomicAdd(&A.dbg[17], (unsigned long long)len);
            }
            if (gone == len) {  // the list is empty now: the next non-empty sequence above
              int nt = 0x7FFFFFFF;
              for (int base = sq_i + 1; base <= hi_seq && nt == 0x7FFFFFFF; base += 64) {
                const int i = base + (int)lane_id();
                const unsigned long long m = __ballot(i <= hi_seq && B.st_len[i <= hi_seq ? i : hi_seq] != 0u);
                if (m) nt = base + (__ffsll((long long)m) - 1);
              }
              sq_i = nt;
            }
          }
          if (lane_id() == 0) {
            const bool empty = sq_i > hi_seq;
            SM.bot_seq = empty ? 0x7FFFFFFF : sq_i;
            if (empty) S.top_seq = -1;
            S.tmp = got_one ? 1u : 0u;
          }
        }
        __syncthreads();
        const bool got = S.tmp != 0;
        const WRec top = S.top;
        __syncthreads();
        if (!got) { lap(0); continue; }
        bump(16, 1);
        if (MULTI && ++pops > WALK_POP_BUDGET) { failed = true; if (tid == 0) S.flag |= 256u; break; }  // the pop budget
        if (tid == 0) B.wc[0] = top;  // the step's range
        __syncthreads();
        first = 0; count = 1; cur_depth = top.depth; do_update = true;
      } else {
        if (A.max_depth > 0 && level >= A.max_depth) break;
        first = 0; count = nw; cur_depth = level;
        do_update = !(A.max_depth > 0 && level + 1 >= A.max_depth);  // the last level's update is dead (impg.rs:2376)
        if (GRID && !do_update) {
          // the last level: published, and shared out among the query's workgroups
          if (tid == 0) { ctl->nw = nw; ctl->rows_run = S.rows_run; }
          wk_publish(&ctl->state, 1u, false);
          published = true;
          unsigned long long cnt_l = 0, ck_l = 0;
          uint32_t rows_l = 0;
          const bool fine = walk_final_level<NW, MODE>(A, q, 0u, A.members, ctl, B.wa, nw, S.rows_run, B, S.wsum, FL, cnt_l, ck_l, rows_l);
          lap(10);
          if (!fine) { failed = true; named = true; break; }  // (walk_final_level has raised the cause: 2 or 128)
          if (tid == 0) { S.acc_count += cnt_l; S.acc_cksum += ck_l; S.rows_run = rows_l; S.nw = 0; }
          __syncthreads();
          break;
        }
      }
      const WRec *R = WK_STACK ? B.wc : B.wa;
      if (tid == 0) S.npc = 0;
      __syncthreads();
      // ---- the level's / pop's ranges in sub-steps ------------------------------------------------------------------
      uint32_t done = first;
      uint32_t sub = min(count, T);
      while (done < first + count && !failed) {
        const uint32_t s_n = min(sub, first + count - done);
        // a. window and hit count of every range (a thread per range)
        uint32_t c = 0;
        if (s_n == 1u) {  // one range (a DFS pop, a BFS's first level): the first wave searches together
          if (tid < 64u) {
            const WRec f = R[done];
            uint32_t a = 0, sn = 0, off0 = 0, cnt0 = 0;
            if (f.seq < v.n_seq) {
              const uint4 *dp = reinterpret_cast<const uint4 *>(v.seg + f.seq);
              const uint4 d0 = dp[0], d1 = dp[1];
              a = d0.x; sn = d0.y;
              if (d0.z) { off0 = d0.w; cnt0 = d1.w; }
            }
            uint32_t l1 = 0, h1 = sn, l2 = 0, h2 = sn;
            if (cnt0) {
              const uint32_t b1 = wk_wave_first<TR>(v.starts_lvl + off0, 0u, cnt0, f.end);
              const uint32_t b2 = wk_wave_first<!TR>(v.pmax_lvl + off0, 0u, cnt0, f.start);
              l1 = b1 < cnt0 ? 64u * b1 : sn; h1 = b1 < cnt0 ? min(l1 + 63u, sn) : sn;
              l2 = b2 < cnt0 ? 64u * b2 : sn; h2 = b2 < cnt0 ? min(l2 + 63u, sn) : sn;
            }
            l1 = wk_wave_first<TR>(v.starts + a, l1, h1, f.end);
            l2 = wk_wave_first<!TR>(v.pmax + a, l2, h2, f.start);
            if (tid == 0) B.win[0] = make_uint2(a + min(l2, l1), a + l1);
          }
        } else if (tid < s_n) {
          const WRec f = R[done + tid];
          uint32_t a = 0, sn = 0, off0 = 0, cnt0 = 0;
          if (f.seq < v.n_seq) {
            const uint4 *dp = reinterpret_cast<const uint4 *>(v.seg + f.seq);
            const uint4 d0 = dp[0], d1 = dp[1];
            a = d0.x; sn = d0.y;
            if (d0.z) { off0 = d0.w; cnt0 = d1.w; }
          }
          uint32_t l1 = 0, h1 = sn, l2 = 0, h2 = sn;
          if (cnt0) {
            uint32_t b1 = 0, e1 = cnt0, b2 = 0, e2 = cnt0;
            dual_search4<TR>(v.starts_lvl + off0, b1, e1, v.pmax_lvl + off0, b2, e2, f.start, f.end);
            l1 = b1 < cnt0 ? 64u * b1 : sn; h1 = b1 < cnt0 ? min(l1 + 63u, sn) : sn;
            l2 = b2 < cnt0 ? 64u * b2 : sn; h2 = b2 < cnt0 ? min(l2 + 63u, sn) : sn;
          }
          dual_search4<TR>(v.starts + a, l1, h1, v.pmax + a, l2, h2, f.start, f.end);
          const uint32_t ub = a + l1, lo = a + min(l2, l1);
          B.win[tid] = make_uint2(lo, ub);
        }
        __syncthreads();
        lap(1);
        // ... the windows' hits counted by a wave per range (a thread walking its own window waits for every load)
        for (uint32_t r = tid >> 6; r < s_n; r += NW) {
          const uint2 w = B.win[r];
          const int32_t qs = R[done + r].start;
          uint32_t k = 0;
          for (uint32_t b = w.x; b < w.y; b += 64u) {
            const uint32_t i = b + lane_id();
            k += (uint32_t)__popcll(__ballot(i < w.y && window_hit<TR>(end_col<TR>(v)[i], qs)));
          }
          if (lane_id() == 0) B.cnt[r] = k;
        }
        __syncthreads();
        if (tid < s_n) c = B.cnt[tid];
        __syncthreads();
        uint32_t P;
        const uint32_t off = wk_scan<NW>(c, S.wsum, P);
        if (P > A.hcap || P >= (1u << WALK_SLOT_BITS)) {
          if (s_n == 1) { failed = true; if (tid == 0) S.flag |= 2u; break; }
          sub = max(1u, s_n >> 1);  // fewer ranges per sub-step
          continue;
        }
        // (MULTI: the sorted copy of a pop of more than 64 hits goes through gp[], 16 bytes a hit -- with the present caps,
        // hcap <= gcap / 2, this cannot fire)
        if (MULTI && P > 64u && 2ull * P > A.gcap) { failed = true; if (tid == 0) S.flag |= 8u; break; }
        if (tid < s_n) B.cnt[tid] = off;
        __syncthreads();
        lap(2);
        // b. the pairs in visit order (a wave per range)
        for (uint32_t r = tid >> 6; r < s_n; r += NW) {
          const uint2 w = B.win[r];
          wk_emit_range<TR>(v, w.x, w.y, R[done + r].start, B.cnt[r], r, B.pair_range, B.pair_entry);
        }
        __syncthreads();
        lap(3);
        // c. projections (a thread per pair), subset filter, counts / checksums / rows in slot order
        uint32_t n_ok = 0;
        for (uint32_t pb = 0; pb < P; pb += T) {
          const uint32_t p = pb + tid;
          bool ok = false;
          uint32_t qid = HIT_NONE;
          int4 hc = make_int4(0, 0, 0, 0);
          uint32_t tgt = 0;
          if (p < P) {
            const WRec f = R[done + B.pair_range[p]];
            tgt = f.seq;
            TileScan res;
            res.found = res.any = false;
            res.pqs = res.pts = res.pqe = res.pte = -1;
#ifdef IMPG_PHASE_CLOCKS
            unsigned long long phase_t[10];
#endif
            project_pair<TR, MODE>(v, B.pair_entry[p], f.start, f.end, p, ident ? A.min_identity : 0.0, A.err_flag, no_sl, A.accepted, ok, qid, res PHASE_PASS);
            if (ok) {
              hc = make_int4(res.pqs, res.pqe, res.pts, res.pte);
              // subset filter: a hit whose sequence is neither the query's own target nor kept is no hit (impg.rs:2430-2439)
              if (A.subset_keep && qid != rq.target_id && !A.subset_keep[qid]) qid = HIT_NONE;
              if (MULTI && qid == tgt) qid = HIT_NONE;  // a hit on the popped sequence itself: not reported, not replayed (multi_impg.rs:883-885)
            }
            B.hqid[p] = qid;
            B.hc[p] = hc;
          }
          if (MULTI) {  // (rows, counts and checksums once the pop's hits are in order, below)
            const unsigned long long okm = __ballot(ok);
            if (lane_id() == 0) n_ok += (uint32_t)__popcll(okm);
            continue;
          }
          const bool emit = qid != HIT_NONE && !(A.min_output_length >= 0 && abs(hc.y - hc.x) < A.min_output_length);  // impg.rs:2482-2504
          unsigned long long ck = 0;
          if (emit) {
            ck = mix64(((unsigned long long)qid << 32) | (uint32_t)hc.x);
            ck = mix64(ck ^ (((unsigned long long)(uint32_t)hc.y << 32) | tgt));
            ck = mix64(ck ^ (((unsigned long long)(uint32_t)hc.z << 32) | (uint32_t)hc.w));
          }
          uint32_t n_emit;
          const uint32_t epos = wk_scan<NW>(emit ? 1u : 0u, S.wsum, n_emit);
          const uint32_t run = S.rows_run;
          if (emit && A.rows && run + epos < row_cap) {
            impg_gpu_interval_t iv{qid, hc.x, hc.y, tgt, hc.z, hc.w};
            A.rows[row_base + run + epos] = iv;
          }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) ck += (unsigned long long)__shfl_xor((long long)ck, o);
          const unsigned long long okm = __ballot(ok);
          if (lane_id() == 0) {
            if (ck) atomicAdd(&S.acc_cksum, ck);
            n_ok += (uint32_t)__popcll(okm);
          }
          __syncthreads();
          if (tid == 0) { S.rows_run = run + n_emit; S.acc_count += n_emit; }
          __syncthreads();
        }
        if (MULTI) {
          // The pop's hits in the order of MultiImpg::query_all_indices (multi_impg.rs:582-592): a rank sort, every hit counting
          // the hits that sort before it (sort5_kernel's way).  A pop of at most 64 hits stays in the wave's registers and is
          // stored back in place; a longer one is read chunk by chunk from the slab and goes through skey[] / gp[].
          __syncthreads();
          int4 *hc2 = reinterpret_cast<int4 *>(B.gp);
          const bool big = P > 64u;
          for (uint32_t base = 0; base < P && P > 1u; base += 64u) {
            const uint32_t i = base + tid;
            uint32_t q5 = HIT_NONE, km = 0;
            int4 k5 = make_int4(0, 0, 0, 0);
            if (i < P) {
              q5 = B.hqid[i];
              if (q5 != HIT_NONE) { k5 = B.hc[i]; km = v.mrank ? v.mrank[B.pair_entry[i]] : 0u; }
            }
            uint32_t pos = 0;
            for (uint32_t b2 = 0; b2 < P; b2 += 64u) {
              uint32_t q2 = q5, jm = km;
              int4 j5 = k5;
              if (b2 != base) {
                const uint32_t i2 = b2 + tid;
                q2 = HIT_NONE; jm = 0; j5 = make_int4(0, 0, 0, 0);
                if (i2 < P) {
                  q2 = B.hqid[i2];
                  if (q2 != HIT_NONE) { j5 = B.hc[i2]; jm = v.mrank ? v.mrank[B.pair_entry[i2]] : 0u; }
                }
              }
              const uint32_t cntl = min(64u, P - b2);
              for (uint32_t t = 0; t < cntl; t++) {
                const uint32_t oq = (uint32_t)__shfl((int)q2, (int)t), om = (uint32_t)__shfl((int)jm, (int)t);
                const int32_t o1 = __shfl(j5.x, (int)t), o2 = __shfl(j5.y, (int)t), o3 = __shfl(j5.z, (int)t), o4 = __shfl(j5.w, (int)t);
                pos += key5_less(oq, o1, o2, o3, o4, om, b2 + t, q5, k5.x, k5.y, k5.z, k5.w, km, i) ? 1u : 0u;
              }
            }
            if (i < P) {  // (every hit of the wave was read before the first is stored; empty slots sort last)
              if (big) { B.skey[pos] = q5; hc2[pos] = k5; }
              else { B.hqid[pos] = q5; B.hc[pos] = k5; }
            }
          }
          __syncthreads();
          if (big) {
            for (uint32_t i = tid; i < P; i += T) { B.hqid[i] = B.skey[i]; B.hc[i] = hc2[i]; }
            __syncthreads();
          }
          // rows, counts and checksums in that order
          const uint32_t tgt = R[done].seq;
          for (uint32_t pb = 0; pb < P; pb += T) {
            const uint32_t p = pb + tid;
            const uint32_t qid = p < P ? B.hqid[p] : HIT_NONE;
            int4 hc = make_int4(0, 0, 0, 0);
            if (qid != HIT_NONE) hc = B.hc[p];
            const bool emit = qid != HIT_NONE && !(A.min_output_length >= 0 && abs(hc.y - hc.x) < A.min_output_length);  // multi_impg.rs:905-914
            unsigned long long ck = 0;
            if (emit) {
              ck = mix64(((unsigned long long)qid << 32) | (uint32_t)hc.x);
              ck = mix64(ck ^ (((unsigned long long)(uint32_t)hc.y << 32) | tgt));
              ck = mix64(ck ^ (((unsigned long long)(uint32_t)hc.z << 32) | (uint32_t)hc.w));
            }
            uint32_t n_emit;
            const uint32_t epos = wk_scan<NW>(emit ? 1u : 0u, S.wsum, n_emit);
            const uint32_t run = S.rows_run;
            if (emit && A.rows && run + epos < row_cap) {
              impg_gpu_interval_t iv{qid, hc.x, hc.y, tgt, hc.z, hc.w};
              A.rows[row_base + run + epos] = iv;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) ck += (unsigned long long)__shfl_xor((long long)ck, o);
            if (lane_id() == 0 && ck) atomicAdd(&S.acc_cksum, ck);
            __syncthreads();
            if (tid == 0) { S.rows_run = run + n_emit; S.acc_count += n_emit; }
            __syncthreads();
          }
        }
        {  // accepted projections of the sub-step (counted before the subset filter, like project_kernel)
          uint32_t tot;
          (void)wk_scan<NW>(lane_id() == 0 ? n_ok : 0u, S.wsum, tot);
          if (tid == 0 && tot) atomicAdd(&A.accepted[(blockIdx.x % COUNT_SLOTS) * COUNT_STRIDE], (unsigned long long)tot);
        }
        lap(4);
        // d. visited update: hits of one sequence replayed in slot order on the sequence's list
        if (do_update && P) {
          const uint32_t np2 = wk_pow2(P);
          uint32_t *keys = np2 <= LCAP ? lkeys : B.skey;
          for (uint32_t p = tid; p < np2; p += T) {
            uint32_t k = 0xFFFFFFFFu;
            if (p < P) {
              const uint32_t qid = B.hqid[p];
              if (qid != HIT_NONE && qid != R[done + B.pair_range[p]].seq) k = (qid << WALK_SLOT_BITS) | p;  // impg.rs:2507
            }
            keys[p] = k;
          }
          __syncthreads();
          wk_sort<NW>(keys, np2);
          lap(5);
          // group heads, the hits' intervals in sorted order
          for (uint32_t i = tid; i < P; i += T) {
            const uint32_t k = keys[i];
            uint32_t head = 0;
            if (k != 0xFFFFFFFFu) {
              head = (i == 0 || (keys[i - 1] >> WALK_SLOT_BITS) != (k >> WALK_SLOT_BITS)) ? 1u : 0u;
              const int4 hc = B.hc[k & ((1u << WALK_SLOT_BITS) - 1u)];
              B.sval[i] = ((unsigned long long)(uint32_t)min(hc.x, hc.y) << 32) | (uint32_t)max(hc.x, hc.y);
            }
            B.gflag[i] = head;
          }
          __syncthreads();
          if (A.dbg && tid == 0) atomicAdd(&A.dbg[22], clock64() - tmark);  // (debug: the heads pass's share of the groups phase)
          if (tid == 0) S.gpused = 0;
          __syncthreads();
          // a thread per group (found by its head)
          for (uint32_t i = tid; i < P; i += T) {
            if (!B.gflag[i]) continue;
            const uint32_t seq = keys[i] >> WALK_SLOT_BITS;
            uint32_t n = 1;
            while (i + n < P && keys[i + n] != 0xFFFFFFFFu && (keys[i + n] >> WALK_SLOT_BITS) == seq) n++;
            uint32_t len = B.tab_len[seq], cap = B.tab_cap[seq], loff = B.tab_off[seq];
            if (A.dbg) { atomicMax(&A.dbg[20], (unsigned long long)n); atomicMax(&A.dbg[21], (unsigned long long)len); }
            const unsigned long long g_t0 = A.dbg ? clock64() : 0ull;
            const int2 *src = B.vpool + loff;
            if (cap == 0u && A.mask_off) {  // first touch under a mask: the list opens as a copy of the map's (impg.rs:2077-2078)
              const uint32_t ma = A.mask_off[seq];
              len = A.mask_off[seq + 1] - ma;
              src = A.mask_ranges + ma;
            }
            const int32_t slen = A.mask_touch_len ? A.mask_touch_len[seq] : v.seq_len[seq];
            if (len + n > cap) {  // the list moves to a bigger place (its old one is abandoned: slabs are per query)
              const uint32_t ncap = max(8u, 2u * (len + n));
              const uint32_t noff = atomicAdd(&S.vused, ncap);
              if (noff + ncap > A.vcap) { atomicOr(&S.flag, 4u); continue; }
              // (eight loads in flight, then their stores: one at a time the copy of a mask's list -- hundreds of ranges --
              // is a chain of that many memory round trips)
              for (uint32_t k = 0; k < len; k += 8u) {
                int2 x[8];
#pragma unroll
                for (uint32_t u = 0; u < 8u; u++) x[u] = k + u < len ? src[k + u] : make_int2(0, 0);
#pragma unroll
                for (uint32_t u = 0; u < 8u; u++) if (k + u < len) B.vpool[noff + k + u] = x[u];
              }
              loff = noff; cap = ncap;
              B.tab_off[seq] = loff; B.tab_cap[seq] = cap;
            }
            const uint32_t pcap = len + 2u * n;
            const uint32_t po = atomicAdd(&S.gpused, pcap);
            if (po + pcap > A.gcap) { atomicOr(&S.flag, 8u); continue; }
            int2 *Pp = B.gp + po;
            uint32_t np = 0;
            len = replay_hits(ListInPlace{B.vpool + loff}, len, B.sval, i, n, slen, A.min_transitive_len, A.mdbr, Pp, np);
            B.tab_len[seq] = len;
            // the group's pieces: sorted by start, overlapping / contiguous ones merged (impg.rs:2568-2584)
            for (uint32_t a = 1; a < np; a++) {
              const int2 x = Pp[a];
              uint32_t j = a;
              while (j > 0 && Pp[j - 1].x > x.x) { Pp[j] = Pp[j - 1]; j--; }
              Pp[j] = x;
            }
            uint32_t w = 0;
            for (uint32_t r = 1; r < np; r++) {
              if (Pp[w].y >= Pp[r].x) Pp[w].y = max(Pp[w].y, Pp[r].y);
              else { w += 1; Pp[w] = Pp[r]; }
            }
            if (np) np = w + 1;
            if (np) {
              const uint32_t dst = atomicAdd(&S.npc, np);
              if (dst + np > A.wcap) { atomicOr(&S.flag, 16u); continue; }
              for (uint32_t k = 0; k < np; k++) B.wb[dst + k] = WRec{seq, Pp[k].x, Pp[k].y, cur_depth + 1u};
            }
            if (A.dbg) atomicMax(&A.dbg[23], clock64() - g_t0);  // (debug: the slowest group of any update)
          }
          __syncthreads();
          if (S.flag) failed = true;
          lap(6);
        }
        done += s_n;
        __syncthreads();
      }
      if (failed) break;
      lap(7);
      // ---- the pieces: sorted by (sequence, start); pieces of one sequence from different sub-steps merged -------------
      const uint32_t npc = S.npc;
      uint32_t n_new = 0;
      if (npc && npc <= LCAP / 2u && npc <= 65536u && v.n_seq <= 65536u) {
        // (round 6: sorted in LDS -- {sequence, start, index} packed into 64-bit keys, the index making them distinct, a bitonic
        // network over them.  Pieces of one sequence with one start may come out in either order of their ends: the merge
        // below takes the larger end and every piece of a level / pop carries the same depth.  The rank sort this replaces --
        // every piece counting the pieces before it, all of them read from the slab -- was a third of a per-call BFS.)
        unsigned long long *pk = reinterpret_cast<unsigned long long *>(lkeys);
        const uint32_t np2 = wk_pow2(npc);
        for (uint32_t i = tid; i < np2; i += T)
          pk[i] = i < npc ? ((unsigned long long)B.wb[i].seq << 48) | ((unsigned long long)((uint32_t)B.wb[i].start ^ 0x80000000u) << 16) | i : ~0ull;
        __syncthreads();
        wk_sort<NW>(pk, np2);
        for (uint32_t i = tid; i < npc; i += T) B.wc[i] = B.wb[(uint32_t)(pk[i] & 0xFFFFull)];
        __syncthreads();
      } else if (npc) {
        for (uint32_t i = tid; i < npc; i += T) B.pkey[i] = ((unsigned long long)B.wb[i].seq << 32) | ((uint32_t)B.wb[i].start ^ 0x80000000u);
        __syncthreads();
        // (a rank sort: every piece counts the pieces that sort before it -- ties by index, so it is stable; a level
        // of a small batch has tens to hundreds of pieces, a pop a handful)
        for (uint32_t i = tid; i < npc; i += T) {
          // rank of piece i = pieces with a smaller key, or an equal key and a smaller index
          const unsigned long long ki = B.pkey[i];
          uint32_t rank = 0;
          for (uint32_t j = 0; j < npc; j++) {
            const unsigned long long kj = B.pkey[j];
            rank += (kj < ki || (kj == ki && j < i)) ? 1u : 0u;
          }
          B.wc[rank] = B.wb[i];
        }
        __syncthreads();
      }
      if (npc) {
        // merge runs of one sequence (a thread per run start)
        for (uint32_t i = tid; i < npc; i += T) B.gflag[i] = (i == 0 || B.wc[i - 1].seq != B.wc[i].seq) ? 1u : 0u;
        __syncthreads();
        for (uint32_t i = tid; i < npc; i += T) {
          if (!B.gflag[i]) continue;
          const uint32_t seq = B.wc[i].seq;
          uint32_t w = i;
          for (uint32_t r = i + 1; r < npc && B.wc[r].seq == seq; r++) {
            if (B.wc[w].end >= B.wc[r].start) B.wc[w].end = max(B.wc[w].end, B.wc[r].end);
            else { w += 1; B.wc[w] = B.wc[r]; }
          }
          // the run's merged records are wc[i .. w]; mark the rest dead
          for (uint32_t r = w + 1; r < npc && B.wc[r].seq == seq; r++) B.wc[r].depth = 0xFFFFFFFFu;
        }
        __syncthreads();
        // compact the live records, in order, into wb
        for (uint32_t b = 0; b < npc; b += T) {
          const uint32_t i = b + tid;
          const bool live = i < npc && B.wc[i].depth != 0xFFFFFFFFu;
          uint32_t tot;
          const uint32_t e = wk_scan<NW>(live ? 1u : 0u, S.wsum, tot);
          if (live) B.wb[n_new + e] = B.wc[i];
          n_new += tot;
        }
        __syncthreads();
      }
      lap(8); peak(19, npc);
      if (!WK_STACK) {
        // BFS: the pieces are the next frontier
        if (n_new > A.wcap) { failed = true; if (tid == 0) S.flag |= 32u; break; }
        for (uint32_t i = tid; i < n_new; i += T) B.wa[i] = B.wb[i];
        __syncthreads();
        if (tid == 0) S.nw = n_new;
        __syncthreads();
        level += 1;
        continue;
      }
      // DFS: push, re-sort, merge (impg.rs:2277-2304).  The pieces wb[0, n_new) are sorted by (sequence, start); the stack
      // is one start-sorted list per sequence, so the re-sort is a merge of every touched sequence's list with its
      // pieces -- existing records first on ties (the reference's sort is stable, the pieces were pushed last) -- and
      // the merge of overlapping / contiguous neighbours a sweep of that list (the first one's depth is kept).
      // A thread per touched sequence; nothing else of the stack moves.
      if (n_new) {
        for (uint32_t i = tid; i < n_new; i += T) B.gflag[i] = (i == 0 || B.wb[i - 1].seq != B.wb[i].seq) ? 1u : 0u;
        __syncthreads();
        for (uint32_t i = tid; i < n_new; i += T) {
          if (!B.gflag[i]) continue;
          const uint32_t seq = B.wb[i].seq;
          uint32_t k = 1;
          while (i + k < n_new && B.wb[i + k].seq == seq) k++;
          uint32_t len = B.st_len[seq], cap = B.st_cap[seq], off = B.st_off[seq];
          const int4 *Lold = B.spool + off;
          if (len + k > cap) {  // the merged list goes to a bigger place
            const uint32_t ncap = max(8u, 2u * (len + k));
            const uint32_t noff = atomicAdd(&S.spused, ncap);
            if (noff + ncap > A.scap) { atomicOr(&S.flag, 32u); continue; }
            off = noff; cap = ncap;
            B.st_off[seq] = off; B.st_cap[seq] = cap;
          }
          int4 *L = B.spool + off;
          // backward two-way merge into L[0, len + k): safe in place (the write index never falls below the read index of
          // the old list) and when the list moves
          // (both heads stay in registers and only the one that moved is read again: every read here is a round trip to
          // the slab, and the loop is as long as the list behind the first piece)
          int a = (int)len - 1, b2 = (int)k - 1, w = (int)(len + k) - 1;
          int4 la = a >= 0 ? Lold[a] : make_int4(0, 0, 0, 0);
          WRec pn = B.wb[i + (uint32_t)b2];
          while (b2 >= 0) {
            if (a >= 0 && la.x > pn.start) {
              L[w--] = la; a--;
              if (a >= 0) la = Lold[a];
            } else {
              L[w--] = make_int4(pn.start, pn.end, (int)pn.depth, 0); b2--;
              if (b2 >= 0) pn = B.wb[i + (uint32_t)b2];
            }
          }
          const uint32_t s0 = a > 0 ? (uint32_t)a : 0u;  // records before this one keep their place and their neighbours
          if (L != Lold) for (; a >= 0; a--) L[a] = Lold[a];  // (the list moved: the records in front of the first piece)
          // neighbours that overlap or touch become one record: a sweep from the last untouched record on, the current
          // record in registers (no read waits for a write), the reads four at a time
          const uint32_t m = len + k;
          int4 cur = L[s0];
          uint32_t wi = s0;
          for (uint32_t r = s0 + 1u; r < m; r += 4u) {
            int4 x[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) x[u] = r + u < m ? L[r + u] : make_int4(0, 0, 0, 0);
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) {
              if (r + u >= m) break;
              if (cur.y >= x[u].x) cur.y = max(cur.y, x[u].y);
              else { L[wi] = cur; wi += 1; cur = x[u]; }
            }
          }
          L[wi] = cur;
          B.st_len[seq] = wi + 1u;
          atomicMax(&S.top_seq, (int)seq);
          if (MULTI) atomicMin(&SM.bot_seq, (int)seq);
        }
        __syncthreads();
        if (S.flag) { failed = true; break; }
      }
      lap(9);
    }
    // ---- the query's totals -----------------------------------------------------------------------------------------
    __syncthreads();
    if (GRID && !published) wk_publish(&ctl->state, 2u, false);  // no last level to share: the helpers leave
    if (tid == 0) {
      if (failed && !named) atomicOr(A.overflow, S.flag ? S.flag : 64u);  // which capacity (the host's debug line names it)
      if (failed && A.dbg) { A.dbg[24] = q; A.dbg[25] = S.flag; A.dbg[26] = rq.target_id; A.dbg[27] = v.n_seq; A.dbg[28] = S.nw; A.dbg[29] = S.npc; A.dbg[30] = S.vused; }
      if (A.count) A.count[q] = S.acc_count;
      if (A.cksum) A.cksum[q] = S.acc_cksum;
      if (A.n_rows) A.n_rows[q] = S.rows_run;
    }
    __syncthreads();
  }
}

#undef WK_STACK
#undef WK_BACK

// 16 waves per query (a handful of queries: a BFS level spread over a workgroup) ...
template <uint32_t NW, uint32_t LCAP, int MODE>
__global__ __launch_bounds__(NW * 64) void walk_kernel(WalkArgs A) { walk_body<NW, LCAP, MODE, false>(A); }
// ... or `members` such workgroups per query (the per-call shape of a depth-limited BFS): the first walks, the others
// wait for the last level and take their share of it
template <uint32_t NW, uint32_t LCAP, int MODE>
__global__ __launch_bounds__(NW * 64) void walk_grid_kernel(WalkArgs A) {
  const uint32_t M = A.members, q = blockIdx.x / M, m = blockIdx.x % M;
  if (m == 0) { walk_body<NW, LCAP, MODE, true>(A); return; }
  __shared__ WalkSlab Bh;
  __shared__ WalkFinalLds FLh;
  __shared__ uint32_t wsum_h[NW];
  if (threadIdx.x == 0) walk_slab_layout(A.slabs + (size_t)blockIdx.x * A.slab_bytes, A.v.n_seq, NW * 64u, A.wcap, A.hcap, A.vcap, A.gcap, A.scap, &Bh);
  __syncthreads();
  WalkGroupCtl *ctl = A.ctl + q;
  if (!wk_wait(&ctl->state, 1u, &FLh.word)) { if (threadIdx.x == 0) atomicOr(A.overflow, 128u); return; }
  if (wk_load(&ctl->state) != 1u) return;
  // the leader's frontier: wa[] of ITS slab
  __shared__ WalkSlab Bl;
  if (threadIdx.x == 0) walk_slab_layout(A.slabs + (size_t)(q * M) * A.slab_bytes, A.v.n_seq, NW * 64u, A.wcap, A.hcap, A.vcap, A.gcap, A.scap, &Bl);
  __syncthreads();
  unsigned long long c0 = 0, c1 = 0;
  uint32_t r = 0;
  (void)walk_final_level<NW, MODE>(A, q, m, M, ctl, Bl.wa, wk_load(&ctl->nw), wk_load(&ctl->rows_run), Bh, wsum_h, FLh, c0, c1, r);
}
// ... or one wave per query (batches): the register budget is set by how many waves a SIMD should hold -- the walk is a
// chain of dependent loads, so resident waves are its throughput (WALK_WAVES_PER_SIMD, kernels.hpp)
// (MULTI: the MultiImpg worklist arm, see walk_body)
template <uint32_t LCAP, int MODE, bool MULTI = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WALK_WAVES_PER_SIMD, WALK_WAVES_PER_SIMD))) void walk_wave_kernel(WalkArgs A) {
  walk_body<1, LCAP, MODE, false, MULTI>(A);
}
