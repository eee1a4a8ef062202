// `impg refine`'s support count (reference src/commands/refine.rs:665-850) on the host, the reference's sequential way: the
// twin the kernels of refine_device.hip are checked against, and the C entry points of both.
#include "refine.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>

#include "partition.hpp"

namespace impg {

namespace {

struct SIv {  // SampleInterval (:62-67)
  int32_t qs, qe, ts, te;
};

inline int64_t adiff(int32_t a, int32_t b) { return a > b ? (int64_t)a - b : (int64_t)b - a; }  // i32::abs_diff

// should_merge (:834-850)
inline bool should_merge(const SIv &a, const SIv &b, int32_t d) {
  if (d < 0) return false;
  const int64_t dist = d;
  return std::min(adiff(a.qe, b.qs), adiff(a.qs, b.qe)) <= dist || std::min(adiff(a.te, b.ts), adiff(a.ts, b.te)) <= dist;
}

// merge_intervals (:799-832): a left fold in (q_start, q_end) order, ties in emission order; d < 0: as they came
void merge_intervals(std::vector<SIv> &iv, int32_t d) {
  if (iv.empty() || d < 0) return;
  std::stable_sort(iv.begin(), iv.end(), [](const SIv &a, const SIv &b) { return a.qs != b.qs ? a.qs < b.qs : a.qe < b.qe; });
  std::vector<SIv> merged;
  SIv cur = iv[0];
  for (size_t i = 1; i < iv.size(); i++) {
    const SIv &nx = iv[i];
    if (should_merge(cur, nx, d)) {
      cur.qs = std::min(cur.qs, nx.qs); cur.qe = std::max(cur.qe, nx.qe);
      cur.ts = std::min(cur.ts, nx.ts); cur.te = std::max(cur.te, nx.te);
    } else {
      merged.push_back(cur);
      cur = nx;
    }
  }
  merged.push_back(cur);
  iv.swap(merged);
}

}  // namespace

void normalise_blacklist(const uint32_t *off, const int32_t *ranges, uint32_t n_seq, std::vector<uint32_t> &off_out, std::vector<int32_t> &rng_out) {
  off_out.assign((size_t)n_seq + 1, 0);
  rng_out.clear();
  if (off[0] != 0) throw Error{IMPG_E_INVALID, "blacklist offsets must start at 0"};
  std::vector<std::pair<int32_t, int32_t>> v;
  for (uint32_t q = 0; q < n_seq; q++) {
    if (off[q + 1] < off[q]) throw Error{IMPG_E_INVALID, "blacklist offsets must not descend"};
    v.clear();
    for (uint32_t k = off[q]; k < off[q + 1]; k++) {
      if (ranges[2 * (size_t)k + 1] < ranges[2 * (size_t)k]) throw Error{IMPG_E_INVALID, "blacklist range with end < start"};
      v.emplace_back(ranges[2 * (size_t)k], ranges[2 * (size_t)k + 1]);
    }
    std::sort(v.begin(), v.end());
    size_t first = rng_out.size();
    for (const auto &r : v) {
      // both ends inclusive: a range that starts at the running end still shares a position with it
      if (rng_out.size() > first && r.first <= rng_out.back()) rng_out.back() = std::max(rng_out.back(), r.second);
      else { rng_out.push_back(r.first); rng_out.push_back(r.second); }
    }
    off_out[q + 1] = (uint32_t)(rng_out.size() / 2);
  }
}

void support_host(const impg_gpu_interval_t *rows, const uint64_t *offsets, const SupportInput &in, SupportOutput &out) {
  out.count.assign(in.n_cand, 0);
  out.surv_off.assign(in.n_cand + 1, 0);
  out.survivors.clear();
  out.longest_group = 0;
  for (uint64_t i = offsets[0]; i < offsets[in.n_cand]; i++)
    if (rows[i].query_id != HIT_NONE && rows[i].query_id >= in.n_seq) throw Error{IMPG_E_INVALID, "a row names an unknown sequence"};
  std::map<uint32_t, std::vector<SIv>> per_sample;  // (the reference's map is hashed; its order shows only under the clamp)
  std::vector<uint32_t> ents;
  for (size_t c = 0; c < in.n_cand; c++) {
    const impg_gpu_range_t &cd = in.cand[c];
    per_sample.clear();
    uint64_t n_rows = 0;
    for (uint64_t i = offsets[c]; i < offsets[c + 1]; i++) {
      const impg_gpu_interval_t &r = rows[i];
      if (r.query_id == HIT_NONE) continue;  // a hole of the slot layout: not a row
      n_rows++;
      if (r.query_id == cd.target_id) continue;  // :687-689
      per_sample[r.query_id].push_back(SIv{std::min(r.q_first, r.q_last), std::max(r.q_first, r.q_last), std::min(r.t_first, r.t_last),
                                           std::max(r.t_first, r.t_last)});
    }
    if (n_rows > 1) {  // :680-682
      const int64_t rs = cd.start, re = cd.end;
      const int64_t span = std::min(std::max<int64_t>(re - rs, 0), (int64_t)std::max(in.span_bp, 0));  // :707-709
      const int64_t left_thr = rs + span, right_thr = re - span;
      ents.clear();
      for (auto &kv : per_sample) {
        out.longest_group = std::max<uint64_t>(out.longest_group, kv.second.size());
        merge_intervals(kv.second, in.merge_distance);
        bool any = false;
        int32_t lo = 0, hi = 0;
        for (const SIv &m : kv.second)
          if (m.ts <= rs && m.te >= re && m.te >= left_thr && m.ts <= right_thr) {  // covers_boundaries (:785-797)
            lo = any ? std::min(lo, m.qs) : m.qs;
            hi = any ? std::max(hi, m.qe) : m.qe;
            any = true;
          }
        if (!any) continue;
        if (!in.bl_off.empty()) {  // :736-748: any range with start <= hi and end >= lo
          const int32_t *r = in.bl_rng.data() + 2 * (size_t)in.bl_off[kv.first];
          uint32_t a = 0, b = in.bl_off[kv.first + 1] - in.bl_off[kv.first];
          while (a < b) {  // the first range with end >= lo
            const uint32_t mid = (a + b) >> 1;
            if (r[2 * mid + 1] < lo) a = mid + 1; else b = mid;
          }
          if (a < in.bl_off[kv.first + 1] - in.bl_off[kv.first] && r[2 * a] <= hi) continue;
        }
        out.survivors.push_back(impg_gpu_survivor_t{kv.first, lo, hi});  // recorded before the key is looked up (:750-756)
        const uint32_t e = in.entity_of ? in.entity_of[kv.first] : kv.first;
        if (e != NO_ENTITY) ents.push_back(e);
      }
      std::sort(ents.begin(), ents.end());
      uint64_t n = (uint64_t)(std::unique(ents.begin(), ents.end()) - ents.begin());
      if (in.max_entities) n = std::min<uint64_t>(n, in.max_entities[c]);  // what is left of the early break (:758-763)
      out.count[c] = (uint32_t)n;
    }
    out.surv_off[c + 1] = out.survivors.size();
  }
  if (!out.want_survivors) { out.survivors.clear(); out.surv_off.clear(); }
}

void SupportDevice::run_host_rows(const impg_gpu_interval_t *rows, const uint64_t *offsets, const SupportInput &in, SupportOutput &out) {
  const uint64_t first = offsets[0], n = offsets[in.n_cand] - first;
  std::vector<uint32_t> off32(in.n_cand + 1);
  for (size_t c = 0; c <= in.n_cand; c++) off32[c] = (uint32_t)(offsets[c] - first);
  up_rows.reserve(std::max<size_t>((size_t)n * sizeof(impg_gpu_interval_t), 256));
  up_off.reserve(std::max<size_t>(off32.size() * 4, 256));
  if (n) IMPG_HIP(hipMemcpyAsync(up_rows.p, rows + first, (size_t)n * sizeof(impg_gpu_interval_t), hipMemcpyHostToDevice, stream));
  IMPG_HIP(hipMemcpyAsync(up_off.p, off32.data(), off32.size() * 4, hipMemcpyHostToDevice, stream));
  IMPG_HIP(hipStreamSynchronize(stream));  // (off32 is a local)
  run(up_rows.as<impg_gpu_interval_t>(), (uint32_t)n, up_off.as<uint32_t>(), in, out);
}

}  // namespace impg

using namespace impg;

extern "C" {

int impg_gpu_support_rows(const impg_gpu_interval_t *rows, const uint64_t *offsets, const impg_gpu_range_t *cand, size_t n_cand, uint32_t n_seq,
                          const uint32_t *entity_of, const uint32_t *max_entities, const uint32_t *blacklist_off,
                          const int32_t *blacklist_ranges, const impg_gpu_support_opts_t *opts, int on_host, int device,
                          uint32_t *count_out, uint64_t *survivor_offsets_out, impg_gpu_survivor_t **survivors_out,
                          uint64_t *longest_group_out) {
  IMPG_TRY
  if (!offsets || !opts || (!cand && n_cand) || (!count_out && n_cand)) throw Error{IMPG_E_INVALID, "null argument"};
  if ((survivor_offsets_out == nullptr) != (survivors_out == nullptr)) throw Error{IMPG_E_INVALID, "survivors need both their offsets and their rows"};
  if (n_cand >= 0x7FFFFFFFu || n_seq >= 0x7FFFFFFFu) throw Error{IMPG_E_UNSUPPORTED, "too many candidates or sequences"};
  for (size_t c = 0; c < n_cand; c++)
    if (offsets[c + 1] < offsets[c]) throw Error{IMPG_E_INVALID, "row offsets must not descend"};
  const uint64_t n_rows = offsets[n_cand] - offsets[0];
  if (n_rows >= (1ull << 30)) throw Error{IMPG_E_UNSUPPORTED, "more than 2^30 rows in one call"};
  if (!rows && n_rows) throw Error{IMPG_E_INVALID, "null argument"};
  if (blacklist_off && !blacklist_ranges && blacklist_off[n_seq]) throw Error{IMPG_E_INVALID, "null argument"};
  SupportInput in;
  in.cand = cand;
  in.n_cand = n_cand;
  in.n_seq = n_seq;
  in.entity_of = entity_of;
  in.max_entities = max_entities;
  in.span_bp = opts->span_bp;
  in.merge_distance = opts->merge_distance;
  if (blacklist_off) normalise_blacklist(blacklist_off, blacklist_ranges, n_seq, in.bl_off, in.bl_rng);
  SupportOutput out;
  out.want_survivors = survivors_out != nullptr;
  if (on_host) support_host(rows, offsets, in, out);
  else {
    require_device(device);
    IMPG_HIP(hipSetDevice(device));
    SupportDevice dev(device, nullptr);
    dev.run_host_rows(rows, offsets, in, out);
  }
  for (size_t c = 0; c < n_cand; c++) count_out[c] = out.count[c];
  if (longest_group_out) *longest_group_out = out.longest_group;
  if (survivors_out) {
    for (size_t c = 0; c <= n_cand; c++) survivor_offsets_out[c] = out.surv_off[c];
    impg_gpu_survivor_t *s = (impg_gpu_survivor_t *)malloc(std::max<size_t>(out.survivors.size(), 1) * sizeof(impg_gpu_survivor_t));
    if (!s) throw std::bad_alloc();
    if (!out.survivors.empty()) memcpy(s, out.survivors.data(), out.survivors.size() * sizeof(impg_gpu_survivor_t));
    *survivors_out = s;
  }
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_entity_ids(const char *const *names, size_t n, int level, const char *separator, uint32_t *entity_out, uint32_t *n_entities_out) {
  IMPG_TRY
  if ((!names && n) || (!entity_out && n)) throw Error{IMPG_E_INVALID, "null argument"};
  if (level != IMPG_SELECT_SAMPLE && level != IMPG_SELECT_HAPLOTYPE) throw Error{IMPG_E_INVALID, "level is IMPG_SELECT_SAMPLE or IMPG_SELECT_HAPLOTYPE"};
  const std::string sep = separator ? separator : "#";
  if (sep.empty()) throw Error{IMPG_E_INVALID, "empty separator"};
  std::map<std::string, uint32_t> ids;
  for (size_t i = 0; i < n; i++) {
    if (!names[i]) throw Error{IMPG_E_INVALID, "null name"};
    const std::string nm = names[i];
    // the prefixes partition's selection groups by, except that a name without the separator has no key
    if (nm.find(sep) == std::string::npos) { entity_out[i] = NO_ENTITY; continue; }
    entity_out[i] = ids.emplace(pansn_prefix(nm, sep, level == IMPG_SELECT_HAPLOTYPE), (uint32_t)ids.size()).first->second;
  }
  if (n_entities_out) *n_entities_out = (uint32_t)ids.size();
  return IMPG_OK;
  IMPG_CATCH
}

}  // extern "C"

// ---- the search (run_refine, refine.rs:81-409) -------------------------------------------------------------------------
struct impg_gpu_refine_run {
  std::vector<impg_gpu_refine_record_t> records;
  std::vector<uint64_t> surv_off;
  std::vector<impg_gpu_survivor_t> survivors;
  uint64_t passes = 0, candidates = 0, parts = 0, rows_to_host = 0, longest_group = 0;
  // per batch (the passes, then the read of the winners' survivors): candidates, wall seconds of the query, HIP-event
  // milliseconds of the engine inside it, wall seconds of the support
  std::vector<double> batch_times;
};

namespace impg {

std::vector<int32_t> build_flanks(int32_t max_extension, int32_t step) {
  std::vector<int32_t> flanks;
  if (max_extension == 0) { flanks.push_back(0); return flanks; }
  int32_t current = 0;
  while (current <= max_extension) {
    flanks.push_back(current);
    if (max_extension - current < step) break;
    current = (int32_t)std::min<int64_t>((int64_t)current + step, INT32_MAX);  // saturating_add
  }
  if (flanks.empty() || flanks.back() != max_extension) flanks.push_back(max_extension);
  std::sort(flanks.begin(), flanks.end());
  flanks.erase(std::unique(flanks.begin(), flanks.end()), flanks.end());
  return flanks;
}

int32_t max_extension_bp(double max_extension, int32_t locus_len) {
  const double v = max_extension <= 1.0 ? std::ceil((double)locus_len * max_extension) : std::ceil(max_extension);
  if (!(v > 0)) return 0;  // (clamp(0, i32::MAX) as i32; NaN casts to 0)
  return v >= 2147483647.0 ? INT32_MAX : (int32_t)v;
}

namespace {

inline int32_t sat32(int64_t v) { return (int32_t)std::min<int64_t>(std::max<int64_t>(v, INT32_MIN), INT32_MAX); }

struct Cand {  // CandidateResult (:70-78) without its survivors
  int32_t start = 0, end = 0, left = 0, right = 0;
  uint32_t count = 0;
};
// compare_candidates(a, b) == Greater (:564-582)
inline bool greater(const Cand &a, const Cand &b) {
  if (a.count != b.count) return a.count > b.count;
  const int64_t at = (int64_t)a.left + a.right, bt = (int64_t)b.left + b.right;
  if (at != bt) return at < bt;
  const int32_t am = std::max(a.left, a.right), bm = std::max(b.left, b.right);
  if (am != bm) return am < bm;
  return (int64_t)a.end - a.start < (int64_t)b.end - b.start;
}
struct Locus {
  impg_gpu_range_t r;
  int32_t len = 0;
  std::vector<int32_t> flanks;
  bool has_max = false, have = false, done = false;
  uint32_t max_entities = 0, original = 0;
  Cand best;
  bool at_max() const { return has_max && have && best.count >= max_entities; }  // check_max (:264-270)
};

// counts (and, on request, survivors) of a batch of candidate regions; max_entities per candidate or null
using EvalFn = std::function<void(const std::vector<impg_gpu_range_t> &, const uint32_t *, SupportOutput &)>;

void check_refine_opts(const impg_gpu_refine_opts_t &o) {  // RefineOpts::validate (main.rs:4454-4473)
  if (o.span_bp < 0) throw Error{IMPG_E_INVALID, "span_bp must be >= 0"};
  if (!(o.max_extension >= 0.0)) throw Error{IMPG_E_INVALID, "max_extension must be >= 0"};
  if (o.extension_step <= 0) throw Error{IMPG_E_INVALID, "extension_step must be > 0"};
}

void refine_search(std::vector<Locus> &loci, const EvalFn &eval, impg_gpu_refine_run &res) {
  std::vector<impg_gpu_range_t> batch;
  std::vector<uint32_t> who, mx;
  std::vector<Cand> cands;
  SupportOutput out;
  bool any_max = false;
  for (const Locus &L : loci) any_max = any_max || L.has_max;
  auto evaluate = [&](bool survivors) {
    mx.resize(batch.size());
    for (size_t c = 0; c < batch.size(); c++) mx[c] = loci[who[c]].has_max ? loci[who[c]].max_entities : 0xFFFFFFFFu;
    out = SupportOutput();
    out.want_survivors = survivors;
    eval(batch, any_max ? mx.data() : nullptr, out);
    if (out.count.size() != batch.size()) throw Error{IMPG_E_INVALID, "internal: a count per candidate"};
    if (!survivors) res.passes++;  // (the read of the winners' survivors is no pass of the search)
    res.candidates += batch.size();
    res.longest_group = std::max(res.longest_group, out.longest_group);
  };
  for (int pass = 0; pass < 4; pass++) {
    batch.clear(); who.clear(); cands.clear();
    for (size_t i = 0; i < loci.size(); i++) {
      Locus &L = loci[i];
      if (L.done) continue;
      auto add = [&](int32_t left, int32_t right) {  // evaluate_candidate's region (:426-438)
        const int32_t start = std::max(sat32((int64_t)L.r.start - left), 0), end = std::min(sat32((int64_t)L.r.end + right), L.len);
        if (end <= start) return;
        Cand c;
        c.start = start; c.end = end;
        c.left = sat32((int64_t)L.r.start - start); c.right = sat32((int64_t)end - L.r.end);  // :466-467
        batch.push_back(impg_gpu_range_t{L.r.target_id, start, end});
        who.push_back((uint32_t)i);
        cands.push_back(c);
      };
      if (pass == 0) add(0, 0);
      else if (pass == 1) { for (int32_t l : L.flanks) if (l > 0) add(l, 0); }
      else if (pass == 2) { const int32_t lf = L.have ? L.best.left : 0; for (int32_t r : L.flanks) add(lf, r); }
      else { const int32_t rf = L.have ? L.best.right : 0; for (int32_t l : L.flanks) add(l, rf); }
    }
    if (!batch.empty()) {
      evaluate(false);
      // a locus's candidates are one stretch of the batch, in flank order: reduce_candidates, then the running best (:254-261)
      for (size_t c = 0; c < batch.size();) {
        Locus &L = loci[who[c]];
        Cand pb = cands[c];
        pb.count = out.count[c];
        size_t e = c + 1;
        for (; e < batch.size() && who[e] == who[c]; e++) {
          Cand x = cands[e];
          x.count = out.count[e];
          if (greater(x, pb)) pb = x;
        }
        if (pass == 0) L.original = pb.count;
        if (!L.have || greater(pb, L.best)) { L.best = pb; L.have = true; }
        c = e;
      }
    }
    for (Locus &L : loci) if (L.at_max()) L.done = true;
  }
  batch.clear(); who.clear();
  for (size_t i = 0; i < loci.size(); i++) {
    const Locus &L = loci[i];
    if (!L.have) throw Error{IMPG_E_INVALID, "no valid flank sizes evaluated for locus " + std::to_string(i)};  // :374-382
    batch.push_back(impg_gpu_range_t{L.r.target_id, L.best.start, L.best.end});
    who.push_back((uint32_t)i);
  }
  res.surv_off.assign(loci.size() + 1, 0);
  if (!batch.empty()) {
    evaluate(true);
    if (out.surv_off.size() != batch.size() + 1) throw Error{IMPG_E_INVALID, "internal: survivors per candidate"};
    res.surv_off = out.surv_off;
    res.survivors = out.survivors;
  }
  for (const Locus &L : loci)
    res.records.push_back(impg_gpu_refine_record_t{L.r.target_id, L.best.start, L.best.end, L.r.start, L.r.end, L.best.left, L.best.right,
                                                   L.best.count, L.original});
}

void init_loci(std::vector<Locus> &loci, const impg_gpu_range_t *in, size_t n, const std::function<int64_t(uint32_t)> &len_of,
               const impg_gpu_refine_opts_t &o) {
  loci.resize(n);
  for (size_t i = 0; i < n; i++) {
    Locus &L = loci[i];
    L.r = in[i];
    if (L.r.end <= L.r.start) throw Error{IMPG_E_INVALID, "locus " + std::to_string(i) + ": end must be greater than start"};  // :153-161
    const int64_t len = len_of(L.r.target_id);
    if (len < 0) throw Error{IMPG_E_INVALID, "locus " + std::to_string(i) + ": target sequence not found in index"};  // :163-168
    L.len = sat32(len);
    const int64_t locus_len = std::max<int64_t>((int64_t)L.r.end - L.r.start, 0);
    L.flanks = build_flanks(max_extension_bp(o.max_extension, sat32(locus_len)), o.extension_step);
  }
}

void fill_support_input(SupportInput &in, uint32_t n_seq, const impg_gpu_refine_opts_t &o, const uint32_t *entity_of, const uint32_t *bl_off,
                        const int32_t *bl_rng) {
  in.n_seq = n_seq;
  in.entity_of = entity_of;
  in.span_bp = o.span_bp;
  in.merge_distance = o.merge_distance;
  if (bl_off) {
    if (!bl_rng && bl_off[n_seq]) throw Error{IMPG_E_INVALID, "null argument"};
    normalise_blacklist(bl_off, bl_rng, n_seq, in.bl_off, in.bl_rng);
  }
}

// rows in host memory -> the twin, or the kernels after an upload
void support_of_host_rows(const impg_gpu_interval_t *rows, const uint64_t *offsets, SupportInput &in, const std::vector<impg_gpu_range_t> &cand,
                          const uint32_t *mx, SupportDevice *dev, SupportOutput &out) {
  in.cand = cand.data();
  in.n_cand = cand.size();
  in.max_entities = mx;
  for (size_t c = 0; c < cand.size(); c++)
    if (offsets[c + 1] < offsets[c]) throw Error{IMPG_E_INVALID, "row offsets must not descend"};
  if (offsets[cand.size()] - offsets[0] >= (1ull << 30)) throw Error{IMPG_E_UNSUPPORTED, "more than 2^30 rows in one pass"};
  if (dev) dev->run_host_rows(rows, offsets, in, out);
  else support_host(rows, offsets, in, out);
}

// compute_max_entities (:589-632) for the distinct targets of the loci, from the index's entries
void index_max_entities(const impg_gpu_index &ix, std::vector<Locus> &loci, const uint32_t *entity_of, const uint8_t *subset_keep) {
  const uint32_t n_seq = ix.view.n_seq;
  if (ix.h_tgt_off.size() != (size_t)n_seq + 1) throw Error{IMPG_E_UNSUPPORTED, "the index has no per-target offsets"};
  std::map<uint32_t, uint32_t> of_target;
  std::vector<uint32_t> qid, ents;
  for (Locus &L : loci) {
    const uint32_t t = L.r.target_id;
    auto it = of_target.find(t);
    if (it == of_target.end()) {
      const uint32_t a = ix.h_tgt_off[t], n = ix.h_tgt_off[t + 1] - a;
      qid.resize(n);
      if (n) IMPG_HIP(hipMemcpy2D(qid.data(), 4, (const char *)ix.view.entries + (size_t)a * sizeof(Entry) + offsetof(Entry, query_id), sizeof(Entry), 4,
                                  n, hipMemcpyDeviceToHost));
      const uint32_t own = entity_of ? entity_of[t] : t;
      ents.clear();
      for (uint32_t q : qid) {
        if (q == t || q >= n_seq) continue;
        if (subset_keep && !subset_keep[q]) continue;
        const uint32_t e = entity_of ? entity_of[q] : q;
        if (e != NO_ENTITY && e != own) ents.push_back(e);
      }
      std::sort(ents.begin(), ents.end());
      it = of_target.emplace(t, (uint32_t)(std::unique(ents.begin(), ents.end()) - ents.begin())).first;
    }
    L.has_max = true;
    L.max_entities = it->second;
  }
}

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct RowsFree { void operator()(impg_gpu_device_rows_t *h) const { impg_gpu_device_rows_free(h); } };
struct ResultsFree { void operator()(impg_gpu_results_t *r) const { impg_gpu_results_free(r); } };

}  // namespace
}  // namespace impg

extern "C" {

int impg_gpu_refine(impg_gpu_index_t *ix, const impg_gpu_range_t *loci_in, size_t n, const impg_gpu_params_t *params,
                    const impg_gpu_refine_opts_t *opts, const uint32_t *entity_of, const uint8_t *subset_keep, const uint32_t *blacklist_off,
                    const int32_t *blacklist_ranges, impg_gpu_refine_t **out) {
  IMPG_TRY
  if (!ix || !params || !opts || !out || (!loci_in && n)) throw Error{IMPG_E_INVALID, "null argument"};
  if (ix->shard || ix->cluster) throw Error{IMPG_E_UNSUPPORTED, "refine runs on an index of one GPU"};
  if (params->store_cigar || params->min_output_length >= 0)
    throw Error{IMPG_E_INVALID, "refine queries without store_cigar and without min_output_length (refine.rs:497-502)"};
  check_refine_opts(*opts);
  Engine::check_params(*params);
  const uint32_t n_seq = ix->view.n_seq;
  std::vector<Locus> loci;
  init_loci(loci, loci_in, n, [&](uint32_t t) -> int64_t { return t < ix->seq.lens.size() ? ix->seq.lens[t] : -1; }, *opts);
  SupportInput sin;
  fill_support_input(sin, n_seq, *opts, entity_of, blacklist_off, blacklist_ranges);
  IMPG_HIP(hipSetDevice(ix->device));
  if (opts->use_max_entities) index_max_entities(*ix, loci, entity_of, subset_keep);
  const bool host_route = opts->support_on_host || params->multi_impg || (params->transitive && params->dfs);
  std::unique_ptr<SupportDevice> dev;
  if (!opts->support_on_host) dev = std::make_unique<SupportDevice>(ix->device, nullptr);
  auto res = std::make_unique<impg_gpu_refine_run>();
  EvalFn eval = [&](const std::vector<impg_gpu_range_t> &cand, const uint32_t *mx, SupportOutput &o) {
    const double t0 = now_s();
    if (host_route) {
      impg_gpu_results_t *r = nullptr;
      const int rc = impg_gpu_query_batch_filtered(ix, cand.data(), cand.size(), params, nullptr, subset_keep, &r);
      if (rc != IMPG_OK) throw Error{rc, impg_gpu_last_error()};
      std::unique_ptr<impg_gpu_results_t, ResultsFree> hold(r);
      const double t1 = now_s();
      double engine_s = 0, assemble_s = 0;
      impg_gpu_results_timing(r, &engine_s, &assemble_s);
      res->rows_to_host += impg_gpu_results_total(r);
      res->parts++;
      IMPG_HIP(hipSetDevice(ix->device));
      support_of_host_rows(impg_gpu_results_intervals(r), impg_gpu_results_offsets(r), sin, cand, mx, dev.get(), o);
      res->batch_times.insert(res->batch_times.end(), {(double)cand.size(), t1 - t0, engine_s * 1e3, now_s() - t1});
      return;
    }
    impg_gpu_device_rows_t *h = nullptr;
    const int rc = query_batch_device_filtered(ix, cand.data(), cand.size(), 0, params, IMPG_ROWS_ORDERED_SLOTS, subset_keep, &h);
    if (rc != IMPG_OK) throw Error{rc, impg_gpu_last_error()};
    std::unique_ptr<impg_gpu_device_rows_t, RowsFree> hold(h);  // (freed before the next pass)
    const double t1 = now_s();
    impg_gpu_stats_t st;
    impg_gpu_device_rows_stats(h, &st);
    IMPG_HIP(hipSetDevice(ix->device));
    o.count.assign(cand.size(), 0);
    if (o.want_survivors) o.surv_off.assign(1, 0);
    size_t next = 0;
    const size_t np = impg_gpu_device_rows_num_parts(h);
    for (size_t k = 0; k < np; k++) {
      impg_gpu_device_part_t pt;
      if (impg_gpu_device_rows_part(h, k, &pt) != IMPG_OK) throw Error{IMPG_E_INVALID, impg_gpu_last_error()};
      if (pt.first_range != next || pt.first_range + pt.n_ranges > cand.size()) throw Error{IMPG_E_INVALID, "internal: the parts of a batch in range order"};
      if (pt.n_slots >= (1ull << 30)) throw Error{IMPG_E_UNSUPPORTED, "a part of more than 2^30 rows: lower chunk_ranges"};
      sin.cand = cand.data() + pt.first_range;
      sin.n_cand = pt.n_ranges;
      sin.max_entities = mx ? mx + pt.first_range : nullptr;
      SupportOutput po;
      po.want_survivors = o.want_survivors;
      dev->run(pt.rows, (uint32_t)pt.n_slots, pt.offsets, sin, po);
      for (size_t c = 0; c < pt.n_ranges; c++) o.count[pt.first_range + c] = po.count[c];
      o.longest_group = std::max(o.longest_group, po.longest_group);
      if (o.want_survivors) {
        const uint64_t base = o.survivors.size();
        for (size_t c = 0; c < pt.n_ranges; c++) o.surv_off.push_back(base + po.surv_off[c + 1]);
        o.survivors.insert(o.survivors.end(), po.survivors.begin(), po.survivors.end());
      }
      next = pt.first_range + pt.n_ranges;
      res->parts++;
    }
    if (next != cand.size()) throw Error{IMPG_E_INVALID, "internal: the parts of a batch cover it"};
    res->batch_times.insert(res->batch_times.end(), {(double)cand.size(), t1 - t0, (double)st.ms_total + impg_gpu_device_rows_place_ms(h), now_s() - t1});
  };
  refine_search(loci, eval, *res);
  ix->refine_stats[REFINE_PASSES] += res->passes;
  ix->refine_stats[REFINE_CANDIDATES] += res->candidates;
  ix->refine_stats[REFINE_PARTS] += res->parts;
  ix->refine_stats[REFINE_ROWS_TO_HOST] += res->rows_to_host;
  uint64_t seen = ix->refine_stats[REFINE_LONGEST_GROUP].load();
  while (seen < res->longest_group && !ix->refine_stats[REFINE_LONGEST_GROUP].compare_exchange_weak(seen, res->longest_group)) {}
  *out = res.release();
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_refine_rows(impg_gpu_rows_cb query, void *ctx, const int64_t *seq_len, uint32_t n_seq, const impg_gpu_range_t *loci_in, size_t n,
                         const impg_gpu_refine_opts_t *opts, const uint32_t *entity_of, const uint32_t *max_entities,
                         const uint32_t *blacklist_off, const int32_t *blacklist_ranges, int device, impg_gpu_refine_t **out) {
  IMPG_TRY
  if (!query || !opts || !out || (!loci_in && n) || (!seq_len && n_seq)) throw Error{IMPG_E_INVALID, "null argument"};
  if (n_seq >= 0x7FFFFFFFu) throw Error{IMPG_E_UNSUPPORTED, "too many sequences"};
  check_refine_opts(*opts);
  std::vector<Locus> loci;
  init_loci(loci, loci_in, n, [&](uint32_t t) -> int64_t { return t < n_seq ? seq_len[t] : -1; }, *opts);
  if (max_entities)
    for (size_t i = 0; i < n; i++) { loci[i].has_max = true; loci[i].max_entities = max_entities[i]; }
  SupportInput sin;
  fill_support_input(sin, n_seq, *opts, entity_of, blacklist_off, blacklist_ranges);
  std::unique_ptr<SupportDevice> dev;
  if (!opts->support_on_host) {
    require_device(device);
    IMPG_HIP(hipSetDevice(device));
    dev = std::make_unique<SupportDevice>(device, nullptr);
  }
  auto res = std::make_unique<impg_gpu_refine_run>();
  EvalFn eval = [&](const std::vector<impg_gpu_range_t> &cand, const uint32_t *mx, SupportOutput &o) {
    const impg_gpu_interval_t *rows = nullptr;
    const uint64_t *offsets = nullptr;
    if (query(ctx, cand.data(), cand.size(), &rows, &offsets) != 0) throw Error{IMPG_E_CANCELLED, "the row source stopped the search"};
    if (!offsets || (!rows && offsets[cand.size()] != offsets[0])) throw Error{IMPG_E_INVALID, "the row source returned no rows"};
    res->parts++;
    support_of_host_rows(rows, offsets, sin, cand, mx, dev.get(), o);
  };
  refine_search(loci, eval, *res);
  *out = res.release();
  return IMPG_OK;
  IMPG_CATCH
}

size_t impg_gpu_refine_num_records(const impg_gpu_refine_t *r) { return r ? r->records.size() : 0; }
const impg_gpu_refine_record_t *impg_gpu_refine_records(const impg_gpu_refine_t *r) { return r ? r->records.data() : nullptr; }
const uint64_t *impg_gpu_refine_survivor_offsets(const impg_gpu_refine_t *r) { return r ? r->surv_off.data() : nullptr; }
const impg_gpu_survivor_t *impg_gpu_refine_survivors(const impg_gpu_refine_t *r) { return r ? r->survivors.data() : nullptr; }
void impg_gpu_refine_stats(const impg_gpu_refine_t *r, uint64_t *passes, uint64_t *candidates, uint64_t *parts) {
  if (!r) return;
  if (passes) *passes = r->passes;
  if (candidates) *candidates = r->candidates;
  if (parts) *parts = r->parts;
}
int impg_gpu_refine_batch_times(const impg_gpu_refine_t *r, double *out, size_t cap, size_t *n_out) {
  IMPG_TRY
  if (!r || !n_out || (!out && cap)) throw Error{IMPG_E_INVALID, "null argument"};
  for (size_t i = 0; i < r->batch_times.size() && i < cap; i++) out[i] = r->batch_times[i];
  *n_out = r->batch_times.size();
  return IMPG_OK;
  IMPG_CATCH
}
void impg_gpu_refine_free(impg_gpu_refine_t *r) { delete r; }

static char *text_copy(const std::string &s, size_t *len) {
  char *p = (char *)malloc(s.size() + 1);
  if (!p) throw std::bad_alloc();
  memcpy(p, s.data(), s.size());
  p[s.size()] = 0;
  *len = s.size();
  return p;
}

int impg_gpu_refine_text(const impg_gpu_refine_t *r, const char *const *names, uint32_t n_seq, const char *const *labels, char **text, size_t *len,
                         char **support_text, size_t *support_len) {
  IMPG_TRY
  if (!r || !text || !len || (!names && n_seq) || (support_text && !support_len)) throw Error{IMPG_E_INVALID, "null argument"};
  std::string t = "#chrom\tstart\tend\tname\toriginal.support\tnew.support\tleft.extension.bp\tright.extension.bp\n", sup;
  std::vector<std::pair<std::string, const impg_gpu_survivor_t *>> ents;
  for (size_t i = 0; i < r->records.size(); i++) {
    const impg_gpu_refine_record_t &rec = r->records[i];
    if (rec.target_id >= n_seq || !names[rec.target_id]) throw Error{IMPG_E_INVALID, "a record's target has no name"};
    const std::string chrom = names[rec.target_id];
    std::string name = labels && labels[i] ? labels[i] : "";
    // (str::trim cuts Unicode White_Space; here the ASCII part of it: a label of other blanks only is printed as it is)
    if (name.find_first_not_of(" \t\n\v\f\r") == std::string::npos || name == ".")
      name = chrom + ":" + std::to_string(rec.original_start) + "-" + std::to_string(rec.original_end);
    t += chrom + "\t" + std::to_string(rec.refined_start) + "\t" + std::to_string(rec.refined_end) + "\t" + name + "\t" +
         std::to_string(rec.original_support_count) + "\t" + std::to_string(rec.support_count) + "\t" + std::to_string(rec.left_extension) + "\t" +
         std::to_string(rec.right_extension) + "\n";
    if (!support_text) continue;
    ents.clear();
    for (uint64_t k = r->surv_off[i]; k < r->surv_off[i + 1]; k++) {
      const impg_gpu_survivor_t &s = r->survivors[k];
      if (s.seq_id >= n_seq || !names[s.seq_id]) throw Error{IMPG_E_INVALID, "a survivor has no name"};
      ents.emplace_back(names[s.seq_id], &s);
    }
    std::sort(ents.begin(), ents.end(), [](const auto &a, const auto &b) { return a.first != b.first ? a.first < b.first : a.second->q_lo < b.second->q_lo; });  // refine.rs:776-780
    for (const auto &e : ents) sup += e.first + "\t" + std::to_string(e.second->q_lo) + "\t" + std::to_string(e.second->q_hi) + "\t" + name + "\n";
  }
  *text = text_copy(t, len);
  if (support_text) *support_text = text_copy(sup, support_len);
  return IMPG_OK;
  IMPG_CATCH
}

}  // extern "C"
