// M ops resolved against the sequences (cigar_resolve.hpp): what the host decides before an op is read, the host twin of
// the kernels, and the C calls of the pass alone.  impg_gpu_index_create_from_paf_resolved is in capi.cpp.
#include "cigar_resolve.hpp"

#include "engine.hpp"

namespace impg {
namespace cigar_resolve {

Plan make_plan(const impg_gpu_record_t *records, size_t n_records, size_t n_ops, const char *const *names_of_ids, const int64_t *seq_len,
               uint32_t n_seq, const SeqStore &st) {
  Plan p;
  p.store_of_id.assign(n_seq, SEQ_ABSENT);
  std::vector<uint8_t> len_ok(n_seq, 0);
  for (uint32_t id = 0; id < n_seq; id++) {
    if (!names_of_ids[id]) continue;
    auto it = st.by_name.find(names_of_ids[id]);
    if (it == st.by_name.end()) continue;
    p.store_of_id[id] = it->second;
    len_ok[id] = (int64_t)(st.off[it->second + 1] - st.off[it->second]) == seq_len[id];
  }
  p.pre.assign(n_records, FLAG_OK);
  p.first.assign(n_records + 1, 0);
  for (size_t i = 0; i < n_records; i++) {
    const impg_gpu_record_t &r = records[i];
    if (r.query_id >= n_seq || r.target_id >= n_seq) throw Error{IMPG_E_INVALID, "record sequence id out of range"};
    if (r.cigar_off + r.cigar_len > n_ops) throw Error{IMPG_E_INVALID, "record CIGAR outside the op pool"};
    p.first[i + 1] = p.first[i] + r.cigar_len;
    if (!r.cigar_len) continue;
    if (p.store_of_id[r.query_id] == SEQ_ABSENT || p.store_of_id[r.target_id] == SEQ_ABSENT) p.pre[i] = FLAG_ABSENT;
    else if (!len_ok[r.query_id] || !len_ok[r.target_id] || r.strand > 1 || r.query_start < 0 || r.query_start > r.query_end ||
             r.query_end > seq_len[r.query_id] || r.target_start < 0 || r.target_start > r.target_end || r.target_end > seq_len[r.target_id])
      p.pre[i] = FLAG_INCONSISTENT;
  }
  return p;
}

void finish(const impg_gpu_record_t *records, size_t n_records, Result &r) {
  impg_gpu_resolve_report_t &rep = r.report;
  rep.records = n_records;
  rep.resolved = rep.absent = rep.inconsistent = rep.ops_in = 0;
  for (size_t i = 0; i < n_records; i++) {
    rep.ops_in += records[i].cigar_len;
    if (!records[i].cigar_len) continue;
    (r.flags[i] == FLAG_OK ? rep.resolved : r.flags[i] == FLAG_ABSENT ? rep.absent : rep.inconsistent)++;
  }
  rep.ops_out = r.n_out;
}

void resolve_host(const impg_gpu_record_t *records, size_t n_records, const uint32_t *ops, const Plan &plan, const SeqStore &st, Result &r,
                  std::vector<uint32_t> &out) {
  r = Result{};
  r.off.resize(n_records);
  r.len.resize(n_records);
  r.flags = plan.pre;
  out.clear();
  impg_gpu_resolve_report_t &rep = r.report;
  for (size_t i = 0; i < n_records; i++) {
    const impg_gpu_record_t &rc = records[i];
    const uint32_t *o = ops + rc.cigar_off;
    r.off[i] = out.size();
    if (rc.cigar_len && r.flags[i] == FLAG_OK) {
      uint64_t st_ = 0, sq = 0;
      bool bad = false;
      for (uint32_t k = 0; k < rc.cigar_len; k++) {
        const uint32_t code = o[k] >> 29, len = o[k] & OP_LEN_MASK;
        if (code > 4) bad = true;
        if (code != 2) st_ += len;
        if (code != 3) sq += len;
      }
      if (bad || st_ != (uint64_t)(rc.target_end - rc.target_start) || sq != (uint64_t)(rc.query_end - rc.query_start)) r.flags[i] = FLAG_INCONSISTENT;
    }
    if (!rc.cigar_len || r.flags[i] != FLAG_OK) {
      out.insert(out.end(), o, o + rc.cigar_len);
      r.len[i] = rc.cigar_len;
      continue;
    }
    const uint8_t *T = (const uint8_t *)st.bases.data() + st.off[plan.store_of_id[rc.target_id]];
    const uint8_t *Q = (const uint8_t *)st.bases.data() + st.off[plan.store_of_id[rc.query_id]];
    uint64_t t = (uint64_t)rc.target_start, q = 0;
    auto differ = [&](uint64_t tp, uint64_t qp) {
      return T[tp] != (rc.strand ? comp(Q[(uint64_t)rc.query_end - 1 - qp]) : Q[(uint64_t)rc.query_start + qp]);
    };
    for (uint32_t k = 0; k < rc.cigar_len; k++) {
      const uint32_t code = o[k] >> 29, len = o[k] & OP_LEN_MASK;
      if (code == 4) {
        rep.m_ops++;
        rep.m_bases += len;
        if (!len) out.push_back(0);
        for (uint32_t p = 0; p < len;) {
          const bool x = differ(t + p, q + p);
          uint32_t e = p + 1;
          while (e < len && differ(t + e, q + e) == x) e++;
          out.push_back((x ? 1u << 29 : 0u) | (e - p));
          (x ? rep.m_x_bases : rep.m_eq_bases) += e - p;
          p = e;
        }
      } else {
        out.push_back(o[k]);
        if (code <= 1)
          for (uint32_t p = 0; p < len; p++) {
            const bool x = differ(t + p, q + p);
            if (code == 0 && x) rep.bad_eq_bases++;
            if (code == 1 && !x) rep.bad_x_bases++;
          }
      }
      if (code != 2) t += len;
      if (code != 3) q += len;
    }
    const uint64_t n = out.size() - r.off[i];
    if (n > OP_LEN_MASK) throw Error{IMPG_E_UNSUPPORTED, "CIGAR longer than 2^29 ops"};
    r.len[i] = (uint32_t)n;
  }
  r.n_out = out.size();
  finish(records, n_records, r);
}

namespace {
template <class T> T *malloc_n(size_t n) {
  T *p = (T *)malloc(std::max<size_t>(n, 1) * sizeof(T));
  if (!p) throw std::bad_alloc();
  return p;
}

int run(const impg_gpu_record_t *records, size_t n_records, const uint32_t *ops, size_t n_ops, const char *const *names_of_ids,
        const int64_t *seq_len, uint32_t n_seq, const impg_gpu_sequences_t *seqs, int on_host, int device, uint32_t tile_bases,
        impg_gpu_record_t **records_out, uint32_t **ops_out, size_t *n_ops_out, uint8_t **flags_out, impg_gpu_resolve_report_t *report) {
  IMPG_TRY
  if ((n_records && !records) || (n_ops && !ops) || (n_seq && (!names_of_ids || !seq_len)) || !seqs || !records_out || !ops_out || !n_ops_out || !flags_out)
    throw Error{IMPG_E_INVALID, "null argument"};
  if (tile_bases % 64 || tile_bases > TILE_BASES_MAX) throw Error{IMPG_E_INVALID, "tile_bases is 0 or a multiple of 64 up to 4096"};
  const SeqStore &st = host_copy(store_of(seqs));
  const Plan plan = make_plan(records, n_records, n_ops, names_of_ids, seq_len, n_seq, st);
  Result r;
  uint32_t *pool = nullptr;
  if (on_host) {
    std::vector<uint32_t> out;
    resolve_host(records, n_records, ops, plan, st, r, out);
    pool = malloc_n<uint32_t>(out.size());
    if (!out.empty()) memcpy(pool, out.data(), out.size() * 4);
  } else {
    require_device(device);
    IMPG_HIP(hipSetDevice(device));
    DevBuf d_ops, d_out;
    d_ops.reserve(std::max<size_t>(n_ops * 4, 256));
    if (n_ops) IMPG_HIP(hipMemcpy(d_ops.p, ops, n_ops * 4, hipMemcpyHostToDevice));
    resolve_device(records, n_records, d_ops.as<uint32_t>(), n_ops, plan, st, tile_bases, device, r, d_out);
    pool = malloc_n<uint32_t>(r.n_out);
    if (r.n_out) {
      const hipError_t e = hipMemcpy(pool, d_out.p, r.n_out * 4, hipMemcpyDeviceToHost);
      if (e != hipSuccess) { free(pool); IMPG_HIP(e); }
    }
  }
  impg_gpu_record_t *recs = malloc_n<impg_gpu_record_t>(n_records);
  uint8_t *flags = malloc_n<uint8_t>(n_records);
  for (size_t i = 0; i < n_records; i++) {
    recs[i] = records[i];
    recs[i].cigar_off = r.off[i];
    recs[i].cigar_len = r.len[i];
    flags[i] = r.flags[i];
  }
  *records_out = recs;
  *ops_out = pool;
  *n_ops_out = (size_t)r.n_out;
  *flags_out = flags;
  if (report) *report = r.report;
  return IMPG_OK;
  IMPG_CATCH
}
}  // namespace

}  // namespace cigar_resolve
}  // namespace impg

extern "C" int impg_gpu_cigar_resolve(const impg_gpu_record_t *records, size_t n_records, const uint32_t *ops, size_t n_ops,
                                      const char *const *names_of_ids, const int64_t *seq_len, uint32_t n_seq, const impg_gpu_sequences_t *seqs,
                                      int on_host, int device, impg_gpu_record_t **records_out, uint32_t **ops_out, size_t *n_ops_out,
                                      uint8_t **flags_out, impg_gpu_resolve_report_t *report) {
  return impg::cigar_resolve::run(records, n_records, ops, n_ops, names_of_ids, seq_len, n_seq, seqs, on_host, device, 0, records_out, ops_out,
                                  n_ops_out, flags_out, report);
}

extern "C" int impg_gpu_selftest_cigar_resolve(const impg_gpu_record_t *records, size_t n_records, const uint32_t *ops, size_t n_ops,
                                               const char *const *names_of_ids, const int64_t *seq_len, uint32_t n_seq,
                                               const impg_gpu_sequences_t *seqs, int on_host, int device, uint32_t tile_bases,
                                               impg_gpu_record_t **records_out, uint32_t **ops_out, size_t *n_ops_out, uint8_t **flags_out,
                                               impg_gpu_resolve_report_t *report) {
  return impg::cigar_resolve::run(records, n_records, ops, n_ops, names_of_ids, seq_len, n_seq, seqs, on_host, device, tile_bases, records_out,
                                  ops_out, n_ops_out, flags_out, report);
}
