// A stand-alone program over the host side of the resolve pass (cigar_resolve.cpp: what the host decides per record, and the
// kernels' host twin), to be built with -fsanitize=address,undefined (`make cigar_resolve_check`).  It makes its own input:
// records on both strands with indels and planted mismatches whose query intervals start at base 0 and end at the last base,
// and the four kinds of record that must be copied and never read (a sequence the store lacks, a stored length that
// differs, an interval past its end, ops that do not add up).  No GPU call is made.
//   cigar_resolve_check [RECORDS]
// Prints the report; exits 0 unless the report disagrees with what was planted or a sanitizer stops it.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "cigar_resolve.hpp"

struct impg_gpu_sequences {
  impg::SeqStore st;
};
static std::string g_said;
namespace impg {
void set_error(const std::string &msg) { g_said = msg; }
void require_device(int) {}
const SeqStore &store_of(const impg_gpu_sequences_t *seqs) { return seqs->st; }
namespace cigar_resolve {
// (the device leg lives in cigar_resolve_device.hip, which this program leaves out)
void resolve_device(const impg_gpu_record_t *, size_t, const uint32_t *, size_t, const Plan &, const SeqStore &, uint32_t, int, Result &, DevBuf &) {
  throw Error{IMPG_E_UNSUPPORTED, "cigar_resolve_check has no device leg"};
}
}  // namespace cigar_resolve
void DevBuf::reserve(size_t) {}
void DevBuf::release() {}
}  // namespace impg

static uint64_t g_state = 88172645463325252ull;
static uint32_t rnd(uint32_t n) {
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return (uint32_t)((g_state >> 11) % n);
}

int main(int argc, char **argv) {
  const size_t n_good = argc > 1 ? (size_t)atol(argv[1]) : 200;
  std::string T(20000, 'A'), Q, other(500, 'C');
  for (char &c : T) c = "ACGTN"[rnd(5)];
  std::vector<impg_gpu_record_t> recs;
  std::vector<uint32_t> ops;
  uint64_t want_x = 0, want_eq = 0;
  for (size_t k = 0; k < n_good; k++) {  // query bases derived from the target op by op, then laid down on the record's strand
    const uint32_t strand = (uint32_t)(k & 1), n_ops = 1 + rnd(5);
    uint32_t t = rnd(15000);
    impg_gpu_record_t r{0, 1, (int32_t)Q.size(), 0, (int32_t)t, 0, ops.size(), 0, strand};
    std::string seg;
    for (uint32_t j = 0; j < n_ops; j++) {
      if (j) {
        const uint32_t gap = 1 + rnd(4), ins = rnd(2);
        ops.push_back((ins ? 2u : 3u) << 29 | gap);
        if (ins) seg.append(gap, 'G');
        else t += gap;
      }
      const uint32_t len = rnd(300);
      ops.push_back(4u << 29 | len);
      for (uint32_t p = 0; p < len; p++) {
        const char b = T[t + p];
        const bool x = rnd(10) == 0;
        seg.push_back(x ? (b == 'A' ? 'C' : 'A') : b);
        (x ? want_x : want_eq)++;
      }
      t += len;
    }
    if (strand) {
      std::string rc(seg.rbegin(), seg.rend());
      for (char &c : rc) c = (char)impg::cigar_resolve::comp((uint8_t)c);
      seg = rc;
    }
    Q += seg;
    r.query_end = (int32_t)Q.size();
    r.target_end = (int32_t)t;
    r.cigar_len = (uint32_t)(ops.size() - r.cigar_off);
    recs.push_back(r);
  }
  auto one_m = [&](uint32_t q, uint32_t tg, int32_t qs, int32_t ts, uint32_t len, int32_t extra) {
    recs.push_back(impg_gpu_record_t{q, tg, qs, qs + (int32_t)len, ts, ts + (int32_t)len + extra, ops.size(), 1, 0});
    ops.push_back(4u << 29 | len);
  };
  one_m(0, 2, 0, 0, 100, 0);                            // "gone": the store lacks it
  one_m(0, 3, 0, 100, 300, 0);                          // "short": the store's copy is shorter than the table says
  one_m(0, 1, 0, (int32_t)T.size() - 50, 100, 0);       // an interval past the target's end
  one_m(0, 1, 0, 10, 100, 1);                           // ops that do not add up
  impg_gpu_sequences seqs;
  impg::SeqStore &st = seqs.st;
  st.off.push_back(0);
  for (auto &nb : {std::make_pair(std::string("Q"), &Q), std::make_pair(std::string("T"), &T), std::make_pair(std::string("short"), &other)}) {
    st.by_name.emplace(nb.first, (uint32_t)st.names.size());
    st.names.push_back(nb.first);
    st.bases += *nb.second;
    st.off.push_back(st.bases.size());
  }
  const char *names[4] = {"Q", "T", "gone", "short"};
  const int64_t lens[4] = {(int64_t)Q.size(), (int64_t)T.size(), 1000, 600};
  impg_gpu_record_t *out_rec = nullptr;
  uint32_t *out_ops = nullptr;
  uint8_t *flags = nullptr;
  size_t n_out = 0;
  impg_gpu_resolve_report_t rep{};
  const int rc = impg_gpu_cigar_resolve(recs.data(), recs.size(), ops.data(), ops.size(), names, lens, 4, &seqs, 1, 0, &out_rec, &out_ops, &n_out, &flags, &rep);
  printf("resolve: %d %s (records %llu resolved %llu absent %llu inconsistent %llu ops %llu -> %llu, M bases %llu = %llu X %llu)\n", rc,
         rc ? g_said.c_str() : "ok", (unsigned long long)rep.records, (unsigned long long)rep.resolved, (unsigned long long)rep.absent,
         (unsigned long long)rep.inconsistent, (unsigned long long)rep.ops_in, (unsigned long long)rep.ops_out, (unsigned long long)rep.m_bases,
         (unsigned long long)rep.m_eq_bases, (unsigned long long)rep.m_x_bases);
  const bool ok = rc == IMPG_OK && rep.resolved == n_good && rep.absent == 1 && rep.inconsistent == 3 && rep.m_x_bases == want_x &&
                  rep.m_eq_bases == want_eq && n_out == rep.ops_out && flags[n_good] == 1 && flags[n_good + 1] == 2 && flags[n_good + 2] == 2 &&
                  flags[n_good + 3] == 2;
  free(out_rec); free(out_ops); free(flags);
  if (!ok) { fprintf(stderr, "the report is not what was planted\n"); return 1; }
  return 0;
}
