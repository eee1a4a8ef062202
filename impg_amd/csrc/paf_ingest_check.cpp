// A stand-alone program over the host side of impg_gpu_index_create_from_paf_streamed (paf_ingest.cpp: the driver and the
// kernels' host twin; sequence_ingest.cpp: the reader), to be built with -fsanitize=address,undefined
// (`make paf_ingest_check`) and run over good and malformed PAF files.  No GPU call is made.
//   paf_ingest_check PIECE_BYTES HASH_BITS POOL_OPS FILE...
// Prints what the route answers for the files; exits 0 unless a sanitizer stops it.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "paf_ingest.hpp"

static std::string g_said;
namespace impg {
void set_error(const std::string &msg) { g_said = msg; }
// (the device leg lives in paf_ingest_device.hip, which this program leaves out)
void paf_ingest_selftest_device(const std::vector<std::string> &, size_t, int, unsigned, uint64_t, paf_ingest::Loaded &, std::vector<impg_gpu_record_t> &,
                                std::vector<uint32_t> &) {
  throw Error{IMPG_E_UNSUPPORTED, "paf_ingest_check has no device leg"};
}
}  // namespace impg

int main(int argc, char **argv) {
  if (argc < 5) { fprintf(stderr, "usage: %s PIECE_BYTES HASH_BITS POOL_OPS FILE...\n", argv[0]); return 2; }
  const uint64_t piece = strtoull(argv[1], nullptr, 10), pool = strtoull(argv[3], nullptr, 10);
  const unsigned hash_bits = (unsigned)atoi(argv[2]);
  std::vector<const char *> paths(argv + 4, argv + argc);
  impg_gpu_record_t *records = nullptr;
  uint32_t *ops = nullptr;
  char *names = nullptr;
  int64_t *lens = nullptr;
  uint64_t *file_first = nullptr, stats[impg::paf_ingest::N_STATS] = {};
  size_t n_records = 0, n_ops = 0, names_len = 0, n_seq = 0;
  const int rc = impg_gpu_selftest_paf_ingest(paths.data(), paths.size(), piece, 1, 0, hash_bits, pool, &records, &n_records, &ops, &n_ops, &names, &names_len,
                                              &lens, &n_seq, &file_first, stats);
  uint64_t sum = 0;
  for (size_t i = 0; !rc && i < n_ops; i++) sum = sum * 1099511628211ull + ops[i];
  for (size_t i = 0; !rc && i < n_records; i++) sum = sum * 1099511628211ull + records[i].cigar_off + records[i].query_id + 3u * records[i].target_id;
  printf("ingest: %d %s (%zu records, %zu ops, %zu sequences, hash %016llx, %llu pieces, %llu carried, %llu grows, %llu regrows)\n", rc,
         rc ? g_said.c_str() : "ok", n_records, n_ops, n_seq, (unsigned long long)sum, (unsigned long long)stats[1], (unsigned long long)stats[4],
         (unsigned long long)stats[5], (unsigned long long)stats[6]);
  free(records); free(ops); free(names); free(lens); free(file_first);
  return 0;
}
