// A stand-alone program over the host side of impg_gpu_index_load_sequences (sequence_ingest.cpp: the reader and the kernels'
// host twin), to be built with -fsanitize=address,undefined (`make sequence_ingest_check`) and run over good and malformed
// files (scripts/sequence_ingest_sanitize.py writes them and runs it).  No GPU call is made.
//   sequence_ingest_check PIECE_BYTES PACKED NAMES LENS FILE...     NAMES / LENS: the index's, comma separated
// Prints what the reader and the whole route answer for the files; exits 0 unless a sanitizer stops it.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/impg_gpu.h"

static std::string g_said;
namespace impg {
void set_error(const std::string &msg) { g_said = msg; }
}  // namespace impg

static std::vector<std::string> split(const std::string &s) {
  std::vector<std::string> out;
  for (size_t at = 0; at <= s.size();) {
    const size_t e = std::min(s.find(',', at), s.size());
    if (e > at) out.push_back(s.substr(at, e - at));
    at = e + 1;
  }
  return out;
}

int main(int argc, char **argv) {
  if (argc < 6) { fprintf(stderr, "usage: %s PIECE_BYTES PACKED NAMES LENS FILE...\n", argv[0]); return 2; }
  const uint64_t piece = strtoull(argv[1], nullptr, 10);
  const int packed = atoi(argv[2]);
  const std::vector<std::string> names = split(argv[3]), len_s = split(argv[4]);
  if (names.size() != len_s.size()) { fprintf(stderr, "one length per name\n"); return 2; }
  std::vector<const char *> nm, paths(argv + 5, argv + argc);
  std::vector<int64_t> lens;
  for (size_t i = 0; i < names.size(); i++) { nm.push_back(names[i].c_str()); lens.push_back(atoll(len_s[i].c_str())); }
  for (const char *p : paths) {
    char *text = nullptr;
    size_t len = 0;
    uint64_t pieces = 0, blocks = 0;
    const int rc = impg_gpu_selftest_sequence_reader(p, piece, &text, &len, &pieces, &blocks);
    printf("reader %s: %d %s (%zu bytes, %llu pieces, %llu blocks)\n", p, rc, rc ? g_said.c_str() : "ok", len, (unsigned long long)pieces, (unsigned long long)blocks);
    free(text);
  }
  std::vector<uint64_t> off(names.size() + 1), run_off(names.size() + 1);
  uint8_t *store = nullptr, *run_byte = nullptr;
  uint32_t *run_start = nullptr, *run_end = nullptr;
  size_t store_bytes = 0;
  uint64_t stats[5] = {0, 0, 0, 0, 0};
  const int rc = impg_gpu_selftest_sequence_ingest_host(paths.data(), paths.size(), nm.data(), lens.data(), names.size(), piece, packed, off.data(), &store,
                                                        &store_bytes, run_off.data(), &run_start, &run_end, &run_byte, stats);
  uint64_t sum = 0;
  for (size_t i = 0; !rc && i < store_bytes; i++) sum = sum * 1099511628211ull + store[i];
  printf("ingest: %d %s (store %zu bytes, hash %016llx, %llu runs, %llu pieces, %llu bases)\n", rc, rc ? g_said.c_str() : "ok", store_bytes,
         (unsigned long long)sum, (unsigned long long)run_off[names.size()], (unsigned long long)stats[0], (unsigned long long)stats[2]);
  free(store); free(run_start); free(run_end); free(run_byte);
  return 0;
}
