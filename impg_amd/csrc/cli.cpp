// impg-gpu: the `impg query` command line (reference src/main.rs:4259-4381,
// :6513-7520) over libimpg_gpu.so, for the BED output path.  Same flags, same
// defaults, same validation order, same bytes on stdout; every BED row of a
// `-b` file goes to the GPU in ONE batch instead of the reference's serial loop
// (main.rs:7435).
#include <unistd.h>

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <fstream>
#include <functional>
#include <string>
#include <vector>

#include "../../include/impg_gpu.h"

namespace {

[[noreturn]] void die(const std::string &msg, int code = 1) {
  fprintf(stderr, "Error: %s\n", msg.c_str());
  exit(code);
}

// clap's "-d" accepts metric suffixes (50k, 1m): main.rs parse of merge distance
bool parse_metric(const char *s, long long *out) {
  char *end = nullptr;
  double v = strtod(s, &end);
  if (end == s) return false;
  long long mul = 1;
  if (*end == 'k' || *end == 'K') { mul = 1000; end++; }
  else if (*end == 'm' || *end == 'M') { mul = 1000000; end++; }
  else if (*end == 'g' || *end == 'G') { mul = 1000000000; end++; }
  if (*end) return false;
  *out = (long long)llround(v * (double)mul);
  return true;
}

struct Target {
  std::string seq, name;
  int32_t start, end;
};

bool parse_i32(const std::string &s, int32_t *v) {
  if (s.empty()) return false;
  size_t i = (s[0] == '+' || s[0] == '-') ? 1 : 0;
  if (i >= s.size()) return false;
  long long x = 0;
  for (; i < s.size(); i++) {
    if (s[i] < '0' || s[i] > '9') return false;
    x = x * 10 + (s[i] - '0');
    if (x > 2147483648ll) return false;
  }
  if (s[0] == '-') x = -x;
  if (x > 2147483647ll) return false;
  *v = (int32_t)x;
  return true;
}

// parse_bed_file (src/commands/partition.rs:1719-1750)
std::vector<Target> parse_bed_file(const std::string &path) {
  std::ifstream in(path);
  if (!in) die("No such file or directory: " + path);
  std::vector<Target> out;
  std::string line;
  while (std::getline(in, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    std::vector<std::string> parts;
    size_t st = 0;
    for (size_t i = 0; i <= line.size(); i++)
      if (i == line.size() || line[i] == '\t') { parts.push_back(line.substr(st, i - st)); st = i + 1; }
    if (parts.size() < 3) die("Invalid BED file format");
    Target t;
    if (!parse_i32(parts[1], &t.start)) die("Invalid start value");
    if (!parse_i32(parts[2], &t.end)) die("Invalid end value");
    if (t.start >= t.end) die("Start value must be less than end value");
    t.seq = parts[0];
    std::string nm;
    if (parts.size() > 3) {
      nm = parts[3];
      size_t a = nm.find_first_not_of(" \t\r\n\v\f"), b = nm.find_last_not_of(" \t\r\n\v\f");
      nm = a == std::string::npos ? "" : nm.substr(a, b - a + 1);
    }
    if (nm.empty() || nm == ".") nm = t.seq + ":" + std::to_string(t.start) + "-" + std::to_string(t.end);
    t.name = nm;
    out.push_back(t);
  }
  return out;
}

void usage() {
  fprintf(stderr,
          "impg-gpu index -a <paf>... -i <file> [--unidirectional] [--order coitrees|sorted] [--device N]\n"
          "impg-gpu query (-a <paf>... | -i <file>) (-r seq:start-end | -b <bed>) (-d <bp> | --no-merge) [-x] [-m N]\n"
          "               [--transitive-dfs] [--multi-impg] [--min-transitive-len N] [--min-distance-between-ranges N]\n"
          "               [-l N] [--min-result-identity F] [--subset-sequence-list FILE] [--original-sequence-coordinates]\n"
          "               [--consider-strandness] [-o auto|bed|bedpe|paf|fasta] [--sequence-files F... | --sequence-list FILE]\n"
          "               [--reverse-complement] [--sequence-store bytes|packed|auto] [--sequence-ingest host|device] [--host-merge] [--unidirectional]\n"
          "               [--alignment-ingest host|device] [--resolve-matches]\n"
          "               [--order coitrees|sorted] [--device N]\n"
          "impg-gpu partition (-a <paf>... | -i <file>) -w <bp> -d <bp> [--min-missing-size N] [--min-boundary-distance N]\n"
          "               [--selection-mode longest|total|sample[,sep]|haplotype[,sep]] [--starting-sequences-file FILE]\n"
          "               [--separate-files] [--no-rehome-singletons] [--output-folder DIR] [-o bed|fasta] [--host-state] [-m N]\n"
          "               [--sequence-files F... | --sequence-list FILE] [--sequence-store bytes|packed|auto] [--reverse-complement]\n"
          "               [--sequence-ingest host|device] [--alignment-ingest host|device] [--resolve-matches]\n"
          "               [--transitive-dfs] [--min-transitive-len N] [--min-distance-between-ranges N] [--min-identity F]\n"
          "               [--unidirectional] [--order coitrees|sorted] [--device N]\n"
          "impg-gpu refine (-a <paf>... | -i <file>) (-r seq:start-end | -b <bed>) (-d <bp> | --no-merge) [--span-bp N]\n"
          "               [--max-extension F] [--extension-step N] [--pansn-mode sample|haplotype] [--support-output FILE]\n"
          "               [--blacklist-bed FILE] [-x] [-m N] [--transitive-dfs] [--multi-impg] [--min-transitive-len N]\n"
          "               [--min-distance-between-ranges N] [--min-result-identity F] [--subset-sequence-list FILE]\n"
          "               [--alignment-ingest host|device] [--resolve-matches --sequence-files F... | --sequence-list FILE]\n"
          "               [--unidirectional] [--order coitrees|sorted] [--device N]\n");
}

// --alignment-ingest host|device (query, partition, refine): who parses the alignment files' lines -- the host
// (impg_gpu_index_create_from_paf) or the device, the files streamed into HBM (impg_gpu_index_create_from_paf_streamed)
bool g_alignment_ingest_device = false;
bool alignment_ingest_arg(const std::string &a, int &i, int argc, char **argv) {
  if (a != "--alignment-ingest") return false;
  if (i + 1 >= argc) die("a value is required for '--alignment-ingest'", 2);
  const std::string sv = argv[++i];
  if (sv != "host" && sv != "device") die("invalid value '" + sv + "' for '--alignment-ingest'", 2);
  g_alignment_ingest_device = sv == "device";
  return true;
}
// --resolve-matches (query, partition, refine, wherever they build an index from -a): every 'M' op is rewritten as the
// '=' / 'X' runs the sequences of --sequence-files / --sequence-list spell before the index is built
// (impg_gpu_index_create_from_paf_resolved); under -v the report is one line on stderr
struct ResolveArgs {
  bool on = false;
  int verbose = 0;
  std::vector<std::string> files;
} g_resolve;
void read_sequence_list(const std::string &seq_list, std::vector<std::string> &seq_files) {  // one path per line (main.rs:4130-4145)
  std::ifstream in(seq_list);
  if (!in) die("No such file or directory: " + seq_list);
  std::string line;
  while (std::getline(in, line)) {
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
    if (!line.empty()) seq_files.push_back(line);
  }
}
// after the arguments are read: what --resolve-matches cannot go with, each with its reason
void resolve_check(const std::string &index_file, bool sequence_ingest_device, const std::vector<std::string> &seq_files, int verbose) {
  if (!g_resolve.on) return;
  if (!index_file.empty()) die("--resolve-matches rewrites the CIGARs while the index is built from -a: a saved index (-i) holds the ops as they were", 2);
  if (g_alignment_ingest_device) die("--resolve-matches sits behind the host's line parser: not with --alignment-ingest device", 2);
  if (sequence_ingest_device) die("--resolve-matches compares against the host's copy of the sequences: not with --sequence-ingest device", 2);
  if (seq_files.empty()) die("--resolve-matches needs the sequences: use --sequence-files or --sequence-list", 2);
  g_resolve.files = seq_files;
  g_resolve.verbose = verbose;
}
int create_from_paf(const std::vector<const char *> &pp, bool unidirectional, int order, int device, impg_gpu_index_t **ix) {
  if (g_resolve.on) {
    std::vector<const char *> sp;
    for (auto &f : g_resolve.files) sp.push_back(f.c_str());
    impg_gpu_sequences_t *seqs = nullptr;
    if (impg_gpu_sequences_from_fasta(sp.data(), sp.size(), &seqs) != IMPG_OK) return IMPG_E_INVALID;
    impg_gpu_resolve_report_t r;
    const int rc = impg_gpu_index_create_from_paf_resolved(pp.data(), (int)pp.size(), seqs, unidirectional ? 0 : 1, order, device, &r, nullptr, ix);
    impg_gpu_sequences_free(seqs);
    if (rc == IMPG_OK && g_resolve.verbose >= 1)
      fprintf(stderr, "[impg-gpu] resolve-matches: records %llu resolved %llu absent %llu inconsistent %llu ops %llu -> %llu; M ops %llu bases %llu = %llu X %llu; "
                      "bad = bases %llu bad X bases %llu\n",
              (unsigned long long)r.records, (unsigned long long)r.resolved, (unsigned long long)r.absent, (unsigned long long)r.inconsistent,
              (unsigned long long)r.ops_in, (unsigned long long)r.ops_out, (unsigned long long)r.m_ops, (unsigned long long)r.m_bases,
              (unsigned long long)r.m_eq_bases, (unsigned long long)r.m_x_bases, (unsigned long long)r.bad_eq_bases, (unsigned long long)r.bad_x_bases);
    return rc;
  }
  if (g_alignment_ingest_device) return impg_gpu_index_create_from_paf_streamed(pp.data(), (int)pp.size(), unidirectional ? 0 : 1, order, device, 0, ix);
  return impg_gpu_index_create_from_paf(pp.data(), (int)pp.size(), unidirectional ? 0 : 1, order, device, ix);
}

// the index of a command: the saved file if it exists, else built from the alignment files (and saved where -i names a file)
impg_gpu_index_t *open_index(const std::vector<std::string> &pafs, const std::string &index_file, bool unidirectional, int order, int device) {
  std::vector<const char *> pp;
  for (auto &p : pafs) pp.push_back(p.c_str());
  impg_gpu_index_t *ix = nullptr;
  FILE *probe = index_file.empty() ? nullptr : fopen(index_file.c_str(), "rb");
  if (probe) {
    fclose(probe);
    if (impg_gpu_index_load(index_file.c_str(), device, &ix) != IMPG_OK) die(impg_gpu_last_error());
  } else {
    if (pafs.empty()) die("No such file or directory: " + index_file);
    if (create_from_paf(pp, unidirectional, order, device, &ix) != IMPG_OK) die(impg_gpu_last_error());
    if (!index_file.empty() && impg_gpu_index_save(ix, index_file.c_str()) != IMPG_OK) die(impg_gpu_last_error());
  }
  return ix;
}

// load_subset_filter (subset_filter.rs:63-82) + one matches() per sequence
std::vector<uint8_t> load_subset_keep(impg_gpu_index_t *ix, const std::string &subset_list) {
  FILE *f = fopen(subset_list.c_str(), "rb");
  if (!f) die("Failed to read subset sequence list '" + subset_list + "'");
  std::string text;
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
  fclose(f);
  const uint32_t ns = impg_gpu_num_seqs(ix);
  std::vector<const char *> nm(ns);
  for (uint32_t i = 0; i < ns; i++) nm[i] = impg_gpu_seq_name(ix, i);
  std::vector<uint8_t> keep(ns);
  size_t entries = 0;
  if (impg_gpu_subset_keep(text.data(), text.size(), nm.data(), ns, keep.data(), &entries) != IMPG_OK) die(impg_gpu_last_error());
  if (entries == 0) die("Subset sequence list '" + subset_list + "' did not contain any sequence names");
  return keep;
}

// `impg partition` (reference src/main.rs partition arguments; src/commands/partition.rs:158-712) with BED output:
// partitions.bed (or partition{N}.bed with --separate-files) in --output-folder, as the reference writes them; or with
// FASTA output, partition{N}.fasta (--separate-files only, main.rs:6366-6376) from --sequence-files / --sequence-list.
int partition_main(int argc, char **argv) {
  std::vector<std::string> pafs;
  std::string index_file, ofmt = "bed", mode = "longest", starting, folder;
  long long window = -1, merge_d = 0, v = 0;
  bool have_d = false, no_merge = false, dfs = false, unidirectional = false, separate = false, rehome = true, host_state = false;
  std::vector<std::string> seq_files;
  std::string seq_list;
  int sequence_store = 0;
  bool ingest_device = false;  // --sequence-ingest device: impg_gpu_index_load_sequences instead of _from_fasta + _set_sequences
  int verbose = 0;
  long max_depth = 2, min_tl = -1, mdbr = 10, min_missing = 3000, min_boundary = 3000;
  double min_ident = NAN;
  int device = 0, order = IMPG_ORDER_COITREES;
  auto num = [](const std::string &flag, const char *x, long lo, long hi) -> long {
    char *end = nullptr;
    errno = 0;
    const long r = strtol(x, &end, 10);
    if (errno || end == x || *end != '\0' || r < lo || r > hi) die("invalid value '" + std::string(x) + "' for '" + flag + "'", 2);
    return r;
  };
  for (int i = 2; i < argc; i++) {
    std::string a = argv[i];
    auto need = [&](const char *f) -> const char * {
      if (i + 1 >= argc) die(std::string("a value is required for '") + f + "'", 2);
      return argv[++i];
    };
    if (a == "-a" || a == "--alignment-files") {
      pafs.push_back(need("-a"));
      while (i + 1 < argc && argv[i + 1][0] != '-') pafs.push_back(argv[++i]);
    } else if (a == "-i" || a == "--index") index_file = need("-i");
    else if (a == "-w" || a == "--window-size") {
      if (!parse_metric(need("-w"), &window) || window < 0 || window > 2147483647ll) die("invalid value for '-w'", 2);
    } else if (a == "-d" || a == "--merge-distance") {
      if (!parse_metric(need("-d"), &merge_d) || merge_d < 0 || merge_d > 2147483647ll) die("invalid value for '-d'", 2);
      have_d = true;
    } else if (a == "--no-merge") no_merge = true;
    else if (a == "--min-missing-size") { if (!parse_metric(need(a.c_str()), &v) || v < 0 || v > 2147483647ll) die("invalid value for '" + a + "'", 2); min_missing = (long)v; }
    else if (a == "--min-boundary-distance") { if (!parse_metric(need(a.c_str()), &v) || v < 0 || v > 2147483647ll) die("invalid value for '" + a + "'", 2); min_boundary = (long)v; }
    else if (a == "--selection-mode") mode = need(a.c_str());
    else if (a == "--starting-sequences-file") starting = need(a.c_str());
    else if (a == "--separate-files") separate = true;
    else if (a == "--no-rehome-singletons") rehome = false;
    else if (a == "--output-folder") folder = need(a.c_str());
    else if (a == "-o" || a == "--output-format") ofmt = need("-o");
    else if (a == "--host-state") host_state = true;
    else if (a == "--sequence-files") {
      seq_files.push_back(need(a.c_str()));
      while (i + 1 < argc && argv[i + 1][0] != '-') seq_files.push_back(argv[++i]);
    } else if (a == "--sequence-list") seq_list = need(a.c_str());
    else if (a == "--sequence-store") {  // the form the sequences take in HBM (option "sequence_store_packed"); --host-state prints from the host copy
      const std::string sv = need(a.c_str());
      if (sv != "bytes" && sv != "packed" && sv != "auto") die("invalid value '" + sv + "' for '--sequence-store'", 2);
      sequence_store = sv == "bytes" ? 0 : sv == "packed" ? 1 : 2;
    } else if (a == "--sequence-ingest") {  // host: parsed on the host and attached; device: streamed into HBM and parsed there (gzip / BGZF too)
      const std::string sv = need(a.c_str());
      if (sv != "host" && sv != "device") die("invalid value '" + sv + "' for '--sequence-ingest'", 2);
      ingest_device = sv == "device";
    } else if (a == "--reverse-complement") {}  // accepted as the reference accepts it: a partition's intervals are all forward
    else if (a == "--transitive-dfs") dfs = true;
    else if (a == "-m" || a == "--max-depth") max_depth = num(a, need("-m"), 0, 65535);
    else if (a == "--min-transitive-len") min_tl = num(a, need(a.c_str()), 0, 2147483647);
    else if (a == "--min-distance-between-ranges") mdbr = num(a, need(a.c_str()), 0, 2147483647);
    else if (a == "--min-identity") {
      char *end = nullptr;
      const char *x = need(a.c_str());
      min_ident = strtod(x, &end);
      if (end == x || *end || !(min_ident == min_ident)) die("invalid value '" + std::string(x) + "' for '" + a + "'", 2);
    } else if (a == "--unidirectional") unidirectional = true;
    else if (a == "--device") device = (int)num(a, need(a.c_str()), 0, 1023);
    else if (a == "--order") {
      std::string o = need("--order");
      if (o != "sorted" && o != "coitrees") die("invalid value '" + o + "' for '--order'", 2);
      order = o == "sorted" ? IMPG_ORDER_SORTED : IMPG_ORDER_COITREES;
    } else if (a == "-t" || a == "--threads") need(a.c_str());  // accepted, unused
    else if (a == "-v" || a == "--verbose") verbose = (int)num(a, need(a.c_str()), 0, 9);  // >= 1: the report of --resolve-matches on stderr
    else if (a == "--resolve-matches") g_resolve.on = true;
    else if (alignment_ingest_arg(a, i, argc, argv)) {}
    else if (a == "-h" || a == "--help") { usage(); return 0; }
    else die("unexpected argument '" + a + "'", 2);
  }
  if (pafs.empty() && index_file.empty()) die("the following required arguments were not provided: --alignment-files", 2);
  if (window < 0) die("the following required arguments were not provided: --window-size", 2);
  if (window == 0) die("--window-size must be greater than 0");
  if (!have_d && !no_merge) die("-d/--merge-distance is required. For `impg partition`, pass `-d <bp>`.");
  if (no_merge) die("--no-merge is not built in impg-gpu partition", 2);
  if (ofmt != "bed" && ofmt != "fasta") die("output format '" + ofmt + "' is not built in impg-gpu partition (bed, fasta)", 2);
  const bool fasta = ofmt == "fasta";
  if (fasta && !separate) die("Single-file output is only supported for BED format. Use --separate-files for FASTA format.");  // main.rs:6366-6376
  if (!seq_files.empty() && !seq_list.empty()) die("Cannot specify both --sequence-files and --sequence-list");
  if (!seq_list.empty()) {  // one path per line (main.rs:4130-4145)
    std::ifstream in(seq_list);
    if (!in) die("No such file or directory: " + seq_list);
    std::string line;
    while (std::getline(in, line)) {
      while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
      if (!line.empty()) seq_files.push_back(line);
    }
  }
  if (fasta && seq_files.empty()) die("FASTA index required for FASTA output");  // partition.rs:1640
  if (ingest_device && host_state && fasta) die("--sequence-ingest device keeps no host copy of the sequences: --host-state cannot print FASTA from it", 2);
  if (ingest_device && sequence_store == 2) die("--sequence-store auto needs the host's copy of the sequences: with --sequence-ingest device choose bytes or packed", 2);
  int selection = IMPG_SELECT_LONGEST;
  std::string kind = mode.substr(0, mode.find(',')), sep = mode.find(',') == std::string::npos ? "#" : mode.substr(mode.find(',') + 1);
  if (kind == "longest" && mode == kind) selection = IMPG_SELECT_LONGEST;
  else if (kind == "total" && mode == kind) selection = IMPG_SELECT_TOTAL;
  else if (kind == "sample") selection = IMPG_SELECT_SAMPLE;
  else if (kind == "haplotype") selection = IMPG_SELECT_HAPLOTYPE;
  else die("Invalid selection mode. Must be 'longest', 'total', 'sample[,sep]', or 'haplotype[,sep]'.");
  resolve_check(index_file, ingest_device, seq_files, verbose);
  impg_gpu_index_t *ix = open_index(pafs, index_file, unidirectional, order, device);
  std::vector<uint32_t> start_ids;
  if (!starting.empty()) {  // partition.rs:186-212: first tab field, trimmed; empty lines, '#' comments and unknown names skipped
    std::ifstream in(starting);
    if (!in) die("Could not open starting sequences file " + starting);
    std::string line;
    while (std::getline(in, line)) {
      std::string name = line.substr(0, line.find('\t'));
      const size_t b = name.find_first_not_of(" \t\r\n\v\f"), e = name.find_last_not_of(" \t\r\n\v\f");
      name = b == std::string::npos ? "" : name.substr(b, e - b + 1);
      if (name.empty() || name[0] == '#') continue;
      const long long id = impg_gpu_seq_id(ix, name.c_str());
      if (id >= 0) start_ids.push_back((uint32_t)id);
    }
  }
  impg_gpu_params_t p;
  memset(&p, 0, sizeof p);
  p.transitive = 1;
  p.dfs = dfs;
  p.max_depth = (uint32_t)max_depth;
  p.min_transitive_len = min_tl < 0 ? 101 : (int32_t)min_tl;
  p.min_distance_between_ranges = (int32_t)mdbr;
  p.min_output_length = -1;
  p.min_identity = min_ident;
  impg_gpu_partition_opts_t o;
  memset(&o, 0, sizeof o);
  o.window_size = window;
  o.merge_distance = (int32_t)merge_d;
  o.min_missing_size = (int32_t)min_missing;
  o.min_boundary_distance = (int32_t)min_boundary;
  o.selection = selection;
  o.separator = sep.c_str();
  o.rehome_singletons = rehome;
  o.state_on_host = host_state;
  if (fasta) {
    std::vector<const char *> sp;
    for (auto &f : seq_files) sp.push_back(f.c_str());
    if (impg_gpu_set_option(ix, "sequence_store_packed", sequence_store) != IMPG_OK) die(impg_gpu_last_error());
    if (ingest_device) {
      if (impg_gpu_index_load_sequences(ix, sp.data(), sp.size()) != IMPG_OK) die(impg_gpu_last_error());
    } else {
      impg_gpu_sequences_t *seqs = nullptr;
      if (impg_gpu_sequences_from_fasta(sp.data(), sp.size(), &seqs) != IMPG_OK) die(impg_gpu_last_error());
      if (impg_gpu_index_set_sequences(ix, seqs) != IMPG_OK) die(impg_gpu_last_error());
      impg_gpu_sequences_free(seqs);  // (the handle shares the store)
    }
  }
  impg_gpu_partition_t *ps = nullptr;
  if (impg_gpu_partition_create(ix, &p, &o, start_ids.data(), start_ids.size(), &ps) != IMPG_OK) die(impg_gpu_last_error());
  uint64_t n_parts = 0;
  if (fasta) {
    if (impg_gpu_partition_run_fasta(ps, folder.empty() ? nullptr : folder.c_str(), &n_parts) != IMPG_OK) die(impg_gpu_last_error());
  } else if (impg_gpu_partition_run(ps, folder.empty() ? nullptr : folder.c_str(), separate, nullptr, nullptr, &n_parts) != IMPG_OK) die(impg_gpu_last_error());
  fprintf(stderr, "[impg-gpu] partitioned into %llu regions\n", (unsigned long long)n_parts);
  impg_gpu_partition_destroy(ps);
  impg_gpu_index_destroy(ix);
  return 0;
}

// parse_blacklist_bed (reference src/commands/refine.rs:879-948) into the CSR table of impg_gpu_refine; a sequence the
// index does not know is never asked for and is left out
void parse_blacklist_bed(const std::string &path, impg_gpu_index_t *ix, std::vector<uint32_t> &off, std::vector<int32_t> &ranges) {
  std::ifstream in(path);
  if (!in) die("No such file or directory: " + path);
  const uint32_t ns = impg_gpu_num_seqs(ix);
  std::vector<std::vector<int32_t>> per(ns);
  std::string line;
  for (size_t line_num = 1; std::getline(in, line); line_num++) {
    const size_t a = line.find_first_not_of(" \t\r\n\v\f"), b = line.find_last_not_of(" \t\r\n\v\f");
    line = a == std::string::npos ? "" : line.substr(a, b - a + 1);
    if (line.empty() || line[0] == '#') continue;
    std::vector<std::string> parts;
    size_t st = 0;
    for (size_t i = 0; i <= line.size(); i++)
      if (i == line.size() || line[i] == '\t') { parts.push_back(line.substr(st, i - st)); st = i + 1; }
    if (parts.size() < 3) die("Line " + std::to_string(line_num) + " has fewer than 3 fields in BED file: " + path);
    int32_t s = 0, e = 0;
    if (!parse_i32(parts[1], &s)) die("Invalid start position on line " + std::to_string(line_num));
    if (!parse_i32(parts[2], &e)) die("Invalid end position on line " + std::to_string(line_num));
    if (e <= s) die("Invalid range on line " + std::to_string(line_num) + ": end (" + std::to_string(e) + ") <= start (" + std::to_string(s) + ")");
    const long long id = impg_gpu_seq_id(ix, parts[0].c_str());
    if (id >= 0) { per[(size_t)id].push_back(s); per[(size_t)id].push_back(e); }
  }
  off.assign((size_t)ns + 1, 0);
  ranges.clear();
  for (uint32_t q = 0; q < ns; q++) {
    ranges.insert(ranges.end(), per[q].begin(), per[q].end());
    off[q + 1] = (uint32_t)(ranges.size() / 2);
  }
}

// `impg refine` (reference src/main.rs:7700-7862, src/commands/refine.rs): the table on stdout, --support-output beside it
int refine_main(int argc, char **argv) {
  std::vector<std::string> pafs;
  std::string index_file, range, bed, pansn, support_out, blacklist_bed, subset_list;
  long long merge_d = 0;
  bool have_d = false, no_merge = false, transitive = false, dfs = false, multi = false, unidirectional = false;
  long max_depth = 2, min_tl = -1, mdbr = 10, span_bp = 1000, step = 1000;
  double min_ident = NAN, max_ext = 0.5;
  int device = 0, order = IMPG_ORDER_COITREES, verbose = 0;
  std::vector<std::string> seq_files;  // --sequence-files / --sequence-list: what --resolve-matches compares against
  std::string seq_list;
  auto num = [](const std::string &flag, const char *x, long lo, long hi) -> long {
    char *end = nullptr;
    errno = 0;
    const long r = strtol(x, &end, 10);
    if (errno || end == x || *end != '\0' || r < lo || r > hi) die("invalid value '" + std::string(x) + "' for '" + flag + "'", 2);
    return r;
  };
  auto real = [](const std::string &flag, const char *v) -> double {
    char *end = nullptr;
    errno = 0;
    const double x = strtod(v, &end);
    if (errno || end == v || *end != '\0' || !(x == x)) die("invalid value '" + std::string(v) + "' for '" + flag + "'", 2);
    return x;
  };
  for (int i = 2; i < argc; i++) {
    std::string a = argv[i];
    auto need = [&](const char *f) -> const char * {
      if (i + 1 >= argc) die(std::string("a value is required for '") + f + "'", 2);
      return argv[++i];
    };
    if (a == "-a" || a == "--alignment-files") {
      pafs.push_back(need("-a"));
      while (i + 1 < argc && argv[i + 1][0] != '-') pafs.push_back(argv[++i]);
    } else if (a == "-i" || a == "--index") index_file = need("-i");
    else if (a == "-r" || a == "--target-range") range = need("-r");
    else if (a == "-b" || a == "--target-bed") bed = need("-b");
    else if (a == "-d" || a == "--merge-distance") {
      if (!parse_metric(need("-d"), &merge_d) || merge_d < 0 || merge_d > 2147483647ll) die("invalid value for '-d'", 2);
      have_d = true;
    } else if (a == "--no-merge") no_merge = true;
    else if (a == "--span-bp") span_bp = num(a, need(a.c_str()), -2147483647 - 1, 2147483647);
    else if (a == "--max-extension") max_ext = real(a, need(a.c_str()));
    else if (a == "--extension-step") step = num(a, need(a.c_str()), -2147483647 - 1, 2147483647);
    else if (a == "--pansn-mode") pansn = need(a.c_str());
    else if (a == "--support-output") support_out = need(a.c_str());
    else if (a == "--blacklist-bed") blacklist_bed = need(a.c_str());
    else if (a == "-x" || a == "--transitive") transitive = true;
    else if (a == "--transitive-dfs") dfs = true;
    else if (a == "--multi-impg") multi = true;
    else if (a == "-m" || a == "--max-depth") max_depth = num(a, need("-m"), 0, 65535);
    else if (a == "--min-transitive-len") min_tl = num(a, need(a.c_str()), 0, 2147483647);
    else if (a == "--min-distance-between-ranges") mdbr = num(a, need(a.c_str()), 0, 2147483647);
    else if (a == "--min-result-identity") min_ident = real(a, need(a.c_str()));
    else if (a == "--subset-sequence-list") subset_list = need(a.c_str());
    else if (a == "--unidirectional") unidirectional = true;
    else if (a == "--device") device = (int)num(a, need(a.c_str()), 0, 1023);
    else if (a == "--order") {
      std::string o = need("--order");
      if (o != "sorted" && o != "coitrees") die("invalid value '" + o + "' for '--order'", 2);
      order = o == "sorted" ? IMPG_ORDER_SORTED : IMPG_ORDER_COITREES;
    } else if (a == "-t" || a == "--threads") need(a.c_str());  // accepted, unused
    else if (a == "-v" || a == "--verbose") verbose = (int)num(a, need(a.c_str()), 0, 9);  // >= 1: the report of --resolve-matches on stderr
    else if (a == "--resolve-matches") g_resolve.on = true;
    else if (a == "--sequence-files") {  // (read by --resolve-matches alone: refine prints no bases)
      seq_files.push_back(need(a.c_str()));
      while (i + 1 < argc && argv[i + 1][0] != '-') seq_files.push_back(argv[++i]);
    } else if (a == "--sequence-list") seq_list = need(a.c_str());
    else if (alignment_ingest_arg(a, i, argc, argv)) {}
    else if (a == "-h" || a == "--help") { usage(); return 0; }
    else die("unexpected argument '" + a + "'", 2);
  }
  // RefineOpts::validate (main.rs:4454-4473), validate_merge_distance
  if (span_bp < 0) die("--span-bp must be >= 0");
  if (max_ext < 0.0) die("--max-extension must be >= 0");
  if (step <= 0) die("--extension-step must be > 0");
  if (!have_d && !no_merge)
    die("-d/--merge-distance is required. For `impg refine`, pass `-d <bp>`. Use `--no-merge` to explicitly disable merging.");
  if (!pansn.empty() && pansn != "sample" && pansn != "haplotype" && pansn != "sequence") die("invalid value '" + pansn + "' for '--pansn-mode'", 2);
  if (pafs.empty() && index_file.empty()) die("the following required arguments were not provided: --alignment-files", 2);
  if (range.empty() && bed.empty()) die("Either --target-range or --target-bed must be provided");
  if (!seq_files.empty() && !seq_list.empty()) die("Cannot specify both --sequence-files and --sequence-list");
  if (!seq_list.empty()) read_sequence_list(seq_list, seq_files);
  resolve_check(index_file, false, seq_files, verbose);
  impg_gpu_index_t *ix = open_index(pafs, index_file, unidirectional, order, device);
  std::vector<uint8_t> keep;
  if (!subset_list.empty()) keep = load_subset_keep(ix, subset_list);
  std::vector<Target> targets;
  if (!range.empty()) {
    char name[4096];
    int32_t s, e;
    if (impg_gpu_parse_target_range(range.c_str(), name, sizeof name, &s, &e) != IMPG_OK) die(impg_gpu_last_error());
    targets.push_back({name, std::string(name) + ":" + std::to_string(s) + "-" + std::to_string(e), s, e});
  } else targets = parse_bed_file(bed);
  const int32_t eff_min_tl = min_tl < 0 ? 101 : (int32_t)min_tl;
  std::vector<impg_gpu_range_t> loci;
  std::vector<const char *> labels;
  for (auto &t : targets) {  // validate_sequence_range, validate_range_min_length (main.rs:7732-7755)
    const long long id = impg_gpu_seq_id(ix, t.seq.c_str());
    if (id < 0) die("Sequence '" + t.seq + "' not found in index");
    const long long len = impg_gpu_seq_len(ix, (uint32_t)id);
    if (t.start < 0) die("Start position " + std::to_string(t.start) + " cannot be negative");
    if (t.end < 0) die("End position " + std::to_string(t.end) + " cannot be negative");
    if (t.start >= t.end) die("Start position must be less than end position");
    if (t.end > len) die("End position " + std::to_string(t.end) + " exceeds sequence length " + std::to_string(len));
    if (t.end - t.start < eff_min_tl)
      die("Range '" + t.name + "' (" + std::to_string(t.end - t.start) + " bp) is below minimum of " + std::to_string(eff_min_tl) +
          " bp. Lower --min-transitive-len or use a longer range");
    loci.push_back({(uint32_t)id, t.start, t.end});
    labels.push_back(t.name.c_str());
  }
  std::vector<uint32_t> bl_off;
  std::vector<int32_t> bl_rng;
  if (!blacklist_bed.empty()) parse_blacklist_bed(blacklist_bed, ix, bl_off, bl_rng);
  const uint32_t ns = impg_gpu_num_seqs(ix);
  std::vector<const char *> nm(ns);
  for (uint32_t i = 0; i < ns; i++) nm[i] = impg_gpu_seq_name(ix, i);
  const bool by_entity = pansn == "sample" || pansn == "haplotype";
  std::vector<uint32_t> ent(ns);
  if (by_entity && impg_gpu_entity_ids(nm.data(), ns, pansn == "sample" ? IMPG_SELECT_SAMPLE : IMPG_SELECT_HAPLOTYPE, "#", ent.data(), nullptr) != IMPG_OK)
    die(impg_gpu_last_error());
  impg_gpu_params_t p;
  memset(&p, 0, sizeof p);
  p.transitive = transitive || dfs;
  p.dfs = dfs;
  p.multi_impg = multi;
  p.max_depth = (uint32_t)max_depth;
  p.min_transitive_len = eff_min_tl;
  p.min_distance_between_ranges = (int32_t)mdbr;
  p.min_output_length = -1;
  p.min_identity = min_ident;
  impg_gpu_refine_opts_t o;
  memset(&o, 0, sizeof o);
  o.span_bp = (int32_t)span_bp;
  o.max_extension = max_ext;
  o.extension_step = (int32_t)step;
  o.merge_distance = no_merge ? -1 : (int32_t)merge_d;
  o.use_max_entities = by_entity;
  impg_gpu_refine_t *res = nullptr;
  if (impg_gpu_refine(ix, loci.data(), loci.size(), &p, &o, by_entity ? ent.data() : nullptr, keep.empty() ? nullptr : keep.data(),
                      bl_off.empty() ? nullptr : bl_off.data(), bl_rng.data(), &res) != IMPG_OK)
    die(impg_gpu_last_error());
  char *text = nullptr, *sup = nullptr;
  size_t len = 0, sup_len = 0;
  if (impg_gpu_refine_text(res, nm.data(), ns, labels.data(), &text, &len, &sup, &sup_len) != IMPG_OK) die(impg_gpu_last_error());
  fwrite(text, 1, len, stdout);
  fflush(stdout);
  if (!support_out.empty()) {
    FILE *f = fopen(support_out.c_str(), "wb");
    if (!f) die("could not create " + support_out);
    fwrite(sup, 1, sup_len, f);
    fclose(f);
  }
  free(text);
  free(sup);
  impg_gpu_refine_free(res);
  impg_gpu_index_destroy(ix);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc >= 2 && strcmp(argv[1], "partition") == 0) return partition_main(argc, argv);
  if (argc >= 2 && strcmp(argv[1], "refine") == 0) return refine_main(argc, argv);
  if (argc < 2 || (strcmp(argv[1], "query") != 0 && strcmp(argv[1], "index") != 0)) {
    usage();
    return 2;
  }
  const bool index_only = strcmp(argv[1], "index") == 0;
  std::string index_file;  // -i: a saved index (impg_gpu_index_save), read if it exists, else written after the build
  std::vector<std::string> pafs;
  std::string range, bed, ofmt = "auto";
  bool have_d = false, no_merge = false, transitive = false, dfs = false, unidirectional = false, multi = false;
  long long merge_d = 0;
  long max_depth = 2, min_tl = -1, mdbr = 10, min_out = -1;
  double min_ident = NAN;
  int verbose = 0;
  bool original_coords = false;  // main.rs:4370
  std::string subset_list;  // --subset-sequence-list: a file of sequence names (main.rs:4357, :11709-11720)
  int device = 0, order = IMPG_ORDER_COITREES;
  // numeric options are parsed whole or refused, as clap does for the reference (a typo must not become 0 = "unlimited")
  auto num = [](const std::string &flag, const char *v, long lo, long hi) -> long {
    char *end = nullptr;
    errno = 0;
    const long x = strtol(v, &end, 10);
    if (errno || end == v || *end != '\0' || x < lo || x > hi) die("invalid value '" + std::string(v) + "' for '" + flag + "'", 2);
    return x;
  };
  auto real = [](const std::string &flag, const char *v) -> double {
    char *end = nullptr;
    errno = 0;
    const double x = strtod(v, &end);
    if (errno || end == v || *end != '\0' || !(x == x)) die("invalid value '" + std::string(v) + "' for '" + flag + "'", 2);
    return x;
  };
  bool consider_strandness = false;  // main.rs:4380
  bool host_merge = false;
  std::vector<std::string> seq_files;  // --sequence-files / --sequence-list (main.rs:4116-4121): what -o fasta prints from
  std::string seq_list;
  bool reverse_complement = false;
  int sequence_store = 0;
  bool ingest_device = false;  // --sequence-ingest device: impg_gpu_index_load_sequences instead of _from_fasta + _set_sequences
  for (int i = 2; i < argc; i++) {
    std::string a = argv[i];
    auto need = [&](const char *f) -> const char * {
      if (i + 1 >= argc) die(std::string("a value is required for '") + f + "'", 2);
      return argv[++i];
    };
    if (a == "-a" || a == "--alignment-files") {
      pafs.push_back(need("-a"));
      while (i + 1 < argc && argv[i + 1][0] != '-') pafs.push_back(argv[++i]);
    } else if (a == "-r" || a == "--target-range") range = need("-r");
    else if (a == "-b" || a == "--target-bed") bed = need("-b");
    else if (a == "-d" || a == "--merge-distance") {
      if (!parse_metric(need("-d"), &merge_d) || merge_d < 0 || merge_d > 2147483647ll) die("invalid value for '-d'", 2);
      have_d = true;
    } else if (a == "--no-merge") no_merge = true;
    else if (a == "-x" || a == "--transitive") transitive = true;
    else if (a == "--transitive-dfs") dfs = true;
    else if (a == "--multi-impg") multi = true;  // per-file indices (the reference's MultiImpg, src/multi_impg.rs)
    else if (a == "-m" || a == "--max-depth") max_depth = num(a, need("-m"), 0, 65535);           // u16 (main.rs:4263)
    else if (a == "--min-transitive-len") min_tl = num(a, need(a.c_str()), 0, 2147483647);
    else if (a == "--min-distance-between-ranges") mdbr = num(a, need(a.c_str()), 0, 2147483647);
    else if (a == "-l" || a == "--min-output-length") min_out = num(a, need("-l"), 0, 2147483647);
    else if (a == "--min-result-identity") min_ident = real(a, need(a.c_str()));
    else if (a == "--consider-strandness") consider_strandness = true;
    else if (a == "--host-merge") host_merge = true;  // BED / BEDPE / PAF / FASTA merges and text on the host (impg_gpu_results_bed / _paf / _fasta) instead of the device
    else if (a == "--sequence-files") {
      seq_files.push_back(need(a.c_str()));
      while (i + 1 < argc && argv[i + 1][0] != '-') seq_files.push_back(argv[++i]);
    } else if (a == "--sequence-list") seq_list = need(a.c_str());
    else if (a == "--reverse-complement") reverse_complement = true;
    else if (a == "--sequence-store") {  // the form the sequences take in HBM (option "sequence_store_packed"); --host-merge prints from the host copy
      const std::string v = need(a.c_str());
      if (v != "bytes" && v != "packed" && v != "auto") die("invalid value '" + v + "' for '--sequence-store'", 2);
      sequence_store = v == "bytes" ? 0 : v == "packed" ? 1 : 2;
    }
    else if (a == "--sequence-ingest") {  // host: parsed on the host and attached; device: streamed into HBM and parsed there (gzip / BGZF too)
      const std::string v = need(a.c_str());
      if (v != "host" && v != "device") die("invalid value '" + v + "' for '--sequence-ingest'", 2);
      ingest_device = v == "device";
    }
    else if (a == "--subset-sequence-list") subset_list = need(a.c_str());
    else if (a == "--original-sequence-coordinates") original_coords = true;
    else if (a == "-o" || a == "--output-format") ofmt = need("-o");
    else if (a == "--unidirectional") unidirectional = true;
    else if (a == "--device") device = (int)num(a, need(a.c_str()), 0, 1023);
    else if (a == "--order") {
      std::string o = need("--order");
      if (o != "sorted" && o != "coitrees") die("invalid value '" + o + "' for '--order'", 2);
      order = o == "sorted" ? IMPG_ORDER_SORTED : IMPG_ORDER_COITREES;
    }
    else if (a == "-i" || a == "--index") index_file = need("-i");
    else if (a == "-v" || a == "--verbose") verbose = (int)num(a, need(a.c_str()), 0, 9);  // >= 1: phase timings on stderr
    else if (a == "-t" || a == "--threads") need(a.c_str());  // accepted, unused
    else if (a == "--resolve-matches") g_resolve.on = true;
    else if (alignment_ingest_arg(a, i, argc, argv)) {}
    else if (a == "-h" || a == "--help") { usage(); return 0; }
    else die("unexpected argument '" + a + "'", 2);
  }
  auto file_exists = [](const std::string &p) { FILE *f = fopen(p.c_str(), "rb"); if (f) fclose(f); return f != nullptr; };
  if (index_only) {  // `impg index` (main.rs:11321-11386): build once, keep the result
    if (pafs.empty() || index_file.empty()) die("impg-gpu index needs --alignment-files and --index", 2);
    if (g_resolve.on) die("--resolve-matches belongs to query, partition and refine: a saved index holds the ops as they were", 2);
    std::vector<const char *> pp;
    for (auto &p : pafs) pp.push_back(p.c_str());
    impg_gpu_index_t *ix = nullptr;
    if (create_from_paf(pp, unidirectional, order, device, &ix) != IMPG_OK)
      die(impg_gpu_last_error());
    if (impg_gpu_index_save(ix, index_file.c_str()) != IMPG_OK) die(impg_gpu_last_error());
    impg_gpu_index_destroy(ix);
    return 0;
  }
  const bool load_saved = !index_file.empty() && file_exists(index_file);
  if (pafs.empty() && !load_saved) die("the following required arguments were not provided: --alignment-files", 2);
  if (range.empty() == bed.empty()) die("exactly one of --target-range and --target-bed is required", 2);
  if (!have_d && !no_merge)  // MERGE_DISTANCE_REQUIRED_TEXT (main.rs:4288-4315)
    die("-d/--merge-distance is required. For `impg query`, pass `-d <bp>`. Use `--no-merge` to explicitly disable merging.");
  const int32_t merge_distance = no_merge ? -1 : (int32_t)merge_d;
  // -o auto: bed for -r, bedpe for -b (main.rs:7365-7373)
  std::string fmt = ofmt == "auto" ? (bed.empty() ? "bed" : "bedpe") : ofmt;
  if (fmt != "bed" && fmt != "bedpe" && fmt != "paf" && fmt != "fasta")
    die("output format '" + fmt + "' is not built in impg-gpu (bed, bedpe, paf, fasta)");
  if (!seq_files.empty() && !seq_list.empty()) die("Cannot specify both --sequence-files and --sequence-list");
  if (!seq_list.empty()) {  // one path per line (main.rs:4130-4145)
    std::ifstream in(seq_list);
    if (!in) die("No such file or directory: " + seq_list);
    std::string line;
    while (std::getline(in, line)) {
      while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
      if (!line.empty()) seq_files.push_back(line);
    }
  }
  if (ingest_device && host_merge) die("--sequence-ingest device keeps no host copy of the sequences: --host-merge cannot print from it", 2);
  if (ingest_device && sequence_store == 2) die("--sequence-store auto needs the host's copy of the sequences: with --sequence-ingest device choose bytes or packed", 2);
  if (fmt == "fasta" && seq_files.empty())  // main.rs:4243
    die("Sequence files (FASTA/AGC) are required for 'fasta' output format. Use --sequence-files or --sequence-list");
  resolve_check(index_file, ingest_device, seq_files, verbose);

  std::vector<const char *> pp;
  for (auto &p : pafs) pp.push_back(p.c_str());
  impg_gpu_index_t *ix = nullptr;
  bool loaded = false;
  bool reference_index = false;  // -i names the reference's own IMPGIDX2 / IMPGIDX1 file: read it, never overwrite it
  if (load_saved) {
    char magic[8] = {0};
    if (FILE *mf = fopen(index_file.c_str(), "rb")) { (void)!fread(magic, 1, 8, mf); fclose(mf); }
    reference_index = memcmp(magic, "IMPGIDX", 7) == 0;
  }
  if (load_saved && reference_index) {
    if (pafs.empty()) die("an IMPG index file stores offsets into its alignment files: pass them with -a, in the order it was built with");
    if (impg_gpu_index_load_impg(index_file.c_str(), pp.data(), (int)pp.size(), order, device, &ix) != IMPG_OK) die(impg_gpu_last_error());
    loaded = true;
  } else if (load_saved) {
    if (impg_gpu_index_load(index_file.c_str(), device, &ix) == IMPG_OK) loaded = true;
    else if (pafs.empty()) die(impg_gpu_last_error());
    else fprintf(stderr, "[impg-gpu] %s: %s -- rebuilding it from the alignment files\n", index_file.c_str(), impg_gpu_last_error());
  }
  if (!loaded) {
    if (create_from_paf(pp, unidirectional, order, device, &ix) != IMPG_OK)
      die(impg_gpu_last_error());
    if (!index_file.empty() && impg_gpu_index_save(ix, index_file.c_str()) != IMPG_OK) die(impg_gpu_last_error());
  }

  if (fmt == "fasta") {
    std::vector<const char *> sp;
    for (auto &f : seq_files) sp.push_back(f.c_str());
    if (impg_gpu_set_option(ix, "sequence_store_packed", sequence_store) != IMPG_OK) die(impg_gpu_last_error());
    if (ingest_device) {
      if (impg_gpu_index_load_sequences(ix, sp.data(), sp.size()) != IMPG_OK) die(impg_gpu_last_error());
    } else {
      impg_gpu_sequences_t *seqs = nullptr;
      if (impg_gpu_sequences_from_fasta(sp.data(), sp.size(), &seqs) != IMPG_OK) die(impg_gpu_last_error());
      if (impg_gpu_index_set_sequences(ix, seqs) != IMPG_OK) die(impg_gpu_last_error());
      impg_gpu_sequences_free(seqs);  // (the handle shares the store)
    }
  }

  std::vector<Target> targets;
  if (!range.empty()) {
    char name[4096];
    int32_t s, e;
    if (range.find(':') == std::string::npos) {  // no interval: the whole sequence [0, len) (main.rs:7290-7310)
      const long long id = impg_gpu_seq_id(ix, range.c_str());
      if (id < 0) die("Sequence '" + range + "' not found in index");
      const long long len = impg_gpu_seq_len(ix, (uint32_t)id);
      targets.push_back({range, range + ":0-" + std::to_string(len), 0, (int32_t)len});
    } else {
      if (impg_gpu_parse_target_range(range.c_str(), name, sizeof name, &s, &e) != IMPG_OK) die(impg_gpu_last_error());
      targets.push_back({name, std::string(name) + ":" + std::to_string(s) + "-" + std::to_string(e), s, e});
    }
  } else {
    targets = parse_bed_file(bed);
  }
  const int32_t eff_min_tl = min_tl < 0 ? 101 : (int32_t)min_tl;  // effective_min_transitive_len (main.rs:4283)
  std::vector<impg_gpu_range_t> ranges;
  std::vector<const char *> names;
  for (auto &t : targets) {
    // validate_sequence_range (main.rs:10458-10520), validate_range_min_length (:10387-10403), perform_query bound (:11632)
    long long id = impg_gpu_seq_id(ix, t.seq.c_str());
    if (id < 0) die("Sequence '" + t.seq + "' not found in index");
    long long len = impg_gpu_seq_len(ix, (uint32_t)id);
    if (t.start < 0) die("Start position " + std::to_string(t.start) + " cannot be negative");
    if (t.end < 0) die("End position " + std::to_string(t.end) + " cannot be negative");
    if (t.start >= t.end) die("Start position must be less than end position");
    if (t.end > len) die("End position " + std::to_string(t.end) + " exceeds sequence length " + std::to_string(len));
    if (t.end - t.start < eff_min_tl)
      die("Range '" + t.name + "' (" + std::to_string(t.end - t.start) + " bp) is below minimum of " +
          std::to_string(eff_min_tl) + " bp. Lower --min-transitive-len or use a longer range");
    ranges.push_back({(uint32_t)id, t.start, t.end});
    names.push_back(t.name.c_str());
  }
  impg_gpu_params_t p;
  memset(&p, 0, sizeof p);
  p.transitive = transitive || dfs;  // --transitive-dfs implies a transitive query
  p.dfs = dfs;
  p.multi_impg = multi;
  p.max_depth = (uint32_t)max_depth;
  p.min_transitive_len = eff_min_tl;
  p.min_distance_between_ranges = (int32_t)mdbr;
  p.min_output_length = min_out < 0 ? -1 : (int32_t)min_out;
  p.min_identity = min_ident;
  p.store_cigar = fmt != "bed" && fmt != "fasta";  // CIGARs for PAF / BEDPE only (main.rs:7447)
  p.original_sequence_coordinates = original_coords;
  p.consider_strandness = consider_strandness;
  impg_gpu_results_t *res = nullptr;
  std::vector<uint8_t> keep;
  if (!subset_list.empty()) keep = load_subset_keep(ix, subset_list);
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = now();
  // BED and BEDPE: the merge and the text on the device, only text crosses PCIe.  An index the device BEDPE route does
  // not serve (a sequence of 2^29 bases or more) says so to an empty batch, before anything is printed: the host route takes it.
  // PAF goes the same way: the merged CIGARs are fused and printed as cg:Z on the device (a tracepoint index is refused there as on the host).
  // FASTA: the records are written on the device from the sequences in HBM (range names play no part in them).
  const int rc_flag = reverse_complement ? 1 : 0;
  typedef std::function<int(impg_gpu_index_t *, const impg_gpu_range_t *, size_t, const impg_gpu_params_t *, const uint8_t *, int32_t, const char *const *, int,
                            uint64_t *, double *)> TextEntry;
  const TextEntry device_entry =
      fmt == "bed" ? TextEntry(impg_gpu_query_batch_bed_fd) : fmt == "bedpe" ? TextEntry(impg_gpu_query_batch_bedpe_fd) : fmt == "paf" ? TextEntry(impg_gpu_query_batch_paf_fd)
      : TextEntry([rc_flag](impg_gpu_index_t *x, const impg_gpu_range_t *r, size_t n, const impg_gpu_params_t *pp, const uint8_t *k, int32_t d,
                            const char *const *nm, int fd, uint64_t *w, double *s3) { return impg_gpu_query_batch_fasta_fd(x, r, n, pp, k, d, nm, rc_flag, fd, w, s3); });
  const bool device_route = !host_merge && (fmt == "bed" || device_entry(ix, nullptr, 0, &p, nullptr, merge_distance, nullptr, fileno(stdout), nullptr, nullptr) == IMPG_OK);
  if (device_route) {
    uint64_t len = 0;
    double sec[3] = {0, 0, 0};
    fflush(stdout);
    if (device_entry(ix, ranges.data(), ranges.size(), &p, keep.empty() ? nullptr : keep.data(), merge_distance, names.data(), fileno(stdout), &len, sec) != IMPG_OK)
      die(impg_gpu_last_error());
    const double t1 = now();
    if (verbose >= 1)
      fprintf(stderr, "[impg-gpu] query + merge + text + write %.2f s (engine %.2f, device merge %.2f, device text + copy + write %.2f), %llu bytes\n",
              t1 - t0, sec[0], sec[1], sec[2], (unsigned long long)len);
    _exit(0);  // (tearing down gigabytes of host buffers and the device context is not worth a second)
  }
  if (impg_gpu_query_batch_filtered(ix, ranges.data(), ranges.size(), &p, nullptr, keep.empty() ? nullptr : keep.data(), &res) != IMPG_OK)
    die(impg_gpu_last_error());
  const double t1 = now();
  char *text = nullptr;
  size_t len = 0;
  const int rc = fmt == "bed" ? impg_gpu_results_bed(res, ix, names.data(), &p, merge_distance, &text, &len)
                 : fmt == "fasta" ? impg_gpu_results_fasta(res, ix, &p, merge_distance, rc_flag, &text, &len)
                              : impg_gpu_results_paf(res, ix, names.data(), &p, merge_distance,
                                                     fmt == "paf" ? IMPG_OUT_PAF : IMPG_OUT_BEDPE, &text, &len);
  if (rc != IMPG_OK) die(impg_gpu_last_error());
  const double t2 = now();
  fwrite(text, 1, len, stdout);
  fflush(stdout);
  if (verbose >= 1) {
    double eng = 0, asm_s = 0;
    impg_gpu_results_timing(res, &eng, &asm_s);
    fprintf(stderr, "[impg-gpu] query %.2f s (engine %.2f, result assembly %.2f), merge + text %.2f s, write %.2f s, %zu intervals, %zu bytes\n",
            t1 - t0, eng, asm_s, t2 - t1, now() - t2, impg_gpu_results_total(res), len);
  }
  free(text);
  impg_gpu_results_free(res);
  impg_gpu_index_destroy(ix);
  return 0;
}
