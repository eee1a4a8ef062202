// `impg partition` on the host (reference src/commands/partition.rs): the host twin of partition_device.hip -- the same
// state and the same algebra, written the way the reference writes them, sequence by sequence -- plus what is host work
// in the reference as well: window generation, the sample / haplotype grouping of names, rehome_singleton_slivers and
// the text writers.  The session (impg_gpu_partition_*) drives either twin.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <map>
#include <new>
#include <unordered_set>

#include "partition.hpp"
#include "text_device.hpp"

namespace impg {
void set_error(const std::string &msg);

// ---- SortedRanges::insert at min_distance 0 (impg.rs:270-353): overlapping and touching ranges are merged ------------
static void sr_insert(std::vector<std::pair<int32_t, int32_t>> &r, int32_t start, int32_t end) {
  if (start > end) std::swap(start, end);
  size_t pos = std::lower_bound(r.begin(), r.end(), start, [](const std::pair<int32_t, int32_t> &a, int32_t s) { return a.first < s; }) - r.begin();
  size_t at;
  if (pos > 0 && r[pos - 1].second >= start) {
    r[pos - 1].second = std::max(r[pos - 1].second, end);
    at = pos - 1;
  } else if (pos < r.size() && end >= r[pos].first) {
    r[pos].first = std::min(start, r[pos].first);
    r[pos].second = std::max(end, r[pos].second);
    at = pos;
  } else {
    r.insert(r.begin() + pos, {start, end});
    return;
  }
  size_t write = at, read = at + 1;  // merge_forward_from (:355-368)
  while (read < r.size() && r[write].second >= r[read].first) {
    r[write].second = std::max(r[write].second, r[read].second);
    read++;
  }
  r.erase(r.begin() + write + 1, r.begin() + read);
}
// first range that can overlap a position: binary_search_by_key + the look at the previous range (:1010-1028)
static size_t first_relevant(const std::vector<std::pair<int32_t, int32_t>> &r, int32_t p) {
  size_t pos = std::lower_bound(r.begin(), r.end(), p, [](const std::pair<int32_t, int32_t> &a, int32_t s) { return a.first < s; }) - r.begin();
  if (pos < r.size() && r[pos].first == p) return pos;
  if (pos > 0 && r[pos - 1].second > p) return pos - 1;
  return pos;
}

HostRegions::HostRegions(const int64_t *seq_len, uint32_t n_seq) : len(n_seq), masked(n_seq), missing(n_seq) {
  for (uint32_t s = 0; s < n_seq; s++) {
    len[s] = (int32_t)std::min<int64_t>(std::max<int64_t>(seq_len[s], 0), INT32_MAX);
    if (len[s] > 0) missing[s].push_back({0, len[s]});
  }
}

// merge_overlaps (:939-976) on rows sorted by (seq, lo)
static void merge_sorted(std::vector<PIv> &v, int32_t d) {
  if (v.size() <= 1) return;
  std::stable_sort(v.begin(), v.end(), [](const PIv &a, const PIv &b) { return a.seq != b.seq ? a.seq < b.seq : a.lo < b.lo; });
  size_t w = 0;
  for (size_t r = 1; r < v.size(); r++) {
    if (v[w].seq != v[r].seq || (int64_t)v[r].lo > (int64_t)v[w].hi + d) v[++w] = v[r];
    else { v[w].lo = std::min(v[w].lo, v[r].lo); v[w].hi = std::max(v[w].hi, v[r].hi); }
  }
  v.resize(w + 1);
}

void HostRegions::apply(const impg_gpu_interval_t *rows, size_t n, int32_t d, int32_t min_missing, int32_t min_boundary, std::vector<PIv> &out) {
  out.clear();
  std::vector<PIv> v(n);
  for (size_t i = 0; i < n; i++) {
    const impg_gpu_interval_t &r = rows[i];
    if (r.query_id >= len.size()) throw Error{IMPG_E_INVALID, "row names an unknown sequence id"};
    if (std::min(r.q_first, r.q_last) < 0) throw Error{IMPG_E_INVALID, "row with a negative coordinate"};
    v[i] = PIv{r.query_id, std::min(r.q_first, r.q_last), std::max(r.q_first, r.q_last)};
  }
  merge_sorted(v, d);
  if (min_boundary > 0)  // extend_to_close_boundaries (:1369-1408)
    for (PIv &x : v) {
      if (x.lo < min_boundary) x.lo = 0;
      if (len[x.seq] - x.hi < min_boundary) x.hi = len[x.seq];
    }
  // mask_and_update_regions (:978-1366), one run of equal sequence ids at a time
  std::vector<std::pair<int32_t, int32_t>> ext, buf;
  for (size_t b = 0; b < v.size();) {
    size_t e = b;
    while (e < v.size() && v[e].seq == v[b].seq) e++;
    const uint32_t s = v[b].seq;
    auto &miss = missing[s];
    auto &mask = masked[s];
    ext.clear();
    if (!miss.empty())
      for (size_t i = b; i < e; i++) {  // step 1: fragments of the missing set shorter than min_missing at either end
        const int32_t ms = v[i].lo, me = v[i].hi;
        for (size_t k = first_relevant(miss, ms); k < miss.size(); k++) {
          const int32_t a = miss[k].first, z = miss[k].second;
          if (a > me) break;
          if (ms > a && ms < z && ms - a < min_missing && ms - a > 0) ext.push_back({a, ms});
          if (me > a && me < z && z - me < min_missing && z - me > 0) ext.push_back({me, z});
        }
      }
    if (!ext.empty()) {  // step 2
      std::stable_sort(ext.begin(), ext.end(), [](const std::pair<int32_t, int32_t> &a, const std::pair<int32_t, int32_t> &b2) { return a.first < b2.first; });
      size_t w = 0;
      for (size_t r = 1; r < ext.size(); r++) {
        if (ext[r].first <= ext[w].second) ext[w].second = std::max(ext[w].second, ext[r].second);
        else ext[++w] = ext[r];
      }
      ext.resize(w + 1);
    }
    buf.clear();
    for (size_t i = b; i < e; i++) {  // step 3
      int32_t start = v[i].lo, end = v[i].hi;
      for (const auto &x : ext)
        if ((x.second >= start && x.first <= start) || (x.first <= end && x.second >= end)) {
          if (x.first < start) start = x.first;
          if (x.second > end) end = x.second;
        }
      buf.push_back({start, end});
      int32_t cur = start;  // the masks as they were before this window
      for (size_t k = first_relevant(mask, cur); k < mask.size(); k++) {
        const int32_t a = mask[k].first, z = mask[k].second;
        if (a > end) break;
        if (z <= cur) continue;
        if (cur < a) out.push_back(PIv{s, cur, a});
        cur = std::max(cur, z);
        if (cur >= end) break;
      }
      if (cur < end) out.push_back(PIv{s, cur, end});
    }
    for (const auto &x : buf) sr_insert(mask, x.first, x.second);  // step 4
    if (!miss.empty()) {  // step 5
      std::vector<std::pair<int32_t, int32_t>> old;
      old.swap(miss);
      for (const auto &m : old) {
        int32_t cur = m.first;
        for (size_t k = first_relevant(mask, m.first); k < mask.size() && cur < m.second; k++) {
          const int32_t a = mask[k].first, z = mask[k].second;
          if (a > m.second) break;
          if (z <= cur) continue;
          if (cur < a) sr_insert(miss, cur, a);
          cur = std::max(cur, z);
        }
        if (cur < m.second) sr_insert(miss, cur, m.second);
      }
    }
    b = e;
  }
  merge_sorted(out, 0);
}

void HostRegions::summary(SelSummary &s) const {
  s = SelSummary();
  s.total.assign(len.size(), 0);
  int64_t best = -1;
  for (uint32_t q = 0; q < len.size(); q++)
    for (const auto &r : missing[q]) {
      const int64_t l = (int64_t)r.second - r.first;
      s.total[q] += l;
      if (l >= best) { best = l; s.any = true; s.seq = q; s.lo = r.first; s.hi = r.second; }  // later wins on a tie (max_by)
    }
}

static void window_range(uint32_t seq, int32_t start, int32_t end, int64_t ws, std::vector<impg_gpu_range_t> &out) {
  const size_t first = out.size();  // :912-932: the tail rule looks at this range's own windows only
  int64_t pos = start;
  while (pos < end) {
    const int64_t we = std::min<int64_t>(pos + ws, end);
    if (we - pos < ws && out.size() > first) out.back().end = end;
    else out.push_back(impg_gpu_range_t{seq, (int32_t)pos, (int32_t)we});
    pos = we;
  }
}

void select_windows(const SelSummary &s, const std::vector<int32_t> &len, int selection, const std::string &sep,
                    const std::vector<std::string> *names, int64_t ws, std::vector<impg_gpu_range_t> &out) {
  out.clear();
  if (ws <= 0) throw Error{IMPG_E_INVALID, "window size must be positive"};
  const uint32_t n_seq = (uint32_t)len.size();
  if (selection == IMPG_SELECT_LONGEST) {
    if (s.any) window_range(s.seq, s.lo, s.hi, ws, out);
    return;
  }
  if (s.total.size() != n_seq) throw Error{IMPG_E_INVALID, "internal: selection without totals"};
  if (selection == IMPG_SELECT_TOTAL) {
    int64_t best = 0;
    int64_t who = -1;
    for (uint32_t q = 0; q < n_seq; q++)
      if (s.total[q] > 0 && s.total[q] >= best) { best = s.total[q]; who = q; }
    if (who >= 0) window_range((uint32_t)who, 0, len[who], ws, out);
    return;
  }
  if (selection != IMPG_SELECT_SAMPLE && selection != IMPG_SELECT_HAPLOTYPE) throw Error{IMPG_E_INVALID, "unknown selection mode"};
  if (!names || names->size() != n_seq) throw Error{IMPG_E_INVALID, "sample / haplotype selection needs the sequence names"};
  if (sep.empty()) throw Error{IMPG_E_INVALID, "empty separator"};
  std::map<std::string, std::pair<int64_t, std::vector<uint32_t>>> groups;  // ordered by prefix: the tie rule of :858-864
  for (uint32_t q = 0; q < n_seq; q++) {
    if (s.total[q] <= 0) continue;  // only sequences still in the missing map (:808-810)
    auto &g = groups[pansn_prefix((*names)[q], sep, selection == IMPG_SELECT_HAPLOTYPE)];
    g.first += s.total[q];
    g.second.push_back(q);
  }
  const std::pair<int64_t, std::vector<uint32_t>> *best = nullptr;
  for (const auto &kv : groups)
    if (!best || kv.second.first >= best->first) best = &kv.second;  // ascending prefixes: the later (greater) wins a tie
  if (!best) return;
  std::vector<uint32_t> ids = best->second;
  std::stable_sort(ids.begin(), ids.end(), [&](uint32_t a, uint32_t b) { return len[a] > len[b]; });  // ties: ascending id
  for (uint32_t q : ids) window_range(q, 0, len[q], ws, out);
}

std::string pansn_prefix(const std::string &nm, const std::string &sep, bool haplotype) {
  const size_t a = nm.find(sep);
  if (!haplotype) return nm.substr(0, a);
  // p1 + sep + p2, p2 = "" without a second field (:819-823)
  const std::string p1 = nm.substr(0, a);
  std::string p2;
  if (a != std::string::npos) {
    const size_t b = nm.find(sep, a + sep.size());
    p2 = nm.substr(a + sep.size(), b == std::string::npos ? std::string::npos : b - a - sep.size());
  }
  return p1 + sep + p2;
}

void starting_windows(const uint32_t *ids, size_t n, const std::vector<int32_t> &len, int64_t ws, std::vector<impg_gpu_range_t> &out) {
  out.clear();
  if (ws <= 0) throw Error{IMPG_E_INVALID, "window size must be positive"};
  for (size_t i = 0; i < n; i++) {
    if (ids[i] >= len.size()) throw Error{IMPG_E_INVALID, "starting sequence id out of range"};
    const uint32_t q = ids[i];
    const int64_t end = len[q];
    int64_t pos = 0;
    while (pos < end) {
      const int64_t we = std::min<int64_t>(pos + ws, end);
      if (we - pos < ws && !out.empty() && out.back().target_id == q) {  // :233-241 (and the loop ends there)
        out.back().end = (int32_t)end;
        break;
      }
      out.push_back(impg_gpu_range_t{q, (int32_t)pos, (int32_t)we});
      pos = we;
    }
  }
}

void rehome_singleton_slivers(std::vector<Partition> &parts) {  // partition.rs:45-156
  if (parts.empty()) return;
  struct Row { uint32_t c; int32_t s, e; size_t p; };
  std::vector<Row> rows;
  for (size_t p = 0; p < parts.size(); p++)
    for (const PIv &iv : parts[p].second) rows.push_back(Row{iv.seq, iv.lo, iv.hi, p});
  std::stable_sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) {
    return a.c != b.c ? a.c < b.c : a.s != b.s ? a.s < b.s : a.e < b.e;
  });
  std::vector<size_t> counts(parts.size(), 0);
  for (const Row &r : rows) counts[r.p]++;
  if (std::count(counts.begin(), counts.end(), (size_t)1) == 0) return;
  for (int pass = 1;; pass++) {
    std::vector<uint8_t> single(parts.size());
    for (size_t p = 0; p < parts.size(); p++) single[p] = counts[p] == 1;
    std::vector<std::pair<size_t, size_t>> pending;
    for (size_t i = 0; i < rows.size(); i++) {
      const Row &r = rows[i];
      if (!single[r.p]) continue;
      const bool hl = i > 0 && rows[i - 1].c == r.c && rows[i - 1].e == r.s;
      const bool hr = i + 1 < rows.size() && rows[i + 1].c == r.c && rows[i + 1].s == r.e;
      const bool ls = hl && !single[rows[i - 1].p], rs = hr && !single[rows[i + 1].p];
      size_t target;
      if (ls && rs) target = counts[rows[i - 1].p] >= counts[rows[i + 1].p] ? rows[i - 1].p : rows[i + 1].p;
      else if (ls) target = rows[i - 1].p;
      else if (rs) target = rows[i + 1].p;
      else continue;
      if (target != r.p) pending.push_back({i, target});
    }
    if (pending.empty() || pass > 100) break;
    for (const auto &pr : pending) {
      counts[rows[pr.first].p]--;
      counts[pr.second]++;
      rows[pr.first].p = pr.second;
    }
  }
  std::vector<std::vector<PIv>> fresh(parts.size());
  for (const Row &r : rows) fresh[r.p].push_back(PIv{r.c, r.s, r.e});
  std::vector<Partition> rebuilt;
  for (size_t p = 0; p < parts.size(); p++)
    if (!fresh[p].empty()) rebuilt.push_back({parts[p].first, std::move(fresh[p])});
  parts.swap(rebuilt);
}

static void bed_line(std::string &t, const std::string &name, const PIv &iv, const uint64_t *pnum) {
  char buf[96];
  t += name;
  const int k = pnum ? snprintf(buf, sizeof buf, "\t%d\t%d\t%llu\n", iv.lo, iv.hi, (unsigned long long)*pnum)
                     : snprintf(buf, sizeof buf, "\t%d\t%d\n", iv.lo, iv.hi);
  t.append(buf, (size_t)k);
}
static std::string single_file_text(const std::vector<Partition> &parts, const std::vector<std::string> &names) {
  std::string t;
  for (const Partition &p : parts)
    for (const PIv &iv : p.second) {
      if (iv.seq >= names.size()) throw Error{IMPG_E_INVALID, "row names an unknown sequence id"};
      bed_line(t, names[iv.seq], iv, &p.first);
    }
  return t;
}
static char *dup_text(const std::string &t, size_t *len) {
  char *p = (char *)malloc(t.size() + 1);
  if (!p) throw std::bad_alloc();
  memcpy(p, t.data(), t.size());
  p[t.size()] = 0;
  if (len) *len = t.size();
  return p;
}
static void write_all(int fd, const char *p, size_t n, const std::string &what) {
  size_t at = 0;
  while (at < n) {
    const ssize_t k = write(fd, p + at, n - at);
    if (k < 0 && errno == EINTR) continue;
    if (k <= 0) throw Error{IMPG_E_IO, "write failed: " + what};
    at += (size_t)k;
  }
}
// folder/name created (the folder too) and opened for writing; `path` is what errors call it
static int create_file(const char *folder, const std::string &name, std::string &path) {
  path = name;
  if (folder && *folder) {
    if (mkdir(folder, 0777) != 0 && errno != EEXIST) {  // create_output_path (:16-28), one level at a time
      std::string f = folder;
      for (size_t i = 1; i < f.size(); i++)
        if (f[i] == '/') { f[i] = 0; mkdir(f.c_str(), 0777); f[i] = '/'; }
      if (mkdir(folder, 0777) != 0 && errno != EEXIST) throw Error{IMPG_E_IO, std::string("cannot create ") + folder};
    }
    path = std::string(folder) + "/" + name;
  }
  const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
  if (fd < 0) throw Error{IMPG_E_IO, "cannot create " + path};
  return fd;
}
static void write_file(const char *folder, const std::string &name, const std::string &text) {
  std::string path;
  const int fd = create_file(folder, name, path);
  size_t at = 0;
  while (at < text.size()) {
    const ssize_t k = write(fd, text.data() + at, text.size() - at);
    if (k <= 0) { close(fd); throw Error{IMPG_E_IO, "write failed: " + path}; }
    at += (size_t)k;
  }
  close(fd);
}

}  // namespace impg

using namespace impg;

struct impg_gpu_regions {
  bool on_host = true;
  std::vector<int32_t> len;
  std::unique_ptr<HostRegions> h;
  std::unique_ptr<DeviceRegions> d;
  std::vector<PIv> last;  // the rows of the last apply / window, kept until the next one (impg_gpu_regions_last_rows)
  void summary(SelSummary &s, bool totals) {
    if (on_host) h->summary(s);
    else d->summary(s, totals);
  }
};

struct impg_gpu_partition {
  impg_gpu_index *ix = nullptr;
  impg_gpu_params_t params;
  impg_gpu_partition_opts_t opts;
  std::string sep = "#";
  impg_gpu_regions regions;
  Engine *engine = nullptr;  // device state: held for the session's life
  std::vector<impg_gpu_range_t> pending;  // the starting sequences' windows, handed out first
  bool have_pending = false;
  DevBuf rows;
  int64_t c_windows = 0, c_partitions = 0, c_mask_uploads = 0, c_rows_to_host = 0, c_walk_windows = 0;
  // FASTA output: the text stream lives as long as the session (made at its first FASTA window)
  TextStream text;
  unsigned long long text_hint = 0;  // the size its buffers get: no window prints more bases than the store holds
  int64_t c_fasta_windows = 0, c_fasta_host_windows = 0;
  ~impg_gpu_partition() {
    if (engine) {
      (void)hipSetDevice(ix->device);
      text.drop();
      rows.release();
      regions.d.reset();
      engine->masked = false;
      return_engine(*ix, engine);
    }
  }
};

static void regions_init(impg_gpu_regions &r, const int64_t *seq_len, uint32_t n_seq, bool on_host, int device, hipStream_t s) {
  r.on_host = on_host;
  r.len.resize(n_seq);
  for (uint32_t q = 0; q < n_seq; q++) r.len[q] = (int32_t)std::min<int64_t>(std::max<int64_t>(seq_len[q], 0), INT32_MAX);
  if (on_host) r.h = std::make_unique<HostRegions>(seq_len, n_seq);
  else {
    require_device(device);
    IMPG_HIP(hipSetDevice(device));
    r.d = std::make_unique<DeviceRegions>(device, seq_len, n_seq, s);
  }
}
static void regions_apply(impg_gpu_regions &r, const impg_gpu_interval_t *rows, size_t n, int32_t d, int32_t mm, int32_t mb, std::vector<PIv> &out) {
  if (d < 0) throw Error{IMPG_E_INVALID, "merge_distance < 0 (--no-merge) is not supported: the reference's own sortedness assertion (partition.rs:1325) does not hold there"};
  if (n >= (1ull << 30)) throw Error{IMPG_E_UNSUPPORTED, "more than 2^30 rows in one window"};
  if (r.on_host) r.h->apply(rows, n, d, mm, mb, out);
  else {
    for (size_t i = 0; i < n; i++) {
      if (rows[i].query_id >= r.len.size()) throw Error{IMPG_E_INVALID, "row names an unknown sequence id"};
      if (std::min(rows[i].q_first, rows[i].q_last) < 0) throw Error{IMPG_E_INVALID, "row with a negative coordinate"};
    }
    IMPG_HIP(hipSetDevice(r.d->device));
    r.d->apply_host_rows(rows, (uint32_t)n, d, mm, mb, out);
  }
}
static void regions_windows(impg_gpu_regions &r, int selection, const std::string &sep, const std::vector<std::string> *names, int64_t ws,
                            std::vector<impg_gpu_range_t> &out) {
  SelSummary s;
  if (!r.on_host) IMPG_HIP(hipSetDevice(r.d->device));
  r.summary(s, selection != IMPG_SELECT_LONGEST);
  select_windows(s, r.len, selection, sep, names, ws, out);
}

extern "C" {

int impg_gpu_regions_create(const int64_t *seq_len, uint32_t n_seq, int on_host, int device, impg_gpu_regions_t **out) {
  IMPG_TRY
  if (!out || (!seq_len && n_seq)) throw Error{IMPG_E_INVALID, "null argument"};
  auto r = std::make_unique<impg_gpu_regions>();
  regions_init(*r, seq_len, n_seq, on_host != 0, device, nullptr);
  *out = r.release();
  return IMPG_OK;
  IMPG_CATCH
}

static void copy_rows(const std::vector<PIv> &v, impg_gpu_partition_row_t *out, size_t cap) {
  for (size_t i = 0; i < v.size() && i < cap; i++) out[i] = impg_gpu_partition_row_t{v[i].seq, v[i].lo, v[i].hi};
}

int impg_gpu_regions_apply(impg_gpu_regions_t *r, const impg_gpu_interval_t *rows, size_t n_rows, int32_t merge_distance,
                           int32_t min_missing_size, int32_t min_boundary_distance, impg_gpu_partition_row_t *out_rows, size_t cap,
                           size_t *n_out) {
  IMPG_TRY
  if (!r || !n_out || (!rows && n_rows) || (!out_rows && cap)) throw Error{IMPG_E_INVALID, "null argument"};
  r->last.clear();
  regions_apply(*r, rows, n_rows, merge_distance, min_missing_size, min_boundary_distance, r->last);
  copy_rows(r->last, out_rows, cap);
  *n_out = r->last.size();
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_regions_apply_device(impg_gpu_regions_t *r, const impg_gpu_interval_t *d_rows, size_t n_rows, int32_t merge_distance,
                                  int32_t min_missing_size, int32_t min_boundary_distance, impg_gpu_partition_row_t *out_rows, size_t cap,
                                  size_t *n_out) {
  IMPG_TRY
  if (!r || !n_out || (!d_rows && n_rows) || (!out_rows && cap)) throw Error{IMPG_E_INVALID, "null argument"};
  if (r->on_host) throw Error{IMPG_E_INVALID, "rows in device memory need a device-state object (on_host = 0)"};
  if (merge_distance < 0) throw Error{IMPG_E_INVALID, "merge_distance < 0 (--no-merge) is not supported"};
  if (n_rows >= (1ull << 30)) throw Error{IMPG_E_UNSUPPORTED, "more than 2^30 rows in one window"};
  r->last.clear();
  IMPG_HIP(hipSetDevice(r->d->device));
  r->d->apply(d_rows, (uint32_t)n_rows, merge_distance, min_missing_size, min_boundary_distance, r->last);
  copy_rows(r->last, out_rows, cap);
  *n_out = r->last.size();
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_regions_last_rows(const impg_gpu_regions_t *r, impg_gpu_partition_row_t *out_rows, size_t cap, size_t *n_out) {
  IMPG_TRY
  if (!r || !n_out || (!out_rows && cap)) throw Error{IMPG_E_INVALID, "null argument"};
  copy_rows(r->last, out_rows, cap);
  *n_out = r->last.size();
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_regions_get(impg_gpu_regions_t *r, int which, uint64_t *off_out, int32_t *ranges_out, size_t cap, size_t *n_ranges) {
  IMPG_TRY
  if (!r || !off_out || !n_ranges || (!ranges_out && cap)) throw Error{IMPG_E_INVALID, "null argument"};
  if (which != IMPG_REGIONS_MASKED && which != IMPG_REGIONS_MISSING) throw Error{IMPG_E_INVALID, "which: masked or missing"};
  const size_t n_seq = r->len.size();
  std::vector<int32_t> flat;
  if (r->on_host) {
    const auto &t = which == IMPG_REGIONS_MASKED ? r->h->masked : r->h->missing;
    off_out[0] = 0;
    for (size_t q = 0; q < n_seq; q++) {
      for (const auto &x : t[q]) { flat.push_back(x.first); flat.push_back(x.second); }
      off_out[q + 1] = flat.size() / 2;
    }
  } else {
    IMPG_HIP(hipSetDevice(r->d->device));
    std::vector<uint32_t> off(n_seq + 1);
    r->d->get(which, off.data(), flat);
    for (size_t q = 0; q <= n_seq; q++) off_out[q] = off[q];
  }
  *n_ranges = flat.size() / 2;
  if (cap) memcpy(ranges_out, flat.data(), std::min(cap, flat.size() / 2) * 8);
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_regions_select(impg_gpu_regions_t *r, int selection, const char *separator, const char *const *names, int64_t window_size,
                            impg_gpu_range_t *windows_out, size_t cap, size_t *n) {
  IMPG_TRY
  if (!r || !n || (!windows_out && cap)) throw Error{IMPG_E_INVALID, "null argument"};
  std::vector<std::string> nm;
  if (names) for (size_t q = 0; q < r->len.size(); q++) nm.push_back(names[q] ? names[q] : "");
  std::vector<impg_gpu_range_t> w;
  regions_windows(*r, selection, separator ? separator : "#", names ? &nm : nullptr, window_size, w);
  for (size_t i = 0; i < w.size() && i < cap; i++) windows_out[i] = w[i];
  *n = w.size();
  return IMPG_OK;
  IMPG_CATCH
}

void impg_gpu_regions_free(impg_gpu_regions_t *r) {
  if (r && r->d) (void)hipSetDevice(r->d->device);
  delete r;
}

int impg_gpu_partition_starting_windows(const uint32_t *seq_ids, size_t n, const int64_t *seq_len, uint32_t n_seq, int64_t window_size,
                                        impg_gpu_range_t *windows_out, size_t cap, size_t *n_out) {
  IMPG_TRY
  if (!n_out || (!seq_ids && n) || (!seq_len && n_seq) || (!windows_out && cap)) throw Error{IMPG_E_INVALID, "null argument"};
  std::vector<int32_t> len(n_seq);
  for (uint32_t q = 0; q < n_seq; q++) len[q] = (int32_t)std::min<int64_t>(std::max<int64_t>(seq_len[q], 0), INT32_MAX);
  std::vector<impg_gpu_range_t> w;
  starting_windows(seq_ids, n, len, window_size, w);
  for (size_t i = 0; i < w.size() && i < cap; i++) windows_out[i] = w[i];
  *n_out = w.size();
  return IMPG_OK;
  IMPG_CATCH
}

static void to_parts(const impg_gpu_partition_row_t *rows, const uint64_t *pnum, size_t n, std::vector<Partition> &parts) {
  for (size_t i = 0; i < n; i++) {
    if (i && pnum[i] < pnum[i - 1]) throw Error{IMPG_E_INVALID, "partition numbers must ascend"};
    if (parts.empty() || parts.back().first != pnum[i]) parts.push_back({pnum[i], {}});
    parts.back().second.push_back(PIv{rows[i].seq_id, std::min(rows[i].start, rows[i].end), std::max(rows[i].start, rows[i].end)});
  }
}

int impg_gpu_partition_rehome(impg_gpu_partition_row_t *rows, uint64_t *partition_num, size_t n) {
  IMPG_TRY
  if ((!rows || !partition_num) && n) throw Error{IMPG_E_INVALID, "null argument"};
  std::vector<Partition> parts;
  to_parts(rows, partition_num, n, parts);
  rehome_singleton_slivers(parts);
  size_t k = 0;
  for (const Partition &p : parts)
    for (const PIv &iv : p.second) {
      rows[k] = impg_gpu_partition_row_t{iv.seq, iv.lo, iv.hi};
      partition_num[k++] = p.first;
    }
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_partition_bed_text(const impg_gpu_partition_row_t *rows, const uint64_t *partition_num, size_t n, const char *const *names,
                                uint32_t n_seq, char **text, size_t *len) {
  IMPG_TRY
  if (!text || ((!rows || !partition_num) && n) || (!names && n_seq)) throw Error{IMPG_E_INVALID, "null argument"};
  std::vector<std::string> nm(n_seq);
  for (uint32_t q = 0; q < n_seq; q++) nm[q] = names[q] ? names[q] : "";
  std::vector<Partition> parts;
  to_parts(rows, partition_num, n, parts);
  *text = dup_text(single_file_text(parts, nm), len);
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_partition_create(impg_gpu_index_t *ix, const impg_gpu_params_t *params, const impg_gpu_partition_opts_t *opts,
                              const uint32_t *starting_seq_ids, size_t n_starting, impg_gpu_partition_t **out) {
  IMPG_TRY
  if (!ix || !params || !opts || !out || (!starting_seq_ids && n_starting)) throw Error{IMPG_E_INVALID, "null argument"};
  if (ix->shard || ix->cluster) throw Error{IMPG_E_UNSUPPORTED, "partition on a sharded index is not built"};
  if (!params->transitive) throw Error{IMPG_E_INVALID, "partition runs the transitive queries (params.transitive = 1)"};
  if (params->store_cigar) throw Error{IMPG_E_INVALID, "partition queries never store CIGARs (partition.rs:369)"};
  if (params->min_output_length >= 0) throw Error{IMPG_E_INVALID, "partition queries have no min_output_length (partition.rs:368)"};
  if (opts->merge_distance < 0) throw Error{IMPG_E_INVALID, "merge_distance < 0 (--no-merge) is not supported: the reference's own sortedness assertion (partition.rs:1325) does not hold there"};
  if (opts->window_size <= 0) throw Error{IMPG_E_INVALID, "window size must be positive"};
  if (opts->selection < IMPG_SELECT_LONGEST || opts->selection > IMPG_SELECT_HAPLOTYPE) throw Error{IMPG_E_INVALID, "unknown selection mode"};
  Engine::check_params(*params);
  auto p = std::make_unique<impg_gpu_partition>();
  p->ix = ix;
  p->params = *params;
  p->opts = *opts;
  if (opts->separator) p->sep = opts->separator;
  p->opts.separator = nullptr;
  if (p->sep.empty()) throw Error{IMPG_E_INVALID, "empty separator"};
  const uint32_t n_seq = (uint32_t)ix->seq.lens.size();
  if (opts->selection >= IMPG_SELECT_SAMPLE && ix->seq.names.size() != n_seq) throw Error{IMPG_E_INVALID, "sample / haplotype selection needs an index with sequence names"};
  IMPG_HIP(hipSetDevice(ix->device));
  if (!opts->state_on_host) {
    p->engine = try_lease_engine(*ix);
    if (!p->engine) throw Error{IMPG_E_UNSUPPORTED, "every engine of the index is held by another handle: free one (a partition session keeps its engine)"};
    p->rows.pool = nullptr;
  }
  regions_init(p->regions, ix->seq.lens.data(), n_seq, opts->state_on_host != 0, ix->device, p->engine ? p->engine->stream : nullptr);
  if (n_starting) {
    starting_windows(starting_seq_ids, n_starting, p->regions.len, opts->window_size, p->pending);
    p->have_pending = !p->pending.empty();
  }
  *out = p.release();
  return IMPG_OK;
  IMPG_CATCH
}

static void next_windows(impg_gpu_partition &p, std::vector<impg_gpu_range_t> &w) {
  if (p.have_pending) { w = p.pending; return; }
  regions_windows(p.regions, p.opts.selection, p.sep, p.opts.selection >= IMPG_SELECT_SAMPLE ? &p.ix->seq.names : nullptr, p.opts.window_size, w);
}

int impg_gpu_partition_next_windows(impg_gpu_partition_t *p, impg_gpu_range_t *windows_out, size_t cap, size_t *n) {
  IMPG_TRY
  if (!p || !n || (!windows_out && cap)) throw Error{IMPG_E_INVALID, "null argument"};
  std::vector<impg_gpu_range_t> w;
  next_windows(*p, w);
  *n = w.size();
  if (w.size() > cap) return IMPG_OK;
  std::copy(w.begin(), w.end(), windows_out);
  p->have_pending = false;
  p->pending.clear();
  return IMPG_OK;
  IMPG_CATCH
}

namespace {
struct MaskAlias {  // the engine reads the session's tables where they lie; its own buffers come back untouched
  Engine &E;
  void *off, *rng, *il, *tl;
  MaskAlias(Engine &e, DeviceRegions &d) : E(e), off(e.mask_off.p), rng(e.mask_ranges.p), il(e.mask_init_len.p), tl(e.mask_touch_len.p) {
    E.mask_off.p = (void *)d.mask_off();
    E.mask_ranges.p = (void *)d.mask_ranges();
    E.mask_init_len.p = E.mask_touch_len.p = d.len.p;
    E.masked = true;
    E.mask_has_empty = d.mask_has_empty;
    E.mask_ranges_total = d.n_mask;
    E.mask_lists = d.n_seq;
  }
  ~MaskAlias() {
    E.mask_off.p = off; E.mask_ranges.p = rng; E.mask_init_len.p = il; E.mask_touch_len.p = tl;
    E.masked = false;
  }
};
void window(impg_gpu_partition &p, const impg_gpu_range_t &w, std::vector<PIv> &out) {
  if (w.start >= w.end) throw Error{IMPG_E_INVALID, "window must satisfy start < end"};
  if (w.target_id >= p.regions.len.size()) throw Error{IMPG_E_INVALID, "window names an unknown sequence id"};
  impg_gpu_index &ix = *p.ix;
  IMPG_HIP(hipSetDevice(ix.device));
  const impg_gpu_partition_opts_t &o = p.opts;
  p.c_windows++;
  // what crossed PCIe for this window's query is read off the index's counters, which are bumped where the copies are
  // issued (apply_mask, assemble_results, walk_query): zero on the device path is observed, not assumed.  (Other threads
  // querying the same handle meanwhile would be counted in.)
  struct Traffic {
    impg_gpu_partition &p;
    const uint64_t up0, rows0;
    explicit Traffic(impg_gpu_partition &p_) : p(p_), up0(p_.ix->mask_table_uploads.load()), rows0(p_.ix->result_rows_to_host.load()) {}
    ~Traffic() {
      p.c_mask_uploads += (int64_t)(p.ix->mask_table_uploads.load() - up0);
      p.c_rows_to_host += (int64_t)(p.ix->result_rows_to_host.load() - rows0);
    }
  } traffic(p);
  if (p.engine) {
    DeviceRegions &d = *p.regions.d;
    const impg_gpu_interval_t *d_rows = nullptr;
    bool walked = false;
    uint32_t n;
    {
      MaskAlias alias(*p.engine, d);
      n = query_rows_device(ix, *p.engine, w, p.params, p.rows, d_rows, walked);
    }
    if (walked) p.c_walk_windows++;
    d.apply(d_rows, n, o.merge_distance, o.min_missing_size, o.min_boundary_distance, out);
    return;
  }
  // host state: what a host binding does today
  HostRegions &h = *p.regions.h;
  const uint32_t n_seq = (uint32_t)h.len.size();
  std::vector<uint32_t> ids(n_seq);
  std::vector<uint64_t> off(n_seq + 1, 0);
  std::vector<int32_t> flat;
  for (uint32_t q = 0; q < n_seq; q++) {
    ids[q] = q;
    for (const auto &x : h.masked[q]) { flat.push_back(x.first); flat.push_back(x.second); }
    off[q + 1] = flat.size() / 2;
  }
  impg_gpu_mask_t m{n_seq, ids.data(), h.len.data(), off.data(), flat.data()};
  impg_gpu_results_t *res = nullptr;
  const int rc = impg_gpu_query_batch_masked(&ix, &w, 1, &p.params, &m, &res);
  if (rc != IMPG_OK) throw Error{rc, impg_gpu_last_error()};
  std::unique_ptr<impg_gpu_results_t, void (*)(impg_gpu_results_t *)> hold(res, impg_gpu_results_free);
  const size_t n = impg_gpu_results_total(res);
  h.apply(impg_gpu_results_intervals(res), n, o.merge_distance, o.min_missing_size, o.min_boundary_distance, out);
}
}  // namespace

int impg_gpu_partition_window(impg_gpu_partition_t *p, const impg_gpu_range_t *w, impg_gpu_partition_row_t *rows_out, size_t cap, size_t *n_out) {
  IMPG_TRY
  if (!p || !w || !n_out || (!rows_out && cap)) throw Error{IMPG_E_INVALID, "null argument"};
  p->regions.last.clear();
  window(*p, *w, p->regions.last);
  copy_rows(p->regions.last, rows_out, cap);
  *n_out = p->regions.last.size();
  if (!p->regions.last.empty()) p->c_partitions++;
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_partition_run(impg_gpu_partition_t *p, const char *folder, int separate_files, char **text, size_t *len, uint64_t *n_partitions) {
  IMPG_TRY
  if (!p) throw Error{IMPG_E_INVALID, "null argument"};
  if (p->ix->seq.names.size() != p->regions.len.size()) throw Error{IMPG_E_INVALID, "BED text needs an index with sequence names"};
  std::vector<Partition> parts;
  uint64_t num = 0;
  std::vector<impg_gpu_range_t> w;
  for (;;) {
    next_windows(*p, w);
    p->have_pending = false;
    p->pending.clear();
    if (w.empty()) break;
    for (const impg_gpu_range_t &r : w) {
      window(*p, r, p->regions.last);
      const std::vector<PIv> &rows = p->regions.last;
      if (rows.empty()) continue;
      p->c_partitions++;
      if (separate_files && !text) {
        std::string t;
        for (const PIv &iv : rows) bed_line(t, p->ix->seq.names[iv.seq], iv, nullptr);
        write_file(folder, "partition" + std::to_string(num) + ".bed", t);
      } else parts.push_back({num, rows});
      num++;
    }
  }
  if (!(separate_files && !text)) {
    if (p->opts.rehome_singletons && !separate_files) rehome_singleton_slivers(parts);
    const std::string t = single_file_text(parts, p->ix->seq.names);
    if (text) *text = dup_text(t, len);
    else if (!parts.empty()) write_file(folder, "partitions.bed", t);
  }
  if (n_partitions) *n_partitions = num;
  return IMPG_OK;
  IMPG_CATCH
}

namespace {
static_assert(sizeof(PIv) == sizeof(impg_gpu_partition_row_t), "PIv and impg_gpu_partition_row_t are one layout");
// the host twin over the handle's own names and bases
void host_rows_fasta(const impg_gpu_index &ix, const impg_gpu_partition_row_t *rows, size_t n, std::string &text) {
  if (!ix.seq_store) throw Error{IMPG_E_INVALID, "FASTA output needs a sequence store (impg_gpu_index_set_sequences)"};
  host_copy(*ix.seq_store);
  const size_t at = text.size();
  partition_fasta_text(rows, n, [&ix](uint32_t id, std::string &name, SeqRef &ref) {
    name = id < ix.seq.names.size() ? ix.seq.names[id] : std::to_string(id);
    const uint32_t s = id < ix.store_of_id.size() ? ix.store_of_id[id] : SEQ_ABSENT;
    if (s == SEQ_ABSENT) return false;
    const SeqStore &st = *ix.seq_store;
    ref = SeqRef{st.bases.data() + st.off[s], st.off[s + 1] - st.off[s]};
    return true;
  }, text);
  ix.fasta_stats[FASTA_RECORDS] += n;
  ix.fasta_stats[FASTA_TEXT_BYTES] += text.size() - at;
}
// One window: query, update, and the text of what the update left, to `sink`.  The window's rows are in regions.last.
void window_fasta(impg_gpu_partition &p, const impg_gpu_range_t &w, const std::function<void(const char *, size_t)> &sink) {
  impg_gpu_index &ix = *p.ix;
  if (!ix.seq_store) throw Error{IMPG_E_INVALID, "FASTA output needs a sequence store (impg_gpu_index_set_sequences)"};
  window(p, w, p.regions.last);
  const std::vector<PIv> &rows = p.regions.last;
  if (rows.empty()) return;
  p.c_partitions++;
  if (p.engine) {
    if (!p.text_hint) {
      const unsigned long long bases = ix.seq_store->off.empty() ? 0ull : ix.seq_store->off.back();
      p.text_hint = bases + bases / 80 + 4096;
    }
    // (the rows the update left in HBM: DeviceRegions::apply has copied them to `last` and waited for the stream)
    device_partition_fasta(*p.engine, ix, p.text, p.regions.d->out_rows.as<PIv>(), (uint32_t)rows.size(), p.text_hint, sink);
    p.c_fasta_windows++;
    // IMPG_PARTITION_TEXT_STREAM_PER_WINDOW (a probe's switch, read on every window): the stream is dropped behind every
    // window, as a per-call writer would allocate it -- what the session-lived stream is measured against
    const char *per_window = getenv("IMPG_PARTITION_TEXT_STREAM_PER_WINDOW");
    if (per_window && *per_window && *per_window != '0') p.text.drop();
    return;
  }
  std::string t;
  host_rows_fasta(ix, reinterpret_cast<const impg_gpu_partition_row_t *>(rows.data()), rows.size(), t);
  p.c_fasta_host_windows++;
  sink(t.data(), t.size());
}
}  // namespace

int impg_gpu_partition_window_fasta(impg_gpu_partition_t *p, const impg_gpu_range_t *w, int fd, char **text, size_t *len, size_t *n_rows) {
  IMPG_TRY
  if (!p || !w || !n_rows || (text && !len)) throw Error{IMPG_E_INVALID, "null argument"};
  if (text) *text = nullptr;
  *n_rows = 0;
  p->regions.last.clear();
  std::string out;
  window_fasta(*p, *w, [&](const char *b, size_t k) {
    if (text) out.append(b, k);
    else write_all(fd, b, k, "the window's FASTA text");
  });
  *n_rows = p->regions.last.size();
  if (text && *n_rows) *text = dup_text(out, len);
  else if (len) *len = 0;
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_partition_run_fasta(impg_gpu_partition_t *p, const char *folder, uint64_t *n_partitions) {
  IMPG_TRY
  if (!p) throw Error{IMPG_E_INVALID, "null argument"};
  const impg_gpu_index &ix = *p->ix;
  if (!ix.seq_store) throw Error{IMPG_E_INVALID, "FASTA output needs a sequence store (impg_gpu_index_set_sequences)"};
  for (size_t id = 0; id < ix.seq.lens.size(); id++)  // every sequence is partitioned eventually: refuse now, not hours in
    if (ix.seq.lens[id] > 0 && (id >= ix.store_of_id.size() || ix.store_of_id[id] == SEQ_ABSENT))
      throw Error{IMPG_E_INVALID, "Sequence '" + (id < ix.seq.names.size() ? ix.seq.names[id] : std::to_string(id)) + "' not found in the sequence store"};
  uint64_t num = 0;
  std::vector<impg_gpu_range_t> w;
  for (;;) {
    next_windows(*p, w);
    p->have_pending = false;
    p->pending.clear();
    if (w.empty()) break;
    for (const impg_gpu_range_t &r : w) {
      struct Out { int fd = -1; std::string path; ~Out() { if (fd >= 0) close(fd); } } out;
      window_fasta(*p, r, [&](const char *b, size_t k) {
        if (out.fd < 0) out.fd = create_file(folder, "partition" + std::to_string(num) + ".fasta", out.path);  // (at the first byte: a refused window leaves no file)
        write_all(out.fd, b, k, out.path);
      });
      if (!p->regions.last.empty()) num++;
    }
  }
  if (n_partitions) *n_partitions = num;
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_partition_rows_fasta(impg_gpu_index_t *ix, const impg_gpu_partition_row_t *rows, size_t n, int on_host, char **text, size_t *len) {
  IMPG_TRY
  if (!ix || !text || !len || (n && !rows)) throw Error{IMPG_E_INVALID, "null argument"};
  if (ix->shard || ix->cluster) throw Error{IMPG_E_UNSUPPORTED, "device-side FASTA on a sharded index"};
  if (!ix->seq_store) throw Error{IMPG_E_INVALID, "FASTA output needs a sequence store (impg_gpu_index_set_sequences)"};
  if (n >= (1ull << 30)) throw Error{IMPG_E_UNSUPPORTED, "more than 2^30 rows in one call"};
  std::string out;
  if (on_host) host_rows_fasta(*ix, rows, n, out);
  else if (n) {
    IMPG_HIP(hipSetDevice(ix->device));
    EngineLease lease(*ix);
    TextStream S;  // (this call's own: made and freed here)
    DevBuf d_rows;
    d_rows.reserve(n * sizeof(PIv));
    IMPG_HIP(hipMemcpyAsync(d_rows.p, rows, n * sizeof(PIv), hipMemcpyHostToDevice, lease->stream));
    device_partition_fasta(*lease, *ix, S, d_rows.as<PIv>(), (uint32_t)n, 0, [&](const char *b, size_t k) { out.append(b, k); });
  }
  *text = dup_text(out, len);
  return IMPG_OK;
  IMPG_CATCH
}

impg_gpu_regions_t *impg_gpu_partition_regions(impg_gpu_partition_t *p) { return p ? &p->regions : nullptr; }

int impg_gpu_partition_counter(const impg_gpu_partition_t *p, const char *key, int64_t *value) {
  IMPG_TRY
  if (!p || !key || !value) throw Error{IMPG_E_INVALID, "null argument"};
  const std::string k = key;
  if (k == "windows") *value = p->c_windows;
  else if (k == "partitions") *value = p->c_partitions;
  else if (k == "mask_uploads") *value = p->c_mask_uploads;
  else if (k == "rows_to_host") *value = p->c_rows_to_host;
  else if (k == "walk_windows") *value = p->c_walk_windows;
  else if (k == "fasta_windows") *value = p->c_fasta_windows;
  else if (k == "fasta_host_windows") *value = p->c_fasta_host_windows;
  else if (k == "text_buffer_allocs") *value = (int64_t)p->text.allocs;
  else if (k == "text_table_uploads") *value = (int64_t)p->text.uploads;
  else if (k == "step_launches") *value = p->regions.d ? (int64_t)p->regions.d->launches : 0;
  else throw Error{IMPG_E_INVALID, "unknown counter: " + k};
  return IMPG_OK;
  IMPG_CATCH
}

void impg_gpu_partition_destroy(impg_gpu_partition_t *p) { delete p; }

}  // extern "C"
