// PAF files streamed into HBM, the host side (paf_ingest.hpp): the driver that keeps lines whole
// across pieces, gives the names the device did not know their ids and rebuilds the name table, and the host twin of the
// kernels (HostBackend), which serves the CPU tests and a stand-alone sanitizer program and is never a fallback.  No HIP
// call in here.  The driver reads two things of a line: where a piece's last '\n' is (memrchr), and the bytes of the names
// that came home as unknown.
#include <sys/stat.h>

#include "engine.hpp"
#include "paf_ingest.hpp"

namespace impg {
namespace paf_ingest {

namespace {

bool compressed(const std::string &path) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return false;
  unsigned char m[2] = {0, 0};
  const size_t k = fread(m, 1, 2, f);
  fclose(f);
  return k == 2 && m[0] == 0x1f && m[1] == 0x8b;
}

void table_place(Table &T, uint32_t id) {
  for (uint32_t k = 0; k < T.cap; k++) {
    uint32_t &s = T.slot[(uint32_t)(T.hash[id] + k) & (T.cap - 1u)];
    if (!s) { s = id + 1u; return; }
  }
  throw Error{IMPG_E_INVALID, "internal: the name table is full"};
}
// name `id` (the next one) enters the table; the table doubles while it is half full
void table_add(Table &T, const std::string &name, unsigned hash_bits) {
  const uint32_t id = (uint32_t)T.hash.size();
  T.hash.push_back(name_hash(name.data(), (uint32_t)name.size(), hash_bits));
  T.pool += name;
  T.off.push_back(T.pool.size());
  if ((uint64_t)(id + 1u) * 2u >= T.cap) {
    if (T.cap >= (1u << 31)) throw Error{IMPG_E_UNSUPPORTED, "more than 2^30 sequence names"};
    T.cap *= 2u;
    T.slot.assign(T.cap, 0u);
    for (uint32_t k = 0; k <= id; k++) table_place(T, k);
  } else table_place(T, id);
}

}  // namespace

uint64_t initial_pool_ops(const std::vector<std::string> &paths) {
  uint64_t ops = 0;
  for (const std::string &p : paths) {
    struct stat st;
    if (stat(p.c_str(), &st) == 0) ops += (uint64_t)st.st_size / 3u * (compressed(p) ? 4u : 1u);
  }
  return std::max<uint64_t>(ops, 64);
}

void load_files(Backend &B, const std::vector<std::string> &paths, size_t piece_bytes, unsigned hash_bits, uint64_t pool_ops, Loaded &out) {
  if (!piece_bytes) piece_bytes = DEFAULT_PIECE;
  if (piece_bytes < 16 || piece_bytes > (1ull << 32) || piece_bytes % 16) throw Error{IMPG_E_INVALID, "piece_bytes is 0 or 16 .. 2^32, a multiple of 16"};
  if (!hash_bits || hash_bits > 64) throw Error{IMPG_E_INVALID, "hash_bits is 1 .. 64"};
  size_t cap = std::min(piece_bytes, MAX_BUFFER);
  out = Loaded();
  B.begin(cap, pool_ops ? pool_ops : initial_pool_ops(paths), hash_bits);
  Table T;
  T.slot.assign(T.cap, 0u);
  T.off.assign(1, 0);
  B.table(T);
  std::vector<Unknown> list;
  std::string bytes;
  std::vector<uint32_t> occ, ids;
  for (const std::string &path : paths) {
    out.file_first.push_back(out.n_records);
    ingest::FileText f(path, &out.stats[INFLATED_BLOCKS]);
    bool ended = false;
    struct Piece { size_t n, tail; };  // the whole lines at the block's front, the bytes behind them
    // fills block `which` behind its `fill` carried bytes.  A block without a '\n' while the text goes on is a line longer
    // than the buffer: the buffer doubles and the read goes on.
    auto next_piece = [&](int which, size_t fill) -> Piece {
      const auto t0 = std::chrono::steady_clock::now();
      Piece p{0, 0};
      for (;;) {
        size_t got = 0;
        if (!ended) {
          got = f.next(B.buffer(which) + fill, cap - fill);
          ended = got < cap - fill;
        }
        const size_t total = fill + got;
        if (ended) { p = Piece{total, 0}; break; }
        const char *b = B.buffer(which);
        const void *nl = memrchr(b, '\n', total);
        if (nl) {
          const size_t n = (size_t)((const char *)nl - b) + 1;
          p = Piece{n, total - n};
          break;
        }
        if (cap >= MAX_BUFFER) throw Error{IMPG_E_UNSUPPORTED, "a line of 4 GiB or more in " + path};
        cap = std::min(cap * 2, MAX_BUFFER);
        B.grow(cap, which, total);
        out.stats[BUFFER_GROWS]++;
        fill = total;
      }
      out.read_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      return p;
    };
    int w = 0;
    Piece p = next_piece(0, 0);
    while (p.n) {
      B.piece_begin(w, p.n);
      if (p.tail) memcpy(B.buffer(w ^ 1), B.buffer(w) + p.n, p.tail);
      out.stats[CARRIED_BYTES] += p.tail;
      const Piece q = next_piece(w ^ 1, p.tail);
      uint32_t n_lines = 0;
      B.piece_unknowns(n_lines, list, bytes);
      const auto t0 = std::chrono::steady_clock::now();
      occ.clear();
      ids.clear();
      bool added = false;
      for (const Unknown &u : list) {  // in occurrence order: ids in first-seen order, the first length wins
        if (u.at + u.len > bytes.size()) throw Error{IMPG_E_INVALID, "internal: an unknown name outside the list's bytes"};
        const std::string name(bytes.data() + u.at, u.len);
        uint32_t id;
        const auto it = out.seq.name_to_id.find(name);
        if (it != out.seq.name_to_id.end()) id = it->second;
        else {
          id = (uint32_t)out.seq.names.size();
          out.seq.name_to_id.emplace(name, id);
          out.seq.names.push_back(name);
          out.seq.lens.push_back(u.seq_len);
          table_add(T, name, hash_bits);
          added = true;
        }
        occ.push_back(u.occ);
        ids.push_back(id);
      }
      if (added) B.table(T);
      out.resolve_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      uint64_t n_ops = 0;
      const uint32_t err = B.piece_end(occ, ids, n_ops, out.stats[POOL_REGROWS]);
      if (err) throw Error{IMPG_E_INVALID, std::string("Failed to parse PAF: ") + line_err_text(err)};
      out.stats[PIECES]++;
      out.stats[TEXT_BYTES] += p.n;
      out.stats[LINES] += n_lines;
      out.stats[UNKNOWN_NAMES] += list.size();
      out.n_records += n_lines;
      out.n_ops += n_ops;
      w ^= 1;
      p = q;
    }
  }
  out.file_first.push_back(out.n_records);
  B.end();
}

// ---- the host twin of the kernels: the same phases over the same arrays ------------------------------------------------------
void HostBackend::begin(size_t buffer_bytes, uint64_t pool_ops, unsigned hb) {
  for (auto &b : buf) b.assign(buffer_bytes, 0);
  pool_cap = (size_t)pool_ops;
  hash_bits = hb;
  records.clear();
  ops.clear();
}
void HostBackend::grow(size_t buffer_bytes, int, size_t) {
  for (auto &b : buf) b.resize(buffer_bytes);
  if (cur) cur = buf[cur_which].data();  // (the piece in flight stays where the kernels' copy of it would be: readable)
}
void HostBackend::piece_begin(int which, size_t n) {
  const char *t = cur = buf[which].data();
  cur_which = which;
  cur_n = n;
  // scan
  line_start.assign(1, 0u);
  for (size_t i = 0; i < n; i++)
    if (t[i] == '\n') line_start.push_back((uint32_t)i + 1u);
  if (t[n - 1] != '\n') line_start.push_back((uint32_t)n + 1u);
  const size_t L = line_start.size() - 1;
  // heads
  heads.resize(L);
  cg_at.assign(L, NONE);
  cg_end.resize(L);
  for (size_t l = 0; l < L; l++) {
    heads[l] = line_head(t, line_start[l], line_start[l + 1] - 1u);
    cg_end[l] = heads[l].end;
  }
  // the tag
  uint32_t line = 0;
  for (size_t p = 0; p < n; p++) {
    const bool field_start = p == 0 || t[p - 1] == '\n' || t[p - 1] == '\t';
    if (field_start && p + 5 <= heads[line].end && memcmp(t + p, "cg:Z:", 5) == 0) cg_at[line] = std::min(cg_at[line], (uint32_t)p);
    if (t[p] == '\n') line++;
  }
  line = 0;
  for (size_t p = 0; p < n; p++) {
    if (t[p] == '\t' && cg_at[line] != NONE && p > cg_at[line]) cg_end[line] = std::min(cg_end[line], (uint32_t)p);
    if (t[p] == '\n') line++;
  }
  // names
  const TableView V{T.cap, T.slot.data(), T.hash.data(), T.off.data(), T.pool.data()};
  ids.assign(2 * L, NONE);
  for (size_t o = 0; o < 2 * L; o++) {
    const Head &h = heads[o >> 1];
    if (h.err) continue;
    const char *nm = t + h.name_at[o & 1];
    ids[o] = table_find(V, nm, h.name_len[o & 1], name_hash(nm, h.name_len[o & 1], hash_bits));
  }
}
void HostBackend::piece_unknowns(uint32_t &n_lines, std::vector<Unknown> &list, std::string &bytes) {
  n_lines = (uint32_t)heads.size();
  list.clear();
  bytes.clear();
  for (size_t o = 0; o < ids.size(); o++) {
    const Head &h = heads[o >> 1];
    if (h.err || ids[o] != NONE) continue;
    list.push_back(Unknown{(uint32_t)o, h.name_len[o & 1], bytes.size(), (int64_t)h.len[o & 1]});
    bytes.append(cur + h.name_at[o & 1], h.name_len[o & 1]);
  }
}
uint32_t HostBackend::piece_end(const std::vector<uint32_t> &occ, const std::vector<uint32_t> &id, uint64_t &n_ops, uint64_t &pool_regrows) {
  for (size_t k = 0; k < occ.size(); k++)
    if (occ[k] < ids.size()) ids[occ[k]] = id[k];
  size_t L = heads.size(), first_bad = L;
  for (size_t l = 0; l < L && first_bad == L; l++)
    if (heads[l].err) first_bad = l;
  // cigars: the lines in front of the first bad head (their checks come first in file order)
  std::vector<uint32_t> got;
  std::vector<uint32_t> cnt(first_bad, 0u);
  bool bad = false;
  for (size_t l = 0; l < first_bad; l++) {
    if (cg_at[l] == NONE) continue;
    const char *s = cur + cg_at[l] + 5u;
    const uint32_t n = cg_end[l] - (cg_at[l] + 5u);
    uint32_t len = 0;
    for (uint32_t i = 0; i < n; i++) {
      const unsigned c = (unsigned char)s[i], d = c - (unsigned)'0';
      if (d <= 9u) { len = len * 10u + d; continue; }
      const uint32_t code = c == '=' ? 0u : c == 'X' ? 1u : c == 'I' ? 2u : c == 'D' ? 3u : c == 'M' ? 4u : 7u;
      if (code == 7u) bad = true;
      got.push_back((code << 29) | len);
      cnt[l]++;
      len = 0;
    }
  }
  if (bad) return LINE_CIGAR;
  if (first_bad < L) return heads[first_bad].err;
  if (ops.size() + got.size() > pool_cap) {
    while (ops.size() + got.size() > pool_cap) pool_cap = std::max<size_t>(pool_cap + pool_cap / 2, 64);
    pool_regrows++;
  }
  // records
  uint64_t at = ops.size();
  for (size_t l = 0; l < L; l++) {
    const Head &h = heads[l];
    if (ids[2 * l] == NONE || ids[2 * l + 1] == NONE) throw Error{IMPG_E_INVALID, "internal: a name without an id"};
    records.push_back(impg_gpu_record_t{ids[2 * l], ids[2 * l + 1], (int32_t)h.c[0], (int32_t)h.c[1], (int32_t)h.c[2], (int32_t)h.c[3], at, cnt[l], h.strand});
    at += cnt[l];
  }
  ops.insert(ops.end(), got.begin(), got.end());
  n_ops = got.size();
  return LINE_OK;
}

}  // namespace paf_ingest

namespace {
template <class T> T *malloc_copy(const T *src, size_t n) {
  T *p = (T *)malloc(std::max<size_t>(n, 1) * sizeof(T));
  if (!p) throw std::bad_alloc();
  if (n) memcpy(p, src, n * sizeof(T));
  return p;
}
}  // namespace

}  // namespace impg

using namespace impg;

extern "C" int impg_gpu_selftest_paf_ingest(const char *const *paths, size_t n_paths, uint64_t piece_bytes, int on_host, int device, unsigned hash_bits,
                                            uint64_t initial_pool_ops, impg_gpu_record_t **records, size_t *n_records, uint32_t **ops, size_t *n_ops,
                                            char **names, size_t *names_len, int64_t **lens, size_t *n_seq, uint64_t **file_first, uint64_t *stats) {
  IMPG_TRY
  if ((n_paths && !paths) || !records || !n_records || !ops || !n_ops || !names || !names_len || !lens || !n_seq || !file_first)
    throw Error{IMPG_E_INVALID, "null argument"};
  std::vector<std::string> p;
  for (size_t i = 0; i < n_paths; i++) {
    if (!paths[i]) throw Error{IMPG_E_INVALID, "null argument"};
    p.push_back(paths[i]);
  }
  paf_ingest::Loaded L;
  std::vector<impg_gpu_record_t> recs;
  std::vector<uint32_t> pool;
  if (on_host) {
    paf_ingest::HostBackend B;
    paf_ingest::load_files(B, p, (size_t)piece_bytes, hash_bits, initial_pool_ops, L);
    recs.swap(B.records);
    pool.swap(B.ops);
  } else {
    paf_ingest_selftest_device(p, (size_t)piece_bytes, device, hash_bits, initial_pool_ops, L, recs, pool);
    L.stats[paf_ingest::DEVICE] = 1;
  }
  std::string joined;
  for (size_t i = 0; i < L.seq.names.size(); i++) {
    if (i) joined.push_back('\n');
    joined += L.seq.names[i];
  }
  *records = malloc_copy(recs.data(), recs.size());
  *n_records = recs.size();
  *ops = malloc_copy(pool.data(), pool.size());
  *n_ops = pool.size();
  *names = malloc_copy(joined.data(), joined.size());
  *names_len = joined.size();
  *lens = malloc_copy(L.seq.lens.data(), L.seq.lens.size());
  *n_seq = L.seq.lens.size();
  *file_first = malloc_copy(L.file_first.data(), L.file_first.size());
  if (stats) for (int k = 0; k < paf_ingest::N_STATS; k++) stats[k] = L.stats[k];
  return IMPG_OK;
  IMPG_CATCH
}
