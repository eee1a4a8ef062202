// Sequence files straight into HBM, the host side (sequence_ingest.hpp): the reader that cuts a
// file's text into pieces -- plain files copied, gzip inflated as one stream, BGZF block by block on a few threads --, the
// driver that turns a piece's header bytes into names, places and the piece's record table, and the host twin of the
// kernels (ingest_piece_host), which serves the CPU tests and a stand-alone sanitizer program and is never a fallback.
// No HIP call in here, and the host never looks at a base outside the twin.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <thread>

#include "engine.hpp"
#include "sequence_ingest.hpp"

namespace impg {
namespace ingest {

namespace {

inline uint32_t le16(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le32(const unsigned char *p) { return le16(p) | (le16(p + 2) << 16); }
enum { PLAIN, GZIP, BGZF };
constexpr size_t BGZF_MAX = 65536;

// the BC subfield of the gzip member at m[o ..): its BSIZE and where the deflate data starts; false: no such member there
bool bgzf_header(const unsigned char *m, size_t sz, size_t o, uint32_t &bsize, size_t &data_at) {
  if (sz - o < 12 || m[o] != 0x1f || m[o + 1] != 0x8b || m[o + 2] != 8 || m[o + 3] != 4) return false;
  const size_t xlen = le16(m + o + 10);
  if (sz - o - 12 < xlen) return false;
  for (size_t p = o + 12, e = o + 12 + xlen; p + 4 <= e;) {
    const size_t slen = le16(m + p + 2);
    if (m[p] == 'B' && m[p + 1] == 'C' && slen == 2 && p + 6 <= e) {
      bsize = le16(m + p + 4);
      data_at = e;
      return true;
    }
    p += 4 + slen;
  }
  return false;
}

struct Block {  // one BGZF block's data and where its text goes
  const unsigned char *src;
  size_t n_src;
  unsigned char *dst;
  uint32_t isize, crc;
};
// raw deflate of exactly b.isize bytes; an empty string: done, else what went wrong.  Never writes beyond dst + isize.
const char *inflate_block(const Block &b) {
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  if (inflateInit2(&zs, -15) != Z_OK) return "zlib would not start";
  unsigned char none;
  zs.next_in = const_cast<unsigned char *>(b.src);
  zs.avail_in = (uInt)b.n_src;
  zs.next_out = b.isize ? b.dst : &none;
  zs.avail_out = b.isize ? b.isize : 1;
  const int rc = inflate(&zs, Z_FINISH);
  const uLong made = zs.total_out;
  inflateEnd(&zs);
  if (rc != Z_STREAM_END) return rc == Z_DATA_ERROR ? "inflate error" : "a block's data ends early or holds more than its ISIZE";
  if (made != b.isize) return "a block's length is not its ISIZE";
  if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), b.dst, b.isize) != b.crc && b.isize) return "CRC mismatch";
  if (!b.isize && b.crc != 0) return "CRC mismatch";
  return "";
}
// the blocks of one piece on min(16, hardware_concurrency) threads (never the machine's CPU count alone)
const char *inflate_blocks(const std::vector<Block> &blocks) {
  const unsigned hw = std::thread::hardware_concurrency();
  const size_t T = std::min<size_t>(std::min<size_t>(16, hw ? hw : 4), blocks.size());
  std::atomic<size_t> next{0};
  std::atomic<const char *> err{""};
  auto work = [&]() {
    for (size_t i; (i = next.fetch_add(1)) < blocks.size();) {
      const char *e = inflate_block(blocks[i]);
      if (*e) { err = e; next = blocks.size(); }
    }
  };
  if (T <= 1) work();
  else {
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; t++) th.emplace_back(work);
    for (auto &t : th) t.join();
  }
  return err.load();
}

}  // namespace

struct FileText::Z { z_stream zs; bool in_member = false; };

FileText::FileText(const std::string &path, uint64_t *inflated_blocks) : path_(path), blocks_(inflated_blocks) {
  const int fd = open(path.c_str(), O_RDONLY);
  if (fd < 0) throw Error{IMPG_E_IO, "No such file or directory: " + path};
  struct stat st;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { close(fd); throw Error{IMPG_E_IO, "not a readable file: " + path}; }
  sz_ = (size_t)st.st_size;
  if (sz_) {
    void *m = mmap(nullptr, sz_, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) throw Error{IMPG_E_IO, "Failed to map file '" + path + "'"};
    m_ = (const unsigned char *)m;
  } else close(fd);
  if (sz_ >= 2 && m_[0] == 0x1f && m_[1] == 0x8b) {
    uint32_t bsize;
    size_t data_at;
    kind_ = bgzf_header(m_, sz_, 0, bsize, data_at) ? BGZF : GZIP;
    if (kind_ == BGZF) bounce_.resize(BGZF_MAX);
    else {
      z_ = new Z;
      memset(&z_->zs, 0, sizeof z_->zs);
      if (inflateInit2(&z_->zs, 15 + 16) != Z_OK) { delete z_; z_ = nullptr; munmap((void *)m_, sz_); throw Error{IMPG_E_IO, "zlib would not start: " + path}; }
    }
  }
}
FileText::~FileText() {
  if (z_) { inflateEnd(&z_->zs); delete z_; }
  if (m_) munmap((void *)m_, sz_);
}

size_t FileText::next(char *dst, size_t cap) {
  if (kind_ == GZIP) return next_gzip(dst, cap);
  if (kind_ == BGZF) return next_bgzf(dst, cap);
  const size_t n = std::min(cap, sz_ - at_);
  if (n) memcpy(dst, m_ + at_, n);
  at_ += n;
  return n;
}

// one stream on one thread; a member's end with bytes behind it starts the next member (zlib checks every CRC and length)
size_t FileText::next_gzip(char *dst, size_t cap) {
  z_stream &zs = z_->zs;
  size_t made = 0;
  while (made < cap) {
    if (!zs.avail_in) {
      if (at_ == sz_) {
        if (z_->in_member) throw Error{IMPG_E_IO, "Failed to decompress '" + path_ + "': the gzip stream is truncated"};
        break;
      }
      const size_t k = std::min<size_t>(sz_ - at_, 1u << 30);
      zs.next_in = const_cast<unsigned char *>(m_ + at_);
      zs.avail_in = (uInt)k;
      at_ += k;
    }
    z_->in_member = true;
    const size_t room = std::min<size_t>(cap - made, 1u << 30);
    zs.next_out = (unsigned char *)dst + made;
    zs.avail_out = (uInt)room;
    const int rc = inflate(&zs, Z_NO_FLUSH);
    made += room - zs.avail_out;
    if (rc == Z_STREAM_END) {
      z_->in_member = false;
      if (zs.avail_in || at_ < sz_) inflateReset(&zs);  // (keeps next_in / avail_in)
    } else if (rc == Z_BUF_ERROR && !zs.avail_in && at_ == sz_) {
      throw Error{IMPG_E_IO, "Failed to decompress '" + path_ + "': the gzip stream is truncated"};
    } else if (rc != Z_OK && rc != Z_BUF_ERROR) {
      throw Error{IMPG_E_IO, "Failed to decompress '" + path_ + "': " + (zs.msg ? zs.msg : "inflate error")};
    }
  }
  return made;
}

// BGZF: the chain walked by BSIZE, every block's text placed by its ISIZE -- straight into the piece where it fits, through
// the bounce buffer where it crosses the piece's end (what is left over opens the next piece)
size_t FileText::next_bgzf(char *dst, size_t cap) {
  size_t made = 0;
  std::vector<Block> blocks;
  auto bad = [&](const std::string &what) { return Error{IMPG_E_IO, "Failed to decompress '" + path_ + "': " + what}; };
  while (made < cap) {
    if (b_at_ < b_n_) {
      const size_t k = std::min(cap - made, b_n_ - b_at_);
      memcpy(dst + made, bounce_.data() + b_at_, k);
      b_at_ += k;
      made += k;
      continue;
    }
    if (at_ == sz_) break;
    uint32_t bsize;
    size_t data_at;
    if (!bgzf_header(m_, sz_, at_, bsize, data_at)) throw bad("a truncated or malformed BGZF block header");
    const size_t total = (size_t)bsize + 1;
    if (total > sz_ - at_) throw bad("a block's BSIZE leads outside the file");
    if (at_ + total < data_at + 8) throw bad("a block's BSIZE is smaller than its header");
    const unsigned char *tail = m_ + at_ + total - 8;
    Block b{m_ + data_at, at_ + total - 8 - data_at, nullptr, le32(tail + 4), le32(tail)};
    if (b.isize > BGZF_MAX) throw bad("a block's ISIZE is beyond 64 KiB");
    at_ += total;
    if (blocks_) ++*blocks_;
    if (b.isize <= cap - made) {
      b.dst = (unsigned char *)dst + made;
      made += b.isize;
      blocks.push_back(b);
    } else {
      b.dst = bounce_.data();
      const char *e = inflate_block(b);
      if (*e) throw bad(e);
      b_at_ = 0;
      b_n_ = b.isize;
    }
  }
  const char *e = inflate_blocks(blocks);
  if (*e) throw bad(e);
  return made;
}

size_t reserve_bytes(const std::vector<int64_t> &lens, bool packed) {
  uint64_t at = packed ? 64 : SEQ_PAD;
  for (const int64_t l : lens) {
    const uint64_t len = (uint64_t)std::max<int64_t>(l, 0);
    at += packed ? (len + 63u) & ~63ull : len;
  }
  return packed ? (size_t)(at / 4u) + 64 : (size_t)((at + 15u) & ~15ull) + 64;
}

void load_files(Backend &B, const std::vector<std::string> &paths, const std::vector<std::string> &name_of_id, const std::vector<int64_t> &lens,
                size_t piece_bytes, bool packed, Loaded &out) {
  const size_t n_ids = lens.size();
  if (piece_bytes < 16 || piece_bytes > (1ull << 32) || piece_bytes % 16) throw Error{IMPG_E_INVALID, "sequence_ingest_piece_bytes is 16 .. 2^32, a multiple of 16"};
  for (const int64_t l : lens)
    if (l > 0xFFFFFFFFll) throw Error{IMPG_E_UNSUPPORTED, "a sequence of 2^32 bases or more"};
  std::unordered_map<std::string, uint32_t> id_of, by_name;
  for (size_t id = 0; id < n_ids; id++) id_of.emplace(name_of_id[id], (uint32_t)id);
  out = Loaded();
  out.packed = packed;
  out.store_of_id.assign(n_ids, SEQ_ABSENT);
  out.off.assign(std::max<size_t>(n_ids, 1), SEQ_NOT_IN_HBM);
  out.plan = PackedPlan(n_ids);
  std::vector<std::vector<SeqRun>> runs_of_id(packed ? n_ids : 0);
  uint64_t at = SEQ_PAD;  // byte form: the next place
  B.begin(piece_bytes, reserve_bytes(lens, packed), packed);

  struct Open { uint64_t dest = NO_PLACE, before = 0; uint32_t len = 0, seq = SEQ_ABSENT, id = SEQ_ABSENT; } open;
  std::vector<Rec> recs;
  std::vector<uint32_t> rec_id;
  std::vector<PieceRun> runs;
  for (const std::string &path : paths) {
    FileText f(path, &out.stats[INFLATED_BLOCKS]);
    B.file_start();
    open = Open();
    bool is_open = false, pending_on = false;
    std::string pending;
    // a complete header line: its name, the sequence's place; the record it opens has had no base yet
    auto resolve = [&](const char *line, size_t n) {
      size_t j = 1;
      while (j < n && line[j] != ' ' && line[j] != '\t' && line[j] != '\r' && line[j] != '\v' && line[j] != '\f') j++;
      const std::string name(line + 1, j - 1);
      if (name.empty()) throw Error{IMPG_E_INVALID, "a '>' line without a name in " + path};
      if (!by_name.emplace(name, (uint32_t)out.names.size()).second) throw Error{IMPG_E_INVALID, "sequence '" + name + "' occurs twice in the sequence files"};
      open = Open();
      open.seq = (uint32_t)out.names.size();
      out.names.push_back(name);
      out.counts.push_back(0);
      const auto it = id_of.find(name);
      if (it == id_of.end()) { out.stats[DROPPED_SEQUENCES]++; return; }
      open.id = it->second;
      open.len = (uint32_t)std::max<int64_t>(lens[open.id], 0);
      out.store_of_id[open.id] = open.seq;
      if (packed) {
        open.dest = out.plan.off[open.id] = out.plan.end;
        out.plan.end += ((uint64_t)open.len + 63u) & ~63ull;
      } else {
        open.dest = out.off[open.id] = at;
        at += open.len;
      }
    };
    auto close_open = [&](uint64_t bases) {
      if (is_open && open.seq != SEQ_ABSENT) out.counts[open.seq] = open.before + bases;
    };
    int which = 0;
    double read_s = 0;
    auto read_next = [&](char *dst) {
      const auto t0 = std::chrono::steady_clock::now();
      const size_t k = f.next(dst, piece_bytes);
      read_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      return k;
    };
    size_t n = read_next(B.buffer(0));
    while (n) {
      B.scan_begin(which, n);
      const size_t n_next = read_next(B.buffer(which ^ 1));
      PieceScan sc;
      B.scan_end(sc);
      out.stats[PIECES]++;
      out.stats[TEXT_BYTES] += n;
      out.stats[BASES] += sc.n_bases;
      if (sc.text_before_head) throw Error{IMPG_E_INVALID, "not a FASTA file (text before the first '>' line): " + path};
      if (sc.head_rank.size() != sc.n_heads) throw Error{IMPG_E_INVALID, "internal: sequence ingest lost a record head"};
      const char *h = sc.header.data();
      const size_t hn = sc.header.size();
      size_t p = 0;
      if (pending_on) {  // the header line that crossed the piece's edge
        const char *e = (const char *)memchr(h, '\n', hn);
        pending.append(h, e ? (size_t)(e - h) : hn);
        p = e ? (size_t)(e - h) + 1 : hn;
        if (e) { resolve(pending.data(), pending.size()); pending_on = false; }
      }
      recs.clear();
      rec_id.clear();
      recs.push_back(Rec{is_open && !pending_on ? open.dest : NO_PLACE, open.before, 0u, open.len});
      rec_id.push_back(open.id);
      uint32_t first_rank = 0;
      for (size_t j = 0; j < sc.n_heads; j++) {
        if (pending_on || p >= hn || h[p] != '>') throw Error{IMPG_E_INVALID, "internal: sequence ingest's header bytes and heads disagree"};
        close_open(sc.head_rank[j] - first_rank);
        first_rank = sc.head_rank[j];
        is_open = true;
        const char *e = (const char *)memchr(h + p, '\n', hn - p);
        if (e) {
          resolve(h + p, (size_t)(e - (h + p)));
          p = (size_t)(e - h) + 1;
        } else {
          pending.assign(h + p, hn - p);
          pending_on = true;
          open = Open();
          p = hn;
        }
        recs.push_back(Rec{open.dest, 0, first_rank, open.len});
        rec_id.push_back(open.id);
      }
      if (p != hn) throw Error{IMPG_E_INVALID, "internal: sequence ingest's header bytes and heads disagree"};
      open.before += sc.n_bases - first_rank;
      if (sc.n_bases) {
        runs.clear();
        B.place(recs.data(), (uint32_t)recs.size(), runs);
        for (const PieceRun &r : runs) {  // a run that continues across a piece's edge: same sequence, same byte, contiguous
          if (r.rec >= rec_id.size() || rec_id[r.rec] == SEQ_ABSENT || !packed) throw Error{IMPG_E_INVALID, "internal: a run outside the piece's records"};
          std::vector<SeqRun> &v = runs_of_id[rec_id[r.rec]];
          if (!v.empty() && v.back().end == r.start && v.back().byte == r.byte) v.back().end = r.end;
          else v.push_back(SeqRun{r.start, r.end, r.byte});
        }
      }
      which ^= 1;
      n = n_next;
    }
    out.read_seconds += read_s;
    if (pending_on) resolve(pending.data(), pending.size());  // a last line without a newline that is a header
    close_open(0);
  }
  B.end();
  for (size_t id = 0; id < n_ids; id++) {
    const uint32_t s = out.store_of_id[id];
    if (s != SEQ_ABSENT && (int64_t)out.counts[s] != lens[id])
      throw Error{IMPG_E_INVALID, "sequence '" + name_of_id[id] + "' has " + std::to_string(out.counts[s]) + " bases in the sequence files and " +
                                      std::to_string(lens[id]) + " in the index"};
  }
  if (packed) {
    static const std::vector<SeqRun> none;
    for (size_t id = 0; id < n_ids; id++) out.plan.add_runs(id, (uint64_t)std::max<int64_t>(lens[id], 0), out.store_of_id[id] == SEQ_ABSENT ? none : runs_of_id[id]);
    out.store_bytes = out.plan.bytes();
  } else out.store_bytes = (size_t)((at + 15u) & ~15ull) + 64;
}

}  // namespace ingest

// ---- the host twin of the kernels: one piece, the same carry, the same outputs ---------------------------------------------
// scan: t[0 .. n) under carry c -> out, and the successor state in c
void ingest_piece_host(const char *t, size_t n, ingest::Carry &c, ingest::PieceScan &out) {
  bool hdr = c.in_header != 0, start = c.at_line_start != 0;
  out = ingest::PieceScan();
  for (size_t i = 0; i < n; i++) {
    const char ch = t[i];
    if (start) hdr = ch == '>';
    if (start && hdr) out.head_rank.push_back((uint32_t)out.n_bases);
    if (hdr) out.header.push_back(ch);
    else if (ch != '\n' && ch != '\r') {
      if (!c.open && out.head_rank.empty()) out.text_before_head = true;
      out.n_bases++;
    }
    start = ch == '\n';
  }
  out.n_heads = out.head_rank.size();
  c = ingest::Carry{(uint32_t)(hdr && !start), (uint32_t)start, (uint32_t)(c.open || out.n_heads), 0u};
}
// place: the same piece under the carry it was scanned with; store: the byte form's bytes or the packed form's stream
void ingest_piece_host(const char *t, size_t n, const ingest::Carry &c, const ingest::Rec *recs, uint32_t n_recs, bool packed, unsigned char *store,
                       size_t store_bytes, std::vector<ingest::PieceRun> &runs) {
  bool hdr = c.in_header != 0, start = c.at_line_start != 0;
  uint32_t rec = 0, rank = 0;
  ingest::PieceRun cur{0, 0, 0, 0};
  bool in_run = false;
  auto flush = [&]() { if (in_run) runs.push_back(cur); in_run = false; };
  for (size_t i = 0; i < n; i++) {
    unsigned char ch = (unsigned char)t[i];
    if (start) hdr = ch == '>';
    if (start && hdr) rec++;
    start = ch == '\n';
    if (hdr || ch == '\n' || ch == '\r') continue;
    const uint32_t r = rank++;
    if (rec >= n_recs) continue;
    const ingest::Rec &R = recs[rec];
    const uint64_t pos = (uint64_t)(r - R.first_rank) + R.before;
    if (R.dest == ingest::NO_PLACE || pos >= R.len) continue;  // counted, never written
    if (ch >= 'a' && ch <= 'z') ch = (unsigned char)(ch - 'a' + 'A');
    const uint64_t P = R.dest + pos;
    if (!packed) {
      if (P < store_bytes) store[P] = ch;
      continue;
    }
    const unsigned code = ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 0u;
    if (P / 4 < store_bytes) store[P / 4] |= (unsigned char)(code << (2u * (P & 3u)));
    if (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T') { flush(); continue; }
    if (in_run && cur.rec == rec && cur.byte == ch && cur.end == pos) cur.end = (uint32_t)pos + 1;
    else {
      flush();
      cur = ingest::PieceRun{rec, (uint32_t)pos, (uint32_t)pos + 1, ch};
      in_run = true;
    }
  }
  flush();
}

namespace {
struct HostBackend : ingest::Backend {
  std::vector<char> buf[2];
  std::vector<unsigned char> store;
  bool packed = false;
  ingest::Carry carry{}, scanned_with{};
  const char *cur = nullptr;
  size_t cur_n = 0;
  void begin(size_t piece_bytes, size_t store_bytes, bool p) override {
    for (auto &b : buf) b.resize(piece_bytes);
    store.assign(store_bytes, 0);
    packed = p;
  }
  char *buffer(int which) override { return buf[which].data(); }
  void file_start() override { carry = ingest::Carry{0, 1, 0, 0}; }
  void scan_begin(int which, size_t n) override { cur = buf[which].data(); cur_n = n; }
  void scan_end(ingest::PieceScan &out) override {
    scanned_with = carry;
    ingest_piece_host(cur, cur_n, carry, out);
  }
  void place(const ingest::Rec *recs, uint32_t n_recs, std::vector<ingest::PieceRun> &runs) override {
    ingest_piece_host(cur, cur_n, scanned_with, recs, n_recs, packed, store.data(), store.size(), runs);
  }
  void end() override {}
};
template <class T> T *malloc_copy(const T *src, size_t n) {
  T *p = (T *)malloc(std::max<size_t>(n, 1) * sizeof(T));
  if (!p) throw std::bad_alloc();
  if (n) memcpy(p, src, n * sizeof(T));
  return p;
}
}  // namespace

}  // namespace impg

using namespace impg;

extern "C" {

int impg_gpu_selftest_sequence_reader(const char *path, uint64_t piece_bytes, char **text, size_t *len, uint64_t *n_pieces, uint64_t *inflated_blocks) {
  IMPG_TRY
  if (!path || !text || !len || !n_pieces || !inflated_blocks) throw Error{IMPG_E_INVALID, "null argument"};
  if (piece_bytes < 16 || piece_bytes > (1ull << 32) || piece_bytes % 16) throw Error{IMPG_E_INVALID, "sequence_ingest_piece_bytes is 16 .. 2^32, a multiple of 16"};
  *n_pieces = *inflated_blocks = 0;
  ingest::FileText f(path, inflated_blocks);
  std::vector<char> piece((size_t)piece_bytes);
  std::string all;
  for (size_t n; (n = f.next(piece.data(), piece.size())) > 0; ++*n_pieces) {
    if (n < piece.size() && f.next(piece.data() + n, piece.size() - n)) throw Error{IMPG_E_INVALID, "internal: a short piece before the text's end"};
    all.append(piece.data(), n);
  }
  *text = malloc_copy(all.data(), all.size());
  *len = all.size();
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_selftest_sequence_ingest_host(const char *const *paths, size_t n_paths, const char *const *names_of_ids, const int64_t *lens, size_t n_ids,
                                           uint64_t piece_bytes, int packed, uint64_t *off, uint8_t **store, size_t *store_bytes, uint64_t *run_off,
                                           uint32_t **run_start, uint32_t **run_end, uint8_t **run_byte, uint64_t *stats) {
  IMPG_TRY
  if ((n_paths && !paths) || (n_ids && (!names_of_ids || !lens || !off)) || !store || !store_bytes || !run_off || !run_start || !run_end || !run_byte)
    throw Error{IMPG_E_INVALID, "null argument"};
  if (packed != 0 && packed != 1) throw Error{IMPG_E_INVALID, "the store's form is 0 (a byte per base) or 1 (packed)"};
  std::vector<std::string> p, names;
  for (size_t i = 0; i < n_paths; i++) {
    if (!paths[i]) throw Error{IMPG_E_INVALID, "null argument"};
    p.push_back(paths[i]);
  }
  for (size_t i = 0; i < n_ids; i++) names.push_back(names_of_ids[i] ? names_of_ids[i] : std::to_string(i));
  HostBackend B;
  ingest::Loaded L;
  ingest::load_files(B, p, names, std::vector<int64_t>(lens, lens + n_ids), (size_t)piece_bytes, packed != 0, L);
  for (size_t id = 0; id < n_ids; id++) off[id] = packed ? L.plan.off[id] : L.off[id];
  std::vector<uint32_t> s, e;
  for (const uint2 &r : L.plan.runs) { s.push_back(r.x); e.push_back(r.y); }
  for (size_t id = 0; id <= n_ids; id++) run_off[id] = L.plan.run_off[id];
  const size_t used = packed ? L.plan.stream_bytes() : L.store_bytes;
  *store = malloc_copy(B.store.data(), std::min(used, B.store.size()));
  *store_bytes = std::min(used, B.store.size());
  *run_start = malloc_copy(s.data(), s.size());
  *run_end = malloc_copy(e.data(), e.size());
  *run_byte = malloc_copy(L.plan.run_byte.data(), L.plan.run_byte.size());
  if (stats) for (int k = 0; k < ingest::N_STATS; k++) stats[k] = L.stats[k];
  return IMPG_OK;
  IMPG_CATCH
}

}  // extern "C"
