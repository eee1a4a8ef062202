// The sequences FASTA output prints: the store (plain FASTA files or arrays of the caller's -> one byte per base, upper
// case), its attachment to an index handle, and the host side of output_results_fasta (main.rs:12351-12415): the
// query-axis sweep with the strands kept apart, then per merged row ">{name}:{start}-{end}[/rc]" and the bases in lines of
// 80.  fasta_device.hip writes the same records in HBM; the parity tests compare both with a restatement of the reference.
#include <cstdio>
#include <thread>

#include "engine.hpp"

struct impg_gpu_sequences {
  std::shared_ptr<impg::SeqStore> s = std::make_shared<impg::SeqStore>();
};

namespace impg {

const SeqStore &store_of(const impg_gpu_sequences_t *seqs) { return *seqs->s; }

void SeqStore::add(const std::string &name, const char *b, size_t n) {
  if (name.empty()) throw Error{IMPG_E_INVALID, "a sequence without a name"};
  if (!by_name.emplace(name, (uint32_t)names.size()).second) throw Error{IMPG_E_INVALID, "sequence '" + name + "' occurs twice in the sequence files"};
  if (off.empty()) off.push_back(0);
  names.push_back(name);
  const size_t at = bases.size();
  bases.append(b, n);
  for (size_t i = at; i < bases.size(); i++) {
    const char c = bases[i];
    if (c >= 'a' && c <= 'z') bases[i] = (char)(c - 'a' + 'A');
  }
  off.push_back(bases.size());
}

void seq_exception_runs(const char *bases, size_t n, std::vector<SeqRun> &runs) {
  for (size_t i = 0; i < n;) {
    const char c = bases[i];
    if (c == 'A' || c == 'C' || c == 'G' || c == 'T') { i++; continue; }
    size_t j = i + 1;
    while (j < n && bases[j] == c) j++;
    runs.push_back(SeqRun{(uint32_t)i, (uint32_t)j, (uint8_t)c});
    i = j;
  }
}

namespace {

// One plain FASTA file into the store: the name runs to the first whitespace of the '>' line, body lines of any length,
// '\r' dropped, an empty sequence allowed, a last line without a newline accepted.
void parse_fasta(SeqStore &st, const std::string &path) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) throw Error{IMPG_E_IO, "No such file or directory: " + path};
  std::string text;
  char buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, k);
  const bool bad = ferror(f) != 0;
  fclose(f);
  if (bad) throw Error{IMPG_E_IO, "read failed: " + path};
  if (text.size() >= 2 && (unsigned char)text[0] == 0x1f && (unsigned char)text[1] == 0x8b)
    throw Error{IMPG_E_UNSUPPORTED, "compressed sequence file (gzip / bgzip) -- decompress it first: " + path};
  std::string name, body;
  bool open = false;
  auto close = [&]() {
    if (open) st.add(name, body.data(), body.size());
    body.clear();
  };
  size_t i = 0;
  const size_t n = text.size();
  while (i < n) {
    size_t e = text.find('\n', i);
    if (e == std::string::npos) e = n;
    if (text[i] == '>') {
      close();
      size_t j = i + 1;
      while (j < e && text[j] != ' ' && text[j] != '\t' && text[j] != '\r' && text[j] != '\v' && text[j] != '\f') j++;
      name.assign(text, i + 1, j - (i + 1));
      if (name.empty()) throw Error{IMPG_E_INVALID, "a '>' line without a name in " + path};
      open = true;
    } else {
      for (size_t j = i; j < e; j++) {
        if (text[j] == '\r') continue;
        if (!open) throw Error{IMPG_E_INVALID, "not a FASTA file (text before the first '>' line): " + path};
        body.push_back(text[j]);
      }
    }
    i = e + 1;
  }
  close();
}

inline char complement(char c) {  // graph.rs:814-828: A/T/C/G/N, every other byte as it is
  switch (c) {
    case 'A': return 'T';
    case 'T': return 'A';
    case 'C': return 'G';
    case 'G': return 'C';
    default: return c;
  }
}

}  // namespace

void fasta_range_text(std::vector<impg_gpu_interval_t> &rows, int32_t merge_distance, bool reverse_complement,
                      const std::function<bool(uint32_t, std::string &, SeqRef &)> &fetch, std::string &text) {
  query_axis_merge(rows, merge_distance, /*merge_strands=*/false);  // merge_strands_for_output("fasta") (main.rs:4395-4409)
  std::string name, rc;
  char buf[64];
  for (const impg_gpu_interval_t &x : rows) {
    const bool fwd = x.q_first <= x.q_last;
    const int32_t start = fwd ? x.q_first : x.q_last, end = fwd ? x.q_last : x.q_first;
    SeqRef ref{nullptr, 0};
    name.clear();
    if (!fetch(x.query_id, name, ref)) throw Error{IMPG_E_INVALID, "Sequence '" + name + "' not found in the sequence store"};
    if (start < 0 || (uint64_t)end > ref.len)
      throw Error{IMPG_E_INVALID, "row " + name + ":" + std::to_string(start) + "-" + std::to_string(end) + " leaves its sequence of " +
                                      std::to_string(ref.len) + " bases"};
    const bool flip = !fwd && reverse_complement;
    text += '>';
    text += name;
    const int k = snprintf(buf, sizeof buf, ":%u-%u%s\n", (uint32_t)start, (uint32_t)end, flip ? "/rc" : "");
    text.append(buf, (size_t)k);
    const size_t L = (size_t)(end - start);
    const char *b = ref.bases + start;
    if (flip) {
      rc.resize(L);
      for (size_t i = 0; i < L; i++) rc[i] = complement(b[L - 1 - i]);
      b = rc.data();
    }
    for (size_t at = 0; at < L; at += 80) {
      text.append(b + at, std::min<size_t>(80, L - at));
      text += '\n';
    }
    if (!L) text += '\n';  // (header, empty line: the reference's answer here rests on htslib and is not pinned)
  }
}

void partition_fasta_text(const impg_gpu_partition_row_t *rows, size_t n, const std::function<bool(uint32_t, std::string &, SeqRef &)> &fetch,
                          std::string &text) {
  std::string name;
  std::vector<SeqRef> refs(n, SeqRef{nullptr, 0});
  size_t bytes = 0;
  for (int pass = 0; pass < 2; pass++)  // as the device route marks them: a sequence the store lacks first, then a row that leaves its own
    for (size_t i = 0; i < n; i++) {
      const impg_gpu_partition_row_t &x = rows[i];
      name.clear();
      const bool have = fetch(x.seq_id, name, refs[i]);
      if (pass == 0) {
        if (!have) throw Error{IMPG_E_INVALID, "Sequence '" + name + "' not found in the sequence store"};
        continue;
      }
      if (x.start < 0 || x.end < x.start || (uint64_t)x.end > refs[i].len)
        throw Error{IMPG_E_INVALID, "row " + name + ":" + std::to_string(x.start) + "-" + std::to_string(x.end) + " leaves its sequence of " +
                                        std::to_string(refs[i].len) + " bases"};
      const size_t L = (size_t)(x.end - x.start);
      bytes += name.size() + 32 + L + (L + 79) / 80;
    }
  text.reserve(text.size() + bytes);
  char buf[64];
  for (size_t i = 0; i < n; i++) {
    const impg_gpu_partition_row_t &x = rows[i];
    name.clear();
    fetch(x.seq_id, name, refs[i]);
    text += '>';
    text += name;
    const int k = snprintf(buf, sizeof buf, ":%u-%u\n", (uint32_t)x.start, (uint32_t)x.end);
    text.append(buf, (size_t)k);
    const size_t L = (size_t)(x.end - x.start);
    const char *b = refs[i].bases + x.start;
    for (size_t at = 0; at < L; at += 80) {  // (chunks(80) of nothing: a record of no bases is its header alone, partition.rs:1672-1676)
      text.append(b + at, std::min<size_t>(80, L - at));
      text += '\n';
    }
  }
}

}  // namespace impg

using namespace impg;

void impg_gpu_index::drop_device_sequences() {
  for (DevBuf *d : {&d_seq_bases, &d_seq_off, &d_seq_run_off, &d_seq_runs, &d_seq_run_byte, &d_seq_blk_off, &d_seq_blk}) d->release();
  seq_packed = false;
  for (int k : {FASTA_STORE_BYTES, FASTA_STORE_PACKED, FASTA_STORE_EXCEPTION_RUNS}) fasta_stats[k] = 0;
}

extern "C" {

int impg_gpu_sequences_from_fasta(const char *const *paths, size_t n_paths, impg_gpu_sequences_t **out) {
  IMPG_TRY
  if (!out || (n_paths && !paths)) throw Error{IMPG_E_INVALID, "null argument"};
  std::unique_ptr<impg_gpu_sequences> h(new impg_gpu_sequences);
  h->s->off.assign(1, 0);
  for (size_t i = 0; i < n_paths; i++) {
    if (!paths[i]) throw Error{IMPG_E_INVALID, "null argument"};
    parse_fasta(*h->s, paths[i]);
  }
  *out = h.release();
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_sequences_from_memory(const char *const *names, const uint64_t *off, const char *bases, size_t n, impg_gpu_sequences_t **out) {
  IMPG_TRY
  if (!out || !off || (n && !names) || (n && off[n] && !bases)) throw Error{IMPG_E_INVALID, "null argument"};
  if (off[0] != 0) throw Error{IMPG_E_INVALID, "sequence offsets start at 0"};
  std::unique_ptr<impg_gpu_sequences> h(new impg_gpu_sequences);
  h->s->off.assign(1, 0);
  for (size_t i = 0; i < n; i++) {
    if (!names[i]) throw Error{IMPG_E_INVALID, "null argument"};
    if (off[i + 1] < off[i]) throw Error{IMPG_E_INVALID, "sequence offsets must not decrease"};
    h->s->add(names[i], bases + off[i], (size_t)(off[i + 1] - off[i]));
  }
  *out = h.release();
  return IMPG_OK;
  IMPG_CATCH
}

size_t impg_gpu_sequences_num(const impg_gpu_sequences_t *s) { return s ? s->s->names.size() : 0; }

const char *impg_gpu_sequences_name(const impg_gpu_sequences_t *s, size_t i) { return s && i < s->s->names.size() ? s->s->names[i].c_str() : nullptr; }

const char *impg_gpu_sequences_bases(const impg_gpu_sequences_t *s, size_t i, uint64_t *len) {
  if (!s || i >= s->s->names.size()) return nullptr;
  if (len) *len = s->s->off[i + 1] - s->s->off[i];
  return s->s->bases.data() + s->s->off[i];
}

int impg_gpu_sequences_exceptions(const impg_gpu_sequences_t *s, size_t i, uint32_t *start, uint32_t *len, uint8_t *byte, size_t cap, size_t *n_runs) {
  IMPG_TRY
  if (!s || !n_runs || (cap && (!start || !len || !byte))) throw Error{IMPG_E_INVALID, "null argument"};
  if (i >= s->s->names.size()) throw Error{IMPG_E_INVALID, "no such sequence in the store"};
  const uint64_t n = s->s->off[i + 1] - s->s->off[i];
  if (n > 0xFFFFFFFFull) throw Error{IMPG_E_UNSUPPORTED, "a sequence of 2^32 bases or more"};
  std::vector<SeqRun> runs;
  seq_exception_runs(s->s->bases.data() + s->s->off[i], (size_t)n, runs);
  for (size_t k = 0; k < runs.size() && k < cap; k++) {
    start[k] = runs[k].start;
    len[k] = runs[k].end - runs[k].start;
    byte[k] = runs[k].byte;
  }
  *n_runs = runs.size();
  return IMPG_OK;
  IMPG_CATCH
}

void impg_gpu_sequences_free(impg_gpu_sequences_t *s) { delete s; }

int impg_gpu_index_set_sequences(impg_gpu_index_t *ix, const impg_gpu_sequences_t *seqs) {
  IMPG_TRY
  if (!ix) throw Error{IMPG_E_INVALID, "null argument"};
  if (ix->shard || ix->cluster) throw Error{IMPG_E_UNSUPPORTED, "a sequence store on a sharded index"};
  IMPG_HIP(hipSetDevice(ix->device));
  for (auto &c : ix->ingest_stats) c = 0;  // (the attached store is no longer one impg_gpu_index_load_sequences made)
  if (!seqs) {
    ix->seq_store.reset();
    ix->store_of_id.clear();
    ix->drop_device_sequences();
    return IMPG_OK;
  }
  if (ix->tp_mode) throw Error{IMPG_E_UNSUPPORTED, "a sequence store on a tracepoint index (it has no sequence names)"};
  const SeqStore &st = *seqs->s;
  // (an index built from bare records has no names: its sequences print as their ids, and are matched as they print)
  std::vector<uint32_t> of(ix->seq.lens.size(), SEQ_ABSENT);
  for (size_t id = 0; id < of.size(); id++) {
    const std::string name = id < ix->seq.names.size() ? ix->seq.names[id] : std::to_string(id);
    const auto it = st.by_name.find(name);
    if (it == st.by_name.end()) continue;
    const uint64_t len = st.off[it->second + 1] - st.off[it->second];
    if ((int64_t)len != ix->seq.lens[id])
      throw Error{IMPG_E_INVALID, "sequence '" + name + "' has " + std::to_string(len) + " bases in the sequence files and " +
                                      std::to_string(ix->seq.lens[id]) + " in the index"};
    of[id] = it->second;
  }
  ix->seq_store = seqs->s;
  ix->store_of_id.swap(of);
  try {
    upload_sequences(*ix);
  } catch (...) {
    ix->seq_store.reset();
    ix->store_of_id.clear();
    ix->drop_device_sequences();
    throw;
  }
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_fasta_text(const impg_gpu_sequences_t *seqs, const char *const *names_of_ids, size_t n_ids, const impg_gpu_interval_t *rows, size_t n,
                        int32_t merge_distance, int reverse_complement, char **text, size_t *len) {
  IMPG_TRY
  if (!seqs || !text || !len || (n && !rows) || (n_ids && !names_of_ids)) throw Error{IMPG_E_INVALID, "null argument"};
  const SeqStore &st = *seqs->s;
  std::vector<impg_gpu_interval_t> v(rows, rows + n);
  std::string out;
  fasta_range_text(v, merge_distance, reverse_complement != 0, [&](uint32_t id, std::string &name, SeqRef &ref) {
    if (id >= n_ids || !names_of_ids[id]) { name = std::to_string(id); return false; }
    name = names_of_ids[id];
    const auto it = st.by_name.find(name);
    if (it == st.by_name.end()) return false;
    ref = SeqRef{st.bases.data() + st.off[it->second], st.off[it->second + 1] - st.off[it->second]};
    return true;
  }, out);
  char *t = (char *)malloc(out.size() + 1);
  if (!t) throw Error{IMPG_E_OOM, "host out of memory"};
  memcpy(t, out.data(), out.size());
  t[out.size()] = 0;
  *text = t;
  *len = out.size();
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_partition_fasta_text(const impg_gpu_sequences_t *seqs, const char *const *names_of_ids, size_t n_ids,
                                  const impg_gpu_partition_row_t *rows, size_t n, char **text, size_t *len) {
  IMPG_TRY
  if (!seqs || !text || !len || (n && !rows) || (n_ids && !names_of_ids)) throw Error{IMPG_E_INVALID, "null argument"};
  const SeqStore &st = *seqs->s;
  std::string out;
  partition_fasta_text(rows, n, [&](uint32_t id, std::string &name, SeqRef &ref) {
    if (id >= n_ids || !names_of_ids[id]) { name = std::to_string(id); return false; }
    name = names_of_ids[id];
    const auto it = st.by_name.find(name);
    if (it == st.by_name.end()) return false;
    ref = SeqRef{st.bases.data() + st.off[it->second], st.off[it->second + 1] - st.off[it->second]};
    return true;
  }, out);
  char *t = (char *)malloc(out.size() + 1);
  if (!t) throw Error{IMPG_E_OOM, "host out of memory"};
  memcpy(t, out.data(), out.size());
  t[out.size()] = 0;
  *text = t;
  *len = out.size();
  return IMPG_OK;
  IMPG_CATCH
}

}  // extern "C"

namespace impg {

// output_results_fasta over every range of a result (impg_gpu_results_fasta), the ranges spread over the host's threads
void render_fasta(const impg_gpu_results &res, const impg_gpu_index &ix, const impg_gpu_params_t &p, int32_t merge_distance, bool reverse_complement,
                  std::vector<std::string> &parts) {
  if (!ix.seq_store) throw Error{IMPG_E_INVALID, "FASTA output needs a sequence store (impg_gpu_index_set_sequences)"};
  const SeqStore &st = host_copy(*ix.seq_store);
  const size_t nr = res.offsets.size() - 1;
  parts.assign(nr, std::string());
  std::atomic<size_t> next{0};
  std::mutex err_m;
  std::exception_ptr err;
  unsigned hw = std::thread::hardware_concurrency();
  const size_t T = std::max<size_t>(1, std::min<size_t>(hw ? hw : 4, nr / 16 + 1));
  auto fetch = [&](uint32_t id, std::string &name, SeqRef &ref) {
    name = id < ix.seq.names.size() ? ix.seq.names[id] : std::to_string(id);
    const uint32_t s = id < ix.store_of_id.size() ? ix.store_of_id[id] : SEQ_ABSENT;
    if (s == SEQ_ABSENT) return false;
    ref = SeqRef{st.bases.data() + st.off[s], st.off[s + 1] - st.off[s]};
    return true;
  };
  auto work = [&]() {
    std::vector<impg_gpu_interval_t> v;
    try {
      for (;;) {
        const size_t i = next.fetch_add(1);
        if (i >= nr) break;
        v.assign(res.intervals.begin() + res.offsets[i], res.intervals.begin() + res.offsets[i + 1]);
        if (!p.transitive && p.min_output_length >= 0) {  // perform_query retain (main.rs:11682-11688)
          v.erase(std::remove_if(v.begin(), v.end(),
                                 [&](const impg_gpu_interval_t &x) { return std::abs((int64_t)x.q_last - x.q_first) < p.min_output_length; }),
                  v.end());
        }
        fasta_range_text(v, merge_distance, reverse_complement, fetch, parts[i]);
      }
    } catch (...) {
      next = nr;  // (the other threads stop at their next range)
      std::lock_guard<std::mutex> lk(err_m);
      if (!err) err = std::current_exception();
    }
  };
  if (T == 1) work();
  else {
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; t++) th.emplace_back(work);
    for (auto &t : th) t.join();
  }
  if (err) std::rethrow_exception(err);
}

}  // namespace impg
