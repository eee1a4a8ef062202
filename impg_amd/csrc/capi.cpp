// extern "C" entry points of libimpg_gpu.so (include/impg_gpu.h).  Nothing
// unwinds across this file: every body is wrapped and mapped to a status code.
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <functional>
#include <thread>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <new>

#include "cigar_resolve.hpp"
#include "engine.hpp"
#include "paf_ingest.hpp"
#include "partition.hpp"
#include "refine.hpp"

namespace impg {
thread_local std::string g_error;
void set_error(const std::string &msg) { g_error = msg; }
void render_paf(const impg_gpu_results &res, const impg_gpu_index &ix, const char *const *range_names,
                const impg_gpu_params_t &p, int32_t merge_distance, bool bedpe, std::vector<std::string> &parts);
void render_bed(const impg_gpu_results &res, const impg_gpu_index &ix, const char *const *range_names,
                const impg_gpu_params_t &p, int32_t merge_distance, std::vector<std::string> &parts);
char *join_parts(std::vector<std::string> &parts, size_t *len);  // bed.cpp
void render_fasta(const impg_gpu_results &res, const impg_gpu_index &ix, const impg_gpu_params_t &p, int32_t merge_distance, bool reverse_complement,
                  std::vector<std::string> &parts);  // sequences.cpp
}  // namespace impg

using namespace impg;


namespace impg {
// One engine = one stream + one set of scratch buffers + the visited sets of the batch in flight.  Calls on one
// handle from several host threads (the trait is Send + Sync: rayon workers share the index) each take their
// own engine: up to max_engines run side by side, further callers wait for one to come back.
static void engine_options(impg_gpu_index &ix, Engine *e) {
  const Options &o = e->opt = ix.opt;
  e->walk_allowed = o.walk_kernel != 0 && !getenv("IMPG_NO_WALK");
  e->walk_bfs = o.walk_kernel == 2;  // (the environment switch runs a whole test suite on the batch engine)
  e->wide_emit = WideEmit{(uint32_t)o.wide_emit_cap, (uint32_t)o.wide_emit_bins, o.lookup_stats != 0};
  e->coop_count = CoopCount{(uint32_t)o.lookup_coop_span, o.lookup_coop != 0};
  e->seg_stats = ix.seg_stats;
  e->proj_stats = ix.proj_stats;
  e->place_block_levels = &ix.place_block_levels;
  e->upd_stats = ix.upd_stats;
  e->dfs_stats = ix.dfs_stats;
  e->lk_stats = ix.lk_stats;
}
// The free engine used last, else a new one while the handle may have more; null: every engine is out.  (eng_m held.)
static Engine *take_or_create(impg_gpu_index &ix) {
  Engine *e = nullptr;
  if (!ix.eng_free.empty()) { e = ix.eng_free.back(); ix.eng_free.pop_back(); }
  else if ((int)ix.engines.size() < ix.max_engines) {
    ix.engines.emplace_back(new Engine(ix.device));
    e = ix.engines.back().get();
  } else return nullptr;
  engine_options(ix, e);
  return e;
}
EngineLease::EngineLease(impg_gpu_index &ix_) : ix(ix_) {
  std::unique_lock<std::mutex> lk(ix.eng_m);
  while (!(e = take_or_create(ix))) ix.eng_cv.wait(lk);
}
// An engine for a handle that keeps it (a partition session): never waits -- null when every engine is out.
Engine *try_lease_engine(impg_gpu_index &ix) {
  std::unique_lock<std::mutex> lk(ix.eng_m);
  return take_or_create(ix);
}
void return_engine(impg_gpu_index &ix, Engine *e) {  // the lease's end: what belonged to it ends here (engine.hpp)
  e->remote = nullptr;
  e->masked = false;
  e->subset_on = false;
  std::lock_guard<std::mutex> lk(ix.eng_m);
  ix.eng_free.push_back(e);
  ix.eng_cv.notify_one();
}
EngineLease::~EngineLease() { return_engine(ix, e); }
}  // namespace impg

namespace impg {

void require_device(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    throw Error{IMPG_E_HIP, "no HIP device available (libimpg_gpu has no CPU fallback)"};
  if (device < 0 || device >= n) throw Error{IMPG_E_INVALID, "device ordinal out of range"};
}

std::unique_ptr<impg_gpu_index> make_index(const impg_gpu_record_t *records, size_t n_records, const uint32_t *ops,
                                           size_t n_ops, const int64_t *seq_len, uint32_t n_seq, int bidirectional,
                                           int order_policy, int device, uint32_t shard, uint32_t n_shards,
                                           const HostSeqIndex *seq, const std::vector<uint64_t> *file_first,
                                           const uint32_t *owner) {
  if ((!records && n_records) || (!ops && n_ops) || (!seq_len && n_seq)) throw Error{IMPG_E_INVALID, "null input array"};
  require_device(device);
  auto ix = std::make_unique<impg_gpu_index>();
  ix->device = device;
  if (seq) ix->seq = *seq;
  if (file_first) {
    if (file_first->size() < 2 || file_first->front() != 0 || file_first->back() != n_records ||
        !std::is_sorted(file_first->begin(), file_first->end()))
      throw Error{IMPG_E_INVALID, "file boundaries must start at 0, end at n_records and be ascending"};
    ix->file_first = *file_first;
  }
  build_index(*ix, records, n_records, ops, n_ops, seq_len, n_seq, bidirectional != 0, order_policy, shard, n_shards, owner);
  { EngineLease warm(*ix); }  // the first engine exists before the first query (stream + counters)
  return ix;
}

}  // namespace impg

namespace impg {
// What the trait returns for one chunk: rows placed by the device (rows_device.hip), one copy across PCIe into a
// pinned block of the result, offsets widened on the host.  `levels` are consumed.
// max_rows: a chunk of several ranges with more rows than this is not assembled -- SplitBatch, the caller halves it
// (the row stream's bound on its host blocks); kernels_done: recorded on the stream once the chunk's last kernel is
// enqueued, ahead of the copies (whoever takes turns on the GPU may let the next one in while the rows cross PCIe)
void assemble_results(Engine &E, const impg_gpu_range_t *h_ranges, uint32_t n, const impg_gpu_params_t &p,
                      std::vector<std::unique_ptr<LevelBufs>> &levels, DevBuf &self_dev, impg_gpu_results &res, uint64_t max_rows,
                      hipEvent_t kernels_done, const std::function<void()> &on_kernels_done) {
  hipStream_t s = E.stream;
  res.ranges.assign(h_ranges, h_ranges + n);
  res.has_cigar = p.store_cigar != 0;
  RowPlan pl;
  plan_rows(E, n, p, levels, self_dev, false, pl);
  const size_t nr = pl.n_rows;
  if (nr > max_rows && n > 1) throw SplitBatch{};
  DevBuf rows, clen, coff, cpool;
  for (DevBuf *b : {&rows, &clen, &coff, &cpool}) b->pool = &E.level_pool;
  rows.reserve(std::max<size_t>(nr * sizeof(impg_gpu_interval_t), 256));
  if (res.has_cigar) clen.reserve(std::max<size_t>(nr * 4, 256));
  scatter_rows(E, levels, pl, RowSinks{rows.as<impg_gpu_interval_t>(), nullptr, nullptr, nullptr, nullptr,
                                       res.has_cigar ? clen.as<uint32_t>() : nullptr});
  // (the row stream reuses `res` chunk after chunk: a chunk a little larger than every one before it must not pin a new
  // block -- seconds for 5 GB --, so its blocks grow with a quarter to spare, within the stream's bound)
  if (max_rows != ~0ull && nr * sizeof(impg_gpu_interval_t) > res.intervals.cap)
    res.intervals.reserve(std::max<size_t>(nr, (size_t)std::min<uint64_t>(max_rows, nr + nr / 4)), true);
  res.intervals.resize(nr, true);
  std::vector<uint32_t> off32((size_t)n + 1);
  IMPG_HIP(hipMemcpyAsync(off32.data(), pl.offsets.p, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, s));
  // (without CIGARs the rows' placement was the chunk's last kernel: the GPU turn ends here, the copy below overlaps the
  // other engine's kernels)
  if (kernels_done && !res.has_cigar) IMPG_HIP(hipEventRecord(kernels_done, s));
  if (nr) IMPG_HIP(hipMemcpyAsync(res.intervals.data(), rows.p, nr * sizeof(impg_gpu_interval_t), hipMemcpyDeviceToHost, s));
  if (res.has_cigar) {
    const uint64_t n_ops = build_row_cigars(E, levels, pl, clen, coff, cpool);
    res.cigar_off.resize(nr + 1, true);
    res.cigar_ops.resize(n_ops, true);
    if (kernels_done) IMPG_HIP(hipEventRecord(kernels_done, s));
    IMPG_HIP(hipMemcpyAsync(res.cigar_off.data(), coff.p, (nr + 1) * 8, hipMemcpyDeviceToHost, s));
    if (n_ops) IMPG_HIP(hipMemcpyAsync(res.cigar_ops.data(), cpool.p, n_ops * 4, hipMemcpyDeviceToHost, s));
  }
  if (kernels_done) { IMPG_HIP(hipEventSynchronize(kernels_done)); if (on_kernels_done) on_kernels_done(); }
  IMPG_HIP(hipStreamSynchronize(s));
  levels.clear();
  res.offsets.resize((size_t)n + 1);
  for (size_t q = 0; q <= n; q++) res.offsets[q] = off32[q];
  res.projected = E.last_projected;
}

const impg_gpu_range_t *upload_ranges(DevBuf &dst, const impg_gpu_range_t *ranges, size_t n, const hipStream_t *async_on) {
  dst.reserve(std::max<size_t>(n * sizeof(impg_gpu_range_t), 256));
  if (n && async_on) IMPG_HIP(hipMemcpyAsync(dst.p, ranges, n * sizeof(impg_gpu_range_t), hipMemcpyHostToDevice, *async_on));
  else if (n) IMPG_HIP(hipMemcpy(dst.p, ranges, n * sizeof(impg_gpu_range_t), hipMemcpyHostToDevice));
  return dst.as<impg_gpu_range_t>();
}

StatSinks::StatSinks(DevBuf &cnt, DevBuf &ck, bool want_count, bool want_cksum, size_t n, const hipStream_t *async_on) {
  auto zeroed = [&](DevBuf &b) {
    b.reserve(std::max<size_t>(n * 8, 256));
    if (async_on) IMPG_HIP(hipMemsetAsync(b.p, 0, n * 8, *async_on));
    else IMPG_HIP(hipMemset(b.p, 0, std::max<size_t>(n * 8, 8)));
    return b.as<unsigned long long>();
  };
  if (want_count) count = zeroed(cnt);
  if (want_cksum) cksum = zeroed(ck);
}
void StatSinks::home(uint64_t *per_range_count, uint64_t *per_range_checksum, size_t n) const {
  if (per_range_count && n) IMPG_HIP(hipMemcpy(per_range_count, count, n * 8, hipMemcpyDeviceToHost));
  if (per_range_checksum && n) IMPG_HIP(hipMemcpy(per_range_checksum, cksum, n * 8, hipMemcpyDeviceToHost));
}

bool run_chunk_rows(const impg_gpu_index &ix, Engine &E, const impg_gpu_range_t *d_ranges, const impg_gpu_range_t *h_ranges, size_t b,
                    size_t e, const impg_gpu_params_t &p, impg_gpu_results &part, std::mutex *gpu_turn, uint64_t max_rows,
                    hipEvent_t kernels_done, const std::function<void()> &on_kernels_done) {
  std::vector<std::unique_ptr<LevelBufs>> levels;
  DevBuf self_dev;
  self_dev.pool = &E.level_pool;
  const auto c0 = std::chrono::steady_clock::now();
  {
    const auto turn = take_turn(gpu_turn);
    RunSpec rs(d_ranges + b, (uint32_t)(e - b), p);
    rs.keep = &levels;
    rs.self_out = &self_dev;
    E.run(ix, rs);
  }
  const auto c1 = std::chrono::steady_clock::now();
  if (e == b) return false;
  assemble_results(E, h_ranges + b, (uint32_t)(e - b), p, levels, self_dev, part, max_rows, kernels_done, on_kernels_done);
  part.approximate = ix.tp_mode;
  part.run_s = std::chrono::duration<double>(c1 - c0).count();
  part.assemble_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - c1).count();
  return true;
}

bool run_chunk_bed(const impg_gpu_index &ix, Engine &E, const impg_gpu_range_t *d_ranges, const impg_gpu_range_t *h_ranges,
                   const char *const *range_names, size_t b, size_t e, const impg_gpu_params_t &p, int32_t merge_distance,
                   const std::function<void(const char *, size_t)> &sink, double *seconds3, std::mutex *gpu_turn, TextFormat format) {
  std::vector<std::unique_ptr<LevelBufs>> levels;
  DevBuf self_dev, rows;
  PafChunkPtr paf;  // (PAF: the chunk's rows, ops and order live until its text is out)
  self_dev.pool = &E.level_pool;
  const auto turn = take_turn(gpu_turn);
  const auto c0 = std::chrono::steady_clock::now();
  RunSpec rs(d_ranges + b, (uint32_t)(e - b), p);
  rs.keep = &levels;
  rs.self_out = &self_dev;
  E.run(ix, rs);
  const auto c1 = std::chrono::steady_clock::now();
  if (e == b) return false;
  uint32_t n_rows = 0;
  const bool fasta = format == TEXT_FASTA || format == TEXT_FASTA_RC;
  if (format == TEXT_PAF) paf = device_paf_rows(E, ix, (uint32_t)(e - b), p, merge_distance, levels, self_dev);
  else if (fasta) {
    uint32_t n_in = 0;
    n_rows = device_fasta_rows(E, ix, (uint32_t)(e - b), p, merge_distance, levels, self_dev, rows, n_in);
    ix.fasta_stats[FASTA_ROWS] += n_in;
    ix.fasta_stats[FASTA_RECORDS] += n_rows;
  }
  else n_rows = (format == TEXT_BEDPE ? device_bedpe_rows : device_bed_rows)(E, ix, (uint32_t)(e - b), p, merge_distance, levels, self_dev, rows);
  const auto c2 = std::chrono::steady_clock::now();
  const std::vector<std::string> rnames = bed_range_names(ix, h_ranges, range_names, b, e);
  const bool orig = p.original_sequence_coordinates != 0;
  if (format == TEXT_PAF) device_paf_text(E, ix, *paf, (uint32_t)(e - b), rnames, orig, sink);
  else if (fasta) device_fasta_text(E, ix, rows, n_rows, format == TEXT_FASTA_RC, sink);
  else (format == TEXT_BEDPE ? device_bedpe_text : device_bed_text)(E, ix, rows, n_rows, (uint32_t)(e - b), rnames, orig, sink);
  const auto c3 = std::chrono::steady_clock::now();
  seconds3[0] += std::chrono::duration<double>(c1 - c0).count();
  seconds3[1] += std::chrono::duration<double>(c2 - c1).count();
  seconds3[2] += std::chrono::duration<double>(c3 - c2).count();
  return true;
}

}  // namespace impg

namespace {
// Runs fn(begin, end) over [0,n) in chunks; a chunk whose level outgrows the pair
// budget (SplitBatch) is retried at half the size.  Queries are independent, so
// any split by ranges gives identical results.
template <class F> void for_chunks(Engine &E, size_t n, F fn) {
  size_t chunk = E.opt.chunk_ranges ? (size_t)E.opt.chunk_ranges : n;
  if (chunk == 0) chunk = 1;
  size_t b = 0;
  while (b < n) {
    size_t e = std::min(n, b + chunk);
    try {
      fn(b, e);
      b = e;
    } catch (const SplitBatch &) {
      if (e - b <= 1) throw Error{IMPG_E_UNSUPPORTED, "a single range exceeds the pair budget"};
      chunk = std::max<size_t>(1, (e - b) / 2);
    }
  }
}

// what the two self-tests (impg_gpu_selftest_bed_rows, _bedpe_rows) share: the rows' number fits the device's 32-bit row
// indices; the names their ranges print under are the caller's, else the range's index
void check_row_count(size_t n_rows) { if (n_rows >= 0xFFFFFFF0ull) throw Error{IMPG_E_INVALID, "too many rows"}; }
std::vector<std::string> default_range_names(uint32_t n_ranges, const char *const *range_names) {
  std::vector<std::string> rnames(n_ranges);
  for (uint32_t q = 0; q < n_ranges; q++) rnames[q] = range_names && range_names[q] ? std::string(range_names[q]) : std::to_string(q);
  return rnames;
}

}  // namespace

namespace {
// The per-query walk (Engine::run_walk) with its rows kept, over the n ranges in E.ranges_dev.  Every query writes into
// its region of W.rows (base[q], cap[q] rows); if one outgrew its region the queries are walked again with every
// query's rows at their final place, back to back -- the walk is deterministic, so the second pass writes exactly what
// the first counted (`exact` is then set).  cnt[q]: the rows of query q.  false: the walk did not take the batch.
bool walk_two_pass(impg_gpu_index &ix, Engine &E, uint32_t n, const impg_gpu_params_t &p, Engine::WalkRows &W,
                   std::vector<unsigned long long> &base, std::vector<uint32_t> &cap, std::vector<uint32_t> &cnt, bool &exact) {
  hipStream_t s = E.stream;
  for (DevBuf *b : {&W.rows, &W.base, &W.cap, &W.n_rows}) b->pool = &E.level_pool;
  W.base.reserve(std::max<size_t>((size_t)n * 8, 256)); W.cap.reserve(std::max<size_t>((size_t)n * 4, 256));
  W.n_rows.reserve(std::max<size_t>((size_t)n * 4, 256));
  cnt.assign(n, 0);
  auto pass = [&]() {
    uint64_t total_rows = 0;
    for (uint32_t q = 0; q < n; q++) total_rows += cap[q];
    W.rows.reserve(std::max<size_t>(total_rows * sizeof(impg_gpu_interval_t), 256));
    IMPG_HIP(hipMemcpyAsync(W.base.p, base.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    IMPG_HIP(hipMemcpyAsync(W.cap.p, cap.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    return E.run_walk(ix, E.ranges_dev.as<impg_gpu_range_t>(), n, p, nullptr, nullptr, nullptr, &W, cnt.data());  // (cnt: the rows every query wrote)
  };
  exact = false;
  if (!pass()) return false;
  bool fits = true;
  for (uint32_t q = 0; q < n; q++) fits = fits && cnt[q] <= cap[q];
  if (fits) return true;
  uint64_t at = 0;
  for (uint32_t q = 0; q < n; q++) { base[q] = at; cap[q] = cnt[q]; at += cnt[q]; }
  const std::vector<uint32_t> want = cnt;
  if (!pass()) return false;
  if (cnt != want) throw Error{IMPG_E_INVALID, "internal: the walk's second pass disagrees with its first"};
  exact = true;
  return true;
}
// The trait's rows from the per-query walk.  A handful of queries write into generous fixed regions of one pool and are
// done in one launch; a batch is counted first (regions of no rows) and walked again.
bool walk_query(impg_gpu_index &ix, Engine &E, uint32_t n, const impg_gpu_params_t &p, impg_gpu_results &res) {
  hipStream_t s = E.stream;
  Engine::WalkRows W;
  const uint32_t each = n <= Engine::SMALL_RANGES ? (1u << 17) : 0u;
  std::vector<unsigned long long> base(n);
  std::vector<uint32_t> cap(n, each), cnt;
  for (uint32_t q = 0; q < n; q++) base[q] = (unsigned long long)q * each;
  bool contiguous = false;
  if (!walk_two_pass(ix, E, n, p, W, base, cap, cnt, contiguous)) return false;
  uint64_t total = 0;
  res.offsets.assign((size_t)n + 1, 0);
  for (uint32_t q = 0; q < n; q++) { res.offsets[q + 1] = res.offsets[q] + cnt[q]; total += cnt[q]; }
  res.intervals.resize(total, true);
  const impg_gpu_interval_t *d_rows = W.rows.as<impg_gpu_interval_t>();
  if (contiguous) {
    if (total) IMPG_HIP(hipMemcpyAsync(res.intervals.data(), d_rows, total * sizeof(impg_gpu_interval_t), hipMemcpyDeviceToHost, s));
  } else {
    for (uint32_t q = 0; q < n; q++)
      if (cnt[q])
        IMPG_HIP(hipMemcpyAsync(res.intervals.data() + res.offsets[q], d_rows + base[q], (size_t)cnt[q] * sizeof(impg_gpu_interval_t),
                                hipMemcpyDeviceToHost, s));
  }
  IMPG_HIP(hipStreamSynchronize(s));
  ix.result_rows_to_host += total;
  res.has_cigar = false;
  res.projected = E.last_projected;
  return true;
}
}  // namespace

namespace impg {
// One transitive query's rows left in HBM for the partition update (partition_device.hip): the per-query walk writes them
// into a generous region first and is run again at the exact size if the query outgrew it; where the walk does not apply
// the batch engine's kept levels are placed in emission order (rows_device.hip), as assemble_results does ahead of its copy.
uint32_t query_rows_device(impg_gpu_index &ix, Engine &E, const impg_gpu_range_t &range, const impg_gpu_params_t &p, DevBuf &rows,
                           const impg_gpu_interval_t *&d_rows, bool &walked) {
  hipStream_t s = E.stream;
  walked = false;
  upload_ranges(E.ranges_dev, &range, 1, &s);
  if (E.walk_applicable(ix, 1, p)) {
    Engine::WalkRows W;
    std::vector<unsigned long long> base(1, 0);
    std::vector<uint32_t> cap(1, 1u << 17), cnt;
    bool exact;
    if (walk_two_pass(ix, E, 1, p, W, base, cap, cnt, exact)) {
      rows.adopt(W.rows);
      d_rows = rows.as<impg_gpu_interval_t>();
      walked = true;
      return cnt[0];
    }
  }
  std::vector<std::unique_ptr<LevelBufs>> levels;
  DevBuf self_dev;
  self_dev.pool = &E.level_pool;
  try {
    RunSpec rs(E.ranges_dev.as<impg_gpu_range_t>(), 1, p);
    rs.keep = &levels;
    rs.self_out = &self_dev;
    E.run(ix, rs);
  } catch (const SplitBatch &) {
    throw Error{IMPG_E_UNSUPPORTED, "a single range exceeds the pair budget"};
  }
  RowPlan pl;
  plan_rows(E, 1, p, levels, self_dev, false, pl);
  if (!rows.pool) rows.pool = &E.level_pool;
  rows.reserve(std::max<size_t>((size_t)pl.n_rows * sizeof(impg_gpu_interval_t), 256));
  scatter_rows(E, levels, pl, RowSinks{rows.as<impg_gpu_interval_t>(), nullptr, nullptr, nullptr, nullptr, nullptr});
  IMPG_HIP(hipStreamSynchronize(s));
  levels.clear();
  d_rows = rows.as<impg_gpu_interval_t>();
  return pl.n_rows;
}
}  // namespace impg

namespace impg {
std::vector<std::string> bed_range_names(const impg_gpu_index &ix, const impg_gpu_range_t *ranges, const char *const *range_names,
                                         size_t b, size_t e) {
  std::vector<std::string> rn(e - b);
  char buf[64];
  for (size_t i = b; i < e; i++) {
    if (range_names && range_names[i]) rn[i - b] = range_names[i];
    else {
      const impg_gpu_range_t &q = ranges[i];
      rn[i - b] = q.target_id < ix.seq.names.size() ? ix.seq.names[q.target_id] : std::to_string(q.target_id);
      const int k = snprintf(buf, sizeof buf, ":%d-%d", q.start, q.end);
      rn[i - b].append(buf, (size_t)k);
    }
  }
  return rn;
}
void check_ranges(const impg_gpu_range_t *ranges, size_t n) {
  if (n >= (1ull << 31)) throw Error{IMPG_E_UNSUPPORTED, "more than 2^31 ranges in one batch"};
  for (size_t i = 0; i < n; i++)
    if (ranges[i].start >= ranges[i].end) throw Error{IMPG_E_INVALID, "query range must satisfy start < end"};
}
// part's rows behind res's.  The first part hands its arrays over; later ones are copied behind them (the
// destination grows geometrically, pinned like its parts).
template <class T> static void append_arr(HostArr<T> &dst, HostArr<T> &src, size_t drop_front = 0) {
  if (dst.empty() && !drop_front) { dst.swap(src); return; }
  const size_t add = src.size() - drop_front, base = dst.size();
  if ((base + add) * sizeof(T) > dst.cap) dst.reserve(std::max(base + add, base + base / 2), dst.pinned || src.pinned);
  dst.n = base + add;
  parallel_memcpy(dst.data() + base, src.data() + drop_front, add * sizeof(T));
}
void append_results(impg_gpu_results &res, impg_gpu_results &part) {
  if (res.offsets.empty()) res.offsets.assign(1, 0);
  if (part.offsets.empty()) part.offsets.assign(1, 0);
  const uint64_t base = res.intervals.size();
  res.approximate = res.approximate || part.approximate;
  if (part.has_cigar) {
    res.has_cigar = true;
    if (res.cigar_off.empty()) res.cigar_off.assign((size_t)1, (uint64_t)0);
    const uint64_t cb = res.cigar_ops.size();
    const size_t at = res.cigar_off.size();
    if (part.cigar_off.size() > 1) {
      if (at == 1 && cb == 0) res.cigar_off.swap(part.cigar_off);
      else {
        append_arr(res.cigar_off, part.cigar_off, 1);
        for (size_t i = at; i < res.cigar_off.size(); i++) res.cigar_off[i] += cb;
      }
    }
    append_arr(res.cigar_ops, part.cigar_ops);
  }
  append_arr(res.intervals, part.intervals);
  if (base == 0 && res.offsets.size() == 1) res.offsets.swap(part.offsets);
  else for (size_t i = 1; i < part.offsets.size(); i++) res.offsets.push_back(base + part.offsets[i]);
  res.projected += part.projected;
  res.run_s += part.run_s;
  res.assemble_s += part.assemble_s;
}
}  // namespace impg

extern "C" {

const char *impg_gpu_last_error(void) { return impg::g_error.c_str(); }

int impg_gpu_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int impg_gpu_index_create(const impg_gpu_record_t *records, size_t n_records, const uint32_t *cigar_ops, size_t n_ops,
                          const int64_t *seq_len, uint32_t n_seq, int bidirectional, int order_policy, int device,
                          impg_gpu_index_t **out) {
  IMPG_TRY
  if (!out) throw Error{IMPG_E_INVALID, "null out"};
  *out = make_index(records, n_records, cigar_ops, n_ops, seq_len, n_seq, bidirectional, order_policy, device, 0, 1, nullptr,
                    nullptr, nullptr).release();
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_index_create_files(const impg_gpu_record_t *records, size_t n_records, const uint32_t *cigar_ops, size_t n_ops,
                                const int64_t *seq_len, uint32_t n_seq, const uint64_t *file_first_record, uint32_t n_files,
                                int bidirectional, int order_policy, int device, impg_gpu_index_t **out) {
  IMPG_TRY
  if (!out || !file_first_record || n_files == 0) throw Error{IMPG_E_INVALID, "bad arguments"};
  std::vector<uint64_t> ff(file_first_record, file_first_record + n_files);
  ff.push_back(n_records);
  *out = make_index(records, n_records, cigar_ops, n_ops, seq_len, n_seq, bidirectional, order_policy, device, 0, 1, nullptr,
                    &ff, nullptr).release();
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_index_create_tracepoints(const impg_gpu_tp_record_t *records, size_t n_records, const int32_t *tracepoints,
                                      const int32_t *query_deltas, const int32_t *diffs, size_t n_segs_total,
                                      const impg_gpu_tp_mode_t *mode, const int64_t *seq_len, uint32_t n_seq, int bidirectional,
                                      int order_policy, int device, impg_gpu_index_t **out) {
  IMPG_TRY
  if (!out || !mode || (n_records && !records) || (n_segs_total && !tracepoints) || (n_seq && !seq_len))
    throw Error{IMPG_E_INVALID, "null argument"};
  if (mode->fastga) {
    if (n_segs_total && !diffs) throw Error{IMPG_E_INVALID, "FASTGA tracepoints come with per-segment diffs"};
    if (mode->trace_spacing <= 0) throw Error{IMPG_E_INVALID, "trace_spacing must be positive"};
  } else if (n_segs_total && !query_deltas) throw Error{IMPG_E_INVALID, "Standard tracepoints come with per-segment query deltas"};
  require_device(device);
  // the shared record shape: cigar_off / cigar_len name the alignment's segments
  std::vector<impg_gpu_record_t> recs(n_records);
  for (size_t i = 0; i < n_records; i++) {
    const impg_gpu_tp_record_t &r = records[i];
    if (r.seg_off + r.n_segs > n_segs_total) throw Error{IMPG_E_INVALID, "record segments outside the pools"};
    recs[i] = impg_gpu_record_t{r.query_id, r.target_id, r.query_start, r.query_end, r.target_start, r.target_end, r.seg_off, r.n_segs,
                                r.strand};
  }
  TpInput tp{records, tracepoints, query_deltas, diffs, n_segs_total, *mode};
  auto ix = std::make_unique<impg_gpu_index>();
  ix->device = device;
  build_index(*ix, recs.data(), n_records, nullptr, n_segs_total, seq_len, n_seq, bidirectional != 0, order_policy, 0, 1, nullptr, &tp);
  { EngineLease warm(*ix); }
  *out = ix.release();
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_index_create_from_paf(const char *const *paths, int n_paths, int bidirectional, int order_policy, int device,
                                   impg_gpu_index_t **out) {
  IMPG_TRY
  if (!out || !paths || n_paths <= 0) throw Error{IMPG_E_INVALID, "bad arguments"};
  require_device(device);
  ParsedPaf pp;
  std::vector<std::string> ps(paths, paths + n_paths);
  const auto t0 = std::chrono::steady_clock::now();
  const bool timing = build_switches().timing;
  auto lap = [&](const char *what, std::chrono::steady_clock::time_point from) {
    if (timing) fprintf(stderr, "[build] %-28s %.3f s\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - from).count());
  };
  // The CIGAR text is tokenised on the device (parse_cigar_to_delta, impg.rs:2935-2950 -> cigar_tokens_kernel): the
  // host only splits lines and fields, the text crosses PCIe once and the ops never exist on the host.  Inputs whose
  // text and ops would not fit next to the index they become (or IMPG_BUILD_HOST=1) are tokenised by the host parser.
  bool raw = !build_switches().host_build;
  if (raw) {
    uint64_t bytes = 0;
    for (auto &p : ps) {
      struct stat st;
      if (stat(p.c_str(), &st) == 0) bytes += (uint64_t)st.st_size * ((p.size() > 3 && p.compare(p.size() - 3, 3, ".gz") == 0) ? 6 : 1);
    }
    size_t free_b = 0, total_b = 0;
    IMPG_HIP(hipSetDevice(device));
    IMPG_HIP(hipMemGetInfo(&free_b, &total_b));
    if (bytes * 8 > free_b) raw = false;  // text + ops (<= 2 bytes of text per op) + the index (~3.4 x the ops)
  }
  parse_paf_files(ps, pp, raw);
  lap(raw ? "parse PAF (lines, fields)" : "parse PAF", t0);
  std::vector<int64_t> lens = pp.seq.lens;
  if (raw) {
    const auto t1 = std::chrono::steady_clock::now();
    DevBuf d_ops;
    const uint64_t n_ops = tokenize_on_device(pp, device, d_ops);
    lap("CIGAR text -> ops (device)", t1);
    auto ix = std::make_unique<impg_gpu_index>();
    ix->device = device;
    ix->seq = pp.seq;
    if (pp.file_first.size() < 2 || pp.file_first.front() != 0 || pp.file_first.back() != pp.records.size())
      throw Error{IMPG_E_INVALID, "internal: bad file boundaries"};
    ix->file_first = pp.file_first;
    ix->build_stats[BUILD_TOKENIZED_DEVICE] = 1;
    if (order_policy != IMPG_ORDER_COITREES && order_policy != IMPG_ORDER_SORTED) throw Error{IMPG_E_INVALID, "bad order policy"};
    if (build_index_device(*ix, pp.records.data(), pp.records.size(), nullptr, n_ops, lens.data(), (uint32_t)lens.size(), bidirectional != 0,
                           order_policy, 0, 1, nullptr, d_ops.as<uint32_t>())) {
      { EngineLease warm(*ix); }
      *out = ix.release();
      return IMPG_OK;
    }
    // (the device was short of memory for the build: the ops come back and the host builder takes over)
    pp.ops.resize(n_ops);
    if (n_ops) IMPG_HIP(hipMemcpy(pp.ops.data(), d_ops.p, n_ops * 4, hipMemcpyDeviceToHost));
  }
  *out = make_index(pp.records.data(), pp.records.size(), pp.ops.data(), pp.ops.size(), lens.data(), (uint32_t)lens.size(),
                    bidirectional, order_policy, device, 0, 1, &pp.seq, &pp.file_first, nullptr).release();
  if (raw) (*out)->build_stats[BUILD_TOKENIZED_DEVICE] = 1;  // (the device tokenised; the host builder took over)
  return IMPG_OK;
  IMPG_CATCH
}

// impg_gpu_index_create_from_paf with the M ops resolved between the tokeniser and the builder (cigar_resolve.hpp): the pool
// is rewritten where it lies in HBM and the builder reads the new one; the records' new offsets and lengths come home for
// its host loops.
int impg_gpu_index_create_from_paf_resolved(const char *const *paths, int n_paths, const impg_gpu_sequences_t *seqs, int bidirectional,
                                            int order_policy, int device, impg_gpu_resolve_report_t *report, uint8_t **flags,
                                            impg_gpu_index_t **out) {
  IMPG_TRY
  if (!out || !paths || n_paths <= 0 || !seqs) throw Error{IMPG_E_INVALID, "bad arguments"};
  if (order_policy != IMPG_ORDER_COITREES && order_policy != IMPG_ORDER_SORTED) throw Error{IMPG_E_INVALID, "bad order policy"};
  require_device(device);
  const SeqStore &st = host_copy(store_of(seqs));
  ParsedPaf pp;
  std::vector<std::string> ps;
  for (int i = 0; i < n_paths; i++) {
    if (!paths[i]) throw Error{IMPG_E_INVALID, "null argument"};
    ps.push_back(paths[i]);
  }
  const bool raw = !build_switches().host_build;
  parse_paf_files(ps, pp, raw);
  IMPG_HIP(hipSetDevice(device));
  DevBuf d_ops, d_new;
  uint64_t n_ops = pp.ops.size();
  if (raw) n_ops = tokenize_on_device(pp, device, d_ops);
  else {
    d_ops.reserve(std::max<size_t>(n_ops * 4, 256));
    if (n_ops) IMPG_HIP(hipMemcpy(d_ops.p, pp.ops.data(), n_ops * 4, hipMemcpyHostToDevice));
  }
  std::vector<const char *> names;
  for (const std::string &n : pp.seq.names) names.push_back(n.c_str());
  std::vector<int64_t> lens = pp.seq.lens;
  const cigar_resolve::Plan plan = cigar_resolve::make_plan(pp.records.data(), pp.records.size(), n_ops, names.data(), lens.data(), (uint32_t)lens.size(), st);
  cigar_resolve::Result res;
  cigar_resolve::resolve_device(pp.records.data(), pp.records.size(), d_ops.as<uint32_t>(), n_ops, plan, st, 0, device, res, d_new);
  d_ops.release();
  for (size_t i = 0; i < pp.records.size(); i++) {
    pp.records[i].cigar_off = res.off[i];
    pp.records[i].cigar_len = res.len[i];
  }
  if (pp.file_first.size() < 2 || pp.file_first.front() != 0 || pp.file_first.back() != pp.records.size())
    throw Error{IMPG_E_INVALID, "internal: bad file boundaries"};
  auto stamp = [&](impg_gpu_index &ix) {
    if (raw) ix.build_stats[BUILD_TOKENIZED_DEVICE] = 1;
    const uint64_t *f = &res.report.records;
    for (int k = 0; k < 12; k++) ix.resolve_stats[k] = f[k];
  };
  auto ix = std::make_unique<impg_gpu_index>();
  ix->device = device;
  ix->seq = pp.seq;
  ix->file_first = pp.file_first;
  if (build_index_device(*ix, pp.records.data(), pp.records.size(), nullptr, res.n_out, lens.data(), (uint32_t)lens.size(), bidirectional != 0,
                         order_policy, 0, 1, nullptr, d_new.as<uint32_t>())) {
    { EngineLease warm(*ix); }
  } else {  // (the device was short of memory for the build: the new ops come home and the host builder takes over)
    pp.ops.resize(res.n_out);
    if (res.n_out) IMPG_HIP(hipMemcpy(pp.ops.data(), d_new.p, res.n_out * 4, hipMemcpyDeviceToHost));
    d_new.release();
    ix = make_index(pp.records.data(), pp.records.size(), pp.ops.data(), pp.ops.size(), lens.data(), (uint32_t)lens.size(), bidirectional,
                    order_policy, device, 0, 1, &pp.seq, &pp.file_first, nullptr);
  }
  stamp(*ix);
  if (flags) {
    uint8_t *f = (uint8_t *)malloc(std::max<size_t>(res.flags.size(), 1));
    if (!f) throw std::bad_alloc();
    if (!res.flags.empty()) memcpy(f, res.flags.data(), res.flags.size());
    *flags = f;
  }
  if (report) *report = res.report;
  *out = ix.release();
  return IMPG_OK;
  IMPG_CATCH
}

// The second way from PAF files to an index: the files streamed into HBM in pieces and parsed there (paf_ingest.hpp).  From
// the hand-off on -- records on the host, the op pool in HBM -- the code is impg_gpu_index_create_from_paf's.  One difference
// in what a bad input is told: that route tokenises last, so a bad head anywhere is reported before any bad CIGAR; this one
// reports whichever line comes first in file order.
int impg_gpu_index_create_from_paf_streamed(const char *const *paths, int n_paths, int bidirectional, int order_policy, int device,
                                            uint64_t piece_bytes, impg_gpu_index_t **out) {
  IMPG_TRY
  if (!out || !paths || n_paths <= 0) throw Error{IMPG_E_INVALID, "bad arguments"};
  require_device(device);
  if (order_policy != IMPG_ORDER_COITREES && order_policy != IMPG_ORDER_SORTED) throw Error{IMPG_E_INVALID, "bad order policy"};
  std::vector<std::string> ps;
  for (int i = 0; i < n_paths; i++) {
    if (!paths[i]) throw Error{IMPG_E_INVALID, "null argument"};
    ps.push_back(paths[i]);
  }
  const bool timing = build_switches().timing;
  const auto t0 = std::chrono::steady_clock::now();
  paf_ingest::Loaded L;
  ParsedPaf pp;
  DevBuf d_ops;
  paf_ingest_device(ps, (size_t)piece_bytes, device, L, pp.records, d_ops);  // (a failure leaves nothing behind: the backend owns every block)
  if (timing)
    fprintf(stderr, "[build] %-28s %.3f s (reader %.3f s, names %.3f s)\n", "PAF streamed into HBM",
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), L.read_seconds, L.resolve_seconds);
  if (const char *hp = getenv("IMPG_PAF_INGEST_TIMING")) {
    if (FILE *f = *hp ? fopen(hp, "a") : nullptr) {  // (behind the backend's line)
      fprintf(f, "handoff_s %.6f reader_s %.6f names_s %.6f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(),
              L.read_seconds, L.resolve_seconds);
      fclose(f);
    }
  }
  pp.seq = L.seq;
  pp.file_first = L.file_first;
  const uint64_t n_ops = L.n_ops;
  std::vector<int64_t> lens = pp.seq.lens;
  auto stamp = [&](impg_gpu_index &ix) {
    ix.build_stats[BUILD_TOKENIZED_DEVICE] = 1;
    for (int k = 0; k < paf_ingest::N_STATS; k++) ix.paf_ingest_stats[k] = L.stats[k];
    ix.paf_ingest_stats[paf_ingest::DEVICE] = 1;
  };
  {
    auto ix = std::make_unique<impg_gpu_index>();
    ix->device = device;
    ix->seq = pp.seq;
    if (pp.file_first.size() < 2 || pp.file_first.front() != 0 || pp.file_first.back() != pp.records.size())
      throw Error{IMPG_E_INVALID, "internal: bad file boundaries"};
    ix->file_first = pp.file_first;
    if (build_index_device(*ix, pp.records.data(), pp.records.size(), nullptr, n_ops, lens.data(), (uint32_t)lens.size(), bidirectional != 0,
                           order_policy, 0, 1, nullptr, d_ops.as<uint32_t>())) {
      { EngineLease warm(*ix); }
      stamp(*ix);
      *out = ix.release();
      return IMPG_OK;
    }
  }
  // (the device was short of memory for the build: the ops come home and the host builder takes over)
  pp.ops.resize(n_ops);
  if (n_ops) IMPG_HIP(hipMemcpy(pp.ops.data(), d_ops.p, n_ops * 4, hipMemcpyDeviceToHost));
  d_ops.release();
  auto ix = make_index(pp.records.data(), pp.records.size(), pp.ops.data(), pp.ops.size(), lens.data(), (uint32_t)lens.size(), bidirectional,
                       order_policy, device, 0, 1, &pp.seq, &pp.file_first, nullptr);
  stamp(*ix);
  *out = ix.release();
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_parse_subsequence(const char *seq_name, char *base_out, size_t base_cap, int32_t *start_offset) {
  IMPG_TRY
  if (!seq_name || !base_out || !start_offset) throw Error{IMPG_E_INVALID, "null argument"};
  size_t base_len = 0;
  uint32_t off = 0;
  const std::string name(seq_name);
  if (!subsequence_origin(name, base_len, off)) return 0;
  if (base_len + 1 > base_cap) throw Error{IMPG_E_INVALID, "name buffer too small"};
  memcpy(base_out, name.data(), base_len);
  base_out[base_len] = '\0';
  *start_offset = (int32_t)off;
  return 1;
  IMPG_CATCH
}

int impg_gpu_subset_keep(const char *list_text, size_t len, const char *const *names, size_t n, uint8_t *keep_out,
                         size_t *n_entries) {
  IMPG_TRY
  if ((!list_text && len) || (n && (!names || !keep_out))) throw Error{IMPG_E_INVALID, "null argument"};
  const size_t e = subset_select(list_text, len, names, n, keep_out);
  if (n_entries) *n_entries = e;
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_index_save(const impg_gpu_index_t *ix, const char *path) {
  IMPG_TRY
  if (!ix || !path) throw Error{IMPG_E_INVALID, "null argument"};
  if (ix->shard || ix->cluster) save_sharded(*ix, path);
  else save_index(*ix, path);
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_index_load(const char *path, int device, impg_gpu_index_t **out) {
  IMPG_TRY
  if (!path || !out) throw Error{IMPG_E_INVALID, "null argument"};
  require_device(device);
  auto ix = std::make_unique<impg_gpu_index>();
  ix->device = device;
  load_index(*ix, path);
  { EngineLease warm(*ix); }
  *out = ix.release();
  return IMPG_OK;
  IMPG_CATCH
}

void impg_gpu_index_destroy(impg_gpu_index_t *ix) { delete ix; }

uint32_t impg_gpu_num_seqs(const impg_gpu_index_t *ix) { return (uint32_t)ix->seq.lens.size(); }
const char *impg_gpu_seq_name(const impg_gpu_index_t *ix, uint32_t id) {
  return id < ix->seq.names.size() ? ix->seq.names[id].c_str() : nullptr;
}
int64_t impg_gpu_seq_len(const impg_gpu_index_t *ix, uint32_t id) { return id < ix->seq.lens.size() ? ix->seq.lens[id] : -1; }
int64_t impg_gpu_seq_id(const impg_gpu_index_t *ix, const char *name) {
  auto it = ix->seq.name_to_id.find(name);
  return it == ix->seq.name_to_id.end() ? -1 : (int64_t)it->second;
}
size_t impg_gpu_num_targets(const impg_gpu_index_t *ix) { return ix->n_targets; }
size_t impg_gpu_target_ids(const impg_gpu_index_t *ix, uint32_t *out, size_t cap) {
  size_t k = 0;
  for (uint32_t s = 0; s + 1 < ix->h_tgt_off.size(); s++)
    if (ix->h_tgt_off[s + 1] != ix->h_tgt_off[s]) {
      if (out && k < cap) out[k] = s;
      k++;
    }
  return k;
}
size_t impg_gpu_num_entries(const impg_gpu_index_t *ix) { return ix->n_entries; }
size_t impg_gpu_num_records(const impg_gpu_index_t *ix) { return ix->n_records; }
size_t impg_gpu_device_bytes(const impg_gpu_index_t *ix) { return ix->device_bytes; }
int impg_gpu_index_approximate(const impg_gpu_index_t *ix) {
  return ix->tp_mode ? 1 : 0;
}

uint64_t impg_gpu_host_pool_trim(uint64_t keep_bytes) { return (uint64_t)impg::pinned_trim((size_t)keep_bytes); }

// (options.hpp is host-only and spells these limits out: they are the kernels')
static_assert(option_row("walk_members")->hi == WALK_MAX_MEMBERS && option_row("wide_emit_cap")->hi == WIDE_CAP && option_row("wide_emit_bins")->hi == WIDE_BINS && option_row("lookup_coop_span")->hi == LOOKUP_COOP_CAP,
              "the option table's limits are the kernels' capacities");

int impg_gpu_set_option(impg_gpu_index_t *ix, const char *key, int64_t value) {
  IMPG_TRY
  if (!ix || !key) throw Error{IMPG_E_INVALID, "null argument"};
  const OptionRow *row = option_row(key);
  if (!row) throw Error{IMPG_E_INVALID, std::string("unknown option ") + key};
  if (!strcmp(key, "sequence_ingest_piece_bytes") && value % 16) throw Error{IMPG_E_INVALID, row->refusal};
  if (!option_store(ix->opt, *row, value)) throw Error{IMPG_E_INVALID, row->refusal};
  if (row->member || !value) return IMPG_OK;
  // the two keys that act instead of storing (options.hpp)
  if (!strcmp(key, "prewarm_result_bytes")) {
    size_t cap = 0;
    void *b = pinned_take((size_t)value, cap);
    pinned_give(b, cap);
  } else if (!ix->shard && !ix->cluster) {  // prewarm_walk
    IMPG_HIP(hipSetDevice(ix->device));
    EngineLease lease(*ix);
    lease->reserve_walk_slabs(*ix, value >= 2);
  }
  return IMPG_OK;
  IMPG_CATCH
}
const char *impg_gpu_option_key(size_t i) { return i < N_OPTIONS ? OPTION_TABLE[i].key : nullptr; }

// impg_gpu_get_counter: every key and the atomic of the handle it reads
// (over_ranks: a multi-GPU handle answers with the sum over its ranks' handles)
struct CounterRow { const char *key; const std::atomic<uint64_t> &(*at)(const impg_gpu_index &); bool over_ranks; };
#define CTR(key, member) {key, [](const impg_gpu_index &ix) -> const std::atomic<uint64_t> & { return ix.member; }, false}
#define CTR_RANKS(key, member) {key, [](const impg_gpu_index &ix) -> const std::atomic<uint64_t> & { return ix.member; }, true}
static const CounterRow COUNTER_TABLE[] = {
    CTR("walk_launches", walk_launches), CTR("walk_fallbacks", walk_fallbacks), CTR("walk_members", walk_last_members), CTR("walk_overflow", walk_last_overflow),
    CTR("small_batches", small_batches),
    CTR("dfs_rounds", dfs_stats[0]), CTR("visited_compactions", dfs_stats[1]),
    CTR("segment_sliced_levels", seg_stats[0]), CTR("segment_retries", seg_stats[1]), CTR("segment_library_levels", seg_stats[2]),
    CTR("project_lane_levels", proj_stats[PROJ_ARM_LANE]), CTR("project_staged_levels", proj_stats[PROJ_ARM_STAGED]),
    CTR("project_staged_rows_levels", proj_stats[PROJ_ARM_STAGED_ROWS]), CTR("project_entries_slots_levels", proj_stats[PROJ_ARM_ENTRIES_SLOTS]),
    CTR("project_entries_qs_levels", proj_stats[PROJ_ARM_ENTRIES_QS]), CTR("project_entries_rows_levels", proj_stats[PROJ_ARM_ENTRIES_ROWS]),
    CTR("project_entries_ident_levels", proj_stats[PROJ_ARM_ENTRIES_IDENT]), CTR("project_tp_levels", proj_stats[PROJ_ARM_TP]),
    CTR("place_offsets_block_levels", place_block_levels),
    CTR("update_lane_groups", upd_stats[UPD_LANE]), CTR("update_mid_groups", upd_stats[UPD_MID]), CTR("update_wave_tiny_groups", upd_stats[UPD_WAVE_TINY]),
    CTR("update_wave_small_groups", upd_stats[UPD_WAVE_SMALL]), CTR("update_wave_large_groups", upd_stats[UPD_WAVE_LARGE]),
    CTR("update_inplace_groups", upd_stats[UPD_INPLACE]), CTR("update_tiled_sort_groups", upd_stats[UPD_TILED_SORT]),
    CTR("update_lane_spill_groups", upd_stats[UPD_LANE_SPILL]),
    CTR("lookup_wide_windows", lk_stats[LK_WIDE]), CTR("lookup_wide_single", lk_stats[LK_SINGLE]), CTR("lookup_wide_grouped", lk_stats[LK_GROUPED]),
    CTR("lookup_wide_group_passes", lk_stats[LK_GROUP_PASSES]), CTR("lookup_wide_overflow", lk_stats[LK_OVERFLOW]),
    CTR("lookup_coop_waves", lk_stats[LK_COOP]), CTR("lookup_lane_waves_mixed", lk_stats[LK_MIXED]), CTR("lookup_lane_waves_span", lk_stats[LK_SPAN]),
    CTR("refine_passes", refine_stats[REFINE_PASSES]), CTR("refine_candidates", refine_stats[REFINE_CANDIDATES]),
    CTR("refine_parts", refine_stats[REFINE_PARTS]), CTR("refine_rows_to_host", refine_stats[REFINE_ROWS_TO_HOST]),
    CTR("refine_longest_group", refine_stats[REFINE_LONGEST_GROUP]),
    CTR("bed_rows", bed_stats[BED_ROWS]), CTR("bed_gap_roots", bed_stats[BED_GAP_ROOTS]), CTR("bed_runs", bed_stats[BED_RUNS]),
    CTR("bed_text_pieces", bed_stats[BED_TEXT_PIECES]), CTR("bed_text_bytes", bed_stats[BED_TEXT_BYTES]),
    CTR("bedpe_rows", bedpe_stats[BEDPE_ROWS]), CTR("bedpe_runs", bedpe_stats[BEDPE_RUNS]),
    CTR("bedpe_joins_contiguous", bedpe_stats[BEDPE_JOINS_CONTIGUOUS]), CTR("bedpe_joins_gap", bedpe_stats[BEDPE_JOINS_GAP]),
    CTR("bedpe_fused_ops", bedpe_stats[BEDPE_FUSED_OPS]), CTR("bedpe_summary_ops", bedpe_stats[BEDPE_SUMMARY_OPS]),
    CTR("bedpe_text_pieces", bedpe_stats[BEDPE_TEXT_PIECES]), CTR("bedpe_text_bytes", bedpe_stats[BEDPE_TEXT_BYTES]),
    CTR("paf_rows", paf_stats[PAF_ROWS]), CTR("paf_runs", paf_stats[PAF_RUNS]),
    CTR("paf_joins_contiguous", paf_stats[PAF_JOINS_CONTIGUOUS]), CTR("paf_joins_gap", paf_stats[PAF_JOINS_GAP]),
    CTR("paf_ops_read", paf_stats[PAF_OPS_READ]), CTR("paf_ops_printed", paf_stats[PAF_OPS_PRINTED]),
    CTR("paf_through_rows", paf_stats[PAF_THROUGH_ROWS]), CTR("paf_text_pieces", paf_stats[PAF_TEXT_PIECES]),
    CTR("paf_text_bytes", paf_stats[PAF_TEXT_BYTES]),
    CTR("fasta_rows", fasta_stats[FASTA_ROWS]), CTR("fasta_records", fasta_stats[FASTA_RECORDS]),
    CTR("fasta_text_pieces", fasta_stats[FASTA_TEXT_PIECES]), CTR("fasta_text_bytes", fasta_stats[FASTA_TEXT_BYTES]),
    CTR("fasta_store_bytes", fasta_stats[FASTA_STORE_BYTES]), CTR("fasta_store_packed", fasta_stats[FASTA_STORE_PACKED]),
    CTR("fasta_store_exception_runs", fasta_stats[FASTA_STORE_EXCEPTION_RUNS]),
    CTR("sequence_ingest_pieces", ingest_stats[0]), CTR("sequence_ingest_text_bytes", ingest_stats[1]), CTR("sequence_ingest_bases", ingest_stats[2]),
    CTR("sequence_ingest_inflated_blocks", ingest_stats[3]), CTR("sequence_ingest_dropped_sequences", ingest_stats[4]),
    CTR("paf_ingest_device", paf_ingest_stats[0]), CTR("paf_ingest_pieces", paf_ingest_stats[1]), CTR("paf_ingest_text_bytes", paf_ingest_stats[2]),
    CTR("paf_ingest_lines", paf_ingest_stats[3]), CTR("paf_ingest_carried_bytes", paf_ingest_stats[4]),
    CTR("paf_ingest_buffer_grows", paf_ingest_stats[5]), CTR("paf_ingest_pool_regrows", paf_ingest_stats[6]),
    CTR("paf_ingest_unknown_names", paf_ingest_stats[7]), CTR("paf_ingest_inflated_blocks", paf_ingest_stats[8]),
    CTR("resolve_records", resolve_stats[0]), CTR("resolve_resolved", resolve_stats[1]), CTR("resolve_absent", resolve_stats[2]),
    CTR("resolve_inconsistent", resolve_stats[3]), CTR("resolve_ops_in", resolve_stats[4]), CTR("resolve_ops_out", resolve_stats[5]),
    CTR("resolve_m_ops", resolve_stats[6]), CTR("resolve_m_bases", resolve_stats[7]), CTR("resolve_m_eq_bases", resolve_stats[8]),
    CTR("resolve_m_x_bases", resolve_stats[9]), CTR("resolve_bad_eq_bases", resolve_stats[10]), CTR("resolve_bad_x_bases", resolve_stats[11]),
    CTR_RANKS("build_device", build_stats[BUILD_DEVICE]), CTR_RANKS("tokenized_device", build_stats[BUILD_TOKENIZED_DEVICE]),
    CTR_RANKS("build_batches", build_stats[BUILD_BATCHES]),
};
#undef CTR
#undef CTR_RANKS
constexpr size_t N_COUNTERS = sizeof(COUNTER_TABLE) / sizeof(COUNTER_TABLE[0]);

int impg_gpu_get_counter(const impg_gpu_index_t *ix, const char *key, int64_t *value_out) {
  IMPG_TRY
  if (!ix || !key || !value_out) throw Error{IMPG_E_INVALID, "null argument"};
  for (const CounterRow &c : COUNTER_TABLE)
    if (!strcmp(c.key, key)) {
      uint64_t v = 0;
      if (c.over_ranks) for_each_rank(*ix, [&](const impg_gpu_index &r) { v += c.at(r).load(); });
      else v = c.at(*ix).load();
      *value_out = (int64_t)v;
      return IMPG_OK;
    }
  throw Error{IMPG_E_INVALID, std::string("unknown counter ") + key};
  IMPG_CATCH
}
const char *impg_gpu_counter_key(size_t i) { return i < N_COUNTERS ? COUNTER_TABLE[i].key : nullptr; }

int impg_gpu_visit_rank(uint32_t n, int order_policy, uint32_t *rank_out) {
  IMPG_TRY
  if (!rank_out && n) throw Error{IMPG_E_INVALID, "null argument"};
  if (order_policy == IMPG_ORDER_COITREES) coitrees_visit_rank(n, rank_out);
  else if (order_policy == IMPG_ORDER_SORTED) for (uint32_t i = 0; i < n; i++) rank_out[i] = i;
  else throw Error{IMPG_E_INVALID, "bad order policy"};
  return IMPG_OK;
  IMPG_CATCH
}

}  // extern "C"
namespace impg {
// masked_regions -> the engine's device tables (the lease's end clears the flag)
void apply_mask(Engine &E, const impg_gpu_index &ix, const impg_gpu_mask_t *m, const impg_gpu_params_t &p) {
  if (!m) return;
  if (!p.transitive) throw Error{IMPG_E_INVALID, "masked_regions belong to the transitive queries"};
  const uint32_t n_seq = ix.view.n_seq;
  if (m->n_seqs && (!m->seq_id || !m->sequence_length || !m->range_off)) throw Error{IMPG_E_INVALID, "null mask array"};
  const uint64_t total = m->n_seqs ? m->range_off[m->n_seqs] : 0;
  if (total >= 0xFFFFFFF0ull) throw Error{IMPG_E_UNSUPPORTED, "mask exceeds 2^32 ranges"};
  if (total && !m->ranges) throw Error{IMPG_E_INVALID, "null mask array"};
  std::vector<uint32_t> off(n_seq + 1, 0);
  // a sequence absent from the map: Impg starts its set with length 0 (visited_entry, impg.rs:2048-2053), MultiImpg
  // with the real length (multi_impg.rs:919-922) except for the query's own target (entry().or_default(), :827-830)
  std::vector<int32_t> init_len(n_seq, 0), touch_len(n_seq, 0);
  bool has_empty = false;
  if (p.multi_impg) for (uint32_t s = 0; s < n_seq; s++) touch_len[s] = (int32_t)std::min<int64_t>(std::max<int64_t>(ix.seq.lens[s], 0), INT32_MAX);
  for (uint32_t i = 0; i < m->n_seqs; i++) {
    const uint32_t s = m->seq_id[i];
    if (s >= n_seq) throw Error{IMPG_E_INVALID, "mask names an unknown sequence id"};
    if (i && s <= m->seq_id[i - 1]) throw Error{IMPG_E_INVALID, "mask sequence ids must be strictly ascending"};
    if (m->range_off[i + 1] < m->range_off[i]) throw Error{IMPG_E_INVALID, "mask offsets must not decrease"};
    off[s + 1] = (uint32_t)(m->range_off[i + 1] - m->range_off[i]);
    init_len[s] = touch_len[s] = m->sequence_length[i];
    for (uint64_t k = m->range_off[i]; k < m->range_off[i + 1]; k++) {
      const int32_t a = m->ranges[2 * k], b = m->ranges[2 * k + 1];
      if (a > b || (k > m->range_off[i] && a <= m->ranges[2 * k - 1]))  // SortedRanges invariant (impg.rs:330-368)
        throw Error{IMPG_E_INVALID, "mask ranges must be sorted, disjoint and non-touching"};
      has_empty = has_empty || a == b;
    }
  }
  for (uint32_t s = 0; s < n_seq; s++) off[s + 1] += off[s];
  // m->ranges is already in sequence-id order
  E.mask_off.reserve((size_t)(n_seq + 1) * 4);
  E.mask_ranges.reserve(std::max<size_t>(total * 8, 256));
  E.mask_init_len.reserve(std::max<size_t>((size_t)n_seq * 4, 256));
  E.mask_touch_len.reserve(std::max<size_t>((size_t)n_seq * 4, 256));
  IMPG_HIP(hipMemcpy(E.mask_off.p, off.data(), (size_t)(n_seq + 1) * 4, hipMemcpyHostToDevice));
  ix.mask_table_uploads++;
  if (total) { IMPG_HIP(hipMemcpy(E.mask_ranges.p, m->ranges, total * 8, hipMemcpyHostToDevice)); ix.mask_table_uploads++; }
  if (n_seq) {
    IMPG_HIP(hipMemcpy(E.mask_init_len.p, init_len.data(), (size_t)n_seq * 4, hipMemcpyHostToDevice));
    IMPG_HIP(hipMemcpy(E.mask_touch_len.p, touch_len.data(), (size_t)n_seq * 4, hipMemcpyHostToDevice));
    ix.mask_table_uploads += 2;
  }
  E.masked = true;
  E.mask_has_empty = has_empty;
  E.mask_ranges_total = total;
  E.mask_lists = m->n_seqs;
}
void apply_subset(Engine &E, const impg_gpu_index &ix, const uint8_t *subset_keep) {
  if (!subset_keep) return;
  const size_t ns = ix.view.n_seq;
  E.subset_keep.reserve(std::max<size_t>(ns, 256));
  if (ns) IMPG_HIP(hipMemcpy(E.subset_keep.p, subset_keep, ns, hipMemcpyHostToDevice));
  E.subset_on = true;
}
}  // namespace impg
extern "C" {

int impg_gpu_query_batch(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                         impg_gpu_results_t **out) {
  return impg_gpu_query_batch_masked(ix, ranges, n, params, nullptr, out);
}

int impg_gpu_query_batch_masked(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n,
                                const impg_gpu_params_t *params, const impg_gpu_mask_t *mask, impg_gpu_results_t **out) {
  return impg_gpu_query_batch_filtered(ix, ranges, n, params, mask, nullptr, out);
}

int impg_gpu_query_batch_filtered(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n,
                                  const impg_gpu_params_t *params, const impg_gpu_mask_t *mask, const uint8_t *subset_keep,
                                  impg_gpu_results_t **out) {
  IMPG_TRY
  if (!ix || !params || !out || (!ranges && n)) throw Error{IMPG_E_INVALID, "null argument"};
  check_ranges(ranges, n);
  Engine::check_params(*params);
  if (ix->shard || ix->cluster) return sharded_query_batch(*ix, ranges, n, *params, mask, subset_keep, out);
  IMPG_HIP(hipSetDevice(ix->device));
  EngineLease lease(*ix);
  Engine &E = *lease;
  apply_mask(E, *ix, mask, *params);
  apply_subset(E, *ix, subset_keep);
  auto res = std::make_unique<impg_gpu_results>();
  res->approximate = ix->tp_mode;  // (run_small and the walk step aside on a tracepoint index: the object below is the one returned)
  if (n && n <= Engine::SMALL_RANGES && !params->transitive) {  // the per-call shape: one chain of launches, one sync
    const auto c0 = std::chrono::steady_clock::now();
    if (E.run_small(*ix, ranges, (uint32_t)n, *params, *res)) {
      res->run_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count();
      *out = res.release();
      return IMPG_OK;
    }
  }
  const impg_gpu_range_t *d_ranges = upload_ranges(E.ranges_dev, ranges, n, &E.stream);
  if (n < (1ull << 31) && E.walk_applicable(*ix, (uint32_t)n, *params)) {  // small transitive batches, DFS batches: one launch
    const auto c0 = std::chrono::steady_clock::now();
    if (walk_query(*ix, E, (uint32_t)n, *params, *res)) {
      res->run_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count();
      res->ranges.assign(ranges, ranges + n);
      *out = res.release();
      return IMPG_OK;
    }
    res = std::make_unique<impg_gpu_results>();  // (a query outgrew its slab: the batch engine takes the batch)
  }
  res->offsets.assign(1, 0);
  for_chunks(E, n, [&](size_t b, size_t e) {
    impg_gpu_results part;
    run_chunk_rows(*ix, E, d_ranges, ranges, b, e, *params, part);
    ix->result_rows_to_host += part.intervals.size();
    append_results(*res, part);
  });
  res->ranges.assign(ranges, ranges + n);
  *out = res.release();
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_query(impg_gpu_index_t *ix, uint32_t target_id, int32_t start, int32_t end, const impg_gpu_params_t *params,
                   impg_gpu_results_t **out) {
  impg_gpu_range_t r{target_id, start, end};
  return impg_gpu_query_batch(ix, &r, 1, params, out);
}

// The trait's rows for a batch that does not fit one result object (the headline's 100 000 ranges return 2.1 x 10^9 rows,
// 51 GB; the reference prints range by range, main.rs:7435-7470): chunks of the batch are computed on two engines in
// turn, each chunk's rows placed on the device and copied into that engine's pinned block while the other engine
// computes the next chunk, and handed to the callback in range order.
int impg_gpu_query_batch_stream(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                                const impg_gpu_mask_t *mask, const uint8_t *subset_keep, size_t chunk_ranges, size_t max_block_bytes,
                                impg_gpu_stream_cb cb, void *ctx, uint64_t *projected_out) {
  IMPG_TRY
  if (!ix) throw Error{IMPG_E_INVALID, "null argument"};
  // On a rank's shard the call is collective and opens with an agreement on the number of chunks: a rank whose own
  // arguments are refused must still take part in it -- its peers are already waiting there -- and says so with the word it
  // contributes, so that every rank leaves together (the refused one with its own error).
  const bool collective = ix->shard && !ix->cluster;
  std::exception_ptr refused;
  try {
    if (!params || !cb || (!ranges && n)) throw Error{IMPG_E_INVALID, "null argument"};
    check_ranges(ranges, n);
    Engine::check_params(*params);
  } catch (...) {
    if (!collective) throw;
    refused = std::current_exception();
  }
  if (!chunk_ranges) chunk_ranges = 8192;
  if (!max_block_bytes) max_block_bytes = 5ull << 29;  // 2.5 GiB: two such blocks go back into the pinned pool (6 GiB) after the call
  const uint64_t max_rows = std::max<uint64_t>(1, max_block_bytes / sizeof(impg_gpu_interval_t));
  uint64_t projected = 0;
  if (ix->shard || ix->cluster) {
    // a sharded index: the chunks one after the other through the collective call.  On a rank's shard (one process per
    // GPU) every chunk is a collective: the ranks agree on the number of calls first -- each brings its own n, so the
    // counts differ -- and a rank that has run out of ranges, or whose consumer has stopped it, keeps taking part with
    // empty chunks until the longest stream is through (its peers' hops need its shard).
    uint64_t my_chunks = std::max<uint64_t>(1, (n + chunk_ranges - 1) / chunk_ranges), n_chunks = my_chunks;
    if (collective) {
      n_chunks = shard_agree_max(*ix, refused ? ~0ull : my_chunks);
      if (refused) std::rethrow_exception(refused);
      if (n_chunks == ~0ull) throw Error{IMPG_E_INVALID, "a peer rank's arguments to the row stream were refused: no rank runs it"};
    }
    bool cancelled = false;
    for (uint64_t c = 0; c < n_chunks; c++) {
      const size_t b = cancelled ? n : std::min<size_t>(n, (size_t)c * chunk_ranges), e = cancelled ? n : std::min(n, b + chunk_ranges);
      impg_gpu_results_t *part = nullptr;
      const int rc = sharded_query_batch(*ix, ranges + b, e - b, *params, mask, subset_keep, &part);
      if (rc != IMPG_OK) return rc;
      std::unique_ptr<impg_gpu_results> own(part);
      projected += part->projected;
      if (e > b && cb(ctx, part, b) != 0) {
        cancelled = true;
        if (ix->cluster) break;  // (one caller, no peers waiting)
      }
    }
    if (cancelled) throw Error{IMPG_E_CANCELLED, "the row stream's consumer stopped it"};
    if (projected_out) *projected_out = projected;
    return IMPG_OK;
  }
  IMPG_HIP(hipSetDevice(ix->device));
  struct Shared {
    std::mutex m;
    std::condition_variable cv;
    size_t next_begin = 0, chunk = 0;
    uint64_t next_seq = 0, deliver_seq = 0;
    bool stop = false;
    std::mutex gpu;  // whose kernels are on the GPU (two chunks' kernels side by side evict each other's lines from L2)
    std::exception_ptr err;
    uint64_t projected = 0;
  } sh;
  sh.chunk = chunk_ranges;
  auto worker = [&]() {
    try {
      IMPG_HIP(hipSetDevice(ix->device));
      EngineLease lease(*ix);
      Engine &E = *lease;
      apply_mask(E, *ix, mask, *params);
      apply_subset(E, *ix, subset_keep);
      const impg_gpu_range_t *d_ranges = upload_ranges(E.ranges_dev, ranges, n, &E.stream);
      struct Ev {  // (an event of the call's own: the engine recycles its pool run by run)
        hipEvent_t e = nullptr;
        Ev() { IMPG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
        ~Ev() { if (e) (void)hipEventDestroy(e); }
      } done_ev;
      hipEvent_t done = done_ev.e;
      impg_gpu_results part;  // reused chunk after chunk: its pinned arrays grow to the largest chunk and stay
      for (;;) {
        size_t b, e;
        uint64_t seq;
        {
          std::unique_lock<std::mutex> lk(sh.m);
          if (sh.stop || sh.next_begin >= n) break;
          b = sh.next_begin; e = std::min(n, b + sh.chunk);
          sh.next_begin = e; seq = sh.next_seq++;
        }
        // the chunk, in pieces if it outgrows the pair budget or the block (pieces are delivered in order within the turn)
        std::vector<std::pair<size_t, size_t>> todo{{b, e}};
        while (!todo.empty()) {
          const auto [pb, pe] = todo.back();
          todo.pop_back();
          std::unique_lock<std::mutex> turn(sh.gpu);  // passed on once the chunk's kernels have run: its copies overlap the other engine's kernels
          try {
            part.offsets.clear(); part.intervals.clear(); part.cigar_off.clear(); part.cigar_ops.clear();
            run_chunk_rows(*ix, E, d_ranges, ranges, pb, pe, *params, part, nullptr, max_rows, done, [&]() { turn.unlock(); });
            ix->result_rows_to_host += part.intervals.size();
          } catch (const SplitBatch &) {
            if (pe - pb <= 1) throw Error{IMPG_E_UNSUPPORTED, "a single range exceeds the pair budget"};
            const size_t mid = pb + (pe - pb) / 2;
            {  // (the chunks still to be dealt start at the size that fitted: a split costs the run that found it out)
              std::lock_guard<std::mutex> lk(sh.m);
              sh.chunk = std::min(sh.chunk, std::max<size_t>(1, (pe - pb) / 2));
            }
            todo.push_back({mid, pe});
            todo.push_back({pb, mid});
            continue;
          }
          if (turn.owns_lock()) turn.unlock();
          // in range order: this chunk's turn comes when every earlier chunk has been handed over
          std::unique_lock<std::mutex> lk(sh.m);
          sh.cv.wait(lk, [&] { return sh.stop || sh.deliver_seq == seq; });
          if (sh.stop) break;
          sh.projected += part.projected;
          lk.unlock();
          if (cb(ctx, &part, pb) != 0) throw Error{IMPG_E_CANCELLED, "the row stream's consumer stopped it"};
        }
        std::lock_guard<std::mutex> lk(sh.m);
        if (sh.stop) break;
        sh.deliver_seq = seq + 1;
        sh.cv.notify_all();
      }
    } catch (...) {
      std::lock_guard<std::mutex> lk(sh.m);
      if (!sh.err) sh.err = std::current_exception();
      sh.stop = true;
      sh.cv.notify_all();
    }
  };
  if (n) {
    std::thread second(worker);
    worker();
    second.join();
  }
  if (sh.err) std::rethrow_exception(sh.err);
  if (projected_out) *projected_out = sh.projected;
  return IMPG_OK;
  IMPG_CATCH
}

size_t impg_gpu_results_num_ranges(const impg_gpu_results_t *r) { return r->offsets.empty() ? 0 : r->offsets.size() - 1; }
size_t impg_gpu_results_total(const impg_gpu_results_t *r) { return r->intervals.size(); }
const uint64_t *impg_gpu_results_offsets(const impg_gpu_results_t *r) { return r->offsets.data(); }
const impg_gpu_interval_t *impg_gpu_results_intervals(const impg_gpu_results_t *r) { return r->intervals.data(); }
uint64_t impg_gpu_results_projected(const impg_gpu_results_t *r) { return r->projected; }
const uint64_t *impg_gpu_results_cigar_offsets(const impg_gpu_results_t *r) { return r->has_cigar ? r->cigar_off.data() : nullptr; }
const uint32_t *impg_gpu_results_cigar_ops(const impg_gpu_results_t *r) { return r->has_cigar ? r->cigar_ops.data() : nullptr; }
void impg_gpu_results_timing(const impg_gpu_results_t *r, double *engine_s, double *assemble_s) {
  if (engine_s) *engine_s = r ? r->run_s : 0;
  if (assemble_s) *assemble_s = r ? r->assemble_s : 0;
}
void impg_gpu_results_free(impg_gpu_results_t *r) { delete r; }

static int stats_impl(impg_gpu_index_t *ix, Engine &E, const impg_gpu_range_t *d_ranges, size_t n, const impg_gpu_params_t *params,
                      uint64_t *per_range_count, uint64_t *per_range_checksum, impg_gpu_stats_t *stats) {
  const StatSinks sinks(E.stat_count, E.stat_cksum, per_range_count, per_range_checksum, n, &E.stream);
  impg_gpu_stats_t tot;
  memset(&tot, 0, sizeof tot);
  for_chunks(E, n, [&](size_t b, size_t e) {
    impg_gpu_stats_t st;
    RunSpec rs(d_ranges + b, (uint32_t)(e - b), *params);
    rs.stats = &st;
    sinks.aim(rs, b);
    // a split retry must not double-count the slice
    if (rs.d_count) IMPG_HIP(hipMemsetAsync(rs.d_count, 0, (e - b) * 8, E.stream));
    if (rs.d_cksum) IMPG_HIP(hipMemsetAsync(rs.d_cksum, 0, (e - b) * 8, E.stream));
    E.run(*ix, rs);
    add_stats(tot, st);
  });
  if (stats) *stats = tot;
  sinks.home(per_range_count, per_range_checksum, n);
  return IMPG_OK;
}

int impg_gpu_query_batch_stats(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                               uint64_t *per_range_count, uint64_t *per_range_checksum, impg_gpu_stats_t *stats) {
  IMPG_TRY
  if (!ix || !params || (!ranges && n)) throw Error{IMPG_E_INVALID, "null argument"};
  check_ranges(ranges, n);
  Engine::check_params(*params);
  if (ix->shard || ix->cluster) return sharded_query_stats(*ix, ranges, false, n, *params, per_range_count, per_range_checksum, stats);
  IMPG_HIP(hipSetDevice(ix->device));
  EngineLease lease(*ix);
  Engine &E = *lease;
  return stats_impl(ix, E, upload_ranges(E.ranges_dev, ranges, n, &E.stream), n, params, per_range_count, per_range_checksum, stats);
  IMPG_CATCH
}

int impg_gpu_query_batch_stats_dev(impg_gpu_index_t *ix, const impg_gpu_range_t *d_ranges, size_t n,
                                   const impg_gpu_params_t *params, uint64_t *per_range_count,
                                   uint64_t *per_range_checksum, impg_gpu_stats_t *stats) {
  IMPG_TRY
  if (!ix || !params || (!d_ranges && n)) throw Error{IMPG_E_INVALID, "null argument"};
  if (n >= (1ull << 31)) throw Error{IMPG_E_UNSUPPORTED, "more than 2^31 ranges in one batch"};
  Engine::check_params(*params);
  if (ix->cluster) throw Error{IMPG_E_INVALID, "device-resident ranges belong to one GPU: a multi-GPU handle takes host ranges"};
  if (ix->shard) return sharded_query_stats(*ix, d_ranges, true, n, *params, per_range_count, per_range_checksum, stats);
  IMPG_HIP(hipSetDevice(ix->device));
  EngineLease lease(*ix);
  return stats_impl(ix, *lease, d_ranges, n, params, per_range_count, per_range_checksum, stats);
  IMPG_CATCH
}

// ---- rows left in HBM ------------------------------------------------------------------------------------------------
// impg_gpu_query_batch_device: the batch's result rows stay on the device, complete -- what SURVEY.md 8(d) calls the result
// record: {range_idx, query_id, q_first, q_last, t_first, t_last} -- for a consumer that lives there too (the BED merges of
// bed_device.hip are one; a caller's own kernels another).  The handle keeps the engine it ran on (its buffers are the
// engine's pooled blocks) until it is freed.
struct impg_gpu_device_rows {
  // (declared first, destroyed last: the chunks' buffers go back to the engine's pool while the lease still holds it)
  std::unique_ptr<impg::EngineLease> lease;
  struct Chunk {
    size_t first = 0, n = 0;
    std::vector<std::unique_ptr<impg::LevelBufs>> levels;  // IMPG_ROWS_ATTRIBUTED
    impg::DevBuf rows, offsets;                            // IMPG_ROWS_ORDERED: impg_gpu_interval_t[n_rows], u32 [n + 1]
    uint64_t n_rows = 0;
  };
  std::vector<std::unique_ptr<Chunk>> chunks;  // (a chunk owns device buffers: not movable)
  struct Part { size_t chunk; size_t level; };
  std::vector<Part> parts;
  // a sharded index: every rank's share (one in a rank process), parts numbered rank by rank; offset / total of the
  // caller's ranges in the collective batch
  std::vector<std::unique_ptr<impg::ShardRows>> shard_rows;
  std::vector<std::pair<size_t, size_t>> shard_parts;  // (rank share, part)
  uint64_t batch_offset = 0, batch_total = 0;
  impg_gpu_index *ix = nullptr;
  impg_gpu_params_t params{};
  size_t n = 0;
  int layout = 0;
  impg_gpu_stats_t stats{};
  float ms_place = 0;  // ordered layout: HIP-event time of the row placement
};

int impg_gpu_query_batch_device(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, int ranges_on_device,
                                const impg_gpu_params_t *params, int layout, impg_gpu_device_rows_t **out) {
  return impg::query_batch_device_filtered(ix, ranges, n, ranges_on_device, params, layout, nullptr, out);
}
}  // extern "C"
// ... with the subset filter of impg_gpu_query_batch_filtered (one GPU only): what refine's passes call (refine.cpp)
int impg::query_batch_device_filtered(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, int ranges_on_device,
                                      const impg_gpu_params_t *params, int layout, const uint8_t *subset_keep, impg_gpu_device_rows_t **out) {
  IMPG_TRY
  if (!ix || !params || !out || (!ranges && n)) throw Error{IMPG_E_INVALID, "null argument"};
  if (subset_keep && (ix->shard || ix->cluster)) throw Error{IMPG_E_UNSUPPORTED, "rows left on the device take a subset filter on one GPU only"};
  if (layout != IMPG_ROWS_ATTRIBUTED && layout != IMPG_ROWS_ORDERED && layout != IMPG_ROWS_ORDERED_SLOTS) throw Error{IMPG_E_INVALID, "unknown row layout"};
  if (n >= (1ull << 31)) throw Error{IMPG_E_UNSUPPORTED, "more than 2^31 ranges in one batch"};
  if (!ranges_on_device) check_ranges(ranges, n);
  Engine::check_params(*params);
  if (ix->shard || ix->cluster) {
    // The final level stays with the ranks that project it (sharded.cpp rank_rows); the ranges are numbered in the collective
    // batch.  Ordered layouts need that level at home in emission order: not offered here.
    if (layout != IMPG_ROWS_ATTRIBUTED)
      throw Error{IMPG_E_UNSUPPORTED, "a sharded index leaves its rows on the device in the attributed layout only (IMPG_ROWS_ATTRIBUTED)"};
    if (params->store_cigar || params->multi_impg || (params->transitive && params->dfs))
      throw Error{IMPG_E_UNSUPPORTED, "impg_gpu_query_batch_device on a sharded index takes Impg::query and query_transitive_bfs without store_cigar"};
    if (ix->cluster && ranges_on_device) throw Error{IMPG_E_INVALID, "device-resident ranges belong to one GPU: a multi-GPU handle takes host ranges"};
    auto h = std::make_unique<impg_gpu_device_rows>();
    h->ix = ix;
    h->params = *params;
    h->n = n;
    h->layout = layout;
    sharded_query_device(*ix, ranges, ranges_on_device != 0, n, *params, h->shard_rows, &h->stats);
    for (size_t r = 0; r < h->shard_rows.size(); r++)
      for (size_t k = 0; k < h->shard_rows[r]->parts.size(); k++) h->shard_parts.push_back({r, k});
    h->batch_offset = ix->cluster ? 0 : h->shard_rows[0]->offset;
    h->batch_total = h->shard_rows[0]->total;
    *out = h.release();
    return IMPG_OK;
  }
  if (params->store_cigar || params->multi_impg || (params->transitive && params->dfs))
    throw Error{IMPG_E_UNSUPPORTED, "impg_gpu_query_batch_device takes Impg::query and query_transitive_bfs without store_cigar"};
  IMPG_HIP(hipSetDevice(ix->device));
  auto h = std::make_unique<impg_gpu_device_rows>();
  h->lease = std::make_unique<EngineLease>(*ix);
  Engine &E = **h->lease;
  // (the slot arrays of a big batch are tens of GB: they go back to the engine's pool when the handle is freed and are
  // the next call's -- the pool's default cap would hipFree / hipMalloc them call after call)
  E.level_pool.max_held = std::max<size_t>(E.level_pool.max_held, (size_t)ix->opt.device_rows_pool_bytes);
  h->ix = ix;
  h->params = *params;
  h->n = n;
  h->layout = layout;
  apply_subset(E, *ix, subset_keep);
  const impg_gpu_range_t *d_ranges = ranges_on_device ? ranges : upload_ranges(E.ranges_dev, ranges, n, &E.stream);
  impg_gpu_stats_t tot;
  memset(&tot, 0, sizeof tot);
  for_chunks(E, n, [&](size_t b, size_t e) {
    auto cp = std::make_unique<impg_gpu_device_rows::Chunk>();
    impg_gpu_device_rows::Chunk &c = *cp;
    c.first = b; c.n = e - b;
    impg_gpu_stats_t st;
    DevBuf self_dev;
    self_dev.pool = &E.level_pool;
    RunSpec rs(d_ranges + b, (uint32_t)(e - b), *params);
    rs.keep = &c.levels;
    rs.stats = &st;
    rs.self_out = layout != IMPG_ROWS_ATTRIBUTED ? &self_dev : nullptr;
    // attributed: a slot names its frontier record (pair_range), so the final level may be fused like a counting run's;
    // ordered: every level's slots are runs in visit order, placed below
    rs.keep_any_order = layout == IMPG_ROWS_ATTRIBUTED;
    rs.ordered_rows = layout == IMPG_ROWS_ORDERED_SLOTS;  // rows placed slot by slot, the fused final level's by its own kernel
    E.run(*ix, rs);
    if (layout == IMPG_ROWS_ORDERED_SLOTS) {
      c.rows.adopt(E.ord_rows);
      c.offsets.adopt(E.ord_offsets);
      c.n_rows = E.ord_total;
      h->ms_place += E.ms_place;
      c.levels.clear();
    }
    if (layout == IMPG_ROWS_ORDERED) {  // the trait's rows (rows_device.hip), left where they are built
      hipEvent_t r0 = E.event(), r1 = E.event();
      IMPG_HIP(hipEventRecord(r0, E.stream));
      RowPlan pl;
      plan_rows(E, (uint32_t)(e - b), *params, c.levels, self_dev, false, pl);
      c.rows.pool = &E.level_pool;
      c.rows.reserve(std::max<size_t>((size_t)pl.n_rows * sizeof(impg_gpu_interval_t), 256));
      scatter_rows(E, c.levels, pl, RowSinks{c.rows.as<impg_gpu_interval_t>(), nullptr, nullptr, nullptr, nullptr, nullptr});
      IMPG_HIP(hipEventRecord(r1, E.stream));
      IMPG_HIP(hipStreamSynchronize(E.stream));
      float ms = 0;
      IMPG_HIP(hipEventElapsedTime(&ms, r0, r1));
      h->ms_place += ms;
      c.offsets.adopt(pl.offsets);
      c.n_rows = pl.n_rows;
      c.levels.clear();
    }
    add_stats(tot, st);
    h->chunks.push_back(std::move(cp));
  });
  for (size_t c = 0; c < h->chunks.size(); c++) {
    if (layout != IMPG_ROWS_ATTRIBUTED) h->parts.push_back({c, 0});
    else for (size_t l = 0; l < h->chunks[c]->levels.size(); l++) h->parts.push_back({c, l});
  }
  h->stats = tot;
  h->batch_total = n;
  *out = h.release();
  return IMPG_OK;
  IMPG_CATCH
}
extern "C" {

static size_t num_parts(const impg_gpu_device_rows_t *h) { return h->shard_rows.empty() ? h->parts.size() : h->shard_parts.size(); }
size_t impg_gpu_device_rows_num_parts(const impg_gpu_device_rows_t *h) { return h ? num_parts(h) : 0; }
int impg_gpu_device_rows_part(const impg_gpu_device_rows_t *h, size_t k, impg_gpu_device_part_t *out) {
  IMPG_TRY
  if (!h || !out || k >= num_parts(h)) throw Error{IMPG_E_INVALID, "no such part"};
  memset(out, 0, sizeof *out);
  const LevelBufs *Lp = nullptr;
  if (!h->shard_rows.empty()) {
    const ShardRowsPart &pt = h->shard_rows[h->shard_parts[k].first]->parts[h->shard_parts[k].second];
    out->first_range = pt.first_range;
    out->n_ranges = pt.n_ranges;
    out->level = pt.level;
    Lp = pt.L.get();
  } else {
    const auto &c = *h->chunks[h->parts[k].chunk];
    out->first_range = c.first;
    out->n_ranges = c.n;
    if (h->layout != IMPG_ROWS_ATTRIBUTED) {
      out->n_slots = c.n_rows;
      out->rows = c.rows.as<impg_gpu_interval_t>();
      out->offsets = c.offsets.as<uint32_t>();
      return IMPG_OK;
    }
    Lp = c.levels[h->parts[k].level].get();
    out->level = (uint32_t)h->parts[k].level;
  }
  const LevelBufs &L = *Lp;
  out->n_slots = L.n_pairs;
  out->n_frontier = L.n_frontier;
  out->query_id = L.qid.as<uint32_t>();
  out->coords = L.coords.as<int32_t>();
  // (a fused final level stores a slot's query id and source as one pair: one store instruction in the kernel instead of two)
  out->source = L.qs_interleaved ? L.qid.as<uint32_t>() + 1 : L.pair_range.as<uint32_t>();
  out->slot_stride = L.qs_interleaved ? 2u : 1u;
  out->frontier = L.frontier.as<impg_gpu_frontier_t>();
  return IMPG_OK;
  IMPG_CATCH
}
int impg_gpu_device_rows_part_device(const impg_gpu_device_rows_t *h, size_t k, int *device_out) {
  IMPG_TRY
  if (!h || !device_out || k >= num_parts(h)) throw Error{IMPG_E_INVALID, "no such part"};
  *device_out = h->shard_rows.empty() ? h->ix->device : h->shard_rows[h->shard_parts[k].first]->device;
  return IMPG_OK;
  IMPG_CATCH
}
int impg_gpu_device_rows_batch_offset(const impg_gpu_device_rows_t *h, uint64_t *offset_out, uint64_t *total_out) {
  IMPG_TRY
  if (!h) throw Error{IMPG_E_INVALID, "null argument"};
  if (offset_out) *offset_out = h->batch_offset;
  if (total_out) *total_out = h->batch_total;
  return IMPG_OK;
  IMPG_CATCH
}
void impg_gpu_device_rows_stats(const impg_gpu_device_rows_t *h, impg_gpu_stats_t *stats) {
  if (h && stats) *stats = h->stats;
}
float impg_gpu_device_rows_place_ms(const impg_gpu_device_rows_t *h) { return h ? h->ms_place : 0.f; }
// the per-range counts and checksums of impg_gpu_query_batch_stats, recomputed from the rows the call left in HBM
int impg_gpu_device_rows_check(impg_gpu_device_rows_t *h, uint64_t *per_range_count, uint64_t *per_range_checksum) {
  IMPG_TRY
  if (!h) throw Error{IMPG_E_INVALID, "null argument"};
  if (h->layout != IMPG_ROWS_ATTRIBUTED) throw Error{IMPG_E_UNSUPPORTED, "impg_gpu_device_rows_check reads the attributed layout (ordered rows: compare them with impg_gpu_query_batch's)"};
  if (!h->shard_rows.empty()) {  // (collective in rank processes: partial sums go to their homes)
    sharded_rows_check(*h->ix, h->shard_rows, h->params, per_range_count, per_range_checksum);
    return IMPG_OK;
  }
  Engine &E = **h->lease;
  IMPG_HIP(hipSetDevice(h->ix->device));
  const size_t n = h->n;
  E.stat_count.reserve(std::max<size_t>(n * 8, 256));
  E.stat_cksum.reserve(std::max<size_t>(n * 8, 256));
  IMPG_HIP(hipMemsetAsync(E.stat_count.p, 0, std::max<size_t>(n * 8, 8), E.stream));
  IMPG_HIP(hipMemsetAsync(E.stat_cksum.p, 0, std::max<size_t>(n * 8, 8), E.stream));
  for (auto &cp : h->chunks)
    for (auto &Lp : cp->levels) {
      auto &c = *cp;
      LevelBufs &L = *Lp;
      if (!L.n_pairs) continue;
      HitArrays ha{L.qid.as<uint32_t>(), L.coords.as<int4>()};
      E.rstat.reserve(std::max<size_t>((size_t)L.n_frontier * 16, 256));
      launch_hit_stats(L.frontier.as<FrontierRec>(), L.n_frontier, L.qs_interleaved ? L.qid.as<uint32_t>() + 1 : L.pair_range.as<uint32_t>(), L.n_pairs, ha,
                       h->params.transitive ? h->params.min_output_length : -1, false, E.rstat.as<unsigned long long>(),
                       E.stat_count.as<unsigned long long>() + c.first, E.stat_cksum.as<unsigned long long>() + c.first, E.stream,
                       L.qs_interleaved ? 2u : 1u);
    }
  IMPG_HIP(hipStreamSynchronize(E.stream));
  if (per_range_count && n) IMPG_HIP(hipMemcpy(per_range_count, E.stat_count.p, n * 8, hipMemcpyDeviceToHost));
  if (per_range_checksum && n) IMPG_HIP(hipMemcpy(per_range_checksum, E.stat_cksum.p, n * 8, hipMemcpyDeviceToHost));
  return IMPG_OK;
  IMPG_CATCH
}
void impg_gpu_device_rows_free(impg_gpu_device_rows_t *h) {
  if (!h) return;
  if (h->ix) (void)hipSetDevice(h->ix->device);
  delete h;
}

long impg_gpu_bed_merge(impg_gpu_interval_t *iv, size_t n, int32_t merge_distance, int merge_strands) {
  try {
    return (long)bed_merge(iv, n, merge_distance, merge_strands != 0);
  } catch (...) {
    impg::set_error("bed_merge failed");
    return IMPG_E_OOM;
  }
}

int impg_gpu_results_bed(const impg_gpu_results_t *res, const impg_gpu_index_t *ix, const char *const *range_names,
                         const impg_gpu_params_t *params, int32_t merge_distance, char **text, size_t *len) {
  IMPG_TRY
  if (!res || !ix || !params || !text || !len) throw Error{IMPG_E_INVALID, "null argument"};
  std::vector<std::string> parts;
  render_bed(*res, *ix, range_names, *params, merge_distance, parts);
  *text = join_parts(parts, len);
  return IMPG_OK;
  IMPG_CATCH
}

// query + merge + the text on the device: only text crosses PCIe, in pinned pieces.  BED: both BED merges
// (bed_device.hip); BEDPE: the CIGAR summaries and merge_adjusted_intervals (bedpe_device.hip).
namespace {
// what the device BEDPE and PAF routes do not serve (the host route, impg_gpu_results_paf, does): raised before anything runs
void bedpe_refusals(const impg_gpu_index &ix, const std::string &what = "BEDPE") {
  if (ix.shard || ix.cluster) throw Error{IMPG_E_UNSUPPORTED, "device-side " + what + " on a sharded index (use impg_gpu_query_batch + impg_gpu_results_paf)"};
  // an op is no longer than the sequence it lies on; a fused op of 2^29 bases or more would wrap into its code bits on the
  // host route (CigarOp::new, impg.rs:90-92), which the sums here do not restate
  for (const int64_t len : ix.seq.lens)
    if (len >= (int64_t)OP_LEN_MASK + 1) throw Error{IMPG_E_UNSUPPORTED, "device-side " + what + " on an index with a sequence of 2^29 bases or more (use impg_gpu_results_paf)"};
  if (ix.tp_mode && !ix.opt.approximate_cigar)
    throw Error{IMPG_E_UNSUPPORTED, "store_cigar on a tracepoint index needs option approximate_cigar = 1 (the approximate mode's "
                                    "CIGAR is a pair of match / mismatch counts, not an alignment)"};
}
// ... and PAF: the reference prints no PAF in approximate mode (render_paf refuses it with the same words)
void paf_refusals(const impg_gpu_index &ix) {
  if (ix.tp_mode)
    throw Error{IMPG_E_UNSUPPORTED, "PAF output of approximate-mode results: the reference offers bed and bedpe there (their CIGAR "
                                    "is a pair of match / mismatch counts, not an alignment)"};
  bedpe_refusals(ix, "PAF");
}
// ... and FASTA: raised before anything runs
void fasta_refusals(const impg_gpu_index &ix) {
  if (ix.shard || ix.cluster) throw Error{IMPG_E_UNSUPPORTED, "device-side FASTA on a sharded index"};
  if (!ix.seq_store) throw Error{IMPG_E_INVALID, "FASTA output needs a sequence store (impg_gpu_index_set_sequences)"};
}
void text_batch(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params, const uint8_t *subset_keep,
                int32_t merge_distance, const char *const *range_names, const std::function<void(const char *, size_t)> &sink,
                double *seconds3, TextFormat format) {
  if (!ix || !params || (!ranges && n)) throw Error{IMPG_E_INVALID, "null argument"};
  check_ranges(ranges, n);
  Engine::check_params(*params);
  impg_gpu_params_t p = *params;
  const bool fasta = format == TEXT_FASTA || format == TEXT_FASTA_RC;
  p.store_cigar = format != TEXT_BED && !fasta ? 1 : 0;  // BED and FASTA never need CIGARs, BEDPE rates them, PAF prints them (main.rs:7447)
  if (fasta) fasta_refusals(*ix);
  else if (format == TEXT_BEDPE) bedpe_refusals(*ix);
  else if (format == TEXT_PAF) paf_refusals(*ix);
  else if (ix->shard || ix->cluster) { sharded_bed_batch(*ix, ranges, n, p, subset_keep, merge_distance, range_names, sink, seconds3); return; }
  IMPG_HIP(hipSetDevice(ix->device));
  EngineLease lease(*ix);
  Engine &E = *lease;
  if (fasta) ix->fasta_stats_reset();
  else if (format == TEXT_BEDPE) ix->bedpe_stats_reset();
  else if (format == TEXT_PAF) ix->paf_stats_reset();
  else ix->bed_stats_reset();
  apply_subset(E, *ix, subset_keep);
  const impg_gpu_range_t *d_ranges = upload_ranges(E.ranges_dev, ranges, n, &E.stream);
  double t3[3] = {0, 0, 0};  // engine, merge, text
  for_chunks(E, n, [&](size_t b, size_t e) { run_chunk_bed(*ix, E, d_ranges, ranges, range_names, b, e, p, merge_distance, sink, t3, nullptr, format); });
  if (seconds3) for (int k = 0; k < 3; k++) seconds3[k] = t3[k];
}
// a text as the caller gets it: malloc'ed and NUL-terminated behind its bytes
char *malloc_text(const std::string &s) {
  char *t = (char *)malloc(s.size() + 1);
  if (!t) throw Error{IMPG_E_OOM, "host out of memory"};
  memcpy(t, s.data(), s.size());
  t[s.size()] = 0;
  return t;
}
// the text arrives in pieces; it is collected into one malloc'ed buffer that grows geometrically
int text_batch_buffer(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params, const uint8_t *subset_keep,
                      int32_t merge_distance, const char *const *range_names, char **text, size_t *len, double *seconds3, TextFormat format) {
  IMPG_TRY
  if (!text || !len) throw Error{IMPG_E_INVALID, "null argument"};
  char *buf = nullptr;
  size_t used = 0, cap = 0;
  struct Guard { char *&b; bool keep = false; ~Guard() { if (!keep) free(b); } } guard{buf};
  text_batch(ix, ranges, n, params, subset_keep, merge_distance, range_names, [&](const char *p, size_t k) {
    if (used + k + 1 > cap) {
      const size_t nc = std::max(cap * 2, used + k + 1 + (1u << 20));
      char *nb = (char *)realloc(buf, nc);
      if (!nb) throw Error{IMPG_E_OOM, "host out of memory"};
      buf = nb; cap = nc;
    }
    memcpy(buf + used, p, k);
    used += k;
  }, seconds3, format);
  if (!buf) buf = malloc_text(std::string());
  buf[used] = 0;
  guard.keep = true;
  *text = buf;
  *len = used;
  return IMPG_OK;
  IMPG_CATCH
}
int text_batch_fd(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params, const uint8_t *subset_keep,
                  int32_t merge_distance, const char *const *range_names, int fd, uint64_t *bytes_written, double *seconds3, TextFormat format) {
  IMPG_TRY
  uint64_t total = 0;
  text_batch(ix, ranges, n, params, subset_keep, merge_distance, range_names, [&](const char *p, size_t k) {
    size_t done = 0;
    while (done < k) {
      const ssize_t w = write(fd, p + done, k - done);
      if (w < 0) {
        if (errno == EINTR) continue;
        throw Error{IMPG_E_IO, std::string("write failed: ") + strerror(errno)};
      }
      done += (size_t)w;
    }
    total += k;
  }, seconds3, format);
  if (bytes_written) *bytes_written = total;
  return IMPG_OK;
  IMPG_CATCH
}
}  // namespace

int impg_gpu_query_batch_bed(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                             const uint8_t *subset_keep, int32_t merge_distance, const char *const *range_names, char **text,
                             size_t *len, double *seconds3) {
  return text_batch_buffer(ix, ranges, n, params, subset_keep, merge_distance, range_names, text, len, seconds3, TEXT_BED);
}
int impg_gpu_query_batch_bed_fd(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                                const uint8_t *subset_keep, int32_t merge_distance, const char *const *range_names, int fd,
                                uint64_t *bytes_written, double *seconds3) {
  return text_batch_fd(ix, ranges, n, params, subset_keep, merge_distance, range_names, fd, bytes_written, seconds3, TEXT_BED);
}
int impg_gpu_query_batch_bedpe(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                               const uint8_t *subset_keep, int32_t merge_distance, const char *const *range_names, char **text,
                               size_t *len, double *seconds3) {
  return text_batch_buffer(ix, ranges, n, params, subset_keep, merge_distance, range_names, text, len, seconds3, TEXT_BEDPE);
}
int impg_gpu_query_batch_bedpe_fd(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                                  const uint8_t *subset_keep, int32_t merge_distance, const char *const *range_names, int fd,
                                  uint64_t *bytes_written, double *seconds3) {
  return text_batch_fd(ix, ranges, n, params, subset_keep, merge_distance, range_names, fd, bytes_written, seconds3, TEXT_BEDPE);
}
int impg_gpu_query_batch_paf(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                             const uint8_t *subset_keep, int32_t merge_distance, const char *const *range_names, char **text,
                             size_t *len, double *seconds3) {
  return text_batch_buffer(ix, ranges, n, params, subset_keep, merge_distance, range_names, text, len, seconds3, TEXT_PAF);
}
int impg_gpu_query_batch_paf_fd(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                                const uint8_t *subset_keep, int32_t merge_distance, const char *const *range_names, int fd,
                                uint64_t *bytes_written, double *seconds3) {
  return text_batch_fd(ix, ranges, n, params, subset_keep, merge_distance, range_names, fd, bytes_written, seconds3, TEXT_PAF);
}

// FASTA (fasta_device.hip): range_names is accepted and unused -- a record is named after its own sequence
int impg_gpu_query_batch_fasta(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                               const uint8_t *subset_keep, int32_t merge_distance, const char *const *range_names, int reverse_complement,
                               char **text, size_t *len, double *seconds3) {
  (void)range_names;
  return text_batch_buffer(ix, ranges, n, params, subset_keep, merge_distance, nullptr, text, len, seconds3, reverse_complement ? TEXT_FASTA_RC : TEXT_FASTA);
}
int impg_gpu_query_batch_fasta_fd(impg_gpu_index_t *ix, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                                  const uint8_t *subset_keep, int32_t merge_distance, const char *const *range_names, int reverse_complement,
                                  int fd, uint64_t *bytes_written, double *seconds3) {
  (void)range_names;
  return text_batch_fd(ix, ranges, n, params, subset_keep, merge_distance, nullptr, fd, bytes_written, seconds3, reverse_complement ? TEXT_FASTA_RC : TEXT_FASTA);
}
int impg_gpu_results_fasta(const impg_gpu_results_t *res, const impg_gpu_index_t *ix, const impg_gpu_params_t *params, int32_t merge_distance,
                           int reverse_complement, char **text, size_t *len) {
  IMPG_TRY
  if (!res || !ix || !params || !text || !len) throw Error{IMPG_E_INVALID, "null argument"};
  std::vector<std::string> parts;
  render_fasta(*res, *ix, *params, merge_distance, reverse_complement != 0, parts);
  *text = join_parts(parts, len);
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_results_paf(const impg_gpu_results_t *res, const impg_gpu_index_t *ix, const char *const *range_names,
                         const impg_gpu_params_t *params, int32_t merge_distance, int format, char **text, size_t *len) {
  IMPG_TRY
  if (!res || !ix || !params || !text || !len) throw Error{IMPG_E_INVALID, "null argument"};
  if (format != IMPG_OUT_PAF && format != IMPG_OUT_BEDPE) throw Error{IMPG_E_INVALID, "unknown output format"};
  std::vector<std::string> parts;
  render_paf(*res, *ix, range_names, *params, merge_distance, format == IMPG_OUT_BEDPE, parts);
  *text = join_parts(parts, len);
  return IMPG_OK;
  IMPG_CATCH
}

// The device BED merge and text on rows the caller brings (diagnostics; tests/test_gpu_bed_device.py): what a chunk of
// impg_gpu_query_batch_bed runs once its rows are placed (bed_device.hip), without a query in front of it.
int impg_gpu_selftest_bed_rows(impg_gpu_index_t *ix, const impg_gpu_interval_t *rows, const uint32_t *row_range, size_t n_rows,
                               uint32_t n_ranges, uint64_t n_seq, int32_t merge_distance, int merge_strands, int original_sequence_coordinates,
                               const char *const *range_names, impg_gpu_bed_row_t **merged_out, size_t *n_merged, char **text, size_t *len,
                               impg_gpu_interval_t **gap_rows_out, uint32_t **gap_range_out, size_t *n_gap) {
  IMPG_TRY
  if (!ix || !merged_out || !n_merged || !text || !len || (n_rows && (!rows || !row_range))) throw Error{IMPG_E_INVALID, "null argument"};
  const bool want_gap = gap_rows_out || gap_range_out || n_gap;
  if (want_gap && !(gap_rows_out && gap_range_out && n_gap)) throw Error{IMPG_E_INVALID, "the gap outputs come together"};
  if (ix->shard || ix->cluster) throw Error{IMPG_E_INVALID, "impg_gpu_selftest_bed_rows takes a single-GPU handle"};
  check_row_count(n_rows);
  n_seq = std::min<uint64_t>(n_seq, 1ull << 32);  // (ids are 32 bits wide)
  for (size_t i = 0; i < n_rows; i++) {
    if (rows[i].query_id >= n_seq || rows[i].target_id >= n_seq) throw Error{IMPG_E_INVALID, "a row's sequence id is not below n_seq"};
    if (row_range[i] >= n_ranges) throw Error{IMPG_E_INVALID, "a row's range index is not below n_ranges"};
  }
  const std::vector<std::string> rnames = default_range_names(n_ranges, range_names);
  IMPG_HIP(hipSetDevice(ix->device));
  EngineLease lease(*ix);
  ix->bed_stats_reset();
  std::vector<impg_gpu_bed_row_t> merged;
  std::string out;
  BedGapRows gap;
  device_bed_selftest(*lease, *ix, rows, row_range, (uint32_t)n_rows, n_ranges, n_seq, merge_distance, merge_strands != 0,
                      original_sequence_coordinates != 0, rnames, merged, out, want_gap ? &gap : nullptr);
  char *t = malloc_text(out);
  impg_gpu_bed_row_t *m = (impg_gpu_bed_row_t *)malloc(std::max<size_t>(merged.size(), 1) * sizeof(impg_gpu_bed_row_t));
  impg_gpu_interval_t *gr = want_gap ? (impg_gpu_interval_t *)malloc(std::max<size_t>(gap.rows.size(), 1) * sizeof(impg_gpu_interval_t)) : nullptr;
  uint32_t *gq = want_gap ? (uint32_t *)malloc(std::max<size_t>(gap.range.size(), 1) * 4) : nullptr;
  if (!m || (want_gap && (!gr || !gq))) { free(m); free(t); free(gr); free(gq); throw Error{IMPG_E_OOM, "host out of memory"}; }
  if (want_gap) {
    if (!gap.rows.empty()) { memcpy(gr, gap.rows.data(), gap.rows.size() * sizeof(impg_gpu_interval_t)); memcpy(gq, gap.range.data(), gap.range.size() * 4); }
    *gap_rows_out = gr; *gap_range_out = gq; *n_gap = gap.rows.size();
  }
  if (!merged.empty()) memcpy(m, merged.data(), merged.size() * sizeof(impg_gpu_bed_row_t));
  *merged_out = m; *n_merged = merged.size(); *text = t; *len = out.size();
  return IMPG_OK;
  IMPG_CATCH
}

// The device FASTA sweep and writer on rows the caller brings (diagnostics; tests/test_gpu_fasta_device.py): what a chunk of
// impg_gpu_query_batch_fasta runs once its rows are placed (bed_device.hip's sweep, fasta_device.hip), without a query in front.
int impg_gpu_selftest_fasta_rows(impg_gpu_index_t *ix, const impg_gpu_interval_t *rows, const uint32_t *row_range, size_t n_rows, uint32_t n_ranges,
                                 int32_t merge_distance, int reverse_complement, char **text, size_t *len) {
  IMPG_TRY
  if (!ix || !text || !len || (n_rows && (!rows || !row_range))) throw Error{IMPG_E_INVALID, "null argument"};
  fasta_refusals(*ix);
  check_row_count(n_rows);
  for (size_t i = 0; i < n_rows; i++) {
    if (rows[i].query_id >= ix->view.n_seq || rows[i].target_id >= ix->view.n_seq) throw Error{IMPG_E_INVALID, "a row's sequence id is not one of the index's"};
    if (row_range[i] >= n_ranges) throw Error{IMPG_E_INVALID, "a row's range index is not below n_ranges"};
  }
  IMPG_HIP(hipSetDevice(ix->device));
  EngineLease lease(*ix);
  ix->fasta_stats_reset();
  std::string out;
  DevBuf merged;
  const uint32_t n_rec = device_fasta_selftest_rows(*lease, *ix, rows, row_range, (uint32_t)n_rows, n_ranges, merge_distance, merged);
  ix->fasta_stats[FASTA_ROWS] += n_rows;
  ix->fasta_stats[FASTA_RECORDS] += n_rec;
  device_fasta_text(*lease, *ix, merged, n_rec, reverse_complement != 0, [&](const char *p, size_t k) { out.append(p, k); });
  *text = malloc_text(out); *len = out.size();
  return IMPG_OK;
  IMPG_CATCH
}

// The device BEDPE / PAF merge and text on rows and CIGARs the caller brings (diagnostics; tests/test_gpu_bedpe_device.py,
// tests/test_gpu_paf_device.py): what a chunk of impg_gpu_query_batch_bedpe / _paf runs once its rows and their ops are
// placed (bedpe_device.hip, paf_device.inc), without a query in front.
static int selftest_cigar_rows(impg_gpu_index_t *ix, const impg_gpu_interval_t *rows, const uint32_t *row_range, size_t n_rows, uint32_t n_ranges,
                               const uint64_t *cigar_off, const uint32_t *cigar_ops, int32_t merge_distance, int original_sequence_coordinates,
                               const char *const *range_names, char **text, size_t *len, bool paf) {
  IMPG_TRY
  if (!ix || !text || !len || !cigar_off || (n_rows && (!rows || !row_range))) throw Error{IMPG_E_INVALID, "null argument"};
  if (paf) paf_refusals(*ix);
  else bedpe_refusals(*ix);
  check_row_count(n_rows);
  if (cigar_off[0] != 0 || (cigar_off[n_rows] && !cigar_ops)) throw Error{IMPG_E_INVALID, "CIGAR offsets start at 0 and come with their ops"};
  for (size_t i = 0; i < n_rows; i++) {
    if (rows[i].query_id >= ix->view.n_seq || rows[i].target_id >= ix->view.n_seq) throw Error{IMPG_E_INVALID, "a row's sequence id is not one of the index's"};
    if (row_range[i] >= n_ranges || (i && row_range[i] < row_range[i - 1])) throw Error{IMPG_E_INVALID, "the rows come grouped by range, range indices below n_ranges"};
    if (cigar_off[i + 1] < cigar_off[i]) throw Error{IMPG_E_INVALID, "CIGAR offsets must not decrease"};
  }
  const std::vector<std::string> rnames = default_range_names(n_ranges, range_names);
  IMPG_HIP(hipSetDevice(ix->device));
  EngineLease lease(*ix);
  if (paf) ix->paf_stats_reset();
  else ix->bedpe_stats_reset();
  std::string out;
  if (n_ranges) (paf ? device_paf_selftest : device_bedpe_selftest)(*lease, *ix, rows, row_range, (uint32_t)n_rows, n_ranges, cigar_off, cigar_ops,
                                                                    merge_distance, original_sequence_coordinates != 0, rnames, out);
  *text = malloc_text(out); *len = out.size();
  return IMPG_OK;
  IMPG_CATCH
}
int impg_gpu_selftest_bedpe_rows(impg_gpu_index_t *ix, const impg_gpu_interval_t *rows, const uint32_t *row_range, size_t n_rows,
                                 uint32_t n_ranges, const uint64_t *cigar_off, const uint32_t *cigar_ops, int32_t merge_distance,
                                 int original_sequence_coordinates, const char *const *range_names, char **text, size_t *len) {
  return selftest_cigar_rows(ix, rows, row_range, n_rows, n_ranges, cigar_off, cigar_ops, merge_distance, original_sequence_coordinates, range_names,
                             text, len, false);
}
int impg_gpu_selftest_paf_rows(impg_gpu_index_t *ix, const impg_gpu_interval_t *rows, const uint32_t *row_range, size_t n_rows,
                               uint32_t n_ranges, const uint64_t *cigar_off, const uint32_t *cigar_ops, int32_t merge_distance,
                               int original_sequence_coordinates, const char *const *range_names, char **text, size_t *len) {
  return selftest_cigar_rows(ix, rows, row_range, n_rows, n_ranges, cigar_off, cigar_ops, merge_distance, original_sequence_coordinates, range_names,
                             text, len, true);
}

// The lookup order's sort checked on its own (diagnostics; tests/test_gpu_parity.py): n pseudo-random keys of `end_bit` bits
// (seed; every 7th key repeats its predecessor's, so equal keys are common) through launch_order_sort on `device`; the result
// must be a permutation of 0 .. n-1 that lists the keys in non-decreasing order, equal keys by ascending index.
int impg_gpu_selftest_order_sort(int device, uint32_t n, unsigned end_bit, uint64_t seed) {
  IMPG_TRY
  if (end_bit < 1 || end_bit > 32) throw Error{IMPG_E_INVALID, "end_bit is 1 .. 32"};
  IMPG_HIP(hipSetDevice(device));
  std::vector<uint32_t> keys(n), perm(n);
  uint64_t x = seed * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
  const uint32_t mask = end_bit >= 32 ? 0xFFFFFFFFu : ((1u << end_bit) - 1u);
  for (uint32_t i = 0; i < n; i++) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    keys[i] = (i % 7u == 3u && i) ? keys[i - 1] : (uint32_t)(x >> 20);  // (bits above end_bit stay set: they must not matter)
  }
  hipStream_t s;
  IMPG_HIP(hipStreamCreate(&s));
  DevBuf ka, kb, pa, pb, sc;
  const size_t nb = std::max<size_t>((size_t)n * 4, 256);
  ka.reserve(nb); kb.reserve(nb); pa.reserve(nb); pb.reserve(nb); sc.reserve(order_sort_scratch_bytes(n));
  IMPG_HIP(hipMemcpyAsync(ka.p, keys.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  IMPG_HIP(hipMemsetAsync(pa.p, 0xA5, nb, s));
  launch_order_sort(ka.as<uint32_t>(), kb.as<uint32_t>(), pa.as<uint32_t>(), pb.as<uint32_t>(), n, end_bit, sc.p, s);
  IMPG_HIP(hipGetLastError());
  IMPG_HIP(hipMemcpyAsync(perm.data(), pa.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipStreamSynchronize(s));
  IMPG_HIP(hipStreamDestroy(s));
#ifdef IMPG_OS_CLOCKS
  {
    unsigned long long c[8];
    order_sort_clocks(c, false);
    fprintf(stderr, "[order sort clocks] n=%u bits=%u tiles x passes=%llu: per tile-pass zero+load %.0f rank %.0f bases %.0f lds %.0f out %.0f cycles\n", n, end_bit, c[7],
            (double)c[0] / c[7], (double)c[1] / c[7], (double)c[2] / c[7], (double)c[3] / c[7], (double)c[4] / c[7]);
    order_sort_clocks(nullptr, true);
  }
#endif
  std::vector<uint8_t> seen(n, 0);
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t i = perm[k];
    if (i >= n || seen[i]) throw Error{IMPG_E_INVALID, "order sort: not a permutation at place " + std::to_string(k)};
    seen[i] = 1;
    if (k) {
      const uint32_t a = keys[perm[k - 1]] & mask, b = keys[i] & mask;
      if (a > b || (a == b && perm[k - 1] > i)) throw Error{IMPG_E_INVALID, "order sort: out of order at place " + std::to_string(k)};
    }
  }
  return IMPG_OK;
  IMPG_CATCH
}

}  // extern "C"
