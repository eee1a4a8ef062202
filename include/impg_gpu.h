/*
 * impg_gpu.h -- C ABI of the MI355X-native batch interval-query + CIGAR
 * coordinate-projection engine (libimpg_gpu.so).
 *
 * This is the drop-in boundary for impg's hot path: a Rust
 * `struct GpuImpg; impl ImpgIndex for GpuImpg` (reference
 * src/impg_index.rs:21-121) is ~150 lines of glue over these entry points
 * (binding sketch in INTEGRATION.md).  Plain pointers and sizes only; no C++
 * or torch types; nothing unwinds across the boundary -- every call returns an
 * int status (0 = ok, <0 = error) and impg_gpu_last_error() gives the message
 * for the calling thread.  All coordinates are i32 and all sequence ids u32,
 * exactly the reference's types (src/impg.rs:164-174, :225).
 *
 * The library requires a gfx950 GPU: there is no CPU fallback.  Index creation
 * and queries fail with IMPG_E_HIP when no device is present.
 */
#ifndef IMPG_GPU_H
#define IMPG_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IMPG_OK 0
#define IMPG_E_INVALID (-1)     /* bad argument / malformed input (the reference panics: impg.rs:88,:506) */
#define IMPG_E_HIP (-2)         /* HIP runtime error / no device */
#define IMPG_E_OOM (-3)
#define IMPG_E_IO (-4)
#define IMPG_E_UNSUPPORTED (-5) /* valid in the reference, not built yet */
#define IMPG_E_CANCELLED (-6)   /* a callback of the caller's asked the call to stop */

typedef struct impg_gpu_index impg_gpu_index_t;
typedef struct impg_gpu_results impg_gpu_results_t;

/* One alignment record as the reference parses it from PAF
 * (AlignmentRecord, src/alignment_record.rs:12-22; parse_paf_line, src/paf.rs:118-177)
 * with its CIGAR already tokenised into packed ops: op = code<<29 | len,
 * codes '='0 'X'1 'I'2 'D'3 'M'4 -- identical to CigarOp (src/impg.rs:81-93). */
typedef struct {
  uint32_t query_id, target_id;
  int32_t query_start, query_end;
  int32_t target_start, target_end;
  uint64_t cigar_off; /* first op of this record in the op pool */
  uint32_t cigar_len; /* number of ops (0 = record has no cg:Z tag) */
  uint32_t strand;    /* 0 '+', 1 '-' */
} impg_gpu_record_t;

/* A query range: (target_id, range_start, range_end) of ImpgIndex::query
 * (src/impg_index.rs:26-35). */
typedef struct {
  uint32_t target_id;
  int32_t start, end;
} impg_gpu_range_t;

/* AdjustedInterval without its CIGAR (src/impg.rs:225): query interval,
 * target interval.  q_first > q_last encodes the reverse strand. */
typedef struct {
  uint32_t query_id;
  int32_t q_first, q_last;
  uint32_t target_id;
  int32_t t_first, t_last;
} impg_gpu_interval_t;

/* Scalars of query / query_transitive_{bfs,dfs} (src/impg_index.rs:26-94) with
 * the CLI defaults of src/main.rs:4259-4285. */
typedef struct {
  int32_t transitive;                  /* 0: Impg::query          (impg.rs:1852) */
  int32_t dfs;                         /* 1: query_transitive_dfs (impg.rs:2057); 0: _bfs (impg.rs:2311) */
  uint32_t max_depth;                  /* u16 in the reference; 0 = unlimited */
  int32_t min_transitive_len;          /* default 101 */
  int32_t min_distance_between_ranges; /* default 10 */
  int32_t min_output_length;           /* < 0 = None */
  double min_identity;                 /* NaN = None (min_gap_compressed_identity) */
  int32_t store_cigar;                 /* BED output never needs it (main.rs:7447) */
  int32_t multi_impg;                  /* 1: MultiImpg semantics (src/multi_impg.rs:495-595, :796-991): every step's hits
                                          sorted by (query_id, q.first, q.last, t.first, t.last), one worklist pop at a
                                          time (front = BFS, back = DFS), unclipped ranges, same-sequence hits skipped */
  int32_t original_sequence_coordinates; /* text writers only (--original-sequence-coordinates, main.rs:4370): a sequence
                                          named "base:START-END" is printed as "base" with START added to its
                                          coordinates (transform_coordinates_to_original, main.rs:4642-4678); PAF
                                          sequence lengths are then 0, as the reference prints them when it has no
                                          sequence files to ask (get_original_sequence_length, main.rs:4681-4704) */
  int32_t consider_strandness;         /* BED writer only (--consider-strandness, main.rs:4380): 1 keeps the two strands
                                          apart in the query-axis merge (merge_strands_for_output, main.rs:4395-4409) */
} impg_gpu_params_t;

/* Order in which overlapping entries of one target are visited; it fixes the
 * emission order of hits (and, through the order-dependent visited-set update
 * of impg.rs:2471-2560, the content of transitive results). */
#define IMPG_ORDER_COITREES 0 /* coitrees 0.4 BasicCOITree::query order (restated) */
#define IMPG_ORDER_SORTED 1   /* ascending target start, ties in input order */

const char *impg_gpu_last_error(void);
int impg_gpu_device_count(void);

/* ---- index: replaces Impg::from_multi_alignment_records (impg.rs:1535-1652),
 *      ForestMap (forest_map.rs:6-32) and the per-target coitrees ------------ */
int impg_gpu_index_create(const impg_gpu_record_t *records, size_t n_records,
                          const uint32_t *cigar_ops, size_t n_ops,
                          const int64_t *seq_len, uint32_t n_seq,
                          int bidirectional, int order_policy, int device,
                          impg_gpu_index_t **out);
/* The same from records of several alignment files: records[file_first_record[f] .. file_first_record[f+1])
 * (the last file ends at n_records) came from file f, as in `records_by_file` of
 * Impg::from_multi_alignment_records (impg.rs:1535).  Only MultiImpg semantics observe the split, and only
 * in the order of hits that agree on all five sort keys (multi_impg.rs:556-592): they stay file by file,
 * each in its own tree's visit order.  impg_gpu_index_create treats all records as one file. */
int impg_gpu_index_create_files(const impg_gpu_record_t *records, size_t n_records,
                                const uint32_t *cigar_ops, size_t n_ops, const int64_t *seq_len,
                                uint32_t n_seq, const uint64_t *file_first_record, uint32_t n_files,
                                int bidirectional, int order_policy, int device, impg_gpu_index_t **out);

/* ---- tracepoint alignments: approximate mode (approximate_mode = true of the trait, impg_index.rs:26-94;
 *      scan_overlapping_tracepoints + project_overlapping_interval_fast, impg.rs:646-823, :1317-1533).
 * The .1aln / .tpa readers stay with the host (onealn.rs, tpa crate): it hands every alignment over as its
 * tracepoints -- n_segs target deltas at tracepoints[seg_off ..] -- plus, per TracepointModeData (onealn.rs:772-782),
 *   Standard: query_deltas[seg_off ..] and the file's max_complexity (per-segment diffs are estimated from it),
 *   FASTGA:   diffs[seg_off ..], the file's trace_spacing and the alignment's query_contig_start (the first query
 *             delta is ((query_contig_start / spacing) + 1) * spacing - query_contig_start, impg.rs:726-735).
 * An index built this way answers every query in approximate mode: the query interval of a hit is interpolated
 * inside the first and the last overlapping trace segment (one f64 division and rounding each, bit-for-bit the
 * reference's arithmetic), its target interval is the (clipped) range itself, and the identity filter sees the
 * segment statistics ("N= MX").  Per alignment the index keeps prefix sums of the four per-segment quantities, so
 * a projection is two binary searches instead of a scan.  Tracepoints and query deltas must be non-negative (they
 * are in files FASTGA / the tracepoints crate write; the reference takes abs() of the former in places) and sum
 * below 2^31 per alignment: IMPG_E_UNSUPPORTED otherwise.  store_cigar is IMPG_E_UNSUPPORTED until option
 * "approximate_cigar" is set to 1 (impg_gpu_set_option).  Every row's CIGAR is then the one
 * project_overlapping_interval_fast returns (impg.rs:1479-1486): [matches '='] if positive, then [mismatches 'X'] if
 * positive -- 0, 1 or 2 ops, the very sums the identity filter sees.  They are statistics, not an alignment: their
 * lengths do not add up to the row's coordinates, which is why a caller has to ask.  The self interval keeps its
 * [(end - start) '='].  A sum of 2^29 or more does not fit a CigarOp (the reference panics, impg.rs:88): IMPG_E_INVALID.
 * impg_gpu_query, impg_gpu_query_batch / _masked / _filtered / _stream take it, on one GPU, a multi-GPU handle and
 * rank processes; impg_gpu_query_batch_device stays without store_cigar.  The
 * exact mode of these files needs the sequences and a WFA realignment and stays with the host. */
typedef struct {
  uint32_t query_id, target_id;
  int32_t query_start, query_end, target_start, target_end;
  uint64_t seg_off; /* first segment of this alignment in the pools */
  uint32_t n_segs;
  uint32_t strand;  /* 0 '+', 1 '-' */
  int64_t query_contig_start; /* FASTGA only */
} impg_gpu_tp_record_t;
typedef struct {
  int32_t fastga;         /* 0 Standard, 1 FASTGA */
  int32_t trace_spacing;  /* FASTGA */
  int32_t max_complexity; /* Standard */
} impg_gpu_tp_mode_t;
int impg_gpu_index_create_tracepoints(const impg_gpu_tp_record_t *records, size_t n_records, const int32_t *tracepoints,
                                      const int32_t *query_deltas /* Standard, else NULL */,
                                      const int32_t *diffs /* FASTGA, else NULL */, size_t n_segs_total,
                                      const impg_gpu_tp_mode_t *mode, const int64_t *seq_len, uint32_t n_seq, int bidirectional,
                                      int order_policy, int device, impg_gpu_index_t **out);

/* The same index sharded by target sequence over the GPUs of this process (see impg_gpu_index_create_multi below): one
 * handle, queries answered in approximate mode by the shards that own the targets. */
int impg_gpu_index_create_tracepoints_multi(const impg_gpu_tp_record_t *records, size_t n_records, const int32_t *tracepoints,
                                            const int32_t *query_deltas, const int32_t *diffs, size_t n_segs_total,
                                            const impg_gpu_tp_mode_t *mode, const int64_t *seq_len, uint32_t n_seq, int bidirectional,
                                            int order_policy, const int *devices, int n_dev, int lanes, impg_gpu_index_t **out);

/* Same, parsing PAF files on the host the way paf.rs:118-194 does; sequence ids
 * are assigned in first-seen order over the files (query then target per line). */
int impg_gpu_index_create_from_paf(const char *const *paths, int n_paths,
                                   int bidirectional, int order_policy,
                                   int device, impg_gpu_index_t **out);
/* The second way from PAF files to the same index: the files (plain, gzip, BGZF -- recognised by their magic, as
 * impg_gpu_index_load_sequences does) are streamed into HBM in pieces of whole lines and parsed there -- lines, fields,
 * the cg:Z: tag and the CIGARs; the host keeps lines whole across pieces and gives the names the device did not know
 * their ids, and reads no other byte of a line.  piece_bytes: 0 = 64 MiB; else 16 .. 2^32, a multiple of 16 (a line longer
 * than the buffer makes the buffer double; offsets in a piece are 32 bits, so a line of 4 GiB is IMPG_E_UNSUPPORTED).  One
 * GPU.  The index is the one impg_gpu_index_create_from_paf builds from the same files.  Errors are that call's, with one
 * difference: that call tokenises last and so reports a bad head anywhere before any "Invalid CIGAR operation"; this
 * one reports the first bad line in file order (a line's head checks before its CIGAR).  Reader trouble is IMPG_E_IO
 * naming the file.  The op pool is reserved from the files' sizes (IMPG_PAF_INGEST_POOL_OPS sets the first size) and
 * grows by half when a piece does not fit; where it cannot, the call fails with IMPG_E_OOM and names
 * impg_gpu_index_create_from_paf.  After a failure no handle exists and no HBM is kept.  Counters "paf_ingest_*". */
int impg_gpu_index_create_from_paf_streamed(const char *const *paths, int n_paths, int bidirectional, int order_policy,
                                            int device, uint64_t piece_bytes, impg_gpu_index_t **out);
/* The hand-off alone, for the tests: what the ingest leaves for the builder, malloc'ed.  on_host = 1 runs the host twin
 * of the kernels (no device needed); hash_bits < 64 truncates the name hash (collisions on purpose); initial_pool_ops
 * sizes the first op pool (0 = the default rule).  stats: the nine "paf_ingest_*" counters in the order of their keys below
 * (may be null). */
int impg_gpu_selftest_paf_ingest(const char *const *paths, size_t n_paths, uint64_t piece_bytes, int on_host, int device,
                                 unsigned hash_bits, uint64_t initial_pool_ops, /* out: */ impg_gpu_record_t **records,
                                 size_t *n_records, uint32_t **ops, size_t *n_ops, char **names /* '\n'-joined, id order */,
                                 size_t *names_len, int64_t **lens, size_t *n_seq, uint64_t **file_first /* n_paths + 1 */,
                                 uint64_t *stats);
/* ---- M ops resolved against the sequences.  The reference counts every 'M' base as a match
 * ("We overestimate num. of matches by assuming 'M' represents matches for simplicity", main.rs:11944; the identity filter
 * alike, impg.rs:2952-2973), so on a PAF written without --eqx its identity filter passes everything.  This pass rewrites,
 * before the index is built, every 'M' op as the '=' / 'X' runs the two sequences spell and checks the '=' and 'X' ops
 * that are there: the index is then the one the same PAF builds with each 'M' written out as its '=' / 'X' runs.
 *   A record with cigar_len > 0 is resolvable if both its sequences are in the store, their stored lengths equal seq_len,
 * 0 <= start <= end <= len on both axes, every op code is <= 4, the lengths of its '=' 'X' 'M' 'D' ops sum to target_end -
 * target_start and those of its '=' 'X' 'M' 'I' ops to query_end - query_start.  Otherwise its ops are copied unchanged and
 * its flag byte is 1 (a sequence absent from the store) or 2 (any other condition); no byte of a sequence is read for it.
 * Records without ops pass through with flag 0.
 *   Position p of an op that starts at (t, q) of its record compares T[target_start + t + p] with Q[query_start + q + p] on
 * '+' and with comp(Q[query_end - 1 - q - p]) on '-' (comp: A<->T, C<->G, every other byte itself; the store is upper
 * case).  Equal bytes match -- N against N too.  An 'M' of length L > 0 becomes its maximal runs of matching / differing
 * positions, '=' (code 0) and 'X' (code 1) ops in order; an 'M' of length 0 becomes one '=' of length 0; '=' 'X' 'I' 'D' are
 * kept verbatim and nothing is fused across op borders ("2=3M" over equal bases is "2=3=").
 *   The report (also the counters "resolve_records", "resolve_resolved", "resolve_absent", "resolve_inconsistent",
 * "resolve_ops_in", "resolve_ops_out", "resolve_m_ops", "resolve_m_bases", "resolve_m_eq_bases", "resolve_m_x_bases",
 * "resolve_bad_eq_bases", "resolve_bad_x_bases" of a handle impg_gpu_index_create_from_paf_resolved made; 0 on every
 * other handle): records = n_records; resolved / absent / inconsistent = records with ops by their flag 0 / 1 / 2; ops_in /
 * ops_out = the records' ops before and after; over the resolvable records: m_ops 'M' ops of m_bases bases, of which
 * m_eq_bases matched and m_x_bases did not, bad_eq_bases positions under an '=' whose bytes differ and bad_x_bases
 * positions under an 'X' whose bytes are equal (such ops are counted, not changed). */
typedef struct {
  uint64_t records, resolved, absent, inconsistent, ops_in, ops_out, m_ops, m_bases, m_eq_bases, m_x_bases, bad_eq_bases, bad_x_bases;
} impg_gpu_resolve_report_t;
typedef struct impg_gpu_sequences impg_gpu_sequences_t; /* the sequence store: impg_gpu_sequences_from_fasta, below */
/* The pass alone.  records address the pool `ops` in any order; names_of_ids[id] / seq_len[id] are the sequence table.
 * Out, malloc'ed: the records with cigar_off (the ops of the records before it: the new pool is in record order) and
 * cigar_len rewritten and every other field untouched, the new pool, a flag byte per record; report may be NULL.
 * on_host = 1 runs the host twin of the kernels (single-threaded; no device needed).  On the device the store's
 * sequences that the table names are uploaded one byte a base beside both pools: IMPG_E_OOM, naming the bytes it
 * wanted, if they do not fit together.  IMPG_E_INVALID: a sequence id >= n_seq, a CIGAR outside the pool;
 * IMPG_E_UNSUPPORTED: a record whose new cigar_len passes the build's limit of 2^29 - 1 ops (the build's own error), a
 * pool of 2^32 op tiles, a store without a host copy (impg_gpu_index_load_sequences). */
int impg_gpu_cigar_resolve(const impg_gpu_record_t *records, size_t n_records, const uint32_t *ops, size_t n_ops,
                           const char *const *names_of_ids, const int64_t *seq_len, uint32_t n_seq,
                           const impg_gpu_sequences_t *seqs, int on_host, int device,
                           impg_gpu_record_t **records_out, uint32_t **ops_out, size_t *n_ops_out, uint8_t **flags_out,
                           impg_gpu_resolve_report_t *report);
/* The same for the tests, with the bases of an op one wave compares: tile_bases = 0 is the default (1 024), else a
 * multiple of 64 up to 4 096 (IMPG_E_INVALID otherwise).  The answer does not depend on it. */
int impg_gpu_selftest_cigar_resolve(const impg_gpu_record_t *records, size_t n_records, const uint32_t *ops, size_t n_ops,
                                    const char *const *names_of_ids, const int64_t *seq_len, uint32_t n_seq,
                                    const impg_gpu_sequences_t *seqs, int on_host, int device, uint32_t tile_bases,
                                    impg_gpu_record_t **records_out, uint32_t **ops_out, size_t *n_ops_out, uint8_t **flags_out,
                                    impg_gpu_resolve_report_t *report);
/* impg_gpu_index_create_from_paf with the pass between the tokeniser and the builder: the host splits lines and fields,
 * the device tokenises, resolves the pool where it lies in HBM and builds from the new pool; only the records' new
 * cigar_off / cigar_len come home, the ops never do.  report and flags (malloc'ed, one byte per record in file order)
 * may be NULL.  No flag makes the call fail: a caller that wants strictness reads the report.  The store is not
 * attached (impg_gpu_index_set_sequences does that, as before).  One GPU. */
int impg_gpu_index_create_from_paf_resolved(const char *const *paths, int n_paths, const impg_gpu_sequences_t *seqs,
                                            int bidirectional, int order_policy, int device,
                                            impg_gpu_resolve_report_t *report, uint8_t **flags, impg_gpu_index_t **out);

/* A built index as one file: the role of the reference's `.impg` file (writer impg.rs:1655-1721, reader
 * :1787-1850; `impg index` / the implicit index cache of `impg query`, main.rs:11321-11386): pay for
 * parsing and tokenising once.  The file holds the device arrays as they sit in HBM plus the sequence
 * table (so the alignment files are not needed again, unlike with `.impg`, which stores byte offsets into
 * them); it is this library's own layout ("IMPGHBM1"), tied to the build's tile constants, and NOT the
 * reference's IMPGIDX2 format.  A rank's shard of a sharded index is saved the same way (one file per rank, the caller
 * names it; it also holds the world size, the rank and the target -> rank map) and comes back with
 * impg_gpu_index_load_rank on a communicator of the same world and rank; a multi handle writes its front file at `path`
 * and its shards at path.shard<k>of<n> and comes back with impg_gpu_index_load_multi -- so the ranks of a job parse the
 * alignments once, not once per rank per start (the role of impg.rs:1655-1850).  load: IMPG_E_INVALID for a
 * foreign or damaged file (or a shard handed to the plain load / the wrong rank), IMPG_E_UNSUPPORTED for a layout
 * version this build does not read. */
int impg_gpu_index_save(const impg_gpu_index_t *, const char *path);
/* The reference's own index file ("IMPGIDX2", or the unidirectional "IMPGIDX1"; writer impg.rs:1655-1721, reader
 * :1787-1850 + :1724-1767; bincode-2 standard encoding): sequence table and every target's intervals come from the
 * file, in the file's order (the order the reference rebuilds its trees from, hence its tie order among equal
 * starts); the CIGARs are read from the alignment files -- the same files, in the same order, the index was built
 * with (impg.rs:1789, :1844; plain-text PAF: offsets into compressed PAF are BGZF virtual offsets,
 * IMPG_E_UNSUPPORTED) -- and tokenised once.  An existing `.impg` cache therefore opens without `impg index`
 * being re-run.  IMPG_E_INVALID for a damaged file or CIGAR text that no longer parses at its offset. */
int impg_gpu_index_load_impg(const char *impg_path, const char *const *alignment_files, int n_files, int order_policy,
                             int device, impg_gpu_index_t **out);
int impg_gpu_index_load(const char *path, int device, impg_gpu_index_t **out);
void impg_gpu_index_destroy(impg_gpu_index_t *);

/* seq_index() (seqidx.rs), target_ids(), num_targets() (impg_index.rs:105-113) */
uint32_t impg_gpu_num_seqs(const impg_gpu_index_t *);
const char *impg_gpu_seq_name(const impg_gpu_index_t *, uint32_t id); /* NULL if created without names */
int64_t impg_gpu_seq_len(const impg_gpu_index_t *, uint32_t id);
int64_t impg_gpu_seq_id(const impg_gpu_index_t *, const char *name);  /* -1 = unknown */
size_t impg_gpu_num_targets(const impg_gpu_index_t *);
size_t impg_gpu_target_ids(const impg_gpu_index_t *, uint32_t *out, size_t cap);
size_t impg_gpu_num_entries(const impg_gpu_index_t *);
size_t impg_gpu_num_records(const impg_gpu_index_t *);
/* HBM the index's arrays hold.  Grows once, by 128 bytes per CIGAR tile, when a query first sets min_identity
 * (min_gap_compressed_identity, impg_index.rs:31): the identity lines -- a third of a full index, read by that filter
 * only -- are built on the device at that point (IMPG_E_OOM if they do not fit); IMPG_IDENTITY_LINES=1 in the
 * environment builds them with the index. */
size_t impg_gpu_device_bytes(const impg_gpu_index_t *);
/* 1: the index was built from tracepoints and answers every query in the reference's approximate mode
 * (approximate_mode = true of the trait methods, src/impg_index.rs:34, :93); 0: built from CIGARs, exact mode.
 * The mode is a property of the index here: a host mirroring the trait refuses a call whose approximate_mode
 * disagrees (IMPG_E_UNSUPPORTED) rather than answer in the other mode. */
int impg_gpu_index_approximate(const impg_gpu_index_t *);

/* Tunables: "pair_budget" (max candidate pairs held in HBM per level; a batch
 * whose level exceeds it is split by ranges, queries being independent) and
 * "chunk_ranges" (initial ranges per chunk, 0 = whole batch), "locality_min"
 * (frontier size from which the projection kernel walks the hit slots in the order
 * of the ranges' windows in the entry array -- a cache-locality order; results
 * are identical either way; 0 = never), "free_slot_order" (1, the default: runs
 * that keep no level -- impg_gpu_query_batch_stats -- lay their hit slots out in
 * that order too; 0: always the reference's slot order; counts and checksums are
 * identical either way),
 * "walk_kernel" (the per-query walk: 0 never, 1 -- the default -- DFS batches of any size and those depth-limited
 * (max_depth >= 2) BFS batches of <= 64 ranges that get at least two workgroups a query out of the launch's share of
 * the compute units -- CUs / max_engines, i.e. <= 32 ranges on a 256-CU device with four engines a handle --, 2 also
 * every other BFS batch of <= 64 ranges) and "walk_members" (workgroups per query of the walk's grid form, which
 * shares a depth-limited BFS's last level out: 0 = as many as fit the share, at most 32; N > 1 = at most N, itself at
 * most 64; 1 = none),
 * "segment_groups" (1, the default: the visited update orders a level's hits by (query, hit sequence) query by query --
 * a query's ranges run by run in frontier order, a counting sort by sequence inside the query; 0: with the library's
 * stable radix sort; results are identical either way) and "segment_parts" (0, the default: a query whose level holds
 * more hits than one wave should take is cut into slices of its frontier ranges, as many as the level's size asks for;
 * N = that many slices on every level that groups by segments -- for tests; results are identical),
 * "wide_emit_cap" (64 .. 4096, the default) and "wide_emit_bins" (2 .. 1024, the default): the hits the lookup sorts in one
 * pass for a window of more than 64 entries, and the rank bins it groups a window's hits by beyond that -- for tests;
 * results are identical,
 * "lookup_coop" (1, the default: a level whose ranges are taken in the lookup order is counted wave by wave, a wave
 * searching once for its 64 ranges and reading their windows from its copy of the index columns; 0: range by range;
 * results identical) and "lookup_coop_span" (4 .. 256, the default: the entries such a wave copies at most; a wave whose
 * ranges span more counts range by range -- for tests; results identical),
 * "place_offsets_blocks" (1, the default: a fused final level's place offsets in two levels, per block of 64 places (a wave of the count pass); 0: one scan over every range -- A/B runs and tests; results identical),
 * "fuse_final_level" (1, the default: the final level of such a run -- no update follows, no row is kept --
 * takes its (range, entry) pairs straight from the lookup's per-range windows inside the projection kernel; the emit
 * pass and its pair lists are skipped; counts and checksums are identical either way),
 * "approximate_cigar" (0, the default: store_cigar on a tracepoint index is IMPG_E_UNSUPPORTED; 1: its rows carry the
 * approximate mode's CIGAR -- see impg_gpu_index_create_tracepoints.  No effect on an index built from CIGARs.  A
 * run-time setting: impg_gpu_index_save does not write it),
 * "regroup_entries" (1, the default: a projection block sorts its 256 pairs by entry before reading the index; results
 * identical), "filter_covered" (visited update: hits covered by their group's old list dropped before the replay -- 0 off,
 * the default, 1 always, 2 long groups; results identical), "device_rows_pool_bytes" (HBM kept between
 * impg_gpu_query_batch_device calls: freed slot arrays, reused by the next call; 160 GiB by default),
 * "update_stats" / "lookup_stats" (0, the default; 1: the "update_*" / "lookup_wide_*" counters below are kept, one small
 * copy per level), "bed_text_piece_bytes" (64 .. 2^40; 256 MiB by default: the text of impg_gpu_query_batch_bed crosses
 * PCIe in pieces of whole rows of at most this many bytes, a piece of one row may be up to 4096 bytes longer; a row
 * beyond that is IMPG_E_UNSUPPORTED; the text is identical for every value; impg_gpu_query_batch_bedpe's text crosses the
 * same way), "bedpe_group_log2" (2 .. 6; 2 by default: impg_gpu_query_batch_bedpe sums a row's CIGAR ops with 2^value
 * lanes; results identical), "paf_group_log2" (2 .. 6; 2 by default: impg_gpu_query_batch_paf fuses and prints a row's CIGAR
 * ops with 2^value lanes; results identical), "sequence_store_packed" (the form impg_gpu_index_set_sequences uploads the
 * sequence store in: 0, the default, one byte per base; 1 two bits per base and a table of runs for every byte that is not
 * A/C/G/T; 2 whichever of the two takes fewer bytes in HBM for the store at hand -- see impg_gpu_index_set_sequences.  Read
 * at attach: changing it does not repack an attached store, detach and attach again for that.  The text is identical for
 * every value), "sequence_ingest_piece_bytes" (16 .. 2^32, a multiple of 16; 64 MiB by default: impg_gpu_index_load_sequences
 * sends a file's text to the device in pieces of this many bytes; the store is identical for every value).  For tests of
 * the multi-rank paths: "lane_schedule" (forced lane start / hand-over order of a sharded
 * batch; 0 = off), "debug_fail_owner" / "debug_fail_home" (failure injection: (rank + 1) << 16 | hop of the batch at which
 * that rank throws on the owner / on the home side of the hop; 0 = off).
 * A multi-GPU handle hands "chunk_ranges", "pair_budget", "locality_min", "debug_fail_owner", "debug_fail_home",
 * "lane_schedule", "fuse_final_level", "device_rows_pool_bytes" and "approximate_cigar" to its shards before every batch;
 * the other settings have no effect on it.  A value outside a key's range, and an unknown key, is IMPG_E_INVALID.
 * Actions rather than settings, so that a process's FIRST call costs what its later ones do: "prewarm_result_bytes" = N
 * pins a host block of N bytes into the result pool now (a 5 GB result pins its block inside the first call
 * otherwise, ~0.3-1 s); "prewarm_walk" = 1 / 2 allocates the per-query walk's slabs (1: the per-call / small-batch BFS
 * shape; 2: also the DFS batch's, ~15 GB) on the index's first engine. */
int impg_gpu_set_option(impg_gpu_index_t *, const char *key, int64_t value);
/* The keys impg_gpu_set_option / impg_gpu_get_counter accept, i = 0, 1, ...; NULL past the last one.  No handle and no
 * device needed: a document or a wrapper can be checked against the library's own tables. */
const char *impg_gpu_option_key(size_t i);
const char *impg_gpu_counter_key(size_t i);
/* Read-only counters of an index handle (no reference counterpart; they tell a test, or an operator, which engine
 * answered): "walk_launches" = per-query walk launches that answered their batch (walk_device.inc: DFS batches, MultiImpg
 * worklists of either end -- not under a mask --, small depth-limited BFS batches incl. masked ones -- the shape of
 * partition.rs:359-391), "walk_fallbacks" = launches whose
 * batch the batch engine had to run again (a query outgrew its slab or its pop budget), "walk_members" = workgroups per query of the
 * last grid-form launch (1: not the grid form), "walk_overflow" = the cause word of the most recent walk launch (0: the
 * launch answered its batch; otherwise the limits its queries outgrew, ORed: 1 unknown target, 2 pairs of one step / of one
 * member's share of the last level, 4 visited pool or a mask list, 8 piece scratch, 16 pieces of one level / pop, 32 DFS
 * stack (a BFS frontier is bounded by 16 first), 64 unnamed, 128 a grid hand-off timed out, 256 pop budget: a MultiImpg worklist explored more than 2^20 pops),
 * "small_batches" = plain batches of <= 64 ranges answered by the one-chain
 * small-batch path; "dfs_rounds" = rounds of the batch engine's DFS / MultiImpg worklist (Engine::run_dfs) in which some
 * query still had a stack -- a round that only drops too-deep records counts, a batch the walk answered adds none --,
 * "visited_compactions" = times a transitive run folded its visited tables into one (Engine::compact_tables); how the visited updates grouped their hits: "segment_sliced_levels" =
 * levels whose queries were cut into slices of their frontier ranges, "segment_retries" = levels counted a second time
 * because one query held more hits than a wave should take, "segment_library_levels" = levels that went through the
 * library's radix sort instead; which kernel projected each level: "project_lane_levels", "project_staged_levels",
 * "project_staged_rows_levels", "project_entries_slots_levels", "project_entries_qs_levels", "project_entries_rows_levels",
 * "project_entries_ident_levels", "project_tp_levels"; "place_offsets_block_levels" = fused final levels whose ranges found
 * their places through per-block offsets (option "place_offsets_blocks") instead of a scan over every range.  With option "update_stats" = 1 (0, the default: nothing is copied or counted) every
 * level's visited update also counts its (query, sequence) groups by the kernel that took them -- "update_lane_groups",
 * "update_mid_groups", "update_wave_tiny_groups", "update_wave_small_groups", "update_wave_large_groups" -- and by the
 * rare path they reached: "update_inplace_groups" (the replay ran on the group's global slice), "update_tiled_sort_groups"
 * (more pieces than the LDS buffer holds), "update_lane_spill_groups" (a lane's pieces left its LDS column).  With option
 * "lookup_stats" = 1 (0, the default: nothing is copied or counted) every level's lookup counts its windows of more than 64
 * entries: "lookup_wide_windows" (all of them), "lookup_wide_single" (hits sorted in one pass), "lookup_wide_grouped" (hits
 * split into groups of rank bins), "lookup_wide_group_passes" (the passes those took), "lookup_wide_overflow" (one rank bin
 * alone beyond the buffer: handed to the wave-per-range kernel); and the waves of a level counted under option
 * "lookup_coop": "lookup_coop_waves" (counted together), "lookup_lane_waves_mixed" (range by range: more than one target,
 * an unknown one or one without entries), "lookup_lane_waves_span" (range by range: a span beyond "lookup_coop_span").
 * Of the last device BED call on the handle
 * (impg_gpu_query_batch_bed, impg_gpu_query_batch_bed_fd, impg_gpu_selftest_bed_rows; zero when it starts, every chunk adds;
 * on a multi-GPU handle its ranks count, not the handle): "bed_rows" = rows entering the merges, "bed_gap_roots" = rows
 * after merge_adjusted_intervals_gap_2d, "bed_runs" = merged rows out, "bed_text_pieces" = text pieces sent to the host,
 * "bed_text_bytes" = bytes printed.  Of the last device BEDPE call on the handle (impg_gpu_query_batch_bedpe,
 * impg_gpu_query_batch_bedpe_fd; kept the same way): "bedpe_rows" = rows after each range's first is dropped,
 * "bedpe_runs" = lines printed, "bedpe_joins_contiguous" / "bedpe_joins_gap" = rows joined to the row before them by either
 * arm of merge_adjusted_intervals, "bedpe_fused_ops" = I / D ops removed by fusing neighbours, at joins and inside joined
 * rows, "bedpe_summary_ops" = CIGAR ops the summary kernel read, "bedpe_text_pieces" = text pieces sent to the host,
 * "bedpe_text_bytes" = bytes printed.  Of the last device PAF call on the handle (impg_gpu_query_batch_paf,
 * impg_gpu_query_batch_paf_fd, impg_gpu_selftest_paf_rows; kept the same way): "paf_rows" = rows after each range's first is
 * dropped, "paf_runs" = lines printed, "paf_joins_contiguous" / "paf_joins_gap" = rows joined to the row before them by
 * either arm of merge_adjusted_intervals, "paf_ops_read" = CIGAR ops of those rows, "paf_ops_printed" = ops written into
 * cg:Z (fused ops, and the raw ops of lines made of one row), "paf_through_rows" = rows that print no op of their own (one
 * group of ops that started in a row before them and goes on), "paf_text_pieces" = text pieces sent to the host,
 * "paf_text_bytes" = bytes printed.  Of the last device FASTA call on the handle (impg_gpu_query_batch_fasta,
 * impg_gpu_query_batch_fasta_fd, impg_gpu_selftest_fasta_rows; kept the same way): "fasta_rows" = rows entering the sweep,
 * "fasta_records" = records printed, "fasta_text_pieces" = text pieces sent to the host, "fasta_text_bytes" = bytes printed;
 * "fasta_store_bytes" = bytes of HBM the attached sequence store takes, in whichever form it has -- the bases, and the
 * packed form's runs and block tables (0: none attached), "fasta_store_packed" = 1 if the attached store is the packed
 * form (0: one byte per base, or none attached), "fasta_store_exception_runs" = the runs of bytes other than A/C/G/T the
 * packed form keeps (0 for the byte form, and with none attached).  Of the last impg_gpu_index_load_sequences on the handle
 * (zero after impg_gpu_index_set_sequences): "sequence_ingest_pieces" = text pieces sent to the device,
 * "sequence_ingest_text_bytes" = bytes of (inflated) text, "sequence_ingest_bases" = bases met, those of dropped sequences
 * included, "sequence_ingest_inflated_blocks" = BGZF blocks inflated, "sequence_ingest_dropped_sequences" = file sequences
 * the index does not know.  Of the ingest of impg_gpu_index_create_from_paf_streamed (all zero on any other index):
 * "paf_ingest_device" = 1 on that route, "paf_ingest_pieces" = text pieces sent to the device, "paf_ingest_text_bytes" =
 * bytes of (inflated) text, "paf_ingest_lines" = lines parsed, "paf_ingest_carried_bytes" = bytes behind a piece's last
 * newline moved to the front of the next piece, "paf_ingest_buffer_grows" = doublings of the piece buffer for a line longer
 * than it, "paf_ingest_pool_regrows" = device-to-device copies of the op pool into a larger one,
 * "paf_ingest_unknown_names" = name occurrences sent home because the device's table did not hold them,
 * "paf_ingest_inflated_blocks" = BGZF blocks inflated.  Of the build of the index itself (a multi-GPU handle answers with the sum over its
 * ranks): "build_device" = 1 if the device builder produced it, 0 if the host builder did (IMPG_BUILD_HOST, tracepoints, a
 * loaded .impg file's entry order, a card short of memory for the build, an index loaded from a saved file);
 * "tokenized_device" = 1 if the device tokenised its CIGAR text (impg_gpu_index_create_from_paf and
 * impg_gpu_index_create_from_paf_streamed on one GPU);
 * "build_batches" = the op-pool uploads of the device build, one tiles launch each (1 unless the pool exceeds the batch
 * size, 64 M ops or IMPG_BUILD_BATCH_OPS). */
int impg_gpu_get_counter(const impg_gpu_index_t *, const char *key, int64_t *value_out);
/* Large result arrays live in pinned host blocks that are recycled through a process-wide pool (at most
 * IMPG_PINNED_POOL_BYTES, default 6 GiB, are kept when results are freed).  Gives pooled blocks back to the system
 * until at most keep_bytes are held; returns the number of bytes freed. */
uint64_t impg_gpu_host_pool_trim(uint64_t keep_bytes);

/* Visit rank of the sorted positions 0..n-1 of an n-entry target under an order
 * policy (what the index stores per entry); host-only, no GPU needed. */
int impg_gpu_visit_rank(uint32_t n, int order_policy, uint32_t *rank_out);

/* ---- queries ------------------------------------------------------------ */
/* Batch form of ImpgIndex::query / query_transitive_bfs / _dfs: one independent
 * query per range (each with its own visited set).  Results are grouped by
 * range, in the reference's emission order, self interval(s) first.
 * Unknown target or a target without alignments => self interval only
 * (impg.rs:1896).  Requires start < end. */
int impg_gpu_query_batch(impg_gpu_index_t *, const impg_gpu_range_t *ranges, size_t n,
                         const impg_gpu_params_t *params, impg_gpu_results_t **out);
/* Single range == batch of one; what a per-call `impl ImpgIndex` binds. */
/* masked_regions: Option<&FxHashMap<u32, SortedRanges>> of query_transitive_bfs / query_transitive_dfs
 * (impg.rs:2062, :2316; multi_impg.rs:692, :727, :801), as partition.rs:250-256, :364, :380 passes it.
 * One map for the whole batch: every range starts from its own clone of it (impg.rs:2077-2081), so a
 * batch under one mask equals the reference's per-range calls with the same map.  The map is given as
 * n_seqs entries in strictly ascending sequence-id order: SortedRanges.sequence_length, and
 * ranges[2*range_off[i] .. 2*range_off[i+1]) as (start, end) pairs, sorted, disjoint and non-touching
 * (the SortedRanges invariant).  Every SortedRanges has min_distance 0, as partition builds them.
 * A sequence absent from the map follows the reference: Impg gives it a set of length 0 (visited_entry,
 * impg.rs:2048-2053: its hits are reported but never expanded), MultiImpg its real length, except the
 * range's own target (entry().or_default(), multi_impg.rs:827-830: no result at all).
 * A range can now have several self intervals, or none; they lead its results in ascending order.
 * mask == NULL is impg_gpu_query_batch.  Only the transitive queries take a mask (IMPG_E_INVALID). */
typedef struct {
  uint32_t n_seqs;
  const uint32_t *seq_id;          /* [n_seqs] */
  const int32_t *sequence_length;  /* [n_seqs] */
  const uint64_t *range_off;       /* [n_seqs + 1] */
  const int32_t *ranges;           /* [2 * range_off[n_seqs]] */
} impg_gpu_mask_t;
int impg_gpu_query_batch_masked(impg_gpu_index_t *, const impg_gpu_range_t *ranges, size_t n,
                                const impg_gpu_params_t *params, const impg_gpu_mask_t *mask,
                                impg_gpu_results_t **out);
/* subset_filter: Option<&SubsetFilter> of the three trait methods (`--subset-sequence-list`).  The name
 * matching (SubsetFilter::matches, subset_filter.rs:23-60: exact / coordinate-stripped / sample / haplotype
 * keys) is host string work and stays with the host: it hands over its verdict per sequence id,
 * subset_keep[num_seqs], non-zero = matches.  A hit is kept iff its query sequence is the range's own
 * target or subset_keep says so -- while exploring for the transitive queries (impg.rs:2176-2185,
 * :2430-2439; multi_impg.rs:888-896: a dropped hit is neither reported nor expanded), after the query
 * otherwise (perform_query, main.rs:11693-11696).  mask and subset_keep may each be NULL. */
int impg_gpu_query_batch_filtered(impg_gpu_index_t *, const impg_gpu_range_t *ranges, size_t n,
                                  const impg_gpu_params_t *params, const impg_gpu_mask_t *mask,
                                  const uint8_t *subset_keep, impg_gpu_results_t **out);
/* The same rows for a batch too big for one result object (the 100 000-range headline batch returns 2.1 x 10^9 rows,
 * 51 GB): the batch is cut into chunks of chunk_ranges ranges (0 = 8192; a chunk that outgrows the pair budget or
 * max_block_bytes of rows -- 0 = 2.5 GiB, two of which the library's pinned pool keeps between calls -- is halved, and so
 * are the chunks after it), two engines compute them in turn, and `cb` receives every chunk
 * as a results object (the impg_gpu_results_* accessors; its range i is ranges[first_range + i]) valid until the
 * callback returns -- IN RANGE ORDER, one call at a time, from a thread of the library, while the next chunk is
 * computed and copied: what a caller that prints or folds range by range consumes (main.rs:7435-7470).  Host memory:
 * two pinned blocks of at most max_block_bytes (+ the CIGAR pools under store_cigar).  A non-zero return of the
 * callback stops the stream (IMPG_E_CANCELLED).  mask / subset_keep as in impg_gpu_query_batch_filtered (NULL = none).
 * On a sharded index the chunks run one after the other through the collective call (no overlap). */
typedef int (*impg_gpu_stream_cb)(void *ctx, const impg_gpu_results_t *chunk, size_t first_range);
int impg_gpu_query_batch_stream(impg_gpu_index_t *, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                                const impg_gpu_mask_t *mask, const uint8_t *subset_keep, size_t chunk_ranges, size_t max_block_bytes,
                                impg_gpu_stream_cb cb, void *ctx, uint64_t *projected_out);
/* The name matching for hosts that do not bring their own SubsetFilter: list_text is the content of a
 * `--subset-sequence-list` file (one name per line, '#' comments; parse_subset_filter, subset_filter.rs:117-141);
 * keep_out[i] = SubsetFilter::matches(names[i]) (:23-60: exact, without ":start-end", or by the
 * sample / sample+haplotype key of "S_hapN…" and "S#N#…" names, :143-176).  *n_entries = SubsetFilter::entry_count
 * (the reference refuses a list with 0 entries, :76-81).  Host-only: needs no device. */
int impg_gpu_subset_keep(const char *list_text, size_t len, const char *const *names, size_t n, uint8_t *keep_out,
                         size_t *n_entries);
int impg_gpu_query(impg_gpu_index_t *, uint32_t target_id, int32_t start, int32_t end,
                   const impg_gpu_params_t *params, impg_gpu_results_t **out);

size_t impg_gpu_results_num_ranges(const impg_gpu_results_t *);
size_t impg_gpu_results_total(const impg_gpu_results_t *);
/* offsets[n_ranges+1] into intervals[]; both owned by the results object */
const uint64_t *impg_gpu_results_offsets(const impg_gpu_results_t *);
const impg_gpu_interval_t *impg_gpu_results_intervals(const impg_gpu_results_t *);
/* store_cigar: the Vec<CigarOp> of every interval (impg.rs:1870-1872, :2878-2886),
 * packed ops at cigar_ops[cigar_offsets[i] .. cigar_offsets[i+1]); NULL when the
 * query ran with store_cigar = 0 */
const uint64_t *impg_gpu_results_cigar_offsets(const impg_gpu_results_t *);
const uint32_t *impg_gpu_results_cigar_ops(const impg_gpu_results_t *);
/* number of Some(..) projections (self intervals excluded) = the work unit of BASELINE.md */
uint64_t impg_gpu_results_projected(const impg_gpu_results_t *);
/* wall seconds the call spent in the engine (lookup / projection / update on the GPU) and in copying the hit
 * slots back and assembling them into per-range result lists on the host */
void impg_gpu_results_timing(const impg_gpu_results_t *, double *engine_s, double *assemble_s);
void impg_gpu_results_free(impg_gpu_results_t *);

/* Throughput form: same computation, results stay in HBM; returns per-range
 * hit counts and an order-independent 64-bit checksum of each range's hits
 * (either may be NULL), the number of projections, and per-stage times. */
typedef struct {
  uint64_t projected;      /* accepted projections */
  uint64_t pairs;          /* (range, entry) candidate pairs examined */
  uint64_t frontier_ranges;/* frontier ranges looked up over all levels */
  uint32_t levels;
  float ms_total;          /* HIP-event time of the whole call on the engine stream */
  float ms_lookup, ms_project, ms_update; /* per-stage kernel time (HIP events) */
  uint64_t project_launches;              /* launches of the projection kernel */
  float ms_exchange;                      /* sharded index: wall time inside the transport (all-gathers + all-to-all-v) */
} impg_gpu_stats_t;
int impg_gpu_query_batch_stats(impg_gpu_index_t *, const impg_gpu_range_t *ranges, size_t n,
                               const impg_gpu_params_t *params, uint64_t *per_range_count,
                               uint64_t *per_range_checksum, impg_gpu_stats_t *stats);
/* Same with the ranges already resident in HBM (device pointer; not for a multi handle, whose ranges span GPUs). */
int impg_gpu_query_batch_stats_dev(impg_gpu_index_t *, const impg_gpu_range_t *d_ranges, size_t n,
                                   const impg_gpu_params_t *params, uint64_t *per_range_count,
                                   uint64_t *per_range_checksum, impg_gpu_stats_t *stats);

/* ---- rows left in HBM ------------------------------------------------------------------------------------
 * The same queries with every result row left ON THE DEVICE, complete and attributable, for a consumer that lives
 * there too (the BED merges of this library are one; a caller's own kernels another): no row crosses PCIe, no
 * per-range statistics are folded.  What the reference's sequential phase pushes per hit -- the AdjustedInterval with
 * the frontier range's target as its target metadata (impg.rs:2491-2503, :1920-1923) -- is here one slot of a PART:
 * the hits of one BFS level (level 0 = the hits of the ranges themselves; a plain query has only that) of one chunk of
 * the batch, as device arrays of n_slots entries
 *     query_id[s*k] the hit's query sequence; 0xFFFFFFFF = the projection returned None (impg.rs:2874-2877), or the
 *                   subset filter dropped the hit: not a row
 *     coords[4k..]  q_first, q_last, t_first, t_last (q_first > q_last: reverse strand)
 *     source[s*k]   index into frontier[]: the frontier record the hit was found with
 *                   (s = slot_stride: 1, or 2 where the part keeps a slot's query_id and source side by side as one
 *                   8-byte pair -- the fused final level, which writes them with one store)
 *     frontier[j]   {target_id, start, end, range_idx}: the row's target sequence (the target interval's metadata) and
 *                   the range of the batch it belongs to, as ranges[first_range + range_idx] (a sharded index: the
 *                   collective batch, below)
 * i.e. SURVEY-style 24 bytes per slot (query_id, four coordinates, source) with range_idx and target_id one
 * look-up away.  Slot order within a part is unspecified (IMPG_ROWS_ATTRIBUTED): the final level is written entry by
 * entry, which is what makes it fast; a caller that needs the reference's emission order asks impg_gpu_query_batch /
 * _stream for it.  Transitive rows shorter than min_output_length (impg.rs:2482-2504) are NOT removed from the
 * slots: compare |q_last - q_first| as the reference does.  The self interval of a range is the range itself
 * (impg.rs:1864-1880, :2345-2363) and is not stored.
 * Takes Impg::query and query_transitive_bfs on a CIGAR or tracepoint index (IMPG_E_UNSUPPORTED: DFS, MultiImpg
 * worklists, store_cigar).  ranges_on_device != 0: `ranges` is a device pointer.
 * One GPU: the handle holds one of the index's engines (max 4) and its HBM until impg_gpu_device_rows_free.
 * A sharded index (IMPG_ROWS_ATTRIBUTED only; the ordered layouts are IMPG_E_UNSUPPORTED there): a multi-GPU handle takes
 * host ranges (ranges_on_device: IMPG_E_INVALID); in rank processes the call is COLLECTIVE -- every rank passes its own
 * ranges, host or device, as with impg_gpu_query_batch_stats.  Ranges are numbered in the COLLECTIVE BATCH: the multi
 * handle's batch, or the ranks' batches concatenated in rank order (impg_gpu_device_rows_batch_offset).  Levels whose hits
 * came home for the visited-set update stay with the home rank, first_range = the home's offset in the collective batch
 * + the chunk's first range.  The final level is never shipped home: it stays in the HBM of the rank that projected
 * it, as OWNER PARTS -- one per slice that owner expanded, first_range = 0, n_ranges = the collective batch size,
 * frontier[].range_idx = the collective range, each with its own copy of the records its source[] indexes.  So
 * first_range + frontier[source[s]].range_idx names a slot's range in every part.  A part's arrays are on the device
 * impg_gpu_device_rows_part_device names.  A sharded handle holds no engine: every array belongs to the handle, freed
 * by impg_gpu_device_rows_free. */
typedef struct impg_gpu_device_rows impg_gpu_device_rows_t;
#define IMPG_ROWS_ATTRIBUTED 0
/* IMPG_ROWS_ORDERED: the trait's own rows instead -- one part per chunk: rows[n_slots] (impg_gpu_interval_t, no holes)
 * grouped by range in the reference's emission order, self interval(s) first, offsets[n_ranges + 1] (u32) into them:
 * exactly what impg_gpu_query_batch returns, left in HBM (transitive rows below min_output_length removed). */
#define IMPG_ROWS_ORDERED 1
/* IMPG_ROWS_ORDERED_SLOTS: the same grouping and order with every SLOT at its place -- a (range, alignment) pair whose
 * projection returned None (impg.rs:2874-2877: 7 in 10^5 at the headline), or whose transitive row is shorter than
 * min_output_length, stays as a HOLE row, query_id = 0xFFFFFFFF, instead of moving every row behind it up: skip those
 * (offsets[] counts them).  Where a row goes then follows from the lookups' counts alone, so the final level's kernel
 * writes its rows itself where they belong -- no scans and scatters over 2 x 10^9 rows: the headline batch's rows are in
 * HBM in emission order in ~49 ms where IMPG_ROWS_ORDERED takes 109 (a lane per place, a range's
 * places in visit order, so that a wave's rows are one stretch of the output). */
#define IMPG_ROWS_ORDERED_SLOTS 2
typedef struct {
  uint32_t target_id;
  int32_t start, end;
  uint32_t range_idx; /* relative to the part's first_range */
} impg_gpu_frontier_t;
typedef struct {
  size_t first_range, n_ranges; /* the chunk of the batch the part belongs to (chunks: "chunk_ranges" / "pair_budget") */
  uint32_t level;               /* BFS level of the part's hits */
  uint32_t n_frontier;
  uint32_t slot_stride;         /* 4-byte words between consecutive slots' query_id (and source) */
  uint64_t n_slots;
  const uint32_t *query_id;     /* [slot_stride * n_slots]  device */
  const int32_t *coords;        /* [4 * n_slots]            device, 16-byte aligned */
  const uint32_t *source;       /* [slot_stride * n_slots]  device */
  const impg_gpu_frontier_t *frontier; /* [n_frontier] device */
  const impg_gpu_interval_t *rows;     /* IMPG_ROWS_ORDERED[_SLOTS]: [n_slots] device (the fields above are NULL / 0) */
  const uint32_t *offsets;             /* IMPG_ROWS_ORDERED[_SLOTS]: [n_ranges + 1] device */
} impg_gpu_device_part_t;
int impg_gpu_query_batch_device(impg_gpu_index_t *, const impg_gpu_range_t *ranges, size_t n, int ranges_on_device,
                                const impg_gpu_params_t *params, int layout, impg_gpu_device_rows_t **out);
size_t impg_gpu_device_rows_num_parts(const impg_gpu_device_rows_t *);
int impg_gpu_device_rows_part(const impg_gpu_device_rows_t *, size_t k, impg_gpu_device_part_t *out);
/* the HIP device that holds part k's arrays (a multi-GPU handle: the device of the rank that holds the part) */
int impg_gpu_device_rows_part_device(const impg_gpu_device_rows_t *, size_t k, int *device_out);
/* where the caller's ranges start in the collective batch, and its size: a rank process's offset = the sizes of the
 * lower ranks' batches; one GPU and a multi-GPU handle: 0 and n */
int impg_gpu_device_rows_batch_offset(const impg_gpu_device_rows_t *, uint64_t *offset_out, uint64_t *total_out);
/* projections, candidate pairs and per-stage times of the call (impg_gpu_stats_t as above) */
void impg_gpu_device_rows_stats(const impg_gpu_device_rows_t *, impg_gpu_stats_t *stats);
/* ordered layout: HIP-event milliseconds the row placement took on top of stats->ms_total */
float impg_gpu_device_rows_place_ms(const impg_gpu_device_rows_t *);
/* Verification: the per-range counts and order-independent checksums of impg_gpu_query_batch_stats, recomputed FROM
 * THE ROWS the call left in HBM (every slot attributed through source[] / frontier[]); either may be NULL.  Arrays of
 * the caller's own ranges.  A sharded index: every rank's partial sums are added (wrapping, as the checksums are); in
 * rank processes the call is COLLECTIVE -- the partial arrays go to their home ranks through the index's communicator. */
int impg_gpu_device_rows_check(impg_gpu_device_rows_t *, uint64_t *per_range_count, uint64_t *per_range_checksum);
void impg_gpu_device_rows_free(impg_gpu_device_rows_t *);

/* ---- BED: merge_adjusted_intervals_gap_2d + merge_query_adjusted_intervals +
 *      output_results_bed (main.rs:12858-13011, :12474-12560, :11849-11892) ---- */
/* In-place merge of one range's results as output_results_bed does for BED
 * (all CIGARs empty).  Returns the new count. */
long impg_gpu_bed_merge(impg_gpu_interval_t *iv, size_t n, int32_t merge_distance,
                        int merge_strands);
/* Render results as BED text.  range_names[i] is BED column 4 of range i.
 * The non-transitive min_output_length retain of perform_query
 * (main.rs:11682-11688) is applied here.  *text is malloc'ed; free() it. */
int impg_gpu_results_bed(const impg_gpu_results_t *, const impg_gpu_index_t *,
                         const char *const *range_names, const impg_gpu_params_t *params,
                         int32_t merge_distance, char **text, size_t *len);

/* perform_query + output_results_bed for a whole batch in one call, with both merges ON THE DEVICE
 * (bed_device.hip): the hit slots never leave HBM; they are turned into rows, sorted, chained
 * (merge_adjusted_intervals_gap_2d) and swept (merge_query_adjusted_intervals) there, and only the merged rows --
 * 16 bytes each -- are formatted there as well; the text crosses PCIe in pinned pieces while the next piece is being
 * formatted.  The text is byte-identical to impg_gpu_query_batch_filtered +
 * impg_gpu_results_bed (what `impg query -o bed` prints: main.rs:7435-7470, :11849-11892).  range_names as in
 * impg_gpu_results_bed (NULL, or NULL entries, = "{name}:{start}-{end}").  subset_keep may be NULL.  seconds3, if
 * not NULL, receives the wall seconds of {engine, device-side merge + copy back, text}.  On an index sharded over GPUs the
 * merges and the text run on each range's home rank and the pieces are concatenated in the caller's order. */
int impg_gpu_query_batch_bed(impg_gpu_index_t *, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                             const uint8_t *subset_keep, int32_t merge_distance, const char *const *range_names, char **text,
                             size_t *len, double *seconds3);
/* The same, the text written to a file descriptor piece by piece instead of collected (what the CLI does: gigabytes
 * of BED never exist as one host buffer). */
int impg_gpu_query_batch_bed_fd(impg_gpu_index_t *, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                                const uint8_t *subset_keep, int32_t merge_distance, const char *const *range_names, int fd,
                                uint64_t *bytes_written, double *seconds3);

/* ---- PAF / BEDPE: results.remove(0) + merge_adjusted_intervals (CIGAR-faithful
 *      merge: contiguity, identical overlap, gaps <= -d) + output_results_paf /
 *      output_results_bedpe with gi:f / bi:f (main.rs:7472-7496, :11894-12103,
 *      :12563-12845, :13014-13180).  The results must come from a query with
 *      store_cigar = 1.  *text is malloc'ed; free() it.
 *      Results of a tracepoint index (option "approximate_cigar") print as IMPG_OUT_BEDPE -- what `impg query
 *      --approximate -o bedpe` prints: the same merge and the same gi:f / bi:f, fed with the two-count CIGARs --
 *      and are IMPG_E_UNSUPPORTED as IMPG_OUT_PAF, a format the reference refuses in approximate mode
 *      (main.rs:7387-7397).  A range holding a row without ops is IMPG_E_UNSUPPORTED in either kind of
 *      index (the reference merges such a range by gaps alone, main.rs:11905-11910: not built). ---- */
#define IMPG_OUT_PAF 0
#define IMPG_OUT_BEDPE 1
int impg_gpu_results_paf(const impg_gpu_results_t *, const impg_gpu_index_t *,
                         const char *const *range_names, const impg_gpu_params_t *params,
                         int32_t merge_distance, int format, char **text, size_t *len);

/* ---- BEDPE on the device (bedpe_device.hip): perform_query + results.remove(0) + merge_adjusted_intervals +
 *      output_results_bedpe for a whole batch in one call, byte-identical to impg_gpu_query_batch_filtered with
 *      store_cigar = 1 + impg_gpu_results_paf(IMPG_OUT_BEDPE) (what `impg query -b` prints by default).  BEDPE prints no
 *      CIGAR, only gi:f / bi:f: every row's ops are summed where the engine left them, rows are sorted, joined with the
 *      row before them and printed on the device; no row and no op crosses PCIe, only text, in pinned pieces (option
 *      "bed_text_piece_bytes").  Arguments, range_names, subset_keep and seconds3 {engine, rows + CIGARs + summaries +
 *      merge, text} as impg_gpu_query_batch_bed; params->store_cigar is taken as 1.  Errors, each raised before any text
 *      of the chunk (option "chunk_ranges") that holds it is delivered: IMPG_E_INVALID for a range without a row to drop
 *      and for a target interval that runs backwards where the reference looks (a range with two rows or more, merge_distance
 *      >= 0); IMPG_E_UNSUPPORTED for a row without ops, and -- where impg_gpu_results_paf still serves -- for a sharded or
 *      multi-GPU handle, for an index with a sequence of 2^29 bases or more (a fused op that long would wrap into its code
 *      bits there) and for a tracepoint index without option "approximate_cigar". ---- */
int impg_gpu_query_batch_bedpe(impg_gpu_index_t *, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                               const uint8_t *subset_keep, int32_t merge_distance, const char *const *range_names, char **text,
                               size_t *len, double *seconds3);
/* The same, the text written to a file descriptor piece by piece (what the CLI does). */
int impg_gpu_query_batch_bedpe_fd(impg_gpu_index_t *, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                                  const uint8_t *subset_keep, int32_t merge_distance, const char *const *range_names, int fd,
                                  uint64_t *bytes_written, double *seconds3);

/* ---- PAF on the device (paf_device.inc): the same call for `impg query -o paf`, byte-identical to
 *      impg_gpu_query_batch_filtered with store_cigar = 1 + impg_gpu_results_paf(IMPG_OUT_PAF).  The merge is BEDPE's; the
 *      merged CIGAR of every line -- its rows' ops and the joins' gap ops, neighbours of one code fused -- is computed and
 *      printed as cg:Z on the device (option "paf_group_log2"), so that only text crosses PCIe.  Arguments, seconds3 and
 *      errors as impg_gpu_query_batch_bedpe, except that a tracepoint index is IMPG_E_UNSUPPORTED whatever its options (the
 *      reference prints no PAF in approximate mode); a line longer than a text piece (option "bed_text_piece_bytes") is
 *      IMPG_E_UNSUPPORTED. ---- */
int impg_gpu_query_batch_paf(impg_gpu_index_t *, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                             const uint8_t *subset_keep, int32_t merge_distance, const char *const *range_names, char **text,
                             size_t *len, double *seconds3);
int impg_gpu_query_batch_paf_fd(impg_gpu_index_t *, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                                const uint8_t *subset_keep, int32_t merge_distance, const char *const *range_names, int fd,
                                uint64_t *bytes_written, double *seconds3);

/* ---- FASTA: `impg query -o fasta` (output_results_fasta, main.rs:12351-12415) -------------------------------------
 * The sequences: plain FASTA files (the name runs to the first whitespace of the '>' line; body lines of any length; '\r'
 * dropped; bytes upper-cased at load; an empty sequence and a last line without a newline are accepted), or arrays of the
 * caller's (names[n], off[n + 1] into bases; upper-cased too).  One byte per base on the host, so IUPAC codes and N stay
 * exact; in HBM one byte per base too, or two bits per base with those bytes kept aside (option "sequence_store_packed").
 * IMPG_E_UNSUPPORTED for a file that starts with the gzip magic 1f 8b (this route has no codec: decompress first, or use
 * impg_gpu_index_load_sequences); IMPG_E_INVALID,
 * naming it, for a name that occurs twice, in one file or across files (the reference lets the last file win);
 * IMPG_E_IO for a file that cannot be read.  Host-only.  _name / _bases: sequence i as the store holds it (NULL past the
 * last; the bases are not NUL-terminated, *len = their number).  (impg_gpu_sequences_t is declared above, with the
 * resolve pass that reads it.) */
int impg_gpu_sequences_from_fasta(const char *const *paths, size_t n_paths, impg_gpu_sequences_t **out);
int impg_gpu_sequences_from_memory(const char *const *names, const uint64_t *off, const char *bases, size_t n, impg_gpu_sequences_t **out);
size_t impg_gpu_sequences_num(const impg_gpu_sequences_t *);
const char *impg_gpu_sequences_name(const impg_gpu_sequences_t *, size_t i);
const char *impg_gpu_sequences_bases(const impg_gpu_sequences_t *, size_t i, uint64_t *len);
/* Sequence i's exceptions as the packed form of the store keeps them (host-only; impg_gpu_index_set_sequences extracts the
 * same at attach): the maximal runs of ONE byte that is not A/C/G/T after upper-casing, in order -- "NNNRR" is two runs --,
 * run k = bases [start[k], start[k] + len[k]) printing as byte[k].  *n_runs = their number; the first min(cap, *n_runs) are
 * written (cap = 0: the arrays may be NULL).  IMPG_E_INVALID past the last sequence. */
int impg_gpu_sequences_exceptions(const impg_gpu_sequences_t *, size_t i, uint32_t *start, uint32_t *len, uint8_t *byte, size_t cap, size_t *n_runs);
void impg_gpu_sequences_free(impg_gpu_sequences_t *);
/* Attaches the store to an index handle: its sequences are matched to the index's by name and their bases uploaded to the
 * handle's device (back to back, one byte per base, padded by 16 bytes or more at both ends; a 64-bit offset per index id,
 * all ones where the store lacks the sequence).  Index sequences the store lacks, and store sequences the index lacks, are
 * tolerated; a sequence whose length differs from impg_gpu_seq_len is IMPG_E_INVALID, naming it.  The handle shares the
 * store's host copy (the host route reads it): the caller may free its own handle at once.  seqs == NULL detaches.  A
 * tracepoint index (it has no names) and a sharded handle: IMPG_E_UNSUPPORTED.  Not to be called while a query runs.
 * Under option "sequence_store_packed" = 1 (or 2, where that is smaller) the bases go to HBM packed instead: two bits per
 * base (A C G T = 0 1 2 3, base i in bits 2 * (i & 3) and up of byte i >> 2), 16 zero bytes in front, every sequence from a
 * multiple of 64 bases on, 64 zero bytes or more behind the last, the offsets counting bases; every other byte packs as 0
 * and is kept as a run (impg_gpu_sequences_exceptions) with a table over each sequence's blocks of 1 024 bases to find its
 * runs by: bases / 4 + 9 bytes per run + 16 bytes per sequence, + 4 bytes per 1 024 bases of a sequence that has runs.  The
 * bases are packed on the device chunk by chunk through one staging buffer (64 MiB), so the attach never holds the store
 * at a byte per base in HBM.  The text every FASTA call prints is the same, byte for byte; the host copy stays as it is. */
int impg_gpu_index_set_sequences(impg_gpu_index_t *, const impg_gpu_sequences_t *seqs);
/* The second way to give an index its sequences: FASTA files streamed straight into HBM.  A file's text -- plain, or inflated
 * on a few host threads if it starts with the gzip magic: BGZF (recognised by its BC subfield) block by block, any other
 * gzip as one stream -- crosses PCIe in pieces of option "sequence_ingest_piece_bytes" through two pinned blocks, and
 * everything that touches a base happens on the device: finding the header lines, dropping the line ends, upper-casing,
 * placing, packing to 2 bits and extracting the runs (sequence_ingest_device.hip).  The store that results is the one
 * impg_gpu_sequences_from_fasta + impg_gpu_index_set_sequences make from the same text, rule for rule (names, bases, empty
 * lines, CRLF, a last line without a newline; a name twice, an empty name and text before the first '>' are IMPG_E_INVALID
 * with the same words; a sequence whose base count differs from impg_gpu_seq_len likewise), in the form option
 * "sequence_store_packed" names at the call: 0 bytes, 1 packed; 2 is IMPG_E_INVALID here (the smaller form is known only
 * once every run is counted: impg_gpu_index_set_sequences keeps that choice).  Sequences are placed in file order, in a
 * reservation made once for ALL of the index's sequences ("fasta_store_bytes" reports what is used); file sequences the
 * index lacks are parsed and dropped, index sequences the files lack are absent as after impg_gpu_index_set_sequences.
 * IMPG_E_IO, naming the file: an unreadable file, a truncated gzip stream, a BSIZE or ISIZE that leads outside the file, a
 * CRC or length mismatch, an inflate error.  IMPG_E_UNSUPPORTED: a tracepoint index, a sharded or multi-GPU handle.  The
 * call replaces any attached store; after a failure the handle has none.  No host copy of the bases exists afterwards:
 * impg_gpu_results_fasta, a partition session with its state on the host, and impg_gpu_partition_rows_fasta(on_host)
 * answer IMPG_E_UNSUPPORTED naming impg_gpu_index_set_sequences.  Sets the "sequence_ingest_*" and "fasta_store_*" counters. */
int impg_gpu_index_load_sequences(impg_gpu_index_t *, const char *const *paths, size_t n_paths);
/* Diagnostics, host-only (no GPU call): the reader alone -- the concatenation of `path`'s pieces of piece_bytes, their
 * number and the BGZF blocks inflated; *text is malloc'ed -- and the whole route with the kernels' host twin
 * (ingest_piece_host, sequence_ingest.cpp) in their place, for an index of n_ids sequences names_of_ids / lens.  packed: 0 or
 * 1.  off[n_ids]: every id's place (bytes, or bases of the packed stream; all ones: absent); *store: the bytes, or the packed
 * stream; run_off[n_ids + 1] and *run_start / *run_end / *run_byte: the packed form's runs by id (ends exclusive);
 * stats[5] (may be NULL): the five "sequence_ingest_*" counters in the order above.  The arrays are malloc'ed; free() them.
 * Errors as impg_gpu_index_load_sequences. */
int impg_gpu_selftest_sequence_reader(const char *path, uint64_t piece_bytes, char **text, size_t *len, uint64_t *n_pieces, uint64_t *inflated_blocks);
int impg_gpu_selftest_sequence_ingest_host(const char *const *paths, size_t n_paths, const char *const *names_of_ids, const int64_t *lens, size_t n_ids,
                                           uint64_t piece_bytes, int packed, uint64_t *off, uint8_t **store, size_t *store_bytes, uint64_t *run_off,
                                           uint32_t **run_start, uint32_t **run_end, uint8_t **run_byte, uint64_t *stats);
/* perform_query + output_results_fasta for a whole batch, the sweep (merge_query_adjusted_intervals alone, strands kept
 * apart: main.rs:12362, :4395-4409) and the records written ON THE DEVICE (fasta_device.hip) from the store in HBM: per merged
 * row ">{name}:{start}-{end}" ("/rc" appended and the bases reverse-complemented -- A/T/C/G/N, other bytes as they are -- on
 * a reverse-strand row under reverse_complement), then the bases in lines of 80; a zero-length row prints its header and an
 * empty line.  Arguments as impg_gpu_query_batch_bed plus reverse_complement; range_names is accepted and unused;
 * params->store_cigar is taken as 0 and original_sequence_coordinates does not touch the text; seconds3 = {engine, rows +
 * merge, text}.  The text crosses PCIe as BED's does (option "bed_text_piece_bytes"): a record longer than a piece is
 * IMPG_E_UNSUPPORTED.  Raised before any text of the chunk that holds it is delivered: IMPG_E_INVALID, naming the sequence,
 * for a merged row on a sequence the store lacks (the reference fails with NotFound) or a row that leaves its sequence;
 * before anything runs: IMPG_E_INVALID without a store, IMPG_E_UNSUPPORTED for a sharded or multi-GPU handle. */
int impg_gpu_query_batch_fasta(impg_gpu_index_t *, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                               const uint8_t *subset_keep, int32_t merge_distance, const char *const *range_names, int reverse_complement,
                               char **text, size_t *len, double *seconds3);
int impg_gpu_query_batch_fasta_fd(impg_gpu_index_t *, const impg_gpu_range_t *ranges, size_t n, const impg_gpu_params_t *params,
                                  const uint8_t *subset_keep, int32_t merge_distance, const char *const *range_names, int reverse_complement,
                                  int fd, uint64_t *bytes_written, double *seconds3);
/* The host twin: the same text from the rows of impg_gpu_query_batch[_filtered] (store_cigar = 0) and the handle's host copy
 * of the store, with the min_output_length retain of impg_gpu_results_bed.  *text is malloc'ed; free() it. */
int impg_gpu_results_fasta(const impg_gpu_results_t *, const impg_gpu_index_t *, const impg_gpu_params_t *params, int32_t merge_distance,
                           int reverse_complement, char **text, size_t *len);
/* One range's rows -> its records, host-only (no handle, no GPU call): the sweep, then the text.  names_of_ids[n_ids]: the
 * name of every sequence id the rows use.  Errors as above.  *text is malloc'ed; free() it. */
int impg_gpu_fasta_text(const impg_gpu_sequences_t *seqs, const char *const *names_of_ids, size_t n_ids, const impg_gpu_interval_t *rows, size_t n,
                        int32_t merge_distance, int reverse_complement, char **text, size_t *len);
/* Diagnostics: the device sweep and writer of impg_gpu_query_batch_fasta on rows the caller brings (row_range[i] = the range
 * of rows[i], below n_ranges; ids below the index's number of sequences), without a query in front.  Errors as
 * impg_gpu_query_batch_fasta.  *text is malloc'ed; free() it.  Sets the "fasta_*" counters. */
int impg_gpu_selftest_fasta_rows(impg_gpu_index_t *ix, const impg_gpu_interval_t *rows, const uint32_t *row_range, size_t n_rows, uint32_t n_ranges,
                                 int32_t merge_distance, int reverse_complement, char **text, size_t *len);

/* ---- host-side ingest helpers (paf.rs, partition.rs parsers) -------------- */
/* parse_cigar_to_delta (impg.rs:2935-2950): returns #ops or <0 */
long impg_gpu_parse_cigar(const char *cigar, size_t len, uint32_t *ops_out, size_t cap);
/* parse_target_range (partition.rs:1752-1763) */
/* parse_subsequence_coordinates (main.rs:4642-4659): "base:START-END" -> 1, base name and START;
 * 0 when the name carries no parsable coordinates.  Host-only. */
int impg_gpu_parse_subsequence(const char *seq_name, char *base_out, size_t base_cap, int32_t *start_offset);
int impg_gpu_parse_target_range(const char *s, char *name_out, size_t name_cap,
                                int32_t *start, int32_t *end);

/* ---- multi-GPU: the index sharded by target sequence over the GPUs of one node ---------
 * Entries live with the rank that owns their target (targets bin-packed by entry count, heaviest first onto the
 * least loaded shard: impg_gpu_shard_assign); a record's ops are stored with its forward entry's owner and with its
 * reversed entry's owner.  Every query lives with its HOME rank -- visited sets, worklists and result order, the
 * sequential state of impg.rs:2471-2560 -- and each hop of the walk sends the frontier records to the owners of
 * their targets (all-to-all-v of 16-byte records) and brings the hits home (16- or 32-byte records), where they are
 * put back into frontier order x visit order before the visited-set update.  The whole loop runs inside this
 * library; the reference has no counterpart (its MultiImpg, multi_impg.rs:495-595, queries per-file indices
 * serially on one host).  Two ways to bring the ranks up:
 *
 *  (1) one process, n_dev GPUs: impg_gpu_index_create_multi / _from_paf_multi return ONE handle.  Every query
 *      entry point above works on it unchanged -- a Rust `impl ImpgIndex` gets the whole node for free.  The ranks
 *      are host threads; exchanges are direct peer copies over xGMI (hipMemcpyPeerAsync).  The batch's ranges are
 *      dealt to the ranks in contiguous blocks; results come back in the caller's order.
 *  (2) one process per GPU (torch.distributed.run / mpirun layout): every rank makes a communicator
 *      (impg_gpu_comm_create_rccl: RCCL send/recv groups over xGMI; rank 0 makes the ids with
 *      impg_gpu_comm_unique_id and the launcher carries them to the others -- or impg_gpu_comm_create_host: the
 *      host's own transport as two callbacks), builds its shard (impg_gpu_index_create_rank / _from_paf_rank),
 *      and then the query entry points are COLLECTIVE: every rank calls the same function with the same params
 *      and ITS OWN ranges (possibly none) and gets the results of its own ranges.
 *
 * `lanes` chunks of a batch ("chunk_ranges") are in flight at once, each on its own engine, stream, host thread
 * and communicator, so one lane's exchange overlaps the other lanes' kernels.
 * impg_gpu_index_save works on a shard and on a multi handle (see there); store_cigar, the
 * device-side BED call and tracepoint indexes work there as on one GPU (the ops follow the hits home).  projected / pairs /
 * stage times of a rank (2) count the work done ON THAT RANK's shard; a multi handle (1) reports the sum of
 * the work and the slowest rank's times. */
typedef struct impg_gpu_comm impg_gpu_comm_t;
#define IMPG_COMM_ID_BYTES 128 /* sizeof(ncclUniqueId) */
/* ids[lanes * IMPG_COMM_ID_BYTES]: one RCCL unique id per lane, made on one rank */
int impg_gpu_comm_unique_id(uint8_t *ids, int lanes);
int impg_gpu_comm_create_rccl(const uint8_t *ids, int lanes, int rank, int world, int device, impg_gpu_comm_t **out);
/* The host's transport.  Both callbacks move HOST memory and return 0 on success; they are called from the lane's
 * own thread (one transport per lane: collectives of different lanes must not share an ordering domain).
 *   allgather_u64: all[r * k + i] = value i of rank r.
 *   alltoallv: bytes [send_off[d], +send_bytes[d]) of `send` go to rank d; bytes from rank s land at recv_off[s]. */
typedef struct {
  void *ctx;
  int (*allgather_u64)(void *ctx, const uint64_t *mine, size_t k, uint64_t *all);
  int (*alltoallv)(void *ctx, const void *send, const uint64_t *send_off, const uint64_t *send_bytes, void *recv,
                   const uint64_t *recv_off, const uint64_t *recv_bytes);
} impg_gpu_host_transport_t;
int impg_gpu_comm_create_host(const impg_gpu_host_transport_t *transports /* [lanes] */, int lanes, int rank, int world,
                              int device, impg_gpu_comm_t **out);
void impg_gpu_comm_destroy(impg_gpu_comm_t *); /* after the indexes that use it */
int impg_gpu_comm_info(const impg_gpu_comm_t *, int *rank, int *world, int *lanes, const char **kind /* "rccl", "host", ... */);
/* Collective self-check of one lane's transport before any index is built on it: an all-gather of known words and,
 * for a host transport, a ragged all-to-all-v of a known pattern over host memory (needs no GPU).
 * IMPG_E_IO if anything arrives wrong. */
int impg_gpu_comm_check(impg_gpu_comm_t *, int lane);
/* (2): this rank's shard.  Every rank passes the SAME records (each keeps what its targets need). */
int impg_gpu_index_create_rank(const impg_gpu_record_t *records, size_t n_records, const uint32_t *cigar_ops, size_t n_ops,
                               const int64_t *seq_len, uint32_t n_seq, const uint64_t *file_first_record /* may be NULL */,
                               uint32_t n_files, int bidirectional, int order_policy, int device, impg_gpu_comm_t *comm,
                               impg_gpu_index_t **out);
int impg_gpu_index_create_from_paf_rank(const char *const *paths, int n_paths, int bidirectional, int order_policy,
                                        int device, impg_gpu_comm_t *comm, impg_gpu_index_t **out);
/* (1): one handle over n_dev GPUs of this process (a device may be listed more than once: its shards share it). */
int impg_gpu_index_create_multi(const impg_gpu_record_t *records, size_t n_records, const uint32_t *cigar_ops, size_t n_ops,
                                const int64_t *seq_len, uint32_t n_seq, const uint64_t *file_first_record /* may be NULL */,
                                uint32_t n_files, int bidirectional, int order_policy, const int *devices, int n_dev,
                                int lanes, impg_gpu_index_t **out);
int impg_gpu_index_create_from_paf_multi(const char *const *paths, int n_paths, int bidirectional, int order_policy,
                                         const int *devices, int n_dev, int lanes, impg_gpu_index_t **out);
/* What impg_gpu_index_save wrote for a rank's shard / for a multi handle, back in HBM without the alignment files.
 * load_rank: collective in the sense that every rank loads its own file before the first query; the file's world and
 * rank must be the communicator's.  load_multi: n_dev must be the number of GPUs the handle was saved over. */
int impg_gpu_index_load_rank(const char *path, int device, impg_gpu_comm_t *comm, impg_gpu_index_t **out);
int impg_gpu_index_load_multi(const char *path, const int *devices, int n_dev, int lanes, impg_gpu_index_t **out);
/* The shard map: owner_out[t] = shard of target t given its entry count (host-only, deterministic). */
int impg_gpu_shard_assign(const uint64_t *entries_per_target, uint32_t n_seq, uint32_t n_shards, uint32_t *owner_out);
/* rank (-1 for a multi handle), world, lanes and the shard map of an index (1 / 0 for a plain one) */
int impg_gpu_index_shard_info(const impg_gpu_index_t *, int *rank, int *world, int *lanes, uint32_t *owner_out, size_t cap);
/* Where the hops of the queries since the last reset spent their wall time, by hop number within a batch (hop 8 and
 * later are counted with hop 8), summed over the lanes: out[(shard * 8 + hop) * 12 + field] with fields
 *   0 hops, then seconds: 1 bucketing the frontier by owner, 2 all-gather of the sizes (incl. the wait for the slowest
 *   rank), 3 frontier records to the owners, 4 the owner's lookup + projection (+ packing the hits), 5 all-gather of
 *   the hit counts, 6 hits (and CIGAR ops) home, 7 putting them back in frontier order; then 8 bytes of frontier
 *   records sent, 9 bytes of hits + ops sent, 10 frontier records received, 11 hits that came home.
 * One shard for a rank's index, n_dev for a multi handle, none for a plain index.  *n_out = doubles written (or
 * needed when out is NULL). */
int impg_gpu_index_hop_profile(impg_gpu_index_t *, double *out, size_t cap, int reset, size_t *n_out);

/* ---- partition: partition_alignments with BED output (src/commands/partition.rs:158-712) --------------------------
 * The loop is sequential -- window k+1 is queried under the mask window k left -- so what lies between two queries is
 * kept where the query's rows are: a REGIONS object holds masked_regions and missing_regions of every sequence as two
 * CSR tables (u32 offsets over the sequence ids, (start, end) pairs), in HBM (on_host = 0) or on the host (on_host = 1:
 * the host twin, the same algebra in plain C++, which needs no GPU).  One window's update is
 *   merge_overlaps(merge_distance) (:939-976), extend_to_close_boundaries (:1369-1408, if min_boundary_distance > 0),
 *   mask_and_update_regions (:978-1366), merge_overlaps(0)
 * on the query-side interval (query_id, min, max) of every row; only those reach BED output, so the target side's
 * proportional adjustments (:1120-1140, :1178-1188) are not built.  State at the start: masked = {}, missing =
 * {(0, len)} for every sequence (a sequence of length 0 starts outside the missing map: it could never be windowed). */
typedef struct impg_gpu_regions impg_gpu_regions_t;
typedef struct impg_gpu_partition impg_gpu_partition_t;
typedef struct {
  uint32_t seq_id;
  int32_t start, end;
} impg_gpu_partition_row_t;
#define IMPG_REGIONS_MASKED 0
#define IMPG_REGIONS_MISSING 1
#define IMPG_SELECT_LONGEST 0   /* the longest missing range; ties: higher sequence id, then the later range */
#define IMPG_SELECT_TOTAL 1     /* the sequence with most missing bases; ties: higher sequence id */
#define IMPG_SELECT_SAMPLE 2    /* "sample[,sep]": the name prefix (first field) with most missing bases, ties by prefix */
#define IMPG_SELECT_HAPLOTYPE 3 /* "haplotype[,sep]": the first two fields */
/* on_host = 0 needs `device`; on_host = 1 ignores it. */
int impg_gpu_regions_create(const int64_t *seq_len, uint32_t n_seq, int on_host, int device, impg_gpu_regions_t **out);
/* One window's update on caller-supplied rows in host memory (device state: the rows are uploaded and the kernels run).
 * Writes at most cap rows -- sorted by (seq_id, start), disjoint -- and the count to *n_out.  The output of a window
 * cannot be bounded ahead of the call and the state has moved on when it returns, so the object keeps the rows until its
 * next apply / window: a count above cap is fetched whole with impg_gpu_regions_last_rows.  merge_distance < 0:
 * IMPG_E_INVALID. */
int impg_gpu_regions_apply(impg_gpu_regions_t *, const impg_gpu_interval_t *rows, size_t n_rows, int32_t merge_distance,
                           int32_t min_missing_size, int32_t min_boundary_distance, impg_gpu_partition_row_t *out_rows, size_t cap,
                           size_t *n_out);
/* The same on rows that already lie in the object's device's memory, as a session's window applies its query's rows
 * (device state only; whatever wrote the rows has completed).  Nothing reads them on the host: a row with a sequence id
 * >= n_seq or a negative coordinate is found by the kernels, the call returns IMPG_E_INVALID and the state -- both
 * tables and everything select answers from -- is what it was before the call. */
int impg_gpu_regions_apply_device(impg_gpu_regions_t *, const impg_gpu_interval_t *d_rows, size_t n_rows, int32_t merge_distance,
                                  int32_t min_missing_size, int32_t min_boundary_distance, impg_gpu_partition_row_t *out_rows,
                                  size_t cap, size_t *n_out);
int impg_gpu_regions_last_rows(const impg_gpu_regions_t *, impg_gpu_partition_row_t *out_rows, size_t cap, size_t *n_out);
/* which = IMPG_REGIONS_MASKED / _MISSING: off_out[n_seq + 1], and the first min(cap, total) ranges as (start, end)
 * pairs; *n_ranges = total.  ranges_out may be NULL with cap 0 to size. */
int impg_gpu_regions_get(impg_gpu_regions_t *, int which, uint64_t *off_out, int32_t *ranges_out, size_t cap, size_t *n_ranges);
/* select_and_window_sequences (:715-937) on the current missing map.  names[n_seq] is needed by SAMPLE / HAPLOTYPE only
 * (separator NULL = "#").  Inside the chosen group the reference orders the sequences by length with an unstable sort:
 * ties go in ascending sequence id here.  *n = windows found (0: nothing is missing any more); at most cap are written. */
int impg_gpu_regions_select(impg_gpu_regions_t *, int selection, const char *separator, const char *const *names,
                            int64_t window_size, impg_gpu_range_t *windows_out, size_t cap, size_t *n);
void impg_gpu_regions_free(impg_gpu_regions_t *);

/* Host-only pieces of the command (no device needed): the windows of a starting-sequences list (:220-246: a short tail
 * window is merged into the previous window OF THE SAME SEQUENCE), rehome_singleton_slivers (:45-156) over rows tagged
 * with their partition's position in the list (partition_idx ascending; the rebuilt order comes back in place, *n_out
 * rows), and write_single_partition_file's text (:1682-1717; *text is malloc'ed). */
int impg_gpu_partition_starting_windows(const uint32_t *seq_ids, size_t n, const int64_t *seq_len, uint32_t n_seq,
                                        int64_t window_size, impg_gpu_range_t *windows_out, size_t cap, size_t *n_out);
int impg_gpu_partition_rehome(impg_gpu_partition_row_t *rows, uint64_t *partition_num, size_t n);
int impg_gpu_partition_bed_text(const impg_gpu_partition_row_t *rows, const uint64_t *partition_num, size_t n,
                                const char *const *names, uint32_t n_seq, char **text, size_t *len);

/* The session: partition_alignments over an index.  state_on_host = 0: the regions live in HBM for the session's life, the
 * query reads the mask table where the kernels maintain it (no host validation, no upload), the query's rows are
 * consumed where the engine leaves them, and per window only the output rows and a few words cross PCIe; the session
 * holds one engine of the index until it is destroyed (IMPG_E_UNSUPPORTED from create when every engine is out -- it
 * never waits).  state_on_host = 1: the loop a host binding writes against the calls above -- mask rebuilt and uploaded
 * every window, rows copied back, algebra on the CPU; holds no engine.  params: a transitive query (BFS or DFS) with
 * store_cigar 0 and min_output_length < 0 (IMPG_E_INVALID otherwise); merge_distance < 0 (--no-merge): IMPG_E_INVALID;
 * a sharded index: IMPG_E_UNSUPPORTED. */
typedef struct {
  int64_t window_size;
  int32_t merge_distance;
  int32_t min_missing_size;      /* reference default 3000 */
  int32_t min_boundary_distance; /* reference default 3000 */
  int32_t selection;             /* IMPG_SELECT_* */
  const char *separator;         /* SAMPLE / HAPLOTYPE; NULL = "#" */
  int32_t rehome_singletons;     /* reference default 1 */
  int32_t state_on_host;
} impg_gpu_partition_opts_t;
int impg_gpu_partition_create(impg_gpu_index_t *, const impg_gpu_params_t *params, const impg_gpu_partition_opts_t *opts,
                              const uint32_t *starting_seq_ids, size_t n_starting, impg_gpu_partition_t **out);
/* The next set of windows (:183-247 first if starting sequences were given, else :715-937); *n = 0: done.  A set larger
 * than cap is not handed out: *n says how many there are. */
int impg_gpu_partition_next_windows(impg_gpu_partition_t *, impg_gpu_range_t *windows_out, size_t cap, size_t *n);
/* Query + update for one window.  *n_out = 0: no partition.  At most cap rows are written; a larger result stays with the
 * session until its next window: impg_gpu_regions_last_rows(impg_gpu_partition_regions(p), ...) fetches it whole. */
int impg_gpu_partition_window(impg_gpu_partition_t *, const impg_gpu_range_t *window, impg_gpu_partition_row_t *rows_out, size_t cap,
                              size_t *n_out);
/* The whole loop, rehoming and text.  text != NULL: the partitions.bed text is returned (malloc'ed) instead of written;
 * else folder/partitions.bed, or folder/partition{N}.bed with separate_files (:1509-1542; no rehoming then, as in the
 * reference); folder NULL = the working directory. */
int impg_gpu_partition_run(impg_gpu_partition_t *, const char *folder, int separate_files, char **text, size_t *len,
                           uint64_t *n_partitions);
/* ---- partition FASTA: `impg partition -o fasta --separate-files` (partition.rs:498-508, :1630-1680) ----------------
 * One file per partition, folder/partition{N}.fasta, N as impg_gpu_partition_run numbers the same window under
 * separate_files (a window that leaves no interval writes no file and takes no number; no rehoming).  A file holds one
 * record per interval of its window, in the order impg_gpu_partition_window returns them: ">{name}:{start}-{end}\n" and
 * bases [start, end) of the sequence as the attached store holds them, in lines of 80, each followed by '\n'.  A record
 * of NO bases is its header line alone -- impg_gpu_query_batch_fasta prints an empty line there, the partition writer
 * (chunks(80) of nothing) prints nothing.  Every interval is forward: there is no reverse_complement argument.  Names as
 * the index has them, ids where it has none.  An interval on a sequence the store lacks, or one that leaves its sequence:
 * IMPG_E_INVALID with impg_gpu_query_batch_fasta's messages, before any byte of that window's text is written.
 * state_on_host = 0: the records are written ON THE DEVICE from the window's intervals where the update leaves them in
 * HBM (no interval goes to the host for the text's sake) and the store in HBM, in either of its forms, and come to the
 * host in pieces of exactly "bed_text_piece_bytes" bytes cut wherever that falls -- no record is refused for its length,
 * unlike impg_gpu_query_batch_fasta's.  The session owns ONE text stream -- the name tables, two piece buffers in HBM,
 * two pinned ones and two events -- made at its first FASTA window and freed with it.  state_on_host = 1: the host
 * twin prints the same bytes from the store's host copy.  Sharded handles and tracepoint indexes take no store and are
 * refused where they already are (impg_gpu_partition_create, impg_gpu_index_set_sequences).
 *
 * impg_gpu_partition_run_fasta: the whole loop.  Before the first window: IMPG_E_INVALID if the index has no store, or
 * if a sequence of non-zero length is absent from it (the message names the first one: every sequence is partitioned
 * eventually) -- the session has then run no window and its tables are untouched.  folder NULL = the working directory.
 * impg_gpu_partition_window_fasta: query, update and text for one window; the text goes to fd, or is returned malloc'ed
 * when text != NULL (fd is then ignored).  *n_rows = 0: no partition and no text.  After a refusal of a record there is
 * no text, but the state HAS moved on, as the reference's would have: the window's rows stay with the session
 * (impg_gpu_regions_last_rows). */
int impg_gpu_partition_run_fasta(impg_gpu_partition_t *, const char *folder, uint64_t *n_partitions);
int impg_gpu_partition_window_fasta(impg_gpu_partition_t *, const impg_gpu_range_t *window, int fd, char **text, size_t *len, size_t *n_rows);
/* The partition writer over the caller's rows (start <= end), printed in the order given: on_host = 0 uploads them and
 * runs the device route on an engine leased for the call, on_host = 1 the host twin.  *text is malloc'ed. */
int impg_gpu_partition_rows_fasta(impg_gpu_index_t *, const impg_gpu_partition_row_t *rows, size_t n, int on_host, char **text, size_t *len);
/* Host-only (no device needed), the sibling of impg_gpu_fasta_text: names_of_ids[id] = the name of sequence id. */
int impg_gpu_partition_fasta_text(const impg_gpu_sequences_t *seqs, const char *const *names_of_ids, size_t n_ids,
                                  const impg_gpu_partition_row_t *rows, size_t n, char **text, size_t *len);
impg_gpu_regions_t *impg_gpu_partition_regions(impg_gpu_partition_t *); /* borrowed */
/* "windows", "partitions", "mask_uploads" (host-to-device copies of mask tables) and "rows_to_host" (query rows copied
 * back): both read off the index's own counters, which are bumped where those copies are issued, as deltas around
 * the session's windows (queries other threads run on the handle meanwhile are counted in), "walk_windows" (windows the per-query walk answered), "step_launches" (kernel launches + rocPRIM calls of the
 * updates; a library sort or scan is several kernels and counts once); of the FASTA calls: "fasta_windows" (windows
 * printed on the device), "fasta_host_windows" (by the host twin), "text_buffer_allocs" (times the text stream's
 * buffers were allocated or grown) and "text_table_uploads" (times its name tables were uploaded).  The index's
 * "fasta_records" / "fasta_text_pieces" / "fasta_text_bytes" count the partition route's records, pieces and bytes on
 * top of what they hold (the host twin has no pieces); the partition calls never reset them. */
int impg_gpu_partition_counter(const impg_gpu_partition_t *, const char *key, int64_t *value);
void impg_gpu_partition_destroy(impg_gpu_partition_t *);

/* ---- refine: the boundary support of `impg refine` (src/commands/refine.rs:665-850) --------------------------------------
 * The reference evaluates a grid of flank extensions per locus, each a query followed by a per-sequence fold over the
 * query's rows.  What is built here is that fold as a batch primitive: the rows of n_cand candidate regions in one call,
 * rows[offsets[c] .. offsets[c + 1]) those of candidate c in the reference's emission order (what impg_gpu_query_batch
 * returns, self interval included; a row with query_id 0xFFFFFFFF is a hole of IMPG_ROWS_ORDERED_SLOTS and is skipped),
 * cand[c] = its target and the clamped region (start, end).  Per candidate (compute_support_sets, :665-783):
 *   a candidate of at most one row supports nothing (:680-682); rows whose query is the candidate's target are dropped;
 *   the others are grouped by query sequence -- the row's target_id is NOT looked at, as in the reference --, a group is
 *   sorted stably by (q_start, q_end) and folded by merge_intervals / should_merge (:799-850; merge_distance < 0: no
 *   merge); a merged interval covers when t_start <= start, t_end >= end, t_end >= start + effective_span and t_start <=
 *   end - effective_span, effective_span = min(max(end - start, 0), max(span_bp, 0)); a group's hull is the min / max
 *   query coordinate of its covering intervals; a group is dropped when a blacklisted range of its sequence shares a
 *   position with [q_lo, q_hi], both ends inclusive on both sides (coitrees' query(first, last), :736-748); every other
 *   group with a hull is a SURVIVOR (seq_id, q_lo, q_hi), and count[c] = the number of distinct entities among the
 *   survivors, min'ed with max_entities[c] where given.
 * entity_of[n_seq] maps a sequence to its entity (PanSN keys are strings and stay with the caller; impg_gpu_entity_ids
 * makes the ids); 0xFFFFFFFF = the sequence has no key: it is a survivor and counts nothing (:750-757).  NULL = every
 * sequence its own entity (level `sequence`).  The blacklist is a CSR table over the sequence ids, blacklist_off[n_seq + 1]
 * and (start, end) pairs in any order (end < start: IMPG_E_INVALID); NULL = none.
 * The one place the output is a SUPERSET of the reference's: the reference stops walking its hash map when the count
 * reaches max_entities (:758-763), so the survivors it prints then depend on hash order; here every survivor is returned
 * and only the count is clamped.
 * on_host = 1: the host twin, plain C++, no GPU.  on_host = 0: the rows are uploaded to `device` and the kernels of
 * refine_device.hip run; each (candidate, sequence) group is folded by one lane -- the fold is order-dependent, not a
 * scan -- so one very long group makes one lane run long (*longest_group_out = the rows of the longest group folded).
 * A row whose query_id is neither a hole nor < n_seq: IMPG_E_INVALID (on the device after the kernels have run; the row
 * is dropped before anything indexes with it).  count_out[n_cand]; survivor_offsets_out[n_cand + 1] and *survivors_out
 * (malloc'ed; free() it), ascending seq_id inside a candidate, both NULL when not wanted. */
typedef struct {
  int32_t span_bp;        /* reference default 1000 */
  int32_t merge_distance; /* < 0 = --no-merge */
} impg_gpu_support_opts_t;
typedef struct {
  uint32_t seq_id;
  int32_t q_lo, q_hi;
} impg_gpu_survivor_t;
int impg_gpu_support_rows(const impg_gpu_interval_t *rows, const uint64_t *offsets, const impg_gpu_range_t *cand, size_t n_cand,
                          uint32_t n_seq, const uint32_t *entity_of, const uint32_t *max_entities, const uint32_t *blacklist_off,
                          const int32_t *blacklist_ranges, const impg_gpu_support_opts_t *opts, int on_host, int device,
                          uint32_t *count_out, uint64_t *survivor_offsets_out, impg_gpu_survivor_t **survivors_out,
                          uint64_t *longest_group_out);
/* Entity ids of PanSN names "sample<sep>haplotype<sep>contig" for level = IMPG_SELECT_SAMPLE (the first field) or
 * IMPG_SELECT_HAPLOTYPE (the first two fields, separator included), numbered as the keys are first seen; separator NULL =
 * "#".  UNPINNED: what sweepga's extract_pansn_key returns for a name with too few fields could not be checked; here a
 * name that does not contain the separator has no key (0xFFFFFFFF) at either level, and "a<sep>b" has both.
 * Host-only: needs no device. */
int impg_gpu_entity_ids(const char *const *names, size_t n, int level, const char *separator, uint32_t *entity_out,
                        uint32_t *n_entities_out);

/* The search: run_refine (refine.rs:81-409) for n loci (target_id, start, end), end > start.  A candidate (left, right)
 * of a locus is the region start = max(s - left, 0), end = min(e + right, len(target)) -- none if end <= start -- with
 * left_extension = s - start and right_extension = end - e, the clamped values (:426-467).  flanks = build_flanks(
 * max_extension_bp, extension_step) (:852-876), max_extension_bp = ceil(locus length x max_extension) for max_extension
 * <= 1, else ceil(max_extension) (:177-185).  Pass 0 evaluates (0, 0): original_support_count.  Unless the best has reached
 * the locus's max_entities, pass 1 evaluates (l, 0) for l > 0, pass 2 (left_best, r) for every r, pass 3 (l, right_best) for
 * every l, each stopping the locus when the maximum is reached; inside a pass the candidates are reduced in flank order and
 * one replaces the best only when compare_candidates is strictly Greater (:548-582: more support, then smaller left + right,
 * then smaller max(left, right), then shorter), and so does the pass's winner against the running best.
 * The reference runs a query per candidate; here the live candidates of ALL loci of a pass are ONE batch, so a run is at most
 * four batches plus one small batch that reads the winners' survivors, whatever n is (counter "refine_passes").
 * impg_gpu_refine: the rows are the index's.  Plain and BFS queries on a CIGAR or tracepoint index leave their rows in HBM
 * (IMPG_ROWS_ORDERED_SLOTS; a batch may come back as several parts -- "chunk_ranges", "pair_budget" -- and the support runs
 * part by part: counter "refine_parts") and only count[] comes home.  DFS and MultiImpg params, which
 * impg_gpu_query_batch_device does not offer, and support_on_host = 1 go through impg_gpu_query_batch_filtered: the rows
 * cross PCIe ("refine_rows_to_host" counts them) and the support runs on them with the kernels, or with the host twin under
 * support_on_host.  "refine_candidates" = candidates evaluated, "refine_longest_group" = the longest (candidate, sequence)
 * group a lane folded.  use_max_entities = 1 (levels sample and haplotype): compute_max_entities (:589-632) per distinct
 * target from the index's entries -- distinct entity_of[] over the target's entries, without entries of the target itself,
 * of sequences subset_keep drops, of sequences without a key, and without the target's own key; the blacklist is not applied.
 * subset_keep as in impg_gpu_query_batch_filtered; entity_of / blacklist as in impg_gpu_support_rows.
 * impg_gpu_refine_rows: the same search over the caller's own row source -- `query` is handed every pass's candidate regions
 * and returns their rows, grouped by region in emission order with offsets[n + 1], valid until its next call; non-zero =
 * IMPG_E_CANCELLED -- with seq_len[n_seq] for the clamp and max_entities[n] per locus (NULL: none).  With support_on_host = 1
 * it needs no GPU; else the rows are uploaded to `device`.
 * Refused: a sharded index (IMPG_E_UNSUPPORTED); store_cigar or min_output_length >= 0 (IMPG_E_INVALID: refine passes
 * neither, :497-502); span_bp < 0, max_extension < 0 or NaN, extension_step <= 0 (RefineOpts::validate, main.rs:4454-4473);
 * a locus with end <= start, an unknown target, or no candidate at all (:153-168, :374-382): IMPG_E_INVALID. */
typedef struct {
  int32_t span_bp;        /* reference default 1000 */
  double max_extension;   /* 0.5 */
  int32_t extension_step; /* 1000 */
  int32_t merge_distance;
  int32_t use_max_entities;
  int32_t support_on_host;
} impg_gpu_refine_opts_t;
typedef struct { /* RefineRecord (refine.rs:41-53) without its strings */
  uint32_t target_id;
  int32_t refined_start, refined_end;
  int32_t original_start, original_end;
  int32_t left_extension, right_extension;
  uint32_t support_count, original_support_count;
} impg_gpu_refine_record_t;
typedef struct impg_gpu_refine_run impg_gpu_refine_t;
typedef int (*impg_gpu_rows_cb)(void *ctx, const impg_gpu_range_t *regions, size_t n, const impg_gpu_interval_t **rows,
                                const uint64_t **offsets);
int impg_gpu_refine(impg_gpu_index_t *, const impg_gpu_range_t *loci, size_t n, const impg_gpu_params_t *params,
                    const impg_gpu_refine_opts_t *opts, const uint32_t *entity_of, const uint8_t *subset_keep,
                    const uint32_t *blacklist_off, const int32_t *blacklist_ranges, impg_gpu_refine_t **out);
int impg_gpu_refine_rows(impg_gpu_rows_cb query, void *ctx, const int64_t *seq_len, uint32_t n_seq, const impg_gpu_range_t *loci,
                         size_t n, const impg_gpu_refine_opts_t *opts, const uint32_t *entity_of, const uint32_t *max_entities,
                         const uint32_t *blacklist_off, const int32_t *blacklist_ranges, int device, impg_gpu_refine_t **out);
size_t impg_gpu_refine_num_records(const impg_gpu_refine_t *);
const impg_gpu_refine_record_t *impg_gpu_refine_records(const impg_gpu_refine_t *);
/* The survivors of the winners (support_entities), read at the end by evaluating the n winning candidates once more:
 * offsets[n + 1] into survivors[], ascending seq_id inside a record; owned by the object. */
const uint64_t *impg_gpu_refine_survivor_offsets(const impg_gpu_refine_t *);
const impg_gpu_survivor_t *impg_gpu_refine_survivors(const impg_gpu_refine_t *);
/* passes (batches) of the run, candidates evaluated and parts the batches came back as: any may be NULL */
void impg_gpu_refine_stats(const impg_gpu_refine_t *, uint64_t *passes, uint64_t *candidates, uint64_t *parts);
/* impg_gpu_refine only: four doubles per batch of the run, the passes in order and then the read of the winners' survivors --
 * candidates in the batch, wall seconds of the query call, HIP-event milliseconds of the engine inside it (stage clocks +
 * row placement; on the routes through the host: the engine's wall milliseconds), wall seconds of the support (upload or
 * kernels, its copies home).  *n_out = doubles there are; at most cap are written. */
int impg_gpu_refine_batch_times(const impg_gpu_refine_t *, double *out, size_t cap, size_t *n_out);
/* The two texts of main.rs:7817-7861: the table -- a header line, then chrom, refined start, refined end, name, original
 * support, new support, left, right -- and the --support-output file: sequence, start, end, name per survivor, sorted by
 * sequence name.  names[n_seq] are the sequence names; labels[i] (labels or an entry may be NULL = "") is the locus's label:
 * blank or "." becomes chrom:start-end of the original locus.  Both malloc'ed (free() them); support_text may be NULL. */
int impg_gpu_refine_text(const impg_gpu_refine_t *, const char *const *names, uint32_t n_seq, const char *const *labels, char **text,
                         size_t *len, char **support_text, size_t *support_len);
void impg_gpu_refine_free(impg_gpu_refine_t *);

/* ---- synthetic workload generators (SplitMix64) ----- */
/* Fills records / ops for `n_records` synthetic alignments (200-op CIGARs by
 * default).  Call with ops == NULL to size: *n_ops_out receives the op count. */
int impg_synth_paf(uint64_t seed, size_t n_records, uint32_t n_seq, int32_t seq_len,
                   int32_t target_span, uint32_t n_blocks, impg_gpu_record_t *records,
                   uint32_t *ops, size_t ops_cap, size_t *n_ops_out);
/* Writes the same alignments as PAF text (PanSN names gNNN#H#chr1). */
int impg_synth_paf_text(uint64_t seed, size_t n_records, uint32_t n_seq, int32_t seq_len,
                        int32_t target_span, uint32_t n_blocks, const char *path);
int impg_synth_seq_name(uint32_t id, char *out, size_t cap);
/* The non-uniform workload of `bench.py --workload skewed` as PAF text: log-normal target spans (1 kb ... the sequence,
 * median 8 kb: 20 ... 10^5 ops a CIGAR) and 1 % of the sequences (the first max(1, n_seq / 100)) chosen as target / as query with
 * probability 0.3 each, i.e. holding ~30 % of a bidirectional index's entries.  Same names and record format as
 * impg_synth_paf_text; *n_ops_out = CIGAR ops written. */
int impg_synth_skewed_paf_text(uint64_t seed, size_t n_records, uint32_t n_seq, int32_t seq_len, const char *path, uint64_t *n_ops_out);
int impg_synth_bed(uint64_t seed, size_t n, uint32_t n_seq, int32_t seq_len, int32_t range_len,
                   impg_gpu_range_t *out);
/* Diagnostics: the engine's own sort of a level's lookup order (impg_amd/csrc/kernels.hip, order_scatter_kernel -- the place
 * of the reference's per-tree query order, which the engine is free to choose: interval_tree lookups commute) run on `n`
 * pseudo-random keys of `end_bit` bits on `device` and checked on the host: a permutation, keys non-decreasing, equal keys
 * in index order.  IMPG_OK or IMPG_E_INVALID with the first offending place in impg_gpu_last_error(). */
int impg_gpu_selftest_order_sort(int device, uint32_t n, unsigned end_bit, uint64_t seed);
/* Diagnostics: the device primitives under every stage on arrays the caller brings (impg_amd/csrc/prims_selftest.hip).  Each
 * returns the device's raw answer and compares nothing, but for the scan's guards.
 *
 * impg_gpu_selftest_scan: the exclusive scan of in[n] (n > 0).  which = 0: launch_exclusive_scan as the engine's scans call
 * it (scratch of scan_scratch_bytes(n), a stream of its own, one synchronisation); which = 1: launch_small_scan, the
 * small-batch path's single block (n <= 1024; its total is 32-bit).  The device copies of in and out start in_shift /
 * out_shift words (0 .. 4) behind a 256-byte boundary: which = 0 runs the single-pass look-back kernel when both are
 * 16-byte aligned and the three kernels otherwise.  out[n]: the offsets written (the low 32 bits of the 64-bit prefixes),
 * *total: the sum.  info[5] = {the form that ran -- 0 look-back, 1 three kernels, 2 the small scan --, the low four bits of
 * in's device address, of out's, the look-back tile, the three-kernel tile (items)}.  64 words of 0xA5A5A5A5 stand in front
 * of out, behind out and behind the scratch: IMPG_E_INVALID, naming the guard, if one of them changed.
 *
 * impg_gpu_selftest_offsets: prims::offsets_and_total on len[n] (n > 0) -- off[n] = the exclusive sums in 64 bits, *total
 * their total; with_host_copy: through the form that brings the offsets home itself (it reads the total from that copy).
 *
 * impg_gpu_selftest_key_sort: prims::KeySort::run, the stable sort by 1 .. 3 keys, least significant first.  A pass's keys
 * (n_keys of 32 or, wide, 64 bits) stand at the rows' own indices, only their low `bits` bits count; perm[m] lists the rows
 * to sort (each < n_keys; first_in_order: the identity with m = n_keys, the first pass then sorts in place).  order[m] = the
 * sorted permutation, ties in incoming order; sorted_keys[m] (of the last pass's width) = the last pass's keys in that order.
 * The keys are copied: the caller's arrays stay as they are. */
typedef struct {
  const void *keys;
  int wide;
  unsigned bits;
} impg_gpu_sort_pass_t;
int impg_gpu_selftest_scan(int device, int which, const uint32_t *in, uint32_t n, uint32_t in_shift, uint32_t out_shift, uint32_t *out,
                           uint64_t *total, uint32_t *info);
int impg_gpu_selftest_offsets(int device, const uint32_t *len, uint32_t n, int with_host_copy, uint64_t *off, uint64_t *total);
int impg_gpu_selftest_key_sort(int device, uint32_t n_keys, const uint32_t *perm, uint32_t m, int first_in_order,
                               const impg_gpu_sort_pass_t *passes, uint32_t n_passes, uint32_t *order, void *sorted_keys);
/* Diagnostics: the device BED merges and text of impg_gpu_query_batch_bed (impg_amd/csrc/bed_device.hip) on rows the
 * caller brings instead of a query's.  rows[i] belongs to range row_range[i] < n_ranges; array order within a range is
 * the emission order the reference's tie rules refer to, rows of different ranges may interleave.  n_seq: the id
 * universe of rows[].query_id / target_id -- it may exceed the handle's; an id the handle has no name for prints as a
 * decimal.  The handle (single-GPU) gives the device, an engine and the sequence names.  range_names: n_ranges strings,
 * or NULL / a NULL entry = the range's index in decimal.  merged_out: the merged rows in output order (grouped by
 * range), text: what they print, NUL-terminated; both malloc'ed, free() them.  gap_rows_out / gap_range_out / n_gap
 * (all three or all NULL): the rows between the two merges with their ranges, in the order the second merge meets them
 * -- a chain of merge_adjusted_intervals_gap_2d stands where its first row stood; malloc'ed.  IMPG_E_INVALID: an id >= n_seq, a range
 * index >= n_ranges, a sharded or multi-GPU handle; IMPG_E_UNSUPPORTED as impg_gpu_query_batch_bed (a row longer than
 * the text buffer; bits(n_ranges) + 2 * bits(n_seq) + 1 > 64, the merges' sort key -- not with merge_distance < 0 and
 * merge_strands = 0, where nothing merges and no key holds a sequence id: n_seq may then be 2^32). */
typedef struct {
  uint32_t range, query_id;
  int32_t start, end; /* printed as u32 */
  uint32_t strand;    /* 0 '+', 1 '-' */
} impg_gpu_bed_row_t;
/* Diagnostics: the device BEDPE merge and text of impg_gpu_query_batch_bedpe (impg_amd/csrc/bedpe_device.hip) on rows and
 * CIGARs the caller brings instead of a query's.  rows[i] belongs to range row_range[i] < n_ranges; the rows come grouped
 * by range (row_range does not decrease), a range's first row being the one that is dropped; cigar_ops[cigar_off[i] ..
 * cigar_off[i + 1]) are row i's packed ops (cigar_off[n_rows + 1], starting at 0); sequence ids are the index's.
 * range_names: NULL, or NULL entries, print the range's index.  Errors as impg_gpu_query_batch_bedpe; IMPG_E_INVALID also
 * for arrays that break the rules above.  *text is malloc'ed; free() it.  Sets the "bedpe_*" counters. */
int impg_gpu_selftest_bedpe_rows(impg_gpu_index_t *ix, const impg_gpu_interval_t *rows, const uint32_t *row_range, size_t n_rows,
                                 uint32_t n_ranges, const uint64_t *cigar_off, const uint32_t *cigar_ops, int32_t merge_distance,
                                 int original_sequence_coordinates, const char *const *range_names, char **text, size_t *len);
/* The same for the device PAF merge and text of impg_gpu_query_batch_paf (impg_amd/csrc/paf_device.inc): same arguments, same
 * rules; errors as impg_gpu_query_batch_paf.  Sets the "paf_*" counters. */
int impg_gpu_selftest_paf_rows(impg_gpu_index_t *ix, const impg_gpu_interval_t *rows, const uint32_t *row_range, size_t n_rows,
                               uint32_t n_ranges, const uint64_t *cigar_off, const uint32_t *cigar_ops, int32_t merge_distance,
                               int original_sequence_coordinates, const char *const *range_names, char **text, size_t *len);
int impg_gpu_selftest_bed_rows(impg_gpu_index_t *ix, const impg_gpu_interval_t *rows, const uint32_t *row_range, size_t n_rows,
                               uint32_t n_ranges, uint64_t n_seq, int32_t merge_distance, int merge_strands,
                               int original_sequence_coordinates, const char *const *range_names,
                               impg_gpu_bed_row_t **merged_out, size_t *n_merged, char **text, size_t *len,
                               impg_gpu_interval_t **gap_rows_out, uint32_t **gap_range_out, size_t *n_gap);

#ifdef __cplusplus
}
#endif
#endif
