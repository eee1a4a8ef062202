"""Host-side mirror of the reference's index interface (trait ImpgIndex,
src/impg_index.rs:21-121) over the C ABI.  Method names and argument meaning
follow the trait; the batch_* methods are the fast path (one launch sequence for
many ranges)."""
import os
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import IMPG_E_UNSUPPORTED, INTERVAL_DTYPE, RANGE_DTYPE, RECORD_DTYPE, ImpgGpuError, Params, Stats, check, lib


def make_params(transitive=False, dfs=False, max_depth=2, min_transitive_len=101, min_distance_between_ranges=10,
                min_output_length=None, min_identity=None, store_cigar=False, multi_impg=False,
                original_sequence_coordinates=False, consider_strandness=False):
    """CLI defaults of src/main.rs:4259-4285."""
    return Params(int(transitive), int(dfs), max_depth, min_transitive_len, min_distance_between_ranges,
                  -1 if min_output_length is None else min_output_length,
                  math.nan if min_identity is None else float(min_identity), int(store_cigar), int(multi_impg),
                  int(original_sequence_coordinates), int(consider_strandness))


def _text_bytes(ptr, n):
    """n bytes at ptr as bytes (ctypes.string_at takes its size as a C int: a PAF text of 2 GiB or more goes the other way)"""
    return C.string_at(ptr, n) if n < (1 << 31) else bytes((C.c_char * n).from_address(ptr.value))


class QueryResults:
    """Vec<AdjustedInterval> per range, in the reference's emission order."""

    def __init__(self, handle, owner, copy=True):
        """copy=False: the arrays are views of the library's buffers (valid while this object lives); a
        transitive batch is hundreds of millions of rows, not worth duplicating."""
        self._h = handle
        self._owner = owner
        L = lib()
        self.n_ranges = L.impg_gpu_results_num_ranges(handle)
        total = L.impg_gpu_results_total(handle)
        self.total = total
        self.offsets = np.ctypeslib.as_array(C.cast(L.impg_gpu_results_offsets(handle), C.POINTER(C.c_uint64)),
                                             shape=(self.n_ranges + 1,)).copy()
        if total:
            raw = np.ctypeslib.as_array(C.cast(L.impg_gpu_results_intervals(handle), C.POINTER(C.c_uint8)),
                                        shape=(total * INTERVAL_DTYPE.itemsize,))
            self.intervals = raw.view(INTERVAL_DTYPE).copy() if copy else raw.view(INTERVAL_DTYPE)
        else:
            self.intervals = np.zeros(0, dtype=INTERVAL_DTYPE)
        self.projected = L.impg_gpu_results_projected(handle)
        self.cigar_off = self.cigar_ops = None
        cop = L.impg_gpu_results_cigar_offsets(handle)
        if cop:
            self.cigar_off = np.ctypeslib.as_array(C.cast(cop, C.POINTER(C.c_uint64)), shape=(total + 1,)).copy()
            nops = int(self.cigar_off[-1])
            self.cigar_ops = (np.ctypeslib.as_array(C.cast(L.impg_gpu_results_cigar_ops(handle), C.POINTER(C.c_uint32)),
                                                    shape=(nops,)).copy() if nops else np.zeros(0, dtype=np.uint32))

    def __getitem__(self, i):
        return self.intervals[self.offsets[i]:self.offsets[i + 1]]

    def timing(self):
        """(seconds in the engine, seconds copying back + assembling) of the call (impg_gpu_results_timing)."""
        a, b = C.c_double(0), C.c_double(0)
        lib().impg_gpu_results_timing(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def cigars(self, i):
        """Vec<CigarOp> (packed u32 ops) of every interval of range i; needs store_cigar."""
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        return [self.cigar_ops[int(self.cigar_off[k]):int(self.cigar_off[k + 1])] for k in range(a, b)]

    def __len__(self):
        return self.n_ranges

    def bed(self, range_names=None, merge_distance=0, params=None):
        """output_results_bed over every range (main.rs:11849-11892)."""
        L = lib()
        p = params or make_params()
        arr = None
        if range_names is not None:
            arr = (C.c_char_p * len(range_names))(*[None if s is None else s.encode() for s in range_names])
        text = C.c_void_p(None)
        ln = C.c_size_t(0)
        check(L.impg_gpu_results_bed(self._h, self._owner._h, arr, C.byref(p), merge_distance, C.byref(text), C.byref(ln)))
        try:
            return C.string_at(text, ln.value).decode()
        finally:
            _lib.free(text)

    def fasta(self, merge_distance=0, params=None, reverse_complement=False, raw=False):
        """output_results_fasta over every range (main.rs:12351-12415), from the host copy of the store the index
        has attached (GpuImpg.set_sequences).  raw: the text as bytes."""
        p = params or make_params()
        text = C.c_void_p(None)
        ln = C.c_size_t(0)
        check(lib().impg_gpu_results_fasta(self._h, self._owner._h, C.byref(p), merge_distance, int(bool(reverse_complement)),
                                           C.byref(text), C.byref(ln)))
        try:
            out = _text_bytes(text, ln.value)
            return out if raw else out.decode()
        finally:
            _lib.free(text)

    def paf(self, range_names=None, merge_distance=0, params=None, fmt="paf", raw=False):
        """output_results_paf / output_results_bedpe over every range (main.rs:11894-12103); the batch
        must have been queried with store_cigar = True.  Results of a tracepoint index print as "bedpe" only
        (the reference refuses "paf" in approximate mode, main.rs:7387-7397).  raw: the text as bytes."""
        L = lib()
        p = params or make_params(store_cigar=True)
        arr = None
        if range_names is not None:
            arr = (C.c_char_p * len(range_names))(*[None if s is None else s.encode() for s in range_names])
        text = C.c_void_p(None)
        ln = C.c_size_t(0)
        check(L.impg_gpu_results_paf(self._h, self._owner._h, arr, C.byref(p), merge_distance, {"paf": 0, "bedpe": 1}[fmt],
                                     C.byref(text), C.byref(ln)))
        try:
            out = _text_bytes(text, ln.value)
            return out if raw else out.decode()
        finally:
            _lib.free(text)

    def __del__(self):
        if getattr(self, "_h", None) and not getattr(self, "_borrowed", False):
            try:
                lib().impg_gpu_results_free(self._h)
            except Exception:
                pass
            self._h = None


_HIP = None


def _hip_memcpy_d2h(dst, src, nbytes, device=None):
    """hipMemcpy device -> host through the HIP runtime the library itself links (tests and probes read device rows back);
    device: the HIP device that holds `src` (made current for the copy)."""
    global _HIP
    if _HIP is None:
        _HIP = C.CDLL("libamdhip64.so")
        _HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _HIP.hipMemcpy.restype = C.c_int
        _HIP.hipGetDevice.argtypes = [C.POINTER(C.c_int)]
        _HIP.hipGetDevice.restype = C.c_int
        _HIP.hipSetDevice.argtypes = [C.c_int]
        _HIP.hipSetDevice.restype = C.c_int
    if nbytes:
        prev = C.c_int(-1)
        if device is not None and _HIP.hipGetDevice(C.byref(prev)) == 0 and prev.value != device:
            _HIP.hipSetDevice(device)
        try:
            rc = _HIP.hipMemcpy(dst, src, nbytes, 2)
        finally:
            if device is not None and prev.value >= 0 and prev.value != device:
                _HIP.hipSetDevice(prev.value)
        if rc != 0:
            raise ImpgGpuError(_lib.IMPG_E_HIP, "hipMemcpy (device to host) failed: %d" % rc)


class DeviceRows:
    """impg_gpu_device_rows_t: the rows of a batch left in HBM (impg_gpu_query_batch_device).  On one GPU it holds one of
    the index's engines until freed (free() or garbage collection).  On a sharded index the parts lie on the ranks that
    hold them (part_device) and range indices are those of the collective batch (batch_offset); in rank processes check()
    is collective: every rank calls it."""

    def __init__(self, handle, owner, n):
        self._h = handle
        self._owner = owner  # keeps the index alive
        self._n = int(n)
        st = Stats()
        lib().impg_gpu_device_rows_stats(self._h, C.byref(st))
        self.stats = st
        self.projected = int(st.projected)
        self.place_ms = float(lib().impg_gpu_device_rows_place_ms(self._h))

    def parts(self):
        out = []
        for k in range(lib().impg_gpu_device_rows_num_parts(self._h)):
            d = _lib.DevicePart()
            check(lib().impg_gpu_device_rows_part(self._h, k, C.byref(d)))
            out.append(d)
        return out

    def part_device(self, k):
        """The HIP device that holds part k's arrays."""
        dev = C.c_int(-1)
        check(lib().impg_gpu_device_rows_part_device(self._h, k, C.byref(dev)))
        return dev.value

    def batch_offset(self):
        """(first range of this caller's ranges in the collective batch, size of that batch); (0, n) on one GPU and on a
        multi-GPU handle."""
        off, tot = C.c_uint64(0), C.c_uint64(0)
        check(lib().impg_gpu_device_rows_batch_offset(self._h, C.byref(off), C.byref(tot)))
        return int(off.value), int(tot.value)

    def part_to_host(self, k):
        """One part copied back from the device that holds it: (first_range, level, query_id[n], coords[n, 4], source[n],
        frontier[n_frontier])."""
        d = self.parts()[k]
        dev = self.part_device(k)
        n, nf, st = int(d.n_slots), int(d.n_frontier), int(d.slot_stride)
        co = np.empty((n, 4), dtype=np.int32)
        fr = np.empty(nf, dtype=_lib.FRONTIER_DTYPE)
        if st == 1:
            qid = np.empty(n, dtype=np.uint32)
            src = np.empty(n, dtype=np.uint32)
            _hip_memcpy_d2h(qid.ctypes.data, d.query_id, n * 4, dev)
            _hip_memcpy_d2h(src.ctypes.data, d.source, n * 4, dev)
        else:  # query_id and source side by side (source = query_id + 1 word)
            assert d.source == d.query_id + 4 and st == 2
            both = np.empty((n, 2), dtype=np.uint32)
            _hip_memcpy_d2h(both.ctypes.data, d.query_id, n * 8, dev)
            qid, src = np.ascontiguousarray(both[:, 0]), np.ascontiguousarray(both[:, 1])
        _hip_memcpy_d2h(co.ctypes.data, d.coords, n * 16, dev)
        _hip_memcpy_d2h(fr.ctypes.data, d.frontier, nf * 16, dev)
        return int(d.first_range), int(d.level), qid, co, src, fr

    def ordered_to_host(self, k=0):
        """IMPG_ROWS_ORDERED part k copied back: (first_range, rows[INTERVAL_DTYPE], offsets[n_ranges + 1])."""
        d = self.parts()[k]
        rows = np.empty(int(d.n_slots), dtype=INTERVAL_DTYPE)
        off = np.empty(int(d.n_ranges) + 1, dtype=np.uint32)
        _hip_memcpy_d2h(rows.ctypes.data, d.rows, rows.nbytes)
        _hip_memcpy_d2h(off.ctypes.data, d.offsets, off.nbytes)
        return int(d.first_range), rows, off

    def check(self, counts=True, checksums=True):
        """impg_gpu_device_rows_check: per-range counts / checksums recomputed from the rows in HBM, for this caller's
        ranges (collective in rank processes)."""
        n = self._n
        cnt = np.zeros(n, dtype=np.uint64) if counts else None
        ck = np.zeros(n, dtype=np.uint64) if checksums else None
        check(lib().impg_gpu_device_rows_check(self._h, cnt.ctypes.data if counts else None, ck.ctypes.data if checksums else None))
        return cnt, ck

    def free(self):
        if self._h:
            lib().impg_gpu_device_rows_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PreparedMask:
    """A masked_regions map already in the C layout (impg_gpu_mask_t + the arrays it points into): per-call users --
    the shape of partition.rs:359-391 -- convert once per change of the map, not once per call."""

    def __init__(self, m, arrays):
        self.m, self.arrays = m, arrays


def prepare_mask(masked_regions):
    return PreparedMask(*GpuImpg._mask(masked_regions))


class Sequences:
    """The sequences FASTA output prints (impg_gpu_sequences_t): one byte per base, upper-cased at load."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_fasta(cls, paths):
        """Plain FASTA files (a path or a list of them); gzip input is IMPG_E_UNSUPPORTED, a name twice IMPG_E_INVALID."""
        if isinstance(paths, (str, bytes, os.PathLike)):
            paths = [paths]
        arr = (C.c_char_p * len(paths))(*[os.fsencode(q) for q in paths])
        h = C.c_void_p(None)
        check(lib().impg_gpu_sequences_from_fasta(arr, len(paths), C.byref(h)))
        return cls(h)

    @classmethod
    def from_arrays(cls, names, sequences):
        """names[i] -> sequences[i] (bytes or str)."""
        seqs = [q.encode() if isinstance(q, str) else bytes(q) for q in sequences]
        if len(names) != len(seqs):
            raise _lib.ImpgGpuError(_lib.IMPG_E_INVALID, "one name per sequence")
        off = np.zeros(len(seqs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(q) for q in seqs], dtype=np.uint64)
        bases = b"".join(seqs)
        arr = (C.c_char_p * len(names))(*[q.encode() if isinstance(q, str) else q for q in names])
        h = C.c_void_p(None)
        check(lib().impg_gpu_sequences_from_memory(arr, off.ctypes.data, bases, len(seqs), C.byref(h)))
        return cls(h)

    def __len__(self):
        return lib().impg_gpu_sequences_num(self._h)

    def name(self, i):
        s = lib().impg_gpu_sequences_name(self._h, i)
        return None if s is None else s.decode()

    def bases(self, i):
        n = C.c_uint64(0)
        q = lib().impg_gpu_sequences_bases(self._h, i, C.byref(n))
        if q is None and n.value == 0 and i >= len(self):
            raise IndexError(i)
        return C.string_at(q, n.value) if n.value else b""

    def items(self):
        return [(self.name(i), self.bases(i)) for i in range(len(self))]

    def exceptions(self, i):
        """impg_gpu_sequences_exceptions (host-only): sequence i's maximal runs of one byte that is not A/C/G/T, as the
        packed store keeps them -> (start, length, byte) arrays (uint32, uint32, uint8), in order."""
        if not 0 <= i < len(self):
            raise IndexError(i)
        n = C.c_size_t(0)
        check(lib().impg_gpu_sequences_exceptions(self._h, i, None, None, None, 0, C.byref(n)))
        start, length, byte = np.zeros(n.value, dtype=np.uint32), np.zeros(n.value, dtype=np.uint32), np.zeros(n.value, dtype=np.uint8)
        if n.value:
            check(lib().impg_gpu_sequences_exceptions(self._h, i, start.ctypes.data, length.ctypes.data, byte.ctypes.data, n.value, C.byref(n)))
        return start, length, byte

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().impg_gpu_sequences_free(self._h)
            except Exception:
                pass
            self._h = None


def fasta_text(sequences, names, rows, merge_distance=0, reverse_complement=False):
    """impg_gpu_fasta_text (host-only): one range's rows (INTERVAL_DTYPE) -> its FASTA records as bytes: the sweep of
    merge_query_adjusted_intervals with the strands apart, then the text.  names[id] = the name of sequence id."""
    a = np.ascontiguousarray(rows, dtype=INTERVAL_DTYPE)
    arr = (C.c_char_p * max(len(names), 1))(*[q.encode() if isinstance(q, str) else q for q in names])
    text, ln = C.c_void_p(None), C.c_size_t(0)
    check(lib().impg_gpu_fasta_text(sequences._h, arr, len(names), a.ctypes.data, a.size, merge_distance, int(bool(reverse_complement)),
                                    C.byref(text), C.byref(ln)))
    try:
        return _text_bytes(text, ln.value)
    finally:
        _lib.free(text)


def partition_fasta_text(sequences, names, rows):
    """impg_gpu_partition_fasta_text (host-only): a partition's intervals [(seq_id, start, end)] -> the records of its
    partition{N}.fasta as bytes: no sweep, every row forward and printed where it stands, a record of no bases is its header
    alone.  names[id] = the name of sequence id."""
    a = np.array([tuple(r) for r in rows], dtype=_lib.PARTITION_ROW_DTYPE)
    arr = (C.c_char_p * max(len(names), 1))(*[q.encode() if isinstance(q, str) else q for q in names])
    text, ln = C.c_void_p(None), C.c_size_t(0)
    check(lib().impg_gpu_partition_fasta_text(sequences._h, arr, len(names), a.ctypes.data, a.size, C.byref(text), C.byref(ln)))
    try:
        return _text_bytes(text, ln.value)
    finally:
        _lib.free(text)


class GpuImpg:
    """`impl ImpgIndex` backed by the HIP engine."""

    def __init__(self, handle):
        self._h = handle

    # ---- construction (Impg::from_multi_alignment_records / load) ------------
    @classmethod
    def from_records(cls, records, ops, seq_len, bidirectional=True, order=_lib.ORDER_COITREES, device=0,
                     file_first=None, devices=None, lanes=2, comm=None):
        """file_first: first record of every alignment file (records_by_file of the reference); only the
        MultiImpg tie order observes it.
        devices=[...]: ONE handle over several GPUs of this process (impg_gpu_index_create_multi).
        comm=Comm: this rank's shard of an index sharded one process per GPU (impg_gpu_index_create_rank);
        queries on it are collective calls."""
        rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        ops = np.ascontiguousarray(ops, dtype=np.uint32)
        sl = np.ascontiguousarray(seq_len, dtype=np.int64)
        h = C.c_void_p(None)
        ff = None if file_first is None else np.ascontiguousarray(file_first, dtype=np.uint64)
        ffp, ffn = (None, 0) if ff is None else (ff.ctypes.data, ff.size)
        if devices is not None:
            dv = np.ascontiguousarray(devices, dtype=np.int32)
            check(lib().impg_gpu_index_create_multi(rec.ctypes.data, rec.size, ops.ctypes.data, ops.size, sl.ctypes.data, sl.size,
                                                    ffp, ffn, int(bidirectional), order, dv.ctypes.data, dv.size, lanes, C.byref(h)))
        elif comm is not None:
            check(lib().impg_gpu_index_create_rank(rec.ctypes.data, rec.size, ops.ctypes.data, ops.size, sl.ctypes.data, sl.size,
                                                   ffp, ffn, int(bidirectional), order, device, comm._h, C.byref(h)))
        elif ff is not None:
            check(lib().impg_gpu_index_create_files(rec.ctypes.data, rec.size, ops.ctypes.data, ops.size, sl.ctypes.data, sl.size,
                                                    ffp, ffn, int(bidirectional), order, device, C.byref(h)))
        else:
            check(lib().impg_gpu_index_create(rec.ctypes.data, rec.size, ops.ctypes.data, ops.size, sl.ctypes.data, sl.size,
                                              int(bidirectional), order, device, C.byref(h)))
        ix = cls(h)
        ix._comm = comm  # the communicator outlives the index
        return ix

    @classmethod
    def load_impg(cls, impg_path, alignment_files, order=_lib.ORDER_COITREES, device=0):
        """impg_gpu_index_load_impg: the reference's own IMPGIDX2 index file + the alignment files it was built from."""
        if isinstance(alignment_files, str):
            alignment_files = [alignment_files]
        arr = (C.c_char_p * len(alignment_files))(*[p.encode() for p in alignment_files])
        h = C.c_void_p(None)
        check(lib().impg_gpu_index_load_impg(os.fsencode(impg_path), arr, len(alignment_files), order, device, C.byref(h)))
        return cls(h)

    @classmethod
    def from_tracepoints(cls, records, tracepoints, seq_len, query_deltas=None, diffs=None, fastga=False, trace_spacing=0,
                         max_complexity=0, bidirectional=True, order=_lib.ORDER_COITREES, device=0, devices=None, lanes=2):
        """impg_gpu_index_create_tracepoints: an index over tracepoint alignments (.1aln / .tpa content handed over as
        arrays); every query on it runs in approximate mode (approximate_mode = true of the trait).  store_cigar is
        refused on it until set_option("approximate_cigar", 1): a row's CIGAR is then the reference's approximate one,
        [matches '='] [mismatches 'X'] with a zero count left out (impg.rs:1479-1486) -- counts, not an alignment --,
        and QueryResults.paf(fmt="bedpe") prints what `impg query --approximate -o bedpe` prints."""
        rec = np.ascontiguousarray(records, dtype=_lib.TP_RECORD_DTYPE)
        tp = np.ascontiguousarray(tracepoints, dtype=np.int32)
        qd = None if query_deltas is None else np.ascontiguousarray(query_deltas, dtype=np.int32)
        df = None if diffs is None else np.ascontiguousarray(diffs, dtype=np.int32)
        sl = np.ascontiguousarray(seq_len, dtype=np.int64)
        mode = _lib.TpMode(int(bool(fastga)), int(trace_spacing), int(max_complexity))
        h = C.c_void_p(None)
        if devices is not None:  # sharded by target sequence over the GPUs of this process
            dv = np.ascontiguousarray(devices, dtype=np.int32)
            check(lib().impg_gpu_index_create_tracepoints_multi(rec.ctypes.data, rec.size, tp.ctypes.data, None if qd is None else qd.ctypes.data,
                                                                None if df is None else df.ctypes.data, tp.size, C.byref(mode), sl.ctypes.data,
                                                                sl.size, int(bidirectional), order, dv.ctypes.data, dv.size, lanes, C.byref(h)))
            return cls(h)
        check(lib().impg_gpu_index_create_tracepoints(rec.ctypes.data, rec.size, tp.ctypes.data, None if qd is None else qd.ctypes.data,
                                                      None if df is None else df.ctypes.data, tp.size, C.byref(mode), sl.ctypes.data,
                                                      sl.size, int(bidirectional), order, device, C.byref(h)))
        return cls(h)

    def save(self, path):
        """impg_gpu_index_save: the built index (device arrays + sequence table) as one file."""
        check(lib().impg_gpu_index_save(self._h, os.fsencode(path)))

    @classmethod
    def load(cls, path, device=0, devices=None, lanes=2, comm=None):
        """impg_gpu_index_load: what `save` wrote, back in HBM without touching the alignment files.
        devices=[...]: a saved multi handle (impg_gpu_index_load_multi); comm=Comm: this rank's saved shard
        (impg_gpu_index_load_rank)."""
        h = C.c_void_p(None)
        if devices is not None:
            dv = np.ascontiguousarray(devices, dtype=np.int32)
            check(lib().impg_gpu_index_load_multi(os.fsencode(path), dv.ctypes.data, dv.size, lanes, C.byref(h)))
        elif comm is not None:
            check(lib().impg_gpu_index_load_rank(os.fsencode(path), device, comm._h, C.byref(h)))
        else:
            check(lib().impg_gpu_index_load(os.fsencode(path), device, C.byref(h)))
        ix = cls(h)
        ix._comm = comm
        return ix

    @classmethod
    def from_paf(cls, paths, bidirectional=True, order=_lib.ORDER_COITREES, device=0, devices=None, lanes=2, comm=None, ingest="host",
                 piece_bytes=None, resolve_matches=None):
        """devices / comm: as in from_records (impg_gpu_index_create_from_paf_multi / _rank).  ingest="device": the files are
        streamed into HBM in pieces of piece_bytes (None: 64 MiB) and parsed there (impg_gpu_index_create_from_paf_streamed;
        one GPU: not with devices= or comm=); "host" is the host's line and field parser.  resolve_matches=Sequences: every
        'M' op is rewritten on the device as the '=' / 'X' runs the sequences spell before the index is built
        (impg_gpu_index_create_from_paf_resolved; ingest="host" on one GPU only); resolve_report() and resolve_flags say
        what the pass found."""
        if isinstance(paths, str):
            paths = [paths]
        if ingest not in ("host", "device"):
            raise ValueError("ingest is 'host' or 'device'")
        if ingest == "device" and (devices is not None or comm is not None):
            raise ValueError("ingest='device' builds on one GPU: not with devices= or comm=")
        if ingest == "host" and piece_bytes is not None:
            raise ValueError("piece_bytes belongs to ingest='device'")
        if resolve_matches is not None and (ingest != "host" or devices is not None or comm is not None):
            raise ValueError("resolve_matches sits behind the host ingest on one GPU: not with ingest='device', devices= or comm=")
        arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
        h = C.c_void_p(None)
        if resolve_matches is not None:
            rep, fl = _lib.ResolveReport(), C.c_void_p(None)
            check(lib().impg_gpu_index_create_from_paf_resolved(arr, len(paths), resolve_matches._h, int(bidirectional), order, device,
                                                                C.byref(rep), C.byref(fl), C.byref(h)))
            ix = cls(h)
            ix._comm = None
            try:
                ix.resolve_flags = np.frombuffer(C.string_at(fl, int(rep.records)), dtype=np.uint8).copy()
            finally:
                _lib.free(fl)
            return ix
        if ingest == "device":
            check(lib().impg_gpu_index_create_from_paf_streamed(arr, len(paths), int(bidirectional), order, device, int(piece_bytes or 0), C.byref(h)))
        elif devices is not None:
            dv = np.ascontiguousarray(devices, dtype=np.int32)
            check(lib().impg_gpu_index_create_from_paf_multi(arr, len(paths), int(bidirectional), order, dv.ctypes.data, dv.size,
                                                             lanes, C.byref(h)))
        elif comm is not None:
            check(lib().impg_gpu_index_create_from_paf_rank(arr, len(paths), int(bidirectional), order, device, comm._h, C.byref(h)))
        else:
            check(lib().impg_gpu_index_create_from_paf(arr, len(paths), int(bidirectional), order, device, C.byref(h)))
        ix = cls(h)
        ix._comm = comm
        return ix

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().impg_gpu_index_destroy(self._h)
            except Exception:  # interpreter shutdown: the binding module may already be torn down
                pass
            self._h = None

    # ---- seq_index() / target_ids() / num_targets() ---------------------------
    def partition_session(self, window_size, merge_distance, params=None, **kw):
        """A PartitionSession on this index; params default to the reference CLI's transitive BFS."""
        return PartitionSession(self, params or make_params(transitive=True), window_size, merge_distance, **kw)

    def partition(self, window_size, merge_distance, params=None, **kw):
        """`impg partition` window by window: yields (partition_num, [(seq_id, start, end)]) before rehoming."""
        s = self.partition_session(window_size, merge_distance, params, **kw)
        try:
            num = 0
            while True:
                ws = s.next_windows()
                if not ws:
                    return
                for w in ws:
                    rows = s.window(*w)
                    if rows:
                        yield num, rows
                        num += 1
        finally:
            s.close()

    def partitions_bed(self, window_size, merge_distance, params=None, **kw):
        """The text of partitions.bed (write_single_partition_file, partition.rs:1682-1717)."""
        s = self.partition_session(window_size, merge_distance, params, **kw)
        try:
            return s.run_text()[0]
        finally:
            s.close()

    def partitions_fasta(self, folder, window_size, merge_distance, params=None, **kw):
        """`impg partition -o fasta --separate-files`: folder/partition{N}.fasta per partition, from the attached sequence
        store (set_sequences); returns the number of partitions."""
        s = self.partition_session(window_size, merge_distance, params, **kw)
        try:
            return s.run_fasta(folder)
        finally:
            s.close()

    def partition_rows_fasta(self, rows, on_host=False):
        """impg_gpu_partition_rows_fasta: the partition FASTA writer over the caller's rows [(seq_id, start, end)], on the
        device (uploaded, printed from the store in HBM in byte-window pieces) or by the host twin.  Returns bytes."""
        a = np.array([tuple(r) for r in rows], dtype=_lib.PARTITION_ROW_DTYPE)
        text, ln = C.c_void_p(None), C.c_size_t(0)
        check(lib().impg_gpu_partition_rows_fasta(self._h, a.ctypes.data, a.size, int(bool(on_host)), C.byref(text), C.byref(ln)))
        try:
            return _text_bytes(text, ln.value)
        finally:
            _lib.free(text)

    def refine(self, loci, params=None, span_bp=1000, max_extension=0.5, extension_step=1000, merge_distance=0, level="sequence",
               separator="#", subset_keep=None, blacklist=None, on_host=False, names=None):
        """`impg refine` (impg_gpu_refine) for loci [(target_id, start, end)]: a RefineResult.  level: 'sequence' | 'sample' |
        'haplotype' (the PanSN level support is counted at; the latter two also stop a locus at its max_entities);
        blacklist {seq_id: [(start, end), ...]}; on_host=True: support_on_host; names: the loci's labels."""
        if level not in ("sequence", "sample", "haplotype"):
            raise ValueError("level is 'sequence', 'sample' or 'haplotype'")
        p = params or make_params()
        n_seq = self.num_seqs()
        seq_names = [self.seq_name(i) for i in range(n_seq)]
        if any(nm is None for nm in seq_names):  # an index made without names: records without chrom and text
            if level != "sequence":
                raise ValueError("levels 'sample' and 'haplotype' need the sequence names")
            seq_names = None
        ent = None if level == "sequence" else entity_ids(seq_names, level, separator)[0]
        keep = None if subset_keep is None else np.ascontiguousarray(subset_keep, dtype=np.uint8)
        if keep is not None and keep.size != n_seq:
            raise ValueError("subset_keep holds one entry per sequence")
        bo, br = _blacklist_table(blacklist, n_seq)
        lo = self._ranges(loci)
        opts = _refine_opts(span_bp, max_extension, extension_step, merge_distance, level != "sequence", on_host)
        ptr = lambda x: None if x is None else x.ctypes.data
        h = C.c_void_p()
        _lib.check(_lib.lib().impg_gpu_refine(self._h, lo.ctypes.data, lo.size, C.byref(p), C.byref(opts), ptr(ent), ptr(keep), ptr(bo), ptr(br),
                                              C.byref(h)))
        try:
            return RefineResult(h, seq_names, list(names) if names is not None else None)
        finally:
            _lib.lib().impg_gpu_refine_free(h)

    def num_seqs(self):
        return lib().impg_gpu_num_seqs(self._h)

    def seq_name(self, i):
        s = lib().impg_gpu_seq_name(self._h, i)
        return None if s is None else s.decode()

    def seq_len(self, i):
        return lib().impg_gpu_seq_len(self._h, i)

    def seq_id(self, name):
        r = lib().impg_gpu_seq_id(self._h, name.encode())
        return None if r < 0 else int(r)

    def num_targets(self):
        return lib().impg_gpu_num_targets(self._h)

    def target_ids(self):
        n = lib().impg_gpu_target_ids(self._h, None, 0)
        out = np.zeros(n, dtype=np.uint32)
        lib().impg_gpu_target_ids(self._h, out.ctypes.data, n)
        return out

    def num_entries(self):
        return lib().impg_gpu_num_entries(self._h)

    def num_records(self):
        return lib().impg_gpu_num_records(self._h)

    def device_bytes(self):
        return lib().impg_gpu_device_bytes(self._h)

    def set_option(self, key, value):
        """impg_gpu_set_option: one of option_keys(); include/impg_gpu.h describes each."""
        check(lib().impg_gpu_set_option(self._h, key.encode(), int(value)))

    def counter(self, key):
        """impg_gpu_get_counter: one of counter_keys(); include/impg_gpu.h describes each.  The "update_*" counters
        move under set_option("update_stats", 1), the "lookup_wide_*" ones under set_option("lookup_stats", 1)."""
        v = C.c_int64(0)
        check(lib().impg_gpu_get_counter(self._h, key.encode(), C.byref(v)))
        return v.value

    def resolve_report(self):
        """The report of from_paf(..., resolve_matches=) as a dict (impg_gpu_resolve_report_t; the "resolve_*" counters):
        all zero on a handle made any other way."""
        return {k: self.counter("resolve_" + k) for k in _lib.RESOLVE_FIELDS}

    # ---- queries ---------------------------------------------------------------
    @staticmethod
    def _ranges(ranges):
        if isinstance(ranges, np.ndarray) and ranges.dtype == RANGE_DTYPE:
            return np.ascontiguousarray(ranges)
        a = np.zeros(len(ranges), dtype=RANGE_DTYPE)
        for i, (t, s, e) in enumerate(ranges):
            a[i] = (t, s, e)
        return a

    @staticmethod
    def _mask(masked_regions):
        """{sequence id: (sequence_length, [(start, end), ...])} -> (impg_gpu_mask_t, arrays kept alive).  A
        PreparedMask (prepare_mask: the conversion done once for many calls) passes through."""
        if isinstance(masked_regions, PreparedMask):
            return masked_regions.m, masked_regions.arrays
        ids = sorted(masked_regions)
        seq = np.array(ids, dtype=np.uint32)
        slen = np.array([masked_regions[i][0] for i in ids], dtype=np.int32)
        off = np.zeros(len(ids) + 1, dtype=np.uint64)
        flat = []
        for k, i in enumerate(ids):
            flat.extend(masked_regions[i][1])
            off[k + 1] = len(flat)
        rng = np.ascontiguousarray(np.array(flat, dtype=np.int32).reshape(-1, 2))
        m = _lib.Mask(len(ids), seq.ctypes.data, slen.ctypes.data, off.ctypes.data, rng.ctypes.data)
        return m, (seq, slen, off, rng)

    def query_batch(self, ranges, params=None, masked_regions=None, subset_keep=None, copy=True, **kw):
        """masked_regions: one map for the whole batch (impg_gpu_query_batch_masked); every range starts
        from its own clone of it, as the reference's per-range calls do (impg.rs:2077-2081).
        subset_keep: uint8[num_seqs], the host's SubsetFilter::matches verdict per sequence id."""
        p = params or make_params(**kw)
        r = self._ranges(ranges)
        h = C.c_void_p(None)
        if subset_keep is not None:
            keep = np.ascontiguousarray(subset_keep, dtype=np.uint8)
            if keep.size != self.num_seqs():
                raise _lib.ImpgGpuError(_lib.IMPG_E_INVALID, "subset_keep needs one entry per sequence")
            m, keepalive = self._mask(masked_regions) if masked_regions is not None else (None, None)
            check(lib().impg_gpu_query_batch_filtered(self._h, r.ctypes.data, r.size, C.byref(p),
                                                      C.byref(m) if m is not None else None, keep.ctypes.data, C.byref(h)))
            del keepalive
        elif masked_regions is not None:
            m, keep = self._mask(masked_regions)
            check(lib().impg_gpu_query_batch_masked(self._h, r.ctypes.data, r.size, C.byref(p), C.byref(m), C.byref(h)))
            del keep
        else:
            check(lib().impg_gpu_query_batch(self._h, r.ctypes.data, r.size, C.byref(p), C.byref(h)))
        return QueryResults(h, self, copy=copy)

    def query_batch_stream(self, ranges, consumer, params=None, masked_regions=None, subset_keep=None, chunk_ranges=0,
                           max_block_bytes=0, copy=False, **kw):
        """impg_gpu_query_batch_stream: the rows of a batch too big for one result object, chunk by chunk in range order.
        consumer(first_range, QueryResults) is called for every chunk (copy=False: its arrays are views of the library's
        pinned block, valid only during the call); a truthy return stops the stream.  Returns the projections counted."""
        p = params or make_params(**kw)
        r = self._ranges(ranges)
        keep = None
        if subset_keep is not None:
            keep = np.ascontiguousarray(subset_keep, dtype=np.uint8)
            if keep.size != self.num_seqs():
                raise _lib.ImpgGpuError(_lib.IMPG_E_INVALID, "subset_keep needs one entry per sequence")
        m, keepalive = self._mask(masked_regions) if masked_regions is not None else (None, None)
        failure = []

        def trampoline(ctx, chunk, first):
            try:
                q = QueryResults.__new__(QueryResults)
                q._borrowed = True
                QueryResults.__init__(q, C.c_void_p(chunk), self, copy=copy)
                return 1 if consumer(int(first), q) else 0
            except BaseException as e:  # (an exception must not unwind through the library's thread)
                failure.append(e)
                return 1

        cb = _lib.STREAM_CB(trampoline)
        proj = C.c_uint64(0)
        rc = lib().impg_gpu_query_batch_stream(self._h, r.ctypes.data, r.size, C.byref(p), C.byref(m) if m is not None else None,
                                               None if keep is None else keep.ctypes.data, chunk_ranges, max_block_bytes,
                                               C.cast(cb, C.c_void_p), None, C.byref(proj))
        del keepalive
        if failure:
            raise failure[0]
        if rc != _lib.IMPG_E_CANCELLED:
            check(rc)
        return proj.value

    def query_batch_bed(self, ranges, params=None, merge_distance=0, range_names=None, subset_keep=None, timing=False, raw=False, **kw):
        """impg_gpu_query_batch_bed: query + both BED merges on the device + text (what `impg query -o bed` prints)."""
        return self._query_batch_text(lib().impg_gpu_query_batch_bed, ranges, params, merge_distance, range_names, subset_keep, timing, raw, kw)

    def query_batch_bedpe(self, ranges, params=None, merge_distance=0, range_names=None, subset_keep=None, timing=False, raw=False, fd=None,
                          **kw):
        """impg_gpu_query_batch_bedpe: query + CIGAR summaries + merge_adjusted_intervals on the device + text (what
        `impg query -b` prints by default); store_cigar is implied.  fd: impg_gpu_query_batch_bedpe_fd -- the text is
        written there and the number of bytes returned in its place."""
        if fd is None:
            return self._query_batch_text(lib().impg_gpu_query_batch_bedpe, ranges, params, merge_distance, range_names, subset_keep, timing,
                                          raw, kw)
        return self._query_batch_text_fd(lib().impg_gpu_query_batch_bedpe_fd, ranges, params, merge_distance, range_names, subset_keep, timing,
                                         fd, kw)

    def query_batch_paf(self, ranges, params=None, merge_distance=0, range_names=None, subset_keep=None, timing=False, raw=False, fd=None,
                        **kw):
        """impg_gpu_query_batch_paf: the same merge, and every line's merged CIGAR fused and printed as cg:Z on the device
        (what `impg query -o paf` prints); store_cigar is implied.  fd: impg_gpu_query_batch_paf_fd -- the text is
        written there and the number of bytes returned in its place."""
        if fd is None:
            return self._query_batch_text(lib().impg_gpu_query_batch_paf, ranges, params, merge_distance, range_names, subset_keep, timing,
                                          raw, kw)
        return self._query_batch_text_fd(lib().impg_gpu_query_batch_paf_fd, ranges, params, merge_distance, range_names, subset_keep, timing,
                                         fd, kw)

    def set_sequences(self, sequences, packed=None):
        """impg_gpu_index_set_sequences: attach a Sequences store (its bases go to HBM), or detach with None.  packed:
        option "sequence_store_packed" set first -- False one byte per base, True two bits per base with the bytes that
        are not A/C/G/T kept as runs, "auto" whichever takes fewer bytes in HBM; None leaves the option as it is."""
        if packed is not None:
            if not any(packed is v for v in (False, True)) and packed != "auto":
                raise ValueError("packed is None, False, True or 'auto'")
            self.set_option("sequence_store_packed", 2 if packed == "auto" else int(packed))
        check(lib().impg_gpu_index_set_sequences(self._h, None if sequences is None else sequences._h))

    def load_sequences(self, paths, packed=None):
        """impg_gpu_index_load_sequences: FASTA files (a path or a list; plain, gzip or BGZF) streamed straight into HBM and
        parsed there; it replaces any attached store and leaves no host copy of the bases.  packed: option
        "sequence_store_packed" set first -- False one byte per base, True packed; None leaves the option as it is ("auto" is
        set_sequences' alone)."""
        if packed is not None:
            if not any(packed is v for v in (False, True)):
                raise ValueError("packed is None, False or True")
            self.set_option("sequence_store_packed", int(packed))
        if isinstance(paths, (str, bytes, os.PathLike)):
            paths = [paths]
        arr = (C.c_char_p * len(paths))(*[os.fsencode(q) for q in paths])
        check(lib().impg_gpu_index_load_sequences(self._h, arr, len(paths)))

    def query_batch_fasta(self, ranges, params=None, merge_distance=0, range_names=None, subset_keep=None, timing=False, raw=False,
                          reverse_complement=False, fd=None, **kw):
        """impg_gpu_query_batch_fasta: query + the query-axis sweep + the records written on the device from the store in
        HBM (what `impg query -o fasta` prints).  fd: impg_gpu_query_batch_fasta_fd -- the text is written there and the
        number of bytes returned in its place."""
        rc = int(bool(reverse_complement))
        if fd is None:
            entry = lambda h, r, n, p, keep, d, names, text, ln, sec: lib().impg_gpu_query_batch_fasta(h, r, n, p, keep, d, names, rc, text, ln, sec)
            return self._query_batch_text(entry, ranges, params, merge_distance, range_names, subset_keep, timing, raw, kw)
        entry = lambda h, r, n, p, keep, d, names, f, done, sec: lib().impg_gpu_query_batch_fasta_fd(h, r, n, p, keep, d, names, rc, f, done, sec)
        return self._query_batch_text_fd(entry, ranges, params, merge_distance, range_names, subset_keep, timing, fd, kw)

    def fasta_rows(self, rows, row_range, n_ranges, merge_distance=0, reverse_complement=False):
        """impg_gpu_selftest_fasta_rows (diagnostics): the device sweep and FASTA writer of query_batch_fasta on the caller's
        rows (INTERVAL_DTYPE; row_range[i] = the range of rows[i]).  Returns the text as bytes."""
        a = np.ascontiguousarray(rows, dtype=INTERVAL_DTYPE)
        rr = np.ascontiguousarray(row_range, dtype=np.uint32)
        if a.size != rr.size:
            raise _lib.ImpgGpuError(_lib.IMPG_E_INVALID, "one range index per row")
        text, ln = C.c_void_p(None), C.c_size_t(0)
        check(lib().impg_gpu_selftest_fasta_rows(self._h, a.ctypes.data, rr.ctypes.data, a.size, n_ranges, merge_distance,
                                                 int(bool(reverse_complement)), C.byref(text), C.byref(ln)))
        try:
            return _text_bytes(text, ln.value)
        finally:
            _lib.free(text)

    def _query_batch_text_fd(self, entry, ranges, params, merge_distance, range_names, subset_keep, timing, fd, kw):
        p = params or make_params(**kw)
        r = self._ranges(ranges)
        arr = None
        if range_names is not None:
            arr = (C.c_char_p * len(range_names))(*[None if s is None else s.encode() for s in range_names])
        keep = None if subset_keep is None else np.ascontiguousarray(subset_keep, dtype=np.uint8)
        done = C.c_uint64(0)
        sec = (C.c_double * 3)()
        check(entry(self._h, r.ctypes.data, r.size, C.byref(p), None if keep is None else keep.ctypes.data, merge_distance, arr, fd,
                    C.byref(done), sec))
        return (done.value, list(sec)) if timing else done.value

    def _query_batch_text(self, entry, ranges, params, merge_distance, range_names, subset_keep, timing, raw, kw):
        p = params or make_params(**kw)
        r = self._ranges(ranges)
        arr = None
        if range_names is not None:
            arr = (C.c_char_p * len(range_names))(*[None if s is None else s.encode() for s in range_names])
        keep = None if subset_keep is None else np.ascontiguousarray(subset_keep, dtype=np.uint8)
        text = C.c_void_p(None)
        ln = C.c_size_t(0)
        sec = (C.c_double * 3)()
        check(entry(self._h, r.ctypes.data, r.size, C.byref(p), None if keep is None else keep.ctypes.data, merge_distance, arr, C.byref(text),
                    C.byref(ln), sec))
        try:
            out = _text_bytes(text, ln.value)
        finally:
            _lib.free(text)
        out = out if raw else out.decode()
        return (out, list(sec)) if timing else out

    def bed_rows(self, rows, row_range, n_ranges, n_seq, merge_distance=0, merge_strands=True, original_sequence_coordinates=False,
                 range_names=None, gap=False):
        """impg_gpu_selftest_bed_rows (diagnostics): the device BED merges and text of query_batch_bed on the caller's
        rows (INTERVAL_DTYPE; row_range[i] = the range of rows[i]).  Returns (merged rows as BED_ROW_DTYPE, text bytes);
        gap=True: also (the rows between the two merges as INTERVAL_DTYPE, their ranges), in their order."""
        a = np.ascontiguousarray(rows, dtype=INTERVAL_DTYPE)
        rr = np.ascontiguousarray(row_range, dtype=np.uint32)
        if a.size != rr.size:
            raise _lib.ImpgGpuError(_lib.IMPG_E_INVALID, "one range index per row")
        arr = None
        if range_names is not None:
            if len(range_names) != n_ranges:
                raise _lib.ImpgGpuError(_lib.IMPG_E_INVALID, "one name per range")
            arr = (C.c_char_p * len(range_names))(*[None if s is None else (s if isinstance(s, bytes) else s.encode()) for s in range_names])
        merged, text = C.c_void_p(None), C.c_void_p(None)
        nm, ln = C.c_size_t(0), C.c_size_t(0)
        grows, grange, ng = C.c_void_p(None), C.c_void_p(None), C.c_size_t(0)
        check(lib().impg_gpu_selftest_bed_rows(self._h, a.ctypes.data, rr.ctypes.data, a.size, n_ranges, n_seq, merge_distance,
                                               int(bool(merge_strands)), int(bool(original_sequence_coordinates)), arr,
                                               C.byref(merged), C.byref(nm), C.byref(text), C.byref(ln),
                                               C.byref(grows) if gap else None, C.byref(grange) if gap else None, C.byref(ng) if gap else None))
        try:
            out = np.frombuffer(C.string_at(merged, nm.value * _lib.BED_ROW_DTYPE.itemsize), dtype=_lib.BED_ROW_DTYPE).copy()
            txt = C.string_at(text, ln.value)
            if gap:
                gr = np.frombuffer(C.string_at(grows, ng.value * INTERVAL_DTYPE.itemsize), dtype=INTERVAL_DTYPE).copy()
                gq = np.frombuffer(C.string_at(grange, ng.value * 4), dtype=np.uint32).copy()
        finally:
            _lib.free(merged)
            _lib.free(text)
            if gap:
                _lib.free(grows)
                _lib.free(grange)
        return (out, txt, gr, gq) if gap else (out, txt)

    def bedpe_rows(self, rows, row_range, n_ranges, cigars, merge_distance=0, original_sequence_coordinates=False, range_names=None):
        """impg_gpu_selftest_bedpe_rows (diagnostics): the device BEDPE merge and text of query_batch_bedpe on the caller's
        rows (INTERVAL_DTYPE, grouped by range: row_range[i] = the range of rows[i], its first row the one that is dropped)
        and their packed CIGAR ops (cigars[i]: uint32 array of rows[i]).  Returns the text as bytes."""
        return self._selftest_cigar_rows(lib().impg_gpu_selftest_bedpe_rows, rows, row_range, n_ranges, cigars, merge_distance,
                                         original_sequence_coordinates, range_names)

    def selftest_paf_rows(self, rows, row_range, n_ranges, cigars, merge_distance=0, original_sequence_coordinates=False, range_names=None):
        """impg_gpu_selftest_paf_rows (diagnostics): the device PAF merge, CIGAR fusing and text of query_batch_paf on the
        caller's rows and ops, given as for bedpe_rows.  Returns the text as bytes."""
        return self._selftest_cigar_rows(lib().impg_gpu_selftest_paf_rows, rows, row_range, n_ranges, cigars, merge_distance,
                                         original_sequence_coordinates, range_names)

    def _selftest_cigar_rows(self, entry, rows, row_range, n_ranges, cigars, merge_distance, original_sequence_coordinates, range_names):
        a = np.ascontiguousarray(rows, dtype=INTERVAL_DTYPE)
        rr = np.ascontiguousarray(row_range, dtype=np.uint32)
        if a.size != rr.size or a.size != len(cigars):
            raise _lib.ImpgGpuError(_lib.IMPG_E_INVALID, "one range index and one CIGAR per row")
        off = np.zeros(a.size + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(cg) for cg in cigars], dtype=np.uint64)
        ops = np.ascontiguousarray(np.concatenate([np.asarray(cg, dtype=np.uint32) for cg in cigars] + [np.zeros(0, dtype=np.uint32)]))
        arr = None
        if range_names is not None:
            arr = (C.c_char_p * len(range_names))(*[None if s is None else (s if isinstance(s, bytes) else s.encode()) for s in range_names])
        text, ln = C.c_void_p(None), C.c_size_t(0)
        check(entry(self._h, a.ctypes.data, rr.ctypes.data, a.size, n_ranges, off.ctypes.data, ops.ctypes.data, merge_distance,
                    int(bool(original_sequence_coordinates)), arr, C.byref(text), C.byref(ln)))
        try:
            return C.string_at(text, ln.value)
        finally:
            _lib.free(text)

    def approximate(self):
        """True for an index built from tracepoints (every answer is the reference's approximate mode)."""
        return bool(lib().impg_gpu_index_approximate(self._h))

    def _check_mode(self, approximate_mode):
        # The reference takes approximate_mode per call (impg.rs:1899): on a CIGAR index it then finds no tracepoints
        # and skips every hit, on a tracepoint index without it it realigns (WFA, not built here).  Answering in the
        # index's own mode instead would hand a caller ported from the trait different rows without a word.
        # None (the default) = the index's own mode; only an explicit mismatch is refused, as the C entry points do
        # through params (impg_gpu_index_approximate, IMPG_E_UNSUPPORTED).
        if approximate_mode is not None and bool(approximate_mode) != self.approximate():
            raise ImpgGpuError(IMPG_E_UNSUPPORTED, "approximate_mode=%s on an index built from %s" %
                               (bool(approximate_mode), "tracepoints" if self.approximate() else "CIGARs"))

    def query(self, target_id, range_start, range_end, store_cigar=False, min_gap_compressed_identity=None,
              sequence_index=None, approximate_mode=None):
        """ImpgIndex::query (impg_index.rs:26-35)."""
        # approximate_mode is a property of the index here: one built from tracepoints (from_tracepoints) answers
        # in approximate mode, one built from CIGARs in exact mode; a call that asks for the other mode is refused
        self._check_mode(approximate_mode)
        p = make_params(transitive=False, store_cigar=store_cigar, min_identity=min_gap_compressed_identity)
        return self.query_batch([(target_id, range_start, range_end)], p)[0]

    def query_transitive_bfs(self, target_id, range_start, range_end, masked_regions=None, max_depth=2,
                             min_transitive_len=101, min_distance_between_ranges=10, min_output_length=None,
                             store_cigar=False, min_gap_compressed_identity=None, sequence_index=None,
                             approximate_mode=None, subset_filter=None):
        """ImpgIndex::query_transitive_bfs (impg_index.rs:79-94)."""
        self._check_mode(approximate_mode)
        p = make_params(True, False, max_depth, min_transitive_len, min_distance_between_ranges, min_output_length,
                        min_gap_compressed_identity, store_cigar)
        return self.query_batch([(target_id, range_start, range_end)], p, masked_regions=masked_regions,
                                subset_keep=subset_filter)[0]

    def query_transitive_dfs(self, target_id, range_start, range_end, masked_regions=None, max_depth=2,
                             min_transitive_len=101, min_distance_between_ranges=10, min_output_length=None,
                             store_cigar=False, min_gap_compressed_identity=None, sequence_index=None,
                             approximate_mode=None, subset_filter=None):
        """ImpgIndex::query_transitive_dfs (impg_index.rs:63-77)."""
        self._check_mode(approximate_mode)
        p = make_params(True, True, max_depth, min_transitive_len, min_distance_between_ranges, min_output_length,
                        min_gap_compressed_identity, store_cigar)
        return self.query_batch([(target_id, range_start, range_end)], p, masked_regions=masked_regions,
                                subset_keep=subset_filter)[0]

    def query_batch_stats(self, ranges, params=None, counts=True, checksums=True, device_ptr=None, n=None, **kw):
        """Throughput form: results stay in HBM; returns (Stats, counts, checksums)."""
        p = params or make_params(**kw)
        st = Stats()
        if device_ptr is None:
            r = self._ranges(ranges)
            n = r.size
        cnt = np.zeros(n, dtype=np.uint64) if counts else None
        ck = np.zeros(n, dtype=np.uint64) if checksums else None
        cp = cnt.ctypes.data if counts else None
        kp = ck.ctypes.data if checksums else None
        if device_ptr is None:
            check(lib().impg_gpu_query_batch_stats(self._h, r.ctypes.data, n, C.byref(p), cp, kp, C.byref(st)))
        else:
            check(lib().impg_gpu_query_batch_stats_dev(self._h, device_ptr, n, C.byref(p), cp, kp, C.byref(st)))
        return st, cnt, ck

    def query_batch_device(self, ranges, params=None, device_ptr=None, n=None, layout=_lib.ROWS_ATTRIBUTED, **kw):
        """impg_gpu_query_batch_device: every result row left in HBM, attributable (DeviceRows).  device_ptr / n: the
        ranges are already on the device."""
        p = params or make_params(**kw)
        h = C.c_void_p(None)
        if device_ptr is None:
            r = self._ranges(ranges)
            n = r.size
            check(lib().impg_gpu_query_batch_device(self._h, r.ctypes.data, r.size, 0, C.byref(p), layout, C.byref(h)))
        else:
            check(lib().impg_gpu_query_batch_device(self._h, device_ptr, n, 1, C.byref(p), layout, C.byref(h)))
        return DeviceRows(h, self, n)

    def hop_profile(self, reset=True):
        """impg_gpu_index_hop_profile: array [shards][8 hops][12 fields] (HOP_PROFILE_FIELDS), zeros for a plain index."""
        n = C.c_size_t(0)
        check(lib().impg_gpu_index_hop_profile(self._h, None, 0, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.float64)
        if n.value:
            check(lib().impg_gpu_index_hop_profile(self._h, out.ctypes.data, out.size, 1 if reset else 0, C.byref(n)))
        return out[:n.value].reshape(-1, 8, 12)

    def shard_info(self):
        """(rank, world, lanes, owner[num_seqs]) of a sharded index; rank -1 = a multi-GPU handle; (0, 1, 1, None) = plain."""
        r, w, l = C.c_int(0), C.c_int(1), C.c_int(1)
        owner = np.zeros(self.num_seqs(), dtype=np.uint32)
        check(lib().impg_gpu_index_shard_info(self._h, C.byref(r), C.byref(w), C.byref(l), owner.ctypes.data, owner.size))
        return r.value, w.value, l.value, (owner if w.value > 1 or r.value != 0 else None)


HOP_PROFILE_FIELDS = ["hops", "route_s", "gather_sizes_s", "records_out_s", "owner_expand_s", "gather_hits_s", "hits_home_s", "reorder_s",
                      "bytes_records_out", "bytes_hits_out", "records_in", "hits_home"]


SELECTION_MODES = {"longest": _lib.SELECT_LONGEST, "total": _lib.SELECT_TOTAL, "sample": _lib.SELECT_SAMPLE,
                   "haplotype": _lib.SELECT_HAPLOTYPE}


def parse_selection_mode(mode):
    """'longest' | 'total' | 'sample[,sep]' | 'haplotype[,sep]' -> (IMPG_SELECT_*, separator) (partition.rs:724-805)."""
    kind, _, sep = mode.partition(",")
    if kind not in SELECTION_MODES or (sep and kind in ("longest", "total")):
        raise ValueError("Invalid selection mode. Must be 'longest', 'total', 'sample[,sep]', or 'haplotype[,sep]'.")
    return SELECTION_MODES[kind], (sep or "#")


def _names_array(names):
    return (C.c_char_p * len(names))(*[n.encode() for n in names])


class Regions:
    """masked_regions / missing_regions of `impg partition` (impg_gpu_regions_t): in HBM, or on the host
    (on_host=True: the host twin, no GPU needed)."""

    def __init__(self, seq_len=None, on_host=False, device=0, _borrowed=None, _owner=None):
        self._owner = _owner
        self._own = _borrowed is None
        if _borrowed is not None:
            self._h = _borrowed
            self.n_seq = _owner.index.num_seqs()
            return
        sl = np.ascontiguousarray(seq_len, dtype=np.int64)
        self.n_seq = int(sl.size)
        h = C.c_void_p()
        _lib.check(_lib.lib().impg_gpu_regions_create(sl.ctypes.data, sl.size, int(on_host), device, C.byref(h)))
        self._h = h

    def apply(self, rows, merge_distance, min_missing_size=3000, min_boundary_distance=3000, device_ptr=None, n=None):
        """One window's update on rows (INTERVAL_DTYPE); returns the window's [(seq_id, start, end)].  device_ptr / n:
        the rows are already on the device (impg_gpu_regions_apply_device)."""
        k = C.c_size_t(0)
        if device_ptr is not None:
            cap = max(16, 2 * n)
            out = np.zeros(cap, dtype=_lib.PARTITION_ROW_DTYPE)
            _lib.check(_lib.lib().impg_gpu_regions_apply_device(self._h, device_ptr, n, merge_distance, min_missing_size,
                                                                min_boundary_distance, out.ctypes.data, cap, C.byref(k)))
            return self._rows(out, k.value)
        a = np.ascontiguousarray(rows, dtype=_lib.INTERVAL_DTYPE)
        cap = max(16, 2 * a.size)
        out = np.zeros(cap, dtype=_lib.PARTITION_ROW_DTYPE)
        _lib.check(_lib.lib().impg_gpu_regions_apply(self._h, a.ctypes.data, a.size, merge_distance, min_missing_size,
                                                     min_boundary_distance, out.ctypes.data, cap, C.byref(k)))
        return self._rows(out, k.value)

    def _rows(self, out, n):
        """The first n rows of `out`, or -- more than it holds -- the rows the object kept, fetched whole."""
        if n > out.size:
            out = np.zeros(n, dtype=_lib.PARTITION_ROW_DTYPE)
            m = C.c_size_t(0)
            _lib.check(_lib.lib().impg_gpu_regions_last_rows(self._h, out.ctypes.data, n, C.byref(m)))
            n = m.value
        return [(int(r["seq_id"]), int(r["start"]), int(r["end"])) for r in out[:n]]

    def get(self, which):
        """{seq id: [(start, end), ...]} of the masked ('masked') or missing ('missing') map; empty lists included."""
        w = {"masked": _lib.REGIONS_MASKED, "missing": _lib.REGIONS_MISSING}[which]
        off = np.zeros(self.n_seq + 1, dtype=np.uint64)
        n = C.c_size_t(0)
        _lib.check(_lib.lib().impg_gpu_regions_get(self._h, w, off.ctypes.data, None, 0, C.byref(n)))
        rng = np.zeros((max(n.value, 1), 2), dtype=np.int32)
        _lib.check(_lib.lib().impg_gpu_regions_get(self._h, w, off.ctypes.data, rng.ctypes.data, n.value, C.byref(n)))
        return {s: [(int(a), int(b)) for a, b in rng[int(off[s]):int(off[s + 1])]] for s in range(self.n_seq)}

    def select(self, mode, window_size, names=None):
        sel, sep = parse_selection_mode(mode)
        arr = _names_array(names) if names is not None else None
        cap = 1 << 10
        while True:
            w = np.zeros(cap, dtype=_lib.RANGE_DTYPE)
            n = C.c_size_t(0)
            _lib.check(_lib.lib().impg_gpu_regions_select(self._h, sel, sep.encode(), arr, window_size, w.ctypes.data, cap, C.byref(n)))
            if n.value <= cap:
                return [(int(r["target_id"]), int(r["start"]), int(r["end"])) for r in w[:n.value]]
            cap = n.value

    def close(self):
        if getattr(self, "_h", None) and self._own:
            _lib.lib().impg_gpu_regions_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass


def starting_windows(seq_ids, seq_len, window_size):
    ids = np.ascontiguousarray(seq_ids, dtype=np.uint32)
    sl = np.ascontiguousarray(seq_len, dtype=np.int64)
    cap = int(sum(int(sl[i]) // window_size + 1 for i in ids)) + 1
    w = np.zeros(cap, dtype=_lib.RANGE_DTYPE)
    n = C.c_size_t(0)
    _lib.check(_lib.lib().impg_gpu_partition_starting_windows(ids.ctypes.data, ids.size, sl.ctypes.data, sl.size, window_size,
                                                              w.ctypes.data, cap, C.byref(n)))
    return [(int(r["target_id"]), int(r["start"]), int(r["end"])) for r in w[:n.value]]


def _flatten_partitions(partitions):
    rows = np.array([(s, a, b) for _, ivs in partitions for s, a, b in ivs], dtype=_lib.PARTITION_ROW_DTYPE)
    num = np.array([p for p, ivs in partitions for _ in ivs], dtype=np.uint64)
    return rows, num


def rehome_singleton_slivers(partitions):
    """[(partition_num, [(seq, start, end), ...])] -> the same after rehome_singleton_slivers (partition.rs:45-156)."""
    rows, num = _flatten_partitions(partitions)
    _lib.check(_lib.lib().impg_gpu_partition_rehome(rows.ctypes.data, num.ctypes.data, rows.size))
    out = []
    for r, p in zip(rows, num):
        if not out or out[-1][0] != int(p):
            out.append((int(p), []))
        out[-1][1].append((int(r["seq_id"]), int(r["start"]), int(r["end"])))
    return out


def partitions_bed_text(partitions, names):
    """write_single_partition_file's text (partition.rs:1682-1717)."""
    rows, num = _flatten_partitions(partitions)
    text = C.c_void_p()
    ln = C.c_size_t(0)
    _lib.check(_lib.lib().impg_gpu_partition_bed_text(rows.ctypes.data, num.ctypes.data, rows.size, _names_array(names), len(names),
                                                      C.byref(text), C.byref(ln)))
    try:
        return C.string_at(text, ln.value).decode()
    finally:
        _lib.free(text)


def entity_ids(names, level, separator="#"):
    """PanSN entity ids of sequence names for level 'sample' / 'haplotype' (impg_gpu_entity_ids): a uint32 array,
    _lib.NO_ENTITY for a name without a key, and the number of entities."""
    lv = {"sample": _lib.SELECT_SAMPLE, "haplotype": _lib.SELECT_HAPLOTYPE}[level]
    out = np.zeros(len(names), dtype=np.uint32)
    n = C.c_uint32(0)
    _lib.check(_lib.lib().impg_gpu_entity_ids(_names_array(names), len(names), lv, separator.encode(), out.ctypes.data, C.byref(n)))
    return out, n.value


def support_rows(rows, offsets, candidates, n_seq, span_bp=1000, merge_distance=0, entity_of=None, max_entities=None, blacklist=None,
                 on_host=False, device=0, survivors=True, stats=None):
    """The boundary support of `impg refine` (impg_gpu_support_rows) for a batch of candidates: rows (INTERVAL_DTYPE) with
    offsets[n_cand + 1], candidates [(target_id, start, end)], blacklist {seq_id: [(start, end), ...]}.  Returns the
    counts, and with survivors=True also [[(seq_id, q_lo, q_hi), ...] per candidate].  on_host=True: the host twin.
    stats: a dict that receives 'longest_group'."""
    a = np.ascontiguousarray(rows, dtype=_lib.INTERVAL_DTYPE)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    cand = GpuImpg._ranges(candidates)
    if off.size != cand.size + 1:
        raise ValueError("offsets must hold one entry more than there are candidates")
    ent = None if entity_of is None else np.ascontiguousarray(entity_of, dtype=np.uint32)
    mx = None if max_entities is None else np.ascontiguousarray(max_entities, dtype=np.uint32)
    if (ent is not None and ent.size != n_seq) or (mx is not None and mx.size != cand.size):
        raise ValueError("entity_of holds one entry per sequence, max_entities one per candidate")
    bo, br = _blacklist_table(blacklist, n_seq)
    opts = _lib.SupportOpts(span_bp, merge_distance)
    count = np.zeros(max(cand.size, 1), dtype=np.uint32)
    soff = np.zeros(cand.size + 1, dtype=np.uint64)
    sv = C.c_void_p()
    longest = C.c_uint64(0)
    ptr = lambda x: None if x is None else x.ctypes.data
    _lib.check(_lib.lib().impg_gpu_support_rows(a.ctypes.data, off.ctypes.data, cand.ctypes.data, cand.size, n_seq, ptr(ent), ptr(mx), ptr(bo), ptr(br),
                                                C.byref(opts), int(on_host), device, count.ctypes.data, soff.ctypes.data if survivors else None,
                                                C.byref(sv) if survivors else None, C.byref(longest)))
    if stats is not None:
        stats["longest_group"] = longest.value
    counts = [int(v) for v in count[:cand.size]]
    if not survivors:
        return counts
    try:
        n = int(soff[-1])
        flat = np.frombuffer(C.string_at(sv, n * _lib.SURVIVOR_DTYPE.itemsize), dtype=_lib.SURVIVOR_DTYPE) if n else []
        flat = [(int(r["seq_id"]), int(r["q_lo"]), int(r["q_hi"])) for r in flat]
    finally:
        _lib.free(sv)
    return counts, [flat[int(soff[c]):int(soff[c + 1])] for c in range(cand.size)]


def _blacklist_table(blacklist, n_seq):
    """{seq_id: [(start, end), ...]} -> (u32 off[n_seq + 1], int32 (start, end) pairs), or (None, None)."""
    if blacklist is None:
        return None, None
    off = np.zeros(n_seq + 1, dtype=np.uint32)
    flat = []
    for s in range(n_seq):
        flat.extend(blacklist.get(s, ()))
        off[s + 1] = len(flat)
    return off, (np.array(flat, dtype=np.int32).reshape(-1, 2) if flat else np.zeros((1, 2), dtype=np.int32))


class RefineResult:
    """The records of a refine run (impg_gpu_refine_t): dicts with the reference's RefineRecord fields -- target_id,
    chrom, refined_start / _end, original_start / _end, label, left_extension / right_extension (applied_*),
    support_count, original_support_count, survivors [(seq_id, q_lo, q_hi)] (support_entities)."""

    def __init__(self, handle, names, labels):
        L = _lib.lib()
        self.names, self.labels = names, labels
        n = L.impg_gpu_refine_num_records(handle)
        recs = np.frombuffer(C.string_at(L.impg_gpu_refine_records(handle), n * _lib.REFINE_RECORD_DTYPE.itemsize),
                             dtype=_lib.REFINE_RECORD_DTYPE) if n else []
        off = np.frombuffer(C.string_at(L.impg_gpu_refine_survivor_offsets(handle), (n + 1) * 8), dtype=np.uint64)
        ns = int(off[-1])
        sv = np.frombuffer(C.string_at(L.impg_gpu_refine_survivors(handle), ns * _lib.SURVIVOR_DTYPE.itemsize),
                           dtype=_lib.SURVIVOR_DTYPE) if ns else []
        sv = [(int(r["seq_id"]), int(r["q_lo"]), int(r["q_hi"])) for r in sv]
        p, c, k = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.impg_gpu_refine_stats(handle, C.byref(p), C.byref(c), C.byref(k))
        self.passes, self.candidates, self.parts = p.value, c.value, k.value
        nt = C.c_size_t(0)
        bt = np.zeros(64, dtype=np.float64)
        _lib.check(L.impg_gpu_refine_batch_times(handle, bt.ctypes.data, bt.size, C.byref(nt)))
        # per batch: candidates, seconds in the query call, the engine's milliseconds inside it, seconds in the support
        self.batch_times = [dict(candidates=int(r[0]), query_s=float(r[1]), engine_ms=float(r[2]), support_s=float(r[3]))
                            for r in bt[:min(nt.value, bt.size)].reshape(-1, 4)]
        self.records = []
        for i, r in enumerate(recs):
            d = {f: int(r[f]) for f in _lib.REFINE_RECORD_DTYPE.names}
            d["chrom"] = names[d["target_id"]] if names else None
            d["label"] = labels[i] if labels else ""
            d["survivors"] = sv[int(off[i]):int(off[i + 1])]
            self.records.append(d)
        self.text, self.support_text = None, None
        if names:
            t, s = C.c_void_p(), C.c_void_p()
            tl, sl = C.c_size_t(0), C.c_size_t(0)
            lab = (C.c_char_p * max(n, 1))(*[(x or "").encode() for x in (labels or [""] * n)])
            _lib.check(L.impg_gpu_refine_text(handle, _names_array(names), len(names), lab, C.byref(t), C.byref(tl), C.byref(s), C.byref(sl)))
            try:
                self.text, self.support_text = C.string_at(t, tl.value).decode(), C.string_at(s, sl.value).decode()
            finally:
                _lib.free(t)
                _lib.free(s)

    def __len__(self):
        return len(self.records)

    def __getitem__(self, i):
        return self.records[i]


def _refine_opts(span_bp, max_extension, extension_step, merge_distance, use_max, on_host):
    return _lib.RefineOpts(span_bp, float(max_extension), extension_step, merge_distance, int(use_max), int(on_host))


def refine_rows(query, seq_len, loci, span_bp=1000, max_extension=0.5, extension_step=1000, merge_distance=0, entity_of=None,
                max_entities=None, blacklist=None, on_host=True, device=0, names=None, labels=None):
    """The refine search over the caller's own row source (impg_gpu_refine_rows): query(regions) -> one array of rows
    (INTERVAL_DTYPE) per region [(target_id, start, end)], in emission order.  on_host=True needs no GPU."""
    sl = np.ascontiguousarray(seq_len, dtype=np.int64)
    lo = GpuImpg._ranges(loci)
    ent = None if entity_of is None else np.ascontiguousarray(entity_of, dtype=np.uint32)
    mx = None if max_entities is None else np.ascontiguousarray(max_entities, dtype=np.uint32)
    bo, br = _blacklist_table(blacklist, sl.size)
    keep = {}
    err = []

    def cb(ctx, regions, n, rows_out, off_out):
        try:
            reg = np.frombuffer(C.string_at(regions, n * RANGE_DTYPE.itemsize), dtype=RANGE_DTYPE)
            per = [np.ascontiguousarray(r, dtype=_lib.INTERVAL_DTYPE) for r in query([(int(r["target_id"]), int(r["start"]), int(r["end"])) for r in reg])]
            keep["off"] = np.concatenate([[0], np.cumsum([p.size for p in per])]).astype(np.uint64)
            keep["rows"] = np.concatenate(per) if per else np.zeros(0, dtype=_lib.INTERVAL_DTYPE)
            if keep["rows"].size == 0:
                keep["rows"] = np.zeros(1, dtype=_lib.INTERVAL_DTYPE)
            rows_out[0] = keep["rows"].ctypes.data
            off_out[0] = keep["off"].ctypes.data
            return 0
        except Exception as e:  # nothing unwinds through the library
            err.append(e)
            return 1

    ptr = lambda x: None if x is None else x.ctypes.data
    opts = _refine_opts(span_bp, max_extension, extension_step, merge_distance, False, on_host)
    h = C.c_void_p()
    rc = _lib.lib().impg_gpu_refine_rows(_lib.ROWS_CB(cb), None, sl.ctypes.data, sl.size, lo.ctypes.data, lo.size, C.byref(opts), ptr(ent), ptr(mx),
                                         ptr(bo), ptr(br), device, C.byref(h))
    if err:
        raise err[0]
    _lib.check(rc)
    try:
        return RefineResult(h, names, labels)
    finally:
        _lib.lib().impg_gpu_refine_free(h)


class PartitionSession:
    """partition_alignments over an index (impg_gpu_partition_t); see GpuImpg.partition."""

    def __init__(self, index, params, window_size, merge_distance, min_missing_size=3000, min_boundary_distance=3000,
                 selection_mode="longest", starting_sequences=None, rehome_singletons=True, state_on_host=False):
        sel, sep = parse_selection_mode(selection_mode)
        self.index = index
        self._sep = sep.encode()
        o = _lib.PartitionOpts(window_size, merge_distance, min_missing_size, min_boundary_distance, sel, self._sep,
                               int(rehome_singletons), int(state_on_host))
        ids = None
        if starting_sequences:
            ids = np.array([s if isinstance(s, (int, np.integer)) else index.seq_id(s) for s in starting_sequences], dtype=np.uint32)
        h = C.c_void_p()
        _lib.check(_lib.lib().impg_gpu_partition_create(index._h, C.byref(params), C.byref(o), None if ids is None else ids.ctypes.data,
                                                        0 if ids is None else ids.size, C.byref(h)))
        self._h = h

    def next_windows(self):
        cap = 1 << 10
        while True:
            w = np.zeros(cap, dtype=_lib.RANGE_DTYPE)
            n = C.c_size_t(0)
            _lib.check(_lib.lib().impg_gpu_partition_next_windows(self._h, w.ctypes.data, cap, C.byref(n)))
            if n.value <= cap:
                return [(int(r["target_id"]), int(r["start"]), int(r["end"])) for r in w[:n.value]]
            cap = n.value

    def window(self, seq_id, start, end, cap=1 << 12):
        w = np.array([(seq_id, start, end)], dtype=_lib.RANGE_DTYPE)
        out = np.zeros(cap, dtype=_lib.PARTITION_ROW_DTYPE)
        n = C.c_size_t(0)
        _lib.check(_lib.lib().impg_gpu_partition_window(self._h, w.ctypes.data, out.ctypes.data, cap, C.byref(n)))
        return self.regions()._rows(out, n.value)

    def run_text(self, separate_files=False):
        """The whole loop; returns (partitions.bed text, number of partitions)."""
        text = C.c_void_p()
        ln = C.c_size_t(0)
        k = C.c_uint64(0)
        _lib.check(_lib.lib().impg_gpu_partition_run(self._h, None, int(separate_files), C.byref(text), C.byref(ln), C.byref(k)))
        try:
            return C.string_at(text, ln.value).decode(), int(k.value)
        finally:
            _lib.free(text)

    def run_files(self, folder, separate_files=False):
        k = C.c_uint64(0)
        _lib.check(_lib.lib().impg_gpu_partition_run(self._h, None if folder is None else folder.encode(), int(separate_files), None, None,
                                                     C.byref(k)))
        return int(k.value)

    def run_fasta(self, folder):
        """The whole loop with FASTA output (impg_gpu_partition_run_fasta): folder/partition{N}.fasta per partition (None: the
        working directory); returns the number of partitions."""
        k = C.c_uint64(0)
        _lib.check(_lib.lib().impg_gpu_partition_run_fasta(self._h, None if folder is None else os.fsencode(folder), C.byref(k)))
        return int(k.value)

    def window_fasta(self, seq_id, start, end, fd=None):
        """Query, update and FASTA text for one window (impg_gpu_partition_window_fasta) -> (rows, text as bytes); with fd the
        text is written there and None returned in its place.  No rows: no partition, no text (b"" / nothing written)."""
        w = np.array([(seq_id, start, end)], dtype=_lib.RANGE_DTYPE)
        n, ln, text = C.c_size_t(0), C.c_size_t(0), C.c_void_p(None)
        _lib.check(_lib.lib().impg_gpu_partition_window_fasta(self._h, w.ctypes.data, -1 if fd is None else fd,
                                                              C.byref(text) if fd is None else None, C.byref(ln), C.byref(n)))
        try:
            rows = self.regions()._rows(np.zeros(0, dtype=_lib.PARTITION_ROW_DTYPE), n.value)
            return rows, (None if fd is not None else _text_bytes(text, ln.value) if n.value else b"")
        finally:
            if text:
                _lib.free(text)

    def regions(self):
        return Regions(_borrowed=C.c_void_p(_lib.lib().impg_gpu_partition_regions(self._h)), _owner=self)

    def counter(self, key):
        v = C.c_int64(0)
        _lib.check(_lib.lib().impg_gpu_partition_counter(self._h, key.encode(), C.byref(v)))
        return int(v.value)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().impg_gpu_partition_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass


def shard_assign(entries_per_target, n_shards):
    """impg_gpu_shard_assign: owner shard of every target (greedy bin-packing by entry count); host-only."""
    c = np.ascontiguousarray(entries_per_target, dtype=np.uint64)
    out = np.zeros(c.size, dtype=np.uint32)
    check(lib().impg_gpu_shard_assign(c.ctypes.data, c.size, n_shards, out.ctypes.data))
    return out


class Comm:
    """impg_gpu_comm_t: the transport between the ranks of an index sharded one process per GPU."""

    def __init__(self, handle, rank, world, lanes, keep=None):
        self._h, self.rank, self.world, self.lanes = handle, rank, world, lanes
        self._keep = keep

    @classmethod
    def rccl(cls, rank, world, device, lanes=2, group=None):
        """RCCL communicators (one per lane).  Rank 0 makes the unique ids; torch.distributed (already
        initialised by the launcher) carries them to the other ranks -- plumbing only: every collective of
        a query runs inside libimpg_gpu.so."""
        import torch.distributed as dist
        ids = np.zeros(lanes * _lib.COMM_ID_BYTES, dtype=np.uint8)
        if rank == 0:
            check(lib().impg_gpu_comm_unique_id(ids.ctypes.data, lanes))
        box = [ids.tobytes()]
        if world > 1:
            dist.broadcast_object_list(box, src=0, group=group)
        ids = np.frombuffer(box[0], dtype=np.uint8).copy()
        h = C.c_void_p(None)
        check(lib().impg_gpu_comm_create_rccl(ids.ctypes.data, lanes, rank, world, device, C.byref(h)))
        return cls(h, rank, world, lanes)

    @classmethod
    def host(cls, rank, world, device, groups):
        """The host's own transport (impg_gpu_comm_create_host): one torch.distributed group per lane, moving
        HOST memory (gloo).  What the multi-rank tests use on a box whose ranks share one GPU."""
        import torch
        import torch.distributed as dist
        lanes = len(groups)
        arr = (_lib.HostTransport * lanes)()
        keep = []

        def make(group):
            def allgather(ctx, mine, k, out):
                try:
                    t = torch.from_numpy(np.ctypeslib.as_array(mine, shape=(k,)).astype(np.int64))
                    parts = [torch.empty_like(t) for _ in range(world)]
                    dist.all_gather(parts, t, group=group)
                    dst = np.ctypeslib.as_array(out, shape=(world * k,))
                    for r in range(world):
                        dst[r * k:(r + 1) * k] = parts[r].numpy().astype(np.uint64)
                    return 0
                except Exception as e:  # noqa: BLE001 -- nothing may unwind into C
                    print("host transport allgather failed:", e, flush=True)
                    return 1

            def alltoallv(ctx, send, soff, sbytes, recv, roff, rbytes):
                try:
                    so = [int(soff[d]) for d in range(world)]
                    sb = [int(sbytes[d]) for d in range(world)]
                    ro = [int(roff[d]) for d in range(world)]
                    rb = [int(rbytes[d]) for d in range(world)]
                    st, rt = sum(sb), sum(rb)
                    src = (torch.from_numpy(np.ctypeslib.as_array(C.cast(send, C.POINTER(C.c_uint8)), shape=(st,)).copy())
                           if st else torch.empty(0, dtype=torch.uint8))
                    dst = torch.empty(rt, dtype=torch.uint8)
                    assert so == list(np.cumsum([0] + sb[:-1])) and ro == list(np.cumsum([0] + rb[:-1]))
                    dist.all_to_all_single(dst, src, output_split_sizes=rb, input_split_sizes=sb, group=group)
                    if rt:
                        np.ctypeslib.as_array(C.cast(recv, C.POINTER(C.c_uint8)), shape=(rt,))[:] = dst.numpy()
                    return 0
                except Exception as e:  # noqa: BLE001
                    print("host transport alltoallv failed:", e, flush=True)
                    return 1
            return _lib.ALLGATHER_CB(allgather), _lib.ALLTOALLV_CB(alltoallv)

        for l, g in enumerate(groups):
            ag, aa = make(g)
            keep += [ag, aa]
            arr[l].ctx = None
            arr[l].allgather_u64 = ag
            arr[l].alltoallv = aa
        h = C.c_void_p(None)
        check(lib().impg_gpu_comm_create_host(arr, lanes, rank, world, device, C.byref(h)))
        return cls(h, rank, world, lanes, keep=(arr, keep))

    def check(self):
        """impg_gpu_comm_check on every lane (collective)."""
        for l in range(self.lanes):
            check(lib().impg_gpu_comm_check(self._h, l))

    def kind(self):
        k = C.c_char_p(None)
        check(lib().impg_gpu_comm_info(self._h, None, None, None, C.byref(k)))
        return k.value.decode()

    def close(self):
        if getattr(self, "_h", None):
            lib().impg_gpu_comm_destroy(self._h)
            self._h = None


def _keys(fn):
    out = []
    while (k := fn(len(out))) is not None:
        out.append(k.decode())
    return out


def resolve_cigars(records, ops, names, seq_len, sequences, on_host=False, device=0, tile_bases=None):
    """impg_gpu_cigar_resolve: every 'M' op of the records rewritten as the '=' / 'X' runs that `sequences` spell ->
    (records, ops, flags, report): the records with cigar_off / cigar_len rewritten, the new pool in record order, a flag
    byte per record (0 resolved or without ops, 1 a sequence absent from the store, 2 inconsistent: ops copied) and the
    report as a dict.  names[id] / seq_len[id]: the sequence table.  on_host: the host twin (no device needed);
    tile_bases: impg_gpu_selftest_cigar_resolve's bases per wave (tests; the answer does not depend on it)."""
    rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
    pool = np.ascontiguousarray(ops, dtype=np.uint32)
    sl = np.ascontiguousarray(seq_len, dtype=np.int64)
    if len(names) != sl.size:
        raise _lib.ImpgGpuError(_lib.IMPG_E_INVALID, "one name per sequence length")
    arr = (C.c_char_p * max(len(names), 1))(*[q.encode() if isinstance(q, str) else q for q in names])
    ro, oo, fo, no, rep = C.c_void_p(None), C.c_void_p(None), C.c_void_p(None), C.c_size_t(0), _lib.ResolveReport()
    head = (rec.ctypes.data, rec.size, pool.ctypes.data, pool.size, arr, sl.ctypes.data, sl.size, sequences._h, int(bool(on_host)), device)
    tail = (C.byref(ro), C.byref(oo), C.byref(no), C.byref(fo), C.byref(rep))
    if tile_bases is None:
        check(lib().impg_gpu_cigar_resolve(*head, *tail))
    else:
        check(lib().impg_gpu_selftest_cigar_resolve(*head, int(tile_bases), *tail))
    try:
        out_rec = np.frombuffer(C.string_at(ro, rec.size * RECORD_DTYPE.itemsize), dtype=RECORD_DTYPE).copy()
        out_ops = np.frombuffer(C.string_at(oo, no.value * 4), dtype=np.uint32).copy()
        flags = np.frombuffer(C.string_at(fo, rec.size), dtype=np.uint8).copy()
    finally:
        for q in (ro, oo, fo):
            _lib.free(q)
    return out_rec, out_ops, flags, rep.as_dict()


def option_keys():
    """impg_gpu_option_key: every key GpuImpg.set_option accepts (no GPU needed)."""
    return _keys(lib().impg_gpu_option_key)


def counter_keys():
    """impg_gpu_counter_key: every key GpuImpg.counter accepts (no GPU needed)."""
    return _keys(lib().impg_gpu_counter_key)


def parse_subsequence(name):
    """impg_gpu_parse_subsequence: (base, start offset) of a "base:START-END" name, or None."""
    buf = C.create_string_buffer(len(name.encode()) + 2)
    off = C.c_int32(0)
    r = lib().impg_gpu_parse_subsequence(name.encode(), buf, len(buf), C.byref(off))
    if r < 0:
        check(r)
    return (buf.value.decode(), int(off.value)) if r == 1 else None


def subset_keep(list_text, names):
    """impg_gpu_subset_keep: (uint8 verdict per name, number of list entries) for a --subset-sequence-list text."""
    data = list_text.encode() if isinstance(list_text, str) else bytes(list_text)
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    keep = np.zeros(len(names), dtype=np.uint8)
    n_entries = C.c_size_t(0)
    check(lib().impg_gpu_subset_keep(data, len(data), arr, len(names), keep.ctypes.data, C.byref(n_entries)))
    return keep, int(n_entries.value)


def bed_merge(intervals, merge_distance, merge_strands=True):
    a = np.ascontiguousarray(intervals, dtype=INTERVAL_DTYPE).copy()
    n = lib().impg_gpu_bed_merge(a.ctypes.data, a.size, merge_distance, int(merge_strands))
    if n < 0:
        check(int(n))
    return a[:n].copy()


def parse_cigar(s):
    b = s.encode() if isinstance(s, str) else s
    out = np.zeros(len(b) + 1, dtype=np.uint32)
    n = lib().impg_gpu_parse_cigar(b, len(b), out.ctypes.data, out.size)
    if n < 0:
        raise ValueError("Invalid CIGAR operation")
    return out[:n].copy()


def parse_target_range(s):
    name = C.create_string_buffer(4096)
    a, b = C.c_int32(0), C.c_int32(0)
    rc = lib().impg_gpu_parse_target_range(s.encode(), name, 4096, C.byref(a), C.byref(b))
    if rc != 0:
        raise ValueError(lib().impg_gpu_last_error().decode())
    return name.value.decode(), a.value, b.value


# ---- synthetic workloads --------------------------------
def synth_paf(seed, n_records, n_seq=200, seq_len=5_000_000, target_span=10_000, n_blocks=100):
    n_ops = C.c_size_t(0)
    check(lib().impg_synth_paf(seed, n_records, n_seq, seq_len, target_span, n_blocks, None, None, 0, C.byref(n_ops)))
    rec = np.zeros(n_records, dtype=RECORD_DTYPE)
    ops = np.zeros(n_ops.value, dtype=np.uint32)
    check(lib().impg_synth_paf(seed, n_records, n_seq, seq_len, target_span, n_blocks, rec.ctypes.data, ops.ctypes.data,
                               ops.size, C.byref(n_ops)))
    return rec, ops, np.full(n_seq, seq_len, dtype=np.int64)


def synth_paf_text(path, seed, n_records, n_seq=200, seq_len=5_000_000, target_span=10_000, n_blocks=100):
    check(lib().impg_synth_paf_text(seed, n_records, n_seq, seq_len, target_span, n_blocks, path.encode()))
    return path


def synth_skewed_paf_text(path, seed, n_records, n_seq=200, seq_len=5_000_000):
    """impg_synth_skewed_paf_text: log-normal alignment lengths, 1 % of the sequences holding ~30 % of the entries; returns the ops written."""
    n = C.c_uint64(0)
    check(lib().impg_synth_skewed_paf_text(seed, n_records, n_seq, seq_len, path.encode(), C.byref(n)))
    return int(n.value)


def synth_seq_name(i):
    b = C.create_string_buffer(64)
    lib().impg_synth_seq_name(i, b, 64)
    return b.value.decode()


def synth_bed(seed, n, n_seq=200, seq_len=5_000_000, range_len=5_000):
    out = np.zeros(n, dtype=RANGE_DTYPE)
    check(lib().impg_synth_bed(seed, n, n_seq, seq_len, range_len, out.ctypes.data))
    return out


# ---- the device primitives on the caller's arrays (diagnostics; tests/test_gpu_prims.py) ---------------------------
SCAN_LOOKBACK, SCAN_THREE_KERNEL, SCAN_SMALL = 0, 1, 2


def selftest_scan(values, which=0, in_shift=0, out_shift=0, device=0):
    """impg_gpu_selftest_scan: the engine's exclusive scan (which=0) or the small-batch path's single-block one (which=1)
    of `values` (u32), the device arrays in_shift / out_shift words behind a 256-byte boundary.  Returns (out, total, info):
    the offsets written, the total, and info = dict(form, in_low4, out_low4, lookback_tile, three_kernel_tile)."""
    a = np.ascontiguousarray(values, dtype=np.uint32)
    out = np.empty(a.size, dtype=np.uint32)
    total = C.c_uint64(0)
    info = np.zeros(5, dtype=np.uint32)
    check(lib().impg_gpu_selftest_scan(device, which, a.ctypes.data, a.size, in_shift, out_shift, out.ctypes.data, C.byref(total),
                                       info.ctypes.data))
    return out, int(total.value), dict(zip(("form", "in_low4", "out_low4", "lookback_tile", "three_kernel_tile"), map(int, info)))


def selftest_offsets(lengths, with_host_copy=False, device=0):
    """impg_gpu_selftest_offsets: the 64-bit offsets of `lengths` (u32) and their total, by prims::offsets_and_total --
    with_host_copy: through the form that copies the offsets home itself."""
    a = np.ascontiguousarray(lengths, dtype=np.uint32)
    off = np.empty(a.size, dtype=np.uint64)
    total = C.c_uint64(0)
    check(lib().impg_gpu_selftest_offsets(device, a.ctypes.data, a.size, int(with_host_copy), off.ctypes.data, C.byref(total)))
    return off, int(total.value)


def selftest_key_sort(n_keys, perm, passes, first_in_order, device=0):
    """impg_gpu_selftest_key_sort: prims::KeySort::run over passes = [(keys, bits), ...], least significant first; keys:
    n_keys of uint32 or (a wide pass) uint64, at the rows' own indices.  Returns (order, sorted_keys)."""
    p = np.ascontiguousarray(perm, dtype=np.uint32)
    arrays = [np.ascontiguousarray(k) for k, _ in passes]
    for k in arrays:
        if k.dtype not in (np.uint32, np.uint64) or k.size != n_keys:
            raise ValueError("a pass's keys are n_keys of uint32 or uint64")
    sp = (_lib.SortPass * len(passes))(*[_lib.SortPass(k.ctypes.data, int(k.dtype == np.uint64), bits)
                                         for k, (_, bits) in zip(arrays, passes)])
    order = np.empty(p.size, dtype=np.uint32)
    sorted_keys = np.empty(p.size, dtype=arrays[-1].dtype)
    check(lib().impg_gpu_selftest_key_sort(device, n_keys, p.ctypes.data, p.size, int(first_in_order), C.cast(sp, C.c_void_p), len(passes),
                                           order.ctypes.data, sorted_keys.ctypes.data))
    return order, sorted_keys


def selftest_sequence_reader(path, piece_bytes):
    """impg_gpu_selftest_sequence_reader (host-only): the reader of load_sequences alone -> (the concatenation of the file's
    pieces, their number, the BGZF blocks inflated)."""
    text, ln, pieces, blocks = C.c_void_p(None), C.c_size_t(0), C.c_uint64(0), C.c_uint64(0)
    check(lib().impg_gpu_selftest_sequence_reader(os.fsencode(path), piece_bytes, C.byref(text), C.byref(ln), C.byref(pieces), C.byref(blocks)))
    try:
        return _text_bytes(text, ln.value), pieces.value, blocks.value
    finally:
        _lib.free(text)


def selftest_sequence_ingest_host(paths, names, lens, piece_bytes, packed):
    """impg_gpu_selftest_sequence_ingest_host (host-only): load_sequences with the kernels' host twin in their place, for an
    index whose ids are names / lens -> dict(off=[n_ids] uint64 (all ones: absent), store=uint8 bytes or packed stream,
    run_off=[n_ids + 1], run_start, run_end, run_byte, stats=[5])."""
    if isinstance(paths, (str, bytes, os.PathLike)):
        paths = [paths]
    n = len(names)
    parr = (C.c_char_p * len(paths))(*[os.fsencode(q) for q in paths])
    narr = (C.c_char_p * n)(*[q.encode() for q in names])
    ln = np.ascontiguousarray(lens, dtype=np.int64)
    off, run_off, stats = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64), np.zeros(5, dtype=np.uint64)
    store, rs, re_, rb, sb = C.c_void_p(None), C.c_void_p(None), C.c_void_p(None), C.c_void_p(None), C.c_size_t(0)
    check(lib().impg_gpu_selftest_sequence_ingest_host(parr, len(paths), narr, ln.ctypes.data, n, piece_bytes, int(bool(packed)), off.ctypes.data,
                                                       C.byref(store), C.byref(sb), run_off.ctypes.data, C.byref(rs), C.byref(re_), C.byref(rb),
                                                       stats.ctypes.data))
    try:
        k = int(run_off[n])
        return dict(off=off[:n], store=np.frombuffer(C.string_at(store, sb.value), dtype=np.uint8), run_off=run_off,
                    run_start=np.frombuffer(C.string_at(rs, 4 * k), dtype=np.uint32), run_end=np.frombuffer(C.string_at(re_, 4 * k), dtype=np.uint32),
                    run_byte=np.frombuffer(C.string_at(rb, k), dtype=np.uint8), stats=stats)
    finally:
        for q in (store, rs, re_, rb):
            _lib.free(q)
