"""impg_gpu_query_batch_fasta (impg_amd/csrc/fasta_device.hip): the query-axis sweep and the FASTA records written on the
device from the sequence store in HBM.  Every text is compared byte for byte with the restatement of tests/fasta_ref.py
(and, on the whole path, with the host twin QueryResults.fasta).  Every case is small."""
import os
import subprocess

import numpy as np
import pytest

import impg_amd
from impg_amd import INTERVAL_DTYPE, Sequences
from oracle import oracle as o
from tests import fasta_ref as ref
from tests.paf_gen import random_paf, random_ranges
from tests.tp_gen import random_tp

pytestmark = pytest.mark.gpu

FASTA_KEYS = ("fasta_rows", "fasta_records", "fasta_text_pieces", "fasta_text_bytes", "fasta_store_bytes")
BED_KEYS = ("bed_rows", "bed_gap_roots", "bed_runs", "bed_text_pieces", "bed_text_bytes")


def write(tmp, name, text):
    path = str(tmp / name)
    with open(path, "w") as f:
        f.write(text)
    return path


# ---- small shapes ---------------------------------------------------------------------------------------------------------
NAMES = ["a", "b", "c"]  # one letter: a record of no bases is ">a:5-5\n\n", 8 bytes -- a lane's 16 bytes can hold three records
SEQ_LEN = 4096
BODY_LENGTHS = [0, 1, 2, 15, 16, 17, 79, 80, 81, 82, 159, 160, 161, 162, 1000]


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """three sequences of 4 096 random bytes behind an index that only has to know their names and lengths"""
    rng = np.random.default_rng(4096)
    seqs = [ref.random_sequence(rng, SEQ_LEN) for _ in NAMES]
    paf = "".join("%s\t%d\t0\t100\t+\t%s\t%d\t0\t100\t100\t100\t60\tcg:Z:100=\n" % (q, SEQ_LEN, t, SEQ_LEN) for q, t in (("a", "b"), ("b", "c")))
    g = impg_amd.GpuImpg.from_paf(write(tmp_path_factory.mktemp("fasta_small"), "small.paf", paf))
    assert [g.seq_name(i) for i in range(3)] == NAMES
    g.set_sequences(Sequences.from_arrays(NAMES, seqs))
    return g, seqs


def crafted_rows():
    """every body length x every residue of the source start mod 16 x both strands, spread over the three sequences; each row
    is its own range, so no two of them merge and the text keeps their order"""
    rows = []
    for k, L in enumerate(BODY_LENGTHS):
        for res in range(16):
            for fwd in (True, False):
                sid = (k + res) % 3
                start = 16 * ((7 * k + 3 * res) % 150) + res
                rows.append((sid, start, start + L) if fwd else (sid, start + L, start))
        for fwd in (True, False):  # ... and at the sequence's first and last bases: the loads reach into the padding
            rows.append((k % 3, 0, L) if fwd else (k % 3, L, 0))
            rows.append((k % 3, SEQ_LEN - L, SEQ_LEN) if fwd else (k % 3, SEQ_LEN, SEQ_LEN - L))
    a = np.zeros(len(rows), dtype=INTERVAL_DTYPE)
    for r, (sid, first, last) in zip(a, rows):
        r["query_id"], r["q_first"], r["q_last"] = sid, first, last
        r["target_id"], r["t_first"], r["t_last"] = sid, 0, abs(last - first)
    return a


def restated(rows, row_range, n_ranges, d, rc, seqs):
    return b"".join(ref.fasta_range(rows[row_range == q], d, rc, lambda i: NAMES[i], lambda i: seqs[i]) for q in range(n_ranges))


@pytest.fixture(scope="module")
def small_texts(small):
    """the restatement's text of the crafted rows, one range per row, for either setting of reverse_complement"""
    _, seqs = small
    rows = crafted_rows()
    rr = np.arange(rows.size, dtype=np.uint32)
    return rows, rr, {rc: restated(rows, rr, rows.size, -1, rc, seqs) for rc in (False, True)}


@pytest.mark.parametrize("rc", [False, True])
def test_small_shapes(small, small_texts, rc):
    g, _ = small
    rows, rr, want = small_texts
    g.set_option("bed_text_piece_bytes", 256 << 20)
    got = g.fasta_rows(rows, rr, rows.size, merge_distance=-1, reverse_complement=rc)
    assert got == want[rc]
    assert got.count(b"/rc\n") == (int(np.sum(rows["q_first"] > rows["q_last"])) if rc else 0) and got.count(b">") == rows.size
    have = {k: g.counter(k) for k in FASTA_KEYS}
    assert have["fasta_rows"] == have["fasta_records"] == rows.size == 15 * (16 * 2 + 4)
    assert have["fasta_text_bytes"] == len(got) and have["fasta_text_pieces"] == 1
    assert have["fasta_store_bytes"] >= 3 * SEQ_LEN + 32


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("d", [0, 30])
def test_small_shapes_merged(small, small_texts, d, rc):
    """the same rows as four ranges: the sweep merges what overlaps or lies within d, the strands apart"""
    g, seqs = small
    rows, _, _ = small_texts
    rr = (np.arange(rows.size, dtype=np.uint32) * 7) % 4
    g.set_option("bed_text_piece_bytes", 256 << 20)
    got = g.fasta_rows(rows, rr, 4, merge_distance=d, reverse_complement=rc)
    assert got == restated(rows, rr, 4, d, rc, seqs)
    assert g.counter("fasta_records") == got.count(b">") < rows.size


@pytest.mark.parametrize("piece", [64, 1024])
def test_pieces(small, small_texts, piece):
    """the text in pieces of 64 and 1 024 bytes: identical, and a piece of one record longer than that (the 1 000-base
    records) still fits the buffer's slack"""
    g, _ = small
    rows, rr, want = small_texts
    g.set_option("bed_text_piece_bytes", piece)
    try:
        for rc in (False, True):
            assert g.fasta_rows(rows, rr, rows.size, merge_distance=-1, reverse_complement=rc) == want[rc]
            assert g.counter("fasta_text_pieces") > 1 and g.counter("fasta_text_bytes") == len(want[rc])
    finally:
        g.set_option("bed_text_piece_bytes", 256 << 20)


def test_record_longer_than_the_piece_buffer(whole):
    """64 + 4 096 bytes of buffer do not hold a record of 20 000 bases: refused, and no text is delivered"""
    g = whole[0]
    rows = np.zeros(2, dtype=INTERVAL_DTYPE)
    rows[0]["query_id"], rows[0]["q_first"], rows[0]["q_last"] = 0, 10, 20
    rows[1]["query_id"], rows[1]["q_first"], rows[1]["q_last"] = 1, 0, WHOLE_LEN
    g.set_option("bed_text_piece_bytes", 64)
    try:
        with pytest.raises(impg_amd.ImpgGpuError) as e:
            g.fasta_rows(rows, [0, 1], 2, merge_distance=-1)
        assert e.value.code == impg_amd.IMPG_E_UNSUPPORTED
        assert g.counter("fasta_text_bytes") == 0 and g.counter("fasta_text_pieces") == 0
    finally:
        g.set_option("bed_text_piece_bytes", 256 << 20)


# ---- whole path -----------------------------------------------------------------------------------------------------------
N_SEQ, WHOLE_LEN = 8, 20000


@pytest.fixture(scope="module")
def whole(tmp_path_factory):
    text, names = random_paf(31, 300, n_seq=N_SEQ, seq_len=WHOLE_LEN)
    path = write(tmp_path_factory.mktemp("fasta_whole"), "whole.paf", text)
    g = impg_amd.GpuImpg.from_paf(path)
    c = o.OracleIndex(paf_paths=[path], preparse=True)
    assert [g.seq_name(i) for i in range(N_SEQ)] == [c.seq_name(i) for i in range(N_SEQ)]
    rng = np.random.default_rng(31)
    seqs = {nm: ref.random_sequence(rng, WHOLE_LEN) for nm in names}
    g.set_sequences(Sequences.from_arrays(names, [seqs[nm] for nm in names]))
    ranges = [(g.seq_id(names[t]), s, e) for t, s, e in random_ranges(31, 32, N_SEQ, WHOLE_LEN, max_len=3000, min_len=200)]
    kw = dict(transitive=True, max_depth=2)
    oracle_rows = [c.query(c.seq_id(g.seq_name(t)), s, e, **kw) for t, s, e in ranges]
    g.paf_path = path  # (for the command line's test)
    return g, c, seqs, ranges, kw, oracle_rows


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("d", [-1, 0, 1000])
def test_whole_path(whole, d, rc):
    """32 ranges, -x -m 2: the device route == the host twin == the restatement on the oracle's rows"""
    g, c, seqs, ranges, kw, oracle_rows = whole
    p = impg_amd.make_params(**kw)
    want = b"".join(ref.fasta_range(rows, d, rc, c.seq_name, lambda i: seqs[c.seq_name(i)]) for rows in oracle_rows)
    got = g.query_batch_fasta(ranges, p, merge_distance=d, reverse_complement=rc, raw=True)
    assert got == want
    assert g.counter("fasta_records") == got.count(b">") >= 32
    assert g.counter("fasta_rows") == sum(r.size for r in oracle_rows) and g.counter("fasta_text_bytes") == len(got)
    assert g.query_batch(ranges, p).fasta(merge_distance=d, params=p, reverse_complement=rc, raw=True) == want
    if rc:
        assert b"/rc\n" in got


def test_whole_path_chunks_pieces_and_fd(whole, tmp_path):
    """the same text chunk by chunk, piece by piece and through a file descriptor; --original-sequence-coordinates and range
    names do not touch it"""
    g, c, seqs, ranges, kw, oracle_rows = whole
    want = b"".join(ref.fasta_range(rows, 0, True, c.seq_name, lambda i: seqs[c.seq_name(i)]) for rows in oracle_rows)
    g.set_option("chunk_ranges", 5)
    g.set_option("bed_text_piece_bytes", 1 << 14)
    try:
        p = impg_amd.make_params(original_sequence_coordinates=True, **kw)
        assert g.query_batch_fasta(ranges, p, merge_distance=0, reverse_complement=True, raw=True, range_names=["r%d" % i for i in range(32)]) == want
        assert g.counter("fasta_text_pieces") > 7
        with open(str(tmp_path / "out.fa"), "wb") as f:
            n = g.query_batch_fasta(ranges, p, merge_distance=0, reverse_complement=True, fd=f.fileno())
        assert n == len(want) and open(str(tmp_path / "out.fa"), "rb").read() == want
    finally:
        g.set_option("chunk_ranges", 0)
        g.set_option("bed_text_piece_bytes", 256 << 20)


def test_plain_query_min_output_length(whole):
    """a plain query with -l: the text writers' retain comes before the sweep, on both routes"""
    g, c, seqs, ranges, _, _ = whole
    p = impg_amd.make_params(min_output_length=150)
    want = b""
    for t, s, e in ranges:
        rows = c.query(c.seq_id(g.seq_name(t)), s, e)
        rows = rows[np.abs(rows["q_last"].astype(np.int64) - rows["q_first"]) >= 150]
        want += ref.fasta_range(rows, 10, False, c.seq_name, lambda i: seqs[c.seq_name(i)])
    assert g.query_batch_fasta(ranges, p, merge_distance=10, raw=True) == want
    assert g.query_batch(ranges, p).fasta(merge_distance=10, params=p, raw=True) == want


def test_command_line(whole, tmp_path):
    """`impg-gpu query -o fasta` prints the restatement's bytes by both routes; without sequence files it dies with the
    reference's message (main.rs:4243)"""
    g, c, seqs, ranges, kw, oracle_rows = whole
    cli = os.path.join(os.path.dirname(impg_amd.__file__), "impg-gpu")
    bed, fa, fa2, lst = (str(tmp_path / n) for n in ("q.bed", "a.fa", "b.fa", "files.txt"))
    with open(bed, "w") as f:
        for t, s, e in ranges:
            f.write("%s\t%d\t%d\n" % (g.seq_name(t), s, e))
    names = sorted(seqs)
    for path, part in ((fa, names[:5]), (fa2, names[5:])):  # lower case and lines of 60: the store upper-cases and joins them
        with open(path, "wb") as f:
            for nm in part:
                f.write(b">%s some description\n" % nm.encode())
                f.write(b"".join(seqs[nm][i:i + 60].lower() + b"\n" for i in range(0, WHOLE_LEN, 60)))
    with open(lst, "w") as f:
        f.write(fa + "\n" + fa2 + "\n")
    base = [cli, "query", "-a", g.paf_path, "-b", bed, "-o", "fasta", "-x", "-m", "2"]
    by_files, by_list = ["--sequence-files", fa, fa2], ["--sequence-list", lst]
    for d_args, d, rc, files in ((["-d", "1000"], 1000, True, by_files), (["-d", "1000"], 1000, True, by_list), (["--no-merge"], -1, False, by_files)):
        want = b"".join(ref.fasta_range(rows, d, rc, c.seq_name, lambda i: seqs[c.seq_name(i)]) for rows in oracle_rows)
        for extra in ([], ["--host-merge"]):
            r = subprocess.run(base + d_args + files + (["--reverse-complement"] if rc else []) + extra, capture_output=True)
            assert r.returncode == 0, r.stderr
            assert r.stdout == want, (d, rc, files[0], extra)
    r = subprocess.run(base + ["-d", "0"], capture_output=True, text=True)
    assert r.returncode != 0 and r.stdout == ""
    assert "Sequence files (FASTA/AGC) are required for 'fasta' output format. Use --sequence-files or --sequence-list" in r.stderr


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_bed_unchanged(whole):
    """query_batch_bed's text and its counters do not move when a FASTA call runs between two BED calls"""
    g, _, _, ranges, kw, _ = whole
    p = impg_amd.make_params(**kw)
    for d in (-1, 0, 1000):
        before = g.query_batch_bed(ranges, p, merge_distance=d, raw=True)
        bed_before = {k: g.counter(k) for k in BED_KEYS}
        assert bed_before["bed_rows"] > 0
        g.query_batch_fasta(ranges, p, merge_distance=d, reverse_complement=True, raw=True)
        assert {k: g.counter(k) for k in BED_KEYS} == bed_before
        assert g.query_batch_bed(ranges, p, merge_distance=d, raw=True) == before
        assert {k: g.counter(k) for k in BED_KEYS} == bed_before


def test_refusals(tmp_path):
    text, names = random_paf(32, 120, n_seq=4, seq_len=WHOLE_LEN)
    g = impg_amd.GpuImpg.from_paf(write(tmp_path, "r.paf", text))
    rng = np.random.default_rng(32)
    seqs = [ref.random_sequence(rng, WHOLE_LEN) for _ in names]
    ranges = [(t, 0, WHOLE_LEN) for t in range(4)]
    p = impg_amd.make_params(transitive=True, max_depth=2)
    # no store attached
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        g.query_batch_fasta(ranges, p)
    assert e.value.code == impg_amd.IMPG_E_INVALID
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        g.query_batch(ranges, p).fasta(params=p)
    assert e.value.code == impg_amd.IMPG_E_INVALID
    # a length mismatch at attach: named, and nothing is attached
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        g.set_sequences(Sequences.from_arrays(names, seqs[:3] + [seqs[3][:-1]]))
    assert e.value.code == impg_amd.IMPG_E_INVALID and "'%s'" % names[3] in str(e.value)
    assert g.counter("fasta_store_bytes") == 0
    # a store that lacks a sequence results land on (and holds one the index lacks): the error names it, the text is empty
    g.set_sequences(Sequences.from_arrays(names[:2] + ["elsewhere"] + names[3:], seqs))
    assert g.counter("fasta_store_bytes") >= 3 * WHOLE_LEN
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        g.query_batch_fasta(ranges, p)
    assert e.value.code == impg_amd.IMPG_E_INVALID and "'%s'" % names[2] in str(e.value)
    assert g.counter("fasta_text_bytes") == 0
    with open(str(tmp_path / "none.fa"), "wb") as f:
        with pytest.raises(impg_amd.ImpgGpuError):
            g.query_batch_fasta(ranges, p, fd=f.fileno())
    assert open(str(tmp_path / "none.fa"), "rb").read() == b""
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        g.query_batch(ranges, p).fasta(params=p)
    assert e.value.code == impg_amd.IMPG_E_INVALID and "'%s'" % names[2] in str(e.value)
    # detached again
    g.set_sequences(None)
    assert g.counter("fasta_store_bytes") == 0
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        g.query_batch_fasta(ranges, p)
    assert e.value.code == impg_amd.IMPG_E_INVALID


def test_tracepoint_index_takes_no_store():
    d = random_tp(41, 50, n_seq=3, seq_len=20_000)
    g = impg_amd.GpuImpg.from_tracepoints(d["records"], d["tracepoints"], d["seq_len"], query_deltas=d["query_deltas"], diffs=d["diffs"],
                                          fastga=d["fastga"], trace_spacing=d["trace_spacing"], max_complexity=d["max_complexity"])
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        g.set_sequences(Sequences.from_arrays(["x"], [b"ACGT"]))
    assert e.value.code == impg_amd.IMPG_E_UNSUPPORTED
