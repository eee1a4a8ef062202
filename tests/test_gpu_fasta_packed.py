"""The packed sequence store (option "sequence_store_packed", impg_amd/csrc/fasta_device.hip): two bits a base in HBM, the
bytes that are not A/C/G/T kept as runs, packed on the device chunk by chunk -- and the FASTA text unchanged.  Every text is
compared byte for byte: with the restatement of tests/fasta_ref.py, with what the same handle prints from the one-byte store,
and on the whole path with the host twin.  Every case is small."""
import os
import subprocess

import numpy as np
import pytest

import impg_amd
from impg_amd import INTERVAL_DTYPE, Sequences
from tests import fasta_ref as ref
from tests.paf_gen import random_paf, random_ranges

pytestmark = pytest.mark.gpu

STORE_KEYS = ("fasta_store_bytes", "fasta_store_packed", "fasta_store_exception_runs")
BODY_LENGTHS = [0, 1, 2, 15, 16, 17, 79, 80, 81, 82, 159, 160, 161, 162, 1000]  # test_gpu_fasta_device.py's
RUN_LENGTHS = [1, 2, 15, 16, 17, 64, 1000]
SHORT = 4093  # the shortest sequence: the crafted rows stay below it


def write(tmp, name, text):
    path = str(tmp / name)
    with open(path, "w") as f:
        f.write(text)
    return path


def random_acgt(rng, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)])


def planted_sequence(rng):
    """ACGT with runs planted: N runs of every length in RUN_LENGTHS starting at every residue mod 16 (the short ones first,
    three or more bases of ACGT between two of them), N immediately followed by R, a run at base 0, a run that ends at the
    last base; the length is 3 mod 4, so the stream's last byte is partly filled.  -> (bytes, [(start, end)] of its runs)"""
    runs, at = [(0, 3)], 8
    for L in RUN_LENGTHS:
        for res in range(16):
            at += 3
            at += (res - at) % 16
            runs.append((at, at + L))
            at += L
    n_then_r = (at + 5, at + 9, at + 12)
    n = at + 40
    n += (3 - n) % 4
    b = bytearray(random_acgt(rng, n))
    for s, e in runs:
        b[s:e] = b"N" * (e - s)
    b[n_then_r[0]:n_then_r[1]] = b"N" * 4
    b[n_then_r[1]:n_then_r[2]] = b"R" * 3
    b[n - 5:] = b"N" * 5
    return bytes(b), runs + [(n_then_r[0], n_then_r[1]), (n_then_r[1], n_then_r[2]), (n - 5, n)]


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """six sequences behind an index that only has to know their names and lengths: pure ACGT of 4 093, 4 096 and 4 099 bases
    (a, e, f), ACGT with planted runs (b), tests/fasta_ref.py's dense alphabet (c: 5 of 14 bytes are exceptions) and all N (d)"""
    rng = np.random.default_rng(4093)
    planted, runs = planted_sequence(rng)
    seqs = {"a": random_acgt(rng, 4093), "b": planted, "c": ref.random_sequence(rng, 4096), "d": b"N" * 4099, "e": random_acgt(rng, 4096),
            "f": random_acgt(rng, 4099)}
    names = list(seqs)
    paf = "".join("%s\t%d\t0\t100\t+\t%s\t%d\t0\t100\t100\t100\t60\tcg:Z:100=\n" % (q, len(seqs[q]), t, len(seqs[t])) for q, t in zip(names, names[1:]))
    g = impg_amd.GpuImpg.from_paf(write(tmp_path_factory.mktemp("fasta_packed"), "small.paf", paf))
    assert [g.seq_name(i) for i in range(len(names))] == names
    return g, names, [seqs[nm] for nm in names], runs


def attach(small, packed, only=None):
    g, names, seqs, _ = small
    keep = [i for i, nm in enumerate(names) if only is None or nm in only]
    g.set_sequences(Sequences.from_arrays([names[i] for i in keep], [seqs[i] for i in keep]), packed=packed)
    return g


def as_rows(triples):
    a = np.zeros(len(triples), dtype=INTERVAL_DTYPE)
    for r, (sid, first, last) in zip(a, triples):
        r["query_id"], r["q_first"], r["q_last"] = sid, first, last
        r["target_id"], r["t_first"], r["t_last"] = sid, 0, abs(last - first)
    return a


def crafted_rows(small):
    """every body length x every residue of the source start mod 64 x both strands, spread over the six sequences; rows at
    every sequence's first and last bases; rows that begin or end inside, at the first base of and at the last base of every
    planted run, and one whose run lies across its column-80 break.  Each row is its own range: none merge."""
    _, names, seqs, runs = small
    rows = []
    for k, L in enumerate(BODY_LENGTHS):
        for res in range(64):
            for fwd in (True, False):
                sid = (k + res) % len(seqs)
                start = 64 * ((7 * k + 3 * res) % 45) + res
                assert start + L <= SHORT
                rows.append((sid, start, start + L) if fwd else (sid, start + L, start))
        for sid, q in enumerate(seqs):
            for fwd in (True, False):
                rows.append((sid, 0, L) if fwd else (sid, L, 0))
                rows.append((sid, len(q) - L, len(q)) if fwd else (sid, len(q), len(q) - L))
    b, n_b = names.index("b"), len(seqs[names.index("b")])
    for s, e in runs:
        mid = (s + e) // 2
        for first in (s, mid, e - 1):  # begins at the run's first base, inside it, at its last base
            rows += [(b, first, min(n_b, first + 100)), (b, min(n_b, first + 100), first)]
        for last in (s + 1, mid + 1, e):  # ends there
            rows += [(b, max(0, last - 100), last), (b, last, max(0, last - 100))]
    s, e = next((s, e) for s, e in runs if e - s == 16 and s > 100)
    rows += [(b, s - 72, s + 200), (b, s + 200, s - 72), (b, e - 200, e + 72), (b, e + 72, e - 200)]  # the run takes columns 72 .. 87
    return as_rows(rows)


def restated(rows, row_range, n_ranges, d, rc, small):
    _, names, seqs, _ = small
    return b"".join(ref.fasta_range(rows[row_range == q], d, rc, lambda i: names[i], lambda i: seqs[i]) for q in range(n_ranges))


@pytest.fixture(scope="module")
def texts(small):
    """the restatement's text of the crafted rows, one range per row, for either setting of reverse_complement"""
    rows = crafted_rows(small)
    rr = np.arange(rows.size, dtype=np.uint32)
    return rows, rr, {rc: restated(rows, rr, rows.size, -1, rc, small) for rc in (False, True)}


def test_planted_runs_are_what_the_store_extracts(small):
    """the fixture's own list of runs is the host's (Sequences.exceptions): what the rows at run edges aim at"""
    _, names, seqs, runs = small
    start, length, byte = Sequences.from_arrays(names, seqs).exceptions(names.index("b"))
    assert sorted(runs) == list(zip(start.tolist(), (start + length).tolist()))
    assert set(byte.tolist()) == {ord("N"), ord("R")} and {e - s for s, e in runs} >= set(RUN_LENGTHS)
    for L in RUN_LENGTHS:
        assert {s % 16 for s, e in runs if e - s == L} == set(range(16))


@pytest.mark.parametrize("rc", [False, True])
def test_packed_text(small, texts, rc):
    rows, rr, want = texts
    g = attach(small, True)
    g.set_option("bed_text_piece_bytes", 256 << 20)
    assert g.counter("fasta_store_packed") == 1
    got = g.fasta_rows(rows, rr, rows.size, merge_distance=-1, reverse_complement=rc)
    assert got == want[rc]
    assert got.count(b">") == rows.size > 2000 and g.counter("fasta_text_pieces") == 1
    # ... and the same handle, the store attached again a byte per base
    attach(small, False)
    assert g.counter("fasta_store_packed") == 0 and g.counter("fasta_store_exception_runs") == 0
    assert g.fasta_rows(rows, rr, rows.size, merge_distance=-1, reverse_complement=rc) == got


def test_store_counters(small):
    g, names, seqs, _ = small
    attach(small, True)
    store = Sequences.from_arrays(names, seqs)
    n_runs = sum(store.exceptions(i)[0].size for i in range(len(names)))
    assert n_runs > 1000 and g.counter("fasta_store_exception_runs") == n_runs and g.counter("fasta_store_packed") == 1
    # changing the option does not repack an attached store
    g.set_option("sequence_store_packed", 0)
    assert g.counter("fasta_store_packed") == 1 and g.counter("fasta_store_exception_runs") == n_runs
    g.set_sequences(None)
    assert [g.counter(k) for k in STORE_KEYS] == [0, 0, 0]
    # a store of pure ACGT: a quarter of a byte a base, 16 bytes a sequence and the padding
    pure = ("a", "e", "f")
    total = sum(len(seqs[names.index(nm)]) for nm in pure)
    attach(small, False, only=pure)
    as_bytes = g.counter("fasta_store_bytes")
    assert as_bytes >= total and g.counter("fasta_store_packed") == 0
    g.set_option("sequence_store_packed", 1)
    assert g.counter("fasta_store_packed") == 0 and g.counter("fasta_store_bytes") == as_bytes
    attach(small, True, only=pure)
    assert g.counter("fasta_store_packed") == 1 and g.counter("fasta_store_exception_runs") == 0
    assert g.counter("fasta_store_bytes") <= total / 4 + 16 * len(pure) + 96
    assert g.counter("fasta_store_bytes") < as_bytes / 2
    # "auto": packed where that is smaller, bytes for the dense alphabet (a run every three bases, nine bytes a run)
    attach(small, "auto", only=pure)
    assert g.counter("fasta_store_packed") == 1 and g.counter("fasta_store_bytes") < as_bytes / 2
    attach(small, "auto", only=("c",))
    assert g.counter("fasta_store_packed") == 0 and g.counter("fasta_store_exception_runs") == 0 and g.counter("fasta_store_bytes") >= 4096
    g.set_sequences(None)
    assert [g.counter(k) for k in STORE_KEYS] == [0, 0, 0]
    with pytest.raises(ValueError):
        g.set_sequences(store, packed=2)


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("d", [0, 30])
def test_packed_text_merged(small, texts, d, rc):
    """the same rows as four ranges: the sweep runs in front and merges what overlaps or lies within d, the strands apart"""
    rows, _, _ = texts
    rr = (np.arange(rows.size, dtype=np.uint32) * 7) % 4
    g = attach(small, True)
    g.set_option("bed_text_piece_bytes", 256 << 20)
    got = g.fasta_rows(rows, rr, 4, merge_distance=d, reverse_complement=rc)
    assert got == restated(rows, rr, 4, d, rc, small)
    assert g.counter("fasta_records") == got.count(b">") < rows.size


@pytest.mark.parametrize("piece", [64, 1024])
def test_packed_text_in_pieces(small, texts, piece):
    rows, rr, want = texts
    g = attach(small, True)
    g.set_option("bed_text_piece_bytes", piece)
    try:
        for rc in (False, True):
            assert g.fasta_rows(rows, rr, rows.size, merge_distance=-1, reverse_complement=rc) == want[rc]
            assert g.counter("fasta_text_pieces") > 1 and g.counter("fasta_text_bytes") == len(want[rc])
    finally:
        g.set_option("bed_text_piece_bytes", 256 << 20)


@pytest.mark.parametrize("chunk", [64, 1000, 4096, 20000])
def test_packed_in_chunks(small, texts, chunk, monkeypatch):
    """the staging chunk of the attach down to 64 bases (1 000 rounds up to 1 024): chunks end inside sequences, between them
    and beyond the last; the store and the text do not move"""
    rows, rr, want = texts
    g = attach(small, True)
    whole = [g.counter(k) for k in STORE_KEYS]
    monkeypatch.setenv("IMPG_SEQ_PACK_CHUNK", str(chunk))
    attach(small, True)
    assert [g.counter(k) for k in STORE_KEYS] == whole
    assert g.fasta_rows(rows, rr, rows.size, merge_distance=-1, reverse_complement=True) == want[True]


def test_refusals_are_the_byte_store_s(small):
    """a row on a sequence the store lacks, a row that leaves its sequence, a length mismatch at attach: the same code and
    message from either form"""
    g, names, seqs, _ = small
    c = names.index("c")
    said = {}
    for packed in (False, True):
        attach(small, packed, only=("a", "b", "d", "e", "f"))
        with pytest.raises(impg_amd.ImpgGpuError) as e:
            g.fasta_rows(as_rows([(0, 10, 50), (c, 10, 50)]), [0, 1], 2, merge_distance=-1)
        lacks = (e.value.code, str(e.value))
        assert g.counter("fasta_text_bytes") == 0
        attach(small, packed)
        with pytest.raises(impg_amd.ImpgGpuError) as e:
            g.fasta_rows(as_rows([(0, 10, 50), (c, 4000, 4097)]), [0, 1], 2, merge_distance=-1, reverse_complement=True)
        leaves = (e.value.code, str(e.value))
        before = [g.counter(k) for k in STORE_KEYS]
        with pytest.raises(impg_amd.ImpgGpuError) as e:
            g.set_sequences(Sequences.from_arrays(names, seqs[:c] + [seqs[c][:-1]] + seqs[c + 1:]), packed=packed)
        mismatch = (e.value.code, str(e.value))
        assert [g.counter(k) for k in STORE_KEYS] == before  # (nothing new is attached: the store of before stays)
        said[packed] = (lacks, leaves, mismatch)
    assert said[True] == said[False]
    assert [code for code, _ in said[True]] == [impg_amd.IMPG_E_INVALID] * 3
    assert "'c' not found" in said[True][0][1] and "leaves its sequence of 4096" in said[True][1][1] and "'c' has 4095" in said[True][2][1]


# ---- whole path -----------------------------------------------------------------------------------------------------------
N_SEQ, WHOLE_LEN = 8, 20000


@pytest.fixture(scope="module")
def whole(tmp_path_factory):
    text, names = random_paf(31, 300, n_seq=N_SEQ, seq_len=WHOLE_LEN)
    path = write(tmp_path_factory.mktemp("fasta_packed_whole"), "whole.paf", text)
    g = impg_amd.GpuImpg.from_paf(path)
    rng = np.random.default_rng(31)
    seqs = {nm: ref.random_sequence(rng, WHOLE_LEN) for nm in names}
    ranges = [(g.seq_id(names[t]), s, e) for t, s, e in random_ranges(31, 32, N_SEQ, WHOLE_LEN, max_len=3000, min_len=200)]
    return g, path, names, seqs, ranges


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("d", [-1, 1000])
def test_whole_path(whole, d, rc):
    """32 ranges, -x -m 2: the packed store's text == the byte store's == the host twin's"""
    g, _, names, seqs, ranges = whole
    store = Sequences.from_arrays(names, [seqs[nm] for nm in names])
    p = impg_amd.make_params(transitive=True, max_depth=2)
    g.set_sequences(store, packed=False)
    want = g.query_batch_fasta(ranges, p, merge_distance=d, reverse_complement=rc, raw=True)
    assert want.count(b">") >= 32 and g.counter("fasta_store_packed") == 0
    g.set_sequences(store, packed=True)
    assert g.counter("fasta_store_packed") == 1 and g.counter("fasta_store_exception_runs") > N_SEQ * WHOLE_LEN // 5
    assert g.query_batch_fasta(ranges, p, merge_distance=d, reverse_complement=rc, raw=True) == want
    assert g.counter("fasta_text_bytes") == len(want)
    assert g.query_batch(ranges, p).fasta(merge_distance=d, params=p, reverse_complement=rc, raw=True) == want


def test_command_line(whole, tmp_path):
    """`impg-gpu query -o fasta --sequence-store packed` prints what it prints without the flag; --host-merge takes the flag
    and prints from the host copy; a value that is none of the three is a usage error"""
    g, paf, names, seqs, ranges = whole
    cli = os.path.join(os.path.dirname(impg_amd.__file__), "impg-gpu")
    bed, fa = str(tmp_path / "q.bed"), str(tmp_path / "a.fa")
    with open(bed, "w") as f:
        for t, s, e in ranges:
            f.write("%s\t%d\t%d\n" % (g.seq_name(t), s, e))
    with open(fa, "wb") as f:
        for nm in names:
            f.write(b">%s\n" % nm.encode() + b"".join(seqs[nm][i:i + 60].lower() + b"\n" for i in range(0, WHOLE_LEN, 60)))
    base = [cli, "query", "-a", paf, "-b", bed, "-o", "fasta", "-x", "-m", "2", "-d", "1000", "--reverse-complement", "--sequence-files", fa]
    plain = subprocess.run(base, capture_output=True)
    assert plain.returncode == 0 and plain.stdout.count(b">") >= 32 and b"/rc\n" in plain.stdout, plain.stderr
    for extra in (["--sequence-store", "packed"], ["--sequence-store", "auto"], ["--sequence-store", "bytes"], ["--sequence-store", "packed", "--host-merge"]):
        r = subprocess.run(base + extra, capture_output=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == plain.stdout, extra
    r = subprocess.run(base + ["--sequence-store", "nibbles"], capture_output=True)
    assert r.returncode == 2 and r.stdout == b""
