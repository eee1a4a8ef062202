"""impg_gpu_index_load_sequences on the device (impg_amd/csrc/sequence_ingest_device.hip): FASTA files streamed into HBM in
pieces and parsed there.  The expected store is always the host route's on the uncompressed text -- Sequences.from_fasta +
set_sequences -- and it is compared through what it prints: impg_gpu_selftest_fasta_rows over whole sequences and seeded
sub-ranges, byte for byte, in both store forms; the piece counter proves that the device route ran, cut where intended."""
import os
import subprocess

import numpy as np
import pytest

import impg_amd
from impg_amd import INTERVAL_DTYPE, Sequences
from tests import seq_ingest_gen as gen
from tests.seq_ingest_gen import malformed, put
from tests.test_seq_ingest_cpu import DROPPED, GHOST

pytestmark = pytest.mark.gpu
STORE_KEYS = ("fasta_store_bytes", "fasta_store_packed", "fasta_store_exception_runs")


def as_rows(triples):
    a = np.zeros(len(triples), dtype=INTERVAL_DTYPE)
    for r, (sid, first, last) in zip(a, triples):
        r["query_id"], r["q_first"], r["q_last"] = sid, first, last
        r["target_id"], r["t_first"], r["t_last"] = sid, 0, abs(last - first)
    return a


def rows_over(lens, present, seed, n_sub=200):
    """every present sequence whole, forward and reverse, and n_sub seeded sub-ranges of them on either strand"""
    rng = np.random.default_rng(seed)
    ids = [i for i in range(len(lens)) if present[i]]
    rows = [(i, 0, lens[i]) for i in ids] + [(i, lens[i], 0) for i in ids]
    for _ in range(n_sub):
        i = ids[int(rng.integers(0, len(ids)))]
        a, b = sorted(int(x) for x in rng.integers(0, lens[i] + 1, size=2))
        rows.append((i, a, b) if rng.random() < 0.5 else (i, b, a))
    return as_rows(rows)


def printed(g, rows):
    rr = np.arange(rows.size, dtype=np.uint32)
    return tuple(g.fasta_rows(rows, rr, rows.size, merge_distance=-1, reverse_complement=rc) for rc in (False, True))


class World:
    """an index that knows names and lengths, the files in every container, and what the host route prints"""

    def __init__(self, tmp, text, seqs, names, lens, seed):
        self.text, self.names, self.lens = text, names, lens
        self.paths = {kind: put(tmp, "w." + kind, data) for kind, data in gen.containers(text).items() if kind in ("plain", "bgzf", "gzip")}
        self.g = impg_amd.GpuImpg.from_paf(put(tmp, "w.paf", gen.paf_of(names, lens).encode()))
        assert [self.g.seq_name(i) for i in range(len(names))] == names and [self.g.seq_len(i) for i in range(len(names))] == lens
        have = {nm for nm, _ in seqs}
        self.rows = rows_over(lens, [nm in have for nm in names], seed)
        self.host = Sequences.from_fasta(self.paths["plain"])
        self.want, self.runs = {}, {}
        for packed in (False, True):  # the reference: computed once, left unchanged
            self.g.set_sequences(self.host, packed=packed)
            self.want[packed] = printed(self.g, self.rows)
            self.runs[packed] = self.g.counter("fasta_store_exception_runs")
        assert self.want[False] == self.want[True] and self.want[True][0] != self.want[True][1] and self.runs[True] > 0
        self.g.set_sequences(None)

    def check(self, paths, piece, packed, texts=None):
        g = self.g
        g.set_option("sequence_ingest_piece_bytes", piece)
        try:
            g.load_sequences(paths, packed=packed)
        finally:
            g.set_option("sequence_ingest_piece_bytes", gen.DEFAULT_PIECE)
        assert printed(g, self.rows) == self.want[packed]
        assert g.counter("fasta_store_exception_runs") == self.runs[packed] and g.counter("fasta_store_packed") == int(packed)
        assert g.counter("sequence_ingest_pieces") == gen.n_pieces(texts or [self.text], piece)
        assert g.counter("sequence_ingest_text_bytes") == sum(len(t) for t in (texts or [self.text]))
        assert 0 < g.counter("fasta_store_bytes")


@pytest.fixture(scope="module")
def edge(tmp_path_factory):
    text, seqs = gen.edge_file()
    names = [nm for nm, _ in seqs if nm != DROPPED] + [GHOST[0]]
    lens = [len(b) for nm, b in seqs if nm != DROPPED] + [GHOST[1]]
    return World(tmp_path_factory.mktemp("seq_ingest_edge"), text, seqs, names, lens, 7)


@pytest.fixture(scope="module")
def large(tmp_path_factory):
    text, seqs = gen.large_file()
    assert 250_000 < len(text) < 400_000 and len(seqs[0][1]) == 200_000 and len(seqs) == 501
    return World(tmp_path_factory.mktemp("seq_ingest_large"), text, seqs, [nm for nm, _ in seqs], [len(b) for _, b in seqs], 8)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("kind", ["plain", "bgzf"])
@pytest.mark.parametrize("piece", gen.PIECE_SIZES + [gen.DEFAULT_PIECE])
def test_edge_file(edge, piece, kind, packed):
    edge.check(edge.paths[kind], piece, packed)
    assert edge.g.counter("sequence_ingest_dropped_sequences") == 1 and edge.g.counter("sequence_ingest_bases") == sum(gen.EDGE_LENGTHS)
    assert (edge.g.counter("sequence_ingest_inflated_blocks") == 5) == (kind == "bgzf")


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("kind,piece", [("plain", 65536), ("plain", gen.DEFAULT_PIECE), ("bgzf", 65536), ("gzip", 65536)])
def test_large_file(large, kind, piece, packed):
    """many blocks per scan, one line that spans pieces, runs that cross piece edges (bases 70 000 .. 70 500 and 131 072)"""
    large.check(large.paths[kind], piece, packed)
    assert large.g.counter("sequence_ingest_dropped_sequences") == 0


def test_several_files(edge, tmp_path):
    """two files in one call, the second with sequences the index lacks; the index sequence no file holds fails as it does
    after set_sequences"""
    g = edge.g
    extra = b">unknown1 x\nACGTNN\n>unknown2\n\n>unknown3\nacgt"
    second = put(tmp_path, "second.fa.gz", gen.bgzf(extra, (7,)))
    ghost = as_rows([(edge.names.index(GHOST[0]), 0, 3)])
    said = {}
    for packed in (False, True):
        edge.check([edge.paths["plain"], second], 48, packed, texts=[edge.text, extra])
        assert g.counter("sequence_ingest_dropped_sequences") == 4
        with pytest.raises(impg_amd.ImpgGpuError) as e:
            g.fasta_rows(ghost, [0], 1, merge_distance=-1)
        said[packed] = (e.value.code, str(e.value))
    g.set_sequences(edge.host, packed=True)
    assert all(g.counter(k) == 0 for k in impg_amd.counter_keys() if k.startswith("sequence_ingest_"))
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        g.fasta_rows(ghost, [0], 1, merge_distance=-1)
    assert said[False] == said[True] == (e.value.code, str(e.value)) and "'ghost' not found" in str(e.value)


def test_refusals_of_the_call(edge):
    g = edge.g
    g.set_sequences(edge.host, packed=False)
    g.set_option("sequence_store_packed", 2)
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        g.load_sequences(edge.paths["plain"])
    assert e.value.code == impg_amd.IMPG_E_INVALID and "sequence_store_packed" in str(e.value)
    assert [g.counter(k) for k in STORE_KEYS] == [0, 0, 0]  # the call replaces the attached store, and a failed one leaves none
    g.set_option("sequence_store_packed", 0)
    for bad in (8, 24, (1 << 32) + 16):
        with pytest.raises(impg_amd.ImpgGpuError):
            g.set_option("sequence_ingest_piece_bytes", bad)
    with pytest.raises(ValueError):
        g.load_sequences(edge.paths["plain"], packed="auto")


def test_errors_leave_no_store_and_a_good_call_follows(edge, tmp_path):
    """every malformed input of the CPU test through the real call (the inputs are files: the kernels see only inflated text)"""
    for key, (paths, names, lens, code, words) in malformed(tmp_path).items():
        g = impg_amd.GpuImpg.from_paf(put(tmp_path, "i.paf", gen.paf_of(names + ["other"], lens + [5]).encode()))
        want = None
        for packed in (False, True):
            g.set_option("sequence_ingest_piece_bytes", 32)
            with pytest.raises(impg_amd.ImpgGpuError) as e:
                g.load_sequences(paths, packed=packed)
            assert e.value.code == code and words in str(e.value), (key, str(e.value))
            assert [g.counter(k) for k in STORE_KEYS] == [0, 0, 0], key
            with pytest.raises(impg_amd.ImpgGpuError) as e:
                g.fasta_rows(as_rows([(0, 0, 1)]), [0], 1, merge_distance=-1)
            assert "needs a sequence store" in str(e.value)
            # a good call follows: the same handle, sequences of the index's lengths
            fixed = put(tmp_path, "fixed.fa", b"".join(b">%s\n%s\n" % (nm.encode(), (b"ACGTN" * 80)[:n]) for nm, n in zip(names, lens)))
            g.load_sequences(fixed, packed=packed)
            got = g.fasta_rows(as_rows([(0, 0, lens[0]), (0, lens[0], 0)]), [0, 1], 2, merge_distance=-1, reverse_complement=True)
            want = want or got
            assert got == want and got.startswith(b">" + names[0].encode() + b":0-%d\n" % lens[0] + (b"ACGTN" * 80)[:min(lens[0], 80)])


# ---- end to end -------------------------------------------------------------------------------------------------------------
SHAPE = dict(n_seq=8, seq_len=40_000, target_span=3_000, n_blocks=40)  # (100 records: about twenty partitions)


@pytest.fixture(scope="module")
def whole(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("seq_ingest_whole")
    paf = str(tmp / "synth.paf")
    impg_amd.synth_paf_text(paf, 11, 100, **SHAPE)
    g = impg_amd.GpuImpg.from_paf(paf)
    rng = np.random.default_rng(11)
    names = [g.seq_name(i) for i in range(g.num_seqs())]
    seqs = [gen._bases(rng, g.seq_len(i)) for i in range(g.num_seqs())]
    fa = b"".join(b">%s some text\n" % nm.encode() + b"".join(bytes(b[i:i + 60]) + b"\n" for i in range(0, len(b), 60)) for nm, b in zip(names, seqs))
    plain, bgz = put(tmp, "seqs.fa", fa), put(tmp, "seqs.fa.gz", gen.bgzf(fa, (65280,)))
    bed = str(tmp / "q.bed")
    ranges = [(int(r["target_id"]), int(r["start"]), int(r["end"])) for r in impg_amd.synth_bed(5, 24, n_seq=8, seq_len=40_000, range_len=3000)]
    ranges = [(g.seq_id(impg_amd.synth_seq_name(t)), s, e) for t, s, e in ranges]
    with open(bed, "w") as f:
        for t, s, e in ranges:
            f.write("%s\t%d\t%d\n" % (g.seq_name(t), s, e))
    return g, paf, plain, bgz, bed, ranges


def folder_files(folder):
    return {nm: open(os.path.join(folder, nm), "rb").read() for nm in sorted(os.listdir(folder))}


@pytest.mark.parametrize("packed", [False, True])
def test_query_and_partition_after_load_sequences(whole, packed, tmp_path):
    g, _, plain, bgz, _, ranges = whole
    p = impg_amd.make_params(transitive=True, max_depth=2)
    run = dict(window_size=10_000, merge_distance=1000)
    g.set_sequences(Sequences.from_fasta(plain), packed=packed)
    want = g.query_batch_fasta(ranges, p, merge_distance=500, reverse_complement=True, raw=True)
    n_parts = g.partitions_fasta(str(tmp_path / "host"), params=p, **run)
    want_files = folder_files(str(tmp_path / "host"))
    assert want.count(b">") >= len(ranges) and b"/rc\n" in want and n_parts == len(want_files) > 3
    g.set_option("sequence_ingest_piece_bytes", 65536)
    try:
        g.load_sequences(bgz, packed=packed)
    finally:
        g.set_option("sequence_ingest_piece_bytes", gen.DEFAULT_PIECE)
    assert g.counter("sequence_ingest_pieces") > 4 and g.counter("sequence_ingest_inflated_blocks") > 4
    assert g.query_batch_fasta(ranges, p, merge_distance=500, reverse_complement=True, raw=True) == want
    assert g.partitions_fasta(str(tmp_path / "device"), params=p, **run) == n_parts
    assert folder_files(str(tmp_path / "device")) == want_files
    # the routes that read the host copy say what to call instead; they do not read an empty string
    res = g.query_batch(ranges, p)
    for call in (lambda: res.fasta(merge_distance=500, params=p, raw=True), lambda: g.partition_rows_fasta([(0, 0, 10)], on_host=True),
                 lambda: g.partitions_fasta(str(tmp_path / "refused"), params=p, state_on_host=True, **run)):
        with pytest.raises(impg_amd.ImpgGpuError) as e:
            call()
        assert e.value.code == impg_amd.IMPG_E_UNSUPPORTED and "impg_gpu_index_set_sequences" in str(e.value)
    assert g.partition_rows_fasta([(0, 0, 10)]).startswith(b">")


def test_command_line(whole, tmp_path):
    """--sequence-ingest device on the bgzipped file prints what the host route prints from the plain one, for query and for
    partition; with --host-merge it is refused up front"""
    _, paf, plain, bgz, bed, _ = whole
    cli = os.path.join(os.path.dirname(impg_amd.__file__), "impg-gpu")
    query = [cli, "query", "-a", paf, "-b", bed, "-o", "fasta", "-x", "-m", "2", "-d", "500", "--reverse-complement", "--sequence-files"]
    host = subprocess.run(query + [plain], capture_output=True, timeout=120)
    assert host.returncode == 0 and host.stdout.count(b">") >= 24, host.stderr
    for extra in ([], ["--sequence-store", "packed"]):
        r = subprocess.run(query + [bgz, "--sequence-ingest", "device"] + extra, capture_output=True, timeout=120)
        assert r.returncode == 0 and r.stdout == host.stdout, (extra, r.stderr)
    r = subprocess.run(query + [bgz, "--sequence-ingest", "host"], capture_output=True, timeout=120)
    assert r.returncode != 0 and b"decompress it first" in r.stderr and r.stdout == b""
    r = subprocess.run(query + [bgz, "--sequence-ingest", "device", "--host-merge"], capture_output=True, timeout=120)
    assert r.returncode == 2 and b"--host-merge" in r.stderr and r.stdout == b""
    r = subprocess.run(query + [bgz, "--sequence-ingest", "gpu"], capture_output=True, timeout=120)
    assert r.returncode == 2 and r.stdout == b""
    part = [cli, "partition", "-a", paf, "-w", "10000", "-d", "1000", "-m", "2", "-o", "fasta", "--separate-files", "--sequence-files"]
    r = subprocess.run(part + [plain, "--output-folder", str(tmp_path / "host")], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(part + [bgz, "--sequence-ingest", "device", "--output-folder", str(tmp_path / "device")], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert folder_files(str(tmp_path / "device")) == folder_files(str(tmp_path / "host")) and len(os.listdir(str(tmp_path / "host"))) > 3
    r = subprocess.run(part + [bgz, "--sequence-ingest", "device", "--host-state", "--output-folder", str(tmp_path / "no")], capture_output=True, timeout=120)
    assert r.returncode == 2 and b"--host-state" in r.stderr
