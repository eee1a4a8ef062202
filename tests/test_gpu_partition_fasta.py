"""`impg partition -o fasta` (impg_gpu_partition_run_fasta / _window_fasta / _rows_fasta; fasta_device.hip's byte-window
write kernel, text_device.hip's session-lived stream, partition.cpp): every text is compared byte for byte with the
restatement of tests/partition_fasta_ref.py.  Every case is small."""
import copy
import os
import subprocess

import numpy as np
import pytest

import impg_amd
from impg_amd import INTERVAL_DTYPE, Sequences
from oracle import oracle as o
from tests import fasta_ref
from tests import partition_fasta_ref as ref
from tests import partition_ref as pr

pytestmark = pytest.mark.gpu

# ---- 1. the writer at the piece edges ---------------------------------------------------------------------------------
SHORT = ["a", "b", "c"]
LONG = [("sample%d#1#chromosome" % k).ljust(30, "x") for k in range(3)]  # a header longer than a lane's 16 bytes, and than most cuts' reach
SEQ_LEN = 4096
BODY_LENGTHS = [0, 1, 2, 15, 16, 17, 79, 80, 81, 82, 159, 160, 161, 162, 1000]
PIECES = [64, 81, 1024, 256 << 20]
CUT_CLASSES = ("header", "first byte", "last byte", "before a line's newline", "after a line's newline", "mid-line")


def write(tmp, name, text):
    path = str(tmp / name)
    with open(path, "w") as f:
        f.write(text)
    return path


def crafted_rows():
    """every body length x every residue of the source start mod 16, spread over the three sequences, then the sequence's first
    and last bases, and one whole sequence at the end"""
    rows = []
    for k, L in enumerate(BODY_LENGTHS):
        for res in range(16):
            start = 16 * ((7 * k + 3 * res) % 150) + res
            rows.append(((k + res) % 3, start, start + L))
        rows.append((k % 3, 0, L))
        rows.append((k % 3, SEQ_LEN - L, SEQ_LEN))
    # (five bases that shift the whole sequence's record so that, under 30-letter names and pieces of 81 bytes -- the length of a
    # full line --, its cuts fall right before the lines' newlines: without them that class of cut is empty there)
    rows.append((2, 7, 12))
    rows.append((1, 0, SEQ_LEN))
    return rows


def cut_classes(rows, names, seqs, piece):
    """where the cuts of a text in pieces of `piece` bytes fall, from the restated text alone: {class: number of cuts}; a cut is
    named after the byte a piece BEGINS with"""
    count = dict.fromkeys(CUT_CLASSES, 0)
    at = 0
    for s, a, b in rows:
        rec = ref.record(names[s], seqs[s], a, b)
        hl = rec.index(b"\n") + 1
        first_cut = -(-at // piece) * piece
        for c in range(max(first_cut, piece), at + len(rec), piece):
            x = c - at
            if x == 0:
                count["first byte"] += 1
            elif x < hl:
                count["header"] += 1
            elif x == len(rec) - 1:
                count["last byte"] += 1
            elif rec[x:x + 1] == b"\n":
                count["before a line's newline"] += 1
            elif rec[x - 1:x] == b"\n":
                count["after a line's newline"] += 1
            else:
                count["mid-line"] += 1
        at += len(rec)
    return count


@pytest.fixture(scope="module", params=["short names", "30-letter names"])
def small(request, tmp_path_factory):
    """three sequences of 4 096 random bytes behind an index that only has to know their names and lengths"""
    names = SHORT if request.param == "short names" else LONG
    assert all(len(n) == (1 if names is SHORT else 30) for n in names)
    rng = np.random.default_rng(4096)
    seqs = [fasta_ref.random_sequence(rng, SEQ_LEN) for _ in names]
    paf = "".join("%s\t%d\t0\t100\t+\t%s\t%d\t0\t100\t100\t100\t60\tcg:Z:100=\n" % (q, SEQ_LEN, t, SEQ_LEN)
                  for q, t in ((names[0], names[1]), (names[1], names[2])))
    g = impg_amd.GpuImpg.from_paf(write(tmp_path_factory.mktemp("partition_fasta_small"), "small.paf", paf))
    assert [g.seq_name(i) for i in range(3)] == names
    store = Sequences.from_arrays(names, seqs)
    rows = crafted_rows()
    return g, store, names, seqs, rows, ref.partition_text(rows, names, seqs)


def test_the_crafted_rows_reach_every_kind_of_cut(small):
    """(needs no device: the restated text and the piece size say where the cuts fall)"""
    _, _, names, seqs, rows, want = small
    for piece in (64, 81):
        count = cut_classes(rows, names, seqs, piece)
        assert sum(count.values()) == (len(want) - 1) // piece
        assert all(count[k] > 0 for k in CUT_CLASSES), (piece, count)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("piece", PIECES)
def test_writer_at_the_piece_edges(small, piece, packed):
    g, store, names, seqs, rows, want = small
    g.set_sequences(store, packed=packed)
    assert g.counter("fasta_store_packed") == int(packed)
    g.set_option("bed_text_piece_bytes", piece)
    try:
        before = {k: g.counter(k) for k in ("fasta_text_pieces", "fasta_text_bytes", "fasta_records")}
        got = g.partition_rows_fasta(rows)
        assert got == want
        assert g.counter("fasta_text_pieces") - before["fasta_text_pieces"] == -(-len(want) // piece)
        assert g.counter("fasta_text_bytes") - before["fasta_text_bytes"] == len(want)
        assert g.counter("fasta_records") - before["fasta_records"] == len(rows)
    finally:
        g.set_option("bed_text_piece_bytes", 256 << 20)


@pytest.mark.parametrize("packed", [False, True])
def test_a_record_of_many_pieces_and_the_query_routes_refusal(small, packed):
    g, store, names, seqs, rows, _ = small
    g.set_sequences(store, packed=packed)
    whole = [(1, 0, SEQ_LEN)]
    want = ref.record(names[1], seqs[1], 0, SEQ_LEN)
    g.set_option("bed_text_piece_bytes", 64)
    try:
        before = g.counter("fasta_text_pieces")
        assert g.partition_rows_fasta(whole) == want  # nothing is refused
        assert g.counter("fasta_text_pieces") - before == -(-len(want) // 64)
        assert g.partition_rows_fasta(whole, on_host=True) == want
        # the query route is as it was (a guard of existing code): its buffer is the piece and 4 096 bytes of slack, which the
        # record under a 30-letter name outgrows (4 187 bytes) and the one under a one-letter name just fits (4 158)
        row = np.zeros(1, dtype=INTERVAL_DTYPE)
        row[0]["query_id"], row[0]["q_first"], row[0]["q_last"] = 1, 0, SEQ_LEN
        assert (len(want) > 64 + 4096) == (len(names[1]) == 30)
        if len(want) > 64 + 4096:
            with pytest.raises(impg_amd.ImpgGpuError) as e:
                g.fasta_rows(row, [0], 1, merge_distance=-1)
            assert e.value.code == impg_amd.IMPG_E_UNSUPPORTED
        else:
            assert g.fasta_rows(row, [0], 1, merge_distance=-1) == want
    finally:
        g.set_option("bed_text_piece_bytes", 256 << 20)


def test_host_twin_prints_the_same_bytes(small):
    g, store, _, _, rows, want = small
    g.set_sequences(store, packed=False)
    assert g.partition_rows_fasta(rows, on_host=True) == want
    assert g.partition_rows_fasta([]) == b"" and g.partition_rows_fasta([], on_host=True) == b""
    assert g.partition_rows_fasta([(0, 5, 5)]) == b">%s:5-5\n" % g.seq_name(0).encode()  # no bases: the header alone


def test_row_refusals_leave_no_text(small):
    g, store, names, _, _, _ = small
    g.set_sequences(store, packed=False)
    before = g.counter("fasta_text_bytes")
    for bad in ([(0, 0, 10), (2, 100, SEQ_LEN + 1)], [(0, 20, 10)], [(1, -1, 10)]):
        for host in (False, True):
            with pytest.raises(impg_amd.ImpgGpuError) as e:
                g.partition_rows_fasta(bad, on_host=host)
            assert e.value.code == impg_amd.IMPG_E_INVALID and "leaves its sequence" in str(e.value)
    assert g.counter("fasta_text_bytes") == before
    g.set_sequences(Sequences.from_arrays(names[:2], [b"A" * SEQ_LEN] * 2))
    try:
        for host in (False, True):
            with pytest.raises(impg_amd.ImpgGpuError) as e:
                g.partition_rows_fasta([(0, 0, 10), (2, 0, 10)], on_host=host)
            assert e.value.code == impg_amd.IMPG_E_INVALID and "'%s' not found" % names[2] in str(e.value)
    finally:
        g.set_sequences(store, packed=False)


# ---- 2. the session end to end ----------------------------------------------------------------------------------------
SEED, N_REC = 3, 2000
SHAPE = dict(n_seq=20, seq_len=200_000, target_span=10_000, n_blocks=100)
RUN = dict(window_size=20_000, merge_distance=1000)
SESSION_KEYS = ("windows", "partitions", "mask_uploads", "rows_to_host", "fasta_windows", "fasta_host_windows", "text_table_uploads",
                "text_buffer_allocs")


@pytest.fixture(scope="module")
def paf(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("partition_fasta") / "synth.paf")
    impg_amd.synth_paf_text(path, SEED, N_REC, **SHAPE)
    return path


@pytest.fixture(scope="module")
def cpu(paf):
    return o.OracleIndex(paf_paths=[paf], preparse=True)


@pytest.fixture(scope="module")
def world(paf, cpu):
    """the index with its store, the sequences, and what the restatement says the files hold"""
    n = cpu.num_seqs()
    names = [cpu.seq_name(s) for s in range(n)]
    rng = np.random.default_rng(200_000)
    seqs = [fasta_ref.random_sequence(rng, cpu.seq_len(s)) for s in range(n)]
    _, parts, _ = pr.partition(cpu, RUN["window_size"], RUN["merge_distance"], rehome=False, max_depth=2)
    assert len(parts) >= 20 and max(len(rows) for _, rows in parts) > 1
    assert [k for k, _ in parts] == list(range(len(parts)))
    files = {"partition%d.fasta" % k: ref.partition_text(rows, names, seqs) for k, rows in parts}
    g = impg_amd.GpuImpg.from_paf(paf)
    assert [g.seq_name(s) for s in range(n)] == names
    store = Sequences.from_arrays(names, seqs)
    g.set_sequences(store, packed=False)
    return g, store, names, seqs, parts, files


@pytest.fixture(scope="module")
def bed_tables(world):
    """the masked and missing tables a BED session leaves on the same index"""
    s = world[0].partition_session(RUN["window_size"], RUN["merge_distance"], impg_amd.make_params(transitive=True, max_depth=2))
    try:
        s.run_text()
        return s.regions().get("masked"), s.regions().get("missing")
    finally:
        s.close()


def run_fasta(g, folder, **kw):
    s = g.partition_session(RUN["window_size"], RUN["merge_distance"], impg_amd.make_params(transitive=True, max_depth=2), **kw)
    try:
        before = {k: g.counter(k) for k in ("fasta_text_bytes", "fasta_text_pieces")}
        n = s.run_fasta(str(folder))
        index = {k: g.counter(k) - v for k, v in before.items()}
        return n, {k: s.counter(k) for k in SESSION_KEYS}, index, (s.regions().get("masked"), s.regions().get("missing"))
    finally:
        s.close()


def check_files(folder, files):
    assert sorted(os.listdir(folder)) == sorted(files)
    for name, want in files.items():
        with open(os.path.join(folder, name), "rb") as f:
            assert f.read() == want, name


def test_session_writes_the_restated_files(world, bed_tables, tmp_path):
    g, _, _, _, parts, files = world
    K = len(parts)
    n, c, index, tables = run_fasta(g, tmp_path / "out")
    assert n == K
    check_files(tmp_path / "out", files)
    assert c["rows_to_host"] == 0 and c["mask_uploads"] == 0
    assert c["fasta_windows"] == K and c["fasta_host_windows"] == 0 and c["partitions"] == K
    assert c["text_table_uploads"] == 1 and c["text_buffer_allocs"] == 1
    assert index["fasta_text_bytes"] == sum(len(t) for t in files.values())
    assert index["fasta_text_pieces"] == K  # every window's text is shorter than a piece
    assert tables == bed_tables


def test_session_in_small_pieces(world, bed_tables, tmp_path):
    g, _, _, _, parts, files = world
    g.set_option("bed_text_piece_bytes", 1 << 14)
    try:
        n, c, index, tables = run_fasta(g, tmp_path / "out")
    finally:
        g.set_option("bed_text_piece_bytes", 256 << 20)
    check_files(tmp_path / "out", files)
    assert index["fasta_text_pieces"] == sum(-(-len(t) // (1 << 14)) for t in files.values()) > len(parts)
    assert c["text_table_uploads"] == 1 and c["text_buffer_allocs"] == 1 and c["rows_to_host"] == 0 and c["mask_uploads"] == 0
    assert tables == bed_tables


def test_session_from_the_packed_store(world, bed_tables, tmp_path):
    g, store, _, _, parts, files = world
    g.set_sequences(store, packed=True)
    try:
        assert g.counter("fasta_store_packed") == 1
        n, c, _, tables = run_fasta(g, tmp_path / "out")
    finally:
        g.set_sequences(store, packed=False)
    check_files(tmp_path / "out", files)
    assert n == c["fasta_windows"] == len(parts) and tables == bed_tables


def test_session_with_its_state_on_the_host(world, bed_tables, tmp_path):
    g, _, _, _, parts, files = world
    n, c, index, tables = run_fasta(g, tmp_path / "out", state_on_host=True)
    check_files(tmp_path / "out", files)
    assert n == c["fasta_host_windows"] == len(parts) and c["fasta_windows"] == 0 and c["text_buffer_allocs"] == 0
    assert index["fasta_text_bytes"] == sum(len(t) for t in files.values())
    assert tables == bed_tables


def test_convenience_call(world, tmp_path):
    g, _, _, _, parts, files = world
    assert g.partitions_fasta(str(tmp_path / "deep" / "er"), RUN["window_size"], RUN["merge_distance"],
                              impg_amd.make_params(transitive=True, max_depth=2)) == len(parts)
    check_files(tmp_path / "deep" / "er", files)


# ---- 3. window by window ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
def test_window_fasta(world, tmp_path, host):
    g, _, names, seqs, parts, _ = world
    p = impg_amd.make_params(transitive=True, max_depth=2)
    a = g.partition_session(RUN["window_size"], RUN["merge_distance"], p, state_on_host=host)
    b = g.partition_session(RUN["window_size"], RUN["merge_distance"], p, state_on_host=True)
    path = str(tmp_path / "windows.fasta")
    fd = os.open(path, os.O_WRONLY | os.O_CREAT, 0o666)
    try:
        ws = a.next_windows()
        assert ws == b.next_windows() and len(ws) >= 5
        texts = []
        for k, w in enumerate(ws[:5]):
            rows, text = a.window_fasta(*w)
            assert rows == parts[k][1]  # (a `longest` run's windows all leave a partition)
            assert text == ref.partition_text(rows, names, seqs)
            texts.append(text)
            rows_b, none = b.window_fasta(*w, fd=fd)
            assert rows_b == rows and none is None
            assert os.fstat(fd).st_size == sum(len(t) for t in texts)
        with open(path, "rb") as f:
            assert f.read() == b"".join(texts)
        assert a.counter("fasta_host_windows" if host else "fasta_windows") == 5 and a.counter("partitions") == 5
    finally:
        os.close(fd)
        a.close()
        b.close()


def test_window_without_a_partition(world, cpu, tmp_path):
    """the second pass over a starting sequence finds it masked (the case of tests/test_gpu_partition.py)"""
    g, _, names, seqs, _, _ = world
    ref_run, parts, _ = pr.partition(cpu, RUN["window_size"], RUN["merge_distance"], starting=[3, 3], rehome=False, max_depth=2,
                                     max_windows=1)
    assert ref_run.count["empty_windows"] >= 1
    s = g.partition_session(RUN["window_size"], RUN["merge_distance"], impg_amd.make_params(transitive=True, max_depth=2),
                            starting_sequences=[names[3], names[3]])
    path = str(tmp_path / "w.fasta")
    fd = os.open(path, os.O_WRONLY | os.O_CREAT, 0o666)
    try:
        empty = 0
        got = []
        for w in s.next_windows():
            size = os.fstat(fd).st_size
            rows, none = s.window_fasta(*w, fd=fd)
            if rows:
                got.append(rows)
                assert os.fstat(fd).st_size - size == len(ref.partition_text(rows, names, seqs))
            else:
                empty += 1
                assert os.fstat(fd).st_size == size  # nothing is written
        assert empty == ref_run.count["empty_windows"] and got == [rows for _, rows in parts]
        assert s.counter("fasta_windows") == len(got) == s.counter("partitions")
    finally:
        os.close(fd)
        s.close()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------
def test_run_refusals(paf, world, tmp_path):
    _, _, names, seqs, _, _ = world
    g = impg_amd.GpuImpg.from_paf(paf)
    p = impg_amd.make_params(transitive=True, max_depth=2)
    for store, word in ((None, "sequence store"), (Sequences.from_arrays(names[:7] + names[8:], seqs[:7] + seqs[8:]), "'%s'" % names[7])):
        if store is not None:
            g.set_sequences(store)
        for host in (False, True):
            s = g.partition_session(RUN["window_size"], RUN["merge_distance"], p, state_on_host=host)
            try:
                with pytest.raises(impg_amd.ImpgGpuError) as e:
                    s.run_fasta(str(tmp_path / "refused"))
                assert e.value.code == impg_amd.IMPG_E_INVALID and word in str(e.value)
                assert s.counter("windows") == 0 and not any(s.regions().get("masked").values())
                assert not os.path.exists(tmp_path / "refused")
            finally:
                s.close()


# ---- 5. the command line ----------------------------------------------------------------------------------------------
def test_command_line(paf, cpu, world, tmp_path):
    _, _, names, seqs, parts, files = world
    cli = os.path.join(os.path.dirname(impg_amd.__file__), "impg-gpu")
    fa = str(tmp_path / "seqs.fa")
    with open(fa, "wb") as f:  # lower case and lines of 60: the store upper-cases and joins them
        for nm, sq in zip(names, seqs):
            f.write(b">%s some description\n" % nm.encode())
            f.write(b"".join(sq[i:i + 60].lower() + b"\n" for i in range(0, len(sq), 60)))
    base = [cli, "partition", "-a", paf, "-w", "20000", "-d", "1000", "-m", "2"]
    fasta = base + ["-o", "fasta", "--separate-files", "--sequence-files", fa]
    for k, extra in enumerate(([], ["--host-state"], ["--sequence-store", "packed", "--reverse-complement"])):
        out = tmp_path / ("out%d" % k)
        r = subprocess.run(fasta + extra + ["--output-folder", str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        check_files(out, files)
    single = tmp_path / "single"
    r = subprocess.run(base + ["-o", "fasta", "--sequence-files", fa, "--output-folder", str(single)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Single-file output is only supported for BED format. Use --separate-files for FASTA format." in r.stderr
    assert not single.exists() or os.listdir(single) == []
    r = subprocess.run(base + ["-o", "fasta", "--separate-files", "--output-folder", str(single)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "FASTA index required for FASTA output" in r.stderr
    assert not single.exists() or os.listdir(single) == []
    # BED output is what it was
    rehomed, _ = pr.rehome_singleton_slivers(copy.deepcopy(parts))
    bed = tmp_path / "bed"
    subprocess.run(base + ["-o", "bed", "--output-folder", str(bed)], check=True, timeout=120)
    assert (bed / "partitions.bed").read_text() == pr.bed_text(rehomed, names)
