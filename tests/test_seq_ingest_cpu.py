"""impg_gpu_index_load_sequences without a GPU (impg_amd/csrc/sequence_ingest.cpp): the reader that cuts a file into pieces,
whatever container it comes in, and the whole route with the kernels' host twin in their place
(impg_gpu_selftest_sequence_ingest_host).  The expected store is always the host route's on the uncompressed text:
Sequences.from_fasta, its bases and its exceptions."""
import gzip

import numpy as np
import pytest

import impg_amd
from impg_amd import Sequences, selftest_sequence_ingest_host, selftest_sequence_reader
from tests import seq_ingest_gen as gen

ABSENT = 0xFFFFFFFFFFFFFFFF
DROPPED = "s5_63"  # a file sequence the index lacks
GHOST = ("ghost", 7)  # an index sequence the files lack


@pytest.fixture(scope="module")
def edge(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("seq_ingest_cpu")
    text, seqs = gen.edge_file()
    paths = {kind: gen.put(tmp, "edge." + kind, data) for kind, data in gen.containers(text).items()}
    host = Sequences.from_fasta(paths["plain"])
    assert host.items() == gen.stored(seqs)
    names = [nm for nm, _ in seqs if nm != DROPPED] + [GHOST[0]]
    lens = [len(b) for nm, b in seqs if nm != DROPPED] + [GHOST[1]]
    return text, seqs, paths, host, names, lens


def test_edge_file_is_what_the_issue_asks_for(edge):
    text, seqs, _, host, _, _ = edge
    assert [len(b) for _, b in seqs] == gen.EDGE_LENGTHS and 3000 < len(text) < 4200
    assert b"\r\n" in text and b"\n\n" in text and not text.endswith(b"\n") and b" x=1" in text and b"\td" in text
    assert any(b">" in b for _, b in seqs) and any(b != b.upper() for _, b in seqs)
    runs = {nm: host.exceptions(i) for i, (nm, _) in enumerate(seqs)}
    s, n, c = runs["s13_1025"]
    assert any(a < 1024 < a + k for a, k in zip(s.tolist(), n.tolist())) and int(s[-1] + n[-1]) == 1025 and int(s[0]) == 0
    assert [x.tolist() for x in runs["s6_64"]] == [[0], [64], [ord("N")]]
    assert any(c.tolist()[i:i + 2] == [ord("N"), ord("R")] and s[i] + n[i] == s[i + 1] for i in range(len(s) - 1))


def test_piece_sizes_meet_every_kind_of_edge(edge):
    """a condition on the tests' inputs: the piece sizes used here and on the GPU cut the edge file inside a name, right
    after '>', between \\r and \\n, between \\n and '>', inside a description, inside a run, on a 16-base word edge and inside
    a word, at a sequence's last base and inside an empty line"""
    text = edge[0]
    met = set()
    for size in gen.PIECE_SIZES:
        assert size % 16 == 0
        met |= gen.edge_kinds(text, size)
    assert met == set(gen.EDGE_KINDS)


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf", "members"])
def test_reader_pieces_are_the_text(edge, kind):
    text, _, paths, _, _, _ = edge
    for size in (16, 48, 80, 4096, gen.DEFAULT_PIECE):
        got, n, blocks = selftest_sequence_reader(paths[kind], size)
        assert got == text and n == len(gen.pieces(text, size))
        assert blocks == (5 if kind == "bgzf" else 0)  # (blocks of 1, 100 and 65 280 input bytes, an empty one, the EOF block)


def test_reader_bgzf_block_shapes(tmp_path):
    """blocks of 65 280 bytes that cross several pieces, a block that ends on a piece's edge, no EOF block, an empty file"""
    rng = np.random.default_rng(5)
    data = bytes(np.frombuffer(b"ACGTN\n", dtype=np.uint8)[rng.integers(0, 6, size=200000)])
    for sizes, eof in (((65280,), True), ((4096,), False), ((1, 65280, 15), True)):
        path = gen.put(tmp_path, "x.bgz", gen.bgzf(data, sizes, eof=eof))
        for piece in (4096, 65536, 1 << 20):
            got, n, _ = selftest_sequence_reader(path, piece)
            assert got == data and n == (len(data) + piece - 1) // piece
    for blob in (b"", gen.BGZF_EOF, gzip.compress(b"")):
        assert selftest_sequence_reader(gen.put(tmp_path, "e.gz", blob), 64)[:2] == (b"", 0)


def check_store(got, host, seqs, names, lens, packed):
    by_name = {nm: i for i, (nm, _) in enumerate(seqs)}
    places = []
    for i, (nm, n) in enumerate(zip(names, lens)):
        off = int(got["off"][i])
        assert (off == ABSENT) == (nm not in by_name), nm  # per-id presence
        r0, r1 = int(got["run_off"][i]), int(got["run_off"][i + 1])
        if off == ABSENT:
            assert r0 == r1
            continue
        want = host.bases(by_name[nm])
        rs, re_, rb = got["run_start"][r0:r1], got["run_end"][r0:r1], got["run_byte"][r0:r1]
        if packed:
            assert off % 64 == 0 and off >= 64
            assert gen.unpack(got["store"], off, n, rs, re_, rb) == want, nm
            s, k, c = host.exceptions(by_name[nm])
            assert (rs.tolist(), (re_ - rs).tolist(), rb.tolist()) == (s.tolist(), k.tolist(), c.tolist()), nm
        else:
            assert off >= 16 and r0 == r1
            assert got["store"][off:off + n].tobytes() == want, nm
        places.append((off, n))
    places.sort()
    assert all(a + n <= b for (a, n), (b, _) in zip(places, places[1:]))  # no two sequences share a place
    return places


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("kind", ["plain", "bgzf"])
def test_twin_store_is_the_host_route_s(edge, kind, packed):
    text, seqs, paths, host, names, lens = edge
    first = None
    for size in gen.PIECE_SIZES + [gen.DEFAULT_PIECE]:
        got = selftest_sequence_ingest_host(paths[kind], names, lens, size, packed)
        check_store(got, host, seqs, names, lens, packed)
        assert got["stats"].tolist()[:3] == [gen.n_pieces([text], size), len(text), sum(gen.EDGE_LENGTHS)]
        assert got["stats"][4] == 1 and (got["stats"][3] > 0) == (kind == "bgzf")
        key = (got["off"].tolist(), got["store"].tobytes(), got["run_start"].tolist(), got["run_end"].tolist())
        first = first or key
        assert key == first  # identical at every piece size


def test_twin_several_files_in_file_order(edge, tmp_path):
    """two files in one call, the second one's sequences first in the index: places follow the files, a file's end closes its
    last record and nothing carries over into the next file"""
    _, seqs, paths, host, names, lens = edge
    a = gen.put(tmp_path, "a.fa", b">x\nacgtNN")  # (no newline: the next file starts a new line whatever this one ends in)
    for packed in (False, True):
        got = selftest_sequence_ingest_host([a, paths["gzip"]], ["x"] + names, [6] + lens, 32, packed)
        rest = dict(got, off=got["off"][1:], run_off=got["run_off"][1:])  # (ids 1 .. are the edge file's)
        places = check_store(rest, host, seqs, names, lens, packed)
        off = int(got["off"][0])
        assert off < places[0][0]
        if packed:
            assert gen.unpack(got["store"], off, 6, got["run_start"][:1], got["run_end"][:1], got["run_byte"][:1]) == b"ACGTNN"
        else:
            assert got["store"][off:off + 6].tobytes() == b"ACGTNN"


def refused(paths, names, lens, piece=32, packed=False):
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        selftest_sequence_ingest_host(paths, names, lens, piece, packed)
    return e.value.code, str(e.value)


def test_errors(tmp_path):
    for key, (paths, names, lens, code, words) in gen.malformed(tmp_path).items():
        for packed in (False, True):
            got = refused(paths, names, lens, 32, packed)
            assert got[0] == code and words in got[1], (key, got)
            if code == -4:
                assert paths[-1] in got[1], (key, got)  # an input error names the file
    # ... and the same refusals in one piece
    for key in ("duplicate across pieces", "wrong CRC", "one base longer"):
        paths, names, lens, code, words = gen.malformed(tmp_path)[key]
        got = refused(paths, names, lens, gen.DEFAULT_PIECE)
        assert got[0] == code and words in got[1], (key, got)
    good = gen.put(tmp_path, "good.fa", b">a\nACGT\n")
    assert refused([good], ["a"], [4], piece=24)[0] == -1 and refused([good], ["a"], [4], piece=0)[0] == -1
    assert selftest_sequence_ingest_host([good], ["a"], [4], 16, False)["store"][16:20].tobytes() == b"ACGT"


def test_a_wrong_file_never_writes_outside_its_sequence(tmp_path):
    """a sequence far longer than the index says: the bases beyond its length are counted and never written -- its neighbour
    and the padding stay as they are (seen through the twin's store before the length error: here the error itself)"""
    path = gen.put(tmp_path, "w.fa", b">a\n" + b"T" * 500 + b"\n>b\nGG\n")
    for packed in (False, True):
        code, msg = refused([path], ["a", "b"], [4, 2], 64, packed)
        assert code == -1 and "'a' has 500 bases in the sequence files and 4 in the index" in msg


def test_from_fasta_still_refuses_gzip_and_the_option_is_registered(edge):
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        Sequences.from_fasta(edge[2]["bgzf"])
    assert e.value.code == impg_amd.IMPG_E_UNSUPPORTED
    assert "sequence_ingest_piece_bytes" in impg_amd.option_keys()
    assert {"sequence_ingest_pieces", "sequence_ingest_text_bytes", "sequence_ingest_bases", "sequence_ingest_inflated_blocks",
            "sequence_ingest_dropped_sequences"} <= set(impg_amd.counter_keys())
