"""The host side of FASTA output (impg_amd/csrc/sequences.cpp), without a GPU: the FASTA parser of the sequence store,
and impg_gpu_fasta_text -- the query-axis sweep and the records -- against the restatement of tests/fasta_ref.py."""
import numpy as np
import pytest

import impg_amd
from impg_amd import INTERVAL_DTYPE, Sequences, fasta_text
from tests import fasta_ref as ref


def put(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


# ---- the parser ---------------------------------------------------------------------------------------------------------
def test_parser_multi_line_bodies_and_one_long_line(tmp_path):
    long_line = b"ACGT" * 5000
    path = put(tmp_path, "a.fa", b">one\nACGT\nAC\nGTTTT\n>two\n" + long_line + b"\n")
    s = Sequences.from_fasta(path)
    assert len(s) == 2
    assert s.items() == [("one", b"ACGTACGTTTT"), ("two", long_line)]


def test_parser_crlf_lower_case_and_description(tmp_path):
    path = put(tmp_path, "a.fa", b">chr1 Homo sapiens chromosome 1\r\nacgtn\r\nRykm\r\n>chr2\tx\r\nNnNn\r\n")
    s = Sequences.from_fasta([path])
    assert s.items() == [("chr1", b"ACGTNRYKM"), ("chr2", b"NNNN")]


def test_parser_empty_sequence_and_no_final_newline(tmp_path):
    path = put(tmp_path, "a.fa", b">empty\n>mid\nAC\n\n>alsoempty\n>last\nACG\nTT")
    s = Sequences.from_fasta(path)
    assert s.items() == [("empty", b""), ("mid", b"AC"), ("alsoempty", b""), ("last", b"ACGTT")]
    path = put(tmp_path, "b.fa", b">only")
    assert Sequences.from_fasta(path).items() == [("only", b"")]


def test_parser_several_files_keep_their_order(tmp_path):
    a = put(tmp_path, "a.fa", b">x\nAC\n")
    b = put(tmp_path, "b.fa", b">y\nGT\n")
    assert Sequences.from_fasta([b, a]).items() == [("y", b"GT"), ("x", b"AC")]


def test_parser_refuses_gzip(tmp_path):
    path = put(tmp_path, "a.fa.gz", b"\x1f\x8b\x08\x00" + b"\x00" * 20)
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        Sequences.from_fasta(path)
    assert e.value.code == impg_amd.IMPG_E_UNSUPPORTED


def test_parser_refuses_duplicate_names(tmp_path):
    one = put(tmp_path, "a.fa", b">x\nAC\n>dup first\nA\n>dup second\nC\n")
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        Sequences.from_fasta(one)
    assert e.value.code == impg_amd.IMPG_E_INVALID and "'dup'" in str(e.value)
    a = put(tmp_path, "b.fa", b">p\nAC\n")
    b = put(tmp_path, "c.fa", b">q\nAC\n>p\nGG\n")
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        Sequences.from_fasta([a, b])
    assert e.value.code == impg_amd.IMPG_E_INVALID and "'p'" in str(e.value)
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        Sequences.from_arrays(["p", "p"], [b"A", b"C"])
    assert e.value.code == impg_amd.IMPG_E_INVALID


def test_parser_refuses_a_missing_file_and_text_without_header(tmp_path):
    with pytest.raises(impg_amd.ImpgGpuError):
        Sequences.from_fasta(str(tmp_path / "nothing.fa"))
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        Sequences.from_fasta(put(tmp_path, "a.fa", b"ACGT\n>x\nAC\n"))
    assert e.value.code == impg_amd.IMPG_E_INVALID


def test_from_arrays_upper_cases():
    s = Sequences.from_arrays(["a", "b", "c"], [b"acgtRYkm", "", "nN"])
    assert s.items() == [("a", b"ACGTRYKM"), ("b", b""), ("c", b"NN")]


# ---- the text ------------------------------------------------------------------------------------------------------------
N_SEQ, SEQ_LEN = 4, 3000


@pytest.fixture(scope="module")
def store():
    rng = np.random.default_rng(20251)
    names = ["s%d" % i for i in range(N_SEQ)]
    seqs = [ref.random_sequence(rng, SEQ_LEN) for _ in range(N_SEQ)]
    return names, seqs, Sequences.from_arrays(names, seqs)


def random_rows(rng, n):
    """rows that overlap, abut and lie up to 60 bases apart, both strands, a few of no length"""
    rows = np.zeros(n, dtype=INTERVAL_DTYPE)
    for r in rows:
        ln = 0 if rng.random() < 0.05 else int(rng.integers(1, 400))
        a = int(rng.integers(0, SEQ_LEN - ln + 1)) if rng.random() < 0.5 else int(rng.integers(0, 12)) * 100
        a = min(a, SEQ_LEN - ln)
        fwd = rng.random() < 0.5
        r["query_id"] = int(rng.integers(0, N_SEQ))
        r["q_first"], r["q_last"] = (a, a + ln) if fwd else (a + ln, a)
        r["target_id"] = int(rng.integers(0, N_SEQ))
        r["t_first"], r["t_last"] = 0, ln
    return rows


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("d", [-1, 0, 50])
def test_fasta_text_is_the_restatement(store, d, rc):
    """300 seeded row sets of 0 .. 24 rows: the sweep keeps the strands apart, d < 0 keeps the emission order"""
    names, seqs, st = store
    rng = np.random.default_rng(77 + d)
    merged_some = reverse_some = 0
    for _ in range(300):
        rows = random_rows(rng, int(rng.integers(0, 25)))
        want = ref.fasta_range(rows, d, rc, lambda i: names[i], lambda i: seqs[i])
        got = fasta_text(st, names, rows, merge_distance=d, reverse_complement=rc)
        assert got == want
        merged_some += want.count(b">") < rows.size
        reverse_some += b"/rc\n" in want
    assert (merged_some > 100) == (d >= 0) and (reverse_some > 100) == rc


@pytest.mark.parametrize("L", [0, 1, 79, 80, 81, 160, 161])
def test_length_table(store, L):
    """the body of L bases is L + ceil(L / 80) bytes, the single newline for L = 0"""
    names, seqs, st = store
    for fwd in (True, False):
        rows = np.zeros(1, dtype=INTERVAL_DTYPE)
        rows[0]["query_id"] = 2
        rows[0]["q_first"], rows[0]["q_last"] = (7, 7 + L) if fwd else (7 + L, 7)
        for rc in (False, True):
            got = fasta_text(st, names, rows, merge_distance=0, reverse_complement=rc)
            header = b">s2:7-%d%s\n" % (7 + L, b"/rc" if rc and not fwd and L else b"")  # (first == last reads as '+')
            assert got.startswith(header)
            body = got[len(header):]
            assert len(body) == ref.body_len(L) == {0: 1, 1: 2, 79: 80, 80: 81, 81: 83, 160: 162, 161: 164}[L]
            assert got == ref.record("s2", seqs[2], int(rows[0]["q_first"]), int(rows[0]["q_last"]), rc)
            assert body.endswith(b"\n") and all(len(ln) == 80 for ln in body.split(b"\n")[:-2])


def test_refusals(store):
    names, seqs, st = store
    rows = np.zeros(1, dtype=INTERVAL_DTYPE)
    rows[0]["query_id"], rows[0]["q_first"], rows[0]["q_last"] = 1, 10, 20
    with pytest.raises(impg_amd.ImpgGpuError) as e:  # a sequence the store lacks: named
        fasta_text(st, ["s0", "elsewhere"], rows)
    assert e.value.code == impg_amd.IMPG_E_INVALID and "'elsewhere'" in str(e.value)
    rows[0]["q_last"] = SEQ_LEN + 1
    with pytest.raises(impg_amd.ImpgGpuError) as e:  # a row that leaves its sequence
        fasta_text(st, names, rows)
    assert e.value.code == impg_amd.IMPG_E_INVALID and "s1" in str(e.value)
