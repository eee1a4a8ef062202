"""impg_gpu_partition_fasta_text (impg_amd/csrc/sequences.cpp): the host writer of `impg partition -o fasta`, against the
restatement of tests/partition_fasta_ref.py.  No GPU."""
import numpy as np
import pytest

import impg_amd
from impg_amd import INTERVAL_DTYPE, Sequences
from tests import fasta_ref
from tests import partition_fasta_ref as ref

BODY_LENGTHS = [0, 1, 2, 15, 16, 17, 79, 80, 81, 82, 159, 160, 161, 162, 1000]
NAMES = ["a", "sample#1#chromosome_30_letters"]
SEQ_LEN = 1500


@pytest.fixture(scope="module")
def store():
    assert [len(n) for n in NAMES] == [1, 30]
    rng = np.random.default_rng(1630)
    seqs = [fasta_ref.random_sequence(rng, SEQ_LEN) for _ in NAMES]
    assert any(c in seqs[0] for c in b"acgtn") and any(c in seqs[0] for c in b"RYKM")  # lower case and IUPAC bytes are there
    return Sequences.from_arrays(NAMES, seqs), seqs


def rows_of(L):
    """the body length at a sequence's first bases, at its last ones and inside it, on both names"""
    return [(s, a, a + L) for s in range(len(NAMES)) for a in (0, SEQ_LEN - L, 37)]


@pytest.mark.parametrize("L", BODY_LENGTHS)
def test_text_is_the_restatement(store, L):
    st, seqs = store
    rows = rows_of(L)
    got = impg_amd.partition_fasta_text(st, NAMES, rows)
    assert got == ref.partition_text(rows, NAMES, seqs)
    assert len(got) == sum(len(">%s:%d-%d\n" % (NAMES[s], a, b)) + ref.body_len(L) for s, a, b in rows)


def test_all_lengths_in_one_text_keep_their_order(store):
    st, seqs = store
    rows = [r for L in reversed(BODY_LENGTHS) for r in rows_of(L)]
    assert impg_amd.partition_fasta_text(st, NAMES, rows) == ref.partition_text(rows, NAMES, seqs)
    assert impg_amd.partition_fasta_text(st, NAMES, []) == b""


def test_a_record_of_no_bases_is_its_header_alone(store):
    st, _ = store
    assert impg_amd.partition_fasta_text(st, NAMES, [(0, 5, 5)]) == b">a:5-5\n"
    assert impg_amd.partition_fasta_text(st, NAMES, [(0, 5, 5), (0, 6, 7)]).startswith(b">a:5-5\n>a:6-7\n")
    # ... and the query writer on the same row still prints its empty line
    row = np.zeros(1, dtype=INTERVAL_DTYPE)
    row[0]["query_id"], row[0]["q_first"], row[0]["q_last"] = 0, 5, 5
    assert impg_amd.fasta_text(st, NAMES, row, merge_distance=-1) == b">a:5-5\n\n"


@pytest.mark.parametrize("rows, word", [([(0, 10, SEQ_LEN + 1)], "leaves its sequence"), ([(0, 20, 10)], "leaves its sequence"),
                                        ([(0, -1, 10)], "leaves its sequence"), ([(0, 0, 10), (2, 0, 10)], "not found")])
def test_refusals(store, rows, word):
    st, _ = store
    names = NAMES + ["elsewhere"]  # the index knows a sequence the store lacks
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        impg_amd.partition_fasta_text(st, names, rows)
    assert e.value.code == impg_amd.IMPG_E_INVALID and word in str(e.value)
