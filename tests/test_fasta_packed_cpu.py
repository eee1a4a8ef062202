"""The packed sequence store's exceptions (impg_gpu_sequences_exceptions, host-only): the maximal runs of one byte that is
not A/C/G/T after upper-casing, as impg_gpu_index_set_sequences extracts them at attach, against a numpy restatement; and the
keys the packed store adds to the option and counter tables."""
import numpy as np
import pytest

import impg_amd
from impg_amd import Sequences
from tests import fasta_ref as ref


def restated_runs(seq):
    """(start, length, byte) of every maximal run of one non-ACGT byte of the upper-cased sequence"""
    b = np.frombuffer(seq.upper(), dtype=np.uint8)
    if b.size == 0:
        return [np.zeros(0, dtype=np.int64)] * 3
    first = np.ones(b.size, dtype=bool)
    first[1:] = b[1:] != b[:-1]  # a byte that differs from the one before it starts a stretch
    start = np.flatnonzero(first)
    length = np.diff(np.append(start, b.size))
    keep = ~np.isin(b[start], np.frombuffer(b"ACGT", dtype=np.uint8))
    return start[keep], length[keep], b[start][keep]


CASES = {
    "empty": b"",
    "all_n": b"N" * 300,
    "pure": b"ACGT" * 75 + b"GATTACA",
    "first_base": b"NN" + b"ACGT" * 20,
    "last_base": b"ACGT" * 20 + b"N",
    "first_and_last": b"R" + b"ACGT" * 20 + b"YYY",
    "three_runs": b"NNNRRN",
    "lower_case": b"acgtnnNNacgtNnrRacgt",
    "dense": ref.random_sequence(np.random.default_rng(7), 5000),
}


@pytest.fixture(scope="module")
def store():
    return Sequences.from_arrays(list(CASES), list(CASES.values()))


@pytest.mark.parametrize("k", range(len(CASES)), ids=list(CASES))
def test_exceptions_match_the_restatement(store, k):
    seq = list(CASES.values())[k]
    start, length, byte = store.exceptions(k)
    want = restated_runs(seq)
    assert (start.dtype, length.dtype, byte.dtype) == (np.uint32, np.uint32, np.uint8)
    assert start.tolist() == want[0].tolist() and length.tolist() == want[1].tolist() and byte.tolist() == want[2].tolist()


def test_known_answers(store):
    names = list(CASES)
    as_tuples = lambda k: list(zip(*(a.tolist() for a in store.exceptions(names.index(k)))))
    assert as_tuples("empty") == [] and as_tuples("pure") == []
    assert as_tuples("all_n") == [(0, 300, ord("N"))]
    assert as_tuples("three_runs") == [(0, 3, ord("N")), (3, 2, ord("R")), (5, 1, ord("N"))]  # adjacent runs of different bytes stay apart
    assert as_tuples("lower_case") == [(4, 4, ord("N")), (12, 2, ord("N")), (14, 2, ord("R"))]  # 'n' joins 'N'
    assert as_tuples("last_base") == [(80, 1, ord("N"))] and as_tuples("first_base") == [(0, 2, ord("N"))]
    dense = store.exceptions(names.index("dense"))
    assert dense[0].size > 1000 and int(dense[1].sum()) == sum(c not in b"ACGT" for c in CASES["dense"].upper())
    with pytest.raises(IndexError):
        store.exceptions(len(CASES))


def test_capacity_and_arguments(store):
    """the C call writes at most `cap` runs and always says how many there are"""
    import ctypes as C
    L = impg_amd.lib()
    k = list(CASES).index("three_runs")
    n = C.c_size_t(99)
    assert L.impg_gpu_sequences_exceptions(store._h, k, None, None, None, 0, C.byref(n)) == 0 and n.value == 3
    start, length, byte = np.full(2, 77, dtype=np.uint32), np.full(2, 77, dtype=np.uint32), np.full(2, 77, dtype=np.uint8)
    assert L.impg_gpu_sequences_exceptions(store._h, k, start.ctypes.data, length.ctypes.data, byte.ctypes.data, 2, C.byref(n)) == 0
    assert n.value == 3 and start.tolist() == [0, 3] and length.tolist() == [3, 2] and byte.tolist() == [ord("N"), ord("R")]
    assert L.impg_gpu_sequences_exceptions(store._h, len(CASES), None, None, None, 0, C.byref(n)) == impg_amd.IMPG_E_INVALID
    assert L.impg_gpu_sequences_exceptions(store._h, k, None, None, None, 0, None) == impg_amd.IMPG_E_INVALID


def test_keys_are_enumerated():
    from impg_amd import _lib
    assert "sequence_store_packed" in impg_amd.option_keys()
    assert {"fasta_store_bytes", "fasta_store_packed", "fasta_store_exception_runs"} <= set(impg_amd.counter_keys())
    assert "impg_gpu_sequences_exceptions" in {n for n, _, _ in _lib.SYMBOLS}
    assert callable(Sequences.exceptions)
