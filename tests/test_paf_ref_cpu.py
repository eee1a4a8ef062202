"""The model of the device PAF route (tests/paf_ref.py: elements, per-element summaries, a suffix scan, every element
printing the groups that start in it) against the oracle's restatement of merge_adjusted_intervals + output_results_paf
(main.rs:11989-12103, :12563-12845), byte for byte, on inputs dense in joins and on chains of one-op rows.  No GPU."""
import pytest

import impg_amd
from oracle import oracle as o
from tests import bedpe_ref, paf_ref as ref
from tests.paf_gen import random_paf, random_ranges

DISTANCES = (-1, 0, 1, 2, 5, 100)


def model_and_oracle(c, ranges, rnames, d, counters, **kw):
    """Every range through both; a range the oracle refuses must be refused by the model.  Returns the lines compared."""
    lines = 0
    min_len = -1 if kw.get("min_output_length") is None else kw["min_output_length"]
    for (t, s, e), rn in zip(ranges, rnames):
        rows, cigars = c.query_cigar(t, s, e, **kw)
        rows = [(r["query_id"], r["q_first"], r["q_last"], r["target_id"], r["t_first"], r["t_last"]) for r in rows]
        try:
            want = c.query_paf(c.seq_name(t), s, e, range_name=rn, merge_distance=d, fmt="paf", **kw)
        except RuntimeError:
            with pytest.raises(ref.Refused):
                ref.paf_range(rows, cigars, d, rn, c.seq_name, c.seq_len, transitive=bool(kw.get("transitive")), min_output_length=min_len)
            continue
        got = ref.paf_range(rows, cigars, d, rn, c.seq_name, c.seq_len, transitive=bool(kw.get("transitive")), min_output_length=min_len,
                            counters=counters)
        assert got == want, (t, s, e, d, kw)
        lines += want.count("\n")
    return lines


def test_model_equals_oracle_on_dense_tilings():
    """40 seeds x 3 ranges x 6 distances; and the inputs are as dense as claimed (the oracle-checked model counts 1 842
    runs of more than one row, 860 of them on the reverse strand)."""
    tally = ref.new_counters()
    lines = 0
    for seed in range(40):
        text, ranges = bedpe_ref.dense_paf(seed)
        c = o.OracleIndex(paf_text=text, preparse=True)
        rnames = ["r%d" % i for i in range(len(ranges))]
        for d in DISTANCES:
            lines += model_and_oracle(c, ranges, rnames, d, tally)
    assert lines > 5000 and tally["multi_runs"] >= 1000 and tally["reverse_multi_runs"] >= 500, (lines, tally)
    assert tally["paf_joins_contiguous"] >= 100 and tally["paf_joins_gap"] >= 100, tally


@pytest.mark.parametrize("seed,weird,incons,max_ops", [(91, False, False, 60), (92, True, False, 60), (93, True, True, 200),
                                                        (94, False, False, 12)])
def test_model_equals_oracle_on_random_pafs(seed, weird, incons, max_ops):
    """The inputs and parameters of test_model_equals_oracle_on_random_pafs (tests/test_bedpe_ref_cpu.py)."""
    sl = 30000
    text, names = random_paf(seed, 300, n_seq=5, seq_len=sl, max_ops=max_ops, weird=weird, inconsistent=incons, self_aln=True)
    c = o.OracleIndex(paf_text=text, preparse=True)
    ranges = random_ranges(seed, 60, 5, sl, max_len=6000, min_len=150)
    rnames = ["r%d" % i for i in range(len(ranges))]
    lines = 0
    for kw in [dict(), dict(transitive=True, max_depth=2), dict(transitive=True, dfs=True, max_depth=3, min_transitive_len=50),
               dict(min_identity=0.7), dict(min_output_length=300)]:
        for d in (-1, 0, 25, 1000):
            lines += model_and_oracle(c, ranges, rnames, d, ref.new_counters(), **kw)
    assert lines > 1000


def test_model_equals_oracle_on_chains():
    """Rows of one op each, neighbours often of one code: groups run through whole rows, on both strands."""
    tally = ref.new_counters()
    for seed in range(12):
        text, ranges = ref.chain_paf(seed)
        c = o.OracleIndex(paf_text=text, preparse=True)
        rnames = ["c%d" % i for i in range(len(ranges))]
        for d in (-1, 0, 1, 5):
            model_and_oracle(c, ranges, rnames, d, tally, min_transitive_len=1)
    assert tally["paf_through_rows"] >= 20 and tally["reverse_through_rows"] >= 1, tally
    assert tally["paf_joins_contiguous"] >= 20 and tally["paf_joins_gap"] >= 20, tally


def test_run_cigar_by_hand():
    """the formulation on strings small enough to fuse by eye"""
    P = lambda cg: [(int(v) >> 29, int(v) & bedpe_ref.OP_LEN_MASK) for v in ref.pack(cg)]
    show = lambda ops: "".join("%d%s" % (ln, ref.OP_CHARS[code]) for code, ln in ops)
    tally = ref.new_counters()
    assert show(ref.run_cigar([P("4="), P("6=")], tally)) == "10=" and tally["paf_through_rows"] == 1
    assert show(ref.run_cigar([P("5=2I3I10="), P("0=5=")])) == "5=5I15="
    assert show(ref.run_cigar([P("3="), P("4="), P("5="), P("2X"), P("1X1=")], tally)) == "12=3X1="
    assert tally["paf_through_rows"] == 3  # the second 6= above, then 4= and 5=; 1X1= prints its 1=
    assert show(ref.run_cigar([P("17=3I"), P("2I") + P("2I20=")])) == "17=7I20="  # a gap's I between a trailing and a leading I
    assert show(ref.run_cigar([P("4D4D12="), P("3D") + P("1D5=")])) == "8D12=4D5="


def test_python_entry_points_exist():
    """The bindings the GPU tests drive: declared in the header, exported by the library, bound in _lib.SYMBOLS."""
    from impg_amd import _lib
    bound = {n for n, _, _ in _lib.SYMBOLS}
    assert {"impg_gpu_query_batch_paf", "impg_gpu_query_batch_paf_fd", "impg_gpu_selftest_paf_rows"} <= bound
    assert callable(impg_amd.GpuImpg.query_batch_paf) and callable(impg_amd.GpuImpg.selftest_paf_rows)
    assert {"paf_rows", "paf_runs", "paf_joins_contiguous", "paf_joins_gap", "paf_ops_read", "paf_ops_printed", "paf_through_rows",
            "paf_text_pieces", "paf_text_bytes"} <= set(impg_amd.counter_keys())
    assert "paf_group_log2" in impg_amd.option_keys()
