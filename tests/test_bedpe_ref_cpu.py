"""The model of the device BEDPE route (tests/bedpe_ref.py: per-row summaries, pairwise joins, sums with local
corrections, integer f32 formatting) against the oracle's restatement of merge_adjusted_intervals +
output_results_bedpe (main.rs:11894-11987, :12563-12845), byte for byte, on inputs dense in joins.  No GPU."""
import numpy as np
import pytest

import impg_amd
from oracle import oracle as o
from tests import bedpe_ref as ref
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
            want = c.query_paf(c.seq_name(t), s, e, range_name=rn, merge_distance=d, fmt="bedpe", **kw)
        except RuntimeError:
            with pytest.raises(ref.Refused):
                ref.bedpe_range(rows, cigars, d, rn, c.seq_name, transitive=bool(kw.get("transitive")), min_output_length=min_len)
            continue
        got = ref.bedpe_range(rows, cigars, d, rn, c.seq_name, transitive=bool(kw.get("transitive")), min_output_length=min_len,
                              counters=counters)
        assert got == want, (t, s, e, d, kw)
        lines += want.count("\n")
    return lines


def test_model_equals_oracle_on_dense_tilings(tmp_path):
    """40 seeds x 3 ranges x 6 distances; and the inputs really are dense: the tallies below are the model's own."""
    tally = ref.new_counters()
    ties = 0
    for seed in range(40):
        text, ranges = ref.dense_paf(seed)
        c = o.OracleIndex(paf_text=text, preparse=True)
        rnames = ["r%d" % i for i in range(len(ranges))]
        for d in DISTANCES:
            model_and_oracle(c, ranges, rnames, d, tally)
        for (t, s, e), rn in zip(ranges, rnames):
            ties += c.query_paf(c.seq_name(t), s, e, range_name=rn, merge_distance=-1, fmt="bedpe").count("gi:f:0.007812\t")
    assert tally["bedpe_joins_contiguous"] >= 100 and tally["bedpe_joins_gap"] >= 100 and tally["joins_reverse"] >= 100, tally
    assert tally["fused_at_joins"] >= 100 and tally["fused_in_rows"] >= 100, tally
    assert ties >= 1  # 1=127X: 1/128 = 0.0078125 prints as 0.007812, ties to even


@pytest.mark.parametrize("seed,weird,incons,max_ops", [(91, False, False, 60), (92, True, False, 60), (93, True, True, 200),
                                                        (94, False, False, 12)])
def test_model_equals_oracle_on_random_pafs(seed, weird, incons, max_ops):
    """The inputs and parameters of test_paf_and_bedpe_bytes (tests/test_gpu_parity.py)."""
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


def test_f32_text():
    """format!("{:.6}") of an f32 with the zeros trimmed, from integers alone."""
    for m, den, want in ((1, 128, "0.007812"), (3, 128, "0.023438"), (1, 1, "1"), (0, 5, "0"), (0, 0, "NaN"), (5, 0, "inf"), (-5, 0, "-inf"),
                         (0, -5, "-0"), (1, 3, "0.333333"), (2, 3, "0.666667"), (-1, 3, "-0.333333"), (10, 1, "10"), (1, 10, "0.1"),
                         (2147483647, 1, "2147483648"), (1, 2147483647, "0"), (999999, 1000000, "0.999999")):
        assert ref.fmt_f32(m, den) == want, (m, den)
    # ... and against the C library's correctly rounded "%.6f" of the same f32 quotient
    rng = np.random.default_rng(5)
    for m, den in rng.integers(-50, 3000, size=(3000, 2)).tolist() + [(k, 128) for k in range(1, 128, 2)]:
        if den == 0:
            continue
        text = "%.6f" % float(np.float32(m) / np.float32(den))
        assert ref.fmt_f32(m, den) == text.rstrip("0").rstrip("."), (m, den)


def test_python_entry_point_exists():
    """The binding the GPU tests drive: declared in the header, exported by the library, bound in _lib.SYMBOLS."""
    from impg_amd import _lib
    bound = {n for n, _, _ in _lib.SYMBOLS}
    assert {"impg_gpu_query_batch_bedpe", "impg_gpu_query_batch_bedpe_fd"} <= bound
    assert callable(impg_amd.GpuImpg.query_batch_bedpe)
    assert {"bedpe_rows", "bedpe_runs", "bedpe_joins_contiguous", "bedpe_joins_gap", "bedpe_fused_ops", "bedpe_summary_ops",
            "bedpe_text_pieces", "bedpe_text_bytes"} <= set(impg_amd.counter_keys())
