"""tests/update_gen.py's cases reach what they are built for -- asserted from the plain model alone -- and the oracle runs
each of them through levels that come back to the group.  No GPU: tests/test_gpu_update_tiers.py runs the same cases on the
engine."""
import pytest

from oracle import oracle as o
from tests import update_gen as ug


@pytest.fixture(scope="module", autouse=True)
def sorted_visits():
    o.set_sorted_visits(True)  # (a level's hits in the order of their records on T: the order the cases are written in)
    yield
    o.set_sorted_visits(False)


@pytest.mark.parametrize("name", list(ug.CASES))
def test_case_reaches_what_it_is_built_for(name):
    case = ug.CASES[name]
    if case.reps == 1:
        got = case.model()
        want = {k: v for k, v in case.expect.items()}
        assert {k: got[k] for k in want} == want, (name, got)
    else:  # one hit per query: every query's group by itself
        for h in case.hits:
            got = ug.model(case.mask, [h], case.lq)
            assert (got["cap"], got["old"], got["tier"]) == (case.expect["cap"], case.expect["old"], case.expect["tier"]), (name, h, got)
            assert got["raw_pieces"] == 1 and not (got["inplace"] or got["tiled"] or got["spill"])
        assert len(case.hits) * case.reps == case.expect["groups"]
    # hits and mask are what the PAF says: inside the sequence, the mask sorted and disjoint
    assert all(0 <= s < e <= case.lq for s, e in case.hits + case.mask)
    assert all(a[1] < b[0] for a, b in zip(case.mask, case.mask[1:]))


def test_every_path_has_a_case_and_a_neighbour():
    """Each tier and each rare path is reached by some case and left alone by another, with and without the pre-pass."""
    seen = [c.model(f) for c in ug.CASES.values() if c.reps == 1 for f in (False, True)]
    assert {m["tier"] for m in seen} == {"lane", "mid", "tiny", "small", "large"}
    for key in ("inplace", "tiled", "spill"):
        assert {bool(m[key]) for m in seen} == {False, True}, key
    for tier in ug.WAVE_CAP:
        assert {bool(m["tiled"]) for m in seen if m["tier"] == tier} == {False, True}, tier
    for tier in ("small", "large"):
        assert {bool(m["inplace"]) for m in seen if m["tier"] == tier} == {False, True}, tier
    assert any(m["leave"] == 0 for m in seen) and any(m["leave"] for m in seen)
    for tier in ("lane", "mid"):
        assert {bool(m["spill"]) for m in seen if m["tier"] == tier} == {False, True}, tier
    cross = ug.CASES["covered-49-to-48"]
    assert (cross.model(False)["tier"], cross.model(True)["tier"]) == ("tiny", "mid")
    # the lists longer than one round of their grid
    assert ug.CASES["many-mid"].expect["groups"] > ug.MID_GRID and ug.CASES["many-tiny"].expect["groups"] > ug.TINY_GRID


@pytest.mark.parametrize("name", list(ug.CASES))
def test_oracle_runs_the_case(name):
    case = ug.CASES[name]
    text, ranges = case.paf()
    c = o.OracleIndex(paf_text=text, bidirectional=False, preparse=True)
    masked = case.masked(c.seq_id) if case.mask else None
    H = len(case.hits)
    for t, s, e in ranges[:H if case.reps > 1 else 1]:
        rows = c.query(c.seq_id(t), s, e, masked_regions=masked, **case.kw(max_depth=4))
        assert len(rows) > (H if case.reps == 1 else 1), (name, len(rows))
        if case.reps == 1:  # levels 3 and 4 come back to Q: rows whose target is R and whose query is Q
            back = rows[(rows["target_id"] == c.seq_id("R")) & (rows["query_id"] == c.seq_id("Q"))]
            assert len(back) > 0, name
            if name.startswith("touching-chain"):  # level 3's tier tells a merged list (M ranges) from an unmerged one (3 M)
                r3 = c.query(c.seq_id(t), s, e, masked_regions=masked, **case.kw(max_depth=3))
                h3 = int(((r3["target_id"] == c.seq_id("R")) & (r3["query_id"] == c.seq_id("Q"))).sum())
                M = len(case.mask)
                assert h3 > 0 and ug.tier_of(M + h3, M) != ug.tier_of(3 * M + h3, 3 * M), (name, h3)
