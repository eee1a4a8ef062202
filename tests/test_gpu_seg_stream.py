"""The update's slot stream (kernels.hip, seg_for_chunks) at its edges, against the oracle.

seg_group_kernel walks the slots of a query's frontier ranges as one flat stream: 64 ranges a base, 64 slots a chunk,
SEG_U = 4 chunks a group (256 slots).  One PAF holds every shape as a query of its own, so the index and the oracle are
built once.  Its sequences: T (the queries), A1 and A2 (the level-2 frontier), B0 .. B4 (the level-2 hits) and C.

  level 1  a query's range on T covers N records A? <- T: N hits, each a piece of its own on A1 / A2, so the level-2
           frontier of the query is N ranges, A1's before A2's, in the order they are written here (sorted by start).
  level 2  the range's window on A? holds L records B? <- A?, their starts two bases apart: its run is L slots, the
           sequence changing from hit to hit (B(k + i) % 5), so a chunk's ballots see every sequence.  "S" runs are
           records A? <- A? (the hit lies on the range's own target: it carries no key), "X" runs come from the OTHER A.
  level 3  one record C <- B? over all of B?, and one over the zone of A? where the S and X hits lie: every piece the
           level-2 update leaves -- and any it loses, misplaces or invents -- is a row of the -m 3 result.

So -m 2 has the level-1 update (one range, a run of N slots) and -m 3 the level-2 update (N ranges, runs of L).  The
shape of every query is asserted from query_batch_stats' counts (N = rows at depth 1, the base's total = rows at depth 2
less those) and from the oracle's rows (each run's length): a generator that degenerates fails instead of passing."""
import numpy as np
import pytest

import impg_amd
from oracle import oracle as o
from tests.test_gpu_fullsize import checksum

pytestmark = pytest.mark.gpu

HL = 110        # a record's length: pieces pass the default min_transitive_len (101)
GAP = 40        # between two pieces on one sequence: beyond the default min_distance_between_ranges (10)
ZONE = 3_000_000  # where the S and X hits lie on A1 / A2; the windows stay below
SEG_COUNTERS = ("segment_sliced_levels", "segment_retries", "segment_library_levels")


class Gen:
    """queries: name -> list of (sequence "A1" / "A2", kind "B" / "S" / "X", L), A1's ranges first."""

    def __init__(self):
        self.lines, self.next, self.queries = [], {}, {}
        self.next["A1z"] = self.next["A2z"] = ZONE

    def take(self, seq, n, gap=GAP):
        a = self.next.get(seq, 1000)
        self.next[seq] = a + n + gap
        return a

    def rec(self, q, qs, t, ts, n, k):
        self.lines.append("%s\tLEN_%s\t%d\t%d\t%s\t%s\tLEN_%s\t%d\t%d\t%d\t%d\t60\tcg:Z:%d=" % (q, q, qs, qs + n, "+-"[k % 2], t, t, ts, ts + n, n, n, n))

    def query(self, name, ranges):
        assert [s for s, _, _ in ranges] == sorted(s for s, _, _ in ranges)
        t0 = self.take("T", 0, 0)
        for i, (seq, kind, L) in enumerate(ranges):
            w = 2 * L + HL + 20
            ts, p = self.take("T", w, 60), self.take(seq, w, 60)
            self.rec(seq, p, "T", ts, w, i)
            other = "A2" if seq == "A1" else "A1"
            for k in range(L):
                q = {"B": "B%d" % ((k + i) % 5), "S": seq, "X": other}[kind]
                qs = self.take(q + "z" if kind != "B" else q, HL)
                self.rec(q, qs, seq, p + 5 + 2 * k, HL, k)
        t1 = self.take("T", 0, 200)
        self.queries[name] = ("T", max(t0 - 10, 0), t1 + 10)

    def text(self):
        for j in range(5):
            self.rec("C", self.take("C", self.next.get("B%d" % j, 1000)), "B%d" % j, 0, self.next.get("B%d" % j, 1000), j)
        for s in ("A1", "A2"):
            n = self.next[s + "z"] - ZONE
            self.rec("C", self.take("C", n), s, ZONE, n, 0)
        names = ["T", "A1", "A2"] + ["B%d" % j for j in range(5)] + ["C"]
        length = {s: max(self.next.get(s, 1000), self.next.get(s + "z", 0)) + 1000 for s in names}
        assert self.next.get("A1", 0) < ZONE and self.next.get("A2", 0) < ZONE
        # (sequence ids go by first appearance and the frontier is sorted by them: four records below every window, where no
        # level looks, name the sequences in the order T < A1 < A2 < B0 .. B4 < C that the shapes are written in)
        body, self.lines = self.lines, []
        for k, (q, t) in enumerate((("T", "A1"), ("A2", "B0"), ("B1", "B2"), ("B3", "B4"))):
            self.rec(q, 0, t, 0, 200, k)
        text = "\n".join(self.lines + body) + "\n"
        for s in names:
            text = text.replace("LEN_%s\t" % s, "%d\t" % length[s])
        return text


def split(n, seqs=("A1", "A2")):
    """n ranges of three B hits each, the first half on A1."""
    return [(seqs[0] if i < (n + 1) // 2 else seqs[1], "B", 3) for i in range(n)]


def cases():
    """name -> ranges; the lists the parametrised tests go through."""
    cs = {}
    # a: N frontier ranges -- the base boundary (63 | 64 | 65) and a third base whose runs the second asks for (129)
    for n in (0, 1, 63, 64, 65, 129):
        cs["a-N%d" % n] = split(n)
    # b: a run of L slots between two short ones -- nothing (the stream skips it), one, the chunk's edges, and 300: five
    # chunks, across the group boundary at 256
    for L in (0, 1, 63, 64, 65, 300):
        cs["b-L%d" % L] = [("A1", "B", 5), ("A1", "B", L), ("A2", "B", 7)]
    # c: the base's total on a chunk edge (64 | 65) and on the group's (255 | 256 | 257 for SEG_U = 4; 511 .. 513 would be
    # SEG_U = 8's), in four runs so that every chunk but the first starts inside a run
    for t in (64, 65, 255, 256, 257, 511, 512, 513):
        cs["c-T%d" % t] = [("A1", "B", t // 4), ("A1", "B", t // 4), ("A2", "B", t // 4), ("A2", "B", t - 3 * (t // 4))]
    # d: a run of hits on the range's own target beside a run of ANOTHER range with hits on that same sequence, in one chunk
    # (10 + 10 + 4 slots): `active` must compare with the lane's own range.  Both ways round: the base's first range is A1's.
    cs["d-self-first"] = [("A1", "S", 10), ("A2", "X", 10), ("A2", "B", 4)]  # A1's own hits: no key; A2's hits on A1: a key
    cs["d-self-last"] = [("A1", "X", 10), ("A1", "B", 4), ("A2", "S", 10)]   # A1's hits on A2: a key; A2's own: none
    return cs


def mixed(rng):
    """300 queries for one batch: every shape above and random ones between them (mostly a few short runs, some empty,
    now and then a long run or many ranges), so that the four waves of a block hold different work."""
    out = dict(cases())
    k = 0
    while len(out) < 300:
        n = int(rng.choice([0, 1, 2, 3, 5, 8, 70], p=[.05, .15, .2, .25, .2, .1, .05]))
        rs = sorted(((str(rng.choice(["A1", "A2"])), str(rng.choice(["B", "B", "B", "S", "X"])),
                      int(rng.choice([0, 1, 2, 9, 30, 64, 100], p=[.1, .15, .2, .3, .15, .05, .05])) if n < 70 else int(rng.integers(0, 4)))
                     for _ in range(n)), key=lambda r: r[0])
        out["g-%03d" % k] = rs
        k += 1
    return out


class World:
    def __init__(self, tmp):
        gen = Gen()
        self.all = mixed(np.random.default_rng(20240607))
        for name, rs in self.all.items():
            gen.query(name, rs)
        path = str(tmp / "seg.paf")
        with open(path, "w") as f:
            f.write(gen.text())
        self.g = impg_amd.GpuImpg.from_paf(path, bidirectional=False)
        self.c = o.OracleIndex(paf_paths=[path], bidirectional=False, preparse=True)
        assert [self.g.seq_name(i) for i in range(self.g.num_seqs())] == [self.c.seq_name(i) for i in range(self.c.num_seqs())]
        assert self.g.seq_id("T") < self.g.seq_id("A1") < self.g.seq_id("A2")
        self.g.set_option("walk_kernel", 0)  # (the batch engine's update is what this file is about)
        self.range = {n: (self.g.seq_id(t), s, e) for n, (t, s, e) in gen.queries.items()}
        self._want = {}

    def want(self, name, depth):
        """The oracle's rows of one query, computed once."""
        if (name, depth) not in self._want:
            t, s, e = self.range[name]
            rows = self.c.query(t, s, e, transitive=True, max_depth=depth)
            self._want[(name, depth)] = (rows, self.c.last_projection_count())
        return self._want[(name, depth)]

    def check(self, names, depths=(2, 3)):
        """query_batch row for row in emission order, query_batch_stats' counts and checksums; returns the stats' counts."""
        ranges = [self.range[n] for n in names]
        counts = {}
        for d in depths:
            p = impg_amd.make_params(transitive=True, max_depth=d)
            res = self.g.query_batch(ranges, p)
            st, cnt, ck = self.g.query_batch_stats(ranges, p)
            proj = 0
            for i, n in enumerate(names):
                rows, pr = self.want(n, d)
                assert res[i].tolist() == rows.tolist(), (n, d)
                assert int(cnt[i]) == len(rows) - 1 and int(ck[i]) == checksum(rows[1:]), (n, d)
                proj += pr
            assert res.projected == proj and int(st.projected) == proj, d
            counts[d] = cnt.tolist()
        return counts

    def assert_shape(self, name):
        """The query reaches the level-2 update as written: N ranges, runs of the lengths given, on the sequences given."""
        shape = self.all[name]
        r = self.range[name]
        cnt = [int(self.g.query_batch_stats([r], impg_amd.make_params(transitive=True, max_depth=d))[1][0]) for d in (1, 2)]
        assert cnt[0] == len(shape), (name, cnt)                       # N: one level-1 hit per range
        assert cnt[1] - cnt[0] == sum(L for _, _, L in shape), (name, cnt)  # the base's (bases') slots
        rows = self.want(name, 2)[0]
        l1 = rows[1:1 + len(shape)]  # (in visit order; the frontier they become is sorted by sequence and start)
        l1 = l1[np.lexsort((np.minimum(l1["q_first"], l1["q_last"]), l1["query_id"]))]
        assert [self.g.seq_name(int(x)) for x in l1["query_id"]] == [s for s, _, _ in shape], name
        l2 = rows[1 + len(shape):]
        for (seq, kind, L), w in zip(shape, l1):  # each run: the level-2 rows whose target interval lies in the range's window
            lo, hi = sorted((int(w["q_first"]), int(w["q_last"])))
            run = l2[(l2["target_id"] == w["query_id"]) & (l2["t_first"] >= lo) & (l2["t_last"] <= hi)]
            assert len(run) == L, (name, seq, kind, L, len(run))
            own = int((run["query_id"] == run["target_id"]).sum())
            assert own == (L if kind == "S" else 0), (name, kind)
            if kind == "X":
                other = self.g.seq_id("A2" if seq == "A1" else "A1")
                assert (run["query_id"] == other).all(), name
        if any(L for _, _, L in shape if L) and any(k != "S" for _, k, L in shape if L):
            assert len(self.want(name, 3)[0]) > len(rows), name  # (the level-2 update's pieces reach level 3's rows)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return World(tmp_path_factory.mktemp("seg_stream"))


def snapshot(g):
    return {k: g.counter(k) for k in SEG_COUNTERS}


@pytest.mark.parametrize("name", list(cases()))
def test_stream_edge(world, name):
    """a - d: one query alone (a grid of one wave), its shape asserted, rows / counts / checksums against the oracle."""
    world.assert_shape(name)
    before = snapshot(world.g)
    world.check([name])
    assert snapshot(world.g) == before, name  # (by segments, a wave per query: no slices, no retry, no library sort)


def test_own_target_runs_carry_no_key(world):
    """d, said outright: the S run adds no piece (its hits lie on the range's own sequence), the X run of the other range
    adds one per hit on that same sequence -- level 3 finds exactly the X pieces in the zone, through C <- A?."""
    for name, x_to in (("d-self-first", "A1"), ("d-self-last", "A2")):  # (x_to: the sequence both runs' hits lie on)
        rows = world.want(name, 3)[0]
        two = len(world.want(name, 2)[0])
        l3 = rows[two:]
        zone = l3[(l3["target_id"] == world.g.seq_id(x_to)) & (l3["t_first"] >= ZONE)]
        assert len(zone) == 10, (name, len(zone))  # the ten X pieces; the ten S hits reached nothing
    world.check(["d-self-first", "d-self-last"])


@pytest.mark.parametrize("parts", [2, 3, 7])
def test_sliced_units(world, parts):
    """e: every shape with its query's ranges cut into `parts` slices, a wave each (more slices than some have ranges)."""
    names = list(cases())
    g = world.g
    before = snapshot(g)
    g.set_option("segment_parts", parts)
    try:
        world.check(names)
    finally:
        g.set_option("segment_parts", 0)
    after = snapshot(g)
    assert after["segment_sliced_levels"] > before["segment_sliced_levels"], (before, after)
    assert after["segment_library_levels"] == before["segment_library_levels"], (before, after)


def test_library_sort_is_a_second_reference(world):
    """f: segment_groups = 0 orders the same hits with the library's radix sort: the same rows, counts and checksums, and
    segment_library_levels rises there and only there."""
    names = list(cases())
    g = world.g
    before = snapshot(g)
    seg = world.check(names)
    mid = snapshot(g)
    assert mid["segment_library_levels"] == before["segment_library_levels"], (before, mid)
    g.set_option("segment_groups", 0)
    try:
        lib = world.check(names)
    finally:
        g.set_option("segment_groups", 1)
    after = snapshot(g)
    assert after["segment_library_levels"] > mid["segment_library_levels"], (mid, after)
    assert seg == lib


def test_mixed_batch(world):
    """g: 300 queries in one batch -- every edge above among random shapes, so a block's four waves differ -- by segments,
    in slices, and by the library sort."""
    names = list(world.all)
    assert len(names) == 300
    g = world.g
    before = snapshot(g)
    ref = world.check(names)
    assert snapshot(g) == before
    g.set_option("segment_parts", 3)
    try:
        assert world.check(names, depths=(3,))[3] == ref[3]
    finally:
        g.set_option("segment_parts", 0)
    g.set_option("segment_groups", 0)
    try:
        st, cnt, ck = g.query_batch_stats([world.range[n] for n in names], impg_amd.make_params(transitive=True, max_depth=3))
    finally:
        g.set_option("segment_groups", 1)
    assert cnt.tolist() == ref[3]
