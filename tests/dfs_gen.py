"""Inputs that put the batch engine's DFS rounds (Engine::run_dfs: the pop chain, the hop, the update, the stack chain) and the
folding of its visited tables (Engine::compact_tables) on their edges, and a sequential model that says what each input reaches.

The fixtures are PAF text only -- never an expected output: that is the oracle's.  Every alignment is one `N=` op (walk_gen's
one-op line), every index is built with bidirectional=False, so `edge(src, ss, dst, ds)` is a one-way step: a query on
src:[ss, ss + n) yields dst:[ds, ds + n).  Sequence ids are given in order of first appearance, a line's query name first; a
fixture that needs an order says so with `id_order`, lines at FAR that no query reaches.
Every fixture's alignments form a graph without cycles (MultiImpg's copies of a step's own interval aside, which its worklist
skips): a walk over it ends whatever a broken fold or merge makes the visited sets forget -- a wrong engine fails, it does not spin.

The model (walk / run) is a plain restatement of query_transitive_dfs (oracle/impg_oracle.cpp impg_dfs) and of MultiImpg's
worklist (multi_transitive: pop at the back for DFS, at the front for BFS) for `=`-only alignments inside their sequences, with
min_distance_between_ranges = 0 and min_transitive_len <= 1: the pieces of a pop are then what its hits' images leave of the
complement of the visited set, whatever the order of the hits.  It returns the rows (a multiset: the order of a pop's hits is the
tree's) and a trace:

  explored        pops that passed the depth test (the reference's frontier lookups)
  dropped         records popped and dropped as too deep
  rounds          explored, plus one if records that are all too deep are left behind the last explored pop: the engine takes
                  every too-deep record off the pop end and explores the first that is not, in one round; a run that is too deep
                  throughout is one round that only drops (whole_run_drops)
  drops_behind    the most records dropped in one round in front of its explored pop
  deep_kept       explored pops that left a too-deep record further down the stack (it must stay: it may yet merge)
  peak            the largest stack after a re-sort and merge (or at the start)
  longest_run     the most records of one sequence in a re-sort, before the merge
  first_deeper / second_deeper / equal_depth
                  touching merges by which of the two records was deeper (the merged record keeps the first one's depth)
  overlaps        merges of records that overlap, `we > rs`, among them contained ones, `we > re`: always 0.  Every record on a
                  stack is a piece cut from the complement of the query's visited set at the time, and the set only grows, so two
                  records of one sequence are disjoint: they can touch, never overlap.  The issue's "record contained in its
                  neighbour" cannot be built from PAF text (the mask lists are the only other input, and a mask yields first
                  pieces that touch); `around` is the nearest thing: an image that contains a waiting record, whose two new
                  pieces merge with it from both sides.
  keys            per explored pop, the sequences that got a visited list (a hit on the popped sequence itself has no key)

and for a batch (every query pops once a round, so a query's k-th explored pop is round k): rounds and levels (the maxima), the
flat stack's size at every round, and the visited tables -- one per round that has a key, folded into one as soon as
`tables + FOLD_SLACK >= MAX_VISITED_TABLES` --: folds, and the most tables one key lay in when a fold came (max_key_tables).
"""
import bisect

from tests.walk_gen import SEQ_LEN, aln

MAX_VISITED_TABLES = 48   # kernels.hpp
FOLD_SLACK = 2            # engine.cpp: `if (tables.size() + 2 >= (size_t)MAX_VISITED_TABLES) compact_tables();`
FAR = 70_000_000
BASE = dict(transitive=True, min_transitive_len=1, min_distance_between_ranges=0)


def D(depth, **kw):
    return dict(BASE, dfs=True, max_depth=depth, **kw)


def B(depth, **kw):
    return dict(BASE, dfs=False, max_depth=depth, **kw)


def edge(src, ss, dst, ds, n=100, strand="+"):
    return aln(dst, ds, src, ss, n, strand)


def id_order(names):
    """lines that do nothing but name the sequences in this order"""
    return [aln(names[i], FAR, names[i + 1] if i + 1 < len(names) else names[0], FAR) for i in range(0, len(names), 2)]


# ---- the model --------------------------------------------------------------------------------------------------------------
class Index:
    def __init__(self, texts):
        self.names, self.ids, self.files = [], {}, []
        for text in texts:
            by_target = {}
            for line in text.splitlines():
                f = line.split("\t")
                qs, qe, ts, te = int(f[2]), int(f[3]), int(f[7]), int(f[8])
                assert f[12] == "cg:Z:%d=" % (qe - qs) and qe - qs == te - ts and 0 <= qs < qe <= SEQ_LEN and 0 <= ts < te <= SEQ_LEN, line
                q, t = self._id(f[0]), self._id(f[5])
                by_target.setdefault(t, []).append((q, qs, qe, f[4], ts, te))
            self.files.append(by_target)

    def _id(self, name):
        if name not in self.ids:
            self.ids[name] = len(self.names)
            self.names.append(name)
        return self.ids[name]

    def hits(self, t, s, e):
        """the rows of one lookup, file by file: (query_id, q_first, q_last, target_id, t_first, t_last)"""
        out = []
        for by_target in self.files:
            for q, qs, qe, strand, ts, te in by_target.get(t, ()):
                a, b = max(s, ts), min(e, te)
                if a < b:
                    out.append((q, qs + (a - ts), qs + (b - ts), t, a, b) if strand == "+" else (q, qe - (a - ts), qe - (b - ts), t, a, b))
        return out


def insert(ranges, a, b):
    """SortedRanges::insert with min_distance 0, inside the sequence: what [a, b) adds to the list, ascending; the list takes it"""
    start, end = (a, b) if a <= b else (b, a)
    out, cur = [], start
    i = bisect.bisect_left(ranges, (start, -1))
    if i > 0 and ranges[i - 1][1] > start:
        i -= 1
    while i < len(ranges) and cur < end:
        rs, re = ranges[i]
        if rs > end:
            break
        if cur < rs:
            out.append((cur, rs))
        cur = max(cur, re)
        i += 1
    if cur < end:
        out.append((cur, end))
    merged = []
    for rs, re in sorted(ranges + [(start, end)]):
        if merged and merged[-1][1] >= rs:
            merged[-1] = (merged[-1][0], max(merged[-1][1], re))
        else:
            merged.append((rs, re))
    ranges[:] = merged
    return out


class Trace:
    def __init__(self):
        self.explored = self.dropped = self.rounds = self.drops_behind = self.deep_kept = self.whole_run_drops = 0
        self.peak = self.longest_run = self.first_deeper = self.second_deeper = self.equal_depth = self.overlaps = 0
        self.keys, self.sizes = [], []


def walk(ix, target, s, e, max_depth, dfs=True, multi_impg=False, min_transitive_len=1, **unused):
    """one query: (rows, Trace)"""
    assert dfs or multi_impg, "a plain BFS is a level at a time: Engine::run, not run_dfs"
    tr, visited = Trace(), {}
    first = insert(visited.setdefault(target, []), s, e)
    rows = [(target, a, b, target, a, b) for a, b in first]
    stack = [[target, a, b, 0] for a, b in first if b - a >= min_transitive_len]
    tr.peak, pending = len(stack), 0

    def deep(r):
        return max_depth > 0 and r[3] >= max_depth

    while stack:
        if not pending:
            tr.sizes.append(len(stack))  # a round begins
        cur = stack.pop() if dfs else stack.pop(0)
        if deep(cur):
            tr.dropped += 1
            pending += 1
            continue
        tr.explored += 1
        tr.drops_behind, pending = max(tr.drops_behind, pending), 0
        tr.deep_kept += any(deep(r) for r in stack)
        keyed = set()
        for row in ix.hits(cur[0], cur[1], cur[2]):
            if row[0] == cur[0]:
                if multi_impg:
                    continue  # MultiImpg skips a hit on the popped sequence; Impg prints it and keeps no list for it
                rows.append(row)
                continue
            rows.append(row)
            keyed.add(row[0])
            for a, b in insert(visited.setdefault(row[0], []), row[1], row[2]):
                if b - a >= min_transitive_len:
                    stack.append([row[0], a, b, cur[3] + 1])
        tr.keys.append(keyed)
        stack.sort(key=lambda r: (r[0], r[1]))  # stable
        run = 0
        for i, r in enumerate(stack):
            run = run + 1 if i and stack[i - 1][0] == r[0] else 1
            tr.longest_run = max(tr.longest_run, run)
        out = []
        for r in stack:
            if out and out[-1][0] == r[0] and out[-1][2] >= r[1]:
                w = out[-1]
                tr.overlaps += w[2] > r[1]
                if w[3] > r[3]:
                    tr.first_deeper += 1
                elif w[3] < r[3]:
                    tr.second_deeper += 1
                else:
                    tr.equal_depth += 1
                w[2] = max(w[2], r[2])
            else:
                out.append(r)
        stack = out
        tr.peak = max(tr.peak, len(stack))
    tr.whole_run_drops = 1 if pending else 0
    tr.rounds = tr.explored + tr.whole_run_drops
    return rows, tr


class BatchTrace:
    pass


def run(ix, queries, kw):
    """a batch: ([rows per query], BatchTrace); queries are (name, start, end)"""
    rows, traces = [], []
    for name, s, e in queries:
        r, t = walk(ix, ix.ids[name], s, e, **{k: v for k, v in kw.items() if k != "transitive" and k != "min_distance_between_ranges"})
        rows.append(r)
        traces.append(t)
    bt = BatchTrace()
    bt.queries = traces
    bt.rounds = max(t.rounds for t in traces)
    bt.levels = max(t.explored for t in traces)
    bt.flat = [sum(t.sizes[k] for t in traces if k < len(t.sizes)) for k in range(bt.rounds)]
    tables = [{(q, ix.ids[name]) for q, (name, _, _) in enumerate(queries)}]
    bt.folds = bt.max_key_tables = bt.first_fold_key_tables = 0
    for k in range(bt.levels):
        keys = {(q, sid) for q, t in enumerate(traces) if k < len(t.keys) for sid in t.keys[k]}
        if not keys:
            continue
        tables.append(keys)
        if len(tables) + FOLD_SLACK >= MAX_VISITED_TABLES:
            count = {}
            for tab in tables:
                for key in tab:
                    count[key] = count.get(key, 0) + 1
            if not bt.folds:
                bt.first_fold_key_tables = max(count.values())
            bt.max_key_tables = max(bt.max_key_tables, max(count.values()))
            bt.folds += 1
            tables = [set().union(*tables)]
    return rows, bt


# ---- the fixtures -------------------------------------------------------------------------------------------------------------
class Case:
    """texts: one PAF text per alignment file (more than one: MultiImpg only).  queries: (name, start, end).  kws: the parameter
    sets the case is meant for, each run as it stands (multi_impg among them where the case is MultiImpg's).  mask: name -> list
    of ranges (the model does not cover masks: oracle only)."""

    def __init__(self, name, texts, queries, kws, mask=None, note=""):
        self.name, self.texts, self.queries, self.kws, self.mask, self.note = name, texts, queries, kws, mask, note
        self.multi = any(kw.get("multi_impg") for kw in kws)
        assert len(texts) == 1 or all(kw.get("multi_impg") for kw in kws), name
        self.modelled = mask is None


def multi(kws):
    return [dict(kw, multi_impg=True) for kw in kws]


def split(lines, n_files, head=0):
    """lines dealt out over n_files texts; the first `head` lines (the id order) stay in the first file"""
    files = [list(lines[:head])] + [[] for _ in range(n_files - 1)]
    for i, line in enumerate(lines[head:]):
        files[i % n_files].append(line)
    return ["".join(f) for f in files]


def depth_merge():
    """The issue's fixture: X:[100, 200) waits at depth 1, the piece X:[0, 100) of depth 3 sorts first and touches it."""
    return [edge("T", 0, "X", 100), edge("T", 0, "Y", 0), edge("Y", 0, "Z", 0), edge("Z", 0, "X", 0), edge("X", 0, "W", 0, 200)]


def depth_merge_mirror():
    """The shallow record sorts first: X:[0, 100) waits at depth 1, X:[100, 200) comes at depth 3; the merged record stays explorable."""
    return [edge("T", 0, "X", 0), edge("T", 0, "Y", 0), edge("Y", 0, "Z", 0), edge("Z", 0, "X", 100), edge("X", 0, "W", 0, 200)]


def merge_three():
    """deep - shallow - deep: X:[100, 200) waits at depth 1, one pop at depth 2 brings X:[0, 100) and X:[200, 300)"""
    return [edge("T", 0, "X", 100), edge("T", 0, "Y", 0), edge("Y", 0, "Z", 0), edge("Z", 0, "X", 0), edge("Z", 0, "X", 200),
            edge("X", 0, "W", 0, 300)]


def around():
    """X:[40, 60) waits at depth 1; an image X:[0, 100) of depth 3 contains it: its pieces [0, 40) and [60, 100) merge with it from both sides"""
    return [edge("T", 40, "X", 40, 20), edge("T", 0, "Y", 0), edge("Y", 0, "Z", 0), edge("Z", 0, "X", 0), edge("X", 0, "W", 0, 100)]


MERGE_ORDER = ["X", "T", "Y", "Z", "W"]


def too_deep_ends(reverse=False):
    """max_depth 2, three queries.  Ids ascend as listed (reverse: descend -- the same stacks seen from the front, for pop_front).
      P   pops P, then M (the far end): its images U1, U2 of depth 2 lie beyond L (depth 1).  Round 3 drops both and explores L,
          whose image R of depth 2 is all that is left: round 4 drops the run, the query dies.
      C   a comb of 6 teeth: every round but the first drops the last tooth's image and explores the next tooth: it lives on.
      S   its only hit is shorter than the others', nothing special: ends in round 2 with an empty stack."""
    order = ["L", "P", "M", "U1", "U2", "R", "C"] + ["c%d" % i for i in range(6)] + ["d%d" % i for i in range(6)] + ["S", "s"]
    lines = id_order(order[::-1] if reverse else order)
    lines += [edge("P", 0, "L", 0), edge("P", 0, "M", 0), edge("M", 0, "U1", 0), edge("M", 0, "U2", 0), edge("L", 0, "R", 0)]
    for i in range(6):
        lines += [edge("C", 0, "c%d" % i, 0), edge("c%d" % i, 0, "d%d" % i, 0)]
    lines += [edge("S", 0, "s", 0, 50)]
    return lines, len(id_order(order))


TOO_DEEP_QUERIES = [("P", 0, 100), ("C", 0, 100), ("S", 0, 100)]


def deep_between(reverse=False):
    """max_depth 3.  Pops: T; F -> G (depth 2); G -> X:[100, 200) (depth 3, too deep).  The stack is then E1, X, E2 by id: the pop
    of E2 must leave X where it is, for E2's image X:[0, 100) of depth 2 merges with it into X:[0, 200) of depth 2, which is
    explored: W:0-200.  Had X been dropped with the too-deep records of some round, the row would be W:0-100."""
    order = ["E1", "T", "X", "E2", "F", "G", "W", "V"]
    lines = id_order(order[::-1] if reverse else order)
    lines += [edge("T", 0, "E1", 0), edge("E2", 0, "X", 0), edge("T", 0, "E2", 0), edge("T", 0, "F", 0), edge("F", 0, "G", 0),
              edge("G", 0, "X", 100), edge("X", 0, "W", 0, 200), edge("E1", 0, "V", 0)]
    return lines, len(id_order(order))


COMB_N = [63, 64, 65, 255, 256, 257]


def comb(n):
    """T:[0, 100) hits n sequences once each, each leads one step on: one pop pushes n records in n groups.  The second steps have
    the higher ids: under max_depth 2 every later round drops one of them and explores the next tooth (n more rounds, a table
    each); under max_depth 0 they are explored too (2 n more rounds)."""
    order = ["T"] + ["c%d" % i for i in range(n)] + ["d%d" % i for i in range(n)]
    lines = id_order(order)
    for i in range(n):
        lines += [edge("T", 0, "c%d" % i, 0), edge("c%d" % i, 0, "d%d" % i, 0)]
    return lines


LONG_RUN = 300


def long_run_places():
    at, out = 0, []
    for i in range(LONG_RUN):
        out.append(at)
        at += 100 if i % 5 == 2 else 300  # every fifth neighbour touches
    return out


def long_run():
    """T:[0, 100) has 300 images on X, disjoint, every fifth touching its neighbour: one merge lane sweeps a run of 300 with merges
    inside it.  X maps on to W in one piece, so every explored record of X shows its extent in a row of W (W has the higher id:
    its records, depth 2, are dropped behind each pop).  The second query's run is a single record."""
    places = long_run_places()
    lines = id_order(["T", "X", "U", "V", "W"])
    lines += [edge("T", 0, "X", at) for at in places]
    lines += [edge("X", 0, "W", 0, places[-1] + 100), edge("U", 0, "V", 0)]
    return lines


RUNGS = 60


def ladder():
    """A:[1000 k, +100) -> B:[1000 k, +100) and B:[1000 k, +100) -> A:[1000 (k + 1), +100) for k < 60: from A:0-100 a DFS with no
    depth limit pops 121 records, the last of which (A:[60000, +100)) finds nothing: 120 projections, 121 rows, 120 tables -- the
    keys (q, A) and (q, B) lie in every other one."""
    lines = []
    for k in range(RUNGS):
        lines += [edge("A", 1000 * k, "B", 1000 * k), edge("B", 1000 * k, "A", 1000 * (k + 1))]
    return lines


def ladder_back():
    """The ladder with a side branch that is met again after a fold.  A's rungs 1 and 3 also map to S:[0, 100) and S:[200, 300), so
    the key (q, S) lies in two tables, and only the newer list knows S:[200, 300); S:[200, 300) leads to Z:[0, 100); S and Z lead
    nowhere else.  The single query folds after its 45th and 90th table.  After the folds B's rung 50 maps to S:[200, 300)
    again: a row and no piece.  A fold that kept the key's oldest list would hand S:[200, 300) out as a new piece: one more pop
    and a second row Z:0-100.  The same with a range first visited between the folds and met again after the second: A's rung 30
    -> S:[400, 500) -> Z:[200, 300), B's rung 58 -> S:[400, 500).  (Ways back into the ladder itself would show the same, but a fold that forgets makes such a walk
    endless: it climbs, folds, forgets the climb and is sent back.  The side branch ends under any fold.  The plain ladder
    cannot tell the two folds apart at all: none of its hits lands on a range visited before.)"""
    return ladder() + [edge("A", 1000, "S", 0), edge("A", 3000, "S", 200), edge("S", 200, "Z", 0), edge("B", 50000, "S", 200),
                       edge("A", 30000, "S", 400), edge("S", 400, "Z", 200), edge("B", 58000, "S", 400)]


def ladder_queries(n=300):
    """n queries that start on different rungs and sides, on sub-ranges of different widths: they end in different rounds"""
    return [("AB"[(i // RUNGS) & 1], 1000 * ((7 * i) % RUNGS) + i % 10, 1000 * ((7 * i) % RUNGS) + 50 + i % 41) for i in range(n)]


STEP_HITS = [63, 64, 65, 128, 129]


def multi_step(h):
    """One step of exactly h hits (slots) on T:[1000, 1500), over three files: distinct images on Q0 .. Q6 on both strands, every
    ninth line a copy of the line before it in the next file (a full five-key tie across files), and two copies of the step's
    own interval (T onto itself, files 0 and 2).  Q1 leads on to R."""
    files = [id_order(["T", "Q0", "Q1", "Q2", "Q3", "Q4", "Q5", "Q6", "R"]), [], []]
    made = 0
    for f in (0, 2):
        files[f].append(edge("T", 1000, "T", 1000, 500))
        made += 1
    i = 0
    while made < h:
        line = edge("T", 1000 + i % 3, "Q%d" % (i % 7), 100 + 11 * (i % 5) + 600 * (i // 35), 500 - i % 3, "+-"[i & 1])
        files[i % 3].append(line)
        made += 1
        if i % 9 == 8 and made < h:
            files[(i + 1) % 3].append(line)
            made += 1
        i += 1
    files[1].append(edge("Q1", 0, "R", 0, 5000))
    return ["".join(f) for f in files]


MULTI_KWS = multi([D(2), B(2), D(0), B(0)])
_cases = [
    Case("depth-merge", ["".join(depth_merge())], [("T", 0, 100)], [D(3), D(4), D(0)]),
    Case("depth-merge-mirror", ["".join(depth_merge_mirror())], [("T", 0, 100)], [D(3), D(4)]),
    Case("merge-three", ["".join(merge_three())], [("T", 0, 100)], [D(3), D(4)]),
    Case("around", ["".join(around())], [("T", 0, 100)], [D(3), D(4)]),
    Case("too-deep-back", ["".join(too_deep_ends()[0])], TOO_DEEP_QUERIES, [D(2)]),
    Case("too-deep-back-multi", split(too_deep_ends()[0], 2, too_deep_ends()[1]), TOO_DEEP_QUERIES, multi([D(2)])),
    Case("too-deep-front-multi", split(too_deep_ends(True)[0], 2, too_deep_ends(True)[1]), TOO_DEEP_QUERIES, multi([B(2)])),
    Case("deep-between-back", ["".join(deep_between()[0])], [("T", 0, 100)], [D(3)]),
    Case("deep-between-back-multi", split(deep_between()[0], 2, deep_between()[1]), [("T", 0, 100)], multi([D(3)])),
    Case("deep-between-front-multi", split(deep_between(True)[0], 2, deep_between(True)[1]), [("T", 0, 100)], multi([B(3)])),
] + [Case("comb-%d" % n, ["".join(comb(n))], [("T", 0, 100)], [D(2), D(0)]) for n in COMB_N] + [
    Case("long-run", ["".join(long_run())], [("T", 0, 100), ("U", 0, 100)], [D(2)]),
    Case("ladder-1", ["".join(ladder())], [("A", 0, 100)], [D(0), D(7)]),
    Case("ladder-300", ["".join(ladder())], ladder_queries(), [D(0), D(7)]),
    Case("ladder-back-1", ["".join(ladder_back())], [("A", 0, 100)], [D(0)]),
    Case("ladder-back-300", ["".join(ladder_back())], ladder_queries(), [D(0)]),
] + [Case("multi-step-%d" % h, multi_step(h), [("T", 1000, 1500), ("T", 1100, 1300)], MULTI_KWS) for h in STEP_HITS] + [
    # the first pieces [0, 30), [30, 60), [60, 100) touch; the first pop, [60, 100), finds nothing (the alignment ends at 60), so the
    # round pushes nothing -- and must merge all the same: the next pop is T:[0, 60), one row Y:0-60
    Case("masked-start", [edge("T", 0, "Y", 0, 60) + edge("Y", 0, "Z", 0, 60)], [("T", 0, 100)], [D(0), D(2)],
         mask={"T": [(30, 30), (60, 60)]}),
]
CASES = {c.name: c for c in _cases}
