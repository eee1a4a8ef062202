"""Fixtures of the resolve pass's tests (tests/eqx_ref.py is the model): PAF texts without '=' / 'X' detail and the sequences
they align, built so that where the bases differ is known by construction.  A record's query bases are derived from its
target stretch op by op and written into a stretch of the query sequence that belongs to it alone.  Sequences have at most
60 000 bases, a fixture at most 600 records."""
import numpy as np

from tests import eqx_ref as ref

VECTORS = [  # target, query, strand, in, out (checked by hand and with the model)
    ("ACGTACGTAC", "ACGAACGTTC", "+", "10M", "3=1X4=1X1="),
    ("ACGTACGTAC", "GTACGTTCGT", "-", "10M", "3=1X6="),
    ("ACGTACGT", "ACGACGT", "+", "3M1D4M", "3=1D4="),
    ("ACGTACGT", "ACGTACGT", "+", "2=3M0M3M", "2=3=0=3="),
    ("NNRA", "NNRT", "+", "4M", "3=1X"),
    ("ANRY", "YRNT", "-", "4M", "4="),
]
def differ_from(b):
    """a base unlike b, whatever b's case: the next of A, C, G, T; an A for every other byte"""
    u = bytes([b]).upper()
    return b"CGTA"[b"ACGT".index(u)] if u in b"ACGT" else b"A"[0]


class Fixture:
    def __init__(self, seed, alphabet=b"ACGT"):
        self.rng = np.random.default_rng(seed)
        self.alphabet = np.frombuffer(alphabet, dtype=np.uint8)
        self.seqs = {}     # name -> bytearray
        self.rows = []     # (qname, qs, qe, strand, tname, ts, te, cigar text or None)
        self.planted = dict(m_x=0, m_eq=0, bad_eq=0, bad_x=0)
        self.drop, self.store_override, self.len_override = set(), {}, {}

    def random(self, n):
        return bytes(self.alphabet[self.rng.integers(0, len(self.alphabet), size=n)])

    def sequence(self, name, n):
        self.seqs[name] = bytearray(self.random(n))

    def record(self, qname, tname, ts, ops, strand="+", gap=0, cigar=True, claim=None):
        """ops: [(code letter, length, differ)]: differ = None (M, =: equal bases; X: unlike ones) or a bool array of the
        positions whose bases differ.  The query bases go behind qname's last record, `gap` random bases apart.
        claim: (dt, dq) added to the ends the line states (a record whose ops do not add up)."""
        T = self.seqs[tname]
        seg = bytearray()
        t = ts
        for code, n, differ in ops:
            if code in "=XM":
                d = np.zeros(n, dtype=bool) if differ is None else np.asarray(differ, dtype=bool)
                if differ is None and code == "X":
                    d[:] = True
                assert len(d) == n and t + n <= len(T)
                seg += bytes(differ_from(T[t + i]) if d[i] else T[t + i] for i in range(n))
                nd = int(d.sum()) if cigar else 0
                n_counted = n if cigar else 0
                if code == "M":
                    self.planted["m_x"] += nd
                    self.planted["m_eq"] += n_counted - nd
                elif code == "=":
                    self.planted["bad_eq"] += nd
                else:
                    self.planted["bad_x"] += n_counted - nd
                t += n
            elif code == "I":
                seg += self.random(n)
            else:
                t += n
        Q = self.seqs.setdefault(qname, bytearray())
        Q += self.random(gap)
        qs = len(Q)
        Q += ref.comp(bytes(seg).upper())[::-1] if strand == "-" else seg
        dt, dq = claim or (0, 0)
        self.rows.append((qname, qs, len(Q) + dq, strand, tname, ts, t + dt, "".join("%d%s" % (n, c) for c, n, _ in ops) if cigar else None))

    # ---- what the tests read ----
    def paf(self):
        lines = []
        for qname, qs, qe, strand, tname, ts, te, cg in self.rows:
            ql = self.len_override.get(qname, len(self.seqs[qname]))
            tl = self.len_override.get(tname, len(self.seqs[tname]))
            f = [qname, ql, qs, qe, strand, tname, tl, ts, te, max(te - ts, 0), max(te - ts, 1), 60]
            lines.append("\t".join(str(x) for x in f) + ("\tcg:Z:" + cg if cg is not None else ""))
        return "".join(ln + "\n" for ln in lines)

    def store(self):
        """{name: bytes} as the FASTA holds them: without the dropped names, with the overridden ones"""
        s = {k: bytes(v) for k, v in self.seqs.items() if k not in self.drop}
        s.update(self.store_override)
        return s

    def fasta(self):
        return "".join(">%s\n%s\n" % (k, "\n".join(v[i:i + 70].decode() for i in range(0, len(v), 70))) for k, v in self.store().items())


def at(n, *positions):
    d = np.zeros(n, dtype=bool)
    for p in positions:
        if 0 <= p < n:
            d[p] = True
    return d


def vectors():
    """the hand-worked table as one fixture's worth of arrays: -> (paf text, store)"""
    lines, store = [], {}
    for k, (t, q, strand, cg, _) in enumerate(VECTORS):
        store["t%d" % k], store["q%d" % k] = t.encode(), q.encode()
        lines.append("q%d\t%d\t0\t%d\t%s\tt%d\t%d\t0\t%d\t1\t1\t60\tcg:Z:%s" % (k, len(q), len(q), strand, k, len(t), len(t), cg))
    return "".join(ln + "\n" for ln in lines), store


BORDER_TILES = (64, 256)
BORDER_STARTS = (0, 1, 15, 16, 17)


def borders():
    """single-M records whose runs begin and end on, before and behind the borders of 64- and 256-base tiles"""
    fx = Fixture(101)
    fx.sequence("T", 1000)
    i = 0
    for tile in BORDER_TILES:
        for L in (1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1, 3 * tile + 7):
            pats = [at(L), np.ones(L, dtype=bool), at(L, 0), at(L, L - 1), at(L, tile - 1), at(L, tile), at(L, tile - 1, tile),
                    np.arange(L) % 2 == 0]
            for d in pats:
                for strand in "+-":
                    fx.record("Q%d" % tile, "T", BORDER_STARTS[i % 5], [("M", L, d)], strand)  # (no gap: Q's first record starts at base 0, its last ends at the last base)
                    i += 1
    return fx


def mixed():
    """aM bI cM dD eM around true '=' / 'X' ops, some '=' / 'X' ops that lie, a 0M and a record without cg:Z"""
    fx = Fixture(102)
    fx.sequence("T", 30000)
    fx.sequence("U", 8000)
    rng = fx.rng
    ts = 100
    for k in range(36):
        a, b, c, d, e = (int(x) for x in rng.integers(1, 400, size=5))
        mm = lambda n, p: rng.random(n) < p
        ops = [("=", 7, None), ("M", a, mm(a, 0.1)), ("I", b % 9 + 1, None), ("M", c, mm(c, 0.02)), ("X", 2, None), ("D", d % 7 + 1, None),
               ("M", e, mm(e, 0.5)), ("=", 5, None)]
        if k % 6 == 1:
            ops[0] = ("=", 7, at(7, 2, 3))      # an '=' over two differing bases
        if k % 6 == 2:
            ops[4] = ("X", 2, at(2, 0))         # an 'X' whose second base is equal
        if k % 6 == 3:
            ops.insert(3, ("M", 0, None))
        fx.record("Q%d" % (k % 3), "T" if k % 4 else "U", ts % 5000, ops, "+-"[k % 2], gap=int(rng.integers(0, 30)), cigar=k != 17)
        ts += 613
    return fx


def flags():
    """four records that cannot be resolved, each between neighbours that can"""
    fx = Fixture(103)
    fx.sequence("T", 5000)
    fx.sequence("SHORT", 900)
    fx.sequence("GONE", 700)
    good = lambda k: fx.record("Q", "T", 50 * k, [("M", 300, fx.rng.random(300) < 0.05), ("D", 2, None), ("M", 40, None)], "+-"[k % 2], gap=3)
    good(0)
    fx.record("Q", "GONE", 10, [("M", 200, None)])                      # the store lacks GONE
    good(1)
    fx.record("Q", "T", 4900, [("M", 100, None)], claim=(0, 0))         # ... and then claim an interval past T's end:
    q, qs, qe, s, t, ts, te, cg = fx.rows[-1]
    fx.rows[-1] = (q, qs, qe, s, t, ts + 50, te + 50, cg)
    good(2)
    fx.record("Q", "T", 1000, [("M", 120, None), ("I", 3, None), ("M", 10, None)], "-", claim=(1, 0))  # ops that do not add up
    good(3)
    fx.record("Q", "SHORT", 100, [("M", 150, None)])                    # the store's SHORT is ten bases shorter than the PAF says
    good(4)
    fx.drop.add("GONE")
    fx.len_override["SHORT"] = 900
    fx.store_override["SHORT"] = bytes(fx.seqs["SHORT"][:890])
    return fx


def bytes_():
    """N, IUPAC codes and lower case in the FASTA, on both strands"""
    fx = Fixture(104, alphabet=b"ACGTNacgtnRYKM")
    fx.sequence("T", 6000)
    for k in range(24):
        n = 150 + 7 * k
        fx.record("Q%d" % (k % 2), "T", 200 * k, [("M", n, fx.rng.random(n) < 0.15), ("I", 2, None), ("M", 33, None), ("D", 1, None), ("M", 64, None)],
                  "+-"[k % 2], gap=k % 5)
    return fx


def random():
    """200 records: divergence planted at 1 % (Q1_*) and at 30 % (Q30_*), with indels, on both strands"""
    fx = Fixture(105)
    rng = fx.rng
    for t in range(3):
        fx.sequence("T%d" % t, 40000)
    for k in range(200):
        p = 0.01 if k % 2 == 0 else 0.30
        ops = []
        for j in range(int(rng.integers(1, 6))):
            n = int(rng.integers(40, 260))
            if j:
                ops.append(("ID"[int(rng.integers(0, 2))], int(rng.integers(1, 6)), None))
            ops.append(("M", n, rng.random(n) < p))
        span = sum(n for c, n, _ in ops if c != "I")
        fx.record("Q%d_%d" % (1 if k % 2 == 0 else 30, k % 2 + (k // 2) % 2 * 2), "T%d" % (k % 3), int(rng.integers(0, 40000 - span)), ops, "+-"[(k // 2) % 2],
                  gap=int(rng.integers(0, 20)))
    return fx


def skew():
    """one record with a single M of 50 000 bases beside 500 records of 1-3 bases"""
    fx = Fixture(106)
    fx.sequence("T", 52000)
    rng = fx.rng
    for k in range(250):
        n = 1 + k % 3
        fx.record("Qs", "T", int(rng.integers(0, 51000)), [("M", n, rng.random(n) < 0.3)], "+-"[k % 2], gap=1)
    fx.record("Qlong", "T", 777, [("M", 50000, rng.random(50000) < 0.01)], "-")
    for k in range(250):
        n = 1 + k % 3
        fx.record("Qs", "T", int(rng.integers(0, 51000)), [("M", n, rng.random(n) < 0.3)], "+-"[k % 2], gap=1)
    return fx


FIXTURES = dict(borders=borders, mixed=mixed, flags=flags, bytes=bytes_, random=random, skew=skew)
_CACHE = {}


def fixture(name):
    """-> dict(fx, paf, store, records, ops, names, seq_len, model=(records, ops, flags, report)); built once a process"""
    if name not in _CACHE:
        if name == "vectors":
            fx, (paf, store) = None, vectors()
        else:
            fx = FIXTURES[name]()
            paf, store = fx.paf(), fx.store()
        recs, ops, names, lens = ref.parse_paf(paf)
        assert len(recs) <= 600 and all(len(v) <= 60000 for v in store.values())
        _CACHE[name] = dict(fx=fx, paf=paf, store=store, records=recs, ops=ops, names=names, seq_len=lens, model=ref.resolve(recs, ops, names, lens, store))
    return _CACHE[name]


ALL = ("vectors",) + tuple(FIXTURES)
