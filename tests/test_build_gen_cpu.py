"""No GPU: the index-build fixtures (tests/build_gen.py) reach the edges they claim, judged on the model's output
(tests/index_ref.py); the pure-Python tokenizer, the oracle and the library's host tokenizer agree on every text; and
read_index parses a file written by a small pure-Python writer of the same format."""
import struct

import numpy as np
import pytest

from impg_amd import index as gi
from oracle import oracle as o
from tests import build_gen as bg
from tests import index_ref as ir


def model(name, prefix_lines=True, identity_lines=True):
    f = bg.fixture(name)
    return f, ir.expected_index(f.records, f.ops, f.seq_len, f.bidirectional, prefix_lines, identity_lines)


# ---- tokenizer ---------------------------------------------------------------------------------------------------------
ALL_TEXTS = dict(bg.TOKEN_TEXTS, code5=bg.CODE5_TEXT)


@pytest.mark.parametrize("name", sorted(ALL_TEXTS))
def test_tokenizers_agree(name):
    text = ALL_TEXTS[name]
    want = o.parse_cigar(text).tolist()
    assert bg.tokenize(text) == want
    assert gi.parse_cigar(text).tolist() == want


def test_lengths_from_2_pow_29_change_the_code():
    got = [bg.tokenize(bg.TOKEN_TEXTS["len_%d" % v])[1] for v in bg.LENGTHS]
    assert got == [0x1FFFFFFF, 0x20000000, 0x20000001, 0x60000001, 0x80000000, 0xFFFFFFFF, 0x0, 0x20000005, 0x4876E7FF]
    assert bg.tokenize(bg.CODE5_TEXT) == [0xA0000000]
    assert o.parse_cigar("536870912=").tolist() == [0x20000000]  # an 'X' of length 0
    assert [t for t in ALL_TEXTS.values() if any(v >> 29 > 4 for v in bg.tokenize(t))] == [bg.TOKEN_TEXTS["len_4294967295"], bg.CODE5_TEXT]


@pytest.mark.parametrize("name,text", bg.bad_texts())
def test_bad_bytes_are_refused_by_all(name, text):
    with pytest.raises(ValueError):
        bg.tokenize(text)
    with pytest.raises(ValueError):
        o.parse_cigar(text)
    with pytest.raises(ValueError):
        gi.parse_cigar(text)


def test_token_texts_sit_on_their_bytes():
    T = bg.TOKEN_TEXTS
    assert T["letter_at_63"][63] == "X" and T["letter_at_63"][60:63].isdigit()
    assert T["letter_at_64"][64] == "X" and T["letter_at_64"][60:64].isdigit()
    assert T["digits_60_66"][60:67] == "1234567" and T["digits_60_66"][59] == "=" and T["digits_60_66"][67] == "="
    assert len(T["letters_64"]) == 64 and len(T["letters_65"]) == 65
    assert T["zeros_70"][:70] == "0" * 70 and bg.tokenize(T["zeros_70"]) == [(2 << 29) | 9]
    assert len(T["mixed_69"]) == 69 and bg.tokenize(T["mixed_69"])[-1] == 123456
    assert bg.tokenize(T["trailing_digits"]) == [5, (1 << 29) | 3]
    assert len(T["trailing_digits_across"]) == 67 and len(bg.tokenize(T["trailing_digits_across"])) == 31
    assert [bg.tokenize(T[k]) for k in ("empty", "digits_only", "letter_only", "zero_len")] == [[], [], [4 << 29], [0]]
    for name, text in bg.bad_texts():
        pos = int(name.rsplit("_", 1)[1])
        assert text[pos] in bg.BAD_BYTES and len(text) == 80 and pos in (0, 63, 64, 79)


def test_token_paf_reads_as_claimed():
    f = bg.fixture("token_paf")
    assert len(f.paf) == 2 and f.file_first.tolist()[0] == 0 and 0 < f.file_first[1] < len(f.records)
    cig = lambda i: f.ops[int(f.records[i]["cigar_off"]):][:int(f.records[i]["cigar_len"])].tolist()  # noqa: E731
    n = len(f.records)
    assert cig(n - 3) == bg.tokenize("4=2I")  # two tags: the first wins
    assert cig(n - 2) == bg.tokenize("6D1=")  # the tag in the tenth field
    assert cig(n - 1) == bg.tokenize("8=1X8=")  # "\r\n"
    assert f.paf[1].endswith("\r\n")
    no_tag = [i for i in range(n) if f.records[i]["cigar_len"] == 0]
    assert len(no_tag) >= 3 and all(0 < i < n - 1 for i in no_tag)
    c = o.OracleIndex(paf_text="".join(f.paf), preparse=True)  # the oracle reads the same sequences and records
    assert c.num_records() == n and [c.seq_name(i) for i in range(c.num_seqs())] == f.names


# ---- the fixtures reach their edges ------------------------------------------------------------------------------------
def test_tile_fill_reaches_its_edges():
    f, w = model("tile_fill")
    E = w["entries"]
    nops = E["nops_flags"] & ir.OP_LEN_MASK
    assert sorted(set(nops.tolist())) == sorted(bg.TILE_FILL_COUNTS)
    tiles = (nops + 25) // 26
    forms = set()
    for e, m in zip(E, tiles.tolist()):
        fl = int(e["nops_flags"])
        forms.add((bool(fl & ir.EF_REVERSED), bool(fl & ir.EF_STRAND), m > 8))
        if m == 0:
            assert e["tcp"].tolist() == [0x7FFFFFFF] * 7
        elif m <= 7:
            assert e["tcp"][m - 1] == e["totT"] and (e["tcp"][m:] == 0x7FFFFFFF).all()
        elif m == 8:  # seven real prefixes; the eighth is the entry's totT field
            assert (np.diff(e["tcp"].astype(np.int64)) >= 0).all() and e["tcp"][6] <= e["totT"] < 0x7FFFFFFF
        else:
            assert w["ext_cp"][int(e["tcp"][0]) + m] == e["totT"] and w["ext_cp"][int(e["tcp"][0])] == 0
    assert forms == {(r, s, x) for r in (False, True) for s in (False, True) for x in (False, True)}
    assert {int(t) for t in tiles} >= {0, 1, 2, 3, 8, 9, 10}
    assert len(w["ext_cp"]) == sum(m + 1 for m in tiles.tolist() if m > 8)
    L = w["op_lines"]
    assert len(L) == sum(((int(r["cigar_len"]) + 25) // 26) for r in f.records)
    lens = L[:, 6:] & ir.OP_LEN_MASK
    real = L[:, 6:] != ir.OP_PAD
    assert (real[:, 0] & (lens[:, 0] == 0)).any() and (real[:, 25] & (lens[:, 25] == 0)).any()
    assert (real.all(axis=1) & (lens == 0).all(axis=1)).any()  # a whole tile of zero-length ops


def test_width_reaches_its_edges():
    f, w = model("width")
    L, P = w["op_lines"], w["pfx"]
    lwide = L[:, 2] == 0xFFFFFFFF
    pwide = (P[:, 0] >> 31) == 1
    assert (pwide <= lwide).all()
    # per record: (first | second tile is the wide one) x (65534: neither line, 65535: the op line alone, 65536: both)
    seen = set()
    base = 0
    for r in f.records:
        m = (int(r["cigar_len"]) + 25) // 26
        assert m == 2
        seen.add((bool(lwide[base]), bool(pwide[base]), bool(lwide[base + 1]), bool(pwide[base + 1])))
        base += m
    assert seen == {(False, False, False, False), (True, False, False, False), (True, True, False, False),
                    (False, False, True, False), (False, False, True, True)}
    # the sum arrives with the last op only: every entry before it fits, the tile's end alone is wide
    ent = P[:, 4:30]
    only_end = pwide & (np.maximum(ent & 0xFFFF, ent >> 16) == np.arange(26)).all(axis=1)  # 26 ops of length 1 ... 1, 65511
    assert only_end.sum() == 4  # 65536 on either axis, as tile 0 and as tile 1
    # ... and first at entry 9 / entry 18 (the copies in words 2, 3)
    for word, k in ((2, 9), (3, 18)):
        assert (P[:, word] == P[:, 4 + k]).all()
        hit = (np.maximum(P[:, 4 + k] & 0xFFFF, P[:, 4 + k] >> 16) >= 65534) & (np.maximum(P[:, 3 + k] & 0xFFFF, P[:, 3 + k] >> 16) < 100)
        assert hit.sum() >= 8
    sums_t = np.where(lwide, 0, L[:, 3] >> 16)
    sums_q = np.where(lwide, 0, L[:, 5] >> 16)
    assert (sums_t == 65534).sum() == 8 and (sums_q == 65534).sum() == 8


def test_gap_mask_reaches_its_edges():
    f, w = model("gap_mask")
    masks = w["idl"][:, 3].tolist()
    assert masks[:4] == [0x2000061, 0x2000061, 0x3FFFFFF, 0x1] and len(masks) == 12


def test_order_fixtures_tie_and_reach_the_signed_ends():
    f, w = model("order_paf")
    b = f.names.index("B")
    s = w["seg"][b]
    seg = w["entries"][int(s["a"]):int(s["a"]) + int(s["n"])]
    assert seg["ts"].tolist() == [40, 100, 100, 100, 100]
    assert [(int(e["nops_flags"]) >> 31, int(e["query_id"])) for e in seg[1:]] == [(0, f.names.index("A")), (0, f.names.index("C")), (1, f.names.index("C")), (1, f.names.index("A"))]
    f, w = model("order_records")
    assert [int(x["n"]) for x in w["seg"]] == [0, 6, 0, 5, 0]
    a = int(w["seg"][1]["a"])
    assert w["starts"][a:a + 6].tolist() == [-5, 0, 0, 7, 20, ir.INT32_MAX]
    assert w["ends"][a + 1] == 10 and w["ends"][a + 2] == ir.INT32_MAX  # the tie keeps record order
    assert w["ends_t"][a + 4] == ir.INT32_MIN and w["ends_t"][a + 5] == ir.INT32_MIN  # te < ts, te == ts
    assert w["pmax"][a + 5] == ir.INT32_MAX
    a3 = int(w["seg"][3]["a"])
    assert (w["pmax"][a3:a3 + 5] < 0).all()  # the running maximum restarted
    for n in (1, 2, 3, 5):
        f, w = model("order_nseq%d" % n)
        assert len(f.seq_len) == n and all(int(x["n"]) > 0 for x in w["seg"])


def test_levels_reach_their_edges():
    f, w = model("levels", identity_lines=False)
    assert [(int(s["n"]), int(s["nlev"])) for s in w["seg"]] == [(1, 0), (64, 0), (65, 1), (4096, 1), (4097, 2), (0, 0)]
    assert [s["cnt"].tolist() for s in w["seg"][2:5]] == [[2, 0, 0, 0], [64, 0, 0, 0], [65, 2, 0, 0]]
    assert len(w["starts_lvl"]) == 2 + 64 + 65 + 2
    assert len(np.unique(w["starts"])) < len(w["starts"]) // 2  # ties
    f3 = bg.fixture("level3")
    w3 = ir.expected_index(f3.records, f3.ops, f3.seq_len, False, lines=False)
    assert int(w3["seg"][0]["nlev"]) == 3 and w3["seg"][0]["cnt"].tolist() == [4097, 65, 2, 0]
    assert w3["starts_lvl"][-1] == w3["starts"][-1] and w3["pmax_lvl"][-1] == w3["pmax"][-1]


def test_pool_shapes():
    shapes = {s: bg.fixture("pool_" + s) for s in ("in_order", "gaps", "shared", "reversed")}
    assert shapes["in_order"].monotone() and shapes["gaps"].monotone()
    assert not shapes["shared"].monotone() and not shapes["reversed"].monotone()
    assert shapes["gaps"].records[0]["cigar_off"] == 5 and len(shapes["gaps"].ops) == len(shapes["in_order"].ops) + 35
    r = shapes["shared"].records
    assert r[3]["cigar_off"] == r[1]["cigar_off"] and r[3]["cigar_len"] == r[1]["cigar_len"]
    want = ir.expected_index(shapes["in_order"].records, shapes["in_order"].ops, shapes["in_order"].seq_len, True, True, True)
    for s in ("gaps", "reversed"):  # the same alignments whatever the pool's layout
        f = shapes[s]
        assert ir.diff_index(ir.expected_index(f.records, f.ops, f.seq_len, True, True, True), want) is None
    with pytest.raises(ValueError):
        model("pool_bad_op")
    # a sharded build: every record is needed by the owner of its target; the model skips a record no owner of THIS shard needs
    f = bg.fixture("pool_bad_op")
    owner = np.array([0, 1, 2])
    bad_rec = f.records[3]
    for shard in range(3):
        needed = shard in (int(bad_rec["target_id"]), int(bad_rec["query_id"]))
        if needed:
            with pytest.raises(ValueError):
                ir.expected_index(f.records, f.ops, f.seq_len, True, owner=owner, shard=shard)
        else:
            ir.expected_index(f.records, f.ops, f.seq_len, True, owner=owner, shard=shard)


def test_sharded_model_partitions_the_entries():
    f = bg.fixture("tile_fill")
    whole = ir.expected_index(f.records, f.ops, f.seq_len, True)
    owner = np.arange(len(f.seq_len)) % 3
    parts = [ir.expected_index(f.records, f.ops, f.seq_len, True, owner=owner, shard=k) for k in range(3)]
    assert sum(len(p["entries"]) for p in parts) == len(whole["entries"])
    assert all(len(p["op_lines"]) < len(whole["op_lines"]) for p in parts)
    for k, p in enumerate(parts):
        for s, d in enumerate(p["seg"]):
            assert (int(d["n"]) == int(whole["seg"][s]["n"])) if owner[s] == k else int(d["n"]) == 0


# ---- read_index against a pure-Python writer ----------------------------------------------------------------------------
def write_index(path, blobs, lens, names, file_first, tgt_off, flags, n_records, n_tiles, n_targets, shard=None):
    """The file format of GpuImpg.save: header, host tables, the 15 arrays, end mark, FNV sum (one sum step per table)."""
    raw = [np.ascontiguousarray(blobs[n]).tobytes() if n in blobs else b"" for n in ir.BLOB_NAMES]
    n_entries = len(blobs["entries"])
    parts = [ir.HEADER.pack(ir.MAGIC, ir.VERSION, 32, 26, 4, 64, len(lens), 0, flags, n_records, n_entries, n_tiles, n_targets,
                            len(names), len(file_first), len(tgt_off), *[len(b) for b in raw]),
             np.asarray(lens, dtype="<i8").tobytes()]
    for nm in names:
        parts += [struct.pack("<I", len(nm)), nm.encode()]
    parts += [np.asarray(file_first, dtype="<u8").tobytes(), np.asarray(tgt_off, dtype="<u4").tobytes()]
    if shard:
        parts += [struct.pack("<3I", shard["world"], shard["rank"], len(shard["owner"])), np.asarray(shard["owner"], dtype="<u4").tobytes()]
    parts += raw + [struct.pack("<Q", ir.END_MARK ^ n_entries)]
    h = ir.FNV_SEED
    for p in parts:
        h = ir.fnv64(h, p)
    with open(path, "wb") as out:
        out.write(b"".join(parts) + struct.pack("<Q", h))


@pytest.mark.parametrize("prefix_lines,identity_lines,sharded", [(True, True, False), (True, False, True), (False, False, False)])
def test_read_index_round_trip(tmp_path, prefix_lines, identity_lines, sharded):
    f = bg.fixture("tile_fill")
    owner = np.arange(len(f.seq_len)) % 2 if sharded else None
    w = ir.expected_index(f.records, f.ops, f.seq_len, True, prefix_lines, identity_lines, owner=owner, shard=1)
    w["rank"] = np.zeros(len(w["entries"]), dtype=np.uint32)
    flags = (0 if prefix_lines else ir.F_NO_PFX) | (ir.F_LAZY_IDL if prefix_lines and not identity_lines else 0) | (ir.F_SHARD if sharded else 0)
    path = str(tmp_path / "x.idx")
    write_index(path, w, f.seq_len, f.names, [0, len(f.records)], w["tgt_off"], flags, len(f.records), len(w["op_lines"]),
                int((w["seg"]["n"] > 0).sum()), shard=dict(world=2, rank=1, owner=owner) if sharded else None)
    got = ir.read_index(path)
    assert ir.diff_index(got, w) is None
    assert got["names"] == f.names and got["lens"].tolist() == f.seq_len.tolist() and got["tgt_off"].tolist() == w["tgt_off"].tolist()
    assert got["n_tiles"] == len(w["op_lines"]) and got["flags"] == flags
    assert (got["shard"]["owner"].tolist() == owner.tolist() and got["shard"]["rank"] == 1) if sharded else got["shard"] is None
    # damage: one flipped bit inside an array fails the sum, a cut file fails before it
    data = bytearray(open(path, "rb").read())
    data[len(data) // 2] ^= 4
    open(path, "wb").write(bytes(data))
    with pytest.raises(ValueError, match="checksum"):
        ir.read_index(path)
    open(path, "wb").write(bytes(data[:-40]))
    with pytest.raises(ValueError):
        ir.read_index(path)


def test_diff_index_names_the_place():
    f, w = model("gap_mask")
    fresh = lambda: {k: np.array(v, copy=True) for k, v in w.items()}  # noqa: E731
    g = fresh()
    assert ir.diff_index(g, w) is None
    g["pfx"][3, 2] ^= 1
    assert ir.diff_index(g, w).startswith("pfx[3] word 2 (copy of entry 9): got 0x")
    g["idl"][2, 3] = 0
    assert ir.diff_index(g, w).startswith("idl[2] word 3 (gap mask): got 0x0, expected 0x3ffffff")  # (blob order: 12 before 14)
    g = fresh()
    g["op_lines"][0, 9] = 7
    assert ir.diff_index(g, w).startswith("op_lines[0] word 9 (op 3): got 0x7, expected 0x")
    g["entries"][1]["tcp"][2] += 1
    assert ir.diff_index(g, w).startswith("entries[1].tcp: got ")
    g["seg"][1]["n"] += 1
    assert ir.diff_index(g, w).startswith("seg[1].n: got ")
    g = fresh()
    g["ext_cp"] = np.zeros(3, dtype=np.uint32)
    assert ir.diff_index(g, w) == "ext_cp: shape (3,), expected (0,)"
