"""The device index build (impg_amd/csrc/index_build_device.hip: eleven kernels, the CIGAR tokenizer among them) against
an independent model of the built index (tests/index_ref.py), against the host builder byte for byte, and against the
oracle for entry order, tokens and refusals -- on fixtures that each sit on one edge of the file (tests/build_gen.py;
tests/test_build_gen_cpu.py proves without a GPU that they do).  Every case asserts the build counters, so a build that
quietly fell back to the host builder fails instead of comparing the host builder with itself."""
import contextlib
import os

import numpy as np
import pytest

import impg_amd
from oracle import oracle as o
from tests import build_gen as bg
from tests import index_ref as ir

pytestmark = pytest.mark.gpu

VARIANTS = {"default": ({}, True, False), "no_prefix_lines": ({"IMPG_PREFIX_LINES": "0"}, False, False),
            "identity_lines": ({"IMPG_IDENTITY_LINES": "1"}, True, True), "lazy_identity_lines": ({}, True, True)}
PAF_FIXTURES = ("tile_fill", "width", "gap_mask", "order_paf", "token_paf")
RECORD_FIXTURES = tuple(n for n in bg.SMALL if n not in PAF_FIXTURES)


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@pytest.fixture(scope="module")
def paf_paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("build_paf")
    out = {}
    for name in PAF_FIXTURES:
        out[name] = []
        for k, text in enumerate(bg.fixture(name).paf):
            out[name].append(str(d / ("%s.%d.paf" % (name, k))))
            with open(out[name][-1], "w", newline="") as f:
                f.write(text)
    return out


def build(f, paths=None, host=False, variant="default", entry=None, batch=None, devices=None, ops=None):
    """One build of fixture f through from_paf (paths) or from_records, by the device or the host builder."""
    kv = dict(VARIANTS[variant][0])
    if host:
        kv["IMPG_BUILD_HOST"] = "1"
    if batch:
        kv["IMPG_BUILD_BATCH_OPS"] = str(batch)
    kw = dict(devices=devices, lanes=1) if devices else {}
    with env(**kv):
        if (entry or ("paf" if f.paf else "records")) == "paf":
            return impg_amd.GpuImpg.from_paf(paths[f.name], bidirectional=f.bidirectional, **kw)
        ff = f.file_first[:-1] if f.paf and len(f.paf) > 1 else None
        return impg_amd.GpuImpg.from_records(f.records, f.ops if ops is None else ops, f.seq_len, bidirectional=f.bidirectional, file_first=ff, **kw)


def touch_identity(g, f):
    """the first query that filters by identity builds the identity lines (here one that hits nothing: no fixture has an
    entry over the middle of sequence 0, and a hit on a record without ops would be refused)"""
    assert len(g.query(0, bg.SEQ_LEN // 2, bg.SEQ_LEN // 2 + 5, min_gap_compressed_identity=0.5)) == 1


def counters(g):
    return tuple(g.counter(k) for k in ("build_device", "tokenized_device", "build_batches"))


_MODEL = {}


def expected(f, variant, owner=None, shard=0):
    key = (f.name, VARIANTS[variant][1:], None if owner is None else (tuple(owner), shard))
    if key not in _MODEL:
        _MODEL[key] = ir.expected_index(f.records, f.ops, f.seq_len, f.bidirectional, *VARIANTS[variant][1:], owner=owner, shard=shard)
    return _MODEL[key]


def same_bytes(a, b, what):
    x, y = open(a, "rb").read(), open(b, "rb").read()
    if x != y:
        ga, gb = ir.read_index(a, check_sum=False), ir.read_index(b, check_sum=False)
        raise AssertionError("%s: device and host files differ: %s" % (what, ir.diff_index(ga, gb, blobs=ir.BLOB_NAMES) or "outside the arrays"))


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", PAF_FIXTURES + RECORD_FIXTURES)
def test_build_matches_model_and_host(tmp_path, paf_paths, name, variant):
    f = bg.fixture(name)
    files = {}
    for mode in ("device", "host"):
        g = build(f, paf_paths, host=mode == "host", variant=variant)
        want_ctr = (0, 0, 0) if mode == "host" else (1, 1 if f.paf else 0, 1 if len(f.records) else 0)
        assert counters(g) == want_ctr, (mode, counters(g))
        if variant == "lazy_identity_lines":
            touch_identity(g, f)
        files[mode] = str(tmp_path / (mode + ".idx"))
        g.save(files[mode])
        del g
    got = ir.read_index(files["device"])
    assert ir.diff_index(got, expected(f, variant)) is None, ir.diff_index(got, expected(f, variant))
    ir.check_ranks(got)
    n_tiles = len(got["op_lines"])
    assert got["flags"] & (ir.F_NO_PFX | ir.F_LAZY_IDL) == (0 if not n_tiles else ir.F_NO_PFX if variant == "no_prefix_lines" else
                                                            ir.F_LAZY_IDL if variant == "default" else 0)
    assert got["tgt_off"].tolist() == expected(f, variant)["tgt_off"].tolist() and got["n_records"] == len(f.records)
    if f.paf:
        assert got["names"] == f.names and got["lens"].tolist() == f.seq_len.tolist() and got["file_first"].tolist() == f.file_first.tolist()
    same_bytes(files["device"], files["host"], name)


def test_level3(tmp_path):
    """262 145 entries on one target (nlev = 3): seg, the columns and the levels against the model; every array host
    against device.  The file is 84 MB: its FNV sum is left to load_index (the interpreted sum would take seconds)."""
    f = bg.fixture("level3")
    files = {}
    for mode in ("device", "host"):
        g = build(f, host=mode == "host")
        assert counters(g) == ((1, 0, 1) if mode == "device" else (0, 0, 0))
        files[mode] = str(tmp_path / (mode + ".idx"))
        g.save(files[mode])
        del g
    got = ir.read_index(files["device"], check_sum=False)
    want = ir.expected_index(f.records, f.ops, f.seq_len, False, lines=False)
    assert int(got["seg"][0]["nlev"]) == 3
    assert ir.diff_index(got, want) is None, ir.diff_index(got, want)
    same_bytes(files["device"], files["host"], "level3")
    impg_amd.GpuImpg.load(files["device"])  # (the native reader checks the sum)


@pytest.mark.parametrize("name", PAF_FIXTURES)
def test_from_paf_against_from_records(tmp_path, paf_paths, name):
    """The same input through both entry points gives the same arrays (header and name table differ).  from_paf reads an op
    pool the device tokenizer left in HBM; from_records is handed the oracle's tokens of the same text."""
    f = bg.fixture(name)
    rec, ops, _, _, _ = bg.paf_records(f.paf, tokens=lambda t: o.parse_cigar(t).tolist())
    assert rec.tolist() == f.records.tolist() and ops.tolist() == f.ops.tolist()  # (the Python tokenizer is the oracle's)
    a, b = build(f, paf_paths), build(f, entry="records", ops=ops)
    assert counters(a) == (1, 1, 1) and counters(b) == (1, 0, 1)
    a.save(str(tmp_path / "paf.idx"))
    b.save(str(tmp_path / "rec.idx"))
    ga, gb = ir.read_index(str(tmp_path / "paf.idx")), ir.read_index(str(tmp_path / "rec.idx"))
    assert ir.diff_index(ga, gb, blobs=ir.BLOB_NAMES) is None, ir.diff_index(ga, gb, blobs=ir.BLOB_NAMES)


def batches_of(f, batch):
    """consecutive records whose ops fit the batch; a record larger than a batch travels alone"""
    n, b0, count = len(f.records), 0, 0
    off, ln = f.records["cigar_off"].astype(np.int64), f.records["cigar_len"].astype(np.int64)
    while b0 < n:
        b1 = b0
        while b1 < n and (b1 == b0 or off[b1] + ln[b1] - off[b0] <= batch):
            b1 += 1
        count, b0 = count + 1, b1
    return count


@pytest.mark.parametrize("batch", [1, 26, 27, 64])
@pytest.mark.parametrize("name", ["pool_in_order", "pool_gaps", "tile_fill"])
def test_batches(tmp_path, name, batch):
    """IMPG_BUILD_BATCH_OPS: the op pool crosses in batches of consecutive records (`cigar_off - ops_first`); the arrays are
    those of the one-batch build and of the model."""
    f = bg.fixture(name)
    assert f.monotone()
    one, many = build(f, entry="records"), build(f, entry="records", batch=batch)
    assert counters(one) == (1, 0, 1)
    want = batches_of(f, batch)
    assert want > 1 and counters(many) == (1, 0, want), (counters(many), want)
    if batch == 26 and name == "tile_fill":
        assert int(f.records["cigar_len"].max()) > batch  # a record larger than a batch
    one.save(str(tmp_path / "one.idx"))
    many.save(str(tmp_path / "many.idx"))
    assert open(str(tmp_path / "one.idx"), "rb").read() == open(str(tmp_path / "many.idx"), "rb").read()
    got = ir.read_index(str(tmp_path / "many.idx"))
    assert ir.diff_index(got, expected(f, "default")) is None, ir.diff_index(got, expected(f, "default"))


def test_non_monotone_pools_upload_whole(tmp_path):
    """a shared CIGAR and a pool in reverse record order: one launch whatever the batch size, ops_first = 0"""
    for name in ("pool_shared", "pool_reversed"):
        f = bg.fixture(name)
        g = build(f, batch=1)
        assert counters(g) == (1, 0, 1)
        g.save(str(tmp_path / (name + ".idx")))
        got = ir.read_index(str(tmp_path / (name + ".idx")))
        assert ir.diff_index(got, expected(f, "default")) is None, ir.diff_index(got, expected(f, "default"))


@pytest.mark.parametrize("name,entry,batch", [("tile_fill", "paf", None), ("tile_fill", "records", 26), ("token_paf", "paf", None),
                                              ("pool_in_order", "records", 1), ("order_records", "records", None)])
def test_sharded(tmp_path, paf_paths, name, entry, batch):
    """devices=[0, 0, 0]: every shard file is the model's index of the entries that shard owns (tile_base numbered over the
    records it needs) and its host-built twin.  With a batch size, batches start at records the shard skips."""
    f = bg.fixture(name)
    paths = {}
    for mode in ("device", "host"):
        g = build(f, paf_paths, host=mode == "host", entry=entry, batch=batch, devices=[0, 0, 0])
        ctr = counters(g)
        if mode == "host":
            assert ctr == (0, 0, 0)
        else:  # sums over the three ranks; a multi handle's PAF is tokenised on the host
            assert ctr[:2] == (3, 0) and (ctr[2] > 3 if batch else ctr[2] == 3), ctr
        paths[mode] = str(tmp_path / (mode + ".idx"))
        g.save(paths[mode])
        del g
    owners = []
    n_ent = 0
    for k in range(3):
        dev = "%s.shard%dof3" % (paths["device"], k)
        got = ir.read_index(dev)
        assert got["shard"]["world"] == 3 and got["shard"]["rank"] == k
        owners.append(got["shard"]["owner"].tolist())
        want = expected(f, "default", owner=owners[0], shard=k)
        assert ir.diff_index(got, want) is None, (k, ir.diff_index(got, want))
        ir.check_ranks(got)
        n_ent += got["n_entries"]
        same_bytes(dev, "%s.shard%dof3" % (paths["host"], k), "%s shard %d" % (name, k))
    assert owners[0] == owners[1] == owners[2] and len(set(owners[0])) > 1
    assert n_ent == len(expected(f, "default")["entries"])


@pytest.mark.parametrize("name", PAF_FIXTURES)
def test_order_and_tokens_against_the_oracle(tmp_path, paf_paths, name):
    """Every target's (start, end, query, strand | reversed << 1) sequence is the oracle tree's; the ops in the op lines
    (padding dropped) are oracle.parse_cigar of each record's text, lengths of 2^29 and more included."""
    f = bg.fixture(name)
    g = build(f, paf_paths)
    assert counters(g) == (1, 1, 1)
    g.save(str(tmp_path / "x.idx"))
    got = ir.read_index(str(tmp_path / "x.idx"))
    c = o.OracleIndex(paf_paths=paf_paths[name], preparse=True)
    E = got["entries"]
    for t in range(c.num_seqs()):
        a, n = int(got["seg"][t]["a"]), int(got["seg"][t]["n"])
        mine = [(int(e["ts"]), int(e["te"]), int(e["query_id"]), ((int(e["nops_flags"]) >> 30) & 1) | ((int(e["nops_flags"]) >> 31) << 1)) for e in E[a:a + n]]
        assert mine == [tuple(r) for r in c.target_entries(t).tolist()], t
    texts = [next((x[5:] for x in line.rstrip("\r").split("\t") if x.startswith("cg:Z:")), "") for text in f.paf for line in text.split("\n") if line.rstrip("\r")]
    assert len(texts) == len(f.records)
    by_record = {}
    for e in E:  # all records are needed here: every entry names its record's tiles
        n = int(e["nops_flags"]) & ir.OP_LEN_MASK
        tiles = got["op_lines"][int(e["tile_base"]):int(e["tile_base"]) + (n + 25) // 26, 6:].reshape(-1)
        assert (tiles[n:] == ir.OP_PAD).all()
        by_record.setdefault((int(e["tile_base"]), n), tiles[:n].tolist())
    want = sorted(o.parse_cigar(t).tolist() for t in texts if t and len(o.parse_cigar(t)))
    assert sorted(v for v in by_record.values() if v) == want


@pytest.mark.parametrize("host", [False, True])
def test_the_2_pow_30_record(tmp_path, host):
    """`5=1073741825=5=`: the reference packs (code << 29) | len without a mask, so the middle op reads as 1I.  Before the
    fix the library answered as for 5=1=5= (q:100-110, q:103-108)."""
    path = str(tmp_path / "r.paf")
    open(path, "w").write(bg.RECORD_2_30)
    with env(**({"IMPG_BUILD_HOST": "1"} if host else {})):
        g = impg_amd.GpuImpg.from_paf(path, bidirectional=False)
    assert counters(g) == ((0, 0, 0) if host else (1, 1, 1))
    c = o.OracleIndex(paf_paths=[path], bidirectional=False, preparse=True)
    t, q = g.seq_id("t"), g.seq_id("q")
    assert c.query(t, 200, 210).tolist() == o.OracleIndex(paf_text=bg.RECORD_2_30.replace("1073741825=", "1I"), bidirectional=False).query(t, 200, 210).tolist()
    ranges = [(t, 200, 210), (t, 203, 208)]
    for (s, e), (qs, qe) in zip([r[1:] for r in ranges], [(100, 111), (103, 109)]):
        got = g.query(t, s, e)
        assert got.tolist() == c.query(t, s, e).tolist()
        assert got[1].tolist() == (q, qs, qe, t, s, e)
    res = g.query_batch(ranges, impg_amd.make_params(store_cigar=True))
    for i, (_, s, e) in enumerate(ranges):
        want, wcg = c.query_cigar(t, s, e)
        assert res[i].tolist() == want.tolist()
        assert [x.tolist() for x in res.cigars(i)] == [x.tolist() for x in wcg]
    assert o.ops_to_pairs(res.cigars(0)[1]) == [(5, "="), (1, "I"), (5, "=")]
    one = g.query(t, 203, 208, store_cigar=True)
    assert one.tolist() == c.query(t, 203, 208).tolist()


def refusal(paths, host):
    with env(**({"IMPG_BUILD_HOST": "1"} if host else {})):
        with pytest.raises(impg_amd.ImpgGpuError) as ei:
            impg_amd.GpuImpg.from_paf(paths)
    return ei.value.code, str(ei.value)


@pytest.mark.parametrize("name,text", bg.bad_texts())
def test_bad_bytes_are_refused_alike(tmp_path, name, text):
    """a byte that is no digit and none of =XIDM, in the first record and in a later one: both builders refuse with the same
    code and message; the oracle refuses the same file"""
    for first in (True, False):
        path = str(tmp_path / ("bad%d.paf" % first))
        open(path, "w").write(bg.bad_paf(text, first))
        dev, host = refusal(path, False), refusal(path, True)
        assert dev == host and dev[0] == impg_amd.IMPG_E_INVALID and "Invalid CIGAR operation" in dev[1], (dev, host)
        with pytest.raises(RuntimeError, match="Invalid CIGAR operation"):
            o.OracleIndex(paf_paths=[path], preparse=True)


@pytest.mark.parametrize("text", bg.REFUSED_AT_BUILD)
def test_code_above_4_is_refused_at_build(tmp_path, text):
    """2684354560= is 0xA0000000 (code 5) and 4294967295= is code 7 after the OR: both builders refuse the index with
    "Invalid CIGAR operation" (the reference panics when the op is first read: DESIGN.md)."""
    for first in (True, False):
        path = str(tmp_path / ("c%d.paf" % first))
        open(path, "w").write(bg.bad_paf(text, first))
        dev, host = refusal(path, False), refusal(path, True)
        assert dev == host and dev[0] == impg_amd.IMPG_E_INVALID and dev[1].endswith("Invalid CIGAR operation"), (dev, host)


def test_code_5_in_the_pool():
    """from_records: code 5 in a record is refused by both builders, in a sharded build too (every record is needed by the
    owner of its target, so no record is skipped by all shards); code 5 in ops no record names is never read (pool_gaps)."""
    f = bg.fixture("pool_bad_op")
    for kw in (dict(), dict(host=True), dict(devices=[0, 0, 0]), dict(devices=[0, 0, 0], host=True), dict(batch=27)):
        with pytest.raises(impg_amd.ImpgGpuError) as ei:
            build(f, **kw)
        assert ei.value.code == impg_amd.IMPG_E_INVALID and str(ei.value).endswith("Invalid CIGAR operation"), kw
