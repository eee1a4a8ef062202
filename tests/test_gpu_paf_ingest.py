"""The streamed PAF ingest on the device (impg_amd/csrc/paf_ingest_device.hip): the hand-off against the Python model of the
reference's parser over the fixtures of tests/paf_ingest_gen.py (tests/test_paf_ingest_cpu.py proves without a GPU that
each sits on its edge), the built index against the one the host's line parser leads to -- the saved files byte for byte:
the file format does not record which route built it --, the error files through the public call, and the command line.
The counters prove in every case that the streamed route ran and cut the text where intended."""
import os
import subprocess

import pytest

import impg_amd
from impg_amd import _lib
from oracle import oracle as o
from tests import build_gen as bg
from tests import index_ref as ir
from tests import paf_ingest_gen as g
from tests import paf_ingest_ref as ref
from tests import seq_ingest_gen as sg

pytestmark = pytest.mark.gpu

CONTAINERS = ("plain", "gzip", "members", "bgzf")
BUILD_GEN_PAFS = ("tile_fill", "width", "gap_mask", "order_paf", "token_paf")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_paf_ingest")


_MODEL = {}


def model(name):
    if name not in _MODEL:
        _MODEL[name] = ref.ingest(g.fixture(name))
    return _MODEL[name]


def compare(got, want, what):
    for k in ("file_first", "names", "lens", "records", "ops"):
        if got[k] != want[k]:
            bad = [(i, a, b) for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b][:3]
            raise AssertionError("%s: %s differs (%d against %d): first %s" % (what, k, len(got[k]), len(want[k]), bad))


# ---- the hand-off against the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("container", CONTAINERS)
@pytest.mark.parametrize("name", sorted(g.FIXTURES))
def test_device_equals_model(folder, name, container):
    """every fixture x piece size x container (pieces of 16 and 48 bytes for the fixtures up to 4 KB: about a thousand pieces
    a case at the most); name hashes cut to one bit and a first pool of 64 ops at two piece sizes each"""
    texts, want = g.fixture(name), model(name)
    paths = g.write(texts, folder, name, container)
    small = sum(len(t) for t in texts) <= 4096
    runs = [(p, 64, 0) for p in g.PIECE_SIZES if p not in (16, 48) or small] + [(256, 1, 0), (0, 1, 0), (1024, 64, 64), (0, 64, 64)]
    for piece, hash_bits, pool in runs:
        got, st = g.selftest(paths, piece, on_host=False, hash_bits=hash_bits, pool_ops=pool)
        what = "%s %s piece %d hash_bits %d pool %d" % (name, container, piece, hash_bits, pool)
        compare(got, want, what)
        c = g.cut(texts, piece)
        assert (st["pieces"], st["carried_bytes"], st["buffer_grows"]) == (c["pieces"], c["carried"], c["grows"]), what
        assert st["device"] == 1 and st["lines"] == len(want["records"]) and st["text_bytes"] == sum(len(t) for t in texts), what
        assert (st["inflated_blocks"] > 0) == (container == "bgzf" and any(texts)), what
        if pool == 64 and len(want["ops"]) > 64:
            assert st["pool_regrows"] > 0, what


# ---- the index the hand-off leads to ------------------------------------------------------------------------------------------
def same_bytes(a, b, what):
    x, y = open(a, "rb").read(), open(b, "rb").read()
    if x != y:
        ga, gb = ir.read_index(a, check_sum=False), ir.read_index(b, check_sum=False)
        raise AssertionError("%s: the streamed and the host route's files differ: %s" % (what, ir.diff_index(ga, gb, blobs=ir.BLOB_NAMES) or "outside the arrays"))


def route_counters(gx):
    return tuple(gx.counter(k) for k in ("paf_ingest_device", "tokenized_device", "build_device"))


def fixture_texts(name):
    if name in BUILD_GEN_PAFS:
        return [t.encode() for t in bg.fixture(name).paf], bg.fixture(name).bidirectional
    return g.fixture(name), True


@pytest.mark.parametrize("name", BUILD_GEN_PAFS + tuple(sorted(g.FIXTURES)))
def test_index_equals_host_route(folder, tmp_path, name):
    texts, bidirectional = fixture_texts(name)
    paths = g.write(texts, folder, "ix_" + name)
    host = impg_amd.GpuImpg.from_paf(paths, bidirectional=bidirectional)
    assert route_counters(host) == (0, 1, 1) and host.counter("paf_ingest_pieces") == 0
    host.save(str(tmp_path / "host.idx"))
    for piece in (256, 4096):
        dev = impg_amd.GpuImpg.from_paf(paths, bidirectional=bidirectional, ingest="device", piece_bytes=piece)
        assert route_counters(dev) == (1, 1, 1), (name, piece)
        c = g.cut(texts, piece)
        assert dev.counter("paf_ingest_pieces") == c["pieces"] and (c["pieces"] > 1 or piece == 4096), (name, piece)
        assert dev.counter("paf_ingest_buffer_grows") == c["grows"] and dev.counter("paf_ingest_carried_bytes") == c["carried"]
        dev.save(str(tmp_path / ("dev%d.idx" % piece)))
        del dev
        same_bytes(str(tmp_path / ("dev%d.idx" % piece)), str(tmp_path / "host.idx"), "%s piece %d" % (name, piece))


def test_every_index_fixture_takes_more_than_one_piece():
    """(the counters above must prove the route: at 256 bytes every fixture is cut into several pieces, and at 4096 every
    fixture that is longer than 4096 bytes -- a fixture of a few hundred bytes is one piece there whatever the route does)"""
    for name in BUILD_GEN_PAFS + tuple(sorted(g.FIXTURES)):
        texts = fixture_texts(name)[0]
        assert g.cut(texts, 256)["pieces"] > 1, name
        assert g.cut(texts, 4096)["pieces"] > 1 or max(len(t) for t in texts) <= 4096, name


@pytest.fixture(scope="module")
def synth(folder):
    """20 000 records of the synthetic workload (about 12 MB), plain and as BGZF, and the host route's saved index"""
    shape = dict(n_seq=200, seq_len=5_000_000, target_span=10_000, n_blocks=100)
    plain = impg_amd.synth_paf_text(str(folder / "synth.paf"), 11, 20000, **shape)
    text = open(plain, "rb").read()
    bgz = str(folder / "synth.paf.gz")
    with open(bgz, "wb") as f:
        f.write(sg.bgzf(text, block_sizes=(65280,), empty_after=-1))
    host = impg_amd.GpuImpg.from_paf(plain)
    host.save(str(folder / "synth_host.idx"))
    del host
    return plain, bgz, str(folder / "synth_host.idx"), shape, len(text)


@pytest.mark.parametrize("which", ("plain", "bgzf"))
def test_synthetic_file(synth, tmp_path, which):
    plain, bgz, host_idx, shape, n_bytes = synth
    dev = impg_amd.GpuImpg.from_paf(plain if which == "plain" else bgz, ingest="device", piece_bytes=1 << 20)
    assert route_counters(dev) == (1, 1, 1) and dev.counter("paf_ingest_pieces") >= n_bytes >> 20 and dev.counter("paf_ingest_lines") == 20000
    assert dev.counter("paf_ingest_text_bytes") == n_bytes and (dev.counter("paf_ingest_inflated_blocks") > 0) == (which == "bgzf")
    dev.save(str(tmp_path / "dev.idx"))
    same_bytes(str(tmp_path / "dev.idx"), host_idx, which)
    c = o.OracleIndex(paf_paths=[plain], preparse=True)
    bed = impg_amd.synth_bed(7, 64, n_seq=shape["n_seq"], seq_len=shape["seq_len"], range_len=5000)
    ranges = [(dev.seq_id(impg_amd.synth_seq_name(int(r["target_id"]))), int(r["start"]), int(r["end"])) for r in bed]
    res = dev.query_batch(ranges, impg_amd.make_params(transitive=True, max_depth=3))
    for i, (t, s, e) in enumerate(ranges):
        assert res[i].tolist() == c.query(t, s, e, transitive=True, max_depth=3).tolist(), i
    assert res.projected > 64


# ---- errors through the public call -------------------------------------------------------------------------------------------
def free_hbm():
    """hipMemGetInfo's free bytes, asked of the HIP runtime the library itself runs on (already loaded: found in the process map)"""
    import ctypes as C
    impg_amd.lib()
    with open("/proc/self/maps") as f:
        path = next(ln.split()[-1] for ln in f if "libamdhip64" in ln)
    hip = C.CDLL(path)
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


@pytest.mark.parametrize("kind", sorted(g.ERRORS))
def test_error_files_through_the_public_call(folder, kind):
    """Same code and message as the host route on the same file, no handle, the HBM back, a good call behind it.  The bound on
    the HBM: every block the ingest takes is its backend's and is freed with hipFree when the call ends, so what may differ
    is the runtime's own bookkeeping, which it grows in 2 MiB granules; a good call runs first so that the code object, the
    stream pools and the pinned pool of the process are in place before the first reading.  16 MiB allows eight granules."""
    bad = g.write(g.error_file(kind), folder, "pub_bad_" + kind)
    good = g.write(g.fixture("files"), folder, "pub_good_" + kind)
    del_me = impg_amd.GpuImpg.from_paf(good, ingest="device", piece_bytes=256)
    del del_me
    with pytest.raises(_lib.ImpgGpuError) as host:
        impg_amd.GpuImpg.from_paf(bad)
    for piece in (256, 4096):
        before = free_hbm()
        with pytest.raises(_lib.ImpgGpuError) as dev:
            impg_amd.GpuImpg.from_paf(bad, ingest="device", piece_bytes=piece)
        after = free_hbm()
        assert (dev.value.code, str(dev.value)) == (host.value.code, str(host.value)) and dev.value.code == _lib.IMPG_E_INVALID
        assert str(dev.value).endswith("Failed to parse PAF: " + g.ERRORS[kind])
        print("free HBM before %d after %d (difference %d bytes)" % (before, after, before - after))
        assert abs(before - after) <= 16 << 20, (before, after)
    ok = impg_amd.GpuImpg.from_paf(good, ingest="device", piece_bytes=256)
    assert ok.counter("paf_ingest_device") == 1 and ok.counter("paf_ingest_lines") == len(model("files")["records"])


def test_reader_trouble_through_the_public_call(folder):
    missing = str(folder / "nowhere.paf")
    with pytest.raises(_lib.ImpgGpuError) as e:
        impg_amd.GpuImpg.from_paf(missing, ingest="device")
    assert e.value.code == _lib.IMPG_E_IO and missing in str(e.value)


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_command_line(synth, tmp_path):
    """--alignment-ingest device prints the bytes --alignment-ingest host prints, from the plain and the bgzipped file"""
    plain, bgz, _, shape, _ = synth
    bed = str(tmp_path / "q.bed")
    with open(bed, "w") as f:
        for r in impg_amd.synth_bed(9, 16, n_seq=shape["n_seq"], seq_len=shape["seq_len"], range_len=5000):
            f.write("%s\t%d\t%d\n" % (impg_amd.synth_seq_name(int(r["target_id"])), int(r["start"]), int(r["end"])))
    cli = os.path.join(os.path.dirname(impg_amd.__file__), "impg-gpu")
    out = {}
    for paf in (plain, bgz):
        for ingest in ("host", "device"):
            r = subprocess.run([cli, "query", "-a", paf, "-b", bed, "-x", "-m", "3", "-d", "0", "--alignment-ingest", ingest], capture_output=True, timeout=120)
            assert r.returncode == 0 and r.stdout.count(b"\n") > 16, r.stderr
            out[paf, ingest] = r.stdout
    assert len(set(out.values())) == 1
    r = subprocess.run([cli, "query", "-a", plain, "-b", bed, "-d", "0", "--alignment-ingest", "gpu"], capture_output=True, timeout=120)
    assert r.returncode == 2 and r.stdout == b""
