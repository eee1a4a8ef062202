"""The streamed PAF ingest without a GPU: the host twin of its kernels behind the real reader and the real driver
(impg_gpu_selftest_paf_ingest, on_host = 1) against a plain Python model of the reference's parser
(tests/paf_ingest_ref.py), for every fixture x piece size x container; the fixtures' own self-checks (each sits on the
edge it names); the counters against the generator's restatement of the piece cutting; the error files; and the
stand-alone sanitizer program over the fixture files."""
import os
import subprocess

import pytest

import impg_amd
from impg_amd import _lib
from tests import paf_ingest_gen as g
from tests import paf_ingest_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTAINERS = ("plain", "gzip", "members", "bgzf")
VARIANTS = ((64, 0), (1, 0), (64, 64))  # (hash_bits, initial_pool_ops)


# ---- the fixtures sit where they say ----------------------------------------------------------------------------------------
def test_fixtures_are_small():
    for name in g.FIXTURES:
        assert all(len(t) <= 16384 for t in g.fixture(name)), name
    for kind in g.ERRORS:
        assert len(g.error_file(kind)[0]) <= 16384


def test_straddle_splits_the_tag_at_every_edge():
    s = g.tag_splits(g.fixture("straddle")[0])
    assert s[16] == {1, 2, 3, 4} and s[1024] == {1, 2, 3, 4} and len(s[4096]) >= 3, s
    assert len(g.fixture("straddle")[0]) > 3 * 4096  # more than one 256-thread block of 16-byte lanes


def test_forms_holds_every_form():
    t = g.fixture("forms")[0]
    lines = ref.lines_of(t)
    f = [ln.split(b"\t") for ln in lines]
    tags = [[k for k, x in enumerate(fl) if x.startswith(g.TAG)] for fl in f]
    assert any(tg and tg[0] < len(fl) - 1 for tg, fl in zip(tags, f))            # not the last field
    assert any(not tg for tg in tags) and any(len(tg) == 2 for tg in tags)         # absent; twice
    assert any(tg[:1] == [0] for tg in tags)                                       # field 0
    assert any(any(x.startswith(b"x" + g.TAG) for x in fl) and not tg for tg, fl in zip(tags, f))
    assert any(fl[-1] == g.TAG for fl in f) and t.count(g.TAG + b"\r\n") == 1      # nothing behind it, with and without '\r'
    assert any(len(fl) == 12 and tg == [11] for tg, fl in zip(tags, f)) and any(len(fl) == 12 and not tg for tg, fl in zip(tags, f))
    assert any(tg[:1] == [20] for tg in tags)                                      # 20 fields before the tag
    assert b"\r\n" in t and not t.endswith(b"\n")
    nums = [ref.to_u64(x) for fl in f for x in fl[1:4]]
    assert any(fl[1].startswith(b"+") for fl in f)
    big = [int(x) for fl in f for x in (fl[2], fl[3], fl[7], fl[8])]
    assert any(2 ** 31 <= v < 2 ** 32 for v in big) and any(v >= 2 ** 64 for v in big) and None not in nums
    names = [x for fl in f for x in (fl[0], fl[5])]
    assert b"" in names and any(a != b and b.startswith(a) and a for a in names for b in names)
    lens = {}
    for fl in f:
        for nm, ln in ((fl[0], fl[1]), (fl[5], fl[6])):
            lens.setdefault(nm, set()).add(ln)
    assert any(len(v) > 1 for v in lens.values())                                   # one name, two lengths
    m = ref.ingest([t])
    assert m["lens"][m["names"].index(b"q1")] == 1000                              # ... the first wins


def test_files_continue_ids_across_an_empty_file():
    texts = g.fixture("files")
    assert len(texts) == 4 and texts[1] == b"" and not texts[2].endswith(b"\n")
    m = ref.ingest(texts)
    assert m["file_first"] == [0, 2, 2, 4, 6] and len(m["names"]) == 7
    per_file = [{x for ln in ref.lines_of(t) for x in (ln.split(b"\t")[0], ln.split(b"\t")[5])} for t in texts]
    assert per_file[0] & per_file[2] and per_file[0] & per_file[3] and per_file[2] - per_file[0] and per_file[3] - per_file[0] - per_file[2]


@pytest.mark.parametrize("name,early", [("big_first", True), ("big_last", False)])
def test_big_cigar_grows_the_buffer(name, early):
    """the 8 KB line makes the buffer double -- before the first piece is done, or after several are"""
    t = g.fixture(name)[0]
    lines = t.split(b"\n")[:-1]
    big = 0 if early else len(lines) - 1
    assert len(lines[big]) > 8000 and all(len(x) < 200 for k, x in enumerate(lines) if k != big)
    for piece in (16, 48, 256, 1024, 4096):
        c = g.cut([t], piece)
        assert c["grows"] >= 1 and (c["grow_at"][-1] == 0 if early else c["grow_at"][-1] > 0), (piece, c["grow_at"])
    assert g.cut([t], 0)["grows"] == 0


@pytest.mark.parametrize("size", [16, 48, 256, 1024, 4096])
def test_crlf_edges(size):
    """a read of the buffer ends between '\\r' and '\\n', and another right behind a '\\n'"""
    t = g.fixture("crlf_%d" % size)[0]
    reads = g.cut([t], size)["reads"][0]
    assert any(0 < r < len(t) and t[r - 1:r + 1] == b"\r\n" for r in reads), reads
    assert any(0 < r < len(t) and t[r - 1:r] == b"\n" for r in reads), reads
    assert t.count(b"\n") == t.count(b"\r\n")


@pytest.mark.parametrize("kind", sorted(g.ERRORS))
def test_error_files_have_one_bad_line_behind_the_first_piece(kind):
    t = g.error_file(kind)[0]
    with pytest.raises(ref.ParseError, match=g.ERRORS[kind].replace("+", r"\+")):
        ref.ingest([t])
    lines = t.split(b"\n")[:-1]
    bad = [k for k, ln in enumerate(lines) if _fails(ln)]
    assert len(bad) == 1
    at = sum(len(ln) + 1 for ln in lines[:bad[0]])
    assert at > 4096  # (whatever the piece size up to 4096, the first piece ends before the bad line)


def _fails(ln):
    try:
        ref.ingest([ln])
        return False
    except ref.ParseError:
        return True


# ---- the host twin against the model ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return tmp_path_factory.mktemp("paf_ingest")


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


@pytest.mark.parametrize("container", CONTAINERS)
@pytest.mark.parametrize("name", sorted(g.FIXTURES))
def test_host_twin_equals_model(folder, name, container):
    texts, want = g.fixture(name), model(name)
    paths = g.write(texts, folder, name, container)
    for piece in g.PIECE_SIZES:
        c = g.cut(texts, piece)
        for hash_bits, pool in VARIANTS:
            got, st = g.selftest(paths, piece, on_host=True, hash_bits=hash_bits, pool_ops=pool)
            what = "%s %s piece %d hash_bits %d pool %d" % (name, container, piece, hash_bits, pool)
            compare(got, want, what)
            assert (st["pieces"], st["carried_bytes"], st["buffer_grows"]) == (c["pieces"], c["carried"], c["grows"]), what
            assert st["text_bytes"] == sum(len(t) for t in texts) and st["lines"] == len(want["records"]) and st["device"] == 0, what
            assert st["unknown_names"] >= len(want["names"]), what
            assert (st["inflated_blocks"] > 0) == (container == "bgzf" and any(texts)), what
            if pool == 64 and len(want["ops"]) > 64:
                assert st["pool_regrows"] > 0, what
            if pool == 0:
                assert st["pool_regrows"] == 0, what


def test_pool_regrows_on_the_big_cigar(folder):
    paths = g.write(g.fixture("big_last"), folder, "regrow")
    got, st = g.selftest(paths, 1024, pool_ops=64)
    assert len(got["ops"]) > 1000 and st["pool_regrows"] >= 1


@pytest.mark.parametrize("container", ("plain", "bgzf"))
@pytest.mark.parametrize("kind", sorted(g.ERRORS))
def test_error_files(folder, kind, container):
    bad = g.write(g.error_file(kind), folder, "bad_" + kind, container)
    good = g.write(g.fixture("files"), folder, "good_after_" + kind, container)
    for piece in g.PIECE_SIZES:
        with pytest.raises(_lib.ImpgGpuError) as e:
            g.selftest(bad, piece)
        assert e.value.code == _lib.IMPG_E_INVALID and str(e.value).endswith("Failed to parse PAF: " + g.ERRORS[kind]), (piece, str(e.value))
        compare(g.selftest(good, piece)[0], model("files"), "a good call after %s" % kind)


@pytest.mark.parametrize("kind", ("same_line", "cigar_first"))
def test_first_bad_line_in_file_order(folder, kind):
    """a line's head checks come before its CIGAR check, and the first bad line in file order is the one reported"""
    texts, msg = g.error_order(kind)
    with pytest.raises(ref.ParseError, match=msg.replace("+", r"\+")):
        ref.ingest(texts)
    paths = g.write(texts, folder, "order_" + kind)
    for piece in g.PIECE_SIZES:
        with pytest.raises(_lib.ImpgGpuError) as e:
            g.selftest(paths, piece)
        assert str(e.value).endswith("Failed to parse PAF: " + msg), (piece, str(e.value))


def test_reader_trouble_names_the_file(folder):
    missing = str(folder / "not_there.paf")
    with pytest.raises(_lib.ImpgGpuError) as e:
        g.selftest([missing], 0)
    assert e.value.code == _lib.IMPG_E_IO and missing in str(e.value)
    cut_short = str(folder / "truncated.paf.gz")
    with open(cut_short, "wb") as f:
        f.write(g.containers(g.fixture("forms")[0])["gzip"][:-20])
    with pytest.raises(_lib.ImpgGpuError) as e:
        g.selftest([cut_short], 256)
    assert e.value.code == _lib.IMPG_E_IO and cut_short in str(e.value)


def test_bad_piece_sizes(folder):
    paths = g.write(g.fixture("files"), folder, "piece")
    for piece in (8, 24, 2 ** 32 + 16):
        with pytest.raises(_lib.ImpgGpuError) as e:
            g.selftest(paths, piece)
        assert e.value.code == _lib.IMPG_E_INVALID


def test_from_paf_refuses_device_ingest_on_several_gpus():
    with pytest.raises(ValueError):
        impg_amd.GpuImpg.from_paf("x.paf", ingest="device", devices=[0, 1])
    with pytest.raises(ValueError):
        impg_amd.GpuImpg.from_paf("x.paf", ingest="device", comm=object())
    with pytest.raises(ValueError):
        impg_amd.GpuImpg.from_paf("x.paf", ingest="elsewhere")


def test_sanitizer_program_over_the_fixtures(folder):
    """`make paf_ingest_check`: the reader, the driver and the host twin under -fsanitize=address,undefined, a program of its own"""
    csrc = os.path.join(ROOT, "impg_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "-s", "paf_ingest_check"])
    exe = os.path.join(ROOT, "impg_amd", "paf_ingest_check")
    for name in sorted(g.FIXTURES):
        for container in ("plain", "bgzf", "gzip"):
            paths = g.write(g.fixture(name), folder, "san_" + name, container)
            for piece, hash_bits, pool in ((16, 64, 64), (256, 1, 0), (0, 64, 0)):
                r = subprocess.run([exe, str(piece), str(hash_bits), str(pool)] + paths, capture_output=True, text=True)
                assert r.returncode == 0 and "ingest: 0 ok (%d records" % len(model(name)["records"]) in r.stdout, (name, r.stdout, r.stderr[-2000:])
    for kind in sorted(g.ERRORS):
        paths = g.write(g.error_file(kind), folder, "san_bad_" + kind)
        r = subprocess.run([exe, "256", "64", "0"] + paths, capture_output=True, text=True)
        assert r.returncode == 0 and "ingest: -1 Failed to parse PAF: " + g.ERRORS[kind] in r.stdout, (kind, r.stdout, r.stderr[-2000:])
