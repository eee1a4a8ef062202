"""Builds impg_amd/sequence_ingest_check (the reader and the host twin of impg_gpu_index_load_sequences under
-fsanitize=address,undefined; a program of its own, no GPU) and runs it over the edge file in every container at several
piece sizes, in both store forms, and over the malformed files of tests/seq_ingest_gen.py.  Fails if any run does not
exit 0 or a sanitizer reports."""
import os
import pathlib
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import seq_ingest_gen as gen  # noqa: E402


def main():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "impg_amd", "csrc"), "-s", "sequence_ingest_check"])
    prog = os.path.join(ROOT, "impg_amd", "sequence_ingest_check")
    runs = 0
    with tempfile.TemporaryDirectory() as d:
        tmp = pathlib.Path(d)
        text, seqs = gen.edge_file()
        names, lens = ",".join(nm for nm, _ in seqs[1:]), ",".join(str(len(b)) for _, b in seqs[1:])
        jobs = []
        for kind, data in gen.containers(text).items():
            path = str(tmp / ("edge." + kind))
            with open(path, "wb") as f:
                f.write(data)
            jobs += [(piece, packed, names, lens, [path]) for piece in gen.PIECE_SIZES + [gen.DEFAULT_PIECE] for packed in (0, 1)]
        for key, (paths, nm, ln, _, _) in gen.malformed(tmp).items():
            jobs += [(piece, packed, ",".join(nm), ",".join(map(str, ln)), paths) for piece in (16, 32, 4096) for packed in (0, 1)]
        for piece, packed, nm, ln, paths in jobs:
            r = subprocess.run([prog, str(piece), str(packed), nm, ln] + paths, capture_output=True, text=True)
            if r.returncode != 0 or "ERROR" in r.stderr or "runtime error" in r.stderr:
                print(r.stdout, r.stderr)
                sys.exit("sequence_ingest_check failed on %r (piece %d, packed %d)" % (paths, piece, packed))
            runs += 1
    print("sequence_ingest_check: %d runs, all clean" % runs)


if __name__ == "__main__":
    main()
