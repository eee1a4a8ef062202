"""output_results_fasta (main.rs:12351-12415) restated in Python: what `impg query -o fasta` prints for one range's rows.

1. the rows are those BED gets (perform_query with store_cigar = false, self interval included);
2. merge_query_adjusted_intervals(results, d, merge_strands = false) ALONE -- no merge_adjusted_intervals_gap_2d; with
   d < 0 nothing merges and the rows keep their emission order;
3. a merged row reads (first, last, '+') if first <= last, else (last, first, '-');
4. the bases are [start, end) of the sequence, every byte upper-cased (faidx.rs:162-188);
5. on '-' with --reverse-complement they are reversed and A/T/C/G/N map to T/A/G/C/N, every other byte kept
   (graph.rs:814-828);
6. ">{name}:{start}-{end}{'/rc' if '-' and --reverse-complement}\\n", the bases in lines of 80 and one '\\n' behind the last
   line: L + ceil(L / 80) bytes for L > 0 bases, the single '\\n' for L = 0;
7. --original-sequence-coordinates does not touch the text;  8. records appear in merged order, range after range."""
import numpy as np

from oracle import oracle as o

ALPHABET = b"ACGTNacgtnRYKM"
_COMPLEMENT = bytes.maketrans(b"ATCGN", b"TAGCN")


def random_sequence(rng, n):
    return bytes(np.frombuffer(ALPHABET, dtype=np.uint8)[rng.integers(0, len(ALPHABET), size=n)])


def fetch(seq, start, end):
    return seq[start:end].upper()


def reverse_complement(seq):
    return seq[::-1].translate(_COMPLEMENT)


def wrap(seq):
    """the body of a record: lines of 80, one newline behind the last; an empty line for no bases"""
    return b"\n".join(seq[i:i + 80] for i in range(0, len(seq), 80)) + b"\n"


def body_len(n):
    return n + (n + 79) // 80 if n else 1


def record(name, seq, first, last, rc):
    start, end, strand = (first, last, "+") if first <= last else (last, first, "-")
    flip = strand == "-" and rc
    bases = fetch(seq, start, end)
    if flip:
        bases = reverse_complement(bases)
    return b">%s:%d-%d%s\n" % (name.encode(), start, end, b"/rc" if flip else b"") + wrap(bases)


def fasta_range(rows, merge_distance, rc, name_of, seq_of):
    """rows: INTERVAL_DTYPE of one range in emission order -> the range's text (bytes)"""
    merged = o.merge_query(rows, merge_distance, merge_strands=False)
    return b"".join(record(name_of(int(r["query_id"])), seq_of(int(r["query_id"])), int(r["q_first"]), int(r["q_last"]), rc) for r in merged)
