"""write_partition_fasta (partition.rs:1630-1680, called from :498-508) restated in Python: what
`impg partition -o fasta --separate-files` writes into partition{N}.fasta.

1. FASTA exists only with separate files (main.rs:6366-6376, partition.rs:527-531): partition number N -- the number the BED
   route gives the same window under --separate-files -- goes to {folder}/partition{N}.fasta; a window that leaves no
   interval writes no file and takes no number; nothing is rehomed (that is the single BED file's, :637);
2. a file holds one record per output interval of its window, in the order of the lines of partition{N}.bed;
3. a record is ">{name}:{start}-{end}\\n" and bases [start, end) of the sequence, every byte upper-cased, in lines of 80,
   each line followed by '\\n' -- `chunks(80)` of nothing yields nothing (:1672-1676), so a record of NO bases is its header
   line alone: L + ceil(L / 80) body bytes for L > 0 and none for L = 0.  (`impg query -o fasta` prints an empty line
   there: step 6 of tests/fasta_ref.py);
4. partition intervals are forward: the "/rc" branch is unreachable, --reverse-complement changes nothing;
5. names print as the index has them; --original-sequence-coordinates plays no part;
6. an interval on a sequence the sequence files lack, or one that leaves its sequence, is an error raised before any byte
   of that window's text is written."""
from tests import fasta_ref


def body_len(n):
    return n + (n + 79) // 80


def record(name, seq, start, end):
    bases = fasta_ref.fetch(seq, start, end)
    return b">%s:%d-%d\n" % (name.encode(), start, end) + b"".join(bases[i:i + 80] + b"\n" for i in range(0, len(bases), 80))


def partition_text(rows, names, seqs):
    """rows: [(seq_id, start, end)] of one partition; names[id], seqs[id] -> the text of its file (bytes)"""
    return b"".join(record(names[s], seqs[s], a, b) for s, a, b in rows)
