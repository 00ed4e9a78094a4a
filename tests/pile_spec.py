"""-pile on the checker side: the per-base pileup of -paf's mappings, straight from the definition of DESIGN.md 4.16, and the
lines of the -pile file.  Builds on map_spec (a read_map tuple per read), aln_spec (the segments and their operations) and
ext_spec (letters, reverse complement); restates none of them.

n is the merged text's length; the table has n rows of six counters in the order A, C, G, T, D, I.  A read contributes iff its
strand != 0 and its mapq >= min_mapq; then each of its segments (p, q, ref_len, query_len, edits, operations) is walked once, left
to right, p from ref_pos, q from query_pos in the scanned strand Q (the read as given, or on strand 2 its reverse complement, as
map_spec.read_map forms it):

  = / X of k   k times: Q[q] upper-cased, if one of A,C,G,T, counts in its column at row p; any other letter nowhere; p, q += 1
  D of k       column D of rows p .. p+k-1; p += k
  I of k       column I of row p, once (dropped when p == n); q += k

Python integers / int64: no overflow."""
import numpy as np

import ext_spec
import map_spec

COLUMNS = "ACGTDI"
_COL = {ord(c): k for k, c in enumerate("ACGT")}


def empty(n: int) -> np.ndarray:
    return np.zeros((n, 6), dtype=np.int64)


def add_read(table: np.ndarray, result, read, min_mapq: int = 0) -> bool:
    """Adds one read (a map_spec.read_map tuple and its letters as given) to the table; True when it contributed."""
    strand, mapq, _, _, segl = result
    if strand == 0 or mapq < min_mapq:
        return False
    n = table.shape[0]
    rec = np.frombuffer(ext_spec._letters(read), dtype=np.uint8)
    Q = bytes(ext_spec.revcomp(rec)) if strand == 2 else bytes(rec)
    for (p, q, _rlen, _qlen, _ed, rl) in segl:
        p, q = int(p), int(q)
        for c, k in rl:
            k = int(k)
            if c in "=X":
                for _ in range(k):
                    col = _COL.get(Q[q] & 0xDF)
                    if col is not None:
                        table[p, col] += 1
                    p += 1
                    q += 1
            elif c == "D":
                table[p:p + k, 4] += 1
                p += k
            elif c == "I":
                if p < n:
                    table[p, 5] += 1
                q += k
            else:
                raise ValueError("operation %r" % c)
    return True


def pile(results, queries, offsets, n: int, min_mapq: int = 0, table=None) -> np.ndarray:
    """The table of a batch: results is a read_map tuple per read (map_spec.filter_reads / golden_map)."""
    table = empty(n) if table is None else table
    q = np.frombuffer(queries, dtype=np.uint8) if isinstance(queries, (bytes, bytearray)) else np.asarray(queries, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.int64)
    assert len(results) == len(off) - 1
    for r, res in enumerate(results):
        add_read(table, res, q[off[r]:off[r + 1]], min_mapq)
    return table


def contributing(results, min_mapq: int = 0) -> int:
    return sum(1 for r in results if r[0] != 0 and r[1] >= min_mapq)


def depth(table: np.ndarray) -> np.ndarray:
    return table[:, :5].sum(axis=1)


def pile_file(table, ref) -> bytes:
    """The -pile file: a line per merged position with a non-zero counter, in reference order -- record name (cut at the first
    blank or tab), 1-based position local to the record, the reference letter in upper case, then A, C, G, T, D, I.  Positions
    that belong to no record (the separators) are skipped.  ref: hostlib.Loaded of the merged reference."""
    T = ext_spec._letters(ref.chars)
    starts = ref.merged_start if ref.s.num > 1 else [0]
    out = []
    for r in range(len(starts)):
        name = map_spec.cut_name(ref.names[r])
        a = int(starts[r])
        for x in range(a, a + int(ref.sizes[r])):
            row = table[x]
            if row.any():
                out.append(b"%s\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % ((name, x - a + 1, bytes([T[x]]).upper()) + tuple(int(v) for v in row)))
    return b"".join(out)
