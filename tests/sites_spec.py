"""-sites on the checker side: the sparse read-out of the pileup, straight from the definition of DESIGN.md 4.17, and the lines
of the -sites file.  numpy and Python integers, no engine.  Builds on pile_spec (the table and the cut of a record's name) and
ext_spec (letters); restates neither.

cnt[p] is row p of the table as counts() returns it, in the order A C G T D I; L(p) the text's letter at p, upper-cased;
d(p) = A+C+G+T+D.  A read-out has a range [first, first + count), a mode and two thresholds, min_depth (1 to 2^31 - 1) and
min_pct (0 to 100).

  mode 0, NONZERO   row p is selected iff one of its six counters is not 0; bit k of its mask is set iff cnt[p][k] != 0.  The
                    thresholds and the letter play no part.
  mode 1, VARIANT   row p is selected iff L(p) is one of A,C,G,T, d(p) >= min_depth and its mask is not 0.  Bit k, k in 0..4
                    and not the column of L(p), is set iff cnt[k] > 0 and 100 * cnt[k] >= min_pct * d; bit 5 iff I > 0 and
                    100 * I >= min_pct * d.

The result is the selected rows in ascending p: pos (uint64, m), counts (uint32, m x 6), alleles (uint8, m: the mask).  Every sum
and product is a Python integer: no overflow."""
import numpy as np

import ext_spec
import map_spec
import pile_spec

NONZERO, VARIANT = 0, 1
COLUMNS = pile_spec.COLUMNS
_COL = {ord(c): k for k, c in enumerate("ACGT")}


def check_rule(mode: int, min_depth: int, min_pct: int) -> None:
    if mode not in (NONZERO, VARIANT):
        raise ValueError("mode %r" % (mode,))
    if not 0 <= min_pct <= 100:
        raise ValueError("min_pct %r" % (min_pct,))
    if mode == VARIANT and not 1 <= min_depth < 2 ** 31:
        raise ValueError("min_depth %r" % (min_depth,))


def row_mask(row, letter: int, mode: int = VARIANT, min_depth: int = 4, min_pct: int = 20) -> int:
    """The allele mask of one row (six counters) under the text's letter (a byte); 0: the row is not selected."""
    c = [int(v) for v in row]
    if mode == NONZERO:
        return sum(1 << k for k in range(6) if c[k] != 0)
    own = _COL.get(letter & 0xDF)
    if own is None:
        return 0
    d = c[0] + c[1] + c[2] + c[3] + c[4]
    if d < min_depth:
        return 0
    return sum(1 << k for k in range(6) if k != own and c[k] > 0 and 100 * c[k] >= min_pct * d)


def sites(table, text, mode: int = VARIANT, min_depth: int = 4, min_pct: int = 20, first: int = 0, count=None):
    """(pos, counts, alleles) of rows [first, first + count) of the table (n x 6) over the text (n letters)."""
    check_rule(mode, min_depth, min_pct)
    T = ext_spec._letters(text)
    n = len(T)
    assert table.shape == (n, 6)
    count = n - first if count is None else count
    assert 0 <= first <= n and 0 <= count <= n - first
    # (only a row with a non-zero counter can have a mask: the others are not looked at one by one)
    live = first + np.nonzero(np.asarray(table[first:first + count]).any(axis=1))[0]
    pos, masks = [], []
    for p in live:
        m = row_mask(table[p], T[p], mode, min_depth, min_pct)
        if m:
            pos.append(int(p))
            masks.append(m)
    counts = np.asarray(table)[pos].astype(np.uint32).reshape(len(pos), 6)
    return np.array(pos, dtype=np.uint64), counts, np.array(masks, dtype=np.uint8)


def calls(mask: int) -> bytes:
    """The set bits of a mask in column order, joined by commas: b"G", b"T,D"."""
    return b",".join(COLUMNS[k:k + 1].encode() for k in range(6) if (mask >> k) & 1)


def sites_file(table, ref, min_depth: int = 4, min_pct: int = 20) -> bytes:
    """The -sites file: a line per row that mode 1 selects, in reference order -- the nine columns of the -pile file (record name
    cut as pile_spec.pile_file cuts it, 1-based position local to the record, the reference letter in upper case, A, C, G, T, D,
    I) and a tenth, the calls.  Positions that belong to no record (the separators) are skipped; no '>' lines.  ref:
    hostlib.Loaded of the merged reference."""
    T = ext_spec._letters(ref.chars)
    pos, counts, alleles = sites(table, ref.chars, VARIANT, min_depth, min_pct)
    starts = ref.merged_start if ref.s.num > 1 else [0]
    out = []
    k = 0
    for r in range(len(starts)):
        name = map_spec.cut_name(ref.names[r])
        a = int(starts[r])
        b = a + int(ref.sizes[r])
        while k < len(pos) and int(pos[k]) < b:
            x = int(pos[k])
            if x >= a:
                out.append(b"%s\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % ((name, x - a + 1, bytes([T[x]]).upper()) +
                                                                          tuple(int(v) for v in counts[k]) + (calls(int(alleles[k])),)))
            k += 1
    return b"".join(out)
