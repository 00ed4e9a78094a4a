"""-vcf on the checker side: the indel events of the read mappings, straight from the definition of DESIGN.md 4.18, and the lines
of the -vcf file.  Python integers, no engine.  Builds on pile_spec (who contributes, the walk of a segment), sites_spec (the SNV
rows), map_spec (the cut of a record's name) and ext_spec (letters, reverse complement); restates none of them.

n is the merged text's length, T the text, fold upper-casing.  A read contributes iff pile_spec says so (strand != 0 and
mapq >= min_mapq); its segments are walked as pile_spec walks them, p in the text, q in the scanned strand Q:

  I of k at (p, q)   an insertion of S = fold(Q[q : q+k]) in front of row p
  D of k at p        a deletion of rows [p, p+k)
  = and X            no event

Observations that are counted and not stored: skipped[0] an insertion of more than 31 letters; skipped[2] an insertion at p == n or
with a letter outside A,C,G,T, a deletion with k > 127, with p + k > n or over a row that is not A,C,G,T; skipped[1] what a table
had no room for (never here: the spec's table is a dict).  The length of an insertion is looked at first.

Left-normalisation, a function of T and the event alone:
  deletion    while p > 0, T[p-1] is one of A,C,G,T and fold(T[p-1]) == fold(T[p+k-1]): p -= 1
  insertion   while p > 0, T[p-1] is one of A,C,G,T and fold(T[p-1]) == S[k-1]: S = fold(T[p-1]) + S[:k-1], p -= 1

The table maps (pos, kind, len, S) -- kind 0 a deletion (S empty), 1 an insertion -- to [fwd, rev], the observations from reads of
strand 1 and 2.  The read-out of a range gives the keys with first <= pos < first + count and fwd + rev >= min_count in ascending
(pos, kind, len, S), S letter by letter with A < C < G < T, as tuples (pos, kind, len, S, fwd, rev)."""
import numpy as np

import ext_spec
import map_spec
import pile_spec
import sites_spec

MAX_INS, MAX_DEL = 31, 127
ACGT = b"ACGT"
_CODE = {c: k for k, c in enumerate(ACGT)}


def is_acgt(byte: int) -> bool:
    return (byte & 0xDF) in _CODE


def fold(b: bytes) -> bytes:
    return bytes(c & 0xDF for c in b)


def pack_letters(S: bytes) -> int:
    """key1 without its marker: letter i at bits 2 * (len - 1 - i)."""
    v = 0
    for c in S:
        v = (v << 2) | _CODE[c]
    return v


def unpack_letters(v: int, k: int) -> bytes:
    return bytes(ACGT[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


def normalise(T: bytes, pos: int, kind: int, k: int, S: bytes = b""):
    """The canonical (pos, S) of a valid event."""
    p = pos
    if kind == 0:
        while p > 0 and is_acgt(T[p - 1]) and (T[p - 1] & 0xDF) == (T[p + k - 1] & 0xDF):
            p -= 1
        return p, b""
    while p > 0 and is_acgt(T[p - 1]) and (T[p - 1] & 0xDF) == S[k - 1]:
        S = bytes([T[p - 1] & 0xDF]) + S[:k - 1]
        p -= 1
    return p, S


def which_skip(T: bytes, pos: int, kind: int, k: int, S: bytes = b""):
    """None for a valid observation, else the index of its skipped counter.  S: the folded letters as they stand in the read."""
    n = len(T)
    if kind == 1:
        if k > MAX_INS:
            return 0
        if k < 1 or pos >= n or len(S) != k or not all(c in _CODE for c in S):
            return 2
        return None
    if kind != 0 or k < 1 or k > MAX_DEL or pos >= n or pos + k > n or not all(is_acgt(c) for c in T[pos:pos + k]):
        return 2
    return None


class Table:
    def __init__(self, text):
        self.T = ext_spec._letters(text)
        self.keys = {}
        self.skipped = [0, 0, 0]

    def observe(self, pos: int, kind: int, k: int, S: bytes = b"", fwd: int = 0, rev: int = 0) -> None:
        """One event with its counts, given in any (not only the canonical) form."""
        if fwd + rev == 0:
            return
        w = which_skip(self.T, pos, kind, k, S)
        if w is not None:
            self.skipped[w] += fwd + rev
            return
        p, S = normalise(self.T, pos, kind, k, S)
        c = self.keys.setdefault((p, kind, k, S), [0, 0])
        c[0] = (c[0] + fwd) % 2 ** 32
        c[1] = (c[1] + rev) % 2 ** 32

    def add_read(self, result, read, min_mapq: int = 0) -> bool:
        strand, mapq, _, _, segl = result
        if strand == 0 or mapq < min_mapq:
            return False
        rec = np.frombuffer(ext_spec._letters(read), dtype=np.uint8)
        Q = bytes(ext_spec.revcomp(rec)) if strand == 2 else bytes(rec)
        fwd, rev = (1, 0) if strand == 1 else (0, 1)
        for (p, q, _rlen, _qlen, _ed, rl) in segl:
            p, q = int(p), int(q)
            for c, k in rl:
                k = int(k)
                if c in "=X":
                    p += k
                    q += k
                elif c == "D":
                    if k:
                        self.observe(p, 0, k, b"", fwd, rev)
                    p += k
                elif c == "I":
                    if k:
                        self.observe(p, 1, k, fold(Q[q:q + k]), fwd, rev)
                    q += k
                else:
                    raise ValueError("operation %r" % c)
        return True

    def add_batch(self, results, queries, offsets, min_mapq: int = 0):
        q = np.frombuffer(queries, dtype=np.uint8) if isinstance(queries, (bytes, bytearray)) else np.asarray(queries, dtype=np.uint8)
        off = np.asarray(offsets, dtype=np.int64)
        assert len(results) == len(off) - 1
        for r, res in enumerate(results):
            self.add_read(res, q[off[r]:off[r + 1]], min_mapq)
        return self

    def events(self, first: int = 0, count=None, min_count: int = 1):
        n = len(self.T)
        count = n - first if count is None else count
        assert 0 <= first <= n and 0 <= count <= n - first and min_count >= 1
        out = [(p, kind, k, S, c[0], c[1]) for (p, kind, k, S), c in self.keys.items()
               if first <= p < first + count and c[0] + c[1] >= min_count]
        return sorted(out, key=order_key)


def order_key(ev):
    """(pos, kind, len, S) with S letter by letter, A < C < G < T."""
    return ev[0], ev[1], ev[2], tuple(_CODE[c] for c in ev[3])


def events(results, queries, offsets, text, min_mapq: int = 0):
    """(events, skipped) of a batch: results is a read_map tuple per read (map_spec.filter_reads)."""
    t = Table(text).add_batch(results, queries, offsets, min_mapq)
    return t.events(), list(t.skipped)


VCF_HEADER_INFO = (b'##INFO=<ID=DP,Number=1,Type=Integer,Description="Depth A+C+G+T+D at the row (SNV) or at the anchor row (indel)">\n'
                   b'##INFO=<ID=AO,Number=1,Type=Integer,Description="Observations of the alternate allele">\n'
                   b'##INFO=<ID=SF,Number=1,Type=Integer,Description="Observations of the alternate allele on forward-strand reads">\n'
                   b'##INFO=<ID=SR,Number=1,Type=Integer,Description="Observations of the alternate allele on reverse-strand reads">\n')


def vcf_header(ref) -> bytes:
    out = [b"##fileformat=VCFv4.2\n"]
    for r in range(ref.s.num):
        out.append(b"##contig=<ID=%s,length=%d>\n" % (map_spec.cut_name(ref.names[r]), int(ref.sizes[r])))
    out.append(VCF_HEADER_INFO)
    out.append(b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
    return b"".join(out)


def event_line(T: bytes, table, ev, name: bytes, a: int, size: int, mdep: int, mpct: int):
    """(POS, line) of one event of the record that starts at a, or None when it is not called."""
    pos, kind, k, S, fwd, rev = ev
    x = pos - a
    anchor = pos - 1 if x > 0 else pos
    d = int(sum(int(v) for v in table[anchor][:5]))
    if d < mdep or 100 * (fwd + rev) < mpct * d:
        return None
    if kind == 0:
        if x > 0:
            POS, REF, ALT = x, T[pos - 1:pos + k], T[pos - 1:pos]
        else:
            if pos + k >= a + size:  # (the record ends with the deletion: no following base)
                return None
            POS, REF, ALT = 1, T[pos:pos + k + 1], T[pos + k:pos + k + 1]
    else:
        if x > 0:
            POS, REF, ALT = x, T[pos - 1:pos], T[pos - 1:pos] + S
        else:
            POS, REF, ALT = 1, T[pos:pos + 1], S + T[pos:pos + 1]
    return POS, b"%s\t%d\t.\t%s\t%s\t.\t.\tDP=%d;AO=%d;SF=%d;SR=%d\n" % (name, POS, REF.upper(), ALT.upper(), d, fwd + rev, fwd, rev)


def vcf_file(table, events, ref, mdep: int = 4, mpct: int = 20) -> bytes:
    """The -vcf file of a pileup table (n x 6, as counts() gives it) and its events (the read-out of the whole text with
    min_count 1): the header, then per record the SNVs of sites_spec.sites(VARIANT, mdep, mpct) -- a line per set bit 0..3 -- and
    the called events, sorted by POS; at one POS the SNVs first (ALT A < C < G < T), then the events in event order.  An event
    whose pos lies in no record (a separator) gives no line.  ref: hostlib.Loaded of the merged reference."""
    T = ext_spec._letters(ref.chars)
    pos, counts, alleles = sites_spec.sites(table, ref.chars, sites_spec.VARIANT, mdep, mpct)
    starts = ref.merged_start if ref.s.num > 1 else [0]
    out = [vcf_header(ref)]
    for r in range(len(starts)):
        name = map_spec.cut_name(ref.names[r])
        a, size = int(starts[r]), int(ref.sizes[r])
        lines = []
        for i in range(len(pos)):
            x = int(pos[i])
            if not a <= x < a + size:
                continue
            d = int(sum(int(v) for v in counts[i][:5]))
            for k in range(4):
                if (int(alleles[i]) >> k) & 1:
                    lines.append(((x - a + 1, 0, len(lines)), b"%s\t%d\t.\t%s\t%s\t.\t.\tDP=%d;AO=%d\n" %
                                  (name, x - a + 1, bytes([T[x]]).upper(), ACGT[k:k + 1], d, int(counts[i][k]))))
        for ev in events:
            if not a <= ev[0] < a + size:
                continue
            got = event_line(T, table, ev, name, a, size, mdep, mpct)
            if got is not None:
                lines.append(((got[0], 1, len(lines)), got[1]))
        out.extend(line for _, line in sorted(lines, key=lambda t: t[0]))
    return b"".join(out)


# ---- the arrays of the C ABI ---------------------------------------------------------------------------------------------------

EVENT_DTYPE = np.dtype([("pos", "<u8"), ("letters", "<u8"), ("fwd", "<u4"), ("rev", "<u4"), ("kind", "u1"), ("len", "u1"), ("pad", "u1", (6,))])


def to_records(evs) -> np.ndarray:
    """Event tuples -> the structured array of slamem_event."""
    out = np.zeros(len(evs), dtype=EVENT_DTYPE)
    for i, (p, kind, k, S, fwd, rev) in enumerate(evs):
        out[i]["pos"], out[i]["kind"], out[i]["len"], out[i]["fwd"], out[i]["rev"] = p, kind, k, fwd, rev
        out[i]["letters"] = pack_letters(S) if kind == 1 else 0
    return out


def from_records(arr):
    return [(int(e["pos"]), int(e["kind"]), int(e["len"]), unpack_letters(int(e["letters"]), int(e["len"])) if e["kind"] == 1 else b"",
             int(e["fwd"]), int(e["rev"])) for e in arr]
