"""-sv on the checker side: the junctions of the read mappings, straight from the definition of DESIGN.md 4.31.  Python integers,
no engine.  Builds on map_spec (the read_map tuples), aln_spec (the segments and their order), pile_spec (who contributes) and
events_spec (fold, is_acgt, the two rules of left-normalisation); restates none of them.

n is the merged text's length, T the text.  A read contributes iff pile_spec says so (strand != 0 and mapq >= min_mapq; under
-dedup the duplicate's record has strand 0).  Its segments come q descending (aln_spec.block_aln); taken in ascending order of the
scanned strand Q, every adjacent pair (a, b) is one junction:

  pe = a.ref_pos + a.ref_len   qe = a.query_pos + a.query_len   ps = b.ref_pos   qs = b.query_pos
  dr = ps - pe >= 0            dq = qs - qe >= 0                (aln_spec.anchors trims overlaps: asserted)
  A = Q[qe:qs]   B = T[pe:ps]   m = min(dr, dq)   L = |dr - dq|

Counted and never stored, looked at in this order: skipped[0] L == 0; skipped[3] m > 64; skipped[2] a row of B, or a compared
letter of A, is none of A,C,G,T; skipped[3] the best split has more than max_mis mismatches; skipped[1] no room in the table (never
here: the spec's table is a dict).

The best split, compared folded:
  deletion (dr > dq)    cost(t) = #{i < t: A[i] != B[i]} + #{t <= i < m: A[i] != B[L + i]}, t in 0..m; the smallest t of least
                        cost; rows [pe + t, pe + t + L) are deleted
  insertion (dq > dr)   cost(t) = #{i < t: B[i] != A[i]} + #{t <= i < m: B[i] != A[L + i]}; S = fold(A[t:t+L]) in front of pe + t
The compared letters of A are A[0:m] and A[|A|-m:]: all of A for a deletion.  The result is left-normalised by events_spec's two
rules, whatever its length.

The table maps (pos, kind, len) -- kind 0 a deletion, 1 an insertion; the inserted letters are not part of the key -- to
[fwd, rev], the observations from reads of strand 1 and 2, modulo 2^32.  The read-out of a range gives the keys with
first <= pos < first + count, fwd + rev >= min_count and len >= min_len, ascending in (pos, kind, len), as tuples
(pos, kind, len, fwd, rev)."""
import numpy as np

import events_spec as es
import ext_spec

MAX_SLOP = 64
DEFAULT_MAX_MIS = 3


def split_costs(A: bytes, B: bytes):
    """cost(t) for t in 0..m of the junction with read letters A and text rows B (not balanced)."""
    A, B = es.fold(A), es.fold(B)
    dq, dr = len(A), len(B)
    m, L = min(dr, dq), abs(dr - dq)
    if dr > dq:
        first = [A[i] != B[i] for i in range(m)]
        second = [A[i] != B[L + i] for i in range(m)]
    else:
        first = [B[i] != A[i] for i in range(m)]
        second = [B[i] != A[L + i] for i in range(m)]
    return [sum(first[:t]) + sum(second[t:]) for t in range(m + 1)]


def classify(T: bytes, Q: bytes, pe: int, qe: int, ps: int, qs: int, max_mis: int = DEFAULT_MAX_MIS, tie: str = "smallest",
             normalise: bool = True, slop: str = "both"):
    """("skip", k) or ("key", pos, kind, len) of one junction.  tie, normalise and slop are the definition at their defaults; the
    other values are the wrong rules that tests/test_sv_host.py shows to differ: tie="largest", normalise=False, slop="query" (the
    slop measured on the read's side alone)."""
    dr, dq = ps - pe, qs - qe
    assert dr >= 0 and dq >= 0 and ps < len(T) and qs <= len(Q), (pe, qe, ps, qs)
    A, B = Q[qe:qs], T[pe:ps]
    m, L = min(dr, dq), abs(dr - dq)
    if L == 0:
        return ("skip", 0)
    if (dq if slop == "query" else m) > MAX_SLOP:
        return ("skip", 3)
    compared = A[:m] + A[len(A) - m:] if m else b""
    if not all(es.is_acgt(c) for c in B) or not all(es.is_acgt(c) for c in compared):
        return ("skip", 2)
    costs = split_costs(A, B)
    least = min(costs)
    if least > max_mis:
        return ("skip", 3)
    t = costs.index(least) if tie == "smallest" else max(i for i, c in enumerate(costs) if c == least)
    if dr > dq:
        pos = es.normalise(T, pe + t, 0, L)[0] if normalise else pe + t
        return ("key", pos, 0, L)
    pos = es.normalise(T, pe + t, 1, L, es.fold(A[t:t + L]))[0] if normalise else pe + t
    return ("key", pos, 1, L)


def read_junctions(result, read, T: bytes, max_mis: int = DEFAULT_MAX_MIS, min_mapq: int = 0, **rule):
    """The classified junctions of one read_map tuple, in ascending order of the scanned strand; None when the read does not
    contribute."""
    strand, mapq, _, _, segl = result
    if strand == 0 or mapq < min_mapq:
        return None
    rec = np.frombuffer(ext_spec._letters(read), dtype=np.uint8)
    Q = bytes(ext_spec.revcomp(rec)) if strand == 2 else bytes(rec)
    asc = list(reversed(segl))
    assert all(int(asc[i][1]) < int(asc[i + 1][1]) for i in range(len(asc) - 1)), "segments come q descending"
    out = []
    for a, b in zip(asc, asc[1:]):
        out.append(classify(T, Q, int(a[0]) + int(a[2]), int(a[1]) + int(a[3]), int(b[0]), int(b[1]), max_mis, **rule))
    return out


class Table:
    def __init__(self, text, max_mis: int = DEFAULT_MAX_MIS):
        self.T = ext_spec._letters(text)
        self.max_mis = max_mis
        self.keys = {}
        self.skipped = [0, 0, 0, 0]
        self.observed = 0  # junctions looked at, stored or not

    def _count(self, key, fwd, rev):
        c = self.keys.setdefault(key, [0, 0])
        c[0] = (c[0] + fwd) % 2 ** 32
        c[1] = (c[1] + rev) % 2 ** 32

    def observe(self, pos: int, kind: int, k: int, fwd: int = 0, rev: int = 0) -> None:
        """One junction record with its counts, as slamem_pileup_add_junctions_* takes it: a deletion is validated and normalised, an
        insertion stays where it is given (its letters are not in the record)."""
        if fwd + rev == 0:
            return
        n = len(self.T)
        bad = kind not in (0, 1) or k < 1 or pos >= n
        if not bad and kind == 0:
            bad = pos + k > n or not all(es.is_acgt(c) for c in self.T[pos:pos + k])
        if bad:
            self.skipped[2] += fwd + rev
            return
        self._count((es.normalise(self.T, pos, 0, k)[0] if kind == 0 else pos, kind, k), fwd, rev)

    def add_read(self, result, read, min_mapq: int = 0) -> bool:
        got = read_junctions(result, read, self.T, self.max_mis, min_mapq)
        if got is None:
            return False
        fwd, rev = (1, 0) if result[0] == 1 else (0, 1)
        for j in got:
            self.observed += 1
            if j[0] == "skip":
                self.skipped[j[1]] += 1
            else:
                self._count(j[1:], fwd, rev)
        return True

    def add_batch(self, results, queries, offsets, min_mapq: int = 0):
        q = np.frombuffer(queries, dtype=np.uint8) if isinstance(queries, (bytes, bytearray)) else np.asarray(queries, dtype=np.uint8)
        off = np.asarray(offsets, dtype=np.int64)
        assert len(results) == len(off) - 1
        for r, res in enumerate(results):
            self.add_read(res, q[off[r]:off[r + 1]], min_mapq)
        return self

    def junctions(self, first: int = 0, count=None, min_count: int = 1, min_len: int = 1):
        n = len(self.T)
        count = n - first if count is None else count
        assert 0 <= first <= n and 0 <= count <= n - first and min_count >= 1
        return sorted((p, kind, k, c[0], c[1]) for (p, kind, k), c in self.keys.items()
                      if first <= p < first + count and c[0] + c[1] >= min_count and k >= min_len)


def junctions(results, queries, offsets, text, max_mis: int = DEFAULT_MAX_MIS, min_mapq: int = 0):
    """(junctions, skipped) of a batch: results is a read_map tuple per read (map_spec.filter_reads)."""
    t = Table(text, max_mis).add_batch(results, queries, offsets, min_mapq)
    return t.junctions(), list(t.skipped)


# ---- the -vcf -sv file ---------------------------------------------------------------------------------------------------------

VCF_HEADER_SV = (b'##ALT=<ID=DEL,Description="Deletion of the rows between two segments of a read">\n'
                 b'##ALT=<ID=INS,Description="Insertion of the letters between two segments of a read">\n'
                 b'##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of the junction: DEL or INS">\n'
                 b'##INFO=<ID=END,Number=1,Type=Integer,Description="Last deleted position; POS for an insertion">\n'
                 b'##INFO=<ID=SVLEN,Number=1,Type=Integer,Description="Inserted letters, or the deleted positions as a negative number">\n')
COLUMNS = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def vcf_header(ref) -> bytes:
    """events_spec's header with the ##ALT and ##INFO lines of the junctions in front of the column line."""
    head = es.vcf_header(ref)
    assert head.endswith(COLUMNS)
    return head[:-len(COLUMNS)] + VCF_HEADER_SV + COLUMNS


def junction_line(T: bytes, table, j, name: bytes, a: int, mdep: int, mpct: int):
    """(POS, line) of one junction of the record that starts at a; None when it lies at the record's first row (no anchor) or is
    not called.  The anchor is row pos - 1, x its 1-based position in the record; the call rule is events_spec's."""
    pos, kind, L, fwd, rev = j
    if pos <= a:
        return None
    x = pos - a
    d = int(sum(int(v) for v in table[pos - 1][:5]))
    if d < mdep or 100 * (fwd + rev) < mpct * d:
        return None
    ref_letter = bytes([T[pos - 1]]).upper()
    if kind == 0:
        info = b"SVTYPE=DEL;END=%d;SVLEN=-%d" % (x + L, L)
        alt = b"<DEL>"
    else:
        info = b"SVTYPE=INS;END=%d;SVLEN=%d" % (x, L)
        alt = b"<INS>"
    return x, b"%s\t%d\t.\t%s\t%s\t.\t.\t%s;DP=%d;AO=%d;SF=%d;SR=%d\n" % (name, x, ref_letter, alt, info, d, fwd + rev, fwd, rev)


def vcf_file(table, events, junctions, ref, mdep: int = 4, mpct: int = 20, min_len: int = 32) -> bytes:
    """The -vcf -sv file of a pileup table (n x 6), its events (events_spec tuples, the whole read-out) and its junctions (the whole
    read-out; those with len >= min_len are written -- the command line's -svmin, default maxed + 1): events_spec.vcf_file's lines
    and, at one POS behind the SNVs and the events, the called junctions in (pos, kind, len) order.  ref: hostlib.Loaded."""
    import map_spec
    import sites_spec
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
                                  (name, x - a + 1, bytes([T[x]]).upper(), es.ACGT[k:k + 1], d, int(counts[i][k]))))
        for ev in events:
            if a <= ev[0] < a + size:
                got = es.event_line(T, table, ev, name, a, size, mdep, mpct)
                if got is not None:
                    lines.append(((got[0], 1, len(lines)), got[1]))
        for j in sorted(junctions):
            if a <= j[0] < a + size and j[2] >= min_len:
                got = junction_line(T, table, j, name, a, mdep, mpct)
                if got is not None:
                    lines.append(((got[0], 2, len(lines)), got[1]))
        out.extend(line for _, line in sorted(lines, key=lambda t: t[0]))
    return b"".join(out)


# ---- the arrays of the C ABI ---------------------------------------------------------------------------------------------------

JUNCTION_DTYPE = np.dtype([("pos", "<u8"), ("len", "<u4"), ("fwd", "<u4"), ("rev", "<u4"), ("kind", "u1"), ("pad", "u1", (3,))])


def to_records(js) -> np.ndarray:
    out = np.zeros(len(js), dtype=JUNCTION_DTYPE)
    for i, (p, kind, k, fwd, rev) in enumerate(js):
        out[i]["pos"], out[i]["kind"], out[i]["len"], out[i]["fwd"], out[i]["rev"] = p, kind, k, fwd, rev
    return out


def from_records(arr):
    return [(int(e["pos"]), int(e["kind"]), int(e["len"]), int(e["fwd"]), int(e["rev"])) for e in arr]
