"""-wq on the checker side: the quality sums of the pileup and the weighted genotypes, letter by letter from the
definition.  Python integers, no engine.  Builds on pile_spec and lowq_spec (the walk of a read's segments, the mask's bit of a
letter), ext_spec (letters, reverse complement) and gt_spec (the call of a row's scores, the order of the genotypes, the record);
extends gt_spec by import and restates none of them.

A letter's quality is qv(b) = 0 if b < off else min(b - off, 93) of its quality byte b, off the Phred offset.  Letter x of the
scanned strand of a strand-2 read has the byte at len - 1 - x.  Q is a table of the pileup's shape; every read that contributes to
the pileup contributes to Q, and wherever pile_spec's (with a mask lowq_spec's) walk adds 1 to column A, C, G or T of a row, Q gets
qv of that letter in the same column of the same row.  D and I add nothing.

The weighted genotype of a row is gt_spec's with one change: the letters i that a genotype does not hold cost
c[i] * E + 1000 * Qs[i] in the place of c[i] * E, Qs the row of Q."""
import numpy as np

import ext_spec
import gt_spec
import lowq_spec
import pile_spec

_COL = {ord(c): k for k, c in enumerate("ACGT")}
WQ_COSTS = (0, 3010, 4771)  # M, H = round(10000 log10 2), E = round(10000 log10 3)
QMAX = 93


def qv(b: int, off: int = 33) -> int:
    return 0 if b < off else min(b - off, QMAX)


def params(ploidy: int = 2, het_q: int = 30, min_depth: int = 4, min_qual: int = 20, costs=WQ_COSTS):
    """gt_spec's parameter tuple with -wq's costs."""
    M, H, E = costs
    return gt_spec.check_params((ploidy, M, H, E, 1000 * het_q, min_depth, min_qual))


# ---- the accumulator -----------------------------------------------------------------------------------------------------------

def add_read(table: np.ndarray, result, read, quals, low=None, min_mapq: int = 0, off: int = 33) -> bool:
    """Adds the qualities of one read (a map_spec.read_map tuple, its letters and its quality bytes as given, low[i] 0/1 per letter
    or None) to the table; True when it contributed."""
    strand, mapq, _, _, segl = result
    if strand == 0 or mapq < min_mapq:
        return False
    n = table.shape[0]
    rec = np.frombuffer(ext_spec._letters(read), dtype=np.uint8)
    L = len(rec)
    assert len(quals) == L and (low is None or len(low) == L)
    Q = bytes(ext_spec.revcomp(rec)) if strand == 2 else bytes(rec)
    for (p, q, _rlen, _qlen, _ed, rl) in segl:
        p, q = int(p), int(q)
        for c, k in rl:
            k = int(k)
            if c in "=X":
                for _ in range(k):
                    given = L - 1 - q if strand == 2 else q
                    col = _COL.get(Q[q] & 0xDF)
                    if col is not None and p < n and not (low is not None and low[given]):
                        table[p, col] += qv(int(quals[given]), off)
                    p += 1
                    q += 1
            elif c == "D":
                p += k
            elif c == "I":
                q += k
            else:
                raise ValueError("operation %r" % c)
    return True


def pile(results, queries, offsets, quals, n: int, mask=None, min_mapq: int = 0, off: int = 33, table=None) -> np.ndarray:
    """Q of a batch: quals is a byte per letter, indexed as queries; mask the low-quality words of lowq_spec or None."""
    table = pile_spec.empty(n) if table is None else table
    q = np.frombuffer(queries, dtype=np.uint8) if isinstance(queries, (bytes, bytearray)) else np.asarray(queries, dtype=np.uint8)
    v = np.frombuffer(quals, dtype=np.uint8) if isinstance(quals, (bytes, bytearray)) else np.asarray(quals, dtype=np.uint8)
    o = np.asarray(offsets, dtype=np.int64)
    assert len(results) == len(o) - 1 and len(v) >= int(o[-1])
    for r, res in enumerate(results):
        a, b = int(o[r]), int(o[r + 1])
        low = None if mask is None else [lowq_spec.bit(mask, j) for j in range(a, b)]
        add_read(table, res, q[a:b], v[a:b], low, min_mapq, off)
    return table


# ---- the weighted genotypes ----------------------------------------------------------------------------------------------------

def snv(row, qs, r: int, p):
    """gt_spec.snv with the quality sums qs[0..3] of the row."""
    ploidy, M, H, E, hp, _min_depth, min_qual = p
    c = [int(v) for v in row[:4]]
    w = [int(v) for v in qs[:4]]
    assert all(0 <= v < 2 ** 32 for v in c + w)
    # the bound of DESIGN.md 4.24 with the new term: four columns of less than 2^32 at a cost of at most 2^20 each, and
    # 1000 * 2^32 < 2^42 per column on top
    assert sum(c) * max(M, H, E) + 1000 * sum(w) + 2 * hp < 2 ** 56
    if ploidy == 2:
        pairs = [(j, k) for k in range(4) for j in range(k + 1)]
        L = [sum(c[i] * ((M if i == j else E) if j == k else (H if i in (j, k) else E)) + (0 if i in (j, k) else 1000 * w[i]) for i in range(4))
             for j, k in pairs]
        S = [L[g] + hp * len({j, k} - {r}) for g, (j, k) in enumerate(pairs)]
        rr = gt_spec.genotype_index(r, r)
    else:
        pairs = [(i, i) for i in range(4)]
        L = [c[i] * M + sum(c[j] * E + 1000 * w[j] for j in range(4) if j != i) for i in range(4)]
        S = [L[i] + (hp if i != r else 0) for i in range(4)]
        rr = r
    best, qual, gq, pl, q64 = gt_spec._call(L, S, rr)
    a, b = pairs[best]
    return (qual, gq, a, b, ploidy, r, pl), best != rr and q64 >= 1000 * min_qual


def genotypes(table, qtable, text, p, first: int = 0, count=None):
    """(pos uint64 (m,), counts uint32 (m, 6), gts GENOTYPE_DTYPE (m,), qsums uint32 (m, 4)) of the selected rows of
    [first, first + count), in ascending position; selection as in gt_spec.genotypes."""
    p = gt_spec.check_params(p)
    T = ext_spec._letters(text)
    n = len(T)
    assert table.shape == (n, 6) and qtable.shape == (n, 6)
    count = n - first if count is None else count
    assert 0 <= first <= n and 0 <= count <= n - first
    # (a row whose A C G T counts are all 0 has, with Q <= 93 * counts, every L equal to 0: rr wins the tie)
    live = first + np.nonzero((np.asarray(table[first:first + count])[:, :4] != 0).any(axis=1)
                              | (np.asarray(qtable[first:first + count])[:, :4] != 0).any(axis=1))[0]
    pos, gts = [], []
    for x in live:
        r = _COL.get(T[x] & 0xDF)
        row = [int(v) for v in table[x]]
        if r is None or sum(row[:5]) < p[5]:
            continue
        g, variant = snv(row, qtable[x], r, p)
        if variant:
            pos.append(int(x))
            gts.append(g)
    counts = np.asarray(table)[pos].astype(np.uint32).reshape(len(pos), 6)
    qsums = np.asarray(qtable)[pos][:, :4].astype(np.uint32).reshape(len(pos), 4)
    return np.array(pos, dtype=np.uint64), counts, gt_spec.to_records(gts), qsums


# ---- the file ------------------------------------------------------------------------------------------------------------------

HEADER_ADQ = (b'##FORMAT=<ID=ADQ,Number=R,Type=Integer,Description="Sum of the base qualities of the observations of the reference and of '
              b'each alternate allele">\n')


def vcf_header(ref, sb: bool = False, fs=None) -> bytes:
    """gt_spec's header (sb: sb_spec's) with ADQ behind its FORMAT lines."""
    import sb_spec
    base = sb_spec.vcf_header(ref, fs) if sb else gt_spec.vcf_header(ref)
    at = base.index(b"#CHROM")
    return base[:at] + HEADER_ADQ + base[at:]


def decorate(line: bytes, adq) -> bytes:
    """A line of the file without -wq with :ADQ behind FORMAT and the sums (None: a dot, an indel line) behind the sample."""
    cols = line[:-1].split(b"\t")
    assert len(cols) == 10
    cols[8] += b":ADQ"
    cols[9] += b":" + (b"." if adq is None else b",".join(b"%d" % v for v in adq))
    return b"\t".join(cols) + b"\n"


def vcf_file(table, qtable, events, ref, p, ftable=None, fs=None, err_q: int = 20) -> bytes:
    """The -vcf -gt -wq file (ftable: with -sb, fs the N of -fs N) of a pileup table, its quality sums and its events.  The rows are
    called by the weighted read-out with p (whose costs are -wq's); the events by gt_spec with the costs of -err, and the rest of p.
    An SNV line is gt_spec's (sb_spec's) of the row and its genotype with ADQ = the quality sums of the reference and the ALT
    letters, in AD's order; an indel line gets a dot."""
    import map_spec
    import sb_spec
    p = gt_spec.check_params(p)
    pe = gt_spec.check_params((p[0],) + gt_spec.gt_costs(err_q) + p[4:])
    T = ext_spec._letters(ref.chars)
    pos, counts, gts, qsums = genotypes(table, qtable, ref.chars, p)
    gl = gt_spec.from_records(gts)
    starts = ref.merged_start if ref.s.num > 1 else [0]
    sb = ftable is not None
    out = [vcf_header(ref, sb, fs)]
    for r in range(len(starts)):
        name = map_spec.cut_name(ref.names[r])
        a, size = int(starts[r]), int(ref.sizes[r])
        lines = []
        for i in range(len(pos)):
            x = int(pos[i])
            if a <= x < a + size:
                g = gl[i]
                alts = sorted({g[2], g[3]} - {g[5]})
                line = gt_spec.snv_line(name, x - a + 1, T[x], counts[i], g)
                if sb:
                    line = sb_spec.decorate(line, sb_spec.snv_table(counts[i], ftable[x], g[5], alts), fs)
                lines.append(((x - a + 1, 0, len(lines)), decorate(line, [int(qsums[i][k]) for k in [g[5]] + alts])))
        mine = [ev for ev in events if a <= ev[0] < a + size]
        anchors = [ev[0] - 1 if ev[0] > a else ev[0] for ev in mine]
        eg, called = gt_spec.genotype_events(mine, [table[x] for x in anchors], pe)
        for ev, g, c, x in zip(mine, gt_spec.from_records(eg), called, anchors):
            got = gt_spec.event_line(T, table, ev, g, int(c), name, a, size)
            if got is not None:
                line = got[1]
                if sb:
                    line = sb_spec.decorate(line, sb_spec.event_table(table[x], ftable[x], int(ev[4]), int(ev[5])), fs)
                lines.append(((got[0], 1, len(lines)), decorate(line, None)))
        out.extend(line for _, line in sorted(lines, key=lambda k: k[0]))
    return b"".join(out)
