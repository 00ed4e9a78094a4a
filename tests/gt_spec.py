"""-gt on the checker side: the genotypes of the pileup's rows and of its indel events, straight from the definition of DESIGN.md
4.24, and the lines of the -vcf -gt file.  Python integers, no engine.  Builds on sites_spec (the letter's column), events_spec
(the VCF header's INFO lines, the order of the events, an event's REF and ALT) and map_spec (the cut of a record's name).

Scores are in milli-Phred.  The parameters are (ploidy, M, H, E, hp, min_depth, min_qual): ploidy 1 or 2; M, H, E the cost of one
observed letter under a genotype that is homozygous for it, heterozygous with it, or does not hold it; hp the prior cost per
non-reference allele; min_depth as in sites_spec; min_qual in Phred, 0 to 999.  gt_costs(q) gives (M, H, E) for a constant error
rate of Phred q.

  SNV rows   c[0..3] the A C G T columns of the row, r the column of the text's letter, d = A+C+G+T+D.  Ploidy 2: the ten genotypes
             (j, k), j <= k, at index g = k (k + 1) / 2 + j; L_g = sum_i c[i] w(i, g), w = M when i == j == k, H when j != k and i
             is one of them, else E.  Ploidy 1: the four genotypes i, L_i = c[i] M + (the others) E.  S_g = L_g + hp * (distinct
             letters of g that are not r).  Best: the smallest S; on a tie the homozygous-reference genotype, then the smallest g.
             qual = S_rr - S_best, gq = min over g != best of S_g - S_best, pl[g] = L_g - min L, each saturating at 2^32 - 1.
             Selected iff the letter is one of A,C,G,T, d >= min_depth, best is not rr and qual >= 1000 * min_qual.
  events     ao = fwd + rev, d the anchor row's depth, ro = d - ao (0 when ao is larger); L_00 = ro M + ao E, L_01 = (ro + ao) H
             (ploidy 2 only), L_11 = ao M + ro E; priors 0, hp, hp; the rest as above, `called` in the place of selected.

A genotype is the tuple (qual, gq, a, b, ploidy, ref, pl) with pl a list of ten; GENOTYPE_DTYPE is its 56 bytes."""
import math

import numpy as np

import events_spec
import ext_spec
import map_spec
import sites_spec

SAT = 2 ** 32 - 1
MAX_COST = 2 ** 20
GENOTYPE_DTYPE = np.dtype([("qual", "<u4"), ("gq", "<u4"), ("a", "u1"), ("b", "u1"), ("ploidy", "u1"), ("ref", "u1"), ("pl", "<u4", (10,)),
                           ("pad", "u1", (4,))])
_COL = {ord(c): k for k, c in enumerate("ACGT")}
ACGT = b"ACGT"


def gt_costs(q: int):
    """(M, H, E) of a constant error rate e = 10^(-q/10), q in 1..93, rounded half up."""
    if not 1 <= q <= 93:
        raise ValueError("q %r" % (q,))
    e = math.pow(10.0, -float(q) / 10.0)
    hom = 1.0 - e
    het = hom / 2.0 + e / 6.0
    third = e / 3.0
    return tuple(int(math.floor(-10000.0 * math.log10(x) + 0.5)) for x in (hom, het, third))


def params(ploidy: int = 2, err_q: int = 20, het_q: int = 30, min_depth: int = 4, min_qual: int = 20):
    """The parameter tuple (ploidy, M, H, E, hp, min_depth, min_qual) of the public interface's arguments."""
    M, H, E = gt_costs(err_q)
    return check_params((ploidy, M, H, E, 1000 * het_q, min_depth, min_qual))


def check_params(p):
    ploidy, M, H, E, hp, min_depth, min_qual = p
    if ploidy not in (1, 2):
        raise ValueError("ploidy %r" % (ploidy,))
    if not (0 <= M <= MAX_COST and 1 <= H <= MAX_COST and 1 <= E <= MAX_COST and 0 <= hp <= MAX_COST):
        raise ValueError("costs %r" % ((M, H, E, hp),))
    if not 1 <= min_depth < 2 ** 31:
        raise ValueError("min_depth %r" % (min_depth,))
    if not 0 <= min_qual <= 999:
        raise ValueError("min_qual %r" % (min_qual,))
    return tuple(int(v) for v in p)


def _call(L, S, rr):
    """(best, qual, gq, pl) of likelihoods L and scores S, rr the homozygous-reference genotype."""
    assert all(0 <= v < 2 ** 64 for v in L + S)  # (the device's arithmetic is unsigned 64-bit)
    sb = min(S)
    best = rr if S[rr] == sb else S.index(sb)
    gq = min(S[g] - sb for g in range(len(S)) if g != best)
    ml = min(L)
    return best, min(S[rr] - sb, SAT), min(gq, SAT), [min(v - ml, SAT) for v in L] + [0] * (10 - len(L)), S[rr] - sb


def genotype_index(j: int, k: int) -> int:
    return k * (k + 1) // 2 + j


def snv(row, r: int, p):
    """(genotype, variant): the genotype of a row's A C G T columns under the reference column r, and whether its best genotype
    is another than rr with qual >= 1000 * min_qual (depth and letter are the caller's)."""
    ploidy, M, H, E, hp, _min_depth, min_qual = p
    c = [int(v) for v in row[:4]]
    if all(v < 2 ** 31 for v in c) and E <= 97771:
        assert sum(c) * max(M, H, E) + 2 * hp < 2 ** 50  # (the bound of DESIGN.md 4.24)
    if ploidy == 2:
        pairs = [(j, k) for k in range(4) for j in range(k + 1)]
        assert [genotype_index(j, k) for j, k in pairs] == list(range(10))
        L = [sum(c[i] * ((M if i == j else E) if j == k else (H if i in (j, k) else E)) for i in range(4)) for j, k in pairs]
        S = [L[g] + hp * len({j, k} - {r}) for g, (j, k) in enumerate(pairs)]
        rr = genotype_index(r, r)
    else:
        pairs = [(i, i) for i in range(4)]
        L = [c[i] * M + (sum(c) - c[i]) * E for i in range(4)]
        S = [L[i] + (hp if i != r else 0) for i in range(4)]
        rr = r
    best, qual, gq, pl, q64 = _call(L, S, rr)
    a, b = pairs[best]
    return (qual, gq, a, b, ploidy, r, pl), best != rr and q64 >= 1000 * min_qual


def event(ao: int, d: int, p):
    """(genotype, called) of an event seen ao times at an anchor row of depth d."""
    ploidy, M, H, E, hp, min_depth, min_qual = p
    ro = d - ao if d > ao else 0
    l00, l01, l11 = ro * M + ao * E, (ro + ao) * H, ao * M + ro * E
    if ploidy == 2:
        L, S, pairs = [l00, l01, l11], [l00, l01 + hp, l11 + hp], [(0, 0), (0, 1), (1, 1)]
    else:
        L, S, pairs = [l00, l11], [l00, l11 + hp], [(0, 0), (1, 1)]
    best, qual, gq, pl, q64 = _call(L, S, 0)
    a, b = pairs[best]
    return (qual, gq, a, b, ploidy, 0, pl), d >= min_depth and best != 0 and q64 >= 1000 * min_qual


def to_records(gts) -> np.ndarray:
    out = np.zeros(len(gts), dtype=GENOTYPE_DTYPE)
    for i, (qual, gq, a, b, ploidy, ref, pl) in enumerate(gts):
        out[i]["qual"], out[i]["gq"], out[i]["a"], out[i]["b"], out[i]["ploidy"], out[i]["ref"] = qual, gq, a, b, ploidy, ref
        out[i]["pl"] = pl
    return out


def from_records(arr):
    return [(int(g["qual"]), int(g["gq"]), int(g["a"]), int(g["b"]), int(g["ploidy"]), int(g["ref"]), [int(v) for v in g["pl"]]) for g in arr]


def genotypes(table, text, p, first: int = 0, count=None):
    """(pos uint64 (m,), counts uint32 (m, 6), gts GENOTYPE_DTYPE (m,)) of the selected rows of [first, first + count) of the table
    (n x 6) over the text (n letters), in ascending position."""
    p = check_params(p)
    T = ext_spec._letters(text)
    n = len(T)
    assert table.shape == (n, 6)
    count = n - first if count is None else count
    assert 0 <= first <= n and 0 <= count <= n - first
    # (a row whose A C G T columns are all 0 has every L equal to 0: rr wins the tie -- those rows are not looked at one by one)
    live = first + np.nonzero(np.asarray(table[first:first + count])[:, :4].any(axis=1))[0]
    pos, gts = [], []
    for x in live:
        r = _COL.get(T[x] & 0xDF)
        row = [int(v) for v in table[x]]
        if r is None or sum(row[:5]) < p[5]:
            continue
        g, variant = snv(row, r, p)
        if variant:
            pos.append(int(x))
            gts.append(g)
    counts = np.asarray(table)[pos].astype(np.uint32).reshape(len(pos), 6)
    return np.array(pos, dtype=np.uint64), counts, to_records(gts)


def genotype_events(events, anchor_rows, p):
    """(gts, called uint8) of event tuples (events_spec's) and the rows (m x 6) of their anchors."""
    p = check_params(p)
    out, called = [], []
    for ev, row in zip(events, anchor_rows):
        g, c = event(int(ev[4]) + int(ev[5]), sum(int(v) for v in row[:5]), p)
        out.append(g)
        called.append(1 if c else 0)
    return to_records(out), np.array(called, dtype=np.uint8)


# ---- the file ------------------------------------------------------------------------------------------------------------------

VCF_HEADER_INFO = (b'##INFO=<ID=DP,Number=1,Type=Integer,Description="Depth A+C+G+T+D at the row (SNV) or at the anchor row (indel)">\n'
                   b'##INFO=<ID=AO,Number=A,Type=Integer,Description="Observations of each alternate allele">\n'
                   b'##INFO=<ID=SF,Number=1,Type=Integer,Description="Observations of the alternate allele on forward-strand reads">\n'
                   b'##INFO=<ID=SR,Number=1,Type=Integer,Description="Observations of the alternate allele on reverse-strand reads">\n')
VCF_HEADER_FORMAT = (b'##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
                     b'##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Depth A+C+G+T+D at the row (SNV) or at the anchor row (indel)">\n'
                     b'##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Observations of the reference and of each alternate allele">\n'
                     b'##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality: the Phred-scaled distance to the second-best genotype, at most 99">\n'
                     b'##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods, the smallest 0">\n')


def phred(milli: int) -> int:
    return (milli + 500) // 1000


def vcf_header(ref) -> bytes:
    out = [b"##fileformat=VCFv4.2\n"]
    for r in range(ref.s.num):
        out.append(b"##contig=<ID=%s,length=%d>\n" % (map_spec.cut_name(ref.names[r]), int(ref.sizes[r])))
    out.append(VCF_HEADER_INFO)
    out.append(VCF_HEADER_FORMAT)
    out.append(b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n")
    return b"".join(out)


def sample_column(g, alleles, dp: int, ad) -> bytes:
    """GT:DP:AD:GQ:PL of a genotype record over the line's alleles (what a and b may be, REF first): the allele numbers of a and
    b ascending, joined by / (one number at ploidy 1); PL the line's genotypes in VCF order, k (k + 1) / 2 + j over the allele
    numbers, minus their own minimum, each rounded as QUAL is; GQ at most 99."""
    qual, gq, a, b, ploidy, _ref, pl = g
    num = sorted((alleles.index(a), alleles.index(b)))
    if ploidy == 2:
        gt = b"%d/%d" % tuple(num)
        # on an SNV line an allele is a letter column and the record's pl is indexed by the letters' pair; on an event line by 0/1
        vals = [pl[genotype_index(min(alleles[j], alleles[k]), max(alleles[j], alleles[k]))] for k in range(len(alleles)) for j in range(k + 1)]
    else:
        gt = b"%d" % num[0]
        vals = [pl[x] for x in alleles]
    low = min(vals)
    return b"GT:DP:AD:GQ:PL\t%s:%d:%s:%d:%s" % (gt, dp, b",".join(b"%d" % v for v in ad), min(phred(gq), 99),
                                                 b",".join(b"%d" % phred(v - low) for v in vals))


def snv_line(name: bytes, pos1: int, letter: int, counts, g) -> bytes:
    """The line of a selected row: ALT the best genotype's letters other than the reference's, ascending."""
    r = g[5]
    alts = sorted({g[2], g[3]} - {r})
    alleles = [r] + alts
    c = [int(v) for v in counts]
    d = sum(c[:5])
    return b"%s\t%d\t.\t%s\t%s\t%d\t.\tDP=%d;AO=%s\t%s\n" % (
        name, pos1, bytes([letter]).upper(), b",".join(ACGT[k:k + 1] for k in alts), phred(g[0]), d, b",".join(b"%d" % c[k] for k in alts),
        sample_column(g, alleles, d, [c[k] for k in alleles]))


def event_line(T: bytes, table, ev, g, called: int, name: bytes, a: int, size: int):
    """(POS, line) of one event of the record that starts at a, or None when it is not called: events_spec's line with every
    event called, QUAL in the place of its '.', and the sample column (AD = ro, ao)."""
    if not called:
        return None
    got = events_spec.event_line(T, table, ev, name, a, size, 1, 0)  # (REF, ALT, INFO; the record's end rule)
    if got is None:
        return None
    POS, line = got
    cols = line[:-1].split(b"\t")
    assert cols[5] == b"."
    cols[5] = b"%d" % phred(g[0])
    pos, fwd, rev = ev[0], ev[4], ev[5]
    anchor = pos - 1 if pos - a > 0 else pos
    d = int(sum(int(v) for v in table[anchor][:5]))
    ao = fwd + rev
    return POS, b"\t".join(cols) + b"\t" + sample_column(g, [0, 1], d, [d - ao if d > ao else 0, ao]) + b"\n"


def vcf_file(table, events, ref, p) -> bytes:
    """The -vcf -gt file of a pileup table (n x 6, as counts() gives it) and its events (the read-out of the whole text with
    min_count 1): the header, then per record a line per selected row and per called event, sorted by POS; at one POS the SNV
    first, then the events in event order.  An event whose pos lies in no record (a separator) gives no line.  ref:
    hostlib.Loaded of the merged reference."""
    p = check_params(p)
    T = ext_spec._letters(ref.chars)
    pos, counts, gts = genotypes(table, ref.chars, p)
    gl = from_records(gts)
    starts = ref.merged_start if ref.s.num > 1 else [0]
    out = [vcf_header(ref)]
    for r in range(len(starts)):
        name = map_spec.cut_name(ref.names[r])
        a, size = int(starts[r]), int(ref.sizes[r])
        lines = []
        for i in range(len(pos)):
            x = int(pos[i])
            if a <= x < a + size:
                lines.append(((x - a + 1, 0, len(lines)), snv_line(name, x - a + 1, T[x], counts[i], gl[i])))
        mine = [ev for ev in events if a <= ev[0] < a + size]
        anchors = [ev[0] - 1 if ev[0] > a else ev[0] for ev in mine]
        eg, called = genotype_events(mine, [table[x] for x in anchors], p)
        for ev, g, c in zip(mine, from_records(eg), called):
            got = event_line(T, table, ev, g, int(c), name, a, size)
            if got is not None:
                lines.append(((got[0], 1, len(lines)), got[1]))
        out.extend(line for _, line in sorted(lines, key=lambda t: t[0]))
    return b"".join(out)
