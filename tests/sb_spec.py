"""-sb on the checker side: the strand table of a -vcf -gt line, FS, and the lines of the -vcf -gt -sb file.
Python integers and floats, no engine.  Builds on gt_spec (the genotypes and the lines of -vcf -gt) and pile_spec (the table).

A table is (rf, rr, af, ar): reference forward, reference reverse, alternative forward, alternative reverse.  `row` is the
position's row of counts() and `frow` the forward accumulator's; no counter of frow is above row's.
  SNV line   r the reference column, ALT the line's alternative letters: rf = frow[r], rr = row[r] - frow[r], af and ar the same
             summed over ALT
  event      af = fwd, ar = rev of the event; d, df the depths A+C+G+T+D of the anchor's two rows: rf = df - af, rr = (d - df) - ar,
             each 0 when it would be negative (the saturating form of gt_spec's ro)
Every cell stops at 2^32 - 1.

FS is the Phred-scaled two-sided Fisher exact test of the table, in doubles, one operation after the other:
  1. s the sum; s > 400: every cell becomes cell * 200 // s
  2. lf[0] = 0, lf[i] = lf[i - 1] + log10(i)
  3. r1 = rf + rr, r2 = af + ar, c1 = rf + af, N the sum;
     logp(x) = lf[r1] + lf[r2] + lf[c1] + lf[N - c1] - lf[N] - lf[x] - lf[r1 - x] - lf[c1 - x] - lf[r2 - c1 + x], left to right
  4. p = the sum of 10 ** logp(x) over x ascending from max(0, c1 - r2) to min(r1, c1) with logp(x) <= logp(rf) + 1e-7
  5. FS = 0 when N == 0 or p >= 1, else -10 * log10(p); printed with %.3f"""
import math

import ext_spec
import gt_spec
import map_spec
import pile_spec  # noqa: F401  (the table's layout: n x 6, columns A C G T D I)

CELL_MAX = 2 ** 32 - 1


def normalise(t):
    t = tuple(int(v) for v in t)
    assert len(t) == 4 and all(0 <= v <= CELL_MAX for v in t)
    s = sum(t)
    return tuple(v * 200 // s for v in t) if s > 400 else t


def fisher_strand(t) -> float:
    rf, rr, af, ar = normalise(t)
    r1, r2, c1 = rf + rr, af + ar, rf + af
    N = r1 + r2
    if N == 0:
        return 0.0
    lf = [0.0]
    for i in range(1, N + 1):
        lf.append(lf[i - 1] + math.log10(float(i)))

    def logp(x):
        v = lf[r1]
        for w in (lf[r2], lf[c1], lf[N - c1]):
            v = v + w
        for w in (lf[N], lf[x], lf[r1 - x], lf[c1 - x], lf[r2 - c1 + x]):
            v = v - w
        return v
    cut = logp(rf) + 1e-7
    p = 0.0
    for x in range(max(0, c1 - r2), min(r1, c1) + 1):
        v = logp(x)
        if v <= cut:
            p = p + math.pow(10.0, v)
    if p >= 1.0:
        return 0.0
    return -10.0 * math.log10(p)


def fs_text(t) -> bytes:
    return b"%.3f" % fisher_strand(t)


def _cell(v: int) -> int:
    return min(max(v, 0), CELL_MAX)


def snv_table(row, frow, r: int, alts):
    row, frow = [int(v) for v in row], [int(v) for v in frow]
    assert all(f <= c for f, c in zip(frow, row))
    return (_cell(frow[r]), _cell(row[r] - frow[r]), _cell(sum(frow[k] for k in alts)), _cell(sum(row[k] - frow[k] for k in alts)))


def event_table(row, frow, fwd: int, rev: int):
    row, frow = [int(v) for v in row], [int(v) for v in frow]
    assert all(f <= c for f, c in zip(frow, row))
    d, df = sum(row[:5]), sum(frow[:5])
    return (_cell(df - fwd), _cell((d - df) - rev), _cell(fwd), _cell(rev))


# ---- the file ------------------------------------------------------------------------------------------------------------------

HEADER_FS = b'##INFO=<ID=FS,Number=1,Type=Float,Description="Phred-scaled p-value of Fisher\'s exact test of the strand table SB">\n'
HEADER_SB = (b'##FORMAT=<ID=SB,Number=4,Type=Integer,Description="Observations of the reference on forward and reverse reads, '
             b'then of the alternate alleles on forward and reverse reads">\n')


def vcf_header(ref, fs=None) -> bytes:
    """gt_spec's header with FS behind the INFO lines, SB behind the FORMAT lines and, with -fs N, the FILTER line in front of
    the INFO lines."""
    out = [b"##fileformat=VCFv4.2\n"]
    for r in range(ref.s.num):
        out.append(b"##contig=<ID=%s,length=%d>\n" % (map_spec.cut_name(ref.names[r]), int(ref.sizes[r])))
    if fs is not None:
        out.append(b'##FILTER=<ID=sb,Description="Strand bias: FS above %d">\n' % fs)
    out += [gt_spec.VCF_HEADER_INFO, HEADER_FS, gt_spec.VCF_HEADER_FORMAT, HEADER_SB,
            b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n"]
    return b"".join(out)


def decorate(line: bytes, t, fs=None) -> bytes:
    """A line of the -vcf -gt file with its table: FILTER, ;FS= behind INFO, :SB behind FORMAT, the four cells behind the sample."""
    cols = line[:-1].split(b"\t")
    assert len(cols) == 10 and cols[6] == b"." and cols[8] == b"GT:DP:AD:GQ:PL"
    if fs is not None:
        assert 0 <= fs <= 999
        cols[6] = b"sb" if fisher_strand(t) > fs else b"PASS"
    cols[7] += b";FS=" + fs_text(t)
    cols[8] += b":SB"
    cols[9] += b":%d,%d,%d,%d" % tuple(t)
    return b"\t".join(cols) + b"\n"


def vcf_file(table, ftable, events, ref, p, fs=None) -> bytes:
    """The -vcf -gt -sb file of a pileup table, the forward accumulator's table and the events: gt_spec.vcf_file line for line,
    every line decorated.  fs: the N of -fs N, or None."""
    p = gt_spec.check_params(p)
    T = ext_spec._letters(ref.chars)
    pos, counts, gts = gt_spec.genotypes(table, ref.chars, p)
    gl = gt_spec.from_records(gts)
    starts = ref.merged_start if ref.s.num > 1 else [0]
    out = [vcf_header(ref, fs)]
    for r in range(len(starts)):
        name = map_spec.cut_name(ref.names[r])
        a, size = int(starts[r]), int(ref.sizes[r])
        lines = []
        for i in range(len(pos)):
            x = int(pos[i])
            if a <= x < a + size:
                g = gl[i]
                alts = sorted({g[2], g[3]} - {g[5]})
                t = snv_table(counts[i], ftable[x], g[5], alts)
                lines.append(((x - a + 1, 0, len(lines)), decorate(gt_spec.snv_line(name, x - a + 1, T[x], counts[i], g), t, fs)))
        mine = [ev for ev in events if a <= ev[0] < a + size]
        anchors = [ev[0] - 1 if ev[0] > a else ev[0] for ev in mine]
        eg, called = gt_spec.genotype_events(mine, [table[x] for x in anchors], p)
        for ev, g, c, x in zip(mine, gt_spec.from_records(eg), called, anchors):
            got = gt_spec.event_line(T, table, ev, g, int(c), name, a, size)
            if got is not None:
                t = event_table(table[x], ftable[x], int(ev[4]), int(ev[5]))
                lines.append(((got[0], 1, len(lines)), decorate(got[1], t, fs)))
        out.extend(line for _, line in sorted(lines, key=lambda k: k[0]))
    return b"".join(out)
