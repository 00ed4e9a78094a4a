"""-cons -gt on the checker side: the consensus sequence of a pileup table, its quality sums and its indel events
with every decision made by the genotype likelihood of -gt.  Python integers, no engine.
Builds on cons_spec (the anchor row, the depth, the order of a row's emissions, the FASTA record), gt_spec (the genotype of a row
and of an event) and qual_spec (the weighted genotype of a row); restates none of them.

table is n x 6 (A C G T D I, as counts() gives it), qtable the quality sums of the same shape (Pileup.quality.counts(); looked at
only when weighted), T the text, E the events as events() gives them (tuples (pos, kind, len, S, fwd, rev) in events_spec's
order).  P_row = (ploidy, M, H, E, hp) are the costs of the rows -- what genotypes(...) would use, WQ_COSTS when weighted -- and
P_ev those of the events -- what genotype_events(...) would use, gt_costs(err_q).  min_gq is in Phred, 0 to 999; a genotype is
confident when its GQ, in 64 bits, is at least 1000 * min_gq milli-Phred.

An event is applied iff its anchor row a (cons_spec.anchor) holds one of A,C,G,T, d(a) >= min_depth, the best genotype of
gt_spec.event(fwd + rev, d(a), P_ev) is homozygous for the event (1/1, or 1 at ploidy 1) and that genotype is confident.  A
heterozygous event is not applied.  Row p emits

  1. the letters of the applied insertion at p with the most observations (a tie: the first in E), also when rule 2 drops the row;
  2. nothing more if an applied deletion covers p;
  3. else N if T[p] is none of A,C,G,T;
  4. else T[p] in lower case if d(p) < min_depth, or A+C+G+T == 0, or the genotype of the row (gt_spec.snv, qual_spec.snv when
     weighted) is not confident;
  5. else the best genotype (a, b) in upper case: the letter when a == b, else the IUPAC code of the two.

stats: rows of rule 4; rows of rule 5 whose byte is not T[p] in upper case; rows of rule 2; insertions emitted; letters inserted;
rows of rule 5 with an IUPAC code; rows of rule 4 that are deep enough and show letters (uncalled for GQ alone); events with pos in
the range whose best genotype is heterozygous and confident (whatever their anchor's depth)."""
import cons_spec
import events_spec
import ext_spec
import gt_spec
import qual_spec

ACGT = b"ACGT"
IUPAC = {(0, 1): b"M", (0, 2): b"R", (0, 3): b"W", (1, 2): b"S", (1, 3): b"Y", (2, 3): b"K"}
RULES = ("deleted", "N", "uncalled", "called")


def rule_params(p, min_depth: int = 1):
    """gt_spec's parameter tuple of P_row or P_ev (min_qual, which nothing here looks at, is 0)."""
    ploidy, M, H, E, hp = (int(v) for v in p[:5])
    return gt_spec.check_params((ploidy, M, H, E, hp, min_depth, 0))


def params(ploidy: int = 2, err_q: int = 20, het_q: int = 30, weighted: bool = False, costs=None):
    """(P_row, P_ev) of the public interface's arguments."""
    ev = (ploidy,) + gt_spec.gt_costs(err_q) + (1000 * het_q,)
    row = (ploidy,) + tuple(costs if costs is not None else qual_spec.WQ_COSTS if weighted else gt_spec.gt_costs(err_q)) + (1000 * het_q,)
    return row, ev


def threshold(min_gq: int) -> int:
    assert 0 <= min_gq <= 999
    return 1000 * min_gq


def confident(g, min_gq: int) -> bool:
    """g: a genotype tuple of gt_spec.  Its gq saturates at 2^32 - 1, far above every threshold, so the comparison is the one of
    the 64-bit value."""
    assert threshold(min_gq) < gt_spec.SAT
    return g[1] >= threshold(min_gq)


def event_genotype_applies(g) -> bool:
    """1/1, or 1 at ploidy 1"""
    return g[2] == 1 and g[3] == 1


def letter_of(a: int, b: int) -> bytes:
    return ACGT[a:a + 1] if a == b else IUPAC[(min(a, b), max(a, b))]


def event_call(T: bytes, table, ev, P_ev, min_depth: int, min_gq: int):
    """(applied, het): het -- the best genotype is heterozygous and confident, whatever the anchor."""
    a = cons_spec.anchor(T, ev[0])
    d = cons_spec.depth(table, a)
    g, _ = gt_spec.event(int(ev[4]) + int(ev[5]), d, rule_params(P_ev))
    sure = confident(g, min_gq)
    ok = events_spec.is_acgt(T[a]) and d >= min_depth and sure and event_genotype_applies(g)
    return ok, sure and g[2] != g[3]


def row(T: bytes, table, qtable, p: int, P_row, min_depth: int, min_gq: int, weighted: bool):
    """(rule, letter, why) of a row that no deletion covers: rules 3 to 5.  why: of an uncalled row 'depth', 'empty' or 'gq'; of a
    called one 'hom' or 'het'."""
    if not events_spec.is_acgt(T[p]):
        return "N", b"N", ""
    own = T[p] & 0xDF
    c = [int(v) for v in table[p][:4]]
    if cons_spec.depth(table, p) < min_depth:
        return "uncalled", bytes([own | 0x20]), "depth"
    if sum(c) == 0:
        return "uncalled", bytes([own | 0x20]), "empty"
    r = ACGT.index(own)
    P = rule_params(P_row)
    g, _ = qual_spec.snv(c, [int(v) for v in qtable[p][:4]], r, P) if weighted else gt_spec.snv(c, r, P)
    if not confident(g, min_gq):
        return "uncalled", bytes([own | 0x20]), "gq"
    return "called", letter_of(g[2], g[3]), "hom" if g[2] == g[3] else "het"


def emissions(text, table, events, P_row, P_ev, min_depth: int = 4, min_gq: int = 20, qtable=None, first: int = 0, count=None):
    """Per row of [first, first + count): (inserted letters, rule, own letter, why), and the number of heterozygous confident events
    with pos in the range."""
    T = ext_spec._letters(text)
    n = len(T)
    count = n - first if count is None else count
    weighted = qtable is not None
    assert 0 <= first <= n and 0 <= count <= n - first and 1 <= min_depth < 2 ** 31
    deleted, ins, het = set(), {}, 0
    for ev in events:  # (in E's order: a later insertion replaces an earlier one only with more observations)
        ok, h = event_call(T, table, ev, P_ev, min_depth, min_gq)
        het += bool(h) and first <= ev[0] < first + count
        if not ok:
            continue
        if ev[1] == 0:
            deleted.update(range(ev[0], ev[0] + ev[2]))
        elif ev[0] not in ins or ev[4] + ev[5] > ins[ev[0]][4] + ins[ev[0]][5]:
            ins[ev[0]] = ev
    out = []
    for p in range(first, first + count):
        S = ins[p][3] if p in ins else b""
        if p in deleted:
            out.append((S, "deleted", b"", ""))
        else:
            out.append((S,) + row(T, table, qtable, p, P_row, min_depth, min_gq, weighted))
    return out, het


def consensus(text, table, events, P_row, P_ev, min_depth: int = 4, min_gq: int = 20, qtable=None, first: int = 0, count=None, bounds=()):
    """(bytes, offs, stats) of rows [first, first + count); qtable: the quality sums, which makes the call the weighted one."""
    T = ext_spec._letters(text)
    em, het = emissions(text, table, events, P_row, P_ev, min_depth, min_gq, qtable, first, count)
    out, starts, stats = [], [], [0] * 8
    size = 0
    for i, (S, rule, letter, why) in enumerate(em):
        starts.append(size)
        out.append(S + letter)
        size += len(S) + len(letter)
        stats[0] += rule == "uncalled"
        stats[1] += rule == "called" and letter[0] != (T[first + i] & 0xDF)
        stats[2] += rule == "deleted"
        stats[3] += len(S) > 0
        stats[4] += len(S)
        stats[5] += why == "het"
        stats[6] += why == "gq"
    stats[7] = het
    starts.append(size)
    offs = []
    for b in bounds:
        assert first <= b <= first + len(em)
        offs.append(starts[b - first])
    return b"".join(out), offs, stats
