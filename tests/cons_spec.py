"""-cons on the checker side: the consensus sequence of a pileup table and its indel events, straight from the definition of
DESIGN.md 4.19, and the FASTA file of the front end.  Python integers, no engine.  Builds on events_spec (the order of E, the
letters) and map_spec (the cut of a record's name); restates neither.

table is n x 6 (A C G T D I, as counts() gives it), T the text, L(p) its letter in upper case, ACGT(p): L(p) is one of A,C,G,T,
d(p) = A+C+G+T+D, E the events as the read-out of the whole text gives them with min_count 1: tuples (pos, kind, len, S, fwd, rev)
in events_spec's order.  The anchor row of an event is pos - 1 if pos >= 1 and ACGT(pos - 1), else pos; the event is applied iff
ACGT(a), d(a) >= min_depth and 2 * (fwd + rev) > d(a).  Row p emits

  1. the letters of the applied insertion at p with the most observations (a tie: the first in E), also when rule 2 drops the row;
  2. nothing more if an applied deletion covers p;
  3. else N if not ACGT(p);
  4. else L(p) in lower case if d(p) < min_depth or A+C+G+T == 0;
  5. else the letter of the largest of A,C,G,T; a tie: L(p) if it is among the largest, else the first in the order A,C,G,T.

stats: rows of rule 4, rows of rule 5 whose letter is not L(p), rows of rule 2, insertions emitted, letters inserted."""
import events_spec
import ext_spec
import map_spec

ACGT = b"ACGT"
RULES = ("deleted", "N", "uncalled", "called")


def anchor(T: bytes, pos: int) -> int:
    return pos - 1 if pos >= 1 and events_spec.is_acgt(T[pos - 1]) else pos


def depth(table, p: int) -> int:
    return sum(int(v) for v in table[p][:5])


def applied(T: bytes, table, ev, min_depth: int) -> bool:
    a = anchor(T, ev[0])
    d = depth(table, a)
    return events_spec.is_acgt(T[a]) and d >= min_depth and 2 * (ev[4] + ev[5]) > d


def row(T: bytes, table, p: int, min_depth: int):
    """(rule, letter, tie) of a row that no deletion covers: rules 3 to 5.  tie: '' none, 'own' the text's letter is among several
    largest, 'first' it is not."""
    if not events_spec.is_acgt(T[p]):
        return "N", b"N", ""
    own = T[p] & 0xDF
    c = [int(v) for v in table[p][:4]]
    if depth(table, p) < min_depth or sum(c) == 0:
        return "uncalled", bytes([own | 0x20]), ""
    top = max(c)
    tied = [k for k in range(4) if c[k] == top]
    if ACGT.index(own) in tied:
        return "called", bytes([own]), "own" if len(tied) > 1 else ""
    return "called", ACGT[tied[0]:tied[0] + 1], "first" if len(tied) > 1 else ""


def emissions(text, table, events, min_depth: int = 4, first: int = 0, count=None):
    """Per row of [first, first + count): (inserted letters, rule, own letter) -- the row emits the first and the third."""
    T = ext_spec._letters(text)
    n = len(T)
    count = n - first if count is None else count
    assert 0 <= first <= n and 0 <= count <= n - first and 1 <= min_depth < 2 ** 31
    deleted, ins = set(), {}
    for ev in events:  # (in E's order: a later insertion replaces an earlier one only with more observations)
        if not applied(T, table, ev, min_depth):
            continue
        if ev[1] == 0:
            deleted.update(range(ev[0], ev[0] + ev[2]))
        elif ev[0] not in ins or ev[4] + ev[5] > ins[ev[0]][4] + ins[ev[0]][5]:
            ins[ev[0]] = ev
    out = []
    for p in range(first, first + count):
        S = ins[p][3] if p in ins else b""
        if p in deleted:
            out.append((S, "deleted", b""))
        else:
            rule, letter, _ = row(T, table, p, min_depth)
            out.append((S, rule, letter))
    return out


def consensus(text, table, events, min_depth: int = 4, first: int = 0, count=None, bounds=()):
    """(bytes, offs, stats) of rows [first, first + count)."""
    T = ext_spec._letters(text)
    em = emissions(text, table, events, min_depth, first, count)
    out, starts, stats = [], [], [0, 0, 0, 0, 0]
    size = 0
    for i, (S, rule, letter) in enumerate(em):
        starts.append(size)
        out.append(S + letter)
        size += len(S) + len(letter)
        stats[0] += rule == "uncalled"
        stats[1] += rule == "called" and letter[0] != (T[first + i] & 0xDF)
        stats[2] += rule == "deleted"
        stats[3] += len(S) > 0
        stats[4] += len(S)
    starts.append(size)
    offs = []
    for b in bounds:
        assert first <= b <= first + len(em)
        offs.append(starts[b - first])
    return b"".join(out), offs, stats


def fasta_record(name: bytes, letters: bytes) -> bytes:
    out = [b">" + map_spec.cut_name(name) + b"\n"]
    for i in range(0, len(letters), 60):
        out.append(letters[i:i + 60] + b"\n")
    return b"".join(out)


def fasta_file(table, events, ref, min_depth: int = 4) -> bytes:
    """The -cons file: a record per reference record, its rows from its first to its end (the separators between the records, and
    an insertion in front of one, are no record's).  ref: hostlib.Loaded of the merged reference."""
    starts = ref.merged_start if ref.s.num > 1 else [0]
    bounds = []
    for r in range(len(starts)):
        bounds += [int(starts[r]), int(starts[r]) + int(ref.sizes[r])]
    seq, offs, _ = consensus(ref.chars, table, events, min_depth, bounds=bounds)
    return b"".join(fasta_record(ref.names[r], seq[offs[2 * r]:offs[2 * r + 1]]) for r in range(len(starts)))
