"""-sam on the checker side: the MD entries, the MD text, the primary segment and the SAM lines, straight from the definition of
DESIGN.md 4.22, and a replay checker that knows nothing of the implementation.  Builds on map_spec (one mapping per read, the
segments in 4.15's order); restates nothing of it.

A read of n letters has, from map_spec.read_map, (strand, mapq, s1, s2, segments), a segment being (ref_pos, query_pos, ref_len,
query_len, edits, [(op, k), ...]) with the operations = X I D left to right in the scanned strand.

  MD entries  walk the operations with p from ref_pos, m = the reference letters under = since the last entry (or the segment's
              start; an I changes neither p nor m): every letter under X or D emits m << 4 | d << 2 | c and sets m = 0 -- d is 1
              under D, c is 0..3 for the text's letter A C G T at p, upper-cased --; after the last operation the closing entry
              m << 4 | 8
  MD text     an X entry prints m and the letter; a D entry with m == 0 whose predecessor in the segment is a D entry continues
              that ^ group, any other D entry prints m, ^ and the letter; the closing entry prints m
  eq          the letters under = of a segment; the primary segment of a read is the one with the largest eq, the first on a tie
  lines       one per segment (an unmapped read: one line with flag 4), soft clips on every line, see sam_lines

Python integers: no overflow."""
import re

import numpy as np

import ext_spec
import map_spec

CLOSE = 8
NO_SEGMENT = 0xFFFFFFFF
MD_RE = re.compile(rb"^[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*$")


def md_entries(seg, T):
    """The entries of one segment.  T: the text's letters (bytes or a uint8 array)."""
    p, m, out = int(seg[0]), 0, []
    for c, k in seg[5]:
        if c == "=":
            m += k
            p += k
        elif c == "I":
            pass
        else:
            for j in range(k):
                letter = int(T[p + j]) & 0xDF
                # gap closing refuses pieces with other letters and the X-drop walk stops in front of them
                assert letter in b"ACGT", "a reference letter under %s that is none of A,C,G,T" % c
                out.append(m << 4 | (4 if c == "D" else 0) | b"ACGT".index(letter))
                m = 0
            p += k
    out.append(m << 4 | CLOSE)
    return out


def md_text(entries) -> bytes:
    out, prev_d = [], False
    for e in entries:
        m = int(e) >> 4
        if int(e) & CLOSE:
            out.append(b"%d" % m)
            break
        letter = b"ACGT"[int(e) & 3:(int(e) & 3) + 1]
        if int(e) & 4:
            out.append(letter if (prev_d and m == 0) else b"%d^" % m + letter)
        else:
            out.append(b"%d" % m + letter)
        prev_d = bool(int(e) & 4)
    return b"".join(out)


def seg_eq(seg) -> int:
    return sum(k for c, k in seg[5] if c == "=")


def primary(segl) -> int:
    """The index of the primary segment among a read's segments; NO_SEGMENT when it has none."""
    if not segl:
        return NO_SEGMENT
    eqs = [seg_eq(s) for s in segl]
    return eqs.index(max(eqs))


def pack_md(reads, T):
    """read_map tuples -> what the engine returns beside map_spec.pack: (entries uint32, offsets per segment, eq per segment,
    primary per read)."""
    md, moff, eq, prim = [], [0], [], []
    for r in reads:
        for s in r[4]:
            md += md_entries(s, T)
            moff.append(len(md))
            eq.append(seg_eq(s))
        prim.append(primary(r[4]))
    return (np.array(md, dtype=np.uint32), np.array(moff, dtype=np.int64), np.array(eq, dtype=np.uint32),
            np.array(prim, dtype=np.uint32))


def cigar(n: int, seg) -> bytes:
    """The line's CIGAR: soft clips around the segment's operations, so that it covers the whole read."""
    q, qlen = int(seg[1]), int(seg[3])
    out = b"%dS" % q if q else b""
    out += b"".join(b"%d%s" % (k, c.encode()) for c, k in seg[5])
    tail = n - q - qlen
    return out + (b"%dS" % tail if tail else b"")


def locate(p: int, ref):
    """(record, position local to it) of merged position p, as PAF finds them."""
    if ref.s.num > 1:
        starts = ref.merged_start
        r = max(i for i in range(len(starts)) if starts[i] <= p)
        return r, p - starts[r]
    return 0, p


def sam_lines(name: bytes, letters: bytes, quals, result, ref, T=None) -> bytes:
    """The SAM lines of one read.  letters: the read as given; quals: its quality bytes or None (FASTA); ref: hostlib.Loaded of the
    merged reference; T: the text the segments' positions count in (ref.chars by default)."""
    strand, mapq, s1, s2, segl = result
    T = ref.chars if T is None else T
    n = len(letters)
    nm = map_spec.cut_name(name)
    if strand == 0 or not segl:
        return b"\t".join([nm, b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", bytes(letters), bytes(quals) if quals is not None else b"*"]) + b"\n"
    rec = np.frombuffer(bytes(letters), dtype=np.uint8)
    seq = bytes(ext_spec.revcomp(rec)) if strand == 2 else bytes(letters)
    qual = b"*" if quals is None else (bytes(quals)[::-1] if strand == 2 else bytes(quals))
    prim = primary(segl)
    where = [locate(int(s[0]), ref) for s in segl]
    cig = [cigar(n, s) for s in segl]
    sa = [b"%s,%d,%s,%s,%d,%d;" % (map_spec.cut_name(ref.names[r]), ts + 1, b"-" if strand == 2 else b"+", cig[i], mapq, int(segl[i][4]))
          for i, (r, ts) in enumerate(where)]
    out = []
    for i, s in enumerate(segl):
        r, ts = where[i]
        flag = (16 if strand == 2 else 0) | (0 if i == prim else 2048)
        f = [nm, b"%d" % flag, map_spec.cut_name(ref.names[r]), b"%d" % (ts + 1), b"%d" % mapq, cig[i], b"*", b"0", b"0", seq, qual,
             b"NM:i:%d" % int(s[4]), b"MD:Z:" + md_text(md_entries(s, T)), b"s1:i:%d" % s1, b"s2:i:%d" % s2]
        if len(segl) > 1:
            f.append(b"SA:Z:" + b"".join(sa[j] for j in range(len(segl)) if j != i))
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


def header(ref) -> bytes:
    out = [b"@HD\tVN:1.6\tSO:unsorted\n"]
    for name, size in zip(ref.names, ref.sizes):
        out.append(b"@SQ\tSN:%s\tLN:%d\n" % (map_spec.cut_name(name), size))
    out.append(b"@PG\tID:slaMEM-hip\tPN:slaMEM-hip\n")
    return b"".join(out)


def sam_file(reads, names, letters, quals, ref) -> bytes:
    """reads: read_map tuples; letters: the reads as given, a bytes each; quals: a bytes each, or None."""
    return header(ref) + b"".join(sam_lines(names[i], letters[i], quals[i] if quals is not None else None, r, ref)
                                  for i, r in enumerate(reads))


# ---- the replay checker: knows the SAM format and the reference, nothing of the implementation ----------------------------------

_CIG = re.compile(rb"(\d+)([=XIDS])")


def _parse_md(md: bytes):
    """-> [(run of matches, 'X' letter | '^' letters | None)]"""
    assert MD_RE.match(md), md
    out = []
    at = 0
    for m in re.finditer(rb"([0-9]+)(\^[A-Z]+|[A-Z])?", md):
        assert m.start() == at
        at = m.end()
        out.append((int(m.group(1)), m.group(2)))
    assert at == len(md)
    return out


def replay_line(fields, ref_records):
    """One mapped line: rebuilds the aligned read letters from the reference, the CIGAR and the MD alone, and compares them with
    SEQ between the clips.  ref_records: {name: upper-cased letters}.  Returns (query length of the CIGAR, letters under X I D)."""
    rname, pos, cg, seq = fields[2], int(fields[3]), fields[5], fields[9]
    tags = dict((t[:2], t[5:]) for t in fields[11:])
    assert b"".join(a + b for a, b in _CIG.findall(cg)) == cg, cg
    ops = [(int(a), b.decode()) for a, b in _CIG.findall(cg)]
    R = ref_records[rname]
    md = _parse_md(tags[b"MD"])
    # the MD as a stream over the reference letters the alignment covers: ('=', None) | ('X', letter) | ('D', letter)
    stream = []
    for run, what in md:
        stream += [("=", None)] * run
        if what is None:
            continue
        if what.startswith(b"^"):
            stream += [("D", bytes([c])) for c in what[1:]]
        else:
            stream.append(("X", what))
    p, q, si, nm = pos - 1, 0, 0, 0
    body = []
    for k, c in ops:
        if c == "S":
            assert q == 0 or q + k == len(seq), "a clip inside the CIGAR"
            q += k
        elif c == "I":
            body.append(seq[q:q + k])
            q += k
            nm += k
        elif c == "D":
            for j in range(k):
                kind, letter = stream[si]
                assert kind == "D" and letter == R[p + j:p + j + 1], "MD and CIGAR disagree under D"
                si += 1
            p += k
            nm += k
        else:
            for j in range(k):
                kind, letter = stream[si]
                si += 1
                refl = R[p + j:p + j + 1]
                if c == "=":
                    assert kind == "=", "MD has an edit under ="
                    body.append(refl)
                else:
                    assert kind == "X" and letter == refl, "MD and reference disagree under X"
                    got = seq[q + j:q + j + 1].upper()
                    assert got != refl, "an X over equal letters"
                    body.append(seq[q + j:q + j + 1])
            p += k
            q += k
            nm += k if c == "X" else 0
    assert si == len(stream), "MD covers other reference letters than the CIGAR"
    lead = ops[0][0] if ops[0][1] == "S" else 0
    tail = ops[-1][0] if ops[-1][1] == "S" and len(ops) > 1 else 0
    aligned = seq[lead:len(seq) - tail]
    assert b"".join(body).upper() == aligned.upper(), "the replayed letters differ from SEQ"
    return q, nm


def replay_check(sam: bytes, ref, names, letters, results, quals=None):
    """The whole file against the reference (hostlib.Loaded, merged) and the reads' slamem_map records (read_map tuples, or
    anything whose [0] is the strand and [4] the segments): every check of the issue's list.  Returns the number of mapped lines."""
    lines = sam.split(b"\n")
    assert lines[-1] == b""
    lines = lines[:-1]
    nh = 0
    while nh < len(lines) and lines[nh].startswith(b"@"):
        nh += 1
    assert lines[0] == b"@HD\tVN:1.6\tSO:unsorted" and lines[nh - 1].startswith(b"@PG")
    sq = [l.split(b"\t") for l in lines[1:nh - 1]]
    assert [(f[0], f[1][3:], int(f[2][3:])) for f in sq] == [(b"@SQ", map_spec.cut_name(nm), sz) for nm, sz in zip(ref.names, ref.sizes)]
    chars = ref.chars
    records = {}
    for i, nm in enumerate(ref.names):
        st = ref.merged_start[i] if ref.s.num > 1 else 0
        records[map_spec.cut_name(nm)] = chars[st:st + ref.sizes[i]].upper()
    body = [l.split(b"\t") for l in lines[nh:]]
    at = mapped = 0
    for i, res in enumerate(results):
        strand, segl = res[0], res[4]
        cnt = len(segl) if strand and len(segl) else 1
        mine = body[at:at + cnt]
        at += cnt
        assert len(mine) == cnt and all(f[0] == map_spec.cut_name(names[i]) for f in mine)
        n = len(letters[i])
        if not (strand and len(segl)):
            assert mine[0][1:9] == [b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0"] and mine[0][9] == bytes(letters[i])
            continue
        assert sum(1 for f in mine if not int(f[1]) & 2048) == 1
        for k, f in enumerate(mine):
            flag = int(f[1])
            assert (flag & 16 != 0) == (strand == 2) and flag & ~(16 | 2048) == 0
            r, ts = locate(int(segl[k][0]), ref)
            assert f[2] == map_spec.cut_name(ref.names[r]) and int(f[3]) == ts + 1
            assert f[6:9] == [b"*", b"0", b"0"]
            qlen, nm = replay_line(f, records)
            tags = dict((t[:2], t[5:]) for t in f[11:])
            assert int(tags[b"NM"]) == nm
            assert qlen == len(f[9]) == n and (f[10] == b"*" or len(f[10]) == n)
            given = bytes(letters[i])
            if strand == 2:
                assert f[9] == bytes(ext_spec.revcomp(np.frombuffer(given, dtype=np.uint8)))
            else:
                assert f[9] == given
            if quals is not None:
                assert f[10] == (bytes(quals[i])[::-1] if strand == 2 else bytes(quals[i]))
            others = [(g[2], g[3], b"-" if int(g[1]) & 16 else b"+", g[5], g[4], dict((t[:2], t[5:]) for t in g[11:])[b"NM"])
                      for j, g in enumerate(mine) if j != k]
            if cnt > 1:
                sa = [tuple(e.split(b",")) for e in tags[b"SA"].split(b";")[:-1]]
                assert tags[b"SA"].endswith(b";") and sa == others
            else:
                assert b"SA" not in tags
            mapped += 1
    assert at == len(body)
    return mapped
