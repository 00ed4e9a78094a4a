"""The definition of -stats in Python, letter by letter, with no cleverness: the table of a batch of mappings,
and the text of the report.  A mapping is a read_map-style tuple (strand, mapq, s1, s2, segments), a segment (ref_pos, query_pos,
ref_len, query_len, edits, [(op, n), ...]) in the coordinates of the scanned strand -- what map_spec.read_map gives and what
test_gpu_sam.results_of makes of an engine result."""
import math

import numpy as np

SECTIONS = {"totals": (0, 24), "mapq": (24, 64), "len": (88, 512), "nm": (600, 128), "cyc_aln": (728, 512), "cyc_mm": (1240, 512),
            "cyc_ins": (1752, 512), "cyc_del": (2264, 512), "sub": (2776, 16), "q_aln": (2792, 96), "q_mm": (2888, 96),
            "ins_len": (2984, 64), "del_len": (3048, 64)}
WORDS = 3112
TOTALS = ("reads", "mapped", "forward", "reverse", "counted", "counted split", "segments", "letters", "counted letters", "matches",
          "mismatches", "insertions", "inserted letters", "deletions", "deleted letters", "segment letters")
_CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
_FOLDS = {"len", "nm", "cyc_aln", "cyc_mm", "cyc_ins", "cyc_del", "ins_len", "del_len"}


def _code(byte: int):
    return _CODE.get(int(byte) & 0xDF)


def table(results, text_letters, queries, offsets, quals=None, phred_offset: int = 33, min_mapq: int = 0) -> np.ndarray:
    """The table of one batch: a uint64 array of WORDS.  text_letters: the reference as the index holds it; queries, offsets: the
    reads as given; quals: a byte per letter, indexed as queries is, or None."""
    t = [0] * WORDS
    T = text_letters if isinstance(text_letters, (bytes, bytearray)) else bytes(np.asarray(text_letters, dtype=np.uint8))
    Q = queries if isinstance(queries, (bytes, bytearray)) else bytes(np.asarray(queries, dtype=np.uint8))
    B = None if quals is None else (quals if isinstance(quals, (bytes, bytearray)) else bytes(np.asarray(quals, dtype=np.uint8)))

    def add(section, k, v=1):
        first, words = SECTIONS[section]
        t[first + min(int(k), words - 1)] += v

    def tot(name, v=1):
        t[TOTALS.index(name)] += v

    assert len(results) == len(offsets) - 1
    for r, (strand, mapq, _s1, _s2, segs) in enumerate(results):
        o, n = int(offsets[r]), int(offsets[r + 1]) - int(offsets[r])
        tot("reads")
        tot("letters", n)
        add("len", n)
        if strand == 0:
            continue
        tot("mapped")
        tot("forward" if strand == 1 else "reverse")
        add("mapq", mapq)
        if mapq < min_mapq:
            continue
        tot("counted")
        tot("counted split", 1 if len(segs) > 1 else 0)
        tot("segments", len(segs))
        tot("counted letters", n)
        tot("segment letters", sum(s[3] for s in segs))
        add("nm", sum(s[4] for s in segs))

        def given(x):  # the index in the read as given of letter x of the scanned strand: its cycle
            assert 0 <= x < n
            return x if strand == 1 else n - 1 - x

        def letter(x):  # letter x of the scanned strand, 0..3 or None
            c = _code(Q[o + given(x)])
            return c if c is None or strand == 1 else 3 - c

        for p, q, _rl, _ql, _e, ops in segs:
            for op, k in ops:
                if op in "=X":
                    for j in range(k):
                        add("cyc_aln", given(q + j))
                        if op == "X":
                            add("cyc_mm", given(q + j))
                        if B is not None:
                            qv = min(93, max(0, B[o + given(q + j)] - phred_offset))
                            add("q_aln", qv)
                            if op == "X":
                                add("q_mm", qv)
                        if op == "X":
                            a, b = _code(T[p + j]), letter(q + j)
                            if a is not None and b is not None:
                                add("sub", 4 * a + b)
                    tot("matches" if op == "=" else "mismatches", k)
                    p += k
                    q += k
                elif op == "I":
                    tot("insertions")
                    tot("inserted letters", k)
                    add("ins_len", k)
                    for j in range(k):
                        add("cyc_ins", given(q + j))
                    q += k
                elif op == "D":
                    tot("deletions")
                    tot("deleted letters", k)
                    add("del_len", k)
                    add("cyc_del", given(q))  # (a deletion has a letter of the scanned strand behind it)
                    p += k
                else:
                    raise AssertionError(op)
    return np.array(t, dtype=np.uint64)


def report(tab) -> str:
    """The text of the -stats file for a table."""
    t = [int(v) for v in tab]
    assert len(t) == WORDS
    out = [f"SN\t{name}\t{t[k]}" for k, name in enumerate(TOTALS)]
    aligned = t[9] + t[10]
    out.append(f"SN\tclipped letters\t{max(t[8] - t[15], 0)}")
    out.append("SN\tmismatch rate\t%.6f" % (t[10] / aligned if aligned else 0.0))
    out.append("SN\tindel rate\t%.6f" % ((t[11] + t[13]) / aligned if aligned else 0.0))

    def num(section, i):
        return f"{i}+" if section in _FOLDS and i == SECTIONS[section][1] - 1 else str(i)

    for tag, section in (("MQ", "mapq"), ("RL", "len"), ("NM", "nm")):
        first, words = SECTIONS[section]
        out += [f"{tag}\t{num(section, i)}\t{t[first + i]}" for i in range(words) if t[first + i]]
    for i in range(512):
        row = [t[SECTIONS[s][0] + i] for s in ("cyc_aln", "cyc_mm", "cyc_ins", "cyc_del")]
        if any(row):
            out.append("CY\t" + num("cyc_aln", i) + "\t" + "\t".join(str(v) for v in row))
    out += [f"SU\t{'ACGT'[i >> 2]}\t{'ACGT'[i & 3]}\t{t[2776 + i]}" for i in range(16) if t[2776 + i]]
    for i in range(96):
        a, m = t[2792 + i], t[2888 + i]
        if a or m:
            out.append("BQ\t%d\t%d\t%d\t%.2f" % (i, a, m, -10.0 * math.log10((m + 1) / (a + 2))))
    for tag, section in (("IL", "ins_len"), ("DL", "del_len")):
        first, words = SECTIONS[section]
        out += [f"{tag}\t{num(section, i)}\t{t[first + i]}" for i in range(words) if t[first + i]]
    return "\n".join(out) + "\n"


def reports_equal(got: str, want: str, tol: float = 0.011) -> bool:
    """Two reports are the same text, the `empirical` column of the BQ rows compared as numbers within tol."""
    a, b = got.split("\n"), want.split("\n")
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x.startswith("BQ\t") and y.startswith("BQ\t"):
            fx, fy = x.split("\t"), y.split("\t")
            if fx[:-1] != fy[:-1] or abs(float(fx[-1]) - float(fy[-1])) > tol:
                return False
        elif x != y:
            return False
    return True
