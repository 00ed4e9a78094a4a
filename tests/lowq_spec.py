"""Base quality on the checker side: the low-quality mask of a batch, the pileup with a mask, and a FASTQ reader,
each straight from its definition.  Builds on pile_spec (the walk of a read's segments), ext_spec (letters, reverse complement)
and restates neither.

The mask is a bit array over the batch's letter buffer: bit j (bit j % 64 of word j // 64 of a uint64 array) belongs to
queries[j], so bit offsets[r] + i belongs to letter i of read r AS GIVEN.  With a mask, pile_spec's rule changes in one place: under
= or X a letter whose bit is set counts nowhere (the row gets nothing from this read).  On strand 2 the scanned strand's letter q
is the given letter len - 1 - q and has that letter's bit.  D and I are as without a mask.

Letter j is low iff max(0, qual[j] - phred_offset) < min_bq.

A FASTQ file: its lines are what "\\n" separates (a final "\\n" ends the last line and starts none; one "\\r" at a line's end is
dropped); they come in records of four -- "@" and the name, the letters, a line that starts with "+", as many quality bytes as the
second line has letter bytes.  Anything else is invalid.  The letters are normalised as FASTA letters are (A, C, G, T of either
case to upper case; any other letter to N, or dropped with acgt_only; everything else dropped), and a dropped letter takes its
quality byte with it; empty records and records shorter than min_len are dropped, as for FASTA."""
import numpy as np

import ext_spec
import pile_spec

_COL = {ord(c): k for k, c in enumerate("ACGT")}


# ---- the mask ------------------------------------------------------------------------------------------------------------------

def pack(quals, min_bq: int, phred_offset: int = 33) -> np.ndarray:
    """(len + 63) // 64 uint64 words: bit j set iff letter j is low; the last word's unused bits are 0."""
    q = np.frombuffer(quals, dtype=np.uint8) if isinstance(quals, (bytes, bytearray)) else np.asarray(quals, dtype=np.uint8)
    out = [0] * ((len(q) + 63) // 64)
    for j, v in enumerate(q.tolist()):
        if max(0, v - phred_offset) < min_bq:
            out[j // 64] |= 1 << (j % 64)
    return np.array(out, dtype=np.uint64)


def from_bits(bits) -> np.ndarray:
    """The words of a 0/1 value per letter."""
    out = [0] * ((len(bits) + 63) // 64)
    for j, b in enumerate(bits):
        if b:
            out[j // 64] |= 1 << (j % 64)
    return np.array(out, dtype=np.uint64)


def bit(mask, j: int) -> int:
    return (int(mask[j // 64]) >> (j % 64)) & 1


# ---- the pileup with a mask ----------------------------------------------------------------------------------------------------

def add_read(table: np.ndarray, result, read, low, min_mapq: int = 0) -> bool:
    """pile_spec.add_read with low[i] (0/1) for letter i of the read as given; low None: pile_spec.add_read."""
    if low is None:
        return pile_spec.add_read(table, result, read, min_mapq)
    strand, mapq, _, _, segl = result
    if strand == 0 or mapq < min_mapq:
        return False
    n = table.shape[0]
    rec = np.frombuffer(ext_spec._letters(read), dtype=np.uint8)
    L = len(rec)
    assert len(low) == L
    Q = bytes(ext_spec.revcomp(rec)) if strand == 2 else bytes(rec)
    for (p, q, _rlen, _qlen, _ed, rl) in segl:
        p, q = int(p), int(q)
        for c, k in rl:
            k = int(k)
            if c in "=X":
                for _ in range(k):
                    given = L - 1 - q if strand == 2 else q
                    col = _COL.get(Q[q] & 0xDF)
                    if col is not None and not low[given]:
                        table[p, col] += 1
                    p += 1
                    q += 1
            elif c == "D":
                table[p:p + k, 4] += 1
                p += k
            elif c == "I":
                if p < n:
                    table[p, 5] += 1
                q += k
            else:
                raise ValueError("operation %r" % c)
    return True


def pile(results, queries, offsets, n: int, mask, min_mapq: int = 0, table=None) -> np.ndarray:
    """The table of a batch with its mask (uint64 words indexed as queries; None: no mask)."""
    table = pile_spec.empty(n) if table is None else table
    q = np.frombuffer(queries, dtype=np.uint8) if isinstance(queries, (bytes, bytearray)) else np.asarray(queries, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.int64)
    assert len(results) == len(off) - 1
    for r, res in enumerate(results):
        a, b = int(off[r]), int(off[r + 1])
        low = None if mask is None else [bit(mask, j) for j in range(a, b)]
        add_read(table, res, q[a:b], low, min_mapq)
    return table


# ---- FASTQ ---------------------------------------------------------------------------------------------------------------------

class InvalidFastq(ValueError):
    pass


def _normalise(letters: bytes, quals: bytes, acgt_only: bool):
    out_l, out_q = bytearray(), bytearray()
    for c, v in zip(letters, quals):
        u = c & 0xDF
        if u in b"ACGT" and (65 <= c <= 90 or 97 <= c <= 122):
            out_l.append(u)
        elif (65 <= c <= 90 or 97 <= c <= 122) and not acgt_only:
            out_l.append(ord("N"))
        else:
            continue
        out_q.append(v)
    return bytes(out_l), bytes(out_q)


def read_fastq(data: bytes, acgt_only: bool = False, min_len: int = 0):
    """(names, letters, quals) per kept record of a FASTQ file's bytes; raises InvalidFastq."""
    if not data.startswith(b"@"):
        raise InvalidFastq("no '@' at the start")
    lines = data.split(b"\n")
    if data.endswith(b"\n"):
        lines.pop()
    lines = [l[:-1] if l.endswith(b"\r") else l for l in lines]
    if len(lines) % 4:
        raise InvalidFastq("%d lines" % len(lines))
    names, letters, quals = [], [], []
    for k in range(0, len(lines), 4):
        head, seq, plus, ql = lines[k:k + 4]
        if not head.startswith(b"@") or not plus.startswith(b"+") or len(seq) != len(ql):
            raise InvalidFastq("record %d" % (k // 4))
        l, v = _normalise(seq, ql, acgt_only)
        if len(l) == 0 or (min_len and len(l) < min_len):
            continue
        names.append(head[1:])
        letters.append(l)
        quals.append(v)
    return names, letters, quals


def write_fastq(records, eol: bytes = b"\n", final_newline: bool = True) -> bytes:
    """records: (name, letters, quals) -> the file's bytes."""
    out = eol.join(b"@" + n + eol + bytes(l) + eol + b"+" + eol + bytes(v) for n, l, v in records)
    return out + (eol if final_newline else b"")
