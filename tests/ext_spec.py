"""-ext on the checker side: the ungapped X-drop extension of a strand block's -mem rows straight from the definition of
DESIGN.md 4.13, letter by letter, and the filter applied to a -mem result or to a golden case's -mem file
(tests/golden/<case>/expected-mems.txt, written by the real reference).

Rows are (p, q, L): p in the merged reference T, q in the scanned strand Q (the record, or its reverse complement).  With the
mismatch penalty P >= 1 and the drop X >= 0, one side of a row:

  s = best = ext = 0
  for t = 0, 1, 2, ...:
      the letters are Q[q + L + t], T[p + L + t] to the right, Q[q - 1 - t], T[p - 1 - t] to the left
      stop when either index lies outside its sequence or either letter is not one of A,C,G,T (case folded)
      s += 1 when the letters are equal, s -= P when not
      if s > best: best = s, ext = t + 1
      if best - s > X: stop

The row becomes (p - extL, q - extL, extL + L + extR) with mm = the positions inside it whose letters differ.  A row is dropped
when an earlier row of its block (by index) gives the same (p, q, length); here that is a set of the triples seen so far, not
the emission order the engine relies on.  Python integers: no overflow."""
import numpy as np

import hostlib
import mum_spec

DEFAULT_PENALTY = 4
DEFAULT_XDROP = 20

_ACGT = frozenset(b"ACGT")
_COMP = np.full(256, ord("N"), dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCATGCA"):
    _COMP[_a] = _b


def revcomp(rec) -> np.ndarray:
    """The reverse strand as the engine scans it: A<->T, C<->G, everything else N."""
    return _COMP[np.asarray(rec, dtype=np.uint8)[::-1]]


def _letters(x) -> bytes:
    return x if isinstance(x, bytes) else bytes(np.asarray(x, dtype=np.uint8))


def extend_side(Q: bytes, T: bytes, qi: int, ti: int, step: int, P: int, X: int):
    """One side from the first letters looked at, Q[qi] and T[ti], moving by `step` (+1 right, -1 left):
    (ext, best score, mismatches among the ext letters)."""
    s = best = ext = mm = mm_best = 0
    t = 0
    while True:
        a, b = qi + step * t, ti + step * t
        if a < 0 or b < 0 or a >= len(Q) or b >= len(T):
            break
        x, y = Q[a] & 0xDF, T[b] & 0xDF
        if x not in _ACGT or y not in _ACGT:
            break
        if x == y:
            s += 1
        else:
            s -= P
            mm += 1
        if s > best:
            best, ext, mm_best = s, t + 1, mm
        if best - s > X:
            break
        t += 1
    return ext, best, mm_best


_IS_ACGT = np.zeros(256, dtype=bool)
for _a in b"ACGTacgt":
    _IS_ACGT[_a] = True


def extend_side_np(Q, T, qi: int, ti: int, step: int, P: int, X: int, chunk: int = 1 << 16):
    """extend_side for sides of a million letters (a genome pair), where a Python loop per letter would take hours: the same
    rule, still on letters, evaluated `chunk` letters at a time with numpy (scores by cumsum, the best so far by a running
    maximum).  Q, T: uint8 arrays.  tests/test_ext_host.py holds it to extend_side."""
    s = best = ext = mm_best = mm = done = 0
    while True:
        # the letters of this chunk: distances done .. done + n - 1
        if step > 0:
            n = min(chunk, len(Q) - (qi + done), len(T) - (ti + done))
            if n <= 0:
                break
            a, b = Q[qi + done:qi + done + n], T[ti + done:ti + done + n]
        else:
            n = min(chunk, qi - done + 1, ti - done + 1)
            if n <= 0:
                break
            a = Q[qi - done - n + 1:qi - done + 1][::-1]
            b = T[ti - done - n + 1:ti - done + 1][::-1]
        ok = _IS_ACGT[a] & _IS_ACGT[b]
        stop = int(np.argmin(ok)) if not ok.all() else n  # the first letter the rule does not look at
        eq = (a[:stop] & 0xDF) == (b[:stop] & 0xDF)
        sc = s + np.cumsum(np.where(eq, 1, -P))
        hi = np.maximum(np.maximum.accumulate(sc), best)
        over = np.flatnonzero(hi - sc > X)
        last = int(over[0]) + 1 if len(over) else stop  # letters of the chunk the rule takes
        if last:
            k = int(np.argmax(sc[:last]))
            if sc[k] > best:
                best, ext, mm_best = int(sc[k]), done + k + 1, mm + int((~eq[:k + 1]).sum())
            s = int(sc[last - 1])
            mm += int((~eq[:last]).sum())
        if len(over) or stop < n:
            break
        done += n
    return ext, best, mm_best


def extend_row(Q, T, row, P: int = DEFAULT_PENALTY, X: int = DEFAULT_XDROP, fast: bool = False):
    """((p', q', length'), mismatches) of one row.  fast: extend_side_np (Q, T as uint8 arrays) in place of extend_side."""
    p, q, ln = (int(v) for v in row)
    side = extend_side_np if fast else extend_side
    er, _, mr = side(Q, T, q + ln, p + ln, +1, P, X)
    el, _, ml = side(Q, T, q - 1, p - 1, -1, P, X)
    return (p - el, q - el, el + ln + er), ml + mr


def block_ext(rows, Q, T, P: int = DEFAULT_PENALTY, X: int = DEFAULT_XDROP, fast: bool = False):
    """The filter of one block: (kept extended rows as (k, 3) int64, their mismatches, the kept mask over `rows`)."""
    if fast:
        Q, T = np.frombuffer(_letters(Q), dtype=np.uint8), np.frombuffer(_letters(T), dtype=np.uint8)
    else:
        Q, T = _letters(Q), _letters(T)
    seen = set()
    out, mms, keep = [], [], []
    for row in np.asarray(rows, dtype=np.int64).reshape(-1, 3):
        seg, mm = extend_row(Q, T, row, P, X, fast)
        keep.append(seg not in seen)
        if seg not in seen:
            seen.add(seg)
            out.append(seg)
            mms.append(mm)
    return (np.array(out, dtype=np.int64).reshape(-1, 3), np.array(mms, dtype=np.int64), np.array(keep, dtype=bool))


def _tri(mems) -> np.ndarray:
    if hasattr(mems, "dtype") and mems.dtype.names:
        return np.stack([mems["ref_pos"], mems["query_pos"], mems["length"]], axis=1).astype(np.int64) if len(mems) else \
            np.zeros((0, 3), dtype=np.int64)
    return np.asarray(mems, dtype=np.int64).reshape(-1, 3)


def filter_blocks(mem, boff, ref, queries, offsets, both: bool, P: int = DEFAULT_PENALTY, X: int = DEFAULT_XDROP,
                  fast: bool = False):
    """The -ext filter of a -mem result as the engine returns it: (rows as (n, 3) int64, new block offsets, mismatches)."""
    tri = _tri(mem)
    boff = np.asarray(boff, dtype=np.int64)
    T = _letters(ref)
    q = np.frombuffer(queries, dtype=np.uint8) if isinstance(queries, (bytes, bytearray)) else np.asarray(queries, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.int64)
    strands = 2 if both else 1
    assert len(boff) - 1 == (len(off) - 1) * strands
    rows, mms, new = [], [], [0]
    for b in range(len(boff) - 1):
        rec = q[off[b // strands]:off[b // strands + 1]]
        k, m, _ = block_ext(tri[boff[b]:boff[b + 1]], revcomp(rec) if b % strands else rec, T, P, X, fast)
        rows.append(k)
        mms.append(m)
        new.append(new[-1] + len(k))
    return (np.concatenate(rows) if rows else np.zeros((0, 3), np.int64), np.array(new, dtype=np.int64),
            np.concatenate(mms) if mms else np.zeros(0, np.int64))


def format_block(name: bytes, reverse: int, rows, mms, ref) -> bytes:
    """A strand block of the output file in plain Python: the -mem lines (1-based; with several reference records ' <record>\\t'
    in front and the position inside the record of the row's first letter), and with mms a fourth column."""
    out = [b">" + name + (b" Reverse" if reverse else b"") + b"\n"]
    starts = ref.merged_start
    for k, (p, q, ln) in enumerate(np.asarray(rows, dtype=np.int64).reshape(-1, 3)):
        line = b""
        if ref.s.num > 1:
            r = max(i for i in range(len(starts)) if starts[i] <= p)
            line = b" " + ref.names[r] + b"\t"
            p -= starts[r]
        line += b"%d\t%d\t%d" % (p + 1, q + 1, ln)
        if mms is not None:
            line += b"\t%d" % int(mms[k])
        out.append(line + b"\n")
    return b"".join(out)


def golden_ext_file(case, P: int = DEFAULT_PENALTY, X: int = DEFAULT_XDROP):
    """The -ext filter of the file the real reference wrote for the -mem case.  Returns (expected -ext file bytes, per-block kept
    rows, per-block mismatches, reference, queries, options)."""
    ref, qs, opts, exp_mems = mum_spec.golden_inputs(case)
    data = open(exp_mems, "rb").read()
    blocks = mum_spec.parse_mems_file(data, ref)
    strands = 2 if "-b" in opts else 1
    assert len(blocks) == qs.n * strands
    chars = np.frombuffer(qs.chars, dtype=np.uint8)
    out, rows_kept, mms_kept = [], [], []
    for b, (_, rows) in enumerate(blocks):
        i, s = b // strands, b % strands
        rec = chars[qs.offsets[i]:qs.offsets[i + 1]]
        k, m, _ = block_ext(rows, revcomp(rec) if s else rec, ref.chars, P, X)
        rows_kept.append(k)
        mms_kept.append(m)
        out.append(format_block(qs.names[i], s, k, m, ref))
    return b"".join(out), rows_kept, mms_kept, ref, qs, opts


def planted_reads(seed: int, count: int = 300, ref_len: int = 40000, read_len: int = 200):
    """The known answer of DESIGN 4.13's test: a random reference over A,C,G,T and reads cut from it, every third one
    reverse-complemented, each with 0-4 substitutions at least 25 letters apart and at least 10 letters from either end (a
    planted letter differs from the one it replaces).  Returns (reference, reads, offsets, [(start in ref, reversed, planted)])."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = rng.choice(acgt, size=ref_len)
    reads, truth = [], []
    for k in range(count):
        a = int(rng.integers(0, ref_len - read_len + 1))
        r = ref[a:a + read_len].copy()
        want = int(rng.integers(0, 5))
        places = []
        for _ in range(200):
            if len(places) == want:
                break
            x = int(rng.integers(10, read_len - 10))
            if all(abs(x - y) >= 25 for y in places):
                places.append(x)
        for x in places:
            r[x] = rng.choice(acgt[acgt != r[x]])
        rev = k % 3 == 2
        reads.append(revcomp(r) if rev else r)
        truth.append((a, rev, len(places)))
    q = np.concatenate(reads)
    off = (np.arange(count + 1, dtype=np.uint64) * np.uint64(read_len))
    return ref, q, off, truth
