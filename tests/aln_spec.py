"""-aln on the checker side: the gapped alignment of a strand block's best chain straight from the definition of DESIGN.md
4.14, with a full edit-distance matrix per gap, and the filter applied to a -mem result or to a golden case's -mem file.  Builds
on chain_spec (which rows are the chain) and ext_spec (the outer ends); restates neither.

Rows are (p, q, L): p in the merged reference T, q in the scanned strand Q.  G is the chain's maximum gap, P and X the X-drop
rule's penalty and drop, E the most edits allowed in one gap.

  anchors   the chain's rows, q ascending; with j in front of i and o = max(0, eq_j - q_i, ep_j - p_i), i is (p+o, q+o, L-o)
  gap       A = Q[eq_j, q_i'), B = T[ep_j, p_i'); D = unit-cost edit distance, letters case-folded; closes iff A and B hold
            A,C,G,T only and D[a][b] <= E; traceback from (a, b): the diagonal step first (= or X), then D (a text letter),
            then I
  segments  maximal runs of anchors joined by closed gaps; the block's outer left and right ends extended by ext_spec's
            one-sided rule; ends at a break are not extended
  result    (ref_pos, query_pos, ref_len, query_len, edits) and the CIGAR, left to right, neighbouring runs merged; segments
            of a block with q descending

Python integers: no overflow."""
import numpy as np

import chain_spec
import ext_spec
import hostlib
import mum_spec

DEFAULT_EDITS = 31
OP_CODE = {"=": 7, "X": 8, "I": 1, "D": 2}  # BAM's codes
CODE_OP = {v: k for k, v in OP_CODE.items()}
_BIG = 1 << 30


def _fold(x) -> np.ndarray:
    return np.frombuffer(ext_spec._letters(x), dtype=np.uint8) & 0xDF


def all_acgt(x) -> bool:
    return bool(ext_spec._IS_ACGT[np.frombuffer(ext_spec._letters(x), dtype=np.uint8)].all())


def edit_matrix(A, B, band=None) -> np.ndarray:
    """D[x][y], the unit-cost edit distance of A[:x] and B[:y] (letters case-folded), one numpy row at a time.  band: cells
    with |y - x| > band + 1 are left at a large value -- no path of at most `band` edits visits them, so every cell of value
    <= band, and every comparison the traceback makes with such a value, is as in the full matrix."""
    A, B = _fold(A), _fold(B)
    a, b = len(A), len(B)
    D = np.full((a + 1, b + 1), _BIG, dtype=np.int64)
    idx = np.arange(b + 1, dtype=np.int64)
    lo, hi = 0, (b if band is None else min(b, band + 1))
    D[0, lo:hi + 1] = idx[lo:hi + 1]
    for x in range(1, a + 1):
        lo = 0 if band is None else max(0, x - band - 1)
        hi = b if band is None else min(b, x + band + 1)
        if lo > hi:
            break
        up = D[x - 1, lo:hi + 1] + 1
        diag = np.full(hi - lo + 1, _BIG, dtype=np.int64)
        s = max(lo, 1)
        diag[s - lo:] = D[x - 1, s - 1:hi] + (B[s - 1:hi] != A[x - 1])
        row = np.minimum(up, diag)
        # a text letter without a query letter: row[y] = min over y' <= y of row[y'] + (y - y')
        row = np.minimum.accumulate(row - idx[lo:hi + 1]) + idx[lo:hi + 1]
        D[x, lo:hi + 1] = np.minimum(row, _BIG)
    return D


def traceback(A, B, D) -> str:
    """The operations of the gap, left to right, by the rule of the definition."""
    A, B = _fold(A), _fold(B)
    x, y = len(A), len(B)
    ops = []
    while x > 0 or y > 0:
        if x > 0 and y > 0 and D[x - 1][y - 1] + (1 if A[x - 1] != B[y - 1] else 0) == D[x][y]:
            ops.append("=" if A[x - 1] == B[y - 1] else "X")
            x, y = x - 1, y - 1
        elif y > 0 and D[x][y - 1] + 1 == D[x][y]:
            ops.append("D")
            y -= 1
        else:
            assert x > 0 and D[x - 1][y] + 1 == D[x][y]
            ops.append("I")
            x -= 1
    return "".join(reversed(ops))


def gap_ops(A, B, E: int = DEFAULT_EDITS):
    """(operations left to right, distance) of a gap that closes, or None."""
    a, b = len(A), len(B)
    if not all_acgt(A) or not all_acgt(B) or abs(a - b) > E:
        return None
    D = edit_matrix(A, B, band=E)
    if D[a][b] > E:
        return None
    return traceback(A, B, D), int(D[a][b])


# ---- the wavefront form: what the kernel evaluates ---------------------------------------------------------------------------

def wavefronts(A, B, E: int):
    """f[s][k]: the largest x with D[x][x + k] <= s (k = y - x), or -1 when the diagonal has no such cell, for s = 0 .. the
    first s that reaches (a, b), at most E.  Returns (f as a list of dicts, s) or (f, None) when E edits do not reach."""
    A, B = _fold(A), _fold(B)
    a, b = len(A), len(B)

    def slide(x, k):
        while x < a and x + k < b and A[x] == B[x + k]:
            x += 1
        return x
    f = []
    for s in range(E + 1):
        cur = {}
        for k in range(-s, s + 1):
            c = -1
            if s == 0:
                c = 0
            else:
                prev = f[s - 1]
                fk, fl, fr = prev.get(k, -1), prev.get(k - 1, -1), prev.get(k + 1, -1)
                if fk >= 0:
                    c = min(fk + 1, a, b - k)
                if fl >= 0:
                    v = min(fl, b - k)
                    if v >= max(0, 1 - k) and v > c:
                        c = v
                if fr >= 0:
                    v = min(fr + 1, a)
                    if v - 1 >= max(0, -k - 1) and v > c:
                        c = v
            if c >= 0:
                c = slide(c, k)
            cur[k] = c
        f.append(cur)
        if cur.get(b - a, -1) >= a:
            return f, s
    return f, None


def wavefront_ops(A, B, E: int = DEFAULT_EDITS):
    """gap_ops from the furthest-reaching points alone: D[x][y] is the first s with f[s][y - x] >= x."""
    a, b = len(A), len(B)
    if not all_acgt(A) or not all_acgt(B) or abs(a - b) > E:
        return None
    f, s = wavefronts(A, B, E)
    if s is None:
        return None
    A, B = _fold(A), _fold(B)
    F = lambda sp, k: f[sp].get(k, -1) if sp >= 0 else -1
    x, y, d = a, b, s
    ops = []
    while x > 0 or y > 0:
        while x > 0 and y > 0 and A[x - 1] == B[y - 1]:
            ops.append("=")
            x, y = x - 1, y - 1
        if x == 0 and y == 0:
            break
        k = y - x
        if x > 0 and y > 0 and F(d - 1, k) >= x - 1 and F(d - 1, k) >= 0:
            ops.append("X")
            x, y = x - 1, y - 1
        elif y > 0 and (x == 0 or (F(d - 1, k - 1) >= x and F(d - 1, k - 1) >= 0)):
            ops.append("D")
            y -= 1
        else:
            ops.append("I")
            x -= 1
        d -= 1
    return "".join(reversed(ops)), s


# ---- a block -----------------------------------------------------------------------------------------------------------------

def runs(ops: str):
    """'==X=' -> [('=', 2), ('X', 1), ('=', 1)]"""
    out = []
    for c in ops:
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return [(c, n) for c, n in out]


def cigar_string(rl) -> str:
    return "".join("%d%s" % (n, c) for c, n in rl)


def _diag_ops(Q: bytes, T: bytes, q0: int, p0: int, n: int) -> str:
    return "".join("=" if (Q[q0 + t] & 0xDF) == (T[p0 + t] & 0xDF) else "X" for t in range(n))


def anchors(chain_rows):
    """The trimmed rows of a chain given q ascending."""
    out = []
    for r in chain_rows:
        p, q, ln = (int(v) for v in r)
        if out:
            pj, qj, lj = prev
            o = max(0, qj + lj - q, pj + lj - p)
            assert o < ln
            p, q, ln = p + o, q + o, ln - o
        prev = tuple(int(v) for v in r)
        out.append((p, q, ln))
    return out


def block_aln(rows, Q, T, G: int = chain_spec.DEFAULT_GAP, P: int = ext_spec.DEFAULT_PENALTY, X: int = ext_spec.DEFAULT_XDROP,
              E: int = DEFAULT_EDITS, gaps_out=None):
    """The segments of one block, q descending: [(ref_pos, query_pos, ref_len, query_len, edits, [(op, n), ...])].  gaps_out: a
    list that takes (A, B, result of gap_ops) of every gap."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    if len(rows) == 0:
        return []
    Q, T = ext_spec._letters(Q), ext_spec._letters(T)
    keep, _ = chain_spec.block_chain(rows, G, windowed=len(rows) > 200)
    chain = sorted((tuple(int(v) for v in r) for r in rows[keep]), key=lambda r: r[1])
    anc = anchors(chain)
    segs = []  # [p0, q0, p1, q1, edits, ops]
    for i, (p, q, ln) in enumerate(anc):
        joined = False
        if i:
            pj, qj, lj = chain[i - 1]
            A, B = Q[qj + lj:q], T[pj + lj:p]
            g = gap_ops(A, B, E)
            if gaps_out is not None:
                gaps_out.append((A, B, g))
            if g is not None:
                s = segs[-1]
                s[2], s[3], s[4], s[5] = p + ln, q + ln, s[4] + g[1], s[5] + g[0] + "=" * ln
                joined = True
        if not joined:
            segs.append([p, q, p + ln, q + ln, 0, "=" * ln])
    # the block's outer ends
    p, q, ln = chain[0]
    el, _, ml = ext_spec.extend_side(Q, T, q - 1, p - 1, -1, P, X)
    s = segs[0]
    s[0], s[1], s[4], s[5] = s[0] - el, s[1] - el, s[4] + ml, _diag_ops(Q, T, q - el, p - el, el) + s[5]
    p, q, ln = chain[-1]
    er, _, mr = ext_spec.extend_side(Q, T, q + ln, p + ln, +1, P, X)
    s = segs[-1]
    s[5] += _diag_ops(Q, T, s[3], s[2], er)
    s[2], s[3], s[4] = s[2] + er, s[3] + er, s[4] + mr
    return [(s[0], s[1], s[2] - s[0], s[3] - s[1], s[4], runs(s[5])) for s in reversed(segs)]


def pack(blocks):
    """Per-block segment lists -> what the engine returns: (segments (n, 5) int64, block offsets, ops uint32, op offsets)."""
    segs, boff, ops, ooff = [], [0], [], [0]
    for segl in blocks:
        for s in segl:
            segs.append(s[:5])
            ops.extend((n << 4) | OP_CODE[c] for c, n in s[5])
            ooff.append(len(ops))
        boff.append(len(segs))
    return (np.array(segs, dtype=np.int64).reshape(-1, 5), np.array(boff, dtype=np.int64), np.array(ops, dtype=np.uint32),
            np.array(ooff, dtype=np.int64))


def filter_blocks(mem, boff, ref, queries, offsets, both: bool, G: int = chain_spec.DEFAULT_GAP, P: int = ext_spec.DEFAULT_PENALTY,
                  X: int = ext_spec.DEFAULT_XDROP, E: int = DEFAULT_EDITS, gaps_out=None):
    """The -aln result of a -mem result as the engine returns it: per-block segment lists (pack() gives the arrays)."""
    tri = ext_spec._tri(mem)
    boff = np.asarray(boff, dtype=np.int64)
    T = ext_spec._letters(ref)
    q = np.frombuffer(queries, dtype=np.uint8) if isinstance(queries, (bytes, bytearray)) else np.asarray(queries, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.int64)
    strands = 2 if both else 1
    assert len(boff) - 1 == (len(off) - 1) * strands
    out = []
    for b in range(len(boff) - 1):
        rec = q[off[b // strands]:off[b // strands + 1]]
        out.append(block_aln(tri[boff[b]:boff[b + 1]], ext_spec.revcomp(rec) if b % strands else rec, T, G, P, X, E, gaps_out))
    return out


def golden_aln(case, G: int = chain_spec.DEFAULT_GAP, P: int = ext_spec.DEFAULT_PENALTY, X: int = ext_spec.DEFAULT_XDROP,
               E: int = DEFAULT_EDITS, gaps_out=None):
    """-aln of the file the real reference wrote for the -mem case: (per-block segment lists, [(Q, T)] per block, reference,
    queries, options)."""
    ref, qs, opts, exp_mems = mum_spec.golden_inputs(case)
    blocks = mum_spec.parse_mems_file(open(exp_mems, "rb").read(), ref)
    strands = 2 if "-b" in opts else 1
    assert len(blocks) == qs.n * strands
    chars = np.frombuffer(qs.chars, dtype=np.uint8)
    out, seqs = [], []
    for b, (_, rows) in enumerate(blocks):
        i, s = b // strands, b % strands
        rec = chars[qs.offsets[i]:qs.offsets[i + 1]]
        Q = bytes(ext_spec.revcomp(rec) if s else rec)
        out.append(block_aln(rows, Q, ref.chars, G, P, X, E, gaps_out))
        seqs.append((Q, ext_spec._letters(ref.chars)))
    return out, seqs, ref, qs, opts


def golden_aln_file(case, G: int = chain_spec.DEFAULT_GAP, P: int = ext_spec.DEFAULT_PENALTY, X: int = ext_spec.DEFAULT_XDROP,
                    E: int = DEFAULT_EDITS) -> bytes:
    """The -aln file of a golden case: golden_aln's segments formatted as the front end's writer does."""
    blocks, _, ref, qs, opts = golden_aln(case, G, P, X, E)
    strands = 2 if "-b" in opts else 1
    return b"".join(format_block(qs.names[b // strands], b % strands, segl, ref) for b, segl in enumerate(blocks))


# ---- a known answer that does not go through the definition -----------------------------------------------------------------

def constructed_reads(seed: int, count: int = 240, ref_len: int = 40000, read_len: int = 200):
    """Reads of read_len letters cut from a random reference over A,C,G,T, each with one kind of edit at places in
    [40, len - 40] at least 40 letters apart: 1-3 substitutions, or one inserted letter that differs from both neighbours, or one
    deleted letter that differs from both neighbours; every third read reverse-complemented.  Returns (reference, reads,
    offsets, [(block, (ref_pos, query_pos, ref_len, query_len, edits), cigar runs)]): the alignment written down from the
    construction, in the strand block where it is found."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = rng.choice(acgt, size=ref_len)
    reads, truth = [], []
    k = 0
    while len(reads) < count:
        a = int(rng.integers(0, ref_len - read_len - 1))
        kind = k % 3
        k += 1
        if kind == 0:
            r = ref[a:a + read_len].copy()
            places = []
            want = int(rng.integers(1, 4))
            for _ in range(200):
                if len(places) == want:
                    break
                x = int(rng.integers(40, read_len - 40))
                if all(abs(x - y) >= 40 for y in places):
                    places.append(x)
            places.sort()
            for x in places:
                r[x] = rng.choice(acgt[acgt != r[x]])
            rl, at = [], 0
            for x in places:
                rl += [("=", x - at), ("X", 1)]
                at = x + 1
            rl.append(("=", read_len - at))
            seg = (a, 0, read_len, read_len, len(places))
        elif kind == 1:  # an inserted letter at x: the read has it, the reference does not
            x = int(rng.integers(40, read_len - 40))
            src = ref[a:a + read_len - 1]
            choices = [c for c in acgt if c != src[x - 1] and c != src[x]]
            r = np.concatenate([src[:x], [choices[0]], src[x:]]).astype(np.uint8)
            rl = [("=", x), ("I", 1), ("=", read_len - x - 1)]
            seg = (a, 0, read_len - 1, read_len, 1)
        else:  # a deleted letter: reference letter a + x is missing from the read; it differs from both neighbours
            src = ref[a:a + read_len + 1]
            xs = [x for x in range(40, read_len - 40) if src[x] != src[x - 1] and src[x] != src[x + 1]]
            if not xs:
                continue
            x = xs[int(rng.integers(0, len(xs)))]
            r = np.concatenate([src[:x], src[x + 1:]]).astype(np.uint8)
            rl = [("=", x), ("D", 1), ("=", read_len - x)]
            seg = (a, 0, read_len + 1, read_len, 1)
        rev = len(reads) % 3 == 2
        reads.append(ext_spec.revcomp(r) if rev else r)
        truth.append((2 * (len(reads) - 1) + (1 if rev else 0), seg, rl))
    q = np.concatenate(reads)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return ref, q, off, truth


# ---- the output file ---------------------------------------------------------------------------------------------------------

def format_block(name: bytes, reverse: int, segl, ref) -> bytes:
    """A strand block of the -aln file: the -mem header, then ref_pos query_pos ref_len query_len edits cigar per segment."""
    out = [b">" + name + (b" Reverse" if reverse else b"") + b"\n"]
    starts = ref.merged_start
    for (p, q, rlen, qlen, ed, rl) in segl:
        line = b""
        if ref.s.num > 1:
            r = max(i for i in range(len(starts)) if starts[i] <= p)
            line = b" " + ref.names[r] + b"\t"
            p -= starts[r]
        line += b"%d\t%d\t%d\t%d\t%d\t%s" % (p + 1, q + 1, rlen, qlen, ed, cigar_string(rl).encode())
        out.append(line + b"\n")
    return b"".join(out)
