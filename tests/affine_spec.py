"""-affine on the checker side: the gaps between chain anchors closed at gap-affine cost, straight from the definition of
DESIGN.md 4.29, with three full Gotoh matrices per gap.  Everything but the gap is aln_spec's (anchors, trimming, breaks, outer
ends, run merging, block order) and is taken from there, not restated.

Costs: x per mismatch, o per gap opened, e per gap letter; a run of L inserted or deleted letters costs o + L e.  E is -maxed and
C = o + e E the bound on a gap's cost.

  matrices   H[x][y] the cost of A[:x], B[:y]; Dm the same when the last step is a text letter (D), Im when it is a strand
             letter (I); Python / int64
  closing    both pieces A,C,G,T only and H[a][b] <= C
  traceback  from (a, b) in state H, the first that applies: the diagonal step if H[x-1][y-1] + sub == H[x][y]; state D if
             Dm[x][y] == H[x][y]; else state I.  State D: emit D, go to (x, y-1); back to H if H[x][y-1] + o + e == Dm[x][y],
             else stay.  State I: emit I, go to (x-1, y); back to H if H[x-1][y] + o + e == Im[x][y], else stay
  edits      the X, I and D letters of the operations (NM), not the cost

wavefront_ops is a model of exactly what k_aln_wave_affine stores and reads."""
import contextlib

import numpy as np

import aln_spec
import chain_spec
import ext_spec
import mum_spec

DEFAULT_COSTS = (4, 6, 2)
COST_MAX = 512  # SLAMEM_ALN_COST_MAX
_INF = 1 << 40


def aln_word(E: int, costs=None) -> int:
    """SLAMEM_ALN_AFFINE"""
    if costs is None:
        return E
    x, o, e = costs
    return E | x << 8 | o << 16 | e << 24


def bound(E: int, costs) -> int:
    return costs[1] + costs[2] * E


def gotoh(A, B, x: int, o: int, e: int):
    """(H, Dm, Im), each (a + 1, b + 1) int64; cells that do not exist hold a large value."""
    A, B = aln_spec._fold(A), aln_spec._fold(B)
    a, b = len(A), len(B)
    H = np.full((a + 1, b + 1), _INF, dtype=np.int64)
    Dm = np.full((a + 1, b + 1), _INF, dtype=np.int64)
    Im = np.full((a + 1, b + 1), _INF, dtype=np.int64)
    idx = np.arange(b + 1, dtype=np.int64)
    H[0, 0] = 0
    if b:
        Dm[0, 1:] = o + e * idx[1:]
        H[0, 1:] = Dm[0, 1:]
    for i in range(1, a + 1):
        Im[i] = np.minimum(H[i - 1] + o + e, Im[i - 1] + e)
        h0 = Im[i].copy()
        if b:
            h0[1:] = np.minimum(h0[1:], H[i - 1, :-1] + np.where(B != A[i - 1], x, 0))
            # Dm[i][y] = min over y' < y of H[i][y'] + o + e (y - y'); a gap is never better opened behind a cell that Dm itself
            # decides (o >= 0), so the cells before Dm is looked at serve
            run = np.minimum.accumulate(h0 - e * idx)
            Dm[i, 1:] = np.minimum(run[:-1] + o + e * idx[1:], _INF)
        H[i] = np.minimum(np.minimum(h0, Dm[i]), _INF)
    return H, Dm, Im


def traceback(A, B, H, Dm, Im, x: int, o: int, e: int) -> str:
    A, B = aln_spec._fold(A), aln_spec._fold(B)
    i, j = len(A), len(B)
    ops, state = [], "H"
    while i > 0 or j > 0:
        if state == "H":
            if i > 0 and j > 0 and H[i - 1][j - 1] + (x if A[i - 1] != B[j - 1] else 0) == H[i][j]:
                ops.append("=" if A[i - 1] == B[j - 1] else "X")
                i, j = i - 1, j - 1
            elif j > 0 and Dm[i][j] == H[i][j]:
                state = "D"
            else:
                assert i > 0 and Im[i][j] == H[i][j]
                state = "I"
        elif state == "D":
            ops.append("D")
            if H[i][j - 1] + o + e == Dm[i][j]:
                state = "H"
            else:
                assert Dm[i][j - 1] + e == Dm[i][j]
            j -= 1
        else:
            ops.append("I")
            if H[i - 1][j] + o + e == Im[i][j]:
                state = "H"
            else:
                assert Im[i - 1][j] + e == Im[i][j]
            i -= 1
    return "".join(reversed(ops))


def edits_of(ops: str) -> int:
    return len(ops) - ops.count("=")


def cost_of(ops: str, x: int, o: int, e: int) -> int:
    """The cost of an operation string as the definition charges it."""
    c, last = 0, ""
    for ch in ops:
        if ch == "X":
            c += x
        elif ch in "ID":
            c += e + (o if ch != last else 0)
        last = ch
    return c


def gap_ops(A, B, E: int = aln_spec.DEFAULT_EDITS, costs=DEFAULT_COSTS):
    """(operations left to right, edits, cost) of a gap that closes, or None."""
    x, o, e = costs
    a, b = len(A), len(B)
    if not aln_spec.all_acgt(A) or not aln_spec.all_acgt(B) or abs(a - b) > E:
        return None
    H, Dm, Im = gotoh(A, B, x, o, e)
    if H[a][b] > o + e * E:
        return None
    ops = traceback(A, B, H, Dm, Im, x, o, e)
    return ops, edits_of(ops), int(H[a][b])


# ---- the wavefront form: what the kernel evaluates ---------------------------------------------------------------------------

def wavefronts(A, B, E: int, costs):
    """The kernel's slab: per score s <= C a dict k -> (M, I, D) over |k| <= kmax(s), or None for a score that is skipped
    (none of its sources s - x, s - o - e, s - e holds a cell).  Returns (slab, kmax, s) with s the first score that reaches
    (a, b), or None when C does not."""
    x, o, e = costs
    A, B = aln_spec._fold(A), aln_spec._fold(B)
    a, b = len(A), len(B)
    C, O = o + e * E, o + e

    def kmax(sp):
        return 0 if sp < O else min(E, (sp - o) // e)

    slab = []

    def held(sp, k):
        return 0 <= sp <= C and slab[sp] is not None and -kmax(sp) <= k <= kmax(sp)

    def get(sp, k, comp):
        return slab[sp][k][comp] if held(sp, k) else -1

    def slide(c, k):
        while c < a and c + k < b and A[c] == B[c + k]:
            c += 1
        return c
    for s in range(C + 1):
        if not (s == 0 or any(sp >= 0 and slab[sp] is not None for sp in (s - x, s - O, s - e))):
            slab.append(None)
            continue
        cur, live = {}, False
        for k in range(-kmax(s), kmax(s) + 1):
            ci = cd = c = -1
            if s == 0:
                c = 0
            else:
                src = max(get(s - O, k + 1, 0), get(s - e, k + 1, 1))
                if src >= 0:
                    v = min(src + 1, a)
                    if v - 1 >= max(0, -k - 1):
                        ci = v
                src = max(get(s - O, k - 1, 0), get(s - e, k - 1, 2))
                if src >= 0:
                    v = min(src, b - k)
                    if v >= max(0, 1 - k):
                        cd = v
                fk = get(s - x, k, 0)
                if fk >= 0:
                    c = min(fk + 1, a, b - k)
                c = max(c, ci, cd)
            if c >= 0:
                c = slide(c, k)
            cur[k] = (c, ci, cd)
            live = live or c >= 0 or ci >= 0 or cd >= 0
        slab.append(cur)
        fin = cur.get(b - a, (-1,))[0] >= a
        if not live:
            slab[s] = None
        if fin:
            return slab, held, s
    return slab, held, None


def wavefront_ops(A, B, E: int = aln_spec.DEFAULT_EDITS, costs=DEFAULT_COSTS):
    """gap_ops from the stored furthest-reaching points alone."""
    x, o, e = costs
    a, b = len(A), len(B)
    if not aln_spec.all_acgt(A) or not aln_spec.all_acgt(B) or abs(a - b) > E:
        return None
    slab, held, s = wavefronts(A, B, E, costs)
    if s is None:
        return None
    A, B = aln_spec._fold(A), aln_spec._fold(B)
    O = o + e
    get = lambda sp, k, comp: slab[sp][k][comp] if held(sp, k) else -1
    i, j, sc, state = a, b, s, "H"
    ops = []
    while i > 0 or j > 0:
        k = j - i
        if state == "H":
            if i > 0 and j > 0 and A[i - 1] == B[j - 1]:
                ops.append("=")
                i, j = i - 1, j - 1
                continue
            m = get(sc - x, k, 0)
            if i > 0 and j > 0 and m >= 0 and m >= i - 1:
                ops.append("X")
                i, j, sc = i - 1, j - 1, sc - x
            else:
                d = get(sc, k, 2)
                state = "D" if j > 0 and (i == 0 or (d >= 0 and d >= i)) else "I"
        elif state == "D":
            m = get(sc - O, k - 1, 0)
            ops.append("D")
            if m >= 0 and m >= i:
                sc, state = sc - O, "H"
            else:
                sc -= e
            j -= 1
        else:
            m = get(sc - O, k + 1, 0)
            ops.append("I")
            if m >= 0 and m >= i - 1:
                sc, state = sc - O, "H"
            else:
                sc -= e
            i -= 1
        assert sc >= 0 and i >= 0 and j >= 0
    ops = "".join(reversed(ops))
    return ops, edits_of(ops), s


def inline_rule(m: int, n: int, E: int, costs):
    """What k_aln_geom decides itself for pieces of one length n <= 64 without a bad letter whose differing letters are the
    bits of m: ('closed', operations, edits), ('broken',) or ('listed',)."""
    x, o, e = costs
    d = bin(m).count("1")
    if d > 2 * (o + e) // x:
        return ("listed",)
    if d * x > o + e * E:
        return ("broken",)
    return ("closed", "".join("X" if (m >> t) & 1 else "=" for t in range(n)), d)


# ---- a block -----------------------------------------------------------------------------------------------------------------

def block_aln(rows, Q, T, G: int = chain_spec.DEFAULT_GAP, P: int = ext_spec.DEFAULT_PENALTY, X: int = ext_spec.DEFAULT_XDROP,
              E: int = aln_spec.DEFAULT_EDITS, costs=DEFAULT_COSTS, gaps_out=None):
    """aln_spec.block_aln with the gap closed by gap_ops above; costs None: aln_spec's own (unit cost).  gaps_out takes
    (A, B, result) of every gap."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    if len(rows) == 0:
        return []
    Q, T = ext_spec._letters(Q), ext_spec._letters(T)
    keep, _ = chain_spec.block_chain(rows, G, windowed=len(rows) > 200)
    chain = sorted((tuple(int(v) for v in r) for r in rows[keep]), key=lambda r: r[1])
    anc = aln_spec.anchors(chain)
    segs = []  # [p0, q0, p1, q1, edits, ops]
    for i, (p, q, ln) in enumerate(anc):
        joined = False
        if i:
            pj, qj, lj = chain[i - 1]
            A, B = Q[qj + lj:q], T[pj + lj:p]
            g = aln_spec.gap_ops(A, B, E) if costs is None else gap_ops(A, B, E, costs)
            if gaps_out is not None:
                gaps_out.append((A, B, g))
            if g is not None:
                s = segs[-1]
                s[2], s[3], s[4], s[5] = p + ln, q + ln, s[4] + g[1], s[5] + g[0] + "=" * ln
                joined = True
        if not joined:
            segs.append([p, q, p + ln, q + ln, 0, "=" * ln])
    p, q, ln = chain[0]
    el, _, ml = ext_spec.extend_side(Q, T, q - 1, p - 1, -1, P, X)
    s = segs[0]
    s[0], s[1], s[4], s[5] = s[0] - el, s[1] - el, s[4] + ml, aln_spec._diag_ops(Q, T, q - el, p - el, el) + s[5]
    p, q, ln = chain[-1]
    er, _, mr = ext_spec.extend_side(Q, T, q + ln, p + ln, +1, P, X)
    s = segs[-1]
    s[5] += aln_spec._diag_ops(Q, T, s[3], s[2], er)
    s[2], s[3], s[4] = s[2] + er, s[3] + er, s[4] + mr
    return [(s[0], s[1], s[2] - s[0], s[3] - s[1], s[4], aln_spec.runs(s[5])) for s in reversed(segs)]


def filter_blocks(mem, boff, ref, queries, offsets, both: bool, G: int = chain_spec.DEFAULT_GAP, P: int = ext_spec.DEFAULT_PENALTY,
                  X: int = ext_spec.DEFAULT_XDROP, E: int = aln_spec.DEFAULT_EDITS, costs=DEFAULT_COSTS, gaps_out=None):
    """The -aln -affine result of a -mem result as the engine returns it: per-block segment lists (aln_spec.pack gives the arrays)."""
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
        out.append(block_aln(tri[boff[b]:boff[b + 1]], ext_spec.revcomp(rec) if b % strands else rec, T, G, P, X, E, costs, gaps_out))
    return out


def golden_aln(case, G: int = chain_spec.DEFAULT_GAP, P: int = ext_spec.DEFAULT_PENALTY, X: int = ext_spec.DEFAULT_XDROP,
               E: int = aln_spec.DEFAULT_EDITS, costs=DEFAULT_COSTS, gaps_out=None):
    """aln_spec.golden_aln at these costs: (per-block segment lists, [(Q, T)] per block, reference, queries, options)."""
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
        out.append(block_aln(rows, Q, ref.chars, G, P, X, E, costs, gaps_out))
        seqs.append((Q, ext_spec._letters(ref.chars)))
    return out, seqs, ref, qs, opts


@contextlib.contextmanager
def in_aln_spec(costs):
    """Inside, aln_spec closes its gaps with gap_ops above at these costs, and with it every spec that is built on aln_spec's
    blocks (map_spec, pile_spec, events_spec and their files): the downstream definitions do not know the costs."""
    unit = aln_spec.gap_ops
    aln_spec.gap_ops = lambda A, B, E=aln_spec.DEFAULT_EDITS: gap_ops(A, B, E, costs)
    try:
        yield
    finally:
        aln_spec.gap_ops = unit


format_block = aln_spec.format_block  # the file's lines do not know the costs


def aln_file(names, blocks, ref, strands: int) -> bytes:
    return b"".join(format_block(names[b // strands], b % strands, segl, ref) for b, segl in enumerate(blocks))
