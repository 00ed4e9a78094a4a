"""-gext on the checker side: the gapped X-drop extension of a block's two outer ends, straight from the definition of DESIGN.md
4.30.  Everything but the ends is affine_spec's (and through it aln_spec's) and is taken from there, not restated.

One end, to the right of the chain's last anchor, which ends at (eq, ep); the left end is the mirror image on reversed pieces.
P and X are -pen and -xdrop, o and e the gap costs of -affine, Z the band (-gext).

  pieces    A = Q from eq up to the first letter that is not A,C,G,T or the strand's end (a letters); B the same of T from ep,
            cut to a + Z letters (b letters)
  score     S = matches - P mismatches - sum over gap runs (o + e L)
  penalty   with k = y - x and the gap-affine penalty p at costs x' = 2P + 2, o' = 2o, e' = 2e + 1: 2S = x + y - p
  attempt   scores s = 0 .. Cp of 4.29's wavefronts M, I, D over p on the diagonals |k| <= Z; a cell whose start x0 (before the
            slide) has best2 - (2 x0 + k - s) > 2X is dead; best2 = the largest 2 M + k - s over the scores below, updated
            after each score in the order k = 0, -1, +1, -2, .. and only when strictly greater; the attempt ends when a score
            and the max(x', o' + e') scores before it hold no live cell
  choice    the attempt's result iff its score is strictly greater than the score of 4.13's ungapped side, else that side

attempt() is the wavefront form (the definition, and a model of what the kernel stores and reads); matrix_attempt() is the
plain banded Gotoh matrix with a free end, which it equals when nothing is pruned.  Python integers: no overflow."""
import contextlib

import numpy as np

import affine_spec
import aln_spec
import chain_spec
import ext_spec

COST_MAX = 512  # Cp: kAlnMaxCost
BAND_MAX = 31
_INF = 1 << 40


def penalty_costs(P: int, costs):
    """(x', o', e') of the penalty p with 2S = x + y - p"""
    _, o, e = costs
    return 2 * P + 2, 2 * o, 2 * e + 1


def score_of(ops: str, P: int, costs) -> int:
    """S of an operation string as the definition charges it."""
    _, o, e = costs
    s, last = 0, ""
    for ch in ops:
        if ch == "=":
            s += 1
        elif ch == "X":
            s -= P
        else:
            s -= e + (o if ch != last else 0)
        last = ch
    return s


def piece(S: bytes, at: int, step: int, limit=None) -> bytes:
    """The letters of S from `at` on in direction `step`, up to the first that is not A,C,G,T or the sequence's end, at most
    `limit`; case folded, in the order they are met."""
    out = bytearray()
    while 0 <= at < len(S) and (limit is None or len(out) < limit):
        c = S[at] & 0xDF
        if c not in ext_spec._ACGT:
            break
        out.append(c)
        at += step
    return bytes(out)


def pieces(Q: bytes, T: bytes, qi: int, ti: int, step: int, Z: int):
    A = piece(Q, qi, step)
    return A, piece(T, ti, step, len(A) + Z)


# ---- the wavefront form --------------------------------------------------------------------------------------------------------

def attempt(A: bytes, B: bytes, Z: int, P: int, X: int, costs, cost_max: int = COST_MAX, info=None):
    """(x, y, operations from the anchor outwards, score S, penalty s) of the best cell; the empty end is (0, 0, '', 0, 0).
    X None: nothing is pruned.  info (a dict) takes 'scores' (the last score processed), 'hit_cost_max', and 'tracebacks'
    [(x, y, s)]."""
    xp, op, ep = penalty_costs(P, costs)
    O = op + ep
    a, b = len(A), len(B)
    back = max(xp, O)

    def kmax(sp):
        return 0 if sp < O else min(Z, (sp - op) // ep)

    slab = []

    def held(sp, k):
        return 0 <= sp < len(slab) and slab[sp] is not None and -kmax(sp) <= k <= kmax(sp)

    def get(sp, k, comp):
        return slab[sp][k][comp] if held(sp, k) else -1

    def slide(c, k):
        while c < a and c + k < b and A[c] == B[c + k]:
            c += 1
        return c
    if X is None:  # no in-band cell costs more: min(a, b) diagonal steps and one gap reach it; later scores hold clamped cells only
        cost_max = min(cost_max, min(a, b) * xp + op + ep * Z)
    best2, best, last_live, s = 0, (0, 0, 0), 0, 0
    for s in range(cost_max + 1):
        if s - last_live > back:
            s -= 1
            break
        if not (s == 0 or any(sp >= 0 and slab[sp] is not None for sp in (s - xp, s - O, s - ep))):
            slab.append(None)
            continue
        cur, live = {}, False
        for k in range(-kmax(s), kmax(s) + 1):
            ci = cd = c = -1
            if s == 0:
                c = 0
            else:
                src = max(get(s - O, k + 1, 0), get(s - ep, k + 1, 1))
                if src >= 0:
                    v = min(src + 1, a)
                    if v - 1 >= max(0, -k - 1):
                        ci = v
                src = max(get(s - O, k - 1, 0), get(s - ep, k - 1, 2))
                if src >= 0:
                    v = min(src, b - k)
                    if v >= max(0, 1 - k):
                        cd = v
                fk = get(s - xp, k, 0)
                if fk >= 0:
                    c = min(fk + 1, a, b - k)
                c = max(c, ci, cd)
            if c >= 0 and X is not None and best2 - (2 * c + k - s) > 2 * X:
                c = ci = cd = -1  # dead
            if c >= 0:
                c = slide(c, k)
                live = True
            cur[k] = (c, ci, cd)
        slab.append(cur if live else None)
        if live:
            last_live = s
            nb2, nb = best2, None
            for k in sorted(cur, key=lambda k: (abs(k), k)):
                c = cur[k][0]
                if c >= 0 and 2 * c + k - s > nb2:
                    nb2, nb = 2 * c + k - s, (c, k, s)
            if nb is not None:
                best2, best = nb2, nb
    if info is not None:
        info["scores"] = s
        info["hit_cost_max"] = s >= cost_max and s - last_live <= back
    x, k, sc = best
    if x == 0 and k == 0 and sc == 0:
        return 0, 0, "", 0, 0
    # 4.29's traceback from the stored points, started at the best cell
    i, j, s0, state = x, x + k, sc, "H"
    ops = []
    while i > 0 or j > 0:
        k = j - i
        if state == "H":
            if i > 0 and j > 0 and A[i - 1] == B[j - 1]:
                ops.append("=")
                i, j = i - 1, j - 1
                continue
            m = get(sc - xp, k, 0)
            if i > 0 and j > 0 and m >= 0 and m >= i - 1:
                ops.append("X")
                i, j, sc = i - 1, j - 1, sc - xp
            else:
                d = get(sc, k, 2)
                state = "D" if j > 0 and (i == 0 or (d >= 0 and d >= i)) else "I"
        elif state == "D":
            m = get(sc - O, k - 1, 0)
            ops.append("D")
            if m >= 0 and m >= i:
                sc, state = sc - O, "H"
            else:
                sc -= ep
            j -= 1
        else:
            m = get(sc - O, k + 1, 0)
            ops.append("I")
            if m >= 0 and m >= i - 1:
                sc, state = sc - O, "H"
            else:
                sc -= ep
            i -= 1
        assert sc >= 0 and i >= 0 and j >= 0
    assert sc == 0
    ops = "".join(reversed(ops))
    assert best2 % 2 == 0 and 2 * score_of(ops, P, costs) == best2 == x + (x + best[1]) - s0  # 2S = x + y - p
    return x, x + best[1], ops, best2 // 2, s0


# ---- the matrix form ------------------------------------------------------------------------------------------------------------

def banded_gotoh(A: bytes, B: bytes, Z: int, xp: int, op: int, ep: int):
    """(H, Dm, Im) of the penalty p over the cells |y - x| <= Z; the others hold a large value."""
    a, b = len(A), len(B)
    H = [[_INF] * (b + 1) for _ in range(a + 1)]
    Dm = [[_INF] * (b + 1) for _ in range(a + 1)]
    Im = [[_INF] * (b + 1) for _ in range(a + 1)]
    H[0][0] = 0
    for i in range(a + 1):
        for j in range(max(0, i - Z), min(b, i + Z) + 1):
            if i == 0 and j == 0:
                continue
            if j > 0 and abs(j - 1 - i) <= Z:
                Dm[i][j] = min(H[i][j - 1] + op + ep, Dm[i][j - 1] + ep)
            if i > 0 and abs(j - i + 1) <= Z:
                Im[i][j] = min(H[i - 1][j] + op + ep, Im[i - 1][j] + ep)
            h = min(Dm[i][j], Im[i][j])
            if i > 0 and j > 0:
                h = min(h, H[i - 1][j - 1] + (xp if A[i - 1] != B[j - 1] else 0))
            H[i][j] = min(h, _INF)
    return H, Dm, Im


def matrix_attempt(A: bytes, B: bytes, Z: int, P: int, costs):
    """attempt() with nothing pruned and no bound on the cost, from the plain matrix: the cell that maximises x + y - H[x][y]
    (= 2S), among equals the smallest H, then the smallest |k|, then the negative k; affine_spec's traceback from there."""
    xp, op, ep = penalty_costs(P, costs)
    a, b = len(A), len(B)
    H, Dm, Im = banded_gotoh(A, B, Z, xp, op, ep)
    best = None
    for i in range(a + 1):
        for j in range(max(0, i - Z), min(b, i + Z) + 1):
            if H[i][j] >= _INF:
                continue
            k = j - i
            key = (-(i + j - H[i][j]), H[i][j], abs(k), k)
            if best is None or key < best[0]:
                best = (key, i, j)
    _, x, y = best
    if x == 0 and y == 0:
        return 0, 0, "", 0, 0
    i, j, state, ops = x, y, "H", []
    while i > 0 or j > 0:
        if state == "H":
            if i > 0 and j > 0 and H[i - 1][j - 1] + (xp if A[i - 1] != B[j - 1] else 0) == H[i][j]:
                ops.append("=" if A[i - 1] == B[j - 1] else "X")
                i, j = i - 1, j - 1
            elif j > 0 and Dm[i][j] == H[i][j]:
                state = "D"
            else:
                assert i > 0 and Im[i][j] == H[i][j]
                state = "I"
        elif state == "D":
            ops.append("D")
            if H[i][j - 1] + op + ep == Dm[i][j]:
                state = "H"
            j -= 1
        else:
            ops.append("I")
            if H[i - 1][j] + op + ep == Im[i][j]:
                state = "H"
            i -= 1
    return x, y, "".join(reversed(ops)), (x + y - H[x][y]) // 2, H[x][y]


# ---- an end ---------------------------------------------------------------------------------------------------------------------

def inline_keeps(a: int, ungapped_score: int, costs) -> bool:
    """Fact (c): an attempt that beats the ungapped side holds a gap, so it scores at most a - (o + e); k_aln_geom keeps the
    ungapped side without listing the end when that side scores at least as much."""
    return ungapped_score >= a - (costs[1] + costs[2])


def end_ops(Q: bytes, T: bytes, qi: int, ti: int, step: int, Z: int, P: int, X: int, costs, info=None):
    """One outer end from the first letters looked at, Q[qi] and T[ti]: (query letters, text letters, edits, operations from the
    anchor outwards, replaced).  Z = 0 with no costs: 4.13's side."""
    ext, score, mm = ext_spec.extend_side(Q, T, qi, ti, step, P, X)
    keep = (ext, ext, mm, aln_spec._diag_ops(Q, T, qi if step > 0 else qi - ext + 1, ti if step > 0 else ti - ext + 1, ext)[::step],
            False)
    if not Z or costs is None:
        return keep
    A, B = pieces(Q, T, qi, ti, step, Z)
    if info is not None:
        info.update(a=len(A), b=len(B), ungapped=score, listed=not inline_keeps(len(A), score, costs))
    x, y, ops, S, s = attempt(A, B, Z, P, X, costs, info=info)
    if info is not None:
        info["gapped"] = S
    if S <= score:
        return keep
    assert not inline_keeps(len(A), score, costs) and ("I" in ops or "D" in ops)  # fact (c)
    return x, y, affine_spec.edits_of(ops), ops, True


# ---- a block --------------------------------------------------------------------------------------------------------------------

def block_aln(rows, Q, T, G: int = chain_spec.DEFAULT_GAP, P: int = ext_spec.DEFAULT_PENALTY, X: int = ext_spec.DEFAULT_XDROP,
              E: int = aln_spec.DEFAULT_EDITS, costs=affine_spec.DEFAULT_COSTS, Z: int = 0, gaps_out=None, ends_out=None):
    """affine_spec.block_aln with the two outer ends by end_ops; ends_out takes an info dict per end ('side', 'replaced', ..)."""
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
            g = aln_spec.gap_ops(A, B, E) if costs is None else affine_spec.gap_ops(A, B, E, costs)
            if gaps_out is not None:
                gaps_out.append((A, B, g))
            if g is not None:
                s = segs[-1]
                s[2], s[3], s[4], s[5] = p + ln, q + ln, s[4] + g[1], s[5] + g[0] + "=" * ln
                joined = True
        if not joined:
            segs.append([p, q, p + ln, q + ln, 0, "=" * ln])
    for side in (-1, +1):
        p, q, ln = chain[0] if side < 0 else chain[-1]
        info = {"side": side}
        if side < 0:
            x, y, ed, ops, rep = end_ops(Q, T, q - 1, p - 1, -1, Z, P, X, costs, info)
            s = segs[0]
            s[0], s[1], s[4], s[5] = s[0] - y, s[1] - x, s[4] + ed, ops[::-1] + s[5]
        else:
            x, y, ed, ops, rep = end_ops(Q, T, q + ln, p + ln, +1, Z, P, X, costs, info)
            s = segs[-1]
            s[2], s[3], s[4], s[5] = s[2] + y, s[3] + x, s[4] + ed, s[5] + ops
        info["replaced"] = rep
        info["ops"] = ops
        if ends_out is not None:
            ends_out.append(info)
    return [(s[0], s[1], s[2] - s[0], s[3] - s[1], s[4], aln_spec.runs(s[5])) for s in reversed(segs)]


def filter_blocks(mem, boff, ref, queries, offsets, both: bool, G: int = chain_spec.DEFAULT_GAP, P: int = ext_spec.DEFAULT_PENALTY,
                  X: int = ext_spec.DEFAULT_XDROP, E: int = aln_spec.DEFAULT_EDITS, costs=affine_spec.DEFAULT_COSTS, Z: int = 0,
                  ends_out=None):
    """The -aln -affine -gext result of a -mem result as the engine returns it: per-block segment lists."""
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
        out.append(block_aln(tri[boff[b]:boff[b + 1]], ext_spec.revcomp(rec) if b % strands else rec, T, G, P, X, E, costs, Z,
                             ends_out=ends_out))
    return out


@contextlib.contextmanager
def in_aln_spec(costs, Z: int):
    """Inside, aln_spec builds its blocks with block_aln above at these costs and this band, and with it every spec that is
    built on aln_spec's blocks (map_spec, pile_spec, events_spec and their files)."""
    was = aln_spec.block_aln
    aln_spec.block_aln = lambda rows, Q, T, G=chain_spec.DEFAULT_GAP, P=ext_spec.DEFAULT_PENALTY, X=ext_spec.DEFAULT_XDROP, \
        E=aln_spec.DEFAULT_EDITS, gaps_out=None: block_aln(rows, Q, T, G, P, X, E, costs, Z, gaps_out)
    try:
        yield
    finally:
        aln_spec.block_aln = was
