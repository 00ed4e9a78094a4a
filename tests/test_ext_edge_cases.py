"""The designed batches of tests/ext_edge_cases.py, checked with the oracle and tests/ext_spec.py alone (no GPU): every read has
exactly the -mem rows its design says, every distance, window bit, length, offset and block size the catalogue names is there,
the X-drop decisions fall as the designs intend, and the cases tell the rule from three wrong ones -- so that
tests/test_gpu_ext_edges.py compares the product on the edges it says it does."""
import functools

import numpy as np

import ext_edge_cases as ec
import ext_spec

W, L = ec.WINDOW, ec.EXT_LANE_MAX
ACGT = frozenset(b"ACGT")


def by_name(name):
    return next(d for d in ec.designs() if d.name == name)


@functools.lru_cache(maxsize=None)
def oracle_blocks(name: str, both: bool) -> tuple:
    """The -mem rows of a design's batch per strand block, in the oracle's (the emission) order: what check() of
    tests/test_gpu_seed.py holds the engine to."""
    from oracle import pyoracle as po
    d = by_name(name)
    q, off = d.arrays()
    om, obc = po.OracleIndex(d.ref.tobytes()).match_batch(q, off, ec.MIN_LEN, both)
    tri = np.stack([om["ref_pos"], om["query_pos"], om["length"]], axis=1).astype(np.int64).reshape(-1, 3)
    cuts = np.concatenate([[0], np.cumsum(obc.astype(np.int64))])
    return tuple(tri[cuts[b]:cuts[b + 1]] for b in range(len(obc)))


@functools.lru_cache(maxsize=None)
def spec_rows(name: str, P: int, X: int) -> tuple:
    """Per read of a design: {designed row: (right ext, left ext, mismatches)} by ext_spec.extend_side on the design strand."""
    d = by_name(name)
    b = d.batch(True, P, X)
    T = d.ref.tobytes()
    out = []
    for k, m in enumerate(d.meta):
        Q = ec.design_strand(b, k).tobytes()
        rows = {}
        for p, q, ln in m["rows"].tolist():
            er, _, mr = ext_spec.extend_side(Q, T, q + ln, p + ln, +1, P, X)
            el, _, ml = ext_spec.extend_side(Q, T, q - 1, p - 1, -1, P, X)
            rows[(p, q, ln)] = (er, el, mr + ml)
        out.append(rows)
    return tuple(out)


def test_the_limits_are_the_kernels():
    assert (ec.EXT_LANE_MAX, ec.PACK_LANE_UNITS, ec.WINDOW) == (32, 16, 64)
    # k_ext_pack_long: 256 lanes stride a record's units
    text = open(ec.CSRC + "/filter_shared.h").read()
    assert "for (uint64_t u = threadIdx.x; u < nu; u += 256u) pack_unit(rec, len, 64u * u, U + u);" in text
    assert ec.PACK_LONG_LANES == 256 and (ec.LONG_RECORD + W - 1) // W > ec.PACK_LONG_LANES and ec.LONG_RECORD % 8
    for x in (L, 2 * L, 4 * L):
        assert {x - 1, x, x + 1} <= set(ec.BLOCK_SIZES)
    assert {1, 2, 200} <= set(ec.BLOCK_SIZES)
    assert set(ec.DISTANCES) == {0, 1, 62, 63, 64, 65, 126, 127, 128, 129} and set(ec.DROP_BITS) == {62, 63, 64, 65}
    assert set(ec.TWIN_DISTANCES) == {1, 31, 32, 33, 63, 64, 65}
    assert set(ec.ALIGN_LENGTHS) == {63, 64, 65, 1023, 1024, 1025}


def test_the_catalogue_is_small_and_every_read_has_its_designed_rows():
    rows = letters = 0
    for d in ec.designs():
        q, off = d.arrays()
        letters += len(q)
        rows += sum(len(m["rows"]) for m in d.meta)
        assert set(np.unique(q)) <= set(b"ACGTN"), d
        for both in (True, False):
            got = oracle_blocks(d.name, both)
            want = ec.expected_blocks(d.batch(both, *d.params[0]))
            assert len(got) == len(want) == (len(off) - 1) * (2 if both else 1)
            for k, (g, w) in enumerate(zip(got, want)):
                g = g[np.lexsort((g[:, 2], g[:, 1], g[:, 0]))]
                assert np.array_equal(g, w), (d, both, k, g.tolist()[:5], w.tolist()[:5])
                # the emission order: q falls, equal q: the length falls
                o = got[k]
                assert not np.any((np.diff(o[:, 1]) > 0) | ((np.diff(o[:, 1]) == 0) & (np.diff(o[:, 2]) > 0)))
    assert rows <= 20_000 and letters <= 300_000, (rows, letters)
    # each family with both strands scanned and with the forward strand alone
    assert {(b.meta["family"], b.both) for b in ec.all_batches()} == {(f, s) for f in ec.FAMILIES for s in (True, False)}


def facing(d, b, k: int, side: str, dist: int) -> str:
    """What the rule meets at distance `dist` from read k's anchor."""
    m = d.meta[k]
    Q = ec.design_strand(b, k)
    a = m["q"] + m["A"] + dist if side == "right" else m["q"] - 1 - dist
    t = a + m["diag"]
    if a < 0 or a >= len(Q):
        return "record_end"
    if t < 0 or t >= len(d.ref):
        return "text_end"
    if d.ref[t] == ec.N_:
        return "separator"
    if Q[a] == ec.N_:
        return "read_N"
    return "match" if Q[a] == d.ref[t] else "mismatch"


def trajectory(d, b, k: int, side: str, P: int) -> list:
    """(s, best) after each letter of the side, up to the letter that ends it whatever X is."""
    out, s, best, dist = [], 0, 0, 0
    while True:
        f = facing(d, b, k, side, dist)
        if f not in ("match", "mismatch"):
            return out
        s += 1 if f == "match" else -P
        best = max(best, s)
        out.append((s, best))
        dist += 1


def test_distances_reach():
    seen, qmod, lenmod, starts = set(), set(), set(), set()
    for d in ec.designs("distances"):
        b = d.batch(True, 4, 20)
        n = len(d.ref)
        for k, m in enumerate(d.meta):
            kind, side, t = m["kind"], m["side"], m["t"]
            # the anchor is a row: [p, p + A) exact, bounded on both sides
            assert (m["p"], m["q"], m["A"]) in {tuple(r) for r in m["rows"].tolist()}, (d, k)
            if t:
                assert facing(d, b, k, side, 0) == "mismatch" and all(facing(d, b, k, side, x) == "match" for x in range(1, t)), (d, k)
            assert facing(d, b, k, side, t) == kind, (d, k, m)
            seen.add((kind, side, t, m["rev"]))
            qmod.add(m["q"] % W)
            if kind == "record_end":
                lenmod.add((side, m["length"] % W))
            if kind == "text_end":
                starts.add((side, m["p"] if side == "left" else n % W))
    for kind in ec.KINDS:
        for side in ("right", "left"):
            for t in ec.DISTANCES:
                assert (kind, side, t, False) in seen and (kind, side, t, True) in seen, (kind, side, t)
    assert {0, 1, 63} <= qmod
    assert {("right", x) for x in (0, 1, 63)} <= lenmod
    assert {("left", p) for p in (0, 1, 63, 64, 65)} <= starts and {("right", x) for x in (0, 1, 63)} <= starts
    assert {len(d.ref) % W for d in ec.designs("distances")} == {0, 1, 63}


def anchor_ext(d, k: int, side: str, P: int, X: int) -> int:
    m = d.meta[k]
    return spec_rows(d.name, P, X)[k][(m["p"], m["q"], m["A"])][0 if side == "right" else 1]


def test_drop_decisions():
    seen = set()
    for d in ec.designs("drop"):
        P, X = d.params[0]
        b = d.batch(True, P, X)
        for k, m in enumerate(d.meta):
            tr = trajectory(d, b, k, m["side"], P)
            bit = m["bit"]
            assert facing(d, b, k, m["side"], bit) == "mismatch" and facing(d, b, k, m["side"], bit + 1) == "match"
            drops = [best - s for s, best in tr]
            assert max(drops[:bit]) <= X and drops[bit] == (X if m["which"] == "exact" else X + 1), (d, k, drops[:bit + 1])
            assert tr[-1][0] > tr[bit][1] and len(tr) - bit > 30   # the exact run behind it would raise the best score
            ext = anchor_ext(d, k, m["side"], P, X)
            assert ext == m["ext"] == (len(tr) if m["which"] == "exact" else bit + 1 - drops[:bit + 1][::-1].index(0)), (d, k, ext, m)
            seen.add((P, X, m["which"], bit, m["side"], m["rev"]))
            # X = 0 and the largest penalty: the side ends at its first mismatch, which bounds the anchor
            assert anchor_ext(d, k, m["side"], P, 0) == 0 == anchor_ext(d, k, m["side"], ec.P_MAX, X) == anchor_ext(d, k, m["side"], ec.P_MAX, ec.X_MAX)
            assert anchor_ext(d, k, m["side"], P, ec.X_MAX) >= m["ext"]
        assert set(d.params[1:]) == {(P, 0), (P, ec.X_MAX), (ec.P_MAX, X), (ec.P_MAX, ec.X_MAX)}
    assert len(seen) == 2 * 2 * 4 * 2 * 2 and {(4, 20), (1, 5)} == {s[:2] for s in seen}


def test_ties_keep_the_shorter_extension():
    seen, straddle, border = set(), set(), set()
    for d in ec.designs("ties"):
        P, X = d.params[0]
        b = d.batch(True, P, X)
        for k, m in enumerate(d.meta):
            side, stop, M = m["side"], m["stop"], m["matches"]
            tr = trajectory(d, b, k, side, P)
            assert facing(d, b, k, side, stop - M - 1) == "mismatch" and all(facing(d, b, k, side, stop - 1 - x) == "match" for x in range(M))
            assert facing(d, b, k, side, stop) == {"record": "record_end", "read_N": "read_N", "xdrop": "mismatch"}[m["end"]]
            s, best = tr[stop - 1]
            before = tr[stop - M - 2][1] if stop - M - 2 >= 0 else 0
            assert (s == before == best) if M == P else (s == before + 1 == best), (d, k, m)
            if m["end"] == "xdrop":   # the mismatches behind end the side, within the letters the design wrote
                drops = [bb - ss for ss, bb in tr[stop:]]
                assert max(drops) > X and drops.index(max(drops)) == X // P, (d, k)
            ext = anchor_ext(d, k, side, P, X)
            assert ext == m["ext"] == (stop - M - 1 if M == P else stop), (d, k, ext, m)
            seen.add((P, m["at"] is None, M == P, m["end"], side, m["rev"]))
            if M > 1 and (stop - M) // W != (stop - 1) // W:
                straddle.add((P, M == P, m["end"], side, m["rev"]))
            if stop == W:
                border.add((P, M == P, m["end"], side, m["rev"]))
    for P in (4, 1):
        for end in ("record", "read_N", "xdrop"):
            for side in ("right", "left"):
                for rev in (False, True):
                    for tie in (True, False):
                        assert (P, True, tie, end, side, rev) in seen and (P, False, tie, end, side, rev) in seen
                        assert (P, tie, end, side, rev) in border     # the side ends where the next window starts
                        assert P == 1 and tie or (P, tie, end, side, rev) in straddle


def test_alignment_reach():
    a, b = ec.designs("alignment")
    for d in (a, b):
        assert d.meta[-1]["record"] == ec.LONG_RECORD and d.meta[-1]["length"] % 8 and d.meta[-1]["start"] % 16 == d.meta[-1]["byte"]
        assert sum(m.get("record") == ec.LONG_RECORD for m in d.meta) == 1
    assert (a.meta[-1]["rev"], b.meta[-1]["rev"]) == (False, True) and a.meta[-1]["start"] % 8 != b.meta[-1]["start"] % 8
    seen, fillers = set(), set()
    for m in a.meta:
        if m.get("filler"):
            assert len(m["rows"]) == 0
            fillers.add(m["length"])
            continue
        assert m["start"] % 16 == m["byte"] and m["length"] == m["record"]
        seen.add((m["record"], m["byte"]))
        seen.add((m["record"], m["byte"] % 8, m["rev"]))
        # rows over the whole record: the first starts at letter 7, the last ends 7 letters in front of the end
        r = m["rows"]
        assert r[:, 1].min() == 7 and (r[:, 1] + r[:, 2]).max() == m["length"] - 7
        units = (m["record"] + W - 1) // W
        seen.add("lane" if units <= ec.PACK_LANE_UNITS else "listed")
    for n in ec.ALIGN_LENGTHS:
        assert {(n, x) for x in range(16)} <= seen and {(n, x, rev) for x in range(8) for rev in (False, True)} <= seen
    assert {"lane", "listed"} <= seen and fillers == set(range(1, 17))
    # every row of such a record grows over all of it: each unit is read by every row
    for d in (a, b):
        for k, m in enumerate(d.meta):
            for (p, q, ln), (er, el, mm) in spec_rows(d.name, 4, 20)[k].items():
                assert (q - el, el + ln + er) == (0, m["length"]) and mm == int((ec.design_strand(d.batch(True, 4, 20), k) != d.ref[m["diag"]:m["diag"] + m["length"]]).sum())


def block_filter(d, both: bool, k: int):
    """(the rows of read k's matching strand block in emission order, their segments, the kept mask) by the spec's rule."""
    m = d.meta[k]
    if m["rev"] and not both:
        return None
    rows = oracle_blocks(d.name, both)[(2 * k + int(m["rev"])) if both else k]
    ext = spec_rows(d.name, 4, 20)[k]
    segs, keep, seen = [], [], set()
    for p, q, ln in rows.tolist():
        er, el, _ = ext[(p, q, ln)]
        seg = (p - el, q - el, el + ln + er)
        keep.append(seg not in seen)
        seen.add(seg)
        segs.append(seg)
    return rows, segs, np.array(keep, dtype=bool)


def test_blocks_reach():
    d, nb = ec.designs("blocks")
    sizes, twin, kept_rows = set(), {"lane": set(), "listed": set()}, set()
    between = 0
    for k, m in enumerate(d.meta):
        rows, segs, keep = block_filter(d, True, k)
        assert len(rows) == m["rows_n"] == len(m["rows"])
        tier = "lane" if len(rows) <= L else "listed"
        if m["kind"] in ("plain", "breaks"):
            assert tuple(np.flatnonzero(keep)) == m["kept"], (k, m["kind"], np.flatnonzero(keep))
            sizes.add((m["kind"], len(rows), m["rev"]))
            if m["kind"] == "breaks":
                kept_rows |= {(e // W, m["rev"]) for e in m["kept"]}
                assert len({s for s in segs}) == len(m["kept"])
        for i in np.flatnonzero(~keep):   # a dropped row: how far back is its nearest twin, and what lies between
            j = max(x for x in range(i) if segs[x] == segs[i])
            twin[tier].add((i - j, m["rev"]))
            if m["kind"] == "twins":
                between += sum(rows[x][0] - rows[x][1] != rows[i][0] - rows[i][1] for x in range(j + 1, i))
                assert all(keep[x] for x in range(j + 1, i))   # the rows of other diagonals between two twins are kept
    for n in ec.BLOCK_SIZES:
        assert ("plain", n, False) in sizes and ("plain", n, True) in sizes
    assert {n for kind, n, _ in sizes if kind == "breaks"} == {65, 127, 128, 129, 200}
    assert {(t, rev) for t in (0, 1, 2) for rev in (False, True)} <= kept_rows   # kept rows in three trips of a wave
    for rev in (False, True):
        assert {(x, rev) for x in ec.TWIN_DISTANCES} <= twin["listed"] and {(1, rev), (L - 1, rev)} <= twin["lane"]
    assert between > 500
    assert any(m["kind"] == "twins" and m["rows_n"] == L for m in d.meta)
    # blocks of 32 and 33 rows side by side, empty ones between
    for both in (True, False):
        got = [len(x) for x in oracle_blocks(nb.name, both)]
        pairs = set(zip(got, got[1:]))
        assert {L, L + 1, 0} == set(got)
        near = {(x, y) for x in (L, L + 1) for y in (L, L + 1)}
        assert near <= pairs
        if not both:
            assert near | {(L, 0), (L + 1, 0), (0, L), (0, L + 1), (0, 0)} <= pairs
    for k, m in enumerate(nb.meta):
        if not m.get("empty"):
            assert tuple(np.flatnonzero(block_filter(nb, True, k)[2])) == (0,)


# ---- three wrong rules, in this file only ------------------------------------------------------------------------------------

def wrong_drop(Q, T, qi, ti, step, P, X):
    """extend_side with `best - s >= X`: a drop of exactly X ends the side."""
    s = best = ext = mm = mm_best = t = 0
    while True:
        a, b = qi + step * t, ti + step * t
        if a < 0 or b < 0 or a >= len(Q) or b >= len(T):
            break
        x, y = Q[a] & 0xDF, T[b] & 0xDF
        if x not in ACGT or y not in ACGT:
            break
        if x == y:
            s += 1
        else:
            s -= P
            mm += 1
        if s > best:
            best, ext, mm_best = s, t + 1, mm
        if best - s >= X:
            break
        t += 1
    return ext, best, mm_best


def wrong_tie(Q, T, qi, ti, step, P, X):
    """extend_side with `s >= best`: a tie takes the longer extension."""
    s = best = ext = mm = mm_best = t = 0
    while True:
        a, b = qi + step * t, ti + step * t
        if a < 0 or b < 0 or a >= len(Q) or b >= len(T):
            break
        x, y = Q[a] & 0xDF, T[b] & 0xDF
        if x not in ACGT or y not in ACGT:
            break
        if x == y:
            s += 1
        else:
            s -= P
            mm += 1
        if s >= best:
            best, ext, mm_best = s, t + 1, mm
        if best - s > X:
            break
        t += 1
    return ext, best, mm_best


def window_walk(Q, T, qi, ti, step, P, X, carry=True):
    """The rule as a walk over 64-letter windows that adds the run of matches in front of each mismatch and in front of the
    letter that ends the side.  carry=False forgets the run left over from the window before."""
    s = best = ext = mm = mm_best = pos = t0 = 0
    while True:
        if not carry:
            pos = t0
        for t in range(t0, t0 + W):
            a, b = qi + step * t, ti + step * t
            inside = a >= 0 and b >= 0 and a < len(Q) and b < len(T)
            x, y = (Q[a] & 0xDF, T[b] & 0xDF) if inside else (0, 0)
            if not inside or x not in ACGT or y not in ACGT:
                s += t - pos
                if s > best:
                    best, ext, mm_best = s, t, mm
                return ext, best, mm_best
            if x != y:
                s += t - pos
                if s > best:
                    best, ext, mm_best = s, t, mm
                s -= P
                mm += 1
                pos = t + 1
                if best - s > X:
                    return ext, best, mm_best
        t0 += W


def differing_reads(family: str, rule) -> int:
    """Reads of a family on which `rule` gives another extension or mismatch count for a designed row than the spec."""
    n = 0
    for d in ec.designs(family):
        P, X = d.params[0]
        b = d.batch(True, P, X)
        T = d.ref.tobytes()
        for k, m in enumerate(d.meta):
            Q = ec.design_strand(b, k).tobytes()
            for (p, q, ln), (er, el, mm) in spec_rows(d.name, P, X)[k].items():
                gr, _, mr = rule(Q, T, q + ln, p + ln, +1, P, X)
                gl, _, ml = rule(Q, T, q - 1, p - 1, -1, P, X)
                if (gr, gl, mr + ml) != (er, el, mm):
                    n += 1
                    break
    return n


def test_the_cases_tell_the_rule_from_wrong_ones():
    assert differing_reads("drop", wrong_drop) >= 16
    assert differing_reads("ties", wrong_tie) >= 16
    for family in ("distances", "ties", "drop"):
        assert differing_reads(family, window_walk) == 0   # (the walk over windows is the rule ...)
    no_carry = functools.partial(window_walk, carry=False)
    assert differing_reads("distances", no_carry) >= 16 and differing_reads("ties", no_carry) >= 16   # (... as long as it carries the run)


def test_the_numpy_spec_equals_the_letter_wise_one_on_every_designed_row():
    for d in ec.designs():
        Tb, Ta = d.ref.tobytes(), d.ref
        for P, X in d.params:
            b = d.batch(True, P, X)
            for k, m in enumerate(d.meta):
                Qa = ec.design_strand(b, k)
                for (p, q, ln), (er, el, mm) in spec_rows(d.name, P, X)[k].items():
                    gr, _, mr = ext_spec.extend_side_np(Qa, Ta, q + ln, p + ln, +1, P, X)
                    gl, _, ml = ext_spec.extend_side_np(Qa, Ta, q - 1, p - 1, -1, P, X)
                    assert (gr, gl, mr + ml) == (er, el, mm), (d, P, X, k, (p, q, ln))
