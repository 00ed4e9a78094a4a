"""The designed table of the -cons -gt tests, shared by test_cons_gt_host.py (the spec on it) and
test_gpu_cons_gt.py (the device against the spec): a text of 400 letters, rows that each show one rule, the events, and the
rows whose GQ sits exactly on a threshold, found by search."""
import numpy as np

import cons_gt_spec as cg
import events_spec as es
import gt_spec
import qual_spec

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
N = 400
MIN_DEPTH = 4
Q = 30  # the quality of every planted letter, but for the row in which the qualities decide
# the rows, by what they show
HOM_REF, HOM_ALT, HET_REF, HET_ALT, SHALLOW, EMPTY, WQ_ROW, BIG, NROW, EDGE0 = 10, 11, 12, 13, 14, 15, 16, 17, 50, 60
# (ploidy, weighted, min_gq, costs): the calls of the designed case; the rows on the threshold of each are planted from EDGE0 on
COMBOS = [(pl, w, gq, None) for pl in (1, 2) for w in (False, True) for gq in (0, 20, 999)] + \
         [(pl, w, gq, (0, 5, 1)) for pl, w, gq in ((1, False, 20), (1, True, 999), (2, False, 20), (2, True, 20))]


def own_column(text):
    code = np.full(len(text), 4, dtype=np.int64)
    for k, c in enumerate(b"ACGT"):
        code[(np.asarray(text) & 0xDF) == c] = k
    return code


def gq_of(c, qs, r, P_row, weighted):
    P = cg.rule_params(P_row)
    return (qual_spec.snv(c, qs, r, P) if weighted else gt_spec.snv(c, r, P))[0][1]


def find_gq_row(target: int, r: int, P_row, weighted: bool):
    """(c, qs) of a row under the reference column r whose GQ is exactly `target` milli-Phred, or None.  The family: a letters of
    the reference's column and b of another; weighted, the other column's quality sum k is free (0 to 93 b) and the reference's
    letters have quality Q each (then, if nothing is found, 0).  For b fixed GQ is linear in a (slope s, measured) and falls by 1000
    per unit of k while the same two genotypes stay in front, so a and k come from one division; the spec then confirms the row."""
    other = (r + 1) % 4

    def row(a, b, k, qr):
        c, qs = [0, 0, 0, 0], [0, 0, 0, 0]
        c[r], c[other], qs[r], qs[other] = a, b, qr * a, k
        return c, qs
    a1 = 1 << 16
    for qr in ((Q, 0) if weighted else (0,)):
        for b in (range(60) if weighted else list(range(3000)) + [20000, 50000]):
            g1, g2 = gq_of(*row(a1, b, 0, qr), r, P_row, weighted), gq_of(*row(a1 + 1, b, 0, qr), r, P_row, weighted)
            s = g2 - g1
            if s <= 0:
                continue
            for k in (range(min(93 * b, 2000) + 1) if weighted else (0,)):
                if (target - g1 + 1000 * k) % s:
                    continue
                a = a1 + (target - g1 + 1000 * k) // s
                if a < 0 or a + b < MIN_DEPTH or a >= 2 ** 31 or Q * a >= 2 ** 32:
                    continue
                if gq_of(*row(a, b, k, qr), r, P_row, weighted) == target:
                    return row(a, b, k, qr)
    return None


def unlike(T, p):
    """a letter that row p - 1 does not hold: an insertion that ends with it stays at p"""
    return bytes([b"ACGT"[(b"ACGT".index(bytes([T[p - 1] & 0xDF])) + 1) % 4]])


_CASE = None


def designed():
    """dict(text, T, table, qtable, raw, E, edges): edges[(combo)] = (row on the threshold, row one below) or None."""
    global _CASE
    if _CASE is not None:
        return _CASE
    rng = np.random.default_rng(61)
    text = rng.choice(ACGT, size=N)
    text[NROW] = ord("N")
    for p, L in ((100, 3), (120, 2)):  # the deletions stay where they are
        text[p - 1] = ACGT[(int(np.where(ACGT == text[p + L - 1])[0][0]) + 1) % 4]
    text[200:210] |= 0x20
    T = bytes(text)
    own = own_column(text)
    t = np.zeros((N, 6), dtype=np.uint32)
    q = np.zeros((N, 6), dtype=np.uint32)
    for p in range(N):  # the background: the text's letter 8 times, and a stray other letter here and there
        if own[p] < 4:
            t[p][own[p]] = 8
            if p % 7 == 3:
                t[p][(own[p] + 1 + p % 3) % 4] = 1
            t[p][4], t[p][5] = p % 3 == 0, p % 5 == 0

    def put(p, **cols):  # o: the text's column, x, y: the next two
        t[p] = 0
        o = int(own[p])
        for k, v in cols.items():
            t[p][{"o": o, "x": (o + 1) % 4, "y": (o + 2) % 4, "d": 4}[k]] = v
    put(HOM_REF, o=60)
    put(HOM_ALT, x=40)
    put(HET_REF, o=10, x=10)
    put(HET_ALT, x=10, y=10)
    put(SHALLOW, o=MIN_DEPTH - 1)
    put(EMPTY, d=6)
    put(WQ_ROW, o=12, x=5)
    put(BIG, o=2 ** 20, x=2 ** 20)
    t[NROW] = (9, 0, 0, 0, 1, 0)
    for a in (99, 119, 139, 51):  # the events' anchors: depth 20
        put(a, o=20)
    q[:, :4] = t[:, :4] * Q
    o = int(own[WQ_ROW])
    q[WQ_ROW][o], q[WQ_ROW][(o + 1) % 4] = 12 * 2, 5 * 40  # many poor reference letters, few good other ones
    edges, at = {}, EDGE0
    for combo in COMBOS:
        ploidy, weighted, min_gq, costs = combo
        P_row, _ = cg.params(ploidy, weighted=weighted, costs=costs)
        pair = []
        for target in (1000 * min_gq, 1000 * min_gq - 1):
            got = find_gq_row(target, int(own[at]), P_row, weighted) if target >= 0 else None
            if got is None:
                break
            t[at], q[at] = got[0] + [0, 0], got[1] + [0, 0]
            pair.append(at)
            at += 1
        edges[combo] = tuple(pair) if len(pair) == 2 else None
    assert at < 99  # (the first anchor of the events)
    raw = [(100, 0, 3, b"", 10, 9),                                    # 19 of 20: 1/1
           (120, 0, 2, b"", 6, 4),                                     # 10 of 20: 0/1
           (140, 1, 2, b"G" + unlike(T, 140), 10, 9), (140, 1, 1, unlike(T, 140), 20, 0),  # two at one position, both 1/1
           (51, 1, 2, b"CA", 10, 9)]                                   # at a record's first base: its anchor is its own row
    spec = es.Table(text)
    for e in raw:
        spec.observe(*e)
    E = spec.events()
    assert spec.skipped == [0, 0, 0] and sorted(e[:3] for e in E) == sorted(e[:3] for e in raw)
    _CASE = dict(text=text, T=T, table=t, qtable=q, raw=raw, E=E, edges=edges, own=own)
    return _CASE


def random_table(n, rng, events=True):
    """A random text with a table, quality sums and events for the properties: rows of every kind at random."""
    text = rng.choice(ACGT, size=n)
    text[rng.choice(n, size=max(1, n // 100), replace=False)] = ord("N")
    own = own_column(text)
    t = np.zeros((n, 6), dtype=np.uint32)
    q = np.zeros((n, 6), dtype=np.uint32)
    for p in range(n):
        k = int(rng.integers(0, 6))
        o = int(own[p]) % 4
        if k == 0:
            t[p][o] = rng.integers(0, 5)
        elif k == 1:
            t[p][4] = rng.integers(0, 9)
        elif k == 2:
            t[p][o] = rng.integers(5, 40)
        elif k == 3:
            t[p][(o + 1 + int(rng.integers(0, 3))) % 4] = rng.integers(1, 40)
        else:
            t[p][:4] = rng.integers(0, 12, size=4)
        q[p][:4] = t[p][:4] * rng.integers(0, 42, size=4)
    raw = []
    if events:
        T = bytes(text)
        for p in rng.choice(np.arange(2, n - 8), size=max(2, n // 40), replace=False):
            p = int(p)
            obs = int(rng.integers(1, 30))
            if rng.integers(0, 2):
                raw.append((p, 0, int(rng.integers(1, 6)), b"", obs, 0))
            else:
                raw.append((p, 1, 2, b"AC", obs // 2, obs - obs // 2))
        spec = es.Table(text)
        for e in raw:
            spec.observe(*e)
        E = spec.events()
    else:
        E = []
    return text, t, q, raw, E
