"""Designed read batches for -ext: reads cut from a random A,C,G,T text with substitutions, N, record ends and
text ends planted so that a mismatch, a sequence end or a decision of the X-drop rule falls on a border the kernels have -- the
64-letter windows of filter_shared.h (walk, window, strand_window), the 8-byte words and the 16 units of pack_unit / k_ext_pack,
the 32 rows of k_ext_dedup -- instead of wherever random data happens to put it.  Pure numpy, seeded; no GPU, no engine.

A read is DESIGNED on the strand that matches the text ("design strand") as a diagonal (text position - read position) and its
letters; every second read is handed over reverse-complemented, so its rows are those of its reverse strand block.  The -mem
rows of a read are known by design: the exact stretches of at least MIN_LEN letters on its diagonal (diag_rows), plus the text
copies a `twins` read plants.  tests/test_ext_edge_cases.py holds that against the oracle, so the seeds below are ones on which no
other diagonal holds a chance match of MIN_LEN letters.

A side of an anchor (an exact stretch [p, p + A) of the text) is written outward as a string, one letter per distance from the
anchor: m the text's letter, x another letter (a substitution), n an N in the read, j a letter that faces no letter of the
text (beyond its ends, on a record separator) or differs from it.  MIN_LEN is fixed at 20 (the designs count letters); every text
here is short enough that 20 >= seed length + 2, which tests/test_gpu_ext_edges.py asserts, so the seed path takes the reads.
"""
import functools
import os
import re
from collections import namedtuple

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slamem_amd", "csrc")


def _constexpr(source: str, name: str) -> int:
    m = re.search(r"constexpr\s+(?:unsigned|uint32_t|uint64_t)\s+" + name + r"\s*=\s*(\d+)u?\s*;", open(os.path.join(CSRC, source)).read())
    assert m, (source, name)
    return int(m.group(1))


def _window() -> int:
    """The width of window(): `a >> 6` picks the unit, `a & 63` the shift."""
    text = open(os.path.join(CSRC, "filter_shared.h")).read()
    sh, mask = re.search(r"const int64_t u = a >> (\d+);", text), re.search(r"const uint32_t sh = \(uint32_t\)\(a & (\d+)\);", text)
    assert sh and mask and (1 << int(sh.group(1))) == int(mask.group(1)) + 1
    return 1 << int(sh.group(1))


EXT_LANE_MAX = _constexpr("ext_filter.hip", "kExtLaneMax")            # rows of a block one lane de-duplicates (32)
PACK_LANE_UNITS = _constexpr("filter_shared.h", "kExtPackLaneUnits")  # units of a record one lane packs (16)
WINDOW = _window()                                                    # letters of a window / a unit (64)
PACK_LONG_LANES = 256                                                 # lanes of k_ext_pack_long: a lane's units are 256 apart

MIN_LEN = 20
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
N_ = ord("N")
P_MAX, X_MAX = 2 ** 32 - 1, 2 ** 32 - 2  # the largest penalty and drop the interface accepts

W = WINDOW
DISTANCES = (0, 1, W - 2, W - 1, W, W + 1, 2 * W - 2, 2 * W - 1, 2 * W, 2 * W + 1)
KINDS = ("mismatch", "record_end", "text_end", "read_N", "separator")
MODS = (0, 1, W - 1)
DROP_BITS = (W - 2, W - 1, W, W + 1)


def tie_places(P: int) -> tuple:
    """Where the tie's mismatch stands: next to the anchor (None), and so that its P or P + 1 matches end on the window border,
    lie across it, or start behind it."""
    return (None,) + tuple(sorted({W - 2 - P, W - 1 - P, W - 3, W - 1}))


ALIGN_LENGTHS = (W - 1, W, W + 1, W * PACK_LANE_UNITS - 1, W * PACK_LANE_UNITS, W * PACK_LANE_UNITS + 1)
LONG_RECORD = W * PACK_LONG_LANES + W + 37  # 258 units: lanes 0 and 1 of k_ext_pack_long take a second one; 5 modulo 8
L = EXT_LANE_MAX
BLOCK_SIZES = (1, 2, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 4 * L - 1, 4 * L, 4 * L + 1, 200)
KEPT_AT = (0, 1, W - 2, W - 1, W, W + 1, 2 * W - 2, 2 * W - 1, 2 * W, 2 * W + 1)  # rows (in emission order) that start a segment
TWIN_DISTANCES = (1, L - 1, L, L + 1, W - 1, W, W + 1)

_COMP = np.full(256, N_, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCATGCA"):
    _COMP[_a] = _b

Batch = namedtuple("Batch", "ref queries offsets min_len both P X meta")


def revcomp(a) -> np.ndarray:
    return _COMP[np.asarray(a, dtype=np.uint8)[::-1]]


def other(rng, c) -> int:
    """A letter of A,C,G,T that is not c."""
    return int(ACGT[(int(np.searchsorted(ACGT, c)) + 1 + int(rng.integers(0, 3))) % 4])


def side_letters(rng, ref, first: int, step: int, spec: str) -> np.ndarray:
    """The letters of a side, outward: letter d faces text position first + step * d."""
    out = np.empty(len(spec), dtype=np.uint8)
    for d, c in enumerate(spec):
        i = first + step * d
        inside = 0 <= i < len(ref) and ref[i] != N_
        if c in "mx":
            assert inside, (spec, d, i)
            out[d] = ref[i] if c == "m" else other(rng, ref[i])
        elif c == "n":
            assert inside
            out[d] = N_
        else:
            assert c == "j"
            out[d] = other(rng, ref[i]) if inside else rng.choice(ACGT)
    return out


def build_read(rng, ref, p: int, A: int, left: str, right: str):
    """(letters, q): the anchor [p, p + A) of the text with its two sides; q = where the anchor starts in the read."""
    assert 0 <= p and p + A <= len(ref) and not np.any(ref[p:p + A] == N_)
    return np.concatenate([side_letters(rng, ref, p - 1, -1, left)[::-1], ref[p:p + A], side_letters(rng, ref, p + A, +1, right)]), len(left)


def diag_rows(ref, letters, diag: int, min_len: int = MIN_LEN) -> np.ndarray:
    """The exact stretches of at least min_len letters of a read on one diagonal, as -mem rows (p, q, length)."""
    n = len(letters)
    i = np.arange(n) + diag
    ok = (i >= 0) & (i < len(ref))
    m = np.zeros(n, dtype=bool)
    m[ok] = (letters[ok] == ref[i[ok]]) & np.isin(letters[ok], ACGT)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], m.astype(np.int8), [0]])))
    return np.array([(s + diag, s, e - s) for s, e in zip(edges[::2], edges[1::2]) if e - s >= min_len], dtype=np.int64).reshape(-1, 3)


class Design:
    """The reads of one text.  params: the (P, X) pairs it is run with, the first the one it is designed for."""

    def __init__(self, name: str, family: str, ref, params=((4, 20),)):
        self.name, self.family, self.ref, self.params = name, family, np.asarray(ref, dtype=np.uint8), tuple(params)
        self.reads, self.meta = [], []

    def add(self, letters, diag, rev: bool, extra_rows=None, **tags):
        """A designed read (letters on the design strand)."""
        rows = diag_rows(self.ref, letters, diag)
        if extra_rows is not None and len(extra_rows):
            rows = np.concatenate([rows, np.asarray(extra_rows, dtype=np.int64).reshape(-1, 3)])
        self.reads.append(revcomp(letters) if rev else np.asarray(letters, dtype=np.uint8))
        self.meta.append(dict(tags, rev=bool(rev), diag=int(diag), rows=rows, start=sum(len(r) for r in self.reads[:-1]), length=len(letters)))

    def add_plain(self, letters, **tags):
        """A read without a row: a filler, a read of N."""
        self.reads.append(np.asarray(letters, dtype=np.uint8))
        self.meta.append(dict(tags, rev=False, diag=None, rows=np.zeros((0, 3), np.int64), start=sum(len(r) for r in self.reads[:-1]),
                              length=len(letters)))

    def arrays(self):
        q = np.concatenate(self.reads)
        off = np.concatenate([[0], np.cumsum([len(r) for r in self.reads])]).astype(np.uint64)
        return q, off

    def batch(self, both: bool, P: int, X: int) -> Batch:
        q, off = self.arrays()
        return Batch(self.ref, q, off, MIN_LEN, both, P, X, dict(name=self.name, family=self.family, reads=self.meta))

    def batches(self):
        return [self.batch(both, P, X) for both in (True, False) for P, X in self.params]

    def __repr__(self):
        return self.name


def expected_blocks(b: Batch) -> list:
    """The designed -mem rows of every strand block, sorted (p, q, length)."""
    strands = 2 if b.both else 1
    out = []
    for m in b.meta["reads"]:
        for s in range(strands):
            r = m["rows"] if int(m["rev"]) == s else m["rows"][:0]
            out.append(r[np.lexsort((r[:, 2], r[:, 1], r[:, 0]))])
    return out


def design_strand(b: Batch, k: int) -> np.ndarray:
    """Read k as it was designed (the strand that matches the text)."""
    m = b.meta["reads"][k]
    r = b.queries[m["start"]:m["start"] + m["length"]]
    return revcomp(r) if m["rev"] else r


def random_text(rng, n: int) -> np.ndarray:
    return rng.choice(ACGT, size=n)


def two_records(rng, mod: int):
    """Two records with the separator N between, n % 64 == mod.  Returns (text, position of the separator)."""
    a = 1600
    b = 1600 + (mod - (a + 1 + 1600)) % W
    t = np.concatenate([random_text(rng, a), [N_], random_text(rng, b)]).astype(np.uint8)
    assert len(t) % W == mod
    return t, a


PLAIN = "x" + "m" * 7  # the side a design says nothing about: a mismatch, seven matches, the record's end


def event_side(kind: str, t: int) -> str:
    """The event `kind` at distance t from the anchor: a mismatch at distance 0 bounds the anchor, matches up to t - 1 (t = 0: the
    event itself bounds the anchor)."""
    lead = "x" + "m" * (t - 1) if t else ""
    return lead + {"mismatch": "x" + "m" * 70, "record_end": "", "text_end": "j" * 10, "read_N": "n" + "m" * 30, "separator": "j" + "m" * 30}[kind]


@functools.lru_cache(maxsize=None)
def distances() -> tuple:
    out = []
    for ti, mod in enumerate(MODS):
        rng = np.random.default_rng(100 + ti)
        ref, sep = two_records(rng, mod)
        n = len(ref)
        d = Design(f"distances-n{mod}", "distances", ref, ((4, 20), (1, 5)))
        k = 0
        for kind in KINDS:
            for side in ("right", "left"):
                for t in DISTANCES:
                    spec = event_side(kind, t)
                    A = 24
                    if side == "right":
                        fill = (MODS[(ti + k) % 3] - 1) % W  # q % 64 of the anchor
                        left, right = "x" + "m" * (fill if fill >= 5 else fill + W), spec
                        if kind == "record_end":  # len % 64
                            A += (MODS[(ti + k // 3) % 3] - (len(left) + A + len(right))) % W
                        p = n - t - A if kind == "text_end" else sep - t - A if kind == "separator" else 400 + 7 * k
                    else:
                        left, right = spec, PLAIN
                        p = t if kind == "text_end" else sep + 1 + t if kind == "separator" else 400 + 7 * k
                    letters, q = build_read(rng, ref, p, A, left, right)
                    d.add(letters, p - q, (k + ti) % 2 == 1, kind=kind, side=side, t=t, q=q, A=A, p=p)
                    k += 1
        out.append(d)
    return tuple(out)


def drop_patterns(P: int, X: int):
    """(a run of mismatches and matches whose last mismatch brings the drop to exactly X, one whose last brings it to X + 1), from
    a state with s == best; in neither does an earlier letter exceed X."""
    if (P, X) == (4, 20):
        return "xxxmmmmxxx", "xxxmmmxxx"
    assert P == 1
    return "x" * X, "x" * (X + 1)


@functools.lru_cache(maxsize=None)
def drop() -> tuple:
    out = []
    for P, X in ((4, 20), (1, 5)):
        rng = np.random.default_rng(200 + P)
        ref = random_text(rng, 4000 + P)
        d = Design(f"drop-P{P}-X{X}", "drop", ref, ((P, X), (P, 0), (P, X_MAX), (P_MAX, X), (P_MAX, X_MAX)))
        k = 0
        for which, pat in zip(("exact", "over"), drop_patterns(P, X)):
            for bit in DROP_BITS:
                for side in ("right", "left"):
                    for rev in (False, True):
                        fill = bit - len(pat)  # the deciding mismatch (the pattern's last) at distance `bit`
                        spec = "x" + "m" * fill + pat + "m" * 40
                        assert spec[bit] == "x" and spec[bit + 1] == "m" and fill > P
                        left, right = (PLAIN, spec) if side == "right" else (spec, PLAIN)
                        p = 300 + 11 * k
                        letters, q = build_read(rng, ref, p, 24, left, right)
                        d.add(letters, p - q, rev, which=which, bit=bit, side=side, q=q, A=24, p=p,
                              ext=len(spec) if which == "exact" else fill + 1)
                        k += 1
        out.append(d)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def ties() -> tuple:
    out = []
    for P, X in ((4, 20), (1, 5)):
        rng = np.random.default_rng(300 + P)
        ref = random_text(rng, 6000 + P)
        d = Design(f"ties-P{P}-X{X}", "ties", ref, ((P, X),))
        k = 0
        for at in tie_places(P):
            for matches in (P, P + 1):
                for end in ("record", "read_N", "xdrop"):
                    for side in ("right", "left"):
                        for rev in (False, True):
                            lead = "x" + "m" * (at - 1) if at else ""   # (s == best after it: at - 1 > P)
                            tail = {"record": "", "read_N": "n" + "m" * 8, "xdrop": "x" * (X // P + 1) + "m" * 30}[end]
                            spec = lead + "x" + "m" * matches + tail
                            base = at or 0
                            left, right = (PLAIN, spec) if side == "right" else (spec, PLAIN)
                            p = 300 + 9 * k
                            letters, q = build_read(rng, ref, p, 24, left, right)
                            d.add(letters, p - q, rev, at=at, matches=matches, end=end, side=side, q=q, A=24, p=p,
                                  stop=base + 1 + matches,  # the distance of the first letter behind the matches
                                  ext=base if matches == P else base + 1 + matches)
                            k += 1
        out.append(d)
    return tuple(out)


def cut_with_subs(rng, ref, a: int, n: int, every: int) -> np.ndarray:
    """ref[a : a + n] with substitutions at 6, n - 7 and every `every` letters between: every stretch between two of them of
    MIN_LEN letters or more is a row, and at P = 4, X = 20 each row grows over the whole record."""
    r = ref[a:a + n].copy()
    for x in sorted(set(range(6, n - 7 - MIN_LEN, every)) | {n - 7}):
        r[x] = other(rng, r[x])
    return r


def _filler(rng, d: Design, target: int) -> None:
    """A read of 1 .. 16 letters (no row) after which the next record starts at byte `target` modulo 16."""
    cur = sum(len(r) for r in d.reads)
    d.add_plain(random_text(rng, (target - cur - 1) % 16 + 1), filler=True)
    assert sum(len(r) for r in d.reads) % 16 == target


@functools.lru_cache(maxsize=None)
def alignment() -> tuple:
    rng = np.random.default_rng(401)
    ref = random_text(rng, 60_000)
    a = Design("alignment", "alignment", ref)
    for k in rng.permutation(16 * len(ALIGN_LENGTHS)):  # (shuffled: the fillers then have every length from 1 to 16)
        r, li = int(k) % 16, int(k) // 16
        n = ALIGN_LENGTHS[li]
        _filler(rng, a, r)
        at = int(rng.integers(0, len(ref) - n))
        a.add(cut_with_subs(rng, ref, at, n, 50), at, (r // 8 + li) % 2 == 1, byte=r, record=n)
    b = Design("alignment-long-reversed", "alignment", ref)
    for d, byte, rev in ((a, 5, False), (b, 11, True)):
        _filler(rng, d, byte)
        at = int(rng.integers(0, len(ref) - LONG_RECORD))
        d.add(cut_with_subs(rng, ref, at, LONG_RECORD, 500), at, rev, byte=byte, record=LONG_RECORD)  # the last record of its batch
    return a, b


STRETCH = MIN_LEN + 1


def block_read(rng, ref, a: int, lens, breaks=()) -> np.ndarray:
    """Exact stretches of `lens` letters cut from ref at a, one substitution between two of them -- X/P + 1 = 6 after the
    stretches (in read order) listed in `breaks`, which neither side of a row crosses at P = 4, X = 20."""
    out, x = [], a
    for j, n in enumerate(lens):
        out.append(ref[x:x + n].copy())
        x += n
        if j + 1 < len(lens):
            w = 6 if j in breaks else 1
            out.append(np.array([other(rng, c) for c in ref[x:x + w]], dtype=np.uint8))
            x += w
    return np.concatenate(out)


class _Copies:
    """Where the text copies of a `twins` read go: a region of the text no read is cut from."""

    def __init__(self, ref, at: int):
        self.ref, self.at = ref, at

    def plant(self, rng, read, q: int) -> tuple:
        """A copy of read[q : q + MIN_LEN] with letters in front and behind that differ from the read's: the row (copy, q, MIN_LEN)."""
        at = self.at + 1
        self.ref[at:at + MIN_LEN] = read[q:q + MIN_LEN]
        self.ref[at - 1], self.ref[at + MIN_LEN] = other(rng, read[q - 1]), other(rng, read[q + MIN_LEN])
        self.at += MIN_LEN + 4
        assert self.at < len(self.ref)
        return at, q, MIN_LEN


def twin_read(rng, ref, copies: _Copies, a: int, distances, head: int, tail: int) -> tuple:
    """A read of one segment whose stretches are STRETCH letters long, but for one of MIN_LEN + d letters per d in `distances`:
    d - 1 text copies of its letters [1, 1 + MIN_LEN) .. [d - 1, d - 1 + MIN_LEN) put d - 1 rows of other diagonals between that
    stretch's row and the row before it in the block (the next stretch's), its nearest twin.  (letters, copy rows, lens)"""
    lens = [STRETCH] * head
    for d in distances:
        lens += [MIN_LEN + d, STRETCH]
    lens += [STRETCH] * tail
    read = block_read(rng, ref, a, lens)
    rows, q = [], 0
    for n in lens:
        rows += [copies.plant(rng, read, q + k) for k in range(1, n - MIN_LEN)] if n > STRETCH else []
        q += n + 1
    return read, rows, lens


@functools.lru_cache(maxsize=None)
def blocks() -> tuple:
    rng = np.random.default_rng(500)
    ref = random_text(rng, 70_000)
    cut = [100]  # reads are cut from the text one after the other: no two share letters

    def take(n):
        cut[0] += n + 50
        assert cut[0] < 55_000
        return cut[0] - n - 50

    copies = _Copies(ref, 56_000)
    d = Design("blocks", "blocks", ref)
    twins = []
    for dist, head, tail in ((TWIN_DISTANCES[1:], 2, 1), ((L - 1,), 0, 0)):  # a listed block with every distance; one of 32 rows with 31
        a = take(sum(MIN_LEN + x + 1 for x in dist) + (len(dist) + head + tail) * (STRETCH + 1))
        twins.append((a,) + twin_read(rng, ref, copies, a, dist, head, tail))
    for n in BLOCK_SIZES:  # (a read and its reverse complement: the same rows, one in each kind of strand block)
        a = take(n * (STRETCH + 1))
        read = block_read(rng, ref, a, [STRETCH] * n)
        for rev in (False, True):
            d.add(read, a, rev, kind="plain", rows_n=n, kept=(0,))
    for n in [s for s in BLOCK_SIZES if s > 2 * L]:
        kept = tuple(e for e in KEPT_AT if e < n)
        a = take(n * (STRETCH + 1) + 5 * len(kept))
        read = block_read(rng, ref, a, [STRETCH] * n, breaks={n - 1 - e for e in kept if e})
        for rev in (False, True):
            d.add(read, a, rev, kind="breaks", rows_n=n, kept=kept)
    for a, read, rows, lens in twins:
        for rev in (False, True):
            d.add(read, a, rev, extra_rows=rows, kind="twins", rows_n=len(lens) + len(rows), lens=tuple(lens))
    nb = Design("blocks-neighbours", "blocks", ref)
    # forward reads alone: every pair of neighbours among 32, 33 and empty; a reversed read in front of a forward one: their blocks
    # are neighbours when both strands are scanned
    order = [(n, False) for n in (L, 0, L + 1, L + 1, L, L, L + 1, 0, 0, L)]
    order += [(L + 1, True), (L, False), (L, True), (L + 1, False), (L, True), (L, False), (L + 1, True), (L + 1, False)]
    for n, rev in order:
        if n == 0:
            nb.add_plain(np.full(40, N_, dtype=np.uint8), empty=True)
        else:
            a = take(n * (STRETCH + 1))
            nb.add(block_read(rng, ref, a, [STRETCH] * n), a, rev, kind="plain", rows_n=n, kept=(0,))
    return d, nb



FAMILIES = {"distances": distances, "drop": drop, "ties": ties, "alignment": alignment, "blocks": blocks}


def designs(family=None) -> list:
    return [d for f, make in FAMILIES.items() if family in (None, f) for d in make()]


def all_batches() -> list:
    return [b for d in designs() for b in d.batches()]
