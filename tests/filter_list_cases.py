"""Designed -mem lists for the three list filters behind K9 (-chain, -smem, -mum), built to sit on the block-size limits
of their kernels and on the edges inside them.  Pure numpy, seeded; tests/test_filter_list_cases.py asserts from the
specs alone that the lists reach what is said here, tests/test_gpu_filter_lists.py runs them through the product.

The limits (test_filter_list_cases.py reads them from the kernels' constexpr lines, so the cases cannot drift off them):
  -chain  a lane handles blocks of up to CHAIN_LANE_MAX rows, a wave larger ones in LDS tiles of CHAIN_TILE rows, CHAIN_TRIP
          candidate rows a trip (the wave's width); the tiles are cut from the block's END: [n - 1024, n), [n - 2048, n - 1024) ...
  -smem   a lane up to SMEM_LANE_MAX rows, a workgroup larger ones in tiles of SMEM_TILE rows, SMEM_ITEMS rows a thread (a
          wave: 512 rows); the forward pass cuts from the block's start, the backward pass from its end
  -mum    a lane tests all pairs up to MUM_PAIR_MAX rows, larger blocks go through two radix sorts and finish()

A row is (p, q, L): p in the reference, q in the scanned strand.  Every block is in the emission order (q descending, then
L non-increasing) except the ones of the out-of-order cases.  A Case is one call of the door: a batch of blocks, the
filter's parameter, and per block what it was built for (`meta`).
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

CHAIN_LANE_MAX, CHAIN_TILE, CHAIN_WAVE_GRID, CHAIN_TRIP = 32, 1024, 2048, 64
SMEM_LANE_MAX, SMEM_TILE, SMEM_ITEMS, SMEM_WG, SMEM_LARGE_GRID = 256, 2048, 8, 256, 256
MUM_PAIR_MAX = 256
SMEM_WAVE_ROWS = 64 * SMEM_ITEMS

CHAIN_SIZES = [0, 1, 2, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 1023, 1024, 1025, 1087, 1088, 1089, 2047, 2048, 2049, 3073]
SMEM_SIZES = [0, 1, 2, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 6145]
MUM_SIZES = [0, 1, 2, 3, 255, 256, 257, 258, 1000, 5000]
GAPS = [1, 50, 5000, 2**31 - 1]
FAR_K = [1, 63, 64, 65, 1023, 1024, 1025]
CONTAINER_D = [1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049]
RUN_LENGTHS = [1, 2, 8, 9, 513, 2100]
END64_TOP = 2**32 - 2  # the q of row 0 in the lists with 64-bit ends
BIG = 2**31  # "large coordinates": p and q between 2^31 and 2^32 - 1 - L


@dataclasses.dataclass
class Case:
    name: str
    filter: str            # "chain", "smem", "mum"
    blocks: list           # (n, 3) int64 arrays
    gap: int = 0           # -chain (0: the default, 5000)
    max_occ: int = 0       # -smem
    meta: list = None      # a dict per block
    slack: int = 0         # capacity = rows + slack

    def __post_init__(self):
        self.blocks = [np.asarray(b, dtype=np.int64).reshape(-1, 3) for b in self.blocks]
        if self.meta is None:
            self.meta = [{} for _ in self.blocks]
        assert len(self.meta) == len(self.blocks)

    @property
    def rows(self) -> int:
        return sum(len(b) for b in self.blocks)

    def batch(self):
        """(all rows, block offsets)"""
        tri = np.concatenate(self.blocks) if self.blocks else np.zeros((0, 3), np.int64)
        return tri.reshape(-1, 3), np.concatenate([[0], np.cumsum([len(b) for b in self.blocks])]).astype(np.int64)

    def __repr__(self):
        return self.name


def rows3(p, q, ln) -> np.ndarray:
    return np.stack([np.asarray(p, np.int64), np.asarray(q, np.int64), np.asarray(ln, np.int64)], axis=1)


def emission_sort(a: np.ndarray) -> np.ndarray:
    """q descending, then L descending (stable: rows of one (q, L) keep their order)."""
    return a[np.lexsort((-a[:, 2], -a[:, 1]))]


def shifted(a: np.ndarray, dp: int, dq: int) -> np.ndarray:
    b = a.copy()
    b[:, 0] += dp
    b[:, 1] += dq
    return b


# ---- -chain -------------------------------------------------------------------------------------------------------------------
def one_diagonal(n: int, gap: int) -> np.ndarray:
    """n rows of 5 letters on one diagonal, min(gap, 2) letters apart: every row links to the next one, every row is kept.
    From gap 2 on a row's best link is reached by its two nearest rows alike (the smaller index takes it)."""
    q = (n - 1 - np.arange(n)) * min(gap, 2) + 3
    return rows3(q + 700, q, np.full(n, 5))


def two_chains(n: int, gap: int) -> np.ndarray:
    """Two chains of n // 2 rows each, interleaved row by row, on diagonals a million apart (a link between them gains
    nothing): equal scores, the chain that ends in row 0 wins.  An odd n has one more row behind them that links to nothing."""
    h = n // 2
    k = np.arange(2 * h)
    q = (2 * h - 1 - k) * 1 + 10 if gap >= 2 else (2 * h - 1 - k) // 2 + 10
    # gap 1: the two chains share their q (a start group of two); otherwise rows of a chain are 2 apart
    p = q + 500 + (k % 2) * 1_000_000
    a = rows3(p, q, np.full(2 * h, 6))
    if n % 2:
        a = np.concatenate([a, rows3([3_000_000], [1], [2])])
    return a


def far_predecessor(n: int, i: int, k: int, between: str) -> np.ndarray:
    """Row i's only admissible predecessor is row i + k (same diagonal, k letters back).  Every other row lies a million
    diagonals away with p rising along the block: its dp against any row behind it is <= 0 and a link to rows i, i + k gains
    nothing.  The k - 1 rows between, all inside the q window: `dp`: as the others (dp <= 0 against row i); `end`: 0 < dp but
    they end where row i ends (eq_j == eq_i: not smaller).  The chain is rows i and i + k, its score 2000 + k."""
    assert 0 <= i and i + k < n and k < 2000
    r = np.arange(n)
    q = 10 + (n - 1 - r)
    p = 2_000_000 + r
    ln = np.full(n, 7)
    lo = 500_000
    p[i + k], ln[i + k] = lo, 2000
    p[i], ln[i] = lo + k, 2000
    if between == "end":
        j = np.arange(i + 1, i + k)
        p[j] = lo - 5
        ln[j] = 2000 + (j - i)  # q_j + L_j == q_i + L_i
    return rows3(p, q, ln)


def far_placements(n: int, k: int) -> list:
    """Places of row i: the predecessor in i's tile, in the tile behind it (its f read from global memory), the block's last row
    (the last, partial trip), the first and the last row of a tile."""
    t = n - CHAIN_TILE  # the first row of the last tile
    want = [0, n - 1 - k, t - 1, t - k, t - k - 1, t - 1 - CHAIN_TILE]
    return sorted({i for i in want if 0 <= i and i + k < n})


def window_edge(gap: int, axis: str, kind: str, dist: int, front: int, back: int) -> tuple:
    """Row i (`front` rows in front of it), dist - 1 rows of its own start group, then the edge row: `in`: dq == dp == gap, the
    window's last row, i's predecessor; `out`: one beyond the gap on `axis` (q: it ends the window; p: inside the window, not
    admissible): no predecessor; `both`: the `in` row and the `out` row behind it.  `back` rows behind link to nothing; back 0:
    the window runs past the block's end.  Returns (rows, i, index of the edge row)."""
    li, le = 50, 20
    pe, qe = 100_000, 100_000
    one = [(gap, gap)] if kind != "out" else []
    if kind != "in":
        near = gap if gap > 1 else gap + 1  # gap 1: a link of drift 1 gains nothing, so the row is beyond the gap on both axes
        one.append((gap + 1, near) if axis == "q" else (near, gap + 1))
    # the edge rows are given by (dq, dp) from row i; row i sits `gap` beyond (pe, qe)
    qi, pi = qe + gap, pe + gap
    edge = [(pi - dp, qi - dq, le) for dq, dp in one]
    if len(edge) == 2 and edge[1][1] == edge[0][1]:
        edge[1] = (edge[1][0], edge[1][1], le - 1)  # (axis p: the two share their q)
    f = np.arange(front)
    fr = rows3(1000 + f, qi + (front - f), np.full(front, 9))
    g = np.arange(dist - 1)
    grp = rows3(3000 + g, np.full(dist - 1, qi), np.full(dist - 1, li - 1))
    t = np.arange(back)
    bk = rows3(pi + 10 + t, min(e[1] for e in edge) - 1 - t, np.full(back, 9))
    a = np.concatenate([fr, rows3([pi], [qi], [li]), grp, np.asarray(edge, np.int64).reshape(-1, 3), bk])
    return a, front, front + dist


def start_groups(n: int, gap: int, m: int = 5) -> np.ndarray:
    """Start groups of m rows: one q, L falling, p on m diagonals 3 apart; the groups min(gap, 4) letters apart."""
    r = np.arange(n)
    g, w = r // m, r % m
    q = ((n - 1) // m - g) * min(gap, 4) + 20
    return rows3(q + 1000 + 3 * w, q, 30 - w)


def no_gain(n: int, gap: int) -> np.ndarray:
    """Every row may have predecessors, none gains: from row to row p falls 40 letters more than q.  (A gap of 1 admits none.)"""
    r = np.arange(n)
    q = (n - 1 - r) + 5
    return rows3(q + 40 * (n - 1 - r) + 100, q, np.full(n, 20))


def random_chain_block(n: int, rng, span: int = 0) -> np.ndarray:
    span = span or max(12, n // 3)
    return emission_sort(rows3(rng.integers(0, span, n) + 50, rng.integers(0, span, n) + 50, rng.integers(1, 13, n)))


def chain_sizes(lo: int = 0) -> list:
    return [n for n in CHAIN_SIZES if n >= lo]


@functools.lru_cache(maxsize=None)
def chain_cases() -> list:
    rng = np.random.default_rng(412)
    out = []
    for gap in GAPS:
        for name, fn in (("one_diagonal", one_diagonal), ("two_chains", two_chains), ("start_groups", start_groups), ("no_gain", no_gain)):
            sizes = chain_sizes()
            out.append(Case(f"chain-{name}-G{gap}", "chain", [fn(n, gap) for n in sizes], gap=gap,
                            meta=[{"pattern": name, "n": n} for n in sizes], slack=3 if gap == 50 else 0))
    # far predecessors: gap == k (the predecessor is the window's last row), and the default
    for k in FAR_K:
        blocks, meta = [], []
        for n in sorted({k + 1, k + 34, 129, 1089, 2049, 3073}):
            if n < k + 1:
                continue
            for i in far_placements(n, k):
                for between in ("dp", "end"):
                    if between == "end" and (k == 1 or i not in (0, n - 1 - k)):
                        continue
                    blocks.append(far_predecessor(n, i, k, between))
                    meta.append({"pattern": "far", "n": n, "i": i, "k": k, "between": between})
        # gap == k: the predecessor is the window's last row; the default gap: the `end` rows are inadmissible by their ends alone
        out.append(Case(f"chain-far-k{k}-G{k}", "chain", blocks, gap=k, meta=meta))
        sel = [t for t, m in enumerate(meta) if m["between"] == "end" or m["n"] <= k + 34]
        out.append(Case(f"chain-far-k{k}-G5000", "chain", [blocks[t] for t in sel], gap=5000, meta=[meta[t] for t in sel]))
    for gap in GAPS:
        blocks, meta = [], []
        for axis in "qp":
            for kind in ("in", "out", "both"):
                for dist in (1, 2, 64, 65, 128):
                    for front, back in ((0, 0), (0, 3), (40, 0), (1000, 70)):
                        if front == 1000 and (kind == "both" or dist not in (64, 65)):
                            continue  # (row i in the tile in front of its window's end: the two trips that matter)
                        a, i, e = window_edge(gap, axis, kind, dist, front, back)
                        blocks.append(a)
                        meta.append({"pattern": "window", "axis": axis, "kind": kind, "dist": dist, "i": i, "edge": e, "n": len(a)})
        out.append(Case(f"chain-window-G{gap}", "chain", blocks, gap=gap, meta=meta))
    for gap in (1, 50):
        sizes = chain_sizes()
        out.append(Case(f"chain-random-G{gap}", "chain", [random_chain_block(n, rng) for n in sizes], gap=gap,
                        meta=[{"pattern": "random", "n": n} for n in sizes]))
    # large coordinates: p and q in [2^31, 2^32 - 1 - L]
    top = 2**32 - 1
    blocks, meta = [], []
    for n in (2, 33, 129, 1025, 2049):
        for name, a in (("one_diagonal", one_diagonal(n, 50)), ("random", random_chain_block(n, rng)), ("start_groups", start_groups(n, 50))):
            hi = shifted(a, top - int((a[:, 0] + a[:, 2]).max()), top - int((a[:, 1] + a[:, 2]).max()))  # the largest end is 2^32 - 1
            for b in (hi, shifted(a, BIG - int(a[:, 0].min()), BIG - int(a[:, 1].min()))):              # the smallest start is 2^31
                blocks.append(b)
                meta.append({"pattern": "large-" + name, "n": n})
    out.append(Case("chain-large-coordinates-G50", "chain", blocks, gap=50, meta=meta))
    a, i, e = window_edge(2**31 - 1, "q", "in", 65, 40, 3)
    out.append(Case("chain-large-coordinates-Gmax", "chain", [shifted(a, BIG - 100_000 - 2000, BIG - 100_000 - 2000),
                                                               shifted(one_diagonal(1089, 2), BIG, BIG)], gap=2**31 - 1,
                    meta=[{"pattern": "large-window", "i": i, "edge": e, "n": len(a)}, {"pattern": "large-one_diagonal", "n": 1089}]))
    return out


# ---- -smem --------------------------------------------------------------------------------------------------------------------
def staircase(n: int, q0: int = 100, seed: int = 1) -> np.ndarray:
    """n rows of 10 letters, 2 apart: no interval contains another, every row is an SMEM row."""
    r = np.arange(n)
    p = np.random.default_rng(seed).permutation(n) * 16 + 40
    return rows3(p, q0 + 2 * (n - 1 - r), np.full(n, 10))


def container_b(n: int, i: int, d: int, q0: int = 100) -> np.ndarray:
    """Rule (b): row i + d (a later start group) ends exactly where row i ends; it contains rows i .. i + d - 1 and no other."""
    a = staircase(n, q0)
    a[i + d, 2] = a[i, 1] + a[i, 2] - a[i + d, 1]
    return a


def container_a(n: int, e: int, m: int, q0: int = 100) -> np.ndarray:
    """Rule (a): rows e .. e + m - 1 share the q of row e - 1 and are shorter: row e - 1, the last row of the thread, wave or tile
    in front of them, contains them."""
    a = staircase(n, q0)
    a[e:e + m, 1] = a[e - 1, 1]
    a[e:e + m, 2] = a[e - 1, 2] - 1 - np.arange(m) // 2  # (pairs of equal length: runs inside the group)
    return a


def equal_ends(n: int, q0: int = 100) -> tuple:
    """Every 7th row x gets, 3 rows behind it, a longer row that ends where x ends (x is contained) or one letter before
    (x is not).  Returns (rows, indices of the contained x, indices of the others)."""
    a = staircase(n, q0)
    inn, out = [], []
    for t, x in enumerate(range(0, n - 3, 7)):
        short = t % 2
        a[x + 3, 2] = a[x, 1] + a[x, 2] - a[x + 3, 1] - short
        (out if short else inn).append(x)
    return a, inn, out


def run_block(length: int, edge: int, q0: int = 100) -> tuple:
    """A run of `length` rows of one (q, L), not contained, that starts 3 rows before row `edge`; 5 rows behind it.
    Returns (rows, index of the run's first row)."""
    a = staircase(edge - 3 + 1 + 5, q0)
    s = edge - 3
    run = np.repeat(a[s:s + 1], length, axis=0)
    run[:, 0] = 1_000_000 + 16 * np.arange(length)
    return np.concatenate([a[:s], run, a[s + 1:]]), s


def random_smem_block(n: int, rng) -> np.ndarray:
    span = max(6, n // 4)
    return emission_sort(rows3(rng.integers(0, 10**6, n), rng.integers(0, span, n) + 10, rng.integers(1, max(3, span // 2), n)))


def run_caps() -> list:
    return sorted({0, 1, 2, 5} | {c for ln in RUN_LENGTHS for c in (ln - 1, ln, ln + 1)})


@functools.lru_cache(maxsize=None)
def smem_cases() -> list:
    rng = np.random.default_rng(413)
    out = []
    # containers at a distance; the 64-bit ends: the same lists with row 0 at q = 2^32 - 2 (rows 0 .. 4 end at 2^32 + 8 .. 2^32,
    # row 5 just below: a container of row 0 must be compared in 64 bits)
    for tag, q0 in (("", 100), ("-end64", 0)):
        blocks, meta = [], []
        for d in CONTAINER_D:
            for n in sorted({d + 1, d + 12, SMEM_LANE_MAX + 1 + d, SMEM_TILE + 1 + d}):
                for i in sorted({0, 5, n - 1 - d}):
                    if i + d >= n:
                        continue
                    base = q0 or END64_TOP - 2 * (n - 1)
                    blocks.append(container_b(n, i, d, base))
                    meta.append({"pattern": "container-b", "n": n, "i": i, "container": i + d})
        for e in (SMEM_ITEMS, SMEM_WAVE_ROWS, SMEM_TILE, 2 * SMEM_TILE):
            for m in (1, 3, 9):
                for n in sorted({e + m, e + m + 5, max(e + m + 5, SMEM_LANE_MAX + 44)}):
                    base = q0 or END64_TOP - 2 * (n - 1)
                    blocks.append(container_a(n, e, m, base))
                    meta.append({"pattern": "container-a", "n": n, "i": e, "container": e - 1})
        for n in (40, SMEM_LANE_MAX + 1, SMEM_TILE + 9):
            a, inn, outs = equal_ends(n, q0 or END64_TOP - 2 * (n - 1))
            blocks.append(a)
            meta.append({"pattern": "equal-ends", "n": n, "contained": inn, "free": outs})
        for occ in ((0, 2) if not tag else (0,)):
            out.append(Case(f"smem-containers{tag}-occ{occ}", "smem", blocks, max_occ=occ, meta=meta))
    # runs under every cap
    blocks, meta = [], []
    for ln in RUN_LENGTHS:
        for edge in (SMEM_ITEMS, SMEM_WAVE_ROWS, SMEM_TILE):
            a, s = run_block(ln, edge)
            blocks.append(a)
            meta.append({"pattern": "run", "n": len(a), "start": s, "length": ln})
    for occ in run_caps():
        out.append(Case(f"smem-runs-occ{occ}", "smem", blocks, max_occ=occ, meta=meta))
    for occ in (0, 1, 2, 5):
        sizes = SMEM_SIZES
        out.append(Case(f"smem-random-occ{occ}", "smem", [random_smem_block(n, rng) for n in sizes], max_occ=occ,
                        meta=[{"pattern": "random", "n": n} for n in sizes], slack=4 if occ == 1 else 0))
    return out


# ---- -mum ---------------------------------------------------------------------------------------------------------------------
MUM_KINDS = ["q-only", "p-only", "equal-interval", "equal-start", "equal-end", "duplicate"]


def mum_block(n: int, rng, p0: int = 40, q0: int = 40) -> tuple:
    """n rows of 10 letters, 20 apart in q and, in another order, in p: no row contains another.  Then of every 4 rows (a, b)
    one pair is rewritten by one of MUM_KINDS in turn.  Returns (rows, per row: the kind that rewrote it or '')."""
    r = np.arange(n)
    a = rows3(p0 + rng.permutation(n) * 20, q0 + 20 * (n - 1 - r), np.full(n, 10))
    kinds = [""] * n
    for t, x in enumerate(range(0, n - 1, 4)):
        kind, y = MUM_KINDS[t % len(MUM_KINDS)], x + 1
        pa, qa, la = (int(v) for v in a[x])
        if kind == "q-only":
            a[y, 1], a[y, 2] = qa + 2, 5
        elif kind == "p-only":
            a[y, 0], a[y, 2] = pa + 2, 5
        elif kind == "equal-interval":   # both go
            a[y, 1], a[y, 2] = qa, la
        elif kind == "equal-start":      # the shorter goes
            a[y, 1], a[y, 2] = qa, la - 3
        elif kind == "equal-end":
            a[y, 1], a[y, 2] = qa + 3, la - 3
        else:
            a[y] = a[x]
        kinds[y] = kind
    return a, kinds


@functools.lru_cache(maxsize=None)
def mum_cases() -> list:
    rng = np.random.default_rng(414)
    out = []
    blocks, meta = [], []
    for n in MUM_SIZES:
        a, kinds = mum_block(n, rng)
        perm = rng.permutation(n)
        for tag, b, pm in (("emitted", emission_sort(a), None), ("as built", a, np.arange(n)), ("shuffled", a[perm], perm)):
            blocks.append(b)
            meta.append({"pattern": tag, "n": n, "of": len(blocks) - (2 if tag == "shuffled" else 1), "perm": pm, "kinds": kinds})
    out.append(Case("mum-kinds", "mum", blocks, meta=meta))
    blocks, meta = [], []
    for n in (3, 256, 257, 1000):
        a, kinds = mum_block(n, rng)
        top = 2**32 - 1
        for b in (shifted(a, top - int((a[:, 0] + a[:, 2]).max()), top - int((a[:, 1] + a[:, 2]).max())),
                  shifted(a, BIG - int(a[:, 0].min()), BIG - int(a[:, 1].min()))):
            perm = rng.permutation(n)
            blocks += [b, b[perm]]
            meta += [{"pattern": "large", "n": n, "kinds": kinds}, {"pattern": "large-shuffled", "n": n, "of": len(blocks) - 2, "perm": perm}]
    out.append(Case("mum-large-coordinates", "mum", blocks, meta=meta, slack=5))
    return out


# ---- batches ------------------------------------------------------------------------------------------------------------------
def shuffled_with_empties(blocks: list, rng) -> tuple:
    """The blocks in a random order, an empty block behind every third."""
    order = rng.permutation(len(blocks))
    out, sizes = [], []
    for t, k in enumerate(order):
        out.append(blocks[k])
        if t % 3 == 0:
            out.append(np.zeros((0, 3), np.int64))
    return out, [len(b) for b in out]


@functools.lru_cache(maxsize=None)
def batch_cases() -> list:
    rng = np.random.default_rng(415)
    out = []
    for slack in (0, 5):
        b, sizes = shuffled_with_empties([random_chain_block(n, rng) if n % 2 else one_diagonal(n, 50) for n in CHAIN_SIZES], rng)
        out.append(Case(f"batch-chain-sizes-slack{slack}", "chain", b, gap=50, slack=slack, meta=[{"n": n} for n in sizes]))
        b, sizes = shuffled_with_empties([random_smem_block(n, rng) for n in SMEM_SIZES], rng)
        out.append(Case(f"batch-smem-sizes-slack{slack}", "smem", b, max_occ=2, slack=slack, meta=[{"n": n} for n in sizes]))
        b, sizes = shuffled_with_empties([mum_block(n, rng)[0] for n in MUM_SIZES], rng)
        out.append(Case(f"batch-mum-sizes-slack{slack}", "mum", b, slack=slack, meta=[{"n": n} for n in sizes]))
    # more listed blocks than the fixed grids take in one pass; -mum: the block ordinal of the sort key needs a second digit
    out.append(Case("batch-chain-2100x33", "chain", [random_chain_block(33, rng) for _ in range(CHAIN_WAVE_GRID + 52)], gap=50))
    out.append(Case("batch-smem-260x257", "smem", [random_smem_block(257, rng) for _ in range(SMEM_LARGE_GRID + 4)], max_occ=2, slack=5))
    out.append(Case("batch-mum-300x257", "mum", [mum_block(257, rng)[0][rng.permutation(257)] for _ in range(300)]))
    return out


# ---- out of the emission order ------------------------------------------------------------------------------------------------
def violated(a: np.ndarray, i: int, how: str) -> np.ndarray:
    """One violation between rows i and i + 1: `q`: q ascending; `L`: equal q, L ascending."""
    b = a.copy()
    if how == "q":
        b[i + 1, 1] = b[i, 1] + 1
    else:
        b[i + 1, 1] = b[i, 1]
        b[i + 1, 2] = b[i, 2] + 1
    return b


ORDER_SIZES = {"chain": ([2, 32, 33, 2049], [0, "n-2", 1023]), "smem": ([2, 256, 257, 4097], [0, "n-2", 7, 511, 2047])}


def _good(filt: str, n: int, rng) -> np.ndarray:
    return one_diagonal(n, 50) if filt == "chain" else staircase(n)


@functools.lru_cache(maxsize=None)
def order_cases() -> list:
    """Batches of 16 blocks: one bad block (number 5) among good ones, for every size, place and kind of violation; and two bad
    blocks, numbers 3 (small: a lane's) and 11 (listed: a wave's or a workgroup's)."""
    rng = np.random.default_rng(416)
    out = []
    for filt, (sizes, places) in ORDER_SIZES.items():
        small, listed = sizes[1], sizes[2]
        good = [_good(filt, n, rng) for n in (0, 1, 5, small, listed, 40, 3, listed + 30, 2, 0, 77, 9, 1, small - 1, listed + 1, 6)]
        for n in sizes:
            for i in sorted({n - 2 if pl == "n-2" else pl for pl in places}):
                if not 0 <= i <= n - 2:
                    continue
                for how in "qL":
                    blocks = list(good)
                    blocks[5] = violated(_good(filt, n, rng), i, how)
                    out.append(Case(f"order-{filt}-n{n}-i{i}-{how}", filt, blocks, gap=50, max_occ=0,
                                    meta=[{"bad": k == 5} for k in range(16)]))
        for how in "qL":
            blocks = list(good)
            blocks[3] = violated(_good(filt, small, rng), small // 2, how)
            blocks[11] = violated(_good(filt, listed, rng), listed - 2, how)
            out.append(Case(f"order-{filt}-two-{how}", filt, blocks, gap=50, meta=[{"bad": k in (3, 11)} for k in range(16)]))
            blocks = list(good)  # the other way round: the listed block has the smaller number
            blocks[3] = violated(_good(filt, listed, rng), 0, how)
            blocks[11] = violated(_good(filt, small, rng), small - 2, how)
            out.append(Case(f"order-{filt}-two-listed-first-{how}", filt, blocks, gap=50, meta=[{"bad": k in (3, 11)} for k in range(16)]))
    return out


def all_cases() -> list:
    return chain_cases() + smem_cases() + mum_cases() + batch_cases()


# ---- the specs applied to a case (computed once, shared by the tests) ---------------------------------------------------------
def as_mems(tri: np.ndarray) -> np.ndarray:
    m = np.zeros(len(tri), dtype=[("ref_pos", "<i8"), ("query_pos", "<i8"), ("length", "<i8")])
    m["ref_pos"], m["query_pos"], m["length"] = tri[:, 0], tri[:, 1], tri[:, 2]
    return m


_EXPECTED = {}


def expected(case: Case):
    """(kept rows, new offsets, scores or None) by the filter's spec."""
    if case.name not in _EXPECTED:
        import chain_spec
        import mum_spec
        import smem_spec
        tri, boff = case.batch()
        if case.filter == "chain":
            res = chain_spec.filter_blocks(tri, boff, case.gap or chain_spec.DEFAULT_GAP, windowed=True)
        elif case.filter == "smem":
            res = smem_spec.filter_blocks(tri, boff, case.max_occ) + (None,)
        else:
            res = mum_spec.filter_blocks(as_mems(tri), boff) + (None,)
        _EXPECTED[case.name] = res
    return _EXPECTED[case.name]
