"""-depth on the checker side: the depth of coverage of a pileup table in its run-length form, straight from the definition of
DESIGN.md 4.20, and the files of the front end.  numpy and Python integers, no engine.  Builds on map_spec (the cut of a record's
name); restates nothing.

table is n x 6 (A C G T D I, as counts() gives it); d(p) is the sum of row p's first five counters, a Python integer.  Levels are
t_1 < ... < t_m, m from 0 to 16, each an integer in [1, 2^32).  The value of a row is v(p) = d(p) when m == 0, else the number of i
with t_i <= d(p), 0 to m.  For a range [first, first + count) inside [0, n], row p is a head iff p == first or v(p) != v(p - 1).
The result is the heads in ascending order as (pos, value): run i spans [pos[i], pos[i + 1]), the last one ends at first + count,
an empty range has no runs, runs of depth 0 are included -- the runs tile the range.

For bounds non-decreasing in [first, first + count] and min_depth in [1, 2^31), cum[j] = (sum of d(p), number of p with
d(p) >= min_depth) over rows first <= p < bounds[j].

A range is a slice: head-ness depends on v(p) and v(p - 1) only (and p == first makes a head of whatever row the range begins
with), so the runs of any range are the whole table's runs clipped to it, and cum of a range differs from the whole's by the
constant pair at `first`."""
import numpy as np

import map_spec


def check_levels(levels) -> list:
    lv = [int(t) for t in levels]
    if len(lv) > 16 or any(not 1 <= t < 2 ** 32 for t in lv) or any(a >= b for a, b in zip(lv, lv[1:])):
        raise ValueError("levels %r" % (levels,))
    return lv


def depth(table) -> list:
    """d(p) of every row, Python integers (five counters below 2^32 each: their sum is exact in 64 bits)."""
    a = np.asarray(table)[:, :5]
    assert a.min(initial=0) >= 0 and a.max(initial=0) < 2 ** 32
    return [int(x) for x in a.astype(np.uint64).sum(axis=1, dtype=np.uint64)]


def value(d: int, levels) -> int:
    return d if not levels else sum(1 for t in levels if t <= d)


def runs(table, levels=(), first: int = 0, count=None):
    """(pos, value) of rows [first, first + count): two uint64 arrays."""
    lv = check_levels(levels)
    n = len(table)
    count = n - first if count is None else count
    assert 0 <= first <= n and 0 <= count <= n - first
    d = depth(np.asarray(table)[max(first - 1, 0):first + count])
    v = [value(x, lv) for x in d]
    off = first - max(first - 1, 0)  # v[off] is row `first`
    pos, val = [], []
    for p in range(first, first + count):
        i = p - first + off
        if p == first or v[i] != v[i - 1]:
            pos.append(p)
            val.append(v[i])
    return np.array(pos, dtype=np.uint64), np.array(val, dtype=np.uint64)


def cum(table, min_depth: int = 1, first: int = 0, bounds=()):
    """cum[j] over rows [first, bounds[j]): a uint64 array of shape (m, 2)."""
    assert 1 <= min_depth < 2 ** 31
    b = [int(x) for x in bounds]
    assert all(first <= x <= len(table) for x in b) and all(x <= y for x, y in zip(b, b[1:]))
    d = depth(np.asarray(table)[first:max(b, default=first)])
    sums, covered = [0], [0]  # in front of row first + i
    for y in d:
        sums.append(sums[-1] + y)
        covered.append(covered[-1] + (y >= min_depth))
    return np.array([(sums[x - first], covered[x - first]) for x in b], dtype=np.uint64).reshape(len(b), 2)


def hundredths(q: int) -> bytes:
    return b"%d.%02d" % divmod(q, 100)


def records(loaded):
    """(name cut as -vcf and -cons cut it, first row, size) of every record of a hostlib.Loaded of the merged reference."""
    starts = loaded.merged_start if loaded.s.num > 1 else [0]
    return [(map_spec.cut_name(loaded.names[r]), int(starts[r]), int(loaded.sizes[r])) for r in range(len(starts))]


def bedgraph_file(table, loaded, levels=()) -> bytes:
    """The -depth file: a line name, start, end, value per run, 0-based, half-open and local to the record; the runs are clipped
    to the records (a separator's row belongs to no record), runs of depth 0 included."""
    out = []
    for name, a, size in records(loaded):
        pos, val = runs(table, levels, a, size)
        ends = [int(x) for x in pos[1:]] + [a + size]
        for s, e, v in zip(pos, ends, val):
            out.append(b"%s\t%d\t%d\t%d\n" % (name, int(s) - a, e - a, int(v)))
    return b"".join(out)


def window_file(table, loaded, n: int) -> bytes:
    """The -depth -win n file: a line name, start, end, mean per window of n rows of each record, the last one shorter; the mean
    is 100 * sum // rows, printed as whole.two digits."""
    assert n >= 1
    out = []
    for name, a, size in records(loaded):
        d = depth(np.asarray(table)[a:a + size])
        for s in range(0, size, n):
            e = min(s + n, size)
            out.append(b"%s\t%d\t%d\t%s\n" % (name, s, e, hundredths(100 * sum(d[s:e]) // (e - s))))
    return b"".join(out)


def summary_lines(table, loaded, min_depth: int = 1) -> bytes:
    """What -depth writes to stderr: a line per record with its length, its rows of depth >= min_depth, their share and the mean
    depth, in the integer formatting of the windows."""
    out = []
    for name, a, size in records(loaded):
        d = depth(np.asarray(table)[a:a + size])
        cov = sum(1 for y in d if y >= min_depth)
        out.append(b"> Depth of %s: %d positions, %d covered (%s %%), mean depth %s\n" %
                   (name, size, cov, hundredths(10000 * cov // size if size else 0), hundredths(100 * sum(d) // size if size else 0)))
    return b"".join(out)
