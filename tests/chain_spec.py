"""-chain on the checker side: the best collinear chain of a strand block's -mem rows straight from the definition of
DESIGN.md 4.12, and the filter applied to a -mem result or to a golden case's -mem file (tests/golden/<case>/expected-mems.txt,
written by the real reference).

Rows are (p, q, L): p in the merged reference, q in the scanned strand.  With eq = q + L, ep = p + L and the maximum gap G >= 1:

  row j may precede row i   iff  0 < q_i - q_j <= G,  0 < p_i - p_j <= G,  eq_j < eq_i,  ep_j < ep_i
  link(j, i)                =    min(L_i, eq_i - eq_j, ep_i - ep_j) - |(p_i - q_i) - (p_j - q_j)|
  f(i)                      =    max(L_i, max over j that may precede i of f(j) + link(j, i))

The predecessor of i is taken only if it gives strictly more than L_i; among the j that reach the maximum, the one with the
smallest index (the row's place in the block as given).  The chain ends in the row of the largest f, smallest index on ties;
the block's chain is that row and its predecessors, its score that f (0 for an empty block).

The checker does not use the order the engine relies on: it evaluates the rows by (q, p) ascending -- a row that may precede
another has a smaller q -- and tests every pair.  Python integers: no overflow."""
import numpy as np

import hostlib
import mum_spec

DEFAULT_GAP = 5000


def _tri(rows) -> np.ndarray:
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3)


def may_precede(rj, ri, gap: int) -> bool:
    pj, qj, lj = (int(x) for x in rj)
    pi, qi, li = (int(x) for x in ri)
    return 0 < qi - qj <= gap and 0 < pi - pj <= gap and qj + lj < qi + li and pj + lj < pi + li


def link(rj, ri) -> int:
    pj, qj, lj = (int(x) for x in rj)
    pi, qi, li = (int(x) for x in ri)
    return min(li, (qi + li) - (qj + lj), (pi + li) - (pj + lj)) - abs((pi - qi) - (pj - qj))


def chain_dp(rows, gap: int = DEFAULT_GAP):
    """rows: the (p, q, L) rows of ONE block, index = place in `rows`.  Returns (f, pred): lists of the best score of a chain
    ending in each row and its predecessor (-1: none)."""
    a = [tuple(int(x) for x in r) for r in _tri(rows)]
    n = len(a)
    f = [r[2] for r in a]
    pred = [-1] * n
    for i in sorted(range(n), key=lambda k: (a[k][1], a[k][0])):
        best, arg = a[i][2], -1
        for j in range(n):  # ascending: the first j that reaches a value keeps it (smallest index)
            if may_precede(a[j], a[i], gap):
                s = f[j] + link(a[j], a[i])
                if s > best:
                    best, arg = s, j
        f[i], pred[i] = best, arg
    return f, pred


def chain_dp_windowed(rows, gap: int = DEFAULT_GAP):
    """The same values for a block whose rows come with q non-increasing (the emission order): vectorised over each row's
    window, for blocks too large for chain_dp's pair loop."""
    a = _tri(rows)
    n = len(a)
    p, q, ln = a[:, 0], a[:, 1], a[:, 2]
    assert n == 0 or bool(np.all(np.diff(q) <= 0))
    f = ln.copy()
    pred = -np.ones(n, dtype=np.int64)
    nq = -q  # ascending
    for i in range(n - 1, -1, -1):
        lo = int(np.searchsorted(nq, -q[i], side="right"))         # first row with q < q_i
        hi = int(np.searchsorted(nq, -(q[i] - gap), side="right"))  # first row with q < q_i - G
        if lo >= hi:
            continue
        dq, dp = q[i] - q[lo:hi], p[i] - p[lo:hi]
        de = ln[i] - ln[lo:hi]
        ok = (dp > 0) & (dp <= gap) & (dq + de > 0) & (dp + de > 0)
        if not ok.any():
            continue
        s = f[lo:hi] + np.minimum(ln[i], np.minimum(dq + de, dp + de)) - np.abs(dp - dq)
        s = np.where(ok, s, -1)
        k = int(np.argmax(s))  # (the first maximum: smallest index)
        if s[k] > ln[i]:
            f[i], pred[i] = s[k], lo + k
    return [int(x) for x in f], [int(x) for x in pred]


def block_chain(rows, gap: int = DEFAULT_GAP, windowed: bool = False):
    """(kept mask, score) of one block."""
    a = _tri(rows)
    n = len(a)
    keep = np.zeros(n, dtype=bool)
    if n == 0:
        return keep, 0
    f, pred = (chain_dp_windowed if windowed else chain_dp)(a, gap)
    end = max(range(n), key=lambda k: (f[k], -k))
    i = end
    while i >= 0:
        keep[i] = True
        i = pred[i]
    return keep, int(f[end])


def chain_score(rows, gap: int = DEFAULT_GAP):
    """The score of `rows` read as ONE chain in the given order (first row first), or None when a row may not precede the
    next."""
    a = _tri(rows)
    if len(a) == 0:
        return 0
    s = int(a[0][2])
    for j in range(len(a) - 1):
        if not may_precede(a[j], a[j + 1], gap):
            return None
        s += link(a[j], a[j + 1])
    return s


def kept_score(kept_rows, gap: int = DEFAULT_GAP):
    """The block score from the kept rows alone, as they stand in the output (q descending: the chain's last row first)."""
    return chain_score(_tri(kept_rows)[::-1], gap)


def in_emission_order(rows) -> bool:
    a = _tri(rows)
    if a.shape[0] < 2:
        return True
    dq, dl = np.diff(a[:, 1]), np.diff(a[:, 2])
    return bool(np.all((dq < 0) | ((dq == 0) & (dl <= 0))))


def filter_blocks(mems, block_offsets, gap: int = DEFAULT_GAP, windowed: bool = False):
    """The -chain filter of a -mem result as the engine returns it (a structured array or (n, 3) triples and the block
    offsets): (kept rows as (n, 3) int64 triples, new block offsets, block scores)."""
    if hasattr(mems, "dtype") and mems.dtype.names:
        tri = np.stack([mems["ref_pos"], mems["query_pos"], mems["length"]], axis=1).astype(np.int64) if len(mems) else \
            np.zeros((0, 3), dtype=np.int64)
    else:
        tri = _tri(mems)
    boff = np.asarray(block_offsets, dtype=np.int64)
    keep = np.zeros(len(tri), dtype=bool)
    scores = np.zeros(len(boff) - 1, dtype=np.int64)
    for b in range(len(boff) - 1):
        keep[boff[b]:boff[b + 1]], scores[b] = block_chain(tri[boff[b]:boff[b + 1]], gap, windowed)
    ck = np.concatenate([[0], np.cumsum(keep.astype(np.int64))])
    return tri[keep], ck[boff], scores


def golden_chain_file(case, gap: int = DEFAULT_GAP):
    """The -chain filter of the file the real reference wrote for the -mem case, formatted by the front end's writer.
    Returns (expected -chain file bytes, per-block kept rows, per-block scores, reference, queries, options)."""
    ref, qs, opts, exp_mems = mum_spec.golden_inputs(case)
    data = open(exp_mems, "rb").read()
    blocks = mum_spec.parse_mems_file(data, ref)
    strands = 2 if "-b" in opts else 1
    assert len(blocks) == qs.n * strands
    out, rows_kept, scores = [], [], []
    for b, (_, rows) in enumerate(blocks):
        name, s = qs.names[b // strands], b % strands
        keep, score = block_chain(rows, gap, windowed=len(rows) > 200)
        k = rows[keep]
        rows_kept.append(k)
        scores.append(score)
        out.append(hostlib.format_block(name, s, k, ref))
    return b"".join(out), rows_kept, scores, ref, qs, opts
