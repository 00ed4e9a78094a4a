"""-smem on the checker side: the super-maximal filter of a strand block's -mem rows, the run lengths the occurrence cap uses,
the two claims of DESIGN.md 4.11 stated by naive substring search, and the filter applied to a golden case's -mem file
(tests/golden/<case>/expected-mems.txt, written by the real reference).

A row (p, q, L) of a block is an SMEM row when no other row of the same block has a query interval [q', q'+L') that strictly
contains [q, q+L) (contains it and differs from it).  Rows of one interval on different diagonals are its occurrences: kept
or dropped together.  The cap max_occ > 0 drops the SMEM rows whose interval more than max_occ rows of the block share.

The checker does not use the emission order the engine relies on: it sorts the block's distinct intervals itself."""
import numpy as np

import hostlib
import mum_spec


def _tri(rows) -> np.ndarray:
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3)


def smem_keep(rows) -> np.ndarray:
    """rows: (n, 3) array of (ref_pos, query_pos, length) of ONE block, in any order.  Returns a bool mask of the rows whose
    query interval no other row's interval strictly contains."""
    a = _tri(rows)
    if a.shape[0] == 0:
        return np.ones(0, dtype=bool)
    q, e = a[:, 1], a[:, 1] + a[:, 2]
    iv, inv = np.unique(np.stack([q, e], axis=1), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    # distinct intervals by start ascending, end descending: an interval is strictly contained iff an interval before it in
    # this order (a smaller start, or the same start and a larger end) ends at or after its end
    order = np.lexsort((-iv[:, 1], iv[:, 0]))
    ends = iv[order, 1]
    before = np.concatenate([[-1], np.maximum.accumulate(ends)[:-1]])
    contained = np.zeros(len(iv), dtype=bool)
    contained[order] = before >= ends
    return ~contained[inv]


def occurrence_counts(rows) -> np.ndarray:
    """Per row: the rows of its block with the same query interval (q, L), itself included."""
    a = _tri(rows)
    if a.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    _, inv, cnt = np.unique(a[:, 1:], axis=0, return_inverse=True, return_counts=True)
    return cnt[inv.reshape(-1)]


def block_keep(rows, max_occ: int = 0) -> np.ndarray:
    keep = smem_keep(rows)
    if max_occ:
        keep &= occurrence_counts(rows) <= max_occ
    return keep


def in_emission_order(rows) -> bool:
    """Query start descending, then length non-increasing (slamem.c:114-193: j runs from the end of the query to its start,
    the match only shrinks while the parent intervals widen)."""
    a = _tri(rows)
    if a.shape[0] < 2:
        return True
    dq = np.diff(a[:, 1])
    dl = np.diff(a[:, 2])
    return bool(np.all((dq < 0) | ((dq == 0) & (dl <= 0))))


def runs_adjacent(rows) -> bool:
    """The rows of one query interval follow each other."""
    a = _tri(rows)
    if a.shape[0] == 0:
        return True
    change = np.concatenate([[True], np.any(a[1:, 1:] != a[:-1, 1:], axis=1)])
    return len(np.unique(a[:, 1:], axis=0)) == int(change.sum())


def occurrences(hay: bytes, s: bytes) -> int:
    """Occurrences of s in hay, overlapping ones included."""
    n, at = 0, hay.find(s)
    while at != -1:
        n += 1
        at = hay.find(s, at + 1)
    return n


def claim1_keep(text: bytes, strand: bytes, rows) -> np.ndarray:
    """Claim 1 by substring search: the row's string extended by one letter to the left (when q > 0) and by one to the right
    (when q + L < |strand|) occurs nowhere in the merged text."""
    a = _tri(rows)
    out = np.zeros(a.shape[0], dtype=bool)
    for k, (p, q, ln) in enumerate(a):
        assert text[p:p + ln] == strand[q:q + ln], "not a match"
        left = q > 0 and text.find(strand[q - 1:q + ln]) != -1
        right = q + ln < len(strand) and text.find(strand[q:q + ln + 1]) != -1
        out[k] = not left and not right
    return out


def claim2_counts(text: bytes, strand: bytes, rows) -> np.ndarray:
    """Claim 2 by substring search: the occurrences of each row's string in the merged text."""
    return np.array([occurrences(text, strand[q:q + ln]) for _, q, ln in _tri(rows)], dtype=np.int64)


def filter_blocks(mems, block_offsets, max_occ: int = 0):
    """The -smem filter of a -mem result as the engine returns it (a structured array or (n, 3) triples and the block
    offsets): (kept rows as (n, 3) int64 triples, new block offsets)."""
    if hasattr(mems, "dtype") and mems.dtype.names:
        tri = np.stack([mems["ref_pos"], mems["query_pos"], mems["length"]], axis=1).astype(np.int64) if len(mems) else \
            np.zeros((0, 3), dtype=np.int64)
    else:
        tri = _tri(mems)
    boff = np.asarray(block_offsets, dtype=np.int64)
    keep = np.zeros(len(tri), dtype=bool)
    for b in range(len(boff) - 1):
        keep[boff[b]:boff[b + 1]] = block_keep(tri[boff[b]:boff[b + 1]], max_occ)
    ck = np.concatenate([[0], np.cumsum(keep.astype(np.int64))])
    return tri[keep], ck[boff]


def golden_smem_file(case, max_occ: int = 0):
    """The -smem filter of the file the real reference wrote for the -mem case, formatted by the front end's writer.
    Returns (expected -smem file bytes, per-block kept rows, reference, queries, options)."""
    ref, qs, opts, exp_mems = mum_spec.golden_inputs(case)
    data = open(exp_mems, "rb").read()
    blocks = mum_spec.parse_mems_file(data, ref)
    strands = 2 if "-b" in opts else 1
    assert len(blocks) == qs.n * strands
    out, rows_kept = [], []
    for b, (_, rows) in enumerate(blocks):
        name, s = qs.names[b // strands], b % strands
        k = rows[block_keep(rows, max_occ)]
        rows_kept.append(k)
        out.append(hostlib.format_block(name, s, k, ref))
    return b"".join(out), rows_kept, ref, qs, opts
