"""-mum on the checker side: the containment filter of a strand block's -mem rows, the naive occurrence count it must equal,
and the filter applied to a golden case's -mem file (tests/golden/<case>/expected-mems.txt, written by the real reference).

A row (p, q, L) of a block is a MUM when no OTHER row of the same block contains it in query coordinates ([q', q'+L') covers
[q, q+L)) nor in reference coordinates (p merged).  Given the complete -mem list this is "the string occurs once in the merged
reference and once in the scanned strand" (DESIGN.md 4.10)."""
import numpy as np

import hostlib
from golden_cases import MANIFEST, case_paths, opt_value


def containment_keep(rows) -> np.ndarray:
    """rows: (n, 3) array of (ref_pos, query_pos, length) of ONE block.  Returns a bool mask of the rows to keep."""
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    n = a.shape[0]
    if n <= 1:
        return np.ones(n, dtype=bool)
    p, q, ln = a[:, 0], a[:, 1], a[:, 2]
    pe, qe = p + ln, q + ln
    # [j, i]: row j contains row i
    cq = (q[:, None] <= q[None, :]) & (qe[:, None] >= qe[None, :])
    cp = (p[:, None] <= p[None, :]) & (pe[:, None] >= pe[None, :])
    c = cq | cp
    np.fill_diagonal(c, False)
    return ~c.any(axis=0)


def occurrences(hay: bytes, s: bytes, stop: int = 2) -> int:
    """Occurrences of s in hay, overlapping ones included, counted up to `stop`."""
    n, at = 0, hay.find(s)
    while at != -1 and n < stop:
        n += 1
        at = hay.find(s, at + 1)
    return n


def naive_keep(text: bytes, strand: bytes, rows) -> np.ndarray:
    """The definition by counting: the row's string occurs exactly once in the text and once in the strand."""
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    out = np.zeros(a.shape[0], dtype=bool)
    for k, (p, q, ln) in enumerate(a):
        s = strand[q:q + ln]
        assert text[p:p + ln] == s, "not a match"
        out[k] = occurrences(text, s) == 1 and occurrences(strand, s) == 1
    return out


def golden_inputs(case):
    """The case's reference (merged, as the front end loads it) and queries, and its options."""
    opts = MANIFEST[case]["opts"]
    ref_fa, q_fa, exp_mems, _ = case_paths(case)
    acgt = 1 if "-n" in opts else 0
    m = int(opt_value(opts, "-m", 0))
    ref = hostlib.Loaded(ref_fa, 1, acgt, m, opt_value(opts, "-r"))
    qs = hostlib.Loaded(q_fa, 0, acgt, m, None)
    return ref, qs, opts, exp_mems


def parse_mems_file(data: bytes, ref):
    """Blocks of a -mem file in order: (header line, (n, 3) uint32 array of 0-based triples in merged coordinates)."""
    starts = {name: int(st) for name, st in zip(ref.names, ref.merged_start)}
    blocks = []
    for line in data.split(b"\n")[:-1]:
        if line.startswith(b">"):
            blocks.append((line, []))
            continue
        f = line.split(b"\t")
        if len(f) == 4:  # " <record name>\t" in front when the reference has several records
            p = starts[f[0][1:]] + int(f[1]) - 1
        else:
            p = int(f[0]) - 1
        blocks[-1][1].append((p, int(f[-2]) - 1, int(f[-1])))
    return [(h, np.array(r, dtype=np.uint32).reshape(-1, 3)) for h, r in blocks]


def golden_mum_file(case):
    """The containment filter of the file the real reference wrote for the -mem case, formatted by the front end's writer
    (the unfiltered rows are formatted too and must give the file back: the parse is checked).  Returns
    (expected -mum file bytes, per-block kept rows, reference, queries, options)."""
    ref, qs, opts, exp_mems = golden_inputs(case)
    data = open(exp_mems, "rb").read()
    blocks = parse_mems_file(data, ref)
    strands = 2 if "-b" in opts else 1
    assert len(blocks) == qs.n * strands
    whole, kept, rows_kept = [], [], []
    for b, (_, rows) in enumerate(blocks):
        name, s = qs.names[b // strands], b % strands
        whole.append(hostlib.format_block(name, s, rows, ref))
        k = rows[containment_keep(rows)]
        rows_kept.append(k)
        kept.append(hostlib.format_block(name, s, k, ref))
    assert b"".join(whole) == data
    return b"".join(kept), rows_kept, ref, qs, opts


def filter_blocks(mems, block_offsets):
    """The containment filter of a -mem result as the engine returns it: (kept rows, new block offsets)."""
    tri = np.stack([mems["ref_pos"], mems["query_pos"], mems["length"]], axis=1).astype(np.int64) if len(mems) else \
        np.zeros((0, 3), dtype=np.int64)
    boff = np.asarray(block_offsets, dtype=np.int64)
    keep = np.zeros(len(tri), dtype=bool)
    for b in range(len(boff) - 1):
        keep[boff[b]:boff[b + 1]] = containment_keep(tri[boff[b]:boff[b + 1]])
    ck = np.concatenate([[0], np.cumsum(keep.astype(np.int64))])
    return tri[keep], ck[boff]
