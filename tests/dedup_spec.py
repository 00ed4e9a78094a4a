"""-dedup on the checker side: which reads of an ordered list of adds are duplicates, straight from the definition of DESIGN.md
4.23.  Builds on map_spec (a read_map tuple per read: strand, mapq, s1, s2, segments) and restates nothing of it; pile_spec,
lowq_spec and events_spec then run over the reads that are kept (keep()).

A read is a candidate iff it would contribute to the pileup -- strand != 0 and mapq >= min_mapq -- and has a segment.  Its key is
(strand, u), u the unclipped 5' position in merged-text coordinates, signed, len the read's length:

  strand 1   L = the segment with the smallest query_pos:              u = ref_pos(L) - query_pos(L)               (may be negative)
  strand 2   R = the segment with the largest query_pos + query_len:   u = ref_pos(R) + ref_len(R) + (len - query_pos(R) - query_len(R))
                                                                                                                   (may exceed n)

(the first such segment in the order they are stored; that order is not relied on: min and max).  Every add has a sequence number,
counted from 0 per accumulator; a read's rank is seq << 32 | its index in the batch.  A candidate is a duplicate iff another
candidate with the same key has a smaller rank.  Non-candidates never claim a key and are never duplicates.

Python integers: no overflow."""
import numpy as np

EMPTY = (1 << 64) - 1  # the packed key of an empty slot
UNMAPPED = (0, 0, 0, 0, [])


def is_candidate(result, min_mapq: int = 0) -> bool:
    strand, mapq, _, _, segl = result
    return strand != 0 and mapq >= min_mapq and len(segl) > 0


def unclipped(result, length: int) -> int:
    """u of a mapped read of `length` letters."""
    strand, _, _, _, segl = result
    assert strand in (1, 2) and len(segl) > 0
    if strand == 1:
        best, u = None, 0
        for (p, q, _rlen, _qlen, _ed, _rl) in segl:
            if best is None or int(q) < best:
                best, u = int(q), int(p) - int(q)
        return u
    best, u = None, 0
    for (p, q, rlen, qlen, _ed, _rl) in segl:
        e = int(q) + int(qlen)
        if best is None or e > best:
            best, u = e, int(p) + int(rlen) + (int(length) - e)
    return u


def key(result, length: int, min_mapq: int = 0):
    """(strand, u) of a candidate; None for a read that is none."""
    if not is_candidate(result, min_mapq):
        return None
    return int(result[0]), unclipped(result, length)


def packed(k) -> int:
    strand, u = k
    v = ((u + (1 << 32)) << 1) | (strand - 1)
    assert 0 <= v < EMPTY
    return v


class Filter:
    """The duplicate filter of one accumulator: add() takes the batches in the order they are enqueued."""

    def __init__(self):
        self.rank = {}  # packed key -> the smallest rank so far
        self.seq = 0
        self.candidates = self.duplicates = 0

    def add(self, results, offsets, min_mapq: int = 0) -> np.ndarray:
        """The flags of one add: 1 for a duplicate, 0 for every other read."""
        off = np.asarray(offsets, dtype=np.int64)
        assert len(results) == len(off) - 1 and len(results) < 1 << 32
        seq, self.seq = self.seq, self.seq + 1
        mine = []
        for r, res in enumerate(results):
            k = key(res, int(off[r + 1] - off[r]), min_mapq)
            mine.append(None if k is None else (packed(k), (seq << 32) | r))
        for kr in mine:  # every candidate claims ...
            if kr is not None:
                self.rank[kr[0]] = min(self.rank.get(kr[0], EMPTY), kr[1])
        flags = np.zeros(len(results), dtype=np.uint8)
        for r, kr in enumerate(mine):  # ... then every candidate looks
            if kr is not None:
                self.candidates += 1
                if self.rank[kr[0]] != kr[1]:
                    flags[r] = 1
                    self.duplicates += 1
        return flags

    def reset(self) -> None:
        self.__init__()


def flags(adds, min_mapq: int = 0):
    """adds: an ordered list of (results, offsets).  The flags of each add, in that order."""
    f = Filter()
    return [f.add(res, off, min_mapq) for res, off in adds]


def keep(results, dup):
    """The batch as the pileup sees it: a read flagged 1 is unmapped, every other read as it was."""
    assert len(results) == len(dup)
    return [UNMAPPED if int(d) == 1 else res for res, d in zip(results, dup)]


def kept_per_key(results, offsets, dup, min_mapq: int = 0) -> dict:
    """packed key -> the indices of the candidates of that key that are not flagged 1."""
    off = np.asarray(offsets, dtype=np.int64)
    out = {}
    for r, res in enumerate(results):
        k = key(res, int(off[r + 1] - off[r]), min_mapq)
        if k is not None:
            out.setdefault(packed(k), [])
            if int(dup[r]) != 1:
                out[packed(k)].append(r)
    return out
