"""-dedup's definition (tests/dedup_spec.py) on mappings written out by hand: no GPU.  A result is a read_map
tuple (strand, mapq, s1, s2, segments), a segment (ref_pos, query_pos, ref_len, query_len, edits, operations)."""
import numpy as np

import dedup_spec as dd

N = 1000  # the text's length in these examples


def seg(p, q, rlen, qlen=None):
    qlen = rlen if qlen is None else qlen
    return (p, q, rlen, qlen, 0, [("=", min(rlen, qlen))])


def read(strand, segs, mapq=60):
    return (strand, mapq, 100, 0, list(segs))


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)


def test_forward_key_may_be_negative():
    # 8 letters clipped in front of a segment that starts at text position 0 and at 3: the 5' end lies in front of the text
    assert dd.unclipped(read(1, [seg(0, 8, 92)]), 100) == -8
    assert dd.unclipped(read(1, [seg(3, 8, 92)]), 100) == -5
    assert dd.unclipped(read(1, [seg(500, 0, 100)]), 100) == 500
    a, b = dd.key(read(1, [seg(0, 8, 92)]), 100), dd.key(read(1, [seg(3, 11, 60)]), 71)
    assert a == b == (1, -8) and dd.packed(a) == ((2 ** 32 - 8) << 1)
    res = [read(1, [seg(0, 8, 92)]), read(1, [seg(3, 11, 60)]), read(1, [seg(0, 7, 93)])]
    assert dd.flags([(res, offsets([100, 71, 100]))])[0].tolist() == [0, 1, 0]


def test_reverse_key_with_a_clip_beyond_the_text():
    # strand 2, scanned-strand coordinates: the segment ends at the text's end and 8 letters of the read lie behind it
    r = read(2, [seg(N - 92, 0, 92)])
    assert dd.unclipped(r, 100) == N + 8
    assert dd.key(r, 100) == (2, N + 8) and dd.packed((2, N + 8)) == (((1 << 32) + N + 8) << 1) | 1
    # the same 5' end from a shorter read with a longer clip, and from a read without a clip that ends 8 letters earlier
    assert dd.unclipped(read(2, [seg(N - 50, 0, 50)]), 58) == N + 8
    assert dd.unclipped(read(2, [seg(N - 108, 0, 100)]), 100) == N - 8
    res = [r, read(2, [seg(N - 50, 0, 50)]), read(2, [seg(N - 108, 0, 100)])]
    assert dd.flags([(res, offsets([100, 58, 100]))])[0].tolist() == [0, 1, 0]


def test_outermost_segments_are_found_wherever_they_are_stored():
    # three segments of one read, query starts 0, 40, 80, in every order of storage: the key never moves
    a, b, c = seg(200, 5, 30), seg(240, 40, 30), (285, 80, 15, 10, 5, [("=", 10), ("D", 5)])
    length = 100
    for order in ((a, b, c), (c, b, a), (b, a, c), (b, c, a), (c, a, b), (a, c, b)):
        assert dd.unclipped(read(1, order), length) == 200 - 5
        # strand 2: R is c (it ends at query 90): 285 + 15 + (100 - 80 - 10)
        assert dd.unclipped(read(2, order), length) == 310
    # the middle one first and last would both be wrong
    assert dd.unclipped(read(1, [b]), length) == 200 and dd.unclipped(read(2, [b]), length) == 240 + 30 + 30


def test_the_same_position_on_both_strands_is_two_keys():
    f, r = read(1, [seg(300, 0, 100)]), read(2, [seg(200, 0, 100)])
    assert dd.unclipped(f, 100) == dd.unclipped(r, 100) == 300
    assert dd.key(f, 100) != dd.key(r, 100) and dd.packed(dd.key(f, 100)) ^ dd.packed(dd.key(r, 100)) == 1
    res = [f, r, f, r]
    assert dd.flags([(res, offsets([100] * 4))])[0].tolist() == [0, 0, 1, 1]


def test_a_read_below_the_quality_does_not_shadow_a_good_one():
    low, good = read(1, [seg(300, 0, 100)], mapq=0), read(1, [seg(300, 0, 150)], mapq=30)
    res, off = [low, good, good], offsets([100, 150, 150])
    assert dd.key(low, 100, 20) is None and dd.key(low, 100, 0) == dd.key(good, 150, 20)
    assert dd.flags([(res, off)], 20)[0].tolist() == [0, 0, 1]  # the first good read is kept
    assert dd.flags([(res, off)], 0)[0].tolist() == [0, 1, 1]   # at quality 0 the first read of all is
    f = dd.Filter()
    f.add(res, off, 20)
    assert (f.candidates, f.duplicates) == (2, 1)
    # an unmapped read and one without a segment are no candidates at any quality
    assert dd.key(dd.UNMAPPED, 100) is None and dd.key((1, 60, 10, 0, []), 100) is None


def test_across_two_adds_the_first_wins():
    x, y = read(1, [seg(300, 0, 100)]), read(2, [seg(500, 0, 100)])
    a, b = ([x, y], offsets([100, 100])), ([y, x, x], offsets([100] * 3))
    assert [f.tolist() for f in dd.flags([a, b])] == [[0, 0], [1, 1, 1]]
    assert [f.tolist() for f in dd.flags([b, a])] == [[0, 0, 1], [1, 1]]
    # the rank is the add's number, then the index: a later add never takes a key from an earlier one, whatever the indices
    assert [f.tolist() for f in dd.flags([([x], offsets([100])), ([y, y, x], offsets([100] * 3))])] == [[0], [0, 1, 1]]
    # one read per key whatever the order, and keep() hands the others on as unmapped
    for adds in ([a, b], [b, a]):
        fl = dd.flags(adds)
        kept = [r for (res, _), f in zip(adds, fl) for r in dd.keep(res, f) if r is not dd.UNMAPPED]
        assert sorted(dd.key(r, 100) for r in kept) == [(1, 300), (2, 600)]
    per = dd.kept_per_key(b[0], b[1], dd.flags([b])[0])
    assert sorted(per.values()) == [[0], [1]]
