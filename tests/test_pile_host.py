"""-pile on the CPU: the definition (tests/pile_spec.py) itself, without the engine -- hand-written segments
and CIGARs whose tables are written out by hand, the depth bound on the golden -mem files, and the -pile file of a reference of
two records."""
import numpy as np
import pytest

import map_spec
import pile_spec
from golden_cases import CASES, MANIFEST
from test_map_host import FakeRef

MEM_CASES = [c for c in CASES if "-mam" not in MANIFEST[c].get("tail", [])]

#        0123456789012345678901
TEXT = b"ACGTTGCAAGCTNACGGATCCA"
N = len(TEXT)
A, Cc, G, T, D, I = range(6)


def one(result, read, min_mapq=0):
    t = pile_spec.empty(N)
    pile_spec.add_read(t, result, read, min_mapq)
    return t


def rows(**at):
    """{position: (column, ...)} -> the table with +1 at each"""
    t = pile_spec.empty(N)
    for p, cols in at.items():
        for c in cols:
            t[int(p[1:]), c] += 1
    return t


def test_exact_read():
    # TEXT[2:8] = GTTGCA
    got = one((1, 60, 6, 0, [(2, 0, 6, 6, 0, [("=", 6)])]), b"GTTGCA")
    assert np.array_equal(got, rows(p2=(G,), p3=(T,), p4=(T,), p5=(G,), p6=(Cc,), p7=(A,)))
    assert list(pile_spec.depth(got)) == [0, 0, 1, 1, 1, 1, 1, 1] + [0] * (N - 8)


def test_substitution():
    # GTaGCA against GTTGCA: the read's letter counts, not the text's; lower case is upper-cased
    got = one((1, 60, 5, 0, [(2, 0, 6, 6, 1, [("=", 2), ("X", 1), ("=", 3)])]), b"GTaGCA")
    assert np.array_equal(got, rows(p2=(G,), p3=(T,), p4=(A,), p5=(G,), p6=(Cc,), p7=(A,)))


def test_deletion_of_three():
    # the read lacks TEXT[4:7] = TGC
    got = one((1, 60, 4, 0, [(2, 0, 7, 4, 3, [("=", 2), ("D", 3), ("=", 2)])]), b"GTAA")
    assert np.array_equal(got, rows(p2=(G,), p3=(T,), p4=(D,), p5=(D,), p6=(D,), p7=(A,), p8=(A,)))
    assert list(pile_spec.depth(got)[2:9]) == [1] * 7


def test_insertion_of_two_counts_once_in_front_of_p():
    got = one((1, 60, 4, 0, [(2, 0, 4, 6, 2, [("=", 2), ("I", 2), ("=", 2)])]), b"GTccTG")
    assert np.array_equal(got, rows(p2=(G,), p3=(T,), p4=(I, T), p5=(G,)))
    assert int(pile_spec.depth(got)[4]) == 1  # (I is not depth)


def test_insertion_at_the_text_end_is_dropped():
    got = one((1, 60, 3, 0, [(N - 3, 0, 3, 5, 2, [("=", 3), ("I", 2)])]), b"CCAgg")
    assert np.array_equal(got, rows(**{"p%d" % (N - 3): (Cc,), "p%d" % (N - 2): (Cc,), "p%d" % (N - 1): (A,)}))
    assert got[:, I].sum() == 0


def test_reverse_strand_counts_the_complement():
    # the read as given is the reverse complement of GTaGCA: TGCtAC; scanned strand Q = GTAGCA
    got = one((2, 60, 5, 0, [(2, 0, 6, 6, 1, [("=", 2), ("X", 1), ("=", 3)])]), b"TGCtAC")
    assert np.array_equal(got, rows(p2=(G,), p3=(T,), p4=(A,), p5=(G,), p6=(Cc,), p7=(A,)))


def test_n_under_equal_is_counted_nowhere():
    # TEXT[10:15] = CTNAC; an IUPAC letter likewise
    got = one((1, 60, 5, 0, [(10, 0, 5, 5, 0, [("=", 5)])]), b"CTNAC")
    assert np.array_equal(got, rows(p10=(Cc,), p11=(T,), p13=(A,), p14=(Cc,)))
    got = one((1, 60, 5, 0, [(10, 0, 5, 5, 0, [("=", 5)])]), b"CTRAC")
    assert int(got[12].sum()) == 0 and int(got.sum()) == 4


def test_threshold_and_unmapped_reads():
    seg = [(2, 0, 6, 6, 0, [("=", 6)])]
    assert one((1, 29, 6, 3, seg), b"GTTGCA", min_mapq=30).sum() == 0
    assert one((1, 30, 6, 3, seg), b"GTTGCA", min_mapq=30).sum() == 6
    assert one((1, 0, 6, 6, seg), b"GTTGCA", min_mapq=0).sum() == 6
    assert one((0, 0, 0, 0, []), b"GTTGCA").sum() == 0
    t = pile_spec.empty(N)
    assert not pile_spec.add_read(t, (0, 0, 0, 0, []), b"ACGT") and pile_spec.add_read(t, (1, 0, 6, 6, seg), b"GTTGCA")


def test_batches_add_up():
    reads = [b"GTTGCA", b"GTAA", b"TGCtAC"]
    res = [(1, 60, 6, 0, [(2, 0, 6, 6, 0, [("=", 6)])]), (1, 10, 4, 0, [(2, 0, 7, 4, 3, [("=", 2), ("D", 3), ("=", 2)])]),
           (2, 60, 5, 0, [(2, 0, 6, 6, 1, [("=", 2), ("X", 1), ("=", 3)])])]
    q = b"".join(reads)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    whole = pile_spec.pile(res, q, off, N)
    parts = pile_spec.pile(res[2:], q, off[2:], N, table=pile_spec.pile(res[:2], q, off[:3], N))
    assert np.array_equal(whole, parts) and pile_spec.contributing(res) == 3 and pile_spec.contributing(res, 11) == 2
    assert int(pile_spec.depth(whole).max()) == 3


@pytest.mark.parametrize("case", MEM_CASES)
def test_golden_cases_depth_is_bounded_by_the_contributing_reads(case):
    results, _, ref, qs, _ = map_spec.golden_map(case)
    n = len(ref.chars)
    for min_mapq in (0, 1):
        table = pile_spec.pile(results, qs.chars, qs.offsets, n, min_mapq)
        k = pile_spec.contributing(results, min_mapq)
        assert int(pile_spec.depth(table).max(initial=0)) <= k and table.min(initial=0) >= 0
        if min_mapq == 0 and k:
            assert table.sum() > 0


def test_pile_file_of_a_two_record_reference():
    recs = [b"ACGTTGCA", b"GGATCCAT"]
    ref = FakeRef(recs, [b"first one", b"second\tx"])
    n = len(ref.chars)  # 8 + 1 + 8: the separator sits at 8
    t = pile_spec.empty(n)
    t[0, A] = 2
    t[7, I] = 1
    t[8, D] = 5          # the separator: belongs to no record
    t[9, G], t[9, T] = 3, 1
    t[16, D] = 4
    want = (b"first\t1\tA\t2\t0\t0\t0\t0\t0\n" b"first\t8\tA\t0\t0\t0\t0\t0\t1\n"
            b"second\t1\tG\t0\t0\t3\t1\t0\t0\n" b"second\t8\tT\t0\t0\t0\t0\t4\t0\n")
    assert pile_spec.pile_file(t, ref) == want and b">" not in want
    assert pile_spec.pile_file(pile_spec.empty(n), ref) == b""
    lower = FakeRef([b"acgt"], [b"r"])
    t = pile_spec.empty(4)
    t[1, Cc] = 1
    assert pile_spec.pile_file(t, lower) == b"r\t2\tC\t0\t1\t0\t0\t0\t0\n"
