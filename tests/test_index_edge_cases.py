"""The designed texts of tests/index_edge_cases.py, looked at by the oracle alone (no GPU): each must really have the
property that tests/test_gpu_index_edges.py builds it for.  These are conditions on the inputs, not on the engine."""
import numpy as np
import pytest

import index_edge_cases as ec


@pytest.mark.parametrize("name", list(ec.DESIGNED))
def test_designed_text_has_its_long_repeats(name):
    from oracle import pyoracle as po
    text = ec.designed_text(name)
    n = len(text)
    lcp = po.OracleIndex(text).lcp[1:n + 1]
    mx = int(lcp.max())
    above = [int((lcp > k).sum()) for k in (256, 4096, 36_864)]
    print(name, "n", n, "max LCP", mx, "rows with LCP > 256 / 4096 / 36864", above)
    assert mx == ec.DESIGNED[name][1]
    assert mx >= ec.MIN_MAX_LCP            # outlasts one coarse-2 stride plus one 4096-letter step
    assert above[2] >= ec.MIN_ROWS_ABOVE_COARSE2
    assert above[1] >= ec.MIN_ROWS_ABOVE_4096
    assert above[0] > above[1] > above[2]  # rows for the 256-letter hand-over and the 4096-letter steps alone
    assert ec.min_sort_rounds(mx) == (12 if name == "tail" else 13)


def test_tail_repeat_ends_at_the_text_end():
    t = ec.designed_text("tail")
    assert t[-45_000:] == t[20_000:65_000] and t[-45_001] != t[19_999]


def test_sizes_cross_what_they_are_there_for():
    n_big = len(ec.designed_text("big"))
    assert n_big + 1 > 2048 * 2048 + 2048          # more than 2048 scan tiles with a tile to spare: the third level
    assert ec.min_levels(n_big + 1) == 5 and ec.min_levels(100_001) == 4
    rows = [n + 1 for n in ec.RANDOM_SIZES]
    assert {2047, 2048, 2049}.issubset(rows) and 4097 in rows and 8192 in rows   # R on both sides of a scan tile; radix tiles
    assert {65_535, 65_536, 65_537}.issubset(ec.RANDOM_SIZES)                    # the n < 2^16 switch, the second coarse-2 sample
    assert ec.min_levels(1_100_001) == 5 and ec.min_levels(1_048_576) == 4
    assert ec.min_sort_rounds(70_000) == 13 and ec.min_sort_rounds(45_000) == 12 and ec.min_sort_rounds(15) == 0


def test_random_text_is_reproducible_and_has_its_repeats():
    a, b = ec.random_text(8191), ec.random_text(8191)
    assert a == b and len(a) == 8191 and set(a) <= set(b"ACGT")
