"""Texts designed to take the index build through the paths that short repeats never reach -- TEST INFRASTRUCTURE ONLY.

Shared by tests/test_index_edge_cases.py (the oracle alone, without a GPU: does each text have the property it is there
for?) and tests/test_gpu_index_edges.py (the built index against the oracle).

The designed texts all hold a repeat far longer than kLcpCoarse2 = 32768 + 4096 letters, so that
  * k_lcp_kasai hands over after 256 letters, wave_extend_lcp takes 4096-letter steps, and the kLcpCoarse1 = 1024 and
    kLcpCoarse2 = 32768 sampled passes have thousands of rows to answer without reading the text,
  * prefix doubling needs ceil(log2((max LCP + 1) / 16)) >= 12 rounds, the late ones over a few thousand survivors,
  * `tail` ends its repeat at the end of the text, so that the comparison runs into '$' and the zero words behind it,
  * `big` has more than 2048 x 2048 rows: the scans of the real build run their third level, the min hierarchy has 5 levels.
The plain random texts put R = n + 1 on both sides of the scan and radix tiles, of the n < 2^16 switch of the filter build,
of the second kLcpCoarse2 sample and of the fifth min level (above 32^4 = 1,048,576 rows).
"""
from __future__ import annotations

import math

import numpy as np

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _letters(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).choice(_ACGT, size=n)


def _dup70k():
    t = _letters(300_000, 2)
    t[150_000:220_000] = t[10_000:80_000]
    return t


def _runs():
    t = _letters(200_000, 3)
    t[50_000:116_000] = ord("A")
    t[130_000:170_000] = ord("N")
    return t


def _tandem():
    t = _letters(200_000, 4)
    t[60_000:60_000 + 400 * 171] = np.tile(t[5000:5171], 400)
    return t


def _tail():
    t = _letters(120_000, 5)
    t[-45_000:] = t[20_000:65_000]
    return t


def _all_a():
    return np.full(70_000, ord("A"), dtype=np.uint8)


def _big():
    t = _letters(4_300_000, 1)
    t[2_000_000:2_070_000] = t[100_000:170_000]
    return t


# name -> (builder, the max LCP its construction gives)
DESIGNED = {"dup70k": (_dup70k, 70_000), "runs": (_runs, 65_999), "tandem": (_tandem, 68_229), "tail": (_tail, 45_000),
            "allA": (_all_a, 69_999), "big": (_big, 70_000)}
NO_COMPACT = ("big",)  # built in the full layout only

# conditions on the designed texts (the oracle alone meets them)
MIN_MAX_LCP = 36_865           # one coarse-2 stride plus one 4096-letter step
MIN_ROWS_ABOVE_COARSE2 = 8_000  # rows with LCP > 36,864
MIN_ROWS_ABOVE_4096 = 40_000

RANDOM_SIZES = [2046, 2047, 2048, 4096, 8191, 65_535, 65_536, 65_537, 1_100_000]


def designed_text(name: str) -> bytes:
    return DESIGNED[name][0]().tobytes()


def random_text(n: int, repeats: int = 4, max_rep: int = 300) -> bytes:
    """Random ACGT with `repeats` planted copies of at most max_rep letters (as rand_text of test_gpu_parity.py)."""
    rng = np.random.default_rng(n * 7 + repeats)
    t = rng.choice(_ACGT, size=n)
    for _ in range(repeats):
        L = int(rng.integers(10, max_rep))
        a, b = int(rng.integers(0, n - L)), int(rng.integers(0, n - L))
        t[b:b + L] = t[a:a + L].copy()
    return t.tobytes()


def min_sort_rounds(max_lcp: int) -> int:
    """After r doubling rounds the suffixes are told apart by their first 16 * 2^r letters: two suffixes that share max_lcp
    letters need 16 * 2^r >= max_lcp + 1."""
    return max(0, math.ceil(math.log2((max_lcp + 1) / 16)))


def min_levels(rows: int) -> int:
    """Levels of the 32-ary min hierarchy over `rows` rows."""
    lv = 0
    while rows > 1:
        rows = (rows + 31) // 32
        lv += 1
    return lv
