"""The eight primitives of slamem_amd/csrc/prims.h, restated in plain numpy -- TEST INFRASTRUCTURE ONLY.

Every definition works in np.uint64 or Python ints, so that nothing wraps unless the definition says so (the u32 sums are
modulo 2^32 because the kernel's type is).  The second half holds the case generators -- sizes and value patterns --
that tests/test_gpu_prims.py runs and whose coverage tests/test_prims_spec.py asserts without a GPU.
"""
from __future__ import annotations

import numpy as np

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1

# ---- definitions --------------------------------------------------------------------------------------------------


def _excl_cumsum_u64(a: np.ndarray) -> np.ndarray:
    """len(a) + 1 exclusive prefix sums of a (uint64 arithmetic; the callers keep the totals below 2^64)."""
    out = np.zeros(a.shape[0] + 1, dtype=np.uint64)
    np.cumsum(a.astype(np.uint64), out=out[1:])
    return out


def exclusive_scan_u32(a: np.ndarray) -> np.ndarray:
    """out[i] = sum(a[:i]) mod 2^32, len(a) outputs."""
    return (_excl_cumsum_u64(a)[:-1] & np.uint64(M32)).astype(np.uint32)


def scan_sum_exclusive_u32_u64(a: np.ndarray, n: int) -> np.ndarray:
    """out[i] = sum(a[:i]) for i in 0..n: n + 1 outputs, none of which depends on a[n:]."""
    return _excl_cumsum_u64(np.asarray(a[:n], dtype=np.uint32))


def scan_sum_exclusive_u64(a: np.ndarray, n: int) -> np.ndarray:
    """The same with u64 input: n + 1 outputs, out[n] the total."""
    return _excl_cumsum_u64(np.asarray(a[:n], dtype=np.uint64))


def scan_max_inclusive_u32(a: np.ndarray) -> np.ndarray:
    """out[i] = max(a[:i + 1])."""
    return np.maximum.accumulate(a.astype(np.uint32)) if a.shape[0] else a.astype(np.uint32)


def scan_sum_exclusive_uint4(a: np.ndarray) -> np.ndarray:
    """a: (n, 4) uint32; four independent exclusive sums, each modulo 2^32."""
    out = np.zeros((a.shape[0] + 1, 4), dtype=np.uint64)
    np.cumsum(a.astype(np.uint64), axis=0, out=out[1:])
    return (out[:-1] & np.uint64(M32)).astype(np.uint32)


def select_indices_u32(flags: np.ndarray) -> np.ndarray:
    """{ i : flags[i] != 0 }, ascending."""
    return np.nonzero(flags != 0)[0].astype(np.uint32)


def select_flagged_u32(a: np.ndarray, flags: np.ndarray) -> np.ndarray:
    """{ a[i] : flags[i] != 0 }, order preserved."""
    return a[flags != 0].astype(np.uint32)


def sort_passes(begin: int, end: int) -> int:
    """8-bit LSD passes over key bits [begin, end)."""
    return 0 if end <= begin else (end - begin + 7) // 8


def last_pass_width(begin: int, end: int) -> int:
    return 0 if end <= begin else ((end - begin - 1) % 8) + 1


def sort_spec(keys: np.ndarray, begin: int, end: int) -> np.ndarray:
    """The permutation of a STABLE sort of keys by their bits [begin, end): the definition.  end <= begin: the identity."""
    n = keys.shape[0]
    if end <= begin:
        return np.arange(n, dtype=np.int64)
    mask = np.uint64(((1 << (end - begin)) - 1) & M64)
    digit = (keys.astype(np.uint64) >> np.uint64(begin)) & mask
    return np.argsort(digit, kind="stable").astype(np.int64)


# ---- where the code changes shape ---------------------------------------------------------------------------------
SCAN_ITEMS = 8                      # consecutive elements per thread (scan.hip, k_scan_apply)
SCAN_WAVE = 64 * SCAN_ITEMS         # elements of one wave
SCAN_TILE = 2048                    # elements per workgroup
SCAN_LEVEL3 = SCAN_TILE * SCAN_TILE  # more elements than this: more than 2048 tiles, the totals are scanned in two levels
SORT_TILE = 4096                    # radix_sort.hip
SORT_TABLE_TILES = 8                # 256 bins x 8 tiles = one scan tile: from 9 tiles on the table's scan has two levels

SCAN_SIZES_SMALL = [0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 6149]
SCAN_SIZES_BIG = [SCAN_LEVEL3 - 1, SCAN_LEVEL3, SCAN_LEVEL3 + 1, 4_200_000]
SCAN_SIZES = SCAN_SIZES_SMALL + SCAN_SIZES_BIG
# a boundary B of the scans: B elements take the smaller shape, B + 1 the larger
SCAN_BOUNDARIES = [SCAN_ITEMS, 64, 256, SCAN_WAVE, SCAN_TILE, 2 * SCAN_TILE, SCAN_LEVEL3]


def scanned_length(n: int, plus_one: bool) -> int:
    """Elements the kernel sequence runs over: the two scans with n + 1 outputs scan n + 1 inputs."""
    return n + 1 if plus_one else n


def _rng(*key) -> np.random.Generator:
    return np.random.default_rng([0x5CA9] + [int(k) for k in key])


# ---- value patterns: each returns [(name, array), ...] -----------------------------------------------------------
SINGLE_ONE_AT = [0, 7, 8, 511, 512, 2047, 2048]  # and n - 1


def patterns_excl_u32(n: int):
    r = _rng(1, n)
    out = [("rand16", r.integers(0, 16, size=n, dtype=np.uint32)), ("ones", np.ones(n, dtype=np.uint32)),
           ("zeros", np.zeros(n, dtype=np.uint32))]
    for p in sorted(set(q for q in SINGLE_ONE_AT + [n - 1] if 0 <= q < n)):
        a = np.zeros(n, dtype=np.uint32)
        a[p] = 1
        out.append((f"one@{p}", a))
    return out


IN_N_POISON = 0xFFFFFFFF  # what in[n] holds in every u32 -> u64 case: out[0..n] must not depend on it


def patterns_u32_u64(n: int):
    """Arrays of n + 1 elements, the last one IN_N_POISON.  'ff' and 'full' are the patterns that cross 2^32."""
    r = _rng(2, n)
    out = []
    for name, body in (("ff", np.full(n, M32, dtype=np.uint32)), ("full", r.integers(0, 1 << 32, size=n, dtype=np.uint32)),
                       ("rand16", r.integers(0, 16, size=n, dtype=np.uint32))):
        out.append((name, np.concatenate([body, np.array([IN_N_POISON], dtype=np.uint32)])))
    return out


CROSSING_U32_U64 = ("ff", "full")


def patterns_u64(n: int):
    """Arrays of n + 1 elements, in[n] = 0 as prims.h demands.  'carry': k * 2^32 + 0xFFFFFFFF, every addition carries
    out of the low word."""
    r = _rng(3, n)
    lt40 = r.integers(0, 1 << 40, size=n, dtype=np.uint64)
    carry = (r.integers(0, 256, size=n, dtype=np.uint64) << np.uint64(32)) | np.uint64(M32)
    z = np.zeros(1, dtype=np.uint64)
    return [("lt40", np.concatenate([lt40, z])), ("carry", np.concatenate([carry, z]))]


CROSSING_U64 = ("lt40", "carry")


def max_spike_positions(n: int):
    """The last element of a tile and the first of the next: of tile 0, and of tile 2047 (where the third level starts)."""
    return [p for p in (SCAN_TILE - 1, SCAN_TILE, SCAN_LEVEL3 - 1, SCAN_LEVEL3) if p < n]


def patterns_max(n: int):
    r = _rng(4, n)
    out = [("rand", r.integers(0, 1 << 32, size=n, dtype=np.uint32)), ("zeros", np.zeros(n, dtype=np.uint32)),
           ("increasing", (np.arange(n, dtype=np.uint64) * np.uint64(1000) + np.uint64(5)).astype(np.uint32))]
    for p in max_spike_positions(n):
        a = r.integers(0, 1 << 31, size=n, dtype=np.uint32)
        a[p] = M32
        out.append((f"spike@{p}", a))
    return out


def patterns_uint4(n: int):
    """(n, 4) uint32.  No two lanes of a pattern can be mistaken for each other."""
    r = _rng(5, n)
    a = np.stack([r.integers(0, 16, size=n, dtype=np.uint32), r.integers(0, 256, size=n, dtype=np.uint32),
                  r.integers(0, 4, size=n, dtype=np.uint32), r.integers(0, 1024, size=n, dtype=np.uint32)], axis=1)
    b = np.stack([np.zeros(n, dtype=np.uint32), np.ones(n, dtype=np.uint32), r.integers(0, 16, size=n, dtype=np.uint32),
                  r.integers(0, 256, size=n, dtype=np.uint32)], axis=1)
    return [("ranges", np.ascontiguousarray(a)), ("zero+ones", np.ascontiguousarray(b))]


FLAG_BYTES = np.array([1, 2, 0x80, 0xFF], dtype=np.uint8)  # what a set flag holds; the contract is "non-zero"
DENSITIES = [("none", 0.0), ("1/1000", 0.001), ("half", 0.5), ("all", 1.0)]


def patterns_flags(n: int):
    """[(name, flags uint8 (n,), values uint32 (n,))]"""
    r = _rng(6, n)
    vals = r.integers(0, 1 << 32, size=n, dtype=np.uint32)
    out = []
    for name, d in DENSITIES:
        on = np.ones(n, dtype=bool) if d >= 1.0 else (r.random(n) < d)
        flags = np.where(on, FLAG_BYTES[r.integers(0, len(FLAG_BYTES), size=n)], 0).astype(np.uint8)
        out.append((name, flags, vals))
    return out


# ---- the sort's cases ------------------------------------------------------------------------------------------
SORT_SIZE_CLASSES = [[0, 1, 2], [63, 64, 65], [255, 256, 257], [1023, 1024, 1025], [4095, 4096, 4097], [8191, 8192, 8193],
                     [36_865], [1_000_003]]
SORT_SIZES = [n for c in SORT_SIZE_CLASSES for n in c]
# B elements take the smaller shape, B + 1 the larger: a wave's row, a workgroup's row, a wave's share of a tile, one tile,
# two tiles.  (The table's scan: one level at 8193 elements -- 3 tiles, 768 counters --, two at 36,865 -- 10 tiles, 2560.)
SORT_BOUNDARIES = [64, 256, 1024, SORT_TILE, 2 * SORT_TILE]
SORT_RANGES = [(0, 0), (0, 1), (0, 8), (0, 13), (0, 16), (0, 33), (0, 48), (0, 62), (0, 64), (8, 24), (3, 20)]
SORT_PATTERNS = ["uniform", "equal", "four", "ascending", "descending", "ff", "heavy"]
HEAVY_DIGIT = 0x5A


def sort_keys(pattern: str, n: int) -> np.ndarray:
    r = _rng(7, n, SORT_PATTERNS.index(pattern))
    if pattern == "uniform":
        return r.integers(0, 1 << 64, size=n, dtype=np.uint64)
    if pattern == "equal":
        return np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)
    if pattern == "four":
        four = np.array([0x0000000000000000, 0x00FF00FF00FF00FF, 0x8000000100000001, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
        return four[r.integers(0, 4, size=n)]
    if pattern == "ascending":
        return np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B1)
    if pattern == "descending":
        return (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B1))[::-1].copy()
    if pattern == "ff":
        return np.full(n, M64, dtype=np.uint64)  # every digit of every pass is the last bin
    if pattern == "heavy":
        # every byte of 4095 of a tile's 4096 keys is HEAVY_DIGIT; the one other key sits at a place that moves with the tile
        k = np.full(n, int.from_bytes(bytes([HEAVY_DIGIT]) * 8, "little"), dtype=np.uint64)
        tiles = (n + SORT_TILE - 1) // SORT_TILE
        at = np.arange(tiles, dtype=np.int64) * SORT_TILE + (np.arange(tiles, dtype=np.int64) * 37 + 1) % SORT_TILE
        at = at[at < n]
        k[at] = r.integers(0, 1 << 64, size=at.shape[0], dtype=np.uint64)
        return k
    raise ValueError(pattern)


def sort_cases():
    """[(n, begin, end, pattern)]: every size class meets every bit range and every key pattern, without the full product --
    the ranges go round the sizes of a class (shifted by one every third, so that every size meets odd and even pass counts),
    the patterns round the cases."""
    out = []
    k = 0
    for cls in SORT_SIZE_CLASSES:
        for j, (b, e) in enumerate(SORT_RANGES):
            out.append((cls[(j + j // 3) % len(cls)], b, e, SORT_PATTERNS[k % len(SORT_PATTERNS)]))
            k += 1
    return out
