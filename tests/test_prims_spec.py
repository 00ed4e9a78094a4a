"""tests/prims_spec.py without a GPU: each definition on answers written by hand, and the coverage that the generated cases
of tests/test_gpu_prims.py claim -- a size on each side of every boundary, sums that really cross 2^32 where the kernels
could drop a carry, totals that stay inside their type, and a sort case list that reaches every pass shape in every size
class.  These asserts are what keeps the GPU file from testing less than it says."""
import numpy as np
import pytest

import prims_spec as ps

U32, U64 = np.uint32, np.uint64


# ---- the definitions -----------------------------------------------------------------------------------------------
def test_exclusive_scan_u32_by_hand():
    assert ps.exclusive_scan_u32(np.array([], dtype=U32)).tolist() == []
    assert ps.exclusive_scan_u32(np.array([3, 0, 5, 1], dtype=U32)).tolist() == [0, 3, 3, 8]
    # modulo 2^32, as the kernel's type dictates
    assert ps.exclusive_scan_u32(np.array([0xFFFFFFFF, 2, 7], dtype=U32)).tolist() == [0, 0xFFFFFFFF, 1]
    assert ps.exclusive_scan_u32(np.array([1], dtype=U32)).dtype == U32


def test_wide_sums_by_hand():
    a = np.array([0xFFFFFFFF, 0xFFFFFFFF, 1, 0xFFFFFFFF], dtype=U32)
    assert ps.scan_sum_exclusive_u32_u64(a, 3).tolist() == [0, 0xFFFFFFFF, 0x1FFFFFFFE, 0x1FFFFFFFF]  # a[3] is not summed
    assert ps.scan_sum_exclusive_u32_u64(a, 0).tolist() == [0]
    assert ps.scan_sum_exclusive_u32_u64(a, 3).dtype == U64
    b = np.array([(1 << 40) - 1, 1, (5 << 32) | 0xFFFFFFFF, 0], dtype=U64)
    assert ps.scan_sum_exclusive_u64(b, 3).tolist() == [0, (1 << 40) - 1, 1 << 40, (1 << 40) + (5 << 32) + 0xFFFFFFFF]
    # no wrap below 2^64
    c = np.array([1 << 63, (1 << 63) - 1, 0], dtype=U64)
    assert ps.scan_sum_exclusive_u64(c, 2).tolist() == [0, 1 << 63, (1 << 64) - 1]


def test_running_max_by_hand():
    assert ps.scan_max_inclusive_u32(np.array([], dtype=U32)).tolist() == []
    assert ps.scan_max_inclusive_u32(np.array([2, 1, 0xFFFFFFFF, 3, 0], dtype=U32)).tolist() == [2, 2, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]
    assert ps.scan_max_inclusive_u32(np.array([0, 0, 4, 4, 9], dtype=U32)).tolist() == [0, 0, 4, 4, 9]


def test_uint4_sums_by_hand():
    a = np.array([[1, 10, 0, 0xFFFFFFFF], [2, 20, 0, 3], [3, 30, 0, 0]], dtype=U32)
    assert ps.scan_sum_exclusive_uint4(a).tolist() == [[0, 0, 0, 0], [1, 10, 0, 0xFFFFFFFF], [3, 30, 0, 2]]
    assert ps.scan_sum_exclusive_uint4(np.zeros((0, 4), dtype=U32)).shape == (0, 4)


def test_selects_by_hand():
    f = np.array([0, 1, 0, 0x80, 0xFF, 0, 2], dtype=np.uint8)
    v = np.array([10, 11, 12, 13, 14, 15, 16], dtype=U32)
    assert ps.select_indices_u32(f).tolist() == [1, 3, 4, 6]
    assert ps.select_flagged_u32(v, f).tolist() == [11, 13, 14, 16]
    assert ps.select_indices_u32(np.zeros(0, dtype=np.uint8)).tolist() == []
    assert ps.select_indices_u32(np.zeros(5, dtype=np.uint8)).tolist() == []


def test_sort_spec_by_hand():
    k = np.array([0x302, 0x101, 0x202, 0x001, 0x102], dtype=U64)
    assert ps.sort_spec(k, 0, 8).tolist() == [1, 3, 0, 2, 4]     # by the low byte; equal bytes keep their order
    assert ps.sort_spec(k, 8, 16).tolist() == [3, 1, 4, 2, 0]    # by the second byte
    assert ps.sort_spec(k, 0, 64).tolist() == [3, 1, 4, 2, 0]
    assert ps.sort_spec(k, 0, 1).tolist() == [0, 2, 4, 1, 3]
    assert ps.sort_spec(k, 0, 0).tolist() == [0, 1, 2, 3, 4]     # end <= begin: the identity
    assert ps.sort_spec(k, 9, 3).tolist() == [0, 1, 2, 3, 4]
    top = np.array([1 << 63, 0, (1 << 63) | 1, 1], dtype=U64)
    assert ps.sort_spec(top, 0, 64).tolist() == [1, 3, 0, 2]     # all 64 bits, unsigned
    assert ps.sort_spec(top, 63, 64).tolist() == [1, 3, 0, 2]
    assert [ps.sort_passes(b, e) for b, e in ps.SORT_RANGES] == [0, 1, 1, 2, 2, 5, 6, 8, 8, 2, 3]
    assert [ps.last_pass_width(b, e) for b, e in ps.SORT_RANGES] == [0, 1, 8, 5, 8, 1, 8, 6, 8, 8, 1]


# ---- the coverage of the generated cases -----------------------------------------------------------------------------
def test_the_size_lists_are_the_ones_asked_for():
    assert ps.SCAN_SIZES == [0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 6149,
                             4_194_303, 4_194_304, 4_194_305, 4_200_000]
    assert ps.SORT_SIZES == [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 36_865,
                             1_000_003]
    assert ps.SORT_RANGES == [(0, 0), (0, 1), (0, 8), (0, 13), (0, 16), (0, 33), (0, 48), (0, 62), (0, 64), (8, 24), (3, 20)]


@pytest.mark.parametrize("plus_one", [False, True], ids=["n", "n+1"])
def test_every_scan_boundary_has_a_size_on_each_side(plus_one):
    lengths = {ps.scanned_length(n, plus_one) for n in ps.SCAN_SIZES}
    for b in ps.SCAN_BOUNDARIES:
        assert b in lengths, f"no scanned length of exactly {b}"
        assert b + 1 in lengths, f"no scanned length of {b} + 1"
    # the third level: more than 2048 tiles
    tiles = lambda m: (m + ps.SCAN_TILE - 1) // ps.SCAN_TILE
    assert max(tiles(m) for m in lengths if m <= ps.SCAN_LEVEL3) == ps.SCAN_TILE
    assert sum(1 for m in lengths if tiles(m) > ps.SCAN_TILE) >= (3 if plus_one else 2)
    assert 0 in {n for n in ps.SCAN_SIZES} and 1 in lengths


def test_every_sort_boundary_has_a_size_on_each_side():
    for b in ps.SORT_BOUNDARIES:
        assert b in ps.SORT_SIZES and b + 1 in ps.SORT_SIZES and b - 1 in ps.SORT_SIZES, b
    tiles = lambda n: (n + ps.SORT_TILE - 1) // ps.SORT_TILE
    # the sort's own table of 256 x tiles counters: one scan tile up to 8 tiles, two levels from 9 on
    assert any(256 * tiles(n) > ps.SCAN_TILE for n in ps.SORT_SIZES) and tiles(36_865) == 10
    assert any(1 < tiles(n) <= ps.SORT_TABLE_TILES for n in ps.SORT_SIZES)
    assert any(n % ps.SORT_TILE not in (0, 1, ps.SORT_TILE - 1) for n in ps.SORT_SIZES if n > 2 * ps.SORT_TILE)


def _crossings(prefix: np.ndarray) -> np.ndarray:
    """Indices i with floor(prefix[i + 1] / 2^32) > floor(prefix[i] / 2^32): element i carries the sum over a multiple of 2^32."""
    hi = prefix >> np.uint64(32)
    return np.nonzero(hi[1:] > hi[:-1])[0]


@pytest.mark.parametrize("which", ["u32_u64", "u64"])
def test_the_crossing_patterns_cross_inside_a_wave_and_across_a_tile(which):
    """A carry into bit 32 that happens (a) between two elements of one wave's 512 and (b) in the prefix a tile hands to the
    next is what a scan that kept 32 bits somewhere -- the shuffles, the LDS words, the tile totals -- would lose."""
    gen, spec, names = ((ps.patterns_u32_u64, ps.scan_sum_exclusive_u32_u64, ps.CROSSING_U32_U64) if which == "u32_u64"
                        else (ps.patterns_u64, ps.scan_sum_exclusive_u64, ps.CROSSING_U64))
    for n in ps.SCAN_SIZES:
        if n < 64:
            continue
        pats = dict(gen(n))
        for name in names:
            pre = spec(pats[name], n)
            # (a) the sum of the first wave's own elements alone crosses 2^32, and so does that of the last full wave
            spans = [0] + ([(n // ps.SCAN_WAVE - 1) * ps.SCAN_WAVE] if n >= 2 * ps.SCAN_WAVE else [])
            for s in spans:
                e = min(n, s + ps.SCAN_WAVE)
                assert int(pre[e]) - int(pre[s]) >= 1 << 32, (which, name, n, s)
                assert len(_crossings(pre[s:e + 1])) >= 1
            # (b) every tile's prefix -- what the levels above hand down -- is beyond 32 bits, and it moved past a multiple of
            #     2^32 inside the tile before
            if n > ps.SCAN_TILE:
                bounds = np.arange(ps.SCAN_TILE, n + 1, ps.SCAN_TILE)
                assert int(pre[bounds].min()) >= 1 << 32, (which, name, n)
                assert np.all((pre[bounds] >> np.uint64(32)) > (pre[bounds - ps.SCAN_TILE] >> np.uint64(32)))


def test_totals_stay_inside_their_type():
    for n in ps.SCAN_SIZES:
        for name, a in ps.patterns_excl_u32(n):
            assert int(a.astype(np.uint64).sum()) < 1 << 32, (name, n)
        for name, a in ps.patterns_u32_u64(n):
            assert a.shape[0] == n + 1 and int(a[n]) == ps.IN_N_POISON
            assert n * 0xFFFFFFFF < 1 << 64  # a bound that cannot itself wrap
        for name, a in ps.patterns_u64(n):
            assert a.shape[0] == n + 1 and int(a[n]) == 0
            assert int(a.max()) < 1 << 41 and n * (1 << 41) < 1 << 64, (name, n)  # a bound that cannot itself wrap
        for name, a in ps.patterns_uint4(n):
            assert a.shape == (n, 4) and a.dtype == U32
            assert all(int(a[:, c].astype(np.uint64).sum()) < 1 << 32 for c in range(4)), (name, n)


def test_the_u32_patterns_are_the_ones_asked_for():
    n = 6149
    names = [p[0] for p in ps.patterns_excl_u32(n)]
    assert names == ["rand16", "ones", "zeros"] + [f"one@{p}" for p in (0, 7, 8, 511, 512, 2047, 2048, n - 1)]
    for name, a in ps.patterns_excl_u32(n)[3:]:
        assert int(a.sum()) == 1 and int(a[int(name[4:])]) == 1
    assert [p[0] for p in ps.patterns_excl_u32(8)] == ["rand16", "ones", "zeros", "one@0", "one@7"]
    assert int(ps.patterns_excl_u32(n)[0][1].max()) == 15


def test_the_max_patterns_put_the_spike_on_both_sides_of_a_tile():
    for n in (2049, 6149, 4_200_000):
        pats = dict(ps.patterns_max(n))
        want = [p for p in (2047, 2048, 2048 * 2048 - 1, 2048 * 2048) if p < n]
        for p in want:
            a = pats[f"spike@{p}"]
            assert int(a[p]) == 0xFFFFFFFF and int(np.delete(a, p).max()) < 1 << 31
        assert len(want) == (4 if n > 2048 * 2048 else 2)
        inc = pats["increasing"].astype(np.int64)
        assert np.all(np.diff(inc) > 0)
        assert not pats["zeros"].any()
    assert [p[0] for p in ps.patterns_max(2048)] == ["rand", "zeros", "increasing", "spike@2047"]


def test_the_uint4_lanes_cannot_be_mistaken_for_each_other():
    for n in (513, 6149):
        pats = dict(ps.patterns_uint4(n))
        a, b = pats["ranges"], pats["zero+ones"]
        tot = [int(a[:, c].astype(np.uint64).sum()) for c in range(4)]
        assert len(set(tot)) == 4
        assert not b[:, 0].any() and np.all(b[:, 1] == 1)
        sa, sb = ps.scan_sum_exclusive_uint4(a), ps.scan_sum_exclusive_uint4(b)
        for s in (sa, sb):
            for c in range(4):
                for d in range(c + 1, 4):
                    assert not np.array_equal(s[:, c], s[:, d])


def test_the_flag_patterns():
    for n in (0, 1, 513, 6149, 4_200_000):
        pats = ps.patterns_flags(n)
        assert [p[0] for p in pats] == ["none", "1/1000", "half", "all"]
        by = {p[0]: p[1] for p in pats}
        assert not by["none"].any() and np.all(by["all"] != 0)
        if n >= 6149:
            d = np.count_nonzero(by["1/1000"]) / n
            assert 0 < d < 0.004, d
            assert 0.45 < np.count_nonzero(by["half"]) / n < 0.55
            for f in (by["half"], by["all"]):
                assert set(np.unique(f).tolist()) - {0} == {1, 2, 0x80, 0xFF}
        assert all(p[2].shape == (n,) and p[2].dtype == U32 for p in pats)


def test_sort_cases_reach_every_pass_shape_in_every_size_class():
    cases = ps.sort_cases()
    assert len(cases) == len(ps.SORT_SIZE_CLASSES) * len(ps.SORT_RANGES)
    assert {c[0] for c in cases} == set(ps.SORT_SIZES)
    for cls in ps.SORT_SIZE_CLASSES:
        mine = [c for c in cases if c[0] in cls]
        ranges = {(b, e) for _, b, e, _ in mine}
        assert ranges == set(ps.SORT_RANGES), cls
        passes = [ps.sort_passes(b, e) for b, e in ranges]
        assert any(p % 2 == 1 for p in passes) and any(p % 2 == 0 and p > 0 for p in passes) and 0 in passes
        assert any(0 < ps.last_pass_width(b, e) < 8 for b, e in ranges)
        assert any(b > 0 for b, e in ranges)
        assert {p for *_, p in mine} == set(ps.SORT_PATTERNS), cls
        # every size of the class itself meets an odd and an even pass count
        for n in cls:
            pn = [ps.sort_passes(b, e) for m, b, e, _ in mine if m == n]
            assert any(p % 2 == 1 for p in pn) and any(p % 2 == 0 for p in pn), n


def test_sort_key_patterns():
    n = 3 * ps.SORT_TILE + 77
    for p in ps.SORT_PATTERNS:
        k = ps.sort_keys(p, n)
        assert k.shape == (n,) and k.dtype == U64
        assert np.array_equal(k, ps.sort_keys(p, n))  # the same keys for the test that runs them
    assert len(np.unique(ps.sort_keys("equal", n))) == 1
    assert len(np.unique(ps.sort_keys("four", n))) == 4
    assert len(np.unique(ps.sort_keys("uniform", n))) == n
    assert np.all(np.diff(ps.sort_keys("ascending", n).astype(object)) > 0)
    assert np.all(np.diff(ps.sort_keys("descending", n).astype(object)) < 0)
    assert np.all(ps.sort_keys("ff", n) == np.uint64(0xFFFFFFFFFFFFFFFF))
    h = ps.sort_keys("heavy", n)
    for shift in range(0, 64, 8):
        d = (h[:ps.SORT_TILE] >> np.uint64(shift)) & np.uint64(0xFF)
        assert np.count_nonzero(d == ps.HEAVY_DIGIT) >= ps.SORT_TILE - 1
    full = int.from_bytes(bytes([ps.HEAVY_DIGIT]) * 8, "little")
    for t in range(3):
        assert np.count_nonzero(h[t * ps.SORT_TILE:(t + 1) * ps.SORT_TILE] == np.uint64(full)) == ps.SORT_TILE - 1
    assert ps.sort_keys("uniform", 0).shape == (0,)
