"""The scan, compaction and radix-sort primitives of slamem_amd/csrc/prims.h, one by one, against tests/prims_spec.py.

What runs is the product's libslamem_hip.so behind tests/prims/libprims_shim.so (tests/prims.py).  The sizes and value
patterns come from prims_spec.py, whose coverage tests/test_prims_spec.py asserts: both sides of every tile / wave /
level boundary, the third level of the scans (more than 2048 tiles), sums that cross 2^32 inside a wave and across tiles,
and for the sort odd and even pass counts, narrow last passes and a non-zero begin_bit in every size class.

Every device buffer is guarded (prims.Guarded: 256 bytes of 0xA5 on both sides, the payload pre-filled with 0xA5), tmp is
exactly the queried size, and after every call the guards of every buffer, the output beyond its defined length and the
return code are checked.  The undersized-tmp cases are the only check of the tmp size arithmetic there is.
"""
import numpy as np
import pytest

import prims as pr
import prims_spec as ps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (there is no CPU path)")
    return pr.lib()


def first_diff(got: np.ndarray, want: np.ndarray, what: str) -> None:
    """Equal, or fail with the first differing element and its neighbours (never the arrays)."""
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if np.array_equal(got, want):
        return
    ne = got != want
    if ne.ndim > 1:
        ne = ne.any(axis=tuple(range(1, ne.ndim)))
    i = int(np.argmax(ne))
    a, b = max(0, i - 2), i + 3
    pytest.fail(f"{what}: {int(ne.sum())} of {got.shape[0]} differ, first at {i}: got[{a}:{b}] = {got[a:b].tolist()}, "
                f"want[{a}:{b}] = {want[a:b].tolist()}")


def intact(*bufs) -> None:
    for k, b in enumerate(bufs):
        assert b.guards_intact(), f"guard bytes of buffer {k} were overwritten"


# ---- exclusive_scan_u32 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ps.SCAN_SIZES)
def test_exclusive_scan_u32(L, n):
    """Out of place and in place (the radix sort and the stream's offsets scan in place), every pattern."""
    words = int(L.prims_scan_u32_tmp_words(n))
    assert words >= 1
    for name, a in ps.patterns_excl_u32(n):
        want = ps.exclusive_scan_u32(a)
        for in_place in (False, True):
            src = pr.Guarded.of(a)
            dst = src if in_place else pr.Guarded(4 * n + 64)   # 16 more words than defined
            tmp = pr.Guarded(4 * words)
            rc = L.prims_exclusive_scan_u32(src.ptr, dst.ptr, n, tmp.ptr)
            what = f"exclusive_scan_u32 n={n} {name} {'in place' if in_place else 'out of place'}"
            assert rc == pr.HIP_SUCCESS, f"{what}: hipError {rc}"
            intact(src, dst, tmp)
            out = dst.payload(np.uint32)
            first_diff(out[:n], want, what)
            if not in_place:
                assert np.array_equal(out[n:], pr.filled(np.uint32, 16)), f"{what}: wrote past out[n]"
                first_diff(src.payload(np.uint32), a, what + " (input)")


# ---- the scans of the two-call convention ----------------------------------------------------------------------------
def run_scan(fn, a_in: np.ndarray, n: int, out_dtype, out_count: int, what: str) -> np.ndarray:
    """Size query, exact tmp, the call, the guards; returns the defined outputs.  16 more elements of out are allocated than
    defined and must keep their fill."""
    item = np.dtype(out_dtype).itemsize
    src = pr.Guarded.of(a_in)
    dst = pr.Guarded(item * (out_count + 16))
    need = pr.tmp_query(fn, src.ptr, dst.ptr, n)
    assert need > 0
    tmp = pr.Guarded(need)
    rc = pr.call(fn, tmp, need, src.ptr, dst.ptr, n)
    assert rc == pr.HIP_SUCCESS, f"{what}: hipError {rc}"
    intact(src, dst, tmp)
    out = dst.payload(out_dtype)
    assert np.array_equal(out[out_count:], pr.filled(out_dtype, 16)), f"{what}: wrote past the defined outputs"
    assert np.array_equal(src.payload(a_in.dtype), a_in.reshape(-1)), f"{what}: the input was modified"
    return out[:out_count]


@pytest.mark.parametrize("n", ps.SCAN_SIZES)
def test_scan_sum_exclusive_u32_u64(L, n):
    """n + 1 inputs are scanned: in[n] is read (here 0xFFFFFFFF) and no output may depend on it."""
    for name, a in ps.patterns_u32_u64(n):
        what = f"scan_sum_exclusive_u32_u64 n={n} {name}"
        got = run_scan(L.prims_scan_sum_exclusive_u32_u64, a, n, np.uint64, n + 1, what)
        first_diff(got, ps.scan_sum_exclusive_u32_u64(a, n), what)


@pytest.mark.parametrize("n", ps.SCAN_SIZES)
def test_scan_sum_exclusive_u64(L, n):
    for name, a in ps.patterns_u64(n):
        what = f"scan_sum_exclusive_u64 n={n} {name}"
        got = run_scan(L.prims_scan_sum_exclusive_u64, a, n, np.uint64, n + 1, what)
        first_diff(got, ps.scan_sum_exclusive_u64(a, n), what)


@pytest.mark.parametrize("n", ps.SCAN_SIZES)
def test_scan_max_inclusive_u32(L, n):
    for name, a in ps.patterns_max(n):
        what = f"scan_max_inclusive_u32 n={n} {name}"
        got = run_scan(L.prims_scan_max_inclusive_u32, a, n, np.uint32, n, what)
        first_diff(got, ps.scan_max_inclusive_u32(a), what)


@pytest.mark.parametrize("n", ps.SCAN_SIZES)
def test_scan_sum_exclusive_uint4(L, n):
    for name, a in ps.patterns_uint4(n):
        what = f"scan_sum_exclusive_uint4 n={n} {name}"
        got = run_scan(L.prims_scan_sum_exclusive_uint4, a, n, np.uint32, 4 * n, what)
        first_diff(got.reshape(n, 4), ps.scan_sum_exclusive_uint4(a), what)


# ---- the selects -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ps.SCAN_SIZES)
@pytest.mark.parametrize("which", ["indices", "flagged"])
def test_selects(L, which, n):
    """Flags are 'non-zero' (1, 2, 0x80, 0xFF); count_out is poisoned before the call; out[count:] keeps its fill; n = 0
    gives count 0."""
    for name, flags, vals in ps.patterns_flags(n):
        what = f"select_{which}_u32 n={n} density {name}"
        f = pr.Guarded.of(flags)
        v = pr.Guarded.of(vals)
        out = pr.Guarded(4 * n)
        cnt = pr.Guarded(4)   # the fill is the poison
        if which == "indices":
            fn, args = L.prims_select_indices_u32, (f.ptr, out.ptr, cnt.ptr, n)
            want = ps.select_indices_u32(flags)
        else:
            fn, args = L.prims_select_flagged_u32, (v.ptr, f.ptr, out.ptr, cnt.ptr, n)
            want = ps.select_flagged_u32(vals, flags)
        need = pr.tmp_query(fn, *args)
        tmp = pr.Guarded(need)
        rc = pr.call(fn, tmp, need, *args)
        assert rc == pr.HIP_SUCCESS, f"{what}: hipError {rc}"
        intact(f, v, out, cnt, tmp)
        count = int(cnt.payload(np.uint32)[0])
        assert count == want.shape[0], f"{what}: count {count}, want {want.shape[0]}"
        got = out.payload(np.uint32)
        first_diff(got[:count], want, what)
        assert np.array_equal(got[count:], pr.filled(np.uint32, n - count)), f"{what}: out[count:] was written"
        assert np.array_equal(f.payload(np.uint8), flags) and np.array_equal(v.payload(np.uint32), vals)


# ---- undersized tmp: refused before anything is written --------------------------------------------------------------
def _undersized(L, which, n):
    a32 = np.arange(n + 1, dtype=np.uint32)
    if which == "scan_max_inclusive_u32":
        return L.prims_scan_max_inclusive_u32, [pr.Guarded.of(a32[:n])], [pr.Guarded(4 * n)], lambda i, o: (i[0].ptr, o[0].ptr, n)
    if which == "scan_sum_exclusive_u32_u64":
        return L.prims_scan_sum_exclusive_u32_u64, [pr.Guarded.of(a32)], [pr.Guarded(8 * (n + 1))], lambda i, o: (i[0].ptr, o[0].ptr, n)
    if which == "scan_sum_exclusive_u64":
        return (L.prims_scan_sum_exclusive_u64, [pr.Guarded.of(a32.astype(np.uint64))], [pr.Guarded(8 * (n + 1))],
                lambda i, o: (i[0].ptr, o[0].ptr, n))
    if which == "scan_sum_exclusive_uint4":
        return (L.prims_scan_sum_exclusive_uint4, [pr.Guarded.of(np.ones((n, 4), dtype=np.uint32))], [pr.Guarded(16 * n)],
                lambda i, o: (i[0].ptr, o[0].ptr, n))
    flags = np.ones(n, dtype=np.uint8)
    if which == "select_indices_u32":
        return L.prims_select_indices_u32, [pr.Guarded.of(flags)], [pr.Guarded(4 * n), pr.Guarded(4)], lambda i, o: (i[0].ptr, o[0].ptr, o[1].ptr, n)
    if which == "select_flagged_u32":
        return (L.prims_select_flagged_u32, [pr.Guarded.of(a32[:n]), pr.Guarded.of(flags)], [pr.Guarded(4 * n), pr.Guarded(4)],
                lambda i, o: (i[0].ptr, i[1].ptr, o[0].ptr, o[1].ptr, n))
    raise ValueError(which)


@pytest.mark.parametrize("n", [0, 6149])
@pytest.mark.parametrize("which", ["scan_max_inclusive_u32", "scan_sum_exclusive_u32_u64", "scan_sum_exclusive_u64",
                                   "scan_sum_exclusive_uint4", "select_indices_u32", "select_flagged_u32"])
def test_undersized_tmp_is_refused(L, which, n):
    """tmp_bytes - 1: hipErrorInvalidValue and no output written (exclusive_scan_u32 takes no size of its tmp: its caller sizes
    it with scan_u32_tmp_words, which test_exclusive_scan_u32 checks with an exact, guarded tmp)."""
    fn, ins, outs, mk = _undersized(L, which, n)
    args = mk(ins, outs)
    need = pr.tmp_query(fn, *args)
    tmp = pr.Guarded(need - 1)
    rc = pr.call(fn, tmp, need - 1, *args)
    assert rc == pr.HIP_ERROR_INVALID_VALUE, f"{which} n={n} with tmp_bytes - 1: hipError {rc}"
    assert tmp.untouched() and all(o.untouched() for o in outs), f"{which}: wrote although it refused"
    intact(*ins)


@pytest.mark.parametrize("n", [0, 4097])
def test_undersized_tmp_is_refused_by_the_sort(L, n):
    keys = ps.sort_keys("uniform", n)
    kin, vin = pr.Guarded.of(keys), pr.Guarded.of(np.arange(n, dtype=np.uint32))
    kout, vout = pr.Guarded(8 * n), pr.Guarded(4 * n)
    args = (kin.ptr, kout.ptr, vin.ptr, vout.ptr, n, 0, 16)
    need = pr.tmp_query(L.prims_sort_pairs_u64_u32, *args)
    tmp = pr.Guarded(need - 1)
    rc = pr.call(L.prims_sort_pairs_u64_u32, tmp, need - 1, *args)
    assert rc == pr.HIP_ERROR_INVALID_VALUE, f"sort n={n} with tmp_bytes - 1: hipError {rc}"
    assert tmp.untouched() and kout.untouched() and vout.untouched()
    assert np.array_equal(kin.payload(np.uint64), keys), "the refused sort clobbered its input"
    intact(kin, vin)


# ---- sort_pairs_u64_u32 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,begin,end,pattern", ps.sort_cases(),
                         ids=[f"{n}-bits{b}_{e}-{p}" for n, b, e, p in ps.sort_cases()])
def test_sort_pairs_u64_u32(L, n, begin, end, pattern):
    """vals_out == the stable permutation exactly (values are arange(n): this is the stability test), keys_out == keys[perm] on
    all 64 bits.  The input buffers are documented as clobbered and are not looked at, beyond their guards."""
    keys = ps.sort_keys(pattern, n)
    perm = ps.sort_spec(keys, begin, end)
    kin, vin = pr.Guarded.of(keys), pr.Guarded.of(np.arange(n, dtype=np.uint32))
    kout, vout = pr.Guarded(8 * (n + 16)), pr.Guarded(4 * (n + 16))
    args = (kin.ptr, kout.ptr, vin.ptr, vout.ptr, n, begin, end)
    need = pr.tmp_query(L.prims_sort_pairs_u64_u32, *args)
    tmp = pr.Guarded(need)
    rc = pr.call(L.prims_sort_pairs_u64_u32, tmp, need, *args)
    what = f"sort_pairs_u64_u32 n={n} bits [{begin},{end}) {pattern} ({ps.sort_passes(begin, end)} passes)"
    assert rc == pr.HIP_SUCCESS, f"{what}: hipError {rc}"
    intact(kin, vin, kout, vout, tmp)
    v, k = vout.payload(np.uint32), kout.payload(np.uint64)
    first_diff(v[:n].astype(np.int64), perm, what + " vals_out")
    first_diff(k[:n], keys[perm], what + " keys_out")
    assert np.array_equal(v[n:], pr.filled(np.uint32, 16)) and np.array_equal(k[n:], pr.filled(np.uint64, 16)), \
        f"{what}: wrote past n"
