"""-depth on the MI355X (slamem_pileup_depth_runs_*, engine.Pileup.depth_runs, the executable): every result is
tests/depth_spec.py applied to the table the same accumulator gives through counts(), compared for exact equality -- on a table
planted row by row (a run over a whole tile and both its borders, a tile of nothing but heads, an empty tile, heads at the tiles'
borders, equal depths in other columns, depths beyond 2^32), on ranges and bounds, on a capacity that is too small, on real
mappings whatever the batches' order, the stream or the number of accumulators; and, without the spec, a known answer in closed
form."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import depth_spec as ds
from test_depth_host import COVER_SEED, cover_answer, cover_depth, cover_sample, pairs
from test_gpu_chain import indel_reads
from test_gpu_map import multi_record_batch
from test_gpu_sites import halves, run_stream, windows, write_fasta

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
SIXTEEN = tuple(range(1, 17))


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


def check(p, table, levels=(), md=1, first=0, count=None, bounds=()):
    pos, val, cum = p.depth_runs(levels if levels else None, md, first, count, bounds=list(bounds) if len(bounds) else None)
    wp, wv = ds.runs(table, levels, first, count)
    assert pos.dtype == np.uint64 and val.dtype == np.uint64 and cum.dtype == np.uint64 and cum.shape == (len(bounds), 2)
    assert np.array_equal(pos, wp) and np.array_equal(val, wv), (levels, first, count)
    assert np.array_equal(cum, ds.cum(table, md, first, bounds)), (levels, md, first, count)
    return pos, val


# ---- planted -------------------------------------------------------------------------------------------------------------------

def planted_tables():
    """A text of 10,000 letters (five tiles of 2,048 rows, the last one short) with a few N, and two tables, the second one the
    first plus a few counts.  In both, tile 3 (rows 6144 .. 8191) is empty, rows 300 .. 302 hold the depth 6 in other columns (all
    in D, all in A, all in A with an I) and row 34 sums beyond 2^32.  In the first, the depth 7 runs from row 2040 to row 4099: one
    run covers tile 1 and both its borders.  In the second, rows 2047 and 4095 stand out and rows 4096 .. 6143 alternate: heads fall
    at 2047, 2048, 4095, 4096, every row of tile 2 is a head, and so are 6144 and n - 1."""
    rng = np.random.default_rng(23)
    n = 10000
    text = rng.choice(ACGT, size=n)
    for x in (100, 1999, 2050, 4500, 9000, 9001):
        text[x] = ord("N")
    t = np.zeros((n, 6), dtype=np.int64)
    for x in np.nonzero(rng.random(n) < 0.4)[0]:  # tiles 0 and 4: random rows in stretches
        if x < 2000 or 8192 <= x < n - 2:
            t[x:x + int(rng.integers(1, 5))] = rng.integers(0, 4, size=6) * (rng.random(6) < 0.6)
    t[2000:2040] = 0
    t[n - 2:] = 0
    t[n - 1] = (0, 5, 0, 0, 0, 0)
    t[2040:4100] = 0
    t[2040:4100, 4] = 7                 # all in D, also under the N at 2050
    t[2100:2200] = (1, 2, 3, 1, 0, 4)   # the same depth in the letters' columns
    t[4100:6144:2] = (8, 0, 0, 0, 0, 0)
    t[4101:6144:2] = (0, 4, 0, 0, 5, 1)
    t[6144:8192] = 0
    t[299] = 0
    t[300], t[301], t[302], t[303] = (0, 0, 0, 0, 6, 0), (6, 0, 0, 0, 0, 0), (6, 0, 0, 0, 0, 9), (0, 0, 0, 0, 0, 6)
    t[30:40] = 0
    t[34] = (2 ** 31 - 1,) * 6
    t[35], t[36] = (20, 0, 0, 0, 0, 0), (0, 0, 0, 0, 21, 0)  # (two depths to the exact read-out, one value to sixteen levels)
    t[100] = (3, 0, 0, 2, 1, 1)         # under an N
    t[1999] = (0, 0, 0, 0, 7, 0)
    more = np.zeros((n, 6), dtype=np.int64)
    more[2047, 1] = 1
    more[4095, 2] = 3
    more[4096:4100:2, 0] = 1
    more[4097:4100:2, 3] = 2
    return text, t, t + more


def test_planted_tables_levels_ranges_and_bounds(eng):
    text, t1, t2 = planted_tables()
    n = len(text)
    # the tables are what the docstring says they are
    e1, e2 = pairs(ds.runs(t1)), pairs(ds.runs(t2))
    assert (2040, 7) in e1 and not any(2040 < p <= 4099 for p, _ in e1) and (4100, 8) in e1
    h2 = {p for p, _ in e2}
    assert {2047, 2048, 4095, 4096, 6144, n - 1} <= h2 and set(range(4096, 6145)) <= h2
    assert not any(2048 < p < 4095 for p in h2) and not any(6144 < p < 8192 for p in h2)
    assert (300, 6) in e1 and not {301, 302} & {p for p, _ in e1} and (303, 0) in e1
    assert (34, 5 * (2 ** 31 - 1)) in e1 and 5 * (2 ** 31 - 1) > 2 ** 32
    assert ds.depth(t1)[100] == 6 and ds.depth(t1)[2050] == 7
    assert (2040, 1) in pairs(ds.runs(t1, (7,))) and (4100, 1) in pairs(ds.runs(t1, (8,))) and (2040, 1) not in pairs(ds.runs(t1, (8,)))
    idx = eng.Index.build(text)
    p = eng.Pileup(idx)
    bounds = [0, 0, 1, 2047, 2048, 2049, 4095, 4096, 6144, 8192, n - 1, n, n]
    ranges = ((2037, 4101), (2047, 2), (2048, 2048), (n - 70, 70), (n, 0), (0, 0), (4100, 1), (6000, 3000))
    for table in (t1, t2):
        p.add_counts((table if table is t1 else t2 - t1).astype(np.uint32))
        assert np.array_equal(p.counts().astype(np.int64), table)
        lens = {}
        for levels in ((), (1,), (4, 30), SIXTEEN, (7,), (8,), (2 ** 32 - 1,)):
            pos, _ = check(p, table, levels, 1, bounds=bounds)
            lens[levels] = len(pos)
        assert lens[()] > lens[SIXTEEN] >= lens[(4, 30)] > 1 and lens[(2 ** 32 - 1,)] == 3
        for md in (4, 7, 8, 2 ** 31 - 1):
            check(p, table, (), md, bounds=bounds)
        for first, count in ranges:
            inner = sorted({first, first + count, min(first + count, max(first, 2048)), min(first + count, max(first, 4096)),
                            first + count // 2})
            for levels in ((), (4, 30)):
                check(p, table, levels, 7, first, count, bounds=[first] + inner + [first + count, first + count])
        # the read-out leaves the accumulator alone
        assert np.array_equal(p.counts().astype(np.int64), table)
    # many bounds: every row, and every row twice
    check(p, t2, (1,), 8, bounds=list(range(n + 1)))
    check(p, t2, (), 1, 2047, 4100, bounds=sorted(list(range(2047, 6148)) * 2))
    p.close()
    idx.close()


# ---- the C ABI: capacity, refusals, host buffers -------------------------------------------------------------------------------

def test_capacity_too_small_reports_the_need_and_writes_nothing_beyond(eng):
    import torch
    from slamem_amd import capi
    text, _, t2 = planted_tables()
    n = len(text)
    idx = eng.Index.build(text)
    p = eng.Pileup(idx)
    p.add_counts(t2.astype(np.uint32))
    wp, wv = ds.runs(t2)
    need = len(wp)
    assert need > 2048
    bounds = [0, 2048, 5000, n]
    wc = ds.cum(t2, 7, 0, bounds)
    L = capi.lib()
    dev = idx.device
    S = 0x5A5A5A5A5A5A5A5A
    bd = torch.from_numpy(np.array(bounds, dtype=np.uint64).view(np.int64)).to(dev)
    total = C.c_uint64()
    for cap in (3, 2049):
        runs = torch.full((cap + 8, 2), S, dtype=torch.int64, device=dev)
        cum = torch.full((len(bounds) + 2, 2), S, dtype=torch.int64, device=dev)
        rc = L.slamem_pileup_depth_runs_device(p._h, 0, n, None, 0, 7, cap, runs.data_ptr(), bd.data_ptr(), len(bounds), cum.data_ptr(),
                                               C.byref(total), None)
        torch.cuda.synchronize()
        assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == need
        assert b"runs" in L.slamem_last_error_message()
        assert bool((runs[cap:] == S).all()) and bool((cum[len(bounds):] == S).all())
        got = runs[:cap].cpu().numpy().view(np.uint64)  # (what fits is the head of the result)
        assert np.array_equal(got[:, 0], wp[:cap]) and np.array_equal(got[:, 1], wv[:cap])
        assert np.array_equal(cum[:len(bounds)].cpu().numpy().view(np.uint64), wc)  # (cum is complete either way)
    # no room at all: the count and cum alone; without bounds the count alone
    cum = torch.full((len(bounds) + 2, 2), S, dtype=torch.int64, device=dev)
    rc = L.slamem_pileup_depth_runs_device(p._h, 0, n, None, 0, 7, 0, None, bd.data_ptr(), len(bounds), cum.data_ptr(), C.byref(total), None)
    torch.cuda.synchronize()
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == need
    assert np.array_equal(cum[:len(bounds)].cpu().numpy().view(np.uint64), wc) and bool((cum[len(bounds):] == S).all())
    lv = (C.c_uint32 * 2)(4, 30)
    rc = L.slamem_pileup_depth_runs_device(p._h, 0, n, lv, 2, 1, 0, None, None, 0, None, C.byref(total), None)
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == len(ds.runs(t2, (4, 30))[0])
    # the host call: the same need, and room for it gives the result
    hr = np.full((need + 2, 2), S, dtype=np.uint64)
    hb = np.array(bounds, dtype=np.uint64)
    hc = np.zeros((len(bounds), 2), dtype=np.uint64)
    rc = L.slamem_pileup_depth_runs_host(p._h, 0, n, None, 0, 7, 5, hr.ctypes.data, hb.ctypes.data, len(hb), hc.ctypes.data, C.byref(total))
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == need and bool((hr[5:] == S).all()) and np.array_equal(hr[:5, 0], wp[:5])
    assert np.array_equal(hc, wc)
    rc = L.slamem_pileup_depth_runs_host(p._h, 0, n, None, 0, 7, need, hr.ctypes.data, hb.ctypes.data, len(hb), hc.ctypes.data, C.byref(total))
    assert rc == capi.SLAMEM_OK and total.value == need and bool((hr[need:] == S).all())
    assert np.array_equal(hr[:need, 0], wp) and np.array_equal(hr[:need, 1], wv) and np.array_equal(hc, wc)
    rc = L.slamem_pileup_depth_runs_host(p._h, 0, n, None, 0, 7, 0, None, None, 0, None, C.byref(total))
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == need
    # the wrapper asks again with the need
    for cap in (3, need, None):
        pos, val, _ = p.depth_runs(capacity=cap)
        assert np.array_equal(pos, wp) and np.array_equal(val, wv)
    assert np.array_equal(p.counts().astype(np.int64), t2)
    p.close()
    idx.close()


def test_argument_refusals(eng):
    from slamem_amd import capi
    text, t1, _ = planted_tables()
    n = len(text)
    idx = eng.Index.build(text)
    p = eng.Pileup(idx)
    L = capi.lib()
    import torch
    dev = idx.device
    room = torch.zeros((64, 2), dtype=torch.int64, device=dev)
    hroom = np.zeros((64, 2), dtype=np.uint64)
    total = C.c_uint64()

    def levels_of(lv):
        return ((C.c_uint32 * len(lv))(*lv) if len(lv) else None), len(lv)

    def dev_call(first, count, lv, md):
        a, k = levels_of(lv)
        return L.slamem_pileup_depth_runs_device(p._h, first, count, a, k, md, 8, room.data_ptr(), None, 0, None, C.byref(total), None)

    def host_call(first, count, lv, md):
        a, k = levels_of(lv)
        return L.slamem_pileup_depth_runs_host(p._h, first, count, a, k, md, 8, hroom.ctypes.data, None, 0, None, C.byref(total))
    for call, name in ((dev_call, b"slamem_pileup_depth_runs_device"), (host_call, b"slamem_pileup_depth_runs_host")):
        for args in ((n + 1, 0, (), 1), (n - 3, 4, (), 1), (0, n + 1, (), 1), (0, 10, tuple(range(1, 18)), 1), (0, 10, (0,), 1),
                     (0, 10, (0, 5), 1), (0, 10, (3, 3), 1), (0, 10, (4, 1), 1), (0, 10, (1, 5, 5), 1), (0, 10, (), 0), (0, 10, (), 2 ** 31),
                     (0, 10, (1,), 2 ** 32 - 1)):
            assert call(*args) == capi.SLAMEM_ERR_ARG, args
            assert name in L.slamem_last_error_message()
        # the edges that are allowed: 16 levels, the largest level and depth, an empty range at the text's end
        assert call(0, 10, SIXTEEN, 2 ** 31 - 1) == capi.SLAMEM_OK and total.value == 1
        assert call(0, 10, (2 ** 32 - 1,), 1) == capi.SLAMEM_OK
        assert call(n, 0, (), 1) == capi.SLAMEM_OK and total.value == 0
    assert L.slamem_pileup_depth_runs_device(None, 0, 0, None, 0, 1, 0, None, None, 0, None, C.byref(total), None) == capi.SLAMEM_ERR_ARG
    assert b"slamem_pileup_depth_runs_device" in L.slamem_last_error_message()
    assert L.slamem_pileup_depth_runs_device(p._h, 0, 10, None, 0, 1, 0, None, None, 0, None, None, None) == capi.SLAMEM_ERR_ARG
    assert L.slamem_pileup_depth_runs_host(None, 0, 0, None, 0, 1, 0, None, None, 0, None, C.byref(total)) == capi.SLAMEM_ERR_ARG
    assert b"slamem_pileup_depth_runs_host" in L.slamem_last_error_message()
    assert L.slamem_pileup_depth_runs_host(p._h, 0, 10, None, 0, 1, 0, None, None, 0, None, None) == capi.SLAMEM_ERR_ARG
    # the host variant: a bound outside the range, bounds that descend
    hc = np.zeros((4, 2), dtype=np.uint64)
    for first, count, b in ((100, 50, [99]), (100, 50, [151]), (100, 50, [120, 119]), (0, 10, [0, 10, 9]), (0, 0, [1])):
        hb = np.array(b, dtype=np.uint64)
        rc = L.slamem_pileup_depth_runs_host(p._h, first, count, None, 0, 1, 8, hroom.ctypes.data, hb.ctypes.data, len(hb), hc.ctypes.data,
                                             C.byref(total))
        assert rc == capi.SLAMEM_ERR_ARG and b"slamem_pileup_depth_runs_host" in L.slamem_last_error_message(), b
    hb = np.array([100, 100, 150, 150], dtype=np.uint64)
    rc = L.slamem_pileup_depth_runs_host(p._h, 100, 50, None, 0, 1, 8, hroom.ctypes.data, hb.ctypes.data, 4, hc.ctypes.data, C.byref(total))
    assert rc == capi.SLAMEM_OK and total.value == 1 and hc.tolist() == [[0, 0], [0, 0], [0, 0], [0, 0]]
    for bad in (dict(levels=(0,)), dict(levels=(2, 2)), dict(levels=tuple(range(1, 18))), dict(min_depth=0), dict(min_depth=2 ** 31),
                dict(first=n + 1, count=0), dict(first=n - 1, count=2)):
        with pytest.raises(capi.SlamemError) as e:
            p.depth_runs(**bad)
        assert e.value.code == capi.SLAMEM_ERR_ARG
    p.close()
    idx.close()


# ---- real mappings -------------------------------------------------------------------------------------------------------------

QUERIES = [((), 1), ((1,), 4), ((1, 4, 30), 2), (SIXTEEN, 1)]


def read_out(p, n, bounds):
    return [p.depth_runs(levels if levels else None, md, bounds=bounds) for levels, md in QUERIES]


def same_read_out(got, want):
    for g, w in zip(got, want):
        assert all(np.array_equal(a, b) for a, b in zip(g, w))


@pytest.mark.parametrize("case", ["indel_reads", "multi_record"])
def test_real_mappings_any_order_the_stream_and_merged_accumulators(eng, case):
    if case == "indel_reads":
        ref, q, off = indel_reads(21)
        min_len = 14
    else:
        ref, q, off = multi_record_batch()
        min_len = 20
    n = len(ref)
    idx = eng.Index.build(ref)
    p = eng.Pileup(idx)
    recs = p.add(q, off, min_len, True)
    assert int((recs["strand"] == 1).sum()) > 10 and int((recs["strand"] == 2).sum()) > 10
    table = p.counts().astype(np.int64)
    bounds = [0, 2048, 3000, 3001, n // 2, n]
    whole = read_out(p, n, bounds)
    for (levels, md), (pos, val, cum) in zip(QUERIES, whole):
        wp, wv = ds.runs(table, levels)
        assert np.array_equal(pos, wp) and np.array_equal(val, wv) and np.array_equal(cum, ds.cum(table, md, 0, bounds)), levels
    # the comparison is not between trivial lists
    assert len(whole[0][0]) > 10 and len(whole[1][0]) > 10 and int(whole[0][2][-1][0]) > 1000
    assert bool((table[:, 4] > 0).any()) == (case == "indel_reads")
    for first, count in ((2037, 4101), (n - 70, 70)):
        check(p, table, (), 1, first, count, bounds=[first, first + count])
        check(p, table, (1, 4), 2, first, count, bounds=[first, first + 11, first + count])
    # the halves in the other order
    (qa, oa), (qb, ob) = halves(q, off)
    p.reset()
    p.add(qb, ob, min_len, True)
    p.add(qa, oa, min_len, True)
    same_read_out(read_out(p, n, bounds), whole)
    # a stream of match type 8 feeds the accumulator
    p.reset()
    run_stream(eng, idx, p, q, windows(off, (len(off) - 1 + 2) // 3), 2, min_len)
    same_read_out(read_out(p, n, bounds), whole)
    # two accumulators, a half each, merged
    a, b = eng.Pileup(idx), eng.Pileup(idx)
    a.add(qa, oa, min_len, True)
    b.add(qb, ob, min_len, True)
    a.add_counts(b.counts())
    assert np.array_equal(a.counts().astype(np.int64), table)
    same_read_out(read_out(a, n, bounds), whole)
    if case == "indel_reads":  # a read alone at each place, three of them with a deleted letter: a depth that column D alone holds
        p.reset()
        p.add(q[:int(off[7])], off[:8].copy(), min_len, True)
        few = p.counts().astype(np.int64)
        assert int(((few[:, :4].sum(axis=1) == 0) & (few[:, 4] > 0)).sum()) == 3
        check(p, few, (), 1, bounds=[0, n])
        assert len(check(p, few, (1,), 1)[0]) == 15  # (seven places covered, the deleted letters among them)
    for x in (a, b, p):
        x.close()
    idx.close()


def test_cover_sample_gives_the_closed_form(eng):
    """A known answer, judged without the spec: a random reference of 12,000 letters and error-free reads of 150 letters from
    every fifth position, alternating strands, at a minimum match length of 20.  Every read maps where it was taken from, so d(p)
    is the number of k with 5k <= p < 5k + 150 and 5k + 150 <= n: the depth climbs by one every five rows to 30, stays, and falls
    by one every five rows to 1 (test_depth_host.cover_answer).  The seed (test_depth_host.COVER_SEED) is fixed, and
    test_depth_host.test_cover_sample_answer_holds_on_the_definition confirms the answer for it on the CPU."""
    ref, q, off = cover_sample(COVER_SEED)
    n = len(ref)
    idx = eng.Index.build(ref)
    p = eng.Pileup(idx)
    recs = p.add(q, off, 20, True)
    assert np.array_equal(recs["strand"], 1 + np.arange(len(off) - 1) % 2)
    pos, val, cum = p.depth_runs(bounds=[0, 150, n - 150, n], min_depth=30)
    print("runs", pairs((pos, val))[:8], "...", len(pos), "cum", cum.tolist())
    assert pairs((pos, val)) == cover_answer() and len(pos) == 59
    d = cover_depth()
    assert cum.tolist() == [[0, 0], [int(d[:150].sum()), 5], [int(d[:n - 150].sum()), n - 295], [150 * (len(off) - 1), n - 290]]
    pos, val, _ = p.depth_runs((1, 30))
    assert pairs((pos, val)) == cover_answer((1, 30)) == [(0, 1), (145, 2), (n - 145, 1)]
    p.close()
    idx.close()


# ---- the executable ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cli_case(eng, tmp_path_factory):
    """The three-record reference of test_gpu_sites.py's CLI test, its files, and the engine's tables at -minq 1 and -minq 0."""
    import hostlib
    tmp = tmp_path_factory.mktemp("depth_cli")
    ref, q, off = multi_record_batch()
    recs = [ref[:3000], ref[3001:8001], ref[8002:]]
    ref_fa, q_fa = str(tmp / "ref.fa"), str(tmp / "reads.fa")
    write_fasta(ref_fa, [(b"one first", recs[0]), (b"two\tsecond", recs[1]), (b"three", recs[2])])
    write_fasta(q_fa, [(b"read%d x" % k, q[int(off[k]):int(off[k + 1])]) for k in range(len(off) - 1)])
    loaded = hostlib.Loaded(ref_fa, 1)
    assert loaded.chars == bytes(ref)
    idx = eng.Index.build(ref)
    p = eng.Pileup(idx)
    p.add(q, off, 20, True, min_mapq=1)
    table = p.counts().astype(np.int64)
    p.reset()
    p.add(q, off, 20, True)
    zero = p.counts().astype(np.int64)
    p.close()
    idx.close()
    assert not np.array_equal(table, zero)
    return tmp, ref_fa, q_fa, loaded, table, zero


@pytest.mark.parametrize("mode", ["runs", "levels", "windows"])
def test_cli_file_is_the_spec_of_the_engines_table(cli_case, mode):
    """slaMEM-hip -b -l 20 -depth -minq 1 ref.fa reads.fa: byte for byte the bedGraph depth_spec formats from the engine's table,
    with one GPU and with two logical GPUs (an accumulator each, added on the device before the read-out); -lev 1,4 and -win 100
    likewise; the summary on stderr is the spec's."""
    tmp, ref_fa, q_fa, loaded, table, zero = cli_case
    extra, want, md = {"runs": ([], ds.bedgraph_file(table, loaded), 1),
                       "levels": (["-lev", "1,4", "-mdep", "4"], ds.bedgraph_file(table, loaded, (1, 4)), 4),
                       "windows": (["-win", "100"], ds.window_file(table, loaded, 100), 1)}[mode]
    assert want.count(b"\n") > 20 and want.startswith(b"one\t0\t") and b"\ntwo\t0\t" in want and b"\nthree\t0\t" in want
    if mode == "runs":
        assert want != ds.bedgraph_file(zero, loaded)
    if mode == "windows":
        assert want.count(b"\n") == 30 + 50 + 40
    base = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for name, env in (("one", base), ("two", dict(base, SLAMEM_LOGICAL_GPUS="2", SLAMEM_BATCH_MB="1"))):
        out = str(tmp / (mode + name + ".txt"))
        r = subprocess.run([EXE, "-b", "-l", "20", "-depth", "-minq", "1"] + extra + ["-o", out, ref_fa, q_fa], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, env=env, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
        assert open(out, "rb").read() == want
        summary = b"".join(l + b"\n" for l in r.stderr.split(b"\n") if l.startswith(b"> Depth of "))
        assert summary == ds.summary_lines(table, loaded, md) and summary.count(b"\n") == 3
        assert b"Saving depth runs" in r.stdout and b"; minimum mapping quality = 1 ; covered from depth = %d\n" % md in r.stdout
