"""The genotype consensus on the MI355X (slamem_pileup_consensus_gt_*, engine.Pileup.consensus(genotype=...)): every output is
tests/cons_gt_spec.py applied to the same table, quality sums and events, compared for exact equality of bytes, offs and the eight
statistics -- the designed rows and events of cons_gt_cases, the edges of the read-out's tiles of 2,048 rows, a tile that emits
nothing and one of heterozygous rows, the capacity rule and the refusals, and the plurality read-out beside it."""
import ctypes as C

import numpy as np
import pytest

import cons_gt_cases as cases
import cons_gt_spec as cg
import cons_spec as cs
import events_spec as es

pytestmark = pytest.mark.gpu

ACGT = cases.ACGT
TILE = 2048
MD = cases.MIN_DEPTH


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


def planted(eng, text, t, q, raw, slots=256):
    idx = eng.Index.build(text)
    p = eng.Pileup(idx, events=True, event_slots=slots, quals=True)
    p.add_counts(t)
    p.quality.add_counts(q)
    if len(raw):
        p.add_events(es.to_records(raw))
    return idx, p


def check(p, T, t, q, E, ploidy=2, weighted=False, min_gq=20, costs=None, first=0, count=None, bounds=()):
    g = dict(ploidy=ploidy, min_gq=min_gq, weighted=weighted, costs=costs)
    got, offs, stats = p.consensus(MD, first, count, bounds=list(bounds) if len(bounds) else None, genotype=g)
    P_row, P_ev = cg.params(ploidy, weighted=weighted, costs=costs)
    want, woffs, wstats = cg.consensus(T, t, E, P_row, P_ev, MD, min_gq, q if weighted else None, first, count, bounds)
    assert got.dtype == np.uint8 and offs.dtype == np.uint64 and len(stats) == 8
    assert bytes(got) == want, (ploidy, weighted, min_gq, first, count)
    assert [int(v) for v in offs] == woffs and stats == wstats, (ploidy, weighted, min_gq, first, count, stats, wstats)
    return want, wstats


def test_designed_case(eng):
    case = cases.designed()
    T, t, q, E = case["T"], case["table"], case["qtable"], case["E"]
    idx, p = planted(eng, case["text"], t, q, case["raw"])
    assert es.from_records(p.events()[0]) == E and np.array_equal(p.counts(), t) and np.array_equal(p.quality.counts(), q)
    bounds = [0, 1, 51, 52, 100, 103, 140, 141, cases.N]
    seen = {}
    for ploidy, weighted, min_gq, costs in cases.COMBOS:
        seen[(ploidy, weighted, min_gq, costs)] = check(p, T, t, q, E, ploidy, weighted, min_gq, costs, bounds=bounds)
    assert len({v[0] for v in seen.values()}) >= 8  # (the calls differ: ploidy, the qualities and the threshold all show)
    assert set(seen[(2, False, 20, None)][0]) & set(b"MRWSYK") and not set(seen[(1, False, 20, None)][0]) & set(b"MRWSYK")
    assert seen[(2, False, 20, None)][1][7] == 1 and seen[(2, False, 20, None)][1][5] >= 3
    for first, count in ((12, 2), (100, 3), (101, 40), (140, 1), (51, 1), (cases.N, 0), (0, 0), (cases.BIG, 1)):
        check(p, T, t, q, E, 2, True, 20, first=first, count=count, bounds=[first, first + count])
    # the table, the quality sums and the events are what they were
    assert es.from_records(p.events()[0]) == E and np.array_equal(p.counts(), t) and np.array_equal(p.quality.counts(), q)
    p.close()
    idx.close()


# ---- tile edges ----------------------------------------------------------------------------------------------------------------

def tile_edge_case(n):
    """Rows of every kind around the tile's edge at 2,048: a homozygous variant on 2046 and, by the size, on the tile's last row
    2047 (a 10:10 row on 2048) or, with 2,049 rows, on the next tile's first row 2048 (a 10:10 row on 2047) -- they show in the read-out without
    events; with 4,097 rows the edge at 4,096 has the variant on 4095 and the 10:10 row on 4096, which no event covers.  With
    the events a homozygous deletion from 2046 crosses the edge, an insertion sits in front of it and one at row 1, and a deletion
    of two rows starts at n - 10."""
    rng = np.random.default_rng(n)
    text = rng.choice(ACGT, size=n)
    text[100:110] |= 0x20
    if n > 2047:  # the deletion from 2046 stays there
        dl = min(4, n - 2046)
        text[2045] = ACGT[(int(np.where(ACGT == text[2046 + dl - 1])[0][0]) + 1) % 4]
    text[n - 11] = ACGT[(int(np.where(ACGT == text[n - 9])[0][0]) + 1) % 4]  # ... and the one from n - 10
    T = bytes(text)
    own = cases.own_column(text)
    t = np.zeros((n, 6), dtype=np.uint32)
    t[np.arange(n), own] = 12
    snv = rng.choice(n, size=60, replace=False)
    t[snv, (own[snv] + 1) % 4] = 30
    het = rng.choice(n, size=60, replace=False)
    t[het, (own[het] + 2) % 4] = 12
    t[rng.choice(n, size=40, replace=False)] = 0
    hom = {2046, 2048 if n == 2049 else 2047, 4095}  # (2,049 rows: the variant on the next tile's first row; else on the tile's last)
    for x in (2046, 2047, 2048, 4095, 4096):
        if x < n:
            t[x] = 0
            t[x][own[x]], t[x][(own[x] + 1) % 4] = (0, 25) if x in hom else (10, 10)
    for a in (0, 2045, n - 11):  # the anchors of the events below
        t[a] = 0
        t[a][own[a]] = 20
    q = np.zeros((n, 6), dtype=np.uint32)
    q[:, :4] = t[:, :4] * rng.integers(2, 41, size=(n, 4)).astype(np.uint32)
    raw = [(1, 1, 1, cases.unlike(T, 1), 19, 0), (n - 10, 0, 2, b"", 0, 20)]
    if n > 2047:
        raw += [(2046, 0, dl, b"", 20, 0), (2046, 1, 2, b"A" + cases.unlike(T, 2046), 10, 9)]
    spec = es.Table(text)
    for e in raw:
        spec.observe(*e)
    E = spec.events()
    _, P_ev = cg.params(2)
    keys = {e[:3] for e in E if cg.event_call(T, t, e, P_ev, MD, 20)[0]}
    assert (1, 1, 1) in keys and (n - 10, 0, 2) in keys and (n <= 2047 or {(2046, 0, dl), (2046, 1, 2)} <= keys)
    return text, T, t, q, raw, E


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_tile_edges_ranges_and_bounds(eng, n):
    text, T, t, q, raw, E = tile_edge_case(n)
    idx, p = planted(eng, text, t, q, raw, 64)
    marks = [0, 1, 2046, 2047, 2048, 2049, 4095, 4096, n]
    for ploidy, weighted in ((2, False), (2, True), (1, True)):
        whole, st = check(p, T, t, q, E, ploidy, weighted, bounds=[b for b in marks if b <= n])
        assert ploidy == 1 or st[5] >= 30
    done = 0
    for first in (1, 2047, 2048):  # (an insertion sits at first = 1; the deletion from 2046 reaches into the ranges that start behind it)
        for count in (0, 1, 2049):
            if first + count > n:
                continue
            check(p, T, t, q, E, 2, True, first=first, count=count, bounds=[b for b in [first] + marks + [first + count] if first <= b <= first + count])
            done += 1
    assert done >= (3 if n == 2047 else 4)
    check(p, T, t, q, E, 2, False, first=0, count=n - 9, bounds=[0, n - 10, n - 9])  # the deletion from n - 10 crosses the range's end
    if n == 4097:  # the second edge, beside the events: the variant on the tile's last row, the IUPAC code on the next one's first
        whole, _ = check(p, T, t, q, E, 2, False, first=4090, count=7)
        assert whole[5:6] in b"ACGT" and whole[5] != T[4095] & 0xDF and whole[6:7] in b"MRWSYK"
    p.close()
    # without the events the rows at the edge show: the variant on the tile's last rows, IUPAC codes on both sides of the edge
    p0 = eng.Pileup(idx, quals=True)
    p0.add_counts(t)
    p0.quality.add_counts(q)
    for weighted in (False, True):
        whole, _ = check(p0, T, t, q, [], 2, weighted, bounds=[b for b in marks if b <= n])
        if n > 2048 and not weighted:  # (with the random qualities a 10:10 row may fall below the least GQ)
            v, h = (2048, 2047) if n == 2049 else (2047, 2048)
            for x in (2046, v):
                assert whole[x:x + 1] in b"ACGT" and whole[x] != T[x] & 0xDF
            assert whole[h:h + 1] in b"MRWSYK"
    check(p0, T, t, q, [], 2, True, first=2047 if n > 2047 else 2040, count=min(2, n - 2047) if n > 2047 else 5)
    p0.close()
    idx.close()


def test_a_tile_that_emits_nothing_and_a_tile_of_hets(eng):
    """4,097 rows: every row of tile 0 is 10:10, and chained homozygous deletions of 127 rows take all of tile 1."""
    n = 4097
    rng = np.random.default_rng(67)
    text = rng.choice(ACGT, size=n)
    starts = list(range(TILE, 2 * TILE, 127))
    for i, s in enumerate(starts + [2 * TILE]):  # the rows in front of the deletions and the last row: a deletion stays where it is
        text[s - 1] = ACGT[i % 2]
    T = bytes(text)
    own = cases.own_column(text)
    t = np.zeros((n, 6), dtype=np.uint32)
    t[np.arange(n), own] = 10
    t[np.arange(TILE - 1), (own[:TILE - 1] + 1 + np.arange(TILE - 1) % 3) % 4] = 10
    q = np.zeros((n, 6), dtype=np.uint32)
    q[:, :4] = t[:, :4] * 30
    raw = [(s, 0, min(127, 2 * TILE - s), b"", 6, 4) for s in starts]
    spec = es.Table(text)
    for e in raw:
        spec.observe(*e)
    E = spec.events()
    assert len(E) == len(raw)
    idx, p = planted(eng, text, t, q, raw, 256)
    for weighted in (False, True):
        want, st = check(p, T, t, q, E, 2, weighted, bounds=[0, 1, 2047, 2048, 2049, 4095, 4096, 4097])
        assert len(want) == TILE + 1 and st[2] == TILE and st[5] == TILE - 1 and not set(want[:TILE - 1]) - set(b"MRWSYK")
    got = p.consensus(MD, 2048, 2048, genotype=dict(weighted=True))
    assert got[0].size == 0 and got[2] == [0, 0, 2048, 0, 0, 0, 0, 0]
    check(p, T, t, q, E, 2, True, first=2047, count=2050, bounds=[2047, 2048, 4096, 4097])
    p.close()
    idx.close()


# ---- the C ABI: capacity, refusals, host buffers; the plurality read-out beside it ----------------------------------------------

def test_capacity_refusals_host_variant_and_plurality_unchanged(eng):
    import torch
    from slamem_amd import capi
    case = cases.designed()
    T, t, q, E, n = case["T"], case["table"], case["qtable"], case["E"], cases.N
    idx, p = planted(eng, case["text"], t, q, case["raw"])
    before = p.consensus(MD, bounds=[0, 100, n])
    want_plur = cs.consensus(T, t, E, MD, bounds=[0, 100, n])
    assert bytes(before[0]) == want_plur[0] and [int(v) for v in before[1]] == want_plur[1] and before[2] == want_plur[2]
    P_row, P_ev = cg.params(2, weighted=True)
    want, _, wstats = cg.consensus(T, t, E, P_row, P_ev, MD, 20, q)
    need = len(want)
    L = capi.lib()
    dev = idx.device
    prm = capi.ConsGtParams(eng._gt_params(2, 20, 30, MD, 0, eng.WQ_COSTS), eng._gt_params(2, 20, 30, MD, 0), MD, 20, 1)
    total, stats = C.c_uint64(), (C.c_uint64 * 8)()
    rc = L.slamem_pileup_consensus_gt_device(p._h, 0, n, C.byref(prm), 0, None, None, 0, None, stats, C.byref(total), None)
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == need and list(stats) == wstats  # (capacity 0, no buffer: the size)
    buf = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=dev)
    for small in (1, 63, need - 1):
        buf.fill_(0x5A)
        rc = L.slamem_pileup_consensus_gt_device(p._h, 0, n, C.byref(prm), small, buf.data_ptr(), None, 0, None, stats, C.byref(total), None)
        torch.cuda.synchronize()
        assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == need and list(stats) == wstats
        assert bool((buf[small:] == 0x5A).all()) and bytes(buf[:small].cpu().numpy()) == want[:small]
    got = p.consensus(MD, capacity=3, genotype=dict(weighted=True))  # (the engine asks once more with the need)
    assert bytes(got[0]) == want and got[2] == wstats
    # the host variant agrees with the device variant
    out = np.full(need + 8, 0x5A, dtype=np.uint8)
    hb = np.array([0, 52, 141, n], dtype=np.uint64)
    ho = np.zeros(len(hb), dtype=np.uint64)
    rc = L.slamem_pileup_consensus_gt_host(p._h, 0, n, C.byref(prm), need, out.ctypes.data, hb.ctypes.data, len(hb), ho.ctypes.data, stats, C.byref(total))
    assert rc == capi.SLAMEM_OK and total.value == need and bytes(out[:need]) == want and bool((out[need:] == 0x5A).all())
    assert [int(v) for v in ho] == cg.consensus(T, t, E, P_row, P_ev, MD, 20, q, bounds=[0, 52, 141, n])[1] and list(stats) == wstats
    out[:] = 0x5A
    rc = L.slamem_pileup_consensus_gt_host(p._h, 0, n, C.byref(prm), 10, out.ctypes.data, None, 0, None, stats, C.byref(total))
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == need and bytes(out[:10]) == want[:10] and bool((out[10:] == 0x5A).all())
    rc = L.slamem_pileup_consensus_gt_host(p._h, 100, 50, C.byref(prm), need, out.ctypes.data, hb.ctypes.data + 16, 1, ho.ctypes.data, stats, C.byref(total))
    assert rc == capi.SLAMEM_OK
    rc = L.slamem_pileup_consensus_gt_host(p._h, 100, 40, C.byref(prm), need, out.ctypes.data, hb.ctypes.data + 16, 1, ho.ctypes.data, stats, C.byref(total))
    assert rc == capi.SLAMEM_ERR_ARG and b"bound" in L.slamem_last_error_message()
    # refusals
    plain = eng.Pileup(idx, events=True)
    plain.add_counts(t)
    for pile, bad in ((plain, dict(weighted=True)), (p, dict(min_gq=1000)), (p, dict(ploidy=3)), (p, dict(costs=(0, 0, 5))), (p, dict(het_q=1000))):
        with pytest.raises((capi.SlamemError, ValueError)) as err:
            pile.consensus(MD, genotype=bad)
        assert not isinstance(err.value, capi.SlamemError) or err.value.code == capi.SLAMEM_ERR_ARG, bad
    with pytest.raises(capi.SlamemError) as err:
        plain.consensus(MD, genotype=dict(weighted=True))
    assert err.value.code == capi.SLAMEM_ERR_ARG and "quality sums" in str(err.value)
    with pytest.raises(capi.SlamemError) as err:
        p.consensus(MD, genotype=dict(min_gq=1000))
    assert err.value.code == capi.SLAMEM_ERR_ARG
    for bad in (dict(first=n + 1, count=0), dict(first=n - 1, count=2), dict(min_depth=0), dict(min_depth=2 ** 31)):
        with pytest.raises(capi.SlamemError) as err:
            p.consensus(genotype={}, **bad)
        assert err.value.code == capi.SLAMEM_ERR_ARG
    with pytest.raises(ValueError):
        p.consensus(MD, genotype=dict(min_qual=3))
    # an accumulator without quality sums runs the unweighted call, and it is the one of the spec
    P2, _ = cg.params(2)
    got = plain.consensus(MD, genotype={})
    assert bytes(got[0]) == cg.consensus(T, t, E[:0], P2, P_ev, MD, 20)[0]
    plain.close()
    # the plurality read-out is what it was before the genotype calls, and nothing of the accumulator was written
    after = p.consensus(MD, bounds=[0, 100, n])
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]) and after[2] == before[2] and len(after[2]) == 5
    assert es.from_records(p.events()[0]) == E and np.array_equal(p.counts(), t) and np.array_equal(p.quality.counts(), q)
    p.close()
    idx.close()
