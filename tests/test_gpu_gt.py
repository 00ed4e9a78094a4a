"""-gt on the MI355X (slamem_pileup_genotypes_*, slamem_pileup_genotype_events_*, engine.Pileup.genotypes / genotype_events, the
executable): every result is tests/gt_spec.py applied to the table the same accumulator gives through counts(), compared for
exact equality, every byte of the genotype records included -- on tables planted row by row (tile borders, the last partial
tile, a full and an empty tile, ties, the largest counts), on ranges, on a capacity that is too small, on planted events, on real
mappings whatever the batches' order or the stream, and on the file the executable writes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import events_spec as es
import gt_spec as gs
from test_gpu_chain import indel_reads
from test_events_host import planted_deletion
from test_gpu_sites import halves, run_stream, windows, write_fasta
from test_sites_host import PLANTED_SEED, planted_sample

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slamem_amd", "host", "slaMEM-hip")
COL = {ord(c): k for k, c in enumerate("ACGT")}
# the arguments of Pileup.genotypes: the defaults, ploidy 1, everything let through, other costs
ARGS = [dict(), dict(ploidy=1), dict(min_depth=1, min_qual=0), dict(ploidy=1, min_depth=1, min_qual=0), dict(err_q=40, het_q=0, min_qual=3),
        dict(err_q=3, het_q=999, min_depth=2)]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


def spec_params(**kw):
    return gs.params(**kw)


def same_genotypes(got, want, what=None):
    pos, counts, gts = got
    assert pos.dtype == np.uint64 and counts.dtype == np.uint32 and gts.dtype == gs.GENOTYPE_DTYPE, what
    assert pos.shape == want[0].shape and counts.shape == want[1].shape and gts.shape == want[2].shape, (what, pos.shape, want[0].shape)
    assert np.array_equal(pos, want[0]) and np.array_equal(counts, want[1]), what
    assert gts.tobytes() == want[2].tobytes(), what  # (every byte: the padding too)


def check_all(p, text, table, args=ARGS, ranges=((0, None),)):
    n = 0
    for kw in args:
        for first, count in ranges:
            want = gs.genotypes(table, text, spec_params(**kw), first, count)
            same_genotypes(p.genotypes(first=first, count=count, **kw), want, (kw, first, count))
            n += len(want[0])
    return n


def variant_row(text, x, ref=10, alt=10, other=0, step=1):
    """The text's letter `ref` times, another letter `alt` times, a third `other` times."""
    r = COL[int(text[x]) & 0xDF]
    row = [0] * 6
    row[r], row[(r + step) % 4], row[(r + step + 1) % 4] = ref, alt, other
    return row


# ---- planted tables ------------------------------------------------------------------------------------------------------------

def planted_table():
    """A text of 2 * 2048 + 5 rows in two records (the separator at 3000) with an N at 2500, and a table: rows 0, 2047, 2048, 4095,
    4096 and n - 1 hold a variant, and so do the separator and the N row (which select nothing); around them hets, hom-alts, two
    alternatives, rows below the depth and below the quality, D and I counters, and random rows."""
    rng = np.random.default_rng(24)
    n = 2 * 2048 + 5
    text = rng.choice(ACGT, size=n)
    text[3000] = text[2500] = ord("N")
    text[5] = ord("a")  # (lower case folds)
    t = np.zeros((n, 6), dtype=np.int64)
    for x in np.nonzero(rng.random(n) < 0.25)[0]:
        t[x] = rng.integers(0, 14, size=6) * (rng.random(6) < 0.5)
    for x in (0, 2047, 2048, 4095, 4096, n - 1, 5):
        t[x] = variant_row(text, x)
    for x in (3000, 2500):
        t[x] = (10, 10, 0, 0, 0, 0)
    t[10] = variant_row(text, 10, 0, 20)            # hom-alt
    t[11] = variant_row(text, 11, 0, 10, 10)        # two alternatives
    t[12] = variant_row(text, 12, 3, 1)             # hom-ref wins
    t[13] = variant_row(text, 13, 2, 2)             # qual 7474: below 20, above 7
    t[14] = variant_row(text, 14, 1, 2)             # depth 3
    t[14, 4] = 1                                    # ... 4 with the D counter
    t[15] = variant_row(text, 15, 1, 2)             # depth 3: the I counter does not count
    t[15, 5] = 7
    t[16] = variant_row(text, 16, 7, 7, step=3)
    return text, t


def test_planted_table_ranges_and_both_ploidies(eng):
    text, table = planted_table()
    n = len(text)
    assert n == 4101
    idx = eng.Index.build(text)
    p = eng.Pileup(idx)
    p.add_counts(table.astype(np.uint32))
    assert np.array_equal(p.counts().astype(np.int64), table)
    # the table is what the docstring says it is
    pos, _, gts = gs.genotypes(table, text, gs.params())
    sel = set(int(x) for x in pos)
    assert {0, 5, 2047, 2048, 4095, 4096, n - 1, 10, 11, 16} <= sel and not {3000, 2500, 12, 13, 15} & sel
    by = {int(x): g for x, g in zip(pos, gts)}
    assert int(by[0]["qual"]) == 157370 and int(by[10]["a"]) == int(by[10]["b"]) != int(by[10]["ref"])
    assert int(by[11]["a"]) != int(by[11]["ref"]) != int(by[11]["b"]) != int(by[11]["a"])
    assert 13 in set(int(x) for x in gs.genotypes(table, text, gs.params(min_qual=7))[0])
    assert 14 in set(int(x) for x in gs.genotypes(table, text, gs.params(min_qual=0))[0])
    assert 15 not in set(int(x) for x in gs.genotypes(table, text, gs.params(min_qual=0))[0])
    assert check_all(p, text, table) > 100
    ranges = ((1000, 3097), (2047, 2), (2048, 2048), (n - 5, 5), (n - 1, 1), (n, 0), (0, 0), (0, 1), (5, 50), (4096, 1), (3000, 1))
    check_all(p, text, table, args=[dict(), dict(ploidy=1, min_qual=0)], ranges=ranges)
    # the read-out leaves the accumulator alone
    assert np.array_equal(p.counts().astype(np.int64), table)
    p.close()
    idx.close()


def test_a_full_tile_and_an_empty_tile(eng):
    """Tile 1 has all 2,048 rows selected, tile 2 none (rows that are looked at and fall to the reference), tile 0 every other row,
    the short tile 3 its first and last: the ranks come from ballots of 64 set bits, of none, and of alternating ones."""
    rng = np.random.default_rng(3)
    n = 3 * 2048 + 7
    text = rng.choice(ACGT, size=n)
    t = np.zeros((n, 6), dtype=np.int64)
    for x in range(0, 2048, 2):
        t[x] = variant_row(text, x, 6, 9, step=1 + x % 3)
    for x in range(2048, 4096):
        t[x] = variant_row(text, x, x % 7, 10 + x % 5, x % 3, step=1 + x % 3)
    for x in range(4096, 6144):
        t[x] = variant_row(text, x, 9, 1)
    t[6144] = variant_row(text, 6144)
    t[n - 1] = variant_row(text, n - 1)
    idx = eng.Index.build(text)
    p = eng.Pileup(idx)
    p.add_counts(table := t.astype(np.uint32))
    for kw in (dict(), dict(ploidy=1)):
        pos = gs.genotypes(t, text, gs.params(**kw))[0]
        assert set(range(2048, 4096)) <= set(int(x) for x in pos) and not any(4096 <= x < 6144 for x in pos)
    assert len(gs.genotypes(t, text, gs.params())[0]) == 1024 + 2048 + 2
    check_all(p, text, t, args=[dict(), dict(ploidy=1)], ranges=((0, None), (2048, 2048), (4096, 2048), (2000, 2200)))
    assert np.array_equal(p.counts(), table)
    p.close()
    idx.close()


def test_ties_and_the_largest_counts(eng):
    """Rows whose scores tie (the reference keeps them, then the smallest g) under costs given through the C interface, and counts
    of 2^31 - 1 and 2^32 - 1: qual, gq and pl saturate, no sum wraps."""
    import torch
    from slamem_amd import capi
    rng = np.random.default_rng(8)
    n = 300
    text = rng.choice(ACGT, size=n)
    big = 2 ** 31 - 1
    t = np.zeros((n, 6), dtype=np.int64)
    for k, x in enumerate(range(10, 90)):
        r = COL[int(text[x])]
        if k % 4 == 0:
            t[x, r], t[x, (r + 1) % 4] = 7, 7                      # het against hom-ref
        elif k % 4 == 1:
            t[x, (r + 1) % 4], t[x, (r + 2) % 4] = 6, 6            # two alternatives alike
        elif k % 4 == 2:
            t[x, (r + 1) % 4], t[x, (r + 2) % 4], t[x, (r + 3) % 4] = 5, 5, 5
        else:
            t[x, :4] = rng.integers(0, 4, size=4)
    t[100] = (big, big, 0, 0, 0, 0)
    t[101] = (big,) * 6
    t[102] = (0, 0, big, big, big, 0)
    t[103] = (2 ** 32 - 1,) * 6
    t[104] = (2 ** 32 - 1, 1, 0, 0, 0, 0)
    t[105] = (0, 2 ** 32 - 1, 0, 2 ** 32 - 2, 0, 0)
    idx = eng.Index.build(text)
    p = eng.Pileup(idx)
    p.add_counts(t.astype(np.uint32))
    got = check_all(p, text, t, args=[dict(), dict(ploidy=1), dict(min_depth=1, min_qual=0), dict(err_q=93, het_q=999, min_depth=1, min_qual=0),
                                      dict(min_depth=2 ** 31 - 1, min_qual=999)])
    assert got > 10
    pos, _, gts = p.genotypes()
    assert 100 in set(int(x) for x in pos) and int(gts[list(pos).index(100)]["qual"]) == gs.SAT
    # costs that make ties, through the C interface
    L = capi.lib()
    dev = idx.device
    for costs in ((2, 10, 30, 50, 0, 1, 0), (2, 5, 5, 5, 0, 1, 0), (2, 1, 1000, 1000, 0, 1, 0), (2, 1000, 1, 1000, 0, 1, 0), (1, 1, 1000, 1000, 0, 1, 0),
                  (2, 2 ** 20, 2 ** 20, 2 ** 20, 2 ** 20, 1, 0), (1, 0, 1, 2 ** 20, 2 ** 20, 1, 999)):
        want = gs.genotypes(t, text, costs)
        cap = n
        pd = torch.zeros(cap, dtype=torch.int64, device=dev)
        cd = torch.zeros((cap, 6), dtype=torch.int32, device=dev)
        gd = torch.zeros(cap * 56, dtype=torch.uint8, device=dev)
        total = C.c_uint64()
        prm = capi.GtParams(*costs)
        assert L.slamem_pileup_genotypes_device(p._h, 0, n, C.byref(prm), cap, pd.data_ptr(), cd.data_ptr(), gd.data_ptr(), C.byref(total),
                                                None) == capi.SLAMEM_OK
        torch.cuda.synchronize()
        m = total.value
        same_genotypes((pd[:m].cpu().numpy().view(np.uint64), cd[:m].cpu().numpy().view(np.uint32),
                        gd[:m * 56].cpu().numpy().view(gs.GENOTYPE_DTYPE)), want, costs)
    p.close()
    idx.close()


# ---- capacity and arguments ----------------------------------------------------------------------------------------------------

def test_capacity_too_small_reports_the_need_and_writes_nothing_beyond(eng):
    import torch
    from slamem_amd import capi
    text, table = planted_table()
    n = len(text)
    idx = eng.Index.build(text)
    p = eng.Pileup(idx)
    p.add_counts(table.astype(np.uint32))
    prm = capi.GtParams(*gs.params(min_depth=1, min_qual=0))
    want = gs.genotypes(table, text, gs.params(min_depth=1, min_qual=0))
    need = len(want[0])
    assert need > 200
    L = capi.lib()
    dev = idx.device
    cap = 3
    pos = torch.full((cap + 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    rows = torch.full((cap + 8, 6), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    gts = torch.full(((cap + 8) * 56,), 0x5A, dtype=torch.uint8, device=dev)
    total = C.c_uint64()
    rc = L.slamem_pileup_genotypes_device(p._h, 0, n, C.byref(prm), cap, pos.data_ptr(), rows.data_ptr(), gts.data_ptr(), C.byref(total), None)
    torch.cuda.synchronize()
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == need
    assert b"selected" in L.slamem_last_error_message()
    assert bool((pos[cap:] == 0x5A5A5A5A5A5A5A5A).all()) and bool((rows[cap:] == 0x5A5A5A5A).all()) and bool((gts[cap * 56:] == 0x5A).all())
    # (what fits is the head of the result)
    same_genotypes((pos[:cap].cpu().numpy().view(np.uint64), rows[:cap].cpu().numpy().view(np.uint32),
                    gts[:cap * 56].cpu().numpy().view(gs.GENOTYPE_DTYPE)), tuple(w[:cap] for w in want))
    # the host call: the same need, and room for it gives the result
    hp, hc = np.zeros(need + 2, dtype=np.uint64), np.zeros((need + 2, 6), dtype=np.uint32)
    hg = np.full((need + 2) * 56, 0x5A, dtype=np.uint8)
    rc = L.slamem_pileup_genotypes_host(p._h, 0, n, C.byref(prm), 5, hp.ctypes.data, hc.ctypes.data, hg.ctypes.data, C.byref(total))
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == need and bool((hg[5 * 56:] == 0x5A).all())
    rc = L.slamem_pileup_genotypes_host(p._h, 0, n, C.byref(prm), need, hp.ctypes.data, hc.ctypes.data, hg.ctypes.data, C.byref(total))
    assert rc == capi.SLAMEM_OK and total.value == need and bool((hg[need * 56:] == 0x5A).all())
    same_genotypes((hp[:need], hc[:need], hg[:need * 56].view(gs.GENOTYPE_DTYPE)), want)
    # no room at all: the count alone
    rc = L.slamem_pileup_genotypes_device(p._h, 0, n, C.byref(prm), 0, None, None, None, C.byref(total), None)
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == need
    # the wrapper asks again with the need
    same_genotypes(p.genotypes(min_depth=1, min_qual=0, capacity=3), want)
    same_genotypes(p.genotypes(min_depth=1, min_qual=0, capacity=need), want)
    p.close()
    idx.close()


def test_argument_refusals(eng):
    from slamem_amd import capi
    text, table = planted_table()
    n = len(text)
    idx = eng.Index.build(text)
    p = eng.Pileup(idx)
    L = capi.lib()
    out = np.zeros(64, dtype=np.uint64)
    o = out.ctypes.data
    total = C.c_uint64()
    good = (2, 44, 3039, 24771, 30000, 4, 20)

    def dev_call(first, count, prm):
        return L.slamem_pileup_genotypes_device(p._h, first, count, C.byref(capi.GtParams(*prm)), 1, o, o, o, C.byref(total), None)

    def host_call(first, count, prm):
        return L.slamem_pileup_genotypes_host(p._h, first, count, C.byref(capi.GtParams(*prm)), 1, o, o, o, C.byref(total))

    def ev_dev_call(first, count, prm):
        return L.slamem_pileup_genotype_events_device(p._h, o, o, 0, C.byref(capi.GtParams(*prm)), o, o, None)

    def ev_host_call(first, count, prm):
        return L.slamem_pileup_genotype_events_host(p._h, o, o, 0, C.byref(capi.GtParams(*prm)), o, o)
    bad_params = [(0,) + good[1:], (3,) + good[1:], (2, 44, 0, 24771, 30000, 4, 20), (2, 44, 3039, 0, 30000, 4, 20),
                  (2, 2 ** 20 + 1, 3039, 24771, 30000, 4, 20), (2, 44, 2 ** 20 + 1, 24771, 30000, 4, 20), (2, 44, 3039, 2 ** 20 + 1, 30000, 4, 20),
                  (2, 44, 3039, 24771, 2 ** 20 + 1, 4, 20), (2, 44, 3039, 24771, 30000, 0, 20), (2, 44, 3039, 24771, 30000, 2 ** 31, 20),
                  (2, 44, 3039, 24771, 30000, 4, 1000)]
    for call, name in ((dev_call, b"slamem_pileup_genotypes_device"), (host_call, b"slamem_pileup_genotypes_host"),
                       (ev_dev_call, b"slamem_pileup_genotype_events_device"), (ev_host_call, b"slamem_pileup_genotype_events_host")):
        for prm in bad_params:
            assert call(0, 10, prm) == capi.SLAMEM_ERR_ARG, (name, prm)
            assert name in L.slamem_last_error_message()
        assert call(0, 10, good) == capi.SLAMEM_OK
    for call in (dev_call, host_call):
        for first, count in ((n + 1, 0), (n - 3, 4), (0, n + 1)):
            assert call(first, count, good) == capi.SLAMEM_ERR_ARG
            assert b"outside the text" in L.slamem_last_error_message()
        # an empty table selects nothing; the largest depth and quality are taken
        assert call(0, n, (1, 0, 1, 1, 0, 2 ** 31 - 1, 999)) == capi.SLAMEM_OK and total.value == 0
    assert L.slamem_pileup_genotypes_device(None, 0, 0, C.byref(capi.GtParams(*good)), 0, None, None, None, C.byref(total), None) == capi.SLAMEM_ERR_ARG
    assert L.slamem_pileup_genotypes_device(p._h, 0, 10, None, 0, None, None, None, C.byref(total), None) == capi.SLAMEM_ERR_ARG
    assert L.slamem_pileup_genotypes_device(p._h, 0, 10, C.byref(capi.GtParams(*good)), 0, None, None, None, None, None) == capi.SLAMEM_ERR_ARG
    # an anchor at or beyond n: the host variant says so before any device work
    ev = es.to_records([(5, 0, 1, b"", 1, 1)])
    g, c = np.zeros(56, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
    for a in (n, n + 5, 2 ** 40):
        anchors = np.array([a], dtype=np.uint64)
        assert L.slamem_pileup_genotype_events_host(p._h, ev.ctypes.data, anchors.ctypes.data, 1, C.byref(capi.GtParams(*good)), g.ctypes.data,
                                                    c.ctypes.data) == capi.SLAMEM_ERR_ARG
        assert b"anchor" in L.slamem_last_error_message()
    for bad in (dict(ploidy=3), dict(ploidy=0), dict(min_depth=0), dict(min_qual=1000), dict(first=n + 1, count=0)):
        with pytest.raises(capi.SlamemError) as e:
            p.genotypes(**bad)
        assert e.value.code == capi.SLAMEM_ERR_ARG
    for bad in (dict(err_q=0), dict(err_q=94), dict(het_q=1000)):
        with pytest.raises(ValueError):
            p.genotypes(**bad)
    with pytest.raises(ValueError):
        p.genotype_events(ev, [n])
    with pytest.raises(capi.SlamemError):
        p.genotype_events(ev, [4], ploidy=3)
    p.close()
    idx.close()


def test_compact_index_is_refused(eng, monkeypatch):
    from slamem_amd import capi
    ref, q, off = indel_reads(13)
    monkeypatch.setenv("SLAMEM_INDEX_LAYOUT", "compact")
    idx = eng.Index.build(ref)
    monkeypatch.delenv("SLAMEM_INDEX_LAYOUT")
    assert idx.info.layout == capi.LAYOUT_COMPACT
    with pytest.raises(capi.SlamemError) as e:  # (no accumulator, so no genotypes: the refusal of the other read-outs)
        eng.Pileup(idx).genotypes()
    assert e.value.code == capi.SLAMEM_ERR_ARG and "text planes" in str(e.value) and "compact" in str(e.value)
    idx.close()


# ---- events --------------------------------------------------------------------------------------------------------------------

def test_planted_events_with_anchors_at_a_records_first_row_and_at_the_last_row(eng):
    from slamem_amd import capi
    rng = np.random.default_rng(31)
    n = 2 * 2048 + 5
    text = rng.choice(ACGT, size=n)
    text[3000] = ord("N")  # two records: 0 .. 2999 and 3001 .. n - 1
    t = np.zeros((n, 6), dtype=np.int64)
    # (pos, kind, len, letters, fwd, rev) and the depth planted on the anchor row
    plan = [((3001, 1, 2, b"GA", 5, 4), 20), ((3001, 0, 1, b"", 10, 10), 20), ((n - 1, 1, 1, b"C", 3, 3), 9), ((n - 1, 0, 1, b"", 0, 9), 9),
            ((0, 1, 3, b"TTA", 2, 2), 40), ((1, 0, 2, b"", 1, 0), 40), ((2048, 1, 1, b"A", 7, 7), 14), ((2049, 0, 3, b"", 30, 0), 20),
            ((500, 0, 1, b"", 2, 2), 8), ((600, 0, 1, b"", 1, 1), 3), ((700, 1, 1, b"G", 2 ** 32 - 1, 2 ** 32 - 1), 2 ** 32 - 1),
            ((800, 0, 1, b"", 7, 0), 14), ((900, 0, 1, b"", 0, 1), 0)]
    evs, anchors = [], []
    for ev, depth in plan:
        a = ev[0] if ev[0] in (0, 3001) else ev[0] - 1
        evs.append(ev)
        anchors.append(a)
        t[a, COL[int(text[a])]] = depth  # (two events of one anchor: the same depth)
    t[699] = (2 ** 32 - 1,) * 6
    assert n - 2 in anchors and 3001 in anchors and 0 in anchors
    idx = eng.Index.build(text)
    p = eng.Pileup(idx, events=True)
    p.add_counts(t.astype(np.uint32))
    table = p.counts().astype(np.int64)
    assert np.array_equal(table, t)
    recs = es.to_records(evs)
    for kw in ARGS:
        want_g, want_c = gs.genotype_events(evs, table[anchors], spec_params(**kw))
        got_g, got_c = p.genotype_events(recs, anchors, **kw)
        assert got_g.dtype == gs.GENOTYPE_DTYPE and got_g.tobytes() == want_g.tobytes(), kw
        assert got_c.dtype == np.uint8 and np.array_equal(got_c, want_c), kw
    want_g, want_c = gs.genotype_events(evs, table[anchors], gs.params())
    assert want_c.tolist()[:8] == [1, 1, 1, 1, 0, 0, 1, 1] and set(want_c.tolist()) == {0, 1}
    assert [(int(g["a"]), int(g["b"])) for g in want_g[:4]] == [(0, 1), (1, 1), (0, 1), (1, 1)]
    # the host variant reads the anchors' rows itself; the events may come from the table as well
    L = capi.lib()
    hg, hc = np.full(len(evs) * 56, 0x5A, dtype=np.uint8), np.full(len(evs), 0x5A, dtype=np.uint8)
    apos = np.array(anchors, dtype=np.uint64)
    assert L.slamem_pileup_genotype_events_host(p._h, recs.ctypes.data, apos.ctypes.data, len(evs), C.byref(capi.GtParams(*gs.params())),
                                                hg.ctypes.data, hc.ctypes.data) == capi.SLAMEM_OK
    assert hg.tobytes() == want_g.tobytes() and np.array_equal(hc, want_c)
    assert p.genotype_events(recs[:0], [])[0].shape == (0,)
    p.close()
    idx.close()




# ---- real mappings -------------------------------------------------------------------------------------------------------------

REAL_ARGS = [dict(), dict(min_depth=1, min_qual=0), dict(ploidy=1, min_depth=2, min_qual=5)]


def two_record_sample():
    """Two records with a known answer.  Record one is test_gpu_sites' generator: a random reference of 12,000 letters and the
    error-free reads of a sample with 20 substitutions, every fifth position, alternating strands -- and beside them error-free
    reads of the reference itself over its first 6,000 letters, so the substitutions there are heterozygous and the others
    homozygous.  Record two is test_events_host's: a reference of 3,000 letters with a run of eight A and 20 reads of a sample
    without three of them.  Returns (merged text, the two records, the substituted positions, the sample, the deletion's position
    in the merged text, reads, offsets); every read has 150 letters."""
    import ext_spec
    ref1, sample, at, q1, _ = planted_sample(PLANTED_SEED)
    extra = [ext_spec.revcomp(ref1[a:a + 150]) if k % 2 else ref1[a:a + 150].copy() for k, a in enumerate(range(0, 6000, 5))]
    ref2, run, q2, _ = planted_deletion()
    text = np.concatenate([ref1, [ord("N")], ref2]).astype(np.uint8)
    q = np.concatenate([q1] + extra + [q2])
    assert len(q) % 150 == 0
    off = np.arange(len(q) // 150 + 1, dtype=np.uint64) * np.uint64(150)
    return text, [ref1, ref2], at, sample, len(ref1) + 1 + run, q, off


def test_real_mappings_any_order_and_the_stream(eng):
    text, _, at, sample, del_pos, q, off = two_record_sample()
    min_len = 20
    idx = eng.Index.build(text)
    p = eng.Pileup(idx, events=True)
    recs = p.add(q, off, min_len, True)
    assert int((recs["strand"] == 1).sum()) > 1000 and int((recs["strand"] == 2).sum()) > 1000
    table = p.counts().astype(np.int64)
    whole = {}
    for k, kw in enumerate(REAL_ARGS):
        got = p.genotypes(**kw)
        same_genotypes(got, gs.genotypes(table, text, spec_params(**kw)), kw)
        whole[k] = got
    # the known answer, judged without the spec: exactly the 20 planted substitutions, heterozygous with the reference's letter
    # where the reference's reads lie as well, homozygous for the sample's letter elsewhere
    pos, counts, gts = whole[0]
    print("planted", list(at), "got", list(pos), [(int(g["a"]), int(g["b"]), int(g["qual"]), int(g["gq"])) for g in gts])
    assert list(pos) == list(at) and len(at) == 20
    for x, g in zip(at, gts):
        r, s = COL[int(text[x])], COL[int(sample[x])]
        assert int(g["ref"]) == r and int(g["ploidy"]) == 2 and int(g["qual"]) >= 20000
        if x < 5800:
            assert (int(g["a"]), int(g["b"])) == (min(r, s), max(r, s)), x
        elif x > 6200:
            assert (int(g["a"]), int(g["b"])) == (s, s), x
    assert any(x < 5800 for x in at) and any(x > 6200 for x in at)
    assert set(int(x) for x in at if x > 6200) <= set(int(x) for x in whole[2][0]) <= set(int(x) for x in at)  # (ploidy 1: the plurality letter)
    check_all(p, text, table, args=[dict(min_depth=1, min_qual=0)], ranges=((2037, 4101), (len(text) - 1700, 1700)))
    # the reads' one event: the deletion of three A, on every read that holds it, so 1/1 at the anchor in front of it
    ev = p.events()[0]
    assert es.from_records(ev) == [(del_pos, 0, 3, b"", 10, 10)]
    anchors = [del_pos - 1]
    evg = {}
    for k, kw in enumerate(REAL_ARGS):
        want_g, want_c = gs.genotype_events(es.from_records(ev), table[anchors], spec_params(**kw))
        got_g, got_c = p.genotype_events(ev, anchors, **kw)
        assert got_g.tobytes() == want_g.tobytes() and np.array_equal(got_c, want_c), kw
        evg[k] = (got_g, got_c)
    assert evg[0][1].tolist() == [1] and (int(evg[0][0][0]["a"]), int(evg[0][0][0]["b"])) == (1, 1)

    def same_as_whole(x):
        for k, kw in enumerate(REAL_ARGS):
            same_genotypes(x.genotypes(**kw), whole[k], kw)
        e2 = x.events()[0]
        assert e2.tobytes() == ev.tobytes()
        for k, kw in enumerate(REAL_ARGS):
            g2, c2 = x.genotype_events(e2, anchors, **kw)
            assert g2.tobytes() == evg[k][0].tobytes() and np.array_equal(c2, evg[k][1])
    # the halves in the other order
    (qa, oa), (qb, ob) = halves(q, off)
    p.reset()
    p.add(qb, ob, min_len, True)
    p.add(qa, oa, min_len, True)
    same_as_whole(p)
    # a stream of match type 8 feeds the accumulator
    p.reset()
    run_stream(eng, idx, p, q, windows(off, 400), 2, min_len)  # (400 reads of 150 letters: inside the stream's 65,536 per batch)
    same_as_whole(p)
    p.close()
    idx.close()


# ---- the executable ------------------------------------------------------------------------------------------------------------

def test_cli_file_is_the_spec_of_the_engines_tables(eng, tmp_path):
    """slaMEM-hip -b -vcf -gt ref.fa reads.fa on the reference of two records: byte for byte the file gt_spec formats from the
    engine's pileup and events; the same with two logical GPUs (the tables and the events merged on GPU 0); with other parameters
    and at ploidy 1 other files; and -vcf without -gt writes what events_spec says, as before."""
    import hostlib
    text, recs, at, _, del_pos, q, off = two_record_sample()
    ref_fa, q_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    write_fasta(ref_fa, [(b"one first", recs[0]), (b"two\tsecond", recs[1])])
    write_fasta(q_fa, [(b"read%d x" % k, q[int(off[k]):int(off[k + 1])]) for k in range(len(off) - 1)])
    loaded = hostlib.Loaded(ref_fa, 1)
    assert loaded.chars == bytes(text)
    idx = eng.Index.build(text)
    p = eng.Pileup(idx, events=True)
    p.add(q, off, 20, True)
    table = p.counts().astype(np.int64)
    ev = es.from_records(p.events()[0])
    p.close()
    idx.close()
    dflt = gs.vcf_file(table, ev, loaded, gs.params())
    loose = gs.vcf_file(table, ev, loaded, gs.params(err_q=10, het_q=5, min_depth=2, min_qual=3))
    hap = gs.vcf_file(table, ev, loaded, gs.params(ploidy=1, err_q=25, het_q=10, min_qual=0))
    head = gs.vcf_header(loaded)
    assert dflt.startswith(head) and dflt.count(b"\n") == head.count(b"\n") + 21 and dflt.count(b";SF=10;SR=10\tGT:DP:AD:GQ:PL\t1/1:") == 1
    assert dflt.count(b"\none\t") == 20 and dflt.count(b"\ntwo\t") == 1 and b"\t0/1:" in dflt and dflt.count(b"\t1/1:") > 5
    assert len({dflt, loose, hap}) == 3 and b"/" not in hap[len(head):].replace(b"GT:DP:AD:GQ:PL", b"")
    base = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for name, env in (("one", base), ("two", dict(base, SLAMEM_LOGICAL_GPUS="2", SLAMEM_BATCH_MB="1"))):
        out = str(tmp_path / (name + ".vcf"))
        r = subprocess.run([EXE, "-b", "-vcf", "-gt", "-o", out, ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
        assert open(out, "rb").read() == dflt
        assert b"Saving variant calls" in r.stdout
        assert b"; minimum depth = 4 ; ploidy = 2 ; error rate = 20 Phred ; prior = 30 Phred ; minimum quality = 20\n" in r.stdout
    for name, args, want in (("hap", ["-ploidy", "1", "-err", "25", "-hetq", "10", "-qual", "0"], hap),):
        out = str(tmp_path / (name + ".vcf"))
        r = subprocess.run([EXE, "-vcf", "-gt"] + args + ["-b", "-o", out, ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=base, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
        assert open(out, "rb").read() == want, name
    r = subprocess.run([EXE, "-vcf", "-b", ref_fa, q_fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=base, timeout=300)
    assert r.returncode == 0 and open(str(tmp_path / "ref-mems.txt"), "rb").read() == es.vcf_file(table, ev, loaded)
    assert b"; minimum depth = 4 ; minimum share = 20 %\n" in r.stdout
