"""-wq on the MI355X (slamem_pileup_enable_quals, slamem_pileup_quality, slamem_pileup_add_quals_device, the k_qual_* kernels,
slamem_pileup_genotypes_weighted_*, engine.Pileup(quals=True)): the quality accumulator against tests/qual_spec.py on the batch of
test_gpu_sb with designed quality strings -- in one add, two adds in either order, through a stream, with a low-quality mask, with
the duplicate filter and beside strand counts -- and against code that was there before: constant quality gives q times a plain
Pileup's counts, a planted Q of zeros gives genotypes(), a planted Q = q * P gives genotypes() with err_cost + 1000 q."""
import ctypes as C

import numpy as np
import pytest

import dedup_spec as dd
import gt_spec as gs
import lowq_spec
import pile_spec
import qual_spec as qs
from test_gpu_aln import batch
from test_gpu_gt import planted_table
from test_gpu_pile import halves, spec_results, windows
from test_gpu_sb import MIN_LEN, MIN_MAPQ, N, sb_batch

pytestmark = pytest.mark.gpu

RUN_VALUES = (2, 12, 23, 37)  # the four values a sequencer bins its qualities into
EVERY = (35, 73, 33, 126, 20, 255, 44, 34)  # a change at every letter: among them '!', '~', a byte below 33 and 255


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


def letter_at_row(res, length, row):
    """The index (in the read as given) of the letter that the read's walk puts on `row` under = or X; None when there is none."""
    strand = res[0]
    for (p, q, _rlen, _qlen, _ed, rl) in res[4]:
        p, q = int(p), int(q)
        for c, k in rl:
            k = int(k)
            if c in "=X":
                if p <= row < p + k:
                    t = q + (row - p)
                    return length - 1 - t if strand == 2 else t
                p += k
                q += k
            elif c == "D":
                p += k
            else:
                q += k
    return None


def exact(res):
    """(p, q, k) of a read whose walk is one = run; None for any other."""
    if res[0] == 0 or len(res[4]) != 1 or len(res[4][0][5]) != 1 or res[4][0][5][0][0] != "=":
        return None
    return int(res[4][0][0]), int(res[4][0][1]), int(res[4][0][5][0][1])


def design_quals(res, off, rng):
    """The batch's quality bytes and what was designed, a list of (what, read) for the test of the batch's own claims."""
    quals = np.zeros(int(off[-1]), dtype=np.uint8)
    made = []
    nq = len(off) - 1
    for k in range(nq):  # four values in runs, as a sequencer bins them
        a, b = int(off[k]), int(off[k + 1])
        x = a
        while x < b:
            run = int(rng.integers(1, 50))
            quals[x:min(b, x + run)] = 33 + RUN_VALUES[int(rng.integers(0, 4))]
            x += run

    def given(k, t):  # letter t of the scanned strand of read k, as an index into quals
        length = int(off[k + 1]) - int(off[k])
        return int(off[k]) + (length - 1 - t if res[k][0] == 2 else t)

    def flat(k, v=33 + 30):
        quals[int(off[k]):int(off[k + 1])] = v

    todo = {(what, s): None for s in (1, 2) for what in ("const", "every", "row64", "row63", "row65", "l7", "l8", "l9", "first", "last")}
    for k in range(nq):
        r, length = res[k], int(off[k + 1]) - int(off[k])
        if r[0] == 0 or r[1] < MIN_MAPQ:
            continue
        big = max(len(s[5]) for s in r[4]) > 32
        if big or k % 7 == 0:  # every wave-kernel read, and every seventh: a change at every letter
            quals[int(off[k]):int(off[k + 1])] = [EVERY[i % len(EVERY)] for i in range(length)]
            made.append(("wave" if big else "every", r[0]))
            todo[("every", r[0])] = k
            continue
        e = exact(r)
        if e is None:
            continue
        p, q, run = e
        row = (p + 10 + 63) // 64 * 64  # a text row with x & 63 == 0, inside the run
        free = [w for (w, s), v in todo.items() if s == r[0] and v is None]
        if not free or run < 50 or row + 2 >= p + run:
            continue
        what = free[0]
        todo[(what, r[0])] = k
        made.append((what, r[0]))
        flat(k)
        if what == "const":
            continue
        if what == "every":
            quals[int(off[k]):int(off[k + 1])] = [EVERY[i % len(EVERY)] for i in range(length)]
        elif what.startswith("row"):  # one change, at the row, a row in front of it, a row behind it
            t = q + (row + {"row64": 0, "row63": -1, "row65": 1}[what] - p)
            for u in range(t, q + run):
                quals[given(k, u)] = 33 + 11
        elif what in ("l7", "l8", "l9"):  # the eight-byte compare's edge
            for u in range(q + int(what[1]), q + run):
                quals[given(k, u)] = 33 + 11
        elif what == "first":
            quals[given(k, q)] = 33 + 5
        elif what == "last":
            quals[given(k, q + run - 1)] = 33 + 5
    for k in range(nq):  # a change on the letter over the N row (2500), for the reads that show one there
        length = int(off[k + 1]) - int(off[k])
        g = letter_at_row(res[k], length, 2500)
        if g is not None and res[k][0] != 0:
            quals[int(off[k]) + g] = 33 + 61
            made.append(("N", res[k][0]))
    return quals, made, todo


@pytest.fixture(scope="module")
def world(eng):
    text, reads = sb_batch()
    idx = eng.Index.build(text)
    q, off = batch(reads)
    res = spec_results(idx, text, q, off, MIN_LEN, True)
    quals, made, todo = design_quals(res, off, np.random.default_rng(27))
    want = pile_spec.pile(res, q, off, N, MIN_MAPQ)
    qwant = qs.pile(res, q, off, quals, N, None, MIN_MAPQ)
    yield dict(text=text, idx=idx, reads=reads, q=q, off=off, res=res, quals=quals, made=made, todo=todo, want=want, qwant=qwant)
    idx.close()


def same(got, want, what=None):
    assert got.dtype == np.uint32 and got.shape == want.shape, what
    bad = np.nonzero((got.astype(np.int64) != want).any(axis=1))[0]
    assert len(bad) == 0, "%s rows %s: got %s, want %s" % (what, bad[:5], got[bad[:5]].tolist(), want[bad[:5]].tolist())


def test_the_batch_is_what_it_claims(eng, world):
    made, todo, qwant, want = world["made"], world["todo"], world["qwant"], world["want"]
    assert all(v is not None for v in todo.values()), [k for k, v in todo.items() if v is None]
    for s in (1, 2):
        assert ("wave", s) in made and ("N", s) in made, s
    vals = set(world["quals"].tolist())
    assert {33, 126, 20, 255} <= vals
    assert not qwant[:, 4:].any() and bool((qwant[:, :4] <= 93 * want[:, :4]).all()) and qwant.sum() > 0
    for x in (2047, 2048, 4095, 4096, N - 1):
        assert qwant[x, :4].sum() > 0, x
    assert (qwant[2500].sum() > 0) == (want[2500, :4].sum() > 0) and want[:, 4].sum() > 0 and want[:, 5].sum() > 0


def test_one_add_ranges_and_reset(eng, world):
    idx, q, off, quals = world["idx"], world["q"], world["off"], world["quals"]
    p = eng.Pileup(idx, quals=True)
    assert p.quality is not None and p.quality.quality is None and p.forward is None
    p.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ, quals=quals)
    same(p.counts(), world["want"], "counts")
    got = p.quality.counts()
    same(got, world["qwant"], "one add")
    for first, count in ((2040, 20), (4090, 11), (N - 1, 1), (0, 0), (2048, 2048), (100, 3000)):  # (starts and ends inside a tile)
        assert np.array_equal(p.quality.counts(first, count), got[first:first + count])
    at = [0, 2047, 2048, 2500, 4095, 4096, N - 1]
    assert np.array_equal(p.quality.rows_at(at), got[at])
    p.reset()
    assert not p.counts().any() and not p.quality.counts().any()
    p.enable_quals()  # (on an empty accumulator, and a second time: nothing changes)
    p.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ, quals=quals.tobytes())
    same(p.quality.counts(), world["qwant"], "after reset")
    p.close()
    assert p.quality._h is None


def test_two_adds_in_either_order(eng, world):
    idx, q, off, quals = world["idx"], world["q"], world["off"], world["quals"]
    (qa, oa), (qb, ob) = halves(q, off)
    cut = len(qa)
    va, vb = quals[:cut], quals[cut:]
    p = eng.Pileup(idx, quals=True)
    for k, order in enumerate((((qa, oa, va), (qb, ob, vb)), ((qb, ob, vb), (qa, oa, va)))):
        for qq, oo, vv in order:
            p.add(qq, oo, MIN_LEN, True, min_mapq=MIN_MAPQ, quals=vv)
        same(p.quality.counts(), world["qwant"], ("order", k))
        same(p.counts(), world["want"], ("order", k))
        p.reset()
    p.close()


def test_stream_with_quality_bytes(eng, world):
    idx, q, off, quals = world["idx"], world["q"], world["off"], world["quals"]
    wins, slots = windows(off, 70), 2
    p = eng.Pileup(idx, quals=True)
    st = eng.Stream(idx, slots, 1 << 16, len(wins[0]) - 1, True, pile=p, min_mapq=MIN_MAPQ, quals=True)
    from slamem_amd import capi
    with pytest.raises(capi.SlamemError) as e:  # a batch without quality bytes would leave Q behind
        st.submit(q, wins[0], 14)
    assert e.value.code == capi.SLAMEM_ERR_ARG and "slamem_stream_submit_quals" in str(e.value)
    for b in range(min(slots - 1, len(wins))):
        st.submit_quals(q, quals, None, wins[b], 14)
    for b in range(len(wins)):
        st.next()
        if b + slots - 1 < len(wins):
            st.submit_quals(q, quals, None, wins[b + slots - 1], 14)
    st.close()
    same(p.counts(), world["want"], "stream counts")
    same(p.quality.counts(), world["qwant"], "stream")
    with pytest.raises(capi.SlamemError) as e:  # the setter needs an accumulator with quality sums
        plain = eng.Pileup(idx)
        eng.Stream(idx, 2, 1 << 16, 64, True, pile=plain, quals=True)
    assert "slamem_stream_set_quals" in str(e.value)
    with pytest.raises(capi.SlamemError) as e:  # and such an accumulator a stream that was told
        st = eng.Stream(idx, 2, 1 << 16, 64, True, pile=p)
        st.submit(q, wins[0], 14)
    assert "slamem_stream_set_quals" in str(e.value)
    st.close()
    plain.close()
    p.close()


def test_low_quality_mask(eng, world):
    idx, q, off, res, quals = world["idx"], world["q"], world["off"], world["res"], world["quals"]
    rng = np.random.default_rng(6)
    bits = (rng.random(int(off[-1])) < 0.08).astype(np.uint8)
    for k in world["todo"].values():  # the masked letter is the one the quality changes on (and its neighbours are not)
        a, b = int(off[k]), int(off[k + 1])
        v = quals[a:b]
        change = a + 1 + np.nonzero(v[1:] != v[:-1])[0]
        bits[a:b] = 0
        bits[change[:3]] = 1
    mask = lowq_spec.from_bits(bits.tolist())
    want = lowq_spec.pile(res, q, off, N, mask, MIN_MAPQ)
    qwant = qs.pile(res, q, off, quals, N, mask, MIN_MAPQ)
    assert qwant.sum() < world["qwant"].sum()
    p = eng.Pileup(idx, quals=True)
    p.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ, lowq=mask, quals=quals)
    same(p.counts(), want, "mask counts")
    same(p.quality.counts(), qwant, "mask")
    p.close()


def test_dedup_and_strands_ride_along(eng, world):
    idx, q, off, res, quals = world["idx"], world["q"], world["off"], world["res"], world["quals"]
    flags = dd.flags([(res, off)], MIN_MAPQ)[0]
    assert (flags == 1).any()
    kept = dd.keep(res, flags)
    want = pile_spec.pile(kept, q, off, N, MIN_MAPQ)
    qwant = qs.pile(kept, q, off, quals, N, None, MIN_MAPQ)
    assert qwant.sum() < world["qwant"].sum()
    p = eng.Pileup(idx, dedup=True, strands=True, events=True, quals=True)
    _, dup = p.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ, dedup=True, quals=quals)
    assert np.array_equal(dup, flags)
    same(p.counts(), want, "dedup counts")
    same(p.quality.counts(), qwant, "dedup")
    ref = eng.Pileup(idx, dedup=True, strands=True, events=True)
    ref.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ, dedup=True)
    assert np.array_equal(ref.counts(), p.counts()) and np.array_equal(ref.forward.counts(), p.forward.counts())
    assert ref.events()[0].tobytes() == p.events()[0].tobytes()
    ref.close()
    p.close()
    # enabled in the other order, without the filter
    p = eng.Pileup(idx, quals=True)
    p.enable_strands()
    p.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ, quals=quals)
    ref = eng.Pileup(idx, strands=True)
    ref.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ)
    assert np.array_equal(ref.counts(), p.counts()) and np.array_equal(ref.forward.counts(), p.forward.counts())
    same(p.quality.counts(), world["qwant"], "strands")
    ref.close()
    p.close()


@pytest.mark.parametrize("v", [0, 1, 40, 93, 200])
def test_constant_quality_is_q_times_a_plain_pileup(eng, world, v):
    idx, q, off = world["idx"], world["q"], world["off"]
    plain = eng.Pileup(idx)
    plain.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ)
    table = plain.counts().astype(np.int64)
    plain.close()
    p = eng.Pileup(idx, quals=True)
    p.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ, quals=np.full(int(off[-1]), min(33 + v, 255), dtype=np.uint8))
    want = min(v, 93) * table
    want[:, 4:] = 0
    same(p.quality.counts(), want, v)
    p.close()
    if v == 40:  # another Phred offset: the same bytes at offset 64 are quality 9
        p = eng.Pileup(idx, quals=True)
        p.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ, quals=np.full(int(off[-1]), 73, dtype=np.uint8), phred_offset=64)
        want = 9 * table
        want[:, 4:] = 0
        same(p.quality.counts(), want, "offset 64")
        p.close()


# ---- the weighted read-out -------------------------------------------------------------------------------------------------------

def same_calls(got, want, what=None):
    assert len(got) == len(want) == 4, what
    assert np.array_equal(got[0], want[0]), (what, got[0][:8], want[0][:8])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3]), what
    assert got[2].tobytes() == want[2].tobytes(), what


def test_weighted_genotypes_of_the_batch_equal_the_spec(eng, world):
    idx, q, off, quals, text = world["idx"], world["q"], world["off"], world["quals"], world["text"]
    p = eng.Pileup(idx, quals=True)
    p.add(q, off, MIN_LEN, True, min_mapq=MIN_MAPQ, quals=quals)
    table, qtable = p.counts().astype(np.int64), p.quality.counts().astype(np.int64)
    for ploidy, min_depth, min_qual in ((2, 1, 0), (1, 2, 3)):
        prm = qs.params(ploidy=ploidy, min_depth=min_depth, min_qual=min_qual)
        want = qs.genotypes(table, qtable, text, prm)
        assert len(want[0]) >= 1
        same_calls(p.genotypes(ploidy=ploidy, min_depth=min_depth, min_qual=min_qual, weighted=True), want, ploidy)
    p.close()


def planted(eng, q):
    """gt's planted table with Q = q * P beside it, through add_counts on the owner and on the quality accumulator."""
    text, table = planted_table()
    qtable = q * table
    qtable[:, 4:] = 0
    idx = eng.Index.build(text)
    p = eng.Pileup(idx, quals=True)
    p.add_counts(table.astype(np.uint32))
    if q:
        p.quality.add_counts(qtable.astype(np.uint32))
    return text, table, qtable, idx, p


@pytest.mark.parametrize("q", [0, 2, 37])
def test_planted_tables_tie_the_read_out_to_genotypes(eng, q):
    text, table, qtable, idx, p = planted(eng, q)
    same(p.quality.counts(), qtable, "planted")
    for ploidy in (1, 2):
        for costs in (qs.WQ_COSTS, gs.gt_costs(20)):
            M, H, E = costs
            got = p.genotypes(ploidy=ploidy, min_depth=2, min_qual=3, weighted=True, costs=costs)
            plain = p.genotypes(ploidy=ploidy, min_depth=2, min_qual=3, costs=(M, H, E + 1000 * q))
            assert len(plain[0]) > 20
            same_calls(got[:3] + (q * plain[1][:, :4],), plain + (got[3],), (ploidy, costs))
            same_calls(got, qs.genotypes(table, qtable, text, qs.params(ploidy=ploidy, min_depth=2, min_qual=3, costs=costs)), "spec")
    # ranges that start and end inside a tile, over the tile edges
    prm = qs.params(min_depth=2, min_qual=3)
    for first, count in ((5, 2040), (2047, 2), (2040, 2061), (4096, 5), (100, 0)):
        same_calls(p.genotypes(min_depth=2, min_qual=3, weighted=True, first=first, count=count),
                   qs.genotypes(table, qtable, text, prm, first, count), (first, count))
    p.close()
    idx.close()


def test_capacity_contract_of_the_weighted_read_out(eng):
    import torch
    from slamem_amd import capi
    text, table, qtable, idx, p = planted(eng, 20)
    prm = qs.params(min_depth=2, min_qual=3)
    want = qs.genotypes(table, qtable, text, prm)
    m, cap = len(want[0]), 7
    assert m > 2 * cap
    params = capi.GtParams(*prm)
    dev = idx.device
    fill = 0x5A
    pos = torch.full((cap + 4,), fill, dtype=torch.int64, device=dev)
    rows = torch.full((cap + 4, 6), fill, dtype=torch.int32, device=dev)
    gts = torch.full(((cap + 4) * 56,), fill, dtype=torch.uint8, device=dev)
    qsums = torch.full((cap + 4, 4), fill, dtype=torch.int32, device=dev)
    total = C.c_uint64()
    rc = capi.lib().slamem_pileup_genotypes_weighted_device(p._h, 0, len(text), C.byref(params), cap, pos.data_ptr(), rows.data_ptr(),
                                                            gts.data_ptr(), qsums.data_ptr(), C.byref(total), None)
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == m  # the need is reported
    assert np.array_equal(pos[:cap].cpu().numpy().view(np.uint64), want[0][:cap])
    assert np.array_equal(qsums[:cap].cpu().numpy().view(np.uint32), want[3][:cap])
    assert gts[:cap * 56].cpu().numpy().tobytes() == want[2][:cap].tobytes()
    for t in (pos[cap:], rows[cap:], gts[cap * 56:], qsums[cap:]):  # nothing is written beyond capacity
        assert bool((t == fill).all())
    # the host entry: the same rows, and the need
    hp, hc, hq = np.zeros(cap, dtype=np.uint64), np.zeros((cap, 6), dtype=np.uint32), np.zeros((cap, 4), dtype=np.uint32)
    hg = np.zeros(cap, dtype=gs.GENOTYPE_DTYPE)
    rc = capi.lib().slamem_pileup_genotypes_weighted_host(p._h, 0, len(text), C.byref(params), cap, hp.ctypes.data, hc.ctypes.data,
                                                          hg.ctypes.data, hq.ctypes.data, C.byref(total))
    assert rc == capi.SLAMEM_ERR_CAPACITY and total.value == m
    assert np.array_equal(hp, want[0][:cap]) and np.array_equal(hc, want[1][:cap]) and np.array_equal(hq, want[3][:cap])
    assert hg.tobytes() == want[2][:cap].tobytes()
    p.close()
    idx.close()


def test_refusals(eng, world):
    from slamem_amd import capi
    idx, q, off, quals = world["idx"], world["q"], world["off"], world["quals"]
    L = capi.lib()
    z = np.zeros(64, dtype=np.uint64).ctypes.data
    p = eng.Pileup(idx, quals=True, strands=True, dedup=True)
    # the three adds without quality bytes, on an accumulator that keeps quality sums
    for name, call in (("slamem_pileup_add_device", lambda h: L.slamem_pileup_add_device(h, z, z, 0, z, z, z, z, z, 0, None)),
                       ("slamem_pileup_add_masked_device", lambda h: L.slamem_pileup_add_masked_device(h, z, z, 0, z, z, z, z, z, 0, None, None)),
                       ("slamem_pileup_add_dedup_device", lambda h: L.slamem_pileup_add_dedup_device(h, z, z, 0, z, z, z, z, z, 0, None, z, None, None))):
        assert call(p._h) == capi.SLAMEM_ERR_ARG, name
        msg = L.slamem_last_error_message()
        assert name.encode() in msg and b"slamem_pileup_add_quals_device" in msg, name
    with pytest.raises(capi.SlamemError) as e:
        p.add(q, off, MIN_LEN, True)
    assert e.value.code == capi.SLAMEM_ERR_ARG and "quality sums" in str(e.value)
    # the children name themselves
    f, c = p.forward, p.quality
    calls = [("slamem_pileup_add_device", lambda h: L.slamem_pileup_add_device(h, z, z, 0, z, z, z, z, z, 0, None)),
             ("slamem_pileup_add_quals_device", lambda h: L.slamem_pileup_add_quals_device(h, z, z, 0, z, z, z, z, z, 0, None, z, 33, 0, None, None, None)),
             ("slamem_pileup_add_events_host", lambda h: L.slamem_pileup_add_events_host(h, z, 0)),
             ("slamem_pileup_enable_events", lambda h: L.slamem_pileup_enable_events(h, 0)),
             ("slamem_pileup_enable_dedup", lambda h: L.slamem_pileup_enable_dedup(h, 0)),
             ("slamem_pileup_enable_strands", lambda h: L.slamem_pileup_enable_strands(h)),
             ("slamem_pileup_enable_quals", lambda h: L.slamem_pileup_enable_quals(h)),
             ("slamem_pileup_free", lambda h: L.slamem_pileup_free(h))]
    for view, word in ((c, b"quality accumulator"), (f, b"forward accumulator")):
        for name, call in calls:
            assert call(view._h) == capi.SLAMEM_ERR_ARG, name
            msg = L.slamem_last_error_message()
            assert name.encode() in msg and word in msg, (name, msg)
    with pytest.raises(capi.SlamemError) as e:
        eng.Stream(idx, 2, 1 << 16, 64, True, pile=c)
    assert "slamem_stream_set_pileup" in str(e.value) and "quality accumulator" in str(e.value)
    assert not p.counts().any() and not c.counts().any() and not f.counts().any()  # (nothing of the above added anything)
    rows = np.zeros((N, 6), dtype=np.uint32)
    rows[7] = (1, 2, 3, 4, 0, 0)
    c.add_counts(rows)  # add_counts on the borrowed handle is allowed
    assert np.array_equal(c.counts(), rows) and not p.counts().any()
    p.close()
    # without enable_quals: the add with quality bytes, the borrowed handle and the weighted read-out are refused
    plain = eng.Pileup(idx)
    with pytest.raises(capi.SlamemError) as e:
        plain.add(q, off, MIN_LEN, True, quals=quals)
    assert e.value.code == capi.SLAMEM_ERR_ARG and "slamem_pileup_enable_quals" in str(e.value)
    assert not plain.counts().any()
    h = C.c_void_p()
    assert L.slamem_pileup_quality(plain._h, C.byref(h)) == capi.SLAMEM_ERR_ARG and not h.value
    with pytest.raises(capi.SlamemError) as e:
        plain.genotypes(weighted=True)
    assert e.value.code == capi.SLAMEM_ERR_ARG and "slamem_pileup_enable_quals" in str(e.value)
    # enable after an add is refused, after a reset it is not
    plain.add(q, off, MIN_LEN, True)
    with pytest.raises(capi.SlamemError) as e:
        plain.enable_quals()
    assert e.value.code == capi.SLAMEM_ERR_ARG and "empty" in str(e.value) and plain.quality is None
    plain.reset()
    plain.enable_quals()
    assert plain.quality is not None and not plain.quality.counts().any()
    with pytest.raises(capi.SlamemError) as e:  # dedup asked of an accumulator without the filter
        plain.add(q, off, MIN_LEN, True, quals=quals, dedup=True)
    assert "slamem_pileup_enable_dedup" in str(e.value)
    plain.close()
    assert L.slamem_pileup_enable_quals(None) == capi.SLAMEM_ERR_ARG and L.slamem_pileup_quality(None, None) == capi.SLAMEM_ERR_ARG


# ---- the stream's other branches -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["mask", "dedup"])
def test_stream_with_a_mask_and_with_the_duplicate_filter(eng, world, mode):
    """Window by window through submit_quals: with a low-quality mask, and with the duplicate filter (whose flags come back through
    dups()); an empty batch in front of the others adds nothing."""
    idx, q, off, res, quals = world["idx"], world["q"], world["off"], world["res"], world["quals"]
    wins, slots = windows(off, 70), 2
    mask = None
    if mode == "mask":
        bits = (np.random.default_rng(8).random(int(off[-1])) < 0.08).astype(np.uint8)
        mask = lowq_spec.from_bits(bits.tolist())
        want = lowq_spec.pile(res, q, off, N, mask, MIN_MAPQ)
        qwant = qs.pile(res, q, off, quals, N, mask, MIN_MAPQ)
        flags = None
    else:
        adds = [(res[int(np.searchsorted(off, w[0])):int(np.searchsorted(off, w[0])) + len(w) - 1], w) for w in wins]
        flags = dd.flags(adds, MIN_MAPQ)
        kept = [r for (rs, _), f in zip(adds, flags) for r in dd.keep(rs, f)]
        assert any((f == 1).any() for f in flags)
        want = pile_spec.pile(kept, q, off, N, MIN_MAPQ)
        qwant = qs.pile(kept, q, off, quals, N, None, MIN_MAPQ)
    p = eng.Pileup(idx, quals=True, dedup=mode == "dedup")
    st = eng.Stream(idx, slots, 1 << 16, len(wins[0]) - 1, True, pile=p, min_mapq=MIN_MAPQ, quals=True, dedup=mode == "dedup")
    st.submit_quals(q, quals, mask, off[:1].copy(), 14)  # no reads
    st.next()
    assert not p.counts().any() and not p.quality.counts().any()
    got_flags = []
    for b in range(min(slots - 1, len(wins))):
        st.submit_quals(q, quals, mask, wins[b], 14)
    for b in range(len(wins)):
        st.next()
        if flags is not None:
            got_flags.append(st.dups().copy())
        if b + slots - 1 < len(wins):
            st.submit_quals(q, quals, mask, wins[b + slots - 1], 14)
    st.close()
    if flags is not None:
        assert all(np.array_equal(a, b) for a, b in zip(got_flags, flags))
    same(p.counts(), want, (mode, "counts"))
    same(p.quality.counts(), qwant, mode)
    p.close()


# ---- the executable --------------------------------------------------------------------------------------------------------------

def test_cli_file_is_the_spec_of_the_engines_tables(eng, world, tmp_path):
    """slaMEM-hip -b -vcf -gt -wq, alone, with -sb -fs 30 and with -bq 10, on one GPU and on two logical ones: byte for byte the file
    qual_spec formats from the engine's tables, quality sums and events.  On the FASTA of the same reads: the same with every quality
    at -err's Q and a line on stderr.  Without -wq: the file of gt_spec and of the formatter that was there, as before."""
    import os
    import subprocess

    import events_spec as es
    import hostlib
    from test_gpu_pile import write_fasta
    from test_gpu_sb import EXE, sample_reads
    from test_gt_host import host_gt_vcf
    text, idx = world["text"], world["idx"]
    reads = world["reads"] + sample_reads(text)
    q, off = batch(reads)
    rng = np.random.default_rng(31)
    quals = (33 + np.array(RUN_VALUES, dtype=np.uint8)[rng.integers(0, 4, size=(int(off[-1]) + 9) // 10)].repeat(10)[:int(off[-1])]).astype(np.uint8)
    quals[::17] = 33 + 41
    quals[5::29] = 126
    quals[7::31] = 33
    ref_fa, q_fa, q_fq = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa"), str(tmp_path / "reads.fq")
    write_fasta(ref_fa, [(b"one first", text[:3000]), (b"two\tsecond", text[3001:])])
    write_fasta(q_fa, [(b"read%d x" % k, r) for k, r in enumerate(reads)])
    with open(q_fq, "wb") as fh:
        fh.write(lowq_spec.write_fastq([(b"read%d x" % k, bytes(r), bytes(quals[int(off[k]):int(off[k + 1])])) for k, r in enumerate(reads)]))
    loaded = hostlib.Loaded(ref_fa, 1)
    assert loaded.chars == bytes(text)
    prm = qs.params(min_depth=2, min_qual=3)
    args = ["-mdep", "2", "-qual", "3", "-minq", str(MIN_MAPQ)]

    def tables(v, bq=0):
        p = eng.Pileup(idx, strands=True, events=True, quals=True)
        p.add(q, off, 20, True, min_mapq=MIN_MAPQ, quals=v, lowq=lowq_spec.pack(v, bq) if bq else None)
        out = p.counts().astype(np.int64), p.forward.counts().astype(np.int64), p.quality.counts().astype(np.int64), es.from_records(p.events()[0])
        p.close()
        return out
    t, f, qt, ev = tables(quals)
    tb, fb, qtb, evb = tables(quals, 10)
    assert qtb.sum() < qt.sum()
    flat = np.full(int(off[-1]), 33 + 25, dtype=np.uint8)
    tf, ff, qtf, evf = tables(flat)
    assert np.array_equal(tf, t) and np.array_equal(qtf[:, :4], 25 * t[:, :4])
    wq = qs.vcf_file(t, qt, ev, loaded, prm)
    lines = wq[len(qs.vcf_header(loaded)):].split(b"\n")[:-1]
    assert len(lines) >= 7 and any(line.endswith(b":.") for line in lines) and any(not line.endswith(b":.") for line in lines)
    base = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    two = dict(base, SLAMEM_LOGICAL_GPUS="2", SLAMEM_BATCH_MB="1")
    plain = gs.vcf_file(t, ev, loaded, gs.params(min_depth=2, min_qual=3))
    assert plain == host_gt_vcf(loaded, t, ev, gs.params(min_depth=2, min_qual=3))
    cases = (("wq1", base, ["-wq"], q_fq, wq), ("wq2", two, ["-wq"], q_fq, wq),
             ("sb", base, ["-wq", "-sb", "-fs", "30"], q_fq, qs.vcf_file(t, qt, ev, loaded, prm, f, 30)),
             ("bq", two, ["-bq", "10", "-wq"], q_fq, qs.vcf_file(tb, qtb, evb, loaded, prm)),
             ("fa", base, ["-wq", "-err", "25"], q_fa, qs.vcf_file(tf, qtf, evf, loaded, prm, err_q=25)),
             ("gt", base, [], q_fq, plain))
    for name, env, extra, reads_file, want in cases:
        out = str(tmp_path / (name + ".vcf"))
        r = subprocess.run([EXE, "-b", "-vcf", "-gt"] + extra + args + ["-o", out, ref_fa, reads_file], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=env, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
        assert open(out, "rb").read() == want, name
        assert (b"; base qualities in the likelihood = on" in r.stdout) == ("-wq" in extra)
        assert (b"FASTA queries carry no base qualities: their letters count with the quality of -err, 25" in r.stderr) == (name == "fa")
