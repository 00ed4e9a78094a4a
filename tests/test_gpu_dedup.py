"""-dedup on the MI355X (slamem_pileup_enable_dedup / _add_dedup_device / _dedup_stats, engine.Pileup(dedup=True), a stream with
the filter on): the flags are tests/dedup_spec.py applied to map_spec.filter_reads of the same engine's -mem list, and the table
(and the events) are pile_spec / lowq_spec / events_spec over the reads that spec keeps -- all compared for exact equality.  One
fixed-seed reference of 3,001 letters in two records, with a planted repeat for the mapping-quality case; the reads are cut from
it."""
import ctypes as C

import numpy as np
import pytest

import dedup_spec as dd
import events_spec as es
import ext_spec
import lowq_spec
import pile_spec
from test_gpu_aln import batch
from test_gpu_pile import same, spec_results, windows

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
MIN_LEN = 20
N = 3001
# where an ordinary read may lie: clear of the repeat's two copies ([200, 400) and [2200, 2400)), of the separator at 1500 and of
# the text's two ends, which the clipped reads use
ZONES = ((520, 1500), (1501, 2150))


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test without a GPU")
    from slamem_amd import engine
    return engine


def reference():
    rng = np.random.default_rng(4231)
    t = rng.choice(ACGT, size=N)
    t[1500] = ord("N")
    t[2200:2400] = t[200:400]
    return t


def edited(rng, frag, subs, indel):
    """A copy of the fragment with `subs` substitutions and (indel 1) two letters deleted or (indel 2) two inserted at its middle;
    the outer 30 letters and the 12 around the middle stay as they are, so both ends are anchored by exact matches."""
    r = frag.copy()
    mid = len(r) // 2
    where = [x for x in range(30, len(r) - 30) if abs(x - mid) > 12]
    for x in rng.choice(where, size=subs, replace=False):
        r[x] = ACGT[(int(np.nonzero(ACGT == r[x])[0][0]) + 1 + int(rng.integers(0, 3))) % 4]
    if indel == 1:
        r = np.concatenate([r[:mid], r[mid + 2:]])
    elif indel == 2:
        r = np.concatenate([r[:mid], ACGT[[(int(np.nonzero(ACGT == r[mid])[0][0]) + 1) % 4] * 2], r[mid:]])
    return r


def anchors(rng, count, length):
    """`count` distinct positions a such that [a, a + length) lies inside a zone."""
    pool = np.concatenate([np.arange(lo, hi - length) for lo, hi in ZONES])
    return [int(a) for a in rng.choice(pool, size=count, replace=False)]


def mixed_batch():
    """Case 1: forty keys with one to six copies each, on both strands; the copies of a key share the 5' end and differ in
    length, in one or two substitutions and, some, in an indel.  Two keys start in 8 and 5 junk letters in front of text position
    0, two reverse keys end in junk behind the last position; four reads map nowhere.  Shuffled, but for two copies with an
    indel, which lead the batch so that a deletion and an insertion are among the reads kept.  Returns the reference, the reads
    and per read (key number or -1, copy number)."""
    ref = reference()
    rng = np.random.default_rng(4232)
    reads, meta = [], []
    pos = anchors(rng, 36, 140)
    for k in range(40):
        strand = 1 + k % 2
        for c in range(1 + k % 6):
            L = 140 - 7 * c
            if k < 36:
                a = pos[k]  # forward: the fragment starts here; reverse: it ends at a + 140
                frag = ref[a:a + L] if strand == 1 else ref[a + 140 - L:a + 140]
                body = edited(rng, frag, 1 + c % 2 if c else 0, 1 + (k // 5) % 2 if (c == 1 and k % 5 == 2) else 0)
            else:
                junk = rng.choice(ACGT, size=8 if k < 38 else 5)
                frag = ref[:L] if strand == 1 else ref[N - L:]
                body = edited(rng, frag, 1 + c % 2 if c else 0, 0)
                body = np.concatenate([junk, body]) if strand == 1 else np.concatenate([body, junk])
            reads.append(body if strand == 1 else ext_spec.revcomp(body))
            meta.append((k, c))
    junk_rng = np.random.default_rng(4233)
    reads += [junk_rng.choice(ACGT, size=100) for _ in range(4)]
    meta += [(-1, 0)] * 4
    order = [int(i) for i in rng.permutation(len(reads))]
    lead = [i for i in order if meta[i] in ((2, 1), (7, 1))]  # a deletion on the forward strand, an insertion on the reverse
    order = lead + [i for i in order if i not in lead]
    return ref, [reads[i] for i in order], [meta[i] for i in order]


def mapped(idx, ref, reads):
    """A read_map tuple per read, each distinct read mapped once."""
    uniq = {}
    for r in reads:
        uniq.setdefault(bytes(r), len(uniq))
    q, off = batch([np.frombuffer(b, dtype=np.uint8) for b in uniq])
    res = spec_results(idx, ref, q, off, MIN_LEN, True)
    return [res[uniq[bytes(r)]] for r in reads]


@pytest.fixture(scope="module")
def world(eng):
    ref, reads, _ = mixed_batch()
    idx = eng.Index.build(ref)
    q, off = batch(reads)
    res = mapped(idx, ref, reads)
    yield dict(ref=ref, idx=idx, reads=reads, q=q, off=off, res=res)
    idx.close()


def got_events(p):
    arr, skipped = p.events()
    return es.from_records(arr), skipped


def run(eng, idx, adds, min_mapq=0, events=False, slots=0, masks=None):
    """The adds, in order, through one accumulator: (flags per add, table, events or None, stats)."""
    p = eng.Pileup(idx, events=events, dedup=True, dedup_slots=slots)
    flags = []
    for k, (q, off) in enumerate(adds):
        recs, dup = p.add(q, off, MIN_LEN, True, min_mapq=min_mapq, dedup=True, lowq=None if masks is None else masks[k])
        assert dup.dtype == np.uint8 and len(dup) == len(off) - 1 == len(recs)
        flags.append(dup)
    out = flags, p.counts(), got_events(p) if events else None, p.dedup_stats()
    p.close()
    return out


def expected(ref, adds, min_mapq=0, masks=None, flags=None):
    """adds: (q, off, results) in order.  The spec's flags (or the given ones) and the tables of the reads they keep."""
    fl = dd.flags([(res, off) for _, off, res in adds], min_mapq) if flags is None else flags
    table, ev = pile_spec.empty(len(ref)), es.Table(ref)
    for k, ((q, off, res), f) in enumerate(zip(adds, fl)):
        kept = dd.keep(res, f)
        lowq_spec.pile(kept, q, off, len(ref), None if masks is None else masks[k], min_mapq, table)
        ev.add_batch(kept, q, off, min_mapq)
    return fl, table, (ev.events(), ev.skipped)


def check_stats(stats, flags, adds, min_mapq=0):
    cand = sum(dd.is_candidate(r, min_mapq) for _, _, res in adds for r in res)
    dup = sum(int((f == 1).sum()) for f in flags)
    room = sum(int((f == 2).sum()) for f in flags)
    assert stats == dict(candidates=cand, duplicates=dup, no_room=room, kept=cand - dup - room)


def split(q, off, cut):
    a, b = int(off[0]), int(off[cut])
    return (q[a:b], (off[:cut + 1] - off[0]).astype(np.uint64)), (q[b:int(off[-1])], (off[cut:] - off[cut]).astype(np.uint64))


# ---- 1: the mixed batch --------------------------------------------------------------------------------------------------------

def test_mixed_batch_flags_table_and_events(eng, world):
    w = world
    q, off, res = w["q"], w["off"], w["res"]
    keys = [dd.key(r, int(off[k + 1] - off[k])) for k, r in enumerate(res)]
    # (the batch is what its docstring says)
    assert len({k for k in keys if k}) == 40 and sum(k is None for k in keys) == 4 == sum(r[0] == 0 for r in res)
    assert {k for k in keys if k and k[1] < 0} == {(1, -8), (1, -5)} and {k for k in keys if k and k[1] > N} == {(2, N + 8), (2, N + 5)}
    assert sum(k[0] == 1 for k in keys if k) > 40 and sum(k[0] == 2 for k in keys if k) > 40
    fl, table, ev = expected(w["ref"], [(q, off, res)])
    assert int(fl[0].sum()) == len(res) - 4 - 40 and len(ev[0]) >= 2 and table[:, 4].sum() > 0 and table[:, 5].sum() > 0
    flags, got, got_ev, stats = run(eng, w["idx"], [(q, off)], events=True)
    assert np.array_equal(flags[0], fl[0])
    same(got, table)
    assert got_ev == ev
    check_stats(stats, flags, [(q, off, res)])
    # without the filter the same accumulator type piles every read: the filter decides something
    plain = eng.Pileup(w["idx"])
    plain.add(q, off, MIN_LEN, True)
    assert not np.array_equal(plain.counts(), got)
    plain.close()


# ---- 2: contention -------------------------------------------------------------------------------------------------------------

def test_three_hundred_copies_of_one_key_keep_the_first(eng, world):
    w = world
    a = ZONES[0][0] + 11
    reads = [w["ref"][a:a + (100, 110, 120)[k % 3]] for k in range(300)]
    q, off = batch(reads)
    res = mapped(w["idx"], w["ref"], reads)
    assert len({dd.key(r, len(x)) for r, x in zip(res, reads)}) == 1
    flags, got, _, stats = run(eng, w["idx"], [(q, off)])
    assert flags[0].tolist() == [0] + [1] * 299
    same(got, pile_spec.pile(res[:1], q[:100], off[:2], N))
    assert stats == dict(candidates=300, duplicates=299, no_room=0, kept=1)


# ---- 3: the split into adds ------------------------------------------------------------------------------------------------------

def test_one_add_two_adds_and_the_adds_reversed(eng, world):
    w = world
    q, off, res = w["q"], w["off"], w["res"]
    cut = (len(off) - 1) // 2
    (qa, oa), (qb, ob) = split(q, off, cut)
    ra, rb = res[:cut], res[cut:]
    one_f, one_t, _, _ = run(eng, w["idx"], [(q, off)])
    two_f, two_t, _, stats = run(eng, w["idx"], [(qa, oa), (qb, ob)])
    assert np.array_equal(np.concatenate(two_f), one_f[0]) and np.array_equal(two_t, one_t)
    check_stats(stats, two_f, [(qa, oa, ra), (qb, ob, rb)])
    # the second half first: another choice of reads, and still one per key -- the first of the batch added first
    rev_f, rev_t, _, _ = run(eng, w["idx"], [(qb, ob), (qa, oa)])
    fl, table, _ = expected(w["ref"], [(qb, ob, rb), (qa, oa, ra)])
    assert all(np.array_equal(g, f) for g, f in zip(rev_f, fl))
    same(rev_t, table)
    assert not np.array_equal(np.concatenate(rev_f[::-1]), one_f[0])
    first = {}
    for part, (o, rs) in enumerate(((ob, rb), (oa, ra))):
        for k, r in enumerate(rs):
            key = dd.key(r, int(o[k + 1] - o[k]))
            if key is not None:
                first.setdefault(key, (part, k))
    kept = {}
    for part, (o, rs) in enumerate(((ob, rb), (oa, ra))):
        for k, r in enumerate(rs):
            key = dd.key(r, int(o[k + 1] - o[k]))
            if key is not None and rev_f[part][k] == 0:
                kept.setdefault(key, []).append((part, k))
    assert kept == {key: [at] for key, at in first.items()} and len(kept) == 40


# ---- 4: the least mapping quality ------------------------------------------------------------------------------------------------

def test_a_repeat_read_of_quality_0_does_not_shadow_a_unique_read(eng, world):
    """[200, 400) stands again at [2200, 2400).  The first read lies inside the repeat (quality 0, on whichever copy); the other two
    start where it starts on either copy and run 100 letters on into unique text."""
    w = world
    ref = w["ref"]
    reads = [ref[300:400], ref[300:500], ref[2300:2500]]
    q, off = batch(reads)
    res = mapped(w["idx"], ref, reads)
    assert res[0][1] == 0 and res[1][1] >= 20 and res[2][1] >= 20 and all(r[0] == 1 for r in res)
    k = [dd.key(r, len(x)) for r, x in zip(res, reads)]
    assert k[0] in (k[1], k[2]) and k[1] != k[2]
    for min_mapq, want in ((20, [0, 0, 0]), (0, [0, int(k[0] == k[1]), int(k[0] == k[2])])):
        fl, table, _ = expected(ref, [(q, off, res)], min_mapq)
        assert fl[0].tolist() == want
        flags, got, _, stats = run(eng, w["idx"], [(q, off)], min_mapq=min_mapq)
        assert flags[0].tolist() == want
        same(got, table)
        check_stats(stats, flags, [(q, off, res)], min_mapq)


# ---- 5: a small table ------------------------------------------------------------------------------------------------------------

def test_sixty_four_slots_hold_forty_keys(eng, world):
    w = world
    q, off, res = w["q"], w["off"], w["res"]
    fl, table, _ = expected(w["ref"], [(q, off, res)])
    flags, got, _, stats = run(eng, w["idx"], [(q, off)], slots=64)
    assert np.array_equal(flags[0], fl[0]) and stats["no_room"] == 0 and stats["kept"] == 40
    same(got, table)


def test_sixty_four_slots_and_a_hundred_and_fifty_keys(eng, world):
    """The table fills: which keys found room is the device's to say.  A read flagged 1 is one the spec calls a duplicate too, the
    reads without room are kept, and the table is the spec's over every read not flagged 1."""
    w = world
    ref = w["ref"]
    rng = np.random.default_rng(4234)
    reads = []
    for k, a in enumerate(anchors(rng, 150, 100)):
        strand = 1 + k % 2
        for L in (100, 90)[:1 + (k % 3 == 0)]:
            frag = ref[a:a + L] if strand == 1 else ref[a + 100 - L:a + 100]
            reads.append(frag if strand == 1 else ext_spec.revcomp(frag))
    reads = [reads[i] for i in rng.permutation(len(reads))]
    q, off = batch(reads)
    res = mapped(w["idx"], ref, reads)
    spec = dd.flags([(res, off)])[0]
    assert len({dd.key(r, len(x)) for r, x in zip(res, reads)}) == 150 and int(spec.sum()) == 50
    flags, got, _, stats = run(eng, w["idx"], [(q, off)], slots=64)
    f = flags[0]
    assert stats["candidates"] == len(reads) == stats["kept"] + stats["duplicates"] + stats["no_room"]
    assert stats["duplicates"] == int((f == 1).sum()) and stats["no_room"] == int((f == 2).sum()) and stats["kept"] == 64
    assert not ((f == 1) & (spec == 0)).any()
    assert int((f == 2).sum()) >= 1
    _, table, _ = expected(ref, [(q, off, res)], flags=[f])
    same(got, table)


# ---- 6: with a low-quality mask --------------------------------------------------------------------------------------------------

def test_low_quality_mask_over_the_kept_reads(eng, world):
    w = world
    q, off, res = w["q"], w["off"], w["res"]
    rng = np.random.default_rng(4235)
    mask = lowq_spec.from_bits((rng.random(int(off[-1])) < 0.1).astype(np.uint8).tolist())
    fl, table, _ = expected(w["ref"], [(q, off, res)], masks=[mask])
    flags, got, _, _ = run(eng, w["idx"], [(q, off)], masks=[mask])
    assert np.array_equal(flags[0], fl[0])
    same(got, table)
    assert not np.array_equal(table, expected(w["ref"], [(q, off, res)])[1])


# ---- 7: reset --------------------------------------------------------------------------------------------------------------------

def test_reset_clears_the_table_the_counters_and_the_order(eng, world):
    w = world
    q, off = w["q"], w["off"]
    p = eng.Pileup(w["idx"], events=True, dedup=True)
    _, dup1 = p.add(q, off, MIN_LEN, True, dedup=True)
    t1, e1, s1 = p.counts(), got_events(p), p.dedup_stats()
    _, again = p.add(q, off, MIN_LEN, True, dedup=True)  # (without a reset every candidate of a second add is a duplicate)
    assert int((again == 1).sum()) == s1["candidates"] and np.array_equal(p.counts(), t1)
    p.reset()
    assert not p.counts().any() and p.dedup_stats() == dict(candidates=0, duplicates=0, no_room=0, kept=0)
    _, dup2 = p.add(q, off, MIN_LEN, True, dedup=True)
    assert np.array_equal(dup1, dup2) and np.array_equal(p.counts(), t1) and got_events(p) == e1 and p.dedup_stats() == s1
    p.close()


# ---- 8: the stream ---------------------------------------------------------------------------------------------------------------

def test_stream_equals_three_direct_adds(eng, world):
    w = world
    q, off, res = w["q"], w["off"], w["res"]
    per = (len(off) - 1 + 2) // 3
    wins = windows(off, per)
    assert len(wins) == 3
    adds = [(q[int(x[0]):int(x[-1])], (x - x[0]).astype(np.uint64)) for x in wins]
    direct_f, direct_t, _, direct_s = run(eng, w["idx"], adds)
    fl, table, _ = expected(w["ref"], [(a[0], a[1], res[b * per:(b + 1) * per]) for b, a in enumerate(adds)])
    assert all(np.array_equal(g, f) for g, f in zip(direct_f, fl))
    same(direct_t, table)
    p = eng.Pileup(w["idx"], dedup=True)
    st = eng.Stream(w["idx"], 3, 1 << 16, per, True, pile=p, dedup=True)
    plain = w["idx"].map_reads(q, off, MIN_LEN, True)[4]
    flags = []
    for x in wins[:2]:
        st.submit(q, x, MIN_LEN)
    for b in range(3):
        total, nothing, _ = st.next()
        assert nothing is None
        flags.append(st.dups())
        assert np.array_equal(st.maps()["strand"], plain["strand"][b * per:(b + 1) * per])  # (the records as the search wrote them)
        if b + 2 < 3:
            st.submit(q, wins[b + 2], MIN_LEN)
    st.close()
    assert all(np.array_equal(g, f) for g, f in zip(flags, direct_f))
    assert np.array_equal(p.counts(), direct_t) and p.dedup_stats() == direct_s
    p.close()


# ---- 9: refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals(eng, world):
    from slamem_amd import capi
    w = world
    idx, q, off = w["idx"], w["q"], w["off"]
    L = capi.lib()
    ARG = capi.SLAMEM_ERR_ARG
    plain = eng.Pileup(idx)
    with pytest.raises(capi.SlamemError) as err:
        plain.add(q, off, MIN_LEN, True, dedup=True)
    assert err.value.code == ARG and "not enabled" in str(err.value)
    assert not plain.counts().any()
    with pytest.raises(capi.SlamemError) as err:
        plain.dedup_stats()
    assert err.value.code == ARG
    for slots in (100, 63, 32, 2 ** 33):
        with pytest.raises(capi.SlamemError) as err:
            eng.Pileup(idx, dedup=True, dedup_slots=slots)
        assert err.value.code == ARG and "power of two" in str(err.value)
    with pytest.raises(ValueError):
        eng.Pileup(idx, dedup_slots=64)
    p = eng.Pileup(idx, dedup=True, dedup_slots=128)
    assert L.slamem_pileup_enable_dedup(p._h, 64) == ARG and b"already" in L.slamem_last_error_message()
    # the stream: the setter needs match type 8, an accumulator with the filter, and comes before the first submit
    def raw(match_type):
        h = C.c_void_p()
        assert L.slamem_stream_create(idx._h, 2, 1 << 16, 64, 1, match_type, C.byref(h)) == capi.SLAMEM_OK
        return h
    h = raw(7)
    assert L.slamem_stream_set_dedup(h, 1) == ARG
    assert L.slamem_stream_destroy(h) == capi.SLAMEM_OK
    h = raw(8)
    assert L.slamem_stream_set_dedup(h, 1) == ARG  # no accumulator yet
    assert L.slamem_stream_set_pileup(h, plain._h, 0) == capi.SLAMEM_OK
    assert L.slamem_stream_set_dedup(h, 1) == ARG and b"slamem_pileup_enable_dedup" in L.slamem_last_error_message()
    assert L.slamem_stream_set_pileup(h, p._h, 0) == capi.SLAMEM_OK
    flags = C.c_void_p()
    assert L.slamem_stream_dups(h, C.byref(flags)) == ARG  # the filter is not switched on
    offs = np.ascontiguousarray(off[:9])
    assert L.slamem_stream_submit(h, q.ctypes.data, offs.ctypes.data, 8, MIN_LEN) == capi.SLAMEM_OK
    assert L.slamem_stream_set_dedup(h, 1) == ARG and b"before the first submit" in L.slamem_last_error_message()
    mems, boff, total, nq = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint32()
    assert L.slamem_stream_next(h, C.byref(mems), C.byref(boff), C.byref(total), C.byref(nq), None) == capi.SLAMEM_OK and nq.value == 8
    assert L.slamem_stream_destroy(h) == capi.SLAMEM_OK
    with pytest.raises(ValueError):
        eng.Stream(idx, 3, 1 << 16, 13, True, paf=True, dedup=True)
    with pytest.raises(capi.SlamemError):
        eng.Stream(idx, 3, 1 << 16, 13, True, pile=plain, dedup=True)
    p.close()
    plain.close()
